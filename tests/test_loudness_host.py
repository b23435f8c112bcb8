"""CPU: ``loudness_ref`` - the float64 restatement of ITU-R BS.1770-4 that ``nomad_degrade_normalize`` is held to - pinned to the
standard's own numbers, the test signals shown to exercise the gate each is named after, and the argument errors of the Python
surface that need no GPU."""
import math
import sys

import numpy as np
import pytest
import torch

import loudness_ref as L
from nomad_amd import _lib
from nomad_amd.engine import Engine
from nomad_amd.nomad import Nomad


def test_k_weighting_at_48_khz_is_the_standards_table():
    (b1, a1), (b2, a2) = L.k_weighting(48000)
    assert abs(b1[0] - 1.53512485958697) < 1e-12
    assert abs(b1[1] - -2.69169618940638) < 1e-12 and abs(b1[2] - 1.19839281085285) < 1e-12
    assert a1[0] == 1.0 and abs(a1[1] - -1.69065929318241) < 1e-12 and abs(a1[2] - 0.73248077421585) < 1e-12
    assert b2.tolist() == [1.0, -2.0, 1.0]
    assert a2[0] == 1.0 and abs(a2[1] - -1.99004745483398) < 1e-12 and abs(a2[2] - 0.99007225036621) < 1e-12


def test_high_pass_poles_at_16_khz_sit_at_radius_0_985():
    _, (_, a2) = L.k_weighting(16000)
    assert abs(math.sqrt(a2[2]) - 0.985) < 1e-3


def test_full_scale_997_hz_sine_reads_the_conformance_point():
    at48 = L.measure(L.sine(96000, 48000), 48000)
    assert abs(at48["level"] - -3.01) < 0.01, at48
    at16 = L.measure(L.sine(32000, 16000), 16000)
    assert abs(at16["level"] - -2.970) < 0.001, at16
    assert at48["blocks"] == at48["total"] == 17 and at16["blocks"] == at16["total"] == 17
    assert at16["peak"] <= 1.0 and L.measure(L.sine(32000, 16000), 16000, "peak")["level"] <= 0.0
    rms = L.measure(L.sine(32000, 16000), 16000, "rms")["level"]
    assert abs(rms - -3.0103) < 1e-3, rms


def test_a_silent_second_falls_to_the_absolute_gate():
    x = L.silent_second(48001, 16000, 21)
    res = L.measure(x, 16000)
    assert res["total"] == 27
    assert res["total"] - res["absolute"] >= 3, res           # the blocks wholly inside the silence, once the filters have rung out
    assert res["margin"] > 1e-6
    loud = L.measure(x[:(48001 - 16000) // 2], 16000)
    # the blocks that straddle an edge of the silence still count: 0.7 dB under the noise alone, not the 1.8 dB of an ungated mean
    assert loud["level"] - 1.0 < res["level"] < loud["level"], (res, loud)


def test_a_passage_15_lu_down_falls_to_the_relative_gate_only():
    x = L.quiet_passage(48001, 16000, 22)
    res = L.measure(x, 16000)
    assert res["absolute"] == res["total"] == 27, res
    assert 0 < res["blocks"] < res["absolute"], res
    assert res["margin"] > 1e-6
    loud = L.measure(x[:2 * 48001 // 3], 16000)
    assert loud["level"] - 1.0 < res["level"] < loud["level"], (res, loud)   # the blocks across the edge still count


def test_short_and_silent_clips_have_no_level():
    hop = 1600
    short = L.measure(L.pcm_noise(4 * hop - 1, 3), 16000)
    assert short["level"] == -math.inf and short["total"] == 0 and short["peak"] > 0
    assert L.measure(L.pcm_noise(4 * hop, 3), 16000)["total"] == 1
    zeros = L.measure(np.zeros(8000, dtype=np.float32), 16000)
    assert zeros["level"] == -math.inf and zeros["total"] == 2 and zeros["absolute"] == 0 and zeros["peak"] == 0.0
    for kind in ("rms", "peak"):
        assert L.measure(np.zeros(8000, dtype=np.float32), 16000, kind)["level"] == -math.inf
    assert L.gain(-math.inf, 0.5, -23.0, -1.0) == 1.0


def test_a_dc_offset_is_removed_by_the_high_pass_and_kept_by_rms_and_peak():
    x = L.dc_offset(16777, 23)
    assert L.measure(x, 16000)["level"] < L.measure(x, 16000, "rms")["level"] - 10.0
    assert L.measure(x, 16000, "peak")["level"] > -6.0


def test_gain_and_ceiling():
    assert L.gain(-20.0, 0.5, -23.0) == 10.0 ** (-3.0 / 20.0)
    assert L.gain(-40.0, 0.5, -23.0, -6.0) == 10.0 ** (-6.0 / 20.0) / 0.5
    x = np.array([0.5, -0.25], dtype=np.float32)
    assert L.apply(x, 2.0).tolist() == [1.0, -0.5]


# ---- the Python surface, no GPU --------------------------------------------------------------------------------------------------
def test_the_entry_points_are_bound():
    assert len(_lib.SIGNATURES["nomad_degrade_normalize"][1]) == 14 and len(_lib.SIGNATURES["nomad_degrade_normalize_scratch_bytes"][1]) == 3
    assert _lib.LOUDNESS_MODE == {"ebu": 0, "rms": 1, "peak": 2} and _lib.ABI_VERSION == 3


def test_check_normalize_refuses_what_the_library_would():
    assert Engine.check_normalize(-23, "ebu", None, 16000)[:2] == (0, -23.0) and math.isnan(Engine.check_normalize(-23, "ebu", None, 16000)[2])
    assert Engine.check_normalize(-3, "peak", -1, 48000) == (2, -3.0, -1.0, 48000)
    for bad, word in ((dict(kind="lufs"), "kind"), (dict(target=float("nan")), "target"), (dict(target=float("inf")), "target"),
                      (dict(peak_db=float("inf")), "peak_db"), (dict(sample_rate=7990), "sample_rate"),
                      (dict(sample_rate=16001), "sample_rate"), (dict(sample_rate=192010), "sample_rate")):
        args = dict(target=-23.0, kind="ebu", peak_db=None, sample_rate=16000)
        args.update(bad)
        with pytest.raises(ValueError, match=word):
            Engine.check_normalize(**args)


class _NoEngine:
    device = "cpu"

    def __getattr__(self, name):
        pytest.fail(f"an argument error reached the engine ({name})")


def _nomad():
    n = Nomad.__new__(Nomad)            # no GPU: only the host side is under test
    n.engine, n.precision, n.group = _NoEngine(), "fp32", None
    return n


def test_normalize_and_loudness_refusals():
    n = _nomad()
    wav = torch.zeros(2, 8000)
    with pytest.raises(ValueError, match="no gradient"):
        n.normalize(wav.clone().requires_grad_())
    with pytest.raises(ValueError, match="no gradient"):
        n.loudness(wav.clone().requires_grad_())
    with pytest.raises(ValueError, match="kind"):
        n.normalize(wav, kind="true-peak")
    with pytest.raises(ValueError, match="kind"):
        n.loudness(wav, kind="lufs")
    with pytest.raises(ValueError, match="target"):
        n.normalize(wav, target=float("nan"))
    with pytest.raises(ValueError, match=r"\(B,1,N\) or \(B,N\)"):
        n.normalize(torch.zeros(8000))
    with pytest.raises(ValueError, match="kind"):
        n.intensity_sweep(wav, torch.zeros(3, 256), clip_factor=[5], normalize=-23, normalize_kind="loud")
    with pytest.raises(ValueError, match="target"):
        n.intensity_sweep(wav, torch.zeros(3, 256), clip_factor=[5], normalize=float("inf"))


@pytest.mark.parametrize("extra,word", [(["--normalize"], "--sweep"), (["--normalize", "-20"], "--sweep"),
                                        (["--sweep", "--clip", "5", "--normalize", "nan"], "--normalize"),
                                        (["--sweep", "--clip", "5", "--normalize", "abc"], "--normalize")])
def test_cli_refuses_normalize_without_sweep_and_levels_that_are_not_finite(extra, word, monkeypatch, capsys):
    from nomad_amd import __main__ as cli
    monkeypatch.setattr(cli, "Nomad", lambda **kw: pytest.fail("the CLI built a Nomad"))
    monkeypatch.setattr(sys, "argv", ["nomad_amd", "--nmr", "a", "--deg", "b"] + extra)
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert e.value.code == 2 and word in capsys.readouterr().err


@pytest.mark.parametrize("extra,want", [(["--normalize"], -23.0), (["--normalize", "-18.5"], -18.5), ([], None)])
def test_cli_hands_the_level_to_the_sweep(extra, want, tmp_path, monkeypatch, capsys):
    import pandas as pd
    from nomad_amd import __main__ as cli
    nmr, deg, out = tmp_path / "nmr", tmp_path / "clean", tmp_path / "out"
    for d in (nmr, deg, out):
        d.mkdir()
    seen = {}

    class _Fake:
        def __init__(self, **kw):
            pass

        def get_embeddings(self, path):
            return pd.concat([pd.DataFrame({"filename": ["r0", "r1"]}), pd.DataFrame(np.ones((2, 256), dtype=np.float32))], axis=1)

        def intensity_sweep(self, clean, references, noise=None, snr_db=None, clip_factor=None, k=None, **kw):
            seen.update(kw)
            return {"CLIP": dict(table=pd.DataFrame({"Condition": [5.0, 40.0], "Distance": [0.3, 0.4]}), SRCC=1.0)}

    monkeypatch.setattr(cli, "Nomad", _Fake)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setattr(sys, "argv", ["nomad_amd", "--mode", "dir", "--nmr", str(nmr), "--deg", str(deg), "--results_path", str(out),
                                      "--sweep", "--clip", "5,40"] + extra)
    cli.main()
    assert seen == ({} if want is None else {"normalize": want})


def test_the_intensity_experiment_hands_the_config_key_to_the_sweep():
    import pandas as pd
    from nomad_amd import train as T
    seen = {}

    class _Sweep:
        def intensity_sweep(self, clean, references, noise=None, snr_db=None, clip_factor=None, **kw):
            seen.update(kw)
            table = pd.DataFrame({"Condition": [1.0, 2.0], "Distance": [0.5, 0.6]})
            return {"CLIP": dict(table=table, SRCC=1.0, embeddings=pd.DataFrame(), scores=np.zeros(2))}

    t = T.Training.__new__(T.Training)
    t.config, t.model, t.nomad = {"degrade_on_device": {"clean": "/clean", "clip": [5, 40], "normalize": -23}}, "model", _Sweep()
    t._load_model = lambda path, allow_w2v: None
    ref = pd.concat([pd.DataFrame({"reference": ["r0", "r1"]}), pd.DataFrame(np.ones((2, 256), dtype=np.float32))], axis=1)
    t.get_nmr_embeddings = lambda: ref.copy()
    t.eval_degradation_intensity("model.pt")
    assert seen == {"normalize": -23}
