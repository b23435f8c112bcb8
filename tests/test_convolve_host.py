"""CPU: the host side of reverberation on the device - ``synthetic_rir`` against its stated formula, the two exports, and the argument
handling of ``Nomad.convolve`` / ``Nomad.intensity_sweep(rt60_s=...)`` / ``Training.eval_degradation_intensity`` / the CLI's
``--rt60`` against recording fake engines (the kernel itself: tests/test_gpu_convolve.py)."""
import ctypes as C
import math
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from nomad_amd import train as T
from nomad_amd.nomad import Nomad, synthetic_rir
from test_degrade_host import LENS, REFS, _SweepEngine, _clean, _nomad, _training


# ---- synthetic_rir ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt60,seed,drr", [(0.1, 0, 0.0), (0.25, 3, 6.0), (0.5, 1, -3.0), (0.01, 7, 0.0), (4.096, 2, 10.0), (2e-4, 0, 0.0)])
def test_synthetic_rir_is_the_stated_formula(rt60, seed, drr):
    h = synthetic_rir(rt60, seed, drr)
    L = min(math.ceil(rt60 * 16000), 65536)
    assert h.dtype == np.float32 and h.shape == (L,) and h[0] == 1.0
    r = np.random.RandomState(seed).standard_normal(L)
    tail = r * 10.0 ** (-3.0 * np.arange(L) / (rt60 * 16000))
    tail[0] = 0.0
    tail *= np.sqrt(10.0 ** (-drr / 10.0) / np.sum(tail ** 2))
    tail[0] = 1.0
    assert np.array_equal(h, tail.astype(np.float32))
    energy = float(np.sum(h[1:].astype(np.float64) ** 2))
    assert abs(energy - 10.0 ** (-drr / 10.0)) <= 1e-6 * 10.0 ** (-drr / 10.0)
    assert np.array_equal(h, synthetic_rir(rt60, seed, drr)), "one seed, one room"
    if L > 4:
        assert not np.array_equal(h, synthetic_rir(rt60, seed + 1, drr)), "another seed, another room"


def test_synthetic_rir_defaults_lengths_and_refusals():
    assert np.array_equal(synthetic_rir(0.05), synthetic_rir(0.05, seed=0, drr_db=0.0))
    assert synthetic_rir(0.05).shape == (800,) and synthetic_rir(0.05 + 1e-6).shape == (801,) and synthetic_rir(4.096).shape == (65536,)
    one = synthetic_rir(1.0 / 16000)
    assert one.shape == (1,) and one[0] == 1.0, "a room of one tap is the direct path"
    for bad in (0.0, -0.1, 4.097, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rt60_s"):
            synthetic_rir(bad)
    with pytest.raises(ValueError, match="drr_db"):
        synthetic_rir(0.1, drr_db=float("nan"))


# ---- the exports -----------------------------------------------------------------------------------------------------------------
def test_the_two_entry_points_are_bound_and_exported(built_lib):
    from nomad_amd import _lib
    lib = C.CDLL(built_lib)
    for name, n in {"nomad_degrade_convolve_scratch_bytes": 2, "nomad_degrade_convolve": 13}.items():
        assert len(_lib.SIGNATURES[name][1]) == n, name
        assert hasattr(lib, name), f"{name} is not exported"
    assert _lib.SIGNATURES["nomad_degrade_convolve_scratch_bytes"][0] is C.c_size_t
    loaded = _lib.load()
    assert loaded.nomad_abi_version() == 3
    assert loaded.nomad_degrade_convolve_scratch_bytes(3, 64) >= 4 * (3 + 64)
    assert loaded.nomad_degrade_convolve_scratch_bytes(3, 65) == 0 and loaded.nomad_last_error()
    assert loaded.nomad_degrade_convolve_scratch_bytes(0, 1) == 0 and loaded.nomad_degrade_convolve_scratch_bytes(3, 0) == 0
    # without a context the call is refused before anything else happens
    assert loaded.nomad_degrade_convolve(None, None, 1, 4, None, None, 1, 4, None, None, None, 0, None) == _lib.NOMAD_ERR_INVALID


# ---- a recording fake engine -----------------------------------------------------------------------------------------------------
class _ReverbEngine(_SweepEngine):
    """``_SweepEngine`` with the convolution: a row holds its clip's value + (taps of its response) / 1e6."""

    def pack_responses(self, irs, ir_lengths=None):
        rows = [torch.as_tensor(h).reshape(-1) for h in irs]
        lens = [int(h.numel()) for h in rows] if ir_lengths is None else [int(n) for n in ir_lengths]
        self.calls.append(("responses", lens))
        return torch.zeros(len(lens), max(lens)), lens

    def degrade_convolve(self, buf, irs, lengths=None, ir_lengths=None):
        if not isinstance(irs, tuple):
            irs = self.pack_responses(irs, ir_lengths)
        out, lens_rep, _ = self._degrade("reverb", buf, [n / 1000.0 for n in irs[1]], lengths)
        return out, lens_rep


def test_convolve_rows_lengths_and_refusals():
    eng = _ReverbEngine()
    n = _nomad(eng)
    irs = [torch.ones(3), np.ones(800, dtype=np.float32)]
    rows, lens = n.convolve(_clean().unsqueeze(1), irs, lengths=LENS)
    assert rows.shape == (8, 3000) and lens == [1000] * 6 + [3000] * 2
    assert eng.calls == [("responses", [3, 800]), ("reverb", LENS, [0.003, 0.8])]
    assert torch.allclose(rows[:, 0], torch.tensor([b + 1 + v / 1e6 for b in range(4) for v in (3, 800)], dtype=torch.float32)), "row b G + g"
    eng.calls.clear()
    rows, lens = n.convolve(_clean(), torch.ones(2, 40), ir_lengths=[40, 7])
    assert rows.shape == (8, 3000) and lens == [3000] * 8 and eng.calls == [("responses", [40, 7]), ("reverb", [3000] * 4, [0.04, 0.007])]
    eng.calls.clear()
    with pytest.raises(ValueError, match=r"\(B,1,N\) or \(B,N\)"):
        n.convolve(torch.zeros(3000), irs)
    with pytest.raises(ValueError, match="produces no gradient"):
        n.convolve(_clean().requires_grad_(True), irs)
    with pytest.raises(ValueError, match="produces no gradient"):
        n.convolve(_clean(), [torch.ones(3, requires_grad=True)])
    with pytest.raises(ValueError, match="1 .. 64"):
        n.convolve(_clean(), [torch.ones(3)] * 65)
    with pytest.raises(ValueError, match="1 .. 64"):
        n.convolve(_clean(), [])
    with pytest.raises(ValueError, match="1 .. 64"):
        n.convolve(_clean(), torch.ones(3))
    with pytest.raises(ValueError, match="'noise' or 'clip'"):
        n.degrade(_clean(), "reverb", [0.5])
    assert eng.calls == []


@pytest.mark.parametrize("k", [None, 2])
def test_sweep_reverb_row_order_batches_and_table(k, capsys):
    eng = _ReverbEngine()
    n = _nomad(eng)
    rt60 = [0.05, 0.0125, 0.025]                     # 800, 200 and 400 taps
    res = n.intensity_sweep(_clean(), REFS, clip_factor=[5, 60], lengths=LENS, k=k, max_batch_samples=6000, rt60_s=rt60, rir_seed=4)
    cuts = [[1000, 1000], [1000], [3000]]            # 6000 samples over 3 rows per clip: as in test_degrade_host
    want = []
    for lens in cuts:
        want += [("clip", lens, [5.0, 60.0]), ("embed", 2 * sum(lens), "fp32"), ("reverb", lens, [0.8, 0.2, 0.4]), ("embed", 3 * sum(lens), "fp32")]
    want.insert(2, ("responses", [800, 200, 400]))   # packed once, with the first batch
    assert eng.calls == want + [("knn", 8, 2) if k else ("pairwise", 8), ("knn", 12, 2) if k else ("pairwise", 12)]
    assert sorted(res) == ["CLIP", "REVERB"]
    r = res["REVERB"]
    assert sorted(r) == ["SRCC", "embeddings", "scores", "table"]
    assert np.allclose(r["scores"], [b + 1 + v / 1e6 for b in range(4) for v in (800, 200, 400)], atol=1e-6), "row b G + g is clip b in room g"
    t = r["table"].sort_values(by="Condition")
    assert list(r["table"].columns) == ["Condition", "Distance"] and t["Condition"].tolist() == sorted(rt60)
    assert np.allclose(t["Distance"], [2.5 + v / 1e6 for v in (200, 400, 800)], atol=1e-6)
    assert list(r["embeddings"]["filepath_deg"][:3]) == ["clip0|REVERB_0", "clip0|REVERB_1", "clip0|REVERB_2"]
    # reverberation alone
    eng.calls.clear()
    only = n.intensity_sweep(_clean(), REFS, lengths=LENS, rt60_s=[0.05])
    assert sorted(only) == ["REVERB"] and eng.calls == [("responses", [800]), ("reverb", LENS, [0.8]), ("embed", 6000, "fp32"), ("pairwise", 4)]


def test_sweep_without_rt60_is_the_call_list_as_before():
    a, b = _ReverbEngine(), _ReverbEngine()
    args = dict(noise=torch.ones(5), snr_db=[40, 0], clip_factor=[5, 60], lengths=LENS, max_batch_samples=6000)
    _nomad(a).intensity_sweep(_clean(), REFS, **args)
    _nomad(b).intensity_sweep(_clean(), REFS, rt60_s=None, rir_seed=9, drr_db=3.0, **args)
    assert a.calls == b.calls and not any(c[0] in ("reverb", "responses") for c in a.calls)
    want = []
    for lens in ([1000, 1000, 1000], [3000]):
        want += [("noise", lens, [40.0, 0.0]), ("embed", 2 * sum(lens), "fp32"), ("clip", lens, [5.0, 60.0]), ("embed", 2 * sum(lens), "fp32")]
    assert a.calls == want + [("pairwise", 8), ("pairwise", 8)]


def test_sweep_reverb_refusals():
    eng = _ReverbEngine()
    n = _nomad(eng)
    with pytest.raises(ValueError, match="snr_db, clip_factor or both, or rt60_s"):
        n.intensity_sweep(_clean(), REFS)
    with pytest.raises(ValueError, match="1 .. 64 levels"):
        n.intensity_sweep(_clean(), REFS, rt60_s=[0.1] * 65)
    for bad in ([0.0], [0.1, 4.1], [float("nan")]):
        with pytest.raises(ValueError, match="rt60_s"):
            n.intensity_sweep(_clean(), REFS, rt60_s=bad)
    with pytest.raises(ValueError, match="produces no gradient"):
        n.intensity_sweep(_clean().requires_grad_(True), REFS, rt60_s=[0.1])
    assert eng.calls == []


# ---- Training.eval_degradation_intensity and the CLI -----------------------------------------------------------------------------
def test_eval_degradation_intensity_passes_rt60(capsys):
    seen = {}

    class _Sweep:
        def intensity_sweep(self, clean, references, noise=None, snr_db=None, clip_factor=None, **kw):
            seen.update(clean=clean, snr_db=snr_db, clip=clip_factor, kw=kw)
            table = pd.DataFrame({"Condition": [0.1, 0.5], "Distance": [0.5, 0.6]})
            return {"REVERB": dict(table=table, SRCC=1.0, embeddings=pd.DataFrame(), scores=np.zeros(2))}

    t = _training({"degrade_on_device": {"clean": "/clean", "rt60": [0.1, 0.5]}}, [], _Sweep())
    res = t.eval_degradation_intensity("model.pt")
    assert seen == dict(clean="/clean", snr_db=None, clip=None, kw={"rt60_s": [0.1, 0.5]})
    assert sorted(res) == ["REVERB"] and "ref_embeddings" in res["REVERB"]


@pytest.mark.parametrize("extra,word", [(["--rt60", "0.5"], "--sweep"),
                                        (["--sweep", "--rt60", "0.5,abc"], "--rt60"),
                                        (["--sweep", "--rt60", "0"], "--rt60"),
                                        (["--sweep", "--rt60", "0.5,4.2"], "--rt60"),
                                        (["--sweep", "--rt60", ",".join(["0.5"] * 65)], "--rt60"),
                                        (["--sweep"], "--snr-db (with --noise), --clip or both")])
def test_cli_argument_errors(extra, word, monkeypatch, capsys):
    from nomad_amd import __main__ as cli
    monkeypatch.setattr(cli, "Nomad", lambda **kw: pytest.fail("the CLI built a Nomad"))
    monkeypatch.setattr(sys, "argv", ["nomad_amd", "--nmr", "a", "--deg", "b"] + extra)
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_cli_sweep_passes_rt60_and_writes_the_table(tmp_path, monkeypatch, capsys):
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

        def intensity_sweep(self, clean, references, noise=None, snr_db=None, clip_factor=None, k=None, rt60_s=None):
            seen.update(clean=clean, noise=noise, snr_db=snr_db, clip=clip_factor, k=k, rt60_s=rt60_s)
            return {"REVERB": dict(table=pd.DataFrame({"Condition": [0.5, 0.1], "Distance": [0.25, 0.2]}), SRCC=1.0)}

    monkeypatch.setattr(cli, "Nomad", _Fake)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setattr(sys, "argv", ["nomad_amd", "--mode", "dir", "--nmr", str(nmr), "--deg", str(deg), "--results_path", str(out),
                                      "--sweep", "--rt60", "0.1,0.5"])
    cli.main()
    assert seen == dict(clean=str(deg), noise=None, snr_db=None, clip=None, k=None, rt60_s=[0.1, 0.5])
    back = pd.read_csv(out / "nomad_intensity.csv")
    assert back.to_dict("list") == {"Degradation": ["REVERB", "REVERB"], "Condition": [0.1, 0.5], "NOMAD": [0.2, 0.25]}
    assert "REVERB: SRCC" in capsys.readouterr().out
