"""CPU: the sox-style reverb's restatement ``freeverb_ref`` against the figures and properties include/nomad_hip.h states, the
binding of ``nomad_degrade_reverb``, and the argument errors of ``Engine.check_reverb`` / ``Nomad.intensity_sweep`` / the CLI that
need no GPU.  (The kernel itself is held to the restatement in test_gpu_freeverb.py.  Agreement with the sox binary is tested nowhere.)"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import freeverb_ref as F
import stream_screen
from conftest import ROOT
from nomad_amd import _lib
from nomad_amd.engine import Engine
from test_degrade_host import LENS, REFS, _SweepEngine, _clean, _nomad, _training


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_delay_tables_and_feedback_at_16_khz():
    ch = F.delays(16000)
    assert len(ch) == 2
    assert ch[0] == ([405, 431, 463, 492, 516, 541, 565, 587], [82, 124, 160, 202])
    assert ch[1] == ([409, 427, 468, 488, 520, 537, 569, 582], [86, 119, 164, 197])
    assert abs(F.feedback(0) - 0.3) < 1e-15 and abs(F.feedback(100) - 0.98) < 1e-15
    assert abs(F.feedback(50) - 0.8816784043380077) < 1e-15
    assert all(F.feedback(a) < F.feedback(a + 1) for a in range(100))


def test_short_rooms_and_one_channel():
    assert len(F.delays(16000, stereo_depth=0.0)) == 1 and len(F.delays(16000, stereo_depth=1.0)) == 2
    combs, allpasses = F.delays(16000, room_scale=0.0, stereo_depth=0.0)[0]
    assert (min(combs), max(combs)) == (40, 59) and allpasses == [82, 124, 160, 202], "the all-passes are not scaled by the room"
    assert min(F.delays(8000, room_scale=0.0)[0][0] + F.delays(8000, room_scale=0.0)[1][0]) == 20
    x = F.noise(900, 3)
    one = F.wet(x, 70, stereo_depth=0.0)
    assert one.shape == (1, 900) and np.array_equal(one[0], F.wet(x, 70)[0]), "channel 0 has no stereo offset"
    assert np.array_equal(F.mix(x, one, as_float32=False), x.astype(np.float64) + one[0])


def test_a_clip_shorter_than_every_delay_comes_back_and_one_sample_later_it_does_not():
    x = F.noise(400, 11)
    assert np.array_equal(F.reverb(x, 100).view(np.uint32), x.view(np.uint32))
    assert not F.wet(x, 100).any()
    y = F.noise(406, 12)
    out = F.reverb(y, 100)
    assert (out != y).nonzero()[0].tolist() == [405], "channel 0's shortest comb is 405 samples: x[0] reaches index 405 and nothing else moves"
    w = F.wet(y, 100)
    assert not w[1].any() and w[0, 405] == float(y[0]) * 0.015, "comb 0 returns x[0]; four empty all-passes flip its sign four times; the gain"


def test_the_wet_path_is_linear_and_shift_invariant():
    n = 1500
    a, b = F.noise(n, 21), F.noise(n, 22)
    wa, wb = F.wet(a, 80, pre_delay_ms=3), F.wet(b, 80, pre_delay_ms=3)
    both = F.wet((a.astype(np.float64) * 0.5 + b.astype(np.float64) * 0.25).astype(np.float32), 80, pre_delay_ms=3)
    # the sum is formed in float32 (the restatement takes float32 input): its rounding, at most 2^-24 of 0.1, passes through at most
    # 0.015 x 8 combs x 1 / (1 - 0.98) x 3^4 (an all-pass's response is -1, 1, 1/2, 1/4, ...: absolute sum 3)
    assert np.abs(both - (0.5 * wa + 0.25 * wb)).max() <= 2.0 ** -24 * 0.1 * 0.015 * 8 * 50 * 81
    assert np.array_equal(F.wet(a * np.float32(0.5), 80, pre_delay_ms=3), 0.5 * wa), "a power of two scales exactly"
    shifted = np.concatenate([np.zeros(37, dtype=np.float32), a])[:n]
    ws = F.wet(shifted, 80, pre_delay_ms=3)
    assert not ws[:, :37 + 48].any() and np.array_equal(ws[:, 37:], wa[:, :n - 37]), "delays, stores and lines start at zero: a shift is a shift"
    assert np.array_equal(F.wet(a, 80, pre_delay_ms=3)[:, 48:], F.wet(a, 80)[:, :n - 48]), "the pre-delay is 48 samples of delay"
    assert np.allclose(F.wet(a, 80, wet_gain_db=6.0), F.wet(a, 80) * 10.0 ** (6.0 / 20.0), rtol=1e-14, atol=0.0), "the wet gain is a factor"


def test_mix_limits_keeps_a_nan_and_rounds_once():
    x = np.array([0.5, -0.5, 0.25, np.nan], dtype=np.float32)
    w = np.array([[0.75, -0.75, 1e-9, 0.0]])
    assert F.mix(x, w).tolist()[:3] == [1.0, -1.0, float(np.float32(0.25 + 1e-9))] and np.isnan(F.mix(x, w)[3])
    assert F.mix(x, w, clamp=False).tolist()[:2] == [1.25, -1.25]
    assert F.mix(x, w, wet_only=True).tolist()[:3] == [0.75, -0.75, float(np.float32(1e-9))] and np.isnan(F.mix(x, w, wet_only=True)[3])
    two = np.array([[0.5, 0.0, 0.0, 0.0], [0.25, 0.0, 0.0, 0.0]])
    assert F.mix(x, two, wet_only=True)[0] == 0.375


# ---- the binding -----------------------------------------------------------------------------------------------------------------------
def _header_struct():
    """``nomad_reverb_params`` as include/nomad_hip.h declares it, rebuilt as a ctypes Structure from the header's own text."""
    text = open(os.path.join(ROOT, "include", "nomad_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} nomad_reverb_params;", text).group(1)
    fields = []
    for ctype, names in re.findall(r"\b(int|double)\s+([^;]+);", body):
        for name in names.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", name)
            t = {"int": C.c_int, "double": C.c_double}[ctype]
            fields.append((m.group(1), t * int(m.group(2)) if m.group(2) else t))
    return type("HeaderReverbParams", (C.Structure,), {"_fields_": fields})


def test_the_struct_is_the_headers():
    hdr = _header_struct()
    assert [n for n, _ in hdr._fields_] == [n for n, _ in _lib.ReverbParams._fields_] == [
        "G", "reverberance", "hf_damping", "room_scale", "stereo_depth", "pre_delay_ms", "wet_gain_db", "wet_only", "clamp", "sample_rate"]
    assert C.sizeof(hdr) == C.sizeof(_lib.ReverbParams) == 576
    for name, _ in hdr._fields_:
        assert getattr(hdr, name).offset == getattr(_lib.ReverbParams, name).offset, name
        assert getattr(hdr, name).size == getattr(_lib.ReverbParams, name).size, name
    assert _lib.ReverbParams.reverberance.size == 64 * 8


def test_the_entry_point_has_one_host_array_and_is_exported(built_lib):
    res, args = _lib.SIGNATURES["nomad_degrade_reverb"]
    slots = [t for t in args if isinstance(t, type) and issubclass(t, C._Pointer) and t._type_ in stream_screen._HOST_ELEMENTS]
    assert len(slots) == 1 and slots[0]._type_ is C.c_int, "the lengths are the call's only int/float/double host array: the levels travel in the struct"
    assert "nomad_degrade_reverb" not in stream_screen._ROLES
    assert res is C.c_int and len(args) == 10 and args[5]._type_ is _lib.ReverbParams
    assert _lib.SIGNATURES["nomad_degrade_reverb_scratch_bytes"] == (C.c_size_t, [C.c_int] * 4)
    lib = C.CDLL(built_lib)
    assert hasattr(lib, "nomad_degrade_reverb") and hasattr(lib, "nomad_degrade_reverb_scratch_bytes")
    loaded = _lib.load()
    assert loaded.nomad_abi_version() == 3
    size = loaded.nomad_degrade_reverb_scratch_bytes
    assert 16 * 3 * 30 * 8000 <= size(3, 8000, 30, 16000) <= 16 * 3 * 30 * 8000 + 1024, "16 bytes per output sample plus the tables"
    assert size(3, 8000, 65, 16000) == 0 and loaded.nomad_last_error()
    assert size(0, 8000, 1, 16000) == 0 and size(3, 8002, 1, 16000) == 0 and size(3, 8000, 1, 7999) == 0 and size(3, 8000, 1, 48001) == 0
    # without a context the call is refused before anything else happens
    assert loaded.nomad_degrade_reverb(None, None, 1, 4, None, None, None, None, 0, None) == _lib.NOMAD_ERR_INVALID


# ---- arguments that need no GPU ----------------------------------------------------------------------------------------------------------
def test_check_reverb_builds_the_struct_and_refuses_what_the_abi_refuses():
    p = Engine.check_reverb([1, 50, 100], hf_damping=30, pre_delay_ms=20, wet_only=True, clamp=False, sample_rate=8000)
    assert (p.G, list(p.reverberance[:3]), p.hf_damping, p.room_scale, p.stereo_depth, p.pre_delay_ms, p.wet_gain_db, p.wet_only, p.clamp,
            p.sample_rate) == (3, [1.0, 50.0, 100.0], 30.0, 100.0, 100.0, 20.0, 0.0, 1, 0, 8000)
    d = Engine.check_reverb(50)
    assert (d.G, d.reverberance[0], d.hf_damping, d.wet_only, d.clamp, d.sample_rate) == (1, 50.0, 50.0, 0, 1, 16000)
    assert Engine.check_reverb(np.array([3.0, 6.0])).G == 2 and Engine.check_reverb(torch.tensor([3.0])).G == 1
    for kw, word in ((dict(reverberance=[101]), "reverberance"), (dict(reverberance=[-1]), "reverberance"), (dict(reverberance=[float("nan")]), "reverberance"),
                     (dict(reverberance=[]), "1 .. 64"), (dict(reverberance=[1] * 65), "1 .. 64"), (dict(hf_damping=100.5), "hf_damping"),
                     (dict(room_scale=-1), "room_scale"), (dict(stereo_depth=float("inf")), "stereo_depth"), (dict(pre_delay_ms=501), "pre_delay_ms"),
                     (dict(wet_gain_db=-10.5), "wet_gain_db"), (dict(sample_rate=7999), "sample_rate"), (dict(sample_rate=48001), "sample_rate")):
        args = dict(reverberance=[50])
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            Engine.check_reverb(**args)


def test_sweep_refuses_both_reverbs_before_it_touches_the_engine():
    from nomad_amd.nomad import Nomad
    n = Nomad.__new__(Nomad)          # no engine: every refusal below comes before the first use of one
    refs = torch.zeros(4, 256)
    clean = torch.zeros(2, 800)
    with pytest.raises(ValueError, match="both fill the REVERB entry"):
        n.intensity_sweep(clean, refs, rt60_s=[0.1], reverberance=[50])
    with pytest.raises(ValueError, match="reverb_params go with reverberance"):
        n.intensity_sweep(clean, refs, rt60_s=[0.1], reverb_params={"hf_damping": 10})
    with pytest.raises(ValueError, match="reverberance"):
        n.intensity_sweep(clean, refs, reverberance=[50, 100.5])
    with pytest.raises(ValueError, match="1 .. 64"):
        n.intensity_sweep(clean, refs, reverberance=list(range(65)))
    with pytest.raises(ValueError, match="room_scale"):
        n.intensity_sweep(clean, refs, reverberance=[50], reverb_params={"room_scale": 101})
    with pytest.raises(TypeError):
        n.intensity_sweep(clean, refs, reverberance=[50], reverb_params={"rt60": 1})
    with pytest.raises(ValueError, match="or reverberance"):
        n.intensity_sweep(clean, refs)


@pytest.mark.parametrize("extra,word", [
    (["--reverb", "1,50"], "--reverb goes with --sweep"),
    (["--sweep", "--reverb", "1,50", "--rt60", "0.2"], "exclude each other"),
    (["--sweep", "--reverb", "1,101"], "from 0 to 100"),
    (["--sweep", "--reverb", "-1"], "from 0 to 100"),
    (["--sweep", "--reverb", ",".join(["5"] * 65)], "1 to 64 levels"),
    (["--sweep", "--reverb", "a,b"], "numbers separated by commas"),
    (["--sweep"], "or --reverb"),
])
def test_cli_argument_errors(extra, word, monkeypatch, capsys):
    from nomad_amd import __main__ as cli
    monkeypatch.setattr(cli, "Nomad", lambda **kw: pytest.fail("the CLI built a Nomad"))
    monkeypatch.setattr(sys, "argv", ["nomad_amd", "--nmr", "a", "--deg", "b"] + extra)
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert e.value.code == 2 and word in capsys.readouterr().err


class _FreeverbEngine(_SweepEngine):
    """``_SweepEngine`` with the reverb: a row holds its clip's value + reverberance / 1000; the shared parameters are recorded."""

    def degrade_reverb(self, buf, reverberance, lengths=None, **params):
        self.calls.append(("params", params))
        out, lens_rep, _ = self._degrade("freeverb", buf, reverberance, lengths)
        return out, lens_rep


def test_sweep_rows_table_and_parameters():
    eng = _FreeverbEngine()
    n = _nomad(eng)
    res = n.intensity_sweep(_clean(), REFS, clip_factor=[5], lengths=LENS, reverberance=[50, 1, 100], reverb_params={"hf_damping": 20})
    assert list(res) == ["CLIP", "REVERB"]
    assert [c for c in eng.calls if c[0] in ("clip", "params", "freeverb")] == [
        ("clip", LENS, [5.0]), ("params", {"hf_damping": 20}), ("freeverb", LENS, [50.0, 1.0, 100.0])]
    want = [b + 1 + v / 1000 for b in range(4) for v in (50, 1, 100)]
    assert np.allclose(res["REVERB"]["scores"], want, atol=1e-6), "row b G + g is clip b at reverberance[g]"
    assert sorted(res["REVERB"]["table"]["Condition"].tolist()) == [1.0, 50.0, 100.0]
    rows, lens = n.reverb(_clean().unsqueeze(1), [3, 95], lengths=LENS, wet_only=True)
    assert rows.shape == (8, 3000) and lens == [1000] * 6 + [3000] * 2 and eng.calls[-2:] == [("params", {"wet_only": True}),
                                                                                             ("freeverb", LENS, [3.0, 95.0])]
    eng.calls.clear()
    with pytest.raises(ValueError, match="produces no gradient"):
        n.reverb(_clean().requires_grad_(True), [50])
    with pytest.raises(ValueError, match=r"\(B,1,N\) or \(B,N\)"):
        n.reverb(torch.zeros(3000), [50])
    with pytest.raises(ValueError, match="reverberance"):
        n.reverb(_clean(), [150])
    assert eng.calls == []


def test_config_key_and_cli_pass_the_levels_on(tmp_path, monkeypatch, capsys):
    seen = {}

    class _Sweep:
        def __init__(self, **kw):
            pass

        def get_embeddings(self, path):
            return pd.concat([pd.DataFrame({"filename": ["r0", "r1"]}), pd.DataFrame(np.ones((2, 256), dtype=np.float32))], axis=1)

        def intensity_sweep(self, clean, references, noise=None, snr_db=None, clip_factor=None, k=None, **kw):
            seen.update(clean=clean, snr_db=snr_db, clip=clip_factor, kw=kw)
            table = pd.DataFrame({"Condition": [50.0, 1.0], "Distance": [0.6, 0.5]})
            return {"REVERB": dict(table=table, SRCC=1.0, embeddings=pd.DataFrame(), scores=np.zeros(2))}

    t = _training({"degrade_on_device": {"clean": "/clean", "reverb": [1, 50], "normalize": -23}}, [], _Sweep())
    res = t.eval_degradation_intensity("model.pt")
    assert seen == dict(clean="/clean", snr_db=None, clip=None, kw={"reverberance": [1, 50], "normalize": -23})
    assert sorted(res) == ["REVERB"] and "ref_embeddings" in res["REVERB"]

    from nomad_amd import __main__ as cli
    nmr, deg, out = tmp_path / "nmr", tmp_path / "clean", tmp_path / "out"
    for d in (nmr, deg, out):
        d.mkdir()
    monkeypatch.setattr(cli, "Nomad", _Sweep)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setattr(sys, "argv", ["nomad_amd", "--mode", "dir", "--nmr", str(nmr), "--deg", str(deg), "--results_path", str(out),
                                      "--sweep", "--reverb", "1,50", "--normalize"])
    cli.main()
    assert seen == dict(clean=str(deg), snr_db=None, clip=None, kw={"reverberance": [1.0, 50.0], "normalize": -23.0})
    back = pd.read_csv(out / "nomad_intensity.csv")
    assert back.to_dict("list") == {"Degradation": ["REVERB", "REVERB"], "Condition": [1.0, 50.0], "NOMAD": [0.5, 0.6]}
    assert "REVERB: SRCC" in capsys.readouterr().out
