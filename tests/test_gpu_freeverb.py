"""GPU: ``nomad_degrade_reverb`` through the C ABI in guarded, NaN-poisoned buffers, against the sample-by-sample float64
restatement ``freeverb_ref``; then ``Nomad.reverb`` / ``Nomad.intensity_sweep(reverberance=...)`` end to end.

What is held here is the algorithm as include/nomad_hip.h states it (restated from memory of sox 14.4 reverb.c).  Agreement with
the sox binary is NOT tested anywhere: sox was not available where this was written.

The bound, for every sample:  |out - ref| <= 2^-24 |ref| + 1e-12 max|x|, ref the float64 value before its one rounding.
* 2^-24 |ref| is that one rounding to fp32.
* 1e-12 max|x| bounds the float64 reassociation of the kernel's ``store`` scan against the serial recurrence: a few units of 2^-53 per
  sample, amplified by at most 1 / (1 - 0.98) = 50; it sits five orders under the first term.
Each case prints the largest deviation it found in units of that bound.

Clips are 0.1-amplitude seeded noise: the output stays under 0.5, so the clamp is idle unless a case is about it.  Lengths: 400
(below every delay of channel 0 at the defaults: the wet path of channel 0 is silent), 1181 (just past 2 x 587 + 1: the longest comb
has come round twice) and 5003 (78 tiles and a partial one); no length is a multiple of the 64-sample tile."""
import ctypes as C

import numpy as np
import pytest
import torch

import freeverb_ref as F
import guard
from nomad_amd import _lib

pytestmark = pytest.mark.gpu

LENS = [400, 1181, 5003]
STRIDE = 5016                      # slack behind the longest clip
LEVELS = [1.0, 50.0, 100.0]
NAN = float("nan")
SHORT = dict(room_scale=0.0, stereo_depth=0.0, pre_delay_ms=20.0, wet_gain_db=10.0)      # combs of 40 .. 59 samples, one channel
_WET = {}


def _clips(amp=0.1):
    return [F.noise(n, 900 + n, amp) for n in LENS]


def _key(p):
    return tuple(sorted((k, float(v)) for k, v in p.items() if k not in ("wet_only", "clamp")))


def _wet(tag, x, level, p):
    """``freeverb_ref.wet`` of one clip at one level, computed once per (clip, level, parameters) and never modified."""
    k = (tag, float(level), _key(p))
    if k not in _WET:
        args = {n: p[n] for n in ("hf_damping", "room_scale", "stereo_depth", "pre_delay_ms", "wet_gain_db", "sample_rate") if n in p}
        _WET[k] = F.wet(x, level, **args)
        _WET[k].setflags(write=False)
    return _WET[k]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _params(levels, **p):
    q = dict(F.DEFAULTS)
    q.update(p)
    s = _lib.ReverbParams(G=len(levels), hf_damping=q["hf_damping"], room_scale=q["room_scale"], stereo_depth=q["stereo_depth"],
                          pre_delay_ms=q["pre_delay_ms"], wet_gain_db=q["wet_gain_db"], wet_only=int(q["wet_only"]), clamp=int(q["clamp"]),
                          sample_rate=int(q["sample_rate"]))
    for g, v in enumerate(levels[:64]):
        s.reverberance[g] = v
    return s


class _Call:
    """One ABI call in guarded buffers: input rows NaN behind their length, output NaN-filled, workspace 0xFF (NaN as float64)."""

    def __init__(self, engine, rows, levels, stride=None, x_off=0, out_off=0, **p):
        self.engine, self.rows, self.levels, self.p = engine, rows, list(levels), p
        self.B, self.G = len(rows), len(levels)
        self.lens = [int(r.shape[0]) for r in rows]
        self.stride = stride if stride is not None else (max(self.lens) + 3) // 4 * 4
        dev = engine.device
        self.guards = g = guard.Guards()
        host = np.full((self.B, self.stride), np.nan, dtype=np.float32)
        for b, x in enumerate(rows):
            host[b, :self.lens[b]] = x
        self.x = g.empty_at((self.B, self.stride), x_off, device=dev, name="x")
        self.x.copy_(torch.from_numpy(host))
        self.out = g.empty_at((self.B * self.G, self.stride), out_off, device=dev, name="out")
        self.out.fill_(NAN)
        fs = int(p.get("sample_rate", 16000))
        need = int(engine.lib.nomad_degrade_reverb_scratch_bytes(self.B, self.stride, self.G, fs))
        self.ws = g.empty_bytes(max(need, 256), dev, 1 << 16, "workspace")
        self.ws.fill_(0xFF)
        self.ws_bytes = need

    def run(self, **over):
        a = dict(x=self.x.data_ptr(), B=self.B, stride=self.stride, lens=self.lens, params=_params(self.levels, **self.p),
                 out=self.out.data_ptr(), ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(over)
        lens = (C.c_int * len(a["lens"]))(*a["lens"]) if a["lens"] is not None else None
        params = C.byref(a["params"]) if a["params"] is not None else None
        rc = self.engine.lib.nomad_degrade_reverb(self.engine.ctx, a["x"], a["B"], a["stride"], lens, params, a["out"], a["ws"], a["ws_bytes"],
                                                  self.engine._stream())
        if lens is not None:      # both host objects may die on return: they do
            lens[:] = [1] * len(lens)
        if a["params"] is not None:
            C.memset(C.byref(a["params"]), 0xFF, C.sizeof(a["params"]))
        torch.cuda.synchronize()
        return rc

    def results(self):
        self.guards.check()
        return self.out.cpu().numpy()


def _judge(out, rows, levels, p, case, tags=None):
    """Every row against the float64 reference within the module's bound, zeros behind every length -> the largest deviation / bound."""
    G, worst = len(levels), 0.0
    for b, x in enumerate(rows):
        n = x.shape[0]
        for g, level in enumerate(levels):
            w = _wet(tags[b] if tags else (case.split("/")[0], b), x, level, p)
            ref = F.mix(x, w, p.get("wet_only", False), p.get("clamp", True), as_float32=False)
            got = out[b * G + g]
            bound = 2.0 ** -24 * np.abs(ref) + 1e-12 * float(np.abs(x).max())
            dev = np.abs(got[:n].astype(np.float64) - ref)
            assert np.isfinite(got[:n]).all(), (case, b, g)
            ratio = float((dev / bound).max())
            worst = max(worst, ratio)
            assert (dev <= bound).all(), (case, b, level, "largest deviation / bound", ratio, "at", int(np.argmax(dev / bound)))
            assert not got[n:].any() and not np.isnan(got[n:]).any(), f"{case} clip {b} level {level}: not zero behind the length"
    print(f"{case}: largest deviation = {worst:.4f} of the bound 2^-24 |ref| + 1e-12 max|x|")
    return worst


# ---- the rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wet_only", [True, False], ids=["wet", "dry+wet"])
def test_rows_match_the_float64_recurrence(engine, wet_only):
    rows = _clips()
    call = _Call(engine, rows, LEVELS, stride=STRIDE, wet_only=wet_only)
    assert call.run() == 0, engine.lib.nomad_last_error()
    out = call.results()
    assert np.abs(out[~np.isnan(out)]).max() < 0.5, "the clamp is meant to be idle here"
    _judge(out, rows, LEVELS, dict(wet_only=wet_only), "defaults/" + ("wet" if wet_only else "dry+wet"), tags=[("clip", n) for n in LENS])
    if wet_only:
        assert not out[0:3, :400].any(), "400 samples are shorter than every delay of both channels: the wet path is silent"
        assert out[3, :1181].any()


@pytest.mark.parametrize("hf_damping", [0.0, 100.0])
def test_delays_shorter_than_a_wave(engine, hf_damping):
    """room_scale = 0: combs of 40 .. 59 samples, so the tile is 40 and 24 lanes idle; one channel; a pre-delay of 320 samples."""
    assert min(F.delays(16000, 0.0, 0.0)[0][0]) == 40 and max(F.delays(16000, 0.0, 0.0)[0][0]) == 59 and len(F.delays(16000, 0.0, 0.0)) == 1
    rows = _clips()
    p = dict(SHORT, hf_damping=hf_damping, wet_only=True)
    call = _Call(engine, rows, LEVELS, stride=STRIDE, **p)
    assert call.run() == 0, engine.lib.nomad_last_error()
    out = call.results()
    assert np.abs(out[~np.isnan(out)]).max() < 0.5
    assert not out[:, :320 + 40].any() and out[:, 360:400].any(), "nothing before pre-delay + shortest comb, something right behind it"
    _judge(out, rows, LEVELS, p, f"short/{hf_damping:g}", tags=[("clip", n) for n in LENS])


def test_8_khz_and_48_khz(engine):
    """The ends of the sample-rate range: combs from 20 samples (8 kHz, room_scale 0) and delay lines of 118 KB (48 kHz)."""
    x = [F.noise(1501, 77)]
    for fs, p in ((8000, dict(room_scale=0.0, wet_only=True)), (48000, dict(wet_only=True))):
        call = _Call(engine, x, [100.0], sample_rate=fs, **p)
        assert call.run() == 0, engine.lib.nomad_last_error()
        _judge(call.results(), x, [100.0], dict(p, sample_rate=fs), f"fs{fs}")


def test_the_clamp_limits_and_its_absence_does_not(engine):
    rows = [F.noise(1181, 31, 2.0), F.noise(2000, 32, 2.0)]
    for clamp in (True, False):
        call = _Call(engine, rows, [100.0], clamp=clamp)
        assert call.run() == 0
        out = call.results()
        for b, x in enumerate(rows):
            n = x.shape[0]
            ref = F.mix(x, _wet(("loud", b), x, 100.0, {}), False, clamp, as_float32=False)
            assert (np.abs(ref) > 1.0).any() != clamp
            bound = 2.0 ** -24 * np.abs(ref) + 1e-12 * float(np.abs(x).max())
            assert (np.abs(out[b, :n].astype(np.float64) - ref) <= bound).all(), (clamp, b)
            if clamp:
                free = F.mix(x, _wet(("loud", b), x, 100.0, {}), False, False, as_float32=False)
                assert (out[b, :n][free > 1.0] == 1.0).all() and (out[b, :n][free < -1.0] == -1.0).all() and (np.abs(free) > 1.0).sum() > 100
            else:
                assert np.abs(out[b, :n]).max() > 1.5


# ---- a row is its clip's own call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offs", [(0, 0), (1, 3), (2, 1), (3, 2)], ids=lambda o: "x%d-out%d" % o)
def test_a_row_has_the_bits_of_its_own_call(engine, offs):
    rows = _clips()
    batch = _Call(engine, rows, LEVELS, stride=STRIDE)
    assert batch.run() == 0
    out = batch.results()
    xo, oo = offs
    for b, x in enumerate(rows):
        n = x.shape[0]
        for g, level in enumerate(LEVELS):
            one = _Call(engine, [x], [level], x_off=xo, out_off=oo)
            assert one.x.data_ptr() % 16 == 4 * xo and one.out.data_ptr() % 16 == 4 * oo
            assert one.run() == 0, engine.lib.nomad_last_error()
            o1 = one.results()
            assert np.array_equal(_bits(o1[0, :n]), _bits(out[b * 3 + g, :n])), (b, level, offs)
            assert not o1[0, n:].any() and not np.isnan(o1[0, n:]).any()
    if offs != (0, 0):
        again = _Call(engine, rows, LEVELS, stride=STRIDE, x_off=xo, out_off=oo)
        assert again.run() == 0
        assert np.array_equal(_bits(again.results()), _bits(out)), "the batch at unaligned addresses (zeros behind the lengths included)"


# ---- non-finite input ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wet_only", [False, True], ids=["dry+wet", "wet"])
@pytest.mark.parametrize("bad,clamp", [(np.nan, True), (np.inf, False)], ids=["nan", "inf-unclamped"])
def test_a_non_finite_sample_stays_in_its_clip_and_behind_its_tile(engine, bad, clamp, wet_only):
    """A NaN passes the limit (both of its comparisons fail); an infinite value is limited to +-1 like any other value above 1, so
    the infinite sample runs without the limit."""
    p = 700
    clean = _clips()
    dirty = [x.copy() for x in clean]
    dirty[2][p] = bad
    ref = _Call(engine, clean, LEVELS, stride=STRIDE, wet_only=wet_only, clamp=clamp)
    assert ref.run() == 0
    out0 = ref.results()
    call = _Call(engine, dirty, LEVELS, stride=STRIDE, wet_only=wet_only, clamp=clamp)
    assert call.run() == 0
    out = call.results()
    assert np.array_equal(_bits(out[:6]), _bits(out0[:6])), "no row of another clip changes"
    for g in range(3):
        row = out[6 + g]
        assert not np.isfinite(row[p]), (g, row[p], "non-finite at p")
        assert np.array_equal(_bits(row[:p - p % 64]), _bits(out0[6 + g, :p - p % 64])), (g, "below p - p % 64 the clean run's bits")
        assert not row[5003:].any() and not np.isnan(row[5003:]).any(), "zeros stay behind the length"
        assert not np.isfinite(row[p + 405:p + 600]).all(), "and the loops bring it back"


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_anything_is_queued(engine):
    lib = engine.lib
    rows = [F.noise(800, 41), F.noise(400, 42)]

    def refused(status, what, levels=(50.0,), **over):
        p = {k: over.pop(k) for k in list(over) if k in F.DEFAULTS}
        call = _Call(engine, rows, list(levels))      # (buffers for the default parameters: a refusal does not depend on them)
        if p:
            over["params"] = _params(list(levels), **p)
        rc = call.run(**over)
        assert rc == status, (what, rc)
        assert lib.nomad_last_error(), what
        call.guards.check(what)
        assert bool(torch.isnan(call.out).all()), f"{what}: the output was written"
        assert bool((call.ws == 0xFF).all()), f"{what}: the workspace was written"

    inv = _lib.NOMAD_ERR_INVALID
    for name in ("x", "lens", "params", "out", "ws"):
        refused(inv, f"NULL {name}", **{name: None})
    g0, g65 = _params([50.0]), _params([50.0])
    g0.G, g65.G = 0, 65
    refused(inv, "G = 0", params=g0)
    refused(inv, "G = 65", params=g65)
    refused(inv, "B = 0", B=0)
    refused(inv, "B = 65536", B=65536)
    refused(inv, "stride no multiple of 4", stride=802)
    refused(inv, "stride = 0", stride=0)
    refused(inv, "stride shorter than a length", stride=796)
    refused(inv, "a length of 0", lens=[800, 0])
    for name, lo, hi in (("hf_damping", 0, 100), ("room_scale", 0, 100), ("stereo_depth", 0, 100), ("pre_delay_ms", 0, 500),
                         ("wet_gain_db", -10, 10)):
        for v in (lo - 0.5, hi + 0.5, NAN, float("inf")):
            refused(inv, f"{name} = {v}", **{name: v})
    for v in (-0.5, 100.5, NAN, float("-inf")):
        refused(inv, f"reverberance = {v}", levels=(50.0, v))
    refused(inv, "sample_rate below 8000", sample_rate=7999)
    refused(inv, "sample_rate above 48000", sample_rate=48001)
    call = _Call(engine, rows, [50.0])
    assert call.run(out=call.x.data_ptr() + 4 * call.stride) == inv, "an output one row into the input"
    call.guards.check()
    assert np.array_equal(_bits(call.x.cpu().numpy()[0]), _bits(rows[0])) and bool((call.ws == 0xFF).all())
    assert call.run(x=call.out.data_ptr() + 4 * (call.stride - 4)) == inv, "an input that ends inside the output"
    assert bool(torch.isnan(call.out).all())
    refused(_lib.NOMAD_ERR_WORKSPACE, "a short workspace", ws_bytes=1024)
    size = lib.nomad_degrade_reverb_scratch_bytes
    assert size(0, 800, 1, 16000) == 0 and size(2, 802, 1, 16000) == 0 and size(2, 800, 65, 16000) == 0 and size(2, 800, 1, 7999) == 0
    assert size(65536, 800, 1, 16000) == 0 and size(2, 800, 0, 16000) == 0 and size(2, 800, 1, 48001) == 0
    assert 16 * 2 * 3 * 800 <= size(2, 800, 3, 16000) <= 16 * 2 * 3 * 800 + 1024, "16 bytes per output sample plus the tables"


# ---- the caller's stream, the caller's host memory --------------------------------------------------------------------------------------
def test_the_call_keeps_to_the_callers_stream_and_is_done_with_host_memory_on_return(engine):
    """``stream_screen.screen``: the call is enqueued on a pool stream that is still held, its input a decoy until the stream moves
    on; the lengths array is overwritten by the screen and the parameter struct by this test as soon as the call has returned."""
    from stream_screen import screen
    lens = [720, 3001, 2000]
    made = []

    def make(seed):
        g = torch.Generator().manual_seed(seed)
        return {"wav": (0.1 * torch.randn(3, 3004, generator=g)).clamp(-1, 1).cuda()}

    def call(e, x):
        check = type(e).check_reverb

        def spy(*a, **k):
            made.append(check(*a, **k))
            return made[-1]

        e.check_reverb = spy
        try:
            out = e.degrade_reverb([x["wav"][i, :n] for i, n in enumerate(lens)], [20.0, 90.0], pre_delay_ms=5)[0]
        finally:
            del e.check_reverb
        C.memmove(C.byref(made[-1]), C.byref(_params([7.0], room_scale=3.0, wet_only=True)), C.sizeof(made[-1]))
        return out

    S = torch.cuda.Stream()
    rep = screen(engine, S, make, call, 100.0, name="degrade_reverb", side="late", names=["rows"])
    print(rep.line())
    assert len(made) == 4 and all(p.G == 1 and p.wet_only == 1 for p in made), "every struct was overwritten behind its call"
    assert not rep.problems, rep.line()
    assert rep.host_arrays == 1, "the lengths are the call's one host array"
    assert rep.held, f"the stream was released before the call returned: the case shows nothing ({rep.line()})"


# ---- the host layers ---------------------------------------------------------------------------------------------------------------
def _padded():
    clean = torch.zeros(3, 5003)
    for b, x in enumerate(_clips()):
        clean[b, :LENS[b]] = torch.from_numpy(x)
    return clean


def test_nomad_reverb_returns_the_abi_rows(engine):
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    call = _Call(engine, _clips(), LEVELS, pre_delay_ms=10, hf_damping=30)
    assert call.run() == 0
    want = call.results()
    with guard.guarded(case="Nomad.reverb"):
        rows, lens = nomad.reverb(_padded(), LEVELS, lengths=LENS, pre_delay_ms=10, hf_damping=30)
    assert lens == [n for n in LENS for _ in range(3)] and rows.shape == (9, 5004) and rows.dtype == torch.float32
    assert np.array_equal(_bits(rows.cpu().numpy()), _bits(want))
    one, lens1 = nomad.reverb(_padded()[:, None, :], 50, lengths=LENS)
    assert one.shape == (3, 5004) and lens1 == LENS


def test_sweep_scores_the_normalized_reverberant_rows(engine):
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    clean, lens = torch.zeros(2, 8000), [8000, 7001]
    for b, n in enumerate(lens):
        clean[b, :n] = torch.from_numpy(F.noise(n, 60 + b))
    gen = torch.Generator().manual_seed(5)
    refs = torch.randn(5, 256, generator=gen, dtype=torch.float64)
    refs = (refs / refs.norm(dim=1, keepdim=True)).float()
    with guard.guarded(case="intensity_sweep(reverberance=)"):
        res = nomad.intensity_sweep(clean, refs, lengths=lens, reverberance=[1, 50, 100], normalize=-23)
    assert list(res) == ["REVERB"]
    res = res["REVERB"]
    rows, lens_rep = nomad.reverb(clean, [1, 50, 100], lengths=lens)
    norm_rows, norm_lens, stats = nomad.normalize(rows, target=-23.0, lengths=lens_rep)
    want = nomad.score(norm_rows, refs, lengths=norm_lens).cpu().numpy()
    assert res["scores"].shape == (6,) and np.array_equal(np.ascontiguousarray(res["scores"]).view(np.uint64),
                                                          np.ascontiguousarray(want.astype(np.float64)).view(np.uint64)), (res["scores"], want)
    assert sorted(res["table"]["Condition"].tolist()) == [1.0, 50.0, 100.0]
    assert np.array_equal(res["gain_db"], 20.0 * np.log10(stats[:, 2].cpu().numpy()))
    with pytest.raises(ValueError, match="REVERB"):
        nomad.intensity_sweep(clean, refs, lengths=lens, reverberance=[1, 50], rt60_s=[0.2])
    with pytest.raises(ValueError, match="hf_damping"):
        nomad.intensity_sweep(clean, refs, lengths=lens, reverberance=[1, 50], reverb_params={"hf_damping": 101})
