"""GPU: ``nomad_degrade_noise`` / ``nomad_degrade_clip`` through the C ABI in guarded, NaN-poisoned buffers, against the float64
restatement ``degrade_ref``; then ``Engine.degrade_*`` / ``Nomad.degrade`` / ``Nomad.intensity_sweep`` end to end.

Bounds (include/nomad_hip.h states the arithmetic):
* clip thresholds: EQUAL to ``degrade_ref``'s - the same float64 expression on exact order statistics; clipped rows: the same bits.
* noise alpha: relative 1e-11.  Two sums of n <= 4099 float64 squares taken in another order differ by at most about
  2 n 2^-53 ~ 1e-12 relatively, sqrt and the two divisions add a few 2^-53; the margin is a factor of 10.
* noise rows: within one float32 ulp of ``degrade_ref``'s row (alpha's 1e-11 can move a float64 sum across a rounding boundary).
The lengths straddle one wave, one pass of the 1024-thread workgroup, a length that is no multiple of 4 and several passes."""
import ctypes as C

import numpy as np
import pytest
import torch

import degrade_ref
import guard
from nomad_amd import _lib

pytestmark = pytest.mark.gpu

LENS = [1, 2, 255, 256, 257, 1025, 4099]
CLIP_LEVELS = [0, 2, 5, 11, 40, 62, 100]
SNR_LEVELS = [0, 1, 8, 15, 25, 40, 50]


def _pcm(n, seed):
    return (np.random.RandomState(seed).randint(-32768, 32768, size=n) / 32768.0).astype(np.float32)


def _pcm_clips():
    return [_pcm(n, 100 + n) for n in LENS]


def _special_clips():
    r = np.random.RandomState(7)
    const = np.full(257, 0.25, dtype=np.float32)
    seven = r.choice(np.linspace(-0.75, 0.75, 7).astype(np.float32), size=1025).astype(np.float32)
    zeros = _pcm(256, 3)
    zeros[::3] = -0.0
    zeros[1::3] = 0.0
    weird = _pcm(4099, 4)
    weird[17] = np.nan
    weird[4000] = np.inf
    weird[5] = -np.inf
    silent = np.zeros(255, dtype=np.float32)
    return [const, seven, zeros, weird, silent]


BATCHES = {"pcm": _pcm_clips, "special": _special_clips}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    """Equal, NaN matching NaN (thresholds and alphas: values; the payload of a computed NaN is not part of the contract)."""
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


class _Call:
    """One ABI call in guarded buffers: input rows padded with NaN, outputs and workspace filled with NaN bytes."""

    def __init__(self, engine, clips, G, stats_shape, stride=None, ws_bytes=None, x_off=0, out_off=0):
        """x_off / out_off: the rows begin that many floats (0 .. 3) behind a 256-byte boundary (``guard.Guards.empty_at``): base
        addresses aligned to 4 or 8 bytes only.  Statistics and workspace stay aligned."""
        self.engine, self.clips, self.G = engine, clips, G
        self.B = len(clips)
        self.lens = [int(c.shape[0]) for c in clips]
        self.stride = stride if stride is not None else (max(self.lens) + 3) // 4 * 4
        dev = engine.device
        self.guards = g = guard.Guards()
        host = np.full((self.B, self.stride), np.nan, dtype=np.float32)
        for b, c in enumerate(clips):
            host[b, :min(self.lens[b], self.stride)] = c[:self.stride]
        self.x = g.empty_at((self.B, self.stride), x_off, device=dev, name="x")
        self.x.copy_(torch.from_numpy(host))
        self.out = g.empty_at((self.B * G, self.stride), out_off, device=dev, name="out")
        self.out.fill_(float("nan"))
        self.stats = g.empty(stats_shape, dtype=torch.float64, device=dev, name="stats")
        self.stats.fill_(float("nan"))
        need = int(engine.lib.nomad_degrade_scratch_bytes(self.B, self.stride, G)) if ws_bytes is None else ws_bytes
        self.ws = g.empty_bytes(max(need, 256), dev, 1 << 16, "workspace")
        self.ws.fill_(0xFF)
        self.ws_bytes = need

    def args(self):
        return self.x.data_ptr(), self.B, self.stride, (C.c_int * self.B)(*self.lens)

    def tail(self):
        return self.ws.data_ptr(), self.ws_bytes, self.engine._stream()

    def results(self):
        self.guards.check()
        return self.out.cpu().numpy().reshape(self.B, self.G, self.stride), self.stats.cpu().numpy()


def _clip(engine, clips, levels, **kw):
    c = _Call(engine, clips, len(levels), (len(clips), len(levels), 2), **kw)
    rc = engine.lib.nomad_degrade_clip(engine.ctx, *c.args(), (C.c_double * len(levels))(*levels), len(levels), c.out.data_ptr(),
                                       c.stats.data_ptr(), *c.tail())
    return rc, c


def _noise(engine, clips, noise, levels, noise_off=0, **kw):
    c = _Call(engine, clips, len(levels), (len(clips), len(levels)), **kw)
    nz = c.guards.empty_at((len(noise),), noise_off, device=engine.device, name="noise")
    nz.copy_(torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float32)))
    rc = engine.lib.nomad_degrade_noise(engine.ctx, *c.args(), nz.data_ptr(), nz.numel(), (C.c_double * len(levels))(*levels), len(levels),
                                        c.out.data_ptr(), c.stats.data_ptr(), *c.tail())
    torch.cuda.synchronize()
    return rc, c


_REF = {}


def _clip_ref(batch, levels):
    """``degrade_ref.clip`` of every clip of a batch, computed once per (batch, levels)."""
    key = ("clip", batch, tuple(levels))
    if key not in _REF:
        _REF[key] = [degrade_ref.clip(x, levels) for x in BATCHES[batch]()]
    return _REF[key]


# ---- clipping --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", sorted(BATCHES))
@pytest.mark.parametrize("levels", [CLIP_LEVELS, [11]], ids=["G7", "G1"])
def test_clip_thresholds_and_rows_are_the_reference_bits(engine, batch, levels):
    clips = BATCHES[batch]()
    rc, call = _clip(engine, clips, levels)
    assert rc == 0, engine.lib.nomad_last_error()
    out, thr = call.results()
    rc2, again = _clip(engine, clips, levels)
    out2, thr2 = again.results()
    assert rc2 == 0 and np.array_equal(_bits(out), _bits(out2)) and np.array_equal(_bits(thr), _bits(thr2)), "run to run"
    for b, (x, (rows, rthr)) in enumerate(zip(clips, _clip_ref(batch, levels))):
        n = x.shape[0]
        assert _same(thr[b], rthr), (batch, b, n, thr[b], rthr)
        assert np.array_equal(_bits(out[b, :, :n]), _bits(rows)), (batch, b, n)
        assert not out[b, :, n:].any() and not np.isnan(out[b, :, n:]).any(), f"clip {b}: rows are zero behind the length"
        if np.isfinite(x).all():
            assert np.isfinite(thr[b]).all() and np.isfinite(out[b, :, :n]).all(), f"clip {b}: the poison leaked"
        for g, cf in enumerate(levels):
            if cf == 0:
                assert np.array_equal(_bits(out[b, g, :n]), _bits(x)), f"clip {b}: level 0 returns the input"
            if cf == 100 and np.isfinite(x).all():
                assert thr[b, g, 0] == thr[b, g, 1] and (out[b, g, :n] == np.float32(thr[b, g, 0])).all(), f"clip {b}: level 100 is the median"
        # a clip's rows are those of its own call
        rc1, one = _clip(engine, [x], levels)
        o1, t1 = one.results()
        assert rc1 == 0 and np.array_equal(_bits(o1[0, :, :n]), _bits(out[b, :, :n])) and np.array_equal(_bits(t1[0]), _bits(thr[b])), (batch, b)


def test_clip_orders_nan_last_like_numpy(engine):
    """The clip with a NaN, +inf and -inf: numpy sorts NaN behind +inf, so the thresholds of level 0 are NaN (nothing is
    clipped), inner percentiles come from the finite samples, and a NaN sample passes through with its bits."""
    x = _special_clips()[3]
    rc, call = _clip(engine, [x], [0, 2, 40])
    assert rc == 0
    out, thr = call.results()
    srt = np.sort(x)
    assert np.isnan(srt[-1]) and np.isinf(srt[-2]) and srt[0] == -np.inf
    assert np.isnan(thr[0, 0]).all()       # level 0: max = NaN; min = -inf + (finite - -inf) * 0 = NaN as well
    assert np.isfinite(thr[0, 1]).all() and np.isfinite(thr[0, 2]).all()
    assert _bits(out[0, :, 17]).tolist() == [int(_bits(x[17:18])[0])] * 3
    assert out[0, 1, 4000] == np.float32(thr[0, 1, 1]) and out[0, 1, 5] == np.float32(thr[0, 1, 0])


# ---- noise -----------------------------------------------------------------------------------------------------------------------
def _check_noise(out, alpha, clips, noise, levels, case):
    for b, x in enumerate(clips):
        n = x.shape[0]
        rows, ralpha, _ = degrade_ref.noise(x, noise, levels)
        fin = np.isfinite(ralpha)
        assert _same(alpha[b][~fin], ralpha[~fin]), (case, b, alpha[b], ralpha)
        assert (np.abs(alpha[b][fin] - ralpha[fin]) <= 1e-11 * np.abs(ralpha[fin])).all(), (case, b, alpha[b], ralpha)
        got = out[b, :, :n]
        rfin = np.isfinite(rows)
        assert _same(got[~rfin], rows[~rfin]), (case, b, "non-finite samples")
        with np.errstate(invalid="ignore"):
            err = np.abs(got[rfin].astype(np.float64) - rows[rfin].astype(np.float64))
        assert (err <= np.spacing(np.abs(rows[rfin])).astype(np.float64)).all(), (case, b, float(err.max()))
        assert not out[b, :, n:].any() and not np.isnan(out[b, :, n:]).any(), f"{case} clip {b}: rows are zero behind the length"


@pytest.mark.parametrize("noise_len", [7, 4099, 5000])
def test_noise_alpha_and_rows(engine, noise_len):
    clips = _pcm_clips()
    noise = _pcm(noise_len, 900 + noise_len) * np.float32(0.3)
    rc, call = _noise(engine, clips, noise, SNR_LEVELS)
    assert rc == 0, engine.lib.nomad_last_error()
    out, alpha = call.results()
    assert np.isfinite(alpha).all() and np.isfinite(out[:, :, :1]).all()
    _check_noise(out, alpha, clips, noise, SNR_LEVELS, f"noise_len={noise_len}")
    rc2, again = _noise(engine, clips, noise, SNR_LEVELS)
    out2, alpha2 = again.results()
    assert rc2 == 0 and np.array_equal(_bits(out), _bits(out2)) and np.array_equal(_bits(alpha), _bits(alpha2)), "run to run"
    for b, x in enumerate(clips):
        n = x.shape[0]
        rc1, one = _noise(engine, [x], noise, SNR_LEVELS)
        o1, a1 = one.results()
        assert rc1 == 0 and np.array_equal(_bits(o1[0, :, :n]), _bits(out[b, :, :n])) and np.array_equal(_bits(a1[0]), _bits(alpha[b])), b


def test_noise_special_inputs_and_silence_give_what_ieee_gives(engine):
    clips = _special_clips()
    noise = _pcm(300, 11) * np.float32(0.1)
    rc, call = _noise(engine, clips, noise, [0, 15])
    assert rc == 0
    out, alpha = call.results()
    _check_noise(out, alpha, clips, noise, [0, 15], "special clips")
    assert (alpha[4] == 0).all() and not out[4].any(), "a silent clip: alpha = 0, the rows stay silent"
    rc, call = _noise(engine, clips, np.zeros(64, dtype=np.float32), [0, 15])
    assert rc == 0
    out, alpha = call.results()
    _check_noise(out, alpha, clips, np.zeros(64, dtype=np.float32), [0, 15], "silent noise")
    assert np.isinf(alpha[0]).all() and np.isnan(out[0, :, :257]).all(), "silent noise: alpha = inf, inf * 0 = NaN"
    assert np.isnan(alpha[4]).all(), "silent clip and silent noise: 0 / 0"
    _, one = _noise(engine, [clips[1]], noise, [8], stride=1028)
    o1, _ = one.results()
    _, g1 = _noise(engine, [clips[1]], noise, SNR_LEVELS, stride=1028)
    o7, _ = g1.results()
    assert np.array_equal(_bits(o1[0, 0]), _bits(o7[0, 2])), "G = 1 gives the row of the sweep"


# ---- rows at addresses that are aligned to 4 or 8 bytes only ------------------------------------------------------------------------
# (x offset, out offset, noise offset) in floats: together, separately, and every residue of 16 bytes on each pointer
OFFSETS = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 0, 0), (0, 3, 0), (0, 0, 2), (2, 1, 3)]


@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: "x%d-out%d-aux%d" % o)
def test_rows_at_unaligned_addresses_have_the_bits_of_the_aligned_call(engine, offs):
    """Both calls read and write sample by sample, so rows whose base is aligned to a float and nothing wider give the aligned
    call's bits - thresholds, alphas and rows -, zeros behind each length, and leave the guards (which begin at the very next
    float on either side) intact.  The header's calling contract promises it."""
    xo, oo, no = offs
    clips = _pcm_clips()
    noise = _pcm(4099, 901) * np.float32(0.3)
    key = ("aligned", "pcm")
    if key not in _REF:
        rc, call = _clip(engine, clips, CLIP_LEVELS)
        assert rc == 0
        rn, calln = _noise(engine, clips, noise, SNR_LEVELS)
        assert rn == 0
        _REF[key] = (call.results(), calln.results())
    (out_c, thr), (out_n, alpha) = _REF[key]
    rc, call = _clip(engine, clips, CLIP_LEVELS, x_off=xo, out_off=oo)
    assert rc == 0, engine.lib.nomad_last_error()
    assert call.x.data_ptr() % 16 == 4 * xo and call.out.data_ptr() % 16 == 4 * oo
    got, gthr = call.results()
    assert np.array_equal(_bits(gthr), _bits(thr)), "clip thresholds"
    assert np.array_equal(_bits(got), _bits(out_c)), "clipped rows (zeros behind the lengths included)"
    for b, n in enumerate(LENS):
        assert not got[b, :, n:].any() and not np.isnan(got[b, :, n:]).any(), f"clip {b}: rows are zero behind the length"
    rc, call = _noise(engine, clips, noise, SNR_LEVELS, noise_off=no, x_off=xo, out_off=oo)
    assert rc == 0, engine.lib.nomad_last_error()
    got, galpha = call.results()
    assert np.array_equal(_bits(galpha), _bits(alpha)), "noise alphas"
    assert np.array_equal(_bits(got), _bits(out_n)), "noisy rows (zeros behind the lengths included)"
    for b, n in enumerate(LENS):
        assert not got[b, :, n:].any() and not np.isnan(got[b, :, n:]).any(), f"clip {b}: rows are zero behind the length"


# ---- argument errors -------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_return_a_status_and_a_message_and_touch_nothing(engine):
    lib, x = engine.lib, _pcm(1025, 1)
    noise = torch.from_numpy(_pcm(64, 2)).to(engine.device)

    def refused(rc, call, status, what):
        torch.cuda.synchronize()
        assert rc == status, (what, rc)
        assert lib.nomad_last_error(), what
        call.guards.check(what)
        assert bool(torch.isnan(call.out).all()) and bool(torch.isnan(call.stats).all()), f"{what}: the outputs were written"

    def clip(levels, G=None, B=None, stride=None, lens=None, ws_bytes=None):
        c = _Call(engine, [x, x[:300]], len(levels), (2, len(levels), 2))
        G = len(levels) if G is None else G
        rc = lib.nomad_degrade_clip(engine.ctx, c.x.data_ptr(), 2 if B is None else B, c.stride if stride is None else stride,
                                    (C.c_int * 2)(*(lens or c.lens)), (C.c_double * len(levels))(*levels), G, c.out.data_ptr(),
                                    c.stats.data_ptr(), c.ws.data_ptr(), c.ws_bytes if ws_bytes is None else ws_bytes, engine._stream())
        return rc, c

    def mix(levels, G=None, noise_len=64, stride=None, lens=None, ws_bytes=None):
        c = _Call(engine, [x, x[:300]], len(levels), (2, len(levels)))
        G = len(levels) if G is None else G
        rc = lib.nomad_degrade_noise(engine.ctx, c.x.data_ptr(), 2, c.stride if stride is None else stride, (C.c_int * 2)(*(lens or c.lens)),
                                     noise.data_ptr(), noise_len, (C.c_double * len(levels))(*levels), G, c.out.data_ptr(),
                                     c.stats.data_ptr(), c.ws.data_ptr(), c.ws_bytes if ws_bytes is None else ws_bytes, engine._stream())
        return rc, c

    many = [float(i) for i in range(65)]
    for call, what in ((clip, "clip"), (mix, "noise")):
        refused(*call([5.0], G=0), _lib.NOMAD_ERR_INVALID, f"{what}: G = 0")
        refused(*call(many[:64], G=65), _lib.NOMAD_ERR_INVALID, f"{what}: G = 65")
        refused(*call([5.0], stride=1026), _lib.NOMAD_ERR_INVALID, f"{what}: stride no multiple of 4")
        refused(*call([5.0], stride=1024), _lib.NOMAD_ERR_INVALID, f"{what}: stride shorter than a length")
        refused(*call([5.0], lens=[1025, 0]), _lib.NOMAD_ERR_INVALID, f"{what}: a length of 0")
        refused(*call([5.0, float("nan")]), _lib.NOMAD_ERR_INVALID, f"{what}: a NaN level")
        refused(*call([float("inf")]), _lib.NOMAD_ERR_INVALID, f"{what}: an infinite level")
        refused(*call([5.0], ws_bytes=1024), _lib.NOMAD_ERR_WORKSPACE, f"{what}: a short workspace")
    refused(*clip([5.0], B=0), _lib.NOMAD_ERR_INVALID, "clip: B = 0")
    refused(*clip([-0.5]), _lib.NOMAD_ERR_INVALID, "clip: a negative clip factor")
    refused(*clip([100.5]), _lib.NOMAD_ERR_INVALID, "clip: a clip factor above 100")
    refused(*mix([5.0], noise_len=0), _lib.NOMAD_ERR_INVALID, "noise: noise_len = 0")
    assert lib.nomad_degrade_scratch_bytes(0, 1028, 1) == 0 and lib.nomad_degrade_scratch_bytes(2, 1026, 1) == 0
    assert lib.nomad_degrade_scratch_bytes(2, 1028, 65) == 0 and lib.nomad_degrade_scratch_bytes(2, 1028, 64) > 2 * 2 * 1028 * 4
    # a NULL optional output is accepted
    c = _Call(engine, [x], 1, (1, 1, 2))
    assert lib.nomad_degrade_clip(engine.ctx, *c.args(), (C.c_double * 1)(5.0), 1, c.out.data_ptr(), None, *c.tail()) == 0
    out, _ = c.results()
    assert np.array_equal(_bits(out[0, :, :1025]), _bits(degrade_ref.clip(x, [5.0])[0]))


# ---- the host layers -------------------------------------------------------------------------------------------------------------
def test_engine_calls_in_guarded_buffers_feed_the_ragged_forward_without_a_copy(engine):
    clips = [torch.from_numpy(_pcm(n, 50 + n)) for n in (6400, 7001, 9600)]
    noise = torch.from_numpy(_pcm(5000, 8) * np.float32(0.2))
    with guard.guarded(case="Engine.degrade_*"):
        out_n, lens_n, alpha = engine.degrade_noise(clips, noise, [0.0, 15.0, 40.0])
        out_c, lens_c, thr = engine.degrade_clip(clips, [5.0, 40.0])
        emb = engine.embed_ragged(None, packed=(out_c, lens_c))
    assert out_n.shape == (9, 9600) and lens_n == [6400] * 3 + [7001] * 3 + [9600] * 3 and alpha.shape == (3, 3)
    assert out_c.shape == (6, 9600) and lens_c == [6400] * 2 + [7001] * 2 + [9600] * 2 and thr.shape == (3, 2, 2)
    for b, x in enumerate(clips):
        rows, rthr = degrade_ref.clip(x.numpy(), [5.0, 40.0])
        n = x.numel()
        assert _same(thr[b].cpu().numpy(), rthr)
        assert np.array_equal(_bits(out_c[2 * b:2 * b + 2, :n].cpu().numpy()), _bits(rows))
    one = engine.embed_ragged([out_c[3, :7001]])
    assert torch.equal(one[0], emb[3]), "a degraded row embeds like the clip it is"
    padded = torch.zeros(3, 9601, device=engine.device)       # a padded tensor whose row stride is no multiple of 4
    for b, x in enumerate(clips):
        padded[b, :x.numel()] = x.to(engine.device)
    out_p, lens_p, thr_p = engine.degrade_clip(padded, [5.0, 40.0], lengths=[6400, 7001, 9600])
    assert lens_p == lens_c and torch.equal(thr_p, thr) and torch.equal(out_p[:, :9600], out_c)


@pytest.mark.parametrize("k", [None, 2])
def test_intensity_sweep_scores_are_score_on_the_degraded_rows(engine, k):
    from nomad_amd.nomad import Nomad
    from nomad_amd.train import intensity_stats
    nomad = Nomad.from_engine(engine)
    gen = torch.Generator().manual_seed(5)
    lens = [6400, 8000, 9600]
    clean = torch.zeros(3, 9600)
    for b, n in enumerate(lens):
        clean[b, :n] = torch.from_numpy(_pcm(n, 70 + b))
    noise = torch.from_numpy(_pcm(3000, 9) * np.float32(0.2))
    refs = torch.randn(5, 256, generator=gen, dtype=torch.float64)
    refs = (refs / refs.norm(dim=1, keepdim=True)).float()
    snr, cf = [0, 15, 40], [5, 40]
    with guard.guarded(case="intensity_sweep"):
        res = nomad.intensity_sweep(clean, refs, noise=noise, snr_db=snr, clip_factor=cf, lengths=lens, k=k)
    assert sorted(res) == ["CLIP", "NOISE"]
    for name, kind, levels in (("NOISE", "noise", snr), ("CLIP", "clip", cf)):
        rows, lens_rep = nomad.degrade(clean, kind, levels, noise=noise if kind == "noise" else None, lengths=lens)
        assert rows.shape == (3 * len(levels), 9600) and lens_rep == [n for n in lens for _ in levels]
        want = nomad.score(rows, refs, lengths=lens_rep, k=k).cpu().numpy()
        got = res[name]["scores"]
        assert got.dtype == np.float64 and np.array_equal(_bits(got), _bits(want)), (name, got, want)
        again = intensity_stats(res[name]["embeddings"], pd_conditions(res[name]["embeddings"], levels), res[name]["embeddings"].iloc[:1, 1:],
                                lambda t, r: want, name)
        assert list(res[name]["table"].columns) == ["Condition", "Distance"]
        assert res[name]["table"].reset_index(drop=True).equals(again["table"].reset_index(drop=True))
        assert res[name]["SRCC"] == again["SRCC"] or (np.isnan(res[name]["SRCC"]) and np.isnan(again["SRCC"]))
        by_level = [want[g::len(levels)].mean() for g in range(len(levels))]
        table = res[name]["table"].sort_values(by="Condition")
        assert table["Condition"].tolist() == sorted(float(v) for v in levels)
        assert np.allclose(table["Distance"].to_numpy(), np.array(by_level)[np.argsort(levels)], rtol=1e-12, atol=0)
    if k is None:
        assert not np.array_equal(res["NOISE"]["scores"], nomad.intensity_sweep(clean, refs, noise=noise, snr_db=snr, lengths=lens,
                                                                                 k=2)["NOISE"]["scores"]), "k takes the k-NN path"


def pd_conditions(df_emb, levels):
    """The (filepath_deg, Condition) table of a sweep: clip b at level g in row b G + g."""
    import pandas as pd
    names = list(df_emb["filepath_deg"])
    return pd.DataFrame({"filepath_deg": names, "Condition": [float(v) for v in levels] * (len(names) // len(levels))})
