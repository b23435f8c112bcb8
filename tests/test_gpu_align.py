"""GPU: ``nomad_align_delay`` and ``nomad_align_shift`` through the C ABI in guarded buffers - clean and degraded rows padded with
NaN behind their lengths, outputs poisoned, workspace filled with 0xFF - against tests/align_ref.py in float64; then the three
launches held to their caller's stream.

Shapes.  The kernel as built (nomad_amd/csrc/align.hip.h) adds one fp32 chain per SLICE = 4096 time steps, gives a workgroup TILE =
4096 lags (16 accumulator tiles of 256) and a part of PART = 8 slices.  Clean lengths 1, 2, 15, 16, 17, 255, 257, SLICE - 1, SLICE,
SLICE + 1, 2 SLICE + 3, 9001; per clean length n the degraded lengths max(n - 5, 1), n, n + 37, n + D; max_delay 0, 1, 15, 16, 127, 128,
300, TILE / 2 - 1, TILE / 2 (2 D + 1 crosses the workgroup's 4096 lags) and 9100, larger than every clip: 2 D + 1 crosses many 256-lag
tiles there and most lags have no overlap.  Every clip meets its four rows at every max_delay in one call (12 x 4 rows); one more
call has G = 64; the own-bits batch spans two parts (PART SLICE + 5 samples).

Bounds.
* integer-valued inputs (x, y in [-8, 8]: every slice's partial sums are <= 64 x 4096 < 2^24) and pure delays of an integer signal:
  the BITS of the float64 sums - no rounding occurs in any order.
* real values: ``|c - c64| <= (SLICE + 8) 2^-24 (sum |x| |y|)[d] + 1e-37 n`` (``align_ref.bound``): derived, not measured.
* recovery: the test first asserts that the float64 peak exceeds the runner-up by more than 4 x that bound, then that the delay is
  exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import align_ref
import guard
from nomad_amd import _lib
from stream_screen import screen

pytestmark = pytest.mark.gpu

SLICE, TILE, PART = 4096, 4096, 8
assert SLICE == align_ref.SLICE
CLEAN_LENS = [1, 2, 15, 16, 17, 255, 257, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 3, 9001]
MAX_DELAYS = [0, 1, 15, 16, 127, 128, 300, TILE // 2 - 1, TILE // 2, 9100]


def _deg_lens(n, D):
    return [max(n - 5, 1), n, n + 37, n + D]


def _pcm(n, seed):
    return (np.random.RandomState(seed).randint(-32768, 32768, size=n) / 32768.0).astype(np.float32)


def _ints(n, seed):
    return np.random.RandomState(seed).randint(-8, 9, size=n).astype(np.float32)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _rows(arrays, stride):
    host = np.full((len(arrays), stride), np.nan, dtype=np.float32)
    for i, a in enumerate(arrays):
        host[i, :min(a.shape[0], stride)] = a[:stride]
    return host


DELAY_POISON = -123456789


class _Delay:
    """One ``nomad_align_delay`` call in guarded buffers; the arguments can be overridden one by one (the refusals)."""

    def __init__(self, engine, clips, rows, D, stride=None, deg_stride=None, x_off=0, y_off=0, want_corr=True):
        """x_off / y_off: the rows begin that many floats (0 .. 3) behind a 256-byte boundary; the strides are the longest lengths
        unless given (no multiple of 4 is asked for)."""
        self.engine, self.B, self.R, self.D = engine, len(clips), len(rows), D
        assert self.R % self.B == 0
        self.G = self.R // self.B
        self.lens, self.dlens = [int(c.shape[0]) for c in clips], [int(r.shape[0]) for r in rows]
        self.stride, self.deg_stride = stride or max(self.lens), deg_stride or max(self.dlens)
        dev = engine.device
        self.guards = g = guard.Guards()
        self.x = g.empty_at((self.B, self.stride), x_off, device=dev, name="clean")
        self.x.copy_(torch.from_numpy(_rows(clips, self.stride)))
        self.y = g.empty_at((self.R, self.deg_stride), y_off, device=dev, name="degraded")
        self.y.copy_(torch.from_numpy(_rows(rows, self.deg_stride)))
        self.delay = g.empty((self.R,), dtype=torch.int32, device=dev, name="delay")
        self.delay.fill_(DELAY_POISON)
        self.peak = g.empty((self.R,), dtype=torch.float64, device=dev, name="peak")
        self.peak.fill_(float("nan"))
        self.corr = None
        if want_corr:
            self.corr = g.empty((self.R, 2 * D + 1), dtype=torch.float64, device=dev, name="corr")
            self.corr.fill_(float("nan"))
        self.ws_bytes = int(engine.lib.nomad_align_scratch_bytes(self.B, self.G, self.stride, self.deg_stride, D))
        assert self.ws_bytes > 0, engine.lib.nomad_last_error()
        self.ws = g.empty_bytes(self.ws_bytes, dev, 1 << 16, "workspace")
        self.ws.fill_(0xFF)

    def run(self, **kw):
        a = dict(ctx=self.engine.ctx, x=self.x.data_ptr(), B=self.B, stride=self.stride, lens=self.lens, y=self.y.data_ptr(), G=self.G,
                 deg_stride=self.deg_stride, dlens=self.dlens, D=self.D, delay=self.delay.data_ptr(), peak=self.peak.data_ptr(),
                 corr=None if self.corr is None else self.corr.data_ptr(), ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(kw)
        lens = (C.c_int * len(a["lens"]))(*a["lens"]) if a["lens"] is not None else None
        dlens = (C.c_int * len(a["dlens"]))(*a["dlens"]) if a["dlens"] is not None else None
        rc = self.engine.lib.nomad_align_delay(a["ctx"], a["x"], a["B"], a["stride"], lens, a["y"], a["G"], a["deg_stride"], dlens, a["D"],
                                               a["delay"], a["peak"], a["corr"], a["ws"], a["ws_bytes"], self.engine._stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return (bool((self.delay == DELAY_POISON).all()) and bool(torch.isnan(self.peak).all()) and bool((self.ws == 0xFF).all())
                and (self.corr is None or bool(torch.isnan(self.corr).all())))

    def results(self):
        """(corr (R, 2 D + 1) or None, delay (R,), peak (R,)) after the guards have been checked."""
        self.guards.check()
        return None if self.corr is None else self.corr.cpu().numpy(), self.delay.cpu().numpy(), self.peak.cpu().numpy()


def _delay(engine, clips, rows, D, **kw):
    call = _Delay(engine, clips, rows, D, **kw)
    rc = call.run()
    assert rc == 0, engine.lib.nomad_last_error()
    return call.results()


class _Shift:
    """One ``nomad_align_shift`` call in guarded buffers."""

    def __init__(self, engine, rows, delays, out_lens, deg_stride=None, out_stride=None, y_off=0, out_off=0):
        self.engine, self.R = engine, len(rows)
        self.dlens, self.olens = [int(r.shape[0]) for r in rows], [int(n) for n in out_lens]
        self.deg_stride, self.out_stride = deg_stride or max(self.dlens), out_stride or max(self.olens) + 3
        dev = engine.device
        self.guards = g = guard.Guards()
        self.y = g.empty_at((self.R, self.deg_stride), y_off, device=dev, name="degraded")
        self.y.copy_(torch.from_numpy(_rows(rows, self.deg_stride)))
        self.delay = g.empty((self.R,), dtype=torch.int32, device=dev, name="delay")
        self.delay.copy_(torch.tensor(list(delays), dtype=torch.int32))
        self.out = g.empty_at((self.R, self.out_stride), out_off, device=dev, name="out")
        self.out.fill_(float("nan"))
        self.ws_bytes = 2 * ((4 * self.R + 255) // 256 * 256)
        self.ws = g.empty_bytes(self.ws_bytes, dev, 1 << 16, "workspace")
        self.ws.fill_(0xFF)

    def run(self, **kw):
        a = dict(ctx=self.engine.ctx, y=self.y.data_ptr(), R=self.R, deg_stride=self.deg_stride, dlens=self.dlens, delay=self.delay.data_ptr(),
                 olens=self.olens, out=self.out.data_ptr(), out_stride=self.out_stride, ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(kw)
        dlens = (C.c_int * len(a["dlens"]))(*a["dlens"]) if a["dlens"] is not None else None
        olens = (C.c_int * len(a["olens"]))(*a["olens"]) if a["olens"] is not None else None
        rc = self.engine.lib.nomad_align_shift(a["ctx"], a["y"], a["R"], a["deg_stride"], dlens, a["delay"], olens, a["out"], a["out_stride"],
                                               a["ws"], a["ws_bytes"], self.engine._stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return bool(torch.isnan(self.out).all()) and bool((self.ws == 0xFF).all())

    def results(self):
        self.guards.check()
        return self.out.cpu().numpy()


def _shift(engine, rows, delays, out_lens, **kw):
    call = _Shift(engine, rows, delays, out_lens, **kw)
    rc = call.run()
    assert rc == 0, engine.lib.nomad_last_error()
    return call.results()


_CACHE = {}


def _batch(engine, kind, D):
    """The 12 x 4 call at max_delay D on integer-valued ('int') or real ('real') inputs -> (clips, rows, corr, delay, peak), made
    once.  The bases are 1 and 3 floats off a 256-byte boundary, the strides the longest lengths (9001 and 9001 + D)."""
    if (kind, D) not in _CACHE:
        make = _ints if kind == "int" else _pcm
        clips = [make(n, 10 + n) for n in CLEAN_LENS]
        rows = [make(m, 1000 * g + n + D) for n in CLEAN_LENS for g, m in enumerate(_deg_lens(n, D))]
        _CACHE[(kind, D)] = (clips, rows) + _delay(engine, clips, rows, D, x_off=1, y_off=3)
    return _CACHE[(kind, D)]


@pytest.mark.parametrize("D", MAX_DELAYS)
def test_integer_inputs_give_the_bits_of_float64(engine, D):
    clips, rows, corr, _, _ = _batch(engine, "int", D)
    for r, y in enumerate(rows):
        x = clips[r // 4]
        n, m = x.shape[0], y.shape[0]
        want = align_ref.corr(x, y, D)
        assert align_ref.magnitude(x, y, D).max() <= 64 * n
        assert np.array_equal(corr[r], want) and not np.signbit(corr[r][want == 0]).any(), (n, m, D)
        d = np.arange(-D, D + 1)
        none = (d >= m) | (d <= -n)
        assert np.array_equal(_bits64(corr[r][none]), _bits64(np.zeros(int(none.sum())))), "a lag with no overlap gives exactly +0"


@pytest.mark.parametrize("D", MAX_DELAYS)
def test_real_values_within_the_running_error_bound(engine, D):
    clips, rows, corr, _, _ = _batch(engine, "real", D)
    worst = 0.0
    for r, y in enumerate(rows):
        x = clips[r // 4]
        ref, bound = align_ref.corr(x, y, D), align_ref.bound(x, y, D)
        err = np.abs(corr[r] - ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (x.shape[0], y.shape[0], D, float((err / bound).max()))
    print(f"max_delay {D}: largest error / bound over the 48 rows: {worst:.4f}")


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("D", MAX_DELAYS)
def test_selection_is_the_rule_on_the_gpus_own_table(engine, kind, D):
    clips, rows, corr, delay, peak = _batch(engine, kind, D)
    for r in range(len(rows)):
        d, p = align_ref.select(corr[r], D)
        assert int(delay[r]) == d and np.array_equal(_bits64(peak[r]), _bits64(p)), (r, D, int(delay[r]), d)
        assert np.array_equal(_bits64(peak[r]), _bits64(corr[r][d + D])), "the peak is that entry's bits"
    none, delay2, peak2 = _delay(engine, clips, rows, D, x_off=1, y_off=3, want_corr=False)
    assert none is None and np.array_equal(delay2, delay) and np.array_equal(_bits64(peak2), _bits64(peak)), "without corr_out_dev"


def test_ties_and_silence(engine):
    """Hand-made rows whose tables tie: a silent row (every lag 0) gets 0; a clip of one impulse against a row of two equal impulses
    at -3 and +3 gets +3, at -2 and +5 gets -2; a negative-only table takes its largest value (no polarity search)."""
    x = np.zeros(64, dtype=np.float32)
    x[20] = 2.0
    rows = [np.zeros(70, dtype=np.float32) for _ in range(4)]
    rows[1][[17, 23]] = 3.0
    rows[2][[18, 25]] = 3.0
    rows[3][:] = -1.0
    rows[3][20 + 4] = -0.25
    corr, delay, peak = _delay(engine, [x], rows, 8)
    assert delay.tolist() == [0, 3, -2, 4] and peak.tolist() == [0.0, 6.0, 6.0, -0.5], (delay, peak)
    for r in range(4):
        assert np.array_equal(corr[r], align_ref.corr(x, rows[r], 8))


def test_sixty_four_rows_per_clip(engine):
    D = 300
    clips = [_ints(257, 1), _ints(SLICE + 3, 2)]
    rows = [_ints(max(n + (g * 37) % 700 - 300, 1), 300 + 64 * b + g) for b, n in enumerate((257, SLICE + 3)) for g in range(64)]
    corr, delay, peak = _delay(engine, clips, rows, D, x_off=2, y_off=1)
    for r, y in enumerate(rows):
        assert np.array_equal(corr[r], align_ref.corr(clips[r // 64], y, D)), (r, y.shape[0])
        assert (int(delay[r]), float(peak[r])) == align_ref.select(corr[r], D)


def test_pure_delays_of_an_integer_signal(engine):
    D = 128
    x = _ints(2 * SLICE + 3, 7)
    shifts = [-D, -17, -1, 0, 1, 16, D]
    rows = [align_ref.shift(x, -d, x.shape[0] + 37) for d in shifts]      # y[i + d] = x[i]
    corr, delay, peak = _delay(engine, [x], rows, D)
    for r, d in enumerate(shifts):
        assert np.array_equal(corr[r], align_ref.corr(x, rows[r], D))
        energy = float((x[max(0, -d):min(x.shape[0], x.shape[0] + 37 - d)].astype(np.float64) ** 2).sum())      # what of x the row holds
        assert int(delay[r]) == d and peak[r] == energy, (d, int(delay[r]))


def _envelope(n):
    return (0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * np.arange(n) / 16000.0)).astype(np.float32)


@pytest.mark.parametrize("D", [16, 128, 300])
@pytest.mark.parametrize("n", [255, 257, 4097, 9001])
@pytest.mark.parametrize("kind", ["noise", "envelope"])
def test_known_delays_are_recovered_exactly(engine, kind, n, D):
    x = _pcm(n, 5 * n + D)
    if kind == "envelope":
        x = (x * _envelope(n)).astype(np.float32)
    # (-17 at max_delay 16 lies outside the lags that are searched: no delay_out can equal it, so it is in no case)
    shifts = sorted({d for d in (-D, -17, -1, 0, 1, 16, D) if abs(d) <= n // 2 and abs(d) <= D})
    rows = []
    for k, d in enumerate(shifts):
        y = align_ref.shift(x, -d, n + 37)                                  # the clip late by d samples, 37 samples longer
        white = np.random.RandomState(7 * n + D + k).standard_normal(n + 37)
        rms = np.sqrt(np.mean(x.astype(np.float64) ** 2))
        y = y + (rms / 10 ** (10 / 20.0) / np.sqrt(np.mean(white ** 2)) * white).astype(np.float32)      # white noise at 10 dB SNR
        rows.append(y.astype(np.float32))
    for d, y in zip(shifts, rows):
        c, bound = align_ref.corr(x, y, D), align_ref.bound(x, y, D)
        runner_up = np.delete(c, d + D).max() if D else -np.inf
        print(f"{kind} n={n} D={D} d={d}: margin / bound = {(c[d + D] - runner_up) / bound.max():.1f}")
        assert c[d + D] - runner_up > 4 * bound.max(), "the float64 peak stands clear of the runner-up by more than 4 x the bound"
    _, delay, _ = _delay(engine, [x], rows, D)
    assert delay.tolist() == shifts


def test_shift_moves_the_bits_and_zero_fills(engine):
    rows = [_pcm(m, 80 + m) for m in (1, 16, 255, 300, 4133, 9001, 9038, 40)]
    rows[2][3] = -0.0
    out_lens = [5, 16, 257, 300, 4096, 9001, 9001, 1000]
    D = 300
    for delays in ([0] * 8, [1, -1, 17, -17, D, -D, 37, -3], [D, -D, -256, 256, -4200, 4133, 9038, -1000], [-1, 16, 255, -300, 4132, -9000, 9037, 40]):
        out = _shift(engine, rows, delays, out_lens, y_off=3, out_off=1)
        assert out.shape == (8, 9004)
        for r, y in enumerate(rows):
            want = align_ref.shift(y, delays[r], out_lens[r], stride=9004)
            assert np.array_equal(_bits32(out[r]), _bits32(want)), (r, delays[r])
    # entirely out of range: all zeros
    out = _shift(engine, rows[:2], [1, -16], [16, 16])
    assert not out.any() and not np.signbit(out).any()


OWN_LENS = [1, 17, 255, 257, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 3, 9001, 400, PART * SLICE - 240, PART * SLICE + 5]


def test_every_row_has_the_bits_of_its_own_call(engine):
    """12 x 4 rows at max_delay 300: a batch at the longest lengths as strides with bases 1 and 3 floats off, the same batch at wider
    strides with bases 2 and 0 floats off, and every row's own B = 1, G = 1 call.  The two longest clips span two parts."""
    D = 300
    clips = [_pcm(n, 20 + n) for n in OWN_LENS]
    rows = [_pcm(m, 2000 * g + n) for n in OWN_LENS for g, m in enumerate(_deg_lens(n, D))]
    out_lens = [n for n in OWN_LENS for _ in range(4)]
    corr, delay, peak = _delay(engine, clips, rows, D, x_off=1, y_off=3)
    moved = _shift(engine, rows, delay.tolist(), out_lens, y_off=3, out_off=1)
    corr2, delay2, peak2 = _delay(engine, clips, rows, D, stride=max(OWN_LENS) + 11, deg_stride=max(OWN_LENS) + D + 6, x_off=2, y_off=0)
    assert np.array_equal(_bits64(corr2), _bits64(corr)) and np.array_equal(delay2, delay) and np.array_equal(_bits64(peak2), _bits64(peak))
    moved2 = _shift(engine, rows, delay.tolist(), out_lens, deg_stride=max(OWN_LENS) + D + 6, out_stride=moved.shape[1], y_off=2, out_off=3)
    assert np.array_equal(_bits32(moved2), _bits32(moved))
    for r, y in enumerate(rows):
        x = clips[r // 4]
        c1, d1, p1 = _delay(engine, [x], [y], D)
        assert np.array_equal(_bits64(c1[0]), _bits64(corr[r])), (x.shape[0], y.shape[0])
        assert int(d1[0]) == int(delay[r]) and np.array_equal(_bits64(p1), _bits64(peak[r:r + 1]))
        m1 = _shift(engine, [y], [int(d1[0])], [x.shape[0]])
        assert np.array_equal(_bits32(m1[0, :x.shape[0]]), _bits32(moved[r, :x.shape[0]])) and not moved[r, x.shape[0]:].any()
        ref, bound = align_ref.corr(x, y, D), align_ref.bound(x, y, D)
        assert (np.abs(corr[r] - ref) <= bound).all(), (x.shape[0], y.shape[0])


def test_non_finite_values_stay_in_their_rows(engine):
    D = 128
    clips = [_pcm(n, 1 + n) for n in (257, SLICE + 1, 9001)]
    rows = [_pcm(n + 37, 50 + 2 * n + g) for n in (257, SLICE + 1, 9001) for g in range(2)]
    clean = _delay(engine, clips, rows, D)
    assert np.isfinite(clean[0]).all() and np.isfinite(clean[2]).all()
    bad = [r.copy() for r in rows]
    bad[3][2000] = np.nan                                       # one degraded row
    corr, delay, peak = _delay(engine, clips, bad, D)
    assert delay[3] == 0 and np.isnan(peak[3]) and np.isnan(corr[3]).any()
    keep = [r for r in range(6) if r != 3]
    assert np.array_equal(_bits64(corr[keep]), _bits64(clean[0][keep])) and np.array_equal(delay[keep], clean[1][keep])
    assert np.array_equal(_bits64(peak[keep]), _bits64(clean[2][keep])), "no other row changes a bit"
    bad_clip = [c.copy() for c in clips]
    bad_clip[2][8000] = np.nan                                  # one clean clip: its G rows
    corr, delay, peak = _delay(engine, bad_clip, rows, D)
    assert delay[4:].tolist() == [0, 0] and np.isnan(peak[4:]).all()
    assert np.array_equal(_bits64(corr[:4]), _bits64(clean[0][:4])) and np.array_equal(delay[:4], clean[1][:4])
    assert np.array_equal(_bits64(peak[:4]), _bits64(clean[2][:4]))
    inf_row = [r.copy() for r in rows]
    inf_row[0][100] = np.inf                                    # +inf meets a padding zero somewhere: NaN
    corr, delay, peak = _delay(engine, clips, inf_row, D)
    assert np.array_equal(_bits64(corr[1:]), _bits64(clean[0][1:])) and np.array_equal(delay[1:], clean[1][1:])


def test_invalid_arguments_return_a_status_and_a_message_and_touch_nothing(engine):
    lib = engine.lib
    clips = [_pcm(1025, 1), _pcm(300, 2)]
    rows = [_pcm(m, 3 + m) for m in (1030, 1000, 337, 290)]
    inv = _lib.NOMAD_ERR_INVALID

    def refused(status, what, **kw):
        c = _Delay(engine, clips, rows, 64)
        rc = c.run(**kw)
        assert rc == status, (what, rc)
        assert lib.nomad_last_error(), what
        c.guards.check(what)
        assert c.untouched(), f"{what}: an output or the workspace was written"

    for name in ("ctx", "x", "lens", "y", "dlens", "delay", "peak", "ws"):
        refused(inv, f"NULL {name}", **{name: None})
    refused(inv, "B = 0", B=0)
    refused(inv, "B = 65536", B=65536)
    refused(inv, "G = 0", G=0)
    refused(inv, "G = 65", G=65)
    refused(inv, "max_delay = -1", D=-1)
    refused(inv, "max_delay = 16385", D=16385)
    refused(inv, "a clean length of 0", lens=[1025, 0])
    refused(inv, "a degraded length of 0", dlens=[1030, 1000, 0, 290])
    refused(inv, "stride = 0", stride=0)
    refused(inv, "stride shorter than a length", stride=1024)
    refused(inv, "deg_stride = 0", deg_stride=0)
    refused(inv, "deg_stride shorter than a length", deg_stride=1029)
    refused(_lib.NOMAD_ERR_WORKSPACE, "a short workspace", ws_bytes=256)

    def shift_refused(status, what, **kw):
        c = _Shift(engine, rows, [1, -1, 5, 0], [1025, 1025, 300, 300])
        rc = c.run(**kw)
        assert rc == status, (what, rc)
        assert lib.nomad_last_error(), what
        c.guards.check(what)
        assert c.untouched(), f"{what}: the output or the workspace was written"

    for name in ("ctx", "y", "dlens", "delay", "olens", "out", "ws"):
        shift_refused(inv, f"shift: NULL {name}", **{name: None})
    shift_refused(inv, "shift: R = 0", R=0)
    shift_refused(inv, "shift: R above 65535 x 64", R=65535 * 64 + 1)
    shift_refused(inv, "shift: a degraded length of 0", dlens=[1030, 0, 337, 290])
    shift_refused(inv, "shift: an output length of 0", olens=[1025, 1025, 0, 300])
    shift_refused(inv, "shift: deg_stride shorter than a length", deg_stride=1029)
    shift_refused(inv, "shift: out_stride shorter than a length", out_stride=1024)
    shift_refused(inv, "shift: out_stride = 0", out_stride=0)
    shift_refused(_lib.NOMAD_ERR_WORKSPACE, "shift: a short workspace", ws_bytes=256)

    size = lib.nomad_align_scratch_bytes
    assert size(0, 1, 100, 100, 5) == 0 and size(65536, 1, 100, 100, 5) == 0 and size(2, 0, 100, 100, 5) == 0 and size(2, 65, 100, 100, 5) == 0
    assert size(2, 2, 0, 100, 5) == 0 and size(2, 2, 100, 0, 5) == 0 and size(2, 2, 100, 100, -1) == 0 and size(2, 2, 100, 100, 16385) == 0
    assert size(2, 2, 100, 100, 0) >= 4 * (2 + 4) + 8 * 4 and size(1, 1, 100, 100, 16384) >= 8 * 32769
    # the largest max_delay is accepted: 16384 samples on a clip of 300
    x, y = _ints(300, 5), _ints(337, 6)
    corr, delay, peak = _delay(engine, [x], [y], 16384)
    assert np.array_equal(corr[0], align_ref.corr(x, y, 16384)) and (int(delay[0]), float(peak[0])) == align_ref.select(corr[0], 16384)


# ---- the host layer --------------------------------------------------------------------------------------------------------------
def test_engine_align_is_delay_then_shift(engine):
    D = 300
    lens = [4000, 9001]
    clips = [torch.from_numpy(_pcm(n, 60 + n)) for n in lens]
    shifts = [[-300, 37], [0, 211]]
    rows = [torch.from_numpy(align_ref.shift(clips[b].numpy(), -d, lens[b] + 50 + 7 * g)) for b in range(2) for g, d in enumerate(shifts[b])]
    with guard.guarded(case="Engine.align"):
        (moved, out_lens), delay, peak = engine.align(engine._pack(clips), engine._pack(rows), 2, D)
        d2, p2, corr = engine.align_delay(engine._pack(clips), engine._pack(rows), 2, D, want_corr=True)
    assert out_lens == [4000, 4000, 9001, 9001] and moved.shape == (4, 9004) and delay.dtype == torch.int32 and peak.dtype == torch.float64
    assert delay.tolist() == [-300, 37, 0, 211] and torch.equal(d2, delay) and torch.equal(p2, peak) and corr.shape == (4, 601)
    for r in range(4):
        want = align_ref.shift(rows[r].numpy(), int(delay[r]), out_lens[r], stride=9004)
        assert np.array_equal(_bits32(moved[r].cpu().numpy()), _bits32(want))
        assert (float(peak[r]), int(delay[r])) == (float(corr[r, int(delay[r]) + D]), align_ref.select(corr[r].cpu().numpy(), D)[0])
    with pytest.raises(ValueError, match="max_delay"):
        engine.align_delay(engine._pack(clips), engine._pack(rows), 2, 16385)
    with pytest.raises(ValueError, match="G rows per clean clip"):
        engine.align_delay(engine._pack(clips), engine._pack(rows[:3]), 2, D)


# ---- the caller's stream ----------------------------------------------------------------------------------------------------------
SPIN_MS = 100.0
S_LENS = [1280, 9001, 16384, 33000]
S_STRIDE, S_DEG_STRIDE, S_G, S_D = 33000, 33040, 2, 300


@pytest.fixture(scope="module")
def eng(built_lib, sd0):
    from nomad_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test running without a GPU")
    e = Engine(sd0, 0)
    yield e
    e.close()


def _wav(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(*shape, generator=g)).clamp(-1, 1).cuda()


def _toy(target):
    """``y = x * 2`` under ``target`` with no wait_stream in either direction: mis-ordered on purpose."""
    def call(_, bufs):
        with torch.cuda.stream(target):
            return bufs["x"] * 2
    return call


def _seen(rep):
    return rep.held and any("clone of output 0" in p and "STALE" in p for p in rep.problems)


@pytest.fixture(scope="module")
def S(eng):
    notes = []
    for attempt in range(4):
        s, other = torch.cuda.Stream(), torch.cuda.Stream()
        rep = screen(eng, s, lambda seed: {"x": _wav(seed, 1 << 16)}, _toy(other), SPIN_MS, name="toy", side=None, watch_abi=False)
        notes.append(f"attempt {attempt}: seen={_seen(rep)} [{rep.line()}]")
        print(notes[-1])
        if _seen(rep):
            return s
    pytest.fail("the screen is blind here: a call mis-ordered on purpose was not seen on any of four pool streams - " + " | ".join(notes))


def _judge(rep):
    print(rep.line())
    assert not rep.problems, rep.line()
    assert rep.host_arrays > 0, f"{rep.name}: no host array went through the C ABI"
    assert rep.held, f"{rep.name}: S was found released when the call returned, so the case shows nothing about producer ordering ({rep.line()})"


def _pair(seed):
    clean = _wav(seed, len(S_LENS), S_STRIDE)
    deg = torch.zeros(len(S_LENS) * S_G, S_DEG_STRIDE, device="cuda")
    for r in range(len(S_LENS) * S_G):
        d = 5 + 7 * r + seed % 11
        k = min(S_STRIDE, S_DEG_STRIDE - d)
        deg[r, d:d + k] = clean[r // S_G, :k]
    return {"clean": clean, "deg": (deg + 0.02 * _wav(seed + 1, len(S_LENS) * S_G, S_DEG_STRIDE)).contiguous()}


S_DLENS = [n + 40 for n in S_LENS for _ in range(S_G)]


class _Tables:
    """Stands between the engine and its library for one call: every ctypes array that goes into a ``nomad_align_*`` entry point
    is overwritten with other valid lengths as soon as the entry point has returned - while S is still held, so ahead of the
    kernels.  The screen itself sees the first host table of an entry point it does not list; this covers the second one too."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("nomad_align_") or name.endswith("_bytes"):
            return fn

        def call(*args):
            rc = fn(*args)
            tables = [a for a in args if isinstance(a, C.Array)]
            assert len(tables) == 2, name
            for t in tables:
                t[:] = [400] * len(t)
            return rc

        return call


def _with_tables_overwritten(fn):
    def call(e, x):
        lib = e.lib
        e.lib = _Tables(lib)
        try:
            return fn(e, x)
        finally:
            e.lib = lib
    return call


def test_align_delay_keeps_to_the_callers_stream(eng, S):
    rep = screen(eng, S, _pair, _with_tables_overwritten(
        lambda e, x: e.align_delay((x["clean"], list(S_LENS)), (x["deg"], list(S_DLENS)), S_G, S_D, want_corr=True)),
                 SPIN_MS, "align_delay", "late", ["delay", "peak", "corr"])
    _judge(rep)


def test_align_shift_keeps_to_the_callers_stream(eng, S):
    def make(seed):
        x = _pair(seed)
        x["delay"] = torch.randint(-S_D, S_D + 1, (len(S_DLENS),), generator=torch.Generator().manual_seed(seed), dtype=torch.int32).cuda()
        del x["clean"]
        return x

    rep = screen(eng, S, make, _with_tables_overwritten(
        lambda e, x: e.align_shift((x["deg"], list(S_DLENS)), x["delay"], [n for n in S_LENS for _ in range(S_G)])[0]),
                 SPIN_MS, "align_shift", "late", ["rows"])
    _judge(rep)


def test_align_keeps_to_the_callers_stream(eng, S):
    """All three launches, the delays going from the second to the third in device memory."""
    def call(e, x):
        (rows, _), delay, peak = e.align((x["clean"], list(S_LENS)), (x["deg"], list(S_DLENS)), S_G, S_D)
        return rows, delay, peak

    rep = screen(eng, S, _pair, _with_tables_overwritten(call), SPIN_MS, "align", "late", ["rows", "delay", "peak"])
    _judge(rep)
