"""GPU: ``nomad_degrade_normalize`` through the C ABI in guarded, NaN-poisoned buffers, against the float64 restatement
``loudness_ref``; then ``Nomad.loudness`` / ``Nomad.normalize`` / ``Nomad.intensity_sweep(normalize=...)`` end to end.

Bounds (include/nomad_hip.h states the arithmetic):
* level: within 1e-9 dB of ``loudness_ref``.  Float64 sums of at most 1e5 terms taken in another order differ by at most about 1e-11
  relatively = 5e-11 dB; the chunked recurrence with its state hand-over, emulated on the CPU, was within 1.4e-13 dB of
  ``scipy.signal.lfilter``.  The margin is a factor of 20.  (A float32 filter misses it: 4e-7 relative in energy.)
* sample peak and number of blocks past both gates: EQUAL.  No input sits on a gate: the reference's smallest distance of any
  block from either gate is asserted to be above 1e-6 dB for every input.
* gain: 1e-9 relative.  Output rows: ``float32(float64(x) gain)`` with the gain read back from the device, bit for bit; zero behind
  the length; guards intact.
* ``Nomad.normalize`` rows re-measured: the target to 1e-4 dB.  Rounding the output to float32 moves a sample by at most 2^-24
  relatively, so the level by at most 20 log10(1 + 2^-24) = 5.2e-7 dB; found: 1.5e-8 dB (ebu), 1.3e-9 dB (rms), 4.9e-7 dB (peak:
  the rounding of the one sample that is the peak).
The lengths straddle one chunk of 1600 samples, one block of 6400 samples (below it there is no level) and several chunks that do
not end on a chunk boundary; 48 kHz has chunks of 4800."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import guard
import loudness_ref as L
from nomad_amd import _lib

pytestmark = pytest.mark.gpu

LENS = [1, 6399, 6400, 6401, 7999, 8000, 8001, 16777, 48001]
NAN = float("nan")


def _noise_rows():
    return [L.pcm_noise(n, 300 + n) for n in LENS]


def _special_rows():
    return [L.silent_second(48001, 16000, 21), L.quiet_passage(48001, 16000, 22), L.dc_offset(16777, 23), np.zeros(8000, dtype=np.float32),
            L.sine(16777, 16000), L.dc_offset(6401, 24), L.sine(7999, 16000), L.quiet_passage(8001, 16000, 25)]


def _rows_48k():
    return [L.pcm_noise(24000, 26), L.sine(33333, 48000)]


BATCHES = {"noise": (_noise_rows, 16000), "special": (_special_rows, 16000), "48k": (_rows_48k, 48000)}
_REF = {}


def _ref(batch, kind):
    """``loudness_ref.measure`` of every row of a batch, computed once per (batch, mode)."""
    if (batch, kind) not in _REF:
        make, fs = BATCHES[batch]
        _REF[batch, kind] = [L.measure(x, fs, kind) for x in make()]
    return _REF[batch, kind]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


class _Call:
    """One ABI call in guarded buffers: input rows NaN behind their length, outputs NaN-filled, workspace 0xFF."""

    def __init__(self, engine, rows, fs=16000, inplace=False, stride=None, x_off=0, out_off=0):
        """x_off / out_off: the rows begin that many floats (0 .. 3) behind a 256-byte boundary (``guard.Guards.empty_at``): base
        addresses aligned to 4 or 8 bytes only (in place: x_off for both).  Statistics and workspace stay aligned."""
        self.engine, self.rows, self.fs = engine, rows, fs
        self.R = len(rows)
        self.lens = [int(r.shape[0]) for r in rows]
        self.stride = stride if stride is not None else (max(self.lens) + 3) // 4 * 4
        dev = engine.device
        self.guards = g = guard.Guards()
        host = np.full((self.R, self.stride), np.nan, dtype=np.float32)
        for r, x in enumerate(rows):
            host[r, :min(self.lens[r], self.stride)] = x[:self.stride]
        self.x = g.empty_at((self.R, self.stride), x_off, device=dev, name="x")
        self.x.copy_(torch.from_numpy(host))
        self.out = self.x if inplace else g.empty_at((self.R, self.stride), out_off, device=dev, name="out")
        if not inplace:
            self.out.fill_(NAN)
        self.stats = g.empty((self.R, 4), dtype=torch.float64, device=dev, name="stats")
        self.stats.fill_(NAN)
        need = int(engine.lib.nomad_degrade_normalize_scratch_bytes(self.R, self.stride, fs))
        self.ws = g.empty_bytes(max(need, 256), dev, 1 << 16, "workspace")
        self.ws.fill_(0xFF)
        self.ws_bytes = need

    def run(self, kind="ebu", target=-23.0, peak_db=NAN, out=True, stats=True, **over):
        a = dict(x=self.x.data_ptr(), R=self.R, stride=self.stride, lens=self.lens, fs=self.fs, mode=_lib.LOUDNESS_MODE.get(kind, kind),
                 target=target, peak_db=peak_db, stats=self.stats.data_ptr() if stats else None,
                 out=out if type(out) is int else self.out.data_ptr() if out else None,      # True / False, or an address of the caller's
                 ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(over)
        rc = self.engine.lib.nomad_degrade_normalize(self.engine.ctx, a["x"], a["R"], a["stride"], (C.c_int * len(a["lens"]))(*a["lens"]),
                                                     a["fs"], a["mode"], a["target"], a["peak_db"], a["out"], a["stats"], a["ws"],
                                                     a["ws_bytes"], self.engine._stream())
        torch.cuda.synchronize()
        return rc

    def results(self):
        self.guards.check()
        return self.out.cpu().numpy(), self.stats.cpu().numpy()


def _check(out, stats, rows, refs, target, peak_db, case):
    for r, (x, ref) in enumerate(zip(rows, refs)):
        n = x.shape[0]
        level, peak, g, blocks = stats[r]
        assert ref["margin"] > 1e-6, (case, r, "the input sits on a gate", ref)
        print(f"{case} row {r} n={n}: level {level!r} (ref {ref['level']!r}), peak {peak!r}, gain {g!r}, blocks {blocks} of {ref['total']}")
        if ref["level"] == -math.inf:
            assert level == -math.inf, (case, r, level)
        else:
            assert abs(level - ref["level"]) <= 1e-9, (case, r, level, ref["level"])
        assert peak == ref["peak"] and blocks == ref["blocks"], (case, r, peak, ref["peak"], blocks, ref["blocks"])
        want = L.gain(ref["level"], ref["peak"], target, None if math.isnan(peak_db) else peak_db)
        assert abs(g - want) <= 1e-9 * want, (case, r, g, want)
        if out is not None:
            assert np.array_equal(_bits(out[r, :n]), _bits(L.apply(x, g))), (case, r, "the row is not float32(float64(x) gain)")
            assert not out[r, n:].any() and not np.isnan(out[r, n:]).any(), f"{case} row {r}: not zero behind the length"


# ---- the measurement and the gain ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,target", [("ebu", -23.0), ("rms", -20.0), ("peak", -1.0)])
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_level_peak_blocks_gain_and_rows(engine, batch, kind, target):
    make, fs = BATCHES[batch]
    rows = make()
    call = _Call(engine, rows, fs)
    assert call.run(kind, target) == 0, engine.lib.nomad_last_error()
    out, stats = call.results()
    _check(out, stats, rows, _ref(batch, kind), target, NAN, f"{batch}/{kind}")
    again = _Call(engine, rows, fs)
    assert again.run(kind, target) == 0
    out2, stats2 = again.results()
    assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(_bits(stats), _bits(stats2)), "run to run"
    # in place equals out of place; measuring alone writes the statistics only
    inplace = _Call(engine, rows, fs, inplace=True)
    assert inplace.run(kind, target) == 0
    out3, stats3 = inplace.results()
    assert np.array_equal(_bits(out), _bits(out3)) and np.array_equal(_bits(stats), _bits(stats3)), "in place"
    only = _Call(engine, rows, fs)
    assert only.run(kind, target, out=False) == 0
    out4, stats4 = only.results()
    assert np.isnan(out4).all() and np.array_equal(_bits(stats), _bits(stats4)), "measure only"
    nostats = _Call(engine, rows, fs)
    assert nostats.run(kind, target, stats=False) == 0
    out5, stats5 = nostats.results()
    assert np.array_equal(_bits(out), _bits(out5)) and np.isnan(stats5).all(), "no statistics wanted"


@pytest.mark.parametrize("batch", ["noise", "special"])
def test_a_row_has_the_bits_of_its_own_call(engine, batch):
    make, fs = BATCHES[batch]
    rows = make()
    call = _Call(engine, rows, fs)
    assert call.run() == 0
    out, stats = call.results()
    for r, x in enumerate(rows):
        n = x.shape[0]
        one = _Call(engine, [x], fs)
        assert one.run() == 0
        o1, s1 = one.results()
        assert np.array_equal(_bits(s1[0]), _bits(stats[r])) and np.array_equal(_bits(o1[0, :n]), _bits(out[r, :n])), (batch, r, s1[0], stats[r])


# (x offset, out offset) in floats: together and separately - one misaligned pointer is enough to leave the 16-byte gain kernel
OFFSETS = [(1, 1), (2, 2), (3, 3), (1, 0), (0, 3), (2, 1)]


def _aligned_rows():
    return [L.pcm_noise(16777, 51), L.pcm_noise(8001, 52), L.sine(16777, 16000), L.pcm_noise(6399, 53)]


def _aligned_ref(engine, kind, target):
    if ("aligned", kind) not in _REF:
        call = _Call(engine, _aligned_rows())
        assert call.run(kind, target) == 0
        _REF["aligned", kind] = call.results()
    return _REF["aligned", kind]


@pytest.mark.parametrize("kind,target", [("ebu", -23.0), ("peak", -1.0)])
@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: "x%d-out%d" % o)
def test_rows_at_unaligned_addresses_have_the_bits_of_the_aligned_call(engine, offs, kind, target):
    """The gain pass moves 16 bytes per thread where both rows' bases are 16-byte aligned and one sample per thread otherwise
    (``loudness_gain_kernel<1>``); the two walks read sample by sample.  Rows of 16777 and 8001 samples (no multiple of 4: the last
    group of four straddles the length) at a stride of 16780 whose base is aligned to a float and nothing wider: the statistics
    and the rows of the aligned call, bit for bit, zeros behind each length, guards intact (they begin at the very next float) -
    out of place, in place and measuring alone."""
    xo, oo = offs
    rows = _aligned_rows()
    out, stats = _aligned_ref(engine, kind, target)
    call = _Call(engine, rows, x_off=xo, out_off=oo)
    assert call.x.data_ptr() % 16 == 4 * xo and call.out.data_ptr() % 16 == 4 * oo
    assert call.run(kind, target) == 0, engine.lib.nomad_last_error()
    got, gstats = call.results()
    assert np.array_equal(_bits(gstats), _bits(stats)), "statistics"
    assert np.array_equal(_bits(got), _bits(out)), "rows (zeros behind the lengths included)"
    for r, x in enumerate(rows):
        n = x.shape[0]
        assert np.array_equal(_bits(got[r, :n]), _bits(L.apply(x, gstats[r, 2]))), (r, "the row is not float32(float64(x) gain)")
        assert not got[r, n:].any() and not np.isnan(got[r, n:]).any(), f"row {r}: not zero behind the length"
    if xo:
        inplace = _Call(engine, rows, inplace=True, x_off=xo)
        assert inplace.out.data_ptr() == inplace.x.data_ptr() and inplace.x.data_ptr() % 16 == 4 * xo
        assert inplace.run(kind, target) == 0
        got3, stats3 = inplace.results()
        assert np.array_equal(_bits(got3), _bits(out)) and np.array_equal(_bits(stats3), _bits(stats)), "in place"
        only = _Call(engine, rows, x_off=xo, out_off=oo)
        assert only.run(kind, target, out=False) == 0
        got4, stats4 = only.results()
        assert np.isnan(got4).all() and np.array_equal(_bits(stats4), _bits(stats)), "measure only"


def test_the_ceiling_lowers_the_gain_exactly(engine):
    rows = _noise_rows()[3:] + [L.sine(16777, 16000), L.sine(7999, 16000, amp=0.5)]
    refs = _ref("noise", "ebu")[3:] + [L.measure(x, 16000) for x in rows[-2:]]
    call = _Call(engine, rows)
    # at -5.5 LUFS a sine (level 2.97 dB under its peak) would peak at -2.53 dBFS, the noise (2 dB under its peak) at -3.5 dBFS
    assert call.run("ebu", -5.5, -3.0) == 0
    out, stats = call.results()
    _check(out, stats, rows, refs, -5.5, -3.0, "ceiling")
    cap = 10.0 ** (-3.0 / 20.0)
    bound = []
    for r, ref in enumerate(refs):
        if 10.0 ** ((-5.5 - ref["level"]) / 20.0) * ref["peak"] > cap:
            bound.append(r)
            assert abs(stats[r, 2] - cap / ref["peak"]) <= 1e-15 * stats[r, 2], (r, stats[r, 2], cap / ref["peak"])
            assert abs(np.abs(out[r]).max() - cap) <= 2.0 ** -24, (r, np.abs(out[r]).max())
        else:
            assert np.abs(out[r]).max() < cap
    assert bound == [len(rows) - 2, len(rows) - 1], "the ceiling binds for the two sines and not for the noise rows"


def test_a_non_finite_sample_voids_its_row_and_no_other(engine):
    clean = [L.pcm_noise(8001, 31), L.pcm_noise(16777, 32), L.pcm_noise(8000, 33), L.pcm_noise(7999, 34)]
    bad = [x.copy() for x in clean]
    bad[1][9000] = np.nan
    bad[3][5] = np.inf
    for kind in L.MODES:
        ref = _Call(engine, clean)
        assert ref.run(kind) == 0
        out0, stats0 = ref.results()
        call = _Call(engine, bad)
        assert call.run(kind) == 0
        out, stats = call.results()
        for r in (0, 2):
            assert np.array_equal(_bits(out[r]), _bits(out0[r])) and np.array_equal(_bits(stats[r]), _bits(stats0[r])), (kind, r)
        for r in (1, 3):
            n = bad[r].shape[0]
            assert not np.isfinite(stats[r]).any(), (kind, r, stats[r])
            assert not np.isfinite(out[r, :n]).any(), (kind, r)
            assert not out[r, n:].any() and not np.isnan(out[r, n:]).any(), (kind, r, "zeros stay behind the length")


def test_argument_errors_return_before_anything_is_queued(engine):
    lib = engine.lib
    rows = [L.pcm_noise(8000, 41), L.pcm_noise(300, 42)]

    def refused(status, what, **over):
        call = _Call(engine, rows)
        rc = call.run(**over)
        assert rc == status, (what, rc)
        assert lib.nomad_last_error(), what
        call.guards.check(what)
        assert bool(torch.isnan(call.out).all()) and bool(torch.isnan(call.stats).all()), f"{what}: the outputs were written"
        return call

    inv = _lib.NOMAD_ERR_INVALID
    refused(inv, "NULL x_dev", x=None)
    refused(inv, "both outputs NULL", out=False, stats=False)
    refused(inv, "R = 0", R=0, lens=[8000])
    refused(inv, "R = 65536", R=65536)
    refused(inv, "stride no multiple of 4", stride=8002)
    refused(inv, "stride shorter than a length", stride=7996)
    refused(inv, "stride = 0", stride=0)
    refused(inv, "a length of 0", lens=[8000, 0])
    refused(inv, "sample_rate below 8000", fs=7990)
    refused(inv, "sample_rate above 192000", fs=192010)
    refused(inv, "sample_rate no multiple of 10", fs=16001)
    refused(inv, "mode = 3", mode=3)
    refused(inv, "mode = -1", mode=-1)
    refused(inv, "a NaN target", target=NAN)
    refused(inv, "an infinite target", target=float("inf"))
    refused(_lib.NOMAD_ERR_WORKSPACE, "a short workspace", ws_bytes=1024)
    call = _Call(engine, rows)
    assert call.run(out=call.x.data_ptr() + 4 * call.stride) == inv, "an output one row into the input"
    call.guards.check()
    assert bool(torch.isnan(call.stats).all()) and np.array_equal(_bits(call.x.cpu().numpy()[0]), _bits(rows[0]))
    assert lib.nomad_degrade_normalize_scratch_bytes(0, 8000, 16000) == 0 and lib.nomad_degrade_normalize_scratch_bytes(2, 8002, 16000) == 0
    assert lib.nomad_degrade_normalize_scratch_bytes(2, 8000, 16001) == 0 and lib.nomad_degrade_normalize_scratch_bytes(65536, 8000, 16000) == 0
    assert lib.nomad_degrade_normalize_scratch_bytes(2, 8000, 16000) >= 2 * 5 * 11 * 8


# ---- the host layers -------------------------------------------------------------------------------------------------------------
def _clips():
    lens = [8000, 7001, 8000]
    clean = torch.zeros(3, 8000)
    for b, n in enumerate(lens):
        clean[b, :n] = torch.from_numpy(L.pcm_noise(n, 70 + b, 0.05 * (b + 1)))
    return clean, lens


def test_normalized_rows_read_the_target(engine):
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    clean, lens = _clips()
    before = nomad.loudness(clean, lens).cpu().numpy()
    want = [L.measure(clean[b, :n].numpy(), 16000)["level"] for b, n in enumerate(lens)]
    assert before.dtype == np.float64 and np.abs(before - want).max() <= 1e-9
    for kind, target in (("ebu", -23.0), ("rms", -30.0), ("peak", -6.0)):
        with guard.guarded(case=f"Nomad.normalize {kind}"):
            rows, lens_out, stats = nomad.normalize(clean, target=target, kind=kind, lengths=lens)
        assert rows.shape == (3, 8000) and lens_out == lens and stats.shape == (3, 4) and stats.dtype == torch.float64
        after = nomad.loudness(rows, lens, kind=kind).cpu().numpy()
        print(f"{kind}: target {target}, re-measured {after.tolist()}, off by {np.abs(after - target).max():.3g} dB")
        assert np.abs(after - target).max() <= 1e-4, (kind, after)
        assert not rows[1, 7001:].any()
        assert torch.equal(stats[:, 0].cpu(), nomad.loudness(clean, lens, kind=kind).cpu())
    rows, _, stats = nomad.normalize(clean, target=0.0, lengths=lens, peak_db=-1.0)
    assert float(rows.abs().max()) <= 10.0 ** (-1.0 / 20.0) * (1 + 2.0 ** -23)
    short = nomad.loudness(clean[:, :6399])
    assert bool(torch.isinf(short).all()) and bool((short < 0).all()), "under 400 ms there is no block"
    same, _, st = nomad.normalize(clean[:, :6399])
    assert torch.equal(same.cpu()[:, :6399], clean[:, :6399]) and st[:, 2].tolist() == [1.0] * 3, "and the clip is returned unchanged"


def test_sweep_without_normalize_is_unchanged_and_with_it_scores_the_normalized_rows(engine):
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    clean, lens = _clips()
    noise = torch.from_numpy(L.pcm_noise(3000, 9, 0.2))
    gen = torch.Generator().manual_seed(5)
    refs = torch.randn(5, 256, generator=gen, dtype=torch.float64)
    refs = (refs / refs.norm(dim=1, keepdim=True)).float()
    snr = [0, 20]
    rows, lens_rep = nomad.degrade(clean, "noise", snr, noise=noise, lengths=lens)
    plain = nomad.intensity_sweep(clean, refs, noise=noise, snr_db=snr, lengths=lens, normalize=None)["NOISE"]
    assert "gain_db" not in plain
    assert np.array_equal(_bits(plain["scores"]), _bits(nomad.score(rows, refs, lengths=lens_rep).cpu().numpy())), "normalize=None: today's bits"
    with guard.guarded(case="intensity_sweep(normalize=-23)"):
        res = nomad.intensity_sweep(clean, refs, noise=noise, snr_db=snr, lengths=lens, normalize=-23)["NOISE"]
    norm_rows, norm_lens, stats = nomad.normalize(rows, target=-23.0, lengths=lens_rep)
    want = nomad.score(norm_rows, refs, lengths=norm_lens).cpu().numpy()
    assert res["scores"].dtype == np.float64 and np.array_equal(_bits(res["scores"]), _bits(want)), (res["scores"], want)
    assert not np.array_equal(res["scores"], plain["scores"]), "the level changes the score: the rows were normalised"
    gain_db = 20.0 * np.log10(stats[:, 2].cpu().numpy())
    assert res["gain_db"].shape == (6,) and np.array_equal(_bits(res["gain_db"]), _bits(gain_db))
    assert np.abs(nomad.loudness(norm_rows, norm_lens).cpu().numpy() + 23.0).max() <= 1e-4
    assert (gain_db[0::2] < gain_db[1::2]).all(), "noise at 0 dB SNR is louder than at 20 dB: it takes the smaller gain"
