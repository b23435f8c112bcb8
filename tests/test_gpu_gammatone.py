"""GPU: ``nomad_gammatone`` through the C ABI in guarded buffers - input NaN behind each length, output NaN-filled, workspace
0xFF - against the long-double restatement ``nsim_ref.spectrogram``.

Bound (include/nomad_hip.h states the arithmetic): every S within REL = 3.6e-11 of the restatement relatively, plus 1e-300
absolutely for S = 0 (digital silence gives exactly 0 on both sides).  The device runs the recurrence in float64, the restatement
in long double; what float64 can differ by on THESE inputs was measured on the CPU: the same per-sample recurrence in numpy float64
against the long-double one (``nsim_ref.spectrogram(x, fs, np.float64)``) over every row of this module.  Largest relative
distance: 1.8e-12, in the 50 Hz band of the 48 kHz sine row (S = 2e-4 there: the band is 55 dB under the tone, and four cascaded
sections with poles at radius 0.996 cancel most of what each puts out); the other rows are between 1e-14 and 1.7e-13 (one second
of speech was at 2.2e-13 while drafting).  The bound is 20 x the largest.  An fp32 filter is 2.3e-4 away (row of 1920 noise
samples): seven orders of magnitude outside it.  Every case prints the device's largest relative distance per row; MEASURED on an
MI355X: 3.0e-12 on that 48 kHz sine row, 1.9e-12 on the 48 kHz noise row, 4.4e-14 to 1.4e-13 on the 16 kHz rows, 0 on silence.

Lengths at 16 kHz (W = 1280, H = 320) straddle one frame (1280, 1281, 1599), two and three frames (1600, 1920), the kernel's
frames-per-workgroup boundary one frame either side (11, 12 and 13 frames for the 12 the kernel exports, read from
csrc/nsim.hip.h) and 16777 (49 frames, five workgroups); at 48 kHz rows of 3840 (one frame) and 33333 samples (31 frames)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import guard
import nsim_ref as N
from conftest import ROOT
from nomad_amd import _lib

pytestmark = pytest.mark.gpu

REL, ABS = 3.6e-11, 1e-300
NAN = float("nan")


def block_frames() -> int:
    text = open(os.path.join(ROOT, "nomad_amd", "csrc", "nsim.hip.h")).read()
    return int(re.search(r"constexpr int kGammatoneBlockFrames = (\d+);", text).group(1))


def frames_len(F: int, fs: int = 16000, extra: int = 0) -> int:
    H = fs // 50
    return 4 * H + (F - 1) * H + extra


def sine(n, fs, freq, amp=0.5):
    return (amp * np.sin(2.0 * np.pi * freq * np.arange(n) / fs)).astype(np.float32)


def dc_offset(n, seed, offset=0.5):
    return (N.pcm_noise(n, seed, 0.1) + np.float32(offset)).astype(np.float32)


def _rows_16k():
    K = block_frames()
    lens = [1280, 1281, 1599, 1600, 1920, frames_len(K - 1, extra=5), frames_len(K), frames_len(K + 1, extra=7), 16777]
    return [N.pcm_noise(n, 500 + n) for n in lens]


def _rows_special():
    K = block_frames()
    cf = N.centres()
    return [sine(frames_len(K), 16000, cf[10]), dc_offset(frames_len(K + 1), 61), np.zeros(1920, dtype=np.float32), sine(1599, 16000, cf[0]),
            sine(1600, 16000, cf[20])]


def _rows_48k():
    return [N.pcm_noise(3840, 71), sine(33333, 48000, N.centres()[15])]


BATCHES = {"noise": (_rows_16k, 16000), "special": (_rows_special, 16000), "48k": (_rows_48k, 48000)}
_REF = {}


def ref(batch):
    """The long-double restatement of every row of a batch, computed once and left unchanged."""
    if batch not in _REF:
        make, fs = BATCHES[batch]
        _REF[batch] = [N.spectrogram(x, fs) for x in make()]
        for S in _REF[batch]:
            S.setflags(write=False)
    return _REF[batch]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Call:
    """One ABI call in guarded buffers."""

    def __init__(self, engine, rows, fs=16000, stride=None, x_off=0):
        self.engine, self.fs = engine, fs
        self.R = len(rows)
        self.lens = [int(r.shape[0]) for r in rows]
        self.stride = stride if stride is not None else (max(self.lens) + 3) // 4 * 4
        self.frames = [N.frames_of(n, fs) for n in self.lens]
        dev = engine.device
        self.guards = g = guard.Guards()
        host = np.full((self.R, self.stride), np.nan, dtype=np.float32)
        for r, x in enumerate(rows):
            host[r, :min(self.lens[r], self.stride)] = x[:self.stride]
        self.x = g.empty_at((self.R, self.stride), x_off, device=dev, name="x")
        self.x.copy_(torch.from_numpy(host))
        self.spec = g.empty((max(sum(self.frames), 1), 21), dtype=torch.float64, device=dev, name="spec")
        self.spec.fill_(NAN)
        need = int(engine.lib.nomad_gammatone_scratch_bytes(self.R, self.stride, fs))
        self.ws = g.empty_bytes(max(need, 256), dev, 1 << 16, "workspace")
        self.ws.fill_(0xFF)
        self.ws_bytes = need

    def run(self, **over):
        a = dict(x=self.x.data_ptr(), R=self.R, stride=self.stride, lens=self.lens, fs=self.fs, spec=self.spec.data_ptr(),
                 ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(over)
        rc = self.engine.lib.nomad_gammatone(self.engine.ctx, a["x"], a["R"], a["stride"], (C.c_int * len(a["lens"]))(*a["lens"]), a["fs"],
                                             a["spec"], a["ws"], a["ws_bytes"], self.engine._stream())
        torch.cuda.synchronize()
        return rc

    def results(self):
        """-> the rows' spectrograms [F_r][21], guards checked."""
        self.guards.check()
        flat = self.spec.cpu().numpy()
        at = np.concatenate([[0], np.cumsum(self.frames)])
        return [flat[at[r]:at[r + 1]] for r in range(self.R)]


def _distance(S, want):
    want64 = np.asarray(want, dtype=np.float64)
    err = np.abs(S.astype(np.longdouble) - want)
    worst = float(np.max(err / np.maximum(np.abs(want), np.longdouble(1e-300)), initial=0.0, where=want != 0))
    assert (err <= REL * np.abs(want) + ABS).all(), (worst, float(err.max()), want64[np.unravel_index(np.argmax(err), err.shape)])
    return worst


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_every_value_is_held_to_the_restatement(engine, batch):
    make, fs = BATCHES[batch]
    rows = make()
    assert engine.lib.nomad_gammatone_frames(rows[0].shape[0], fs) == N.frames_of(rows[0].shape[0], fs)
    call = Call(engine, rows, fs)
    assert call.run() == 0, engine.lib.nomad_last_error()
    got = call.results()
    for r, (S, want) in enumerate(zip(got, ref(batch))):
        assert S.shape == want.shape and np.isfinite(S).all(), (batch, r, S.shape, want.shape)
        worst = _distance(S, want)
        print(f"{batch} row {r} n={rows[r].shape[0]} F={S.shape[0]}: largest relative distance {worst:.3g} (bound {REL:g})")
        if not rows[r].any():
            assert not S.any(), "digital silence gives S = 0 exactly"
    again = Call(engine, rows, fs)
    assert again.run() == 0
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again.results())), "run to run"


@pytest.mark.parametrize("batch", ["noise", "special"])
def test_a_row_has_the_bytes_of_its_own_call(engine, batch):
    make, fs = BATCHES[batch]
    rows = make()
    call = Call(engine, rows, fs)
    assert call.run() == 0
    got = call.results()
    for r, x in enumerate(rows):
        one = Call(engine, [x], fs, stride=(x.shape[0] + 3) // 4 * 4 + 8 * (r % 2))
        assert one.run() == 0
        assert np.array_equal(_bits(one.results()[0]), _bits(got[r])), (batch, r)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_rows_at_unaligned_addresses_keep_their_bits(engine, off):
    rows = _rows_16k()[4:]
    base = Call(engine, rows)
    assert base.run() == 0
    call = Call(engine, rows, x_off=off)
    assert call.x.data_ptr() % 16 == 4 * off
    assert call.run() == 0, engine.lib.nomad_last_error()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(base.results(), call.results()))


def test_a_nan_sample_voids_exactly_the_frames_that_hold_it(engine):
    rows = _rows_16k()[4:]
    clean = Call(engine, rows)
    assert clean.run() == 0
    want = clean.results()
    bad = [x.copy() for x in rows]
    hits = {0: 1500, 3: 2000, 4: 16776}          # row -> the position of its NaN (row 4: the very last sample, in no whole frame)
    bad[0][1500] = np.nan
    bad[3][2000] = np.inf
    bad[4][16776] = np.nan
    call = Call(engine, bad)
    assert call.run() == 0
    got = call.results()
    for r, S in enumerate(got):
        F = S.shape[0]
        held = np.array([r in hits and 320 * t <= hits[r] < 320 * t + 1280 for t in range(F)])
        assert np.isnan(S[held]).all() and np.array_equal(_bits(S[~held]), _bits(want[r][~held])), (r, np.isnan(S).any(axis=1))
    assert np.isnan(got[0]).any() and np.isnan(got[3]).any() and not np.isnan(got[4]).any()


def test_argument_errors_return_before_anything_is_queued(engine):
    lib = engine.lib
    rows = [N.pcm_noise(1920, 41), N.pcm_noise(1280, 42)]

    def refused(status, what, **over):
        call = Call(engine, rows)
        rc = call.run(**over)
        assert rc == status, (what, rc)
        assert lib.nomad_last_error(), what
        call.guards.check(what)
        assert bool(torch.isnan(call.spec).all()), f"{what}: the output was written"
        assert bool((call.ws == 0xFF).all()), f"{what}: the workspace was written"

    inv = _lib.NOMAD_ERR_INVALID
    refused(inv, "a length of 1279: below one frame", lens=[1920, 1279])
    refused(inv, "NULL x_dev", x=None)
    refused(inv, "NULL output", spec=None)
    refused(inv, "NULL workspace", ws=None)
    refused(inv, "R = 0", R=0, lens=[1920])
    refused(inv, "R = 65536", R=65536)
    refused(inv, "stride no multiple of 4", stride=1922)
    refused(inv, "stride shorter than a length", stride=1916)
    refused(inv, "stride = 0", stride=0)
    refused(inv, "a rate below 16000", fs=15950)
    refused(inv, "a rate above 48000", fs=48050)
    refused(inv, "a rate that is no multiple of 50", fs=16010)
    refused(_lib.NOMAD_ERR_WORKSPACE, "ws_bytes - 1", ws_bytes=Call(engine, rows).ws_bytes - 1)
    assert lib.nomad_gammatone_scratch_bytes(0, 1920, 16000) == 0 and lib.nomad_gammatone_scratch_bytes(2, 1922, 16000) == 0
    assert lib.nomad_gammatone_scratch_bytes(2, 1920, 16010) == 0 and lib.nomad_gammatone_scratch_bytes(65536, 1920, 16000) == 0
    assert lib.nomad_gammatone_scratch_bytes(2, 1920, 16000) >= 21 * 10 * 8
    assert [lib.nomad_gammatone_frames(n, 16000) for n in (1279, 1280, 1600, 16777)] == [0, 1, 2, 49]
    assert lib.nomad_gammatone_frames(33333, 48000) == 31 and lib.nomad_gammatone_frames(33333, 8000) <= 0


def test_engine_gammatone_takes_packed_rows_without_a_copy(engine):
    rows = _rows_16k()[3:6]
    want = ref("noise")[3:6]
    with guard.guarded(case="Engine.gammatone"):
        spec, frames = engine.gammatone([torch.from_numpy(x) for x in rows])
    assert frames == [S.shape[0] for S in want] and spec.shape == (sum(frames), 21) and spec.dtype == torch.float64
    got = spec.cpu().numpy()
    _distance(got, np.concatenate(want))
    buf, lens = engine._pack([torch.from_numpy(x) for x in rows])
    spec2, _ = engine.gammatone(packed=(buf, lens))
    assert np.array_equal(_bits(spec2.cpu().numpy()), _bits(got))
    with pytest.raises(ValueError, match="shorter than one frame"):
        engine.gammatone([torch.zeros(1279)])
    with pytest.raises(ValueError, match="sample_rate"):
        engine.gammatone([torch.zeros(4000)], sample_rate=8000)
