"""GPU: ``nomad_nsim`` through the C ABI in guarded buffers on the device's OWN spectrograms, against the restatement's map
(``nsim_ref.nsim_map``, float64) on those same spectrograms read back - the stage on its own input; then ``Nomad.nsim`` end to end.

B = 3 clean clips with F = 1, 2 and 92 frames (1500 and 1700 samples of PCM noise, and tests/golden/wavs/nmr-data/FI53_04.wav),
G = 3 rows each: the clip itself, and the clip with ``RandomState(0).randn`` noise at 20 dB and 5 dB SNR by the reference's formula.

Bounds, both derived from what float64 can differ by on THESE inputs, measured on the CPU:
* the stage: the map evaluated in numpy float64 against the same map in long double, on the float64 spectrograms of these nine
  pairs at the two intensity ranges used below (1 and 45): largest distance of an NSIM 4.3e-14, of a band value 4.9e-13 - both on
  the clips of one and two frames at range 1, where the variance w * X^2 - mu^2 cancels 1e3 against C3 = 4.5e-4; on the 92-frame
  clip they are 1.4e-15 and 1.8e-14 (the draft of the measure saw 2e-15 on it).  MAP_BOUND = 20 x the largest = 9.8e-12, for scores
  and band values alike.  An fp32 FILTER in front of the map moves the 92-frame clip's NSIM at 5 dB by 4.4e-7.
* end to end (``Nomad.degrade`` + ``Nomad.nsim`` against ``nsim_ref.nsim`` on the degraded rows read back): the device's spectrogram
  is float64 where the restatement's is long double, so the bound is measured in the same way over the whole chain - float64
  spectrogram and map against long-double spectrogram and map on the four degraded rows: largest distance 2.6e-15 for an NSIM,
  2.1e-14 for a band value; E2E_BOUND = 20 x the larger = 4.2e-13.
Every case prints the device's largest distance; MEASURED on an MI355X: 3.2e-14 for an NSIM and 4.2e-13 for a band value against the
restatement's map, 3.8e-14 end to end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import guard
import nsim_ref as N
from conftest import ROOT
from nomad_amd import _lib, wavio

pytestmark = pytest.mark.gpu

MAP_BOUND = 9.8e-12
E2E_BOUND = 4.2e-13
NAN = float("nan")
G = 3
SNRS = [20.0, 5.0]
E2E_SNRS = [30.0, 20.0, 10.0, 0.0]


def golden_clip():
    x, fs = wavio.read_wav(os.path.join(ROOT, "tests", "golden", "wavs", "nmr-data", "FI53_04.wav"))
    assert fs == 16000
    return np.asarray(x, dtype=np.float32).reshape(-1)


def clean_clips():
    return [N.pcm_noise(1500, 81), N.pcm_noise(1700, 82), golden_clip()]


def degraded_rows(clean):
    """Row b G + g: g = 0 the clip itself, then the two SNRs."""
    rows = []
    for x in clean:
        noise = np.random.RandomState(0).randn(x.shape[0])
        rows += [x.copy()] + [N.add_noise(x, noise, snr) for snr in SNRS]
    return rows


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def specs(engine):
    """The device's spectrograms of the clean clips and of their degraded rows, made once: (spec_ref, spec_deg, frames)."""
    clean = clean_clips()
    spec_ref, frames = engine.gammatone([torch.from_numpy(x) for x in clean])
    spec_deg, dframes = engine.gammatone([torch.from_numpy(x) for x in degraded_rows(clean)])
    assert frames == [1, 2, 92] and dframes == [f for f in frames for _ in range(G)]
    torch.cuda.synchronize()
    return spec_ref.clone(), spec_deg.clone(), frames


class Call:
    """One ``nomad_nsim`` call in guarded buffers: outputs NaN-filled, workspace 0xFF."""

    def __init__(self, engine, spec_ref, spec_deg, frames, g=G):
        self.engine, self.frames, self.G = engine, [int(f) for f in frames], g
        self.B = len(frames)
        dev = engine.device
        self.guards = gd = guard.Guards()
        self.ref = gd.empty(tuple(spec_ref.shape), dtype=torch.float64, device=dev, name="spec_ref")
        self.ref.copy_(spec_ref)
        self.deg = gd.empty(tuple(spec_deg.shape), dtype=torch.float64, device=dev, name="spec_deg")
        self.deg.copy_(spec_deg)
        self.nsim = gd.empty((self.B, g), dtype=torch.float64, device=dev, name="nsim")
        self.nsim.fill_(NAN)
        self.bands = gd.empty((self.B, g, 21), dtype=torch.float64, device=dev, name="bands")
        self.bands.fill_(NAN)
        need = int(engine.lib.nomad_nsim_scratch_bytes(self.B, g, sum(self.frames)))
        self.ws = gd.empty_bytes(max(need, 256), dev, 1 << 16, "workspace")
        self.ws.fill_(0xFF)
        self.ws_bytes = need

    def run(self, bands=True, **over):
        a = dict(ref=self.ref.data_ptr(), deg=self.deg.data_ptr(), B=self.B, G=self.G, frames=self.frames, L=1.0, nsim=self.nsim.data_ptr(),
                 bands=self.bands.data_ptr() if bands else None, ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(over)
        rc = self.engine.lib.nomad_nsim(self.engine.ctx, a["ref"], a["deg"], a["B"], a["G"], (C.c_int * len(a["frames"]))(*a["frames"]), a["L"],
                                        a["nsim"], a["bands"], a["ws"], a["ws_bytes"], self.engine._stream())
        torch.cuda.synchronize()
        return rc

    def results(self):
        self.guards.check()
        return self.nsim.cpu().numpy(), self.bands.cpu().numpy()


def _pairs(spec_ref, spec_deg, frames, g=G):
    """(b, g, R, D) of every degraded row, from the packed spectrograms read back."""
    R, D = spec_ref.cpu().numpy(), spec_deg.cpu().numpy()
    at = np.concatenate([[0], np.cumsum(frames)])
    for b, F in enumerate(frames):
        for k in range(g):
            lo = g * at[b] + k * F
            yield b, k, R[at[b]:at[b + 1]], D[lo:lo + F]


def test_scores_and_band_values_are_held_to_the_restatements_map(engine, specs):
    spec_ref, spec_deg, frames = specs
    call = Call(engine, spec_ref, spec_deg, frames)
    assert call.run() == 0, engine.lib.nomad_last_error()
    score, bands = call.results()
    worst = [0.0, 0.0]
    for b, k, R, D in _pairs(spec_ref, spec_deg, frames):
        want, want_bands, _ = N.nsim_map(R, D)
        worst = [max(worst[0], abs(score[b, k] - want)), max(worst[1], float(np.abs(bands[b, k] - want_bands).max()))]
        print(f"clip {b} (F={frames[b]}) row {k}: NSIM {score[b, k]!r}, restatement {float(want)!r}")
        assert abs(score[b, k] - want) <= MAP_BOUND, (b, k, score[b, k], want)
        assert np.abs(bands[b, k] - want_bands).max() <= MAP_BOUND, (b, k)
        if k == 0:
            assert abs(score[b, k] - 1.0) <= MAP_BOUND and np.abs(bands[b, k] - 1.0).max() <= MAP_BOUND, "a row equal to its clean clip gives 1"
    print(f"largest distance from the restatement's map: NSIM {worst[0]:.3g}, band value {worst[1]:.3g} (bound {MAP_BOUND:g})")
    assert (score[:, 0] > score[:, 1]).all() and (score[:, 1] > score[:, 2]).all(), score
    # without the band values the scores keep their bits; run to run
    plain = Call(engine, spec_ref, spec_deg, frames)
    assert plain.run(bands=False) == 0
    score2, bands2 = plain.results()
    assert np.array_equal(_bits(score2), _bits(score)) and np.isnan(bands2).all()
    # another intensity range changes C1 and C3 and with them the score
    other = Call(engine, spec_ref, spec_deg, frames)
    assert other.run(L=45.0) == 0
    score3, _ = other.results()
    for b, k, R, D in _pairs(spec_ref, spec_deg, frames):
        assert abs(score3[b, k] - N.nsim_map(R, D, 45.0)[0]) <= MAP_BOUND
    assert not np.array_equal(score3[:, 1:], score[:, 1:])


def test_a_row_has_the_bytes_of_its_own_call(engine, specs):
    spec_ref, spec_deg, frames = specs
    call = Call(engine, spec_ref, spec_deg, frames)
    assert call.run() == 0
    score, bands = call.results()
    for b, k, R, D in _pairs(spec_ref, spec_deg, frames):
        one = Call(engine, torch.from_numpy(R.copy()), torch.from_numpy(D.copy()), [frames[b]], g=1)
        assert one.run() == 0
        s1, b1 = one.results()
        assert np.array_equal(_bits(s1[0, 0]), _bits(score[b, k])) and np.array_equal(_bits(b1[0, 0]), _bits(bands[b, k])), (b, k)


def test_a_silent_pair_gives_exactly_one(engine):
    zeros = torch.zeros(3, 21, dtype=torch.float64)
    call = Call(engine, zeros, zeros, [3], g=1)
    assert call.run() == 0
    score, bands = call.results()
    assert score[0, 0] == 1.0 and (bands == 1.0).all()
    spec, frames = engine.gammatone([torch.zeros(1920)])
    assert frames == [3] and not spec.cpu().numpy().any()


def test_a_nan_frame_voids_its_row_and_no_other(engine, specs):
    spec_ref, spec_deg, frames = specs
    clean = Call(engine, spec_ref, spec_deg, frames)
    assert clean.run() == 0
    score0, bands0 = clean.results()
    bad = spec_deg.clone()
    at = G * (frames[0] + frames[1]) + 1 * frames[2] + 40      # clip 2, row 1, frame 40
    bad[at, 7] = NAN
    call = Call(engine, spec_ref, bad, frames)
    assert call.run() == 0
    score, bands = call.results()
    assert np.isnan(score[2, 1]) and np.isnan(bands[2, 1]).all()
    keep = np.ones((3, G), dtype=bool)
    keep[2, 1] = False
    assert np.array_equal(_bits(score[keep]), _bits(score0[keep])) and np.array_equal(_bits(bands[keep]), _bits(bands0[keep]))
    # a NaN in the clean spectrogram voids the clip's G rows and no other clip's
    bad_ref = spec_ref.clone()
    bad_ref[frames[0], 0] = NAN                                  # clip 1, frame 0
    call = Call(engine, bad_ref, spec_deg, frames)
    assert call.run() == 0
    score, bands = call.results()
    assert np.isnan(score[1]).all() and np.isnan(bands[1]).all()
    assert np.array_equal(_bits(score[[0, 2]]), _bits(score0[[0, 2]])) and np.array_equal(_bits(bands[[0, 2]]), _bits(bands0[[0, 2]]))


def test_argument_errors_return_before_anything_is_queued(engine, specs):
    spec_ref, spec_deg, frames = specs
    lib = engine.lib

    def refused(status, what, **over):
        call = Call(engine, spec_ref, spec_deg, frames)
        rc = call.run(**over)
        assert rc == status, (what, rc)
        assert lib.nomad_last_error(), what
        call.guards.check(what)
        assert bool(torch.isnan(call.nsim).all()) and bool(torch.isnan(call.bands).all()), f"{what}: the outputs were written"
        assert bool((call.ws == 0xFF).all()), f"{what}: the workspace was written"

    inv = _lib.NOMAD_ERR_INVALID
    refused(inv, "NULL spec_ref_dev", ref=None)
    refused(inv, "NULL spec_deg_dev", deg=None)
    refused(inv, "NULL nsim_out_dev", nsim=None)
    refused(inv, "NULL workspace", ws=None)
    refused(inv, "B = 0", B=0)
    refused(inv, "B = 65536", B=65536)
    refused(inv, "G = 0", G=0)
    refused(inv, "G = 65", G=65)
    refused(inv, "a frame count of 0", frames=[1, 0, 92])
    refused(inv, "an intensity range of 0", L=0.0)
    refused(inv, "a negative intensity range", L=-1.0)
    refused(inv, "a NaN intensity range", L=NAN)
    refused(inv, "an infinite intensity range", L=float("inf"))
    refused(_lib.NOMAD_ERR_WORKSPACE, "ws_bytes - 1", ws_bytes=Call(engine, spec_ref, spec_deg, frames).ws_bytes - 1)
    assert lib.nomad_nsim_scratch_bytes(0, 3, 95) == 0 and lib.nomad_nsim_scratch_bytes(3, 0, 95) == 0
    assert lib.nomad_nsim_scratch_bytes(3, 65, 95) == 0 and lib.nomad_nsim_scratch_bytes(3, 3, 2) == 0
    assert lib.nomad_nsim_scratch_bytes(3, 3, 95) >= 3 * 3 * 95 * 21 * 8
    from nomad_amd._lib import NomadHipError
    with pytest.raises(NomadHipError, match="nomad_nsim_scratch_bytes"):
        engine._scratch_size(lib.nomad_nsim_scratch_bytes, "nomad_nsim_scratch_bytes", 3, 65, 95)


def test_nomad_nsim_end_to_end_falls_with_the_noise_and_agrees_with_the_restatement(engine):
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    x = golden_clip()
    clean = torch.from_numpy(x)[None, :]
    noise = torch.from_numpy(np.random.RandomState(0).randn(x.shape[0]).astype(np.float32))
    rows, lens = nomad.degrade(clean, "noise", E2E_SNRS, noise=noise)
    with guard.guarded(case="Nomad.nsim"):
        score, bands = nomad.nsim((rows, lens), clean, bands=True)
    assert score.shape == (1, 4) and score.dtype == torch.float64 and bands.shape == (1, 4, 21)
    got = score.cpu().numpy()[0]
    assert (np.diff(got) < 0).all() and got[0] < 1.0, got
    host = rows.cpu().numpy()
    worst = 0.0
    for g, snr in enumerate(E2E_SNRS):
        want, want_bands = N.nsim(x, host[g, :lens[g]])
        worst = max(worst, abs(got[g] - want), float(np.abs(bands.cpu().numpy()[0, g] - want_bands).max()))
        print(f"{snr} dB: NSIM {got[g]!r}, restatement {want!r}")
        assert abs(got[g] - want) <= E2E_BOUND and np.abs(bands.cpu().numpy()[0, g] - want_bands).max() <= E2E_BOUND, (snr, got[g], want)
    print(f"largest distance from the restatement end to end: {worst:.3g} (bound {E2E_BOUND:g})")
    # a tensor of clean's shape is G = 1; the clip with itself is 1
    same = nomad.nsim(clean, clean).cpu().numpy()
    assert same.shape == (1, 1) and abs(same[0, 0] - 1.0) <= MAP_BOUND
    one = nomad.nsim(rows[1:2, :x.shape[0]], clean).cpu().numpy()
    assert np.array_equal(_bits(one[0, 0]), _bits(got[1])), "the row on its own has its bits"
    with pytest.raises(ValueError, match="G rows per clean clip"):
        nomad.nsim((rows[:3], lens[:3]), torch.cat([clean, clean]))


def test_sweep_with_nsim_scores_the_same_rows_and_adds_their_nsim(engine):
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    lens = [8000, 7001]
    clean = torch.zeros(2, 8000)
    for b, n in enumerate(lens):
        clean[b, :n] = torch.from_numpy(N.pcm_noise(n, 90 + b, 0.1 * (b + 1)))
    gen = torch.Generator().manual_seed(5)
    refs = torch.randn(5, 256, generator=gen, dtype=torch.float64)
    refs = (refs / refs.norm(dim=1, keepdim=True)).float()
    cf = [5.0, 40.0]
    plain = nomad.intensity_sweep(clean, refs, clip_factor=cf, lengths=lens)["CLIP"]
    assert "nsim" not in plain
    with guard.guarded(case="intensity_sweep(nsim=True)"):
        res = nomad.intensity_sweep(clean, refs, clip_factor=cf, lengths=lens, nsim=True)["CLIP"]
    assert np.array_equal(_bits(res["scores"]), _bits(plain["scores"])), "the scores are those of the sweep without it"
    rows, lens_rep = nomad.degrade(clean, "clip", cf, lengths=lens)
    want = nomad.nsim((rows, lens_rep), clean, lengths=lens).cpu().numpy().reshape(-1)
    assert res["nsim"].shape == (4,) and np.array_equal(_bits(res["nsim"]), _bits(want)) and res["conditions"].tolist() == cf * 2
    assert (want[0::2] > want[1::2]).all(), want
