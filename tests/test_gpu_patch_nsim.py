"""GPU: ``nomad_nsim_patches`` through the C ABI in guarded buffers (outputs NaN-filled, workspace 0xFF) on the device's OWN
spectrograms, against ``nomad_nsim`` on the cut-outs (bits), against the restatement's selection run on the device's own candidate
table (bits), and end to end against ``patch_nsim_ref`` from the waveforms.

The batch: B = 3 clean clips of F = 1, 8 and 92 frames at patch 8 / search 6 - PCM noise of 1500 and 3800 samples (3840 samples,
as first written down, make 9 frames; the case is about ONE patch whose window is clamped at both ends, so the clip has the 8
frames) and tests/golden/wavs/nmr-data/FI53_04.wav - with G = 3 rows each: the clip itself, its jump copy (late by 2 frames in its
first half and by 5 in its second, Fd = F + 5) and a row SHORTER than the clip (1280, 2560 and 20000 samples: 1, 5 and 59 frames;
5 < patch, so that row has no candidate).  So one call holds a clip without a patch, one patch with the window clamped at both
ends, a row with no candidate, a clamped ``hi``, and 168 cells / 13 candidates, neither a multiple of a wave or of four waves.

Bounds.  Candidates, band values and the selection are EQUALITIES (the same inputs and the same order of float64 additions).  End to
end (``Nomad.nsim_patches`` against ``patch_nsim_ref`` from the waveforms, whose spectrogram is long double where the device's is
float64) the bound is derived as tests/test_gpu_nsim.py derives its E2E_BOUND: the float64 chain (spectrogram, candidates,
selection) against the same chain in long double on the three rows of the end-to-end case, on the CPU: largest distance 7.8e-16 for
a score, 1.2e-14 for a band value; E2E_BOUND = 20 x the larger = 2.4e-13.  The offsets may be demanded equal because the chosen
chain beats every chain that differs in one patch by 0.106 on the noisy row (tests/test_patch_nsim_host.py guards that margin).
MEASURED on an MI355X: 6.7e-16 for a score and 1.1e-14 for a band value end to end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import guard
import nsim_ref as N
import patch_nsim_ref as PR
from conftest import ROOT
from nomad_amd import _lib, wavio

pytestmark = pytest.mark.gpu

E2E_BOUND = 2.4e-13
NAN = float("nan")
G = 3
PATCH, SEARCH, RATIO, NEED = 8, 6, 1e-4, 8
PLACES = 2 * SEARCH + 1
H = 320


def golden_clip():
    x, fs = wavio.read_wav(os.path.join(ROOT, "tests", "golden", "wavs", "nmr-data", "FI53_04.wav"))
    assert fs == 16000
    return np.asarray(x, dtype=np.float32).reshape(-1)


def clean_clips():
    return [N.pcm_noise(1500, 81), N.pcm_noise(3800, 82), golden_clip()]


def degraded_rows(clean):
    """Row b G + g: g = 0 the clip itself, 1 its jump copy, 2 a shorter row."""
    rows = []
    for x, short in zip(clean, (1280, 2560, 20000)):
        rows += [x.copy(), PR.jump_copy(x), x[:short].copy()]
    return rows


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def specs(engine):
    """The device's spectrograms of the clean clips and of their rows, made once: (spec_ref, spec_deg, frames, deg_frames)."""
    clean = clean_clips()
    spec_ref, frames = engine.gammatone([torch.from_numpy(x) for x in clean])
    spec_deg, dframes = engine.gammatone([torch.from_numpy(x) for x in degraded_rows(clean)])
    assert frames == [1, 8, 92] and dframes == [1, 6, 1, 8, 13, 5, 92, 97, 59]
    torch.cuda.synchronize()
    return spec_ref.clone(), spec_deg.clone(), frames, dframes


class Call:
    """One ``nomad_nsim_patches`` call in guarded buffers: outputs NaN-filled (offsets -77), workspace 0xFF."""

    def __init__(self, engine, spec_ref, spec_deg, frames, dframes, g=G, patch=PATCH, search=SEARCH):
        self.engine, self.frames, self.dframes, self.G = engine, [int(f) for f in frames], [int(f) for f in dframes], g
        self.B, self.patch, self.search = len(frames), patch, search
        self.P = max(1, max(self.frames) // patch)
        dev = engine.device
        self.guards = gd = guard.Guards()
        self.ref = gd.empty(tuple(spec_ref.shape), dtype=torch.float64, device=dev, name="spec_ref")
        self.ref.copy_(spec_ref)
        self.deg = gd.empty(tuple(spec_deg.shape), dtype=torch.float64, device=dev, name="spec_deg")
        self.deg.copy_(spec_deg)
        self.nsim = gd.empty((self.B, g), dtype=torch.float64, device=dev, name="nsim")
        self.bands = gd.empty((self.B, g, 21), dtype=torch.float64, device=dev, name="bands")
        self.offsets = gd.empty((self.B, g, self.P), dtype=torch.int32, device=dev, name="offsets")
        self.patch_nsim = gd.empty((self.B, g, self.P), dtype=torch.float64, device=dev, name="patch_nsim")
        self.cand = gd.empty((self.B, g, self.P, 2 * search + 1), dtype=torch.float64, device=dev, name="cand")
        for t in (self.nsim, self.bands, self.patch_nsim, self.cand):
            t.fill_(NAN)
        self.offsets.fill_(-77)
        need = int(engine.lib.nomad_nsim_patches_scratch_bytes(self.B, g, sum(self.frames), sum(self.dframes), patch, search))
        self.ws = gd.empty_bytes(max(need, 256), dev, 1 << 16, "workspace")
        self.ws.fill_(0xFF)
        self.ws_bytes = need

    def run(self, bands=True, offsets=True, patch_nsim=True, cand=True, **over):
        a = dict(ref=self.ref.data_ptr(), deg=self.deg.data_ptr(), B=self.B, G=self.G, frames=self.frames, dframes=self.dframes,
                 patch=self.patch, search=self.search, ratio=RATIO, need=min(NEED, self.patch), L=1.0, P=self.P, nsim=self.nsim.data_ptr(),
                 bands=self.bands.data_ptr() if bands else None, offsets=self.offsets.data_ptr() if offsets else None,
                 patch_nsim=self.patch_nsim.data_ptr() if patch_nsim else None, cand=self.cand.data_ptr() if cand else None,
                 ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(over)
        rc = self.engine.lib.nomad_nsim_patches(self.engine.ctx, a["ref"], a["deg"], a["B"], a["G"], (C.c_int * len(a["frames"]))(*a["frames"]),
                                                (C.c_int * len(a["dframes"]))(*a["dframes"]), a["patch"], a["search"], a["ratio"], a["need"],
                                                a["L"], a["P"], a["nsim"], a["bands"], a["offsets"], a["patch_nsim"], a["cand"], a["ws"],
                                                a["ws_bytes"], self.engine._stream())
        torch.cuda.synchronize()
        return rc

    def results(self):
        self.guards.check()
        return {k: getattr(self, k).cpu().numpy() for k in ("nsim", "bands", "offsets", "patch_nsim", "cand")}

    def untouched(self):
        return (all(bool(torch.isnan(t).all()) for t in (self.nsim, self.bands, self.patch_nsim, self.cand))
                and bool((self.offsets == -77).all()) and bool((self.ws == 0xFF).all()))


def _rows(spec_ref, spec_deg, frames, dframes, g=G):
    """(b, k, R, D) of every degraded row, from the packed spectrograms read back."""
    R, D = spec_ref.cpu().numpy(), spec_deg.cpu().numpy()
    at, dat = np.concatenate([[0], np.cumsum(frames)]), np.concatenate([[0], np.cumsum(dframes)])
    for b in range(len(frames)):
        for k in range(g):
            r = b * g + k
            yield b, k, R[at[b]:at[b + 1]], D[dat[r]:dat[r + 1]]


@pytest.fixture(scope="module")
def batch(engine, specs):
    """The batch's call, and ``nomad_nsim`` on the cut-out pair of every finite candidate as ONE call (B = the candidates, G = 1,
    frames = patch): (results, {(b, k, p, c): (nsim, bands [21])})."""
    spec_ref, spec_deg, frames, dframes = specs
    call = Call(engine, spec_ref, spec_deg, frames, dframes)
    assert call.run() == 0, engine.lib.nomad_last_error()
    res = call.results()
    cuts_r, cuts_d, where = [], [], []
    for b, k, R, D in _rows(*specs):
        for p in range(frames[b] // PATCH):
            for c in range(PLACES):
                if np.isfinite(res["cand"][b, k, p, c]):
                    u = p * PATCH - SEARCH + c
                    assert 0 <= u and u + PATCH <= D.shape[0], "a candidate outside the row"
                    cuts_r.append(R[p * PATCH:(p + 1) * PATCH])
                    cuts_d.append(D[u:u + PATCH])
                    where.append((b, k, p, c))
    n = len(where)
    assert 1 <= n <= 65535
    score, bands = engine.nsim_of_spectrograms(torch.from_numpy(np.concatenate(cuts_r)).to(engine.device),
                                               torch.from_numpy(np.concatenate(cuts_d)).to(engine.device), [PATCH] * n, 1)
    score, bands = score.cpu().numpy().reshape(-1), bands.cpu().numpy().reshape(n, 21)
    return res, {w: (score[i], bands[i]) for i, w in enumerate(where)}


def _cand_bands(cuts, b, k, P):
    out = np.full((P, PLACES, 21), np.nan)
    for (bb, kk, p, c), (_, bands) in cuts.items():
        if (bb, kk) == (b, k):
            out[p, c] = bands
    return out


def test_every_candidate_has_the_bits_of_nomad_nsim_on_the_cut_out_pair(specs, batch):
    """Case 1: and the finite entries are exactly the kept patches' windows."""
    res, cuts = batch
    frames = specs[2]
    for b, k, R, D in _rows(*specs):
        P = frames[b] // PATCH
        kept = PR.kept_table(R, D.shape[0], PATCH, SEARCH, RATIO, NEED)
        for p in range(res["cand"].shape[2]):
            lo, hi = PR.window(p, PATCH, SEARCH, D.shape[0]) if p < P and kept[p] else (1, 0)
            want = np.zeros(PLACES, dtype=bool)
            want[max(lo - (p * PATCH - SEARCH), 0):max(hi - (p * PATCH - SEARCH) + 1, 0)] = lo <= hi
            assert np.array_equal(np.isfinite(res["cand"][b, k, p]), want), (b, k, p)
    assert len(cuts) > 250
    for (b, k, p, c), (score, _) in cuts.items():
        assert _same(res["cand"][b, k, p, c], score), (b, k, p, c, res["cand"][b, k, p, c], score)
    # the chosen candidates' band values, added in ascending patch order, are the row's band values
    for b, k, R, D in _rows(*specs):
        on = [p for p in range(frames[b] // PATCH) if res["offsets"][b, k, p] >= 0]
        if on:
            acc = np.zeros(21)
            for p in on:
                acc = acc + cuts[(b, k, p, res["offsets"][b, k, p] - (p * PATCH - SEARCH))][1]
            assert _same(res["bands"][b, k], acc / np.float64(len(on))), (b, k)


def test_activity_and_the_kept_table_are_the_restatements(engine, specs, batch):
    """Case 2: on the device's own spectrogram read back.  The kept table shows in which patches have candidates; the activity
    flags themselves show at patch 1 / search 0 against the clip itself, where a patch is one frame and kept iff it is active."""
    res, _ = batch
    spec_ref, spec_deg, frames, dframes = specs
    for b, k, R, D in _rows(*specs):
        P = frames[b] // PATCH
        kept = PR.kept_table(R, D.shape[0], PATCH, SEARCH, RATIO, NEED)
        assert np.array_equal(np.isfinite(res["cand"][b, k, :P]).any(axis=1), kept), (b, k)
        assert np.array_equal(res["offsets"][b, k, :P] >= 0, kept) and (res["offsets"][b, k, P:] == -1).all(), (b, k)
    assert list(np.nonzero(res["offsets"][2, 1] >= 0)[0]) == [0, 2, 3, 4, 5, 6, 7, 8, 10]
    call = Call(engine, spec_ref, spec_ref, frames, frames, g=1, patch=1, search=0)
    assert call.run() == 0, engine.lib.nomad_last_error()
    flags = call.results()["offsets"]
    for b, k, R, _ in _rows(spec_ref, spec_ref, frames, frames, g=1):
        act = PR.activity(R, RATIO)
        assert np.array_equal(flags[b, 0, :frames[b]] >= 0, act), b
    assert int(PR.activity(spec_ref.cpu().numpy()[9:], RATIO).sum()) == 87


def test_the_selection_has_the_bits_of_the_restatement_on_the_devices_own_candidates(specs, batch):
    """Case 3."""
    res, cuts = batch
    frames = specs[2]
    for b, k, R, D in _rows(*specs):
        P = frames[b] // PATCH
        kept = PR.kept_table(R, D.shape[0], PATCH, SEARCH, RATIO, NEED)
        want = PR.results(res["cand"][b, k, :P], _cand_bands(cuts, b, k, P), kept, PATCH, SEARCH, D.shape[0])
        print(f"clip {b} (F={frames[b]}) row {k} (Fd={D.shape[0]}): NSIM {res['nsim'][b, k]!r}, kept {want['kept']}, offsets {want['offsets']}")
        assert np.array_equal(res["offsets"][b, k, :P], want["offsets"]), (b, k)
        assert _same(res["nsim"][b, k], want["nsim"]) and _same(res["patch_nsim"][b, k, :P], want["patch_nsim"]), (b, k)
        assert _same(res["bands"][b, k], want["bands"]), (b, k)
        assert np.isnan(res["patch_nsim"][b, k, P:]).all()
    assert np.isnan(res["nsim"][0]).all() and np.isnan(res["nsim"][1, 2]), "no patch, no candidate: NaN"
    assert res["nsim"][1, 0] == 1.0 and res["offsets"][1, 0, 0] == 0
    on = res["offsets"][2, 1] >= 0
    assert list((res["offsets"][2, 1] - np.arange(11) * PATCH)[on]) == [2, 2, 2, 2, 2, 5, 5, 5, 5], "the jump row's delays"
    assert list((res["offsets"][2, 0] - np.arange(11) * PATCH)[on]) == [0] * 9 and res["nsim"][2, 0] == 1.0


def test_nomad_nsim_patches_end_to_end_agrees_with_the_restatement(engine):
    """Case 4."""
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    x = golden_clip()
    y = PR.jump_copy(x)
    rows = [x, y, N.add_noise(y, np.random.RandomState(0).randn(y.shape[0]), 20.0)]
    deg = torch.zeros(3, max(r.shape[0] for r in rows))
    for i, r in enumerate(rows):
        deg[i, :r.shape[0]] = torch.from_numpy(r)
    with guard.guarded(case="Nomad.nsim_patches"):
        res = nomad.nsim_patches(deg, torch.from_numpy(x)[None, :], degraded_lengths=[r.shape[0] for r in rows], patch_s=0.16, search_s=0.12)
    assert res["nsim"].shape == (1, 3) and res["bands"].shape == (1, 3, 21) and res["offsets"].shape == (1, 3, 11)
    assert res["offsets"].dtype == torch.int32 and res["kept"].cpu().tolist() == [[9, 9, 9]] and "delay" not in res
    worst = [0.0, 0.0]
    for g, row in enumerate(rows):
        want = PR.nsim_patches(x, row, patch_s=0.16, search_s=0.12, dtype=np.longdouble)
        got, got_bands = res["nsim"][0, g].item(), res["bands"][0, g].cpu().numpy()
        worst = [max(worst[0], abs(got - want["nsim"])), max(worst[1], float(np.abs(got_bands - want["bands"]).max()))]
        print(f"row {g}: NSIM {got!r}, restatement {float(want['nsim'])!r}")
        assert np.array_equal(res["offsets"][0, g].cpu().numpy(), want["offsets"]), g
        assert abs(got - want["nsim"]) <= E2E_BOUND and np.abs(got_bands - want["bands"]).max() <= E2E_BOUND, (g, got, want["nsim"])
        assert np.abs(res["patch_nsim"][0, g].cpu().numpy()[want["offsets"] >= 0] - want["patch_nsim"][want["offsets"] >= 0]).max() <= E2E_BOUND
    print(f"largest distance from the restatement end to end: NSIM {worst[0]:.3g}, band value {worst[1]:.3g} (bound {E2E_BOUND:g})")
    # global alignment first, then the patch search: the jump row's first half is then in place and its second late by 3 frames
    aligned = nomad.nsim_patches(deg[1:2], torch.from_numpy(x)[None, :], degraded_lengths=[y.shape[0]], patch_s=0.16, search_s=0.12,
                                 max_delay_s=0.2)
    off = aligned["offsets"][0, 0].cpu().numpy()
    rel = (off - np.arange(11) * PATCH)[off >= 0]
    d = int(aligned["delay"][0, 0])
    assert d in (2 * H, 5 * H) and (list(rel) == [0] * 5 + [3] * 4 if d == 2 * H else list(rel[-4:]) == [0] * 4), (d, rel)


def test_a_row_has_the_bytes_of_its_own_call_and_optional_outputs_change_nothing(engine, specs, batch):
    """Case 5."""
    res, _ = batch
    spec_ref, spec_deg, frames, dframes = specs
    for b, k, R, D in _rows(*specs):
        one = Call(engine, torch.from_numpy(R.copy()), torch.from_numpy(D.copy()), [frames[b]], [D.shape[0]], g=1)
        assert one.run() == 0
        r1 = one.results()
        P = one.P
        assert _same(r1["nsim"][0, 0], res["nsim"][b, k]) and _same(r1["bands"][0, 0], res["bands"][b, k]), (b, k)
        assert np.array_equal(r1["offsets"][0, 0], res["offsets"][b, k, :P]) and _same(r1["patch_nsim"][0, 0], res["patch_nsim"][b, k, :P])
        assert _same(r1["cand"][0, 0], res["cand"][b, k, :P]), (b, k)
    for off in ("bands", "offsets", "patch_nsim", "cand"):
        call = Call(engine, spec_ref, spec_deg, frames, dframes)
        assert call.run(**{off: False}) == 0
        r2 = call.results()
        for key in ("nsim", "bands", "patch_nsim", "cand"):
            if key == off:
                assert np.isnan(r2[key]).all(), key
            else:
                assert _same(r2[key], res[key]), (off, key)
        assert (r2["offsets"] == -77).all() if off == "offsets" else np.array_equal(r2["offsets"], res["offsets"])
    bare = Call(engine, spec_ref, spec_deg, frames, dframes)
    assert bare.run(bands=False, offsets=False, patch_nsim=False, cand=False) == 0
    assert _same(bare.results()["nsim"], res["nsim"])


def test_search_zero_is_nomad_nsim_of_the_cut_outs_at_zero_offset(engine, specs):
    """Case 6: an aligned row of equal length."""
    spec_ref, spec_deg, frames, dframes = specs
    R = spec_ref.cpu().numpy()[9:]
    x = golden_clip()
    noisy = N.add_noise(x, np.random.RandomState(0).randn(x.shape[0]), 20.0)
    spec, f = engine.gammatone([torch.from_numpy(noisy)])
    assert f == [92]
    call = Call(engine, torch.from_numpy(R.copy()), spec, [92], [92], g=1, search=0)
    assert call.run() == 0
    res = call.results()
    kept = PR.kept_table(R, 92, PATCH, 0, RATIO, NEED)
    on = [p for p in range(11) if kept[p]]
    assert on == [0, 2, 3, 4, 5, 6, 7, 8, 10] and list(res["offsets"][0, 0][on]) == [p * PATCH for p in on]
    D = spec.cpu().numpy()
    cut_r = np.concatenate([R[p * PATCH:(p + 1) * PATCH] for p in on])
    cut_d = np.concatenate([D[p * PATCH:(p + 1) * PATCH] for p in on])
    score, _ = engine.nsim_of_spectrograms(torch.from_numpy(cut_r).to(engine.device), torch.from_numpy(cut_d).to(engine.device), [PATCH] * len(on), 1)
    assert _same(res["patch_nsim"][0, 0][on], score.cpu().numpy().reshape(-1)) and _same(res["cand"][0, 0, on, 0], res["patch_nsim"][0, 0][on])
    assert 0.5 < res["nsim"][0, 0] < 1.0


# ---- the gate ------------------------------------------------------------------------------------------------------------------------
GAP = 40


@pytest.fixture(scope="module")
def gap(engine):
    """The golden clip with 40 frames of zeros inserted at its middle, and two degraded copies at 20 dB: one with noise only in the
    middle 10 frames of the gap besides, one without -> (spec_ref, spec_quiet, spec_noisy, F, first frame of the gap)."""
    x = golden_clip()
    half = (x.shape[0] // 2) // H * H
    clean = np.concatenate([x[:half], np.zeros(GAP * H, np.float32), x[half:]])
    quiet = np.concatenate([N.add_noise(x, np.random.RandomState(0).randn(x.shape[0]), 20.0)[:half], np.zeros(GAP * H, np.float32),
                            N.add_noise(x, np.random.RandomState(0).randn(x.shape[0]), 20.0)[half:]])
    noisy = quiet.copy()
    noisy[half + 15 * H:half + 25 * H] = 0.05 * np.random.RandomState(3).randn(10 * H).astype(np.float32)
    spec, frames = engine.gammatone([torch.from_numpy(v) for v in (clean, quiet, noisy)])
    F = frames[0]
    assert frames == [F] * 3 and F == 92 + GAP
    torch.cuda.synchronize()
    return spec[:F].clone(), spec[F:2 * F].clone(), spec[2 * F:].clone(), F, half // H


def test_the_gate_keeps_silence_out_of_the_score(engine, gap):
    """Case 7: at search 2 the patches in the gap are not kept, the score has the same bits with and without noise in the gap, and
    the whole-clip ``nomad_nsim`` of the two copies differs."""
    spec_ref, quiet, noisy, F, g0 = gap
    out = []
    for deg in (quiet, noisy):
        call = Call(engine, spec_ref, deg, [F], [F], g=1, search=2)
        assert call.run() == 0
        out.append(call.results())
    on = out[0]["offsets"][0, 0] >= 0
    silent = [p for p in range(F // PATCH) if p * PATCH >= g0 and (p + 1) * PATCH <= g0 + GAP - 3]      # frames wholly inside the zeros
    assert len(silent) >= 3 and not on[silent].any(), "a patch of silence was kept"
    assert on.sum() >= 4
    for key in ("nsim", "bands", "patch_nsim", "cand"):
        assert _same(out[0][key], out[1][key]), key
    assert np.array_equal(out[0]["offsets"], out[1]["offsets"])
    whole = [engine.nsim_of_spectrograms(spec_ref, deg, [F], 1)[0].item() for deg in (quiet, noisy)]
    print(f"patch-wise {out[0]['nsim'][0, 0]!r} with and without the noise; whole-clip {whole[0]!r} without, {whole[1]!r} with")
    assert whole[0] != whole[1]


def test_a_nan_voids_its_row_and_no_other(engine, specs, batch, gap):
    """Case 8."""
    res, _ = batch
    spec_ref, spec_deg, frames, dframes = specs
    dat = np.concatenate([[0], np.cumsum(dframes)])
    bad = spec_deg.clone()
    bad[dat[7] + 40, 7] = NAN                                     # clip 2, row 1 (the jump copy), frame 40: inside kept windows
    call = Call(engine, spec_ref, bad, frames, dframes)
    assert call.run() == 0
    got = call.results()
    assert np.isnan(got["nsim"][2, 1]) and np.isnan(got["bands"][2, 1]).all() and np.isnan(got["patch_nsim"][2, 1]).all()
    assert (got["offsets"][2, 1] == -1).all()
    keep = np.ones((3, G), dtype=bool)
    keep[2, 1] = False
    for key in ("nsim", "bands", "patch_nsim", "cand"):
        assert _same(got[key][keep], res[key][keep]), key
    assert np.array_equal(got["offsets"][keep], res["offsets"][keep])
    # a NaN in the clean spectrogram voids the clip's G rows and no other clip's
    bad_ref = spec_ref.clone()
    bad_ref[1 + 3, 0] = NAN                                        # clip 1, frame 3
    call = Call(engine, bad_ref, spec_deg, frames, dframes)
    assert call.run() == 0
    got = call.results()
    assert np.isnan(got["nsim"][1]).all() and np.isnan(got["bands"][1]).all() and (got["offsets"][1] == -1).all()
    for key in ("nsim", "bands", "patch_nsim"):
        assert _same(got[key][[0, 2]], res[key][[0, 2]]), key
    assert np.array_equal(got["offsets"][[0, 2]], res["offsets"][[0, 2]])
    # a NaN in the gap, outside every window, is not seen
    g_ref, quiet, _, F, g0 = gap
    plain = Call(engine, g_ref, quiet, [F], [F], g=1, search=2)
    assert plain.run() == 0
    holed = quiet.clone()
    holed[g0 + 18, 3] = NAN
    call = Call(engine, g_ref, holed, [F], [F], g=1, search=2)
    assert call.run() == 0
    a, b = plain.results(), call.results()
    assert np.isfinite(b["nsim"][0, 0])
    for key in ("nsim", "bands", "patch_nsim", "cand"):
        assert _same(a[key], b[key]), key


def test_a_silent_pair_gives_exactly_one(engine):
    """Case 9: a silent clip is active everywhere."""
    zeros = torch.zeros(19, 21, dtype=torch.float64)
    call = Call(engine, zeros, zeros, [19], [19], g=1)
    assert call.run() == 0
    res = call.results()
    assert res["nsim"][0, 0] == 1.0 and (res["bands"] == 1.0).all() and list(res["offsets"][0, 0]) == [0, 8]
    assert (res["patch_nsim"][0, 0] == 1.0).all()


def test_argument_errors_return_before_anything_is_queued(engine, specs):
    """Case 10."""
    spec_ref, spec_deg, frames, dframes = specs
    lib = engine.lib

    def refused(status, what, **over):
        call = Call(engine, spec_ref, spec_deg, frames, dframes)
        rc = call.run(**over)
        assert rc == status, (what, rc)
        assert lib.nomad_last_error(), what
        call.guards.check(what)
        assert call.untouched(), f"{what}: an output or the workspace was written"

    inv = _lib.NOMAD_ERR_INVALID
    refused(inv, "NULL spec_ref_dev", ref=None)
    refused(inv, "NULL spec_deg_dev", deg=None)
    refused(inv, "NULL nsim_out_dev", nsim=None)
    refused(inv, "NULL workspace", ws=None)
    refused(inv, "B = 0", B=0)
    refused(inv, "B = 65536", B=65536)
    refused(inv, "G = 0", G=0)
    refused(inv, "G = 65", G=65)
    refused(inv, "patch = 0", patch=0)
    refused(inv, "patch = 65", patch=65)
    refused(inv, "search = -1", search=-1)
    refused(inv, "search = 129", search=129)
    refused(inv, "vad_ratio = 0", ratio=0.0)
    refused(inv, "vad_ratio above 1", ratio=1.5)
    refused(inv, "a NaN vad_ratio", ratio=NAN)
    refused(inv, "min_active_frames = 0", need=0)
    refused(inv, "min_active_frames above patch", need=PATCH + 1)
    refused(inv, "an intensity range of 0", L=0.0)
    refused(inv, "a NaN intensity range", L=NAN)
    refused(inv, "an infinite intensity range", L=float("inf"))
    refused(inv, "a clean frame count of 0", frames=[1, 0, 92])
    refused(inv, "a degraded frame count of 0", dframes=[1, 6, 1, 8, 13, 0, 92, 97, 59])
    refused(inv, "out_patches = 0", P=0)
    refused(inv, "out_patches below a clip's patches", P=10)
    refused(_lib.NOMAD_ERR_WORKSPACE, "ws_bytes - 1", ws_bytes=Call(engine, spec_ref, spec_deg, frames, dframes).ws_bytes - 1)
    size = lib.nomad_nsim_patches_scratch_bytes
    assert size(0, 3, 101, 282, 8, 6) == 0 and size(3, 0, 101, 282, 8, 6) == 0 and size(3, 65, 101, 282, 8, 6) == 0
    assert size(3, 3, 2, 282, 8, 6) == 0 and size(3, 3, 101, 8, 8, 6) == 0 and size(3, 3, 101, 282, 0, 6) == 0
    assert size(3, 3, 101, 282, 65, 6) == 0 and size(3, 3, 101, 282, 8, -1) == 0 and size(3, 3, 101, 282, 8, 129) == 0
    assert size(3, 3, 101, 282, 8, 6) >= 3 * 12 * 13 * 8
    assert lib.nomad_nsim_patch_count(92, 8) == 11 and lib.nomad_nsim_patch_count(7, 8) == 0 and lib.nomad_nsim_patch_count(92, 0) == 0
    from nomad_amd._lib import NomadHipError
    with pytest.raises(NomadHipError, match="nomad_nsim_patches_scratch_bytes"):
        engine._scratch_size(size, "nomad_nsim_patches_scratch_bytes", 3, 65, 101, 282, 8, 6)


def test_the_host_layers_hand_out_nsim_patches_bits(engine, tmp_path):
    """Case 11: ``Nomad.nsim(patch_s=)``, ``nsim_files(patch_s=)`` on the golden wav folders, ``mine_triplets(patch_s=)``."""
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    x = golden_clip()
    clean = torch.from_numpy(x)[None, :]
    noise = torch.from_numpy(np.random.RandomState(0).randn(x.shape[0]).astype(np.float32))
    rows, lens = nomad.degrade(clean, "noise", [20.0, 5.0], noise=noise)
    want = nomad.nsim_patches((rows, lens), clean, patch_s=0.16, search_s=0.12)
    score, bands = nomad.nsim((rows, lens), clean, bands=True, patch_s=0.16, search_s=0.12)
    assert _same(score.cpu().numpy(), want["nsim"].cpu().numpy()) and _same(bands.cpu().numpy(), want["bands"].cpu().numpy())
    assert score.shape == (1, 2) and 1.0 > score[0, 0] > score[0, 1]
    plain = nomad.nsim((rows, lens), clean)
    assert not _same(plain.cpu().numpy(), score.cpu().numpy()), "the whole-clip measure is another number"
    score_d, delay = nomad.nsim((rows, lens), clean, patch_s=0.16, search_s=0.12, max_delay_s=0.05)
    assert delay.cpu().tolist() == [[0, 0]] and _same(score_d.cpu().numpy(), score.cpu().numpy())
    # files: the golden folders, every file against itself and against another file
    folder = os.path.join(ROOT, "tests", "golden", "wavs")
    refs = [os.path.join(folder, "nmr-data", n) for n in ("FI53_04.wav", "MJ60_10.wav")]
    degs = [refs[0], os.path.join(folder, "test-data", "445-123860-0012_NOISE_15.wav")]
    table = nomad.nsim_files(degs, refs, max_delay_s=0.1, patch_s=0.16, search_s=0.12, results_path=str(tmp_path))
    assert list(table.columns) == ["filepath_ref", "filepath_deg", "delay_samples", "delay_s", "NSIM", "patches_kept", "offset_min_frames",
                                   "offset_max_frames"]
    assert table["NSIM"][0] == 1.0 and table["patches_kept"][0] == 9 and table["offset_min_frames"][0] == 0 == table["offset_max_frames"][0]
    for k in range(2):
        c, d = nomad.load_processing(refs[k]), nomad.load_processing(degs[k])
        one = nomad.nsim_patches(d, c, patch_s=0.16, search_s=0.12, max_delay_s=0.1)
        assert _same(table["NSIM"][k], one["nsim"].item()) and table["patches_kept"][k] == int(one["kept"].item()), k
        assert table["delay_samples"][k] == int(one["delay"].item())
    assert "patches_kept" not in nomad.nsim_files(degs[:1], refs[:1], max_delay_s=0.1).columns
    # the mine: two short clips, one of them too short for a patch of 0.4 s
    lens2 = [16000, 6000]
    two = torch.zeros(2, 16000)
    for b, n in enumerate(lens2):
        two[b, :n] = torch.from_numpy(N.pcm_noise(n, 70 + b, 0.1))
    cf = [5.0, 20.0, 40.0]
    A, P, Ng, info = nomad.mine_triplets(two, clip_factor=cf, normalize=None, lengths=lens2, N=1, hard_sampling=True, seed=2, patch_s=0.4)
    assert info["no_patches"] == [1] and np.isnan(info["nsim"][1]).all() and set(info["triplets"]["clip"].tolist()) <= {0}
    rows2, lens_rep = nomad.degrade(two, "clip", cf, lengths=lens2)
    again = nomad.nsim_patches((rows2, lens_rep), two, lengths=lens2, patch_s=0.4, search_s=0.4)
    assert _same(info["nsim"], again["nsim"].cpu().numpy()) and again["kept"].cpu().tolist() == [[2, 2, 2], [0, 0, 0]]
    assert len(A[1]) == len(info["triplets"]["clip"]) and all(n == 16000 for n in A[1])
