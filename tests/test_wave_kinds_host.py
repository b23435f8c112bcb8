"""CPU: the waveforms of tests/wave_kinds.py and the references test_gpu_wave_kinds_f64.py holds the engine to on them.  A GPU failure
there must mean the kernel, so here the reference alone is shown to be usable on these inputs: the kinds are what their rows claim,
the float64 and fp32 oracles stay finite (forward and d loss / d waveform), the head's ReLU kink leaves almost every channel decided,
every triplet hinge of the parameter-gradient cases sits away from its switch point, and the engine's conv0 formulation (float64
one-pass statistics, fp32 scale / shift, fp32 y), restated on the CPU, stays within ``8 e32 + 1e-7 top`` of float64 for every kind -
so the GPU test may demand it of the kernel.  Measured here (err / e32 of the restatement): constant 4.0, the others 0.5 - 1.1."""
import pytest
import torch

import ref64
import wave_kinds as K
from oracle import nomad_oracle as O

MARGIN = 1.0            # test_gpu_wave_kinds_f64.MARGIN
HINGE_CLEAR = 1e-3      # a thousand times the fp32 error of a distance between unit-norm embeddings


@pytest.fixture(scope="module")
def short():
    return K.batch(K.N_SHORT)


def test_kinds_are_deterministic_and_what_their_rows_claim(short, sd0):
    names, wav = short
    assert names == K.NAMES and wav.shape == (11, K.N_SHORT)
    again = K.kinds(K.N_SHORT)
    assert all(torch.equal(wav[i], again[k]) for i, k in enumerate(names))
    assert not torch.equal(K.kinds(K.N_SHORT, K.SEED + 1)["faint"], again["faint"])
    k = again
    assert not k["silence"].any() and bool((k["constant"] == 0.5).all())
    assert k["faint"].abs().max() < 1e-3 and k["faint"].std() > 5e-5
    assert int((k["impulse"] != 0).sum()) == 1 and k["impulse"][K.N_SHORT // 2] == 1.0
    assert set(k["square"].unique().tolist()) <= {-1.0, 0.0, 1.0} and (k["square"].abs() == 1).float().mean() > 0.99
    assert (k["full_scale"].abs() == 1).float().mean() > 0.25
    assert torch.equal(k["int16"] * 32768, torch.round(k["int16"] * 32768)) and not torch.equal(k["int16"], k["half_silent"])
    _, counts = k["hard_clipped"].unique(return_counts=True)
    top2 = counts.sort(descending=True).values[:2]
    assert int(top2.sum()) >= 0.3 * K.N_SHORT and int(top2[1]) >= 0.1 * K.N_SHORT, top2
    assert k["noisy_m20db"].abs().max() > 1.0
    assert not k["half_silent"][K.N_SHORT // 2:].any() and k["half_silent"][:K.N_SHORT // 2].abs().max() > 0.2
    mean, var = K.conv0_stats64(sd0, k["dc_offset"])
    assert (mean * mean / var).max().item() > 1e4
    # the ragged clips: every kind at its own length, the same properties of the degenerate ones
    rnames, clips = K.ragged()
    assert rnames == K.NAMES and [c.numel() for c in clips] == list(K.RAGGED_N.values())
    assert not clips[0].any() and bool((clips[1] == 0.5).all()) and clips[9].abs().max() > 1.0


def test_geometries():
    from nomad_amd.weights import num_frames
    assert num_frames(K.N_SHORT) == 65 and K.conv0_frames(K.N_SHORT) == 4175            # five statistics chunks of 1024
    assert K.conv0_frames(K.N_LONG) == 8193 and K.N_LONG == 40970                       # 8192 + 1: a one-frame second chunk
    assert -(-K.conv0_frames(K.N_LONG) // 64) == 129                                    # chunks of the GroupNorm backward's sums
    assert set(K.QUIET) | set(K.LOUD) == set(K.NAMES) and set(K.LONG_KINDS) <= set(K.NAMES)


def test_oracles_are_finite_and_the_kink_cap_holds(short, sd0):
    names, wav = short
    undecided = ref64.head_relu_undecided(sd0, wav)            # asserts <= 64 of 768 itself
    print(f"WAVE KINDS head columns within KINK of zero: {int(undecided.sum())}")
    assert int(undecided.sum()) <= 64
    gen = torch.Generator().manual_seed(K.SEED)
    B, T = wav.shape[0], 65
    hw = (torch.rand(256, 768, generator=gen) * 2 - 1) / 768 ** 0.5
    hb = (torch.rand(256, generator=gen) * 2 - 1) / 768 ** 0.5
    hw[:, undecided] = 0.0
    Gl = torch.randn(12, B, T, 768, generator=gen) / (B * T * 768)
    Ge = torch.randn(B, 256, generator=gen) / (B * 256)
    for dt in (torch.float64, torch.float32):
        sd = ref64.cast(sd0, dt)
        with torch.no_grad():
            x, layers = O.backbone(sd, wav.to(dt))
        assert torch.isfinite(x).all() and all(torch.isfinite(y).all() for y in layers), dt
        g = ref64.lossnet_dwav(*ref64.cast((sd0, wav, hw, hb, Gl, Ge), dt), feature_grad_mult=0.1)
        assert torch.isfinite(g).all(), dt
        top = g.abs().amax(1)
        print(f"WAVE KINDS {dt} max |d loss / d wav| per kind: " + ", ".join(f"{k} {v:.2e}" for k, v in zip(names, top.tolist())))
        assert (top > 0).all()


def test_the_ragged_clips_and_the_long_kinds_keep_the_kink_cap(sd0):
    _, clips = K.ragged()
    undecided = torch.zeros(768, dtype=torch.bool)
    for w in clips:
        undecided |= ref64.head_relu_undecided(sd0, w[None])
    assert int(undecided.sum()) <= 64, int(undecided.sum())
    _, long_ = K.batch(K.N_LONG, ["dc_offset"])
    assert int(ref64.head_relu_undecided(sd0, long_).sum()) <= 64


@pytest.mark.parametrize("group", ["quiet", "loud"])
def test_no_triplet_hinge_sits_at_its_switch_point(group):
    """TripletMarginLoss is piecewise linear: a triplet whose d(a, p) - d(a, n) + margin lies within the forward's rounding of 0 has
    its gradient decided by rounding.  Every hinge of both groups is at least HINGE_CLEAR away, and some triplet is active."""
    from nomad_amd.weights import seeded_state_dict
    sd = ref64.cast(seeded_state_dict(3, qk_gain=3.0), torch.float64)
    A, P, N = K.triplet_group(K.QUIET if group == "quiet" else K.LOUD)
    with torch.no_grad():
        ea, ep, en = (O.triplet_forward(sd, w.double()) for w in (A, P, N))
    pd = torch.nn.functional.pairwise_distance
    hinge = pd(ea, ep) - pd(ea, en) + MARGIN
    print(f"WAVE KINDS {group} hinges: " + ", ".join(f"{h:.4f}" for h in hinge.tolist()))
    assert hinge.abs().min().item() >= HINGE_CLEAR and (hinge > 0).any()


def test_the_conv0_formulation_is_sound_on_every_kind(short, sd0):
    names, wav = short
    taps = {}
    for dt in (torch.float64, torch.float32):
        t = {}
        with torch.no_grad():
            O.feature_extractor(ref64.cast(sd0, dt), wav.to(dt), t)
        taps[dt] = t["conv0"]
    bad = []
    for i, name in enumerate(names):
        got = K.conv0_fold_restated(sd0, wav[i])
        (err, e32, bound), = ref64.measure(got, taps[torch.float64][i], taps[torch.float32][i]).values()
        print(f"WAVE KINDS conv0 restated {name}: err {err:.3e} e32 {e32:.3e} err/e32 {err / e32 if e32 else float('inf'):.2f}")
        if not err <= bound:
            bad.append((name, err, e32, bound))
    assert not bad, bad
