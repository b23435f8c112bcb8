"""CPU: what a non-finite clip does in the REFERENCE arithmetic - the contract tests/test_gpu_nonfinite.py holds the HIP paths to - and
that the assertions of tests/nonfinite.py reject the two ways the engine got it wrong.

1. The oracle experiment.  ``oracle.nomad_oracle.lossnet_forward``, ``seeded_state_dict(0)``, B = 3, T = 5 (``nonfinite.N_TINY``
   samples, three of them behind the last conv0 frame).  One sample of clip 1 is NaN, +Inf or -Inf at the first, the middle or the
   last sample conv0 reads: in all 9 cases every element of all 13 outputs of clip 1 is NaN, and clips 0 and 2 keep the clean run's
   bits (conv0's GroupNorm takes its statistics over the whole clip, so one sample reaches every frame; no operation mixes clips).  A
   poisoned sample behind the last conv0 frame changes no bit anywhere.  The same for the rows the windowed and the span heads form
   (``O.head`` on the rows of a window / on the concatenated rows of a row's spans, as test_gpu_windows.py and test_gpu_spans.py
   restate them), for the per-utterance loss terms, the scores and the triplet loss, and once at the ``small`` geometry (T = 65).
   The autograd masks property B uses for gradients: d loss / d estimate of the poisoned clip is NaN on every sample conv0 reads and an
   exact zero on the unread tail - so the oracle's mask of a clip with a tail is NOT all-NaN and ``nonfinite.same_mask`` falls to the
   any / none answer there, and is elementwise for a clip without a tail; the other clips' gradients keep the clean bits; every
   parameter gradient of a triplet step with one poisoned anchor is NaN everywhere.
2. Teeth.  The head restated with ``torch.fmax(x, 0)`` - what ``fmaxf(x, 0.f)`` computes - gives the NaN clip the finite embedding
   normalize(bias): ``nonfinite.contained`` rejects it.  A triplet loss with ``fmax`` is finite: the NaN assertion rejects it.
3. The geometries: what each reaches, as arithmetic on the dispatch thresholds (bf16: ``test_gpu_bf16_stages_f64.forward_kernels``;
   fp32: ``nonfinite.pick_tile_f32`` / ``mixed_split_rows``, whose constants are compared with the source text).
"""
import pytest
import torch
import torch.nn.functional as F

import nonfinite as NF
import ref64
from nomad_amd.weights import num_frames, num_windows
from oracle import nomad_oracle as O

B, J = 3, 1
WIN, HOP = 2, 1                                         # T = 5: windows over frames 0-1, 1-2, 2-3, 3-4
SPANS = [[(0, 2)], [(1, 2), (3, 5)], [(0, 5)]]          # rows of every clip: one span, two spans, the whole clip


def _head(sd):
    return sd["embedding_layer.1.weight"], sd["embedding_layer.1.bias"]


def _outputs(sd, wav, relu=F.relu):
    """{name: (B, ...)}: the 12 layers, the embedding, the window rows and the span rows of every clip, the per-utterance loss terms
    against a clean batch of its own, the scores against three references."""
    w, b = _head(sd)

    def head(x):
        return F.normalize(F.linear(relu(torch.mean(x, 1)), w, b), dim=1)

    with torch.no_grad():
        x, layers = O.backbone(sd, wav, required_seq_len_multiple=2)
        clean = NF.waves(wav.shape[0], wav.shape[1], NF.SEED + 1)                       # the loss's clean side: always finite
        T = x.shape[1]
        out = {f"layer{l}": y for l, y in enumerate(layers)}
        out["emb"] = head(x)
        if relu is F.relu:
            assert torch.equal(torch.nan_to_num(out["emb"]), torch.nan_to_num(O.head(x, w, b)))      # the restatement is the oracle's head
        n = min(WIN, T)
        out["windows"] = torch.stack([head(x[:, k * HOP:k * HOP + n]) for k in range(num_windows(T, WIN, HOP))], 1)
        out["spans"] = torch.stack([head(torch.cat([x[:, a:e] for a, e in row], 1)) for row in SPANS], 1)
        refs = F.normalize(torch.randn(3, 256, generator=torch.Generator().manual_seed(5)), dim=1)
        out["score"] = torch.cdist(out["emb"].double(), refs.double()).mean(1)
        xc, lc = O.backbone(sd, clean, required_seq_len_multiple=2)
        out["loss_terms"] = sum((a - c).abs().mean((1, 2)) for a, c in zip(layers, lc)) + (out["emb"] - head(xc)).abs().mean(1)
    return out


@pytest.fixture(scope="module")
def tiny(sd0):
    wav = NF.waves(B, NF.N_TINY)
    assert num_frames(NF.N_TINY) == 5
    return wav, _outputs(sd0, wav)


def _check_all(case, clean, bad, own):
    for k in clean:
        NF.contained(f"{case} {k}", clean[k], bad[k], clean[k], own)


@pytest.mark.parametrize("value, where", NF.FULL)
def test_oracle_a_poisoned_sample_makes_its_clip_nan_and_no_other(sd0, tiny, value, where):
    wav, clean = tiny
    bad = _outputs(sd0, NF.poison_batch(wav, J, NF.position(NF.N_TINY, where), NF.VALUES[value]))
    assert len(clean) == 12 + 5
    _check_all(f"oracle {value} {where}", clean, bad, NF.rows_of([1] * B, J))


@pytest.mark.parametrize("value", list(NF.VALUES))
def test_oracle_the_unread_tail_changes_nothing(sd0, tiny, value):
    wav, clean = tiny
    at = NF.tail_position(NF.N_TINY)
    assert at == NF.N_TINY - 1 and NF.position(NF.N_TINY, "last_read") == NF.N_TINY - 4
    bad = _outputs(sd0, NF.poison_batch(wav, J, at, NF.VALUES[value]))
    _check_all(f"oracle tail {value}", clean, bad, None)


def test_oracle_at_the_small_geometry(sd0):
    """T = 65, B = 3, NaN in the middle of clip 1: the forward's 13 outputs."""
    g = NF.SMALL
    wav = NF.waves(g["B"], g["n"])
    w, b = _head(sd0)
    with torch.no_grad():
        clean = O.lossnet_forward(sd0, wav, w, b)
        bad = O.lossnet_forward(sd0, NF.poison_batch(wav, g["j"], g["n"] // 2, NF.NAN), w, b)
    assert clean[0].shape == (g["B"], g["T"], 768)
    for i in range(13):
        NF.contained(f"oracle small output {i}", clean[i], bad[i], clean[i], NF.rows_of([1] * g["B"], g["j"]))


def test_frame_energy_frames():
    """Sample i lies in the 400 samples of frame t exactly when 320 t <= i < 320 t + 400: one or two frames, none for the tail."""
    n, T = NF.SMALL["n"], NF.SMALL["T"]
    assert NF.frames_reading(0, T) == [0] and NF.frames_reading(n // 2, T) == [32] and NF.frames_reading(399, T) == [0, 1]
    assert NF.frames_reading(NF.position(n, "last_read"), T) == [] and NF.frames_reading(NF.tail_position(n), T) == []
    assert 320 * (T - 1) + 400 <= NF.position(n, "last_read")     # conv0 reads further than the last encoder frame's 400 samples
    x = NF.poison(NF.waves(1, n)[0], n // 2, NF.NAN).double()
    e = x.unfold(0, 400, 320).pow(2).mean(1)
    assert e.shape == (T,) and torch.isnan(e).nonzero().flatten().tolist() == [32]


# ---- the autograd masks of property B ---------------------------------------------------------------------------------------------
def _dloss(sd, est, clean):
    w, b = _head(sd)
    e = est.clone().requires_grad_(True)
    oe = O.lossnet_forward(sd, e, w, b, feature_grad_mult=0.1, required_seq_len_multiple=2)
    with torch.no_grad():
        oc = O.lossnet_forward(sd, clean, w, b, required_seq_len_multiple=2)
    terms = sum((a - c).abs().mean((1, 2)) for a, c in zip(oe[:12], oc[:12])) + (oe[12] - oc[12]).abs().mean(1)
    (g,) = torch.autograd.grad(terms.sum(), e)
    return terms.detach(), g


@pytest.mark.parametrize("value, where", NF.REDUCED)
def test_oracle_gradient_mask_of_the_loss(sd0, value, where):
    n = NF.N_TINY
    est, clean = NF.waves(B, n), NF.waves(B, n, NF.SEED + 1)
    t0, g0 = _dloss(sd0, est, clean)
    t1, g1 = _dloss(sd0, NF.poison_batch(est, J, NF.position(n, where), NF.VALUES[value]), clean)
    other = ~NF.rows_of([1] * B, J)
    assert torch.isnan(t1[J]) and torch.equal(t1[other], t0[other])
    assert torch.equal(g1[other], g0[other]) and torch.isfinite(g0).all()
    read = NF.position(n, "last_read") + 1
    assert torch.isnan(g1[J, :read]).all(), "every sample conv0 reads"
    assert not g1[J, read:].any() and read == n - 3, "the unread tail: exact zeros"
    # what same_mask makes of it: elementwise on a clip without a tail, any / none with one
    assert NF.same_mask("read part", g1[J, :read], g1[J, :read]) == "elementwise"
    assert NF.same_mask("whole clip", g1[J], g1[J]) == "any"
    with pytest.raises(AssertionError):
        NF.same_mask("a finite gradient where the oracle's is NaN", g0[J], g1[J])
    with pytest.raises(AssertionError):
        NF.same_mask("one finite element", torch.cat([g1[J, :read - 1], g0[J, :1]]), g1[J, :read])


def test_oracle_parameter_gradients_of_a_triplet_step_with_one_poisoned_anchor(sd0):
    A, P, N = ref64.triplet_batch(2, 5, 3)
    A = NF.poison_batch(A, 1, A.shape[1] // 2, NF.NAN)
    loss, grads = ref64.triplet_grads(sd0, A, P, N, 1.0)
    assert torch.isnan(loss)
    assert len(grads) > 100 and all(torch.isnan(g).all() for g in grads.values()), [k for k, g in grads.items() if not torch.isnan(g).all()][:5]


def test_torch_distances_with_a_nan_row():
    """cdist, its row means and the paired distance: a NaN row of a is a NaN row of the matrix, a NaN row of b a NaN column and
    every mean; float64 autograd makes da's row / db everywhere non-finite and the reverse."""
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(5, 256, generator=g, dtype=torch.float64), torch.randn(7, 256, generator=g, dtype=torch.float64)
    an, bn = a.clone(), b.clone()
    an[2, 100], bn[4, 0] = NF.NAN, NF.NAN
    d = torch.cdist(an, b)
    assert torch.isnan(d[2]).all() and torch.isfinite(d[[0, 1, 3, 4]]).all() and torch.isnan(d.mean(1)).tolist() == [False, False, True, False, False]
    d = torch.cdist(a, bn)
    assert torch.isnan(d[:, 4]).all() and torch.isfinite(d[:, [0, 1, 2, 3, 5, 6]]).all() and torch.isnan(d.mean(1)).all()
    x = an.clone().requires_grad_(True)
    y = b.clone().requires_grad_(True)
    (x[:, None] - y[None]).pow(2).sum(-1).sqrt().sum().backward()
    assert torch.isnan(x.grad[2]).all() and torch.isfinite(x.grad[[0, 1, 3, 4]]).all() and torch.isnan(y.grad).all()


# ---- teeth ------------------------------------------------------------------------------------------------------------------------
def _fmax_relu(x):
    return torch.fmax(x, torch.zeros(()))               # IEEE maxNum: what fmaxf(x, 0.f) computes - 0 for a NaN


def test_a_head_with_fmax_is_rejected(sd0, tiny):
    wav, clean = tiny
    bad_wav = NF.poison_batch(wav, J, NF.N_TINY // 2, NF.NAN)
    right, wrong = _outputs(sd0, bad_wav), _outputs(sd0, bad_wav, relu=_fmax_relu)
    own = NF.rows_of([1] * B, J)
    w, b = _head(sd0)
    for k in ("emb", "windows", "spans", "score"):        # (the loss terms also read the layers: NaN either way)
        NF.contained(k, clean[k], right[k], clean[k], own)
        assert torch.isfinite(wrong[k]).all(), k          # finite and plausible ...
        with pytest.raises(AssertionError, match="are not NaN"):
            NF.contained(k, clean[k], wrong[k], clean[k], own)
    assert torch.equal(wrong["emb"][J], F.normalize(b, dim=0))           # ... the same embedding for every broken clip
    for k in clean:                                        # on finite input the two heads are the same bits
        assert torch.equal(_outputs(sd0, wav, relu=_fmax_relu)[k], clean[k]), k


def test_a_triplet_hinge_with_fmax_is_rejected():
    g = torch.Generator().manual_seed(4)
    a, p, n = (F.normalize(torch.randn(4, 256, generator=g), dim=1) for _ in range(3))
    a[2] = NF.NAN
    right = F.triplet_margin_loss(a, p, n, margin=1.0)
    hinge = F.pairwise_distance(a, p) - F.pairwise_distance(a, n) + 1.0
    wrong = _fmax_relu(hinge).mean()
    assert torch.isnan(right) and torch.isfinite(wrong)
    assert torch.equal(torch.clamp_min(hinge, 0).mean().isnan(), torch.tensor(True))
    with pytest.raises(AssertionError):
        assert torch.isnan(wrong), "the loss of a batch with a NaN anchor"


def test_relu_select_restated():
    """``relu_keep_nan`` (rowops.hip.h): x > 0 ? x : (x != x ? x : 0) over the edge values - torch.relu's result on every one."""
    x = torch.tensor([NF.NAN, NF.INF, -NF.INF, 0.0, -0.0, 1e-45, -1e-45, 3.0, -3.0])
    sel = torch.where(x > 0, x, torch.where(x != x, x, torch.zeros(())))
    want = torch.relu(x)
    assert torch.equal(torch.isnan(sel), torch.isnan(want)) and torch.equal(torch.nan_to_num(sel), torch.nan_to_num(want))
    assert not torch.signbit(sel[3:5]).any() and sel[1] == NF.INF and sel[2] == 0 and torch.isnan(sel[0])


# ---- the geometries ----------------------------------------------------------------------------------------------------------------
def test_lengths_and_positions():
    for n in [NF.N_TINY, NF.SMALL["n"], NF.MID["n"]] + NF.RAGGED_N:
        L0 = NF.conv0_frames(n)
        assert (n - 10) % 5 != 0 and n % 320 and n % 5
        assert [NF.position(n, w) for w in NF.POSITIONS] == [0, n // 2, 5 * (L0 - 1) + 9]
        assert NF.position(n, "last_read") < NF.tail_position(n) == n - 1 < 5 * L0 + 9       # one more frame would not fit
    assert [num_frames(n) for n in NF.RAGGED_N] == NF.RAGGED_T == [1, 64, 2, 65, 130, 35]
    assert num_frames(NF.SMALL["n"]) == 65 and num_frames(NF.MID["n"]) == 130
    assert NF.RAGGED_J == [0, 3, 5] and NF.RAGGED_T[3] == 65 and len(NF.RAGGED_T) == 6
    assert len(NF.FULL) == 9 and set(NF.REDUCED) <= set(NF.FULL)


def test_the_bf16_geometries_reach_what_they_claim():
    from test_gpu_bf16_stages_f64 import GEOMS, attention_queries, forward_kernels, posconv_frames
    gemms = ["projection", "qkv", "out_proj", "fc1", "fc2"]
    s = forward_kernels(NF.SMALL["B"], NF.SMALL["n"])
    M = NF.SMALL["B"] * 65
    assert all(s[k] == "64x64" for k in gemms) and s["attention"] == 128 and s["posconv"] == 128
    assert M % 4 == 3 and 65 % 64 == 1                   # a last LayerNorm wave of 3 rows; partial key and query blocks
    m = forward_kernels(NF.MID["B"], NF.MID["n"])
    assert m["posconv"] == 256 and m["attention"] == 128 and m["qkv"] == m["fc1"] == "256x256"
    assert all(m[k] == "128x128" for k in ("projection", "out_proj", "fc2"))
    assert NF.MID["B"] % 2 == 1 and NF.MID["j"] // 2 == (NF.MID["j"] + 1) // 2 == 1       # clips 2 and 3 share a pos-conv workgroup
    assert sorted({posconv_frames(T) for T in NF.RAGGED_T}) == [128, 256]
    assert GEOMS["large"][:2] == (NF.BF16_LARGE_B, NF.N_10S)
    l = forward_kernels(NF.BF16_LARGE_B, NF.N_10S)
    assert l["attention"] == attention_queries(NF.BF16_LARGE_B, 499) == 256 and l["posconv"] == 512
    assert all(l[k].startswith("persistent") for k in ("qkv", "out_proj", "fc1", "fc2")) and l["conv1"] == "persistent"


def test_the_attention_backward_kernels_by_clip_length():
    """attention_bwd.hip.h: clips of at most 64 frames take the fused kernel, longer ones the three kernels."""
    import os
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nomad_amd", "csrc", "attention_bwd.hip.h")).read()
    assert "if (T <= 64 && !dc.threshold && !force_three)" in text and "if (T > 64) return;" in text
    assert NF.SMALL["T"] > 64 and NF.MID["T"] > 64 and {T <= 64 for T in NF.RAGGED_T} == {True, False}


def test_the_fp32_large_batch_is_the_smallest_on_the_mixed_kernel():
    c = NF.dispatch_constants()
    assert c == dict(min_fill=NF.MIXED_MIN_FILL, max_fill=NF.MIXED_MAX_FILL, penalty=(1.08, 1.03), big=True, rounds1500=True, small=True,
                     slots=True, mixed_on_33=True), c
    assert NF.F32_LARGE_B == 25 and NF.f32_mixed_gemms(25) == ["fc1"]
    assert not any(NF.f32_mixed_gemms(b) for b in range(1, 25))
    M = 25 * 499
    assert NF.pick_tile_f32(M, 3072) == 33 and NF.mixed_split_rows(M, 3072) == 10752 < M       # 42 row tiles of 256, the rest 128 x 128
    assert NF.pick_tile_f32(24 * 499, 3072) == 31        # one clip fewer: 128 x 128 tiles throughout
    assert (25 - 1) // 2 == 12                            # the poisoned clip: rows 5988 .. 6486, inside the 256 x 128 part
