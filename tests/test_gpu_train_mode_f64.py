"""GPU: what a fine-tuning run executes and the eval-mode float64 files do not reach - model.train() arithmetic, bf16x3
products on the gradient paths, and Adam with its resume path - against float64 with plain fp32 as the yardstick
(tests/ref64.py: err_gpu <= c * e32 + 1e-7 * top, per tensor).  Weights seeded_state_dict(3, qk_gain=3.0), inputs
0.1 * randn clamped, margin 1.0, n = ref64.n_for(T) samples per clip, as in test_gpu_train_f64.py.  Every engine call runs
inside ``guard.guarded()`` (exact workspaces and outputs between guard bytes); no call needed an exemption.

A. Train mode, fp32 products, c = ref64.C = 8.  Engine and oracle get the same ``O.Stochastic`` settings (the engine's
counter-based masks, restated in the oracle); compared: the three embeddings and the loss (one group), every parameter
gradient (one group).  "sep" = the reference's three embed_train / train_backward calls, one seed and LayerDrop mask per
branch (``ref64.triplet_step``); "merged" = one batch with train_set_branches(masks), one seed
(``ref64.merged_triplet_step``).  Per-branch B, T and what each geometry crosses:

    5, 35   sep, merged  0.1/0.1/0.1, masks (0xFF7, 0xFFE, 0x7BF)   pos-conv dW slices 2, 2, 1, 0; the per-branch mask offsets
                                                                    (bh0, idx0) start at clips 5 and 10
    9, 57   merged       0.1/0.1/0.1, layer 4 dropped by all,       513 rows per branch, 1539 merged: dW contractions whose last
                         layer 9 by one branch                      512-row slice is almost all padding; pos-conv slices 3, 3, 3, 0
    9, 57   merged       0.1/0.1/0.1, all masks 0xFFF               the one-launch-sequence path with dropout on
    2, 127 / 128 / 129   sep, 0.1/0.1/0.1                           two tiles, two full tiles, a third tile of one row; eval mode
                                                                    changes its attention kernel at T = 128, train mode does not
    2, 129  sep          attention_dropout 0.5 only                 half of every row's probabilities masked over three key
                                                                    tiles (the normaliser stays the unmasked one)
    2, 257  merged       0.1/0.1/0.1, masks differ                  five tiles, above kAttnResidentMaxT
    2, 499  merged       0.1/0.1/0.1, masks as LayerDrop 0.05       the reference's clip length (160000 samples): eight tiles,
                         would draw them                            the last of 51 rows.  B = 2, not 8: the oracle pair of this
                                                                    case takes minutes, and B = 8 is run in eval mode elsewhere
    5, 35   sep          0.1/0.1/0.25, convnet trainable,           conv and GroupNorm gradients behind dropout_input (site 0)
                         feature_grad_mult 0.1
    5, 35   merged       none, train_set_frozen(True)               frozen slices exactly 0, the six trainable tensors equal the
                                                                    float64 gradients of the unfrozen model

Seeds are (0x1234567 << 20) + 977 * i: both 32-bit halves non-zero, so both hash rounds carry seed bits.  Before a case
compares, it asserts on the float64 reference: every triplet's hinge argument d(a,p) - d(a,n) + margin > 1e-3 and the loss
> 0; each dropout site in use drops between 0.8 p and 1.2 p of its elements; each LayerDrop mask of a "masks" case drops a
layer; and, once per geometry class on the CPU (not at T = 499), DISCRIMINATION: the float64 oracle with seed + 1 on one
branch (sep) or with the clips rolled by one within every branch and the embeddings rolled back (merged: the same function
of the same clips, only the element index of every mask moves) differs from the true float64 result by more than 100 x the
bound in the embeddings and in every fc2 / out_proj weight gradient of a layer that runs.

B. gemm_precision = "bf16x3" on the gradient paths, c = C_X3P = 80 (test_gpu_forward_f64.py's constant for bf16x3 products
on fp32 buffers): the training step in eval arithmetic at (5, 35) sep and merged, (9, 57) merged, (5, 35) with the extractor
trainable; in train mode at (5, 35) merged with A's masks (against the same oracle pair as the fp32-products run); the loss
path (embed_train + embed_backward, test_gpu_backward_f64._loss_path_case) at 32 x 16384 with feature_grad_mult 0.1 and
1.0 and on both sides of the eight split-K switches.  3 x (8, 160000) merged in this mode lives in
test_gpu_train_f64.py::test_train_step_at_the_reference_shape_vs_float64, next to the oracle pair it shares.  Whatever
the yardstick says, a gradient tensor off by more than 1e-3 of its maximum fails (the header's claim for this mode).

C. Adam and resume, c = 8, ``top`` per vector (parameters ~1, exp_avg_sq down to 1e-24): torch.optim.Adam in float64
(truth) and fp32 (yardstick) on the flat parameter vector, two learning rates split at head_begin.  Gradients are written
(train_write(1)): per segment a scale from {0, 1e-12, 1e-8 (= eps), 1e-4, 1, 1e2}, random signs, a fixed tenth of exact
zeros, frozen-extractor slices zero.  Steps 1, 2, 3 from a fresh engine, then a resume at step 1000 and at step 100000 from
written parameters and moments (train_write(0 / 2 / 3), train_set_step); parameters, exp_avg and exp_avg_sq are compared
after every step.  Elements whose gradient is always zero keep their parameter bits and zero moments; train_read returns
the bits train_write wrote; afterwards embed() equals the oracle on train_state_dict().

Measured on one MI355X, worst err_gpu / e32 per group (the "F64 ..." lines of a -s run):

    A  train mode, fp32 products     embeddings and loss 2.2 - 3.5 (sep B=2 T=129);  gradients 4.4 - 7.0 (sep B=2 T=129,
                                    out_proj.bias; T=499 merged: 5.0; convnet trainable: 5.8; freeze_all: 5.0)       c = 8
    B  bf16x3, training step           embeddings and loss 19.3 - 20.6;  gradients 27.7 - 32.2 in eval arithmetic (3 x (8, 160000)
                                       in test_gpu_train_f64.py: 26.9), 39.4 in train mode (final_layer_norm.weight)    c = 80
    B  bf16x3, loss path               d loss / d waveform 9.8 - 14.0 (M = 2696)                                        c = 80
    C  Adam                            1.00 for parameters, exp_avg and exp_avg_sq at every step, resumed ones included;
                                       embed() afterwards 3.4                                                           c = 8
    discrimination                     a moved mask misses the bound by 3.5e4 x to 1.4e5 x

Two findings went into the code with this file.  Adam: the kernel formed 1 - beta2 as 1.0f - 0.999f = 0.99998713e-3, so every
exp_avg_sq was 1.3e-5 (relative) below torch's - 115 to 181 x e32 in an fp32 restatement of that kernel on the CPU, against
this file's 8; nomad_train_adam_step now takes the betas as doubles and forms 1 - beta on the host.  The loss path's (8, 336)
case sat on the kink of the head's ReLU (ref64.head_relu_undecided): its bf16x3 run was 1332 x e32 off in one clip.

Run time: 2 min 20 s on one MI355X host with 16 CPU threads, nearly all of it CPU: the training steps' oracle pairs 45 s,
the loss path's oracle pairs about 55 s, Adam's two CPU optimisers over 94 M parameters 28 s; the engine calls together
take under 10 s."""
import time

import pytest
import torch
import torch.nn.functional as F

import guard
import ref64
from nomad_amd.weights import num_frames
from oracle import nomad_oracle as O
from test_gpu_backward_f64 import SWITCHES, _loss_path_case
from test_gpu_forward_f64 import C_X3P

pytestmark = pytest.mark.gpu

MARGIN = 1.0
P_ALL = dict(dropout=0.1, attention_dropout=0.1, dropout_input=0.1)
MASKS_5x35 = (0xFF7, 0xFFE, 0x7BF)
MASKS_9x57 = (0xFEF, 0xDEF, 0xFEF)          # layer 4 dropped by all, layer 9 by the positive branch
MASKS_2x257 = (0xFFD, 0xEFF, 0xFDF)
MASKS_2x499 = (0xFFB, 0xF7F, 0xBFF)         # encoder_layerdrop 0.05: 0.6 dropped layers per branch on average
FREEZE_ALL_TRAINABLE = ("ssl_model.post_extract_proj.weight", "ssl_model.post_extract_proj.bias", "ssl_model.layer_norm.weight",
                        "ssl_model.layer_norm.bias", "embedding_layer.1.weight", "embedding_layer.1.bias")
X3_GATE = 1e-3                              # include/nomad_hip.h: a bf16x3 GEMM is within ~3e-5 (relative) of the fp32 one


def _seed(i):
    return (0x1234567 << 20) + 977 * i


@pytest.fixture(scope="module")
def sd_train():
    from nomad_amd.weights import seeded_state_dict
    return seeded_state_dict(3, qk_gain=3.0)


def _engine(sd, precision):
    from nomad_amd.engine import Engine
    eng = Engine({k: v.clone() for k, v in sd.items()}, 0)
    eng.gemm_precision = precision
    return eng


@pytest.fixture(scope="module")
def engines(built_lib, sd_train):
    """{"fp32" | "bf16x3": a training engine with that gemm_precision} (an engine of its own per mode)."""
    engs = {p: _engine(sd_train, p) for p in ("fp32", "bf16x3")}
    for e in engs.values():
        e.train_enable()
    yield engs
    for e in engs.values():
        e.close()


@pytest.fixture(scope="module")
def x3_loss_engine(built_lib, sd0):
    eng = _engine(sd0, "bf16x3")
    yield eng
    eng.close()


# ---- the engine's step -------------------------------------------------------------------------------------------------------
def _apply(eng, st):
    if st is None:
        eng.train_set_stochastic()
    else:
        eng.train_set_stochastic(st.dropout, st.attention_dropout, st.dropout_input, st.seed, st.layer_mask)


def _restore(eng, fgm):
    eng.train_set_stochastic()
    eng.train_set_branches(None)
    eng.train_set_convnet(False)
    eng.train_set_frozen(False)
    eng.feature_grad_mult = fgm


def _step_sep(eng, A, P, N, stochs, case, convnet=False, fgm=None):
    """zero_grad, the reference's three forwards (one setting per branch, set again before each backward), loss, three
    backwards -> (loss, embeddings (3B, 256), {key: gradient})."""
    stochs = stochs if stochs is not None else [None] * 3
    old = eng.feature_grad_mult
    try:
        eng.train_set_convnet(convnet)
        if fgm is not None:
            eng.feature_grad_mult = fgm
        with guard.guarded(case=case):
            eng.train_zero_grad()
            outs = []
            for w, st in zip((A, P, N), stochs):
                _apply(eng, st)
                outs.append(eng.embed_train(w.cuda()))
            loss, da, dp, dn = eng.triplet_loss(outs[0][0], outs[1][0], outs[2][0], MARGIN)
            for w, (emb, layers, saved), d, st in zip((A, P, N), outs, (da, dp, dn), stochs):
                _apply(eng, st)
                eng.train_backward(w.cuda(), layers, saved, d)
            flat = eng.train_read(1)
            res = loss.cpu().reshape(()), torch.cat([o[0] for o in outs]).cpu(), eng.train_unflatten(flat)
    finally:
        _restore(eng, old)
    return res


def _step_merged(eng, A, P, N, st, case, frozen=False):
    """One merged batch A | P | N with one seed; st.branch_masks (or 0xFFF each) per branch."""
    B = A.shape[0]
    old = eng.feature_grad_mult
    masks = list(st.branch_masks) if st is not None and st.branch_masks is not None else [0xFFF] * 3
    try:
        eng.train_set_frozen(frozen)
        _apply(eng, st)
        eng.train_set_branches(masks)
        with guard.guarded(case=case):
            w = torch.cat([A, P, N]).cuda()
            emb, layers, saved = eng.embed_train(w)
            loss, da, dp, dn = eng.triplet_loss(emb[:B].contiguous(), emb[B:2 * B].contiguous(), emb[2 * B:].contiguous(), MARGIN)
            eng.train_zero_grad()
            eng.train_backward(w, layers, saved, torch.cat([da, dp, dn]))
            flat = eng.train_read(1)
            res = loss.cpu().reshape(()), emb.cpu(), eng.train_unflatten(flat)
    finally:
        _restore(eng, old)
    return res


# ---- the float64 / fp32 oracle pair, once per case, and what it must satisfy ----------------------------------------------------
_PAIRS = {}
ORACLE_S = [0.0]


def _pair(key, fn, *args, **kw):
    if key not in _PAIRS:
        t0 = time.time()
        _PAIRS[key] = ref64.both(fn, *args, **kw)
        ORACLE_S[0] += time.time() - t0
        print(f"oracle pair {key}: {time.time() - t0:.0f} s (file so far {ORACLE_S[0]:.0f} s)")
    return _PAIRS[key]


def _hinge(emb64):
    B = emb64.shape[0] // 3
    a, p, n = emb64[:B], emb64[B:2 * B], emb64[2 * B:]
    return F.pairwise_distance(a, p) - F.pairwise_distance(a, n) + MARGIN


def _assert_active(case, r64):
    loss64, emb64, _ = r64
    h = _hinge(emb64)
    assert emb64.dtype == torch.float64 and h.min().item() > 1e-3 and loss64.item() > 0, (case, h.tolist())


def _sites(st, mask):
    """[(site, kind, p)] of the dropout sites a forward with LayerDrop mask ``mask`` (the union over branches) uses."""
    out = [(0, "row", st.dropout_input), (1, "row", st.dropout)]
    for l in range(12):
        if (mask >> l) & 1:
            out += [(2 + 3 * l, "attn", st.attention_dropout), (3 + 3 * l, "row", st.dropout), (4 + 3 * l, "row", st.dropout)]
    return [s for s in out if s[2] > 0]


def _assert_mask_rates(case, st, B, T):
    """Each site in use drops between 0.8 p and 1.2 p of the elements of a (B, T, 768) / (B, 12, T, T) tensor."""
    mask = st.layer_mask
    if st.branch_masks is not None:
        mask = 0
        for m in st.branch_masks:
            mask |= m
    for site, kind, p in _sites(st, mask):
        shape = (B, T, 768) if kind == "row" else (B, 12, T, T)
        rate = (st.mult(site, shape, p) == 0).float().mean().item()
        assert 0.8 * p <= rate <= 1.2 * p, (case, site, p, rate)


def _assert_layerdrop(masks):
    assert all((m & 0xFFF) != 0xFFF for m in masks), masks


def _ran(k, masks):
    """Is ``k`` a parameter of an encoder layer that at least one branch runs (or of no layer at all)?"""
    if "encoder.layers." not in k:
        return True
    l = int(k.split("encoder.layers.")[1].split(".")[0])
    return any((m >> l) & 1 for m in masks)


def _assert_discriminates(case, r64, r32, changed64, masks, c=ref64.C):
    """``changed64``: the float64 oracle with one deliberate change to where the masks fall.  It must miss the bound of
    the true result by a factor of 100 in the embeddings and in every fc2 / out_proj weight gradient of a layer that runs."""
    (_, emb64, g64), (_, emb32, g32), (_, emb_c, g_c) = r64, r32, changed64
    m = ref64.measure({"emb": emb_c}, {"emb": emb64}, {"emb": emb32}, c=c)
    keys = [k for k in g64 if (k.endswith("fc2.weight") or k.endswith("out_proj.weight")) and _ran(k, masks)]
    m.update({k: v for k, v in ref64.measure(g_c, g64, g32, c=c).items() if k in keys})
    assert len(keys) >= 2
    ratios = {k: err / bound for k, (err, e32, bound) in m.items()}
    low = min(ratios, key=ratios.get)
    print(f"F64 {case}: discrimination, a moved mask misses the bound by {ratios[low]:.3g} x ('{low}') to {max(ratios.values()):.3g} x")
    assert ratios[low] > 100, (case, low, ratios[low])


def _compare(case, got, r64, r32, c=ref64.C, gate=None):
    """Embeddings and loss as one group, the gradients as another.  The loss is one scalar, whose fp32 error can be small
    by chance; it is a 2-Lipschitz function of the embeddings (two distances of unit vectors), so its yardstick is at
    least the embeddings' e32."""
    (loss, emb, grads), (loss64, emb64, g64), (loss32, emb32, g32) = got, r64, r32
    assert set(g64) <= set(grads) and all(torch.isfinite(v).all() for v in grads.values())
    e_emb = (emb32.double() - emb64).abs().max().item()
    ref64.check(case + " emb, loss", {"emb": emb, "loss": loss}, {"emb": emb64, "loss": loss64}, {"emb": emb32, "loss": loss32},
                {"loss": e_emb}, c=c)
    ref64.check(case + " grads", {k: grads[k] for k in g64}, g64, g32, c=c)
    if gate is not None:
        for k, want in g64.items():
            assert (grads[k].double() - want).abs().max().item() <= gate * want.abs().max().item() + ref64.FLOOR * max(
                v.abs().max().item() for v in g64.values()), (case, k)


def _stochs(masks, **p):
    return [O.Stochastic(seed=_seed(i), layer_mask=m, **p) for i, m in enumerate(masks)]


def _roll_all(fn, sd, A, P, N, st):
    """The merged float64 oracle on every branch rolled by one clip, results rolled back: clip j of a branch now sits where
    clip j + 1 sat, so the same clips meet the masks of other element indices, and nothing else changes."""
    B = A.shape[0]
    loss, emb, g = fn(*ref64.cast((sd, A.roll(1, 0), P.roll(1, 0), N.roll(1, 0)), torch.float64), MARGIN, stoch=st)
    return loss, torch.cat([emb[i * B:(i + 1) * B].roll(-1, 0) for i in range(3)]), g


# ---- A: train mode ---------------------------------------------------------------------------------------------------------------
def _sep_case(engines, sd, B, T, stochs, case, discriminate=False, modes=("fp32",), **kw):
    A, P, N = ref64.triplet_batch(B, T, seed=B * 100 + T)
    okw = dict(freeze_convnet=False, feature_grad_mult=kw["fgm"]) if kw.get("convnet") else {}
    r64, r32 = _pair(case, ref64.triplet_step, sd, A, P, N, MARGIN, stoch=stochs, **okw)
    _assert_active(case, r64)
    for st in stochs:
        _assert_mask_rates(case, st, B, T)
    if discriminate:
        moved = [stochs[0], O.Stochastic(stochs[1].seed + 1, stochs[1].dropout, stochs[1].attention_dropout,
                                         stochs[1].dropout_input, stochs[1].layer_mask), stochs[2]]
        changed = ref64.triplet_step(*ref64.cast((sd, A, P, N), torch.float64), MARGIN, stoch=moved, **okw)
        _assert_discriminates(case, r64, r32, changed, [s.layer_mask for s in stochs])
    for mode in modes:
        got = _step_sep(engines[mode], A, P, N, stochs, case, **kw)
        _compare(f"{case} {mode}", got, r64, r32, *((C_X3P, X3_GATE) if mode == "bf16x3" else ()))
    return got


def _merged_case(engines, sd, B, T, masks, case, discriminate=False, modes=("fp32",), p=P_ALL):
    A, P, N = ref64.triplet_batch(B, T, seed=B * 100 + T)
    st = O.Stochastic(seed=_seed(3), branch_masks=masks, **p)
    r64, r32 = _pair(case, ref64.merged_triplet_step, sd, A, P, N, MARGIN, stoch=st)
    _assert_active(case, r64)
    _assert_mask_rates(case, st, 3 * B, T)
    if discriminate:
        _assert_discriminates(case, r64, r32, _roll_all(ref64.merged_triplet_step, sd, A, P, N, st), masks)
    for mode in modes:
        got = _step_merged(engines[mode], A, P, N, st, case)
        _compare(f"{case} {mode}", got, r64, r32, *((C_X3P, X3_GATE) if mode == "bf16x3" else ()))
        for l in (l for l in range(12) if not any((m >> l) & 1 for m in masks)):   # a layer no branch ran: exactly no gradient
            assert all(float(v.abs().max()) == 0.0 for k, v in got[2].items() if f"encoder.layers.{l}." in k), (case, l)
    return got


def test_train_mode_separate_calls_b5(engines, sd_train):
    _assert_layerdrop(MASKS_5x35)
    _sep_case(engines, sd_train, 5, 35, _stochs(MASKS_5x35, **P_ALL), "train mode sep B=5 T=35", discriminate=True)


def test_train_mode_merged_b5_with_fp32_and_bf16x3_products(engines, sd_train):
    """Also section B's train-mode case: the bf16x3-products engine against the same oracle pair."""
    _assert_layerdrop(MASKS_5x35)
    _merged_case(engines, sd_train, 5, 35, MASKS_5x35, "train mode merged B=5 T=35", discriminate=True, modes=("fp32", "bf16x3"))


def test_train_mode_merged_b9_with_layerdrop(engines, sd_train):
    _assert_layerdrop(MASKS_9x57)
    assert [l for l in range(12) if not any((m >> l) & 1 for m in MASKS_9x57)] == [4]
    _merged_case(engines, sd_train, 9, 57, MASKS_9x57, "train mode merged B=9 T=57 masks", discriminate=True)


def test_train_mode_merged_b9_one_launch_sequence(engines, sd_train):
    _merged_case(engines, sd_train, 9, 57, (0xFFF,) * 3, "train mode merged B=9 T=57 no LayerDrop")


@pytest.mark.parametrize("T", [127, 128, 129])
def test_train_mode_across_the_eval_kernel_switch(engines, sd_train, T):
    _sep_case(engines, sd_train, 2, T, _stochs((0xFFF,) * 3, **P_ALL), f"train mode sep B=2 T={T}", discriminate=T == 129)


def test_train_mode_half_of_the_probabilities_masked(engines, sd_train):
    _sep_case(engines, sd_train, 2, 129, _stochs((0xFFF,) * 3, dropout=0.0, attention_dropout=0.5, dropout_input=0.0),
              "train mode sep B=2 T=129 attention_dropout 0.5")


def test_train_mode_merged_five_tiles(engines, sd_train):
    _assert_layerdrop(MASKS_2x257)
    _merged_case(engines, sd_train, 2, 257, MASKS_2x257, "train mode merged B=2 T=257", discriminate=True)


def test_train_mode_merged_at_the_reference_clip_length(engines, sd_train):
    assert ref64.n_for(499) <= 160000 and num_frames(160000) == 499
    _assert_layerdrop(MASKS_2x499)
    B = 2
    g = torch.Generator().manual_seed(499)
    A, P, N = [(0.1 * torch.randn(B, 160000, generator=g)).clamp(-1, 1) for _ in range(3)]
    case = "train mode merged B=2 n=160000 T=499"
    st = O.Stochastic(seed=_seed(3), branch_masks=MASKS_2x499, **P_ALL)
    r64, r32 = _pair(case, ref64.merged_triplet_step, sd_train, A, P, N, MARGIN, stoch=st)
    _assert_active(case, r64)
    _assert_mask_rates(case, st, 3 * B, 499)
    _compare(case, _step_merged(engines["fp32"], A, P, N, st, case), r64, r32)


def test_train_mode_with_the_convnet_trainable(engines, sd_train):
    stochs = _stochs((0xFFF,) * 3, dropout=0.1, attention_dropout=0.1, dropout_input=0.25)
    case = "train mode sep convnet B=5 T=35"
    loss, emb, grads = _sep_case(engines, sd_train, 5, 35, stochs, case, convnet=True, fgm=0.1)
    assert all(grads[k].abs().max().item() > 0 for k in grads if "feature_extractor" in k)


# ---- eval arithmetic: freeze_all (A's last row) and B's training steps on bf16x3 products -----------------------------------------
def _eval_pair(sd, B, T, **okw):
    A, P, N = ref64.triplet_batch(B, T, seed=B * 100 + T)
    case = f"eval B={B} T={T}" + (" convnet" if okw else "")
    r64, r32 = _pair(case, ref64.triplet_step, sd, A, P, N, MARGIN, **okw)
    _assert_active(case, r64)
    return A, P, N, r64, r32


def test_freeze_all_merged_b5(engines, sd_train):
    A, P, N, r64, r32 = _eval_pair(sd_train, 5, 35)
    case = "freeze_all merged B=5 T=35"
    loss, emb, grads = _step_merged(engines["fp32"], A, P, N, None, case, frozen=True)
    trainable = lambda r: (r[0], r[1], {k: r[2][k] for k in FREEZE_ALL_TRAINABLE})   # noqa: E731
    _compare(case, (loss, emb, grads), trainable(r64), trainable(r32))
    for k, v in grads.items():
        assert (v.abs().max().item() > 0) if k in FREEZE_ALL_TRAINABLE else (torch.count_nonzero(v).item() == 0), k


def test_bf16x3_training_step_b5_separate_and_merged(engines, sd_train):
    A, P, N, r64, r32 = _eval_pair(sd_train, 5, 35)
    _compare("x3 train sep B=5 T=35", _step_sep(engines["bf16x3"], A, P, N, None, "x3 sep"), r64, r32, C_X3P, X3_GATE)
    _compare("x3 train merged B=5 T=35", _step_merged(engines["bf16x3"], A, P, N, None, "x3 merged"), r64, r32, C_X3P, X3_GATE)


def test_bf16x3_training_step_b9_merged(engines, sd_train):
    A, P, N, r64, r32 = _eval_pair(sd_train, 9, 57)
    _compare("x3 train merged B=9 T=57", _step_merged(engines["bf16x3"], A, P, N, None, "x3 merged"), r64, r32, C_X3P, X3_GATE)


def test_bf16x3_training_step_with_the_convnet_trainable(engines, sd_train):
    A, P, N, r64, r32 = _eval_pair(sd_train, 5, 35, freeze_convnet=False, feature_grad_mult=0.1)
    got = _step_sep(engines["bf16x3"], A, P, N, None, "x3 convnet", convnet=True, fgm=0.1)
    _compare("x3 train convnet B=5 T=35", got, r64, r32, C_X3P, X3_GATE)


# ---- B: the loss path on bf16x3 products ------------------------------------------------------------------------------------------
@pytest.fixture
def x3_grad_mult(x3_loss_engine):
    default = x3_loss_engine.feature_grad_mult

    def set_(m):
        x3_loss_engine.feature_grad_mult = m
    yield set_
    x3_loss_engine.feature_grad_mult = default


def _x3_loss_path(eng, sd0, B, T, mult, seed, grad_mult, n=None):
    assert eng.gemm_precision == "bf16x3"
    with guard.guarded(case=f"x3 loss path B={B} T={T}"):
        return _loss_path_case(eng, sd0, B, T, mult, seed, grad_mult, n=n, c=C_X3P, gate=X3_GATE, tag="x3 ")


@pytest.mark.parametrize("mult", [0.1, 1.0])
def test_bf16x3_loss_path_at_the_product_shape(x3_loss_engine, sd0, mult, x3_grad_mult):
    assert _x3_loss_path(x3_loss_engine, sd0, 32, 50, mult, 4, x3_grad_mult, n=16384) > 0


@pytest.mark.parametrize("B,T", [bt for v in SWITCHES.values() for bt in v],
                         ids=[f"{k.split()[0]}-{'below' if i == 0 else 'above'}" for k, v in SWITCHES.items() for i in range(2)])
def test_bf16x3_loss_path_across_the_split_k_switches(x3_loss_engine, sd0, B, T, x3_grad_mult):
    _x3_loss_path(x3_loss_engine, sd0, B, T, 1.0, B * 1000 + T, x3_grad_mult)


# ---- C: Adam and resume -----------------------------------------------------------------------------------------------------------
SCALES = (0.0, 1e-12, 1e-8, 1e-4, 1.0, 1e2)
LR_BODY, LR_HEAD = 1e-3, 1e-2       # large steps, so that stale derived weights would be obvious in the forward


class _TorchAdam:
    """torch.optim.Adam on the flat parameter vector in ``dtype``: two groups split at head_begin, as train_triplet.py's."""

    def __init__(self, flat, head, dtype):
        self.body = torch.nn.Parameter(flat[:head].to(dtype).clone())
        self.head = torch.nn.Parameter(flat[head:].to(dtype).clone())
        self.opt = torch.optim.Adam([{"params": [self.body], "lr": LR_BODY}, {"params": [self.head]}], lr=LR_HEAD)

    def set_state(self, m, v, step):
        """The optimiser as it stands after ``step`` steps with these moments (its own state set directly)."""
        h = self.body.numel()
        for p, lo, hi in ((self.body, 0, h), (self.head, h, m.numel())):
            self.opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": m[lo:hi].to(p.dtype).clone(),
                                 "exp_avg_sq": v[lo:hi].to(p.dtype).clone()}

    def step(self, grad):
        h = self.body.numel()
        self.body.grad, self.head.grad = grad[:h].to(self.body.dtype).clone(), grad[h:].to(self.body.dtype).clone()
        self.opt.step()

    def vectors(self):
        cat = lambda name: torch.cat([self.opt.state[p][name] for p in (self.body, self.head)])   # noqa: E731
        return {"param": torch.cat([self.body.detach(), self.head.detach()]), "exp_avg": cat("exp_avg"), "exp_avg_sq": cat("exp_avg_sq")}


def _adam_gradients(eng, gen, zero):
    """Per segment one scale of SCALES (cycling, so both learning-rate groups meet every scale), random signs and sizes,
    exact zeros where ``zero`` is set, the conv feature extractor's slices zero (frozen)."""
    total, _ = eng.train_param_count()
    g = torch.zeros(total)
    trainable = [s for s in eng.train_segments() if "feature_extractor" not in s[0]]
    for i, (k, o, n) in enumerate(trainable):
        g[o:o + n] = SCALES[i % len(SCALES)] * torch.randn(n, generator=gen)
    g[zero] = 0.0
    return g


def _adam_compare(case, eng, t64, t32, always_zero, p0):
    with guard.guarded(case=case):
        got = {"param": eng.train_read(0).cpu(), "exp_avg": eng.train_read(2).cpu(), "exp_avg_sq": eng.train_read(3).cpu()}
    r64, r32 = t64.vectors(), t32.vectors()
    for name in got:                                  # one vector per check: ``top`` of its own
        ref64.check(f"{case} {name}", got[name], r64[name], r32[name])
    if always_zero is not None:
        assert torch.equal(got["param"][always_zero].view(torch.int32), p0[always_zero].view(torch.int32))
        assert not got["exp_avg"][always_zero].any() and not got["exp_avg_sq"][always_zero].any()


def test_adam_three_steps_resume_and_weights_follow(built_lib, sd_train):
    eng = _engine(sd_train, "fp32")
    try:
        eng.train_enable()
        total, head = eng.train_param_count()
        gen = torch.Generator().manual_seed(5)
        p0 = eng.train_read(0).cpu()
        zero = torch.rand(total, generator=gen) < 0.1
        t64, t32 = _TorchAdam(p0, head, torch.float64), _TorchAdam(p0, head, torch.float32)
        always_zero = torch.ones(total, dtype=torch.bool)
        for step in (1, 2, 3):
            g = _adam_gradients(eng, gen, zero)
            always_zero &= g == 0
            assert (g != 0).sum().item() > total // 4 and always_zero.sum().item() > total // 10
            t64.step(g)
            t32.step(g)
            with guard.guarded(case=f"adam step {step}"):
                eng.train_write(1, g.cuda())
                eng.adam_step(LR_BODY, LR_HEAD)
            _adam_compare(f"adam step {step}", eng, t64, t32, always_zero, p0)

        for t in (1000, 100000):
            # moments of a run that has seen gradients of each segment's size: |m| ~ 0.3 scale, v ~ scale^2, in fp32, so that
            # all three optimisers start from the same numbers
            p = t64.vectors()["param"].float()
            scale = _adam_gradients(eng, gen, zero)
            m = 0.3 * scale
            v = (scale * scale * (0.5 + torch.rand(total, generator=gen))).float()
            t64, t32 = _TorchAdam(p, head, torch.float64), _TorchAdam(p, head, torch.float32)
            t64.set_state(m, v, t)
            t32.set_state(m, v, t)
            with guard.guarded(case=f"adam resume at {t}"):
                for what, vec in ((0, p), (2, m), (3, v)):
                    eng.train_write(what, vec.cuda())
                eng.train_set_step(t)
                g = _adam_gradients(eng, gen, zero)
                eng.train_write(1, g.cuda())
                for what, vec in ((0, p), (1, g), (2, m), (3, v)):     # read after write: the same bits
                    assert torch.equal(eng.train_read(what).cpu().view(torch.int32), vec.view(torch.int32)), what
                eng.adam_step(LR_BODY, LR_HEAD)
            t64.step(g)
            t32.step(g)
            _adam_compare(f"adam resume at step {t}", eng, t64, t32, None, None)

        # the derived kernel-layout weights were rebuilt from the master copy: the forward is the oracle's on train_state_dict()
        new_sd = eng.train_state_dict()
        assert set(new_sd) == set(sd_train)
        assert torch.equal(eng.train_flatten(new_sd).cpu(), eng.train_read(0).cpu())
        wav = ref64.triplet_batch(2, 18, seed=2)[0]
        with torch.no_grad():
            e64, e32 = ref64.both(O.triplet_forward, new_sd, wav)
        with guard.guarded(case="embed after adam"):
            emb = eng.embed(wav.cuda()).cpu()
        ref64.check("embed after the adam steps", emb, e64, e32)
    finally:
        eng.close()
