"""GPU: the triplet fine-tuning step's parameter gradients against float64, with plain fp32 as the yardstick
(tests/ref64.py: err_gpu <= 8 e32 + 1e-7 top, per tensor).  test_gpu_train.py holds the same step to 2e-4 of each
tensor's largest gradient against the fp32 oracle, at B <= 3; here the batch- and length-dependent paths of
train_backward are crossed:

* B = 5 and 9 clips per branch: the pos-conv weight gradient splits the batch into min(B, 4) slices of ceil(B / 4) clips
  (5 -> 2, 2, 1, 0; 9 -> 3, 3, 3, 0: an empty last slice);
* rows just above a multiple of 512, where the dW GEMMs' contraction (Mp = ceil512(M)) is almost all zero padding
  in its last slice: 9 x 57 = 513 rows per branch, 3 x 9 x 57 = 1539 merged, 3 x 5 x 35 = 525 merged;
* the conv feature extractor trainable (freeze_convnet: False);
* the reference's own shape, 3 x (8, 160000) as one merged batch: T = 499, 11976 rows (tests/manual/check_train_fullsize.py
  runs the same step against the fp32 oracle)."""
import pytest
import torch

import ref64
from nomad_amd.weights import num_frames

pytestmark = pytest.mark.gpu

MARGIN = 1.0


@pytest.fixture(scope="module")
def sd_train():
    from nomad_amd.weights import seeded_state_dict
    return seeded_state_dict(3, qk_gain=3.0)


@pytest.fixture(scope="module")
def teng(built_lib, sd_train):
    from nomad_amd.engine import Engine
    eng = Engine({k: v.clone() for k, v in sd_train.items()}, 0)
    eng.train_enable()
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def xeng(built_lib, sd_train):
    """The same engine with gemm_precision = "bf16x3" (three bf16 products per fp32 product, fp32 buffers)."""
    from nomad_amd.engine import Engine
    eng = Engine({k: v.clone() for k, v in sd_train.items()}, 0)
    eng.gemm_precision = "bf16x3"
    eng.train_enable()
    yield eng
    eng.close()


def _batch(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    n = ref64.n_for(T)
    return [(0.1 * torch.randn(B, n, generator=g)).clamp(-1, 1) for _ in range(3)]


def _step_separate(eng, A, P, N):
    eng.train_zero_grad()
    outs = [eng.embed_train(w.cuda()) for w in (A, P, N)]
    loss, da, dp, dn = eng.triplet_loss(outs[0][0], outs[1][0], outs[2][0], MARGIN)
    for w, (emb, layers, saved), d in zip((A, P, N), outs, (da, dp, dn)):
        eng.train_backward(w.cuda(), layers, saved, d)
    return loss.item(), eng.train_unflatten(eng.train_read(1))


def _step_merged(eng, A, P, N):
    B = A.shape[0]
    w = torch.cat([A, P, N]).cuda()
    eng.train_set_branches([0xFFF] * 3)
    try:
        emb, layers, saved = eng.embed_train(w)
        loss, da, dp, dn = eng.triplet_loss(emb[:B].contiguous(), emb[B:2 * B].contiguous(), emb[2 * B:].contiguous(), MARGIN)
        eng.train_zero_grad()
        eng.train_backward(w, layers, saved, torch.cat([da, dp, dn]))
    finally:
        eng.train_set_branches(None)
    return loss.item(), eng.train_unflatten(eng.train_read(1))


def _check(case, got, loss, r64, r32, c=ref64.C):
    (loss64, g64), (loss32, g32) = r64, r32
    assert loss64.item() > 0                    # some triplet is active, otherwise the gradients are vacuous
    assert abs(loss - loss64.item()) <= c * abs(loss32.item() - loss64.item()) + 1e-6, (loss, loss64.item(), loss32.item())
    ref64.check(case, {k: got[k] for k in g64}, g64, g32, c=c)


@pytest.mark.parametrize("B,T", [(5, 35), (9, 57)])
def test_train_step_vs_float64_separate_and_merged(teng, sd_train, B, T):
    """One oracle step (eval-mode arithmetic is batch-independent, so the reference's three calls and one merged batch
    are the same function) against the engine's three calls and its merged batch."""
    A, P, N = _batch(B, T, seed=B * 100 + T)
    r64, r32 = ref64.both(ref64.triplet_grads, sd_train, A, P, N, MARGIN)
    loss, got = _step_separate(teng, A, P, N)
    _check(f"train separate B={B} T={T} M={B * T}", got, loss, r64, r32)
    loss, got = _step_merged(teng, A, P, N)
    _check(f"train merged B={B} T={T} M={3 * B * T}", got, loss, r64, r32)


def test_train_step_with_the_convnet_trainable_vs_float64(teng, sd_train):
    """freeze_convnet: False at B = 5: conv0..6 weights and the GroupNorm affine as well, feature_grad_mult 0.1."""
    B, T = 5, 35
    A, P, N = _batch(B, T, seed=7)
    r64, r32 = ref64.both(ref64.triplet_grads, sd_train, A, P, N, MARGIN, freeze_convnet=False, feature_grad_mult=0.1)
    old = teng.feature_grad_mult
    teng.train_set_convnet(True)
    teng.feature_grad_mult = 0.1
    try:
        loss, got = _step_separate(teng, A, P, N)
    finally:
        teng.train_set_convnet(False)
        teng.feature_grad_mult = old
    _check(f"train convnet B={B} T={T}", got, loss, r64, r32)


def test_train_step_at_the_reference_shape_vs_float64(teng, xeng, sd_train):
    """3 x (8, 160000) merged: T = 499 (eight 64-row attention tiles, the last one of 51 rows), 11976 rows.  The oracle pair
    of this geometry takes minutes, so the bf16x3-products engine is compared against the same pair, with the constant
    of that arithmetic (test_gpu_forward_f64.C_X3P; test_gpu_train_mode_f64.py section B holds the smaller shapes) and
    the ceiling of 1e-3 of each gradient's maximum."""
    from test_gpu_forward_f64 import C_X3P
    B, n = 8, 160000
    assert num_frames(n) == 499
    g = torch.Generator().manual_seed(0)
    A, P, N = [(0.1 * torch.randn(B, n, generator=g)).clamp(-1, 1) for _ in range(3)]
    r64, r32 = ref64.both(ref64.triplet_grads, sd_train, A, P, N, MARGIN)
    loss, got = _step_merged(teng, A, P, N)
    _check("train merged reference shape 3x(8,160000) M=11976", got, loss, r64, r32)
    loss, got = _step_merged(xeng, A, P, N)
    _check("x3 train merged reference shape 3x(8,160000) M=11976", got, loss, r64, r32, c=C_X3P)
    top = max(v.abs().max().item() for v in r64[1].values())
    for k, want in r64[1].items():
        assert (got[k].double() - want).abs().max().item() <= 1e-3 * want.abs().max().item() + ref64.FLOOR * top, k
