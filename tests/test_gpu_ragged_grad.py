"""GPU: exact-length (ragged) batches on the gradient paths - nomad_embed_train_ragged, nomad_embed_backward_ragged,
nomad_train_backward_ragged, nomad_l1_loss(_backward)_ragged, ``Nomad.forward(estimate, clean, lengths)`` and
``Training(pad_mode="exact")``.

Two kinds of checks:

* equal bits (fine-tuning mode, where no GEMM splits K): a clip of a mixed batch comes out with the bits of its own B = 1 call
  (embedding, layer outputs, d loss / d waveform), a permuted batch permutes the per-clip results, and an equal-length batch
  handed to the ragged entry points gives the bits of the equal-length entry points - forward, d waveform and the whole
  gradient vector, in eval mode and with dropout + per-branch LayerDrop (the packed mask indices of an equal-length batch are
  the equal-length ones);
* float64 (tests/ref64.py as it is: err_gpu <= 8 e32 + 1e-7 top; test_gpu_forward_f64.C_X3P in front of e32 for bf16x3
  products): the truth of a ragged batch is the oracle run per clip at that clip's exact length (B = 1), the results
  concatenated, then the loss and torch.autograd over the whole thing.

The mixed batches hold clips on both sides of every per-clip switch in ONE batch: T_c = 1, 2, 64 | 65 (fused | three-kernel
attention backward, and the forward's short-clip | long-clip kernel at 64), 130 (a partial last 64-row tile), odd and even
L_i at every conv level (asserted below), one clip much longer than the rest (T = 499), B = 9 and 5.

Every float64 case prints its figures (``F64 ...`` lines: err_gpu, e32, err_gpu / e32, share of the bound) before it
asserts.  Measured on one MI355X (err_gpu / e32, worst tensor per case):

    loss path fp32, d loss / d estimate and d clean (L1 signs pinned, section 2)   2.72   (0.34 of the bound)
    the same against float64's own L1 signs (not asserted, see section 2)          1071   on the T = 64 clip: one flipped sign
    loss value fp32: 8.20252991 against 8.20252993                                 err 2.2e-8 = 0.05 of half an fp32 ulp
    loss value bf16x3 products: 8.20252705                                         err 2.9e-6 = 6.0 half ulps (C_X3P = 80)
    L1 differences within KINK of zero                                             727 of 6 994 944
    padded, equal-length loss on the same tensors                                  2.66449475: 5e6 bounds away
    merged ragged step, eval mode: gradients / bf16x3 products                     4.85 / 26.5 (embeddings 7.70)
    merged ragged step, freeze_all                                                 3.38
    merged ragged step, dropout + per-branch LayerDrop                             3.70
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard
import ref64
from nomad_amd import _lib
from nomad_amd.weights import num_frames
from oracle import nomad_oracle as O

pytestmark = pytest.mark.gpu

MARGIN = 1.0
MIXED_T = [1, 2, 35, 64, 65, 130, 57, 200, 499]      # B = 9
MIXED_EXTRA = [0, 150, 37, 111, 163, 5, 251, 83, 301]  # samples on top of ref64.n_for(T) (kept where T stays): odd and even L_i
LOSS_T = [1, 64, 65, 130, 499]                        # B = 5
LOSS_EXTRA = [0, 111, 163, 5, 301]
KS, SS = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)


def conv_lens(n):
    out = []
    for k, s in zip(KS, SS):
        n = (n - k) // s + 1
        out.append(n)
    return out


def clip_samples(T, extra):
    n = ref64.n_for(T)
    return n + extra if num_frames(n + extra) == T else n


def make_clips(Ts, extras, seed):
    g = torch.Generator().manual_seed(seed)
    return [(0.1 * torch.randn(clip_samples(T, e), generator=g)).clamp(-1, 1) for T, e in zip(Ts, extras)]


def test_the_mixed_batches_cross_every_per_clip_switch():
    for Ts, ex in ((MIXED_T, MIXED_EXTRA), (LOSS_T, LOSS_EXTRA)):
        L = [conv_lens(clip_samples(T, e)) for T, e in zip(Ts, ex)]
        assert [l[6] for l in L] == Ts
        for i in range(7):
            assert {l[i] % 2 for l in L} == {0, 1}, (i, [l[i] for l in L])
        assert min(Ts) == 1 and 64 in Ts and 65 in Ts and 130 in Ts and max(Ts) == 499


@pytest.fixture(scope="module")
def sd_train():
    from nomad_amd.weights import seeded_state_dict
    return seeded_state_dict(3, qk_gain=3.0)


def _engine(sd, x3=False, train=True):
    from nomad_amd.engine import Engine
    eng = Engine({k: v.clone() for k, v in sd.items()}, 0)
    if x3:
        eng.gemm_precision = "bf16x3"
    if train:
        eng.train_enable()
    return eng


@pytest.fixture(scope="module")
def teng(built_lib, sd_train):
    eng = _engine(sd_train)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def xeng(built_lib, sd_train):
    eng = _engine(sd_train, x3=True)
    yield eng
    eng.close()


def _rows(Ts):
    return np.concatenate([[0], np.cumsum(Ts)]).tolist()


# ---- 1. equal bits, fine-tuning mode -----------------------------------------------------------------------------------------
def test_a_clip_of_a_mixed_batch_has_the_bits_of_its_own_call(teng):
    clips = [c.cuda() for c in make_clips(MIXED_T, MIXED_EXTRA, seed=11)]
    B, r = len(clips), _rows(MIXED_T)
    M = r[-1]
    emb, layers, saved, batch = teng.embed_train_ragged(clips)
    assert layers.shape == (12, M, 768) and emb.shape == (B, 256)
    assert torch.equal(emb, teng.embed_ragged(clips))                      # the scoring path's bits
    g = torch.Generator().manual_seed(5)
    G = (torch.randn(12, M, 768, generator=g) / (M * 768)).cuda()
    Ge = (torch.randn(B, 256, generator=g) / (B * 256)).cuda()
    dwav = teng.embed_backward_ragged(batch, layers, saved, G, Ge)
    assert torch.isfinite(dwav).all()
    for c, clip in enumerate(clips):
        T, n = MIXED_T[c], clip.numel()
        e1, l1, s1 = teng.embed_train(clip[None])
        assert torch.equal(e1[0], emb[c]), c
        assert torch.equal(l1[:, 0], layers[:, r[c]:r[c + 1]]), c
        d1 = teng.embed_backward(clip[None], l1, s1, G[:, r[c]:r[c + 1]].reshape(12, 1, T, 768).contiguous(), Ge[c:c + 1].contiguous())
        assert torch.equal(d1[0], dwav[c, :n]), (c, (d1[0] - dwav[c, :n]).abs().max().item())
        assert not dwav[c, n:].any(), c                                    # zero behind the clip's length
    # a permuted batch permutes the per-clip results and nothing else
    perm = [4, 8, 0, 6, 2, 7, 1, 5, 3]
    pe, pl, ps, pb = teng.embed_train_ragged([clips[i] for i in perm])
    Gp = torch.cat([G[:, r[i]:r[i + 1]] for i in perm], dim=1).contiguous()
    pd_ = teng.embed_backward_ragged(pb, pl, ps, Gp, Ge[perm].contiguous())
    assert torch.equal(pe, emb[perm])
    assert torch.equal(pl, torch.cat([layers[:, r[i]:r[i + 1]] for i in perm], dim=1))
    for j, i in enumerate(perm):
        n = clips[i].numel()
        assert torch.equal(pd_[j, :n], dwav[i, :n]), (j, i)


def _equal_step(eng, w, B3, ragged, stochastic):
    """forward, d waveform and one fine-tuning backward over w (3 branches), through either set of entry points."""
    if stochastic:
        eng.train_set_stochastic(dropout=0.1, attention_dropout=0.1, dropout_input=0.1, seed=0x1234567887654321 >> 2, layer_mask=0xFFF)
        eng.train_set_branches([0xFFF & ~(1 << 3), 0xFFF, 0xFFF & ~((1 << 3) | (1 << 11))])
    try:
        if ragged:
            emb, layers, saved, batch = eng.embed_train_ragged(w, [w.shape[1]] * w.shape[0])
        else:
            emb, layers, saved = eng.embed_train(w)
        loss, da, dp, dn = eng.triplet_loss(emb[:B3].contiguous(), emb[B3:2 * B3].contiguous(), emb[2 * B3:].contiguous(), MARGIN)
        demb = torch.cat([da, dp, dn])
        eng.train_zero_grad()
        if ragged:
            eng.train_backward_ragged(batch, layers, saved, demb)
        else:
            eng.train_backward(w, layers, saved, demb)
        grad = eng.train_read(1).clone()
        dwav = None
        if not stochastic:   # (the loss path's backward has no regularisation)
            gl = torch.ones_like(layers) / layers.numel()
            dwav = eng.embed_backward_ragged(batch, layers, saved, gl, demb) if ragged else eng.embed_backward(w, layers, saved, gl, demb)
    finally:
        eng.train_set_branches(None)
        eng.train_set_stochastic()
    return emb.clone(), layers.reshape(12, -1, 768).clone(), grad, dwav, loss.item()


@pytest.mark.parametrize("stochastic", [False, True], ids=["eval", "dropout-layerdrop"])
@pytest.mark.parametrize("T", [35, 130], ids=["T35-fused-attn-bwd", "T130-three-kernels"])
def test_an_equal_length_batch_through_the_ragged_entry_points_has_the_equal_length_bits(teng, T, stochastic):
    B3 = 2
    g = torch.Generator().manual_seed(T)
    w = (0.1 * torch.randn(3 * B3, ref64.n_for(T) + 7, generator=g)).clamp(-1, 1).cuda()
    ref = _equal_step(teng, w, B3, False, stochastic)
    got = _equal_step(teng, w, B3, True, stochastic)
    assert ref[4] > 0 and got[4] == ref[4]
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert torch.equal(got[2], ref[2]), (got[2] - ref[2]).abs().max().item()      # the gradient vector: same rows, same summation order
    assert ref[2].abs().max().item() > 0
    if not stochastic:
        assert torch.equal(got[3], ref[3])
    else:   # the masks did something: the eval-mode embeddings differ
        assert not torch.equal(ref[0], _equal_step(teng, w, B3, False, False)[0])


# ---- 2. the loss path vs float64 --------------------------------------------------------------------------------------------
# The L1 terms make the loss piecewise linear: d|e - c| / de = sign(e - c), and where a difference sits at the forward's own
# rounding level that sign is decided by rounding, not by the backward (tests/test_gpu_backward.py states the same for the
# equal-length path: "elements whose difference sits at the fp32 noise floor flip between implementations").  With the 8.6 million
# layer elements of the batch below a handful of differences lie within 1e-6 of zero, each flip moves one entry of d loss /
# d layers by 2 / (768 M), and the clip it belongs to then differs from float64 by ~1e-3 of its gradient - a thousand e32, no
# error of any kernel (measured: the T = 64 clip at err_gpu / e32 = 1071 against float64's own signs, the loss itself at 0.02 e32).  The kink is taken out of the comparison the way ref64.head_relu_undecided takes the head's ReLU out:
# the engine's own sign pattern G = d loss / d (layers, emb) is (1) held to float64's signs, bit for bit, on every element whose
# float64 difference is at least ref64.KINK away from zero (the undecided rest must be rare), and (2) handed to the float64 oracle as
# the cotangent, so that estimate.grad is compared with J^T G in float64 under ref64's bound - every kernel of the forward and the
# backward is then held to float64, and the L1 backward to exact equality where float64 decides it.
def _ragged_loss_oracle(sd, est, cln, hw, hb, mult):
    """NomadLoss over the concatenation of the clips' valid frames, every clip through the oracle at its exact length (B = 1)
    -> (loss, [12 layer differences (M, 768), embedding difference (B, 256)]: estimate - clean), in the dtype of the arguments."""
    with torch.no_grad():
        oe = [O.lossnet_forward(sd, e[None], hw, hb, feature_grad_mult=mult, required_seq_len_multiple=2) for e in est]
        oc = [O.lossnet_forward(sd, c[None], hw, hb, feature_grad_mult=mult, required_seq_len_multiple=2) for c in cln]
    cat = lambda outs: [torch.cat([o[i][0] if i < 12 else o[i] for o in outs]) for i in range(13)]
    ce, cc = cat(oe), cat(oc)
    return O.nomad_loss(cc, ce), [a - b for a, b in zip(ce, cc)]


def _ragged_cotangent_oracle(sd, clips, hw, hb, Gl, Ge, mult):
    """[d (sum_l <layer_l, Gl[l]> + <emb, Ge>) / d clip] with every clip through the oracle at its exact length; Gl (12, M, 768)
    packed, Ge (B, 256)."""
    r = _rows(LOSS_T)
    return [ref64.lossnet_dwav(sd, w[None], hw, hb, Gl[:, r[i]:r[i + 1]][:, None], Ge[i:i + 1], mult)[0] for i, w in enumerate(clips)]


def _padded(clips):
    n = max(c.numel() for c in clips)
    return torch.stack([F.pad(c, (0, n - c.numel())) for c in clips])[:, None]


def _loss_case(nmd, sd0, c, tag, clean_grad=False):
    est, cln = make_clips(LOSS_T, LOSS_EXTRA, seed=21), make_clips(LOSS_T, LOSS_EXTRA, seed=22)
    lens = [e.numel() for e in est]
    B, M = len(lens), sum(LOSS_T)
    gen = torch.Generator().manual_seed(23)
    hw = (torch.rand(256, 768, generator=gen) * 2 - 1) / 768 ** 0.5
    hb = (torch.rand(256, generator=gen) * 2 - 1) / 768 ** 0.5
    undecided = torch.zeros(768, dtype=torch.bool)
    for w in est + cln:
        undecided |= ref64.head_relu_undecided(sd0, w[None])
    assert int(undecided.sum()) <= 64, int(undecided.sum())
    hw[:, undecided] = 0.0
    eng, mult = nmd.engine, nmd.engine.feature_grad_mult
    r64, r32 = ref64.both(_ragged_loss_oracle, sd0, est, cln, hw, hb, mult=mult)
    head = (hw.cuda(), hb.cuda())
    nmd.lossnet_layers.embedding_weight, nmd.lossnet_layers.embedding_bias = head
    E = _padded(est).cuda().requires_grad_(True)
    Cn = _padded(cln).cuda().requires_grad_(clean_grad)
    loss = nmd.forward(E, Cn, lengths=lens)
    loss.backward()
    # The loss is ONE fp32 number: its e32 is a single draw of rounding noise and can fall below what the format resolves (the fp32
    # oracle's loss lands 2.2e-8 from float64's 8.2025 with 16 CPU threads, 9.3e-7 with another count; half an fp32 ulp is 4.8e-7).
    # ref64.measure's e32_min is for exactly this: the yardstick is at least half an ulp of the fp32 result, the least any fp32
    # computation of this value can promise.
    l64 = r64[0].item()
    half_ulp = float(np.spacing(np.float32(abs(l64)))) / 2
    res = ref64.check(f"{tag} ragged loss value gpu {loss.item():.9g} f64 {l64:.9g}", loss.detach().cpu(), r64[0], r32[0],
                      e32_min={"": half_ulp}, c=c)
    bound = res[""][2]
    for i, n in enumerate(lens):   # exactly zero behind every length
        assert not E.grad[i, 0, n:].any(), i
        if clean_grad:
            assert not Cn.grad[i, 0, n:].any(), i
    # the engine's sign pattern: the same calls Nomad.forward made (deterministic: the same bits, checked through the loss)
    with torch.no_grad():
        e_emb, e_layers, _, _ = eng.embed_train_ragged(E.detach(), lens, head, save=False)
        c_emb, c_layers, _, _ = eng.embed_train_ragged(Cn.detach(), lens, head, save=False)
        assert torch.equal(eng.l1_loss(e_layers, c_layers, e_emb, c_emb), loss.detach())
        Gl, Ge = eng.l1_loss_backward(e_layers, c_layers, e_emb, c_emb, torch.ones(()))
    Gl, Ge = Gl.cpu(), Ge.cpu()
    # (1) float64's signs wherever float64 decides them
    D = torch.stack(r64[1][:12])
    decided = D.abs() >= ref64.KINK
    want = (torch.sign(D) * (1.0 / (M * 768))).float()      # l1_bwd_kernel: (float)(1 / numel) * upstream, by sign
    frac = 1.0 - decided.double().mean().item()
    print(f"F64 {tag} ragged L1 signs: {int((~decided).sum())} of {D.numel()} layer differences within {ref64.KINK:g} of zero")
    assert frac < 1e-3                                        # differences are O(1): 2 KINK x their density at zero ~ 1e-4
    assert torch.equal(Gl[decided], want[decided])
    De = r64[1][12]
    dec_e = De.abs() >= ref64.KINK
    assert dec_e.double().mean().item() > 0.98
    assert torch.equal(Ge[dec_e], (torch.sign(De) * (1.0 / (B * 256))).float()[dec_e])
    # (2) estimate.grad (and clean.grad) against J^T G in float64
    g64, g32 = ref64.both(_ragged_cotangent_oracle, sd0, est, hw, hb, Gl, Ge, mult=mult)
    got = {f"dest{i}": E.grad[i, 0, :n].cpu() for i, n in enumerate(lens)}
    want64 = {f"dest{i}": g for i, g in enumerate(g64)}
    want32 = {f"dest{i}": g for i, g in enumerate(g32)}
    if clean_grad:   # |e - c| is symmetric: the clean side's cotangent is the negated pattern
        with torch.no_grad():
            Hl, He = eng.l1_loss_backward(c_layers, e_layers, c_emb, e_emb, torch.ones(()))
        assert torch.equal(Hl.cpu(), -Gl) and torch.equal(He.cpu(), -Ge)
        h64, h32 = ref64.both(_ragged_cotangent_oracle, sd0, cln, hw, hb, -Gl, -Ge, mult=mult)
        got.update({f"dcln{i}": Cn.grad[i, 0, :n].cpu() for i, n in enumerate(lens)})
        want64.update({f"dcln{i}": g for i, g in enumerate(h64)})
        want32.update({f"dcln{i}": g for i, g in enumerate(h32)})
    ref64.check(f"{tag} ragged loss path T={LOSS_T} clean_grad={clean_grad}", got, want64, want32, c=c)
    # the argument is honoured: the padded, equal-length loss on the same tensors is another number
    with torch.no_grad():
        padded = nmd.forward(E.detach(), Cn.detach()).item()
    print(f"F64 {tag} padded loss {padded:.9g}: |padded - exact| / bound = {abs(padded - l64) / bound:.3g}")
    assert abs(padded - l64) >= 100 * bound


def test_nomad_forward_with_lengths_vs_float64(built_lib, sd0):
    from nomad_amd.nomad import Nomad
    nmd = Nomad(weights=sd0)
    try:
        _loss_case(nmd, sd0, ref64.C, "fp32")
        _loss_case(nmd, sd0, ref64.C, "fp32", clean_grad=True)
    finally:
        nmd.engine.close()


def test_nomad_forward_with_lengths_bf16x3_vs_float64(built_lib, sd0):
    from nomad_amd.nomad import Nomad
    from test_gpu_forward_f64 import C_X3P
    nmd = Nomad(weights=sd0, precision="bf16x3")
    try:
        _loss_case(nmd, sd0, C_X3P, "bf16x3")
    finally:
        nmd.engine.close()


def test_lossnet_layers_with_lengths_and_graphed_loss(built_lib, sd0):
    from nomad_amd.nomad import Nomad
    nmd = Nomad(weights=sd0)
    try:
        clips = make_clips(LOSS_T, LOSS_EXTRA, seed=31)
        lens = [c.numel() for c in clips]
        outs = nmd.lossnet_layers(_padded(clips).cuda(), lengths=torch.tensor(lens))
        assert len(outs) == 13 and all(o.shape == (sum(LOSS_T), 768) for o in outs[:12]) and outs[12].shape == (5, 256)
        r = _rows(LOSS_T)
        for c, clip in enumerate(clips):   # outside fine-tuning mode too the ragged forward never splits K: the scoring path's values
            one = nmd.lossnet_layers(clip[None, None].cuda(), lengths=[lens[c]])
            assert torch.equal(one[11], outs[11][r[c]:r[c + 1]]) and torch.equal(one[12][0], outs[12][c])
        with pytest.raises(ValueError, match="ONE batch shape"):
            nmd.graphed_loss(_padded(clips).cuda(), _padded(clips).cuda(), lengths=lens)
    finally:
        nmd.engine.close()


# ---- 3. the fine-tuning step vs float64 --------------------------------------------------------------------------------------
class PackedStochastic(O.Stochastic):
    """The engine's masks for ONE clip of a ragged batch, restated: element indices are those of the packed tensors - an
    activation site indexes [M][768], so clip c's (1, T_c, 768) block starts at element 768 * sum_{j<c} T_j; the attention
    probabilities of clip c are the [12][T_c][T_c] block at 12 * sum_{j<c} T_j^2."""

    def __init__(self, row0, attn0, **kw):
        super().__init__(**kw)
        self.row0, self.attn0 = int(row0), int(attn0)

    def mult(self, site, shape, p):
        p32 = np.float32(p)
        if p32 <= 0:
            return torch.ones(tuple(shape))
        attn = site >= 2 and (site - 2) % 3 == 0
        first = self.attn0 if attn else self.row0 * 768
        t = float(p32) * 4294967296.0
        threshold = np.uint32(4294967295 if t >= 4294967295.0 else int(t + 0.5))
        idx = np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(first)
        lo, hi = np.uint32(self.seed & 0xFFFFFFFF), np.uint32((self.seed >> 32) & 0xFFFFFFFF)
        with np.errstate(over="ignore"):
            h = self._fmix32(idx.astype(np.uint32) ^ lo ^ np.uint32((site * 0x9E3779B9) & 0xFFFFFFFF))
            h = self._fmix32(h + (idx >> np.uint64(32)).astype(np.uint32) * np.uint32(0x85EBCA77) + hi)
        scale = np.float32(1.0) / (np.float32(1.0) - p32)
        return torch.from_numpy(np.where(h >= threshold, scale, np.float32(0)).astype(np.float32).reshape(tuple(shape)))


STEP_T = [[1, 64, 499], [2, 65, 130], [35, 57, 200]]      # anchor | positive | negative: 9 clips
STEP_EXTRA = [[0, 111, 301], [150, 163, 5], [37, 251, 83]]


def _step_clips(seed):
    return [make_clips(t, e, seed + i) for i, (t, e) in enumerate(zip(STEP_T, STEP_EXTRA))]


def _ragged_step_oracle(sd, clips, stochs=None, freeze_all=False):
    """Every clip through the oracle at its exact length, the triplet loss over the concatenated embeddings, autograd to the
    trainable parameters -> (loss, embeddings (3B, 256), {key: gradient})."""
    sd, keys = ref64._live(sd, True)
    flat = [c for br in clips for c in br]
    st = stochs if stochs is not None else [None] * len(flat)
    e = torch.cat([O.triplet_forward(sd, c[None], s, 1.0) for c, s in zip(flat, st)])
    B = len(clips[0])
    loss = torch.nn.TripletMarginLoss(margin=MARGIN)(e[:B], e[B:2 * B], e[2 * B:])
    if freeze_all:
        keys = [k for k in keys if "encoder" not in k]
    grads = torch.autograd.grad(loss, [sd[k] for k in keys], allow_unused=True)
    return loss.detach(), e.detach(), {k: (g if g is not None else torch.zeros_like(sd[k])) for k, g in zip(keys, grads)}


def _engine_step(eng, clips, reg=None, masks=None):
    flat = [c.cuda() for br in clips for c in br]
    B = len(clips[0])
    if reg is not None:
        eng.train_set_stochastic(**reg)
        eng.train_set_branches(masks)
    try:
        emb, layers, saved, batch = eng.embed_train_ragged(flat)
        loss, da, dp, dn = eng.triplet_loss(emb[:B].contiguous(), emb[B:2 * B].contiguous(), emb[2 * B:].contiguous(), MARGIN)
        eng.train_zero_grad()
        eng.train_backward_ragged(batch, layers, saved, torch.cat([da, dp, dn]))
    finally:
        eng.train_set_branches(None)
        eng.train_set_stochastic()
    return loss.cpu().reshape(()), emb.cpu(), eng.train_unflatten(eng.train_read(1))


def _check_step(case, got, r64, r32, c=ref64.C):
    """test_gpu_train_mode_f64's comparison as it is: every hinge active in float64; embeddings and loss as one group (the loss,
    one scalar, with the embeddings' e32 as its least yardstick), the gradients as another; ref64's constants only."""
    import test_gpu_train_mode_f64 as TM
    TM._assert_active(case, r64)
    TM._compare(case, got, r64, r32, c=c)


def test_merged_ragged_step_eval_mode_vs_float64(teng, xeng, sd_train):
    from test_gpu_forward_f64 import C_X3P
    clips = _step_clips(41)
    r64, r32 = ref64.both(_ragged_step_oracle, sd_train, clips)
    _check_step(f"ragged train eval T={STEP_T}", _engine_step(teng, clips), r64, r32)
    _check_step(f"x3 ragged train eval T={STEP_T}", _engine_step(xeng, clips), r64, r32, c=C_X3P)


def test_merged_ragged_step_freeze_all_vs_float64(teng, sd_train):
    clips = _step_clips(43)
    r64, r32 = ref64.both(_ragged_step_oracle, sd_train, clips, freeze_all=True)
    teng.train_set_frozen(True)
    try:
        got = _engine_step(teng, clips)
    finally:
        teng.train_set_frozen(False)
    _check_step(f"ragged train freeze_all T={STEP_T}", got, r64, r32)
    frozen = [k for k in got[2] if "encoder" in k and "feature_extractor" not in k]
    assert frozen and all(not got[2][k].any() for k in frozen)


def test_merged_ragged_step_train_mode_vs_float64(teng, sd_train):
    """Dropout at every site + LayerDrop per branch, the masks restated by PackedStochastic.  First, as
    test_gpu_train_mode_f64.py does (its _assert_active / _assert_discriminates, its rate limits): every hinge is active, every
    site in use drops between 0.8 p and 1.2 p of the packed tensor it indexes, and the float64 oracle with every clip's masks
    moved to the next clip's offsets misses the bound 100-fold in the embeddings and in every fc2 / out_proj weight gradient of a
    layer that runs - the test can tell the packed indexing from another one.  Then the engine."""
    import test_gpu_train_mode_f64 as TM
    clips = _step_clips(47)
    P = 0.1
    seed = 0x0123456789ABCDEF >> 2
    masks = [0xFFF & ~(1 << 2), 0xFFF, 0xFFF & ~((1 << 2) | (1 << 9))]
    TM._assert_layerdrop([masks[0], masks[2]])
    Ts = [t for br in STEP_T for t in br]
    r = _rows(Ts)
    a = np.concatenate([[0], np.cumsum([12 * t * t for t in Ts])]).tolist()
    kw = dict(seed=seed, dropout=P, attention_dropout=P, dropout_input=P)

    def stochs(shift=0):
        return [PackedStochastic(r[(i + shift) % len(Ts)], a[(i + shift) % len(Ts)], layer_mask=masks[i // 3], **kw) for i in range(len(Ts))]

    case = f"ragged train mode T={STEP_T} masks={[hex(x) for x in masks]}"
    whole = PackedStochastic(0, 0, layer_mask=0xFFF, **kw)      # the packed tensors as the engine indexes them: [M][768], 12 sum T_c^2
    for site, kind, p in TM._sites(whole, 0xFFF):
        rate = (whole.mult(site, (r[-1], 768) if kind == "row" else (a[-1],), p) == 0).float().mean().item()
        assert 0.8 * p <= rate <= 1.2 * p, (site, kind, rate)
    r64, r32 = ref64.both(_ragged_step_oracle, sd_train, clips, stochs=stochs())
    TM._assert_active(case, r64)
    moved = _ragged_step_oracle(*ref64.cast((sd_train, clips), torch.float64), stochs=stochs(1))
    TM._assert_discriminates(case, r64, r32, moved, masks)
    reg = dict(dropout=P, attention_dropout=P, dropout_input=P, seed=seed, layer_mask=0xFFF)
    _check_step(case, _engine_step(teng, clips, reg, masks), r64, r32)


def test_three_adam_steps_on_ragged_gradients(built_lib, sd_train):
    """Three fine-tuning steps over the mixed ragged batch: nomad_train_backward_ragged's gradient vector, then nomad_train_adam_step,
    against torch.optim.Adam in float64 and fp32 fed the same gradient (test_gpu_train_mode_f64._adam_compare and its bound:
    parameters and both moments after every step; the frozen extractor's slices keep their bits and zero moments).  The step after
    an update runs on the updated weights: at the end the ragged forward is the float64 oracle's on train_state_dict()."""
    import test_gpu_train_mode_f64 as TM
    eng = _engine(sd_train)
    try:
        total, head = eng.train_param_count()
        p0 = eng.train_read(0).cpu()
        t64, t32 = TM._TorchAdam(p0, head, torch.float64), TM._TorchAdam(p0, head, torch.float32)
        always_zero = torch.ones(total, dtype=torch.bool)
        for step in (1, 2, 3):
            clips = _step_clips(60 + step)
            loss, emb, _ = _engine_step(eng, clips)
            assert loss.item() > 0
            g = eng.train_read(1).cpu()
            assert torch.isfinite(g).all() and (g != 0).sum().item() > total // 2
            always_zero &= g == 0
            t64.step(g)
            t32.step(g)
            eng.adam_step(TM.LR_BODY, TM.LR_HEAD)
            TM._adam_compare(f"adam step {step} on ragged gradients", eng, t64, t32, always_zero, p0)
        assert always_zero.sum().item() > total // 100            # the frozen conv feature extractor
        new_sd = eng.train_state_dict()
        flat = [c for br in _step_clips(64) for c in br]
        with torch.no_grad():
            e64, e32 = ref64.both(lambda sd, ws: torch.cat([O.triplet_forward(sd, w[None]) for w in ws]), new_sd, flat)
        got = eng.embed_train_ragged([c.cuda() for c in flat])[0].cpu()
        ref64.check("ragged forward after the adam steps", got, e64, e32)
    finally:
        eng.close()


# ---- 4. Training(pad_mode="exact") -------------------------------------------------------------------------------------------
def _toy(tmp_path):
    from test_gpu_train import _config, _write_wav
    import pandas as pd
    rng = np.random.RandomState(1)
    rows = []
    for i in range(6):
        names = {}
        for j, (role, noise) in enumerate((("Anchor", 0.0), ("Positive", 0.01), ("Negative", 0.2))):
            base = 0.1 * rng.randn(5000 + 1900 * ((i + j) % 4) + 37 * i)      # every file its own length
            name = f"/{role}_{i}.wav"
            _write_wav(str(tmp_path) + name, base + noise * rng.randn(base.size))
            names[role] = name
        rows.append(dict(db=1 + i % 2, **names))
    csv = str(tmp_path / "triplets.csv")
    pd.DataFrame(rows).to_csv(csv, index=False)
    return csv, _config


NO_REG = dict(dropout=0.0, attention_dropout=0.0, dropout_input=0.0, encoder_layerdrop=0.0)


def test_training_with_exact_lengths(tmp_path):
    from nomad_amd.train import Training
    csv, _config = _toy(tmp_path)
    with pytest.raises(ValueError, match="freeze_convnet"):
        Training(_config(tmp_path, csv, pad_mode="exact", freeze_convnet=False))
    with pytest.raises(ValueError, match="pad_mode"):
        Training(_config(tmp_path, csv, pad_mode="longest"))
    tr = Training(_config(tmp_path, csv, pad_mode="exact", num_epochs=1))
    try:
        (A, la), (P, lp), (N, ln) = next(iter(tr.valid_loader))
        assert A.shape == P.shape == N.shape and A.shape[:2] == (3, 1) and len(set(la.tolist() + lp.tolist() + ln.tolist())) > 3
        # validation = the triplet loss over embed_ragged embeddings, bit for bit
        clips = [w[0, :n].cuda() for W, L in ((A, la), (P, lp), (N, ln)) for w, n in zip(W, L.tolist())]
        e = tr.engine.embed_ragged(clips)
        want = tr.engine.triplet_loss(e[:3].contiguous(), e[3:6].contiguous(), e[6:].contiguous(), tr.margin, want_grad=False)[0]
        got = tr.train_step((A, la), (P, lp), (N, ln), training=False)
        assert torch.equal(got, want)
        before = tr.engine.train_read(0).clone()
        train_loss = tr.train()
        valid_loss = tr.eval()
        assert np.isfinite(train_loss) and np.isfinite(valid_loss) and train_loss > 0
        assert not torch.equal(tr.engine.train_read(0), before)
    finally:
        tr.engine.close()


def test_training_pad_mode_batch_is_the_padded_step(tmp_path):
    """pad_mode "batch" (spelled out) on files of different lengths == the padded train_step called directly, as the existing
    tests call it: loss and parameters after one step, bit for bit."""
    from nomad_amd.train import Training, TripletDataset
    csv, _config = _toy(tmp_path)
    out = []
    for cfg in (_config(tmp_path, csv, pad_mode="batch"), _config(tmp_path, csv)):
        tr = Training(cfg, regularisation=NO_REG)
        try:
            A, P, N = next(iter(tr.valid_loader))
            assert torch.is_tensor(A) and A.dim() == 3
            if "pad_mode" not in cfg:   # the step on hand-padded tensors
                rows = [tr.valid_set[i] for i in range(3)]
                A, P, N = (TripletDataset.zero_pad_wav([r[k] for r in rows]) for k in range(3))
            loss = tr.train_step(A, P, N)
            out.append((loss.clone(), tr.engine.train_read(0).clone()))
        finally:
            tr.engine.close()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---- 5. ABI errors and poison ------------------------------------------------------------------------------------------------
def _abi_setup(eng, clips, guards=None, poison=False):
    """Buffers of exactly the sizes the library asks for (inside guards, NaN-filled when asked) for one ragged forward + backward."""
    lib, ctx = eng.lib, eng.ctx
    B = len(clips)
    lens = [c.numel() for c in clips]
    stride = max(lens) + 5
    arr = (C.c_int * B)(*lens)
    M = sum(num_frames(n) for n in lens)
    n = C.c_size_t()
    sizes = {}
    for name in ("nomad_workspace_bytes_ragged", "nomad_saved_bytes_ragged", "nomad_backward_workspace_bytes_ragged",
                 "nomad_train_workspace_bytes_ragged"):
        assert getattr(lib, name)(ctx, B, arr, C.byref(n)) == 0, lib.nomad_last_error()
        sizes[name] = n.value

    def buf(shape, name, dtype=torch.float32):
        if guards is None:
            t = torch.empty(shape, dtype=dtype, device="cuda")
        else:
            t = guards.empty(shape, dtype, "cuda", name=name)
        if poison:
            t.view(-1).view(torch.uint8).fill_(0xFF)      # NaN as floats
        return t

    wav = torch.zeros(B, stride, device="cuda")
    for i, c in enumerate(clips):
        wav[i, :lens[i]] = c.cuda()
        wav[i, lens[i]:] = float("nan")                   # never read
    d = dict(B=B, lens=lens, stride=stride, arr=arr, M=M, wav=wav, sizes=sizes,
             emb=buf((B, 256), "emb"), layers=buf((12, M, 768), "layers"),
             saved=buf((sizes["nomad_saved_bytes_ragged"],), "saved", torch.uint8),
             ws=buf((sizes["nomad_workspace_bytes_ragged"],), "fwd workspace", torch.uint8),
             bws=buf((sizes["nomad_backward_workspace_bytes_ragged"],), "bwd workspace", torch.uint8),
             tws=buf((sizes["nomad_train_workspace_bytes_ragged"],), "train workspace", torch.uint8),
             dwav=buf((B, stride), "dwav"), dlayers=buf((12, M, 768), "dlayers"), demb=buf((B, 256), "demb"),
             loss=buf((1,), "loss"), scratch=buf((lib.nomad_l1_scratch_bytes(),), "l1 scratch", torch.uint8))
    return d


def _fwd_args(eng, d, **over):
    a = dict(wav=d["wav"].data_ptr(), B=d["B"], stride=d["stride"], arr=d["arr"], emb=d["emb"].data_ptr(), layers=d["layers"].data_ptr(),
             saved=d["saved"].data_ptr(), saved_bytes=d["saved"].numel(), ws=d["ws"].data_ptr(), ws_bytes=d["ws"].numel())
    a.update(over)
    return (eng.ctx, a["wav"], a["B"], a["stride"], a["arr"], None, None, a["emb"], a["layers"], a["saved"], a["saved_bytes"], a["ws"],
            a["ws_bytes"], None)


def _bwd_args(eng, d, **over):
    a = dict(wav=d["wav"].data_ptr(), B=d["B"], stride=d["stride"], arr=d["arr"], layers=d["layers"].data_ptr(), saved=d["saved"].data_ptr(),
             saved_bytes=d["saved"].numel(), dlayers=d["dlayers"].data_ptr(), demb=d["demb"].data_ptr(), dwav=d["dwav"].data_ptr(),
             ws=d["bws"].data_ptr(), ws_bytes=d["bws"].numel())
    a.update(over)
    return (eng.ctx, a["wav"], a["B"], a["stride"], a["arr"], None, None, a["layers"], a["saved"], a["saved_bytes"], a["dlayers"], a["demb"],
            a["dwav"], a["ws"], a["ws_bytes"], None)


def _train_args(eng, d, **over):
    a = dict(B=d["B"], arr=d["arr"], saved_bytes=d["saved"].numel(), ws_bytes=d["tws"].numel())
    a.update(over)
    return (eng.ctx, d["wav"].data_ptr(), a["B"], d["stride"], a["arr"], d["layers"].data_ptr(), d["saved"].data_ptr(), a["saved_bytes"],
            d["demb"].data_ptr(), d["tws"].data_ptr(), a["ws_bytes"], None)


SMALL_T, SMALL_EXTRA = [1, 2, 64, 65, 130, 35], [0, 150, 111, 163, 5, 37]


def test_ragged_argument_errors_return_their_status_and_write_nothing(teng):
    lib, INV, WSP = teng.lib, _lib.NOMAD_ERR_INVALID, _lib.NOMAD_ERR_WORKSPACE
    clips = make_clips(SMALL_T, SMALL_EXTRA, seed=51)
    d = _abi_setup(teng, clips)
    for k in ("emb", "layers", "dwav", "dlayers", "demb"):
        d[k].fill_(7.0)
    for k in ("saved", "ws", "bws", "tws"):
        d[k].fill_(7)
    short = (C.c_int * d["B"])(*([d["stride"] + 1] + d["lens"][1:]))        # a clip longer than the stride
    tiny = (C.c_int * d["B"])(*([399] + d["lens"][1:]))                     # below the receptive field
    fwd, bwd, trn = lib.nomad_embed_train_ragged, lib.nomad_embed_backward_ragged, lib.nomad_train_backward_ragged
    assert fwd(*_fwd_args(teng, d, wav=None)) == INV
    assert fwd(*_fwd_args(teng, d, layers=None)) == INV
    assert fwd(*_fwd_args(teng, d, arr=None)) == INV
    assert fwd(*_fwd_args(teng, d, B=0)) == INV
    assert fwd(*_fwd_args(teng, d, saved=None)) == INV                      # a size without a block
    assert fwd(*_fwd_args(teng, d, arr=tiny)) == INV
    assert fwd(*_fwd_args(teng, d, arr=short)) == INV and b"longer than the row stride" in lib.nomad_last_error()
    assert fwd(*_fwd_args(teng, d, ws_bytes=d["ws"].numel() - 1)) == WSP
    assert fwd(*_fwd_args(teng, d, saved_bytes=d["saved"].numel() - 1)) == WSP and b"saved block" in lib.nomad_last_error()
    assert bwd(*_bwd_args(teng, d, dwav=None)) == INV
    assert bwd(*_bwd_args(teng, d, demb=None)) == INV
    assert bwd(*_bwd_args(teng, d, arr=short)) == INV
    assert bwd(*_bwd_args(teng, d, ws_bytes=d["bws"].numel() - 1)) == WSP
    assert bwd(*_bwd_args(teng, d, saved_bytes=d["saved"].numel() - 1)) == WSP
    assert trn(*_train_args(teng, d, ws_bytes=d["tws"].numel() - 1)) == WSP
    assert trn(*_train_args(teng, d, arr=None)) == INV
    n = C.c_size_t()
    for name in ("nomad_saved_bytes_ragged", "nomad_backward_workspace_bytes_ragged", "nomad_train_workspace_bytes_ragged"):
        assert getattr(lib, name)(teng.ctx, d["B"], tiny, C.byref(n)) == INV
        assert getattr(lib, name)(teng.ctx, d["B"], None, C.byref(n)) == INV
    # B % branches != 0: 6 clips, 4 branches
    teng.train_set_branches([0xFFF] * 4)
    try:
        assert fwd(*_fwd_args(teng, d)) == INV and b"equal branches" in lib.nomad_last_error()
        assert trn(*_train_args(teng, d)) == INV and b"equal branches" in lib.nomad_last_error()
    finally:
        teng.train_set_branches(None)
    # a trainable conv feature extractor with a ragged call
    teng.train_set_convnet(True)
    try:
        assert fwd(*_fwd_args(teng, d)) == INV and b"equal-length" in lib.nomad_last_error()
        assert trn(*_train_args(teng, d)) == INV and b"equal-length" in lib.nomad_last_error()
    finally:
        teng.train_set_convnet(False)
    sc = d["scratch"].data_ptr()
    assert lib.nomad_l1_loss_ragged(teng.ctx, d["layers"].data_ptr(), d["layers"].data_ptr(), d["emb"].data_ptr(), d["emb"].data_ptr(),
                                    d["M"], 0, d["loss"].data_ptr(), sc, None) == INV
    assert lib.nomad_l1_loss_ragged(teng.ctx, None, d["layers"].data_ptr(), d["emb"].data_ptr(), d["emb"].data_ptr(),
                                    d["M"], d["B"], d["loss"].data_ptr(), sc, None) == INV
    assert lib.nomad_l1_loss_backward_ragged(teng.ctx, d["layers"].data_ptr(), d["layers"].data_ptr(), d["emb"].data_ptr(), d["emb"].data_ptr(),
                                             d["M"], d["B"], None, d["dlayers"].data_ptr(), d["demb"].data_ptr(), None) == INV
    torch.cuda.synchronize()
    for k in ("emb", "layers", "dwav", "dlayers", "demb"):                  # nothing was written
        assert bool((d[k] == 7.0).all()), k
    for k in ("saved", "ws", "bws", "tws"):
        assert bool((d[k] == 7).all()), k
    # and the context still works
    assert fwd(*_fwd_args(teng, d)) == 0, lib.nomad_last_error()
    torch.cuda.synchronize()
    assert torch.equal(d["emb"], teng.embed_ragged([c.cuda() for c in clips]))


def test_ragged_entry_points_read_only_what_they_wrote_and_stay_inside_their_buffers(teng):
    """Workspaces, saved block, outputs and dwav pre-filled with NaN inside guarded buffers: finite results, the bits of a
    clean run, nothing written outside, dwav behind the lengths 0 (not NaN)."""
    lib = teng.lib
    clips = make_clips(SMALL_T, SMALL_EXTRA, seed=53)
    ref = teng.embed_train_ragged([c.cuda() for c in clips])
    g = torch.Generator().manual_seed(54)
    other_emb = torch.randn(len(clips), 256, generator=g).cuda()
    other_layers = ref[1] + 0.01 * torch.randn(ref[1].shape, generator=g).cuda()
    guards = guard.Guards()
    d = _abi_setup(teng, clips, guards, poison=True)
    assert lib.nomad_embed_train_ragged(*_fwd_args(teng, d)) == 0, lib.nomad_last_error()
    assert torch.equal(d["emb"], ref[0]) and torch.equal(d["layers"], ref[1])
    up = torch.ones(1, device="cuda")
    assert lib.nomad_l1_loss_ragged(teng.ctx, d["layers"].data_ptr(), other_layers.data_ptr(), d["emb"].data_ptr(), other_emb.data_ptr(),
                                    d["M"], d["B"], d["loss"].data_ptr(), d["scratch"].data_ptr(), None) == 0
    assert lib.nomad_l1_loss_backward_ragged(teng.ctx, d["layers"].data_ptr(), other_layers.data_ptr(), d["emb"].data_ptr(),
                                             other_emb.data_ptr(), d["M"], d["B"], up.data_ptr(), d["dlayers"].data_ptr(),
                                             d["demb"].data_ptr(), None) == 0
    want = sum(F.l1_loss(d["layers"][i], other_layers[i]) for i in range(12)) + F.l1_loss(d["emb"], other_emb)
    assert torch.isfinite(d["loss"]).all() and abs(d["loss"].item() - want.item()) < 1e-5 * want.item()
    assert torch.isfinite(d["dlayers"]).all() and torch.isfinite(d["demb"]).all()
    assert lib.nomad_embed_backward_ragged(*_bwd_args(teng, d)) == 0, lib.nomad_last_error()
    assert torch.isfinite(d["dwav"]).all()
    for i, n in enumerate(d["lens"]):
        assert not d["dwav"][i, n:].any(), i
        assert d["dwav"][i, :n].abs().max().item() > 0, i
    clean = teng.embed_backward_ragged(ref[3], ref[1], ref[2], d["dlayers"], d["demb"])
    assert torch.equal(clean[:, :max(d["lens"])], d["dwav"][:, :max(d["lens"])])
    total, _ = teng.train_param_count()
    teng.train_write(1, torch.full((total,), float("nan"), device="cuda"))
    teng.train_zero_grad()
    assert lib.nomad_train_backward_ragged(*_train_args(teng, d)) == 0, lib.nomad_last_error()
    grad = teng.train_read(1)
    assert torch.isfinite(grad).all() and grad.abs().max().item() > 0
    # the forward without a saved block: layer outputs only
    d2 = _abi_setup(teng, clips, guards, poison=True)
    assert lib.nomad_embed_train_ragged(*_fwd_args(teng, d2, saved=None, saved_bytes=0)) == 0, lib.nomad_last_error()
    assert torch.equal(d2["emb"], ref[0]) and torch.equal(d2["layers"], ref[1])
    guards.check("ragged gradient entry points")
