"""GPU: the backward kernels and the loss path's d loss / d waveform against float64, with plain fp32 as the yardstick
(tests/ref64.py: err_gpu <= 8 e32 + 1e-7 top).  test_gpu_backward.py compares the same entry points against fp32 at
1e-3 / 5e-5 relative; this file checks them at the precision fp32 arithmetic actually has, at the shapes and across the
batch- and length-dependent switches where a kernel goes wrong:

* attention backward (diag_attention_bwd) over T = 1 .. 499 - the fused kernel (T <= 64) and the three-kernel path with
  its partial last tile - with mild and peaky logits and a forced late rescale;
* LayerNorm backward (diag_layernorm_bwd) over M = 1 .. 11976 rows, with rows of mean^2 / var = 1e4 and constant rows;
* embed_train + embed_backward at configs[4]'s shape (32 x 16384) and on both sides of every split-K switch of the
  loss path: the dense GEMMs split while ceil(M / 64) * N / 64 < 512 (M <= 640 for fc1, N = 3072; M <= 896 for the
  QKV GEMM, N = 2304; M <= 2688 for N = 768) and the pos-conv while its 4 x M x 768 partials fit the split-K block
  (M <= 2730; its tile count would allow M <= 3840)."""
import pytest
import torch
import torch.nn.functional as F

import ref64
from nomad_amd.weights import num_frames

pytestmark = pytest.mark.gpu


# ---- attention backward -------------------------------------------------------------------------------------------------
def _attention(qkv, dctx, B, T):
    """ctx = softmax(q k^T) v per head (q arrives pre-scaled, as in the engine), lse, and d <ctx, dctx> / d qkv."""
    qkv = qkv.clone().requires_grad_(True)
    q, k, v = (qkv[:, i * 768:(i + 1) * 768].view(B, T, 12, 64).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2)
    ctx = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * T, 768)
    (d,) = torch.autograd.grad((ctx * dctx).sum(), qkv)
    lse = torch.logsumexp(s, -1).reshape(B * 12, T)
    return {"out": ctx.detach(), "lse": lse.detach(), "dq": d[:, :768], "dk": d[:, 768:1536], "dv": d[:, 1536:]}


def _attention_lse_form(qkv, dctx, B, T):
    """The kernels' formulation of the same values, written out: probabilities recomputed as exp(s - lse), and the softmax
    backward's row term as D = rowsum(dctx * out) instead of autograd's sum_j p_j dP_j."""
    q, k, v = (qkv[:, i * 768:(i + 1) * 768].view(B, T, 12, 64).transpose(1, 2) for i in range(3))
    do = dctx.view(B, T, 12, 64).transpose(1, 2)
    s = q @ k.transpose(-1, -2)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    ds = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
    flat = lambda t: t.transpose(1, 2).reshape(B * T, 768)  # noqa: E731
    return {"out": flat(o), "lse": lse.reshape(B * 12, T), "dq": flat(ds @ k), "dk": flat(ds.transpose(-1, -2) @ q),
            "dv": flat(p.transpose(-1, -2) @ do)}


def _attention_case(engine, qkv, dctx, B, T, case):
    """Yardstick: per tensor, the larger fp32 error of the two formulations (ref64's docstring).  dq / dk also get the
    first-order rounding of the kernels' row term, u * max_rows sum_d |dctx * out| * max |k| (resp. |q|): dP_j and D are
    two different fp32 dot products of the same row, so dS = p (dP - D) keeps their rounding difference even where the
    exact value is 0.  Autograd's form cancels exactly for a one-hot row (T = 1: its e32 is 0 for dq / dk); against it
    alone the GPU measured 7-73x the floor there and 10x e32 at T = 2 with gain 8, while every longer clip stayed within
    7.5x e32 without this term."""
    r64, r32 = ref64.both(_attention, qkv, dctx, B, T)
    r32b = _attention_lse_form(qkv, dctx, B, T)
    r32 = {k: max((r32[k], r32b[k]), key=lambda t: (t.double() - r64[k]).abs().max().item()) for k in r64}
    dabs = (dctx.abs().double() * r64["out"].abs()).view(B * T, 12, 64).sum(-1).max().item()
    e_row = {"dq": 2.0 ** -24 * dabs * qkv[:, 768:1536].abs().max().item(), "dk": 2.0 ** -24 * dabs * qkv[:, :768].abs().max().item()}
    out, lse, dqkv = engine.diag_attention_bwd(qkv.cuda(), dctx.cuda(), B, T)
    got = {"out": out, "lse": lse, "dq": dqkv[:, :768], "dk": dqkv[:, 768:1536], "dv": dqkv[:, 1536:]}
    assert all(torch.isfinite(t).all() for t in got.values())
    # out / lse are values, dq / dk / dv one gradient: each group gets the floor of its own largest entry
    ref64.check(case + " fwd", {k: got[k] for k in ("out", "lse")}, {k: r64[k] for k in ("out", "lse")},
                {k: r32[k] for k in ("out", "lse")})
    ref64.check(case + " bwd", {k: got[k] for k in ("dq", "dk", "dv")}, {k: r64[k] for k in ("dq", "dk", "dv")},
                {k: r32[k] for k in ("dq", "dk", "dv")}, e_row)


@pytest.mark.parametrize("gain", [1.0, 8.0])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 17, 63, 64, 65, 127, 128, 129, 149, 199, 499])
def test_attention_backward_vs_float64(engine, T, B, gain):
    """Both backward forms (one fused launch for T <= 64, rowdot + dkv + dq over 64-row tiles above) and the forward's
    out / lse that the backward recomputes its probabilities from; gain 8 makes the softmax peaky (logit std ~16)."""
    g = torch.Generator().manual_seed(1000 * T + 10 * B + int(gain))
    qkv = torch.randn(B * T, 2304, generator=g) * 0.5
    qkv[:, :768] *= gain
    dctx = torch.randn(B * T, 768, generator=g)
    _attention_case(engine, qkv, dctx, B, T, f"attention B={B} T={T} gain={gain:g}")


@pytest.mark.parametrize("T", [129, 499])
def test_attention_backward_with_a_late_rescale(engine, T):
    """One query row whose maximum logit sits on the clip's last key - inside the last, partial key tile - 30 above the
    rest of the row: the forward's running max is overtaken at the very end (rescale by ~e^-30) and the backward's
    lse-recomputed probabilities of that row are a near one-hot."""
    B = 2
    g = torch.Generator().manual_seed(77 + T)
    qkv = torch.randn(B * T, 2304, generator=g) * 0.5
    dctx = torch.randn(B * T, 768, generator=g)
    for b, h, r in ((1, 7, 3), (0, 0, T - 1), (1, 11, T // 2)):
        q = qkv[b * T + r, 64 * h:64 * h + 64]
        kl = qkv[b * T + T - 1, 768 + 64 * h:768 + 64 * h + 64]
        kl += q * (30.0 / q.dot(q))                     # logit of (r, T - 1) raised by exactly 30
    _attention_case(engine, qkv, dctx, B, T, f"attention late rescale B={B} T={T}")


# ---- LayerNorm backward -------------------------------------------------------------------------------------------------
def _layernorm_dx(x, up, gamma):
    x = x.clone().requires_grad_(True)
    y = F.layer_norm(x, (x.shape[1],), gamma, torch.zeros_like(gamma), 1e-5)
    (dx,) = torch.autograd.grad((y * up).sum(), x)
    return dx


@pytest.mark.parametrize("N", [512, 768])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 17, 1600, 11976])
def test_layernorm_backward_vs_float64(engine, M, N):
    """Four rows per workgroup, so M = 1, 3, 5, 17 leave a partial last block; configs[4]'s 1600 rows and the reference
    training step's 11976.  Every fifth row has mean^2 / var = 1e4 (a large offset the mean must remove before the
    variance); the last row is constant (var = 0: xhat = 0 and only the eps keeps rstd finite)."""
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.randn(M, N, generator=g) * 2 + 0.3
    x[::5] = torch.randn(x[::5].shape, generator=g) * 0.5 + 50.0
    if M > 1:
        x[-1] = 0.75
    gamma = 1 + 0.1 * torch.randn(N, generator=g)
    # an upstream gradient correlated with xhat, as a real one is: the mean(gg * xhat) term is then of the size of gg itself
    xc = x - x.mean(1, keepdim=True)
    up = torch.randn(M, N, generator=g) + 2 * xc / xc.std(1, keepdim=True).clamp_min(1e-3)
    r64, r32 = ref64.both(_layernorm_dx, x, up, gamma)
    dx = engine.diag_layernorm_bwd(x.cuda(), up.cuda(), gamma.cuda()).cpu()
    assert torch.isfinite(dx).all()
    # each kind of row on its own scale (the constant row's rstd = 1 / sqrt(eps) makes its dx ~300x the others')
    offset = torch.zeros(M, dtype=torch.bool)
    offset[::5] = True
    constant = torch.zeros(M, dtype=torch.bool)
    if M > 1:
        constant[-1] = True
    for kind, rows in (("plain", ~offset & ~constant), ("offset", offset & ~constant), ("constant", constant)):
        if rows.any():
            ref64.check(f"layernorm bwd M={M} N={N} {kind} rows", dx[rows], r64[rows], r32[rows])


# ---- the loss path: embed_train + embed_backward ---------------------------------------------------------------------------
@pytest.fixture
def grad_mult(engine):
    default = engine.feature_grad_mult

    def set_(m):
        engine.feature_grad_mult = m
    yield set_
    engine.feature_grad_mult = default


def _loss_path_case(engine, sd0, B, T, mult, seed, grad_mult, n=None, c=ref64.C, gate=None, tag=""):
    """n: samples per clip (None: the fewest that give T frames).  c, gate, tag: for an engine in another GEMM mode
    (test_gpu_train_mode_f64.py) - the constant in front of e32, a ceiling relative to the largest gradient, a case prefix."""
    grad_mult(mult)
    n = n if n is not None else ref64.n_for(T)
    assert num_frames(n) == T
    gen = torch.Generator().manual_seed(seed)
    wav = (0.1 * torch.randn(B, n, generator=gen)).clamp(-1, 1)
    hw = (torch.rand(256, 768, generator=gen) * 2 - 1) / 768 ** 0.5
    hb = (torch.rand(256, generator=gen) * 2 - 1) / 768 ** 0.5
    hw[:, ref64.head_relu_undecided(sd0, wav)] = 0.0    # (8, 336): channel 382 of clip 4 has a time mean of 2.8e-7
    G_layers = torch.randn(12, B, T, 768, generator=gen) / (B * T * 768)
    G_emb = torch.randn(B, 256, generator=gen) / (B * 256)
    head = (hw.cuda(), hb.cuda())
    emb, layers, saved = engine.embed_train(wav.cuda(), head)
    assert layers.shape == (12, B, T, 768)
    dwav = engine.embed_backward(wav.cuda(), layers, saved, G_layers.cuda(), G_emb.cuda(), head)
    assert torch.isfinite(dwav).all()
    r64, r32 = ref64.both(ref64.lossnet_dwav, sd0, wav, hw, hb, G_layers, G_emb, feature_grad_mult=mult)
    ref64.check(f"{tag}loss path B={B} T={T} M={B * T} n={n} fgm={mult:g}", dwav, r64, r32, c=c)
    if gate is not None:
        assert (dwav.cpu().double() - r64).abs().max().item() <= gate * r64.abs().max().item()
    # samples no output frame depends on: exactly zero in float64, and on the GPU
    unused = r64 == 0
    assert torch.equal(dwav.cpu()[unused], torch.zeros(int(unused.sum())))
    return int(unused.sum()) // B


@pytest.mark.parametrize("mult", [0.1, 1.0])
def test_loss_path_at_the_product_shape_vs_float64(engine, sd0, mult, grad_mult):
    """configs[4]: nomad.forward + backward on 2 x (32, 16384) - here one side, B = 32 clips of 16384 samples, T = 50,
    M = 1600 rows.  The N = 768 GEMMs of both directions and the pos-conv split K there (the N = 2304 and N = 3072 ones,
    900 and 1200 tiles, do not).  16384 samples leave tails no frame covers in conv layers 0, 3, 4, 5 and 6 (the fewest
    samples for 50 frames, 16080, leave none); the last 4 samples, which conv0 never reaches, get exactly zero gradient."""
    assert _loss_path_case(engine, sd0, 32, 50, mult, 4, grad_mult, n=16384) > 0


# (B, T) pairs on both sides of each switch, the fewest samples for those frames (ref64.n_for): M = B * T
SWITCHES = {
    "fc1 (N=3072) split-K": [(5, 128), (5, 129)],           # M = 640 | 645
    "qkv (N=2304) split-K": [(4, 224), (4, 225)],           # M = 896 | 900
    "N=768 split-K": [(8, 336), (8, 337)],                  # M = 2688 | 2696
    "pos-conv split-K": [(10, 273), (10, 274)],             # M = 2730 | 2740
}


@pytest.mark.parametrize("B,T", [bt for v in SWITCHES.values() for bt in v],
                         ids=[f"{k.split()[0]}-{'below' if i == 0 else 'above'}" for k, v in SWITCHES.items() for i in range(2)])
def test_loss_path_across_the_split_k_switches_vs_float64(engine, sd0, B, T, grad_mult):
    _loss_path_case(engine, sd0, B, T, 1.0, B * 1000 + T, grad_mult)
