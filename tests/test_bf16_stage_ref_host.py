"""CPU only: the stage checker of ``bf16_stage_ref.py`` discriminates (the role ``_assert_discriminates`` plays in
test_gpu_train_mode_f64.py).  A correct kernel is EMULATED on the CPU - the kernels' own arithmetic restated in fp32: K summed in
chunks of 32 like the matrix cores' k-steps, the cubic-tail GELU of gemm_f32.hip.h, conv0's hi / lo split without the lo x lo
products, probabilities rounded to bf16 with the row sums taken from the rounded values, then ONE rounding to bf16 - and must
pass the derived bound for every stage kind; nine mutations of it, one at a time, must each be rejected.  This is where the
bounds of test_gpu_bf16_stages_f64.py are validated before any GPU run.  Geometry: 2 clips of T = 70 frames (M = 140: a partial
key block of 6 behind one of 64, three 64-row blocks)."""
import pytest
import torch
import torch.nn.functional as F

import bf16_stage_ref as S
from bf16_stage_ref import bf16v

B, T = 2, 70
M = B * T


@pytest.fixture(scope="module")
def W(sd0):
    return S.Weights(sd0)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the emulated kernels ---------------------------------------------------------------------------------------------------
def gelu_cubic(x):
    """gemm_f32.hip.h gelu_bf16out (the shipped cubic tail), fp32."""
    a = x.abs()
    q = a * -2.48856321e-2 + -4.98820007e-1
    q = q * a + -1.129246
    q = q * a + -1.00353169
    return x.clamp_min(0.0) - a * torch.exp2(q)


def gemm_emul(x, w, bias=None, res=None, gelu=False):
    """fp32 accumulation over k-steps of 32 in sequence, bias, GELU, residual: the epilogue's order; not yet rounded."""
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k0 in range(0, x.shape[1], 32):
        acc = acc + x[:, k0:k0 + 32] @ w[:, k0:k0 + 32].t()
    if bias is not None:
        acc = acc + bias
    if gelu:
        acc = gelu_cubic(acc)
    return acc if res is None else acc + res


def ln_emul(x, g, b, mean_from=None):
    mean = (x if mean_from is None else mean_from).mean(-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + 1e-5)
    return d * rstd * g + b


def attention_emul(qkv, nb, t, drop_last_key=False, natural_exp=False):
    q, k, v = (qkv[:, i * 768:(i + 1) * 768].view(nb, t, 12, 64).transpose(1, 2) for i in range(3))
    if drop_last_key:
        k, v = k[:, :, :-1], v[:, :, :-1]
    s = q @ k.transpose(-1, -2)                                  # log2 units: q carries log2 e
    s = s - s.amax(-1, keepdim=True)
    p = bf16v(torch.exp(s) if natural_exp else torch.exp2(s))    # rounded before the PV product ...
    o = (p @ v) / p.sum(-1, keepdim=True)                        # ... and the row sums come from the rounded P
    return o.transpose(1, 2).reshape(nb * t, 768)


# ---- one case per stage kind: inputs, the emulation (with an optional mutation), the check --------------------------------------
def case_gn_and_conv0(W, mut=None):
    wav = (0.1 * torch.randn(B, 2000, generator=_gen(1))).clamp(-1, 1)
    L0 = (2000 - 10) // 5 + 1
    w0, (gamma, beta) = W.conv0(), W.gn()
    sums, sums_abs = S.gn_sums(wav)
    S.check_sums("gn sums", sums.clone(), sums, sums_abs, L0)
    (sc64, sh64), (sc32, sh32) = S.gn_fold(sums, wav, w0, gamma, beta)
    S.check_f32("gn_fold", "gn_fold", (sc64.float(), sh64.float()), (sc64, sh64), (sc32, sh32))   # the kernel: double, rounded to fp32
    scale, shift = sc64.float(), sh64.float()
    xwin = wav.unfold(1, 10, 5).reshape(B * L0, 10)
    xh, wh = bf16v(xwin), bf16v(w0)
    xl, wl = bf16v(xwin - xh), bf16v(w0 - wh)
    c = xh @ wh.t() + xh @ wl.t() + xl @ wh.t()
    sr, hr = scale.repeat_interleave(L0, 0), shift.repeat_interleave(L0, 0)
    got = gelu_cubic(c * sr + hr).bfloat16()
    y64, y32, a = S.conv0(xwin, sr, hr, w0)
    S.check_bf16("conv0", "conv0", got, y64, y32, a)


def case_conv(W, i, mut=None):
    k = S.CONV_K[i]
    L = 141
    x = bf16v(F.gelu(torch.randn(B, L, 512, generator=_gen(10 + i))))
    win = S.conv_windows(x, k)
    assert win.shape[0] == M
    emu_in = win.clone()
    if mut == "conv_shift":                                      # output frame 7 of clip 0 from input frames 15 .. instead of 14 ..
        emu_in[7] = x[0, 15:15 + k].reshape(-1)
    got = gemm_emul(emu_in, W.conv(i), gelu=True).bfloat16()
    y64, y32 = S.conv(win, W.conv(i))
    S.check_bf16("conv", f"conv{i}", got, y64, y32, S.A_GELU)


def case_layernorm(W, n, mut=None):
    g, b = W.feature_ln() if n == 512 else W.encoder_ln()
    x = bf16v(torch.randn(M, n, generator=_gen(n)) + 0.3 * torch.randn(M, 1, generator=_gen(n + 1)))
    mean_from = None
    if mut == "ln_mean":                                         # row 9 normalised with row 10's mean
        mean_from = x.clone()
        mean_from[9] = x[10]
    got = ln_emul(x, g, b, mean_from).bfloat16()
    y64, y32 = S.layernorm(x, g, b)
    S.check_bf16("layernorm", f"layernorm{n}", got, y64, y32)


def case_projection(W, mut=None):
    w, b = W.proj()
    x = bf16v(torch.randn(M, 512, generator=_gen(20)))
    y = gemm_emul(x, w, b).bfloat16()
    xpad = torch.zeros(16, B, T + 128, 48, dtype=torch.bfloat16)
    xpad[:, :, 64:64 + T] = y.view(B, T, 16, 48).permute(2, 0, 1, 3)
    if mut == "xpad_pad":                                        # one pad frame that is not zero
        xpad[3, 1, 10, 7] = 2.0 ** -20
    bi, ti = torch.arange(M) // T, torch.arange(M) % T
    y64, y32 = S.linear(x, w, b)
    S.check_bf16("projection", "projection", S.xpad_rows(xpad, bi, ti), y64, y32)
    S.check_zero("xpad leading pad frames", xpad[:, :, :64])
    S.check_zero("xpad trailing pad frames", xpad[:, :, 64 + T:])


def case_posconv(W, mut=None):
    w, bias = W.pos()
    xpad = torch.zeros(16, B, T + 128, 48)
    xpad[:, :, 64:64 + T] = bf16v(0.5 * torch.randn(16, B, T, 48, generator=_gen(30)))
    xp = S.xpad_clips(xpad)
    conv = torch.cat([gemm_emul(xp[:, :, 48 * g:48 * g + 48].unfold(1, 128, 1)[:, :T].permute(0, 1, 3, 2).reshape(M, 6144),
                                w[48 * g:48 * g + 48].permute(0, 2, 1).reshape(48, 6144)) for g in range(16)], 1)
    got = (gelu_cubic(conv + bias) + xp[:, 64:64 + T].reshape(M, 768)).view(B, T, 768)
    if mut == "clip_last_frame":                                 # the last frame of clip 0 computed from clip 1's slab
        got = got.clone()
        got[0, T - 1] = got[1, T - 1]
    y64, y32 = S.posconv(xp, w, bias)
    S.check_bf16("posconv", "posconv", got.bfloat16(), y64, y32, S.A_GELU)
    # (and the sampled form - one window of 129 padded frames per output frame - is the same reference)
    bi, ti = torch.tensor([0, 0, 1, 1]), torch.tensor([0, T - 1, 0, T - 1])
    w64, _ = S.posconv(S.xpad_windows(xpad, bi, ti), w, bias)
    assert (w64[:, 0] - y64[bi, ti]).abs().max().item() < 1e-12


def _layer_inputs(seed):
    g = _gen(seed)
    return bf16v(torch.randn(M, 768, generator=g)), bf16v(0.3 * torch.randn(M, 768, generator=g))


def case_qkv(W, mut=None):
    lw = W.layer(0)
    x, _ = _layer_inputs(40)
    got = gemm_emul(x, lw["qkv_w"], lw["qkv_b"]).bfloat16()
    y64, y32 = S.linear(x, lw["qkv_w"], lw["qkv_b"])
    S.check_bf16("qkv", "qkv", got, y64, y32)


def case_attention(W, mut=None):
    qkv = torch.randn(M, 2304, generator=_gen(50))
    qkv[:, :1536] *= (6.0 ** 0.5) * 0.35                         # logits with sigma ~ 6: a few dominant keys per row
    qkv[:, :768] *= S.LOG2E
    qkv = bf16v(qkv)
    got = attention_emul(qkv, B, T, drop_last_key=mut == "attn_last_key", natural_exp=mut == "q_log2e").bfloat16()
    q, k, v = (qkv[:, i * 768:(i + 1) * 768].view(B, T, 768) for i in range(3))
    y64, y32, a = S.attention(q, k, v)
    S.check_bf16("attention", "attention", got, y64.reshape(M, 768), y32.reshape(M, 768), a.reshape(M, 768))


def case_out_proj(W, mut=None):
    lw = W.layer(0)
    x, ctx = _layer_inputs(60)
    res = x.clone()
    if mut == "no_residual":                                     # the residual omitted for one 64-row block
        res[64:128] = 0.0
    got = gemm_emul(ctx, lw["o_w"], lw["o_b"], res=res).bfloat16()
    y64, y32 = S.linear(ctx, lw["o_w"], lw["o_b"], x)
    S.check_bf16("out_proj", "out_proj", got, y64, y32)


def case_fc1(W, mut=None):
    lw = W.layer(0)
    x2, _ = _layer_inputs(70)
    bias = lw["fc1_b"].clone()
    if mut == "bias_shift":                                      # column j's bias used for column j + 1 in one 16-column block
        bias[33:48] = lw["fc1_b"][32:47]
    got = gemm_emul(x2, lw["fc1_w"], bias, gelu=True).bfloat16()
    y64, y32 = S.linear(x2, lw["fc1_w"], lw["fc1_b"], gelu=True)
    S.check_bf16("fc1", "fc1", got, y64, y32, S.A_GELU)


def case_fc2(W, mut=None):
    lw = W.layer(0)
    x2, _ = _layer_inputs(80)
    h = bf16v(F.gelu(torch.randn(M, 3072, generator=_gen(81))))
    h[5, -1] = 1.0
    emu_h = h.clone()
    if mut == "gemm_last_k":                                     # the last K element dropped for one row
        emu_h[5, -1] = 0.0
    got = gemm_emul(emu_h, lw["fc2_w"], lw["fc2_b"], res=x2).bfloat16()
    y64, y32 = S.linear(h, lw["fc2_w"], lw["fc2_b"], x2)
    S.check_bf16("fc2", "fc2", got, y64, y32)


def case_head(W, mut=None):
    w, b = W.head()
    x = bf16v(torch.randn(B, T, 768, generator=_gen(90)))
    got = F.normalize(F.relu(x.sum(1) * (1.0 / T)) @ w.t() + b, dim=1)
    y64, y32 = S.head(x, w, b)
    S.check_f32("head", "head", got, y64, y32)


CASES = {
    "gn_and_conv0": case_gn_and_conv0,
    "conv1": lambda W, mut=None: case_conv(W, 1, mut),
    "conv5": lambda W, mut=None: case_conv(W, 5, mut),
    "layernorm512": lambda W, mut=None: case_layernorm(W, 512, mut),
    "layernorm768": lambda W, mut=None: case_layernorm(W, 768, mut),
    "projection": case_projection,
    "posconv": case_posconv,
    "qkv": case_qkv,
    "attention": case_attention,
    "out_proj": case_out_proj,
    "fc1": case_fc1,
    "fc2": case_fc2,
    "head": case_head,
}

MUTATIONS = [("fc2", "gemm_last_k"), ("fc1", "bias_shift"), ("conv1", "conv_shift"), ("posconv", "clip_last_frame"),
             ("projection", "xpad_pad"), ("layernorm768", "ln_mean"), ("out_proj", "no_residual"),
             ("attention", "attn_last_key"), ("attention", "q_log2e")]


@pytest.mark.parametrize("kind", sorted(CASES))
def test_the_checker_passes_an_emulated_correct_kernel(W, kind):
    CASES[kind](W)


@pytest.mark.parametrize("kind,mut", MUTATIONS)
def test_the_checker_rejects_a_mutated_kernel(W, kind, mut):
    with pytest.raises(AssertionError) as e:
        CASES[kind](W, mut)
    print(f"{mut}: {str(e.value)[:300]}")
    assert "first at" in str(e.value)                            # the checker's own report, with the offending index


def test_the_gelu_term_is_the_cubic_tails_distance_from_erf():
    """A_GELU bounds the shipped form's distance from the erf GELU (float64) over the range activations take."""
    x = torch.linspace(-14, 14, 560001)
    d = (gelu_cubic(x).double() - F.gelu(x.double())).abs().max().item()
    assert 4e-5 < d < S.A_GELU, d


def test_the_implicit_gemm_forms_are_the_convolutions(W):
    """conv_windows + GEMM is F.conv1d(stride 2); posconv is the grouped F.conv1d(padding 64) with its last output dropped."""
    x = torch.randn(B, 37, 512, generator=_gen(3)).double()
    for i in (1, 5):
        w = W.f32(S.P + f"feature_extractor.conv_layers.{i}.0.weight").double()
        ref = F.gelu(F.conv1d(x.transpose(1, 2), bf16v(w).double(), stride=2)).transpose(1, 2)
        y64, _ = S.conv(S.conv_windows(x.float(), S.CONV_K[i]), W.conv(i))
        assert (y64.view(ref.shape) - ref).abs().max().item() < 1e-12
    w, bias = W.pos()
    xin = bf16v(torch.randn(B, 21, 768, generator=_gen(4)))
    ref = F.conv1d(xin.double().transpose(1, 2), w.double(), bias.double(), padding=64, groups=16)[:, :, :-1]
    ref = xin.double() + F.gelu(ref).transpose(1, 2)
    y64, _ = S.posconv(F.pad(xin, (0, 0, 64, 64)), w, bias)
    assert (y64 - ref).abs().max().item() < 1e-12


def test_weights_are_rounded_once_from_the_librarys_fp32_values(W, sd0):
    """q rows: (w * 2^-3) * log2 e in fp32, then bf16 - not bf16(w) * log2 e; k / v rows: bf16(w)."""
    lw = W.layer(0)
    q = sd0[S.P + "encoder.layers.0.self_attn.q_proj.weight"].float()
    assert torch.equal(lw["qkv_w"][:768], ((q * 0.125) * S.LOG2E_F32).bfloat16().float())
    assert not torch.equal(lw["qkv_w"][:768], bf16v(bf16v(q * 0.125) * S.LOG2E_F32))
    assert torch.equal(lw["qkv_w"][768:1536], bf16v(sd0[S.P + "encoder.layers.0.self_attn.k_proj.weight"]))
    assert torch.equal(lw["qkv_b"][1536:], sd0[S.P + "encoder.layers.0.self_attn.v_proj.bias"].float())
    w, _ = W.pos()
    v, g = sd0[S.P + "encoder.pos_conv.0.weight_v"].double(), sd0[S.P + "encoder.pos_conv.0.weight_g"].double()
    ref = g * v / v.pow(2).sum((0, 1), keepdim=True).sqrt()
    assert (w.double() - ref).abs().max().item() <= 2.0 ** -8 * ref.abs().max().item()
