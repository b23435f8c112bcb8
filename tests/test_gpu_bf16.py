"""GPU: the bf16 path (BASELINE config C5) - bf16 MFMA GEMM kernel and the bf16 scoring forward, checked against
exact integer data, a float64 reference, and this library's own fp32 path (the reference has no bf16)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16_TILES = {0: (256, 128), 1: (128, 128), 2: (128, 64), 3: (256, 256), 4: (64, 64), 5: (128, 128), 6: (256, 128),
              9: (256, 256), 10: (256, 256), 11: (128, 128), 12: (128, 128), 13: (256, 128), 14: (256, 128), 15: (256, 256),
              16: (256, 256), 42: (256, 256),    # 16: the deep-pipelined kernel as shipped (three B buffers); 42: with two (diag library)
              55: (256, 192), 56: (256, 192)}    # the same schedule on 256 x 192 tiles (N = 768 GEMMs of config C5): three / two B buffers


@pytest.mark.parametrize("tile", sorted(BF16_TILES))
@pytest.mark.parametrize("M", [1, 200, 257, 1000])
def test_gemm_bf16_exact_integer_asymmetric(engine_for, tile, M):
    bm, bn = BF16_TILES[tile]
    N, K = 2 * bn, (256 if tile in (16, 42, 55, 56) else 192)  # the deep-pipelined kernels walk K tiles in pairs: K % 128 == 0
    g = torch.Generator().manual_seed(M + tile)
    A = torch.randint(-1, 2, (M, K), generator=g).float()
    W = torch.randint(-1, 2, (N, K), generator=g).float()
    W[:, ::7] = 1.0                      # break symmetry
    ref = (A.double() @ W.double().T)    # |C| <= K <= 256: exact in bf16 (8-bit significand)
    out = engine_for("bf16", tile).diag_gemm_bf16(A.bfloat16().cuda(), W.bfloat16().cuda(), tile=tile).float().cpu()
    assert torch.equal(out.double(), ref)


@pytest.mark.parametrize("tile,M,N,K", [(0, 1500, 256, 768), (1, 700, 768, 3072), (2, 260, 64, 6144), (4, 84, 768, 512),
                                        (3, 600, 512, 1536), (16, 777, 768, 3072), (16, 1500, 512, 1536),
                                        (16, 300, 2304, 768), (16, 4113, 256, 128), (42, 777, 768, 3072), (42, 300, 2304, 768),
                                        (55, 777, 768, 3072), (55, 1500, 768, 768), (55, 300, 2304, 768), (55, 4113, 192, 128),
                                        (56, 777, 768, 3072), (56, 300, 192, 256)])
@pytest.mark.parametrize("epi", ["none", "bias_gelu", "bias_res"])
def test_gemm_bf16_epilogues(engine_for, tile, M, N, K, epi):
    g = torch.Generator().manual_seed(5)
    A = torch.randn(M, K, generator=g).bfloat16()
    W = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16()
    bias = torch.randn(N, generator=g) if "bias" in epi else None
    R = torch.randn(M, N, generator=g).bfloat16() if "res" in epi else None
    ref = A.double() @ W.double().T
    if bias is not None:
        ref = ref + bias.double()
    if "gelu" in epi:
        ref = F.gelu(ref)
    if R is not None:
        ref = ref + R.double()
    out = engine_for("bf16", tile).diag_gemm_bf16(A.cuda(), W.cuda(), bias.cuda() if bias is not None else None,
                                                  R.cuda() if R is not None else None, gelu="gelu" in epi, tile=tile).cpu()
    err = (out.double() - ref).abs().max().item()
    assert err < 2 ** -7 * max(1.0, ref.abs().max().item()), err      # one bf16 rounding of the output


@pytest.mark.parametrize("M,N,K", [(4000, 768, 3072), (2999, 768, 768), (513, 2304, 768), (255, 768, 128)])
@pytest.mark.parametrize("epi", ["none", "bias_gelu", "bias_res"])
def test_gemm_bf16_192_column_tiles_are_bit_identical(engine_for, M, N, K, epi):
    """The 256 x 192 tiles (run_gemm_bf16 takes them where they save a round of CUs) change no bit: same k order per element."""
    g = torch.Generator().manual_seed(M)
    A = torch.randn(M, K, generator=g).bfloat16().cuda()
    W = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16().cuda()
    bias = torch.randn(N, generator=g).cuda() if "bias" in epi else None
    R = torch.randn(M, N, generator=g).bfloat16().cuda() if "res" in epi else None
    outs = [engine_for("bf16", t).diag_gemm_bf16(A, W, bias, R, gelu="gelu" in epi, tile=t) for t in (16, 55, 56, 57, 58, 1)]   # 57 / 58: the residual prefetch, general / plain epilogue (16 resolves to one of them)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


@pytest.mark.parametrize("M,N,K", [(70000, 768, 3072), (70000, 768, 768), (47968, 2304, 768), (40000, 512, 1536), (2999, 768, 768),
                                    (513, 2304, 768), (255, 768, 128), (256 * 300 + 17, 256, 256), (100000, 256, 128),
                                    (192 * 250 + 1, 768, 768), (191, 256, 256), (97, 512, 384), (23984, 768, 3072)])
@pytest.mark.parametrize("epi", ["none", "bias", "bias_gelu", "bias_res"])
def test_gemm_bf16_persistent_kernel_is_bit_identical(engine_for, M, N, K, epi):
    """Round 5: the persistent 256 x 256 kernel (gemm_bf16_p9.hip.h; tile 60 = epilogue interleaved into the next tile's first K tile,
    63 = every epilogue between tiles) against the one-tile-per-workgroup kernel 58 and the 128 x 128 kernel 1: same k order per
    element, same epilogue arithmetic - the same bits.  Shapes from less than one tile per workgroup to 9 tiles per workgroup, a ragged
    last row tile, K of 2 to 48 K tiles; repeated, because what this guards against (a staged K tile read early, a stale bias
    register) shows up in some runs only.  Round 6: tile 68 = the same instantiation in its run-time SHORT mode (192-row tiles: 96 rows
    per wave row, the surplus LDS-DMA pieces and stores made harmless by data), 64 = never short; 60 picks by the round count."""
    g = torch.Generator().manual_seed(M + K)
    A = torch.randn(M, K, generator=g).bfloat16().cuda()
    W = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16().cuda()
    bias = torch.randn(N, generator=g).cuda() if "bias" in epi else None
    R = torch.randn(M, N, generator=g).bfloat16().cuda() if "res" in epi else None
    eng = engine_for("bf16", 63)   # (the diag library: it has every instantiation)
    ref = eng.diag_gemm_bf16(A, W, bias, R, gelu="gelu" in epi, tile=58)
    assert torch.equal(eng.diag_gemm_bf16(A, W, bias, R, gelu="gelu" in epi, tile=1), ref)
    out = torch.empty_like(ref)
    for t in (60, 63, 68, 64):
        for rep in range(6 if t != 64 else 2):
            out.fill_(float("nan"))
            eng.diag_gemm_bf16(A, W, bias, R, gelu="gelu" in epi, tile=t, out=out)
            assert torch.equal(out, ref), (t, rep)


def test_bf16_gelu_keeps_a_non_finite_activation_non_finite(engine_for):
    """the first bf16-output GELU, x * sigmoid(g(x)), turned an activation that had overflowed to -inf into NaN where the erf form
    gives -0.  The present form, max(x, 0) - |x| 2^q(|x|) (gemm_f32.hip.h gelu_bf16out; q a cubic that falls monotonically), turns every
    non-finite input into NaN (inf * 0; torch.nn.functional.gelu in fp32 does the same for -inf, and on the CPU for +inf) - an overflow stays
    visible - and gives for finite inputs the GELU to 5.5e-5: a hugely negative activation gives the exact -0 (2^q underflows to 0)."""
    g = torch.Generator().manual_seed(3)
    M, N, K = 512, 256, 128
    A = torch.randn(M, K, generator=g).bfloat16().cuda()
    W = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16().cuda()
    bias = torch.randn(N, generator=g)
    bias[3], bias[77], bias[130], bias[200], bias[201] = float("-inf"), float("inf"), float("nan"), -1e30, -50.0
    bias = bias.cuda()
    eng = engine_for("bf16", 63)
    ref = torch.nn.functional.gelu(A.float() @ W.float().t() + bias)
    for t in (1, 60):
        out = eng.diag_gemm_bf16(A, W, bias, None, gelu=True, tile=t).float()
        assert torch.isnan(out[:, 3]).all() and torch.isnan(out[:, 77]).all() and torch.isnan(out[:, 130]).all()
        assert (out[:, 200] == 0).all() and (out[:, 201] == 0).all()
        ok = torch.ones(N, dtype=torch.bool)
        ok[[3, 77, 130]] = False
        assert (out[:, ok.cuda()] - ref[:, ok.cuda()]).abs().max() < 0.02


@pytest.mark.parametrize("M,N,K,epi", [(47968, 768, 768, "bias_res"), (2999, 2304, 768, "bias"), (40000, 512, 1536, "bias_gelu"), (192 * 7 + 5, 768, 3072, "bias_res")])
def test_gemm_bf16_persistent_kernel_whole_line_stores_are_bit_identical(built_lib, sd0, monkeypatch, M, N, K, epi):
    """Round 6: the persistent kernel can store 8 rows x 128 bytes per instruction (lanes fr / fr + 8 of a 16-lane row swap a 16-byte chunk by
    DPP) instead of the accumulator's 16 rows x 64 bytes.  Measured and left OFF (NOMAD_BF16_P9_WL, diag library), but the path stays in the kernel:
    the same bytes in the same places, 256- and 192-row tiles, interleaved and between-tile epilogues."""
    from nomad_amd.engine import Engine
    g = torch.Generator().manual_seed(M + K)
    A = torch.randn(M, K, generator=g).bfloat16().cuda()
    W = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16().cuda()
    bias = torch.randn(N, generator=g).cuda()
    R = torch.randn(M, N, generator=g).bfloat16().cuda() if "res" in epi else None
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("NOMAD_BF16_P9_WL", flag)
        eng = Engine(sd0, 0, diag=True)
        res = []
        for t in (60, 68):
            out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
            eng.diag_gemm_bf16(A, W, bias, R, gelu="gelu" in epi, tile=t, out=out)
            res.append(out)
        torch.cuda.synchronize()
        outs.append(res)
        eng.close()
    assert torch.isfinite(outs[0][0].float()).all()
    for t in range(2):
        assert torch.equal(outs[0][t], outs[1][t]) and torch.equal(outs[0][0], outs[1][t])


LOG2E = 1.4426950408889634


@pytest.mark.parametrize("B,T", [(32, 1499), (16, 1499), (19, 1030), (21, 1281), (23, 999)])
def test_bf16_attention_tail_round_as_half_size_workgroups_is_bit_identical(built_lib, sd0, monkeypatch, B, T):
    """Round 6 probe (diag library only; measured slower, so the product keeps one launch): the work items of a sparsely filled last round of
    256-query workgroups run as 128-query workgroups in a second launch (run_attention_bf16, NOMAD_BF16_ATTN_TAIL eighths; 0 = one launch):
    the same 32-query waves over the same 32-key blocks - every bit the same, which is also what makes a clip's bits independent of its batch.  Shapes: configs[4]'s (4.5 rounds) and its two-stream half (2.25); clips whose last 128-query block lies past their end
    (T = 1030: 9 blocks of 10; T = 1281: 11 of 12, and a last round 0.95 full, which only the flag 8 splits); a tail of 0.16 round (T = 999)."""
    from nomad_amd.engine import Engine
    g = torch.Generator().manual_seed(B * T)
    qkv = torch.randn(B * T, 2304, generator=g)
    qkv[:, :1536] *= 0.35
    qkv[:, :768] *= LOG2E
    x = qkv.bfloat16().cuda()
    outs = []
    for flag in ("0", "4", "8"):
        monkeypatch.setenv("NOMAD_BF16_ATTN_TAIL", flag)
        eng = Engine(sd0, 0, diag=True)
        out = eng.diag_attention_bf16(x, B, T, q_has_log2e=True)
        torch.cuda.synchronize()
        outs.append(out.clone())
        eng.close()
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # (and the 128-query kernel alone, which small batches take, gives a single clip of the batch the same bits)
    monkeypatch.delenv("NOMAD_BF16_ATTN_TAIL")
    eng = Engine(sd0, 0, diag=True)
    one = eng.diag_attention_bf16(x[(B - 1) * T:].contiguous(), 1, T, q_has_log2e=True)
    torch.cuda.synchronize()
    eng.close()
    assert torch.equal(one, outs[1][(B - 1) * T:])


def _attention_case(engine, qkv32, B, T, log2e):
    """qkv32 fp32 (B*T, 2304) -> (kernel output, float64 reference from the bf16 values the kernel actually saw)."""
    x = qkv32.clone()
    if log2e:
        x[:, :768] *= LOG2E          # what the bf16 forward's QKV projection hands the kernel: q * 64^-0.5 * log2(e)
    x = x.bfloat16()
    xd = x.double()
    if log2e:
        xd[:, :768] /= LOG2E
    q, k, v = (xd[:, i * 768:(i + 1) * 768].view(B, T, 12, 64).transpose(1, 2) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).transpose(1, 2).reshape(B * T, 768)
    out = engine.diag_attention_bf16(x.cuda(), B, T, q_has_log2e=log2e).cpu()
    return out, ref


@pytest.mark.parametrize("B,T", [(2, 50), (1, 64), (1, 65), (1, 199), (1, 257), (1, 330), (90, 130)])
@pytest.mark.parametrize("gain", [1.0, 6.0])
@pytest.mark.parametrize("log2e", [True])
def test_attention_bf16(engine, B, T, gain, log2e):
    """Both workgroup shapes (128 / 256 queries: B = 90 crosses the switch), partial last key blocks and query blocks."""
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B * T, 2304, generator=g)
    qkv[:, :1536] *= (gain ** 0.5) * 0.35
    out, ref = _attention_case(engine, qkv, B, T, log2e)
    assert torch.isfinite(out.float()).all()
    # P is rounded to bf16 before the PV product and the output is stored in bf16: ~2^-8 relative each
    tol = 1.2e-2 * max(1.0, ref.abs().max().item())
    assert (out.double() - ref).abs().max().item() < tol


@pytest.mark.parametrize("T,spike_key", [(1499, 700), (1499, 1498), (300, 64), (300, 299)])
def test_attention_bf16_forced_late_rescale(engine, T, spike_key):
    """The deferred rescale is a rare, data-dependent branch: force it.  One key late in the sequence whose logit
    against every 7th query dwarfs the running reference maximum (all earlier blocks ran with the small one), in
    head 3 only; full-tensor float64 reference."""
    g = torch.Generator().manual_seed(T + spike_key)
    qkv = torch.randn(T, 2304, generator=g) * 0.5
    sign = torch.tensor([1.0 if d % 2 else -1.0 for d in range(64)])
    qkv[spike_key, 768 + 3 * 64:768 + 4 * 64] = 4.0 * sign
    qkv[::7, 3 * 64:4 * 64] = 0.6 * sign               # logit 0.6 * 4 * 64 = 154 against the spiked key
    out, ref = _attention_case(engine, qkv, 1, T, True)
    assert torch.isfinite(out.float()).all()
    err = (out.double() - ref).abs()
    assert err.max().item() < 2.5e-2 * max(1.0, ref.abs().max().item()), err.max().item()
    # the spiked rows of head 3 are (almost exactly) the spiked key's value row
    vrow = qkv[spike_key, 1536 + 3 * 64:1536 + 4 * 64].bfloat16().double()
    assert (out[::7, 3 * 64:4 * 64].double() - vrow).abs().max().item() < 2e-2


def test_embed_bf16_vs_fp32_path(engine):
    gen = torch.Generator().manual_seed(0)
    wav = (0.1 * torch.randn(8, 64000, generator=gen)).clamp(-1, 1).cuda()
    e32 = engine.embed(wav)
    e16 = engine.embed_bf16(wav)
    torch.cuda.synchronize()
    assert torch.isfinite(e16).all()
    assert (e16.norm(dim=1) - 1).abs().max().item() < 1e-5
    err = (e16 - e32).abs().max().item()
    cos = F.cosine_similarity(e16, e32, dim=1).min().item()
    d32, m32 = engine.pairwise(e32[:6].contiguous(), e32[6:].contiguous())
    d16, m16 = engine.pairwise(e16[:6].contiguous(), e16[6:].contiguous())
    serr = (d16 - d32).abs().max().item()
    print(f"bf16 vs fp32: embedding max|err| {err:.3e}, min cosine {cos:.6f}, score max|err| {serr:.3e}")
    assert err < 3e-3 and cos > 0.99997 and serr < 1.2e-3      # measured 9.5e-4 / 0.99999 / 3.6e-4


def test_bf16_follows_weight_updates(built_lib, sd0):
    """The bf16 weight copies are rebuilt after the master weights change (fine-tuning, nomad_train_write): the twin of
    test_gpu_bf16x3.py::test_bf16x3_follows_weight_updates, held to the bf16-against-fp32 bound of test_embed_bf16_vs_fp32_path."""
    from nomad_amd.engine import Engine
    eng = Engine(sd0, 0)
    try:
        gen = torch.Generator().manual_seed(8)
        wav = (0.1 * torch.randn(2, 20000, generator=gen)).cuda()
        before = eng.embed_bf16(wav).clone()
        eng.train_enable()
        theta = eng.train_read()
        eng.train_write(0, theta * 1.01)
        after = eng.embed_bf16(wav)
        ref = eng.embed(wav)
        err = (after - ref).abs().max().item()
        cos = F.cosine_similarity(after, ref, dim=1).min().item()
        print(f"bf16 after a weight update vs fp32: embedding max|err| {err:.3e}, min cosine {cos:.6f}")
        assert not torch.equal(before, after)
        assert err < 3e-3 and cos > 0.99997
    finally:
        eng.close()


def test_embed_bf16_peaky_weights(engine_peaky):
    """The same against the conftest 'peaky' model (q / k gain 6: attention logits with sigma ~ 6, a few dominant keys per row, activation
    outliers - what trained weights look like and the seeded ones do not): the bf16 attention's late rescales, the bf16-output GELU's tails
    and the bf16 residual stream on data that exercises them.  Ten times looser than the seeded case: a logit of 20 carries 0.04-0.08 of bf16
    rounding from q and k alone, and the softmax turns that into per cent of a probability ("expect ~1e-2, not 1e-4"; the fp32-class
    alternative on the same matrix cores is bf16x3, 5e-5 on these weights)."""
    gen = torch.Generator().manual_seed(6)
    wav = (0.3 * torch.randn(6, 64000, generator=gen)).clamp(-1, 1).cuda()
    e32 = engine_peaky.embed(wav)
    e16 = engine_peaky.embed_bf16(wav)
    torch.cuda.synchronize()
    assert torch.isfinite(e16).all() and (e16.norm(dim=1) - 1).abs().max().item() < 1e-5
    err = (e16 - e32).abs().max().item()
    cos = F.cosine_similarity(e16, e32, dim=1).min().item()
    print(f"bf16 vs fp32 (peaky): embedding max|err| {err:.3e}, min cosine {cos:.6f}")
    assert err < 2e-2 and cos > 0.997      # measured 9.5e-3 / 0.99887 (seeded weights: 1.0e-3 / 0.999988): q / k rounded to bf16 under logits of +-20
    again = engine_peaky.embed_bf16(wav)
    assert torch.equal(again, e16)
    one = engine_peaky.embed_bf16(wav[4:5].contiguous())
    assert torch.equal(one[0], e16[4])


def test_embed_bf16_long_form(engine):
    """Config C5's shape: 30 s clips (T = 1499)."""
    gen = torch.Generator().manual_seed(1)
    wav = (0.1 * torch.randn(2, 480000, generator=gen)).clamp(-1, 1).cuda()
    e32 = engine.embed(wav)
    e16 = engine.embed_bf16(wav)
    assert torch.isfinite(e16).all()
    assert (e16 - e32).abs().max().item() < 3e-3 and F.cosine_similarity(e16, e32, dim=1).min().item() > 0.99997
    one = engine.embed_bf16(wav[1:2].contiguous())
    assert torch.equal(one[0], e16[1])      # batch invariance holds in bf16 too


def test_ragged_bf16_bit_identical_to_single_clips(engine):
    """nomad_embed_ragged_bf16: clips of different lengths in one launch sequence, each bit-equal to its own
    nomad_embed_bf16 call (and close to the fp32 path)."""
    g = torch.Generator().manual_seed(21)
    lens = [16384, 400, 27225, 9001, 64000, 30267, 5000, 12345, 48000]
    waves = [(0.1 * torch.randn(n, generator=g)).clamp(-1, 1) for n in lens]
    rag = engine.embed_ragged(waves, bf16=True)
    for i, w in enumerate(waves):
        single = engine.embed_bf16(w[None, :].cuda())
        assert torch.equal(rag[i], single[0]), (i, lens[i])
    f32 = engine.embed_ragged(waves)
    assert (rag - f32).abs().max().item() < 5e-3
    assert torch.nn.functional.cosine_similarity(rag, f32, dim=1).min().item() > 0.9995  # the 1-frame clip has no time averaging
    with pytest.raises(ValueError):
        engine.embed_ragged(waves, head=(torch.zeros(256, 768).cuda(), torch.zeros(256).cuda()), bf16=True)


def test_bf16_layernorm_rows_per_wave_do_not_change_a_bit(built_lib, sd0, monkeypatch):
    """Round 6: the bf16 forward's LayerNorm takes 4 consecutive rows per wave (one gamma / beta fetch for the four); a row's arithmetic is the
    one-row kernel's.  Batches whose row count is not a multiple of 16 (the last workgroup's waves have 1-3 rows, or none)."""
    from nomad_amd.engine import Engine
    g = torch.Generator().manual_seed(77)
    cases = [(0.1 * torch.randn(b, n, generator=g)).clamp(-1, 1).cuda() for b, n in ((3, 16384), (1, 400), (5, 27225), (2, 9001))]
    outs = []
    for flag in ("1", "4"):
        monkeypatch.setenv("NOMAD_BF16_LN_ROWS", flag)
        eng = Engine(sd0, 0, diag=True)
        outs.append([eng.embed_bf16(w).clone() for w in cases])
        torch.cuda.synchronize()
        eng.close()
    for a, b in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_ragged_bf16_with_a_long_clip_in_the_batch(engine):
    """A 30 s clip (T = 1499) next to short ones: the batch's longest clip picks the pos-conv's frames per workgroup (512 here, 256 / 128 in
    the single-clip calls of the short files) - every clip still bit-equal to its own nomad_embed_bf16 call."""
    g = torch.Generator().manual_seed(22)
    lens = [480000, 400, 64000, 5000, 90000]
    waves = [(0.1 * torch.randn(n, generator=g)).clamp(-1, 1) for n in lens]
    rag = engine.embed_ragged(waves, bf16=True)
    for i, w in enumerate(waves):
        single = engine.embed_bf16(w[None, :].cuda())
        assert torch.equal(rag[i], single[0]), (i, lens[i])


def test_predict_in_bf16_precision(built_lib):
    """Nomad(precision='bf16').predict on the reference's example files: same files, same layout, scores within 1e-3 of
    the fp32 run."""
    import os
    from conftest import GOLD
    from nomad_amd.nomad import Nomad
    nmr, deg = os.path.join(GOLD, "wavs", "nmr-data"), os.path.join(GOLD, "wavs", "test-data")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        a32, m32 = Nomad(weights="seeded").predict("dir", nmr, deg, results_path=d)
        a16, m16 = Nomad(weights="seeded", precision="bf16").predict("dir", nmr, deg, results_path=d)
    assert list(m16.columns) == list(m32.columns) and list(m16.index) == list(m32.index)
    assert abs(m16.values - m32.values).max() < 2e-3
    with pytest.raises(ValueError):
        Nomad(weights="seeded", precision="fp16")


@pytest.mark.parametrize("B,N", [(3, 64000), (2, 400), (1, 16395), (5, 3335), (2, 1375), (1, 2090)])
def test_conv0_on_the_matrix_cores(built_lib, sd0, B, N):
    """conv0 + GroupNorm + GELU of the bf16 path as one v_mfma_f32_16x16x32_bf16 per 16 channels x 16 frames (hi / lo split of
    waveform and weights along K, frontend.hip.h): against a float64 reference to one bf16 rounding, and against the VALU kernel
    it replaces (at most one bf16 ulp apart, almost everywhere equal).  N covers full blocks of 256 frames, a single short block,
    and tails that end inside different 16-frame tiles of a wave."""
    import ctypes as C
    from nomad_amd import _lib
    from nomad_amd.engine import Engine
    eng = Engine(sd0, 0, diag=True)
    lib = eng.lib
    _lib.check(lib.nomad_enable_bf16(eng.ctx), "nomad_enable_bf16")
    lib.nomad_diag_conv0_bf16.restype = C.c_int
    lib.nomad_diag_conv0_bf16.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L0 = (N - 10) // 5 + 1
    gen = torch.Generator().manual_seed(N)
    wav = (0.1 * torch.randn(B, N, generator=gen)).clamp(-1, 1)
    wav_dev = wav.cuda()
    outs = []
    for variant in (0, 4):
        out = torch.full((B, L0, 512), float("nan"), dtype=torch.bfloat16, device="cuda")
        scratch = torch.empty(8 * 65 * B * 16 + 8 * 512 * B + 4096, dtype=torch.uint8, device="cuda")
        assert lib.nomad_diag_conv0_bf16(eng.ctx, wav_dev.data_ptr(), B, N, out.data_ptr(), scratch.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream, variant) == 0
        torch.cuda.synchronize()
        outs.append(out.float().cpu())
    eng.close()
    w = sd0["ssl_model.feature_extractor.conv_layers.0.0.weight"].double()                  # (512, 1, 10)
    y = F.conv1d(wav.double().unsqueeze(1), w, stride=5)                           # (B, 512, L0)
    y = F.group_norm(y, 512, sd0["ssl_model.feature_extractor.conv_layers.0.2.weight"].double(), sd0["ssl_model.feature_extractor.conv_layers.0.2.bias"].double(), 1e-5)
    ref = F.gelu(y).transpose(1, 2)                                                # (B, L0, 512)
    for name, out in zip(("VALU kernel", "matrix-core kernel"), outs):
        assert torch.isfinite(out).all(), name
        err = (out.double() - ref).abs()
        # one bf16 rounding of the output (half an ulp is 2^-8 |x| at the bottom of a binade) + the fp32-class conv
        # (the matrix-core kernel drops the x_lo w_lo products: 2^-16 of the tap magnitudes, an absolute 1e-5 next to O(1) values, and
        # evaluates the bf16-output GELU, gemm_f32.hip.h gelu_bf16out: 5.5e-5 from the erf GELU; the VALU kernel keeps the erf form)
        bad = err > 1.02 * 2 ** -8 * ref.abs() + (4e-5 + 5.6e-5 if name.startswith("matrix") else 1e-6)
        if bad.any():
            i = torch.nonzero(bad)[0].tolist()
            raise AssertionError(f"{name}: {int(bad.sum())} elements off, first at {i}: out {out[tuple(i)].item()!r} ref {ref[tuple(i)].item()!r}")
    diff = (outs[0] - outs[1]).abs()
    assert (diff <= 2 ** -7 * outs[0].abs() + 8e-5 + 5.6e-5).all(), diff.max().item()      # never more than one bf16 ulp + the GELU forms' distance apart (outputs near zero: the absolute 2^-16 floor)
    frac = (diff > 0).float().mean().item()
    assert frac < 0.12, frac                                                        # and different in a minority of the elements only (5.5e-5 is a bf16 ulp where |gelu| < 0.014: the negative tail)


@pytest.mark.parametrize("B,T", [(2, 1499), (3, 199), (2, 50), (1, 1), (1, 130), (2, 513), (1, 257), (5, 199), (3, 100), (7, 128), (4, 256)])
def test_posconv_with_the_input_slab_in_lds(built_lib, sd0, B, T):
    """posconv_bf16_slab_kernel (the bf16 forward's positional convolution: a workgroup keeps the (frames + 128) x 48 input slab of one
    clip and group in LDS and streams the weights through registers) against the grouped GEMM it replaced, on the same bf16 input and
    weights: the two differ in fp32 summation order only, i.e. by at most one rounding of the bf16 output.  T covers one / several /
    partial workgroup tiles (512, 256 and 128 frames per workgroup), a single frame, and waves without any valid row."""
    import ctypes as C
    from nomad_amd import _lib
    from nomad_amd.engine import Engine
    eng = Engine(sd0, 0, diag=True)
    lib = eng.lib
    _lib.check(lib.nomad_enable_bf16(eng.ctx), "nomad_enable_bf16")
    lib.nomad_diag_posconv_bf16.restype = C.c_int
    lib.nomad_diag_posconv_bf16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    gen = torch.Generator().manual_seed(100 * B + T)
    xpad = torch.zeros(16, B, T + 128, 48)
    xpad[:, :, 64:64 + T] = torch.randn(16, B, T, 48, generator=gen)
    xdev = xpad.bfloat16().cuda()
    outs = []
    for variant in (0, 1):
        y = torch.full((B * T, 768), float("nan"), dtype=torch.bfloat16, device="cuda")
        assert lib.nomad_diag_posconv_bf16(eng.ctx, xdev.data_ptr(), y.data_ptr(), B, T, torch.cuda.current_stream().cuda_stream, variant) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(y.float()).all()
        outs.append(y.float().cpu())
    diff = (outs[1] - outs[0]).abs()
    tol = 2.0 ** -7 * outs[0].abs().clamp_min(0.25)      # one bf16 ulp of the larger of |y| and 0.25
    assert (diff <= tol).all(), (diff.max().item(), (diff > tol).sum().item())
    assert (diff > 0).float().mean().item() < 0.2        # (most outputs round to the same bf16 value)
    again = torch.empty_like(y)
    assert lib.nomad_diag_posconv_bf16(eng.ctx, xdev.data_ptr(), again.data_ptr(), B, T, torch.cuda.current_stream().cuda_stream, 1) == 0
    torch.cuda.synchronize()
    assert torch.equal(again, y)
    eng.close()
