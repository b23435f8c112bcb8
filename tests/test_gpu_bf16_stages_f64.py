"""GPU: every stage of the bf16 forward (``forward_bf16_run``: the README's 30 s / batch 32 line) against float64 ON ITS OWN INPUT.

The diag library records the buffer of any stage of the next equal-length ``nomad_embed_bf16`` call (``nomad_diag_set_snapshot``,
four stages per forward; the forward is bit-reproducible, so 25 forwards of the same input collect all 99).  Stage s is then held
to the plain torch restatement of ``bf16_stage_ref.py`` evaluated on the GPU's own input of that stage - itself a snapshot: conv i
on conv i - 1's output, out_proj on the attention's output and the previous LayerNorm (its residual), fc2 on fc1's output and LN1 -
with the weights as the library holds them.  bf16 rounding does not accumulate across stages, so the bound stays at ONE rounding of
the stage's output plus its fp32-class arithmetic; ``bf16_stage_ref``'s docstring derives it (nothing measured on the GPU enters),
and ``test_bf16_stage_ref_host.py`` shows on the CPU that it passes a correct kernel and rejects nine single mutations.  What
this adds to the end-to-end gates (test_gpu_forward_f64 C_BF16, test_embed_bf16_vs_fp32_path) and to the bit-identity tests between
kernels of this library: a mistake two kernels share, or a mistake in how the forward CALLS them (a wrong last frame of a
stride-2 conv, a pad frame of xpad that is not zero, a stale bias in one tile), moves a unit-norm embedding by less than bf16
already costs it - and moves its own stage by orders of magnitude more than this bound.

Stage numbers (the CK(...) calls of forward_bf16_run): 0 GroupNorm sums (double), 1 / 2 scale / shift (fp32), 3 .. 9 conv0 .. conv6,
10 feature LayerNorm, 11 xpad (the projection, group-major and padded), 12 pos-conv + input, 13 encoder LayerNorm, 14 + 7 l + {0 .. 6}
layer l: qkv, attention, out_proj + x, LN1, fc1 + GELU, fc2 + x2, LN2; 98 the embeddings - which must be the tensor ``embed_bf16``
returns (that pins the numbering to the library).

Geometries: the smallest that reach each branch the forward can take (test_the_geometries_cross_every_dispatch_branch restates the
thresholds of run_gemm_bf16, run_attention_bf16 and run_posconv_bf16_slab on the CPU and fails when one moves):
    one_frame     1 clip, T = 1 (400 samples): every tile a single partial one
    small, small_peaky   B = 3, T = 65 (M = 195 < 512), weights sd0 / peaky: 64 x 64 GEMM tiles, the 128-query attention with
                  partial blocks, the pos-conv in 128-frame mode, last 4-row LayerNorm waves with 3 rows and none.  In full.
    mid           B = 5, T = 130 (M = 650): 128 x 128 tiles for N = 768 / 512, 256 x 256 for N = 2304 / 3072, the pos-conv in
                  256-frame mode with two clips per workgroup.  In full.
    large         B = 44 x 10 s (T = 499, M = 21 956) as ONE call: the persistent kernel for every layer GEMM (258 tiles at N = 768,
                  there in its 192-row mode; 256-row at N = 2304 / 3072) and conv1..5, 128 x 128 for conv6, the one-tile 256 x 256 kernel
                  with general addressing for the projection, the 256-query attention, the pos-conv in 512-frame mode.  Here the
                  reference is computed on SAMPLED rows (about 512 per stage, gathered on the GPU): first and last row, both sides of
                  the 192- and 256-row boundaries of the last two row tiles, first and last frame of several clips, the rest
                  seeded at random (another draw per stage); a conv row gathers its 2 - 3 input frames, a pos-conv frame its window
                  of xpad, the attention is checked for sampled queries of three clips against those clips' full K / V; the head, the
                  GroupNorm stages and xpad's zero frames in full.

Measured on one MI355X: worst err / bound per stage kind, and in brackets the worst share of the fp32-class budget (1 + 2^-8) delta
an element needs beyond half an ulp of its own binade (``bf16_stage_ref.Report``).  err / bound sits at 1 / 1.02 = 0.98 for every
large bf16 tensor - some element always lies half an ulp from float64 at the bottom of a binade - so the share is the telling
number: the GELU stages spend 0.9 of delta on the cubic tail's 5.5e-5 (of A_GELU = 5.6e-5), the plain GEMMs and LayerNorms a fifth
of it at the most, the attention up to 0.88 of its P |V| term on the peaky weights.  No stage missed its bound; no kernel changed.

                 gn_sums gn_fold  conv0        conv         layernorm    projection   posconv      qkv          attention    out_proj     fc1          fc2          head
    one_frame    0.052   0.039    0.945 (.64)  0.957 (.90)  0.975 (.00)  0.956 (.00)  0.918 (.76)  0.970 (.01)  0.000 (.00)  0.954 (.01)  0.972 (.92)  0.962 (.02)  0.053
    small        0.010   0.039    0.969 (.73)  0.974 (.90)  0.976 (.03)  0.974 (.04)  0.973 (.95)  0.976 (.11)  0.528 (.27)  0.976 (.05)  0.975 (.91)  0.976 (.17)  0.047
    small_peaky  0.011   0.037    0.969 (.73)  0.974 (.90)  0.975 (.03)  0.974 (.02)  0.972 (.95)  0.975 (.10)  0.875 (.88)  0.976 (.04)  0.975 (.90)  0.976 (.14)  0.061
    mid          0.008   0.041    0.970 (.75)  0.974 (.91)  0.976 (.03)  0.975 (.06)  0.974 (.94)  0.975 (.07)  0.515 (.22)  0.976 (.07)  0.975 (.90)  0.976 (.15)  0.049
    large        0.006   0.050    0.964 (.69)  0.972 (.91)  0.975 (.02)  0.974 (.05)  0.973 (.94)  0.976 (.10)  0.498 (.10)  0.976 (.08)  0.974 (.90)  0.976 (.20)  0.058

(T = 1: the attention's output is v itself.)  A case takes 0.7 - 4 s (mid, the largest reference computed in full: 4 s).

Left unchecked: the ragged bf16 forward records no stages by design - test_ragged_bf16_bit_identical_to_single_clips ties it bit
for bit to single-clip calls, which the B = 1 geometry here covers; rows outside the sample at the large geometry (every kernel
that runs there also runs in full at a smaller one, except the persistent GEMM and the 256-query attention: those are sampled
across every tile-boundary class, and held in full against other kernels by the bit-identity tests of test_gpu_bf16.py)."""
import ctypes as C

import pytest
import torch

import bf16_stage_ref as S
import ref64
from nomad_amd.weights import conv_lengths, num_frames

N_STAGES = 99
N_SAMPLE = 512
NUM_CUS = 256       # MI355X
# name -> (clips, samples per clip, weights, reference on sampled rows only)
GEOMS = {
    "one_frame": (1, ref64.n_for(1), "sd0", False),
    "small": (3, ref64.n_for(65), "sd0", False),
    "small_peaky": (3, ref64.n_for(65), "peaky", False),
    "mid": (5, ref64.n_for(130), "sd0", False),
    "large": (44, 160000, "sd0", True),
}


# ---- the forward's choice of kernel per shape, restated ---------------------------------------------------------------------------
def gemm_kernel(M, N, K, plain=True):
    """run_gemm_bf16's tile < 0 branch (groups = 1).  plain: C / R are plain matrices (p8_plain_cr; not the projection into xpad)."""
    if N % 128 != 0:
        return "64x64" if M < 512 else "128x64"
    if M < 512:
        return "64x64"
    if N % 256 == 0 and K % 128 == 0 and -(-M // 256) * (N // 256) >= 256:
        return "persistent" if plain else "256x256 deep"
    return "256x256" if N % 256 == 0 and (N >= 1024 or M >= 100000) else "128x128"


def persistent_short(M, N):
    """The persistent kernel's 192-row mode for a batch that runs alone (run_gemm_bf16 case 60)."""
    grid = 8 * max(1, NUM_CUS // 8)
    tn = N // 256
    r_full, r_short = -(-(-(-M // 256) * tn) // grid), -(-(-(-M // 192) * tn) // grid)
    return 0.80 * r_short < 0.95 * r_full


def attention_queries(B, T):
    return 256 if -(-T // 256) * B * 12 >= 1024 else 128


def posconv_frames(T):
    return 512 if T > 256 else 256 if T > 128 else 128


def forward_kernels(B, n):
    """{what: kernel} for one equal-length call."""
    L = conv_lengths(n)
    M = B * L[6]
    k = {f"conv{i}": gemm_kernel(B * L[i], 512, S.CONV_K[i] * 512) for i in range(1, 7)}
    k["projection"] = gemm_kernel(M, 768, 512, plain=False)
    for name, N, K in (("qkv", 2304, 768), ("out_proj", 768, 768), ("fc1", 3072, 768), ("fc2", 768, 3072)):
        k[name] = gemm_kernel(M, N, K)
        if k[name] == "persistent":
            k[name] += " 192" if persistent_short(M, N) else " 256"
    k["attention"] = attention_queries(B, L[6])
    k["posconv"] = posconv_frames(L[6])
    return k


def test_the_geometries_cross_every_dispatch_branch():
    """Whoever moves a threshold of run_gemm_bf16 / run_attention_bf16 / run_posconv_bf16_slab moves it here too - and then sees
    whether the four geometries still reach every kernel."""
    assert GEOMS["one_frame"][1] == 400 and num_frames(400) == 1
    T = {g: num_frames(n) for g, (B, n, _, _) in GEOMS.items()}
    assert T == {"one_frame": 1, "small": 65, "small_peaky": 65, "mid": 130, "large": 499}
    for g in ("small", "mid"):                       # the fewest samples for T: the k = 3 convs' inputs (conv0..3's outputs) have odd lengths
        assert all(l % 2 == 1 for l in conv_lengths(GEOMS[g][1])[:4]), conv_lengths(GEOMS[g][1])
    k = {g: forward_kernels(B, n) for g, (B, n, _, _) in GEOMS.items()}
    gemms = ["projection", "qkv", "out_proj", "fc1", "fc2"] + [f"conv{i}" for i in range(1, 7)]
    for g in ("one_frame", "small"):                 # (the convs have their own row counts: B * L_i; at one frame all of them are below 512)
        assert all(k[g][x] == "64x64" for x in (gemms if g == "one_frame" else gemms[:5] + ["conv5", "conv6"])), k[g]
        assert k[g]["attention"] == 128 and k[g]["posconv"] == 128
    M = GEOMS["small"][0] * 65
    assert M < 512 and M % 16 == 3 and M % 64 != 0   # 4-row LayerNorm waves: the last workgroup's get 3 rows, then none
    assert 65 % 64 == 1                              # a partial key block and a partial 32-query wave
    m = k["mid"]
    assert GEOMS["mid"][0] * 130 >= 512
    assert all(m[x] == "128x128" for x in ["projection", "out_proj", "fc2"] + [f"conv{i}" for i in range(1, 7)]), m
    assert m["qkv"] == m["fc1"] == "256x256" and m["attention"] == 128 and m["posconv"] == 256
    assert GEOMS["mid"][0] % 2 == 1                  # two clips per pos-conv workgroup: the last one holds a single clip
    l = k["large"]
    B, n = GEOMS["large"][:2]
    Lc = conv_lengths(n)
    assert -(-B * 499 // 256) * 3 == 258
    assert all(l[f"conv{i}"] == "persistent" for i in range(1, 6)) and l["conv6"] == "128x128", l
    assert min(B * Lc[i] for i in range(1, 6)) >= 32513 > B * Lc[6]
    assert l["projection"] == "256x256 deep"
    assert l["out_proj"] == l["fc2"] == "persistent 192" and l["qkv"] == l["fc1"] == "persistent 256", l
    assert l["attention"] == 256 and -(-499 // 256) * B * 12 == 1056 and l["posconv"] == 512
    assert forward_kernels(B - 1, n)["out_proj"] == "128x128" and forward_kernels(B - 2, n)["attention"] == 128   # the smallest such batch
    kinds = set()
    for g in k:
        kinds |= {v.split()[0] if isinstance(v, str) else v for x, v in k[g].items() if x in gemms}
    assert kinds == {"64x64", "128x128", "256x256", "persistent"}


# ---- collecting the stages -----------------------------------------------------------------------------------------------------
def stage_bytes(B, n):
    L = conv_lengths(n)
    T = L[6]
    M = B * T
    sizes = [B * 65 * 8, B * 512 * 4, B * 512 * 4] + [B * L[i] * 512 * 2 for i in range(7)]
    sizes += [M * 512 * 2, 16 * B * (T + 128) * 48 * 2, M * 768 * 2, M * 768 * 2]
    for _ in range(12):
        sizes += [M * w * 2 for w in (2304, 768, 768, 768, 3072, 768, 768)]
    sizes.append(B * 256 * 4)
    assert len(sizes) == N_STAGES
    return sizes


def collect(eng, wav):
    """The 99 stage buffers of nomad_embed_bf16(wav) as ONE call (bytes, device), four per forward; every buffer starts as 0xFF
    bytes (NaN in every format recorded), so a stage that was not copied cannot pass."""
    from nomad_amd import _lib
    lib = eng.lib
    lib.nomad_diag_set_cksum.restype = C.c_int
    lib.nomad_diag_set_cksum.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.nomad_diag_set_snapshot.restype = C.c_int
    lib.nomad_diag_set_snapshot.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    B, n = wav.shape
    sizes = stage_bytes(B, n)
    bufs = [torch.full((s,), 255, dtype=torch.uint8, device="cuda") for s in sizes]
    table = torch.zeros(1, dtype=torch.int64, device="cuda")     # snapshots are taken only while a checksum table is armed
    emb = torch.empty(B, 256, dtype=torch.float32, device="cuda")
    for s0 in range(0, N_STAGES, 4):
        _lib.check(lib.nomad_diag_set_cksum(eng.ctx, table.data_ptr(), 1, 1), "nomad_diag_set_cksum")
        for slot in range(4):
            st = s0 + slot
            live = st < N_STAGES
            _lib.check(lib.nomad_diag_set_snapshot(eng.ctx, slot, st if live else -1, bufs[st].data_ptr() if live else None,
                                                   sizes[st] if live else 0), "nomad_diag_set_snapshot")
        lib.nomad_set_concurrent_parts(eng.ctx, 1)               # a batch that runs alone: the persistent kernel may take 192-row tiles
        eng._embed_bf16_into(wav, emb, side=False)
    torch.cuda.synchronize()
    return bufs


def sample_rows(M, L, B, seed):
    """About N_SAMPLE rows of a (B * L)-row buffer: first and last, both sides of the 192- and 256-row boundaries of the last two
    row tiles, first and last frame of the first, second, middle and last clip, the rest at random."""
    if M <= N_SAMPLE:
        return torch.arange(M)
    must = {0, M - 1}
    for step in (192, 256):
        last = (M - 1) // step * step
        must |= {last - step - 1, last - step, last - 1, last}
    for b in {0, 1, B // 2, B - 1}:
        must |= {b * L, b * L + L - 1}
    g = torch.Generator().manual_seed(seed)
    extra = torch.randint(0, M, (N_SAMPLE - len(must),), generator=g).tolist()
    return torch.tensor(sorted(r for r in must | set(extra) if 0 <= r < M))


def sample_queries(T, seed):
    if T <= 176:
        return torch.arange(T)
    must = {0, T - 1}
    for step in (32, 128, 256):
        for e in range(step, T, step):
            must |= {e - 1, e}
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(sorted(must | set(torch.randint(0, T, (120,), generator=g).tolist())))


def check_geometry(name, eng, Wt, wav, sampled):
    B, n = wav.shape
    L = conv_lengths(n)
    T = L[6]
    M = B * T
    rep = S.Report(name)
    wav_dev = wav.cuda()
    returned = eng.embed_bf16(wav_dev).clone()                   # (enables the bf16 weights; large batches: the two-stream split)
    snap = collect(eng, wav_dev)
    bf = lambda s, cols: snap[s].view(torch.bfloat16).view(-1, cols)
    host = lambda t: t.float().cpu()
    pick = lambda s, cols, rows: host(bf(s, cols).index_select(0, rows.cuda()))
    rows_of = lambda m, l, seed: sample_rows(m, l, B, seed) if sampled else torch.arange(m)

    # stage 98 is what the call returns; the last layer's output is finite everywhere
    emb = snap[98].view(torch.float32).view(B, 256)
    assert torch.equal(emb, returned), "stage 98 is not the embedding the call returned: the stage numbering moved"
    assert bool(torch.isfinite(bf(97, 768).float()).all()), "non-finite values in the last layer's output"

    # stages 0 - 2: the GroupNorm sums, folded into scale / shift
    w0, (gamma, beta) = Wt.conv0(), Wt.gn()
    sums, sums_abs = S.gn_sums(wav)
    stats = snap[0].view(torch.float64).view(B, 65).cpu()
    S.check_sums(f"{name} stage 0", stats, sums, sums_abs, L[0], rep)
    scale, shift = (snap[s].view(torch.float32).view(B, 512).cpu() for s in (1, 2))
    f64, f32 = S.gn_fold(stats, wav, w0, gamma, beta)
    S.check_f32("gn_fold", f"{name} stages 1-2", (scale, shift), f64, f32, rep)

    # stage 3: conv0 + GroupNorm + GELU from the waveform and the GPU's own scale / shift
    rows = rows_of(B * L[0], L[0], 3)
    b, t = rows // L[0], rows % L[0]
    xwin = wav[b[:, None], 5 * t[:, None] + torch.arange(10)[None, :]]
    y64, y32, a = S.conv0(xwin, scale[b], shift[b], w0)
    S.check_bf16("conv0", f"{name} stage 3 conv0", pick(3, 512, rows), y64, y32, a, rep, rows)

    # stages 4 - 9: conv1..6 as implicit GEMMs over the previous conv's output
    for i in range(1, 7):
        k = S.CONV_K[i]
        rows = rows_of(B * L[i], L[i], 3 + i)
        b, t = rows // L[i], rows % L[i]
        src = (b * L[i - 1] + 2 * t)[:, None] + torch.arange(k)[None, :]
        xwin = host(bf(2 + i, 512)[src.cuda()]).reshape(rows.numel(), k * 512)
        y64, y32 = S.conv(xwin, Wt.conv(i))
        S.check_bf16("conv", f"{name} stage {3 + i} conv{i}", pick(3 + i, 512, rows), y64, y32, S.A_GELU, rep, rows)

    # stage 10: the feature LayerNorm
    rows = rows_of(M, T, 10)
    y64, y32 = S.layernorm(pick(9, 512, rows), *Wt.feature_ln())
    S.check_bf16("layernorm", f"{name} stage 10 feature LN", pick(10, 512, rows), y64, y32, 0.0, rep, rows)

    # stage 11: the projection, scattered into xpad; its pad frames exactly zero (the whole buffer, on the GPU)
    xpad = snap[11].view(torch.bfloat16).view(16, B, T + 128, 48)
    S.check_zero(f"{name} stage 11 xpad, leading pad frames", xpad[:, :, :64])
    S.check_zero(f"{name} stage 11 xpad, trailing pad frames", xpad[:, :, 64 + T:])
    rows = rows_of(M, T, 11)
    b, t = rows // T, rows % T
    y64, y32 = S.linear(pick(10, 512, rows), *Wt.proj())
    S.check_bf16("projection", f"{name} stage 11 projection", host(S.xpad_rows(xpad, b.cuda(), t.cuda())), y64, y32, 0.0, rep, rows)

    # stage 12: x + gelu(pos_conv(x) + bias) from xpad
    pw, pb = Wt.pos()
    if sampled:
        rows = rows_of(M, T, 12)
        b, t = rows // T, rows % T
        y64, y32 = S.posconv(host(S.xpad_windows(xpad, b.cuda(), t.cuda())), pw, pb)
        y64, y32 = y64[:, 0], y32[:, 0]
    else:
        rows = torch.arange(M)
        y64, y32 = (y.reshape(M, 768) for y in S.posconv(host(S.xpad_clips(xpad)), pw, pb))
    S.check_bf16("posconv", f"{name} stage 12 pos-conv", pick(12, 768, rows), y64, y32, S.A_GELU, rep, rows)

    # stage 13: the encoder LayerNorm
    rows = rows_of(M, T, 13)
    y64, y32 = S.layernorm(pick(12, 768, rows), *Wt.encoder_ln())
    S.check_bf16("layernorm", f"{name} stage 13 encoder LN", pick(13, 768, rows), y64, y32, 0.0, rep, rows)

    clips = torch.tensor(sorted({0, B // 2, B - 1})) if sampled else torch.arange(B)
    for l in range(12):
        s = 14 + 7 * l
        x_in = s - 1                                             # the previous LN2 (layer 0: the encoder LayerNorm)
        lw = Wt.layer(l)
        tag = f"{name} layer {l}"
        rows = rows_of(M, T, s)
        y64, y32 = S.linear(pick(x_in, 768, rows), lw["qkv_w"], lw["qkv_b"])
        S.check_bf16("qkv", f"{tag} stage {s} qkv", pick(s, 2304, rows), y64, y32, 0.0, rep, rows)

        tq = sample_queries(T, s) if sampled else torch.arange(T)
        qkv = bf(s, 2304).view(B, T, 2304)[clips.cuda()]
        q, kk, vv = host(qkv[:, tq.cuda(), :768]), host(qkv[:, :, 768:1536]), host(qkv[:, :, 1536:])
        y64, y32, a = S.attention(q, kk, vv)
        got = host(bf(s + 1, 768).view(B, T, 768)[clips.cuda()][:, tq.cuda()])
        qrows = (clips[:, None] * T + tq[None, :]).flatten()
        flat = lambda y: y.reshape(-1, 768)
        S.check_bf16("attention", f"{tag} stage {s + 1} attention", flat(got), flat(y64), flat(y32), flat(a), rep, qrows)

        rows = rows_of(M, T, s + 2)
        y64, y32 = S.linear(pick(s + 1, 768, rows), lw["o_w"], lw["o_b"], pick(x_in, 768, rows))
        S.check_bf16("out_proj", f"{tag} stage {s + 2} out_proj + x", pick(s + 2, 768, rows), y64, y32, 0.0, rep, rows)

        rows = rows_of(M, T, s + 3)
        y64, y32 = S.layernorm(pick(s + 2, 768, rows), lw["ln1_w"], lw["ln1_b"])
        S.check_bf16("layernorm", f"{tag} stage {s + 3} LN1", pick(s + 3, 768, rows), y64, y32, 0.0, rep, rows)

        rows = rows_of(M, T, s + 4)
        y64, y32 = S.linear(pick(s + 3, 768, rows), lw["fc1_w"], lw["fc1_b"], gelu=True)
        S.check_bf16("fc1", f"{tag} stage {s + 4} fc1 + GELU", pick(s + 4, 3072, rows), y64, y32, S.A_GELU, rep, rows)

        rows = rows_of(M, T, s + 5)
        y64, y32 = S.linear(pick(s + 4, 3072, rows), lw["fc2_w"], lw["fc2_b"], pick(s + 3, 768, rows))
        S.check_bf16("fc2", f"{tag} stage {s + 5} fc2 + x2", pick(s + 5, 768, rows), y64, y32, 0.0, rep, rows)

        rows = rows_of(M, T, s + 6)
        y64, y32 = S.layernorm(pick(s + 5, 768, rows), lw["ln2_w"], lw["ln2_b"])
        S.check_bf16("layernorm", f"{tag} stage {s + 6} LN2", pick(s + 6, 768, rows), y64, y32, 0.0, rep, rows)

    # stage 98: the head reading bf16
    y64, y32 = S.head(host(bf(97, 768).view(B, T, 768)), *Wt.head())
    S.check_f32("head", f"{name} stage 98 head", emb.cpu(), y64, y32, rep)
    rep.print()
    del snap
    torch.cuda.empty_cache()
    return rep


@pytest.fixture(scope="module")
def engine_diag_peaky(built_lib, sd_peaky):
    from nomad_amd.engine import Engine
    eng = Engine(sd_peaky, 0, diag=True)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def stage_weights(sd0, sd_peaky):
    return {"sd0": S.Weights(sd0), "peaky": S.Weights(sd_peaky)}


@pytest.mark.gpu
@pytest.mark.parametrize("geom", list(GEOMS))
def test_every_stage_of_the_bf16_forward_against_float64_on_its_own_input(request, engine_diag, stage_weights, geom):
    B, n, which, sampled = GEOMS[geom]
    eng = engine_diag if which == "sd0" else request.getfixturevalue("engine_diag_peaky")
    g = torch.Generator().manual_seed(1000 + B)
    wav = ((0.3 if which == "peaky" else 0.1) * torch.randn(B, n, generator=g)).clamp(-1, 1)
    rep = check_geometry(geom, eng, stage_weights[which], wav, sampled)
    assert set(rep.worst) == {"gn_sums", "gn_fold", "conv0", "conv", "layernorm", "projection", "posconv", "qkv", "attention",
                              "out_proj", "fc1", "fc2", "head"}
