// libnomad_hip.so - engine + C ABI (include/nomad_hip.h).  gfx950 only.
//
// The engine owns: repacked fp32 weights in HBM and a pool of hipEvents for the in-library
// timers.  Everything else (waveforms, outputs, scratch) belongs to the caller.  nomad_embed
// enqueues the whole wav2vec 2.0 BASE forward + head on the caller's stream:
//
//   wav_stats -> gn_fold -> conv0+GN+GELU            (frontend.hip.h)
//   conv1..6 as implicit GEMM + GELU                 (gemm_f32.hip.h, A = time-major activations)
//   LayerNorm(512) -> post_extract_proj GEMM (+bias) writing into the zero-padded pos-conv buffer
//   grouped pos-conv GEMM (+bias, GELU, +x) -> LayerNorm(768)
//   12 x { QKV GEMM -> attention -> out_proj GEMM (+bias,+x) -> LN -> fc1 GEMM (+bias,GELU)
//          -> fc2 GEMM (+bias,+x) -> LN }
//   head (mean_t, ReLU, Linear 768->256, L2 normalise)
#include "nomad_ctx.hip.h"

// The device pass of this file is compiled WITHOUT the packed-FP32 VALU instructions (v_pk_fma_f32 / v_pk_mul_f32 /
// v_pk_add_f32 / v_pk_mov_b32: nomad_amd/build.py passes -target-feature -packed-fp32-ops).  DESIGN.md, "The packed-FP32
// hazard": on MI355X a v_pk_fma_f32 whose low half reads the HIGH register of a source pair (op_sel) can lose that product
// in lanes 48-63 while waves of a bf16 32x32x16-MFMA GEMM from ANOTHER kernel share its SIMD - the cause of the round-2
// "bf16 nondeterminism".  Those instructions are the compiler's choice (SLP vectorisation of scalar source), so the
// target feature is off for every kernel rather than relying on kernels never being co-scheduled.
#include "attention.hip.h"
#include "attention_bf16_v3.hip.h"
#include "posconv_bf16_slab.hip.h"
#include "attention_f32_v2.hip.h"
#include "attention_bwd.hip.h"
#include "backward.hip.h"
#include "degrade.hip.h"
#include "degrade_convolve.hip.h"
#include "reverb.hip.h"
#include "loudness.hip.h"
#include "nsim.hip.h"
#include "nsim_bwd.hip.h"
#include "nsim_patches.hip.h"
#include "align.hip.h"
#include "frontend.hip.h"
#include "gemm_bf16.hip.h"
#include "gemm_bf16_8phase.hip.h"
#include "gemm_bf16_p9.hip.h"
#include "gemm_bf16x3.hip.h"
#include "gemm_f32.hip.h"
#include "head.hip.h"
#ifdef NOMAD_DIAG  // libnomad_diag.so only: experiments kept for A/B measurements (tools/, tests of the experimental tiles)
#endif
#include "pairwise.hip.h"
#include "posconv_wino_f32.hip.h"
#include "posconv_fft_f32.hip.h"
#include "rowops.hip.h"
#include "train.hip.h"
#include "wav_reader.h"

namespace {

struct Shapes {
    int B, N, L[7], T, M;
};

bool make_shapes(int B, int N, Shapes* s) {
    s->B = B;
    s->N = N;
    int len = N;
    for (int i = 0; i < 7; ++i) {
        if (len < kConvK[i]) return false;
        len = (len - kConvK[i]) / kConvS[i] + 1;
        s->L[i] = len;
    }
    s->T = len;
    s->M = B * len;
    return len >= 1;
}

size_t align_up(size_t v) { return (v + 255) & ~size_t(255); }

// Workspace carve.  With keep=false the conv stack ping-pongs between two buffers.
// doubles in a forward's GroupNorm-statistics region: [B][65] final sums + [B][chunks][65] per-chunk partial sums
size_t stats_doubles(int B, int max_l0) {
    return (size_t)kStatsPerClip * B * (1 + stats_chunk_slots(max_l0));
}
// the two launches that fill it (frontend.hip.h); L0: conv-0 frames per clip (0 with lens), max_l0: the longest clip's
void launch_wav_stats(const float* wav, int ld, int L0, int max_l0, int B, double* stats, const int* lens, hipStream_t s) {
    const int nchunk = stats_chunk_slots(max_l0);
    double* part = stats + (size_t)kStatsPerClip * B;
    hipLaunchKernelGGL(wav_stats_kernel, dim3(nchunk, B), dim3(256), 0, s, wav, ld, L0, part, lens);
    hipLaunchKernelGGL(wav_stats_fold_kernel, dim3(B), dim3(128), 0, s, part, nchunk, L0, stats, lens);
}

// bytes of the operand / product buffers of the pos-conv in nested F(2,2) form (posconv_wino_f32.hip.h) over that many operand
// frames / rows of one operand
size_t pos_wino_q_bytes(long long q_frames) { return sizeof(float) * 16 * kPwOps * 48 * (size_t)q_frames; }
size_t pos_wino_s_bytes(long long q_rows) { return sizeof(float) * 16 * kPwOps * 48 * (size_t)q_rows; }

// The form an fp32 forward of this context runs its pos-conv in, and so which buffers its workspace holds for it: the direct
// 128-tap GEMM (none), the nested F(2,2) form (operands and products) or the frequency domain (the two spectra,
// posconv_fft_f32.hip.h).  A forward runs one form, so the layouts hold one form's buffers.
enum PosForm { kPosDirect = 0, kPosWino = 1, kPosFft = 2 };
PosForm pos_form(const nomad_ctx* c) { return c->tune.f32_posconv_fft ? kPosFft : c->tune.f32_posconv_wino ? kPosWino : kPosDirect; }

// floats in the split-K block of a small layer-output forward (Layout::splitk), 0 where that forward does not split: S x M x N
// for the largest transformer problem splitk_applies / posconv_splitk_applies let through at M = s.M frames (S x N <= 6144: fc1
// 2 x 3072, qkv 2 x 2304, fc2 / pos-conv 4 x 768), never more than the fixed cap those checks use.  The conv GEMMs of one clip
// have M = L[i] > s.M rows: they split only where their partials fit too (SplitKPlan::floats).
size_t layers_splitk_floats(const Shapes& s) {
    return s.M < kSplitKLayersMaxM ? std::min(kSplitKPartFloats, (size_t)6144 * (size_t)s.M) : 0;
}

struct Layout {
    size_t stats, scale, shift, conv[7], featln, xpad, x, x2, y, qkv, ctxb, h, splitk, pwq, pws, pfx, pfy, total;
};

Layout make_layout(const Shapes& s, bool keep, PosForm pos) {
    Layout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off += align_up(bytes);
        return o;
    };
    l.stats = take(sizeof(double) * stats_doubles(s.B, s.L[0]));
    l.scale = take(sizeof(float) * 512 * s.B);
    l.shift = take(sizeof(float) * 512 * s.B);
    auto conv_bytes = [&](int i) { return sizeof(float) * 512 * (size_t)s.B * s.L[i]; };
    if (keep) {
        for (int i = 0; i < 7; ++i) l.conv[i] = take(conv_bytes(i));
        l.featln = take(conv_bytes(6));
    } else {
        const size_t a = take(conv_bytes(0)), b = take(conv_bytes(1));
        for (int i = 0; i < 7; ++i) l.conv[i] = (i % 2 == 0) ? a : b;
        l.featln = b;  // conv6 lands in a; LN(512) writes to b
    }
    const size_t act = sizeof(float) * 768 * (size_t)s.M;
    l.xpad = take(sizeof(float) * 768 * (size_t)s.B * (s.T + 128));
    l.x = take(act);
    l.x2 = take(act);
    l.y = take(act);
    l.qkv = take(act * 3);
    l.ctxb = take(act);
    l.h = take(act * 4);
    // partial products of the split-K GEMMs of a small layer-output forward (forward_run): part of the CALL's workspace, so that
    // whether such a forward splits depends on its shape alone - not on which streams other calls are running on
    const size_t sk = layers_splitk_floats(s);
    l.splitk = sk ? take(sk * sizeof(float)) : 0;
    if (pos == kPosWino) {   // operands and products of the pos-conv in nested F(2,2) form
        const size_t q = (size_t)(s.T + kPwRate - 1) / kPwRate;
        l.pwq = take(pos_wino_q_bytes((long long)s.B * (q + kPwTaps - 1)));
        l.pws = take(pos_wino_s_bytes((long long)s.B * q));
    } else if (pos == kPosFft) {   // the spectra on either side of the bin products
        l.pfx = take(pos_fft_spec_bytes((long long)s.B * pos_fft_blocks(s.T)));
        l.pfy = take(pos_fft_spec_bytes((long long)s.B * pos_fft_blocks(s.T)));
    }
    l.total = off;
    return l;
}

// ---- ragged batches: clips of different lengths packed back to back ----------------------------------------
// The reference embeds files one at a time (nomad.py:171-183) because every file has its own length; zero-padding
// a batch would change GroupNorm statistics and the time mean.  Here clips of ANY lengths share one launch
// sequence with no padding: every per-frame tensor is packed [sum_c L_i(c)][channels], the transformer GEMMs and
// LayerNorms see plain packed rows, and only the kernels that care about clip boundaries (front end, conv row maps,
// pos-conv buffer, attention, head) read per-clip prefix sums.  Each row goes through exactly the arithmetic it
// would see at batch 1, so results are bit-identical to per-clip calls.
struct RaggedShapes {
    int B = 0, max_l0 = 0, max_t = 0, min_t = 1 << 30;
    long long rows[7] = {};   // total frames per conv level
    long long P = 0;          // total padded pos-conv frames, sum (T_c + 128)
    long long blocks = 0;     // total pos-conv frame blocks, sum ceil(T_c / kPosBlk) (bf16x3 path)
    long long pairs[5] = {};  // total output pairs of conv1 .. conv4 (Winograd form), sum ceil(L_i / 2)
    long long q_rows = 0, q_frames = 0;    // pos-conv in nested F(2,2) form: total operand rows, sum ceil(T_c / kPwRate), and frames, + kPwTaps - 1 each
                                           // (their prefix sums are formed on the device, in the call's workspace: posconv_wino_prefix_kernel)
    long long units = 0;                   // pos-conv in the frequency domain: total units, sum ceil(T_c / kPfBlk) (prefix sums: posconv_fft_prefix_kernel)
    long long even[4] = {}, odd[4] = {};   // backward: total even / odd frames of conv levels 0 .. 3, sum ceil(L_i / 2) / sum floor(L_i / 2)
    // [lens(B) | pref_0 (B+1) | ... | pref_6 (B+1) | ppref (B+1) | bpref (B+1) | pairpref_1 .. pairpref_4 (B+1) |
    //  upref_0 .. upref_6 | epref_0 .. epref_3 | opref_0 .. opref_3 (B+1 each)]: the last three groups are the backward's -
    //  upref_i[c] = pref_i[c] + 2 c, clip c's first row in a padded dU buffer of level i (every clip: L_i + 2 rows); epref_i /
    //  opref_i: prefix sums of the even (ceil(L_i / 2)) and odd (floor(L_i / 2)) frames of level i, the rows of the two GEMMs of a
    //  k = 3 / stride 2 transposed convolution
    std::vector<int> meta;
    size_t off_lens() const { return 0; }
    size_t off_pref(int i) const { return (size_t)B + (size_t)i * (B + 1); }
    size_t off_ppref() const { return (size_t)B + (size_t)7 * (B + 1); }
    size_t off_bpref() const { return (size_t)B + (size_t)8 * (B + 1); }
    size_t off_pairpref(int i) const { return (size_t)B + (size_t)(8 + i) * (B + 1); }   // i = 1 .. 4
    size_t off_upref(int i) const { return (size_t)B + (size_t)(13 + i) * (B + 1); }     // i = 0 .. 6
    size_t off_epref(int i) const { return (size_t)B + (size_t)(20 + i) * (B + 1); }     // i = 0 .. 3
    size_t off_opref(int i) const { return (size_t)B + (size_t)(24 + i) * (B + 1); }     // i = 0 .. 3
};

bool make_ragged(int B, const int* lens, RaggedShapes* r) {
    *r = RaggedShapes{};   // (the totals below accumulate)
    r->B = B;
    r->meta.assign((size_t)B + 28 * (size_t)(B + 1), 0);
    for (int c = 0; c < B; ++c) {
        Shapes sh;
        if (!make_shapes(1, lens[c], &sh)) return false;
        r->meta[c] = lens[c];
        for (int i = 0; i < 7; ++i) {
            r->meta[r->off_pref(i) + c + 1] = r->meta[r->off_pref(i) + c] + sh.L[i];
            r->rows[i] += sh.L[i];
        }
        for (int i = 1; i <= 4; ++i) {
            r->meta[r->off_pairpref(i) + c + 1] = r->meta[r->off_pairpref(i) + c] + (sh.L[i] + 1) / 2;
            r->pairs[i] += (sh.L[i] + 1) / 2;
        }
        for (int i = 0; i < 7; ++i) r->meta[r->off_upref(i) + c + 1] = r->meta[r->off_upref(i) + c] + sh.L[i] + 2;
        for (int i = 0; i < 4; ++i) {
            r->meta[r->off_epref(i) + c + 1] = r->meta[r->off_epref(i) + c] + (sh.L[i] + 1) / 2;
            r->meta[r->off_opref(i) + c + 1] = r->meta[r->off_opref(i) + c] + sh.L[i] / 2;
            r->even[i] += (sh.L[i] + 1) / 2;
            r->odd[i] += sh.L[i] / 2;
        }
        r->meta[r->off_ppref() + c + 1] = r->meta[r->off_ppref() + c] + sh.T + 128;
        r->P += sh.T + 128;
        const int q = (sh.T + kPwRate - 1) / kPwRate;
        r->q_rows += q;
        r->q_frames += q + kPwTaps - 1;
        r->units += pos_fft_blocks(sh.T);
        const int nb = (sh.T + kPosBlk - 1) / kPosBlk;
        r->meta[r->off_bpref() + c + 1] = r->meta[r->off_bpref() + c] + nb;
        r->blocks += nb;
        r->max_l0 = sh.L[0] > r->max_l0 ? sh.L[0] : r->max_l0;
        r->max_t = sh.T > r->max_t ? sh.T : r->max_t;
        r->min_t = sh.T < r->min_t ? sh.T : r->min_t;
    }
    return r->rows[0] < (1LL << 31) / 512 * 256;  // row counts stay well inside int
}

// The batch geometry every forward sequence reads its row maps, clip lengths and prefix sums from, so that one sequence per
// precision serves equal-length batches (geom_uniform) and ragged ones (geom_ragged).
struct BatchGeom {
    int B = 0;
    long long rows[7] = {};        // total frames per conv level; rows[6] = M
    long long pad_rows = 0;        // rows of one group of the padded pos-conv buffer
    long long grp_stride = 0;      // elements of one group of that buffer
    int max_l0 = 0, min_t = 0, max_t = 0;
    int wav_ld = 0;                // samples between clips of the wav buffer
    int L[7] = {}, T = 0;          // frames per clip and conv level, T = L[6]: equal-length batches; 0 when ragged (the kernels
                                   // read lens / prefixes instead)
    size_t meta_ints = 0;          // ragged: ints of the device metadata (RaggedShapes::meta); 0 for an equal-length batch
    const int* lens = kNoInts;     // ragged: device pointers into that metadata; kNoInts for an equal-length batch
    const int* pref[7] = {};       // frame prefix sums per conv level (pref[6]: the encoder's frames)
    const int* ppref = kNoInts;    // padded pos-conv frame prefix sums
    RowMap conv_amap[7] = {};      // im2col rows of conv layer i over the output of layer i - 1
    long long pairs[5] = {};       // output pairs of conv1 .. conv4 in polyphase Winograd form (fp32)
    const int* pairpref[5] = {};   // ragged: their prefix sums
    RowMap pad_map{};              // post_extract_proj output rows in the group-major, padded pos-conv buffer
    RowMap pos_amap{};             // fp32 / bf16 pos-conv rows: row (clip, t) starts at padded frame t, taps are contiguous
    // bf16x3 pos-conv as a GEMM over blocks of kPosBlk frames: input rows, output rows (in y), residual rows
    long long pos_blocks = 0;
    RowMap blk_amap{}, blk_cmap{}, blk_rmap{};
    PosWinoGeom pos_wino{};        // the fp32 pos-conv in nested F(2,2) form (posconv_wino_f32.hip.h)
    PosFftGeom pos_fft{};          // ... and in the frequency domain (posconv_fft_f32.hip.h)
    double attn_flops = 0.0;
    // the backward's: padded dU rows, even / odd frames of conv levels 0 .. 3 and their prefix sums (ragged), and the HOST copy of
    // the encoder's frame prefix sums (ragged; LayerDrop branches are clip ranges) - valid as long as the RaggedShapes it came from
    const int* upref[7] = {};
    const int* epref[4] = {};
    const int* opref[4] = {};
    long long even[4] = {}, odd[4] = {};
    const int* host_tpref = nullptr;
    bool ragged() const { return meta_ints != 0; }
    long long clip_row0(int c) const { return host_tpref ? host_tpref[c] : (long long)c * T; }   // first encoder frame of clip c
};

// allocates nothing: the equal-length forwards build one per call
BatchGeom geom_uniform(const Shapes& sh) {
    BatchGeom g;
    g.B = sh.B;
    for (int i = 0; i < 7; ++i) {
        g.rows[i] = (long long)sh.B * sh.L[i];
        g.L[i] = sh.L[i];
    }
    g.pad_rows = (long long)sh.B * (sh.T + 128);
    g.grp_stride = g.pad_rows * 48;
    g.max_l0 = sh.L[0];
    g.min_t = g.max_t = g.T = sh.T;
    g.wav_ld = sh.N;
    const long long pad_ld = (long long)(sh.T + 128) * 48;
    for (int i = 1; i < 7; ++i) g.conv_amap[i] = RowMap{0, (long long)sh.L[i - 1] * 512, sh.L[i], kConvS[i] * 512};
    for (int i = 1; i <= 4; ++i) g.pairs[i] = (long long)sh.B * ((sh.L[i] + 1) / 2);
    g.pad_map = RowMap{64LL * 48, pad_ld, sh.T, 48};
    g.pos_amap = RowMap{0, pad_ld, sh.T, 48};
    const int nb = (sh.T + kPosBlk - 1) / kPosBlk;
    g.pos_blocks = (long long)sh.B * nb;
    g.blk_amap = RowMap{0, pad_ld, nb, kPosBlk * 48};
    g.blk_rmap = RowMap{64LL * 48, pad_ld, nb, kPosBlk * 48};
    g.blk_cmap = RowMap{0, (long long)sh.T * 768, nb, kPosBlk * 768};
    g.attn_flops = 4.0 * sh.B * 12.0 * (double)sh.T * sh.T * 64;
    const int q = (sh.T + kPwRate - 1) / kPwRate;
    g.pos_wino = PosWinoGeom{sh.B, sh.T, nullptr, nullptr, nullptr, nullptr, g.pad_rows, (long long)sh.B * q, (long long)sh.B * (q + kPwTaps - 1), q};
    g.pos_fft = PosFftGeom{sh.B, sh.T, nullptr, nullptr, nullptr, g.pad_rows, sh.B * pos_fft_blocks(sh.T), pos_fft_blocks(sh.T)};
    for (int i = 0; i < 4; ++i) {
        g.even[i] = (long long)sh.B * ((sh.L[i] + 1) / 2);
        g.odd[i] = (long long)sh.B * (sh.L[i] / 2);
    }
    return g;
}

// meta: the device copy of rs.meta, which the row maps point into (nullptr: sizing only)
BatchGeom geom_ragged(const RaggedShapes& rs, int stride, const int* meta) {
    BatchGeom g;
    g.B = rs.B;
    for (int i = 0; i < 7; ++i) g.rows[i] = rs.rows[i];
    g.pad_rows = rs.P;
    g.grp_stride = rs.P * 48;
    g.max_l0 = rs.max_l0;
    g.min_t = rs.min_t;
    g.max_t = rs.max_t;
    g.wav_ld = stride;
    g.meta_ints = rs.meta.size();
    auto at = [&](size_t off) { return meta ? meta + off : nullptr; };
    g.lens = at(rs.off_lens());
    for (int i = 0; i < 7; ++i) g.pref[i] = at(rs.off_pref(i));
    g.ppref = at(rs.off_ppref());
    for (int i = 1; i < 7; ++i) g.conv_amap[i] = RowMap{0, 0, 0, kConvS[i] * 512, g.pref[i], g.pref[i - 1], rs.B, 512};
    for (int i = 1; i <= 4; ++i) {
        g.pairs[i] = rs.pairs[i];
        g.pairpref[i] = at(rs.off_pairpref(i));
    }
    g.pad_map = RowMap{64LL * 48, 0, 0, 48, g.pref[6], g.ppref, rs.B, 48};
    g.pos_amap = RowMap{0, 0, 0, 48, g.pref[6], g.ppref, rs.B, 48};
    const int* bpref = at(rs.off_bpref());
    g.pos_blocks = rs.blocks;
    g.blk_amap = RowMap{0, 0, 0, kPosBlk * 48, bpref, g.ppref, rs.B, 48};
    g.blk_rmap = RowMap{64LL * 48, 0, 0, kPosBlk * 48, bpref, g.ppref, rs.B, 48};
    g.blk_cmap = RowMap{0, 0, 0, kPosBlk * 768, bpref, g.pref[6], rs.B, 768};
    for (int i = 0; i < 7; ++i) g.upref[i] = at(rs.off_upref(i));
    for (int i = 0; i < 4; ++i) {
        g.epref[i] = at(rs.off_epref(i));
        g.opref[i] = at(rs.off_opref(i));
        g.even[i] = rs.even[i];
        g.odd[i] = rs.odd[i];
    }
    g.pos_wino = PosWinoGeom{rs.B, 0, g.pref[6], g.ppref, nullptr, nullptr, rs.P, rs.q_rows, rs.q_frames,
                             (rs.max_t + kPwRate - 1) / kPwRate};
    g.pos_fft = PosFftGeom{rs.B, 0, g.pref[6], g.ppref, nullptr, rs.P, (int)rs.units, pos_fft_blocks(rs.max_t)};
    g.host_tpref = rs.meta.data() + rs.off_pref(6);
    for (int i = 0; i < rs.B; ++i) {
        const double t = rs.meta[rs.off_pref(6) + i + 1] - rs.meta[rs.off_pref(6) + i];
        g.attn_flops += 4.0 * 12.0 * t * t * 64;
    }
    return g;
}

// Workspace of every forward except the fp32 equal-length one (Layout): the ragged metadata, the front end's statistics, two
// ping-pong conv buffers and the activations, elem_bytes per element (bf16: 2; fp32 or two bf16 planes: 4).
struct ActLayout {
    size_t meta, stats, scale, shift, conva, convb, xpad, x, x2, y, qkv, ctxb, h, pwq, pws, pwmeta, pfx, pfy, pfmeta, total;
    long long capa, capb;  // elements per plane of the two conv ping-pong buffers
    long long xpad_plane;  // elements per plane of the padded pos-conv buffer, + xpad_slack zeroed elements (bf16x3)
};

// pos: the fp32 forward with its pos-conv in nested F(2,2) form or in the frequency domain - the buffers of that form.
ActLayout make_act_layout(const BatchGeom& g, size_t elem_bytes, size_t xpad_slack, PosForm pos = kPosDirect) {
    ActLayout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off += align_up(bytes);
        return o;
    };
    const size_t e = elem_bytes, M = (size_t)g.rows[6];
    l.capa = 512LL * g.rows[0];
    l.capb = 512LL * g.rows[1];
    l.meta = take(sizeof(int) * g.meta_ints);
    l.stats = take(sizeof(double) * stats_doubles(g.B, g.max_l0));
    l.scale = take(sizeof(float) * 512 * g.B);
    l.shift = take(sizeof(float) * 512 * g.B);
    l.conva = take(e * l.capa);
    l.convb = take(e * l.capb);
    l.xpad_plane = 768LL * g.pad_rows + (long long)xpad_slack;
    l.xpad = take(e * (size_t)l.xpad_plane);
    l.x = take(e * 768 * M);
    l.x2 = take(e * 768 * M);
    l.y = take(e * 768 * M);
    l.qkv = take(e * 2304 * M);
    l.ctxb = take(e * 768 * M);
    l.h = take(e * 3072 * M);
    if (pos == kPosWino) {
        l.pwq = take(pos_wino_q_bytes(g.pos_wino.q_frames));
        l.pws = take(pos_wino_s_bytes(g.pos_wino.q_rows));
        l.pwmeta = take(sizeof(int) * 2 * (size_t)(g.B + 1));   // ragged: operand row / frame prefix sums
    } else if (pos == kPosFft) {
        l.pfx = take(pos_fft_spec_bytes(g.pos_fft.units));
        l.pfy = take(pos_fft_spec_bytes(g.pos_fft.units));
        l.pfmeta = take(sizeof(int) * (size_t)(g.B + 1));       // ragged: unit prefix sums
    }
    l.total = off;
    return l;
}

struct RaggedBatch {
    RaggedShapes rs;
    BatchGeom g;
    ActLayout lay;
};

constexpr unsigned kMetaRing = 16;   // staged host copies of ragged metadata (nomad_ctx::ragged_meta_ring)

// What every ragged entry point does first, in three steps that the forwards run through ragged_prologue and the training-mode
// forward / the backward run one by one (their own size checks sit between the second and the third).  Errors name `who`.
// 1. ragged_shapes: the argument checks (ok: the caller's own) and the prefix sums; stride >= 0: no clip longer than its row.
int ragged_shapes(const char* who, bool ok, int B, int stride, const int* lens_host, RaggedShapes* rs) {
    if (!ok || !lens_host || B <= 0 || !make_ragged(B, lens_host, rs)) return fail(NOMAD_ERR_INVALID, "%s: bad argument (B=%d)", who, B);
    for (int i = 0; stride >= 0 && i < B; ++i)
        if (lens_host[i] > stride) return fail(NOMAD_ERR_INVALID, "%s: clip %d longer than the row stride", who, i);
    return 0;
}
// 2. the geometry without device pointers (geom_ragged(rs, stride, nullptr)) and the caller's layout over it: sizing.
// 3. ragged_upload: the metadata's copy to `meta` (inside the call's workspace), queued on s ahead of every kernel of the call, and
//    the geometry over that copy.  The host copy must outlive the asynchronous transfer: it is staged in a ring of kMetaRing vectors
//    in the context.  A loss step with a gradient to both arguments queues four such copies (two forwards, two backwards), a
//    fine-tuning step two, so a slot is written again only kMetaRing / 4 = 4 steps later - and a later step's calls are queued
//    behind this one's kernels on the caller's stream, which consume the metadata's device copy long before.
int ragged_upload(nomad_ctx* c, const RaggedShapes& rs, int stride, int* meta, hipStream_t s, BatchGeom* g) {
    std::vector<int>& staged = c->ragged_meta_ring[c->ragged_seq++ % kMetaRing];
    staged = rs.meta;
    HIP_TRY(hipMemcpyAsync(meta, staged.data(), sizeof(int) * staged.size(), hipMemcpyHostToDevice, s));
    *g = geom_ragged(rs, stride, meta);
    return 0;
}

// The span table of nomad_embed_spans* travels the same way: checked and laid out on the host (spans_stage), its device copy queued
// by span_upload right behind the ragged metadata's - after every check of the call, ahead of its kernels - from a ring slot of its
// own: a span call takes two slots, so a score_spans step with a gradient (one forward, one backward) takes the four of ragged_upload.
struct SpanStage {
    std::vector<int> host;  // laid out as the device block: head.hip.h, span_table
    int* dev = nullptr;     // the head of the caller's scratch
    int R = 0, S = 0;
    float* gw = nullptr;    // [R][768] behind the table: the backward's per-row gradients
};
int span_upload(nomad_ctx* c, const SpanStage& st, hipStream_t s) {
    std::vector<int>& staged = c->ragged_meta_ring[c->ragged_seq++ % kMetaRing];
    staged = st.host;
    HIP_TRY(hipMemcpyAsync(st.dev, staged.data(), sizeof(int) * staged.size(), hipMemcpyHostToDevice, s));
    return 0;
}

// The scoring forwards' prologue: the three steps over the ActLayout.  c == nullptr: nomad_workspace_bytes_ragged*, sizing only.
int ragged_prologue(const char* who, nomad_ctx* c, bool ok, int B, int stride, const int* lens_host, size_t elem_bytes,
                    size_t xpad_slack, RaggedBatch* r, void* workspace = nullptr, size_t workspace_bytes = 0, hipStream_t s = nullptr,
                    PosForm pos = kPosDirect) {
    if (int rc = ragged_shapes(who, ok, B, c ? stride : -1, lens_host, &r->rs)) return rc;
    r->g = geom_ragged(r->rs, stride, nullptr);
    r->lay = make_act_layout(r->g, elem_bytes, xpad_slack, pos);
    if (!c) return 0;
    if (workspace_bytes < r->lay.total)
        return fail(NOMAD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", who, workspace_bytes, r->lay.total);
    return ragged_upload(c, r->rs, stride, reinterpret_cast<int*>(static_cast<char*>(workspace) + r->lay.meta), s, &r->g);
}

// What a training-mode forward keeps for the backward pass (all fp32, carved from the caller's `saved` block).
struct SavedLayer {
    float *qkv, *ctx, *lse, *y1, *u, *y2;
};
struct Saved {
    float *gn_scale, *gn_shift, *gn_mean, *gn_rstd;
    float* u[7];   // pre-GELU conv outputs, layers 1..6, compact [B][L_i][512]
    float* c6;     // conv6 post-GELU output = LayerNorm(512) input
    float *y0, *upc;  // encoder LayerNorm input, pos-conv pre-GELU
    SavedLayer L[NOMAD_NUM_LAYERS];
    size_t total;
};

Saved make_saved(const BatchGeom& s, void* base) {
    Saved v{};
    size_t off = 0;
    char* b = static_cast<char*>(base);
    auto take = [&](size_t floats) {
        float* ptr = reinterpret_cast<float*>(b + off);
        off += align_up(floats * sizeof(float));
        return ptr;
    };
    const size_t M = (size_t)s.rows[6];
    v.gn_scale = take(512 * (size_t)s.B);
    v.gn_shift = take(512 * (size_t)s.B);
    v.gn_mean = take(512 * (size_t)s.B);
    v.gn_rstd = take(512 * (size_t)s.B);
    for (int i = 1; i < 7; ++i) v.u[i] = take(512 * (size_t)s.rows[i]);
    v.c6 = take(512 * M);
    v.y0 = take(768 * M);
    v.upc = take(768 * M);
    for (int l = 0; l < NOMAD_NUM_LAYERS; ++l) {
        v.L[l].qkv = take(2304 * M);
        v.L[l].ctx = take(768 * M);
        v.L[l].lse = take(12 * M);
        v.L[l].y1 = take(768 * M);
        v.L[l].u = take(3072 * M);
        v.L[l].y2 = take(768 * M);
    }
    v.total = off;
    return v;
}

// Scratch of nomad_embed_backward.  train = true adds what the parameter gradients need (nomad_train_backward):
// two transposed operand buffers [3072][Mp], split-K partial products, the recomputed pos-conv input.
struct BwdLayout {
    size_t meta, gx, dya, dyb, dh, dqkv, dug, f1, f2, bufa, bufb, partial, gnfold, cwtab, attnd, total;   // meta: ragged batches only
    int nchunks, nstat;   // frame chunks of the conv0 parameter-gradient pass / of the GroupNorm-backward statistics pass
    size_t ta, tb, kpart, xg, dwe, lnpart, headp, headdz, dmask;
    int Mp, pos_split, ln_blocks;
    size_t h0, convtmp, c0part;  // trainable conv feature extractor: recomputed conv0 output, one layer's dW, conv0 partials
    long long conv_cols;         // columns of the conv layers' transposed operands: B * ceil512(L_1)
};

constexpr size_t kSplitPartFloats = (size_t)16 * 2304 * 768;  // >= S * Nout * Kin for every split chosen below

inline long long conv_lp(int L) { return ((long long)L + 511) / 512 * 512; }  // a clip's columns in the conv dW operands

BwdLayout make_bwd_layout(const BatchGeom& s, bool train = false, bool train_conv = false) {
    BwdLayout l{};
    size_t off = 0;
    auto take = [&](size_t floats) {
        size_t o = off;
        off += align_up(floats * sizeof(float));
        return o;
    };
    const size_t M = (size_t)s.rows[6];
    l.meta = take(sizeof(int) * s.meta_ints / sizeof(float));   // (nothing for an equal-length batch)
    l.gx = take(768 * M);
    l.dya = take(768 * M);
    l.dyb = take(768 * M);
    l.dh = take(3072 * M);
    l.dqkv = take(2304 * M);
    l.dug = take(768 * (size_t)s.pad_rows);
    l.f1 = take(512 * M);
    l.f2 = take(512 * M);
    l.bufa = take(512 * (size_t)(s.rows[0] + 2LL * s.B));
    l.bufb = take(512 * (size_t)(s.rows[1] + 2LL * s.B));
    l.nchunks = (s.max_l0 + kGnChunk - 1) / kGnChunk;
    l.nstat = (s.max_l0 + kGnStatsChunk - 1) / kGnStatsChunk;
    l.partial = take(1024 * (size_t)s.B * l.nstat);
    l.gnfold = take(1024 * (size_t)s.B);
    l.cwtab = take((size_t)512 * 16 * s.B);
    l.attnd = take(12 * M);
    if (train) {
        l.Mp = ((int)M + 511) / 512 * 512;  // contraction length of the dW GEMMs: any split S | 16 keeps K % 32 == 0
        l.pos_split = s.B < 4 ? s.B : 4;
        l.ln_blocks = ((int)M + kLnRows - 1) / kLnRows;
        // conv dW GEMMs (freeze_convnet: False): dU^T [512][cols] and the transposed im2col [taps * 512][cols]
        l.conv_cols = train_conv ? (long long)s.B * conv_lp(s.L[1]) : 0;
        l.ta = take(std::max((size_t)3072 * l.Mp, (size_t)(512 * l.conv_cols)));
        l.tb = take(std::max((size_t)3072 * l.Mp, (size_t)(1536 * l.conv_cols)));
        const size_t pos_part = (size_t)l.pos_split * 16 * 128 * 2304;
        l.kpart = take(pos_part > kSplitPartFloats ? pos_part : kSplitPartFloats);
        l.xg = take(768 * (size_t)s.pad_rows);
        l.dwe = take((size_t)768 * 6144);
        l.lnpart = take(std::max((size_t)l.ln_blocks * 2 * 768, (size_t)16 * kPbChunks * 48));  // also the pos-conv bias partials
        l.headp = take((size_t)s.B * 768);
        l.headdz = take((size_t)s.B * 256);
        l.dmask = take(768 * M);
        if (train_conv) {
            l.h0 = take(512 * (size_t)s.rows[0]);
            l.convtmp = take((size_t)512 * 1536);
            l.c0part = take((size_t)5120 * s.B * l.nchunks);
        }
    }
    l.total = off;
    return l;
}

// The master parameters as ONE flat fp32 vector: every parameter of nomad_best_model.pt that train_triplet.py can train
// (mask_emb gets no gradient with mask=False) - encoder front, the 12 layers, the conv feature extractor, the head last, so that
// `emb_w` splits body from head.  Gradients and the Adam moments use the same offsets.  q/k/v of a layer are stored fused
// [q | k | v] in checkpoint scale.
struct LayerOffsets {
    size_t qkv_w, qkv_b, o_w, o_b, ln1_w, ln1_b, fc1_w, fc1_b, fc2_w, fc2_b, ln2_w, ln2_b;
};
struct ParamOffsets {
    size_t fln_w, fln_b, proj_w, proj_b, pos_g, pos_v, pos_b, eln_w, eln_b;
    LayerOffsets L[NOMAD_NUM_LAYERS];
    size_t conv0_w, gn_w, gn_b, conv_w[7];  // the conv feature extractor (checkpoint layout [co][ci][tap]): its slices keep a zero
                                            // gradient unless nomad_train_set_convnet(ctx, 1) (config freeze_convnet: False)
    size_t emb_w, emb_b, total;
};

// One tensor of the checkpoint, as for_each_param visits it.
struct Param {
    std::string key;    // checkpoint key (nomad_train_segment)
    size_t count;       // floats
    const float* host;  // where it sits in nomad_weights
    size_t* slot;       // its offset in the master vector is *slot + sub (sub != 0: k and v inside the fused [q | k | v])
    size_t sub;
    float** alias;      // the context pointer the engine reads it through when that is the tensor as it stands (uploaded as it
                        // is by nomad_create, pointed at the master vector by nomad_train_enable); nullptr where the engine reads
                        // a derived copy: q/k/v (fused, q scaled), pos_g / pos_v (weight norm folded), conv1..6 (repacked)
};

// THE parameter inventory, in the master vector's order: everything that uploads, lays out, names or aliases the checkpoint's
// parameters walks it.  w, po, c: the structures the visits point into (a walk that needs only names and sizes passes blanks).
template <class F>
void for_each_param(const nomad_weights& w, ParamOffsets& po, nomad_ctx& c, F&& f) {
    auto v = [&](const std::string& key, size_t n, const float* host, size_t& slot, float** alias, size_t sub = 0) {
        f(Param{key, n, host, &slot, sub, alias});
    };
    const std::string p = "ssl_model.";
    v(p + "layer_norm.weight", 512, w.feat_ln_w, po.fln_w, &c.fln_w);
    v(p + "layer_norm.bias", 512, w.feat_ln_b, po.fln_b, &c.fln_b);
    v(p + "post_extract_proj.weight", 768 * 512, w.proj_w, po.proj_w, &c.proj_w);
    v(p + "post_extract_proj.bias", 768, w.proj_b, po.proj_b, &c.proj_b);
    v(p + "encoder.pos_conv.0.weight_g", 128, w.pos_g, po.pos_g, nullptr);
    v(p + "encoder.pos_conv.0.weight_v", (size_t)768 * 48 * 128, w.pos_v, po.pos_v, nullptr);
    v(p + "encoder.pos_conv.0.bias", 768, w.pos_b, po.pos_b, &c.pos_b);
    v(p + "encoder.layer_norm.weight", 768, w.enc_ln_w, po.eln_w, &c.eln_w);
    v(p + "encoder.layer_norm.bias", 768, w.enc_ln_b, po.eln_b, &c.eln_b);
    for (int l = 0; l < NOMAD_NUM_LAYERS; ++l) {
        const nomad_layer_weights& lw = w.layers[l];
        LayerOffsets& lo = po.L[l];
        LayerDev& d = c.layers[l];
        const std::string b = p + "encoder.layers." + std::to_string(l) + ".";
        const size_t ww = 768 * 768;
        v(b + "self_attn.q_proj.weight", ww, lw.q_w, lo.qkv_w, nullptr);
        v(b + "self_attn.k_proj.weight", ww, lw.k_w, lo.qkv_w, nullptr, ww);
        v(b + "self_attn.v_proj.weight", ww, lw.v_w, lo.qkv_w, nullptr, 2 * ww);
        v(b + "self_attn.q_proj.bias", 768, lw.q_b, lo.qkv_b, nullptr);
        v(b + "self_attn.k_proj.bias", 768, lw.k_b, lo.qkv_b, nullptr, 768);
        v(b + "self_attn.v_proj.bias", 768, lw.v_b, lo.qkv_b, nullptr, 1536);
        v(b + "self_attn.out_proj.weight", ww, lw.o_w, lo.o_w, &d.o_w);
        v(b + "self_attn.out_proj.bias", 768, lw.o_b, lo.o_b, &d.o_b);
        v(b + "self_attn_layer_norm.weight", 768, lw.ln1_w, lo.ln1_w, &d.ln1_w);
        v(b + "self_attn_layer_norm.bias", 768, lw.ln1_b, lo.ln1_b, &d.ln1_b);
        v(b + "fc1.weight", (size_t)3072 * 768, lw.fc1_w, lo.fc1_w, &d.fc1_w);
        v(b + "fc1.bias", 3072, lw.fc1_b, lo.fc1_b, &d.fc1_b);
        v(b + "fc2.weight", (size_t)768 * 3072, lw.fc2_w, lo.fc2_w, &d.fc2_w);
        v(b + "fc2.bias", 768, lw.fc2_b, lo.fc2_b, &d.fc2_b);
        v(b + "final_layer_norm.weight", 768, lw.ln2_w, lo.ln2_w, &d.ln2_w);
        v(b + "final_layer_norm.bias", 768, lw.ln2_b, lo.ln2_b, &d.ln2_b);
    }
    const std::string fe = p + "feature_extractor.conv_layers.";
    v(fe + "0.0.weight", 512 * 10, w.conv_w[0], po.conv0_w, &c.conv0_w);
    v(fe + "0.2.weight", 512, w.gn_w, po.gn_w, &c.gn_w);
    v(fe + "0.2.bias", 512, w.gn_b, po.gn_b, &c.gn_b);
    for (int i = 1; i < 7; ++i) v(fe + std::to_string(i) + ".0.weight", (size_t)512 * 512 * kConvK[i], w.conv_w[i], po.conv_w[i], nullptr);
    v("embedding_layer.1.weight", 256 * 768, w.emb_w, po.emb_w, &c.emb_w);
    v("embedding_layer.1.bias", 256, w.emb_b, po.emb_b, &c.emb_b);
}

// Checkpoint key -> slice of the master vector (nomad_train_segment), and the offsets the kernels' call sites use: one walk, once.
struct Segment {
    std::string name;
    size_t offset, count;
};
struct ParamTable {
    ParamOffsets off;
    std::vector<Segment> segs;
};
const ParamTable& param_table() {
    static const ParamTable table = [] {
        ParamTable t{};
        const nomad_weights no_weights{};
        nomad_ctx no_ctx;   // only addresses are formed
        size_t off = 0;
        for_each_param(no_weights, t.off, no_ctx, [&](const Param& p) {
            if (p.sub == 0) *p.slot = off;
            t.segs.push_back({p.key, off, p.count});
            off += p.count;  // every segment is a multiple of 4 floats: 16-byte alignment is preserved
        });
        t.off.total = off;
        return t;
    }();
    return table;
}
const ParamOffsets& param_offsets() { return param_table().off; }
const std::vector<Segment>& segments() { return param_table().segs; }

// Every device buffer a context owns comes from here: allocated once - a pointer that is already set is kept, so an enable call
// that is repeated after a weight update, or retried after a failure, allocates nothing twice - optionally cleared, and recorded
// for nomad_destroy.
template <class T>
int dev_alloc(nomad_ctx* c, const char* who, size_t n, T** out, bool zero = false) {
    if (*out) return 0;
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, n * sizeof(T));
    if (e == hipSuccess && zero && (e = hipMemset(d, 0, n * sizeof(T))) != hipSuccess) (void)hipFree(d);
    if (e != hipSuccess) return fail(NOMAD_ERR_HIP, "%s: %zu bytes of device memory: %s", who, n * sizeof(T), hipGetErrorString(e));
    c->allocs.push_back(d);
    *out = static_cast<T*>(d);
    return 0;
}

int upload(nomad_ctx* c, const char* who, const float* host, size_t n, float** out) {
    if (int rc = dev_alloc(c, who, n, out)) return rc;
    HIP_TRY(hipMemcpy(*out, host, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// One GEMM weight of the model and the copies the other paths keep of it; a copy that a weight does not have is a null slot.
struct GemmWeight {
    const float* w;  // fp32 in kernel layout [N][K]: what the fp32 forward contracts with
    int N, K;
    bf16_t** w16;    // nomad_enable_bf16
    bf16s_t** wx;    // nomad_enable_bf16x3: hi | lo bf16 planes
    float** wT;      // build_backward_weights: [K][N]
};

// THE list of GEMM weights: f(GemmWeight) -> error code; the walk ends at the first failure.
template <class F>
int for_each_gemm_weight(nomad_ctx* c, F&& f) {
    int rc = 0;
    auto v = [&](const float* w, int N, int K, bf16_t** w16, bf16s_t** wx, float** wT) {
        if (rc == 0) rc = f(GemmWeight{w, N, K, w16, wx, wT});
    };
    for (int i = 1; i < 7; ++i)  // (their dX copies are cut by tap, not one transpose: build_backward_weights)
        v(c->conv_w[i], 512, kConvK[i] * 512, &c->conv_w16[i], &c->conv_wx[i], nullptr);
    v(c->proj_w, 768, 512, &c->proj_w16, &c->proj_wx, &c->proj_wT);
    for (int l = 0; l < NOMAD_NUM_LAYERS; ++l) {
        const LayerDev& d = c->layers[l];
        v(d.qkv_w, 2304, 768, &c->qkv_w16[l], &c->qkv_wx[l], &c->qkv_wT[l]);
        v(d.o_w, 768, 768, &c->o_w16[l], &c->o_wx[l], &c->o_wT[l]);
        v(d.fc1_w, 3072, 768, &c->fc1_w16[l], &c->fc1_wx[l], &c->fc1_wT[l]);
        v(d.fc2_w, 768, 3072, &c->fc2_w16[l], &c->fc2_wx[l], &c->fc2_wT[l]);
    }
    return rc;
}

void transpose(const float* in, int ld_in, float* out, int ld_out, int R, int C, hipStream_t s) {  // out[C][R] = in[R][C]^T
    hipLaunchKernelGGL(transpose_kernel, dim3((C + 31) / 32, (R + 31) / 32), dim3(32, 8), 0, s, in, ld_in, out, ld_out, R, C);
}

// Every weight copy the dX chain of the backward contracts with, from the kernel-layout forward weights, queued on s
// (nomad_enable_backward: the null stream; refresh_weights: the caller's).  The buffers are nomad_enable_backward's.
void build_backward_weights(nomad_ctx* c, hipStream_t s) {
    for (int i = 1; i <= 4; ++i) {  // k = 3: forward repack is [n][tap*512 + c]
        transpose(c->conv_w[i] + 2 * 512, 1536, c->conv_bw_even[i], 1024, 512, 512, s);        // tap 2 pairs with dU[t'-1]
        transpose(c->conv_w[i], 1536, c->conv_bw_even[i] + 512, 1024, 512, 512, s);            // tap 0 pairs with dU[t']
        transpose(c->conv_w[i] + 512, 1536, c->conv_bw_odd[i], 512, 512, 512, s);              // tap 1
    }
    for (int i = 5; i <= 6; ++i)  // k = 2: [n][tap*512 + c] -> [(tap*512 + c)][n]
        transpose(c->conv_w[i], 1024, c->conv_bw2[i], 512, 512, 1024, s);
    hipLaunchKernelGGL(posconv_bwd_weight_kernel, dim3(16 * 64), dim3(256), 0, s, c->pos_w, c->pos_wb);
    (void)for_each_gemm_weight(c, [&](const GemmWeight& g) {
        if (g.wT) transpose(g.w, g.K, *g.wT, g.N, g.N, g.K, s);
        return 0;
    });
}


// Small-M dense GEMMs of the loss forward / backward (config C4: M = 1600): N = 768 is 300 tiles of 64 x 64 on 256 CUs,
// 44 CUs get two tiles and the launch takes two tiles' time (fc2: 82 us where a balanced split would take 48).  The
// contraction is cut into S fixed slices - S x as many, shorter workgroups - whose partial products are added in slice
// order by splitk_epilogue_kernel together with bias / GELU / residual: deterministic, no atomics.
// Whether a GEMM splits is a function of the call's plan and the problem alone.
static bool splitk_applies(const SplitKPlan& plan, const GemmParams& p, int groups, int tile, int* S) {
    if (!plan.part || groups != 1 || tile != 37) return false;
    if (p.DG || p.Upre || p.c_colblk || p.kchunk != p.K || p.n_valid != p.N || p.N % 64) return false;
    const bool c_plain = p.cmap.clip_rows >= p.M && p.cmap.off == 0 && p.cmap.ld == p.N;
    const bool r_plain = !p.R || (p.rmap.clip_rows >= p.M && p.rmap.off == 0 && p.rmap.ld == p.N);
    if (!c_plain || !r_plain || p.amap.clip_rows < p.M) return false;
    const long long tiles = (long long)((p.M + 63) / 64) * (p.N / 64);
    if (tiles >= 512 || p.K < 768) return false;
    *S = p.K >= 2304 ? 4 : 2;
    // S x M x N partials must fit the block being written: layers_splitk_floats sizes a layer-output forward's by the transformer
    // GEMMs, and a one-clip conv GEMM (M = L[i] rows, several times the frames) can exceed it
    return p.K % (*S * 32) == 0 && (size_t)*S * p.N <= 6144 && (size_t)*S * p.M * p.N <= plan.floats;
}

// The S slices (ordinary launches: straight to the dispatch), then the epilogue - the one place that decides whether it also does the
// row operation behind the GEMM (fuse), and the one place that reads the two Tuning switches.
static int run_gemm_splitk(nomad_ctx* c, const SplitKPlan& plan, const GemmParams& p, int S, hipStream_t s, const SplitKFusion* fuse,
                           bool* fused) {
    GemmParams q = p;
    q.K = p.K / S;
    q.kchunk = q.K;
    q.a_goff = q.K;
    q.w_goff = q.K;
    q.C = plan.part;
    q.cmap = plain_map(p.M, p.N);
    q.c_goff = (long long)p.M * p.N;
    q.bias = nullptr;
    q.R = nullptr;
    q.gelu = 0;
    if (int rc = gemm_f32_dispatch(c, q, S, 37, s)) return rc;
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    if (fuse && fuse->kind == SplitKFusion::kLnBwd && p.N == 768 && !p.gelu && !p.bias && c->tune.splitk_lnb_fuse) {
        hipLaunchKernelGGL((layernorm_bwd_kernel<3, true>), dim3((unsigned)((p.M + 3) / 4)), dim3(256), 0, s, fuse->x, plan.part,
                           fuse->g2, fuse->gamma, fuse->out, p.M, S, p.R);
        HIP_TRY(hipGetLastError());
        *fused = true;
        return 0;
    }
    if (fuse && fuse->kind == SplitKFusion::kLn && p.N == 768 && !p.gelu && c->tune.splitk_ln_fuse) {
        hipLaunchKernelGGL(splitk_epilogue_ln_kernel, dim3((unsigned)((p.M + 3) / 4)), dim3(256), 0, s, plan.part, S, p.M, p.bias, p.R, p.C,
                           fuse->gamma, fuse->beta, fuse->out, fuse->out2);
        HIP_TRY(hipGetLastError());
        *fused = true;
        return 0;
    }
    const long long count4 = (long long)p.M * p.N / 4;
    hipLaunchKernelGGL(splitk_epilogue_kernel, dim3((unsigned)((count4 + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(plan.part), S, count4, p.N / 4, reinterpret_cast<const float4*>(p.bias),
                       reinterpret_cast<const float4*>(p.R), reinterpret_cast<float4*>(p.C), p.gelu);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The grouped pos-conv (16 groups x [M x 48 x 6144]) at the loss path's M = 1600 is 7 row tiles x 16 groups = 112 workgroups with a
// serial K loop of 384 tiles: 331 us per launch on fewer than half of the CUs (three launches per configs[3] step).  K in 4 fixed
// slices over blockIdx.z (448 workgroups), partial products added in slice order by posconv_splitk_epilogue_kernel.  Where the
// dense GEMMs of the same call split (splitk_applies): never on a scoring entry point.
static bool posconv_splitk_applies(const SplitKPlan& plan, const GemmParams& p, int groups, int tile) {
    if (!plan.part || groups != 16 || tile != 48) return false;
    if (p.DG || p.K != 6144 || p.kchunk != p.K || p.n_valid != 48 || p.c_goff != 48) return false;
    const bool c_plain = p.cmap.clip_rows >= p.M && p.cmap.off == 0 && p.cmap.ld == 768;
    return c_plain && (long long)((p.M + 255) / 256) * 16 < 256 && (size_t)4 * p.M * 768 <= plan.floats;
}

static int run_posconv_splitk(nomad_ctx* c, const SplitKPlan& plan, const GemmParams& p, hipStream_t s) {
    constexpr int S = 4;
    GemmParams q = p;
    q.K = p.K / S;
    q.kchunk = q.K;
    q.a_soff = q.K;
    q.w_soff = q.K;
    q.C = plan.part;
    q.cmap = plain_map(p.M, 768);
    q.c_soff = (long long)p.M * 768;
    q.bias = nullptr;
    q.R = nullptr;
    q.Upre = nullptr;
    q.gelu = 0;
    {
        Scope sc(c, s, NOMAD_K_GEMM, 2.0 * p.M * 48.0 * p.K * 16, NOMAD_K_GEMM_FINE);
        HIP_TRY(gemm_f32_n48_split(q, 16, s, S));
    }
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(posconv_splitk_epilogue_kernel, dim3(p.M), dim3(192), 0, s, plan.part, S, p.M, p.bias, p.R, p.rmap, p.r_goff, p.Upre, p.C,
                       p.gelu);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

int run_gemm(nomad_ctx* c, const GemmParams& p, int groups, int tile, hipStream_t s, const SplitKPlan& plan, const SplitKFusion* fuse,
             bool* fused) {
    if (fused) *fused = false;
    int S = 0;
    if (splitk_applies(plan, p, groups, tile, &S)) return run_gemm_splitk(c, plan, p, S, s, fuse, fused);
    if (posconv_splitk_applies(plan, p, groups, tile)) return run_posconv_splitk(c, plan, p, s);
    return gemm_f32_dispatch(c, p, groups, tile, s);
}

namespace {

// conv layer i of an fp32-product forward runs in polyphase Winograd form (conv_s2_f32.hip.h): the k = 3 / stride 2 layers,
// fp32 products only (the bf16x3 products on fp32 buffers keep the implicit GEMM), NOMAD_F32_CONV_WINO (default on).  The one
// fp32 forward sequence (forward_run) asks here, so embed, embed_train, layer outputs and the ragged forward switch together.
bool conv_wino(const nomad_ctx* c, int i) { return c->tune.f32_conv_wino && !c->gemm_x3 && kConvK[i] == 3 && kConvS[i] == 2; }

// The pos-conv of an fp32-product forward runs in nested F(2,2) form (posconv_wino_f32.hip.h): fp32 products only, as above;
// NOMAD_F32_POSCONV_WINO.  Asked by forward_run alone, so every fp32 entry point, uniform or ragged, switches together.
bool posconv_wino(const nomad_ctx* c) { return c->tune.f32_posconv_wino && !c->gemm_x3; }

// pos_w -> pos_wt, queued on s: behind everything that writes pos_w (nomad_create, refresh_weights), never anywhere else - a
// forward cannot see transformed weights older than pos_w.
int rebuild_posconv_wino_weights(nomad_ctx* c, hipStream_t s) {
    hipLaunchKernelGGL(posconv_wino_weight_kernel, dim3(16 * kPwOps * 64), dim3(256), 0, s, c->pos_w, c->pos_wt);
    HIP_TRY(hipGetLastError());
    return 0;
}

// x + gelu(pos_conv(x) + bias) in nested F(2,2) form.  xpad: the padded group-major input; wt: the transformed weights
// [16 * kPwOps][64][kPwK]; y / upre (nullable): [sum T][768]; wq / ws: the operand and product buffers (pos_wino_q_bytes /
// pos_wino_s_bytes of geo); qmeta: 2 (B + 1) ints for a ragged batch's operand prefix sums, formed here.  One launch of the
// N = 48 GEMM kernel over 16 * kPwOps groups, a plain store; the same instantiation for every batch, so a clip's values do not
// depend on its batch.
int run_posconv_wino(nomad_ctx* c, const float* xpad, const float* wt, const float* bias, float* y, float* upre,
                     const PosWinoGeom& geo_in, float* wq, float* ws, int* qmeta, hipStream_t s) {
    PosWinoGeom geo = geo_in;
    if (geo.q_rows >= (1LL << 31) / 48) return fail(NOMAD_ERR_INVALID, "pos-conv: %lld operand rows", geo.q_rows);
    if (geo.tpref && !qmeta) return fail(NOMAD_ERR_INVALID, "pos-conv: a ragged batch without its operand prefix sums");
    {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        if (geo.tpref) {
            hipLaunchKernelGGL(posconv_wino_prefix_kernel, dim3(1), dim3(64), 0, s, geo.tpref, geo.B, qmeta);
            geo.qpref = qmeta;
            geo.qbase = qmeta + geo.B + 1;
        }
        hipLaunchKernelGGL(posconv_wino_input_kernel, dim3((geo.max_q + kPwTaps - 1 + 15) / 16, 16 * geo.B), dim3(192), 0, s, xpad, wq, geo);
        HIP_TRY(hipGetLastError());
    }
    GemmParams p{};
    p.A = wq;
    if (geo.tpref) p.amap = RowMap{0, 0, 0, 48, geo.qpref, geo.qbase, geo.B, 48};
    else p.amap = RowMap{0, (long long)(geo.max_q + kPwTaps - 1) * 48, geo.max_q, 48};
    p.a_goff = geo.q_frames * 48;
    p.K = kPwK;
    p.kchunk = kPwK;
    p.W = wt;
    p.ldw = kPwK;
    p.w_goff = 64LL * kPwK;
    p.C = ws;
    p.M = (int)geo.q_rows;
    p.cmap = plain_map(p.M, 48);
    p.rmap = p.cmap;
    p.c_goff = geo.q_rows * 48;
    p.N = 64;
    p.n_valid = 48;
    int rc;
    if ((rc = gemm_f32_dispatch(c, p, 16 * kPwOps, 48, s))) return rc;   // never splits K (counted with its executed FLOPs: 2 M' 48 kPwK per group)
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(posconv_wino_output_kernel, dim3((geo.max_q + 15) / 16, 16 * geo.B), dim3(192), 0, s, ws, bias, xpad, y, upre, geo);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The pos-conv of an fp32-product forward runs in the frequency domain (posconv_fft_f32.hip.h): fp32 products only;
// NOMAD_F32_POSCONV_FFT, ahead of NOMAD_F32_POSCONV_WINO.  Asked by forward_run alone, like posconv_wino.
bool posconv_fft(const nomad_ctx* c) { return c->tune.f32_posconv_fft && !c->gemm_x3; }

// the twiddle tables of that form, once per context
int build_posconv_fft_tables(nomad_ctx* c, hipStream_t s) {
    if (int rc = dev_alloc(c, "pos-conv twiddles", (size_t)2 * kPfN, &c->pos_tw64)) return rc;
    if (int rc = dev_alloc(c, "pos-conv twiddles", (size_t)2 * kPfN, &c->pos_tw32)) return rc;
    hipLaunchKernelGGL(posconv_fft_twiddle_kernel, dim3(kPfN / 256), dim3(256), 0, s, reinterpret_cast<double2*>(c->pos_tw64),
                       reinterpret_cast<float2*>(c->pos_tw32));
    HIP_TRY(hipGetLastError());
    return 0;
}

// v (as pos_w) -> wf, queued on s; for the context's own weights behind everything that writes pos_w, like the nested form's.
int launch_posconv_fft_weights(nomad_ctx* c, const float* v, float* wf, hipStream_t s) {
    hipLaunchKernelGGL(posconv_fft_weight_kernel, dim3(kPfBins, 16), dim3(256), 0, s, v, reinterpret_cast<const double2*>(c->pos_tw64), wf);
    HIP_TRY(hipGetLastError());
    return 0;
}

// x + gelu(pos_conv(x) + bias) in the frequency domain.  xpad: the padded group-major input; wf: the transformed weights
// [16][257][96][96]; y / upre (nullable): [sum T][768]; sx / sy: the two spectra (pos_fft_spec_bytes of geo.units each); umeta:
// B + 1 ints for a ragged batch's unit prefix sums, formed here.  The same three kernels for every batch.
int run_posconv_fft(nomad_ctx* c, const float* xpad, const float* wf, const float* bias, float* y, float* upre,
                    const PosFftGeom& geo_in, float* sx, float* sy, int* umeta, hipStream_t s) {
    PosFftGeom geo = geo_in;
    if (!c->pos_tw32) return fail(NOMAD_ERR_INVALID, "pos-conv: no twiddle tables");
    if (geo.units <= 0 || geo.units >= (1 << 30) / kPfCols || 16LL * geo.B > 65535)
        return fail(NOMAD_ERR_INVALID, "pos-conv: %d units of %d clips", geo.units, geo.B);
    if (geo.tpref && !umeta) return fail(NOMAD_ERR_INVALID, "pos-conv: a ragged batch without its unit prefix sums");
    const float2* tw = reinterpret_cast<const float2*>(c->pos_tw32);
    const dim3 grid(3 * geo.max_blocks, 16 * geo.B);
    {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        if (geo.tpref) {
            hipLaunchKernelGGL(posconv_fft_prefix_kernel, dim3(1), dim3(64), 0, s, geo.tpref, geo.B, umeta);
            geo.upref = umeta;
        }
        hipLaunchKernelGGL(posconv_fft_forward_kernel, grid, dim3(256), 0, s, xpad, tw, sx, geo);
        HIP_TRY(hipGetLastError());
    }
    {
        Scope sc(c, s, NOMAD_K_GEMM, 2.0 * 16 * kPfBins * kPfCols * kPfCols * (double)geo.units);
        hipLaunchKernelGGL(posconv_fft_bins_kernel, dim3(kPfBins, 16), dim3(256), 0, s, sx, wf, sy, geo.units);
        HIP_TRY(hipGetLastError());
    }
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(posconv_fft_inverse_kernel, grid, dim3(256), 0, s, sy, tw, bias, xpad, y, upre, geo);
    HIP_TRY(hipGetLastError());
    return 0;
}


int run_layernorm(nomad_ctx* c, const float* in, const float* g, const float* b, float* out, float* out2, int M, int N,
                  hipStream_t s) {
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    const int blocks = (M + 3) / 4;
    if (N == 768) hipLaunchKernelGGL((layernorm_kernel<3, float, float>), dim3(blocks), dim3(256), 0, s, in, g, b, out, out2, M);
    else if (N == 512) hipLaunchKernelGGL((layernorm_kernel<2, float, float>), dim3(blocks), dim3(256), 0, s, in, g, b, out, out2, M);
    else return fail(NOMAD_ERR_INVALID, "layernorm: N=%d unsupported", N);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Which rows of frames the head pools, forward and backward: whole clips (the default), windows of `win` frames every `hop`
// (nomad_embed_windows*), or the rows of the caller's span table (nomad_embed_spans*, SpanStage; ragged batches only).
// gw (backward only): [rows][768], the per-row gradients between the backward's two launches, in the caller's scratch.
struct HeadRows {
    int win = 0, hop = 0;
    const SpanStage* spans = nullptr;
    float* gw = nullptr;
    bool whole_clips() const { return !win && !spans; }
    static HeadRows over_spans(const SpanStage* st) { return {0, 0, st, st->gw}; }
};

// One launch over the rows, for run_head and backward_run: launch(rows, grid) with the device's WindowRows or SpanRows (head.hip.h).
// T: frames per clip of an equal-length batch; max_t: frames of the longest clip.
template <class Launch>
int head_rows_launch(const char* who, const HeadRows& h, int B, int T, int max_t, const int* tpref, Launch&& launch) {
    if (h.spans) {
        if (!tpref) return fail(NOMAD_ERR_INVALID, "%s: the span head needs a ragged batch", who);
        launch(SpanRows{h.spans->dev, h.spans->R, h.spans->S, tpref}, dim3(h.spans->R));
    } else {
        launch(WindowRows{tpref ? 0 : T, h.win, h.hop, tpref}, dim3(head_num_windows(max_t, h.win, h.hop), B));
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// mean/ReLU/Linear/normalise head (head.hip.h).  T: frames per clip (the longest clip's with tpref).
// Whole clips, two stages; pool: scratch of at least (M / 64 + B) * 768 floats (M = total frames) - every caller passes its FFN
// hidden buffer.  features (nomad_embed_features*): `emb` is [B][768] and takes the time means themselves (head_mean_kernel) - no
// embedding.
// rows (windows or spans): `emb` is [n_rows][256], one row per window / per row of the span table (head_rows_kernel, one launch, no
// scratch).
struct HeadMode {
    bool features = false;
    HeadRows rows;
    long long n_rows = 0;
    HeadMode() = default;
    HeadMode(bool f) : features(f) {}
    static HeadMode windows(int win, int hop, long long n) {
        HeadMode m;
        m.rows.win = win, m.rows.hop = hop, m.n_rows = n;
        return m;
    }
    static HeadMode over_spans(const SpanStage* st) {
        HeadMode m;
        m.rows = HeadRows::over_spans(st), m.n_rows = st->R;
        return m;
    }
};

template <typename TIn>
int run_head(nomad_ctx* c, const TIn* x, int B, int T, const float* w, const float* b, float* emb, const int* tpref,
             float* pool, hipStream_t s, HeadMode mode = {}) {
    const bool features = mode.features;
    if (!mode.rows.whole_clips()) {
        Scope sc(c, s, NOMAD_K_ROW, 2.0 * (double)mode.n_rows * 768 * 256);
        return head_rows_launch("run_head", mode.rows, B, T, T, tpref, [&](auto rows, dim3 grid) {
            hipLaunchKernelGGL((head_rows_kernel<TIn, decltype(rows)>), grid, dim3(1024), 0, s, x, rows, w, b, emb);
        });
    }
    Scope sc(c, s, NOMAD_K_ROW, features ? 0.0 : 2.0 * B * 768 * 256);
    hipLaunchKernelGGL(head_pool_kernel<TIn>, dim3((T + kHeadChunk - 1) / kHeadChunk, B), dim3(256), 0, s, x, tpref ? 0 : T, pool, tpref);
    if (features) hipLaunchKernelGGL(head_mean_kernel, dim3(B), dim3(256), 0, s, pool, tpref ? 0 : T, emb, tpref);
    else hipLaunchKernelGGL(head_kernel, dim3(B), dim3(1024), 0, s, pool, tpref ? 0 : T, w, b, emb, tpref);
    HIP_TRY(hipGetLastError());
    return 0;
}

DropCfg make_drop(const nomad_ctx* c, float p) {
    DropCfg d{};
    d.seed_lo = (uint32_t)c->drop_seed;
    d.seed_hi = (uint32_t)(c->drop_seed >> 32);
    const double t = (double)p * 4294967296.0;
    d.threshold = p <= 0.f ? 0u : (t >= 4294967295.0 ? 4294967295u : (uint32_t)(t + 0.5));
    d.scale = 1.0f / (1.0f - p);
    return d;
}


// fp32 attention.  An equal-length batch: clips [c0, c0 + nc) (nc = 0: all of them), with dropout when dc has a threshold.
// A ragged one: every clip.
int run_attention(nomad_ctx* c, const BatchGeom& g, const float* qkv, float* out, float* lse, hipStream_t s,
                  const DropCfg* dc = nullptr, uint32_t site = 0, int c0 = 0, int nc = 0) {
    if (g.ragged()) {   // clips [c0, c0 + nc) (nc = 0: all); qkv / out / lse are the whole batch's
        Scope sc(c, s, NOMAD_K_ATTN, g.attn_flops);
        const int nb = nc ? nc : g.B;
        if (dc && dc->threshold) {   // attention dropout: this kernel for every clip, as for an equal-length batch; mask offsets per clip
            hipLaunchKernelGGL((attention_f32_kernel<float, true>), dim3((g.max_t + 63) / 64, nb * 12), dim3(256), 0, s, qkv, out, lse, 0,
                               g.pref[6], *dc, site, c0 * 12);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        // clips of kAttnV2MinT frames or more: attention_f32_v2_kernel; shorter ones: attention_f32_kernel (each skips the
        // other's clips) - exactly the kernel the clip would get in a batch of its own
        if (g.max_t >= kAttnV2MinT) HIP_TRY(launch_attention_f32_v2(qkv, out, lse, nb, g.max_t, g.pref[6] + c0, s, kAttnV2MinT));
        if (g.min_t < kAttnV2MinT)
            hipLaunchKernelGGL(attention_f32_kernel<float>, dim3((std::min(g.max_t, kAttnV2MinT - 1) + 63) / 64, nb * 12), dim3(256), 0,
                               s, qkv, out, lse, 0, g.pref[6], DropCfg{}, 0u, c0 * 12, 0LL, kAttnV2MinT);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const int B = nc ? nc : g.B, T = g.T, bh0 = c0 * 12;
    const double flops = 4.0 * B * 12.0 * (double)T * T * 64;
    Scope sc(c, s, NOMAD_K_ATTN, flops);
    const dim3 grid((T + 63) / 64, B * 12);
    if (dc && dc->threshold)
        hipLaunchKernelGGL((attention_f32_kernel<float, true>), grid, dim3(256), 0, s, qkv, out, lse, T, kNoInts, *dc, site, bh0);
    else if (T >= kAttnV2MinT)  // by the clip's length only: the same clip takes the same kernel in every batch
        HIP_TRY(launch_attention_f32_v2(qkv, out, lse, B, T, kNoInts, s));
    else
        hipLaunchKernelGGL((attention_f32_kernel<float, false>), grid, dim3(256), 0, s, qkv, out, lse, T, kNoInts, DropCfg{}, 0u, 0);
    HIP_TRY(hipGetLastError());
    return 0;
}

// y = (resid ? resid : 0) + dropout(x) over n floats of an [M][768] tensor (x == y allowed)
int run_dropout(nomad_ctx* c, const float* x, const float* resid, float* y, long long n, const DropCfg& d, uint32_t site,
                hipStream_t s, unsigned long long idx0 = 0) {
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(dropout_add_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(resid),
                       reinterpret_cast<float4*>(y), n / 4, d, site, idx0);
    HIP_TRY(hipGetLastError());
    return 0;
}

// nomad_set_encoder_depth below 12: only the loss's layer-output forwards and their backward run a cut encoder; every other entry
// point refuses before anything is queued - a truncated encoder behind a score or a fine-tuning step is never a silent result.
int refuse_cut(const nomad_ctx* c, const char* who) {
    if (!c || c->encoder_depth == NOMAD_NUM_LAYERS) return 0;
    return fail(NOMAD_ERR_INVALID, "%s: the encoder depth is %d (nomad_set_encoder_depth): only nomad_embed with layers_dev, "
                "nomad_embed_train[_ragged] and nomad_embed_backward[_ragged] run a cut encoder", who, c->encoder_depth);
}

}  // namespace

extern "C" {

const char* nomad_last_error(void) { return g_err; }
const char* nomad_version(void) {
#ifdef NOMAD_DIAG
    return "nomad_hip 0.3 (gfx950) + experimental kernel instantiations (libnomad_diag.so)";
#else
    return "nomad_hip 0.3 (gfx950)";
#endif
}
int nomad_abi_version(void) { return NOMAD_ABI_VERSION; }

int nomad_wav_probe(const char* const* paths, int n, nomad_wav_info* info, int* status, int threads) {
    if (n < 0 || (n > 0 && (!paths || !info || !status))) return fail(NOMAD_ERR_INVALID, "nomad_wav_probe: null argument");
    try {
        wav::parallel_for(n, threads, [&](int i, int) { status[i] = paths[i] ? wav::probe_one(paths[i], &info[i]) : NOMAD_ERR_INVALID; });
    } catch (const std::exception& e) {
        return fail(NOMAD_ERR_IO, "nomad_wav_probe: %s", e.what());
    }
    return NOMAD_OK;
}

int nomad_wav_frames_at(const nomad_wav_info* info, int target_rate, long long* frames) {
    if (!info || !frames || target_rate <= 0 || info->sample_rate <= 0)
        return fail(NOMAD_ERR_INVALID, "nomad_wav_frames_at: bad argument");
    *frames = wav::resampled_frames(info->frames, info->sample_rate, target_rate);
    return NOMAD_OK;
}

int nomad_wav_read_rows(const char* const* paths, const nomad_wav_info* info, int n, const int* row, float* dst_host,
                        long long stride, int target_rate, int* status, int threads) {
    if (n < 0 || (n > 0 && (!paths || !info || !dst_host || !status)) || stride < 0 || target_rate <= 0)
        return fail(NOMAD_ERR_INVALID, "nomad_wav_read_rows: bad argument");
    for (int i = 0; i < n; ++i)
        if (!paths[i] || info[i].sample_rate <= 0 || wav::resampled_frames(info[i].frames, info[i].sample_rate, target_rate) > stride ||
            (row && row[i] < 0))
            return fail(NOMAD_ERR_INVALID, "nomad_wav_read_rows: file %d: %lld frames at %d Hz do not fit a row of %lld", i, info[i].frames,
                        info[i].sample_rate, stride);
    try {
        const int nt = std::max(1, std::min(threads, n));
        std::vector<std::vector<unsigned char>> raw((size_t)nt);
        std::vector<std::vector<float>> mono((size_t)nt);      // a file at another rate is decoded here first
        std::vector<wav::ResampleKernel> kern((size_t)nt);     // per-thread cache of the last kernel built
        std::vector<int> kern_rate((size_t)nt, 0);
        wav::parallel_for(n, nt, [&](int i, int t) {
            float* dst = dst_host + (size_t)(row ? row[i] : i) * (size_t)stride;
            if (info[i].sample_rate == target_rate) {
                status[i] = wav::read_one(paths[i], info[i], dst, raw[(size_t)t]);
                return;
            }
            std::vector<float>& m = mono[(size_t)t];
            if ((long long)m.size() < info[i].frames) m.resize((size_t)info[i].frames);
            status[i] = wav::read_one(paths[i], info[i], m.data(), raw[(size_t)t]);
            if (status[i] != NOMAD_OK) return;
            if (kern_rate[(size_t)t] != info[i].sample_rate) {
                kern[(size_t)t] = wav::make_resample_kernel(info[i].sample_rate, target_rate);
                kern_rate[(size_t)t] = info[i].sample_rate;
            }
            wav::resample_into(m.data(), info[i].frames, kern[(size_t)t], dst,
                               wav::resampled_frames(info[i].frames, info[i].sample_rate, target_rate));
        });
    } catch (const std::exception& e) {
        return fail(NOMAD_ERR_IO, "nomad_wav_read_rows: %s", e.what());
    }
    for (int i = 0; i < n; ++i)
        if (status[i] != NOMAD_OK) return fail(status[i], "nomad_wav_read_rows: %s: %s", paths[i], status[i] == NOMAD_ERR_IO ? "read failed" : "unsupported encoding");
    return NOMAD_OK;
}

int nomad_num_frames(int n_samples) {
    Shapes s;
    return make_shapes(1, n_samples, &s) ? s.T : 0;
}

int nomad_create(nomad_ctx** out, int device, const nomad_weights* w) {
    if (!out || !w) return fail(NOMAD_ERR_INVALID, "nomad_create: null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(NOMAD_ERR_NO_DEVICE, "nomad_create: no HIP device %d (count %d); this engine has no CPU path",
                    device, ndev);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(NOMAD_ERR_NO_DEVICE, "nomad_create: device %d is %s, kernels are built for gfx950 only", device,
                    prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    nomad_ctx* c = new nomad_ctx();
    c->device = device;
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
#ifdef NOMAD_DIAG
    tuning_from_env(c->tune);
#endif
    int rc = 0;
    auto up = [&](const float* h, size_t n, float** d) {
        if (rc == 0) rc = upload(c, "nomad_create", h, n, d);
    };
    // every tensor the engine reads as it stands ...
    ParamOffsets po = param_offsets();
    for_each_param(*w, po, *c, [&](const Param& p) {
        if (p.alias) up(p.host, p.count, p.alias);
    });
    // ... and the derived copies, formed on the HOST here: conv1..6 repacked, weight norm folded, q/k/v fused with q scaled.
    // refresh_weights forms the same three from the master vector on the DEVICE after a weight update (conv_repack_kernel,
    // posconv_fold_kernel, scale_rows_kernel).  The repack and the scale are exact either way; the two weight-norm folds add
    // their 36 864 squares per tap in different orders, so a scale can differ in its last bit - two routes on purpose.
    for (int i = 1; i < 7 && rc == 0; ++i) {
        const int k = kConvK[i];
        std::vector<float> r((size_t)512 * k * 512);
        for (int n = 0; n < 512; ++n)
            for (int ci = 0; ci < 512; ++ci)
                for (int t = 0; t < k; ++t) r[(size_t)n * k * 512 + t * 512 + ci] = w->conv_w[i][((size_t)n * 512 + ci) * k + t];
        up(r.data(), r.size(), &c->conv_w[i]);
    }
    if (rc == 0) {  // fold weight_norm(dim=2): w = v * g[k] / ||v[:, :, k]||, then [group][64][tap*48 + cin]
        std::vector<double> nrm(128, 0.0);
        for (size_t o = 0; o < 768; ++o)
            for (size_t ci = 0; ci < 48; ++ci)
                for (size_t t = 0; t < 128; ++t) {
                    const double v = w->pos_v[(o * 48 + ci) * 128 + t];
                    nrm[t] += v * v;
                }
        std::vector<float> sc(128);
        for (int t = 0; t < 128; ++t) sc[t] = (float)((double)w->pos_g[t] / std::sqrt(nrm[t]));
        std::vector<float> r((size_t)16 * 64 * 6144, 0.f);
        for (size_t g = 0; g < 16; ++g)
            for (size_t n = 0; n < 48; ++n)
                for (size_t ci = 0; ci < 48; ++ci)
                    for (size_t t = 0; t < 128; ++t)
                        r[(g * 64 + n) * 6144 + t * 48 + ci] = w->pos_v[((g * 48 + n) * 48 + ci) * 128 + t] * sc[t];
        up(r.data(), r.size(), &c->pos_w);
        if (rc == 0 && c->tune.f32_posconv_wino) {
            rc = dev_alloc(c, "nomad_create: pos-conv weights", (size_t)16 * kPwOps * 64 * kPwK, &c->pos_wt);
            if (rc == 0) rc = rebuild_posconv_wino_weights(c, nullptr);
            if (rc == 0 && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(NOMAD_ERR_HIP, "nomad_create: pos-conv weights: kernel");
        }
        if (rc == 0) rc = build_posconv_fft_tables(c, nullptr);   // (every context: nomad_diag_posconv_fft runs the form whatever the switch says)
        if (rc == 0 && c->tune.f32_posconv_fft) {
            rc = dev_alloc(c, "nomad_create: pos-conv weights", kPfWeightFloats, &c->pos_wf);
            if (rc == 0) rc = launch_posconv_fft_weights(c, c->pos_w, c->pos_wf, nullptr);
        }
        if (rc == 0 && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(NOMAD_ERR_HIP, "nomad_create: pos-conv spectrum: kernel");
    }
    for (int l = 0; l < NOMAD_NUM_LAYERS && rc == 0; ++l) {
        const nomad_layer_weights& lw = w->layers[l];
        std::vector<float> qkv((size_t)2304 * 768), qb(2304);
        for (size_t i = 0; i < (size_t)768 * 768; ++i) {
            qkv[i] = lw.q_w[i] * 0.125f;  // fairseq MultiheadAttention: q *= head_dim^-0.5 (exact in fp32)
            qkv[(size_t)768 * 768 + i] = lw.k_w[i];
            qkv[(size_t)2 * 768 * 768 + i] = lw.v_w[i];
        }
        for (int i = 0; i < 768; ++i) {
            qb[i] = lw.q_b[i] * 0.125f;
            qb[768 + i] = lw.k_b[i];
            qb[1536 + i] = lw.v_b[i];
        }
        up(qkv.data(), qkv.size(), &c->layers[l].qkv_w);
        up(qb.data(), qb.size(), &c->layers[l].qkv_b);
    }
    if (rc == 0) {
        double* d = nullptr;
        rc = dev_alloc(c, "nomad_create: pairwise scratch", (size_t)kPairScratchDoubles, &d);
        if (rc == 0) c->pair_scratch.emplace_back(kNoStream, d);
    }
    if (rc != 0) {
        nomad_destroy(c);
        return rc;
    }
    *out = c;
    return 0;
}

void nomad_destroy(nomad_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (void* p : c->allocs) (void)hipFree(p);
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    delete c;
}

int nomad_diag_keep_intermediates(nomad_ctx* c, int on) {
    if (!c) return fail(NOMAD_ERR_INVALID, "null ctx");
    c->keep = on != 0;
    return 0;
}

int nomad_workspace_bytes(const nomad_ctx* c, int B, int n_samples, size_t* bytes) {
    Shapes s;
    if (!c || !bytes || B <= 0 || !make_shapes(B, n_samples, &s))
        return fail(NOMAD_ERR_INVALID, "nomad_workspace_bytes: bad shape B=%d N=%d", B, n_samples);
    *bytes = make_layout(s, c->keep, pos_form(c)).total;
    return 0;
}

int nomad_diag_workspace_region(const nomad_ctx* c, int B, int n_samples, const char* name, size_t* offset,
                                size_t* bytes) {
    Shapes s;
    if (!c || !name || !offset || !bytes || !make_shapes(B, n_samples, &s))
        return fail(NOMAD_ERR_INVALID, "nomad_diag_workspace_region: bad argument");
    const Layout l = make_layout(s, c->keep, pos_form(c));
    if (strncmp(name, "conv", 4) == 0 && name[4] >= '0' && name[4] <= '6' && name[5] == 0) {
        const int i = name[4] - '0';
        *offset = l.conv[i];
        *bytes = sizeof(float) * 512 * (size_t)B * s.L[i];
    } else if (strcmp(name, "featln") == 0) {
        *offset = l.featln;
        *bytes = sizeof(float) * 512 * (size_t)s.M;
    } else if (strcmp(name, "encin") == 0) {
        *offset = l.x;
        *bytes = sizeof(float) * 768 * (size_t)s.M;
    } else if (strcmp(name, "xpad") == 0) {  // group-major [16][B][T+128][48]
        *offset = l.xpad;
        *bytes = sizeof(float) * 768 * (size_t)B * (s.T + 128);
    } else {
        return fail(NOMAD_ERR_INVALID, "unknown region %s", name);
    }
    return 0;
}

}  // extern "C"

// The fp32 forward's buffers: the conv output of every level (aliasing ping-pong buffers unless the equal-length layout keeps
// them), the LayerNorm(512) output and the activations.
struct F32Bufs {
    double* stats;
    float *scale, *shift, *conv[7], *featln, *xpad, *x, *x2, *y, *qkv, *ctxb, *h;
    float *pwq = nullptr, *pws = nullptr;   // operands / products of the pos-conv in nested F(2,2) form (nullptr: the layout has none)
    int* pwmeta = nullptr;                  // ... and, for a ragged batch, the operands' 2 (B + 1) prefix sums
    float *pfx = nullptr, *pfy = nullptr;   // the spectra of the pos-conv in the frequency domain (nullptr: the layout has none)
    int* pfmeta = nullptr;                  // ... and, for a ragged batch, the units' B + 1 prefix sums
};

// The fp32 forward, over an equal-length or a ragged batch.  sv == nullptr: scoring mode (intermediates alias inside the
// workspace).  sv != nullptr: training mode - every tensor the backward needs is written to its slot in `sv` instead.
// ws_splitk: the workspace's split-K block of an equal-length layer-output forward, or the empty plan.
// A ragged batch takes sv, its dropout and LayerDrop (branches: equal groups of clips, of any lengths) and layers_out like an
// equal-length one, packed; it never splits K, so that a clip's values never depend on the batch it is in.
static int forward_run(nomad_ctx* c, const float* wav, const BatchGeom& g, const F32Bufs& bf, const float* head_w,
                       const float* head_b, float* emb, float* layers_out, const SplitKPlan& ws_splitk, hipStream_t s,
                       const Saved* sv, HeadMode mode = {}) {
    if (g.ragged() && ws_splitk.part) return fail(NOMAD_ERR_INVALID, "fp32 forward: split-K needs an equal-length batch");
    const int B = g.B, T = g.T, M = (int)g.rows[6];
    // nomad_set_encoder_depth: layers 0 .. depth - 1, then stop - no head, rows [depth, 12) of layers_out and emb stay unwritten
    const int depth = c->encoder_depth;
    if (depth < NOMAD_NUM_LAYERS && (!layers_out || mode.features || mode.rows.win)) return refuse_cut(c, "fp32 forward");
    // the loss forward of Nomad.forward() (saving activations, not fine-tuning): small-M GEMMs may split K.  Round 4: so may the
    // other branch of that loss - a forward that returns the 12 layer outputs (LossNetLayers: `clean`, or `estimate` under
    // no_grad) on fewer than 4096 frames.  The split is a function of the GEMM shape only (fixed slices, ordered fold): the
    // results are deterministic, but they are the loss path's bits, not the scoring path's - nomad_embed WITHOUT layer outputs
    // (TripletModel / predict) never splits, whatever the batch.  The partial sums live in the call's own workspace (round 5; they
    // were two context-wide blocks handed to launch streams by hipEventQuery: whether a third stream's forward split depended on
    // timing).  Training mode: the context's block (nomad_enable_backward).
    const SplitKPlan splitk = c->train_ready || g.ragged() ? SplitKPlan{}
                              : sv                         ? SplitKPlan{c->splitk_part, kSplitKPartFloats}
                              : layers_out                 ? ws_splitk
                                                           : SplitKPlan{};
    int rc;
    // model.train() regularisation: only in the training-mode forward, only when switched on
    const bool reg = sv != nullptr;
    const DropCfg d_in = make_drop(c, reg ? c->p_input : 0.f), d_res = make_drop(c, reg ? c->p_drop : 0.f),
                  d_att = make_drop(c, reg ? c->p_attn : 0.f);
    // LayerDrop: one mask for the call, or one per branch (equal groups of clips) of a merged batch
    int nbr = 1;
    unsigned bmask[4] = {reg ? c->layer_mask : 0xFFFu, 0xFFFu, 0xFFFu, 0xFFFu};
    if (reg && c->branches > 1) {
        if (B % c->branches) return fail(NOMAD_ERR_INVALID, "nomad_embed_train: B=%d is not %d equal branches", B, c->branches);
        nbr = c->branches;
        for (int i = 0; i < nbr; ++i) bmask[i] = c->branch_mask[i];
    }
    const long long act = (long long)M * 768;

    // ---- front end: conv0 + GroupNorm + GELU ------------------------------------------------
    float* gn_scale = sv ? sv->gn_scale : bf.scale;
    float* gn_shift = sv ? sv->gn_shift : bf.shift;
    {
        Scope sc(c, s, NOMAD_K_FRONT, 0.0);
        launch_wav_stats(wav, g.wav_ld, g.L[0], g.max_l0, B, bf.stats, g.lens, s);
        hipLaunchKernelGGL(gn_fold_kernel, dim3(B), dim3(512), 0, s, bf.stats, c->conv0_w, c->gn_w, c->gn_b, g.L[0],
                           gn_scale, gn_shift, sv ? sv->gn_mean : nullptr, sv ? sv->gn_rstd : nullptr, g.lens);
    }
    {
        Scope sc(c, s, NOMAD_K_FRONT, 2.0 * (double)g.rows[0] * 512 * 10);
        hipLaunchKernelGGL(conv0_gn_gelu_kernel<float>, dim3((g.max_l0 + kConv0Frames - 1) / kConv0Frames, B), dim3(256), 0, s,
                           wav, g.wav_ld, g.L[0], c->conv0_w, gn_scale, gn_shift, bf.conv[0], g.lens, g.pref[0]);
    }
    HIP_TRY(hipGetLastError());

    // ---- conv1..6: implicit GEMM over time-major activations --------------------------------
    for (int i = 1; i < 7; ++i) {
        if (conv_wino(c, i)) {   // conv1 .. conv4: 5 products per output pair instead of 6 (conv_s2_f32.hip.h)
            if ((rc = run_conv_s2_f32(c, bf.conv[i - 1], c->conv_w[i], bf.conv[i], sv ? sv->u[i] : nullptr, B, g.L[i - 1], g.L[i],
                                      g.pairpref[i], g.pref[i], g.pref[i - 1], (int)g.pairs[i], s)))
                return rc;
            continue;
        }
        GemmParams p{};
        p.A = bf.conv[i - 1];
        p.amap = g.conv_amap[i];
        p.K = kConvK[i] * 512;
        p.kchunk = p.K;
        p.W = c->conv_w[i];
        p.ldw = p.K;
        p.C = (sv && i == 6) ? sv->c6 : bf.conv[i];
        p.Upre = sv ? sv->u[i] : nullptr;
        p.M = (int)g.rows[i];
        p.N = 512;
        p.n_valid = 512;
        p.cmap = plain_map(p.M, 512);
        p.rmap = p.cmap;
        p.gelu = 1;
        if ((rc = run_gemm(c, p, 1, pick_tile(c, p.M, 512, p.K), s, splitk))) return rc;
    }

    // ---- LayerNorm(512) + post_extract_proj into the padded pos-conv buffer ------------------
    if ((rc = run_layernorm(c, sv ? sv->c6 : bf.conv[6], c->fln_w, c->fln_b, bf.featln, nullptr, M, 512, s)))
        return rc;
    // group-major pos-conv buffer xg[16][clip][T+128][48]; x (post_extract_proj output) sits at frames 64..64+T
    float* xpad = bf.xpad;
    {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        hipLaunchKernelGGL(zero_pad_rows_kernel<float>, dim3(16 * B), dim3(256), 0, s, xpad, T, g.pref[6], g.ppref, B);
    }
    {
        GemmParams p = dense(bf.featln, 512, c->proj_w, c->proj_b, nullptr, xpad, M, 768, 512, 0);
        p.cmap = g.pad_map;
        p.c_colblk = 48;
        p.c_colblk_stride = g.grp_stride;
        if ((rc = run_gemm(c, p, 1, pick_tile(c, M, 768, 512), s, splitk))) return rc;
    }
    if (d_in.threshold) {  // dropout_input: on the features that feed both the pos-conv and its residual
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        hipLaunchKernelGGL(dropout_groups_kernel, dim3(M), dim3(192), 0, s, xpad, T, g.grp_stride, d_in, kSiteInput, g.pref[6], g.ppref, B);
    }
    // ---- pos-conv: 16 groups x (M x 48 x 6144), x + gelu(conv + bias) -------------------------
    if (posconv_fft(c)) {   // one 48 x 48 complex product per bin instead of 128 taps (posconv_fft_f32.hip.h)
        if (!bf.pfx || !bf.pfy || !c->pos_wf) return fail(NOMAD_ERR_INVALID, "fp32 forward: no workspace for the pos-conv spectra");
        if ((rc = run_posconv_fft(c, xpad, c->pos_wf, c->pos_b, sv ? sv->y0 : bf.y, sv ? sv->upc : nullptr, g.pos_fft, bf.pfx, bf.pfy, bf.pfmeta, s)))
            return rc;
    } else if (posconv_wino(c)) {   // 9 / 16 of the products (posconv_wino_f32.hip.h)
        if (!bf.pwq || !bf.pws) return fail(NOMAD_ERR_INVALID, "fp32 forward: no workspace for the pos-conv operands");
        if ((rc = run_posconv_wino(c, xpad, c->pos_wt, c->pos_b, sv ? sv->y0 : bf.y, sv ? sv->upc : nullptr, g.pos_wino, bf.pwq, bf.pws, bf.pwmeta, s)))
            return rc;
    } else {
        GemmParams p{};
        p.A = xpad;
        p.amap = g.pos_amap;
        p.a_goff = g.grp_stride;
        p.K = 6144;
        p.kchunk = 6144;
        p.W = c->pos_w;
        p.ldw = 6144;
        p.w_goff = 64LL * 6144;
        p.bias = c->pos_b;
        p.bias_goff = 48;
        p.C = sv ? sv->y0 : bf.y;
        p.Upre = sv ? sv->upc : nullptr;
        p.cmap = plain_map(M, 768);
        p.c_goff = 48;
        p.R = xpad;
        p.rmap = g.pad_map;
        p.r_goff = g.grp_stride;
        p.M = M;
        p.N = 64;
        p.n_valid = 48;
        p.gelu = 1;
        if ((rc = run_gemm(c, p, 16, 48, s, splitk))) return rc;  // one instantiation for every batch size: same summation order
    }
    float* x = bf.x;
    float* x2 = bf.x2;
    float* y = bf.y;
    if ((rc = run_layernorm(c, sv ? sv->y0 : y, c->eln_w, c->eln_b, x, nullptr, M, 768, s))) return rc;
    if (d_res.threshold && (rc = run_dropout(c, x, nullptr, x, act, d_res, kSiteEncoder, s))) return rc;

    // ---- 12 post-LN transformer layers --------------------------------------------------------
    // One layer over clips [c0, c0 + nc) (rows r0 = c0*T ..): the whole batch, or one branch of it when LayerDrop
    // decided differently for the branches.  Rows are independent, so a sub-range call is the same arithmetic.
    auto run_layer = [&](int l, int c0, int nc) -> int {
        const LayerDev& d = c->layers[l];
        const long long r0 = g.clip_row0(c0);   // (a ragged batch: the clips' prefix sums)
        const int Ms = nc == B ? M : (int)(g.clip_row0(c0 + nc) - r0);
        const long long acts = (long long)Ms * 768;
        float* xs = x + r0 * 768;
        float* x2s = x2 + r0 * 768;
        float* hs = bf.h + r0 * 3072;
        float* qkv = (sv ? sv->L[l].qkv : bf.qkv) + r0 * 2304;
        float* ctxb = (sv ? sv->L[l].ctx : bf.ctxb) + r0 * 768;
        float* y1 = (sv ? sv->L[l].y1 : y) + r0 * 768;
        float* y2 = (sv ? sv->L[l].y2 : y) + r0 * 768;
        float* lse = sv ? sv->L[l].lse + 12 * r0 : nullptr;
        float* lo = layers_out ? layers_out + (size_t)l * M * 768 + r0 * 768 : nullptr;
        const unsigned long long idx0 = (unsigned long long)r0 * 768;
        int rc;
        if ((rc = run_gemm(c, dense(xs, 768, d.qkv_w, d.qkv_b, nullptr, qkv, Ms, 2304, 768, 0), 1, pick_tile(c, Ms, 2304, 768), s, splitk)))
            return rc;
        // (a ragged batch: the attention kernels address clips through the whole batch's prefix sums - whole-batch pointers)
        if (g.ragged() ? (rc = run_attention(c, g, qkv - r0 * 2304, ctxb - r0 * 768, lse ? lse - 12 * r0 : nullptr, s, &d_att, site_attn(l), c0, nc))
                       : (rc = run_attention(c, g, qkv, ctxb, lse, s, &d_att, site_attn(l), c0, nc)))
            return rc;
        // residual dropout: y = x + dropout(W a + b) needs the branch on its own, so the residual add moves out
        // of the GEMM epilogue into the dropout kernel
        // (the LayerNorm behind a residual GEMM: inside the GEMM's split-K epilogue where it has one - configs[3] - else on its own;
        // not offered under residual dropout, where the residual is no longer the GEMM's)
        const SplitKFusion ln1 = SplitKFusion::ln(d.ln1_w, d.ln1_b, x2s, nullptr), ln2 = SplitKFusion::ln(d.ln2_w, d.ln2_b, xs, lo);
        bool ln_done = false;
        if ((rc = run_gemm(c, dense(ctxb, 768, d.o_w, d.o_b, d_res.threshold ? nullptr : xs, y1, Ms, 768, 768, 0), 1,
                           pick_tile(c, Ms, 768, 768), s, splitk, d_res.threshold ? nullptr : &ln1, &ln_done)))
            return rc;
        if (d_res.threshold && (rc = run_dropout(c, y1, xs, y1, acts, d_res, site_proj(l), s, idx0))) return rc;
        if (!ln_done && (rc = run_layernorm(c, y1, d.ln1_w, d.ln1_b, x2s, nullptr, Ms, 768, s))) return rc;
        {
            GemmParams p = dense(x2s, 768, d.fc1_w, d.fc1_b, nullptr, hs, Ms, 3072, 768, 1);
            p.Upre = sv ? sv->L[l].u + r0 * 3072 : nullptr;
            if ((rc = run_gemm(c, p, 1, pick_tile(c, Ms, 3072, 768), s, splitk))) return rc;
        }
        if ((rc = run_gemm(c, dense(hs, 3072, d.fc2_w, d.fc2_b, d_res.threshold ? nullptr : x2s, y2, Ms, 768, 3072, 0), 1,
                           pick_tile(c, Ms, 768, 3072), s, splitk, d_res.threshold ? nullptr : &ln2, &ln_done)))
            return rc;
        if (d_res.threshold && (rc = run_dropout(c, y2, x2s, y2, acts, d_res, site_ffn(l), s, idx0))) return rc;
        return ln_done ? 0 : run_layernorm(c, y2, d.ln2_w, d.ln2_b, xs, lo, Ms, 768, s);
    };
    for (int l = 0; l < depth; ++l) {
        unsigned all = 1u, any = 0u;
        for (int br = 0; br < nbr; ++br) {
            all &= (bmask[br] >> l) & 1u;
            any |= (bmask[br] >> l) & 1u;
        }
        if (all) {
            if ((rc = run_layer(l, 0, B))) return rc;
            continue;
        }
        for (int br = 0; br < nbr; ++br) {  // LayerDrop: identity for a dropped branch, the layer for the others
            const int c0 = br * (B / nbr), nc = B / nbr;
            if ((bmask[br] >> l) & 1u) {
                if ((rc = run_layer(l, c0, nc))) return rc;
            } else if (layers_out) {
                const long long r0 = g.clip_row0(c0), nr = g.clip_row0(c0 + nc) - r0;
                HIP_TRY(hipMemcpyAsync(layers_out + (size_t)l * M * 768 + r0 * 768, x + r0 * 768,
                                       sizeof(float) * (size_t)nr * 768, hipMemcpyDeviceToDevice, s));
            }
        }
        (void)any;
    }

    // ---- head -----------------------------------------------------------------------------------
    // the FFN hidden buffer is dead by now: scratch for the time sums
    // (a cut encoder has no embedding: every layer's LayerNorm - fused into a split-K epilogue or not - and its copy into layers_out
    // are complete when run_layer returns, so there is nothing else to flush)
    if (depth < NOMAD_NUM_LAYERS) return 0;
    return run_head<float>(c, x, B, g.max_t, head_w ? head_w : c->emb_w, head_b ? head_b : c->emb_b, emb, g.pref[6], bf.h, s, mode);
}

// nomad_embed / nomad_embed_train: an equal-length batch in the Layout of make_layout.  who: the entry point the errors name;
// features: nomad_embed_features (`emb` is [B][768], see run_head).
static int forward_impl(nomad_ctx* c, const float* wav, int B, int n_samples, const float* head_w, const float* head_b,
                        float* emb, float* layers_out, void* workspace, size_t workspace_bytes, nomad_stream_t stream,
                        const Saved* sv, const char* who = "nomad_embed", HeadMode mode = {}) {
    Shapes sh;
    if (!c || !wav || !emb || !workspace || B <= 0 || !make_shapes(B, n_samples, &sh))
        return fail(NOMAD_ERR_INVALID, "%s: bad argument (B=%d, n_samples=%d)", who, B, n_samples);
    const Layout lay = make_layout(sh, c->keep, pos_form(c));
    if (workspace_bytes < lay.total)
        return fail(NOMAD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", who, workspace_bytes, lay.total);
    char* ws = static_cast<char*>(workspace);
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    F32Bufs bf{reinterpret_cast<double*>(ws + lay.stats), F(lay.scale), F(lay.shift), {}, F(lay.featln), F(lay.xpad), F(lay.x),
               F(lay.x2), F(lay.y), F(lay.qkv), F(lay.ctxb), F(lay.h)};
    if (pos_form(c) == kPosWino) bf.pwq = F(lay.pwq), bf.pws = F(lay.pws);
    if (pos_form(c) == kPosFft) bf.pfx = F(lay.pfx), bf.pfy = F(lay.pfy);
    for (int i = 0; i < 7; ++i) bf.conv[i] = F(lay.conv[i]);
    const SplitKPlan ws_splitk = lay.splitk != 0 ? SplitKPlan{F(lay.splitk), layers_splitk_floats(sh)} : SplitKPlan{};
    return forward_run(c, wav, geom_uniform(sh), bf, head_w, head_b, emb, layers_out, ws_splitk, static_cast<hipStream_t>(stream), sv, mode);
}

// layers_out / saved (nomad_embed_train_ragged): the packed layer outputs and, with a saved block, the training-mode forward.
static int forward_ragged(nomad_ctx* c, const float* wav, int B, int stride, const int* lens_host, const float* head_w,
                          const float* head_b, float* emb, void* workspace, size_t workspace_bytes,
                          nomad_stream_t stream, const char* who = "nomad_embed_ragged", HeadMode mode = {},
                          float* layers_out = nullptr, void* saved = nullptr, size_t saved_bytes = 0) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    RaggedBatch r;
    if (int rc = ragged_shapes(who, c && wav && emb && workspace, B, stride, lens_host, &r.rs)) return rc;
    r.g = geom_ragged(r.rs, stride, nullptr);
    r.lay = make_act_layout(r.g, sizeof(float), 0, pos_form(c));
    if (workspace_bytes < r.lay.total) return fail(NOMAD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", who, workspace_bytes, r.lay.total);
    Saved sv{};
    if (saved) {   // every check before the first byte is queued
        sv = make_saved(r.g, saved);
        if (saved_bytes < sv.total) return fail(NOMAD_ERR_WORKSPACE, "%s: saved block %zu < required %zu", who, saved_bytes, sv.total);
        if (c->branches > 1 && B % c->branches) return fail(NOMAD_ERR_INVALID, "%s: B=%d is not %d equal branches", who, B, c->branches);
    }
    if (int rc = ragged_upload(c, r.rs, stride, reinterpret_cast<int*>(static_cast<char*>(workspace) + r.lay.meta), s, &r.g)) return rc;
    if (mode.rows.spans)
        if (int rc = span_upload(c, *mode.rows.spans, s)) return rc;
    char* ws = static_cast<char*>(workspace);
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const ActLayout& lay = r.lay;
    F32Bufs bf{reinterpret_cast<double*>(ws + lay.stats), F(lay.scale), F(lay.shift), {}, F(lay.convb), F(lay.xpad), F(lay.x),
               F(lay.x2), F(lay.y), F(lay.qkv), F(lay.ctxb), F(lay.h)};
    if (pos_form(c) == kPosWino) bf.pwq = F(lay.pwq), bf.pws = F(lay.pws), bf.pwmeta = reinterpret_cast<int*>(ws + lay.pwmeta);
    if (pos_form(c) == kPosFft) bf.pfx = F(lay.pfx), bf.pfy = F(lay.pfy), bf.pfmeta = reinterpret_cast<int*>(ws + lay.pfmeta);
    for (int i = 0; i < 7; ++i) bf.conv[i] = F(i % 2 ? lay.convb : lay.conva);   // conv6 lands in conva, LN(512) writes to convb
    return forward_run(c, wav, r.g, bf, head_w, head_b, emb, layers_out, SplitKPlan{}, s, saved ? &sv : nullptr, mode);
}

// One backward GEMM: C[M][N] = A[M][K] * Wt[N][K]^T (Wt = transposed forward weight), optional GELU' and residual.
// plan / fuse / fused: run_gemm's.
static int bwd_gemm(nomad_ctx* c, const float* A, const float* Wt, float* C, int M, int N, int K, const float* DG,
                    const float* R, hipStream_t s, const SplitKPlan& plan, const SplitKFusion* fuse = nullptr, bool* fused = nullptr) {
    GemmParams p = dense(A, K, Wt, nullptr, R, C, M, N, K, 0);
    p.DG = DG;
    p.dgmap = plain_map(M, N);
    return run_gemm(c, p, 1, pick_tile(c, M, N, K), s, plan, fuse, fused);
}

static int run_ln_bwd(nomad_ctx* c, const float* x, const float* g, const float* g2, const float* gamma, float* dx, int M,
                      int N, hipStream_t s) {
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    const int blocks = (M + 3) / 4;
    if (N == 768) hipLaunchKernelGGL(layernorm_bwd_kernel<3>, dim3(blocks), dim3(256), 0, s, x, g, g2, gamma, dx, M);
    else hipLaunchKernelGGL(layernorm_bwd_kernel<2>, dim3(blocks), dim3(256), 0, s, x, g, g2, gamma, dx, M);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- bf16 path (config C5) -----------------------------------------------------------------------------
// bf16 attention (attention_bf16_v3.hip.h: the 16-wide matrix shape, K / V staged by LDS-DMA; q carries log2(e)).  T = frames per clip
// (the longest clip's with tpref).  256-query workgroups with 128-key tiles when that still gives the chip >= 2 rounds of them,
// 128-query ones with 64-key tiles for small batches - a clip's bits do not depend on its batch (the wave composition - 32
// consecutive queries - is the same in both workgroup shapes, so the deferred-rescale decisions and every bit are too).
static hipError_t run_attention_bf16(const nomad_ctx* c, const bf16_t* qkv, bf16_t* out, int B, int T, const int* tpref, hipStream_t s) {
    const bool big = (long long)((T + 255) / 256) * B * 12 >= 1024;
#ifdef NOMAD_DIAG
    // Round 6 probe, measured slower and kept out of the product (profiles/NOTEBOOK.md "the last round of the bf16 attention"): two
    // 256-query workgroups fit a CU, so the launch runs in rounds of 2 x CUs items (configs[4]: 2304 items = 4.5 rounds of 512); here
    // the items of a last round at most `bf16_attn_tail` / 8 full run as twice as many 128-query workgroups in a second launch (the
    // same 32-query waves and 32-key blocks: every bit the same).  227 -> 240 us: a CU with ONE 256-query workgroup in the last round
    // already runs it faster (2 waves per SIMD), and the 128-query workgroups stage 64-key tiles.
    const int nq = (T + 255) / 256, items = nq * B * 12, slots = 2 * c->num_cus, tail = items % slots;
    if (big && tail != 0 && tail * 8 <= slots * c->tune.bf16_attn_tail) {
        if (hipError_t e = launch_attention_bf16_v3<8, 128, 4>(qkv, out, B, T, tpref, s, 0, items - tail); e != hipSuccess) return e;
        // (128-query items: clip-head bh, query block 2 qb + {0, 1} - item numbers double; a second half past the clip's end returns at once)
        return launch_attention_bf16_v3_items<4, 64, 4>(qkv, out, T, 2 * nq, tpref, s, 2 * (items - tail), 2 * tail);
    }
#endif
    return big ? launch_attention_bf16_v3<8, 128, 4>(qkv, out, B, T, tpref, s) : launch_attention_bf16_v3<4, 64, 4>(qkv, out, B, T, tpref, s);
}

// x + gelu(pos_conv(x) + bias) of the bf16 forward from the padded group-major buffer: y[M][768] (posconv_bf16_slab.hip.h).  max_t: the
// (longest) clip's frames; tpref / ppref: nullptr for a uniform batch.  The frames per workgroup follow the clip length only to keep
// short clips from idling waves and from streaming the weights for a few rows - an output's bits do not depend on it.
static int run_posconv_bf16_slab(nomad_ctx* c, const bf16_t* xpad, bf16_t* y, int max_t, int B, long long M, const int* tpref,
                                 const int* ppref, hipStream_t s) {
    Scope sc(c, s, NOMAD_K_GEMM, 2.0 * (double)M * 768.0 * 6144.0);
    hipError_t e;
    if (max_t > 256) e = launch_posconv_bf16_slab<8, 1>(xpad, c->pos_wfrag16, c->pos_b, y, max_t, B, tpref, ppref, s);        // 512 frames of one clip
    else if (max_t > 128) e = launch_posconv_bf16_slab<8, 2>(xpad, c->pos_wfrag16, c->pos_b, y, max_t, B, tpref, ppref, s);   // 256 frames of two clips
    else e = launch_posconv_bf16_slab<4, 2>(xpad, c->pos_wfrag16, c->pos_b, y, max_t, B, tpref, ppref, s);                    // 128 frames of two clips
    HIP_TRY(e);
    return 0;
}

// wav rows `stride` apart; lens == nullptr: every clip has l0 frames, else ragged (max_l0 = the longest clip's, pref0 = packed rows)
static void launch_conv0_bf16(nomad_ctx* c, const float* wav, int stride, int l0, int max_l0, int B, const float* scale,
                              const float* shift, bf16_t* out, const int* lens, const int* pref0, hipStream_t s) {
    // the matrix-core kernel (conv0_wfrag: nomad_enable_bf16); the VALU kernel it replaced (1.02-1.13 against 0.88 ms at 32 x 30 s) stays
    // in libnomad_diag.so as a test reference (nomad_diag_conv0_bf16)
    hipLaunchKernelGGL((conv0_mfma_gn_gelu_kernel<kConv0MfmaOcc, kConv0MfmaUf>), dim3((max_l0 + kConv0MfmaFrames - 1) / kConv0MfmaFrames, B), dim3(256), 0, s, wav,
                       stride, l0, c->conv0_wfrag, scale, shift, out, lens, pref0);
}

// plain C / R matrices AND an A map whose divisions have magic numbers (uniform clips of at least two rows, n-fastest tile walk):

#ifdef NOMAD_DIAG
// Race hunting (tools/race_hunt_bf16.py): order-independent checksum of `nseg` equal byte segments of a buffer -
// out[seg] += sum_i word[i] * ((i & 1023) + 1) mod 2^64 (integer adds commute: the value does not depend on scheduling).
__global__ __launch_bounds__(256) void cksum_kernel(const uint32_t* __restrict__ p, long long words, unsigned long long* __restrict__ out) {
    const uint32_t* s = p + (long long)blockIdx.y * words;
    unsigned long long acc = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < words; i += (long long)gridDim.x * 256)
        acc += (unsigned long long)s[i] * (unsigned long long)((i & 1023) + 1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(out + blockIdx.y, acc);
}
// One stage of a forward: segment `seg` of the buffer goes to slot [stage][seg] of the context's checksum table.
struct CkSum {
    nomad_ctx* c;
    hipStream_t s;
    unsigned long long* tab;
    int stages, segs, stage = 0;
    int snap[4];
    void* sdst[4];
    size_t scap[4];
    // on = false (a ragged forward): records nothing, and leaves an armed table / snapshot to the next equal-length call
    CkSum(nomad_ctx* c_, hipStream_t s_, bool on) : c(c_), s(s_), tab(on ? c_->cksum : nullptr), stages(c_->cksum_stages), segs(c_->cksum_segs) {
        if (!on) return;
        for (int k = 0; k < 4; ++k) {
            snap[k] = c->snap_stage[k];
            sdst[k] = c->snap_dst[k];
            scap[k] = c->snap_cap[k];
            c->snap_stage[k] = -1;
        }
        c->cksum = nullptr;  // one forward per nomad_diag_set_cksum / nomad_diag_set_snapshot
        if (tab) (void)hipMemsetAsync(tab, 0, sizeof(unsigned long long) * stages * segs, s);
    }
    void operator()(const void* p, int nseg, size_t seg_bytes) {
        if (!tab) return;
        for (int k = 0; k < 4; ++k)
            if (snap[k] == stage && sdst[k]) {
                const size_t n = std::min(scap[k], (size_t)nseg * seg_bytes);
                (void)hipMemcpyAsync(sdst[k], p, n, hipMemcpyDeviceToDevice, s);
            }
        if (stage < stages && nseg <= segs && seg_bytes % 4 == 0) {
            const long long words = (long long)(seg_bytes / 4);
            const int gx = (int)((words + 256 * 16 - 1) / (256 * 16));
            hipLaunchKernelGGL(cksum_kernel, dim3(gx < 1 ? 1 : (gx > 256 ? 256 : gx), nseg), dim3(256), 0, s,
                               static_cast<const uint32_t*>(p), words, tab + (size_t)stage * segs);
        }
        ++stage;
    }
};
#else
struct CkSum {
    CkSum(nomad_ctx*, hipStream_t, bool) {}
    void operator()(const void*, int, size_t) {}
};
#endif

template <int VPT>
static void launch_ln_bf16(const bf16_t* in, const float* g, const float* b, bf16_t* out, int M, hipStream_t s, int rows) {
    if (rows == 4)
        hipLaunchKernelGGL((layernorm_kernel<VPT, bf16_t, bf16_t, 4>), dim3((M + 15) / 16), dim3(256), 0, s, in, g, b, out,
                           static_cast<float*>(nullptr), M);
    else
        hipLaunchKernelGGL((layernorm_kernel<VPT, bf16_t, bf16_t, 1>), dim3((M + 3) / 4), dim3(256), 0, s, in, g, b, out,
                           static_cast<float*>(nullptr), M);
}

// Scoring forward with bf16 activations / weights and fp32 accumulation, statistics and softmax, over an equal-length or a
// ragged batch (mixed-length long-form files, config C5 through predict: every clip sees the arithmetic of its own
// single-clip call).  The diag library's checksum / snapshot stages are recorded on equal-length calls only.
static int forward_bf16_run(nomad_ctx* c, const float* wav, const BatchGeom& g, const ActLayout& lay, float* emb, char* ws,
                            hipStream_t s, HeadMode mode = {}) {
    auto H = [&](size_t off) { return reinterpret_cast<bf16_t*>(ws + off); };
    auto asf = [](const bf16_t* p_) { return reinterpret_cast<const float*>(p_); };  // GemmParams carries typeless pointers
    auto asfm = [](bf16_t* p_) { return reinterpret_cast<float*>(p_); };
    const int B = g.B, T = g.T, M = (int)g.rows[6];
    int rc;
    double* stats = reinterpret_cast<double*>(ws + lay.stats);
    float* scale = reinterpret_cast<float*>(ws + lay.scale);
    float* shift = reinterpret_cast<float*>(ws + lay.shift);
    bf16_t* cb[2] = {H(lay.conva), H(lay.convb)};
    CkSum CK(c, s, !g.ragged());  // no-op in the product library
    {
        Scope sc(c, s, NOMAD_K_FRONT, 0.0);
        launch_wav_stats(wav, g.wav_ld, g.L[0], g.max_l0, B, stats, g.lens, s);
        hipLaunchKernelGGL(gn_fold_kernel, dim3(B), dim3(512), 0, s, stats, c->conv0_w, c->gn_w, c->gn_b, g.L[0], scale,
                           shift, static_cast<float*>(nullptr), static_cast<float*>(nullptr), g.lens);
    }
    CK(stats, B, sizeof(double) * kStatsPerClip);
    CK(scale, B, sizeof(float) * 512);
    CK(shift, B, sizeof(float) * 512);
    {
        Scope sc(c, s, NOMAD_K_FRONT, 2.0 * (double)g.rows[0] * 512 * 10);
        launch_conv0_bf16(c, wav, g.wav_ld, g.L[0], g.max_l0, B, scale, shift, cb[0], g.lens, g.pref[0], s);
    }
    CK(cb[0], B, sizeof(bf16_t) * 512 * (size_t)g.L[0]);
    for (int i = 1; i < 7; ++i) {
        GemmParams p{};
        p.A = asf(cb[(i - 1) % 2]);
        p.amap = g.conv_amap[i];
        p.K = kConvK[i] * 512;
        p.kchunk = p.K;
        p.W = asf(c->conv_w16[i]);
        p.ldw = p.K;
        p.C = asfm(cb[i % 2]);
        p.M = (int)g.rows[i];
        p.N = 512;
        p.n_valid = 512;
        p.cmap = plain_map(p.M, 512);
        p.rmap = p.cmap;
        p.gelu = 1;
        if ((rc = run_gemm_bf16(c, p, 1, s))) return rc;
        CK(cb[i % 2], B, sizeof(bf16_t) * 512 * (size_t)g.L[i]);
    }
    bf16_t* conv6 = cb[0];
    bf16_t* featln = cb[1];
    {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        launch_ln_bf16<2>(conv6, c->fln_w, c->fln_b, featln, M, s, c->tune.bf16_ln_rows);
    }
    CK(featln, B, sizeof(bf16_t) * 512 * (size_t)T);
    bf16_t* xpad = H(lay.xpad);
    {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        hipLaunchKernelGGL(zero_pad_rows_kernel<bf16_t>, dim3(16 * B), dim3(256), 0, s, xpad, T, g.pref[6], g.ppref, B);
    }
    {
        GemmParams p = dense(asf(featln), 512, asf(c->proj_w16), c->proj_b, nullptr, asfm(xpad), M, 768, 512, 0);
        p.cmap = g.pad_map;
        p.c_colblk = 48;
        p.c_colblk_stride = g.grp_stride;
        if ((rc = run_gemm_bf16(c, p, 1, s))) return rc;
    }
    CK(xpad, 16 * B, sizeof(bf16_t) * 48 * (size_t)(T + 128));
    bf16_t *x = H(lay.x), *x2 = H(lay.x2), *y = H(lay.y), *qkv = H(lay.qkv), *ctxb = H(lay.ctxb), *hb = H(lay.h);
    // (posconv_bf16_slab.hip.h; the grouped GEMM on 128 x 64 tiles it replaced is the reference of its test: nomad_diag_posconv_bf16)
    if ((rc = run_posconv_bf16_slab(c, xpad, y, g.max_t, B, M, g.pref[6], g.ppref, s))) return rc;
    const size_t clip768 = sizeof(bf16_t) * 768 * (size_t)T;
    CK(y, B, clip768);
    {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        launch_ln_bf16<3>(y, c->eln_w, c->eln_b, x, M, s, c->tune.bf16_ln_rows);
    }
    CK(x, B, clip768);
    for (int l = 0; l < NOMAD_NUM_LAYERS; ++l) {
        const LayerDev& d = c->layers[l];
        if ((rc = run_gemm_bf16(c, dense(asf(x), 768, asf(c->qkv_w16[l]), c->qkv_b16[l], nullptr, asfm(qkv), M, 2304, 768, 0), 1, s)))
            return rc;
        CK(qkv, B, clip768 * 3);
        {
            Scope sc(c, s, NOMAD_K_ATTN, g.attn_flops);
            HIP_TRY(run_attention_bf16(c, qkv, ctxb, B, g.max_t, g.pref[6], s));
        }
        CK(ctxb, B, clip768);
        if ((rc = run_gemm_bf16(c, dense(asf(ctxb), 768, asf(c->o_w16[l]), d.o_b, asf(x), asfm(y), M, 768, 768, 0), 1, s)))
            return rc;
        CK(y, B, clip768);
        {
            Scope sc(c, s, NOMAD_K_ROW, 0.0);
            launch_ln_bf16<3>(y, d.ln1_w, d.ln1_b, x2, M, s, c->tune.bf16_ln_rows);
        }
        CK(x2, B, clip768);
        if ((rc = run_gemm_bf16(c, dense(asf(x2), 768, asf(c->fc1_w16[l]), d.fc1_b, nullptr, asfm(hb), M, 3072, 768, 1), 1, s)))
            return rc;
        CK(hb, B, clip768 * 4);
        if ((rc = run_gemm_bf16(c, dense(asf(hb), 3072, asf(c->fc2_w16[l]), d.fc2_b, asf(x2), asfm(y), M, 768, 3072, 0), 1, s)))
            return rc;
        CK(y, B, clip768);
        {
            Scope sc(c, s, NOMAD_K_ROW, 0.0);
            launch_ln_bf16<3>(y, d.ln2_w, d.ln2_b, x, M, s, c->tune.bf16_ln_rows);
        }
        CK(x, B, clip768);
    }
    rc = run_head<bf16_t>(c, x, B, g.max_t, c->emb_w, c->emb_b, emb, g.pref[6], reinterpret_cast<float*>(hb), s, mode);
    CK(emb, B, sizeof(float) * (mode.features ? 768 : 256));
    return rc;
}

static int forward_bf16(nomad_ctx* c, const float* wav, int B, int n_samples, float* emb, void* workspace,
                        size_t workspace_bytes, nomad_stream_t stream, const char* who = "nomad_embed_bf16", HeadMode mode = {}) {
    Shapes sh;
    if (!c || !wav || !emb || !workspace || B <= 0 || !make_shapes(B, n_samples, &sh))
        return fail(NOMAD_ERR_INVALID, "%s: bad argument (B=%d, n_samples=%d)", who, B, n_samples);
    if (!c->bf16_ready) return fail(NOMAD_ERR_INVALID, "%s: call nomad_enable_bf16 first", who);
    const BatchGeom g = geom_uniform(sh);
    const ActLayout lay = make_act_layout(g, sizeof(bf16_t), 0);
    if (workspace_bytes < lay.total)
        return fail(NOMAD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", who, workspace_bytes, lay.total);
    return forward_bf16_run(c, wav, g, lay, emb, static_cast<char*>(workspace), static_cast<hipStream_t>(stream), mode);
}

static int forward_ragged_bf16(nomad_ctx* c, const float* wav, int B, int stride, const int* lens_host, float* emb,
                               void* workspace, size_t workspace_bytes, nomad_stream_t stream,
                               const char* who = "nomad_embed_ragged_bf16", HeadMode mode = {}) {
    if (c && !c->bf16_ready) return fail(NOMAD_ERR_INVALID, "%s: call nomad_enable_bf16 first", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    RaggedBatch r;
    if (int rc = ragged_prologue(who, c, c && wav && emb && workspace, B, stride, lens_host, sizeof(bf16_t), 0,
                                 &r, workspace, workspace_bytes, s))
        return rc;
    if (mode.rows.spans)
        if (int rc = span_upload(c, *mode.rows.spans, s)) return rc;
    return forward_bf16_run(c, wav, r.g, r.lay, emb, static_cast<char*>(workspace), s, mode);
}


// ---- bf16x3 path: fp32-class results on the bf16 matrix cores ------------------------------------------------
// Every dense / conv GEMM runs as three bf16 MFMA products over split operands (gemm_bf16_8phase.hip.h, X3), the
// activations between them live as split planes (dtypes.hip.h) or fp32 - 4 bytes per element either way:
//   conv0 -> split -> conv1..6 (split) -> LN -> split -> post_extract_proj -> split (group-major, padded)
//   -> grouped pos-conv as a Toeplitz GEMM over blocks of 5 frames (N = 5 x 48 per group) -> fp32 -> LN -> split
//   per layer: QKV -> split -> bf16x3 attention -> split -> out-proj (+ split residual) -> fp32 -> LN -> split
//              -> fc1 + GELU -> split -> fc2 (+ split residual) -> fp32 -> LN -> split (fp32 after the last layer)
// Accumulators, bias / GELU / residual, LayerNorm statistics, softmax and the head are fp32 as in the fp32 path.

// bf16x3 attention: K / V of a head resident in LDS when every clip is short enough, the tiled kernel otherwise.
// waves: 0 = tiled kernel, 4 / 8 = resident kernel with that many waves per (clip, head); -1 = the path's choice.
static int run_attention_x3(nomad_ctx* c, const bf16s_t* qkv, long long in_plane, bf16s_t* out, long long out_plane, int B,
                            int T, int max_t, const int* tpref, double flops, hipStream_t s, int waves = -1) {
    Scope sc(c, s, NOMAD_K_ATTN, flops);
    if (waves < 0) waves = max_t <= kAttnResidentMaxT ? kAttnResidentWaves : 0;
    if (waves > 0) {
        if (max_t > kAttnResidentMaxT) return fail(NOMAD_ERR_INVALID, "bf16x3 resident attention: T = %d > %d", max_t, kAttnResidentMaxT);
        static LdsAttrOnce attr_set;
        HIP_TRY(attr_set.ensure(reinterpret_cast<const void*>(attention_x3_resident_kernel), 160 * 1024));
        hipLaunchKernelGGL(attention_x3_resident_kernel, dim3(B * 12), dim3(waves * 64), attn_x3_resident_lds(max_t), s, qkv,
                           in_plane, out, out_plane, T, attn_x3_resident_rows(max_t), tpref);
    } else {
        hipLaunchKernelGGL(attention_x3_kernel, dim3((max_t + 63) / 64, B * 12), dim3(256), 0, s, qkv, in_plane, out, out_plane, T,
                           tpref);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// bf16x3: the padded pos-conv buffer has kXpadSlack zeroed elements behind each plane - the last frame block of a clip reads up
// to kPosBlk - 1 frames past the clip's padding
constexpr int kXpadSlack = 256;

static GemmParams dense_x3(const bf16s_t* A, long long a_plane, int lda, const bf16s_t* W, const float* bias,
                           const bf16s_t* R, long long r_plane, void* C, long long c_plane, int M, int N, int K, int gelu) {
    GemmParams p = dense(reinterpret_cast<const float*>(A), lda, reinterpret_cast<const float*>(W), bias,
                         reinterpret_cast<const float*>(R), static_cast<float*>(C), M, N, K, gelu);
    p.a_plane = a_plane;
    p.w_plane = (long long)N * K;
    p.r_plane = r_plane;
    p.c_plane = c_plane;
    return p;
}

// The GEMM instantiation of the path (run_gemm_bf16 tile ids): the kernel that stages every plane once
// (gemm_bf16x3.hip.h), 2-3 % ahead of the K-concatenated form (20 / 21) in profiles/r01_gemm_bf16x3_shapes.json.
// One instantiation for every shape and batch size: a clip's bits do not depend on the batch it is in.
constexpr int kX3Split = 27, kX3F32 = 28;

static int forward_x3_run(nomad_ctx* c, const float* wav, const BatchGeom& g, const ActLayout& lay, float* emb,
                          char* ws, hipStream_t s, const float* head_w = nullptr, const float* head_b = nullptr,
                          float* layers_out = nullptr, HeadMode mode = {}) {
    auto S = [&](size_t off) { return reinterpret_cast<bf16s_t*>(ws + off); };
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const int B = g.B, M = (int)g.rows[6];
    const int *lens = g.lens, *tpref = g.pref[6];
    const long long pl768 = 768LL * M, pl3072 = 3072LL * M;
    int rc;
    double* stats = reinterpret_cast<double*>(ws + lay.stats);
    float* scale = F(lay.scale);
    float* shift = F(lay.shift);
    bf16s_t* cb[2] = {S(lay.conva), S(lay.convb)};
    const long long cap[2] = {lay.capa, lay.capb};
    {
        Scope sc(c, s, NOMAD_K_FRONT, 0.0);
        launch_wav_stats(wav, g.wav_ld, g.L[0], g.max_l0, B, stats, lens, s);
        hipLaunchKernelGGL(gn_fold_kernel, dim3(B), dim3(512), 0, s, stats, c->conv0_w, c->gn_w, c->gn_b, g.L[0], scale,
                           shift, static_cast<float*>(nullptr), static_cast<float*>(nullptr), lens);
    }
    {
        Scope sc(c, s, NOMAD_K_FRONT, 2.0 * (double)g.rows[0] * 512 * 10);
        hipLaunchKernelGGL(conv0_gn_gelu_kernel<bf16s_t>, dim3((g.max_l0 + kConv0Frames - 1) / kConv0Frames, B), dim3(256), 0,
                           s, wav, g.wav_ld, g.L[0], c->conv0_w, scale, shift, cb[0], lens, g.pref[0], cap[0]);
    }
    for (int i = 1; i < 7; ++i) {
        GemmParams p{};
        p.A = reinterpret_cast<const float*>(cb[(i - 1) % 2]);
        p.a_plane = cap[(i - 1) % 2];
        p.amap = g.conv_amap[i];
        p.K = kConvK[i] * 512;
        p.kchunk = p.K;
        p.W = reinterpret_cast<const float*>(c->conv_wx[i]);
        p.w_plane = 512LL * p.K;
        p.ldw = p.K;
        p.C = reinterpret_cast<float*>(cb[i % 2]);
        p.c_plane = cap[i % 2];
        p.M = (int)g.rows[i];
        p.N = 512;
        p.n_valid = 512;
        p.cmap = plain_map(p.M, 512);
        p.rmap = p.cmap;
        p.gelu = 1;
        if ((rc = run_gemm_bf16(c, p, 1, s, kX3Split))) return rc;
    }
    bf16s_t* conv6 = cb[0];
    bf16s_t* featln = cb[1];
    {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        hipLaunchKernelGGL((layernorm_kernel<2, bf16s_t, bf16s_t>), dim3((M + 3) / 4), dim3(256), 0, s, conv6, c->fln_w,
                           c->fln_b, featln, static_cast<float*>(nullptr), M, cap[0], cap[1]);
    }
    bf16s_t* xpad = S(lay.xpad);
    {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        for (int pl = 0; pl < 2; ++pl) {  // the padding frames (and the slack behind them) are zero in both planes
            bf16_t* plane = reinterpret_cast<bf16_t*>(xpad) + pl * lay.xpad_plane;
            hipLaunchKernelGGL(zero_pad_rows_kernel<bf16_t>, dim3(16 * B), dim3(256), 0, s, plane, g.T, tpref, g.ppref, B);
            HIP_TRY(hipMemsetAsync(plane + 768LL * g.pad_rows, 0, kXpadSlack * sizeof(bf16_t), s));
        }
    }
    {
        GemmParams p = dense_x3(featln, cap[1], 512, c->proj_wx, c->proj_b, nullptr, 0, xpad, lay.xpad_plane, M, 768, 512, 0);
        p.cmap = g.pad_map;
        p.c_colblk = 48;
        p.c_colblk_stride = g.grp_stride;
        if ((rc = run_gemm_bf16(c, p, 1, s, kX3Split))) return rc;
    }
    bf16s_t *x = S(lay.x), *x2 = S(lay.x2), *ctxb = S(lay.ctxb), *hb = S(lay.h);
    float* y = F(lay.y);
    bf16s_t* qkv = S(lay.qkv);
    const long long pl2304 = 2304LL * M;
    {   // grouped pos-conv, x + gelu(conv + bias), as 16 dense GEMMs over blocks of kPosBlk frames:
        // row = (clip, block i): the 132 padded input frames from 5 i on (contiguous in the group-major buffer);
        // column (j, co) = output frame 5 i + j, channel co of the group (Toeplitz weight, posconv_toeplitz_kernel)
        GemmParams p{};
        p.A = reinterpret_cast<const float*>(xpad);
        p.a_plane = lay.xpad_plane;
        p.amap = g.blk_amap;
        p.a_goff = g.grp_stride;
        p.K = kPosKt;
        p.kchunk = kPosKt;
        p.W = reinterpret_cast<const float*>(c->pos_wx);
        p.w_plane = 16LL * 256 * kPosKt;
        p.ldw = kPosKt;
        p.w_goff = 256LL * kPosKt;
        p.bias = c->pos_bx;
        p.bias_goff = 256;
        p.C = y;
        p.cmap = g.blk_cmap;
        p.c_goff = 48;
        p.c_colblk = 48;
        p.c_colblk_stride = 768;   // column block j = the next frame's row of y
        p.c_blk_step = kPosBlk;
        p.c_clip_frames = g.T;
        p.R = reinterpret_cast<const float*>(xpad);   // residual: frame 64 + 5 i + j of the same buffer = rmap(row) + j * 48 + co
        p.r_plane = lay.xpad_plane;
        p.rmap = g.blk_rmap;
        p.r_goff = g.grp_stride;
        p.M = (int)g.pos_blocks;
        p.N = 256;
        p.n_valid = kPosBlk * 48;
        p.gelu = 1;
        if ((rc = run_gemm_bf16(c, p, 16, s, kX3F32))) return rc;
    }
    auto ln = [&](const float* in, const float* gm, const float* bt, bf16s_t* out, float* out2 = nullptr) {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        hipLaunchKernelGGL((layernorm_kernel<3, float, bf16s_t>), dim3((M + 3) / 4), dim3(256), 0, s, in, gm, bt, out, out2, M,
                           0LL, pl768);
    };
    ln(y, c->eln_w, c->eln_b, x);
    for (int l = 0; l < NOMAD_NUM_LAYERS; ++l) {
        const LayerDev& d = c->layers[l];
        if ((rc = run_gemm_bf16(c, dense_x3(x, pl768, 768, c->qkv_wx[l], d.qkv_b, nullptr, 0, qkv, pl2304, M, 2304, 768, 0), 1, s, kX3Split)))
            return rc;
        if ((rc = run_attention_x3(c, qkv, pl2304, ctxb, pl768, B, g.T, g.max_t, tpref, g.attn_flops, s))) return rc;
        if ((rc = run_gemm_bf16(c, dense_x3(ctxb, pl768, 768, c->o_wx[l], d.o_b, x, pl768, y, 0, M, 768, 768, 0), 1, s, kX3F32)))
            return rc;
        ln(y, d.ln1_w, d.ln1_b, x2);
        if ((rc = run_gemm_bf16(c, dense_x3(x2, pl768, 768, c->fc1_wx[l], d.fc1_b, nullptr, 0, hb, pl3072, M, 3072, 768, 1), 1, s, kX3Split)))
            return rc;
        if ((rc = run_gemm_bf16(c, dense_x3(hb, pl3072, 3072, c->fc2_wx[l], d.fc2_b, x2, pl768, y, 0, M, 768, 3072, 0), 1, s, kX3F32)))
            return rc;
        // layer_results (nomad.py:250-253): the fp32 LayerNorm output, written next to its split copy
        float* lo = layers_out ? layers_out + (size_t)l * M * 768 : nullptr;
        if (l + 1 < NOMAD_NUM_LAYERS) ln(y, d.ln2_w, d.ln2_b, x, lo);
        else if ((rc = run_layernorm(c, y, d.ln2_w, d.ln2_b, reinterpret_cast<float*>(x), lo, M, 768, s))) return rc;
    }
    return run_head<float>(c, reinterpret_cast<const float*>(x), B, g.max_t, head_w ? head_w : c->emb_w, head_b ? head_b : c->emb_b, emb,
                           tpref, reinterpret_cast<float*>(hb), s, mode);
}

static int forward_x3(nomad_ctx* c, const float* wav, int B, int n_samples, float* emb, void* workspace,
                      size_t workspace_bytes, nomad_stream_t stream, const float* head_w = nullptr, const float* head_b = nullptr,
                      float* layers_out = nullptr, const char* who = "nomad_embed_bf16x3", HeadMode mode = {}) {
    Shapes sh;
    if (!c || !wav || !emb || !workspace || B <= 0 || !make_shapes(B, n_samples, &sh) || (!head_w != !head_b))
        return fail(NOMAD_ERR_INVALID, "%s: bad argument (B=%d, n_samples=%d)", who, B, n_samples);
    if (!c->x3_ready) return fail(NOMAD_ERR_INVALID, "%s: call nomad_enable_bf16x3 first", who);
    const BatchGeom g = geom_uniform(sh);
    const ActLayout lay = make_act_layout(g, 4, kXpadSlack);
    if (workspace_bytes < lay.total)
        return fail(NOMAD_ERR_WORKSPACE, "%s: workspace %zu < required %zu", who, workspace_bytes, lay.total);
    return forward_x3_run(c, wav, g, lay, emb, static_cast<char*>(workspace), static_cast<hipStream_t>(stream), head_w, head_b,
                          layers_out, mode);
}

static int forward_ragged_x3(nomad_ctx* c, const float* wav, int B, int stride, const int* lens_host, float* emb,
                             void* workspace, size_t workspace_bytes, nomad_stream_t stream,
                             const char* who = "nomad_embed_ragged_bf16x3", HeadMode mode = {}) {
    if (c && !c->x3_ready) return fail(NOMAD_ERR_INVALID, "%s: call nomad_enable_bf16x3 first", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    RaggedBatch r;
    if (int rc = ragged_prologue(who, c, c && wav && emb && workspace, B, stride, lens_host, 4, kXpadSlack,
                                 &r, workspace, workspace_bytes, s))
        return rc;
    if (mode.rows.spans)
        if (int rc = span_upload(c, *mode.rows.spans, s)) return rc;
    return forward_x3_run(c, wav, r.g, r.lay, emb, static_cast<char*>(workspace), s, nullptr, nullptr, nullptr, mode);
}

extern "C" {

int nomad_enable_bf16(nomad_ctx* c) {
    if (!c) return fail(NOMAD_ERR_INVALID, "null ctx");
    if (c->bf16_ready) return 0;
    HIP_TRY(hipSetDevice(c->device));
    // A weight update (nomad_train_adam_step / nomad_train_write) rebuilt the fp32 kernel-layout weights on the CALLER's
    // stream, which may be a non-blocking stream the null stream does not wait for: drain the device before converting.
    HIP_TRY(hipDeviceSynchronize());
    static const char who[] = "nomad_enable_bf16";   // (a buffer that exists is reused: re-enabling after a weight update)
    auto to_bf16 = [&](const float* src, size_t n, bf16_t** out) -> int {
        if (int rc = dev_alloc(c, who, n, out)) return rc;
        hipLaunchKernelGGL(to_bf16_kernel, dim3(1024), dim3(256), 0, 0, src, *out, (long long)(n / 4));
        return 0;
    };
    int rc;
    if ((rc = for_each_gemm_weight(c, [&](const GemmWeight& g) { return to_bf16(g.w, (size_t)g.N * g.K, g.w16); }))) return rc;
    // what is not a plain conversion of one GEMM weight: conv0's and the pos-conv's operands in MFMA fragment order ...
    if ((rc = dev_alloc(c, who, (size_t)8 * 4 * 64 * 8, &c->conv0_wfrag))) return rc;
    hipLaunchKernelGGL(conv0_wfrag_kernel, dim3(32), dim3(64), 0, 0, c->conv0_w, c->conv0_wfrag);
    if ((rc = to_bf16(c->pos_w, (size_t)16 * 64 * 6144, &c->pos_w16))) return rc;
    if ((rc = dev_alloc(c, who, posconv_wfrag_elems(), &c->pos_wfrag16))) return rc;
    hipLaunchKernelGGL(posconv_wfrag_kernel, dim3(16 * 192), dim3(192), 0, 0, c->pos_w, c->pos_wfrag16);
    for (int l = 0; l < NOMAD_NUM_LAYERS; ++l) {  // ... and the q rows of the fused QKV weight and bias, which also carry log2(e)
        const LayerDev& d = c->layers[l];
        hipLaunchKernelGGL(to_bf16_scaled_kernel, dim3(1024), dim3(256), 0, 0, d.qkv_w, c->qkv_w16[l], (long long)2304 * 768 / 4,
                           (long long)768 * 768 / 4, kLog2e);  // q rows: q * 64^-0.5 * log2(e), rounded to bf16 once
        if ((rc = dev_alloc(c, who, 2304, &c->qkv_b16[l]))) return rc;
        hipLaunchKernelGGL(scale_head_kernel, dim3(9), dim3(256), 0, 0, d.qkv_b, c->qkv_b16[l], 2304, 768, kLog2e);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    c->bf16_ready = true;
    return 0;
}

int nomad_workspace_bytes_bf16(const nomad_ctx* c, int B, int n_samples, size_t* bytes) {
    Shapes sh;
    if (!c || !bytes || B <= 0 || !make_shapes(B, n_samples, &sh))
        return fail(NOMAD_ERR_INVALID, "nomad_workspace_bytes_bf16: bad shape B=%d N=%d", B, n_samples);
    *bytes = make_act_layout(geom_uniform(sh), sizeof(bf16_t), 0).total;
    return 0;
}

int nomad_embed_bf16(nomad_ctx* c, const float* wav, int B, int n_samples, float* emb, void* workspace,
                     size_t workspace_bytes, nomad_stream_t stream) {
    if (int rc = refuse_cut(c, "nomad_embed_bf16")) return rc;
    return forward_bf16(c, wav, B, n_samples, emb, workspace, workspace_bytes, stream);
}


int nomad_enable_bf16x3(nomad_ctx* c) {
    if (!c) return fail(NOMAD_ERR_INVALID, "null ctx");
    if (c->x3_ready) return 0;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());  // see nomad_enable_bf16: the fp32 weights may have been rebuilt on another stream
    static const char who[] = "nomad_enable_bf16x3";   // (a buffer that exists is reused: re-enabling after a weight update)
    int rc = for_each_gemm_weight(c, [&](const GemmWeight& g) -> int {
        const size_t n = (size_t)g.N * g.K;
        if (int rc = dev_alloc(c, who, 2 * n, g.wx)) return rc;
        hipLaunchKernelGGL(split_bf16_kernel, dim3(1024), dim3(256), 0, 0, g.w, *g.wx, (long long)n, (long long)(n / 4));
        return 0;
    });
    if (rc) return rc;
    {  // what is not a split copy of one GEMM weight: the pos-conv in Toeplitz form and its bias
        const size_t n = (size_t)16 * 256 * kPosKt;
        if ((rc = dev_alloc(c, who, 2 * n, &c->pos_wx))) return rc;
        if ((rc = dev_alloc(c, who, (size_t)16 * 256, &c->pos_bx))) return rc;
        hipLaunchKernelGGL(posconv_toeplitz_kernel, dim3(16 * 256), dim3(256), 0, 0, c->pos_w, c->pos_wx, (long long)n);
        hipLaunchKernelGGL(posconv_toeplitz_bias_kernel, dim3(16), dim3(256), 0, 0, c->pos_b, c->pos_bx);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    c->x3_ready = true;
    return 0;
}

int nomad_workspace_bytes_bf16x3(const nomad_ctx* c, int B, int n_samples, size_t* bytes) {
    Shapes sh;
    if (!c || !bytes || B <= 0 || !make_shapes(B, n_samples, &sh))
        return fail(NOMAD_ERR_INVALID, "nomad_workspace_bytes_bf16x3: bad shape B=%d N=%d", B, n_samples);
    *bytes = make_act_layout(geom_uniform(sh), 4, kXpadSlack).total;
    return 0;
}

int nomad_workspace_bytes_ragged_bf16x3(const nomad_ctx* c, int B, const int* lengths_host, size_t* bytes) {
    RaggedBatch r;
    if (int rc = ragged_prologue("nomad_workspace_bytes_ragged_bf16x3", nullptr, c && bytes, B, 0, lengths_host, 4, kXpadSlack, &r)) return rc;
    *bytes = r.lay.total;
    return 0;
}

int nomad_embed_ragged_bf16x3(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, float* emb,
                              void* workspace, size_t workspace_bytes, nomad_stream_t stream) {
    if (int rc = refuse_cut(c, "nomad_embed_ragged_bf16x3")) return rc;
    return forward_ragged_x3(c, wav, B, stride, lengths_host, emb, workspace, workspace_bytes, stream);
}

int nomad_embed_bf16x3(nomad_ctx* c, const float* wav, int B, int n_samples, float* emb, void* workspace,
                       size_t workspace_bytes, nomad_stream_t stream) {
    if (int rc = refuse_cut(c, "nomad_embed_bf16x3")) return rc;
    return forward_x3(c, wav, B, n_samples, emb, workspace, workspace_bytes, stream);
}

int nomad_embed_layers_bf16x3(nomad_ctx* c, const float* wav, int B, int n_samples, const float* head_w, const float* head_b,
                              float* emb, float* layers_out, void* workspace, size_t workspace_bytes, nomad_stream_t stream) {
    if (!layers_out) return fail(NOMAD_ERR_INVALID, "nomad_embed_layers_bf16x3: layers_out is NULL");
    if (int rc = refuse_cut(c, "nomad_embed_layers_bf16x3")) return rc;   // (no depth cut on split bf16 storage)
    return forward_x3(c, wav, B, n_samples, emb, workspace, workspace_bytes, stream, head_w, head_b, layers_out);
}

int nomad_diag_split_bf16(nomad_ctx* c, const float* in, void* out, long long plane, long long n, int inverse,
                          nomad_stream_t stream) {
    if (!c || !in || !out || n <= 0 || n % 4 || plane < n) return fail(NOMAD_ERR_INVALID, "nomad_diag_split_bf16: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (inverse)  // `in` is the split buffer, `out` the fp32 one
        hipLaunchKernelGGL(unsplit_bf16_kernel, dim3(1024), dim3(256), 0, s, reinterpret_cast<const bf16s_t*>(in), plane,
                           static_cast<float*>(out), n / 4);
    else
        hipLaunchKernelGGL(split_bf16_kernel, dim3(1024), dim3(256), 0, s, in, static_cast<bf16s_t*>(out), plane, n / 4);
    HIP_TRY(hipGetLastError());
    return 0;
}

int nomad_diag_attention_bf16x3(nomad_ctx* c, const void* qkv, void* out, int B, int T, int waves, nomad_stream_t stream) {
    if (!c || !qkv || !out || B <= 0 || T <= 0) return fail(NOMAD_ERR_INVALID, "nomad_diag_attention_bf16x3: bad argument");
    return run_attention_x3(c, static_cast<const bf16s_t*>(qkv), (long long)B * T * 2304, static_cast<bf16s_t*>(out),
                            (long long)B * T * 768, B, T, T, kNoInts, 4.0 * B * 12.0 * (double)T * T * 64,
                            static_cast<hipStream_t>(stream), waves);
}

int nomad_diag_gemm_bf16x3(nomad_ctx* c, const void* A, const void* W, const float* bias, const void* R, void* C, int M,
                           int N, int K, int gelu, int out_f32, nomad_stream_t stream) {
    if (!c || !A || !W || !C || M <= 0 || N % 256 || K % ((out_f32 % 100 == 12 || out_f32 % 100 == 13) ? 192 : out_f32 % 100 >= 7 ? 64 : 128))
        return fail(NOMAD_ERR_INVALID, "nomad_diag_gemm_bf16x3: bad argument (N %% 256, K %% 128; K %% 64 for the staged kernel)");
    const int group_m = out_f32 / 100;  // measurement knob: variant + 100 * group_m (tile_coords)
    out_f32 %= 100;
    GemmParams p = dense_x3(static_cast<const bf16s_t*>(A), (long long)M * K, K, static_cast<const bf16s_t*>(W), bias,
                            static_cast<const bf16s_t*>(R), (long long)M * N, C, (long long)M * N, M, N, K, gelu);
    p.group_m = group_m;
    return run_gemm_bf16(c, p, 1, static_cast<hipStream_t>(stream), 20 + (out_f32 < 0 ? 0 : out_f32 > 13 ? 13 : out_f32));
}

int nomad_workspace_bytes_ragged_bf16(const nomad_ctx* c, int B, const int* lengths_host, size_t* bytes) {
    RaggedBatch r;
    if (int rc = ragged_prologue("nomad_workspace_bytes_ragged_bf16", nullptr, c && bytes, B, 0, lengths_host, sizeof(bf16_t), 0, &r))
        return rc;
    *bytes = r.lay.total;
    return 0;
}

int nomad_embed_ragged_bf16(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, float* emb,
                            void* workspace, size_t workspace_bytes, nomad_stream_t stream) {
    if (int rc = refuse_cut(c, "nomad_embed_ragged_bf16")) return rc;
    return forward_ragged_bf16(c, wav, B, stride, lengths_host, emb, workspace, workspace_bytes, stream);
}

#ifdef NOMAD_DIAG
/* Race hunting: the NEXT nomad_embed_bf16 call on this context writes table[stage][seg] (stages x segs 64-bit sums, device
 * memory) - stage order: GroupNorm sums, scale, shift, conv0..6, feature LN, padded projection (16 x B segments), pos-conv,
 * encoder LN, then per layer qkv / ctx / out_proj+res / LN1 / fc1 / fc2+res / LN2, last the embeddings; seg = clip. */
int nomad_diag_set_cksum(nomad_ctx* c, unsigned long long* table_dev, int stages, int segs) {
    if (!c) return fail(NOMAD_ERR_INVALID, "null ctx");
    c->cksum = table_dev;
    c->cksum_stages = stages;
    c->cksum_segs = segs;
    return 0;
}
/* ... and copies the buffer of stage `stage` (up to cap bytes) to dst_dev on the forward's stream; slot 0..3. */
int nomad_diag_set_snapshot(nomad_ctx* c, int slot, int stage, void* dst_dev, size_t cap) {
    if (!c || slot < 0 || slot > 3) return fail(NOMAD_ERR_INVALID, "nomad_diag_set_snapshot: bad argument");
    c->snap_stage[slot] = stage;
    c->snap_dst[slot] = dst_dev;
    c->snap_cap[slot] = cap;
    return 0;
}
/* Poison test (tests/test_gpu_poison.py): fill, on `stream`, every context-owned device buffer whose content is not meant to
 * outlive a call with `byte`, so that a later call shows any element it reads before writing.  Filled (each one is written in
 * full by the call that reads it, before it reads it):
 *   splitk_part     split-K partial slices of the loss forward / backward (nomad_enable_backward)
 *   pair_scratch    every nomad_pairwise block, bound to a stream or not: per-(ref tile, deg row) row sums
 *   tap_partial     weight-norm backward and refresh_weights: per-block tap sums (nomad_train_enable)
 *   tap_dot         weight-norm backward: the per-tap dot products folded from tap_partial
 * Left alone (state): the weights and every derived copy of them (conv_bw_*, *_wT, pos_w / pos_wb, bf16 / split copies ...),
 * theta, adam_m, adam_v, grad (written by nomad_train_write), and pos_nrm2: ||v_t||^2 of the pos-conv weight norm, derived from
 * theta by refresh_weights together with pos_w and read by every later backward, as pos_w is by every forward. */
int nomad_diag_poison_scratch(nomad_ctx* c, int byte, nomad_stream_t stream) {
    if (!c || byte < 0 || byte > 255) return fail(NOMAD_ERR_INVALID, "nomad_diag_poison_scratch: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(c->device));
    if (c->splitk_part) HIP_TRY(hipMemsetAsync(c->splitk_part, byte, kSplitKPartFloats * sizeof(float), s));
    {
        std::lock_guard<std::mutex> lock(c->pair_mu);
        for (const auto& e : c->pair_scratch) HIP_TRY(hipMemsetAsync(e.second, byte, sizeof(double) * kPairScratchDoubles, s));
    }
    if (c->tap_partial) HIP_TRY(hipMemsetAsync(c->tap_partial, byte, (size_t)576 * 128 * sizeof(double), s));
    if (c->tap_dot) HIP_TRY(hipMemsetAsync(c->tap_dot, byte, 128 * sizeof(double), s));
    return 0;
}
/* The bf16 forward's front end alone: waveform statistics -> GroupNorm scale / shift -> conv0 + GroupNorm + GELU as bf16
 * out_dev [B][L0][512]; scratch_dev: 8 * 65 * B * (1 + chunks) + 2 * 4 * 512 * B bytes (race hunting: the victim kernel).
 * variant: conv0_gn_gelu_kernel's VAR (0 = the forward's kernel, bit 0 no LDS, bit 1 scalar tap loop). */
int nomad_diag_conv0_bf16(nomad_ctx* c, const float* wav, int B, int n_samples, void* out_dev, void* scratch_dev,
                          nomad_stream_t stream, int variant) {
    Shapes sh;
    if (!c || !wav || !out_dev || !scratch_dev || !make_shapes(B, n_samples, &sh)) return fail(NOMAD_ERR_INVALID, "nomad_diag_conv0_bf16");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* stats = static_cast<double*>(scratch_dev);
    float* scale = reinterpret_cast<float*>(stats + stats_doubles(B, sh.L[0]));
    float* shift = scale + 512 * (size_t)B;
    launch_wav_stats(wav, n_samples, sh.L[0], sh.L[0], B, stats, kNoInts, s);
    hipLaunchKernelGGL(gn_fold_kernel, dim3(B), dim3(512), 0, s, stats, c->conv0_w, c->gn_w, c->gn_b, sh.L[0], scale, shift,
                       static_cast<float*>(nullptr), static_cast<float*>(nullptr), kNoInts);
    const dim3 grid((sh.L[0] + kConv0Frames - 1) / kConv0Frames, B);
    bf16_t* out = static_cast<bf16_t*>(out_dev);
#define NOMAD_C0(V)                                                                                                             \
    case V:                                                                                                                     \
        hipLaunchKernelGGL((conv0_gn_gelu_kernel<bf16_t, V>), grid, dim3(256), 0, s, wav, n_samples, sh.L[0], c->conv0_w, scale, \
                           shift, out, kNoInts, kNoInts, 0LL);                                                                  \
        break;
    switch (variant) {
        NOMAD_C0(0) NOMAD_C0(1) NOMAD_C0(2) NOMAD_C0(3)
#define NOMAD_C0M(V, OCC, UF, ABL)                                                                                                \
    case V:                                                                                                                     \
        if (!c->conv0_wfrag) return fail(NOMAD_ERR_INVALID, "nomad_diag_conv0_bf16: variant %d needs nomad_enable_bf16", V);    \
        hipLaunchKernelGGL((conv0_mfma_gn_gelu_kernel<OCC, UF, ABL>), dim3((sh.L[0] + kConv0MfmaFrames - 1) / kConv0MfmaFrames, B), \
                           dim3(256), 0, s, wav, n_samples, sh.L[0], c->conv0_wfrag, scale, shift, out, kNoInts, kNoInts);      \
        break;
        NOMAD_C0M(4, kConv0MfmaOcc, kConv0MfmaUf, 0)   // the matrix-core kernel as the bf16 forward launches it (needs nomad_enable_bf16)
        NOMAD_C0M(5, 3, 2, 0) NOMAD_C0M(6, 3, 1, 0) NOMAD_C0M(7, 3, 4, 0)   // other budgets / unrolls (tools/conv0_time.py)
        NOMAD_C0M(9, 4, 1, 2)                                             // timing probe: no GELU
#undef NOMAD_C0M
        default: return fail(NOMAD_ERR_INVALID, "nomad_diag_conv0_bf16: variant %d", variant);
    }
#undef NOMAD_C0
    HIP_TRY(hipGetLastError());
    return 0;
}
#endif

#ifdef NOMAD_DIAG
/* The bf16 forward's positional convolution alone: y_dev [B*T][768] bf16 = x + gelu(pos_conv(x) + bias) from xpad_dev, the padded
 * group-major input [16][B][T + 128][48] bf16 (zero frames 0..63 and T+64.. of every clip).  variant 1: posconv_bf16_slab.hip.h (what
 * the forward launches); 0: the grouped GEMM on 128 x 64 tiles it replaced.  Needs nomad_enable_bf16. */
int nomad_diag_posconv_bf16(nomad_ctx* c, const void* xpad_dev, void* y_dev, int B, int T, nomad_stream_t stream, int variant) {
    if (!c || !xpad_dev || !y_dev || B <= 0 || T <= 0 || !c->pos_w16) return fail(NOMAD_ERR_INVALID, "nomad_diag_posconv_bf16: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bf16_t* xpad = static_cast<const bf16_t*>(xpad_dev);
    bf16_t* y = static_cast<bf16_t*>(y_dev);
    const long long M = (long long)B * T;
    if (variant == 1) return run_posconv_bf16_slab(c, xpad, y, T, B, M, nullptr, nullptr, s);
    if (variant != 0) return fail(NOMAD_ERR_INVALID, "nomad_diag_posconv_bf16: variant %d", variant);
    const long long grp_stride = (long long)B * (T + 128) * 48;
    auto asf = [](const bf16_t* p_) { return reinterpret_cast<const float*>(p_); };  // GemmParams carries typeless pointers
    auto asfm = [](bf16_t* p_) { return reinterpret_cast<float*>(p_); };
    GemmParams p{};
    p.A = asf(xpad);
    p.amap = RowMap{0, (long long)(T + 128) * 48, T, 48};
    p.a_goff = grp_stride;
    p.K = 6144;
    p.kchunk = 6144;
    p.W = asf(c->pos_w16);
    p.ldw = 6144;
    p.w_goff = 64LL * 6144;
    p.bias = c->pos_b;
    p.bias_goff = 48;
    p.C = asfm(y);
    p.cmap = plain_map(M, 768);
    p.c_goff = 48;
    p.R = asf(xpad);
    p.rmap = RowMap{64LL * 48, (long long)(T + 128) * 48, T, 48};
    p.r_goff = grp_stride;
    p.M = (int)M;
    p.N = 64;
    p.n_valid = 48;
    p.gelu = 1;
    return run_gemm_bf16(c, p, 16, s);
}

// timeline of the last probe GEMM: out_host[6 * n] = per workgroup {entry, loop start, loop end, stores done, HW_ID, XCC_ID}.  The probe kernels
// live in two translation units, each with its own copy of the device buffer: the copy with the newer stamps is the last probe's.
int nomad_diag_timeline(unsigned long long* out_host, int n) {
    if (!out_host || n <= 0 || n > kTimelineSlots) return fail(NOMAD_ERR_INVALID, "nomad_diag_timeline: bad argument");
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> a(6 * (size_t)n), b(6 * (size_t)n);
    if (int rc = gemm_f32_timeline_read(a.data(), n)) return rc;
    if (int rc = gemm_bf16_timeline_read(b.data(), n)) return rc;
    unsigned long long ma = 0, mb = 0;
    for (int i = 0; i < n; ++i) { ma = std::max(ma, a[6 * (size_t)i]); mb = std::max(mb, b[6 * (size_t)i]); }
    std::memcpy(out_host, (ma >= mb ? a : b).data(), sizeof(unsigned long long) * 6 * (size_t)n);
    return 0;
}

/* Test hook: the fp32 pos-conv alone on the caller's operands, in the form NOMAD_F32_POSCONV_WINO selects - nested F(2,2)
 * (posconv_wino_f32.hip.h) or, with NOMAD_F32_POSCONV_WINO=0 or bf16x3 products, the direct 128-tap GEMM - whether or not this
 * context's forwards run the frequency domain instead (nomad_diag_posconv_fft is that form's hook).  x: the padded
 * group-major input [16][sum_c (T_c + 128)][48] (zero frames 0..63 and T_c + 64.. of every clip); v: weights as pos_w,
 * [16][64][6144]; bias: [768] or null; y = x + gelu(u), u (nullable) = pos_conv(x) + bias: [sum_c T_c][768].  lens_host: the
 * clips' frame counts T_c.  ragged = 0: the uniform launch (every T_c equal), 1: the ragged one.  Synchronous. */
int nomad_diag_posconv(nomad_ctx* c, const float* x, const float* v, const float* bias, float* y, float* u, int B,
                       const int* lens_host, int ragged, nomad_stream_t stream) {
    if (!c || !x || !v || !y || !lens_host || B <= 0) return fail(NOMAD_ERR_INVALID, "nomad_diag_posconv: bad argument");
    std::vector<int> meta(4 * (size_t)(B + 1), 0);   // frame / padded frame prefix sums; room for the operands' (run_posconv_wino)
    int max_t = 0;
    long long q_rows = 0;
    for (int b = 0; b < B; ++b) {
        const int T = lens_host[b], q = (T + kPwRate - 1) / kPwRate;
        if (T <= 0 || (!ragged && T != lens_host[0])) return fail(NOMAD_ERR_INVALID, "nomad_diag_posconv: clip %d of %d frames", b, T);
        meta[b + 1] = meta[b] + T;
        meta[(B + 1) + b + 1] = meta[(B + 1) + b] + T + 128;
        q_rows += q;
        max_t = std::max(max_t, T);
    }
    PosWinoGeom geo{B, ragged ? 0 : lens_host[0], nullptr, nullptr, nullptr, nullptr, meta[(B + 1) + B], q_rows,
                    q_rows + (long long)B * (kPwTaps - 1), (max_t + kPwRate - 1) / kPwRate};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t meta_bytes = (sizeof(int) * meta.size() + 255) & ~size_t(255), wt_bytes = sizeof(float) * 16 * kPwOps * 64 * kPwK;
    const size_t q_bytes = (pos_wino_q_bytes(geo.q_frames) + 255) & ~size_t(255);
    char* d = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), meta_bytes + wt_bytes + q_bytes + pos_wino_s_bytes(geo.q_rows)));
    int* dm = reinterpret_cast<int*>(d);
    float* wt = reinterpret_cast<float*>(d + meta_bytes);
    float* wq = reinterpret_cast<float*>(d + meta_bytes + wt_bytes);
    float* ws = reinterpret_cast<float*>(d + meta_bytes + wt_bytes + q_bytes);
    int rc = 0;
    if (hipMemcpy(dm, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice) != hipSuccess) rc = fail(NOMAD_ERR_HIP, "nomad_diag_posconv: copy");
    if (ragged) {
        geo.tpref = dm;
        geo.ppref = dm + (B + 1);
    }
    if (rc == 0 && posconv_wino(c)) {
        hipLaunchKernelGGL(posconv_wino_weight_kernel, dim3(16 * kPwOps * 64), dim3(256), 0, s, v, wt);
        rc = run_posconv_wino(c, x, wt, bias, y, u, geo, wq, ws, dm + 2 * (B + 1), s);
    } else if (rc == 0) {
        const int T = lens_host[0], M = meta[B];
        GemmParams p{};
        p.A = x;
        p.amap = ragged ? RowMap{0, 0, 0, 48, dm, dm + (B + 1), B, 48} : RowMap{0, (long long)(T + 128) * 48, T, 48};
        p.a_goff = geo.pad_rows * 48;
        p.K = 6144;
        p.kchunk = 6144;
        p.W = v;
        p.ldw = 6144;
        p.w_goff = 64LL * 6144;
        p.bias = bias;
        p.bias_goff = 48;
        p.C = y;
        p.Upre = u;
        p.cmap = plain_map(M, 768);
        p.c_goff = 48;
        p.R = x;
        p.rmap = p.amap;
        p.rmap.off = 64LL * 48;
        p.r_goff = p.a_goff;
        p.M = M;
        p.N = 64;
        p.n_valid = 48;
        p.gelu = 1;
        rc = gemm_f32_dispatch(c, p, 16, 48, s);
    }
    if (rc == 0 && hipStreamSynchronize(s) != hipSuccess) rc = fail(NOMAD_ERR_HIP, "nomad_diag_posconv: kernel");
    (void)hipFree(d);
    return rc;
}
#endif

/* Test hook: the fp32 pos-conv alone on the caller's operands in the frequency domain (posconv_fft_f32.hip.h), whatever form this
 * context's forwards run.  Arguments as nomad_diag_posconv.  Synchronous. */
int nomad_diag_posconv_fft(nomad_ctx* c, const float* x, const float* v, const float* bias, float* y, float* u, int B,
                           const int* lens_host, int ragged, nomad_stream_t stream) {
    if (!c || !x || !v || !y || !lens_host || B <= 0) return fail(NOMAD_ERR_INVALID, "nomad_diag_posconv_fft: bad argument");
    std::vector<int> meta(3 * (size_t)(B + 1), 0);   // frame / padded frame prefix sums; room for the units' (run_posconv_fft)
    int max_t = 0;
    long long units = 0;
    for (int b = 0; b < B; ++b) {
        const int T = lens_host[b];
        if (T <= 0 || (!ragged && T != lens_host[0])) return fail(NOMAD_ERR_INVALID, "nomad_diag_posconv_fft: clip %d of %d frames", b, T);
        meta[b + 1] = meta[b] + T;
        meta[(B + 1) + b + 1] = meta[(B + 1) + b] + T + 128;
        units += pos_fft_blocks(T);
        max_t = std::max(max_t, T);
    }
    if (units >= (1 << 30) / kPfCols) return fail(NOMAD_ERR_INVALID, "nomad_diag_posconv_fft: %lld units", units);
    PosFftGeom geo{B, ragged ? 0 : lens_host[0], nullptr, nullptr, nullptr, meta[(B + 1) + B], (int)units, pos_fft_blocks(max_t)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t meta_bytes = (sizeof(int) * meta.size() + 255) & ~size_t(255), wf_bytes = sizeof(float) * kPfWeightFloats;
    const size_t spec_bytes = (pos_fft_spec_bytes(units) + 255) & ~size_t(255);
    char* d = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), meta_bytes + wf_bytes + 2 * spec_bytes));
    int* dm = reinterpret_cast<int*>(d);
    float* wf = reinterpret_cast<float*>(d + meta_bytes);
    float* sx = reinterpret_cast<float*>(d + meta_bytes + wf_bytes);
    float* sy = reinterpret_cast<float*>(d + meta_bytes + wf_bytes + spec_bytes);
    int rc = 0;
    if (hipMemcpy(dm, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice) != hipSuccess) rc = fail(NOMAD_ERR_HIP, "nomad_diag_posconv_fft: copy");
    if (ragged) {
        geo.tpref = dm;
        geo.ppref = dm + (B + 1);
    }
    if (rc == 0) rc = launch_posconv_fft_weights(c, v, wf, s);
    if (rc == 0) rc = run_posconv_fft(c, x, wf, bias, y, u, geo, sx, sy, dm + 2 * (B + 1), s);
    if (rc == 0 && hipStreamSynchronize(s) != hipSuccess) rc = fail(NOMAD_ERR_HIP, "nomad_diag_posconv_fft: kernel");
    (void)hipFree(d);
    return rc;
}

int nomad_diag_gemm_bf16(nomad_ctx* c, const void* A, const void* W, const float* bias, const void* R, void* C, int M,
                         int N, int K, int gelu, int tile, nomad_stream_t stream) {
    static const int kBN[] = {128, 128, 64, 256, 64, 128, 128, 128, 128, 256, 256, 128, 128, 128, 128, 256, 256, 256, 256, 256};
    const bool big256 = tile == 36 || (tile >= 42 && tile <= 54) || tile == 57 || tile == 58 || (tile >= 60 && tile <= 68);
    if (tile == 55 || tile == 56) {  // 256 x 192 tiles of the deep-pipelined kernel
        if (!c || !A || !W || !C || M <= 0) return fail(NOMAD_ERR_INVALID, "nomad_diag_gemm_bf16: bad argument");
        if (N % 192 || K % 128) return fail(NOMAD_ERR_INVALID, "nomad_diag_gemm_bf16: N %% 192 or K %% 128 != 0");
        GemmParams p192 = dense(static_cast<const float*>(A), K, static_cast<const float*>(W), bias, static_cast<const float*>(R),
                                static_cast<float*>(C), M, N, K, gelu);
        return run_gemm_bf16(c, p192, 1, static_cast<hipStream_t>(stream), tile);
    }
    if (!c || !A || !W || !C || M <= 0 || tile < 0 || (!big256 && tile >= static_cast<int>(sizeof(kBN) / sizeof(kBN[0])))) return fail(NOMAD_ERR_INVALID, "nomad_diag_gemm_bf16: bad argument");
    if (N % (big256 ? 256 : kBN[tile]) || K % 64) return fail(NOMAD_ERR_INVALID, "nomad_diag_gemm_bf16: N %% %d or K %% 64 != 0", big256 ? 256 : kBN[tile]);
    GemmParams p = dense(static_cast<const float*>(A), K, static_cast<const float*>(W), bias, static_cast<const float*>(R),
                         static_cast<float*>(C), M, N, K, gelu);
    return run_gemm_bf16(c, p, 1, static_cast<hipStream_t>(stream), tile);
}

int nomad_embed(nomad_ctx* c, const float* wav, int B, int n_samples, const float* head_w, const float* head_b,
                float* emb, float* layers_out, void* workspace, size_t workspace_bytes, nomad_stream_t stream) {
    if (!layers_out)   // the scoring forward; with layers_out it is the loss's no-gradient branch, which runs a cut encoder
        if (int rc = refuse_cut(c, "nomad_embed without layers_dev")) return rc;
    return forward_impl(c, wav, B, n_samples, head_w, head_b, emb, layers_out, workspace, workspace_bytes, stream, nullptr);
}

int nomad_workspace_bytes_ragged(const nomad_ctx* c, int B, const int* lengths_host, size_t* bytes) {
    RaggedBatch r;
    if (int rc = ragged_prologue("nomad_workspace_bytes_ragged", nullptr, c && bytes, B, 0, lengths_host, sizeof(float), 0, &r, nullptr, 0, nullptr,
                                 c ? pos_form(c) : kPosDirect))
        return rc;
    *bytes = r.lay.total;
    return 0;
}

int nomad_embed_ragged(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, const float* head_w,
                       const float* head_b, float* emb, void* workspace, size_t workspace_bytes, nomad_stream_t stream) {
    if (int rc = refuse_cut(c, "nomad_embed_ragged")) return rc;
    return forward_ragged(c, wav, B, stride, lengths_host, head_w, head_b, emb, workspace, workspace_bytes, stream);
}

// Pooled backbone features (Origw2v.forward): the forward of `precision` with head_mean_kernel as its last stage.
int nomad_embed_features(nomad_ctx* c, const float* wav, int B, int n_samples, int precision, float* feat, void* workspace,
                         size_t workspace_bytes, nomad_stream_t stream) {
    static const char who[] = "nomad_embed_features";
    if (int rc = refuse_cut(c, who)) return rc;
    switch (precision) {
        case NOMAD_PRECISION_F32:
            return forward_impl(c, wav, B, n_samples, nullptr, nullptr, feat, nullptr, workspace, workspace_bytes, stream, nullptr, who, true);
        case NOMAD_PRECISION_BF16X3:
            return forward_x3(c, wav, B, n_samples, feat, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr, who, true);
        case NOMAD_PRECISION_BF16:
            return forward_bf16(c, wav, B, n_samples, feat, workspace, workspace_bytes, stream, who, true);
    }
    return fail(NOMAD_ERR_INVALID, "%s: unknown precision %d", who, precision);
}

int nomad_embed_features_ragged(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, int precision,
                                float* feat, void* workspace, size_t workspace_bytes, nomad_stream_t stream) {
    static const char who[] = "nomad_embed_features_ragged";
    if (int rc = refuse_cut(c, who)) return rc;
    switch (precision) {
        case NOMAD_PRECISION_F32:
            return forward_ragged(c, wav, B, stride, lengths_host, nullptr, nullptr, feat, workspace, workspace_bytes, stream, who, true);
        case NOMAD_PRECISION_BF16X3:
            return forward_ragged_x3(c, wav, B, stride, lengths_host, feat, workspace, workspace_bytes, stream, who, true);
        case NOMAD_PRECISION_BF16:
            return forward_ragged_bf16(c, wav, B, stride, lengths_host, feat, workspace, workspace_bytes, stream, who, true);
    }
    return fail(NOMAD_ERR_INVALID, "%s: unknown precision %d", who, precision);
}

// Embeddings over windows of frames (scores over time): the forward of `precision` with head_windows_kernel as its last stage.
// Every argument check of that forward holds; the windows add theirs ahead of it, so nothing is queued on an error.
static int windows_args(const char* who, const nomad_ctx* c, int precision, int win, int hop, const float* head_w, const float* head_b) {
    if (int rc = refuse_cut(c, who)) return rc;
    if (win < 1 || hop < 1) return fail(NOMAD_ERR_INVALID, "%s: bad window (win=%d, hop=%d frames)", who, win, hop);
    if (!head_w != !head_b) return fail(NOMAD_ERR_INVALID, "%s: head_w_dev and head_b_dev must both be set or both be NULL", who);
    if (head_w && precision != NOMAD_PRECISION_F32)
        return fail(NOMAD_ERR_INVALID, "%s: a head override needs NOMAD_PRECISION_F32 (precision %d)", who, precision);
    return 0;
}

int nomad_num_windows(int T, int win, int hop) { return head_num_windows(T, win, hop); }

int nomad_embed_windows(nomad_ctx* c, const float* wav, int B, int n_samples, int precision, int win, int hop, const float* head_w,
                        const float* head_b, float* emb, void* workspace, size_t workspace_bytes, nomad_stream_t stream) {
    static const char who[] = "nomad_embed_windows";
    if (int rc = windows_args(who, c, precision, win, hop, head_w, head_b)) return rc;
    const HeadMode mode = HeadMode::windows(win, hop, (long long)(B > 0 ? B : 0) * head_num_windows(nomad_num_frames(n_samples), win, hop));
    switch (precision) {
        case NOMAD_PRECISION_F32:
            return forward_impl(c, wav, B, n_samples, head_w, head_b, emb, nullptr, workspace, workspace_bytes, stream, nullptr, who, mode);
        case NOMAD_PRECISION_BF16X3:
            return forward_x3(c, wav, B, n_samples, emb, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr, who, mode);
        case NOMAD_PRECISION_BF16:
            return forward_bf16(c, wav, B, n_samples, emb, workspace, workspace_bytes, stream, who, mode);
    }
    return fail(NOMAD_ERR_INVALID, "%s: unknown precision %d", who, precision);
}

int nomad_embed_windows_ragged(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, int precision, int win,
                               int hop, const float* head_w, const float* head_b, float* emb, void* workspace,
                               size_t workspace_bytes, nomad_stream_t stream) {
    static const char who[] = "nomad_embed_windows_ragged";
    if (int rc = windows_args(who, c, precision, win, hop, head_w, head_b)) return rc;
    long long n = 0;   // the kernel forms each clip's first output row from the frame prefix sums the forward uploads anyway
    for (int i = 0; lengths_host && i < B; ++i) n += head_num_windows(nomad_num_frames(lengths_host[i]), win, hop);
    const HeadMode mode = HeadMode::windows(win, hop, n);
    switch (precision) {
        case NOMAD_PRECISION_F32:
            return forward_ragged(c, wav, B, stride, lengths_host, head_w, head_b, emb, workspace, workspace_bytes, stream, who, mode);
        case NOMAD_PRECISION_BF16X3:
            return forward_ragged_x3(c, wav, B, stride, lengths_host, emb, workspace, workspace_bytes, stream, who, mode);
        case NOMAD_PRECISION_BF16:
            return forward_ragged_bf16(c, wav, B, stride, lengths_host, emb, workspace, workspace_bytes, stream, who, mode);
    }
    return fail(NOMAD_ERR_INVALID, "%s: unknown precision %d", who, precision);
}

int nomad_saved_bytes(const nomad_ctx* c, int B, int n_samples, size_t* bytes) {
    Shapes sh;
    if (!c || !bytes || B <= 0 || !make_shapes(B, n_samples, &sh))
        return fail(NOMAD_ERR_INVALID, "nomad_saved_bytes: bad shape B=%d N=%d", B, n_samples);
    *bytes = make_saved(geom_uniform(sh), nullptr).total;
    return 0;
}

int nomad_backward_workspace_bytes(const nomad_ctx* c, int B, int n_samples, size_t* bytes) {
    Shapes sh;
    if (!c || !bytes || B <= 0 || !make_shapes(B, n_samples, &sh))
        return fail(NOMAD_ERR_INVALID, "nomad_backward_workspace_bytes: bad shape B=%d N=%d", B, n_samples);
    *bytes = make_bwd_layout(geom_uniform(sh)).total;
    return 0;
}

int nomad_embed_train(nomad_ctx* c, const float* wav, int B, int n_samples, const float* head_w, const float* head_b,
                      float* emb, float* layers_out, void* saved, size_t saved_bytes, void* workspace,
                      size_t workspace_bytes, nomad_stream_t stream) {
    Shapes sh;
    if (!c || !saved || !layers_out || B <= 0 || !make_shapes(B, n_samples, &sh))
        return fail(NOMAD_ERR_INVALID, "nomad_embed_train: bad argument");
    const Saved sv = make_saved(geom_uniform(sh), saved);
    if (saved_bytes < sv.total)
        return fail(NOMAD_ERR_WORKSPACE, "nomad_embed_train: saved block %zu < required %zu", saved_bytes, sv.total);
    return forward_impl(c, wav, B, n_samples, head_w, head_b, emb, layers_out, workspace, workspace_bytes, stream, &sv);
}

static int ragged_geom_for_size(const char* who, const nomad_ctx* c, int B, const int* lens, size_t* bytes, RaggedShapes* rs) {
    if (!c || !bytes || !lens || B <= 0 || !make_ragged(B, lens, rs)) return fail(NOMAD_ERR_INVALID, "%s: bad argument (B=%d)", who, B);
    return 0;
}

int nomad_ragged_metadata(int B, const int* lengths_host, int* out_host, size_t capacity, size_t* count) {
    RaggedShapes rs;
    if (!count || !lengths_host || B <= 0 || !make_ragged(B, lengths_host, &rs))
        return fail(NOMAD_ERR_INVALID, "nomad_ragged_metadata: bad argument (B=%d)", B);
    *count = rs.meta.size();
    if (out_host) {
        if (capacity < rs.meta.size()) return fail(NOMAD_ERR_WORKSPACE, "nomad_ragged_metadata: room for %zu ints < %zu", capacity, rs.meta.size());
        std::copy(rs.meta.begin(), rs.meta.end(), out_host);
    }
    return 0;
}

int nomad_saved_bytes_ragged(const nomad_ctx* c, int B, const int* lengths_host, size_t* bytes) {
    RaggedShapes rs;
    if (int rc = ragged_geom_for_size("nomad_saved_bytes_ragged", c, B, lengths_host, bytes, &rs)) return rc;
    *bytes = make_saved(geom_ragged(rs, 0, nullptr), nullptr).total;
    return 0;
}

int nomad_backward_workspace_bytes_ragged(const nomad_ctx* c, int B, const int* lengths_host, size_t* bytes) {
    RaggedShapes rs;
    if (int rc = ragged_geom_for_size("nomad_backward_workspace_bytes_ragged", c, B, lengths_host, bytes, &rs)) return rc;
    *bytes = make_bwd_layout(geom_ragged(rs, 0, nullptr)).total;
    return 0;
}

int nomad_train_workspace_bytes_ragged(const nomad_ctx* c, int B, const int* lengths_host, size_t* bytes) {
    RaggedShapes rs;
    if (int rc = ragged_geom_for_size("nomad_train_workspace_bytes_ragged", c, B, lengths_host, bytes, &rs)) return rc;
    *bytes = make_bwd_layout(geom_ragged(rs, 0, nullptr), true, false).total;
    return 0;
}

int nomad_embed_train_ragged(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, const float* head_w,
                             const float* head_b, float* emb, float* layers_out, void* saved, size_t saved_bytes, void* workspace,
                             size_t workspace_bytes, nomad_stream_t stream) {
    if (!c || !layers_out || (saved == nullptr) != (saved_bytes == 0))
        return fail(NOMAD_ERR_INVALID, "nomad_embed_train_ragged: bad argument");
    if (saved && c->train_ready && c->train_convnet)
        return fail(NOMAD_ERR_INVALID,
                    "nomad_embed_train_ragged: a trainable conv feature extractor (nomad_train_set_convnet) needs an equal-length batch");
    return forward_ragged(c, wav, B, stride, lengths_host, head_w, head_b, emb, workspace, workspace_bytes, stream,
                          "nomad_embed_train_ragged", false, layers_out, saved, saved_bytes);
}

int nomad_enable_backward(nomad_ctx* c) {
    if (!c) return fail(NOMAD_ERR_INVALID, "null ctx");
    if (c->bwd_ready) return 0;
    HIP_TRY(hipSetDevice(c->device));
    static const char who[] = "nomad_enable_backward";
    int rc;
    for (int i = 1; i <= 4; ++i) {
        if ((rc = dev_alloc(c, who, (size_t)512 * 1024, &c->conv_bw_even[i]))) return rc;
        if ((rc = dev_alloc(c, who, (size_t)512 * 512, &c->conv_bw_odd[i]))) return rc;
    }
    for (int i = 5; i <= 6; ++i)
        if ((rc = dev_alloc(c, who, (size_t)1024 * 512, &c->conv_bw2[i]))) return rc;
    if ((rc = dev_alloc(c, who, (size_t)16 * 64 * 6144, &c->pos_wb))) return rc;
    if ((rc = for_each_gemm_weight(c, [&](const GemmWeight& g) { return g.wT ? dev_alloc(c, who, (size_t)g.N * g.K, g.wT) : 0; }))) return rc;
    build_backward_weights(c, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = dev_alloc(c, who, kSplitKPartFloats, &c->splitk_part))) return rc;
    c->bwd_ready = true;
    return 0;
}

}  // extern "C"

static int l1_backward_rows(const char* who, nomad_ctx* c, const float* a_layers, const float* b_layers, const float* a_emb,
                            const float* b_emb, long long rows, int B, const float* upstream, float* dlayers, float* demb,
                            nomad_stream_t stream) {
    if (!c || !a_layers || !b_layers || !a_emb || !b_emb || !upstream || !dlayers || !demb || B <= 0 || rows < B)
        return fail(NOMAD_ERR_INVALID, "%s: bad argument", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long per_layer = rows * 768;
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(l1_bwd_kernel, dim3(2048), dim3(256), 0, s, reinterpret_cast<const float4*>(a_layers),
                       reinterpret_cast<const float4*>(b_layers), per_layer * 12 / 4, 1.0f / (float)per_layer, upstream,
                       reinterpret_cast<float4*>(dlayers));
    hipLaunchKernelGGL(l1_bwd_kernel, dim3(64), dim3(256), 0, s, reinterpret_cast<const float4*>(a_emb),
                       reinterpret_cast<const float4*>(b_emb), (long long)B * 64, 1.0f / (float)(B * 256), upstream,
                       reinterpret_cast<float4*>(demb));
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

int nomad_l1_loss_backward(nomad_ctx* c, const float* a_layers, const float* b_layers, const float* a_emb,
                           const float* b_emb, int B, int T, const float* upstream, float* dlayers, float* demb,
                           nomad_stream_t stream) {
    return l1_backward_rows("nomad_l1_loss_backward", c, a_layers, b_layers, a_emb, b_emb, T > 0 ? (long long)B * T : 0, B, upstream,
                            dlayers, demb, stream);
}

int nomad_l1_loss_backward_ragged(nomad_ctx* c, const float* a_layers, const float* b_layers, const float* a_emb,
                                  const float* b_emb, long long M, int B, const float* upstream, float* dlayers, float* demb,
                                  nomad_stream_t stream) {
    return l1_backward_rows("nomad_l1_loss_backward_ragged", c, a_layers, b_layers, a_emb, b_emb, M, B, upstream, dlayers, demb, stream);
}

}  // extern "C"

// dW[Nout][Kin] += scale * dY^T X from the transposed operands TA = dY^T [Nout][Mp], TB = X^T [Kin][Mp]: the forward's
// GEMM kernel with the contraction split over `S` groups, partial products folded in fixed order.
static int dw_gemm(nomad_ctx* c, const float* TA, const float* TB, int Nout, int Kin, int Mp, float* part, float* out,
                   int rows_scaled, float scale, hipStream_t s) {
    // 128x64 tiles; enough splits for ~1500 workgroups (measured on the training shapes: 512 -> 1536 workgroups
    // is 4 % of a step, beyond that nothing)
    // (bf16x3 products, nomad_set_gemm_precision: 128x128 tiles of four 64x64 wave tiles - 12 MFMAs per 4 fragment splits)
    const bool wide = c->gemm_x3 && Kin % 128 == 0;
    const int tile = wide ? 20 : 34;
    const int tiles = (Nout / 128) * (Kin / (wide ? 128 : 64));
    int S = 1;
    while (S < 16 && tiles * S < 1536 && (size_t)(2 * S) * Nout * Kin <= kSplitPartFloats) S *= 2;
    if ((size_t)S * Nout * Kin > kSplitPartFloats) return fail(NOMAD_ERR_INVALID, "dw_gemm: partial buffer too small");
    const int Kc = Mp / S;
    GemmParams p = dense(TA, Mp, TB, nullptr, nullptr, part, Nout, Kin, Kc, 0);
    p.ldw = Mp;
    p.a_goff = Kc;
    p.w_goff = Kc;
    p.c_goff = (long long)Nout * Kin;
    int rc;
    if ((rc = gemm_f32_dispatch(c, p, S, tile, s))) return rc;   // (its own split over the groups: never run_gemm's)
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    const long long n4 = (long long)Nout * Kin / 4, n4s = (long long)rows_scaled * Kin / 4;
    const float4* p4 = reinterpret_cast<const float4*>(part);
    float4* o4 = reinterpret_cast<float4*>(out);
    if (n4s > 0)  // leading rows with their own scale (q rows of the fused q/k/v weight); every partial keeps stride n4
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((n4s + 255) / 256)), dim3(256), 0, s, p4, S, n4, n4s, o4, scale);
    if (n4 > n4s) {
        // rows after the scaled block: same partial stride, shifted start
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((n4 - n4s + 255) / 256)), dim3(256), 0, s, p4 + n4s, S, n4,
                           n4 - n4s, o4 + n4s, 1.0f);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The backward sequence, over an equal-length or a ragged batch (the geometry of the forward it belongs to): one sequence serves
// both, the way forward_run does.  Ragged: per-frame tensors are packed, the padded dU buffers of the conv stack hold clip c's
// L_i(c) + 2 rows at row upref_i[c], the kernels that care about clip boundaries read the prefix sums; small-M GEMMs never split
// K (a clip's gradient does not depend on its batch).  The conv feature extractor's parameter gradients need an equal-length batch.
// wb (nomad_embed_windows_backward*, nomad_embed_spans_backward_ragged): demb holds one row per WINDOW, or per ROW of the span
// table, and the head stage is the rows head's backward - head_rows_bwd_kernel and the windows' or the spans' scatter (head.hip.h)
// through the gw block in the caller's scratch - instead of head_bwd_kernel; everything below gx is unchanged.
static int backward_run(nomad_ctx* c, const float* wav, const BatchGeom& g, const Saved& sv, const BwdLayout& lay, const float* head_w,
                        const float* head_b, const float* layers_out, const float* dlayers, const float* demb, float* dwav,
                        char* ws, hipStream_t s, bool train, const HeadRows* wb = nullptr) {
    const bool conv_pg = train && c->train_convnet;  // parameter gradients of the conv feature extractor too
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const int B = g.B, T = g.T, M = (int)g.rows[6], n_samples = g.wav_ld;
    const bool rg = g.ragged();
    const int* const tpref = g.pref[6];   // kNoInts for an equal-length batch
    // d loss / d waveform of Nomad.forward(): small-M GEMMs may split K, into the context's block
    const SplitKPlan splitk = train || c->train_ready || rg ? SplitKPlan{} : SplitKPlan{c->splitk_part, kSplitKPartFloats};
    float *gx = F(lay.gx), *dya = F(lay.dya), *dyb = F(lay.dyb), *dh = F(lay.dh), *dqkv = F(lay.dqkv);
    int rc;
    // the regularisation of the forward this backward belongs to (the caller re-sets it: nomad_train_set_stochastic)
    const DropCfg d_in = make_drop(c, train ? c->p_input : 0.f), d_res = make_drop(c, train ? c->p_drop : 0.f),
                  d_att = make_drop(c, train ? c->p_attn : 0.f);
    int nbr = 1;  // LayerDrop masks: one for the call, or one per branch of a merged batch (see forward_run)
    unsigned bmask[4] = {train ? c->layer_mask : 0xFFFu, 0xFFFu, 0xFFFu, 0xFFFu};
    if (train && c->branches > 1) {
        if (B % c->branches) return fail(NOMAD_ERR_INVALID, "nomad_train_backward: B=%d is not %d equal branches", B, c->branches);
        nbr = c->branches;
        for (int i = 0; i < nbr; ++i) bmask[i] = c->branch_mask[i];
    }
    const long long act = (long long)M * 768;
    float* dmask = train ? F(lay.dmask) : nullptr;

    // ---- parameter-gradient helpers (train only); Ms rows of the (sub-)batch, Mps = Ms rounded up to 512 ------
    const ParamOffsets& po = param_offsets();
    auto G = [&](size_t off) { return c->grad + off; };
    float *TA = train ? F(lay.ta) : nullptr, *TB = train ? F(lay.tb) : nullptr, *part = train ? F(lay.kpart) : nullptr;
    auto tpose = [&](const float* in, int C, float* out, bool gelu, int Ms, int Mps) {  // out[C][Mps] = f(in[Ms][C])^T, zero padded
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        const dim3 grid(Mps / 64, (C + 63) / 64), blk(256);
        if (gelu) hipLaunchKernelGGL(transpose_pad_kernel<1>, grid, blk, 0, s, in, C, out, Mps, Ms, C);
        else hipLaunchKernelGGL(transpose_pad_kernel<0>, grid, blk, 0, s, in, C, out, Mps, Ms, C);
    };
    auto rowsum = [&](const float* in, int rows, float* out, float scale, int Mps) {  // bias gradient from dY^T
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        hipLaunchKernelGGL(rowsum_acc_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, in, Mps, rows, out, scale);
    };
    auto ln_params = [&](const float* x, const float* g, const float* g2, int N, float* dgam, float* dbet, int Ms) {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        float* lp = F(lay.lnpart);
        const int nblk = (Ms + kLnRows - 1) / kLnRows;
        if (N == 768) hipLaunchKernelGGL(ln_param_partial_kernel<3>, dim3(nblk), dim3(256), 0, s, x, g, g2, lp, Ms);
        else hipLaunchKernelGGL(ln_param_partial_kernel<2>, dim3(nblk), dim3(256), 0, s, x, g, g2, lp, Ms);
        hipLaunchKernelGGL(ln_param_final_kernel, dim3(2 * N / 64), dim3(256), 0, s, lp, nblk, N, dgam, dbet);
    };

    // parameter gradients of the ENCODER (pos-conv, encoder LayerNorm, the 12 layers): not with freeze_all, where only
    // post_extract_proj, the feature LayerNorm and the head stay trainable (train_triplet.py:76-79)
    const bool pg = train && !c->freeze_encoder;
    // nomad_set_encoder_depth: the forward stopped behind layer depth - 1.  No head; the gradient that enters that layer is
    // dlayers[depth - 1] alone, so its LayerNorm backward reads it in gx's place (first_cut) - what the uncut run computes from a gx
    // of exact zeros plus that row.  Rows >= depth of dlayers and demb are not read.
    const int depth = train ? NOMAD_NUM_LAYERS : c->encoder_depth;
    bool first_cut = depth < NOMAD_NUM_LAYERS;
    // ---- head -> d loss / d x_12 -------------------------------------------------------------------
    if (!first_cut && wb) {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        const float* x12 = layers_out + (size_t)11 * M * 768;
        const dim3 per_frame((g.max_t + 3) / 4, B);
        auto stage1 = [&](auto rows, dim3 grid) {
            hipLaunchKernelGGL(head_rows_bwd_kernel<decltype(rows)>, grid, dim3(1024), 0, s, x12, rows, head_w ? head_w : c->emb_w,
                               head_b ? head_b : c->emb_b, demb, wb->gw);
            if constexpr (std::is_same_v<decltype(rows), SpanRows>)
                hipLaunchKernelGGL(head_spans_scatter_kernel, per_frame, dim3(256), 0, s, wb->gw, rows, gx);
            else hipLaunchKernelGGL(head_windows_scatter_kernel, per_frame, dim3(256), 0, s, wb->gw, rows, gx);
        };
        if ((rc = head_rows_launch("backward_run", *wb, B, T, g.max_t, tpref, stage1))) return rc;
    } else if (!first_cut) {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        hipLaunchKernelGGL(head_bwd_kernel, dim3(B), dim3(1024), 0, s, layers_out + (size_t)11 * M * 768, T,
                           head_w ? head_w : c->emb_w, head_b ? head_b : c->emb_b, demb, gx,
                           train ? F(lay.headp) : nullptr, train ? F(lay.headdz) : nullptr, tpref);
        if (train)
            hipLaunchKernelGGL(head_param_grad_kernel, dim3(256), dim3(256), 0, s, F(lay.headp), F(lay.headdz), B,
                               G(po.emb_w), G(po.emb_b));
    }
    // ---- 12 transformer layers, last to first ---------------------------------------------------------
    // One layer over clips [c0, c0 + nc): the whole batch, or one branch when LayerDrop split the branches.
    bool lnb_prefused = false;   // the LayerNorm backward at the head of the next bwd_layer call (or the encoder's) ran inside the last GEMM's epilogue
    bool whole_batch = true;     // every layer runs for every clip (no LayerDrop branch skips one)
    for (int l = 0; l < NOMAD_NUM_LAYERS; ++l)
        for (int br = 0; br < nbr; ++br) whole_batch = whole_batch && ((bmask[br] >> l) & 1u);
    auto bwd_layer = [&](int l, int c0, int nc) -> int {
        const LayerDev& d = c->layers[l];
        const LayerOffsets& lo = po.L[l];
        const long long r0 = g.clip_row0(c0);   // (a ragged batch: the clips' prefix sums)
        const int Ms = (int)(g.clip_row0(c0 + nc) - r0), Mps = (Ms + 511) / 512 * 512;
        const long long acts = (long long)Ms * 768;
        const unsigned long long idx0 = (unsigned long long)r0 * 768;
        const SavedLayer& sl0 = sv.L[l];
        const float *y2 = sl0.y2 + r0 * 768, *y1 = sl0.y1 + r0 * 768, *u = sl0.u + r0 * 3072, *qkv = sl0.qkv + r0 * 2304,
                    *ctx = sl0.ctx + r0 * 768, *lse = sl0.lse + 12 * r0;
        float *gxs = gx + r0 * 768, *dyas = dya + r0 * 768, *dybs = dyb + r0 * 768, *dhs = dh + r0 * 3072,
              *dqkvs = dqkv + r0 * 2304, *dmasks = dmask ? dmask + r0 * 768 : nullptr;
        const float* dl = dlayers ? dlayers + (size_t)l * M * 768 + r0 * 768 : nullptr;
        int rc;
        if (first_cut) {
            if ((rc = run_ln_bwd(c, y2, dl, nullptr, d.ln2_w, dyas, Ms, 768, s))) return rc;
        } else if (!lnb_prefused && (rc = run_ln_bwd(c, y2, gxs, dl, d.ln2_w, dyas, Ms, 768, s))) return rc;   // dy2 (prefused: by the layer above's last GEMM)
        first_cut = false;
        lnb_prefused = false;
        // dy2 feeds the residual as is and the fc2 branch through its dropout mask
        const float* dy2b = dyas;
        if (d_res.threshold) {
            if ((rc = run_dropout(c, dyas, nullptr, dmasks, acts, d_res, site_ffn(l), s, idx0))) return rc;
            dy2b = dmasks;
        }
        if (pg) {
            ln_params(y2, gxs, dl, 768, G(lo.ln2_w), G(lo.ln2_b), Ms);
            tpose(dy2b, 768, TA, false, Ms, Mps);
            rowsum(TA, 768, G(lo.fc2_b), 1.0f, Mps);
            tpose(u, 3072, TB, true, Ms, Mps);  // h = gelu(u), recomputed
            if ((rc = dw_gemm(c, TA, TB, 768, 3072, Mps, part, G(lo.fc2_w), 0, 1.0f, s))) return rc;
        }
        if ((rc = bwd_gemm(c, dy2b, c->fc2_wT[l], dhs, Ms, 3072, 768, u, nullptr, s, splitk))) return rc;      // du = (dy2 W2) * gelu'(u)
        if (pg) {
            tpose(dhs, 3072, TA, false, Ms, Mps);
            rowsum(TA, 3072, G(lo.fc1_b), 1.0f, Mps);
            // fc1's input = LayerNorm(y1), recomputed into gx (the upstream gradient it held has been consumed)
            if ((rc = run_layernorm(c, y1, d.ln1_w, d.ln1_b, gxs, nullptr, Ms, 768, s))) return rc;
            tpose(gxs, 768, TB, false, Ms, Mps);
            if ((rc = dw_gemm(c, TA, TB, 3072, 768, Mps, part, G(lo.fc1_w), 0, 1.0f, s))) return rc;
        }
        // (dX-only backward: when the GEMM splits K, the LayerNorm backward forms dx1 from the partial products itself)
        const SplitKFusion ln1_bwd = SplitKFusion::ln_bwd(y1, nullptr, d.ln1_w, dyas);
        bool ln1_done = false;
        if ((rc = bwd_gemm(c, dhs, c->fc1_wT[l], dybs, Ms, 768, 3072, nullptr, dyas, s, splitk, train ? nullptr : &ln1_bwd, &ln1_done)))
            return rc;                                                                                 // dx1 = du W1 + dy2
        if (!ln1_done && (rc = run_ln_bwd(c, y1, dybs, nullptr, d.ln1_w, dyas, Ms, 768, s))) return rc;   // dy1
        if (pg) ln_params(y1, dybs, nullptr, 768, G(lo.ln1_w), G(lo.ln1_b), Ms);
        const float* dy1b = dyas;  // dy1 through out_proj's dropout mask
        if (d_res.threshold) {
            if ((rc = run_dropout(c, dyas, nullptr, dmasks, acts, d_res, site_proj(l), s, idx0))) return rc;
            dy1b = dmasks;
        }
        if (pg) {
            tpose(dy1b, 768, TA, false, Ms, Mps);
            rowsum(TA, 768, G(lo.o_b), 1.0f, Mps);
            tpose(ctx, 768, TB, false, Ms, Mps);
            if ((rc = dw_gemm(c, TA, TB, 768, 768, Mps, part, G(lo.o_w), 0, 1.0f, s))) return rc;
        }
        if ((rc = bwd_gemm(c, dy1b, c->o_wT[l], dybs, Ms, 768, 768, nullptr, nullptr, s, splitk))) return rc;  // dctx
        if (rg) {   // the whole batch's pointers and prefix sums, clips [c0, c0 + nc); fused or three kernels by each CLIP's length
            Scope sc(c, s, NOMAD_K_ATTN, 3.5 * g.attn_flops * nc / B);
            HIP_TRY(launch_attention_bwd_ragged(sl0.qkv, sl0.ctx, dyb, sl0.lse, F(lay.attnd), dqkv, tpref, B, c0, nc, (int)r0, (int)r0 + Ms,
                                                g.max_t, g.min_t, d_att, site_attn(l), s, !c->tune.attn_bwd_small));
        } else {
            Scope sc(c, s, NOMAD_K_ATTN, 14.0 * nc * 12.0 * (double)T * T * 64);  // 7 T x T x 64 products (S, dP twice)
            HIP_TRY(launch_attention_bwd(qkv, ctx, dybs, lse, F(lay.attnd), dqkvs, nc, T, d_att, site_attn(l), s, c0 * 12, !c->tune.attn_bwd_small));
        }
        if (pg) {
            // the forward's fused weight holds q scaled by head_dim^-0.5: d q_proj = 0.125 * d fused rows 0..767
            tpose(dqkvs, 2304, TA, false, Ms, Mps);
            rowsum(TA, 768, G(lo.qkv_b), 0.125f, Mps);
            rowsum(TA + (size_t)768 * Mps, 1536, G(lo.qkv_b) + 768, 1.0f, Mps);
            const float* xin = layers_out + (size_t)(l > 0 ? l - 1 : 0) * M * 768 + r0 * 768;
            if (l == 0) {  // layer 0 reads dropout(LayerNorm(y0)): recomputed into dyb (dctx has been consumed)
                if ((rc = run_layernorm(c, sv.y0 + r0 * 768, c->eln_w, c->eln_b, dybs, nullptr, Ms, 768, s))) return rc;
                if (d_res.threshold && (rc = run_dropout(c, dybs, nullptr, dybs, acts, d_res, kSiteEncoder, s, idx0))) return rc;
                xin = dybs;
            }
            tpose(xin, 768, TB, false, Ms, Mps);
            if ((rc = dw_gemm(c, TA, TB, 2304, 768, Mps, part, G(lo.qkv_w), 768, 0.125f, s))) return rc;
        }
        // dx_in = dqkv Wqkv + dy1; what follows it is the LayerNorm backward of the layer below (its LN2, with that layer's output gradient) or
        // of the encoder's LayerNorm: fused into the split-K epilogue where the whole batch walks the layers together (no LayerDrop)
        const SplitKFusion below = l > 0 ? SplitKFusion::ln_bwd(sv.L[l - 1].y2, dlayers ? dlayers + (size_t)(l - 1) * M * 768 : nullptr,
                                                                c->layers[l - 1].ln2_w, dya)
                                         : SplitKFusion::ln_bwd(sv.y0, nullptr, c->eln_w, dya);
        const bool offer = !train && whole_batch && !d_res.threshold;
        return bwd_gemm(c, dqkvs, c->qkv_wT[l], gxs, Ms, 768, 2304, nullptr, dyas, s, splitk, offer ? &below : nullptr, &lnb_prefused);
    };
    for (int l = depth - 1; l >= 0; --l) {
        unsigned all = 1u;
        for (int br = 0; br < nbr; ++br) all &= (bmask[br] >> l) & 1u;
        if (all) {
            if ((rc = bwd_layer(l, 0, B))) return rc;
            continue;
        }
        for (int br = 0; br < nbr; ++br)  // LayerDrop: identity in the forward, identity here, per branch
            if ((bmask[br] >> l) & 1u)
                if ((rc = bwd_layer(l, br * (B / nbr), B / nbr))) return rc;
    }
    const int Mp = lay.Mp;
    // ---- encoder input: LayerNorm, x + gelu(pos_conv(x)) --------------------------------------------
    if (d_res.threshold && (rc = run_dropout(c, gx, nullptr, gx, act, d_res, kSiteEncoder, s))) return rc;
    if (!lnb_prefused && (rc = run_ln_bwd(c, sv.y0, gx, nullptr, c->eln_w, dya, M, 768, s))) return rc;   // dy0
    if (pg) ln_params(sv.y0, gx, nullptr, 768, G(po.eln_w), G(po.eln_b), M);
    const long long grp_stride = g.grp_stride;
    {
        float* dug = F(lay.dug);
        {
            Scope sc(c, s, NOMAD_K_ROW, 0.0);
            hipLaunchKernelGGL(zero_pad_rows_kernel<float>, dim3(16 * B), dim3(256), 0, s, dug, T, tpref, g.ppref, B);
            hipLaunchKernelGGL(dgelu_to_groups_kernel, dim3(M), dim3(192), 0, s, dya, sv.upc, dug, T, grp_stride, tpref, g.ppref, B);
        }
        GemmParams p{};
        p.A = dug;
        p.amap = g.pos_amap;  // row (clip, t) starts at buffer frame t + 1
        p.amap.off = 48;
        p.a_goff = grp_stride;
        p.K = 6144;
        p.kchunk = 6144;
        p.W = c->pos_wb;
        p.ldw = 6144;
        p.w_goff = 64LL * 6144;
        p.C = dyb;
        p.cmap = plain_map(M, 768);
        p.c_goff = 48;
        p.R = dya;
        p.rmap = plain_map(M, 768);
        p.r_goff = 48;
        p.M = M;
        p.N = 64;
        p.n_valid = 48;
        if ((rc = run_gemm(c, p, 16, 48, s, splitk))) return rc;  // one instantiation for every batch size: same summation order
    }
    if (train) {
        float *dug = F(lay.dug), *xg = F(lay.xg), *dwe = F(lay.dwe), *featln = F(lay.f2);
        // post_extract_proj's input (LayerNorm of the extractor output) is recomputed, not saved
        if ((rc = run_layernorm(c, sv.c6, c->fln_w, c->fln_b, featln, nullptr, M, 512, s))) return rc;
        if (pg) {
        // ---- pos-conv parameters: bias, then weight_g / weight_v through the weight norm --------------------
        {
            Scope sc(c, s, NOMAD_K_ROW, 0.0);
            hipLaunchKernelGGL(posconv_bias_partial_kernel, dim3(kPbChunks, 16), dim3(256), 0, s, dug, g.pad_rows, F(lay.lnpart));
            hipLaunchKernelGGL(posconv_bias_final_kernel, dim3(1), dim3(768), 0, s, F(lay.lnpart), G(po.pos_b));
        }
        // the conv's input (post_extract_proj output, group-major, zero padded) is recomputed, not saved
        {
            Scope sc(c, s, NOMAD_K_ROW, 0.0);
            hipLaunchKernelGGL(zero_pad_rows_kernel<float>, dim3(16 * B), dim3(256), 0, s, xg, T, tpref, g.ppref, B);
        }
        {
            GemmParams p = dense(featln, 512, c->proj_w, c->proj_b, nullptr, xg, M, 768, 512, 0);
            p.cmap = g.pad_map;
            p.c_colblk = 48;
            p.c_colblk_stride = grp_stride;
            if ((rc = gemm_f32_dispatch(c, p, 1, pick_tile(c, M, 768, 512), s))) return rc;   // (fine-tuning only)
        }
        if (d_in.threshold) {
            Scope sc(c, s, NOMAD_K_ROW, 0.0);
            hipLaunchKernelGGL(dropout_groups_kernel, dim3(M), dim3(192), 0, s, xg, T, grp_stride, d_in, kSiteInput, tpref, g.ppref, B);
        }
        {
            const int S = lay.pos_split, cps = (B + S - 1) / S;
            Scope sc(c, s, NOMAD_K_GEMM, 2.0 * M * 768.0 * 48 * 128);
            hipLaunchKernelGGL(posconv_dw_kernel, dim3(128 / kPdwTaps, 16, S), dim3(256), 0, s, dug, xg, part, B, T, cps, tpref, g.ppref, grp_stride);
            hipLaunchKernelGGL(posconv_dw_gather_kernel, dim3(768), dim3(256), 0, s, part, S, dwe);
            hipLaunchKernelGGL(tap_dot_partial_kernel, dim3(576), dim3(256), 0, s, dwe, c->theta + po.pos_v, c->tap_partial);
            hipLaunchKernelGGL(tap_sum_final_kernel, dim3(1), dim3(1024), 0, s, c->tap_partial, 576, c->tap_dot);
            hipLaunchKernelGGL(posconv_wn_bwd_kernel, dim3(768 * 48 * 128 / 256), dim3(256), 0, s, dwe, c->theta + po.pos_v,
                               c->theta + po.pos_g, c->pos_nrm2, c->tap_dot, G(po.pos_v), G(po.pos_g));
        }
        }
        // ---- post_extract_proj parameters (its output went through dropout_input) ------------------------
        if (d_in.threshold && (rc = run_dropout(c, dyb, nullptr, dyb, act, d_in, kSiteInput, s))) return rc;
        tpose(dyb, 768, TA, false, M, Mp);
        rowsum(TA, 768, G(po.proj_b), 1.0f, Mp);
        tpose(featln, 512, TB, false, M, Mp);
        if ((rc = dw_gemm(c, TA, TB, 768, 512, Mp, part, G(po.proj_w), 0, 1.0f, s))) return rc;
    }
    // ---- post_extract_proj, LayerNorm(512), GELU of conv6 ----------------------------------------------
    if ((rc = bwd_gemm(c, dyb, c->proj_wT, F(lay.f1), M, 512, 768, nullptr, nullptr, s, splitk))) return rc;
    if (train) ln_params(sv.c6, F(lay.f1), nullptr, 512, G(po.fln_w), G(po.fln_b), M);
    HIP_TRY(hipGetLastError());
    if (!dwav && !conv_pg) return 0;  // frozen conv feature extractor (freeze_convnet: True): nothing upstream needs a gradient
    if (c->feature_grad_mult == 0.f) {  // fairseq runs the extractor under no_grad then: no gradient reaches it or the waveform
        if (dwav) HIP_TRY(hipMemsetAsync(dwav, 0, sizeof(float) * (size_t)B * n_samples, s));
        return 0;
    }
    // d W_i of conv layer i (freeze_convnet: False): dU_i^T x im2col(input)^T contracted over all frames, per-clip column
    // blocks of conv_lp(L_i) (zero padded), the same split-K dW GEMM as the encoder's, then back to [co][ci][tap]
    auto conv_dw = [&](int i, const float* dU, const float* in, long long in_clip, bool gelu_in) -> int {
        const int Lout = g.L[i], taps = kConvK[i], Kin = taps * 512;   // (equal-length batches only)
        const int Lp = (int)conv_lp(Lout);
        const long long cols = (long long)B * Lp;
        {
            Scope sc(c, s, NOMAD_K_ROW, 0.0);
            hipLaunchKernelGGL(transpose_clips_kernel<0>, dim3(Lp / 64, 8, B), dim3(256), 0, s, dU + 512, (long long)(Lout + 2) * 512, 512,
                               TA, cols, Lp, Lout, 512);
            const dim3 grid(Lp / 64, Kin / 64, B);
            if (gelu_in)
                hipLaunchKernelGGL(transpose_clips_kernel<1>, grid, dim3(256), 0, s, in, in_clip, kConvS[i] * 512, TB, cols, Lp, Lout, Kin);
            else
                hipLaunchKernelGGL(transpose_clips_kernel<0>, grid, dim3(256), 0, s, in, in_clip, kConvS[i] * 512, TB, cols, Lp, Lout, Kin);
        }
        float* tmp = F(lay.convtmp);
        HIP_TRY(hipMemsetAsync(tmp, 0, sizeof(float) * 512 * (size_t)Kin, s));
        int rc2;
        if ((rc2 = dw_gemm(c, TA, TB, 512, Kin, (int)cols, part, tmp, 0, 1.0f, s))) return rc2;
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        const long long n = 512LL * Kin;
        hipLaunchKernelGGL(conv_grad_permute_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tmp, G(po.conv_w[i]), taps);
        return 0;
    };
    if ((rc = run_ln_bwd(c, sv.c6, F(lay.f1), nullptr, c->fln_w, F(lay.f2), M, 512, s))) return rc;
    float* bufs[2] = {F(lay.bufa), F(lay.bufb)};  // dU6 -> a, dU5 -> b, ..., dU1 -> b, G0 -> a
    {
        HIP_TRY(hipMemsetAsync(bufs[0], 0, sizeof(float) * 512 * (size_t)(M + 2LL * B), s));
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        const RowMap om = rg ? RowMap{512, 0, 0, 512, tpref, g.upref[6], B, 512} : RowMap{512, (long long)(T + 2) * 512, T, 512};
        // GradMultiply(features, feature_grad_mult) sits on the extractor's (post-GELU) output: its backward scales the
        // gradient that enters GELU'
        hipLaunchKernelGGL(dgelu_rows512_kernel, dim3(M), dim3(128), 0, s, F(lay.f2), sv.u[6], bufs[0], om, M,
                           c->feature_grad_mult);
    }
    // ---- conv6..conv1: transposed strided convolutions as GEMMs over the padded dU buffers -------------
    for (int i = 6; i >= 1; --i) {
        const float* dU = bufs[i % 2];        // [B][L_i + 2][512], data at rows 1..L_i (ragged: clip c's L_i(c) + 2 rows at row upref_i[c])
        float* out = bufs[(i + 1) % 2];
        const int Lout = g.L[i], Lin = g.L[i - 1];   // (0 for a ragged batch: the maps below read the prefix sums)
        const bool to_g0 = (i == 1);          // conv0's output gradient is compact and gets no GELU' here
        const long long out_clip = to_g0 ? (long long)Lin * 512 : (long long)(Lin + 2) * 512;
        const long long out_off = to_g0 ? 0 : 512;
        const int* const obase = to_g0 ? g.pref[0] : g.upref[i - 1];   // ragged: the clips' first rows in `out`
        // logical rows by `pref` (ragged) or `rows` per clip: the A rows in dU, the C rows in out, the GELU' rows in the saved u
        auto amap_of = [&](long long off, int rows, const int* pref) {
            return rg ? RowMap{off, 0, 0, 512, pref, g.upref[i], B, 512} : RowMap{off, (long long)(Lout + 2) * 512, rows, 512};
        };
        auto cmap_of = [&](long long off, int rows, const int* pref) {
            return rg ? RowMap{off, 0, 0, 1024, pref, obase, B, 512} : RowMap{off, out_clip, rows, 1024};
        };
        auto dgmap_of = [&](long long off, int rows, const int* pref) {
            return rg ? RowMap{off, 0, 0, 1024, pref, g.pref[i - 1], B, 512} : RowMap{off, (long long)Lin * 512, rows, 1024};
        };
        // the two GEMMs below write frames 0 .. covered - 1 of every clip (k = 3: every input frame; k = 2: 2 L_out of them); what they
        // do not write is zeroed here: the two pad rows of a padded buffer and the frames behind the last window (a full memset of
        // the buffer cost 20-40 us per layer at configs[3]'s size)
        if (!to_g0) {
            const int covered = kConvK[i] == 2 ? 2 * Lout : Lin;
            Scope sc(c, s, NOMAD_K_ROW, 0.0);
            if (rg)
                hipLaunchKernelGGL(zero_rows512_ragged_kernel, dim3(B), dim3(256), 0, s, out, g.upref[i - 1], g.pref[i - 1], g.pref[i],
                                   kConvK[i] == 2 ? 1 : 0);
            else
                hipLaunchKernelGGL(zero_rows512_kernel, dim3(B), dim3(256), 0, s, out, out_clip, 0, 1, covered + 1, Lin + 2);
        } else if (kConvK[i] == 2) {
            HIP_TRY(hipMemsetAsync(out, 0, sizeof(float) * 512 * (size_t)g.rows[0], s));   // (not reached: conv1 has k = 3 and writes every frame of G0)
        }
        if (conv_pg) {  // input of layer i: gelu(u_{i-1}) recomputed in the transpose; for i = 1 conv0's output, recomputed whole
            if (i == 1) {
                Scope sc(c, s, NOMAD_K_FRONT, 0.0);
                hipLaunchKernelGGL(conv0_gn_gelu_kernel<float>, dim3((g.L[0] + kConv0Frames - 1) / kConv0Frames, B), dim3(256), 0, s, wav,
                                   n_samples, g.L[0], c->conv0_w, sv.gn_scale, sv.gn_shift, F(lay.h0), kNoInts, kNoInts, 0LL);
            }
            const float* in = i == 1 ? F(lay.h0) : sv.u[i - 1];
            if ((rc = conv_dw(i, dU, in, (long long)Lin * 512, i != 1))) return rc;
        }
        GemmParams p{};
        p.A = dU;
        p.C = out;
        p.DG = to_g0 ? nullptr : sv.u[i - 1];
        p.rmap = plain_map(1, 1);
        if (kConvK[i] == 2) {
            p.amap = amap_of(512, Lout, g.pref[i]);
            p.K = 512;
            p.W = c->conv_bw2[i];
            p.N = 1024;
            p.M = (int)g.rows[i];
            p.cmap = cmap_of(out_off, Lout, g.pref[i]);
            p.dgmap = dgmap_of(0, Lout, g.pref[i]);
            p.kchunk = p.K; p.ldw = p.K; p.n_valid = p.N;
            if ((rc = run_gemm(c, p, 1, pick_tile(c, p.M, p.N, p.K), s, splitk))) return rc;
        } else {
            const int E = (Lin + 1) / 2, O = Lin / 2;
            // even input frames 2t': dU[t'-1] W_tap2 + dU[t'] W_tap0
            p.amap = amap_of(0, E, g.epref[i - 1]);
            p.K = 1024;
            p.W = c->conv_bw_even[i];
            p.N = 512;
            p.M = (int)g.even[i - 1];
            p.cmap = cmap_of(out_off, E, g.epref[i - 1]);
            p.dgmap = dgmap_of(0, E, g.epref[i - 1]);
            p.kchunk = p.K; p.ldw = p.K; p.n_valid = p.N;
            if ((rc = run_gemm(c, p, 1, pick_tile(c, p.M, p.N, p.K), s, splitk))) return rc;
            // odd input frames 2t'+1: dU[t'] W_tap1
            p.amap = amap_of(512, O, g.opref[i - 1]);
            p.K = 512;
            p.W = c->conv_bw_odd[i];
            p.M = (int)g.odd[i - 1];
            p.cmap = cmap_of(out_off + 512, O, g.opref[i - 1]);
            p.dgmap = dgmap_of(512, O, g.opref[i - 1]);
            p.kchunk = p.K; p.ldw = p.K;
            if (p.M > 0 && (rc = run_gemm(c, p, 1, pick_tile(c, p.M, p.N, p.K), s, splitk))) return rc;
        }
    }
    // ---- conv0 + GroupNorm -> d loss / d waveform -------------------------------------------------------
    {
        const float* G0 = bufs[0];
        float* partial = F(lay.partial);
        if (dwav) HIP_TRY(hipMemsetAsync(dwav, 0, sizeof(float) * (size_t)B * n_samples, s));
        Scope sc(c, s, NOMAD_K_FRONT, 0.0);
        const dim3 grid(lay.nchunks, B);
        float* fold = F(lay.gnfold);
        // (a ragged batch: grids over the longest clip's chunks, a clip's workgroups leave behind its last frame; dwav behind a
        // clip's length keeps the zeros of the memset above)
        hipLaunchKernelGGL(gn_bwd_stats_kernel, dim3(lay.nstat, B), dim3(256), 0, s, wav, n_samples, g.L[0], c->conv0_w, sv.gn_scale,
                           sv.gn_shift, sv.gn_mean, sv.gn_rstd, G0, partial, g.pref[0]);
        hipLaunchKernelGGL(gn_bwd_fold_kernel, dim3(B), dim3(512), 0, s, partial, lay.nstat, g.L[0], c->conv0_w, sv.gn_scale, sv.gn_shift,
                           sv.gn_mean, sv.gn_rstd, fold, F(lay.cwtab), g.pref[0]);
        if (dwav)
            hipLaunchKernelGGL(conv0_bwd_kernel, dim3((g.max_l0 + kC0Frames - 1) / kC0Frames, B), dim3(256), 0, s, wav, n_samples, g.L[0],
                               F(lay.cwtab), G0, dwav, g.pref[0]);
        if (conv_pg) {  // conv0 weight, GroupNorm gamma / beta
            hipLaunchKernelGGL(conv0_param_partial_kernel, grid, dim3(256), 0, s, wav, n_samples, g.L[0], c->conv0_w, sv.gn_scale,
                               sv.gn_shift, sv.gn_mean, sv.gn_rstd, G0, fold, lay.nchunks, F(lay.c0part));
            hipLaunchKernelGGL(conv0_param_final_kernel, dim3(24), dim3(256), 0, s, F(lay.c0part), fold, B, lay.nchunks,
                               G(po.conv0_w), G(po.gn_w), G(po.gn_b));
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

static int backward_impl(nomad_ctx* c, const float* wav, int B, int n_samples, const float* head_w, const float* head_b,
                         const float* layers_out, const void* saved, size_t saved_bytes, const float* dlayers,
                         const float* demb, float* dwav, void* workspace, size_t workspace_bytes,
                         nomad_stream_t stream, bool train, const char* who = "nomad_embed_backward", const HeadRows* wb = nullptr) {
    Shapes sh;
    const bool cut = c && c->encoder_depth < NOMAD_NUM_LAYERS;   // a cut encoder has no embedding: demb is ignored, dlayers carries everything
    if (!c || !wav || !layers_out || !saved || (cut ? !dlayers : !demb) || (!dwav && !train) || !workspace || B <= 0 ||
        !make_shapes(B, n_samples, &sh))
        return fail(NOMAD_ERR_INVALID, "%s: bad argument%s", who, cut ? " (encoder depth below 12: dlayers_dev is required)" : "");
    if (!c->bwd_ready) return fail(NOMAD_ERR_INVALID, "%s: call nomad_enable_backward first", who);
    if (train && !c->train_ready) return fail(NOMAD_ERR_INVALID, "nomad_train_backward: call nomad_train_enable first");
    const BatchGeom g = geom_uniform(sh);
    const Saved sv = make_saved(g, const_cast<void*>(saved));
    const BwdLayout lay = make_bwd_layout(g, train, train && c->train_convnet);
    if (saved_bytes < sv.total || workspace_bytes < lay.total)
        return fail(NOMAD_ERR_WORKSPACE, "%s: saved %zu/%zu, workspace %zu/%zu", who, saved_bytes, sv.total,
                    workspace_bytes, lay.total);
    if (train && c->branches > 1 && B % c->branches)
        return fail(NOMAD_ERR_INVALID, "nomad_train_backward: B=%d is not %d equal branches", B, c->branches);
    return backward_run(c, wav, g, sv, lay, head_w, head_b, layers_out, dlayers, demb, dwav, static_cast<char*>(workspace),
                        static_cast<hipStream_t>(stream), train, wb);
}

// nomad_embed_backward_ragged / nomad_train_backward_ragged: the ragged prologue's steps over the BwdLayout.
static int backward_ragged(const char* who, nomad_ctx* c, const float* wav, int B, int stride, const int* lens_host, const float* head_w,
                           const float* head_b, const float* layers_out, const void* saved, size_t saved_bytes, const float* dlayers,
                           const float* demb, float* dwav, void* workspace, size_t workspace_bytes, nomad_stream_t stream,
                           bool train, const HeadRows* wb = nullptr) {
    RaggedShapes rs;
    const bool cut = c && c->encoder_depth < NOMAD_NUM_LAYERS;   // (a cut encoder: demb is ignored, dlayers is required)
    if (int rc = ragged_shapes(who, c && wav && layers_out && saved && (cut ? dlayers != nullptr : demb != nullptr) && (dwav || train) && workspace,
                               B, stride, lens_host, &rs))
        return rc;
    if (!c->bwd_ready) return fail(NOMAD_ERR_INVALID, "%s: call nomad_enable_backward first", who);
    if (train && !c->train_ready) return fail(NOMAD_ERR_INVALID, "%s: call nomad_train_enable first", who);
    if (train && c->train_convnet)
        return fail(NOMAD_ERR_INVALID, "%s: a trainable conv feature extractor (nomad_train_set_convnet) needs an equal-length batch", who);
    BatchGeom g = geom_ragged(rs, stride, nullptr);
    const BwdLayout lay = make_bwd_layout(g, train, false);
    const Saved sv = make_saved(g, const_cast<void*>(saved));
    if (saved_bytes < sv.total || workspace_bytes < lay.total)
        return fail(NOMAD_ERR_WORKSPACE, "%s: saved %zu/%zu, workspace %zu/%zu", who, saved_bytes, sv.total, workspace_bytes, lay.total);
    if (train && c->branches > 1 && B % c->branches) return fail(NOMAD_ERR_INVALID, "%s: B=%d is not %d equal branches", who, B, c->branches);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    if (int rc = ragged_upload(c, rs, stride, reinterpret_cast<int*>(ws + lay.meta), s, &g)) return rc;
    if (wb && wb->spans)
        if (int rc = span_upload(c, *wb->spans, s)) return rc;
    return backward_run(c, wav, g, sv, lay, head_w, head_b, layers_out, dlayers, demb, dwav, ws, s, train, wb);
}

// ---- fine-tuning state ------------------------------------------------------------------------------------
namespace {

// Rebuild every kernel-layout weight that is not a plain alias of the master vector: the fused, q-scaled q/k/v
// weights, the weight-normed pos-conv kernel, the repacked convs, and the copies the backward contracts with.
int refresh_weights(nomad_ctx* c, hipStream_t s) {
    const ParamOffsets& po = param_offsets();
    // The derived fp32 weights, formed on the DEVICE from the master vector: weight norm folded, conv1..6 repacked, q/k/v scaled.
    // nomad_create forms the same three on the HOST from the checkpoint; the repack and the scale are exact either way, the two
    // weight-norm folds add their squares in different orders (a scale can differ in its last bit) - two routes on purpose.
    hipLaunchKernelGGL(tap_dot_partial_kernel, dim3(576), dim3(256), 0, s, c->theta + po.pos_v, (const float*)nullptr,
                       c->tap_partial);
    hipLaunchKernelGGL(tap_sum_final_kernel, dim3(1), dim3(1024), 0, s, c->tap_partial, 576, c->pos_nrm2);
    hipLaunchKernelGGL(posconv_fold_kernel, dim3(768), dim3(256), 0, s, c->theta + po.pos_v, c->theta + po.pos_g,
                       c->pos_nrm2, c->pos_w);
    if (c->pos_wt)
        if (int rc = rebuild_posconv_wino_weights(c, s)) return rc;
    if (c->pos_wf)
        if (int rc = launch_posconv_fft_weights(c, c->pos_w, c->pos_wf, s)) return rc;
    for (int i = 1; i < 7; ++i) {  // conv feature extractor: kernel layout [co][tap * 512 + ci]
        const long long n = 512LL * 512 * kConvK[i];
        hipLaunchKernelGGL(conv_repack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c->theta + po.conv_w[i], c->conv_w[i],
                           kConvK[i]);
    }
    for (int l = 0; l < NOMAD_NUM_LAYERS; ++l) {
        const LayerDev& d = c->layers[l];
        const LayerOffsets& lo = po.L[l];
        const long long w4 = (long long)2304 * 768 / 4, q4 = (long long)768 * 768 / 4;
        hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)((w4 + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const float4*>(c->theta + lo.qkv_w), reinterpret_cast<float4*>(d.qkv_w), w4, q4, 0.125f);
        hipLaunchKernelGGL(scale_rows_kernel, dim3(3), dim3(256), 0, s, reinterpret_cast<const float4*>(c->theta + lo.qkv_b),
                           reinterpret_cast<float4*>(d.qkv_b), 576LL, 192LL, 0.125f);
    }
    build_backward_weights(c, s);
    HIP_TRY(hipGetLastError());
    c->bf16_ready = false;  // the bf16 copies (if any) are stale now; nomad_enable_bf16 rebuilds them
    c->x3_ready = false;    // likewise the split copies (nomad_enable_bf16x3)
    return 0;
}

}  // namespace

extern "C" {

int nomad_set_gemm_precision(nomad_ctx* c, int mode) {
    if (!c || (mode != 0 && mode != 1)) return fail(NOMAD_ERR_INVALID, "nomad_set_gemm_precision: mode must be 0 (fp32 MFMA) or 1 (bf16x3 products)");
    c->gemm_x3 = mode;
    return 0;
}

int nomad_get_gemm_precision(const nomad_ctx* c, int* mode) {
    if (!c || !mode) return fail(NOMAD_ERR_INVALID, "nomad_get_gemm_precision: null argument");
    *mode = c->gemm_x3;
    return 0;
}

int nomad_set_feature_grad_mult(nomad_ctx* c, float mult) {
    if (!c || !(mult >= 0.f)) return fail(NOMAD_ERR_INVALID, "nomad_set_feature_grad_mult: bad argument");
    c->feature_grad_mult = mult;
    return 0;
}

int nomad_get_feature_grad_mult(const nomad_ctx* c, float* mult) {
    if (!c || !mult) return fail(NOMAD_ERR_INVALID, "nomad_get_feature_grad_mult: bad argument");
    *mult = c->feature_grad_mult;
    return 0;
}

int nomad_set_encoder_depth(nomad_ctx* c, int depth) {
    if (!c || depth < 1 || depth > NOMAD_NUM_LAYERS)
        return fail(NOMAD_ERR_INVALID, "nomad_set_encoder_depth: depth %d is outside 1 .. %d", depth, NOMAD_NUM_LAYERS);
    c->encoder_depth = depth;
    return 0;
}

int nomad_get_encoder_depth(const nomad_ctx* c, int* depth) {
    if (!c || !depth) return fail(NOMAD_ERR_INVALID, "nomad_get_encoder_depth: null argument");
    *depth = c->encoder_depth;
    return 0;
}

int nomad_embed_backward(nomad_ctx* c, const float* wav, int B, int n_samples, const float* head_w, const float* head_b,
                         const float* layers_out, const void* saved, size_t saved_bytes, const float* dlayers,
                         const float* demb, float* dwav, void* workspace, size_t workspace_bytes,
                         nomad_stream_t stream) {
    if (!dwav) return fail(NOMAD_ERR_INVALID, "nomad_embed_backward: bad argument");
    return backward_impl(c, wav, B, n_samples, head_w, head_b, layers_out, saved, saved_bytes, dlayers, demb, dwav,
                         workspace, workspace_bytes, stream, false);
}

int nomad_embed_backward_ragged(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, const float* head_w,
                                const float* head_b, const float* layers_out, const void* saved, size_t saved_bytes,
                                const float* dlayers, const float* demb, float* dwav, void* workspace, size_t workspace_bytes,
                                nomad_stream_t stream) {
    if (!dwav) return fail(NOMAD_ERR_INVALID, "nomad_embed_backward_ragged: bad argument");
    return backward_ragged("nomad_embed_backward_ragged", c, wav, B, stride, lengths_host, head_w, head_b, layers_out, saved, saved_bytes,
                           dlayers, demb, dwav, workspace, workspace_bytes, stream, false);
}

// ---- the windowed head on the gradient path: nomad_embed_train[_ragged] / nomad_embed_backward[_ragged] with head_windows_kernel
// and its backward as the head stage.  Every check of those calls holds; the windows add theirs ahead, so nothing is queued on an error.
static int windows_grad_args(const char* who, const nomad_ctx* c, int win, int hop, const float* head_w, const float* head_b) {
    if (int rc = windows_args(who, c, NOMAD_PRECISION_F32, win, hop, head_w, head_b)) return rc;
    // fine-tuning mode: the training-mode forward then draws dropout and LayerDrop masks that this backward (d loss / d waveform with
    // frozen weights) does not replay, and the head's own parameter gradients have no windowed form
    if (c && c->train_ready) return fail(NOMAD_ERR_INVALID, "%s: not in fine-tuning mode (nomad_train_enable)", who);
    return 0;
}

int nomad_window_cover(int T, int win, int hop, int t, int* k_lo, int* k_hi) {
    if (!k_lo || !k_hi || T < 1 || win < 1 || hop < 1 || t < 0 || t >= T)
        return fail(NOMAD_ERR_INVALID, "nomad_window_cover: bad argument (T=%d, win=%d, hop=%d, t=%d)", T, win, hop, t);
    head_window_cover(T, win, hop, t, k_lo, k_hi);
    return 0;
}

int nomad_windows_backward_scratch_bytes(long long n_windows, size_t* bytes) {
    if (!bytes || n_windows <= 0) return fail(NOMAD_ERR_INVALID, "nomad_windows_backward_scratch_bytes: bad argument (n_windows=%lld)", n_windows);
    *bytes = align_up(sizeof(float) * 768 * (size_t)n_windows);   // gw [n_windows][768]
    return 0;
}

int nomad_embed_train_windows(nomad_ctx* c, const float* wav, int B, int n_samples, int win, int hop, const float* head_w,
                              const float* head_b, float* emb, float* layers_out, void* saved, size_t saved_bytes, void* workspace,
                              size_t workspace_bytes, nomad_stream_t stream) {
    static const char who[] = "nomad_embed_train_windows";
    if (int rc = windows_grad_args(who, c, win, hop, head_w, head_b)) return rc;
    Shapes sh;
    if (!c || !saved || !layers_out || B <= 0 || !make_shapes(B, n_samples, &sh)) return fail(NOMAD_ERR_INVALID, "%s: bad argument", who);
    const Saved sv = make_saved(geom_uniform(sh), saved);
    if (saved_bytes < sv.total) return fail(NOMAD_ERR_WORKSPACE, "%s: saved block %zu < required %zu", who, saved_bytes, sv.total);
    const HeadMode mode = HeadMode::windows(win, hop, (long long)B * head_num_windows(sh.T, win, hop));
    return forward_impl(c, wav, B, n_samples, head_w, head_b, emb, layers_out, workspace, workspace_bytes, stream, &sv, who, mode);
}

int nomad_embed_train_windows_ragged(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, int win, int hop,
                                     const float* head_w, const float* head_b, float* emb, float* layers_out, void* saved,
                                     size_t saved_bytes, void* workspace, size_t workspace_bytes, nomad_stream_t stream) {
    static const char who[] = "nomad_embed_train_windows_ragged";
    if (int rc = windows_grad_args(who, c, win, hop, head_w, head_b)) return rc;
    if (!c || !layers_out || !saved) return fail(NOMAD_ERR_INVALID, "%s: bad argument", who);
    long long n = 0;
    for (int i = 0; lengths_host && i < B; ++i) n += head_num_windows(nomad_num_frames(lengths_host[i]), win, hop);
    return forward_ragged(c, wav, B, stride, lengths_host, head_w, head_b, emb, workspace, workspace_bytes, stream, who,
                          HeadMode::windows(win, hop, n), layers_out, saved, saved_bytes);
}

int nomad_embed_windows_backward(nomad_ctx* c, const float* wav, int B, int n_samples, int win, int hop, const float* head_w,
                                 const float* head_b, const float* layers_out, const void* saved, size_t saved_bytes, const float* demb,
                                 float* dwav, void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes,
                                 nomad_stream_t stream) {
    static const char who[] = "nomad_embed_windows_backward";
    if (int rc = windows_grad_args(who, c, win, hop, head_w, head_b)) return rc;
    Shapes sh;
    if (!c || !demb || !dwav || !scratch || B <= 0 || !make_shapes(B, n_samples, &sh)) return fail(NOMAD_ERR_INVALID, "%s: bad argument", who);
    const size_t need = align_up(sizeof(float) * 768 * (size_t)B * head_num_windows(sh.T, win, hop));
    if (scratch_bytes < need) return fail(NOMAD_ERR_WORKSPACE, "%s: scratch %zu < required %zu", who, scratch_bytes, need);
    const HeadRows wb{win, hop, nullptr, static_cast<float*>(scratch)};
    return backward_impl(c, wav, B, n_samples, head_w, head_b, layers_out, saved, saved_bytes, nullptr, demb, dwav, workspace,
                         workspace_bytes, stream, false, who, &wb);
}

int nomad_embed_windows_backward_ragged(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, int win, int hop,
                                        const float* head_w, const float* head_b, const float* layers_out, const void* saved,
                                        size_t saved_bytes, const float* demb, float* dwav, void* scratch, size_t scratch_bytes,
                                        void* workspace, size_t workspace_bytes, nomad_stream_t stream) {
    static const char who[] = "nomad_embed_windows_backward_ragged";
    if (int rc = windows_grad_args(who, c, win, hop, head_w, head_b)) return rc;
    if (!c || !demb || !dwav || !scratch || !lengths_host || B <= 0) return fail(NOMAD_ERR_INVALID, "%s: bad argument", who);
    long long n = 0;
    bool frames_ok = true;   // (a clip below one frame: left to the shape checks below, NOMAD_ERR_INVALID)
    for (int i = 0; i < B; ++i) {
        const int t = nomad_num_frames(lengths_host[i]);
        frames_ok = frames_ok && t >= 1;
        n += head_num_windows(t, win, hop);
    }
    const size_t need = align_up(sizeof(float) * 768 * (size_t)n);
    if (frames_ok && scratch_bytes < need) return fail(NOMAD_ERR_WORKSPACE, "%s: scratch %zu < required %zu", who, scratch_bytes, need);
    const HeadRows wb{win, hop, nullptr, static_cast<float*>(scratch)};
    return backward_ragged(who, c, wav, B, stride, lengths_host, head_w, head_b, layers_out, saved, saved_bytes, nullptr, demb, dwav,
                           workspace, workspace_bytes, stream, false, &wb);
}

// ---- the head over caller-given spans of frames: nomad_embed_spans_ragged and its gradient path.  The windows calls with a table of
// rows of spans in place of (win, hop): every check of those calls holds, the table's come ahead, nothing is queued on an error.
static size_t span_table_bytes(int B, int R, int S) { return align_up(sizeof(int) * span_table_ints(B, R, S)); }

// The table's checks, then its host copy in the device block's layout and its place (and gw's) in the caller's scratch.
static int spans_stage(const char* who, int B, const int* lens_host, int R, const int* row_clip, const int* row_ptr, const int* spans,
                       void* scratch, size_t scratch_bytes, bool backward, SpanStage* st) {
    if (R < 1) return fail(NOMAD_ERR_INVALID, "%s: a span table needs at least one row (R=%d)", who, R);
    if (!row_clip || !row_ptr || !spans) return fail(NOMAD_ERR_INVALID, "%s: a NULL span table pointer (row_clip, row_ptr or spans)", who);
    if (!lens_host || B <= 0 || !scratch) return fail(NOMAD_ERR_INVALID, "%s: bad argument (B=%d)", who, B);
    if (row_ptr[0] != 0) return fail(NOMAD_ERR_INVALID, "%s: row_ptr[0] is %d, not 0", who, row_ptr[0]);
    for (int r = 0; r < R; ++r) {
        const int cl = row_clip[r];
        if (cl < 0 || cl >= B) return fail(NOMAD_ERR_INVALID, "%s: row %d names clip %d, outside [0, %d)", who, r, cl, B);
        if (r && cl < row_clip[r - 1]) return fail(NOMAD_ERR_INVALID, "%s: row %d names clip %d behind row %d's clip %d (row_clip must not decrease)", who, r, cl, r - 1, row_clip[r - 1]);
        if (row_ptr[r + 1] <= row_ptr[r]) return fail(NOMAD_ERR_INVALID, "%s: row %d has no span (row_ptr %d .. %d)", who, r, row_ptr[r], row_ptr[r + 1]);
        const int T = nomad_num_frames(lens_host[cl]);
        for (int i = row_ptr[r]; i < row_ptr[r + 1]; ++i) {
            const int t0 = spans[2 * i], t1 = spans[2 * i + 1], k = i - row_ptr[r];
            if (t0 < 0 || t1 > T || t0 >= t1)
                return fail(NOMAD_ERR_INVALID, "%s: row %d, span %d is [%d, %d): not inside clip %d's %d frames", who, r, k, t0, t1, cl, T);
            if (k && t0 < spans[2 * i - 1])
                return fail(NOMAD_ERR_INVALID, "%s: row %d, span %d [%d, %d) overlaps or precedes span %d, which ends at %d", who, r, k, t0, t1, k - 1, spans[2 * i - 1]);
        }
    }
    const int S = row_ptr[R];
    const size_t need = span_table_bytes(B, R, S) + (backward ? align_up(sizeof(float) * 768 * (size_t)R) : 0);
    if (scratch_bytes < need) return fail(NOMAD_ERR_WORKSPACE, "%s: scratch %zu < required %zu", who, scratch_bytes, need);
    st->R = R, st->S = S;
    st->dev = static_cast<int*>(scratch);
    st->gw = backward ? reinterpret_cast<float*>(static_cast<char*>(scratch) + span_table_bytes(B, R, S)) : nullptr;
    st->host.reserve(span_table_ints(B, R, S));
    st->host.assign(row_clip, row_clip + R);
    st->host.insert(st->host.end(), row_ptr, row_ptr + R + 1);
    st->host.insert(st->host.end(), spans, spans + 2 * (size_t)S);
    for (int b = 0, r = 0; b <= B; ++b) {   // clip_row[b]: the first row of a clip >= b
        while (r < R && row_clip[r] < b) ++r;
        st->host.push_back(r);
    }
    return 0;
}

int nomad_spans_scratch_bytes(int B, int R, int S, int backward, size_t* bytes) {
    if (!bytes || B < 1 || R < 1 || S < R)
        return fail(NOMAD_ERR_INVALID, "nomad_spans_scratch_bytes: bad argument (B=%d, R=%d, S=%d)", B, R, S);
    *bytes = span_table_bytes(B, R, S) + (backward ? align_up(sizeof(float) * 768 * (size_t)R) : 0);
    return 0;
}

int nomad_embed_spans_ragged(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, int precision, int R,
                             const int* row_clip, const int* row_ptr, const int* spans, const float* head_w, const float* head_b,
                             float* emb, void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes,
                             nomad_stream_t stream) {
    static const char who[] = "nomad_embed_spans_ragged";
    if (int rc = windows_args(who, c, precision, 1, 1, head_w, head_b)) return rc;
    if (precision != NOMAD_PRECISION_F32 && precision != NOMAD_PRECISION_BF16X3 && precision != NOMAD_PRECISION_BF16)
        return fail(NOMAD_ERR_INVALID, "%s: unknown precision %d", who, precision);
    SpanStage st;
    if (int rc = spans_stage(who, B, lengths_host, R, row_clip, row_ptr, spans, scratch, scratch_bytes, false, &st)) return rc;
    const HeadMode mode = HeadMode::over_spans(&st);
    switch (precision) {
        case NOMAD_PRECISION_F32:
            return forward_ragged(c, wav, B, stride, lengths_host, head_w, head_b, emb, workspace, workspace_bytes, stream, who, mode);
        case NOMAD_PRECISION_BF16X3:
            return forward_ragged_x3(c, wav, B, stride, lengths_host, emb, workspace, workspace_bytes, stream, who, mode);
        default:
            return forward_ragged_bf16(c, wav, B, stride, lengths_host, emb, workspace, workspace_bytes, stream, who, mode);
    }
}

int nomad_embed_train_spans_ragged(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, int R,
                                   const int* row_clip, const int* row_ptr, const int* spans, const float* head_w, const float* head_b,
                                   float* emb, float* layers_out, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                                   void* workspace, size_t workspace_bytes, nomad_stream_t stream) {
    static const char who[] = "nomad_embed_train_spans_ragged";
    if (int rc = windows_grad_args(who, c, 1, 1, head_w, head_b)) return rc;
    if (!c || !layers_out || !saved) return fail(NOMAD_ERR_INVALID, "%s: bad argument", who);
    SpanStage st;
    if (int rc = spans_stage(who, B, lengths_host, R, row_clip, row_ptr, spans, scratch, scratch_bytes, false, &st)) return rc;
    return forward_ragged(c, wav, B, stride, lengths_host, head_w, head_b, emb, workspace, workspace_bytes, stream, who,
                          HeadMode::over_spans(&st), layers_out, saved, saved_bytes);
}

int nomad_embed_spans_backward_ragged(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, int R,
                                      const int* row_clip, const int* row_ptr, const int* spans, const float* head_w,
                                      const float* head_b, const float* layers_out, const void* saved, size_t saved_bytes,
                                      const float* demb, float* dwav, void* scratch, size_t scratch_bytes, void* workspace,
                                      size_t workspace_bytes, nomad_stream_t stream) {
    static const char who[] = "nomad_embed_spans_backward_ragged";
    if (int rc = windows_grad_args(who, c, 1, 1, head_w, head_b)) return rc;
    if (!c || !demb || !dwav) return fail(NOMAD_ERR_INVALID, "%s: bad argument", who);
    SpanStage st;
    if (int rc = spans_stage(who, B, lengths_host, R, row_clip, row_ptr, spans, scratch, scratch_bytes, true, &st)) return rc;
    const HeadRows wb = HeadRows::over_spans(&st);
    return backward_ragged(who, c, wav, B, stride, lengths_host, head_w, head_b, layers_out, saved, saved_bytes, nullptr, demb, dwav,
                           workspace, workspace_bytes, stream, false, &wb);
}

// Frame energies (rowops.hip.h, frame_energy_kernel): the clips go to the kernel kEnergyClips at a time, their metadata by value,
// so the call needs neither scratch nor a staged copy.
int nomad_frame_energy(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, double* energy, nomad_stream_t stream) {
    static const char who[] = "nomad_frame_energy";
    if (!c || !wav || !lengths_host || !energy || B <= 0 || stride <= 0) return fail(NOMAD_ERR_INVALID, "%s: bad argument (B=%d)", who, B);
    for (int i = 0; i < B; ++i) {
        if (lengths_host[i] > stride) return fail(NOMAD_ERR_INVALID, "%s: clip %d longer than the row stride", who, i);
        if (nomad_num_frames(lengths_host[i]) < 1)
            return fail(NOMAD_ERR_INVALID, "%s: clip %d of %d samples is shorter than one frame", who, i, lengths_host[i]);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long done = 0;
    for (int c0 = 0; c0 < B; c0 += kEnergyClips) {
        const int nc = B - c0 < kEnergyClips ? B - c0 : kEnergyClips;
        EnergyClips cl{};
        int max_t = 0;
        for (int i = 0; i < nc; ++i) {
            const int t = nomad_num_frames(lengths_host[c0 + i]);
            cl.len[i] = lengths_host[c0 + i];
            cl.fpref[i + 1] = cl.fpref[i] + t;
            max_t = t > max_t ? t : max_t;
        }
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        hipLaunchKernelGGL(frame_energy_kernel, dim3((max_t + 3) / 4, nc), dim3(256), 0, s, wav + (size_t)c0 * stride, (long long)stride, cl,
                           energy + done);
        done += cl.fpref[nc];
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int nomad_train_num_segments(void) { return (int)segments().size(); }

int nomad_train_segment(int i, char* name, size_t name_cap, size_t* offset, size_t* count) {
    const auto& v = segments();
    if (i < 0 || i >= (int)v.size() || !name || !offset || !count || name_cap <= v[i].name.size())
        return fail(NOMAD_ERR_INVALID, "nomad_train_segment: bad argument");
    memcpy(name, v[i].name.c_str(), v[i].name.size() + 1);
    *offset = v[i].offset;
    *count = v[i].count;
    return 0;
}

int nomad_train_param_count(size_t* total, size_t* head_begin) {
    if (!total) return fail(NOMAD_ERR_INVALID, "nomad_train_param_count: null argument");
    const ParamOffsets& po = param_offsets();
    *total = po.total;
    if (head_begin) *head_begin = po.emb_w;
    return 0;
}

int nomad_train_enable(nomad_ctx* c, const nomad_weights* w) {
    if (!c || !w) return fail(NOMAD_ERR_INVALID, "nomad_train_enable: null argument");
    if (c->train_ready) return 0;
    int rc;
    if ((rc = nomad_enable_backward(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    static const char who[] = "nomad_train_enable";
    ParamOffsets po = param_offsets();
    if ((rc = dev_alloc(c, who, po.total, &c->theta, true))) return rc;
    if ((rc = dev_alloc(c, who, po.total, &c->grad, true))) return rc;
    if ((rc = dev_alloc(c, who, po.total, &c->adam_m, true))) return rc;
    if ((rc = dev_alloc(c, who, po.total, &c->adam_v, true))) return rc;
    if ((rc = dev_alloc(c, who, 128, &c->pos_nrm2, true))) return rc;
    if ((rc = dev_alloc(c, who, 128, &c->tap_dot, true))) return rc;
    if ((rc = dev_alloc(c, who, (size_t)576 * 128, &c->tap_partial, true))) return rc;
    for_each_param(*w, po, *c, [&](const Param& p) {
        if (rc == 0 && hipMemcpy(c->theta + *p.slot + p.sub, p.host, p.count * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(NOMAD_ERR_HIP, "nomad_train_enable: upload failed");
    });
    if (rc) return rc;
    // From here on the engine reads these parameters straight from the master vector (same layout as the checkpoint); only
    // q/k/v (fused, q scaled), the pos-conv kernel, conv1..6 and the backward's copies are derived (refresh_weights).
    for_each_param(*w, po, *c, [&](const Param& p) {
        if (p.alias) *p.alias = c->theta + *p.slot + p.sub;
    });
    if ((rc = refresh_weights(c, 0))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    c->adam_t = 0;
    c->train_ready = true;
    return 0;
}

int nomad_train_workspace_bytes(const nomad_ctx* c, int B, int n_samples, size_t* bytes) {
    Shapes sh;
    if (!c || !bytes || B <= 0 || !make_shapes(B, n_samples, &sh))
        return fail(NOMAD_ERR_INVALID, "nomad_train_workspace_bytes: bad shape B=%d N=%d", B, n_samples);
    *bytes = make_bwd_layout(geom_uniform(sh), true, c->train_convnet).total;
    return 0;
}

int nomad_train_zero_grad(nomad_ctx* c, nomad_stream_t stream) {
    if (!c || !c->train_ready) return fail(NOMAD_ERR_INVALID, "nomad_train_zero_grad: call nomad_train_enable first");
    HIP_TRY(hipMemsetAsync(c->grad, 0, param_offsets().total * sizeof(float), static_cast<hipStream_t>(stream)));
    return 0;
}

int nomad_train_backward(nomad_ctx* c, const float* wav, int B, int n_samples, const float* layers_out, const void* saved,
                         size_t saved_bytes, const float* demb, void* workspace, size_t workspace_bytes,
                         nomad_stream_t stream) {
    if (int rc = refuse_cut(c, "nomad_train_backward")) return rc;
    return backward_impl(c, wav, B, n_samples, nullptr, nullptr, layers_out, saved, saved_bytes, nullptr, demb, nullptr,
                         workspace, workspace_bytes, stream, true);
}

int nomad_train_backward_ragged(nomad_ctx* c, const float* wav, int B, int stride, const int* lengths_host, const float* layers_out,
                                const void* saved, size_t saved_bytes, const float* demb, void* workspace, size_t workspace_bytes,
                                nomad_stream_t stream) {
    if (int rc = refuse_cut(c, "nomad_train_backward_ragged")) return rc;
    return backward_ragged("nomad_train_backward_ragged", c, wav, B, stride, lengths_host, nullptr, nullptr, layers_out, saved, saved_bytes,
                           nullptr, demb, nullptr, workspace, workspace_bytes, stream, true);
}

int nomad_triplet_loss(nomad_ctx* c, const float* a, const float* p, const float* n, int B, float margin, float* loss,
                       float* da, float* dp, float* dn, nomad_stream_t stream) {
    if (!c || !a || !p || !n || !loss || B <= 0 || (da && (!dp || !dn)))
        return fail(NOMAD_ERR_INVALID, "nomad_triplet_loss: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(triplet_loss_kernel, dim3(1), dim3(256), 0, s, a, p, n, B, margin, loss, da, dp, dn);
    HIP_TRY(hipGetLastError());
    return 0;
}

int nomad_train_adam_step(nomad_ctx* c, float lr_body, float lr_head, double beta1, double beta2, float eps,
                          nomad_stream_t stream) {
    if (!c || !c->train_ready) return fail(NOMAD_ERR_INVALID, "nomad_train_adam_step: call nomad_train_enable first");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const ParamOffsets& po = param_offsets();
    c->adam_t += 1;
    const double bc1 = 1.0 - std::pow(beta1, (double)c->adam_t);
    const double bc2 = 1.0 - std::pow(beta2, (double)c->adam_t);
    const long long n4 = (long long)po.total / 4;
    {
        Scope sc(c, s, NOMAD_K_ROW, 0.0);
        hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<float4*>(c->theta),
                           reinterpret_cast<const float4*>(c->grad), reinterpret_cast<float4*>(c->adam_m),
                           reinterpret_cast<float4*>(c->adam_v), n4, (long long)po.emb_w / 4, lr_body, lr_head, (float)(1.0 - beta1),
                           (float)beta2, (float)(1.0 - beta2), eps, (float)bc1, (float)std::sqrt(bc2));
    }
    HIP_TRY(hipGetLastError());
    return refresh_weights(c, s);
}

// what: 0 parameters, 1 gradients, 2 Adam exp_avg, 3 Adam exp_avg_sq.  Device-to-device on the stream.
static float* train_buffer(nomad_ctx* c, int what) {
    switch (what) {
        case 0: return c->theta;
        case 1: return c->grad;
        case 2: return c->adam_m;
        case 3: return c->adam_v;
        default: return nullptr;
    }
}

int nomad_train_read(nomad_ctx* c, int what, float* dst_dev, nomad_stream_t stream) {
    if (!c || !c->train_ready || !dst_dev || !train_buffer(c, what))
        return fail(NOMAD_ERR_INVALID, "nomad_train_read: bad argument");
    HIP_TRY(hipMemcpyAsync(dst_dev, train_buffer(c, what), param_offsets().total * sizeof(float),
                           hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return 0;
}

int nomad_train_write(nomad_ctx* c, int what, const float* src_dev, nomad_stream_t stream) {
    if (!c || !c->train_ready || !src_dev || !train_buffer(c, what))
        return fail(NOMAD_ERR_INVALID, "nomad_train_write: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(train_buffer(c, what), src_dev, param_offsets().total * sizeof(float),
                           hipMemcpyDeviceToDevice, s));
    return what == 0 ? refresh_weights(c, s) : 0;
}

int nomad_train_set_stochastic(nomad_ctx* c, float dropout, float attention_dropout, float dropout_input,
                               unsigned long long seed, unsigned layer_mask) {
    auto bad = [](float p) { return !(p >= 0.f && p < 1.f); };
    if (!c || bad(dropout) || bad(attention_dropout) || bad(dropout_input))
        return fail(NOMAD_ERR_INVALID, "nomad_train_set_stochastic: probabilities must be in [0, 1)");
    c->p_drop = dropout;
    c->p_attn = attention_dropout;
    c->p_input = dropout_input;
    c->drop_seed = seed;
    c->layer_mask = layer_mask & 0xFFFu;
    return 0;
}

int nomad_train_set_branches(nomad_ctx* c, int branches, const unsigned* layer_masks) {
    if (!c || branches < 1 || branches > 4 || (branches > 1 && !layer_masks))
        return fail(NOMAD_ERR_INVALID, "nomad_train_set_branches: 1..4 branches, one mask each");
    c->branches = branches;
    for (int i = 0; i < branches && layer_masks; ++i) c->branch_mask[i] = layer_masks[i] & 0xFFFu;
    return 0;
}

int nomad_train_set_frozen(nomad_ctx* c, int freeze_encoder) {
    if (!c) return fail(NOMAD_ERR_INVALID, "nomad_train_set_frozen: null ctx");
    c->freeze_encoder = freeze_encoder != 0;
    return 0;
}

int nomad_train_set_convnet(nomad_ctx* c, int trainable) {
    if (!c) return fail(NOMAD_ERR_INVALID, "nomad_train_set_convnet: null ctx");
    c->train_convnet = trainable != 0;
    return 0;
}

int nomad_train_set_step(nomad_ctx* c, long long step) {
    if (!c || !c->train_ready || step < 0) return fail(NOMAD_ERR_INVALID, "nomad_train_set_step: bad argument");
    c->adam_t = step;
    return 0;
}

int nomad_set_concurrent_parts(nomad_ctx* c, int parts) {
    if (!c || parts < 1) return fail(NOMAD_ERR_INVALID, "nomad_set_concurrent_parts: ctx %p, parts = %d", (void*)c, parts);
    c->tune.concurrent_parts = parts;
    return 0;
}

int nomad_build_flags(void) {
    int f = 0;
#ifdef NOMAD_PACKED_FP32_BUILD
    f |= NOMAD_BUILD_PACKED_FP32;
#endif
#ifdef NOMAD_DIAG
    f |= NOMAD_BUILD_DIAG;
#endif
    return f;
}

}  // extern "C"

// The context's scratch block of launch stream s (nomad_pairwise, nomad_cdist).
static int pair_scratch_for(nomad_ctx* c, hipStream_t s, double** out) {
    // per-(ref tile, deg row) partial sums live in a context-owned scratch, one block per launch stream (calls on the same
    // stream are ordered, calls on different streams must not share it): the block of nomad_create goes to the first
    // stream that calls, any further stream allocates its own on its first call
    double* scratch = nullptr;
    *out = nullptr;
    std::unique_lock<std::mutex> pair_lock(c->pair_mu);   // look-up, binding and allocation of a stream's block: one thread at a time
    for (const auto& e : c->pair_scratch)
        if (e.first == s) {
            scratch = e.second;
            break;
        }
    if (!scratch) {
        // a block whose stream slot was released by an earlier recycle (first == kNoStream) is taken before anything new is
        // allocated; at most 64 blocks (1 GB) ever exist, whatever the number of stream handles a long-lived process goes through
        for (auto& e : c->pair_scratch)
            if (e.first == kNoStream) {
                e.first = s;
                scratch = e.second;
                break;
            }
    }
    if (!scratch) {
        if (c->pair_scratch.size() >= 64) {  // every block is bound: drain the device once and release all bindings but this one
            HIP_TRY(hipDeviceSynchronize());
            for (auto& e : c->pair_scratch) e.first = kNoStream;
            c->pair_scratch[0].first = s;
            scratch = c->pair_scratch[0].second;
        } else {
            HIP_TRY(hipSetDevice(c->device));
            if (int rc = dev_alloc(c, "pairwise scratch", (size_t)kPairScratchDoubles, &scratch)) return rc;
            c->pair_scratch.emplace_back(s, scratch);
        }
    }
    pair_lock.unlock();
    *out = scratch;
    return 0;
}

extern "C" {

int nomad_pairwise(nomad_ctx* c, const float* deg, int Nd, const float* ref, int Nr, double* dist, double* mean,
                   nomad_stream_t stream) {
    if (!c || !deg || !ref || !mean || Nd <= 0 || Nr <= 0)
        return fail(NOMAD_ERR_INVALID, "nomad_pairwise: bad argument (Nd=%d, Nr=%d)", Nd, Nr);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* scratch = nullptr;
    if (int rc = pair_scratch_for(c, s, &scratch)) return rc;
    Scope sc(c, s, NOMAD_K_PAIR, 3.0 * 256 * (double)Nd * Nr);
    // deg rows are processed in slabs that fit the scratch
    const int ntiles = (Nr + kPairTile - 1) / kPairTile;
    const long long slab_max = (kPairScratchDoubles / ntiles) / kPairTile * kPairTile;
    if (slab_max < kPairTile) return fail(NOMAD_ERR_INVALID, "nomad_pairwise: Nr=%d is too large for the scratch", Nr);
    for (long long d0 = 0; d0 < Nd; d0 += slab_max) {
        const int nd = (int)std::min<long long>(slab_max, Nd - d0);
        hipLaunchKernelGGL(pairwise_tile_kernel<256>, dim3(ntiles, (nd + kPairTile - 1) / kPairTile), dim3(256), 0, s, deg + d0 * 256, nd,
                           ref, Nr, 256, dist ? dist + d0 * Nr : nullptr, scratch);
        hipLaunchKernelGGL(pairwise_mean_kernel, dim3((nd + 255) / 256), dim3(256), 0, s, scratch, ntiles, nd, Nr, mean + d0);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// nomad_pairwise with the row width as an argument (pairwise_tile_kernel<0>: the same arithmetic chain, bit-identical at D = 256).
int nomad_cdist(nomad_ctx* c, const float* a, int Na, const float* b, int Nb, int D, double* dist, double* mean,
                nomad_stream_t stream) {
    if (!c || !a || !b || !mean || Na <= 0 || Nb <= 0 || D <= 0 || D % 4 || D > kCdistMaxD)
        return fail(NOMAD_ERR_INVALID, "nomad_cdist: bad argument (Na=%d, Nb=%d, D=%d: a positive multiple of 4, at most %d)", Na, Nb, D,
                    kCdistMaxD);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* scratch = nullptr;
    if (int rc = pair_scratch_for(c, s, &scratch)) return rc;
    Scope sc(c, s, NOMAD_K_PAIR, 3.0 * D * (double)Na * Nb);
    const int ntiles = (Nb + kPairTile - 1) / kPairTile;
    const long long slab_max = (kPairScratchDoubles / ntiles) / kPairTile * kPairTile;   // rows of `a` per launch pair
    if (slab_max < kPairTile) return fail(NOMAD_ERR_INVALID, "nomad_cdist: Nb=%d is too large for the scratch", Nb);
    for (long long d0 = 0; d0 < Na; d0 += slab_max) {
        const int nd = (int)std::min<long long>(slab_max, Na - d0);
        hipLaunchKernelGGL(pairwise_tile_kernel<0>, dim3(ntiles, (nd + kPairTile - 1) / kPairTile), dim3(256), 0, s, a + d0 * D, nd, b, Nb, D,
                           dist ? dist + d0 * Nb : nullptr, scratch);
        hipLaunchKernelGGL(pairwise_mean_kernel, dim3((nd + 255) / 256), dim3(256), 0, s, scratch, ntiles, nd, Nb, mean + d0);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int nomad_paired_distance(nomad_ctx* c, const float* a, const float* b, int N, int D, double* out, nomad_stream_t stream) {
    if (!c || !a || !b || !out || N <= 0 || D <= 0 || D % 4 || D > kCdistMaxD)
        return fail(NOMAD_ERR_INVALID, "nomad_paired_distance: bad argument (N=%d, D=%d: a positive multiple of 4, at most %d)", N, D,
                    kCdistMaxD);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scope sc(c, s, NOMAD_K_PAIR, 3.0 * D * (double)N);
    hipLaunchKernelGGL(paired_distance_kernel, dim3((N + kPairTile - 1) / kPairTile), dim3(256), 0, s, a, b, N, D, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int nomad_cdist_backward_scratch_bytes(int Na, int Nb, size_t* bytes) {
    if (!bytes || Na <= 0 || Nb <= 0) return fail(NOMAD_ERR_INVALID, "nomad_cdist_backward_scratch_bytes: bad argument (Na=%d, Nb=%d)", Na, Nb);
    *bytes = sizeof(double) * (size_t)Na * (size_t)Nb;   // W [Na][Nb]
    return 0;
}

// The backward of nomad_cdist (pairwise.hip.h): the weights W = c / d from the forward's chain, then one ordered reduction per output.
int nomad_cdist_backward(nomad_ctx* c, const float* a, int Na, const float* b, int Nb, int D, const double* gdist, const double* gmean,
                         float* da, float* db, void* scratch, size_t scratch_bytes, nomad_stream_t stream) {
    constexpr int kMaxRows = 65535 * kPairTile;   // one grid row per 64 rows
    if (!c || !a || !b || !scratch || (!gdist && !gmean) || (!da && !db) || Na <= 0 || Nb <= 0 || Na > kMaxRows || Nb > kMaxRows ||
        D <= 0 || D % 4 || D > kCdistMaxD)
        return fail(NOMAD_ERR_INVALID,
                    "nomad_cdist_backward: bad argument (Na=%d, Nb=%d, D=%d: a positive multiple of 4, at most %d; one upstream and one "
                    "output at least)", Na, Nb, D, kCdistMaxD);
    if (scratch_bytes < sizeof(double) * (size_t)Na * (size_t)Nb)
        return fail(NOMAD_ERR_WORKSPACE, "nomad_cdist_backward: scratch of %zu bytes, %zu needed", scratch_bytes,
                    sizeof(double) * (size_t)Na * (size_t)Nb);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scope sc(c, s, NOMAD_K_PAIR, (3.0 + 3.0 * ((da != nullptr) + (db != nullptr))) * D * (double)Na * Nb);
    double* W = static_cast<double*>(scratch);
    const int ta = (Na + kPairTile - 1) / kPairTile, tb = (Nb + kPairTile - 1) / kPairTile, tk = (D + kPairTile - 1) / kPairTile;
    hipLaunchKernelGGL(cdist_weights_kernel, dim3(tb, ta), dim3(256), 0, s, a, Na, b, Nb, D, gdist, gmean, W);
    if (da) hipLaunchKernelGGL(cdist_reduce_kernel<true>, dim3(tk, ta), dim3(256), 0, s, a, Na, b, Nb, D, W, Nb, da);
    if (db) hipLaunchKernelGGL(cdist_reduce_kernel<false>, dim3(tk, tb), dim3(256), 0, s, b, Nb, a, Na, D, W, Nb, db);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- nearest references (pairwise.hip.h: knn_tile_kernel, knn_merge_kernel, knn_scatter_kernel) ----
constexpr int kKnnMaxRows = 65535 * kPairTile;   // nomad_cdist_backward's limit: one grid row per 64 rows

// candidates of every (64-column tile, row): k float64 distances, then k int32 columns
static size_t knn_candidates(int Na, int Nb, int k) { return (size_t)((Nb + kPairTile - 1) / kPairTile) * (size_t)Na * (size_t)k; }

int nomad_knn_scratch_bytes(int Na, int Nb, int k, size_t* bytes) {
    if (!bytes || Na <= 0 || Nb <= 0 || Na > kKnnMaxRows || Nb > kKnnMaxRows || k < 1 || k > kKnnMax || k > Nb)
        return fail(NOMAD_ERR_INVALID, "nomad_knn_scratch_bytes: bad argument (Na=%d, Nb=%d, k=%d: 1 .. min(%d, Nb))", Na, Nb, k, kKnnMax);
    *bytes = knn_candidates(Na, Nb, k) * (sizeof(double) + sizeof(int));
    return 0;
}

int nomad_knn(nomad_ctx* c, const float* a, int Na, const float* b, int Nb, int D, int k, double* dist, double* knn_dist, int* knn_idx,
              double* score, void* scratch, size_t scratch_bytes, nomad_stream_t stream) {
    if (!c || !a || !b || !knn_dist || !knn_idx || !score || !scratch || Na <= 0 || Nb <= 0 || Na > kKnnMaxRows || Nb > kKnnMaxRows ||
        D <= 0 || D % 4 || D > kCdistMaxD || k < 1 || k > kKnnMax || k > Nb)
        return fail(NOMAD_ERR_INVALID,
                    "nomad_knn: bad argument (Na=%d, Nb=%d, D=%d: a positive multiple of 4, at most %d; k=%d: 1 .. min(%d, Nb))", Na, Nb, D,
                    kCdistMaxD, k, kKnnMax);
    const size_t n = knn_candidates(Na, Nb, k);
    if (scratch_bytes < n * (sizeof(double) + sizeof(int)))
        return fail(NOMAD_ERR_WORKSPACE, "nomad_knn: scratch of %zu bytes, %zu needed", scratch_bytes, n * (sizeof(double) + sizeof(int)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scope sc(c, s, NOMAD_K_PAIR, 3.0 * D * (double)Na * Nb);
    double* cand_d = static_cast<double*>(scratch);
    int* cand_i = reinterpret_cast<int*>(cand_d + n);
    const int ta = (Na + kPairTile - 1) / kPairTile, tb = (Nb + kPairTile - 1) / kPairTile;
    if (D == 256)
        hipLaunchKernelGGL(knn_tile_kernel<256>, dim3(tb, ta), dim3(256), 0, s, a, Na, b, Nb, D, k, dist, cand_d, cand_i);
    else
        hipLaunchKernelGGL(knn_tile_kernel<0>, dim3(tb, ta), dim3(256), 0, s, a, Na, b, Nb, D, k, dist, cand_d, cand_i);
    hipLaunchKernelGGL(knn_merge_kernel, dim3((Na + 3) / 4), dim3(256), 0, s, cand_d, cand_i, tb, Na, k, knn_dist, knn_idx, score);
    HIP_TRY(hipGetLastError());
    return 0;
}

int nomad_knn_backward_scratch_bytes(int Na, int Nb, int k, size_t* bytes) {
    if (!bytes || Na <= 0 || Nb <= 0 || Na > kKnnMaxRows || Nb > kKnnMaxRows || k < 1 || k > kKnnMax || k > Nb)
        return fail(NOMAD_ERR_INVALID, "nomad_knn_backward_scratch_bytes: bad argument (Na=%d, Nb=%d, k=%d: 1 .. min(%d, Nb))", Na, Nb, k,
                    kKnnMax);
    *bytes = 2 * sizeof(double) * (size_t)Na * (size_t)Nb;   // the dense upstream G and the weights W, [Na][Nb] each
    return 0;
}

// The backward of nomad_knn: the dense upstream of the selected pairs into the scratch, then nomad_cdist_backward's launches on it.
int nomad_knn_backward(nomad_ctx* c, const float* a, int Na, const float* b, int Nb, int D, int k, const int* knn_idx, const double* g_knn,
                       const double* g_score, float* da, float* db, void* scratch, size_t scratch_bytes, nomad_stream_t stream) {
    if (!c || !a || !b || !knn_idx || !scratch || (!g_knn && !g_score) || (!da && !db) || Na <= 0 || Nb <= 0 || Na > kKnnMaxRows ||
        Nb > kKnnMaxRows || D <= 0 || D % 4 || D > kCdistMaxD || k < 1 || k > kKnnMax || k > Nb)
        return fail(NOMAD_ERR_INVALID,
                    "nomad_knn_backward: bad argument (Na=%d, Nb=%d, D=%d: a positive multiple of 4, at most %d; k=%d: 1 .. min(%d, Nb); one "
                    "upstream and one output at least)", Na, Nb, D, kCdistMaxD, k, kKnnMax);
    const size_t matrix = sizeof(double) * (size_t)Na * (size_t)Nb;
    if (scratch_bytes < 2 * matrix)
        return fail(NOMAD_ERR_WORKSPACE, "nomad_knn_backward: scratch of %zu bytes, %zu needed", scratch_bytes, 2 * matrix);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scope sc(c, s, NOMAD_K_PAIR, (3.0 + 3.0 * ((da != nullptr) + (db != nullptr))) * D * (double)Na * Nb);
    double* G = static_cast<double*>(scratch);
    double* W = G + (size_t)Na * (size_t)Nb;   // not G itself: cdist_weights_kernel takes both as __restrict__
    const int ta = (Na + kPairTile - 1) / kPairTile, tb = (Nb + kPairTile - 1) / kPairTile, tk = (D + kPairTile - 1) / kPairTile;
    hipLaunchKernelGGL(knn_scatter_kernel, dim3(Na), dim3(256), 0, s, knn_idx, g_knn, g_score, Nb, k, G);
    hipLaunchKernelGGL(cdist_weights_kernel, dim3(tb, ta), dim3(256), 0, s, a, Na, b, Nb, D, G, static_cast<const double*>(nullptr), W);
    if (da) hipLaunchKernelGGL(cdist_reduce_kernel<true>, dim3(tk, ta), dim3(256), 0, s, a, Na, b, Nb, D, W, Nb, da);
    if (db) hipLaunchKernelGGL(cdist_reduce_kernel<false>, dim3(tk, tb), dim3(256), 0, s, b, Nb, a, Na, D, W, Nb, db);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- degradations on packed clips (degrade.hip.h) ----
// Scratch: [levels: 2 x 64 float64 | lengths: B int32, to 256 bytes | alpha [B][G] or thresholds [B][G][2] float64, to 256 bytes |
// two key rows of the sort, [B][stride] uint32 each].  One size for both calls (the noise call uses the first three blocks).
struct DegradeLayout {
    size_t lens, stats, keys0, keys1, total;
};
static DegradeLayout degrade_layout(int B, int stride, int G) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    DegradeLayout l;
    l.lens = 2 * kDegradeMaxLevels * sizeof(double);
    l.stats = up(l.lens + sizeof(int) * (size_t)B);
    l.keys0 = up(l.stats + 2 * sizeof(double) * (size_t)B * (size_t)G);
    l.keys1 = l.keys0 + up(sizeof(unsigned) * (size_t)B * (size_t)stride);
    l.total = l.keys1 + up(sizeof(unsigned) * (size_t)B * (size_t)stride);
    return l;
}

size_t nomad_degrade_scratch_bytes(int B, int stride, int G) {
    if (B < 1 || stride < 4 || stride % 4 || G < 1 || G > kDegradeMaxLevels) {
        (void)fail(NOMAD_ERR_INVALID, "nomad_degrade_scratch_bytes: bad argument (B=%d, stride=%d: a positive multiple of 4, G=%d: 1 .. %d)", B,
                   stride, G, kDegradeMaxLevels);
        return 0;
    }
    return degrade_layout(B, stride, G).total;
}

// What both calls check; 0 or a status with the message set.
static int degrade_check(const char* who, nomad_ctx* c, const float* x, int B, int stride, const int* lens, const double* levels, int G,
                         float* out, void* ws, size_t ws_bytes) {
    if (!c || !x || !lens || !levels || !out || !ws) return fail(NOMAD_ERR_INVALID, "%s: a NULL context, input, lengths, levels, output or workspace", who);
    if (G < 1 || G > kDegradeMaxLevels) return fail(NOMAD_ERR_INVALID, "%s: G=%d levels, 1 .. %d are supported", who, G, kDegradeMaxLevels);
    if (B < 1 || B > 65535) return fail(NOMAD_ERR_INVALID, "%s: B=%d clips, 1 .. 65535 are supported", who, B);
    if (stride < 4 || stride % 4) return fail(NOMAD_ERR_INVALID, "%s: stride=%d is not a positive multiple of 4", who, stride);
    for (int b = 0; b < B; ++b)
        if (lens[b] < 1 || lens[b] > stride)
            return fail(NOMAD_ERR_INVALID, "%s: clip %d has length %d, 1 .. stride=%d are supported", who, b, lens[b], stride);
    for (int g = 0; g < G; ++g)
        if (!std::isfinite(levels[g])) return fail(NOMAD_ERR_INVALID, "%s: level %d is not finite", who, g);
    const size_t need = degrade_layout(B, stride, G).total;
    if (ws_bytes < need) return fail(NOMAD_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    return 0;
}

// The per-level factors (2 G float64 at most) and the lengths, staged in the context's ring and copied ahead of the kernels.
static int degrade_upload(nomad_ctx* c, const double* factors, int nf, const int* lens, int B, char* ws, const DegradeLayout& l, hipStream_t s) {
    std::vector<char>& staged = c->degrade_meta_ring[c->degrade_seq++ % 16];
    staged.assign(l.lens + sizeof(int) * (size_t)B, 0);
    memcpy(staged.data(), factors, sizeof(double) * (size_t)nf);
    memcpy(staged.data() + l.lens, lens, sizeof(int) * (size_t)B);
    HIP_TRY(hipMemcpyAsync(ws, staged.data(), staged.size(), hipMemcpyHostToDevice, s));
    return 0;
}

int nomad_degrade_noise(nomad_ctx* c, const float* x, int B, int stride, const int* lens, const float* noise, int noise_len,
                        const double* snr_db, int G, float* out, double* alpha_out, void* ws, size_t ws_bytes, nomad_stream_t stream) {
    if (int rc = degrade_check("nomad_degrade_noise", c, x, B, stride, lens, snr_db, G, out, ws, ws_bytes)) return rc;
    if (!noise || noise_len < 1) return fail(NOMAD_ERR_INVALID, "nomad_degrade_noise: a NULL noise signal or noise_len=%d < 1", noise_len);
    double ratio[kDegradeMaxLevels];
    for (int g = 0; g < G; ++g) ratio[g] = std::pow(10.0, snr_db[g] / 10.0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const DegradeLayout l = degrade_layout(B, stride, G);
    char* w = static_cast<char*>(ws);
    if (int rc = degrade_upload(c, ratio, G, lens, B, w, l, s)) return rc;
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    const double* ratio_dev = reinterpret_cast<const double*>(w);
    const int* lens_dev = reinterpret_cast<const int*>(w + l.lens);
    double* alpha = reinterpret_cast<double*>(w + l.stats);
    hipLaunchKernelGGL(degrade_noise_alpha_kernel, dim3(B), dim3(kDegradeThreads), 0, s, x, stride, lens_dev, noise, noise_len, ratio_dev, G,
                       alpha, alpha_out);
    hipLaunchKernelGGL(degrade_noise_write_kernel, dim3((stride + 255) / 256, B), dim3(256), 0, s, x, stride, lens_dev, noise, noise_len,
                       static_cast<const double*>(alpha), G, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int nomad_degrade_clip(nomad_ctx* c, const float* x, int B, int stride, const int* lens, const double* clip_factor, int G, float* out,
                       double* thresholds_out, void* ws, size_t ws_bytes, nomad_stream_t stream) {
    if (int rc = degrade_check("nomad_degrade_clip", c, x, B, stride, lens, clip_factor, G, out, ws, ws_bytes)) return rc;
    double q[2 * kDegradeMaxLevels];
    for (int g = 0; g < G; ++g) {
        if (clip_factor[g] < 0.0 || clip_factor[g] > 100.0)
            return fail(NOMAD_ERR_INVALID, "nomad_degrade_clip: clip factor %d is %g, outside [0, 100]", g, clip_factor[g]);
        q[2 * g] = (clip_factor[g] / 2) / 100.0;
        q[2 * g + 1] = (100 - clip_factor[g] / 2) / 100.0;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const DegradeLayout l = degrade_layout(B, stride, G);
    char* w = static_cast<char*>(ws);
    if (int rc = degrade_upload(c, q, 2 * G, lens, B, w, l, s)) return rc;
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    const double* q_dev = reinterpret_cast<const double*>(w);
    const int* lens_dev = reinterpret_cast<const int*>(w + l.lens);
    double* thr = reinterpret_cast<double*>(w + l.stats);
    hipLaunchKernelGGL(degrade_sort_kernel, dim3(B), dim3(kDegradeThreads), 0, s, x, stride, lens_dev, reinterpret_cast<unsigned*>(w + l.keys0),
                       reinterpret_cast<unsigned*>(w + l.keys1), q_dev, G, thr, thresholds_out);
    hipLaunchKernelGGL(degrade_clip_write_kernel, dim3((stride + 255) / 256, B), dim3(256), 0, s, x, stride, lens_dev,
                       static_cast<const double*>(thr), G, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- convolution with impulse responses (degrade_convolve.hip.h) ----
// Scratch: [clip lengths: B int32, to 256 bytes | response lengths: G int32, to 256 bytes].
static size_t convolve_lens_bytes(int B) { return (sizeof(int) * (size_t)B + 255) / 256 * 256; }

size_t nomad_degrade_convolve_scratch_bytes(int B, int G) {
    if (B < 1 || B > 65535 || G < 1 || G > kRirMaxResponses) {
        (void)fail(NOMAD_ERR_INVALID, "nomad_degrade_convolve_scratch_bytes: bad argument (B=%d: 1 .. 65535, G=%d: 1 .. %d)", B, G, kRirMaxResponses);
        return 0;
    }
    return convolve_lens_bytes(B) + convolve_lens_bytes(G);
}

int nomad_degrade_convolve(nomad_ctx* c, const float* x, int B, int stride, const int* lens, const float* ir, int G, int ir_stride,
                           const int* ir_lens, float* out, void* ws, size_t ws_bytes, nomad_stream_t stream) {
    const char* who = "nomad_degrade_convolve";
    if (!c || !x || !lens || !ir || !ir_lens || !out || !ws)
        return fail(NOMAD_ERR_INVALID, "%s: a NULL context, input, lengths, responses, response lengths, output or workspace", who);
    if (G < 1 || G > kRirMaxResponses) return fail(NOMAD_ERR_INVALID, "%s: G=%d responses, 1 .. %d are supported", who, G, kRirMaxResponses);
    if (B < 1 || B > 65535) return fail(NOMAD_ERR_INVALID, "%s: B=%d clips, 1 .. 65535 are supported", who, B);
    if (stride < 4 || stride % 4) return fail(NOMAD_ERR_INVALID, "%s: stride=%d is not a positive multiple of 4", who, stride);
    if (ir_stride < 4 || ir_stride % 4) return fail(NOMAD_ERR_INVALID, "%s: ir_stride=%d is not a positive multiple of 4", who, ir_stride);
    for (int b = 0; b < B; ++b)
        if (lens[b] < 1 || lens[b] > stride)
            return fail(NOMAD_ERR_INVALID, "%s: clip %d has length %d, 1 .. stride=%d are supported", who, b, lens[b], stride);
    for (int g = 0; g < G; ++g)
        if (ir_lens[g] < 1 || ir_lens[g] > kRirMaxTaps || ir_lens[g] > ir_stride)
            return fail(NOMAD_ERR_INVALID, "%s: response %d has %d taps, 1 .. min(%d, ir_stride=%d) are supported", who, g, ir_lens[g],
                        kRirMaxTaps, ir_stride);
    const long long tiles = ((long long)stride + kRirTile - 1) / kRirTile;
    if (tiles * B * G > 0x7fffffffLL)
        return fail(NOMAD_ERR_INVALID, "%s: B G ceil(stride / %d) = %lld workgroups, more than one launch holds", who, kRirTile, tiles * B * G);
    const size_t need = convolve_lens_bytes(B) + convolve_lens_bytes(G);
    if (ws_bytes < need) return fail(NOMAD_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(ws);
    // the two length tables, staged in the context's ring and copied ahead of the kernel (as degrade_upload does)
    std::vector<char>& staged = c->degrade_meta_ring[c->degrade_seq++ % 16];
    staged.assign(need, 0);
    memcpy(staged.data(), lens, sizeof(int) * (size_t)B);
    memcpy(staged.data() + convolve_lens_bytes(B), ir_lens, sizeof(int) * (size_t)G);
    HIP_TRY(hipMemcpyAsync(w, staged.data(), need, hipMemcpyHostToDevice, s));
    double flops = 0.0;   // 2 sum_i min(L, i + 1) per row
    for (int b = 0; b < B; ++b)
        for (int g = 0; g < G; ++g) {
            const double m = ir_lens[g] < lens[b] ? ir_lens[g] : lens[b];
            flops += 2.0 * (m * (m + 1) / 2 + ((double)lens[b] - m) * ir_lens[g]);
        }
    Scope sc(c, s, NOMAD_K_ROW, flops);
    hipLaunchKernelGGL(degrade_convolve_kernel, dim3((unsigned)(tiles * B * G)), dim3(kRirThreads), 0, s, x, stride,
                       reinterpret_cast<const int*>(w), ir, ir_stride, reinterpret_cast<const int*>(w + convolve_lens_bytes(B)), G, (int)tiles, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- loudness normalisation of packed rows (loudness.hip.h) ----
// Scratch: [lengths: R int32, to 256 bytes | per chunk (end state, max|x|, sum x^2): [R][C][6] float64 | entry states [R][C][4] |
// sums of y^2 [R][C] | statistics [R][4]], C = ceil(stride / hop) chunks of hop = sample_rate / 10 samples per row.
struct LoudnessLayout {
    int hop, C;
    size_t cs, entry, ysum, stats, total;
};
static LoudnessLayout loudness_layout(int R, int stride, int sample_rate) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    LoudnessLayout l;
    l.hop = sample_rate / 10;
    l.C = (int)(((long long)stride + l.hop - 1) / l.hop);
    const size_t slots = (size_t)R * (size_t)l.C;
    l.cs = up(sizeof(int) * (size_t)R);
    l.entry = l.cs + up(sizeof(double) * kLoudnessChunkStats * slots);
    l.ysum = l.entry + up(sizeof(double) * 4 * slots);
    l.stats = l.ysum + up(sizeof(double) * slots);
    l.total = l.stats + up(sizeof(double) * 4 * (size_t)R);
    return l;
}
static bool loudness_shape_ok(int R, int stride, int sample_rate) {
    return R >= 1 && R <= 65535 && stride >= 4 && stride % 4 == 0 && sample_rate >= 8000 && sample_rate <= 192000 && sample_rate % 10 == 0;
}

size_t nomad_degrade_normalize_scratch_bytes(int R, int stride, int sample_rate) {
    if (!loudness_shape_ok(R, stride, sample_rate)) {
        (void)fail(NOMAD_ERR_INVALID,
                   "nomad_degrade_normalize_scratch_bytes: bad argument (R=%d: 1 .. 65535, stride=%d: a positive multiple of 4, sample_rate=%d: "
                   "a multiple of 10 in 8000 .. 192000)", R, stride, sample_rate);
        return 0;
    }
    return loudness_layout(R, stride, sample_rate).total;
}

int nomad_degrade_normalize(nomad_ctx* c, const float* x, int R, int stride, const int* lens, int sample_rate, int mode, double target,
                            double peak_db, float* out, double* stats_out, void* ws, size_t ws_bytes, nomad_stream_t stream) {
    const char* who = "nomad_degrade_normalize";
    if (!c || !x || !lens || !ws) return fail(NOMAD_ERR_INVALID, "%s: a NULL context, input, lengths or workspace", who);
    if (!out && !stats_out) return fail(NOMAD_ERR_INVALID, "%s: both outputs are NULL: nothing to do", who);
    if (R < 1 || R > 65535) return fail(NOMAD_ERR_INVALID, "%s: R=%d rows, 1 .. 65535 are supported", who, R);
    if (stride < 4 || stride % 4) return fail(NOMAD_ERR_INVALID, "%s: stride=%d is not a positive multiple of 4", who, stride);
    if (sample_rate < 8000 || sample_rate > 192000 || sample_rate % 10)
        return fail(NOMAD_ERR_INVALID, "%s: sample_rate=%d, a multiple of 10 in 8000 .. 192000 is supported", who, sample_rate);
    if (mode < kLoudnessEbu || mode > kLoudnessPeak) return fail(NOMAD_ERR_INVALID, "%s: mode=%d, 0 (ebu), 1 (rms) or 2 (peak)", who, mode);
    if (!std::isfinite(target)) return fail(NOMAD_ERR_INVALID, "%s: the target level is not finite", who);
    for (int r = 0; r < R; ++r)
        if (lens[r] < 1 || lens[r] > stride)
            return fail(NOMAD_ERR_INVALID, "%s: row %d has length %d, 1 .. stride=%d are supported", who, r, lens[r], stride);
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out), bytes = sizeof(float) * (size_t)R * (size_t)stride;
    if (out && oa != xa && oa < xa + bytes && xa < oa + bytes)
        return fail(NOMAD_ERR_INVALID, "%s: the output overlaps the input without being the input (in place: out_dev = x_dev)", who);
    const LoudnessLayout l = loudness_layout(R, stride, sample_rate);
    if (ws_bytes < l.total) return fail(NOMAD_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, l.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(ws);
    std::vector<char>& staged = c->degrade_meta_ring[c->degrade_seq++ % 16];
    staged.assign(sizeof(int) * (size_t)R, 0);
    memcpy(staged.data(), lens, staged.size());
    HIP_TRY(hipMemcpyAsync(w, staged.data(), staged.size(), hipMemcpyHostToDevice, s));
    const LoudnessFilter f = loudness_filter(sample_rate, l.hop);
    const bool ebu = mode == kLoudnessEbu;
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    const int* lens_dev = reinterpret_cast<const int*>(w);
    double* cs = reinterpret_cast<double*>(w + l.cs);
    double* entry = reinterpret_cast<double*>(w + l.entry);
    double* ysum = reinterpret_cast<double*>(w + l.ysum);
    double* stats = reinterpret_cast<double*>(w + l.stats);
    const dim3 chunk_grid((unsigned)((l.C + 63) / 64), (unsigned)R), row_grid((unsigned)((R + 63) / 64));
    hipLaunchKernelGGL(loudness_chunk_kernel<false>, chunk_grid, dim3(64), 0, s, x, stride, lens_dev, l.hop, l.C, f, ebu, cs,
                       static_cast<const double*>(nullptr), static_cast<double*>(nullptr));
    if (ebu) {
        hipLaunchKernelGGL(loudness_carry_kernel, row_grid, dim3(64), 0, s, lens_dev, R, l.hop, l.C, f, static_cast<const double*>(cs), entry);
        hipLaunchKernelGGL(loudness_chunk_kernel<true>, chunk_grid, dim3(64), 0, s, x, stride, lens_dev, l.hop, l.C, f, true,
                           static_cast<double*>(nullptr), static_cast<const double*>(entry), ysum);
    }
    hipLaunchKernelGGL(loudness_gate_kernel, row_grid, dim3(64), 0, s, lens_dev, R, l.hop, l.C, mode, target,
                       std::isnan(peak_db) ? peak_db : std::pow(10.0, peak_db / 20.0), static_cast<const double*>(cs),
                       static_cast<const double*>(ysum), stats, stats_out);
    if (out) {
        const bool wide = (xa | oa) % 16 == 0;
        if (wide)
            hipLaunchKernelGGL(loudness_gain_kernel<4>, dim3((unsigned)((stride / 4 + 255) / 256), (unsigned)R), dim3(256), 0, s, x, stride,
                               lens_dev, static_cast<const double*>(stats), out);
        else
            hipLaunchKernelGGL(loudness_gain_kernel<1>, dim3((unsigned)((stride + 255) / 256), (unsigned)R), dim3(256), 0, s, x, stride,
                               lens_dev, static_cast<const double*>(stats), out);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- sox-style reverb: comb and all-pass recurrences (reverb.hip.h) ----
// Scratch: [lengths: B int32, to 256 bytes | feedback: G float64, to 256 bytes | wet [2][B G][stride] float64].
struct ReverbLayout {
    size_t feedback, wet, plane, total;   // plane: doubles per channel
};
static ReverbLayout reverb_layout(int B, int stride, int G) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    ReverbLayout l;
    l.feedback = up(sizeof(int) * (size_t)B);
    l.wet = l.feedback + up(sizeof(double) * (size_t)G);
    l.plane = (size_t)B * (size_t)G * (size_t)stride;
    l.total = l.wet + 2 * sizeof(double) * l.plane;
    return l;
}
static bool reverb_shape_ok(int B, int stride, int G, int sample_rate) {
    return B >= 1 && B <= 65535 && G >= 1 && G <= kReverbMaxLevels && stride >= 4 && stride % 4 == 0 && sample_rate >= 8000 &&
           sample_rate <= 48000;
}

size_t nomad_degrade_reverb_scratch_bytes(int B, int stride, int G, int sample_rate) {
    if (!reverb_shape_ok(B, stride, G, sample_rate)) {
        (void)fail(NOMAD_ERR_INVALID,
                   "nomad_degrade_reverb_scratch_bytes: bad argument (B=%d: 1 .. 65535, stride=%d: a positive multiple of 4, G=%d: 1 .. %d, "
                   "sample_rate=%d: 8000 .. 48000)", B, stride, G, kReverbMaxLevels, sample_rate);
        return 0;
    }
    return reverb_layout(B, stride, G).total;
}

int nomad_degrade_reverb(nomad_ctx* c, const float* x, int B, int stride, const int* lens, const nomad_reverb_params* params, float* out,
                         void* ws, size_t ws_bytes, nomad_stream_t stream) {
    const char* who = "nomad_degrade_reverb";
    if (!c || !x || !lens || !params || !out || !ws)
        return fail(NOMAD_ERR_INVALID, "%s: a NULL context, input, lengths, parameters, output or workspace", who);
    const nomad_reverb_params q = *params;   // the caller's struct is read here and never again
    const int G = q.G;
    if (G < 1 || G > kReverbMaxLevels) return fail(NOMAD_ERR_INVALID, "%s: G=%d levels, 1 .. %d are supported", who, G, kReverbMaxLevels);
    if (B < 1 || B > 65535) return fail(NOMAD_ERR_INVALID, "%s: B=%d clips, 1 .. 65535 are supported", who, B);
    if (stride < 4 || stride % 4) return fail(NOMAD_ERR_INVALID, "%s: stride=%d is not a positive multiple of 4", who, stride);
    if (q.sample_rate < 8000 || q.sample_rate > 48000)
        return fail(NOMAD_ERR_INVALID, "%s: sample_rate=%d, 8000 .. 48000 is supported", who, q.sample_rate);
    auto in_range = [](double v, double lo, double hi) { return std::isfinite(v) && v >= lo && v <= hi; };
    for (int g = 0; g < G; ++g)
        if (!in_range(q.reverberance[g], 0.0, 100.0))
            return fail(NOMAD_ERR_INVALID, "%s: reverberance[%d]=%g, 0 .. 100 is supported", who, g, q.reverberance[g]);
    if (!in_range(q.hf_damping, 0.0, 100.0) || !in_range(q.room_scale, 0.0, 100.0) || !in_range(q.stereo_depth, 0.0, 100.0))
        return fail(NOMAD_ERR_INVALID, "%s: hf_damping=%g, room_scale=%g, stereo_depth=%g: each 0 .. 100", who, q.hf_damping, q.room_scale,
                    q.stereo_depth);
    if (!in_range(q.pre_delay_ms, 0.0, 500.0)) return fail(NOMAD_ERR_INVALID, "%s: pre_delay_ms=%g, 0 .. 500 is supported", who, q.pre_delay_ms);
    if (!in_range(q.wet_gain_db, -10.0, 10.0)) return fail(NOMAD_ERR_INVALID, "%s: wet_gain_db=%g, -10 .. 10 is supported", who, q.wet_gain_db);
    if ((q.wet_only != 0 && q.wet_only != 1) || (q.clamp != 0 && q.clamp != 1))
        return fail(NOMAD_ERR_INVALID, "%s: wet_only=%d and clamp=%d are 0 or 1", who, q.wet_only, q.clamp);
    for (int b = 0; b < B; ++b)
        if (lens[b] < 1 || lens[b] > stride)
            return fail(NOMAD_ERR_INVALID, "%s: clip %d has length %d, 1 .. stride=%d are supported", who, b, lens[b], stride);
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
    const uintptr_t xbytes = sizeof(float) * (size_t)B * (size_t)stride, obytes = xbytes * (size_t)G;
    if (oa < xa + xbytes && xa < oa + obytes) return fail(NOMAD_ERR_INVALID, "%s: the output overlaps the input", who);
    const ReverbPlan plan = reverb_plan(q.hf_damping, q.room_scale, q.stereo_depth, q.pre_delay_ms, q.wet_gain_db, q.wet_only, q.clamp, q.sample_rate);
    const size_t lds = sizeof(double) * (size_t)plan.lds_doubles;
    if (plan.tile < 1 || lds > kReverbLdsMax)
        return fail(NOMAD_ERR_INVALID, "%s: delays from %d samples, %zu bytes of delay lines: outside what a workgroup holds", who, plan.tile, lds);
    const ReverbLayout l = reverb_layout(B, stride, G);
    if (ws_bytes < l.total) return fail(NOMAD_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, l.total);
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(reverb_wet_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(ws);
    // the lengths and the levels' feedback, staged in the context's ring and copied ahead of the kernels
    std::vector<char>& staged = c->degrade_meta_ring[c->degrade_seq++ % 16];
    staged.assign(l.wet, 0);
    memcpy(staged.data(), lens, sizeof(int) * (size_t)B);
    double* fb = reinterpret_cast<double*>(staged.data() + l.feedback);
    for (int g = 0; g < G; ++g) fb[g] = reverb_feedback(q.reverberance[g]);
    HIP_TRY(hipMemcpyAsync(w, staged.data(), l.wet, hipMemcpyHostToDevice, s));
    double samples = 0.0;
    for (int b = 0; b < B; ++b) samples += lens[b];
    Scope sc(c, s, NOMAD_K_ROW, samples * G * plan.channels * (kReverbCombs * 7.0 + kReverbAllpass * 3.0 + 1.0));
    const int* lens_dev = reinterpret_cast<const int*>(w);
    double* wet = reinterpret_cast<double*>(w + l.wet);
    hipLaunchKernelGGL(reverb_wet_kernel, dim3((unsigned)(B * G), (unsigned)plan.channels), dim3(kReverbThreads), lds, s, x, stride, lens_dev,
                       reinterpret_cast<const double*>(w + l.feedback), G, plan, wet);
    hipLaunchKernelGGL(reverb_mix_kernel, dim3((unsigned)(B * G)), dim3(256), 0, s, x, stride, lens_dev, G, static_cast<const double*>(wet),
                       l.plane, plan, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- gammatone spectrograms and NSIM (nsim.hip.h) ----
int nomad_gammatone_frames(int n_samples, int sample_rate) {
    if (!gammatone_rate_ok(sample_rate)) return 0;
    const int H = sample_rate / 50, W = 4 * H;
    return n_samples < W ? 0 : (n_samples - W) / H + 1;
}

// Scratch: [lengths: R int32, to 256 bytes | frame prefix sums: R + 1 int64, to 256 bytes | the bank: [21][10] float64].
struct GammatoneLayout {
    size_t fpref, coef, total;
};
static GammatoneLayout gammatone_layout(int R) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    GammatoneLayout l;
    l.fpref = up(sizeof(int) * (size_t)R);
    l.coef = l.fpref + up(sizeof(long long) * ((size_t)R + 1));
    l.total = l.coef + up(sizeof(double) * kGammatoneCoefs * kGammatoneBands);
    return l;
}

size_t nomad_gammatone_scratch_bytes(int R, int stride, int sample_rate) {
    if (R < 1 || R > 65535 || stride < 4 || stride % 4 || !gammatone_rate_ok(sample_rate)) {
        (void)fail(NOMAD_ERR_INVALID,
                   "nomad_gammatone_scratch_bytes: bad argument (R=%d: 1 .. 65535, stride=%d: a positive multiple of 4, sample_rate=%d: a multiple "
                   "of 50 in %d .. %d)", R, stride, sample_rate, kGammatoneMinRate, kGammatoneMaxRate);
        return 0;
    }
    return gammatone_layout(R).total;
}

int nomad_gammatone(nomad_ctx* c, const float* x, int R, int stride, const int* lens, int sample_rate, double* spec, void* ws,
                    size_t ws_bytes, nomad_stream_t stream) {
    const char* who = "nomad_gammatone";
    if (!c || !x || !lens || !spec || !ws) return fail(NOMAD_ERR_INVALID, "%s: a NULL context, input, lengths, output or workspace", who);
    if (R < 1 || R > 65535) return fail(NOMAD_ERR_INVALID, "%s: R=%d rows, 1 .. 65535 are supported", who, R);
    if (stride < 4 || stride % 4) return fail(NOMAD_ERR_INVALID, "%s: stride=%d is not a positive multiple of 4", who, stride);
    if (!gammatone_rate_ok(sample_rate))
        return fail(NOMAD_ERR_INVALID, "%s: sample_rate=%d, a multiple of 50 in %d .. %d is supported", who, sample_rate, kGammatoneMinRate,
                    kGammatoneMaxRate);
    const int H = sample_rate / 50, W = 4 * H;
    int max_f = 0;
    for (int r = 0; r < R; ++r) {
        if (lens[r] < W || lens[r] > stride)
            return fail(NOMAD_ERR_INVALID, "%s: row %d has length %d, one frame of %d samples .. stride=%d are supported", who, r, lens[r], W, stride);
        const int f = (lens[r] - W) / H + 1;
        max_f = f > max_f ? f : max_f;
    }
    const GammatoneLayout l = gammatone_layout(R);
    if (ws_bytes < l.total) return fail(NOMAD_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, l.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(ws);
    std::vector<char>& staged = c->degrade_meta_ring[c->degrade_seq++ % 16];
    staged.assign(l.total, 0);
    memcpy(staged.data(), lens, sizeof(int) * (size_t)R);
    long long* fp = reinterpret_cast<long long*>(staged.data() + l.fpref);
    for (int r = 0; r < R; ++r) fp[r + 1] = fp[r] + ((lens[r] - W) / H + 1);
    const double frames = (double)fp[R];
    gammatone_bank(sample_rate, reinterpret_cast<double*>(staged.data() + l.coef), nullptr);
    HIP_TRY(hipMemcpyAsync(w, staged.data(), l.total, hipMemcpyHostToDevice, s));
    Scope sc(c, s, NOMAD_K_ROW, 2.0 * 16.0 * frames * kGammatoneBands * W);
    const size_t lds = sizeof(float) * (size_t)(kGammatoneBlockFrames + 3) * (size_t)(H + 1);   // at most 57 660 bytes (48 kHz)
    hipLaunchKernelGGL(gammatone_frames_kernel, dim3((unsigned)((max_f + kGammatoneBlockFrames - 1) / kGammatoneBlockFrames), (unsigned)R),
                       dim3(256), lds, s, x, stride, reinterpret_cast<const int*>(w), reinterpret_cast<const long long*>(w + l.fpref),
                       reinterpret_cast<const double*>(w + l.coef), H, spec);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Scratch: [frames: B int32, to 256 bytes | frame prefix sums: B + 1 int64, to 256 bytes | planes [3][G total_frames][21] float64].
struct NsimLayout {
    size_t fpref, planes, total;
};
static NsimLayout nsim_layout(int B, int G, long long total_frames) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    NsimLayout l;
    l.fpref = up(sizeof(int) * (size_t)B);
    l.planes = l.fpref + up(sizeof(long long) * ((size_t)B + 1));
    l.total = l.planes + 3 * sizeof(double) * (size_t)G * (size_t)total_frames * kGammatoneBands;
    return l;
}

size_t nomad_nsim_scratch_bytes(int B, int G, long long total_frames) {
    if (B < 1 || B > 65535 || G < 1 || G > 64 || total_frames < B || total_frames > (1ll << 31)) {
        (void)fail(NOMAD_ERR_INVALID, "nomad_nsim_scratch_bytes: bad argument (B=%d: 1 .. 65535, G=%d: 1 .. 64, total_frames=%lld: B .. 2^31)", B, G,
                   total_frames);
        return 0;
    }
    return nsim_layout(B, G, total_frames).total;
}

int nomad_nsim(nomad_ctx* c, const double* spec_ref, const double* spec_deg, int B, int G, const int* frames, double intensity_range,
               double* nsim_out, double* bands_out, void* ws, size_t ws_bytes, nomad_stream_t stream) {
    const char* who = "nomad_nsim";
    if (!c || !spec_ref || !spec_deg || !frames || !nsim_out || !ws)
        return fail(NOMAD_ERR_INVALID, "%s: a NULL context, spectrogram, frame counts, output or workspace", who);
    if (B < 1 || B > 65535) return fail(NOMAD_ERR_INVALID, "%s: B=%d clips, 1 .. 65535 are supported", who, B);
    if (G < 1 || G > 64) return fail(NOMAD_ERR_INVALID, "%s: G=%d rows per clip, 1 .. 64 are supported", who, G);
    if (!std::isfinite(intensity_range) || !(intensity_range > 0.0))
        return fail(NOMAD_ERR_INVALID, "%s: the intensity range must be finite and positive, got %g", who, intensity_range);
    long long total = 0;
    for (int b = 0; b < B; ++b) {
        if (frames[b] < 1) return fail(NOMAD_ERR_INVALID, "%s: clip %d has %d frames, at least 1 is needed", who, b, frames[b]);
        total += frames[b];
    }
    if (total > (1ll << 31)) return fail(NOMAD_ERR_INVALID, "%s: %lld frames in all, at most 2^31 are supported", who, total);
    const NsimLayout l = nsim_layout(B, G, total);
    if (ws_bytes < l.total) return fail(NOMAD_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, l.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(ws);
    std::vector<char>& staged = c->degrade_meta_ring[c->degrade_seq++ % 16];
    staged.assign(l.planes, 0);
    memcpy(staged.data(), frames, sizeof(int) * (size_t)B);
    long long* fp = reinterpret_cast<long long*>(staged.data() + l.fpref);
    for (int b = 0; b < B; ++b) fp[b + 1] = fp[b] + frames[b];
    HIP_TRY(hipMemcpyAsync(w, staged.data(), l.planes, hipMemcpyHostToDevice, s));
    const double C1 = (0.01 * intensity_range) * (0.01 * intensity_range), C3 = (0.03 * intensity_range) * (0.03 * intensity_range) / 2.0;
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(nsim_kernel, dim3((unsigned)(B * G)), dim3(256), 0, s, spec_ref, spec_deg, G, reinterpret_cast<const int*>(w),
                       reinterpret_cast<const long long*>(w + l.fpref), total, C1, C3, reinterpret_cast<double*>(w + l.planes), nsim_out, bands_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- NSIM as a loss (nsim_bwd.hip.h) ----
// Scratch: nomad_gammatone's three tables, then y: [R F(stride)][W][21] float64, F(stride) the whole frames of a row as long as
// the stride (the helper does not know the lengths; the call uses the rows' own frame counts, packed).
static size_t gammatone_backward_y_bytes(long long frames, int W) { return sizeof(double) * (size_t)frames * (size_t)W * kGammatoneBands; }

size_t nomad_gammatone_backward_scratch_bytes(int R, int stride, int sample_rate) {
    const int W = gammatone_rate_ok(sample_rate) ? sample_rate / 50 * 4 : 0;
    if (R < 1 || R > 65535 || stride < 4 || stride % 4 || !W || stride < W) {
        (void)fail(NOMAD_ERR_INVALID,
                   "nomad_gammatone_backward_scratch_bytes: bad argument (R=%d: 1 .. 65535, stride=%d: a positive multiple of 4 and at least one "
                   "frame, sample_rate=%d: a multiple of 50 in %d .. %d)", R, stride, sample_rate, kGammatoneMinRate, kGammatoneMaxRate);
        return 0;
    }
    return gammatone_layout(R).total + gammatone_backward_y_bytes((long long)R * nomad_gammatone_frames(stride, sample_rate), W);
}

int nomad_gammatone_backward(nomad_ctx* c, const float* x, int R, int stride, const int* lens, int sample_rate, const double* dspec, float* dx,
                             void* ws, size_t ws_bytes, nomad_stream_t stream) {
    const char* who = "nomad_gammatone_backward";
    if (!c || !x || !lens || !dspec || !dx || !ws)
        return fail(NOMAD_ERR_INVALID, "%s: a NULL context, input, lengths, spectrogram gradient, output or workspace", who);
    if (R < 1 || R > 65535) return fail(NOMAD_ERR_INVALID, "%s: R=%d rows, 1 .. 65535 are supported", who, R);
    if (stride < 4 || stride % 4) return fail(NOMAD_ERR_INVALID, "%s: stride=%d is not a positive multiple of 4", who, stride);
    if (!gammatone_rate_ok(sample_rate))
        return fail(NOMAD_ERR_INVALID, "%s: sample_rate=%d, a multiple of 50 in %d .. %d is supported", who, sample_rate, kGammatoneMinRate,
                    kGammatoneMaxRate);
    const int H = sample_rate / 50, W = 4 * H;
    int max_f = 0;
    for (int r = 0; r < R; ++r) {
        if (lens[r] < W || lens[r] > stride)
            return fail(NOMAD_ERR_INVALID, "%s: row %d has length %d, one frame of %d samples .. stride=%d are supported", who, r, lens[r], W, stride);
        const int f = (lens[r] - W) / H + 1;
        max_f = f > max_f ? f : max_f;
    }
    const GammatoneLayout l = gammatone_layout(R);
    const size_t need = l.total + gammatone_backward_y_bytes((long long)R * nomad_gammatone_frames(stride, sample_rate), W);
    if (ws_bytes < need) return fail(NOMAD_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(ws);
    std::vector<char>& staged = c->degrade_meta_ring[c->degrade_seq++ % 16];
    staged.assign(l.total, 0);
    memcpy(staged.data(), lens, sizeof(int) * (size_t)R);
    long long* fp = reinterpret_cast<long long*>(staged.data() + l.fpref);
    for (int r = 0; r < R; ++r) fp[r + 1] = fp[r] + ((lens[r] - W) / H + 1);
    const double frames = (double)fp[R];
    gammatone_bank(sample_rate, reinterpret_cast<double*>(staged.data() + l.coef), nullptr);
    HIP_TRY(hipMemcpyAsync(w, staged.data(), l.total, hipMemcpyHostToDevice, s));
    Scope sc(c, s, NOMAD_K_ROW, 2.0 * 2.0 * 16.0 * frames * kGammatoneBands * W);
    const size_t lds = sizeof(float) * (size_t)(kGammatoneBlockFrames + 3) * (size_t)(H + 1);   // the forward's: at most 57 660 bytes (48 kHz)
    const int* lens_dev = reinterpret_cast<const int*>(w);
    const long long* fpref_dev = reinterpret_cast<const long long*>(w + l.fpref);
    double* y = reinterpret_cast<double*>(w + l.total);
    hipLaunchKernelGGL(gammatone_adjoint_kernel, dim3((unsigned)((max_f + kGammatoneBlockFrames - 1) / kGammatoneBlockFrames), (unsigned)R),
                       dim3(256), lds, s, x, stride, lens_dev, fpref_dev, reinterpret_cast<const double*>(w + l.coef), H, dspec, y);
    hipLaunchKernelGGL(gammatone_gather_kernel, dim3((unsigned)((stride + 255) / 256), (unsigned)R), dim3(256), 0, s,
                       static_cast<const double*>(y), stride, lens_dev, fpref_dev, H, dx);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Scratch: nomad_nsim's two tables, then planes [9][G total_frames][21] float64.
static NsimLayout nsim_backward_layout(int B, int G, long long total_frames) {
    NsimLayout l = nsim_layout(B, G, total_frames);
    l.total = l.planes + kNsimBwdPlanes * sizeof(double) * (size_t)G * (size_t)total_frames * kGammatoneBands;
    return l;
}

size_t nomad_nsim_backward_scratch_bytes(int B, int G, long long total_frames) {
    if (B < 1 || B > 65535 || G < 1 || G > 64 || total_frames < B || total_frames > (1ll << 31)) {
        (void)fail(NOMAD_ERR_INVALID, "nomad_nsim_backward_scratch_bytes: bad argument (B=%d: 1 .. 65535, G=%d: 1 .. 64, total_frames=%lld: B .. 2^31)",
                   B, G, total_frames);
        return 0;
    }
    return nsim_backward_layout(B, G, total_frames).total;
}

int nomad_nsim_backward(nomad_ctx* c, const double* spec_ref, const double* spec_deg, int B, int G, const int* frames, double intensity_range,
                        const double* grad_nsim, double* dspec_deg_out, void* ws, size_t ws_bytes, nomad_stream_t stream) {
    const char* who = "nomad_nsim_backward";
    if (!c || !spec_ref || !spec_deg || !frames || !grad_nsim || !dspec_deg_out || !ws)
        return fail(NOMAD_ERR_INVALID, "%s: a NULL context, spectrogram, frame counts, gradient, output or workspace", who);
    if (B < 1 || B > 65535) return fail(NOMAD_ERR_INVALID, "%s: B=%d clips, 1 .. 65535 are supported", who, B);
    if (G < 1 || G > 64) return fail(NOMAD_ERR_INVALID, "%s: G=%d rows per clip, 1 .. 64 are supported", who, G);
    if (!std::isfinite(intensity_range) || !(intensity_range > 0.0))
        return fail(NOMAD_ERR_INVALID, "%s: the intensity range must be finite and positive, got %g", who, intensity_range);
    long long total = 0;
    for (int b = 0; b < B; ++b) {
        if (frames[b] < 1) return fail(NOMAD_ERR_INVALID, "%s: clip %d has %d frames, at least 1 is needed", who, b, frames[b]);
        total += frames[b];
    }
    if (total > (1ll << 31)) return fail(NOMAD_ERR_INVALID, "%s: %lld frames in all, at most 2^31 are supported", who, total);
    const NsimLayout l = nsim_backward_layout(B, G, total);
    if (ws_bytes < l.total) return fail(NOMAD_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, l.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(ws);
    std::vector<char>& staged = c->degrade_meta_ring[c->degrade_seq++ % 16];
    staged.assign(l.planes, 0);
    memcpy(staged.data(), frames, sizeof(int) * (size_t)B);
    long long* fp = reinterpret_cast<long long*>(staged.data() + l.fpref);
    for (int b = 0; b < B; ++b) fp[b + 1] = fp[b] + frames[b];
    HIP_TRY(hipMemcpyAsync(w, staged.data(), l.planes, hipMemcpyHostToDevice, s));
    const double C1 = (0.01 * intensity_range) * (0.01 * intensity_range), C3 = (0.03 * intensity_range) * (0.03 * intensity_range) / 2.0;
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(nsim_backward_kernel, dim3((unsigned)(B * G)), dim3(256), 0, s, spec_ref, spec_deg, G, reinterpret_cast<const int*>(w),
                       reinterpret_cast<const long long*>(w + l.fpref), total, C1, C3, grad_nsim, reinterpret_cast<double*>(w + l.planes),
                       dspec_deg_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- patch-wise NSIM (nsim_patches.hip.h) ----
int nomad_nsim_patch_count(int frames, int patch) { return frames < 1 || patch < 1 || patch > kPatchMax ? 0 : frames / patch; }

// Scratch, every part rounded up to 256 bytes: [clean frame counts: B int32 | degraded frame counts: B G int32 | clean frame prefix
// sums: B + 1 int64 | degraded frame prefix sums: B G + 1 int64 | patch prefix sums: B + 1 int64 || E: total_ref float64 |
// activity: total_ref int32 | kept: TP int32 | clipbad: B int32 | candidates [G TP][2 search + 1] float64 | back-pointers
// [G TP][2 search + 1] int32 | link, pick: [G TP] int32 each].  TP = the patches of all clean clips; the size helper takes its
// bound total_ref / patch.  The parts ahead of || come from the host.
struct PatchLayout {
    size_t dframes, fpref, dpref, ppref, E, active, kept, clipbad, cand, back, link, pick, total;
};
static PatchLayout patch_layout(int B, int G, long long total_ref, long long TP, int search) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t R = (size_t)B * (size_t)G, places = 2 * (size_t)search + 1, rp = (size_t)G * (size_t)(TP < 1 ? 1 : TP);
    PatchLayout l;
    l.dframes = up(sizeof(int) * (size_t)B);
    l.fpref = l.dframes + up(sizeof(int) * R);
    l.dpref = l.fpref + up(sizeof(long long) * ((size_t)B + 1));
    l.ppref = l.dpref + up(sizeof(long long) * (R + 1));
    l.E = l.ppref + up(sizeof(long long) * ((size_t)B + 1));
    l.active = l.E + up(sizeof(double) * (size_t)total_ref);
    l.kept = l.active + up(sizeof(int) * (size_t)total_ref);
    l.clipbad = l.kept + up(sizeof(int) * (size_t)(TP < 1 ? 1 : TP));
    l.cand = l.clipbad + up(sizeof(int) * (size_t)B);
    l.back = l.cand + up(sizeof(double) * rp * places);
    l.link = l.back + up(sizeof(int) * rp * places);
    l.pick = l.link + up(sizeof(int) * rp);
    l.total = l.pick + up(sizeof(int) * rp);
    return l;
}
constexpr long long kPatchMaxFrames = 1ll << 31;

size_t nomad_nsim_patches_scratch_bytes(int B, int G, long long total_ref_frames, long long total_deg_frames, int patch, int search) {
    if (B < 1 || B > 65535 || G < 1 || G > 64 || total_ref_frames < B || total_ref_frames > kPatchMaxFrames ||
        total_deg_frames < (long long)B * G || total_deg_frames > 64 * kPatchMaxFrames || patch < 1 || patch > kPatchMax || search < 0 ||
        search > kPatchSearchMax) {
        (void)fail(NOMAD_ERR_INVALID,
                   "nomad_nsim_patches_scratch_bytes: bad argument (B=%d: 1 .. 65535, G=%d: 1 .. 64, total_ref_frames=%lld: B .. 2^31, "
                   "total_deg_frames=%lld: B G .. 2^37, patch=%d: 1 .. %d, search=%d: 0 .. %d)", B, G, total_ref_frames, total_deg_frames, patch,
                   kPatchMax, search, kPatchSearchMax);
        return 0;
    }
    return patch_layout(B, G, total_ref_frames, total_ref_frames / patch, search).total;
}

int nomad_nsim_patches(nomad_ctx* c, const double* spec_ref, const double* spec_deg, int B, int G, const int* frames, const int* deg_frames,
                       int patch, int search, double vad_ratio, int min_active_frames, double intensity_range, int out_patches,
                       double* nsim_out, double* bands_out, int* offsets_out, double* patch_nsim_out, double* cand_out, void* ws,
                       size_t ws_bytes, nomad_stream_t stream) {
    const char* who = "nomad_nsim_patches";
    if (!c || !spec_ref || !spec_deg || !frames || !deg_frames || !nsim_out || !ws)
        return fail(NOMAD_ERR_INVALID, "%s: a NULL context, spectrogram, frame counts, output or workspace", who);
    if (B < 1 || B > 65535) return fail(NOMAD_ERR_INVALID, "%s: B=%d clips, 1 .. 65535 are supported", who, B);
    if (G < 1 || G > 64) return fail(NOMAD_ERR_INVALID, "%s: G=%d rows per clip, 1 .. 64 are supported", who, G);
    if (patch < 1 || patch > kPatchMax) return fail(NOMAD_ERR_INVALID, "%s: patch=%d frames, 1 .. %d are supported", who, patch, kPatchMax);
    if (search < 0 || search > kPatchSearchMax)
        return fail(NOMAD_ERR_INVALID, "%s: search=%d frames, 0 .. %d are supported", who, search, kPatchSearchMax);
    if (!(vad_ratio > 0.0 && vad_ratio <= 1.0)) return fail(NOMAD_ERR_INVALID, "%s: vad_ratio=%g, a value in (0, 1] is needed", who, vad_ratio);
    if (min_active_frames < 1 || min_active_frames > patch)
        return fail(NOMAD_ERR_INVALID, "%s: min_active_frames=%d, 1 .. patch=%d are supported", who, min_active_frames, patch);
    if (!std::isfinite(intensity_range) || !(intensity_range > 0.0))
        return fail(NOMAD_ERR_INVALID, "%s: the intensity range must be finite and positive, got %g", who, intensity_range);
    const long long R = (long long)B * G;
    long long total = 0, dtotal = 0, TP = 0;
    int maxP = 0;
    for (int b = 0; b < B; ++b) {
        if (frames[b] < 1) return fail(NOMAD_ERR_INVALID, "%s: clip %d has %d frames, at least 1 is needed", who, b, frames[b]);
        total += frames[b];
        TP += frames[b] / patch;
        maxP = frames[b] / patch > maxP ? frames[b] / patch : maxP;
    }
    for (long long r = 0; r < R; ++r) {
        if (deg_frames[r] < 1) return fail(NOMAD_ERR_INVALID, "%s: degraded row %lld has %d frames, at least 1 is needed", who, r, deg_frames[r]);
        dtotal += deg_frames[r];
    }
    if (total > kPatchMaxFrames || dtotal > 64 * kPatchMaxFrames)
        return fail(NOMAD_ERR_INVALID, "%s: %lld clean and %lld degraded frames in all, at most 2^31 and 2^37 are supported", who, total, dtotal);
    if (out_patches < 1 || out_patches < maxP)
        return fail(NOMAD_ERR_INVALID, "%s: out_patches=%d, at least 1 and the %d patches of the longest clip are needed", who, out_patches, maxP);
    if (R * (long long)(maxP < 1 ? 1 : maxP) > 0x7fffffffLL)
        return fail(NOMAD_ERR_INVALID, "%s: %lld workgroups, more than one launch holds", who, R * (long long)maxP);
    const PatchLayout l = patch_layout(B, G, total, TP, search);
    if (ws_bytes < l.total) return fail(NOMAD_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, l.total);
    int W = 4;
    size_t lds = sizeof(double) * (patch_staged_doubles(patch, search) + (size_t)W * patch_wave_doubles(patch));
    if (lds > kPatchLdsMax) {
        W = 2;
        lds = sizeof(double) * (patch_staged_doubles(patch, search) + (size_t)W * patch_wave_doubles(patch));
    }
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(patch_candidates_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const size_t sel_lds = sizeof(double) * ((size_t)(2 * kGammatoneBands + 2) * (size_t)patch + patch_wave_doubles(patch));
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(ws);
    std::vector<char>& staged = c->degrade_meta_ring[c->degrade_seq++ % 16];
    staged.assign(l.E, 0);
    memcpy(staged.data(), frames, sizeof(int) * (size_t)B);
    memcpy(staged.data() + l.dframes, deg_frames, sizeof(int) * (size_t)R);
    long long* fp = reinterpret_cast<long long*>(staged.data() + l.fpref);
    long long* dp = reinterpret_cast<long long*>(staged.data() + l.dpref);
    long long* pp = reinterpret_cast<long long*>(staged.data() + l.ppref);
    for (int b = 0; b < B; ++b) {
        fp[b + 1] = fp[b] + frames[b];
        pp[b + 1] = pp[b] + frames[b] / patch;
    }
    for (long long r = 0; r < R; ++r) dp[r + 1] = dp[r] + deg_frames[r];
    HIP_TRY(hipMemcpyAsync(w, staged.data(), l.E, hipMemcpyHostToDevice, s));
    const double C1 = (0.01 * intensity_range) * (0.01 * intensity_range), C3 = (0.03 * intensity_range) * (0.03 * intensity_range) / 2.0;
    PatchTables tb;
    tb.frames = reinterpret_cast<const int*>(w);
    tb.dframes = reinterpret_cast<const int*>(w + l.dframes);
    tb.fpref = reinterpret_cast<const long long*>(w + l.fpref);
    tb.dpref = reinterpret_cast<const long long*>(w + l.dpref);
    tb.ppref = reinterpret_cast<const long long*>(w + l.ppref);
    tb.kept = reinterpret_cast<const int*>(w + l.kept);
    tb.clipbad = reinterpret_cast<const int*>(w + l.clipbad);
    double* cand = reinterpret_cast<double*>(w + l.cand);
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(patch_activity_kernel, dim3((unsigned)B), dim3(256), 0, s, spec_ref, tb.frames, tb.fpref, tb.ppref, patch, vad_ratio,
                       min_active_frames, reinterpret_cast<double*>(w + l.E), reinterpret_cast<int*>(w + l.active),
                       reinterpret_cast<int*>(w + l.kept), reinterpret_cast<int*>(w + l.clipbad));
    if (maxP > 0)
        hipLaunchKernelGGL(patch_candidates_kernel, dim3((unsigned)(R * maxP)), dim3(64 * W), lds, s, spec_ref, spec_deg, G, tb, patch, search,
                           maxP, C1, C3, cand);
    hipLaunchKernelGGL(patch_select_kernel, dim3((unsigned)R), dim3(256), sel_lds, s, spec_ref, spec_deg, G, tb, patch, search, C1, C3,
                       static_cast<const double*>(cand), reinterpret_cast<int*>(w + l.back), reinterpret_cast<int*>(w + l.link),
                       reinterpret_cast<int*>(w + l.pick), out_patches, nsim_out, bands_out, offsets_out, patch_nsim_out, cand_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- time alignment: delay search and shift (align.hip.h) ----
// Scratch: [clean lengths: B int32, to 256 bytes | degraded lengths: B G int32, to 256 bytes | parts [B G][pmax][2 D + 1] float64],
// pmax = the parts of a clip as long as the stride.  nomad_align_shift uses the front of it: [degraded lengths | output lengths].
struct AlignLayout {
    int pmax;
    size_t dlens, parts, total;
};
static size_t align_lens_bytes(long long rows) { return (sizeof(int) * (size_t)rows + 255) / 256 * 256; }
static AlignLayout align_layout(int B, int G, int stride, int max_delay) {
    AlignLayout l;
    l.pmax = align_parts(stride);
    l.dlens = align_lens_bytes(B);
    l.parts = l.dlens + align_lens_bytes((long long)B * G);
    l.total = l.parts + sizeof(double) * (size_t)B * (size_t)G * (size_t)l.pmax * (size_t)(2 * max_delay + 1);
    const size_t shift = 2 * align_lens_bytes((long long)B * G);
    l.total = l.total < shift ? shift : l.total;
    return l;
}
constexpr int kAlignMaxStride = 1 << 30;

size_t nomad_align_scratch_bytes(int B, int G, int stride, int deg_stride, int max_delay) {
    if (B < 1 || B > 65535 || G < 1 || G > 64 || stride < 1 || stride > kAlignMaxStride || deg_stride < 1 || deg_stride > kAlignMaxStride ||
        max_delay < 0 || max_delay > kAlignMaxDelay) {
        (void)fail(NOMAD_ERR_INVALID,
                   "nomad_align_scratch_bytes: bad argument (B=%d: 1 .. 65535, G=%d: 1 .. 64, stride=%d, deg_stride=%d: 1 .. 2^30, max_delay=%d: "
                   "0 .. %d)", B, G, stride, deg_stride, max_delay, kAlignMaxDelay);
        return 0;
    }
    return align_layout(B, G, stride, max_delay).total;
}

int nomad_align_delay(nomad_ctx* c, const float* clean, int B, int stride, const int* lens, const float* deg, int G, int deg_stride,
                      const int* deg_lens, int max_delay, int* delay_out, double* peak_out, double* corr_out, void* ws, size_t ws_bytes,
                      nomad_stream_t stream) {
    const char* who = "nomad_align_delay";
    if (!c || !clean || !lens || !deg || !deg_lens || !delay_out || !peak_out || !ws)
        return fail(NOMAD_ERR_INVALID, "%s: a NULL context, clean rows, lengths, degraded rows, degraded lengths, delay or peak output or workspace", who);
    if (B < 1 || B > 65535) return fail(NOMAD_ERR_INVALID, "%s: B=%d clips, 1 .. 65535 are supported", who, B);
    if (G < 1 || G > 64) return fail(NOMAD_ERR_INVALID, "%s: G=%d rows per clip, 1 .. 64 are supported", who, G);
    if (max_delay < 0 || max_delay > kAlignMaxDelay)
        return fail(NOMAD_ERR_INVALID, "%s: max_delay=%d samples, 0 .. %d are supported", who, max_delay, kAlignMaxDelay);
    if (stride < 1 || stride > kAlignMaxStride) return fail(NOMAD_ERR_INVALID, "%s: stride=%d, 1 .. 2^30 are supported", who, stride);
    if (deg_stride < 1 || deg_stride > kAlignMaxStride)
        return fail(NOMAD_ERR_INVALID, "%s: deg_stride=%d, 1 .. 2^30 are supported", who, deg_stride);
    const long long R = (long long)B * G;
    for (int b = 0; b < B; ++b)
        if (lens[b] < 1 || lens[b] > stride)
            return fail(NOMAD_ERR_INVALID, "%s: clip %d has length %d, 1 .. stride=%d are supported", who, b, lens[b], stride);
    for (long long r = 0; r < R; ++r)
        if (deg_lens[r] < 1 || deg_lens[r] > deg_stride)
            return fail(NOMAD_ERR_INVALID, "%s: degraded row %lld has length %d, 1 .. deg_stride=%d are supported", who, r, deg_lens[r], deg_stride);
    const AlignLayout l = align_layout(B, G, stride, max_delay);
    const int nl = 2 * max_delay + 1, lag_blocks = (nl + kAlignTile - 1) / kAlignTile;
    if (R * lag_blocks * l.pmax > 0x7fffffffLL)
        return fail(NOMAD_ERR_INVALID, "%s: %lld workgroups, more than one launch holds", who, R * lag_blocks * l.pmax);
    if (ws_bytes < l.total) return fail(NOMAD_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, l.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(ws);
    std::vector<char>& staged = c->degrade_meta_ring[c->degrade_seq++ % 16];
    staged.assign(l.parts, 0);
    memcpy(staged.data(), lens, sizeof(int) * (size_t)B);
    memcpy(staged.data() + l.dlens, deg_lens, sizeof(int) * (size_t)R);
    HIP_TRY(hipMemcpyAsync(w, staged.data(), l.parts, hipMemcpyHostToDevice, s));
    const int* lens_dev = reinterpret_cast<const int*>(w);
    double* parts = reinterpret_cast<double*>(w + l.parts);
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(align_corr_kernel, dim3((unsigned)(R * lag_blocks * l.pmax)), dim3(kAlignThreads), 0, s, clean, stride, lens_dev, deg,
                       deg_stride, reinterpret_cast<const int*>(w + l.dlens), G, max_delay, lag_blocks, l.pmax, parts);
    hipLaunchKernelGGL(align_select_kernel, dim3((unsigned)R), dim3(256), 0, s, static_cast<const double*>(parts), lens_dev, G, max_delay,
                       l.pmax, delay_out, peak_out, corr_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int nomad_align_shift(nomad_ctx* c, const float* deg, int R, int deg_stride, const int* deg_lens, const int* delay, const int* out_lens,
                      float* out, int out_stride, void* ws, size_t ws_bytes, nomad_stream_t stream) {
    const char* who = "nomad_align_shift";
    if (!c || !deg || !deg_lens || !delay || !out_lens || !out || !ws)
        return fail(NOMAD_ERR_INVALID, "%s: a NULL context, degraded rows, lengths, delays, output lengths, output or workspace", who);
    if (R < 1 || R > 65535 * 64) return fail(NOMAD_ERR_INVALID, "%s: R=%d rows, 1 .. 65535 x 64 are supported", who, R);
    if (deg_stride < 1 || deg_stride > kAlignMaxStride)
        return fail(NOMAD_ERR_INVALID, "%s: deg_stride=%d, 1 .. 2^30 are supported", who, deg_stride);
    if (out_stride < 1 || out_stride > kAlignMaxStride)
        return fail(NOMAD_ERR_INVALID, "%s: out_stride=%d, 1 .. 2^30 are supported", who, out_stride);
    for (int r = 0; r < R; ++r) {
        if (deg_lens[r] < 1 || deg_lens[r] > deg_stride)
            return fail(NOMAD_ERR_INVALID, "%s: degraded row %d has length %d, 1 .. deg_stride=%d are supported", who, r, deg_lens[r], deg_stride);
        if (out_lens[r] < 1 || out_lens[r] > out_stride)
            return fail(NOMAD_ERR_INVALID, "%s: output row %d has length %d, 1 .. out_stride=%d are supported", who, r, out_lens[r], out_stride);
    }
    const long long tiles = ((long long)out_stride + 255) / 256;
    if (tiles * R > 0x7fffffffLL) return fail(NOMAD_ERR_INVALID, "%s: %lld workgroups, more than one launch holds", who, tiles * R);
    const size_t tab = align_lens_bytes(R), need = 2 * tab;
    if (ws_bytes < need) return fail(NOMAD_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(ws);
    std::vector<char>& staged = c->degrade_meta_ring[c->degrade_seq++ % 16];
    staged.assign(need, 0);
    memcpy(staged.data(), deg_lens, sizeof(int) * (size_t)R);
    memcpy(staged.data() + tab, out_lens, sizeof(int) * (size_t)R);
    HIP_TRY(hipMemcpyAsync(w, staged.data(), need, hipMemcpyHostToDevice, s));
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(align_shift_kernel, dim3((unsigned)(tiles * R)), dim3(256), 0, s, deg, deg_stride, reinterpret_cast<const int*>(w), delay,
                       reinterpret_cast<const int*>(w + tab), (int)tiles, out, out_stride);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t nomad_l1_scratch_bytes(void) { return sizeof(double) * (kL1Blocks + 8); }

}  // extern "C"

// The L1 loss over `rows` frames of B clips: rows = B * T (nomad_l1_loss) or the packed frames of a ragged batch.
static int l1_loss_rows(const char* who, nomad_ctx* c, const float* a_layers, const float* b_layers, const float* a_emb,
                        const float* b_emb, long long rows, int B, float* loss, void* scratch, nomad_stream_t stream) {
    if (!c || !a_layers || !b_layers || !a_emb || !b_emb || !loss || !scratch || B <= 0 || rows < B)
        return fail(NOMAD_ERR_INVALID, "%s: bad argument", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long per_layer = rows * 768;
    const long long n4 = per_layer * 12 / 4;
    double* partial = static_cast<double*>(scratch);
    Scope sc(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(l1_partial_kernel, dim3(kL1Blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(a_layers),
                       reinterpret_cast<const float4*>(b_layers), n4, a_emb, b_emb, B * 256, partial);
    hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(256), 0, s, partial, (double)per_layer, (double)B * 256, loss);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

int nomad_l1_loss(nomad_ctx* c, const float* a_layers, const float* b_layers, const float* a_emb, const float* b_emb,
                  int B, int T, float* loss, void* scratch, nomad_stream_t stream) {
    return l1_loss_rows("nomad_l1_loss", c, a_layers, b_layers, a_emb, b_emb, T > 0 ? (long long)B * T : 0, B, loss, scratch, stream);
}

int nomad_l1_loss_ragged(nomad_ctx* c, const float* a_layers, const float* b_layers, const float* a_emb, const float* b_emb,
                         long long M, int B, float* loss, void* scratch, nomad_stream_t stream) {
    return l1_loss_rows("nomad_l1_loss_ragged", c, a_layers, b_layers, a_emb, b_emb, M, B, loss, scratch, stream);
}

}  // extern "C"

// ---- weighted, per-utterance NomadLoss -----------------------------------------------------------
namespace {

// Scratch of nomad_l1_loss_weighted[_backward], a function of (M, B) only: the prefix sums | the chunk sums [13][cmax], cmax = M / 16 + B
// bounding the chunks of any split of M frames over B clips | S [13][B].
struct L1wLayout {
    size_t meta, partial, sums, total;
    long long cmax;
};

L1wLayout l1w_layout(long long M, int B) {
    L1wLayout l{};
    l.cmax = M / kL1wChunk + B;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += align_up(bytes); return at; };
    l.meta = take(sizeof(int) * 2 * ((size_t)B + 1));
    l.partial = take(sizeof(double) * 13 * (size_t)l.cmax);
    l.sums = take(sizeof(double) * 13 * (size_t)B);
    l.total = off;
    return l;
}

struct L1wPlan {
    L1wLayout lay;
    L1Weights wt;
    std::vector<int> meta;   // pref[B + 1] | cpref[B + 1]
    int chunks = 0;
    bool any_layer = false;
};

// Every argument check of the two entry points (nothing is queued before it has passed) and the host side of the metadata.
int l1w_plan(const char* who, const nomad_ctx* c, long long M, int B, const int* frames_host, const float* weights_host, int reduction,
             const void* scratch, size_t scratch_bytes, L1wPlan* p) {
    if (!c || !weights_host || !scratch || B <= 0 || M < B || M > 0x7fffffffLL || (reduction != NOMAD_L1_BATCH && reduction != NOMAD_L1_PER_CLIP))
        return fail(NOMAD_ERR_INVALID, "%s: bad argument (M=%lld, B=%d, reduction=%d)", who, M, B, reduction);
    bool any = false;
    for (int i = 0; i < 13; ++i) {
        const float w = weights_host[i];
        if (!(w >= 0.f) || !std::isfinite(w)) return fail(NOMAD_ERR_INVALID, "%s: weight %d is not a finite number >= 0", who, i);
        p->wt.w[i] = w;
        any = any || w != 0.f;
        p->any_layer = p->any_layer || (i < 12 && w != 0.f);
    }
    if (!any) return fail(NOMAD_ERR_INVALID, "%s: every weight is 0", who);
    if (!frames_host && M % B) return fail(NOMAD_ERR_INVALID, "%s: M=%lld is not B=%d equal clips and frames_host is NULL", who, M, B);
    p->meta.assign(2 * ((size_t)B + 1), 0);
    int* pref = p->meta.data();
    int* cpref = pref + B + 1;
    for (int b = 0; b < B; ++b) {
        const long long t = frames_host ? frames_host[b] : M / B;
        if (t < 1 || pref[b] + t > M) return fail(NOMAD_ERR_INVALID, "%s: frames_host[%d] = %lld (at least 1 each, M=%lld in all)", who, b, t, M);
        pref[b + 1] = pref[b] + (int)t;
        cpref[b + 1] = cpref[b] + (int)((t + kL1wChunk - 1) / kL1wChunk);
    }
    if (pref[B] != M) return fail(NOMAD_ERR_INVALID, "%s: frames_host sums to %d, M is %lld", who, pref[B], M);
    p->chunks = cpref[B];
    p->lay = l1w_layout(M, B);
    if (scratch_bytes < p->lay.total) return fail(NOMAD_ERR_WORKSPACE, "%s: scratch %zu < required %zu", who, scratch_bytes, p->lay.total);
    return 0;
}

// The prefix sums' copy into the scratch, queued ahead of the kernels; the host copy is staged in the context's ring (ragged_upload).
int l1w_upload(nomad_ctx* c, const L1wPlan& p, char* scratch, hipStream_t s) {
    std::vector<int>& staged = c->l1w_meta_ring[c->l1w_seq++ % 16];
    staged = p.meta;
    HIP_TRY(hipMemcpyAsync(scratch + p.lay.meta, staged.data(), sizeof(int) * staged.size(), hipMemcpyHostToDevice, s));
    return 0;
}

}  // namespace

extern "C" {

int nomad_l1_weighted_scratch_bytes(long long M, int B, size_t* bytes) {
    if (!bytes || B <= 0 || M < B) return fail(NOMAD_ERR_INVALID, "nomad_l1_weighted_scratch_bytes: bad argument (M=%lld, B=%d)", M, B);
    *bytes = l1w_layout(M, B).total;
    return 0;
}

int nomad_l1_loss_weighted(nomad_ctx* c, const float* a_layers, const float* b_layers, const float* a_emb, const float* b_emb,
                           long long M, int B, const int* frames_host, const float* weights_host, int reduction, float* loss,
                           double* terms, void* scratch, size_t scratch_bytes, nomad_stream_t stream) {
    static const char who[] = "nomad_l1_loss_weighted";
    L1wPlan p;
    if (int rc = l1w_plan(who, c, M, B, frames_host, weights_host, reduction, scratch, scratch_bytes, &p)) return rc;
    if (!loss || (p.any_layer && (!a_layers || !b_layers)) || (p.wt.w[12] != 0.f && (!a_emb || !b_emb)))
        return fail(NOMAD_ERR_INVALID, "%s: a tensor with a non-zero weight (or loss_dev) is NULL", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* sc = static_cast<char*>(scratch);
    if (int rc = l1w_upload(c, p, sc, s)) return rc;
    const int* meta = reinterpret_cast<const int*>(sc + p.lay.meta);
    double* partial = reinterpret_cast<double*>(sc + p.lay.partial);
    Scope scope(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(l1w_partial_kernel, dim3(p.chunks, 13), dim3(256), 0, s, a_layers, b_layers, M, a_emb, b_emb, B, meta, p.wt,
                       p.lay.cmax, partial);
    hipLaunchKernelGGL(l1w_final_kernel, dim3(1), dim3(256), 0, s, partial, p.lay.cmax, meta, B, p.wt, reduction == NOMAD_L1_PER_CLIP ? 1 : 0,
                       reinterpret_cast<double*>(sc + p.lay.sums), loss, terms);
    HIP_TRY(hipGetLastError());
    return 0;
}

int nomad_l1_loss_weighted_backward(nomad_ctx* c, const float* a_layers, const float* b_layers, const float* a_emb,
                                    const float* b_emb, long long M, int B, const int* frames_host, const float* weights_host,
                                    int reduction, int depth, const float* upstream, float* dlayers, float* demb, void* scratch,
                                    size_t scratch_bytes, nomad_stream_t stream) {
    static const char who[] = "nomad_l1_loss_weighted_backward";
    L1wPlan p;
    if (int rc = l1w_plan(who, c, M, B, frames_host, weights_host, reduction, scratch, scratch_bytes, &p)) return rc;
    if (depth < 1 || depth > NOMAD_NUM_LAYERS) return fail(NOMAD_ERR_INVALID, "%s: depth %d is outside 1 .. %d", who, depth, NOMAD_NUM_LAYERS);
    for (int i = depth; i < 13; ++i)   // (the embedding needs the whole encoder)
        if (depth < NOMAD_NUM_LAYERS && p.wt.w[i] != 0.f)
            return fail(NOMAD_ERR_INVALID, "%s: weight %d is not 0 but the depth is %d: its gradient would not be written", who, i, depth);
    const bool emb = p.wt.w[12] != 0.f;
    if (!upstream || !dlayers || (p.any_layer && (!a_layers || !b_layers)) || (emb && (!a_emb || !b_emb || !demb)))
        return fail(NOMAD_ERR_INVALID, "%s: a tensor with a non-zero weight (or upstream_dev / dlayers_dev) is NULL", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* sc = static_cast<char*>(scratch);
    if (int rc = l1w_upload(c, p, sc, s)) return rc;
    Scope scope(c, s, NOMAD_K_ROW, 0.0);
    hipLaunchKernelGGL(l1w_bwd_kernel, dim3(p.chunks, depth + (emb ? 1 : 0)), dim3(256), 0, s, a_layers, b_layers, M, a_emb, b_emb, B,
                       reinterpret_cast<const int*>(sc + p.lay.meta), p.wt, depth, reduction == NOMAD_L1_PER_CLIP ? 1 : 0, upstream, dlayers, demb);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- measurement -----------------------------------------------------------------------------
int nomad_profile_enable(nomad_ctx* c, int on) {
    if (!c) return fail(NOMAD_ERR_INVALID, "null ctx");
    if (on && !c->ev_ready) {
        HIP_TRY(hipSetDevice(c->device));
        c->ev.resize(kEventChunk);
        c->ev_class.resize(kEventChunk / 2);
        for (int i = 0; i < kEventChunk; ++i) HIP_TRY(hipEventCreate(&c->ev[i]));
        c->ev_ready = true;
    }
    c->prof = on != 0;
    return 0;
}

static int profile_drain(nomad_ctx* c) {
    for (int i = 0; i + 1 < c->ev_used; i += 2) {
        HIP_TRY(hipEventSynchronize(c->ev[i + 1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
        const int code = c->ev_class[i / 2];
        c->p_ms[code & 0xff] += ms;
        if (code >> 8) c->p_ms[(code >> 8) - 1] += ms;
    }
    c->ev_used = 0;
    return 0;
}

int nomad_profile_reset(nomad_ctx* c) {
    if (!c) return fail(NOMAD_ERR_INVALID, "null ctx");
    int rc = profile_drain(c);
    c->prof_overflow = false;
    for (int i = 0; i < NOMAD_K_COUNT; ++i) {
        c->p_ms[i] = 0;
        c->p_n[i] = 0;
        c->p_fl[i] = 0;
    }
    return rc;
}

int nomad_profile_read(nomad_ctx* c, double ms[NOMAD_K_COUNT], long long launches[NOMAD_K_COUNT],
                       double flops[NOMAD_K_COUNT]) {
    if (!c || !ms || !launches || !flops) return fail(NOMAD_ERR_INVALID, "null argument");
    int rc = profile_drain(c);
    if (rc) return rc;
    if (c->prof_overflow) return fail(NOMAD_ERR_HIP, "nomad_profile_read: the event pool could not grow; counters are incomplete");
    for (int i = 0; i < NOMAD_K_COUNT; ++i) {
        ms[i] = c->p_ms[i];
        launches[i] = c->p_n[i];
        flops[i] = c->p_fl[i];
    }
    return 0;
}


// One wave spins for `spin_ticks` ticks of the 100 MHz wall counter and reports the shader-clock cycles that passed:
// launched on a second stream while a kernel under test runs, it reads the clock that kernel actually gets.
__global__ void clock_probe_kernel(unsigned long long spin_ticks, unsigned long long* out) {
    const unsigned long long w0 = wall_clock64(), c0 = __builtin_readcyclecounter();
    unsigned long long w1 = w0;
    while (w1 - w0 < spin_ticks) {
        __builtin_amdgcn_s_sleep(32);
        w1 = wall_clock64();
    }
    out[0] = __builtin_readcyclecounter() - c0;
    out[1] = w1 - w0;
}

int nomad_diag_clock_probe(nomad_ctx* c, unsigned long long spin_ticks, unsigned long long* out_dev, nomad_stream_t stream) {
    if (!c || !out_dev) return fail(NOMAD_ERR_INVALID, "nomad_diag_clock_probe: bad argument");
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), spin_ticks, out_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int nomad_diag_layernorm(nomad_ctx* c, const float* in, const float* g, const float* b, float* out, int M, int N,
                         nomad_stream_t stream) {
    if (!c || !in || !g || !b || !out || M <= 0) return fail(NOMAD_ERR_INVALID, "nomad_diag_layernorm: bad argument");
    return run_layernorm(c, in, g, b, out, nullptr, M, N, static_cast<hipStream_t>(stream));
}

int nomad_diag_layernorm_bwd(nomad_ctx* c, const float* x, const float* g, const float* gamma, float* dx, int M, int N,
                             nomad_stream_t stream) {
    if (!c || !x || !g || !gamma || !dx || M <= 0 || (N != 512 && N != 768))
        return fail(NOMAD_ERR_INVALID, "nomad_diag_layernorm_bwd: bad argument");
    return run_ln_bwd(c, x, g, nullptr, gamma, dx, M, N, static_cast<hipStream_t>(stream));
}

int nomad_diag_attention_bwd(nomad_ctx* c, const float* qkv, const float* dctx, float* ctx_out, float* lse, float* dqkv,
                             int B, int T, nomad_stream_t stream) {
    if (!c || !qkv || !dctx || !ctx_out || !lse || !dqkv || B <= 0 || T <= 0)
        return fail(NOMAD_ERR_INVALID, "nomad_diag_attention_bwd: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    BatchGeom g;
    g.B = B;
    g.T = T;
    int rc = run_attention(c, g, qkv, ctx_out, lse, s);
    if (rc) return rc;
    float* D = nullptr;  // diagnostics only: the product path carves this from the caller's workspace
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&D), sizeof(float) * 12 * (size_t)B * T));
    const hipError_t e = launch_attention_bwd(qkv, ctx_out, dctx, lse, D, dqkv, B, T, DropCfg{}, 0, s, 0, !c->tune.attn_bwd_small);
    (void)hipStreamSynchronize(s);
    (void)hipFree(D);
    if (e != hipSuccess) return fail(NOMAD_ERR_HIP, "attention backward: %s", hipGetErrorString(e));
    return 0;
}

int nomad_diag_attention_bf16(nomad_ctx* c, const void* qkv, void* out, int B, int T, int q_has_log2e, nomad_stream_t stream) {
    if (!c || !qkv || !out || B <= 0 || T <= 0) return fail(NOMAD_ERR_INVALID, "nomad_diag_attention_bf16: bad argument");
    if (!q_has_log2e)
        return fail(NOMAD_ERR_INVALID, "nomad_diag_attention_bf16: q must carry log2(e) - the kernel that scaled q itself went with round 5's move to 16x16x32");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scope sc(c, s, NOMAD_K_ATTN, 4.0 * B * 12.0 * (double)T * T * 64);
    HIP_TRY(run_attention_bf16(c, static_cast<const bf16_t*>(qkv), static_cast<bf16_t*>(out), B, T, nullptr, s));
    return 0;
}

int nomad_diag_attention(nomad_ctx* c, const float* qkv, float* out, int B, int T, nomad_stream_t stream) {
    if (!c || !qkv || !out || B <= 0 || T <= 0) return fail(NOMAD_ERR_INVALID, "nomad_diag_attention: bad argument");
    BatchGeom g;
    g.B = B;
    g.T = T;
    return run_attention(c, g, qkv, out, nullptr, static_cast<hipStream_t>(stream));
}

}  // extern "C"
