// conv1 .. conv4 (k = 3, stride 2, 512 -> 512 channels, no bias, GELU) in polyphase Winograd form, fp32 products (round 7).
//
// Output frame t of a clip is y[t] = GELU(w0 x[2t] + w1 x[2t+1] + w2 x[2t+2]) (x: 512-channel input frames, w0 w1 w2: the
// [512 out][512 in] tap matrices of conv_w, stored [out][tap * 512 + in]).  Per output PAIR s of a clip:
//     P[s]    = (w0 + w2) x[4s+2]
//     y[2s]   = GELU( w0 (x[4s]   - x[4s+2]) + w1 x[4s+1] + P[s] )
//     y[2s+1] = GELU( w2 (x[4s+4] - x[4s+2]) + w1 x[4s+3] + P[s] )
// Winograd F(2,2) on the even input phase plus the odd phase's one tap: 5 products per output pair instead of 6 (K = 2560
// instead of 3072 per pair).  The transforms are a weight SUM and input DIFFERENCES, formed in registers between the LDS reads
// and the MFMAs (scalar v_add / v_sub: DESIGN.md section 5 on packed fp32); nothing derived is stored, so the kernel always
// reads the live conv_w.  When a clip has an odd number L of output frames its last pair has no odd output: that pair's frames
// 4s+3 / 4s+4 may not exist and are read clamped to the clip's last frame (the odd accumulator is then never stored).  A pair
// never reads across its clip, so a clip's bits do not depend on its batch; every launch contracts in the same order, so the
// tile / batch / ragged layout changes no bit either.
//
// Workgroup: 128 pairs x 128 output columns (256 output rows), 8 waves as 4 (pairs) x 2 (columns), wave tile 32 pairs x 64
// columns.  Two accumulator sets per wave, E (even rows) and O (odd rows), each 2 x 4 sub-blocks of v_mfma_f32_16x16x4_f32 = 32
// registers: the 64 accumulator registers of the 256 x 128 conv GEMM tile, and with them two workgroups per CU.
//   phase 1 (32 steps of 16 channels): E += (w0 + w2) f2                       1 MFMA stream
//   copy    O := E
//   phase 2 (64 steps of 8 channels):  E += [w0 | w1] . [f0 - f2 | f1]         2 MFMA streams, each contracting 16 k per
//                                      O += [w1 | w2] . [f3 | f4 - f2]         4 k-steps: lane group g < 2 the first term's
//                                                                              channel chunk g, g >= 2 the second's chunk g - 2
// Accumulators are TRANSPOSED (W as the first MFMA operand, as gemm_f32.hip.h OPT bit 1024): a lane owns one pair row per
// 16-row sub-block and four consecutive columns, stored straight from the registers (16-byte stores, no LDS slab).
//
// Staging: LDS-DMA (buffer_load ... lds, gemm_f32.hip.h), two stages of 32 KiB, vmcnt(0) + barrier per step (the STAGES = 2
// scheme of gemm_f32_glds_body).  A phase-2 stage is eight planes [128 rows][8 floats]: input frames f0 .. f4 of the tile's
// pairs, then taps w0 w1 w2 of its columns - 2048 16-byte chunks, four per thread, and every wave-instruction fills 1 KiB of
// ONE plane.  A phase-1 stage is three planes [128][16]: f2, w0, w2.  XOR swizzle on the source address and on the fragment
// read as in gemm_f32.hip.h: chunk c of row r sits at c ^ ((r / RB) % KC), RB = 16 / KC rows per 256-byte bank row.
// Behind each stage, 132 floats of zeros (one fragment row + one 16-row sub-tile step): lanes whose operand has no difference
// subtract a zero read from there, so every lane runs the same v_sub per element (x - 0 == x exactly).
#pragma once
#include "gemm_f32.hip.h"

namespace nomad {

struct ConvS2Params {
    const float* X;      // input frames, [rows][512]
    const float* W;      // [512][1536]: taps w0 w1 w2 of output channel n at n * 1536 + {0, 512, 1024}
    float* Y;            // output frames, [rows][512]
    float* Upre;         // nullable: the pre-activation, same index as Y (training forward)
    int pairs;           // output pairs of the whole batch (the M of this launch)
    int tiles_m;         // ceil(pairs / 128); the grid is tiles_m x 4 column tiles
    // uniform batches: every clip has L output / Lin input frames and ppc = ceil(L / 2) pairs (pair -> clip: fast_div)
    int L, Lin, ppc;
    unsigned ppc_magic;  // 0: a single clip, or one pair per clip
    int ppc_shift;
    // ragged batches (pp != nullptr): clip c owns pairs pp[c] .. pp[c+1]-1, output rows opref[c] .., input rows ipref[c] ..
    const int* pp;
    const int* opref;
    const int* ipref;
    int nclips;
};

struct ConvS2Cfg {
    static constexpr int BMP = 128, BN = 128, NT = 512;
    static constexpr int STAGE = 8 * 1024 + 132;   // floats: eight 4 KiB planes + the zero block
    static constexpr int ZOFF = 8 * 1024;
    static constexpr int LDS_BYTES = 2 * STAGE * 4;
};

// Where pair s reads and writes: its first input row (frame 4j of its clip), its clip's last input row, its even output row,
// and whether its odd output exists.
struct PairRows {
    long long in0, in_last, out0;
    bool odd_ok;
};

template <bool RAGGED>
__device__ __forceinline__ PairRows conv_s2_pair(const ConvS2Params& p, int s) {
    PairRows r;
    if (RAGGED) {
        int lo = 0, hi = p.nclips;   // largest c with pp[c] <= s
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (p.pp[mid] <= s) lo = mid;
            else hi = mid;
        }
        const int j = s - p.pp[lo];
        const int L = p.opref[lo + 1] - p.opref[lo];
        r.in0 = (long long)p.ipref[lo] + 4 * j;
        r.in_last = (long long)p.ipref[lo + 1] - 1;
        r.out0 = (long long)p.opref[lo] + 2 * j;
        r.odd_ok = 2 * j + 1 < L;
    } else {
        const int c = p.ppc_magic ? fast_div(s, p.ppc_magic, p.ppc_shift) : (p.ppc == 1 ? s : 0);
        const int j = s - c * p.ppc;
        r.in0 = (long long)c * p.Lin + 4 * j;
        r.in_last = (long long)c * p.Lin + p.Lin - 1;
        r.out0 = (long long)c * p.L + 2 * j;
        r.odd_ok = 2 * j + 1 < p.L;
    }
    return r;
}

template <bool RAGGED>
__global__ __launch_bounds__(512, 4) void conv_s2_f32_kernel(const ConvS2Params p) {
    using Cfg = ConvS2Cfg;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int nwg = p.tiles_m * 4;
    const int wg = xcd_remap(blockIdx.x, nwg);
    const int tile_m = wg >> 2, tile_n = wg & 3;
    const int m0 = tile_m * Cfg::BMP, n0 = tile_n * Cfg::BN;

    // zero blocks behind both stages (ordered before their first read by the first barrier of the loop)
    if (tid < 2 * 33) *reinterpret_cast<f32x4*>(smem + (tid / 33) * Cfg::STAGE + Cfg::ZOFF + (tid % 33) * 4) = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- DMA geometry ----
    const long long tile_in0 = conv_s2_pair<RAGGED>(p, m0).in0;
    const float* const a_tile = uniform_ptr(p.X + tile_in0 * 512);
    const float* const b_tile = uniform_ptr(p.W + (long long)n0 * 1536);
    // phase 1: chunk id tid + 512 i of planes f2 / w0 / w2 [128][16]: row r1 = tid / 4, chunk tid % 4
    int v1a, v1b;
    {
        const int r1 = tid >> 2, lc = (tid & 3) ^ ((r1 >> 2) & 3);
        const int s = min(m0 + r1, p.pairs - 1);
        const PairRows pr = conv_s2_pair<RAGGED>(p, s);
        v1a = (int)(((pr.in0 + 2 - tile_in0) * 512 + lc * 4) * 4);
        v1b = (r1 * 1536 + lc * 4) * 4;
    }
    // phase 2: chunk id tid + 512 i, plane id / 256 (uniform per wave-instruction), row (tid % 256) / 2, chunk tid % 2.
    // i = 0, 1: frames f0 and f0 + 2 (f0 = tid / 256); i = 2: frame 4 (f0 = 0) or tap w0 (f0 = 1); i = 3: tap 1 + f0.
    const int f0 = wave >> 2;   // uniform
    int v2a[3], v2b;
    {
        const int r = (tid & 255) >> 1, lc = (tid & 1) ^ ((r >> 3) & 1);
        const int s = min(m0 + r, p.pairs - 1);
        const PairRows pr = conv_s2_pair<RAGGED>(p, s);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int f = i == 2 ? 4 : f0 + 2 * i;
            const long long row = min(pr.in0 + f, pr.in_last);
            v2a[i] = (int)(((row - tile_in0) * 512 + lc * 4) * 4);
        }
        v2b = (r * 1536 + lc * 4) * 4;
    }
    auto issue = [&](const int q, const int buf) {
        float* st = smem + buf * Cfg::STAGE + wave * 256;
        if (q < 32) {
            const int k0 = q * 16;
            dma16_buffer(a_tile, (lptr_t)(st), v1a, k0 * 4);
            dma16_buffer(b_tile, (lptr_t)(st + 2048), v1b, k0 * 4);
            dma16_buffer(b_tile, (lptr_t)(st + 4096), v1b, (k0 + 1024) * 4);
        } else {
            const int k0 = (q - 32) * 8;
            dma16_buffer(a_tile, (lptr_t)(st), v2a[0], k0 * 4);
            dma16_buffer(a_tile, (lptr_t)(st + 2048), v2a[1], k0 * 4);
            if (f0 == 0) dma16_buffer(a_tile, (lptr_t)(st + 4096), v2a[2], k0 * 4);
            else dma16_buffer(b_tile, (lptr_t)(st + 4096), v2b, k0 * 4);
            dma16_buffer(b_tile, (lptr_t)(st + 6144), v2b, ((1 + f0) * 512 + k0) * 4);
        }
    };

    // ---- fragment read offsets (floats within a stage) ----
    const int fi = lane & 15, g = lane >> 4;
    const int ra = wm * 32 + fi, rb = wn * 64 + fi;   // + 16 si / + 16 sj: the same swizzle (16 is a multiple of RB * KC)
    // phase 1 ([128][16], KC = 4, RB = 4): logical chunk g
    const int sw1 = (g ^ ((fi >> 2) & 3)) * 4;
    const int o1a = ra * 16 + sw1, o1b = 2048 + rb * 16 + sw1;
    // phase 2 ([128][8], KC = 2, RB = 8): logical chunk g & 1 of plane ...
    const int sw2 = ((g & 1) ^ (fi >> 3)) * 4;
    const bool lo = g < 2;
    const int oEF = (lo ? 0 : 1024) + ra * 8 + sw2;             // f0 | f1
    const int oES = lo ? 2048 + ra * 8 + sw2 : Cfg::ZOFF;        // f2 | 0
    const int oOF = (lo ? 3072 : 4096) + ra * 8 + sw2;          // f3 | f4
    const int oOS = lo ? Cfg::ZOFF : 2048 + ra * 8 + sw2;        // 0  | f2
    const int oBE = (lo ? 5120 : 6144) + rb * 8 + sw2;          // w0 | w1
    const int oBO = (lo ? 6144 : 7168) + rb * 8 + sw2;          // w1 | w2

    f32x4 E[2][4], O[2][4];
#pragma unroll
    for (int si = 0; si < 2; ++si)
#pragma unroll
        for (int sj = 0; sj < 4; ++sj) E[si][sj] = (f32x4){0.f, 0.f, 0.f, 0.f};

    auto rd = [&](const float* base, int off) { return *reinterpret_cast<const f32x4*>(base + off); };
    auto mm = [&](f32x4 (&acc)[2][4], const f32x4 (&a)[2], const f32x4 (&b)[4]) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int si = 0; si < 2; ++si)
#pragma unroll
                for (int sj = 0; sj < 4; ++sj) acc[si][sj] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[sj][c], a[si][c], acc[si][sj], 0, 0, 0);
    };
    auto step1 = [&](const float* st) {
        f32x4 a[2], b[4];
#pragma unroll
        for (int si = 0; si < 2; ++si) a[si] = rd(st, o1a + si * 256);
#pragma unroll
        for (int sj = 0; sj < 4; ++sj) {
            const f32x4 u = rd(st, o1b + sj * 256), v = rd(st, o1b + 2048 + sj * 256);
#pragma unroll
            for (int e = 0; e < 4; ++e) b[sj][e] = u[e] + v[e];
        }
        mm(E, a, b);
    };
    auto operand = [&](const float* st, int of, int os, f32x4 (&a)[2]) {
#pragma unroll
        for (int si = 0; si < 2; ++si) {
            const f32x4 u = rd(st, of + si * 128), v = rd(st, os + si * 128);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[si][e] = u[e] - v[e];
        }
    };
    auto step2 = [&](const float* st) {
        f32x4 a[2], b[4];
        operand(st, oEF, oES, a);
#pragma unroll
        for (int sj = 0; sj < 4; ++sj) b[sj] = rd(st, oBE + sj * 128);
        mm(E, a, b);
        // the O stream's fragments are read behind the E stream's MFMAs: both operand sets live at once would not fit next to
        // the 64 accumulator registers in the 128-register budget of two workgroups per CU
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        operand(st, oOF, oOS, a);
#pragma unroll
        for (int sj = 0; sj < 4; ++sj) b[sj] = rd(st, oBO + sj * 128);
        mm(O, a, b);
    };

    // Step q (phase 1: q < 32, phase 2: 32 <= q < 96) sits in stage q & 1.  Both loops are unrolled by two so that the stage is
    // an immediate offset of every ds_read (a run-time stage base costs a VGPR per fragment offset: 66 registers spilled).
    auto wait_step = [] {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // this step has landed in every wave's share; every wave is done with the other stage
    };
    float* const st0 = smem;
    float* const st1 = smem + Cfg::STAGE;
    issue(0, 0);
    for (int q = 0; q < 32; q += 2) {
        wait_step();
        issue(q + 1, 1);
        step1(st0);
        wait_step();
        issue(q + 2, 0);   // (q = 30: the first phase-2 step)
        step1(st1);
    }
#pragma unroll
    for (int si = 0; si < 2; ++si)
#pragma unroll
        for (int sj = 0; sj < 4; ++sj) O[si][sj] = E[si][sj];
    for (int q = 32; q < 96; q += 2) {
        wait_step();
        issue(q + 1, 1);
        step2(st0);
        wait_step();
        if (q + 2 < 96) issue(q + 2, 0);
        step2(st1);
    }

    // ---- direct epilogue: sub-block (si, sj) of E / O holds pair row 16 si + fi, columns 16 sj + 4 g .. + 3 ----
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));   // the epilogue's per-lane indices are computed here, not kept live across the K loops
    const int col = n0 + wn * 64 + 4 * (lane_e >> 4);
#pragma unroll
    for (int si = 0; si < 2; ++si) {
        const int s = m0 + wm * 32 + (lane_e & 15) + 16 * si;
        if (s >= p.pairs) continue;
        const PairRows pr = conv_s2_pair<RAGGED>(p, s);
        const long long ie = pr.out0 * 512 + col, io = ie + 512;
#pragma unroll
        for (int sj = 0; sj < 4; ++sj) {
            f32x4 ve = E[si][sj], vo = O[si][sj];
            if (p.Upre) {
                *reinterpret_cast<f32x4*>(p.Upre + ie + sj * 16) = ve;
                if (pr.odd_ok) *reinterpret_cast<f32x4*>(p.Upre + io + sj * 16) = vo;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ve[e] = gelu_erf(ve[e]);
                vo[e] = gelu_erf(vo[e]);
            }
            *reinterpret_cast<f32x4*>(p.Y + ie + sj * 16) = ve;
            if (pr.odd_ok) *reinterpret_cast<f32x4*>(p.Y + io + sj * 16) = vo;
        }
    }
}

}  // namespace nomad
