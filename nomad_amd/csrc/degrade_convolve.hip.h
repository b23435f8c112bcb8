// Reverberation as what it is for any fixed setting - a causal FIR filter: every clip convolved with each of G impulse responses,
// cut to the clip's length, written straight into the (B G, stride) layout nomad_embed_ragged reads (row b G + g = clip b through
// response g):   out[b G + g][i] = sum_{k = 0}^{min(L_g - 1, i)} h_g[k] x_b[i - k]   (include/nomad_hip.h states the contract).
//
// Direct form on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation, an fmaf chain per output).
// BOTH MFMA dimensions are time, so the utilisation does not depend on G: a 16 x 16 accumulator tile holds 256 consecutive outputs,
//     out[t0 + 16 i + j] = sum_m T[j][m] X[m][i],   T[j][m] = h[c0 + 240 + j - m] (zero outside the chunk's taps),
//                                                    X[m][i] = x[t0 - c0 - 240 + 16 i + m],
// the taps being walked in chunks of 241 (c0 = 0, 241, ...): 241 taps + the 15 rows a Toeplitz tile is skewed by = a K extent of 256
// = 64 MFMAs, of which 241 / 256 = 94 % is arithmetic the formula asks for.  A workgroup (4 waves) owns one row and 4096 outputs of
// it, a wave 4 accumulator tiles (1024 outputs); per chunk the workgroup stages two 1-D slabs in LDS - 4352 samples and the chunk's
// taps reversed, 19.5 KB together whatever L is - and both fragments are read from them:
//   * T (the A operand) depends on (j, m) only: one ds_read_b32 serves the wave's 4 tiles.  Lane (j, m) reads hs[m - j + 15]: the 64
//     lanes touch 19 consecutive words, lanes with one address share it - no bank conflict.
//   * X (the B operand): lanes step by 16 samples, 8-way conflicted on a flat image (32 banks).  The image is SKEWED instead: sample p
//     is stored at p + p / 16, so the 16 columns of a fragment are 17 words apart and every group of 32 lanes covers the 32 banks.
// Staging is masked: samples before the clip's start and from its length on are zeros, taps from the response's length on are
// zeros; nothing behind a length reaches the arithmetic (the caller may keep anything there).
//
// Order.  Per output the chunks in ascending order, inside a chunk the taps in DESCENDING order (m ascending), four products per
// MFMA.  The last chunk starts at the first group of four MFMAs that holds one of its taps, and a tile's chunks end with the last tap any of its
// outputs can reach: both depend on (n, L) and on the output's place in its row only, so a row has the bits of its clip's own
// B = 1, G = 1 call.  Products with a padding zero are formed (0 x): a non-finite sample or tap can therefore reach up to 255 outputs
// further than the formula says, inside its own row only.
//
// Bound.  2 L FLOP per output on the matrix cores at 94 % (long L) of their fp32 rate, less the ragged last tile of a row (up to
// 4095 outputs' worth) and the last chunk's padding.  Per MFMA (32 cycles per SIMD) a wave issues 1.25 ds_read_b32; staging is
// 18 loads per thread against 256 MFMAs per wave, with a workgroup barrier on each side and no double buffer: the overlap comes from
// the 7 other workgroups a CU holds.  Not done: the X fragment shared over a clip's G responses, wider LDS reads, a second slab.
#pragma once
#include <hip/hip_runtime.h>

namespace nomad {

constexpr int kRirMaxResponses = 64;
constexpr int kRirMaxTaps = 65536;
constexpr int kRirThreads = 256;
constexpr int kRirSubs = 4;                                   // accumulator tiles (256 outputs each) per wave
constexpr int kRirTile = (kRirThreads / 64) * kRirSubs * 256;   // outputs per workgroup: 4096
constexpr int kRirK = 256;                                    // K extent of a chunk: 64 MFMAs
constexpr int kRirChunk = kRirK - 15;                        // taps per chunk: 241
constexpr int kRirXSlab = kRirTile + kRirK;                 // samples staged per chunk
constexpr int kRirXWords = kRirXSlab + kRirXSlab / 16;      // ... skewed: sample p at p + p / 16
constexpr int kRirHWords = kRirK + 16;                       // hs[q] = h[c0 + 255 - q], q = m - j + 15 in [0, 271)

typedef float conv_f32x4 __attribute__((ext_vector_type(4)));

// Grid: B G tiles blocks, block = row * tiles + tile (a row's tiles are neighbours: they share the clip and the response in L2).
// x [B][stride], lens [B]; ir [G][ir_stride], ir_lens [G]; out [B G][stride].  tiles = ceil(stride / kRirTile).
__global__ __launch_bounds__(kRirThreads) void degrade_convolve_kernel(const float* __restrict__ x, int stride, const int* __restrict__ lens,
                                                                        const float* __restrict__ ir, int ir_stride,
                                                                        const int* __restrict__ ir_lens, int G, int tiles,
                                                                        float* __restrict__ out) {
    __shared__ float xs[kRirXWords];
    __shared__ float hs[kRirHWords];
    const int row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const int b = row / G, g = row - b * G;
    const int n = lens[b], L = ir_lens[g];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, fg = lane >> 4;
    const int T0 = tile * kRirTile;
    const float* xr = x + (size_t)b * (size_t)stride;
    const float* hr = ir + (size_t)g * (size_t)ir_stride;
    float* orow = out + (size_t)row * (size_t)stride;

    conv_f32x4 acc[kRirSubs];
#pragma unroll
    for (int u = 0; u < kRirSubs; ++u) acc[u] = conv_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    if (T0 < n) {
        const bool active = T0 + wave * (kRirSubs * 256) < n;   // a wave whose outputs all lie behind the length only stages
        const int t_last = (n < T0 + kRirTile ? n : T0 + kRirTile) - 1;
        const int k_last = L - 1 < t_last ? L - 1 : t_last;      // the last tap any output of this tile reaches
        const int xw = (wave * kRirSubs * 256 + 16 * fi) / 16 * 17 + fg;   // skewed word of sample 256 (4 wave + u) + 16 fi + m, less u and m
        for (int c0 = 0; c0 <= k_last; c0 += kRirChunk) {
            const int xbase = T0 - c0 - (kRirChunk - 1);
            for (int p = tid; p < kRirXSlab; p += kRirThreads) {
                const int idx = xbase + p;
                xs[p + (p >> 4)] = (idx >= 0 && idx < n) ? xr[idx] : 0.0f;
            }
            for (int q = tid; q < kRirHWords; q += kRirThreads) {
                const int k = c0 + (kRirK - 1) - q;
                hs[q] = (k >= c0 && k < c0 + kRirChunk && k < L) ? hr[k] : 0.0f;
            }
            __syncthreads();
            if (active) {
                const int cv = L - c0 < kRirChunk ? L - c0 : kRirChunk;   // taps of this chunk
                const int q0 = (kRirChunk - cv) >> 4;   // T[j][m] = 0 for m < 241 - cv: the first group of 4 MFMAs (16 m) with a tap
                const float* ha = hs + (fg - fi + 15);
                for (int sq = q0; sq < kRirK / 16; ++sq) {
                    float a[4], xv[4][kRirSubs];
#pragma unroll
                    for (int s4 = 0; s4 < 4; ++s4) {
                        a[s4] = ha[16 * sq + 4 * s4];
#pragma unroll
                        for (int u = 0; u < kRirSubs; ++u) xv[s4][u] = xs[xw + 17 * sq + 4 * s4 + u * 272];   // m = 16 sq + 4 s4 + fg: m + m / 16
                    }
#pragma unroll
                    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                        for (int u = 0; u < kRirSubs; ++u)
                            acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s4], xv[s4][u], acc[u], 0, 0, 0);
                }
            }
            __syncthreads();
        }
    }

    // lane (fi, fg) holds outputs t .. t + 3 of each of its tiles; zeros from the length to the end of the row
    const bool aligned = (reinterpret_cast<size_t>(out) & 15) == 0;
#pragma unroll
    for (int u = 0; u < kRirSubs; ++u) {
        const int t = T0 + (wave * kRirSubs + u) * 256 + 16 * fi + 4 * fg;
        if (aligned && t + 3 < n) {
            *reinterpret_cast<float4*>(orow + t) = make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (t + r < stride) orow[t + r] = t + r < n ? acc[u][r] : 0.0f;
        }
    }
}

}  // namespace nomad
