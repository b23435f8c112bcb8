// Time alignment of degraded rows with their clean clips: the cross-correlation of every (clean clip b, degraded row r = b G + g) pair
// at every integer lag d in [-D, D], the lag of its largest value, and the row shifted by it (include/nomad_hip.h states the contract):
//     c_r[d] = sum over i with 0 <= i < n_b and 0 <= i + d < m_r of x_b[i] y_r[i + d]        (d > 0: the degraded row is late).
//
// Direct form on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation), as degrade_convolve.hip.h
// does for convolution - but here BOTH MFMA dimensions are lag: a 16 x 16 accumulator tile holds 256 consecutive lags,
//     c[d0 + 16 j + i] = sum_t A[i][t] B[t][j],   A[i][t] = y[t + i + d0]   (a Hankel fragment of the degraded row),
//                                                  B[t][j] = x[t - 16 j]    (the clean clip at a stride of 16),
// t running over [0, n + 240) with zeros outside either signal.  A workgroup (4 waves) owns one row, up to 16 lag tiles (kAlignTile =
// 4096 lags; tile q of the workgroup belongs to wave q mod 4, so a short lag range is spread over the waves) and a span of time, which
// it walks in slabs of 1024 steps.  Per slab both signals are staged in LDS once, masked at their lengths (nothing behind a length is
// read), and both fragments are read from there with ds_read_b32 (32 banks, the two halves of a wave apart):
//   * A: lane (i, k) reads ys[16 s + 4 q + k + i + 256 tile]: the 32 lanes of a half touch 17 consecutive words - no bank conflict.
//   * B: lanes step by 16 samples, 8-way conflicted on a flat image.  The image is SKEWED: sample p is stored at p + 2 (p / 16), so the
//     16 columns of a fragment are 18 words apart - the even banks for k = 0, the odd ones for k = 1: every half covers the 32 banks.
//     One B value serves all of the wave's tiles: 1 + 1 / 4 LDS reads per MFMA with four tiles.
// A slab is skipped where no sample of the degraded row can meet any lag of the workgroup (only zeros would be added).
//
// Order.  Per lag one fp32 chain per SLICE of kAlignSlice = 4096 consecutive time steps t, slices being [0, 4096), [4096, 8192), ...;
// in a chain t ascends, four products per MFMA.  The slices are then added in float64 in ascending order: a workgroup adds its own
// (up to kAlignPartSlices = 8, a PART) in registers, and align_select_kernel adds the parts of a lag, again ascending, without
// atomics.  Slices and parts are fixed by n_b alone, the skipped slabs by (n_b, m_r, D): row r of any batch has the bits of its own
// B = 1, G = 1 call.  Integer-valued inputs whose sums stay below 2^24 per slice give the exact float64 sums.  Products with a
// padding zero are formed (0 x): a non-finite sample makes lags NaN that it does not reach by the formula, inside its own row only -
// and any NaN makes the row's delay 0 and its peak NaN anyway.
//
// Bound.  2 overlap FLOP per lag at 1.25 ds_read_b32 per MFMA; staging is 25 loads per thread against 1024 MFMAs per wave with a
// barrier on each side and no double buffer (the overlap comes from the other workgroups a CU holds: 25.2 KB of LDS each).  Wasted:
// the 240 steps of skew per row, the lags between 2 D + 1 and the next multiple of 256, and, where D is not small against n, the
// steps of a slab in which a tile has no overlap.
//
// NOT here (the header says the same): sub-sample delays, clock drift, per-patch re-alignment, a polarity search (the sign of c
// counts), a gradient.
#pragma once
#include <hip/hip_runtime.h>

namespace nomad {

constexpr int kAlignMaxDelay = 16384;
constexpr int kAlignSlice = 4096;                              // time steps of one fp32 chain
constexpr int kAlignPartSlices = 8;                            // slices a workgroup adds up in float64 registers
constexpr int kAlignThreads = 256;
constexpr int kAlignSubs = 4;                                  // accumulator tiles (256 lags each) per wave
constexpr int kAlignTile = (kAlignThreads / 64) * kAlignSubs * 256;   // lags per workgroup: 4096
constexpr int kAlignSlab = 1024;                               // time steps staged at once
constexpr int kAlignSkew = 240;                                // x[t - 16 j], j < 16
constexpr int kAlignYWords = kAlignSlab + kAlignTile - 256 + 16;      // ys[p] = y[S0 + d_base + p]
constexpr int kAlignXSlab = kAlignSlab + kAlignSkew;           // xs: x[S0 - 240 + p], p at p + 2 (p / 16)
constexpr int kAlignXWords = kAlignXSlab / 16 * 18;

typedef float align_f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int align_slices(int n) { return (n + kAlignSkew + kAlignSlice - 1) / kAlignSlice; }
__host__ __device__ inline int align_parts(int n) { return (align_slices(n) + kAlignPartSlices - 1) / kAlignPartSlices; }

// One slab of 1024 time steps into the wave's NU tiles.  ya = ys + k + i + 256 wave, xb = xs + 18 (15 - j) + k.
template <int NU>
__device__ __forceinline__ void align_slab(const float* __restrict__ ya, const float* __restrict__ xb, align_f32x4 (&acc)[kAlignSubs]) {
    for (int sq = 0; sq < kAlignSlab / 16; ++sq) {
        float a[4][NU], b[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            b[s4] = xb[18 * sq + 4 * s4];
#pragma unroll
            for (int u = 0; u < NU; ++u) a[s4][u] = ya[16 * sq + 4 * s4 + 1024 * u];
        }
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int u = 0; u < NU; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s4][u], b[s4], acc[u], 0, 0, 0);
    }
}

// Grid: R lag_blocks pmax blocks, block = (row * lag_blocks + lag block) * pmax + part.  x [B][stride], lens [B]; y [B G][deg_stride],
// dlens [B G]; part [B G][pmax][2 D + 1] float64: part p of a row's lags, written for p < align_parts(n_b) only.
__global__ __launch_bounds__(kAlignThreads) void align_corr_kernel(const float* __restrict__ x, int stride, const int* __restrict__ lens,
                                                                    const float* __restrict__ y, int deg_stride,
                                                                    const int* __restrict__ dlens, int G, int D, int lag_blocks, int pmax,
                                                                    double* __restrict__ part) {
    __shared__ float ys[kAlignYWords];
    __shared__ float xs[kAlignXWords];
    int blk = blockIdx.x;
    const int p = blk % pmax;
    blk /= pmax;
    const int lb = blk % lag_blocks, row = blk / lag_blocks;
    const int n = lens[row / G], m = dlens[row];
    const int ns = align_slices(n);
    const int s_first = p * kAlignPartSlices;
    if (s_first >= ns) return;
    const int s_end = ns < s_first + kAlignPartSlices ? ns : s_first + kAlignPartSlices;
    const int nl = 2 * D + 1, l0 = lb * kAlignTile, d_base = l0 - D;
    const int nt = (nl - l0 + 255) / 256 < 16 ? (nl - l0 + 255) / 256 : 16;   // lag tiles of this workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, fg = lane >> 4;
    const int nu = wave < nt ? (nt - wave + 3) / 4 : 0;                      // tiles wave, wave + 4, ... of them
    const float* xr = x + (size_t)(row / G) * (size_t)stride;
    const float* yr = y + (size_t)row * (size_t)deg_stride;
    const float* ya = ys + fg + fi + 256 * wave;
    const float* xb = xs + 18 * (15 - fi) + fg;

    double sum[kAlignSubs][4];
#pragma unroll
    for (int u = 0; u < kAlignSubs; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[u][r] = 0.0;

    for (int sl = s_first; sl < s_end; ++sl) {
        align_f32x4 acc[kAlignSubs];
#pragma unroll
        for (int u = 0; u < kAlignSubs; ++u) acc[u] = align_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int S0 = sl * kAlignSlice; S0 < (sl + 1) * kAlignSlice && S0 < n + kAlignSkew; S0 += kAlignSlab) {
            const int ybase = S0 + d_base;
            if (ybase >= m || ybase + kAlignYWords <= 0) continue;   // no sample of the row under any lag of this workgroup
            for (int q = tid; q < kAlignYWords; q += kAlignThreads) {
                const int idx = ybase + q;
                ys[q] = (idx >= 0 && idx < m) ? yr[idx] : 0.0f;
            }
            for (int q = tid; q < kAlignXSlab; q += kAlignThreads) {
                const int idx = S0 - kAlignSkew + q;
                xs[q + 2 * (q >> 4)] = (idx >= 0 && idx < n) ? xr[idx] : 0.0f;
            }
            __syncthreads();
            switch (nu) {
                case 4: align_slab<4>(ya, xb, acc); break;
                case 3: align_slab<3>(ya, xb, acc); break;
                case 2: align_slab<2>(ya, xb, acc); break;
                case 1: align_slab<1>(ya, xb, acc); break;
                default: break;
            }
            __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < kAlignSubs; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[u][r] += (double)acc[u][r];
    }

    // lane (fi, fg) holds lags l .. l + 3 of each of its tiles
    double* prow = part + ((size_t)row * (size_t)pmax + (size_t)p) * (size_t)nl;
#pragma unroll
    for (int u = 0; u < kAlignSubs; ++u) {
        if (u >= nu) break;
        const int l = l0 + 256 * (4 * u + wave) + 16 * fi + 4 * fg;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (l + r < nl) prow[l + r] = sum[u][r];
    }
}

// (c1, d1) goes before (c2, d2): the larger value, then the smaller |lag|, then the non-negative lag.
__device__ __forceinline__ bool align_before(double c1, int d1, double c2, int d2) {
    if (c1 != c2) return c1 > c2;
    const int a1 = d1 < 0 ? -d1 : d1, a2 = d2 < 0 ? -d2 : d2;
    return a1 != a2 ? a1 < a2 : d1 > d2;
}

// One workgroup per row: the parts of every lag added in ascending order, the lag of the largest sum.  Any NaN: delay 0, peak NaN.
__global__ __launch_bounds__(256) void align_select_kernel(const double* __restrict__ part, const int* __restrict__ lens, int G, int D, int pmax,
                                                           int* __restrict__ delay, double* __restrict__ peak, double* __restrict__ corr) {
    __shared__ double sc[256];
    __shared__ int sd[256];
    __shared__ int snan[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int parts = align_parts(lens[row / G]), nl = 2 * D + 1;
    const double* prow = part + (size_t)row * (size_t)pmax * (size_t)nl;
    double best_c = 0.0;
    int best_d = 0, have = 0, nan = 0;
    for (int l = tid; l < nl; l += 256) {
        double c = prow[l];
        for (int p = 1; p < parts; ++p) c += prow[(size_t)p * (size_t)nl + l];
        if (corr) corr[(size_t)row * (size_t)nl + l] = c;
        if (c != c) {
            nan = 1;
        } else if (!have || align_before(c, l - D, best_c, best_d)) {
            best_c = c;
            best_d = l - D;
            have = 1;
        }
    }
    // a thread without a lag stands in with -inf at a lag further out than any: it goes before no real entry
    sc[tid] = have ? best_c : -__builtin_huge_val();
    sd[tid] = have ? best_d : 0x7fffffff;
    snan[tid] = nan;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            if (align_before(sc[tid + h], sd[tid + h], sc[tid], sd[tid])) {
                sc[tid] = sc[tid + h];
                sd[tid] = sd[tid + h];
            }
            snan[tid] |= snan[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        delay[row] = snan[0] ? 0 : sd[0];
        peak[row] = snan[0] ? __builtin_nan("") : sc[0];
    }
}

// Grid: R tiles blocks of 256 samples, block = row * tiles + tile.  out[r][i] = y[r][i + delay[r]] inside both lengths, else 0.
__global__ __launch_bounds__(256) void align_shift_kernel(const float* __restrict__ y, int deg_stride, const int* __restrict__ dlens,
                                                          const int* __restrict__ delay, const int* __restrict__ olens, int tiles,
                                                          float* __restrict__ out, int out_stride) {
    const int row = blockIdx.x / tiles, i = (blockIdx.x - row * tiles) * 256 + threadIdx.x;
    if (i >= out_stride) return;
    const long long j = (long long)i + delay[row];
    const bool inside = i < olens[row] && j >= 0 && j < dlens[row];
    out[(size_t)row * (size_t)out_stride + i] = inside ? y[(size_t)row * (size_t)deg_stride + (size_t)j] : 0.0f;
}

}  // namespace nomad
