// Row-wise kernels: LayerNorm (SURVEY.md K5/K8 and the two post-LN norms of every encoder layer), the frame
// energies and the NomadLoss L1 reduction (K15, nomad.py:267-282); the embedding head is in head.hip.h.
// All are HBM-bound: one wave per row, 16-byte loads, statistics by wavefront (64-lane) shuffles.
#pragma once
#include <hip/hip_runtime.h>

#include "dtypes.hip.h"

namespace nomad {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// torch.relu / clamp_min(0): max(x, 0) that keeps a NaN.  `fmaxf(x, 0.f)` returns 0 for a NaN (IEEE maxNum), which turned a clip whose
// encoder output is NaN into the finite embedding normalize(bias).  Both selects are true selects, so every other x gives the bits
// v_max_f32(x, 0) gave: x for x > 0 (+Inf included), +0 for x < 0, -Inf, -0 and +0.
__device__ __forceinline__ float relu_keep_nan(float x) { return x > 0.f ? x : (x != x ? x : 0.f); }

// Sum over the S slices of a split-K GEMM's partial products for one float4: ((p[0] + p[stride4]) + p[2 stride4]) + ... in slice order,
// with the loads of the first kSliceBurst slices issued BEFORE the first add.  Round 6: written as `for (s = 1; s < S; ++s) a += p[s * stride4]`
// with a run-time S hipcc emits load - s_waitcnt vmcnt(0) - add per slice, and the epilogue kernels of configs[3] (1632 rows: one wave of
// work per CU, nothing else to hide a round trip behind) spent 6 dependent memory round trips per column chunk.  S is wave-uniform.
constexpr int kSliceBurst = 8;
__device__ __forceinline__ void load_slices4(float4 (&t)[kSliceBurst], const float4* __restrict__ p, long long stride4, int S) {
#pragma unroll
    for (int s = 0; s < kSliceBurst; ++s)
        if (s < S) t[s] = p[s * stride4];
}
__device__ __forceinline__ float4 add_slices4(const float4 (&t)[kSliceBurst], const float4* __restrict__ p, long long stride4, int S) {
    float4 a = t[0];
#pragma unroll
    for (int s = 1; s < kSliceBurst; ++s)
        if (s < S) {
            a.x += t[s].x; a.y += t[s].y; a.z += t[s].z; a.w += t[s].w;
        }
    for (int s = kSliceBurst; s < S; ++s) {
        const float4 b = p[s * stride4];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    return a;
}
__device__ __forceinline__ float4 sum_slices4(const float4* __restrict__ p, long long stride4, int S) {
    float4 t[kSliceBurst];
    load_slices4(t, p, stride4, S);
    return add_slices4(t, p, stride4, S);
}

// One row of LayerNorm by one wave: lane l holds elements 4 (l + 64 i) .. + 3 of the row, i < VPT (N = 256 VPT).  layernorm_kernel below
// and the split-K epilogue that normalises its own rows (splitk_epilogue_ln_kernel, train.hip.h) run exactly this code - one summation
// order, so a row's result does not depend on which kernel normalised it.
template <int VPT, typename TOut>
__device__ __forceinline__ void ln_row_finish(const float4 (&v)[VPT], const float4 (&g)[VPT], const float4 (&bb)[VPT], TOut* __restrict__ o,
                                              long long out_plane, float4* __restrict__ o2, int lane) {
    constexpr int N = 256 * VPT;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPT; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    const float mean = wave_sum(s) * (1.0f / N);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
        q += (a * a + b * b) + (c * c + d * d);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / N) + 1e-5f);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        float4 r;
        r.x = (v[i].x - mean) * rstd * g[i].x + bb[i].x;
        r.y = (v[i].y - mean) * rstd * g[i].y + bb[i].y;
        r.z = (v[i].z - mean) * rstd * g[i].z + bb[i].z;
        r.w = (v[i].w - mean) * rstd * g[i].w + bb[i].w;
        store4p<TOut>(o + 4 * (lane + 64 * i), out_plane, r);
        if (o2) o2[lane + 64 * i] = r;
    }
}

// out[m][:] = (in[m][:] - mean) * rstd * gamma + beta; optional second copy out2 (layer_results).
// VPT float4 per lane: N = 256 * VPT (512 -> 2, 768 -> 3).  grid: ceil(M / (4 ROWS)) blocks of 256 threads; a wave normalises ROWS
// consecutive rows with one fetch of gamma / beta (round 6: at one bf16 row per wave the 6 KB of gamma and beta a wave pulls through the
// vector cache are twice the 3 KB of the row it reads and writes; the bf16 forward takes 4 rows per wave, all their loads in flight at once).
// A row's arithmetic is ln_row_finish whatever ROWS is.
template <int VPT, typename TIn = float, typename TOut = float, int ROWS = 1>
__global__ __launch_bounds__(256) void layernorm_kernel(const TIn* __restrict__ in, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, TOut* __restrict__ out,
                                                        float* __restrict__ out2, int M, long long in_plane = 0,
                                                        long long out_plane = 0) {
    constexpr int N = 256 * VPT;
    const int lane = threadIdx.x & 63;
    const int m0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS;
    if (m0 >= M) return;
    float4 v[ROWS][VPT], g[VPT], bb[VPT];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const TIn* row = in + (long long)min(m0 + r, M - 1) * N;
#pragma unroll
        for (int i = 0; i < VPT; ++i) v[r][i] = load4p<TIn>(row + 4 * (lane + 64 * i), in_plane);
    }
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        g[i] = reinterpret_cast<const float4*>(gamma)[lane + 64 * i];
        bb[i] = reinterpret_cast<const float4*>(beta)[lane + 64 * i];
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int m = m0 + r;
        if (m < M)
            ln_row_finish<VPT, TOut>(v[r], g, bb, out + (long long)m * N, out_plane, out2 ? reinterpret_cast<float4*>(out2 + (long long)m * N) : nullptr, lane);
    }
}

// Mean square of every encoder frame's 400 samples (nomad_frame_energy): e[fpref[c] + t] = (sum_{i < 400} x_c[320 t + i]^2) / 400
// in float64 - a float's square is exact in double.  One wave per frame: lane l adds samples l, l + 64, ... in order, then the
// wave's xor butterfly; a frame is a function of its own samples only, in a fixed order.  Up to kEnergyClips clips per launch,
// their frame prefix sums and lengths by value.  grid: (ceil(frames of the longest clip / 4), clips) blocks of 256 threads.
constexpr int kEnergyClips = 64;
struct EnergyClips {
    int fpref[kEnergyClips + 1];   // frames ahead of clip c inside this launch's part of e
    int len[kEnergyClips];         // samples of clip c
};
__global__ __launch_bounds__(256) void frame_energy_kernel(const float* __restrict__ x, long long stride, EnergyClips cl,
                                                           double* __restrict__ e) {
    const int c = blockIdx.y, lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= cl.fpref[c + 1] - cl.fpref[c]) return;
    const float* xf = x + (long long)c * stride + 320LL * t;
    const int avail = min(400, cl.len[c] - 320 * t);   // 400 for every frame the conv stack counts
    double acc = 0.0;
    for (int i = lane; i < avail; i += 64) {
        const double v = (double)xf[i];
        acc += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) e[cl.fpref[c] + t] = acc / 400.0;
}

// NomadLoss.  Stage 1: per-block fp64 partial sums of |a-b| over the 12 layer tensors (n_layer
// float4s in total) and over the embeddings; stage 2: one block folds the partials in fixed order.
constexpr int kL1Blocks = 1024;
__global__ __launch_bounds__(256) void l1_partial_kernel(const float4* __restrict__ a, const float4* __restrict__ b,
                                                         long long n4, const float* __restrict__ ea,
                                                         const float* __restrict__ eb, int ne,
                                                         double* __restrict__ partial) {
    __shared__ double red[4];
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)kL1Blocks * 256) {
        const float4 x = a[i], y = b[i];
        s += (double)((fabsf(x.x - y.x) + fabsf(x.y - y.y)) + (fabsf(x.z - y.z) + fabsf(x.w - y.w)));
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    if (blockIdx.x == 0) {  // embedding term, one block
        __syncthreads();
        double se = 0.0;
        for (int i = threadIdx.x; i < ne; i += 256) se += (double)fabsf(ea[i] - eb[i]);
        se = wave_sum(se);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = se;
        __syncthreads();
        if (threadIdx.x == 0) partial[kL1Blocks] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

__global__ __launch_bounds__(256) void l1_final_kernel(const double* __restrict__ partial, double layer_elems,
                                                       double emb_elems, float* __restrict__ loss) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < kL1Blocks; i += 256) s += partial[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double layers = (red[0] + red[1]) + (red[2] + red[3]);
        // 12 terms each a mean over layer_elems elements, plus the embedding term
        loss[0] = (float)(layers / layer_elems + partial[kL1Blocks] / emb_elems);
    }
}

// Weighted, per-utterance NomadLoss (nomad_l1_loss_weighted).  A (layer, clip) slab - the clip's rows pref[b] .. pref[b + 1] of layer i,
// contiguous in [12][B][T][768] and in packed [12][M][768] alike - is cut into chunks of kL1wChunk frames counted from the CLIP's first
// frame, one workgroup each: differences in fp32, accumulated in fp64, the fixed fold of l1_partial_kernel.  A chunk's sum depends on
// the clip's own values only, whatever batch it is in.  Stage 2 folds a slab's chunk sums in chunk order into S[13][B] and combines
// them (below).  No atomics: the result is identical run to run.  A term with weight 0 is never read.
// meta (device ints): pref[B + 1] frame prefix sums | cpref[B + 1] chunk prefix sums.
constexpr int kL1wChunk = 16;
struct L1Weights {
    float w[13];
};

__device__ __forceinline__ int l1w_clip_of(const int* __restrict__ cpref, int B, int chunk) {
    int lo = 0, hi = B;   // the clip b with cpref[b] <= chunk < cpref[b + 1] (every clip has at least one chunk)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cpref[mid] <= chunk) lo = mid;
        else hi = mid;
    }
    return lo;
}

// grid: (chunks of the batch, 13).  y < 12: chunk x of layer y -> partial[y * cstride + x]; y = 12: workgroup x < B takes clip x's 256
// embedding values -> partial[12 * cstride + x].
__global__ __launch_bounds__(256) void l1w_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, long long M,
                                                          const float* __restrict__ ea, const float* __restrict__ eb, int B,
                                                          const int* __restrict__ meta, L1Weights wt, long long cstride,
                                                          double* __restrict__ partial) {
    __shared__ double red[4];
    const int i = blockIdx.y;
    if (wt.w[i] == 0.f) return;   // (uniform over the workgroup)
    double s = 0.0;
    if (i == 12) {
        if ((int)blockIdx.x >= B) return;
        const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
        s = (double)fabsf(ea[e] - eb[e]);
    } else {
        const int* pref = meta;
        const int* cpref = meta + B + 1;
        const int clip = l1w_clip_of(cpref, B, (int)blockIdx.x);
        const long long f0 = pref[clip] + (long long)((int)blockIdx.x - cpref[clip]) * kL1wChunk;
        const long long left = pref[clip + 1] - f0;
        const int n4 = (int)(left < kL1wChunk ? left : kL1wChunk) * 192;
        const float4* a4 = reinterpret_cast<const float4*>(a + ((long long)i * M + f0) * 768);
        const float4* b4 = reinterpret_cast<const float4*>(b + ((long long)i * M + f0) * 768);
        for (int k = threadIdx.x; k < n4; k += 256) {
            const float4 x = a4[k], y = b4[k];
            // (every |a - b| enters the fp64 sum on its own: the terms then differ from any other fp64 summation by its order alone)
            s += ((double)fabsf(x.x - y.x) + (double)fabsf(x.y - y.y)) + ((double)fabsf(x.z - y.z) + (double)fabsf(x.w - y.w));
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[(long long)i * cstride + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup.  S[i][b] = the slab's chunk sums in chunk order; terms[i][b] = S / n (0 where the weight is 0), n = T_b * 768 (256 for
// the embedding).  per_clip: loss[b] = sum_i w_i S[i][b] / n[i][b]; else loss[0] = sum_i w_i (sum_b S[i][b]) / (sum_b n[i][b]) - i and
// b ascending, in fp64.
__global__ __launch_bounds__(256) void l1w_final_kernel(const double* __restrict__ partial, long long cstride,
                                                        const int* __restrict__ meta, int B, L1Weights wt, int per_clip,
                                                        double* __restrict__ S, float* __restrict__ loss, double* __restrict__ terms) {
    __shared__ double lsum[13];
    const int* pref = meta;
    const int* cpref = meta + B + 1;
    for (int p = threadIdx.x; p < 13 * B; p += 256) {
        const int i = p / B, b = p - i * B;
        double s = 0.0;
        if (wt.w[i] != 0.f) {
            if (i == 12) s = partial[12 * cstride + b];
            else
                for (int ch = cpref[b]; ch < cpref[b + 1]; ++ch) s += partial[(long long)i * cstride + ch];
        }
        S[p] = s;
        if (terms) terms[p] = wt.w[i] != 0.f ? s / (i == 12 ? 256.0 : (double)(pref[b + 1] - pref[b]) * 768.0) : 0.0;
    }
    __syncthreads();
    if (per_clip) {
        for (int b = threadIdx.x; b < B; b += 256) {
            const double nl = (double)(pref[b + 1] - pref[b]) * 768.0;
            double l = 0.0;
            for (int i = 0; i < 13; ++i)
                if (wt.w[i] != 0.f) l += (double)wt.w[i] * (S[i * B + b] / (i == 12 ? 256.0 : nl));
            loss[b] = (float)l;
        }
        return;
    }
    if (threadIdx.x < 13) {
        double s = 0.0;
        if (wt.w[threadIdx.x] != 0.f)
            for (int b = 0; b < B; ++b) s += S[threadIdx.x * B + b];
        lsum[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double l = 0.0;
        for (int i = 0; i < 13; ++i)
            if (wt.w[i] != 0.f) l += (double)wt.w[i] * (lsum[i] / (i == 12 ? (double)B * 256.0 : (double)pref[B] * 768.0));
        loss[0] = (float)l;
    }
}

}  // namespace nomad
