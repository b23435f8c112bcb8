// Row-wise kernels: LayerNorm (SURVEY.md K5/K8 and the two post-LN norms of every encoder layer),
// the embedding head (K13: mean_t -> ReLU -> Linear(768,256) -> L2 normalise, nomad.py:228-230)
// and the NomadLoss L1 reduction (K15, nomad.py:267-282).  All are HBM-bound: one wave per row,
// 16-byte loads, statistics by wavefront (64-lane) shuffles.
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

// ---- head: mean over time -> ReLU -> Linear(768, 256) -> L2 normalise (nomad.py:228-230) ---------------------------
// Stage 1, head_pool_kernel: the time sum of a clip in chunks of kHeadChunk frames, one workgroup per (chunk, clip), so
// that a 30 s clip (T = 1499) is summed by 24 workgroups instead of one thread column walking 1499 rows (452 us for a
// batch of 32 such clips with the single-stage kernel, 40 x the time of reading the 74 MB once).
// Wave w of the workgroup takes frames w, w + 4, ... of the chunk, lane l the columns 4l + 256j (j = 0..2); the four
// waves are folded in fixed order.  Chunk j of clip b (rows r0 .. r0 + T - 1 of x) goes to slot r0 / 64 + b + j of
// `pool` - unique for packed clips of any lengths, at most M / 64 + B slots.  The summation order depends on T only:
// batch-invariant and deterministic.
constexpr int kHeadChunk = 64;
template <typename TIn = float>
__global__ __launch_bounds__(256) void head_pool_kernel(const TIn* __restrict__ x, int T, float* __restrict__ pool,
                                                        const int* __restrict__ tpref = nullptr) {
    __shared__ float4 part[4][3][64];
    const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long row0 = (long long)b * T;
    if (tpref) {  // ragged batch: this clip's own frame range
        row0 = tpref[b];
        T = tpref[b + 1] - tpref[b];
    }
    if (j * kHeadChunk >= T) return;
    const int t_end = min(T, (j + 1) * kHeadChunk);
    float4 acc[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = j * kHeadChunk + wave; t < t_end; t += 4) {
        const TIn* r = x + (row0 + t) * 768 + 4 * lane;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float4 v = load4<TIn>(r + 256 * q);
            acc[q].x += v.x; acc[q].y += v.y; acc[q].z += v.z; acc[q].w += v.w;
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) part[wave][q][lane] = acc[q];
    __syncthreads();
    if (wave == 0) {
        float* dst = pool + (row0 / kHeadChunk + b + j) * 768 + 4 * lane;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float4 a = part[0][q][lane];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const float4 o = part[w][q][lane];
                a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
            }
            *reinterpret_cast<float4*>(dst + 256 * q) = a;
        }
    }
}

// Stage 2.  grid: B blocks of 1024 threads.  pool (stage 1) -> emb [B][256].
// Round 6: 16 waves instead of 4 - with one 4-wave workgroup per clip a batch of 32 clips (configs[3]) kept 128 waves busy streaming the
// 786 KB of W each: 66 us per launch, all of it load latency.  Wave w now takes output rows 16 w .. 16 w + 15, four rows (48 loads) in
// flight per trip.  A row's dot product is still one wave's: lane l multiplies elements l + 64 i in the order i = 0 .. 11, then the
// wave sum - the same bits as before; the squared norm is summed by waves 0 .. 3 over e[64 w ..] and folded as before.
__global__ __launch_bounds__(1024) void head_kernel(const float* __restrict__ pool, int T, const float* __restrict__ w,
                                                    const float* __restrict__ bias, float* __restrict__ emb,
                                                    const int* __restrict__ tpref = nullptr) {
    __shared__ float pooled[768];
    __shared__ float e[256];
    __shared__ float wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    long long row0 = (long long)b * T;
    if (tpref) {
        row0 = tpref[b];
        T = tpref[b + 1] - tpref[b];
    }
    if (tid < 256) {
        const float* pb = pool + (row0 / kHeadChunk + b) * 768;
        const int nchunk = (T + kHeadChunk - 1) / kHeadChunk;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int j = 0; j < nchunk; ++j) {  // chunks in order
            const float* r = pb + (long long)j * 768;
            s0 += r[tid];
            s1 += r[tid + 256];
            s2 += r[tid + 512];
        }
        const float inv = 1.0f / (float)T;
        pooled[tid] = relu_keep_nan(s0 * inv);
        pooled[tid + 256] = relu_keep_nan(s1 * inv);
        pooled[tid + 512] = relu_keep_nan(s2 * inv);
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    float p[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) p[i] = pooled[lane + 64 * i];
#pragma unroll 1
    for (int o0 = wave * 16; o0 < wave * 16 + 16; o0 += 4) {
        float wv[4][12];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 12; ++i) wv[u][i] = w[(long long)(o0 + u) * 768 + lane + 64 * i];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 12; ++i) d = fmaf(wv[u][i], p[i], d);
            d = wave_sum(d);
            if (lane == 0) e[o0 + u] = d + bias[o0 + u];
        }
    }
    __syncthreads();
    if (tid < 256) {
        const float v = e[tid];
        const float ss = wave_sum(v * v);
        if (lane == 0) wsum[wave] = ss;
    }
    __syncthreads();
    if (tid < 256) {
        const float nrm = sqrtf((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
        emb[(long long)b * 256 + tid] = e[tid] / fmaxf(nrm, 1e-12f);  // F.normalize eps
    }
}

// Stage 2 of the pooled backbone features (Origw2v.forward, networks.py:29-34: res['x'].mean(1), no ReLU, no Linear, no
// normalisation).  grid: B blocks of 256 threads.  pool (stage 1) -> feat [B][768]: a clip's chunks folded in order and
// `sum * (1 / T)`, the expression head_kernel forms before its ReLU.
__global__ __launch_bounds__(256) void head_mean_kernel(const float* __restrict__ pool, int T, float* __restrict__ feat,
                                                        const int* __restrict__ tpref = nullptr) {
    const int b = blockIdx.x, tid = threadIdx.x;
    long long row0 = (long long)b * T;
    if (tpref) {
        row0 = tpref[b];
        T = tpref[b + 1] - tpref[b];
    }
    const float* pb = pool + (row0 / kHeadChunk + b) * 768;
    const int nchunk = (T + kHeadChunk - 1) / kHeadChunk;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int j = 0; j < nchunk; ++j) {  // chunks in order
        const float* r = pb + (long long)j * 768;
        s0 += r[tid];
        s1 += r[tid + 256];
        s2 += r[tid + 512];
    }
    const float inv = 1.0f / (float)T;
    float* o = feat + (long long)b * 768;
    o[tid] = s0 * inv;
    o[tid + 256] = s1 * inv;
    o[tid + 512] = s2 * inv;
}

// Windows of frames (nomad_embed_windows*): W = 1 for a clip of T <= win frames, else (T - win) / hop + 1; window k covers
// frames [k hop, k hop + min(win, T)).  Frames behind the last full window belong to no window (torch.Tensor.unfold).
__host__ __device__ inline int head_num_windows(int T, int win, int hop) {
    if (T < 1 || win < 1 || hop < 1) return 0;
    return T <= win ? 1 : (T - win) / hop + 1;
}

// The windows that cover frame t of a clip (0 <= t < T; T, win, hop >= 1): k_lo .. k_hi, consecutive.  Window k covers t when
// k hop <= t < k hop + n with n = min(win, T), so k_hi = min(W - 1, t / hop) and k_lo = max(0, ceil((t - n + 1) / hop)).
// k_lo > k_hi: no window covers t - a gap between windows (hop > win) or the tail behind the last full window.  The one place
// this arithmetic lives: the backward's scatter (backward.hip.h) and nomad_window_cover.
__host__ __device__ inline void head_window_cover(int T, int win, int hop, int t, int* k_lo, int* k_hi) {
    const int n = win < T ? win : T, last = head_num_windows(T, win, hop) - 1, a = t - n + 1;
    *k_hi = t / hop < last ? t / hop : last;
    *k_lo = a <= 0 ? 0 : (a - 1) / hop + 1;
}

// The head over windows of frames, both stages in one workgroup: window k of clip b -> one row of emb, in the arithmetic
// of head_pool_kernel + head_kernel applied to the window's rows as if they were a clip of their own, so a window that
// covers a whole clip has the bits of that clip's embedding, and a window's 256 values are a function of its own rows only.
// grid: (windows of the longest clip, B) blocks of 1024 threads; a block past its clip's last window returns.
//   time sum: chunks of kHeadChunk frames counted from the WINDOW's first frame; waves 0..3 take frames w, w + 4, ... of
//     a chunk (lane l the columns 4l + 256q), are folded in the order 0..3 by wave 0, which adds the chunk sums in chunk
//     order to a running sum in its registers - no scratch, no atomics; overlapping windows re-read their rows from L2.
//   then sum * (1.0f / n), ReLU, and head_kernel's Linear and norm on all 16 waves, operation for operation.
// Output rows: clip 0's windows, then clip 1's, ...: row wbase(b) + k with wbase(b) = b W for an equal-length batch and
// the sum of the earlier clips' window counts, formed here from the frame prefix sums, for a ragged one.
template <typename TIn = float>
__global__ __launch_bounds__(1024) void head_windows_kernel(const TIn* __restrict__ x, int T, int win, int hop,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ emb, const int* __restrict__ tpref = nullptr) {
    __shared__ float4 part[4][3][64];
    __shared__ float pooled[768];
    __shared__ float e[256];
    __shared__ float wsum[4];
    __shared__ int wcnt[16];
    const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long row0 = (long long)b * T;
    if (tpref) {
        row0 = tpref[b];
        T = tpref[b + 1] - tpref[b];
    }
    if (k >= head_num_windows(T, win, hop)) return;   // the same for every thread of the block
    long long orow = (long long)b * head_num_windows(T, win, hop) + k;
    if (tpref) {   // windows of clips 0 .. b - 1 (integers: any order gives the same sum)
        int cnt = 0;
        for (int c = tid; c < b; c += 1024) cnt += head_num_windows(tpref[c + 1] - tpref[c], win, hop);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0) wcnt[wave] = cnt;
        __syncthreads();
        int base = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) base += wcnt[i];
        orow = (long long)base + k;
    }
    const int n = min(win, T);
    const TIn* xw = x + (row0 + (long long)k * hop) * 768;   // rows [k hop, k hop + n) of the clip: k hop + n <= T
    float4 run[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) run[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t0 = 0; t0 < n; t0 += kHeadChunk) {   // chunks in order
        if (wave < 4) {
            const int t_end = min(n, t0 + kHeadChunk);
            float4 acc[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int t = t0 + wave; t < t_end; t += 4) {
                const TIn* r = xw + (long long)t * 768 + 4 * lane;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float4 v = load4<TIn>(r + 256 * q);
                    acc[q].x += v.x; acc[q].y += v.y; acc[q].z += v.z; acc[q].w += v.w;
                }
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) part[wave][q][lane] = acc[q];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                float4 a = part[0][q][lane];
#pragma unroll
                for (int u = 1; u < 4; ++u) {
                    const float4 o = part[u][q][lane];
                    a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
                }
                run[q].x += a.x; run[q].y += a.y; run[q].z += a.z; run[q].w += a.w;
            }
        }
        __syncthreads();   // part is rewritten by the next chunk
    }
    if (wave == 0) {
        const float inv = 1.0f / (float)n;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float* p = pooled + 256 * q + 4 * lane;
            p[0] = relu_keep_nan(run[q].x * inv);
            p[1] = relu_keep_nan(run[q].y * inv);
            p[2] = relu_keep_nan(run[q].z * inv);
            p[3] = relu_keep_nan(run[q].w * inv);
        }
    }
    __syncthreads();
    float p[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) p[i] = pooled[lane + 64 * i];
#pragma unroll 1
    for (int o0 = wave * 16; o0 < wave * 16 + 16; o0 += 4) {
        float wv[4][12];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 12; ++i) wv[u][i] = w[(long long)(o0 + u) * 768 + lane + 64 * i];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 12; ++i) d = fmaf(wv[u][i], p[i], d);
            d = wave_sum(d);
            if (lane == 0) e[o0 + u] = d + bias[o0 + u];
        }
    }
    __syncthreads();
    if (tid < 256) {
        const float v = e[tid];
        const float ss = wave_sum(v * v);
        if (lane == 0) wsum[wave] = ss;
    }
    __syncthreads();
    if (tid < 256) {
        const float nrm = sqrtf((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
        emb[orow * 256 + tid] = e[tid] / fmaxf(nrm, 1e-12f);  // F.normalize eps
    }
}

// ---- spans of frames (nomad_embed_spans*) -----------------------------------------------------------------------------------
// The span table on the device, one block of ints: row_clip[R], row_ptr[R + 1], spans[S][2] = (t0, t1), clip_row[B + 1].
// Row r belongs to clip row_clip[r] and pools spans row_ptr[r] .. row_ptr[r + 1] - 1 (ascending, not overlapping, inside the clip:
// the host checks all of it before the table is queued); the rows of clip b are clip_row[b] .. clip_row[b + 1] - 1.
struct SpanTable {
    const int *row_clip, *row_ptr, *spans, *clip_row;
};
__host__ __device__ inline size_t span_table_ints(int B, int R, int S) { return (size_t)2 * R + 1 + (size_t)2 * S + B + 1; }
__host__ __device__ inline SpanTable span_table(const int* tab, int R, int S) {
    return SpanTable{tab, tab + R, tab + 2 * R + 1, tab + 2 * R + 1 + 2 * S};
}

// The row's virtual frame index (0 .. n - 1 over the concatenation of its spans) -> the frame of the clip.  Virtual indices are
// asked for in ascending order, so the cursor only moves forward; v < n keeps it inside the row's spans.
struct SpanCursor {
    const int* sp;   // the row's first span
    int vbase, t0, len;
    __device__ explicit SpanCursor(const int* first) : sp(first), vbase(0), t0(first[0]), len(first[1] - first[0]) {}
    __device__ int frame(int v) {
        while (v >= vbase + len) {
            vbase += len;
            sp += 2;
            t0 = sp[0];
            len = sp[1] - t0;
        }
        return t0 + (v - vbase);
    }
};

__device__ inline int span_row_frames(const SpanTable& tb, int r) {
    int n = 0;
    for (int i = tb.row_ptr[r]; i < tb.row_ptr[r + 1]; ++i) n += tb.spans[2 * i + 1] - tb.spans[2 * i];
    return n;
}

// The head over rows of spans: row r -> emb[r][256].  head_windows_kernel, operation for operation, on the row's virtual frames
// 0 .. n - 1 (n = the sum of its spans' lengths): chunks of kHeadChunk virtual frames counted from the row's first frame run
// across span boundaries, waves 0..3 take virtual frames w, w + 4, ... of a chunk and are folded 0..3 into the running sum in
// chunk order; then sum * (1.0f / n), ReLU, head_kernel's Linear and norm on 16 waves.  Only the virtual -> actual mapping (a
// SpanCursor per wave) is new, so a row of one span [a, a + n) has the bits of a window over those frames and a row whose spans
// concatenate to the whole clip has the bits of the clip's embedding.  grid: R blocks of 1024 threads; ragged batches only
// (tpref: the frame prefix sums).  No scratch, no atomics.
template <typename TIn = float>
__global__ __launch_bounds__(1024) void head_spans_kernel(const TIn* __restrict__ x, const int* __restrict__ tab, int R, int S,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ emb, const int* __restrict__ tpref) {
    __shared__ float4 part[4][3][64];
    __shared__ float pooled[768];
    __shared__ float e[256];
    __shared__ float wsum[4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SpanTable tb = span_table(tab, R, S);
    const long long row0 = tpref[tb.row_clip[r]];
    const int n = span_row_frames(tb, r);   // the same for every thread of the block
    const TIn* xc = x + row0 * 768;
    SpanCursor cur(tb.spans + 2 * tb.row_ptr[r]);
    float4 run[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) run[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int v0 = 0; v0 < n; v0 += kHeadChunk) {   // chunks in order
        if (wave < 4) {
            const int v_end = min(n, v0 + kHeadChunk);
            float4 acc[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int v = v0 + wave; v < v_end; v += 4) {
                const TIn* rp = xc + (long long)cur.frame(v) * 768 + 4 * lane;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float4 val = load4<TIn>(rp + 256 * q);
                    acc[q].x += val.x; acc[q].y += val.y; acc[q].z += val.z; acc[q].w += val.w;
                }
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) part[wave][q][lane] = acc[q];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                float4 a = part[0][q][lane];
#pragma unroll
                for (int u = 1; u < 4; ++u) {
                    const float4 o = part[u][q][lane];
                    a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
                }
                run[q].x += a.x; run[q].y += a.y; run[q].z += a.z; run[q].w += a.w;
            }
        }
        __syncthreads();   // part is rewritten by the next chunk
    }
    if (wave == 0) {
        const float inv = 1.0f / (float)n;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float* p = pooled + 256 * q + 4 * lane;
            p[0] = relu_keep_nan(run[q].x * inv);
            p[1] = relu_keep_nan(run[q].y * inv);
            p[2] = relu_keep_nan(run[q].z * inv);
            p[3] = relu_keep_nan(run[q].w * inv);
        }
    }
    __syncthreads();
    float p[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) p[i] = pooled[lane + 64 * i];
#pragma unroll 1
    for (int o0 = wave * 16; o0 < wave * 16 + 16; o0 += 4) {
        float wv[4][12];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 12; ++i) wv[u][i] = w[(long long)(o0 + u) * 768 + lane + 64 * i];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 12; ++i) d = fmaf(wv[u][i], p[i], d);
            d = wave_sum(d);
            if (lane == 0) e[o0 + u] = d + bias[o0 + u];
        }
    }
    __syncthreads();
    if (tid < 256) {
        const float v = e[tid];
        const float ss = wave_sum(v * v);
        if (lane == 0) wsum[wave] = ss;
    }
    __syncthreads();
    if (tid < 256) {
        const float nrm = sqrtf((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
        emb[(long long)r * 256 + tid] = e[tid] / fmaxf(nrm, 1e-12f);  // F.normalize eps
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
