// The embedding head (K13: mean_t -> ReLU -> Linear(768, 256) -> L2 normalise, nomad.py:228-230) and its backward, over whole clips,
// over windows of frames and over rows of caller-given spans.  Every step of the arithmetic is written ONCE below as a
// __device__ __forceinline__ piece and the kernels are sequences of pieces, so the bit contracts between them - a one-span row equals
// a window, a whole-clip window equals the clip's embedding, the backward's pooled and ReLU mask equal the forward's - hold because
// both sides run the same code, and a fix lands in one place.
#pragma once
#include <hip/hip_runtime.h>

#include "dtypes.hip.h"
#include "rowops.hip.h"

namespace nomad {

constexpr int kHeadChunk = 64;   // frames per chunk of the time sum

// ---- which frames a workgroup pools, and where its row goes -------------------------------------------------------------------------
// Windows of frames (nomad_embed_windows*): W = 1 for a clip of T <= win frames, else (T - win) / hop + 1; window k covers
// frames [k hop, k hop + min(win, T)).  Frames behind the last full window belong to no window (torch.Tensor.unfold).
__host__ __device__ inline int head_num_windows(int T, int win, int hop) {
    if (T < 1 || win < 1 || hop < 1) return 0;
    return T <= win ? 1 : (T - win) / hop + 1;
}

// The windows that cover frame t of a clip (0 <= t < T; T, win, hop >= 1): k_lo .. k_hi, consecutive.  Window k covers t when
// k hop <= t < k hop + n with n = min(win, T), so k_hi = min(W - 1, t / hop) and k_lo = max(0, ceil((t - n + 1) / hop)).
// k_lo > k_hi: no window covers t - a gap between windows (hop > win) or the tail behind the last full window.  The one place
// this arithmetic lives: the backward's scatter and nomad_window_cover.
__host__ __device__ inline void head_window_cover(int T, int win, int hop, int t, int* k_lo, int* k_hi) {
    const int n = win < T ? win : T, last = head_num_windows(T, win, hop) - 1, a = t - n + 1;
    *k_hi = t / hop < last ? t / hop : last;
    *k_lo = a <= 0 ? 0 : (a - 1) / hop + 1;
}

// Clip b's first row of x and, through T, its frames: b T of an equal-length batch, the frame prefix sums of a ragged one.
__device__ __forceinline__ long long head_clip(const int* __restrict__ tpref, int b, int& T) {
    if (!tpref) return (long long)b * T;
    T = tpref[b + 1] - tpref[b];
    return tpref[b];
}

// The windows of clips 0 .. b - 1 of a ragged batch, from the frame prefix sums: every thread of the workgroup of kThreads (its
// kernel's launch bound) counts the clips tid, tid + kThreads, ..; lanes by xor butterfly, waves through LDS (integers: any order
// gives the same sum).  Whole workgroups only - it holds a barrier.  kThreads is a template argument because the waves' counts
// are then read back in one unrolled burst: a loop over blockDim.x / 64 reads them one LDS round trip after the other, 0.4 us more
// per launch of the 16-wave kernels.
template <int kThreads>
__device__ __forceinline__ long long windows_before(const int* __restrict__ tpref, int b, int win, int hop) {
    __shared__ int wcnt[kThreads / 64];
    const int tid = threadIdx.x;
    int cnt = 0;
    for (int c = tid; c < b; c += kThreads) cnt += head_num_windows(tpref[c + 1] - tpref[c], win, hop);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
    __syncthreads();
    long long base = 0;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) base += wcnt[i];
    return base;
}

struct ConsecutiveFrames {   // frame v of the row is the v-th row behind its first: the mapping is the address add
    __device__ __forceinline__ int frame(int v) const { return v; }
};

// Window blockIdx.x of clip blockIdx.y.  Output rows: clip 0's windows, then clip 1's, ...: row wbase(b) + k with wbase(b) = b W
// for an equal-length batch (T: frames per clip, tpref NULL) and the earlier clips' window counts for a ragged one (T ignored).
struct WindowRows {
    int T, win, hop;
    const int* tpref;
    // What a workgroup of a rows kernel works on.  first: the row of x its frames are counted from; n frames, frame v at row
    // first + frames.frame(v); the row `out` of the output.  valid = false: a block past its clip's last window (the same for every
    // thread of the block).
    struct Row {
        long long first, out;
        int n;
        ConsecutiveFrames frames;
        bool valid;
    };
    template <int kThreads>
    __device__ __forceinline__ long long wbase(int b, int Tb) const {
        return tpref ? windows_before<kThreads>(tpref, b, win, hop) : (long long)b * head_num_windows(Tb, win, hop);
    }
    __device__ __forceinline__ Row row() const {   // (of a kernel of 1024 threads)
        const int b = blockIdx.y, k = blockIdx.x;
        int Tb = T;
        const long long row0 = head_clip(tpref, b, Tb);
        if (k >= head_num_windows(Tb, win, hop)) return Row{0, 0, 0, {}, false};
        // rows [k hop, k hop + n) of the clip: k hop + n <= T
        return Row{row0 + (long long)k * hop, wbase<1024>(b, Tb) + k, min(win, Tb), {}, true};
    }
};

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

// Row blockIdx.x of the span table (ragged batches only: tpref, the frame prefix sums) -> row blockIdx.x of the output.  Its n
// virtual frames (the sum of its spans' lengths) are counted from the clip's first frame through a SpanCursor per wave.
struct SpanRows {
    const int* tab;
    int R, S;
    const int* tpref;
    struct Row {
        long long first, out;
        int n;
        SpanCursor frames;
        bool valid;
    };
    __device__ __forceinline__ Row row() const {
        const SpanTable tb = span_table(tab, R, S);
        const int r = blockIdx.x;
        const long long first = tpref[tb.row_clip[r]];   // (two dependent loads: issued ahead of the loop over the spans)
        const int i0 = tb.row_ptr[r], i1 = tb.row_ptr[r + 1];
        int n = 0;   // the same for every thread of the block
        for (int i = i0; i < i1; ++i) n += tb.spans[2 * i + 1] - tb.spans[2 * i];
        return Row{first, r, n, SpanCursor(tb.spans + 2 * i0), true};
    }
};

// ---- the time sum ---------------------------------------------------------------------------------------------------------------------
// One row of 768 values into / out of a lane's three float4s: lane l holds the columns 4l + 256q (float4 l + 64q of the row).
template <typename TIn>
__device__ __forceinline__ void head_row_add(float4 (&acc)[3], const TIn* __restrict__ row, int lane) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float4 v = load4<TIn>(row + 4 * lane + 256 * q);
        acc[q].x += v.x; acc[q].y += v.y; acc[q].z += v.z; acc[q].w += v.w;
    }
}
__device__ __forceinline__ void head_row_store(const float4 (&v)[3], float* __restrict__ row, int lane) {
#pragma unroll
    for (int q = 0; q < 3; ++q) reinterpret_cast<float4*>(row)[lane + 64 * q] = v[q];
}
__device__ __forceinline__ void head_row_zero(float4 (&acc)[3]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// The LDS image of four waves' partial sums, part[wave][q][lane].  Float j of part[w][q][l] is column 256q + 4l + j, so as floats
// the image is [4][768] in column order: wave w's column c at part_floats(part)[w][c] - the forward reads it as float4s, the backward
// as float4s for the time sum and as floats for the four slices of W^T dz.
typedef float4 HeadPart[4][3][64];
__device__ __forceinline__ float (*part_floats(HeadPart& part))[768] { return reinterpret_cast<float(*)[768]>(part); }

// Waves 0 .. 3 only: wave w sums the frames t0 + w, t0 + w + 4, .. < t_end (frame v at row fr.frame(v) behind xc) into part[w].
template <typename TIn, class Frames>
__device__ __forceinline__ void head_partial_sums(const TIn* __restrict__ xc, Frames& fr, int t0, int t_end, HeadPart& part, int lane, int wave) {
    float4 acc[3];
    head_row_zero(acc);
    for (int t = t0 + wave; t < t_end; t += 4) head_row_add<TIn>(acc, xc + (long long)fr.frame(t) * 768, lane);
#pragma unroll
    for (int q = 0; q < 3; ++q) part[wave][q][lane] = acc[q];
}
// The four partial sums of a lane's float4 q, folded in wave order: ((p0 + p1) + p2) + p3.
__device__ __forceinline__ float4 head_fold_0123(const HeadPart& part, int q, int lane) {
    float4 a = part[0][q][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const float4 o = part[w][q][lane];
        a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
    }
    return a;
}

// THE CHUNKED TIME SUM (head_pool_kernel + head_kernel's, and every rows kernel's, forward and backward): the n frames in chunks
// of kHeadChunk counted from the first; waves 0..3 take frames w, w + 4, .. of a chunk and are folded 0..3 by wave 0, which adds the
// chunk sums in chunk order to the running sum `run` in its registers (valid in wave 0 only) - no scratch, no atomics.
// Whole workgroups of at least four waves.
template <typename TIn, class Frames>
__device__ __forceinline__ void head_sum_rows(const TIn* __restrict__ xc, Frames& fr, int n, HeadPart& part, float4 (&run)[3]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    head_row_zero(run);
    for (int t0 = 0; t0 < n; t0 += kHeadChunk) {   // chunks in order
        if (wave < 4) head_partial_sums<TIn>(xc, fr, t0, min(n, t0 + kHeadChunk), part, lane, wave);
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float4 a = head_fold_0123(part, q, lane);
                run[q].x += a.x; run[q].y += a.y; run[q].z += a.z; run[q].w += a.w;
            }
        }
        __syncthreads();   // part is rewritten by the next chunk
    }
}
// ... and its end in wave 0: pooled = ReLU(sum * (1.0f / n)) and, for a backward, mask = the ReLU's derivative over n.
__device__ __forceinline__ void head_pooled_from_sum(const float4 (&run)[3], int n, float* __restrict__ pooled, float* __restrict__ mask) {
    const int lane = threadIdx.x & 63;
    if (threadIdx.x >= 64) return;
    const float inv = 1.0f / (float)n;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float m[4] = {run[q].x * inv, run[q].y * inv, run[q].z * inv, run[q].w * inv};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pooled[256 * q + 4 * lane + j] = relu_keep_nan(m[j]);
            if (mask) mask[256 * q + 4 * lane + j] = m[j] > 0.f ? inv : 0.f;
        }
    }
}

// THE ONE-PASS TIME SUM of head_bwd_kernel, and only of it: waves 0..3 take frames w, w + 4, .. of the WHOLE clip in one pass and
// are folded (p0 + p1) + (p2 + p3) by the first 256 threads.  This is not the chunked sum above: its fold is paired where that one
// is sequential, and past kHeadChunk frames a wave's partial sum runs across what are chunk boundaries there.  So `pooled` may
// differ from head_kernel's in the last bits and, for a mean within rounding of 0, the ReLU mask with it (known
// warts).  It is kept as it is because it is the arithmetic of every gradient through nomad_embed_backward* / nomad_train_backward*.
__device__ __forceinline__ void head_pooled_one_pass(const float* __restrict__ xb, int T, HeadPart& part, float* __restrict__ pooled,
                                                     float* __restrict__ mask) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    ConsecutiveFrames fr;
    if (wave < 4) head_partial_sums<float>(xb, fr, 0, T, part, lane, wave);
    __syncthreads();
    if (tid < 256) {
        float(*psum)[768] = part_floats(part);
        const float inv = 1.0f / (float)T;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int c = tid + 256 * j;
            const float m = ((psum[0][c] + psum[1][c]) + (psum[2][c] + psum[3][c])) * inv;
            pooled[c] = relu_keep_nan(m);
            mask[c] = m > 0.f ? inv : 0.f;
        }
    }
}

// ---- Linear, norm, and the gradient of both ---------------------------------------------------------------------------------------
// out[o] = <w[o][:], pooled> + bias[o], o < 256, on 16 waves: wave w takes output rows 16 w .. 16 w + 15, four rows (48 loads) in
// flight per trip (round 6: with one 4-wave workgroup per clip a batch of 32 clips kept 128 waves busy streaming the 786 KB of W
// each: 66 us per launch, all of it load latency).  A row's dot product is one wave's: lane l multiplies elements l + 64 i in the
// order i = 0 .. 11, then the wave sum.  Starts with a barrier (pooled is complete behind it); out is complete behind the next.
__device__ __forceinline__ void head_linear(const float* __restrict__ pooled, const float* __restrict__ w, const float* __restrict__ bias,
                                            float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
            if (lane == 0) out[o0 + u] = d + bias[o0 + u];
        }
    }
}

// dst[0 .. 255] = e / max(|e|, 1e-12): the squared norm is summed by waves 0 .. 3 over e[64 w ..] and folded (w0 + w1) + (w2 + w3).
// Starts with a barrier (e is complete behind it).
__device__ __forceinline__ void head_normalize_store(const float* __restrict__ e, float* __restrict__ wsum, float* __restrict__ dst) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();
    if (tid < 256) {
        const float v = e[tid];
        const float ss = wave_sum(v * v);
        if (lane == 0) wsum[wave] = ss;
    }
    __syncthreads();
    if (tid < 256) {
        const float nrm = sqrtf((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
        dst[tid] = e[tid] / fmaxf(nrm, 1e-12f);  // F.normalize eps
    }
}

// The backward of one row from z = W pooled + b and de = d loss / d normalize(z): nrm and e as the forward forms them, <e, de>,
// dz = (de - e <e, de>) / nrm (left in dz[256]), dp[c] = sum_o W[o][c] dz[o] in four fixed slices of 64 rows (slice q = tid / 256
// takes o = 64 q .. 64 q + 63 for the columns tid % 256 + 256 j, coalesced over c) folded (s0 + s1) + (s2 + s3) through `part`,
// which the time sum no longer needs; pooled[c] = dp[c] mask[c] (pooled is dead: it carries the row out).  1024 threads.  Starts
// with a barrier (z is complete behind it) and ends with one (pooled and dz are).
__device__ __forceinline__ void head_grad_row(const float* __restrict__ z, const float* __restrict__ de, const float* __restrict__ w,
                                              const float* __restrict__ mask, float* __restrict__ pooled, HeadPart& part,
                                              float* __restrict__ dz, float* __restrict__ red, float* __restrict__ red2) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float(*psum)[768] = part_floats(part);
    __syncthreads();
    float zv = 0.f, dev = 0.f;
    if (tid < 256) {
        zv = z[tid];
        dev = de[tid];
        const float ss = wave_sum(zv * zv);
        if (lane == 0) red[wave] = ss;
    }
    __syncthreads();
    const float nrm = fmaxf(sqrtf((red[0] + red[1]) + (red[2] + red[3])), 1e-12f);
    const float ev = zv / nrm;
    if (tid < 256) {
        const float dot = wave_sum(ev * dev);
        if (lane == 0) red2[wave] = dot;
    }
    __syncthreads();
    if (tid < 256) {
        const float edot = (red2[0] + red2[1]) + (red2[2] + red2[3]);
        dz[tid] = (dev - ev * edot) / nrm;
    }
    __syncthreads();
    {
        const int q = tid >> 8, c0 = tid & 255;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll 8
        for (int o = 64 * q; o < 64 * q + 64; ++o) {
            const float* wr = w + (long long)o * 768;
            const float dzo = dz[o];
            d0 = fmaf(wr[c0], dzo, d0); d1 = fmaf(wr[c0 + 256], dzo, d1); d2 = fmaf(wr[c0 + 512], dzo, d2);
        }
        psum[q][c0] = d0; psum[q][c0 + 256] = d1; psum[q][c0 + 512] = d2;
    }
    __syncthreads();
    if (tid < 768) {
        const float d = (psum[0][tid] + psum[1][tid]) + (psum[2][tid] + psum[3][tid]);
        pooled[tid] = d * mask[tid];
    }
    __syncthreads();
}

// ---- forward kernels ----------------------------------------------------------------------------------------------------------------
// Whole clips in two stages.  Stage 1, head_pool_kernel: the time sum of a clip in chunks of kHeadChunk frames, one workgroup per
// (chunk, clip), so that a 30 s clip (T = 1499) is summed by 24 workgroups instead of one thread column walking 1499 rows (452 us
// for a batch of 32 such clips with the single-stage kernel, 40 x the time of reading the 74 MB once).  A chunk is summed as
// head_sum_rows sums it (head_partial_sums, head_fold_0123).  Chunk j of clip b (rows r0 .. r0 + T - 1 of x) goes to slot
// r0 / 64 + b + j of `pool` - unique for packed clips of any lengths, at most M / 64 + B slots.  The summation order depends on T
// only: batch-invariant and deterministic.
template <typename TIn = float>
__global__ __launch_bounds__(256) void head_pool_kernel(const TIn* __restrict__ x, int T, float* __restrict__ pool,
                                                        const int* __restrict__ tpref = nullptr) {
    __shared__ HeadPart part;
    const int b = blockIdx.y, j = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row0 = head_clip(tpref, b, T);
    if (j * kHeadChunk >= T) return;
    ConsecutiveFrames fr;
    head_partial_sums<TIn>(x + row0 * 768, fr, j * kHeadChunk, min(T, (j + 1) * kHeadChunk), part, lane, wave);
    __syncthreads();
    if (wave == 0) {
        float4 a[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) a[q] = head_fold_0123(part, q, lane);
        head_row_store(a, pool + (row0 / kHeadChunk + b + j) * 768, lane);
    }
}

// A clip's chunk sums of stage 1 added in chunk order, by 256 threads: thread `tid` the columns tid, tid + 256, tid + 512.
__device__ __forceinline__ void head_clip_sums(const float* __restrict__ pool, long long row0, int b, int T, float (&s)[3]) {
    const float* pb = pool + (row0 / kHeadChunk + b) * 768;
    const int nchunk = (T + kHeadChunk - 1) / kHeadChunk, tid = threadIdx.x;
    s[0] = s[1] = s[2] = 0.f;
    for (int j = 0; j < nchunk; ++j) {  // chunks in order
        const float* r = pb + (long long)j * 768;
        s[0] += r[tid];
        s[1] += r[tid + 256];
        s[2] += r[tid + 512];
    }
}

// Stage 2.  grid: B blocks of 1024 threads.  pool (stage 1) -> emb [B][256].
__global__ __launch_bounds__(1024) void head_kernel(const float* __restrict__ pool, int T, const float* __restrict__ w,
                                                    const float* __restrict__ bias, float* __restrict__ emb,
                                                    const int* __restrict__ tpref = nullptr) {
    __shared__ float pooled[768];
    __shared__ float e[256];
    __shared__ float wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long row0 = head_clip(tpref, b, T);
    if (tid < 256) {
        float s[3];
        head_clip_sums(pool, row0, b, T, s);
        const float inv = 1.0f / (float)T;
#pragma unroll
        for (int j = 0; j < 3; ++j) pooled[tid + 256 * j] = relu_keep_nan(s[j] * inv);
    }
    head_linear(pooled, w, bias, e);
    head_normalize_store(e, wsum, emb + (long long)b * 256);
}

// Stage 2 of the pooled backbone features (Origw2v.forward, networks.py:29-34: res['x'].mean(1), no ReLU, no Linear, no
// normalisation).  grid: B blocks of 256 threads.  pool (stage 1) -> feat [B][768]: a clip's chunks folded in order and
// `sum * (1 / T)`, the expression head_kernel forms before its ReLU.
__global__ __launch_bounds__(256) void head_mean_kernel(const float* __restrict__ pool, int T, float* __restrict__ feat,
                                                        const int* __restrict__ tpref = nullptr) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long row0 = head_clip(tpref, b, T);
    float s[3];
    head_clip_sums(pool, row0, b, T, s);
    const float inv = 1.0f / (float)T;
#pragma unroll
    for (int j = 0; j < 3; ++j) feat[(long long)b * 768 + tid + 256 * j] = s[j] * inv;
}

// The head over rows of frames - windows (WindowRows) or rows of spans (SpanRows) - both stages in one workgroup: one row of emb
// per workgroup, in the arithmetic of head_pool_kernel + head_kernel applied to the row's frames as if they were a clip of their
// own.  So a window that covers a whole clip, and a span row whose spans concatenate to it, have the bits of that clip's embedding;
// a row of one span [a, a + n) has the bits of a window over those frames (only the frame mapping differs, and a window's is the
// address add); and a row's 256 values are a function of its own frames only.  Overlapping rows re-read their frames from L2.
// grid: (windows of the longest clip, B) or (R) blocks of 1024 threads.
template <typename TIn, class Rows>
__global__ __launch_bounds__(1024) void head_rows_kernel(const TIn* __restrict__ x, Rows rows, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ emb) {
    __shared__ HeadPart part;
    __shared__ float pooled[768];
    __shared__ float e[256];
    __shared__ float wsum[4];
    typename Rows::Row r = rows.row();
    if (!r.valid) return;
    float4 run[3];
    head_sum_rows<TIn>(x + r.first * 768, r.frames, r.n, part, run);
    head_pooled_from_sum(run, r.n, pooled, nullptr);
    head_linear(pooled, w, bias, e);
    head_normalize_store(e, wsum, emb + r.out * 256);
}

// ---- backward kernels ---------------------------------------------------------------------------------------------------------------
// e = normalize(W relu(mean_t x) + b).  Given de -> gx[b][t][:] = relu'(mean) * (W^T dz) / T for every t.
// grid: B blocks of 1024 threads (round 6: 16 waves - with 4 the kernel took 55 us for the 32 clips of configs[3], all of it the
// latency of streaming W twice through 128 waves).  The time sum is head_pooled_one_pass - NOT the forward's chunked sum, see
// there; z = W pooled + b as in head_kernel; then head_grad_row.  pooled_out / dz_out: what the head's own parameter gradients
// need (train.hip.h: head_param_grad_kernel).
__global__ __launch_bounds__(1024) void head_bwd_kernel(const float* __restrict__ x, int T, const float* __restrict__ w,
                                                        const float* __restrict__ bias, const float* __restrict__ de,
                                                        float* __restrict__ gx, float* __restrict__ pooled_out = nullptr,
                                                        float* __restrict__ dz_out = nullptr,
                                                        const int* __restrict__ tpref = nullptr) {
    __shared__ float mask[768], z[256], dz[256], red[4], red2[4];
    __shared__ __attribute__((aligned(16))) float pooled[768];   // (read as float4)
    __shared__ HeadPart part;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = head_clip(tpref, b, T);
    head_pooled_one_pass(x + row0 * 768, T, part, pooled, mask);
    if (dz_out && tid < 256) {   // (a thread's own three columns)
#pragma unroll
        for (int j = 0; j < 3; ++j) pooled_out[(long long)b * 768 + tid + 256 * j] = pooled[tid + 256 * j];
    }
    head_linear(pooled, w, bias, z);
    head_grad_row(z, de + (long long)b * 256, w, mask, pooled, part, dz, red, red2);
    if (dz_out && tid < 256) dz_out[(long long)b * 256 + tid] = dz[tid];
    float4 gv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) gv[i] = reinterpret_cast<const float4*>(pooled)[lane + 64 * i];
    for (int t = wave; t < T; t += 16) head_row_store(gv, gx + (row0 + t) * 768, lane);
}

// The backward of head_rows_kernel in two launches, no atomics.  Stage 1, head_rows_bwd_kernel: row `out` of de [rows][256] ->
// gw[out][c] = (mean_c > 0 ? 1 / n : 0) (W^T dz)[c], the gradient of the row's time MEAN's columns spread over its n frames: what
// every frame of the row receives from it.  grid and row order: the forward's.  The time sum is the forward's own code, so pooled
// and the ReLU mask have the forward's bits; from there head_bwd_kernel's.  Every row of gw is written whole.
template <class Rows>
__global__ __launch_bounds__(1024) void head_rows_bwd_kernel(const float* __restrict__ x, Rows rows, const float* __restrict__ w,
                                                             const float* __restrict__ bias, const float* __restrict__ de,
                                                             float* __restrict__ gw) {
    __shared__ float mask[768], z[256], dz[256], red[4], red2[4];
    __shared__ __attribute__((aligned(16))) float pooled[768];   // (read as float4)
    __shared__ HeadPart part;
    typename Rows::Row r = rows.row();
    if (!r.valid) return;
    float4 run[3];
    head_sum_rows<float>(x + r.first * 768, r.frames, r.n, part, run);
    head_pooled_from_sum(run, r.n, pooled, mask);
    head_linear(pooled, w, bias, z);
    head_grad_row(z, de + r.out * 256, w, mask, pooled, part, dz, red, red2);
    if (threadIdx.x < 192) reinterpret_cast<float4*>(gw + r.out * 768)[threadIdx.x] = reinterpret_cast<const float4*>(pooled)[threadIdx.x];
}

// Stage 2, the scatter: gx[frame t of clip b][:] = the sum of the gw rows whose frames contain t, rows ascending into one fp32
// accumulator.  A frame no row contains gets exact zeros: EVERY row of gx is written, nothing is assumed cleared.
// grid: (ceil(frames of the longest clip / 4), B) blocks of 256 threads, one wave per frame, lane l the float4s l, l + 64, l + 128
// of the row.  Which rows contain t is the two kernels' own:
// windows - the consecutive windows k_lo .. k_hi of head_window_cover, so the order depends on (T, win, hop, t) only; none in a gap
// between windows (hop > win) or in the tail behind the last full window.
__global__ __launch_bounds__(256) void head_windows_scatter_kernel(const float* __restrict__ gw, WindowRows rows, float* __restrict__ gx) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
    int T = rows.T;
    const long long row0 = head_clip(rows.tpref, b, T);
    if ((int)blockIdx.x * 4 >= T) return;   // the same for every thread of the block
    const long long wbase = rows.wbase<256>(b, T);
    if (t >= T) return;
    int k_lo, k_hi;
    head_window_cover(T, rows.win, rows.hop, t, &k_lo, &k_hi);
    float4 acc[3];
    head_row_zero(acc);
    for (int k = k_lo; k <= k_hi; ++k) head_row_add<float>(acc, gw + (wbase + k) * 768, lane);
    head_row_store(acc, gx + (row0 + t) * 768, lane);
}

// spans - the rows r of clip b (clip_row[b] .. clip_row[b + 1] - 1) one of whose spans contains t: the row's spans are scanned per
// frame, every lane of a wave on the same frame; every frame of a clip without a row gets zeros.
__global__ __launch_bounds__(256) void head_spans_scatter_kernel(const float* __restrict__ gw, SpanRows rows, float* __restrict__ gx) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
    int T = 0;
    const long long row0 = head_clip(rows.tpref, b, T);
    if (t >= T) return;
    const SpanTable tb = span_table(rows.tab, rows.R, rows.S);
    float4 acc[3];
    head_row_zero(acc);
    for (int r = tb.clip_row[b]; r < tb.clip_row[b + 1]; ++r) {
        bool in = false;
        for (int i = tb.row_ptr[r]; i < tb.row_ptr[r + 1] && tb.spans[2 * i] <= t; ++i) in = in || t < tb.spans[2 * i + 1];
        if (in) head_row_add<float>(acc, gw + (long long)r * 768, lane);
    }
    head_row_store(acc, gx + (row0 + t) * 768, lane);
}

}  // namespace nomad
