// Degradations on packed clips: additive noise at a target SNR and percentile clipping, G levels of each per clip, written
// straight into the (B G, stride) layout nomad_embed_ragged reads (row b G + g = clip b at level g).  The arithmetic is the
// reference's utils/degradations.py restated (include/nomad_hip.h states both formulas); everything here is per clip, so a clip's
// rows never depend on the batch it is in.
//
// Clipping needs np.percentile's linear rule on the clip's own samples, i.e. EXACT order statistics - up to 4 G of them per clip.
// degrade_sort_kernel sorts each clip: one workgroup of 1024 threads per clip, an LSD radix sort of order-preserving 32-bit keys
// in 4 passes of 8 bits between two key rows in the caller's scratch.  The clip is streamed in chunks of 1024 keys (a 10 s clip
// is 640 KB of keys, four times the LDS); per chunk a key's place is
//     base[digit] (keys of smaller digits + this digit's keys of earlier chunks) + this digit's keys of lower waves of the chunk
//     + its rank among the lanes of its wave with the same digit (8 ballots),
// which is stable, and all of it is integer arithmetic on LDS counters each written by one lane - no atomics in the scatter.  The
// four digit histograms come from one pass over the samples ahead of the scatters (integer LDS atomics: the counts do not depend
// on the order of arrival).  After the sort every rank of every level is one load, so G does not enter the sort's cost.
//
// Bound.  Per sample the sort reads 4 bytes for the histograms and reads + writes 4 bytes in each of 4 passes: 36 bytes, all of
// which stay in L2 for the clips of one batch (64 clips of 10 s: 2 x 41 MB of keys).  The limit is not bytes: a clip is ONE
// workgroup, so a batch of B clips occupies B of the 256 CUs, and each chunk of 1024 keys costs four workgroup barriers and a
// 16-step serial LDS scan per digit.  Splitting a clip over several workgroups (a global digit scan per pass) is the next lever.
// The write kernels stream: 4 bytes read and 4 G bytes written per sample.
#pragma once
#include <hip/hip_runtime.h>

namespace nomad {

constexpr int kDegradeMaxLevels = 64;
constexpr int kDegradeThreads = 1024;   // one workgroup per clip in the sort and in the noise statistics
constexpr int kDegradeWaves = kDegradeThreads / 64;

// float32 bits -> a key whose unsigned order is numpy's sort order: negatives below positives, -0.0 directly below +0.0 (numpy
// calls them equal; no threshold can tell which comes first), every NaN - of either sign - as the one largest key.
__device__ __forceinline__ unsigned degrade_key(float v) {
    const unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float degrade_unkey(unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

// numpy's default (linear) percentile on sorted keys: h = (n - 1) q with q = p / 100 formed on the host, v = a + (b - a) t in
// float64 with two roundings, as numpy's own a + (b - a) * t has - no fused multiply-add.
__device__ __forceinline__ double degrade_percentile(const unsigned* sorted, int n, double q) {
#pragma clang fp contract(off)
    const double h = (double)(n - 1) * q;
    const double fl = floor(h);
    int lo = (int)fl;
    lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);   // q lies in [0, 1]: a clamp that never binds, kept so that no index leaves the clip
    const int hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
    const double t = h - fl;
    const double a = (double)degrade_unkey(sorted[lo]), b = (double)degrade_unkey(sorted[hi]);
    const double d = (b - a) * t;
    return a + d;
}

// One workgroup per clip.  x [B][stride] fp32, lens [B]; keys0 / keys1 [B][stride] key rows (scratch; the sorted clip ends in
// keys0); q [2 G] = (p_lo / 100, p_hi / 100) per level; thr [B][G][2] float64 (scratch) and thr_out (the caller's copy, or null).
__global__ __launch_bounds__(kDegradeThreads) void degrade_sort_kernel(const float* __restrict__ x, int stride, const int* __restrict__ lens,
                                                                       unsigned* __restrict__ keys0, unsigned* __restrict__ keys1,
                                                                       const double* __restrict__ q, int G, double* __restrict__ thr,
                                                                       double* __restrict__ thr_out) {
    __shared__ unsigned hist[4][256];               // digit counts of the 4 passes, then their exclusive prefix sums
    __shared__ unsigned wave_cnt[kDegradeWaves][256];  // per chunk: this digit's keys in each wave, then where each wave's begin
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lens[b];
    const size_t row = (size_t)b * (size_t)stride;
    const float* xr = x + row;
    unsigned* k0 = keys0 + row;
    unsigned* k1 = keys1 + row;

    for (int i = tid; i < 4 * 256; i += kDegradeThreads) (&hist[0][0])[i] = 0u;
    __syncthreads();
    for (int i = tid; i < n; i += kDegradeThreads) {
        const unsigned k = degrade_key(xr[i]);
        atomicAdd(&hist[0][k & 255u], 1u);
        atomicAdd(&hist[1][(k >> 8) & 255u], 1u);
        atomicAdd(&hist[2][(k >> 16) & 255u], 1u);
        atomicAdd(&hist[3][k >> 24], 1u);
    }
    __syncthreads();
    if (tid < 4) {   // exclusive prefix sums, 256 steps each
        unsigned run = 0u;
        for (int d = 0; d < 256; ++d) {
            const unsigned c = hist[tid][d];
            hist[tid][d] = run;
            run += c;
        }
    }
    __syncthreads();

    for (int pass = 0; pass < 4; ++pass) {
        const unsigned* src = (pass & 1) ? k1 : k0;   // pass 0 reads the samples themselves instead
        unsigned* dst = (pass & 1) ? k0 : k1;         // x -> k1 -> k0 -> k1 -> k0
        const int shift = 8 * pass;
        unsigned base = tid < 256 ? hist[pass][tid] : 0u;   // thread d < 256 carries digit d's next free place through the chunks
        for (int c0 = 0; c0 < n; c0 += kDegradeThreads) {
            for (int i = tid; i < kDegradeWaves * 256; i += kDegradeThreads) (&wave_cnt[0][0])[i] = 0u;
            __syncthreads();
            const int i = c0 + tid;
            const bool valid = i < n;
            unsigned key = 0u;
            if (valid) key = pass == 0 ? degrade_key(xr[i]) : src[i];
            const unsigned d = (key >> shift) & 255u;
            unsigned long long peers = __ballot(valid);
            for (int bit = 0; bit < 8; ++bit) {
                const bool one = (d >> bit) & 1u;
                const unsigned long long m = __ballot(one);
                peers &= one ? m : ~m;
            }
            const unsigned rank = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
            const unsigned count = (unsigned)__popcll(peers);
            if (valid && rank + 1u == count) wave_cnt[wave][d] = count;   // the digit's last lane of the wave: one writer per counter
            __syncthreads();
            if (tid < 256) {
                unsigned run = base;
                for (int w = 0; w < kDegradeWaves; ++w) {
                    const unsigned c = wave_cnt[w][tid];
                    wave_cnt[w][tid] = run;
                    run += c;
                }
                base = run;
            }
            __syncthreads();
            if (valid) {
                const unsigned pos = wave_cnt[wave][d] + rank;
                if (pos < (unsigned)n) dst[pos] = key;   // always true (the histograms count these very keys); no store leaves the row
            }
            __syncthreads();
        }
        // the barrier above also orders this pass's global stores before the next pass's loads (one workgroup, one CU)
    }
    // the sorted clip is in k0
    for (int j = tid; j < 2 * G; j += kDegradeThreads) {
        const double v = degrade_percentile(k0, n, q[j]);
        thr[(size_t)b * 2 * G + j] = v;
        if (thr_out) thr_out[(size_t)b * 2 * G + j] = v;
    }
}

// out[b G + g][i] = x > v_hi ? (float)v_hi : x < v_lo ? (float)v_lo : x, compared in float64; zeros behind the clip's length.
// Grid (ceil(stride / 256), B), 256 threads: a thread reads its sample once and writes it at every level.
__global__ __launch_bounds__(256) void degrade_clip_write_kernel(const float* __restrict__ x, int stride, const int* __restrict__ lens,
                                                                 const double* __restrict__ thr, int G, float* __restrict__ out) {
    __shared__ double sthr[2 * kDegradeMaxLevels];
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    for (int j = threadIdx.x; j < 2 * G; j += 256) sthr[j] = thr[(size_t)b * 2 * G + j];
    __syncthreads();
    if (i >= stride) return;
    const bool valid = i < lens[b];
    const float xf = valid ? x[(size_t)b * stride + i] : 0.0f;
    const double xd = (double)xf;
    float* o = out + (size_t)b * G * stride + i;
    for (int g = 0; g < G; ++g) {
        const double vlo = sthr[2 * g], vhi = sthr[2 * g + 1];
        const float y = xd > vhi ? (float)vhi : xd < vlo ? (float)vlo : xf;
        o[(size_t)g * stride] = valid ? y : 0.0f;
    }
}

// alpha[b][g] = (xp / ratio[g]) / sp with xp = sqrt(mean x^2), sp = sqrt(mean s[i mod Ls]^2), both means over the clip's n samples,
// ratio[g] = 10^(snr_db[g] / 10) formed on the host.  One workgroup per clip: thread t sums the squares of samples t, t + 1024, ...
// in float64 (the square of a float is exact in float64), the 1024 partial sums are folded by halves in LDS - an order fixed by n
// alone.  No special cases: a silent clip or silent noise gives what IEEE arithmetic gives.
__global__ __launch_bounds__(kDegradeThreads) void degrade_noise_alpha_kernel(const float* __restrict__ x, int stride, const int* __restrict__ lens,
                                                                              const float* __restrict__ noise, int Ls,
                                                                              const double* __restrict__ ratio, int G,
                                                                              double* __restrict__ alpha, double* __restrict__ alpha_out) {
    __shared__ double sx[kDegradeThreads], ss[kDegradeThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = lens[b];
    const float* xr = x + (size_t)b * (size_t)stride;
    double ax = 0.0, as = 0.0;
    for (int i = tid; i < n; i += kDegradeThreads) {
        const double xv = (double)xr[i], sv = (double)noise[i % Ls];
        ax += xv * xv;
        as += sv * sv;
    }
    sx[tid] = ax;
    ss[tid] = as;
    __syncthreads();
    for (int half = kDegradeThreads / 2; half > 0; half >>= 1) {
        if (tid < half) {
            sx[tid] += sx[tid + half];
            ss[tid] += ss[tid + half];
        }
        __syncthreads();
    }
    if (tid < G) {
        const double xp = sqrt(sx[0] / (double)n), sp = sqrt(ss[0] / (double)n);
        const double a = (xp / ratio[tid]) / sp;
        alpha[(size_t)b * G + tid] = a;
        if (alpha_out) alpha_out[(size_t)b * G + tid] = a;
    }
}

// out[b G + g][i] = (float)((double)x[i] + alpha[b][g] * (double)s[i mod Ls]): product and sum rounded separately in float64, then
// once to fp32; zeros behind the clip's length.  Grid and threads as degrade_clip_write_kernel.
__global__ __launch_bounds__(256) void degrade_noise_write_kernel(const float* __restrict__ x, int stride, const int* __restrict__ lens,
                                                                  const float* __restrict__ noise, int Ls, const double* __restrict__ alpha,
                                                                  int G, float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double sal[kDegradeMaxLevels];
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    for (int j = threadIdx.x; j < G; j += 256) sal[j] = alpha[(size_t)b * G + j];
    __syncthreads();
    if (i >= stride) return;
    const bool valid = i < lens[b];
    const double xd = valid ? (double)x[(size_t)b * stride + i] : 0.0;
    const double sd = valid ? (double)noise[i % Ls] : 0.0;
    float* o = out + (size_t)b * G * stride + i;
    for (int g = 0; g < G; ++g) {
        const double p = sal[g] * sd;
        o[(size_t)g * stride] = valid ? (float)(xd + p) : 0.0f;
    }
}

}  // namespace nomad
