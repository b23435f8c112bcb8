// Gammatone spectrograms of packed rows and the NSIM of a clean spectrogram with its degraded ones: the similarity the reference
// takes from ViSQOL for every (clean, degraded) pair before it samples triplets (src/utils/nsim_triplet_sampling.py).  Modelled on
// what ViSQOL's speech mode is remembered to do, NOT checked against the ViSQOL binary; include/nomad_hip.h states the measure in
// full and is the definition.  Works on the [R][stride] rows the degrade_* calls write.
//
// gammatone_frames_kernel - the hot path.  A (frame, band) value is one recurrence of W = 4 H steps (H = fs / 50) through four
// second-order sections in float64 from the zero state: 16 multiply-adds per step, four of them in a row inside one section and the
// four sections in a row behind each other.  The mapping and its reasons:
//   * one lane per (frame, band), a wave = kGammatoneWaveFrames = 3 frames x 21 bands (63 of 64 lanes busy), a workgroup = 4 waves =
//     kGammatoneBlockFrames = 12 consecutive frames of one row.  The 21 bands of a frame read the same sample at every step, so a
//     wave's LDS read has three distinct addresses and the rest is broadcast.
//   * the workgroup's span of samples, W + (k - 1) H for its k <= 12 frames, is staged in LDS once as fp32 (the conversion to
//     float64 is exact and costs one instruction of the seventeen per step): 19.2 KB at 16 kHz, 57.6 KB at 48 kHz, so eight resp.
//     two workgroups share a CU and every SIMD has waves to switch between while a float64 result is on its way.  The span is kept
//     as rows of H samples with one float of padding behind each: the three frames of a wave then sit H + 1 floats apart, on three
//     different banks (H is a multiple of 32 at the usual rates, and ds_read_b32 has 32 banks: unpadded, the frames of a lane group
//     would collide at every step).
//   * the cascade is skewed: at step i section j works on sample i - j, on what section j - 1 put out the step before.  The four
//     sections of a step are then independent of each other and the dependent chain of a step is one section's (three operations)
//     instead of four sections'.  Every operation, its operands and the order of the sum of squares are those of the plain cascade.
//   * no atomics, one fixed order: a value depends on its own W samples and the rate, so a row has the bits of its own R = 1 call
//     whatever the batch, the stride and the base address.  Rows are read sample by sample (4-byte alignment is all they need) and
//     only the samples of whole frames are read: nothing behind a length.
// A non-finite sample makes the frames that hold it NaN: every lane multiplies its samples by zero into a check value on the way.
//
// nsim_kernel - one workgroup per degraded row, 256 threads; the clean spectrogram is read by each of its G rows and computed
// once.  Phases, a barrier between each, planes in the workspace ([F][21] float64 per row: clean dB, degraded dB, map):
//   dB and the absolute floor (one thread per value) -> the per-frame peak over both and the relative floor (one thread per frame,
//   bands in ascending order, clean first) -> the minimum over both (per-thread minima in index order, folded in LDS by halves; a
//   minimum does not depend on its order, and a NaN is carried by a flag beside it) -> subtract -> the map (one thread per value) ->
//   the band means: thread b walks column b over the F frames in ascending order (a SEQUENTIAL walk, no fold), thread 0 then adds
//   the 21 band values in ascending order.  Every order depends on F alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace nomad {

constexpr int kGammatoneBands = 21;
constexpr int kGammatoneWaveFrames = 3;     // frames per wave: 3 x 21 = 63 lanes
constexpr int kGammatoneBlockFrames = 12;   // frames per workgroup of 4 waves (tests/test_gpu_gammatone.py reads this line)
static_assert(kGammatoneBlockFrames == 4 * kGammatoneWaveFrames && kGammatoneWaveFrames * kGammatoneBands <= 64, "lane mapping");
constexpr int kGammatoneCoefs = 10;                              // per band: b0[4], b1[4], a1, a2
constexpr int kGammatoneMinRate = 16000, kGammatoneMaxRate = 48000;

inline bool gammatone_rate_ok(int fs) { return fs >= kGammatoneMinRate && fs <= kGammatoneMaxRate && fs % 50 == 0; }

// The bank for the sample rate fs: coef[band][10] = numerators b0 and b1 of the four sections (the gain divided into the first
// section's), then the common a1 and a2.  Band 0 is the lowest.  Host, float64 (complex arithmetic written out).
inline void gammatone_bank(int fs, double* coef, double* centres) {
    const double pi = 3.14159265358979323846;
    const double EarQ = 9.26449, minBW = 24.7, lo = 50.0, hi = 8000.0;
    const int N = kGammatoneBands;
    const double T = 1.0 / (double)fs;
    for (int band = 0; band < N; ++band) {
        const int i = N - band;   // Slaney's i = 1 .. N runs from the highest centre down
        const double cf = -(EarQ * minBW) + std::exp((double)i * (std::log(lo + EarQ * minBW) - std::log(hi + EarQ * minBW)) / (double)N) * (hi + EarQ * minBW);
        const double ERB = cf / EarQ + minBW, B = 1.019 * 2.0 * pi * ERB;
        const double c = std::cos(2.0 * pi * cf * T), s = std::sin(2.0 * pi * cf * T), e = std::exp(B * T);
        const double a1 = -2.0 * c / e, a2 = std::exp(-2.0 * B * T);
        const double rp = std::sqrt(3.0 + std::pow(2.0, 1.5)), rm = std::sqrt(3.0 - std::pow(2.0, 1.5));
        const double A1[4] = {-(2.0 * T * c / e + 2.0 * rp * T * s / e) / 2.0, -(2.0 * T * c / e - 2.0 * rp * T * s / e) / 2.0,
                              -(2.0 * T * c / e + 2.0 * rm * T * s / e) / 2.0, -(2.0 * T * c / e - 2.0 * rm * T * s / e) / 2.0};
        // the response of the cascade at z = exp(j 2 pi cf T): with u = 1 / z, prod_k (T + A1k u) / (1 + a1 u + a2 u^2)^4
        const double ur = c, ui = -s, u2r = ur * ur - ui * ui, u2i = 2.0 * ur * ui;
        const double dr = 1.0 + a1 * ur + a2 * u2r, di = a1 * ui + a2 * u2i;
        double pr = 1.0, pi_ = 0.0;
        for (int k = 0; k < 4; ++k) {
            const double nr = T + A1[k] * ur, ni = A1[k] * ui, den = dr * dr + di * di;
            const double qr = (nr * dr + ni * di) / den, qi = (ni * dr - nr * di) / den;
            const double tr = pr * qr - pi_ * qi, ti = pr * qi + pi_ * qr;
            pr = tr;
            pi_ = ti;
        }
        const double g = std::sqrt(pr * pr + pi_ * pi_);
        double* o = coef + kGammatoneCoefs * band;
        for (int k = 0; k < 4; ++k) {
            o[k] = k == 0 ? T / g : T;
            o[4 + k] = k == 0 ? A1[k] / g : A1[k];
        }
        o[8] = a1;
        o[9] = a2;
        if (centres) centres[band] = cf;
    }
}

// One sample through one section (transposed direct form II, b2 = 0): y = b0 x + z1; z1 = b1 x - a1 y + z2; z2 = -a2 y.
__device__ __forceinline__ double gammatone_section(double b0, double b1, double a1, double a2, double x, double& z1, double& z2) {
    const double y = b0 * x + z1;
    z1 = b1 * x - a1 * y + z2;
    z2 = -a2 * y;
    return y;
}

// Grid (ceil(max F / 12), R), 256 threads, dynamic LDS (W + 11 H) / H * (H + 1) floats.  Lane l < 63 of wave w: frame
// 12 blockIdx.x + 3 w + l / 21, band l % 21.  spec[fpref[r] + t][band] <- sqrt(sum_i y_i^2 / W).
__global__ __launch_bounds__(256) void gammatone_frames_kernel(const float* __restrict__ x, int stride, const int* __restrict__ lens,
                                                               const long long* __restrict__ fpref, const double* __restrict__ coef, int H,
                                                               double* __restrict__ spec) {
    extern __shared__ float gt_span[];
    const int r = blockIdx.y, t0 = blockIdx.x * kGammatoneBlockFrames;
    const int W = 4 * H, n = lens[r];
    const int F = (n - W) / H + 1;
    if (t0 >= F) return;   // the whole workgroup: no barrier is left behind
    const int k = F - t0 < kGammatoneBlockFrames ? F - t0 : kGammatoneBlockFrames;
    const int span = W + (k - 1) * H;   // (t0 + k - 1) H + W <= n: inside the row's length
    const float* xr = x + (size_t)r * (size_t)stride + (size_t)t0 * (size_t)H;
    for (int s = threadIdx.x; s < span; s += 256) gt_span[s + s / H] = xr[s];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = wave * kGammatoneWaveFrames + lane / kGammatoneBands, band = lane % kGammatoneBands;
    if (lane >= kGammatoneWaveFrames * kGammatoneBands || f >= k) return;
    const double* cb = coef + kGammatoneCoefs * band;
    const double b00 = cb[0], b01 = cb[1], b02 = cb[2], b03 = cb[3], b10 = cb[4], b11 = cb[5], b12 = cb[6], b13 = cb[7], a1 = cb[8], a2 = cb[9];
    double z10 = 0.0, z20 = 0.0, z11 = 0.0, z21 = 0.0, z12 = 0.0, z22 = 0.0, z13 = 0.0, z23 = 0.0;
    double acc = 0.0;
    float chk = 0.0f;   // 0 * x summed: NaN once a sample is not finite
    const float* p = gt_span + f * (H + 1);
    // the skewed cascade: y0, y1, y2 are what sections 0 .. 2 put out at the step before
    double y0, y1, y2;
    {   // steps 0 .. 2: the pipe fills
        float v = p[0];
        chk = fmaf(0.0f, v, chk);
        y0 = gammatone_section(b00, b10, a1, a2, (double)v, z10, z20);
        v = p[1];
        chk = fmaf(0.0f, v, chk);
        y1 = gammatone_section(b01, b11, a1, a2, y0, z11, z21);
        y0 = gammatone_section(b00, b10, a1, a2, (double)v, z10, z20);
        v = p[2];
        chk = fmaf(0.0f, v, chk);
        y2 = gammatone_section(b02, b12, a1, a2, y1, z12, z22);
        y1 = gammatone_section(b01, b11, a1, a2, y0, z11, z21);
        y0 = gammatone_section(b00, b10, a1, a2, (double)v, z10, z20);
    }
    for (int q = 0; q < 4; ++q) {
        const float* pq = p + q * (H + 1);
        for (int i = q == 0 ? 3 : 0; i < H; ++i) {
            const float v = pq[i];
            chk = fmaf(0.0f, v, chk);
            const double y3 = gammatone_section(b03, b13, a1, a2, y2, z13, z23);
            y2 = gammatone_section(b02, b12, a1, a2, y1, z12, z22);
            y1 = gammatone_section(b01, b11, a1, a2, y0, z11, z21);
            y0 = gammatone_section(b00, b10, a1, a2, (double)v, z10, z20);
            acc += y3 * y3;
        }
    }
    {   // steps W .. W + 2: the pipe drains
        double y3 = gammatone_section(b03, b13, a1, a2, y2, z13, z23);
        y2 = gammatone_section(b02, b12, a1, a2, y1, z12, z22);
        y1 = gammatone_section(b01, b11, a1, a2, y0, z11, z21);
        acc += y3 * y3;
        y3 = gammatone_section(b03, b13, a1, a2, y2, z13, z23);
        y2 = gammatone_section(b02, b12, a1, a2, y1, z12, z22);
        acc += y3 * y3;
        y3 = gammatone_section(b03, b13, a1, a2, y2, z13, z23);
        acc += y3 * y3;
    }
    const double S = chk != chk ? (double)NAN : sqrt(acc / (double)W);
    spec[((size_t)fpref[r] + (size_t)(t0 + f)) * kGammatoneBands + band] = S;
}

// ---- NSIM ----
// max / min that a NaN enters and never leaves (no comparison with a NaN is true).
__device__ __forceinline__ double nsim_max(double a, double b) { return (b > a || b != b) ? b : a; }   // a NaN in a stays: b > NaN is false
__device__ __forceinline__ double nsim_min(double a, double b) { return (b < a || b != b) ? b : a; }

__device__ __forceinline__ double nsim_db(double s) {
    const double eps = 2.220446049250313e-16;   // 2^-52
    const double v = nsim_max(eps, s);
    return nsim_max(-45.0, 10.0 * log10(v));
}

// The 3 x 3 window over plane a (and the products with plane b) at (t, band), edges replicated; the nine terms row by row of the
// window: frames t - 1, t, t + 1 outside, bands band - 1, band, band + 1 inside.
__device__ __forceinline__ void nsim_window(const double* __restrict__ R, const double* __restrict__ D, int F, int t, int band, double& mr,
                                            double& md, double& rr, double& dd, double& rd) {
    const double w[3][3] = {{0.0113, 0.0838, 0.0113}, {0.0838, 0.6193, 0.0838}, {0.0113, 0.0838, 0.0113}};
    mr = md = rr = dd = rd = 0.0;
    for (int dt = -1; dt <= 1; ++dt) {
        int tt = t + dt;
        tt = tt < 0 ? 0 : tt >= F ? F - 1 : tt;
        for (int db = -1; db <= 1; ++db) {
            int bb = band + db;
            bb = bb < 0 ? 0 : bb >= kGammatoneBands ? kGammatoneBands - 1 : bb;
            const double a = R[(size_t)tt * kGammatoneBands + bb], b = D[(size_t)tt * kGammatoneBands + bb], ww = w[dt + 1][db + 1];
            mr += ww * a;
            md += ww * b;
            rr += ww * (a * a);
            dd += ww * (b * b);
            rd += ww * (a * b);
        }
    }
}

// The map at (t, band) from the floored planes with their minimum subtracted: what nsim_kernel and the patch search
// (nsim_patches.hip.h) both evaluate, so that a patch candidate has the bits of a nomad_nsim call on the cut-out pair.
__device__ __forceinline__ double nsim_cell(const double* __restrict__ R, const double* __restrict__ D, int F, int t, int band, double C1,
                                            double C3) {
    double mr, md, rr, dd, rd;
    nsim_window(R, D, F, t, band, mr, md, rr, dd, rd);
    double vr = rr - mr * mr, vd = dd - md * md;
    vr = vr < 0.0 ? 0.0 : vr;   // a NaN is not below 0: it stays
    vd = vd < 0.0 ? 0.0 : vd;
    const double cov = rd - mr * md;
    return (2.0 * mr * md + C1) / (mr * mr + md * md + C1) * ((cov + C3) / (sqrt(vr) * sqrt(vd) + C3));
}

// The two walks: a band's column of the map over the F frames in ascending order, and the 21 band values in ascending order.
__device__ __forceinline__ double nsim_band_mean(const double* __restrict__ M, int F, int band) {
    double acc = 0.0;
    for (int t = 0; t < F; ++t) acc += M[(size_t)t * kGammatoneBands + band];
    return acc / (double)F;
}
__device__ __forceinline__ double nsim_of_bands(const double* __restrict__ band_mean) {
    double acc = 0.0;
    for (int k = 0; k < kGammatoneBands; ++k) acc += band_mean[k];
    return acc / (double)kGammatoneBands;
}

// Grid B G, 256 threads.  Degraded row j = b G + g: clean frames spec_ref[fpref[b] ..][21], its own spec_deg[G fpref[b] + g F_b ..][21];
// planes: [3][G total][21] float64 at the row's own offset.  nsim[j], bands[j][21] (or null).
__global__ __launch_bounds__(256) void nsim_kernel(const double* __restrict__ spec_ref, const double* __restrict__ spec_deg, int G,
                                                   const int* __restrict__ frames, const long long* __restrict__ fpref, long long total,
                                                   double C1, double C3, double* __restrict__ planes, double* __restrict__ nsim,
                                                   double* __restrict__ bands) {
    __shared__ double red[256];
    __shared__ int bad[256];
    __shared__ double band_mean[kGammatoneBands];
    const int j = blockIdx.x, b = j / G, g = j % G, tid = threadIdx.x;
    const int F = frames[b];
    const size_t at = (size_t)G * (size_t)fpref[b] + (size_t)g * (size_t)F, plane = (size_t)G * (size_t)total * kGammatoneBands;
    const double* sr = spec_ref + (size_t)fpref[b] * kGammatoneBands;
    const double* sd = spec_deg + at * kGammatoneBands;
    double* R = planes + at * kGammatoneBands;
    double* D = R + plane;
    double* M = D + plane;
    const int n = F * kGammatoneBands;
    for (int i = tid; i < n; i += 256) {
        R[i] = nsim_db(sr[i]);
        D[i] = nsim_db(sd[i]);
    }
    __syncthreads();
    for (int t = tid; t < F; t += 256) {
        double* rt = R + (size_t)t * kGammatoneBands;
        double* dt = D + (size_t)t * kGammatoneBands;
        double peak = rt[0];
        for (int k = 1; k < kGammatoneBands; ++k) peak = nsim_max(peak, rt[k]);
        for (int k = 0; k < kGammatoneBands; ++k) peak = nsim_max(peak, dt[k]);
        const double floor_t = peak - 45.0;
        for (int k = 0; k < kGammatoneBands; ++k) {
            rt[k] = nsim_max(floor_t, rt[k]);   // a NaN floor stays, a NaN value enters
            dt[k] = nsim_max(floor_t, dt[k]);
        }
    }
    __syncthreads();
    double lo = INFINITY;
    int nan = 0;
    for (int i = tid; i < n; i += 256) {
        const double a = R[i], d = D[i];
        nan |= (a != a) | (d != d);
        lo = (a < lo) ? a : lo;
        lo = (d < lo) ? d : lo;
    }
    red[tid] = lo;
    bad[tid] = nan;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) {
            red[tid] = red[tid + h] < red[tid] ? red[tid + h] : red[tid];
            bad[tid] |= bad[tid + h];
        }
        __syncthreads();
    }
    const double least = bad[0] ? (double)NAN : red[0];
    for (int i = tid; i < n; i += 256) {
        R[i] -= least;
        D[i] -= least;
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int t = i / kGammatoneBands, band = i % kGammatoneBands;
        M[i] = nsim_cell(R, D, F, t, band, C1, C3);
    }
    __syncthreads();
    if (tid < kGammatoneBands) {
        const double v = nsim_band_mean(M, F, tid);
        band_mean[tid] = v;
        if (bands) bands[(size_t)j * kGammatoneBands + tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        nsim[j] = nsim_of_bands(band_mean);
    }
}

}  // namespace nomad
