// Loudness of packed rows and the linear gain that brings them to a target: ITU-R BS.1770-4 for one channel (the "ebu" mode of
// ffmpeg-normalize, which the reference's rendering scripts run over every degraded file), plus that tool's rms and peak modes.
// Works on the [R][stride] rows nomad_embed_ragged reads, in place if the caller wants.
//
// The measurement (include/nomad_hip.h states it in full):
//   K-weighting: two cascaded biquads in float64, coefficients formed on the host from the sample rate (loudness_filter below);
//   blocks of 4 hop samples every hop = fs / 10 samples (400 ms, 75 % overlap), whole blocks only, z_j = mean square of block j,
//   l_j = -0.691 + 10 log10 z_j; absolute gate l_j > -70, relative gate 10 dB under the mean of the absolute-gated blocks;
//   L = -0.691 + 10 log10(mean z_j over the blocks past both gates), -inf if no block passes the absolute gate.
//   The peak is the SAMPLE peak max|x|, not the 4x oversampled true peak.
//
// The recurrence made parallel without changing its value.  A row is cut into chunks of hop samples; the cascade is linear, so the
// state behind a chunk is M s + e: s the state in front of it, e the state the chunk leaves from a zero state, M the cascade's
// transition over hop samples of silence (4 x 4, formed on the host by running the same recurrence on the four unit states).
//   loudness_chunk_kernel<false>  one thread per chunk: the cascade from the zero state -> e, and the chunk's max|x| and sum x^2
//   loudness_carry_kernel         one thread per row: s_0 = 0, s_{j+1} = M s_j + e_j over the row's whole chunks
//   loudness_chunk_kernel<true>   one thread per WHOLE chunk: the cascade again from s_j -> sum y^2, the 100 ms sums the blocks are
//                                 made of (block j = chunks j .. j + 3; a trailing partial chunk is in no block)
//   loudness_gate_kernel          one thread per row: the chunk sums in ascending order, the two gates, level, peak, gain
//   loudness_gain_kernel          out[i] = (float)((double)x[i] g), zeros behind the length
// Everything is float64 and every sum has one fixed order that depends on the row's length and the sample rate alone, so a row has
// the bits of its own R = 1 call.  In float64 the hand-over is exact up to rounding (the poles of the high-pass sit at radius 0.985
// at 16 kHz: 1600 steps shrink an error in s by 1e-11).
//
// The chunk walk reads 4 bytes per lane, 4 hop bytes apart between lanes, and relies on the caches: a lane's 128-byte line serves
// its next 32 samples, and the walk is bound by its float64 chain (12 multiply-adds per sample, 3 of them dependent), not by loads.
// Traffic floor of a normalising call: the rows read twice (two walks), then read and written once by the gain pass.
// Non-finite samples: max|x| is formed so that a NaN sticks; a row whose peak is not finite gets NaN level, gain and block count,
// so every output sample of [0, n) is NaN - no other row sees it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace nomad {

constexpr int kLoudnessEbu = 0, kLoudnessRms = 1, kLoudnessPeak = 2;
constexpr int kLoudnessChunkStats = 6;   // per chunk: the four end-state numbers, max|x|, sum x^2

// Both biquads in transposed direct form II: y = b0 x + z1; z1 = b1 x - a1 y + z2; z2 = b2 x - a2 y.  The high-pass has b = [1, -2, 1].
struct LoudnessFilter {
    double b0, b1, b2, a1, a2;   // stage 1, the shelf
    double h1, h2;               // stage 2, the high-pass: a1, a2
    double M[16];                // row-major: state behind hop samples of silence = M state
};

// One sample through the cascade; s = (z1, z2 of the shelf, z1, z2 of the high-pass).  Host and device run the same lines.
__host__ __device__ __forceinline__ double loudness_step(const LoudnessFilter& f, double x, double s[4]) {
    const double y1 = f.b0 * x + s[0];
    s[0] = f.b1 * x - f.a1 * y1 + s[1];
    s[1] = f.b2 * x - f.a2 * y1;
    const double y2 = y1 + s[2];
    s[2] = -2.0 * y1 - f.h1 * y2 + s[3];
    s[3] = y1 - f.h2 * y2;
    return y2;
}

// The coefficients of BS.1770-4's two stages re-derived for the sample rate fs (at 48 kHz: the standard's table), and M.
inline LoudnessFilter loudness_filter(int fs, int hop) {
    const double pi = 3.14159265358979323846;
    LoudnessFilter f;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / (double)fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        f.b0 = (Vh + Vb * K / Q + K * K) / a0;
        f.b1 = 2.0 * (K * K - Vh) / a0;
        f.b2 = (Vh - Vb * K / Q + K * K) / a0;
        f.a1 = 2.0 * (K * K - 1.0) / a0;
        f.a2 = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / (double)fs), a0 = 1.0 + K / Q + K * K;
        f.h1 = 2.0 * (K * K - 1.0) / a0;
        f.h2 = (1.0 - K / Q + K * K) / a0;
    }
    for (int k = 0; k < 4; ++k) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        s[k] = 1.0;
        for (int i = 0; i < hop; ++i) (void)loudness_step(f, 0.0, s);
        for (int r = 0; r < 4; ++r) f.M[4 * r + k] = s[r];
    }
    return f;
}

// Grid (ceil(C / 64), R), 64 threads: thread j of row r walks chunk j = samples [j hop, min((j + 1) hop, n)).
// SECOND = false: from the zero state; cs [R][C][6] <- (end state, max|x|, sum x^2); every chunk, a trailing partial one included.
//   filter = false (rms and peak modes): the cascade is skipped and the end state left unwritten (nothing reads it).
// SECOND = true: whole chunks only, from entry [R][C][4]; ysum [R][C] <- sum y^2.
template <bool SECOND>
__global__ __launch_bounds__(64) void loudness_chunk_kernel(const float* __restrict__ x, int stride, const int* __restrict__ lens, int hop, int C,
                                                            LoudnessFilter f, bool filter, double* __restrict__ cs,
                                                            const double* __restrict__ entry, double* __restrict__ ysum) {
    const int r = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
    const int n = lens[r];
    const long long i0 = (long long)j * hop;
    if (j >= C || i0 >= n) return;
    const int i1 = (int)(i0 + hop < n ? i0 + hop : n);
    if (SECOND && i1 - (int)i0 < hop) return;
    const float* xr = x + (size_t)r * (size_t)stride;
    const size_t slot = (size_t)r * (size_t)C + (size_t)j;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (SECOND) {
        for (int k = 0; k < 4; ++k) s[k] = entry[4 * slot + k];
        double acc = 0.0;
        for (int i = (int)i0; i < i1; ++i) {
            const double y = loudness_step(f, (double)xr[i], s);
            acc += y * y;
        }
        ysum[slot] = acc;
    } else {
        double peak = 0.0, acc = 0.0;
        for (int i = (int)i0; i < i1; ++i) {
            const double v = (double)xr[i], av = fabs(v);
            peak = (av > peak || av != av) ? av : peak;   // a NaN enters and stays: no later comparison with it is true
            acc += v * v;
            if (filter) (void)loudness_step(f, v, s);
        }
        double* o = cs + kLoudnessChunkStats * slot;
        if (filter)
            for (int k = 0; k < 4; ++k) o[k] = s[k];
        o[4] = peak;
        o[5] = acc;
    }
}

// One thread per row: entry[r][0] = 0, entry[r][j + 1] = M entry[r][j] + e_j for the row's whole chunks (the products of a
// row of M are added in ascending column order, then e).  Entries are written for chunks 0 .. whole - 1, the ones the second walk reads.
__global__ __launch_bounds__(64) void loudness_carry_kernel(const int* __restrict__ lens, int R, int hop, int C, LoudnessFilter f,
                                                            const double* __restrict__ cs, double* __restrict__ entry) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    const int whole = lens[r] / hop;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < whole && j < C; ++j) {
        const size_t slot = (size_t)r * (size_t)C + (size_t)j;
        for (int k = 0; k < 4; ++k) entry[4 * slot + k] = s[k];
        const double* e = cs + kLoudnessChunkStats * slot;
        double t[4];
        for (int k = 0; k < 4; ++k) t[k] = ((f.M[4 * k] * s[0] + f.M[4 * k + 1] * s[1]) + f.M[4 * k + 2] * s[2]) + f.M[4 * k + 3] * s[3] + e[k];
        for (int k = 0; k < 4; ++k) s[k] = t[k];
    }
}

__device__ __forceinline__ double loudness_lufs(double z) { return -0.691 + 10.0 * log10(z); }

// One thread per row: level, sample peak, gain, blocks past both gates -> stats [R][4] (the gain pass reads the gain there) and
// stats_out (the caller's copy, or null).  peak_lin = 10^(peak_db / 20) from the host, NaN for no ceiling.
__global__ __launch_bounds__(64) void loudness_gate_kernel(const int* __restrict__ lens, int R, int hop, int C, int mode, double target,
                                                           double peak_lin, const double* __restrict__ cs, const double* __restrict__ ysum,
                                                           double* __restrict__ stats, double* __restrict__ stats_out) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    const int n = lens[r];
    const int whole = n / hop, chunks = whole + (n % hop != 0);
    const double* c0 = cs + kLoudnessChunkStats * (size_t)r * (size_t)C;
    double peak = 0.0, xsum = 0.0;
    for (int j = 0; j < chunks; ++j) {
        const double p = c0[kLoudnessChunkStats * j + 4];
        peak = (p > peak || p != p) ? p : peak;
        xsum += c0[kLoudnessChunkStats * j + 5];
    }
    double level, blocks = 0.0;
    if (mode == kLoudnessEbu) {
        const double* y = ysum + (size_t)r * (size_t)C;
        const int nb = whole - 3;   // <= 0: the row is shorter than one block
        const double per = 4.0 * (double)hop;
        double za = 0.0;
        int na = 0;
        for (int j = 0; j < nb; ++j) {
            const double z = (((y[j] + y[j + 1]) + y[j + 2]) + y[j + 3]) / per;
            if (loudness_lufs(z) > -70.0) {
                za += z;
                ++na;
            }
        }
        level = -INFINITY;
        if (na > 0) {
            const double gamma = loudness_lufs(za / (double)na) - 10.0;
            double zr = 0.0;
            int nr = 0;
            for (int j = 0; j < nb; ++j) {
                const double z = (((y[j] + y[j + 1]) + y[j + 2]) + y[j + 3]) / per;
                const double l = loudness_lufs(z);
                if (l > -70.0 && l > gamma) {
                    zr += z;
                    ++nr;
                }
            }
            if (nr > 0) level = loudness_lufs(zr / (double)nr);
            blocks = (double)nr;
        }
    } else if (mode == kLoudnessRms) {
        level = 20.0 * log10(sqrt(xsum / (double)n));
    } else {
        level = 20.0 * log10(peak);
    }
    double g = 1.0;
    if (!(peak <= 1.79769313486231570815e308)) {   // a NaN or infinite sample: the whole row is void
        level = NAN;
        g = NAN;
        blocks = NAN;
    } else if (level != -INFINITY) {
        g = pow(10.0, (target - level) / 20.0);
        if (peak_lin == peak_lin) {
            const double cap = peak_lin / peak;
            g = g < cap ? g : cap;
        }
    }
    const double v[4] = {level, peak, g, blocks};
    for (int k = 0; k < 4; ++k) {
        stats[4 * (size_t)r + k] = v[k];
        if (stats_out) stats_out[4 * (size_t)r + k] = v[k];
    }
}

// out[r][i] = (float)((double)x[r][i] g_r) for i < n_r, 0 behind it.  Grid (ceil(stride / (256 V)), R), 256 threads, V samples per
// thread: V = 4 (16-byte loads and stores) where both base addresses are 16-byte aligned, else V = 1.  out may be x: a thread reads
// its own samples before it writes them.
template <int V>
__global__ __launch_bounds__(256) void loudness_gain_kernel(const float* x, int stride, const int* __restrict__ lens,
                                                            const double* __restrict__ stats, float* out) {
    const int r = blockIdx.y;
    const long long at_row = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (at_row >= stride) return;
    const int i = (int)at_row;
    const int n = lens[r];
    const double g = stats[4 * (size_t)r + 2];
    const size_t at = (size_t)r * (size_t)stride + (size_t)i;
    if (V == 4) {   // stride is a multiple of 4: the four samples are inside the row
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < n) v = *reinterpret_cast<const float4*>(x + at);
        v.x = i < n ? (float)((double)v.x * g) : 0.0f;
        v.y = i + 1 < n ? (float)((double)v.y * g) : 0.0f;
        v.z = i + 2 < n ? (float)((double)v.z * g) : 0.0f;
        v.w = i + 3 < n ? (float)((double)v.w * g) : 0.0f;
        *reinterpret_cast<float4*>(out + at) = v;
    } else {
        out[at] = i < n ? (float)((double)x[at] * g) : 0.0f;
    }
}

}  // namespace nomad
