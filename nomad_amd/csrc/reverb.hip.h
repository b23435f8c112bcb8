// Sox-style reverb (the Freeverb network behind `sox ... reverb P`) as the recurrences it is made of: per output channel eight
// parallel comb filters with a one-pole low-pass in the feedback loop, their sum through four all-pass filters in series, the
// channels averaged into a mono row.  G reverberance levels per clip in one call, rows in the (B G, stride) layout
// nomad_embed_ragged reads.  include/nomad_hip.h states the algorithm in full; it is a restatement FROM MEMORY of sox 14.4 reverb.c
// that has never been run against the sox binary: its fidelity to sox is not measured.  The tests hold the kernels to that text.
//
//   comb i, sample t:     o = line_i[t - D_i];  store_i = o + (store_i - o) damp;  line_i[t] = in + store_i feedback;  acc += o
//   all-pass j, sample t: o = ap_j[t - D_j];    ap_j[t] = acc + o / 2;             acc = o - acc
//
// Where the recurrences are sequential.  Every filter reads what it wrote D samples ago, so inside a time tile of T <= min D samples
// all reads come from earlier tiles: the eight combs are independent, the T samples of a tile are independent, and the all-passes
// have no chain inside a tile at all.  The one sample-to-sample chain is the low-pass, store_t = damp store_{t-1} + (1 - damp) o_t:
// a first-order linear scan, done across the lanes of a wave.
//
//   reverb_wet_kernel   one workgroup per (row, channel), 9 waves.  T = min(64, shortest delay of the call): lane l of a tile is
//                       sample t0 + l.  Waves 0 .. 7: comb i.  Its delay line is a ring of exactly D_i doubles in LDS, so the slot
//                       read (t - D_i) is the slot written (t); the store scan is Kogge-Stone over the lanes (6 steps, each
//                       b_l += damp^(2^j) b_{l - 2^j}), then the carry of the tile before enters as damp^(l + 1) carry.  The
//                       outputs o go to one of two [8][64] LDS planes.  Wave 8, one tile behind the combs (one barrier per tile):
//                       adds the eight o in the order 7 .. 0, runs the four all-passes (rings of D_j doubles in LDS), and writes
//                       wet = acc gain as float64 into the channel's wet plane in the workspace.
//   reverb_mix_kernel   y = dry x + mean over the channels of wet (two channels: 0.5 (wet_0 + wet_1)), the clamp, ONE rounding to
//                       fp32; zeros from the length to the stride.
//
// Everything is float64.  No atomics.  The order of every sum and of the scan depends on the lane = t mod T and on the parameters
// alone - T follows the delays, which follow (sample rate, room scale, stereo depth), never B, G or the reverberance - so row b G + g
// has the bits of the clip's own B = 1, G = 1 call.  Against the sample-by-sample recurrence the scan reassociates: a few units of
// 2^-53 per sample, amplified by at most 1 / (1 - feedback) <= 50.
// LDS: (sum of one channel's delays + 2 x 8 x 64) doubles: 44.7 KB at 16 kHz with the default room, 118 KB at 48 kHz - no delay line
// lives in global memory.  Workspace: the tables plus 8 bytes per output sample and channel, written (t < n) before it is read (t < n).
// Non-finite samples: the scan passes values from lower lanes to higher ones only (a select, not a product with zero, masks the lanes
// a step does not reach), so a non-finite sample at p changes nothing below p in its own rows and nothing in any other row.
// Not done: more than one sample per lane where every delay allows a longer tile, DPP row shifts in place of the LDS permutes of
// the scan, the two channels of a row sharing one read of x.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace nomad {

constexpr int kReverbMaxLevels = 64;
constexpr int kReverbCombs = 8, kReverbAllpass = 4;
constexpr int kReverbTileMax = 64;                          // one sample per lane
constexpr int kReverbThreads = 64 * (kReverbCombs + 1);     // a wave per comb and one for the all-passes
constexpr size_t kReverbLdsMax = 160 * 1024;

// What the host derives from the parameters (reverb_plan below); passed to the kernels by value.
struct ReverbPlan {
    int channels;                                           // 1 + ceil(stereo_depth / 100): 1 or 2
    int comb[2][kReverbCombs], allpass[2][kReverbAllpass];  // delays in samples, per channel
    int tile;                                               // min(64, the shortest delay of either channel)
    int pre;                                                // pre-delay in samples
    int lds_doubles;                                        // the larger channel's rings + the two planes of comb outputs
    double damp, one_minus_damp, gain, dry;
    int clamp;
};

inline double reverb_feedback(double reverberance) {
    const double a = -1.0 / std::log(1.0 - 0.3);
    const double b = 100.0 / (std::log(1.0 - 0.98) * a + 1.0);
    return 1.0 - std::exp((reverberance - b) / (a * b));
}

inline ReverbPlan reverb_plan(double hf_damping, double room_scale, double stereo_depth, double pre_delay_ms, double wet_gain_db,
                              int wet_only, int clamp, int sample_rate) {
    static const int comb_len[kReverbCombs] = {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617};
    static const int allpass_len[kReverbAllpass] = {225, 341, 441, 556};
    ReverbPlan p;
    const double scale = room_scale / 100.0 * 0.9 + 0.1, depth = stereo_depth / 100.0, r = sample_rate * (1.0 / 44100.0);
    p.damp = hf_damping / 100.0 * 0.3 + 0.2;
    p.one_minus_damp = 1.0 - p.damp;
    p.gain = std::pow(10.0, wet_gain_db / 20.0) * 0.015;
    p.dry = wet_only ? 0.0 : 1.0;
    p.clamp = clamp;
    p.pre = (int)(pre_delay_ms / 1000.0 * sample_rate + 0.5);
    p.channels = depth > 0.0 ? 2 : 1;
    p.tile = kReverbTileMax;
    p.lds_doubles = 0;
    for (int c = 0; c < 2; ++c) {
        double off = c * depth;
        int sum = 0;
        for (int i = 0; i < kReverbCombs; ++i, off = -off) {
            p.comb[c][i] = (int)(scale * r * (comb_len[i] + 12.0 * off) + 0.5);
            sum += p.comb[c][i];
            if (c < p.channels && p.comb[c][i] < p.tile) p.tile = p.comb[c][i];
        }
        for (int j = 0; j < kReverbAllpass; ++j, off = -off) {
            p.allpass[c][j] = (int)(r * (allpass_len[j] + 12.0 * off) + 0.5);
            sum += p.allpass[c][j];
            if (c < p.channels && p.allpass[c][j] < p.tile) p.tile = p.allpass[c][j];
        }
        if (c < p.channels && sum > p.lds_doubles) p.lds_doubles = sum;
    }
    p.lds_doubles += 2 * kReverbCombs * kReverbTileMax;
    return p;
}

// Grid (B G, channels), kReverbThreads threads, plan.lds_doubles doubles of dynamic LDS.
// x [B][stride], lens [B], feedback [G]; wet [channels][B G][stride] float64: samples [0, n) of every row are written.
__global__ __launch_bounds__(kReverbThreads) void reverb_wet_kernel(const float* __restrict__ x, int stride, const int* __restrict__ lens,
                                                                     const double* __restrict__ feedback, int G, ReverbPlan plan,
                                                                     double* __restrict__ wet) {
    extern __shared__ double reverb_lds[];
    const int row = blockIdx.x, ch = blockIdx.y;
    const int b = row / G, g = row - b * G;
    const int n = lens[b];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = plan.tile;
    double* planes = reverb_lds;                                   // [2][8][64]: the combs' outputs of the tile in flight and the one before
    double* rings = reverb_lds + 2 * kReverbCombs * kReverbTileMax;
    const int ring_doubles = plan.lds_doubles - 2 * kReverbCombs * kReverbTileMax;
    for (int i = tid; i < ring_doubles; i += kReverbThreads) rings[i] = 0.0;

    // this wave's ring(s): a comb wave has one, the all-pass wave four
    int D[kReverbAllpass], at[kReverbAllpass], pos[kReverbAllpass];
    if (wave < kReverbCombs) {
        int o = 0;
        for (int i = 0; i < wave; ++i) o += plan.comb[ch][i];
        D[0] = plan.comb[ch][wave];
        at[0] = o;
        pos[0] = 0;
    } else {
        int o = 0;
        for (int i = 0; i < kReverbCombs; ++i) o += plan.comb[ch][i];
        for (int j = 0; j < kReverbAllpass; ++j) {
            D[j] = plan.allpass[ch][j];
            at[j] = o;
            pos[j] = 0;
            o += D[j];
        }
    }
    const double damp = plan.damp, fb = feedback[g];
    // damp^(2^j) for the scan's steps, damp^(lane + 1) for the carry
    double step_pow[6];
    step_pow[0] = damp;
    for (int j = 1; j < 6; ++j) step_pow[j] = step_pow[j - 1] * step_pow[j - 1];
    double carry_pow = damp;
    for (int i = 0; i < lane; ++i) carry_pow *= damp;
    double carry = 0.0;                                            // store behind the tile before

    const float* xr = x + (size_t)b * (size_t)stride;
    double* wrow = wet + ((size_t)ch * gridDim.x + (size_t)row) * (size_t)stride;
    const int tiles = (n + T - 1) / T;
    auto input = [&](int t) -> double {
        const int s = t - plan.pre;
        return (lane < T && t < n && s >= 0) ? (double)xr[s] : 0.0;
    };
    double in_next = wave < kReverbCombs ? input(lane) : 0.0;
    __syncthreads();

    for (int k = 0; k <= tiles; ++k) {
        if (wave < kReverbCombs) {
            if (k < tiles) {
                const int t = k * T + lane;
                const bool live = lane < T && t < n;
                const double in = in_next;
                in_next = input(t + T);                             // the next tile's samples are on their way during this one
                int slot = pos[0] + lane;
                slot = slot >= D[0] ? slot - D[0] : slot;
                double* line = rings + at[0];
                const double o = live ? line[slot] : 0.0;
                // store_t = damp store_{t-1} + (1 - damp) o_t over the tile's lanes
                double s = plan.one_minus_damp * o;
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const double below = __shfl_up(s, 1u << j, 64);
                    s = lane >= (1 << j) ? fma(step_pow[j], below, s) : s;
                }
                s = fma(carry_pow, carry, s);
                carry = __shfl(s, T - 1, 64);
                if (live) {
                    line[slot] = in + s * fb;
                    planes[((k & 1) * kReverbCombs + wave) * kReverbTileMax + lane] = o;
                }
                pos[0] += T;
                pos[0] = pos[0] >= D[0] ? pos[0] - D[0] : pos[0];
            }
        } else if (k >= 1) {
            const int t = (k - 1) * T + lane;
            const bool live = lane < T && t < n;
            if (live) {
                const double* o8 = planes + ((k - 1) & 1) * kReverbCombs * kReverbTileMax + lane;
                double acc = 0.0;
#pragma unroll
                for (int i = kReverbCombs - 1; i >= 0; --i) acc += o8[i * kReverbTileMax];
#pragma unroll
                for (int j = kReverbAllpass - 1; j >= 0; --j) {
                    int slot = pos[j] + lane;
                    slot = slot >= D[j] ? slot - D[j] : slot;
                    double* ap = rings + at[j];
                    const double o = ap[slot];
                    ap[slot] = acc + o * 0.5;
                    acc = o - acc;
                }
                wrow[t] = acc * plan.gain;
            }
#pragma unroll
            for (int j = 0; j < kReverbAllpass; ++j) {
                pos[j] += T;
                pos[j] = pos[j] >= D[j] ? pos[j] - D[j] : pos[j];
            }
        }
        __syncthreads();
    }
}

// out[row][t] = (float)clamp(dry x[b][t] + mean_c wet_c[row][t]) for t < n_b, 0 behind it.  Grid B G, 256 threads: a block per row.
__global__ __launch_bounds__(256) void reverb_mix_kernel(const float* __restrict__ x, int stride, const int* __restrict__ lens, int G,
                                                         const double* __restrict__ wet, size_t plane, ReverbPlan plan,
                                                         float* __restrict__ out) {
    const int row = blockIdx.x, b = row / G;
    const int n = lens[b];
    const float* xr = x + (size_t)b * (size_t)stride;
    const double* w0 = wet + (size_t)row * (size_t)stride;
    float* orow = out + (size_t)row * (size_t)stride;
    for (int t = threadIdx.x; t < stride; t += 256) {
        float y = 0.0f;
        if (t < n) {
            const double w = plan.channels == 2 ? 0.5 * (w0[t] + w0[plane + t]) : w0[t];
            double v = plan.dry * (double)xr[t] + w;
            if (plan.clamp) v = v > 1.0 ? 1.0 : v < -1.0 ? -1.0 : v;   // a NaN fails both comparisons and stays
            y = (float)v;
        }
        orow[t] = y;
    }
}

}  // namespace nomad
