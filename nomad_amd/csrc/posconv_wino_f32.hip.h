// fp32 pos-conv in nested F(2,2) form: the element-wise kernels around ONE launch of gemm_f32_n48_kernel (gemm_f32.hip.h).
//
// One group of the positional convolution is the 128-tap stride-1 correlation C[t] = sum_k A[t + k] V[k] (A: the zero-padded
// input frames of a clip, 48 channels; V[k]: the 48 x 48 tap matrix).  For tap pairs j and output pairs s
//     D0[r] = A[2r] - A[2r+1]      V0[j] = V[2j]
//     Z1[r] = A[2r+1]              VS[j] = V[2j] + V[2j+1]
//     D2[r] = A[2r+2] - A[2r+1]    V1[j] = V[2j+1]
//     m1[s] = sum_j D0[s+j] V0[j]   m2[s] = sum_j Z1[s+j] VS[j]   m3[s] = sum_j D2[s+j] V1[j]
//     C[2s] = m1[s] + m2[s]         C[2s+1] = m2[s] + m3[s]
// - three half-rate correlations of half the taps instead of four (the F(2,2) form conv_s2_f32.hip.h uses for conv1 .. conv4).
// Each m is a correlation of the same kind, so the identity applies again: kPwLevels = 2 leaves 9 quarter-rate 32-tap
// correlations per group, 9 / 16 of the products.  Only input differences, weight sums and output sums occur: no fractional
// constant, no subtraction of products.
//
// Operand p of a group (p = 3 a + b at two levels: a the outer, b the inner digit) is again an overlapping-row GEMM (row u reads
// kPwTaps consecutive 48-channel frames), so the kPwOps x 16 operands go through the N = 48 kernel as kPwOps x 16 "groups":
//     posconv_wino_input_kernel   xpad [16][frames][48]               -> Q [16 * kPwOps][sum_c (q_c + kPwTaps - 1)][48]
//     gemm_f32_n48_kernel         Q x Wt [16 * kPwOps][64][kPwTaps*48] -> S [16 * kPwOps][sum_c q_c][48]           (plain store)
//     posconv_wino_output_kernel  S -> output sums, + bias, (Upre), GELU, + residual -> y [sum_c T_c][768]
// with q_c = ceil(T_c / kPwRate) rows per clip.  Every frame of Q and every row of S that is read is written by the same call.
// The surplus outputs of a T_c that is no multiple of kPwRate read input frames up to T_c + 128 + kPwRate - 2: the input kernel
// takes frames behind the clip's T_c + 128 as the zeros they stand for, and the output kernel drops rows >= T_c.
#pragma once
#include "gemm_f32.hip.h"

namespace nomad {

#ifndef NOMAD_POSCONV_WINO_LEVELS
#define NOMAD_POSCONV_WINO_LEVELS 2
#endif
constexpr int kPwLevels = NOMAD_POSCONV_WINO_LEVELS;
static_assert(kPwLevels == 1 || kPwLevels == 2, "nested F(2,2): one or two levels");
constexpr int kPwRate = 1 << kPwLevels;             // output frames per row of an operand
constexpr int kPwOps = kPwLevels == 2 ? 9 : 3;      // operands (correlations) per group
constexpr int kPwTaps = 128 / kPwRate;              // taps of each
constexpr int kPwK = kPwTaps * 48;                  // their contraction length

// Where the clips of a batch sit.  Uniform batch (tpref == nullptr): B clips of T frames.  Ragged: prefix sums (device) of the
// clips' frames (tpref), padded frames (ppref: T_c + 128 each), operand rows (qpref: q_c each) and operand frames (qbase:
// q_c + kPwTaps - 1 each; the last two from posconv_wino_prefix_kernel).
struct PosWinoGeom {
    int B, T;
    const int *tpref, *ppref, *qpref, *qbase;
    long long pad_rows;   // padded frames of one group of xpad
    long long q_rows;     // rows of one operand: sum_c q_c
    long long q_frames;   // frames of one operand buffer: sum_c (q_c + kPwTaps - 1)
    int max_q;            // the longest clip's q_c
};

// A ragged batch's operand prefix sums from its frame prefix sums: qmeta[0 .. B] = qpref, qmeta[B + 1 .. 2 B + 1] = qbase.  They
// live in the call's workspace (the host's metadata block keeps its layout).  One workgroup; B is a batch size.
__global__ __launch_bounds__(64) void posconv_wino_prefix_kernel(const int* __restrict__ tpref, int B, int* __restrict__ qmeta) {
    if (threadIdx.x != 0) return;
    int rows = 0, frames = 0;
    for (int b = 0; b < B; ++b) {
        qmeta[b] = rows;
        qmeta[B + 1 + b] = frames;
        const int q = (tpref[b + 1] - tpref[b] + kPwRate - 1) / kPwRate;
        rows += q;
        frames += q + kPwTaps - 1;
    }
    qmeta[B] = rows;
    qmeta[2 * B + 1] = frames;
}

struct PosWinoClip {
    int T;                // frames
    long long pad0;       // first padded frame in a group of xpad
    long long row0;       // first output row (of [sum T][768])
    long long q0, qf0;    // first operand row / operand frame
};

__device__ __forceinline__ PosWinoClip pos_wino_clip(const PosWinoGeom& g, int b) {
    PosWinoClip c;
    if (g.tpref) {
        c.T = g.tpref[b + 1] - g.tpref[b];
        c.pad0 = g.ppref[b];
        c.row0 = g.tpref[b];
        c.q0 = g.qpref[b];
        c.qf0 = g.qbase[b];
    } else {
        const int q = (g.T + kPwRate - 1) / kPwRate;
        c.T = g.T;
        c.pad0 = (long long)b * (g.T + 128);
        c.row0 = (long long)b * g.T;
        c.q0 = (long long)b * q;
        c.qf0 = (long long)b * (q + kPwTaps - 1);
    }
    return c;
}

// the three operands of one F(2,2) level from three consecutive samples: x0 - x1, x1, x2 - x1
__device__ __forceinline__ void pos_wino_split(const f32x4& x0, const f32x4& x1, const f32x4& x2, f32x4 (&o)[3]) {
    o[0] = x0 - x1;
    o[1] = x1;
    o[2] = x2 - x1;
}

// Weight transform, once per weight version: pos_w [16][64][6144] (k = tap * 48 + ci, rows 48 .. 63 zero) ->
// wt [16 * kPwOps][64][kPwK].  Operand digit d of a level takes tap bit 0 (d = 0), both (d = 1: the sum) or tap bit 1 (d = 2); the
// outer level pairs with the low bit of the tap offset.  Every sum is formed in float64 and rounded once.
// grid: 16 * kPwOps * 64 blocks.
__global__ __launch_bounds__(256) void posconv_wino_weight_kernel(const float* __restrict__ pos_w, float* __restrict__ wt) {
    const int n = blockIdx.x & 63, gp = blockIdx.x >> 6;
    const int g = gp / kPwOps, op = gp - g * kPwOps;
    const int da = kPwLevels == 2 ? op / 3 : op, db = kPwLevels == 2 ? op % 3 : 1;
    const float* w = pos_w + ((long long)g * 64 + n) * 6144;
    float* o = wt + (long long)blockIdx.x * kPwK;
    for (int k = threadIdx.x; k < kPwK; k += 256) {
        const int i = k / 48, ci = k - i * 48;
        double acc = 0.0;
        if (n < 48) {
#pragma unroll
            for (int d = 0; d < kPwRate; ++d) {
                const int lo = d & 1, hi = d >> 1;
                const bool in_a = da == 1 || (da >> 1) == lo;
                const bool in_b = kPwLevels == 1 || db == 1 || (db >> 1) == hi;
                if (in_a && in_b) acc += (double)w[(i * kPwRate + d) * 48 + ci];
            }
        }
        o[k] = (float)acc;
    }
}

// Input transform.  grid: (ceil((max_q + kPwTaps - 1) / 16), 16 * B), 192 threads = 16 operand frames x 12 float4.
__global__ __launch_bounds__(192) void posconv_wino_input_kernel(const float* __restrict__ xpad, float* __restrict__ Q, const PosWinoGeom geo) {
    const int g = blockIdx.y / geo.B, b = blockIdx.y - g * geo.B;
    const PosWinoClip c = pos_wino_clip(geo, b);
    const int nq = (c.T + kPwRate - 1) / kPwRate + kPwTaps - 1;   // operand frames of this clip
    const int fr = threadIdx.x / 12, v = threadIdx.x - fr * 12;
    const int q = blockIdx.x * 16 + fr;
    if (q >= nq) return;
    constexpr int NX = 2 * kPwRate - 1;   // input frames behind one operand frame: 3 or 7
    const int nf = c.T + 128;             // (frames behind it stand for zeros)
    const float* src = xpad + ((long long)g * geo.pad_rows + c.pad0) * 48 + v * 4;
    f32x4 x[NX];
#pragma unroll
    for (int d = 0; d < NX; ++d) {
        const int f = kPwRate * q + d;
        x[d] = f < nf ? *reinterpret_cast<const f32x4*>(src + (long long)f * 48) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    float* dst = Q + ((long long)g * kPwOps * geo.q_frames + c.qf0 + q) * 48 + v * 4;
    const long long op_stride = geo.q_frames * 48;
    if constexpr (kPwLevels == 1) {
        f32x4 o[3];
        pos_wino_split(x[0], x[1], x[2], o);
#pragma unroll
        for (int a = 0; a < 3; ++a) *reinterpret_cast<f32x4*>(dst + a * op_stride) = o[a];
    } else {
        f32x4 p[3][3];   // p[e][a]: outer operand a at half-rate frame 2 q + e
#pragma unroll
        for (int e = 0; e < 3; ++e) pos_wino_split(x[2 * e], x[2 * e + 1], x[2 * e + 2], p[e]);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            f32x4 o[3];
            pos_wino_split(p[0][a], p[1][a], p[2][a], o);
#pragma unroll
            for (int bb = 0; bb < 3; ++bb) *reinterpret_cast<f32x4*>(dst + (a * 3 + bb) * op_stride) = o[bb];
        }
    }
}

// Output transform and the pos-conv's epilogue: the output sums of the levels, then + bias, the optional pre-activation store,
// GELU and the residual from xpad, in the order of the N = 48 kernel's own epilogue.  y / upre: [sum T][768].
// grid: (ceil(max_q / 16), 16 * B), 192 threads = 16 operand rows x 12 float4.
__global__ __launch_bounds__(192) void posconv_wino_output_kernel(const float* __restrict__ S, const float* __restrict__ bias,
                                                                  const float* __restrict__ xpad, float* __restrict__ y,
                                                                  float* __restrict__ upre, const PosWinoGeom geo) {
    const int g = blockIdx.y / geo.B, b = blockIdx.y - g * geo.B;
    const PosWinoClip c = pos_wino_clip(geo, b);
    const int nq = (c.T + kPwRate - 1) / kPwRate;
    const int ur = threadIdx.x / 12, v = threadIdx.x - ur * 12;
    const int u = blockIdx.x * 16 + ur;
    if (u >= nq) return;
    const float* src = S + ((long long)g * kPwOps * geo.q_rows + c.q0 + u) * 48 + v * 4;
    const long long op_stride = geo.q_rows * 48;
    f32x4 n[kPwOps];
#pragma unroll
    for (int p = 0; p < kPwOps; ++p) n[p] = *reinterpret_cast<const f32x4*>(src + p * op_stride);
    f32x4 out[kPwRate];
    if constexpr (kPwLevels == 1) {
        out[0] = n[0] + n[1];
        out[1] = n[1] + n[2];
    } else {
        f32x4 m[3][2];   // m[a][h]: outer correlation a at half-rate output 2 u + h
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            m[a][0] = n[a * 3] + n[a * 3 + 1];
            m[a][1] = n[a * 3 + 1] + n[a * 3 + 2];
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            out[2 * h] = m[0][h] + m[1][h];
            out[2 * h + 1] = m[1][h] + m[2][h];
        }
    }
    const f32x4 bv = bias ? *reinterpret_cast<const f32x4*>(bias + g * 48 + v * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* res = xpad + ((long long)g * geo.pad_rows + c.pad0 + 64) * 48 + v * 4;
#pragma unroll
    for (int e = 0; e < kPwRate; ++e) {
        const int t = kPwRate * u + e;
        if (t >= c.T) break;
        f32x4 val = out[e] + bv;
        const long long idx = (c.row0 + t) * 768 + g * 48 + v * 4;
        if (upre) *reinterpret_cast<f32x4*>(upre + idx) = val;
#pragma unroll
        for (int k = 0; k < 4; ++k) val[k] = gelu_erf(val[k]);
        val += *reinterpret_cast<const f32x4*>(res + (long long)t * 48);
        *reinterpret_cast<f32x4*>(y + idx) = val;
    }
}

}  // namespace nomad
