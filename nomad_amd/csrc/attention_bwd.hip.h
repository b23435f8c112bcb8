// Attention backward on the matrix cores (v_mfma_f32_16x16x4_f32), flash style: the T x T probabilities are
// recomputed from the saved log-sum-exp, nothing of size T x T touches HBM.  Deterministic: no atomics - two
// kernels, each owning its output rows and streaming the other side through LDS:
//
//   attn_bwd_rowdot_kernel  D[b,h,q]   = sum_d dO[q,d] O[q,d]                                  (one pass, HBM-bound)
//   attn_bwd_dkv_kernel     one workgroup = 64 keys of one (clip, head), wave = 16 keys, loops over query tiles:
//       S[q][key]  = Q K^T,  dP[q][key] = dO V^T          A = Q / dO rows from LDS, B = K / V from registers
//       P = exp(S - lse[q]),  Pm = P * Mk (attention dropout),  dS = P * (dP * Mk - D[q])
//       dV[key][d] += sum_q Pm[q][key] dO[q][d],  dK[key][d] += sum_q dS[q][key] Q[q][d]
//     The S / dP accumulators are directly the A operand of the second pair of products: lane (key = lane&15,
//     g = lane>>4) holds queries {16*sub + 4g + r}, and MFMA k-step r contracts exactly those (the contraction order
//     is free) - the same register-reuse trick as the forward kernel (attention.hip.h), mirrored.
//   attn_bwd_dq_kernel      one workgroup = 64 queries, wave = 16 queries, loops over key tiles; the forward's own
//     transposed layout: S^T[key][q] = K Q^T, dP^T = V dO^T (A from LDS, B = Q / dO registers), then
//       dQ^T[d][q] += sum_key K[key][d] dS^T[key][q]        A = K from LDS, B = the dS^T accumulator itself
//
// qkv / dqkv: [B*T][2304] = [q (pre-scaled by 1/8) | k | v]; dO: [B*T][768]; lse, D: [B*12][T].
// Ragged batches (tpref: the WHOLE batch's frame prefix sums; a launch covers the clips from (clip, head) bh0 on): rows are packed,
// lse / D hold clip c's [12][T_c] block at 12 * tpref[c], the attention-dropout mask of clip c its [12][T_c][T_c] block at
// attn_mask_base(tpref, c).  Every pointer is then the whole batch's.  Which form a clip takes - the fused kernel (T_c <= 64, no
// dropout) or the three kernels - is decided by the CLIP's length, never the batch's, so that a clip runs the same kernel and comes
// out with the same bits in every batch (the rule run_attention states for the forward): a mixed batch launches both, each kernel
// leaves the other's clips alone (t_skip / t_min).
#pragma once
#include <hip/hip_runtime.h>

#include "attention.hip.h"
#include "dropout.hip.h"
#include "dtypes.hip.h"

namespace nomad {

// grid: ceil(M/4) blocks of 256 threads, one wave per row m = b*T + t; 16 lanes per head.
__global__ __launch_bounds__(256) void attn_bwd_rowdot_kernel(const float* __restrict__ o, const float* __restrict__ dO,
                                                              float* __restrict__ D, int M, int T,
                                                              const int* __restrict__ tpref = nullptr, int nclips = 0,
                                                              int m0 = 0, int t_min = 0) {
    const int lane = threadIdx.x & 63, m = m0 + blockIdx.x * 4 + (threadIdx.x >> 6);   // (ragged: rows m0 .. M - 1 of the batch)
    if (m >= M) return;
    int b, t;
    long long d0;   // D of (clip b, head 0, frame 0)
    if (tpref) {
        b = clip_of_row(tpref, nclips, m);
        t = m - tpref[b];
        T = tpref[b + 1] - tpref[b];
        if (T < t_min) return;   // the fused kernel's clip
        d0 = 12LL * tpref[b];
    } else {
        b = m / T;
        t = m - b * T;
        d0 = (long long)b * 12 * T;
    }
    const float4* op = reinterpret_cast<const float4*>(o + (long long)m * 768);
    const float4* gp = reinterpret_cast<const float4*>(dO + (long long)m * 768);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float4 a = op[lane + 64 * i], g = gp[lane + 64 * i];
        float s = (a.x * g.x + a.y * g.y) + (a.z * g.z + a.w * g.w);
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 8);
        if ((lane & 15) == 0) D[d0 + (long long)((lane >> 4) + 4 * i) * T + t] = s;
    }
}

// Stage a 64-row x 64-float tile (rows row0.., clamped to T-1) of a [.][ld] tensor into LDS via registers.
__device__ __forceinline__ void abw_fetch(f32x4 (&reg)[4], const float* __restrict__ src, long long ld, int row0, int T,
                                          int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = tid + i * 256, row = id >> 4, c4 = id & 15;
        int r = row0 + row;
        r = r < T ? r : T - 1;
        reg[i] = *reinterpret_cast<const f32x4*>(src + (long long)r * ld + c4 * 4);
    }
}
__device__ __forceinline__ void abw_store(float* __restrict__ dst, const f32x4 (&reg)[4], int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = tid + i * 256, row = id >> 4, c4 = id & 15;
        *reinterpret_cast<f32x4*>(dst + row * kAttnLD + c4 * 4) = reg[i];
    }
}

template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                           const float* __restrict__ lse, const float* __restrict__ D,
                                                           float* __restrict__ dqkv, int T, DropCfg dc, uint32_t site, int bh0,
                                                           const int* __restrict__ tpref = nullptr, int t_min = 0) {
    __shared__ __attribute__((aligned(16))) float Qs[64 * kAttnLD];
    __shared__ __attribute__((aligned(16))) float Gs[64 * kAttnLD];  // dO tile
    __shared__ __attribute__((aligned(16))) float lse_s[64];
    __shared__ __attribute__((aligned(16))) float D_s[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, g = lane >> 4;
    const int bh = blockIdx.y;
    int b = bh / 12;
    const int h = bh - b * 12;
    const int k0 = blockIdx.x * 64;
    long long row0 = (long long)b * T;
    unsigned long long mask0 = (unsigned long long)(bh0 + bh) * T * T;   // this (clip, head)'s [T][T] block of the dropout mask
    if (tpref) {
        b += bh0 / 12;
        row0 = tpref[b];
        T = tpref[b + 1] - tpref[b];
        if (k0 >= T || T < t_min) return;   // whole workgroup, before any barrier
        if (DROP) mask0 = attn_mask_base(tpref, b) + (unsigned long long)h * T * T;
    }
    const float* qb = qkv + row0 * 2304 + h * 64;
    const float* gb = dO + row0 * 768 + h * 64;
    const float* lb = lse + 12 * row0 + (long long)h * T;
    const float* Db = D + 12 * row0 + (long long)h * T;
    const int key = k0 + wave * 16 + fi;
    const int key_ld = key < T ? key : T - 1;
    const bool wave_active = k0 + wave * 16 < T;  // wave-uniform

    // B operands: this lane's key, d = 16*dd + 4g + c
    f32x4 kf[4], vf[4];
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) {
        kf[dd] = *reinterpret_cast<const f32x4*>(qb + (long long)key_ld * 2304 + 768 + dd * 16 + g * 4);
        vf[dd] = *reinterpret_cast<const f32x4*>(qb + (long long)key_ld * 2304 + 1536 + dd * 16 + g * 4);
    }
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) dk[i] = dv[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int ntiles = (T + 63) / 64;
    f32x4 qreg[4], greg[4];
    float lreg = 0.f, dreg = 0.f;
    auto fetch = [&](int qt) {
        abw_fetch(qreg, qb, 2304, qt * 64, T, tid);
        abw_fetch(greg, gb, 768, qt * 64, T, tid);
        if (tid < 64) {
            const int q = qt * 64 + tid;
            lreg = q < T ? lb[q] : 0.f;
            dreg = q < T ? Db[q] : 0.f;
        }
    };
    fetch(0);
    for (int qt = 0; qt < ntiles; ++qt) {
        __syncthreads();
        abw_store(Qs, qreg, tid);
        abw_store(Gs, greg, tid);
        if (tid < 64) {
            lse_s[tid] = lreg;
            D_s[tid] = dreg;
        }
        __syncthreads();
        if (qt + 1 < ntiles) fetch(qt + 1);
        if (!wave_active) continue;
        const int q0 = qt * 64;
        const int nsub = min(4, (T - q0 + 15) / 16);  // query sub-tiles holding at least one valid row (uniform)
        for (int sub = 0; sub < nsub; ++sub) {
            f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
                const f32x4 qa = *reinterpret_cast<const f32x4*>(Qs + (sub * 16 + fi) * kAttnLD + dd * 16 + g * 4);
                const f32x4 ga = *reinterpret_cast<const f32x4*>(Gs + (sub * 16 + fi) * kAttnLD + dd * 16 + g * 4);
                s = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[0], kf[dd][0], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[0], vf[dd][0], dp, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[1], kf[dd][1], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[1], vf[dd][1], dp, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[2], kf[dd][2], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[2], vf[dd][2], dp, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[3], kf[dd][3], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[3], vf[dd][3], dp, 0, 0, 0);
            }
            // lane: key (column fi), queries q0 + 16*sub + 4g + r
            const f32x4 lv = *reinterpret_cast<const f32x4*>(lse_s + sub * 16 + g * 4);
            const f32x4 Dv = *reinterpret_cast<const f32x4*>(D_s + sub * 16 + g * 4);
            f32x4 pm, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = q0 + sub * 16 + g * 4 + r;
                const bool ok = q < T && key < T;
                const float p = ok ? fast_exp(s[r] - lv[r]) : 0.f;
                const float mk = (DROP && ok) ? drop_mult(dc, site, mask0 + (unsigned long long)q * T + key) : 1.0f;
                pm[r] = p * mk;
                ds[r] = p * (dp[r] * mk - Dv[r]);
            }
            // dV += Pm^T dO, dK += dS^T Q : k-step r contracts queries 16*sub + 4g + r
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* grow = Gs + (sub * 16 + g * 4 + r) * kAttnLD + fi;
                const float* qrow = Qs + (sub * 16 + g * 4 + r) * kAttnLD + fi;
#pragma unroll
                for (int di = 0; di < 4; ++di) {
                    dv[di] = __builtin_amdgcn_mfma_f32_16x16x4f32(pm[r], grow[di * 16], dv[di], 0, 0, 0);
                    dk[di] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[r], qrow[di * 16], dk[di], 0, 0, 0);
                }
            }
        }
    }
    // accumulators: row = key 4g + r of this wave's 16, column d = 16*di + fi
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int kk = k0 + wave * 16 + g * 4 + r;
        if (kk < T) {
            float* dst = dqkv + (row0 + kk) * 2304 + h * 64 + fi;
#pragma unroll
            for (int di = 0; di < 4; ++di) {
                dst[768 + di * 16] = dk[di][r];
                dst[1536 + di * 16] = dv[di][r];
            }
        }
    }
}

template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                          const float* __restrict__ lse, const float* __restrict__ D,
                                                          float* __restrict__ dqkv, int T, DropCfg dc, uint32_t site, int bh0,
                                                          const int* __restrict__ tpref = nullptr, int t_min = 0) {
    __shared__ __attribute__((aligned(16))) float Ks[64 * kAttnLD];
    __shared__ __attribute__((aligned(16))) float Vs[64 * kAttnLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, g = lane >> 4;
    const int bh = blockIdx.y;
    int b = bh / 12;
    const int h = bh - b * 12;
    long long row0 = (long long)b * T;
    unsigned long long mask0 = (unsigned long long)(bh0 + bh) * T * T;
    if (tpref) {
        b += bh0 / 12;
        row0 = tpref[b];
        T = tpref[b + 1] - tpref[b];
        if ((int)blockIdx.x * 64 >= T || T < t_min) return;   // whole workgroup, before any barrier
        if (DROP) mask0 = attn_mask_base(tpref, b) + (unsigned long long)h * T * T;
    }
    const float* qb = qkv + row0 * 2304 + h * 64;
    const float* gb = dO + row0 * 768 + h * 64;
    const int q = blockIdx.x * 64 + wave * 16 + fi;
    const int q_ld = q < T ? q : T - 1;
    const bool wave_active = blockIdx.x * 64 + wave * 16 < T;

    f32x4 qf[4], gf[4];
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) {
        qf[dd] = *reinterpret_cast<const f32x4*>(qb + (long long)q_ld * 2304 + dd * 16 + g * 4);
        gf[dd] = *reinterpret_cast<const f32x4*>(gb + (long long)q_ld * 768 + dd * 16 + g * 4);
    }
    const float lse_q = lse[12 * row0 + (long long)h * T + q_ld], D_q = D[12 * row0 + (long long)h * T + q_ld];
    f32x4 dq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) dq[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int ntiles = (T + 63) / 64;
    f32x4 kreg[4], vreg[4];
    auto fetch = [&](int kt) {
        abw_fetch(kreg, qb + 768, 2304, kt * 64, T, tid);
        abw_fetch(vreg, qb + 1536, 2304, kt * 64, T, tid);
    };
    fetch(0);
    for (int kt = 0; kt < ntiles; ++kt) {
        __syncthreads();
        abw_store(Ks, kreg, tid);
        abw_store(Vs, vreg, tid);
        __syncthreads();
        if (kt + 1 < ntiles) fetch(kt + 1);
        if (!wave_active) continue;
        const int k0 = kt * 64;
        const int nsub = min(4, (T - k0 + 15) / 16);
        for (int sub = 0; sub < nsub; ++sub) {
            f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
                const f32x4 ka = *reinterpret_cast<const f32x4*>(Ks + (sub * 16 + fi) * kAttnLD + dd * 16 + g * 4);
                const f32x4 va = *reinterpret_cast<const f32x4*>(Vs + (sub * 16 + fi) * kAttnLD + dd * 16 + g * 4);
                s = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[0], qf[dd][0], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(va[0], gf[dd][0], dp, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[1], qf[dd][1], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(va[1], gf[dd][1], dp, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[2], qf[dd][2], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(va[2], gf[dd][2], dp, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[3], qf[dd][3], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(va[3], gf[dd][3], dp, 0, 0, 0);
            }
            // lane: query (column fi), keys k0 + 16*sub + 4g + r
            f32x4 ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + sub * 16 + g * 4 + r;
                const bool ok = q < T && key < T;
                const float p = ok ? fast_exp(s[r] - lse_q) : 0.f;
                const float mk = (DROP && ok) ? drop_mult(dc, site, mask0 + (unsigned long long)q * T + key) : 1.0f;
                ds[r] = p * (dp[r] * mk - D_q);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* krow = Ks + (sub * 16 + g * 4 + r) * kAttnLD + fi;
#pragma unroll
                for (int di = 0; di < 4; ++di)
                    dq[di] = __builtin_amdgcn_mfma_f32_16x16x4f32(krow[di * 16], ds[r], dq[di], 0, 0, 0);
            }
        }
    }
    if (q < T) {  // dQ^T accumulators: row d = 16*di + 4g + r, column = this lane's query
        float* dst = dqkv + (row0 + q) * 2304 + h * 64 + g * 4;
#pragma unroll
        for (int di = 0; di < 4; ++di) {
            *reinterpret_cast<f32x4*>(dst + di * 16) = dq[di];
        }
    }
}

// ---- T <= 64: the three kernels above as ONE launch (round 6) --------------------------------------------------------------------
// configs[3] (nomad.forward() on 1 s clips, T = 50) ran rowdot + dkv + dq as 36 launches of 5-15 us per step, each a single workgroup
// per (clip, head) that re-reads the same four 64 x 64 tiles.  Here one workgroup per (clip, head) stages Q, K, V, dO once, takes
// D = rowdot(dO, O) into LDS, then runs the dkv body (wave = 16 keys) and the dq body (wave = 16 queries) on the staged tiles.  Every
// product, sum and exponential is the one the three-kernel path computes, in the same order: bit-identical results
// (tests/test_gpu_backward.py::test_attention_backward); the choice depends on T alone, so a clip's bits do not depend on its batch.
// No attention dropout here (the fine-tuning path with dropout keeps the three kernels).  D is still written: the caller's scratch.
constexpr int kAttnBwdSmallLds = (4 * 64 * kAttnLD + 128) * 4;
__global__ __launch_bounds__(256) void attn_bwd_small_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                             const float* __restrict__ dO, const float* __restrict__ lse,
                                                             float* __restrict__ D, float* __restrict__ dqkv, int T,
                                                             const int* __restrict__ tpref = nullptr, int bh0 = 0) {
    extern __shared__ __attribute__((aligned(16))) float abw_smem[];   // kAttnBwdSmallLds bytes (four 64 x 68 tiles: over the 64 KB static limit)
    float* const Qs = abw_smem;
    float* const Gs = Qs + 64 * kAttnLD;  // dO
    float* const Ks = Gs + 64 * kAttnLD;
    float* const Vs = Ks + 64 * kAttnLD;
    float* const lse_s = Vs + 64 * kAttnLD;
    float* const D_s = lse_s + 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, g = lane >> 4;
    const int bh = blockIdx.x;
    int b = bh / 12;
    const int h = bh - b * 12;
    long long row0 = (long long)b * T;
    if (tpref) {   // ragged batch: clips of more than 64 frames belong to the three kernels
        b += bh0 / 12;
        row0 = tpref[b];
        T = tpref[b + 1] - tpref[b];
        if (T > 64) return;   // whole workgroup, before any barrier
    }
    const long long ld0 = 12 * row0 + (long long)h * T;   // this (clip, head)'s row of lse / D
    const float* qb = qkv + row0 * 2304 + h * 64;
    const float* gb = dO + row0 * 768 + h * 64;
    const float* ob = o + row0 * 768 + h * 64;
    {
        f32x4 r0[4], r1[4], r2[4], r3[4];
        abw_fetch(r0, qb, 2304, 0, T, tid);
        abw_fetch(r1, gb, 768, 0, T, tid);
        abw_fetch(r2, qb + 768, 2304, 0, T, tid);
        abw_fetch(r3, qb + 1536, 2304, 0, T, tid);
        // D[q] = sum_d dO[q][d] O[q][d]: 16 lanes per row, lane j holds d = 4 j .. 4 j + 3, then the xor tree - attn_bwd_rowdot_kernel's order
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int q = pass * 16 + (tid >> 4), j = tid & 15;
            const int qr = q < T ? q : T - 1;
            const f32x4 a = *reinterpret_cast<const f32x4*>(ob + (long long)qr * 768 + 4 * j);
            const f32x4 gg = *reinterpret_cast<const f32x4*>(gb + (long long)qr * 768 + 4 * j);
            float sdot = (a[0] * gg[0] + a[1] * gg[1]) + (a[2] * gg[2] + a[3] * gg[3]);
            sdot += __shfl_xor(sdot, 1);
            sdot += __shfl_xor(sdot, 2);
            sdot += __shfl_xor(sdot, 4);
            sdot += __shfl_xor(sdot, 8);
            if (j == 0) {
                D_s[q] = q < T ? sdot : 0.f;
                if (q < T) D[ld0 + q] = sdot;
            }
        }
        if (tid < 64) lse_s[tid] = tid < T ? lse[ld0 + tid] : 0.f;
        abw_store(Qs, r0, tid);
        abw_store(Gs, r1, tid);
        abw_store(Ks, r2, tid);
        abw_store(Vs, r3, tid);
    }
    __syncthreads();
    if (wave * 16 >= T) return;   // (wave-uniform; no barrier below)
    const int nsub = min(4, (T + 15) / 16);
    // ---- dK, dV: this wave's 16 keys -------------------------------------------------------------------------------------------
    {
        const int key = wave * 16 + fi;
        const int key_ld = key < T ? key : T - 1;
        f32x4 kf[4], vf[4];
#pragma unroll
        for (int dd = 0; dd < 4; ++dd) {
            kf[dd] = *reinterpret_cast<const f32x4*>(Ks + key_ld * kAttnLD + dd * 16 + g * 4);
            vf[dd] = *reinterpret_cast<const f32x4*>(Vs + key_ld * kAttnLD + dd * 16 + g * 4);
        }
        f32x4 dk[4], dv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) dk[i] = dv[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int sub = 0; sub < nsub; ++sub) {
            f32x4 sacc = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
                const f32x4 qa = *reinterpret_cast<const f32x4*>(Qs + (sub * 16 + fi) * kAttnLD + dd * 16 + g * 4);
                const f32x4 ga = *reinterpret_cast<const f32x4*>(Gs + (sub * 16 + fi) * kAttnLD + dd * 16 + g * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    sacc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[c], kf[dd][c], sacc, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[c], vf[dd][c], dp, 0, 0, 0);
                }
            }
            const f32x4 lv = *reinterpret_cast<const f32x4*>(lse_s + sub * 16 + g * 4);
            const f32x4 Dv = *reinterpret_cast<const f32x4*>(D_s + sub * 16 + g * 4);
            f32x4 pm, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = sub * 16 + g * 4 + r;
                const bool ok = q < T && key < T;
                const float pr = ok ? fast_exp(sacc[r] - lv[r]) : 0.f;
                pm[r] = pr * 1.0f;
                ds[r] = pr * (dp[r] * 1.0f - Dv[r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* grow = Gs + (sub * 16 + g * 4 + r) * kAttnLD + fi;
                const float* qrow = Qs + (sub * 16 + g * 4 + r) * kAttnLD + fi;
#pragma unroll
                for (int di = 0; di < 4; ++di) {
                    dv[di] = __builtin_amdgcn_mfma_f32_16x16x4f32(pm[r], grow[di * 16], dv[di], 0, 0, 0);
                    dk[di] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[r], qrow[di * 16], dk[di], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kk = wave * 16 + g * 4 + r;
            if (kk < T) {
                float* dst = dqkv + (row0 + kk) * 2304 + h * 64 + fi;
#pragma unroll
                for (int di = 0; di < 4; ++di) {
                    dst[768 + di * 16] = dk[di][r];
                    dst[1536 + di * 16] = dv[di][r];
                }
            }
        }
    }
    // ---- dQ: this wave's 16 queries --------------------------------------------------------------------------------------------
    {
        const int q = wave * 16 + fi;
        const int q_ld = q < T ? q : T - 1;
        f32x4 qf[4], gf[4];
#pragma unroll
        for (int dd = 0; dd < 4; ++dd) {
            qf[dd] = *reinterpret_cast<const f32x4*>(Qs + q_ld * kAttnLD + dd * 16 + g * 4);
            gf[dd] = *reinterpret_cast<const f32x4*>(Gs + q_ld * kAttnLD + dd * 16 + g * 4);
        }
        const float lse_q = lse_s[q_ld], D_q = D_s[q_ld];
        f32x4 dq[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) dq[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int sub = 0; sub < nsub; ++sub) {
            f32x4 sacc = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
                const f32x4 ka = *reinterpret_cast<const f32x4*>(Ks + (sub * 16 + fi) * kAttnLD + dd * 16 + g * 4);
                const f32x4 va = *reinterpret_cast<const f32x4*>(Vs + (sub * 16 + fi) * kAttnLD + dd * 16 + g * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    sacc = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[c], qf[dd][c], sacc, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x4f32(va[c], gf[dd][c], dp, 0, 0, 0);
                }
            }
            f32x4 ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = sub * 16 + g * 4 + r;
                const bool ok = q < T && key < T;
                const float pr = ok ? fast_exp(sacc[r] - lse_q) : 0.f;
                ds[r] = pr * (dp[r] * 1.0f - D_q);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* krow = Ks + (sub * 16 + g * 4 + r) * kAttnLD + fi;
#pragma unroll
                for (int di = 0; di < 4; ++di)
                    dq[di] = __builtin_amdgcn_mfma_f32_16x16x4f32(krow[di * 16], ds[r], dq[di], 0, 0, 0);
            }
        }
        if (q < T) {
            float* dst = dqkv + (row0 + q) * 2304 + h * 64 + g * 4;
#pragma unroll
            for (int di = 0; di < 4; ++di) *reinterpret_cast<f32x4*>(dst + di * 16) = dq[di];
        }
    }
}

// D scratch: [B*12][T] floats.
// bh0: (clip, head) index of the first clip within the whole batch (dropout mask indexing of a per-branch call)
inline hipError_t launch_attention_bwd(const float* qkv, const float* o, const float* dO, const float* lse, float* D,
                                       float* dqkv, int B, int T, const DropCfg& dc, uint32_t site, hipStream_t s,
                                       int bh0 = 0, bool force_three = false) {
    const int M = B * T;
    if (T <= 64 && !dc.threshold && !force_three) {   // by the clip's length only: one fused launch (bit-identical to the three below)
        static LdsAttrOnce attr_set;
        if (hipError_t e = attr_set.ensure(reinterpret_cast<const void*>(attn_bwd_small_kernel), kAttnBwdSmallLds); e != hipSuccess) return e;
        hipLaunchKernelGGL(attn_bwd_small_kernel, dim3(B * 12), dim3(256), kAttnBwdSmallLds, s, qkv, o, dO, lse, D, dqkv, T, static_cast<const int*>(nullptr), 0);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(attn_bwd_rowdot_kernel, dim3((M + 3) / 4), dim3(256), 0, s, o, dO, D, M, T, static_cast<const int*>(nullptr), 0, 0, 0);
    const dim3 grid((T + 63) / 64, B * 12);
    if (dc.threshold) {
        hipLaunchKernelGGL(attn_bwd_dkv_kernel<true>, grid, dim3(256), 0, s, qkv, dO, lse, D, dqkv, T, dc, site, bh0, static_cast<const int*>(nullptr), 0);
        hipLaunchKernelGGL(attn_bwd_dq_kernel<true>, grid, dim3(256), 0, s, qkv, dO, lse, D, dqkv, T, dc, site, bh0, static_cast<const int*>(nullptr), 0);
    } else {
        hipLaunchKernelGGL(attn_bwd_dkv_kernel<false>, grid, dim3(256), 0, s, qkv, dO, lse, D, dqkv, T, dc, site, bh0, static_cast<const int*>(nullptr), 0);
        hipLaunchKernelGGL(attn_bwd_dq_kernel<false>, grid, dim3(256), 0, s, qkv, dO, lse, D, dqkv, T, dc, site, bh0, static_cast<const int*>(nullptr), 0);
    }
    return hipGetLastError();
}

// The same over clips [c0, c0 + nc) of a ragged batch of `nclips` clips (every pointer and tpref: the whole batch's; rows
// [m0, m1) are those clips' frames; max_t / min_t: the batch's longest / shortest clip).
inline hipError_t launch_attention_bwd_ragged(const float* qkv, const float* o, const float* dO, const float* lse, float* D,
                                              float* dqkv, const int* tpref, int nclips, int c0, int nc, int m0, int m1, int max_t,
                                              int min_t, const DropCfg& dc, uint32_t site, hipStream_t s, bool force_three = false) {
    const bool fused = !dc.threshold && !force_three;   // clips of at most 64 frames take the fused kernel
    const int bh0 = c0 * 12;
    if (fused && min_t <= 64) {
        static LdsAttrOnce attr_set;
        if (hipError_t e = attr_set.ensure(reinterpret_cast<const void*>(attn_bwd_small_kernel), kAttnBwdSmallLds); e != hipSuccess) return e;
        hipLaunchKernelGGL(attn_bwd_small_kernel, dim3(nc * 12), dim3(256), kAttnBwdSmallLds, s, qkv, o, dO, lse, D, dqkv, 0, tpref, bh0);
    }
    if (!fused || max_t > 64) {
        const int t_min = fused ? 65 : 0;
        hipLaunchKernelGGL(attn_bwd_rowdot_kernel, dim3((m1 - m0 + 3) / 4), dim3(256), 0, s, o, dO, D, m1, 0, tpref, nclips, m0, t_min);
        const dim3 grid((max_t + 63) / 64, nc * 12);
        if (dc.threshold) {
            hipLaunchKernelGGL(attn_bwd_dkv_kernel<true>, grid, dim3(256), 0, s, qkv, dO, lse, D, dqkv, 0, dc, site, bh0, tpref, t_min);
            hipLaunchKernelGGL(attn_bwd_dq_kernel<true>, grid, dim3(256), 0, s, qkv, dO, lse, D, dqkv, 0, dc, site, bh0, tpref, t_min);
        } else {
            hipLaunchKernelGGL(attn_bwd_dkv_kernel<false>, grid, dim3(256), 0, s, qkv, dO, lse, D, dqkv, 0, dc, site, bh0, tpref, t_min);
            hipLaunchKernelGGL(attn_bwd_dq_kernel<false>, grid, dim3(256), 0, s, qkv, dO, lse, D, dqkv, 0, dc, site, bh0, tpref, t_min);
        }
    }
    return hipGetLastError();
}

}  // namespace nomad
