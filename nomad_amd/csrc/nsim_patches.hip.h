// Patch-wise NSIM: the clean spectrogram cut into patches, the active ones kept, each searched for in the degraded spectrogram, the
// chain of best places chosen and the patches' similarities averaged (nomad_nsim_patches; include/nomad_hip.h states the measure in
// full and is the definition, tests/patch_nsim_ref.py restates it).  Modelled on what ViSQOL's speech mode is remembered to do, NOT
// checked against the ViSQOL binary.  A candidate is nomad_nsim of the cut-out pair and has its bits: everything per value, per cell
// and per walk is nsim.hip.h's own (nsim_db, nsim_max, nsim_window inside nsim_cell, nsim_band_mean, nsim_of_bands); what this
// file adds is where the values are kept and who computes them.
//
// patch_activity_kernel - one workgroup per clean clip: the frame energies (products rounded, then added: no contraction), their
// NaN-sticky maximum folded in LDS, the activity flags, and per patch whether enough of its frames are active.
//
// patch_candidates_kernel - the hot path.  One workgroup per (degraded row, patch); a patch that is not kept, or has no candidate in
// this row, leaves before any barrier.  The mapping and its reasons:
//   * staged ONCE per workgroup, in LDS, as dB: the clean patch [patch][21] and the degraded slab [hi - lo + patch][21] that all
//     candidates of the window [lo, hi] read, so nsim_db (a log10) runs once per spectrogram value and not once per candidate
//     (2 search + 1 times less); beside them the per-frame maxima of either plane, combined per pairing by one nsim_max (a maximum
//     does not depend on its order, and a NaN sticks either way).
//   * candidates are dealt over the waves (candidate j of the window goes to wave j mod W in round j / W); a candidate's patch x 21
//     cells are dealt over the wave's 64 lanes, cell i = lane + 64 k.  Per candidate a wave keeps three planes of its own in LDS
//     (the floored clean and degraded planes with the minimum subtracted, and the map) and 21 band values: the planes are what
//     nsim_window reads, with the edges replicated at the PATCH's edges.  The minimum over both planes is folded per lane in cell
//     order, then across the wave by xor shuffles (a minimum does not depend on its order; a NaN is carried by a flag beside it).
//   * LDS budget in float64 values: 21 patch + 21 (patch + 2 search) + 2 patch + 2 search staged, 63 patch + 24 per wave.  patch 20 /
//     search 60: 27.9 KB + 4 x 10.3 KB = 69 KB, two workgroups per CU; the largest case (patch 64 / search 128) is 67.6 KB + 32.4 KB
//     per wave, so the host drops from W = 4 to W = 2 waves where four do not fit into 160 KB.  The bits do not depend on W.
//   * banks: every plane is rows of 21 float64 = 42 dwords, cells consecutive.  A half-wave's 32 consecutive cells are 256
//     consecutive bytes: one bank row of ds_read_b64, conflict-free; a window tap reads the same run moved by 21 dt + db cells,
//     with two equal addresses (a broadcast) where an edge is replicated.  The stores are one float64 per lane, consecutive.
//   * expected issue balance, NOT measured: per cell 18 LDS reads against about 60 float64 operations, a division and two square
//     roots in nsim_cell, so the map phase should be bound by the float64 pipe (the guides state no float64 rate for gfx950; the
//     vector rate AMD publishes is 78.6 TFLOP/s); the floor phase is two reads and two stores per cell; the walks are serial: 21
//     lanes add `patch` values each, then one lane adds 21, while the other lanes of that wave idle.  The phases are separated by
//     workgroup barriers (four per round), so the waves of a workgroup walk together and it is the second workgroup of the CU that
//     fills those gaps.  tools/bench_patch_nsim.py measures the stage.
//   * no atomics, one fixed order per candidate that depends on `patch` alone: a candidate has the bits of nomad_nsim (B = 1,
//     G = 1, frames = patch) on the cut-outs whatever the batch, the window and W.
//
// patch_select_kernel - one workgroup per degraded row.  Walks the kept patches in order: T_k[u] = T_{k-1}[a_k(u)] + q_k[u] with
// a_k(u) the best place of the patch before at or ahead of u; "best so far" is an inclusive scan under a total order (larger T,
// then nearer to the patch's own start, then the earlier place) done by wave 0, each lane owning ceil((2 search + 1) / 64) <= 5
// consecutive places: a lane-local walk, a shuffle scan of the lanes' bests, and the lanes' exclusive result applied.  Choosing
// under a total order does not depend on the scan's shape.  Thread 0 traces the chain back; then the chosen candidates are computed
// once more (by patch_candidate, the same code) for their band values, added in ascending patch order.
#pragma once
#include <hip/hip_runtime.h>

#include "nsim.hip.h"

namespace nomad {

constexpr int kPatchMax = 64, kPatchSearchMax = 128;
constexpr int kPatchPlacesMax = 2 * kPatchSearchMax + 1;      // 257
constexpr size_t kPatchLdsMax = 160 * 1024;

// float64 values of LDS: what a workgroup stages for a window of `places` = 2 search + 1, and what one wave needs per candidate
__host__ __device__ inline size_t patch_staged_doubles(int patch, int search) { return (size_t)(kGammatoneBands + 1) * (size_t)(2 * patch + 2 * search); }
__host__ __device__ inline size_t patch_wave_doubles(int patch) { return 3 * (size_t)kGammatoneBands * (size_t)patch + 24; }

// Grid B, 256 threads.  E[fpref[b] + t], active[fpref[b] + t], kept[ppref[b] + p], clipbad[b].
__global__ __launch_bounds__(256) void patch_activity_kernel(const double* __restrict__ spec_ref, const int* __restrict__ frames,
                                                             const long long* __restrict__ fpref, const long long* __restrict__ ppref,
                                                             int patch, double vad_ratio, int min_active, double* __restrict__ E,
                                                             int* __restrict__ active, int* __restrict__ kept, int* __restrict__ clipbad) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x, F = frames[b];
    const double* sr = spec_ref + (size_t)fpref[b] * kGammatoneBands;
    double* Eb = E + (size_t)fpref[b];
    int* ab = active + (size_t)fpref[b];
    double top = -INFINITY;
    for (int t = tid; t < F; t += 256) {
        double acc = 0.0;
        for (int k = 0; k < kGammatoneBands; ++k) {
            const double v = sr[(size_t)t * kGammatoneBands + k];
            acc = __dadd_rn(acc, __dmul_rn(v, v));   // the product rounded, then added: never one fused operation
        }
        Eb[t] = acc;
        top = nsim_max(top, acc);
    }
    red[tid] = top;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) red[tid] = nsim_max(red[tid], red[tid + h]);
        __syncthreads();
    }
    top = red[0];
    const double thr = __dmul_rn(vad_ratio, top);
    for (int t = tid; t < F; t += 256) ab[t] = Eb[t] >= thr ? 1 : 0;   // its own E: no barrier needed for it
    if (tid == 0) clipbad[b] = top != top ? 1 : 0;
    __syncthreads();                                                   // the flags of other threads, through memory
    const int P = (int)(ppref[b + 1] - ppref[b]);
    for (int p = tid; p < P; p += 256) {
        int n = 0;
        for (int t = 0; t < patch; ++t) n += ab[(size_t)p * patch + t];
        kept[(size_t)ppref[b] + p] = n >= min_active ? 1 : 0;
    }
}

// dB planes of `rows` frames from a spectrogram, and their per-frame maxima (bands ascending): all threads of the workgroup.
__device__ __forceinline__ void patch_stage(const double* __restrict__ spec, int rows, double* __restrict__ plane, double* __restrict__ peak,
                                            int tid, int threads) {
    for (int i = tid; i < rows * kGammatoneBands; i += threads) plane[i] = nsim_db(spec[i]);
    __syncthreads();
    for (int t = tid; t < rows; t += threads) {
        const double* row = plane + (size_t)t * kGammatoneBands;
        double top = row[0];
        for (int k = 1; k < kGammatoneBands; ++k) top = nsim_max(top, row[k]);
        peak[t] = top;
    }
}

// One candidate: nomad_nsim of the clean patch Rdb [patch][21] and the degraded frames Ddb [patch][21] (dB planes in LDS, pr / pd
// their per-frame maxima).  EVERY thread of the workgroup calls it the same number of times - it holds three barriers -, and the
// waves with `live` compute, each on planes of its own (Rw, Dw, Mw [patch][21]; bw [21] receives the band values).  Lane 0 of a
// live wave returns the NSIM.  The caller needs no barrier between two calls: what a call writes first, the call before stopped
// reading ahead of its own last barrier.
__device__ __forceinline__ double patch_candidate(bool live, const double* __restrict__ Rdb, const double* __restrict__ Ddb,
                                                  const double* __restrict__ pr, const double* __restrict__ pd, int patch, double C1,
                                                  double C3, double* __restrict__ Rw, double* __restrict__ Dw, double* __restrict__ Mw,
                                                  double* __restrict__ bw, int lane) {
    const int n = patch * kGammatoneBands;
    double lo = INFINITY;
    int nan = 0;
    if (live) {
        for (int i = lane; i < n; i += 64) {
            const int t = i / kGammatoneBands;
            const double floor_t = nsim_max(pr[t], pd[t]) - 45.0;
            const double a = nsim_max(floor_t, Rdb[i]), d = nsim_max(floor_t, Ddb[i]);   // a NaN floor stays, a NaN value enters
            Rw[i] = a;
            Dw[i] = d;
            nan |= (a != a) | (d != d);
            lo = (a < lo) ? a : lo;
            lo = (d < lo) ? d : lo;
        }
    }
    for (int h = 32; h >= 1; h >>= 1) {
        const double o = __shfl_xor(lo, h);
        lo = o < lo ? o : lo;
        nan |= __shfl_xor(nan, h);
    }
    const double least = nan ? (double)NAN : lo;
    if (live) {
        for (int i = lane; i < n; i += 64) {   // the lane's own cells
            Rw[i] -= least;
            Dw[i] -= least;
        }
    }
    __syncthreads();
    if (live) {
        for (int i = lane; i < n; i += 64) Mw[i] = nsim_cell(Rw, Dw, patch, i / kGammatoneBands, i % kGammatoneBands, C1, C3);
    }
    __syncthreads();
    if (live && lane < kGammatoneBands) bw[lane] = nsim_band_mean(Mw, patch, lane);
    __syncthreads();
    return (live && lane == 0) ? nsim_of_bands(bw) : 0.0;
}

// The tables of a call, all in the workspace.  rp = G ppref[b] + g P_b + p numbers the (row, patch) pairs.
struct PatchTables {
    const int* frames;          // [B]
    const int* dframes;         // [B G]
    const long long* fpref;     // [B + 1] clean frames ahead of clip b
    const long long* dpref;     // [B G + 1] degraded frames ahead of row r
    const long long* ppref;     // [B + 1] patches ahead of clip b
    const int* kept;            // [sum P_b] enough active frames
    const int* clipbad;         // [B] a NaN in the clean clip
};

// Grid R maxP (flat: row r = blockIdx.x / maxP, patch p = blockIdx.x % maxP), 64 W threads, dynamic LDS
// 8 (patch_staged_doubles + W patch_wave_doubles) bytes.  cand[rp][u - (s - search)] <- q_p[u] for u in [lo, hi].
__global__ __launch_bounds__(256) void patch_candidates_kernel(const double* __restrict__ spec_ref, const double* __restrict__ spec_deg, int G,
                                                               PatchTables tb, int patch, int search, int maxP, double C1, double C3,
                                                               double* __restrict__ cand) {
    extern __shared__ double pcand_lds[];
    const int r = (int)(blockIdx.x / (unsigned)maxP), p = (int)(blockIdx.x % (unsigned)maxP);
    const int b = r / G, g = r % G, tid = threadIdx.x, threads = blockDim.x, W = threads >> 6, wave = tid >> 6, lane = tid & 63;
    const int P = (int)(tb.ppref[b + 1] - tb.ppref[b]);
    if (p >= P || !tb.kept[(size_t)tb.ppref[b] + p]) return;   // the whole workgroup: no barrier is left behind
    const int Fd = tb.dframes[r], s = p * patch;
    const int lo = s - search > 0 ? s - search : 0, hi = s + search < Fd - patch ? s + search : Fd - patch;
    if (lo > hi) return;
    const int slab = hi - lo + patch, places = 2 * search + 1;   // slab <= patch + 2 search frames, all inside the row: hi + patch <= Fd
    double* Rdb = pcand_lds;
    double* Dsl = Rdb + (size_t)kGammatoneBands * patch;
    double* pr = Dsl + (size_t)kGammatoneBands * (patch + 2 * search);
    double* pd = pr + patch;
    double* mine = pd + (patch + 2 * search) + (size_t)wave * patch_wave_doubles(patch);
    double* Rw = mine;
    double* Dw = Rw + (size_t)kGammatoneBands * patch;
    double* Mw = Dw + (size_t)kGammatoneBands * patch;
    double* bw = Mw + (size_t)kGammatoneBands * patch;
    patch_stage(spec_ref + ((size_t)tb.fpref[b] + (size_t)s) * kGammatoneBands, patch, Rdb, pr, tid, threads);
    patch_stage(spec_deg + ((size_t)tb.dpref[r] + (size_t)lo) * kGammatoneBands, slab, Dsl, pd, tid, threads);
    __syncthreads();
    const size_t rp = (size_t)G * (size_t)tb.ppref[b] + (size_t)g * (size_t)P + (size_t)p;
    double* out = cand + rp * (size_t)places + (lo - (s - search));
    const int n = hi - lo + 1, rounds = (n + W - 1) / W;
    for (int c = 0; c < rounds; ++c) {
        const int j = c * W + wave;
        const bool live = j < n;
        const int off = live ? j : 0;
        const double q = patch_candidate(live, Rdb, Dsl + (size_t)off * kGammatoneBands, pr, pd + off, patch, C1, C3, Rw, Dw, Mw, bw, lane);
        if (live && lane == 0) out[j] = q;
    }
}

// The order of the selection among places of one window: larger T, then nearer to the patch's start (column `search`), then the
// earlier place.  x, y are columns of the window; y < 0 stands for "none yet".
__device__ __forceinline__ bool patch_better(const double* __restrict__ T, int search, int x, int y) {
    if (y < 0) return true;
    const double tx = T[x], ty = T[y];
    if (tx != ty) return tx > ty;
    const int dx = x < search ? search - x : x - search, dy = y < search ? search - y : y - search;
    return dx != dy ? dx < dy : x < y;
}

// Grid B G, 256 threads, dynamic LDS 8 (44 patch + patch_wave_doubles(patch)) bytes.  back [rp][places] int32, link / pick [rp] int32.
__global__ __launch_bounds__(256) void patch_select_kernel(const double* __restrict__ spec_ref, const double* __restrict__ spec_deg, int G,
                                                           PatchTables tb, int patch, int search, double C1, double C3,
                                                           const double* __restrict__ cand, int* __restrict__ back, int* __restrict__ link,
                                                           int* __restrict__ pick, int out_patches, double* __restrict__ nsim,
                                                           double* __restrict__ bands, int* __restrict__ offsets,
                                                           double* __restrict__ patch_nsim, double* __restrict__ cand_out) {
    extern __shared__ double psel_lds[];
    __shared__ double Ta[kPatchPlacesMax], Tb[kPatchPlacesMax];
    __shared__ int best[kPatchPlacesMax];
    __shared__ int bad;
    const int r = blockIdx.x, b = r / G, g = r % G, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int P = (int)(tb.ppref[b + 1] - tb.ppref[b]), Fd = tb.dframes[r], places = 2 * search + 1;
    const size_t rp0 = (size_t)G * (size_t)tb.ppref[b] + (size_t)g * (size_t)P;
    const size_t o0 = (size_t)r * (size_t)out_patches;
    for (int i = tid; i < out_patches; i += 256) {
        if (offsets) offsets[o0 + i] = -1;
        if (patch_nsim) patch_nsim[o0 + i] = (double)NAN;
    }
    if (cand_out)
        for (size_t i = tid; i < (size_t)out_patches * places; i += 256) cand_out[o0 * places + i] = (double)NAN;
    if (tid == 0) bad = tb.clipbad[b];
    __syncthreads();
    double* Tp = Ta;   // the patch before: T over its window's columns
    double* Tc = Tb;
    int K = 0, prev = -1, plo = 0, phi = 0, ps = 0;   // the kept patch before, its window [plo, phi] and start
    for (int p = 0; p < P; ++p) {
        const int s = p * patch;
        const int lo = s - search > 0 ? s - search : 0, hi = s + search < Fd - patch ? s + search : Fd - patch;
        const size_t rp = rp0 + (size_t)p;
        if (tid == 0) pick[rp] = -1;
        if (!tb.kept[(size_t)tb.ppref[b] + p] || lo > hi) continue;   // uniform over the workgroup
        const int c0 = lo - (s - search), c1 = hi - (s - search);
        for (int c = c0 + tid; c <= c1; c += 256) {
            const double q = cand[rp * (size_t)places + c];
            if (cand_out) cand_out[(o0 + (size_t)p) * places + c] = q;
            if (q != q) bad = 1;
            if (prev < 0) {
                Tc[c] = q;
            } else {
                const int u = s - search + c, m = u < phi ? u : phi;   // m >= plo: the windows' starts do not decrease
                const int a = best[m - (ps - search)];
                back[rp * (size_t)places + c] = a;
                Tc[c] = Tp[a] + q;
            }
        }
        if (tid == 0) link[rp] = prev;
        __syncthreads();
        if (wave == 0) {   // best[c] <- the best column in [c0, c] under the order
            const int chunk = (places + 63) / 64, first = lane * chunk;
            int mine = -1;
            for (int c = first; c < first + chunk; ++c)
                if (c >= c0 && c <= c1) {
                    if (patch_better(Tc, search, c, mine)) mine = c;
                    best[c] = mine;
                }
            int incl = mine;
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl, d);
                if (lane >= d && o >= 0 && patch_better(Tc, search, o, incl)) incl = o;
            }
            int excl = __shfl_up(incl, 1);
            if (lane == 0) excl = -1;
            if (excl >= 0)
                for (int c = first; c < first + chunk; ++c)
                    if (c >= c0 && c <= c1 && patch_better(Tc, search, excl, best[c])) best[c] = excl;
        }
        __syncthreads();
        double* t = Tp;
        Tp = Tc;
        Tc = t;
        prev = p;
        plo = lo;
        phi = hi;
        ps = s;
        ++K;
    }
    (void)plo;
    const bool live = K > 0 && !bad;   // `bad` was last written ahead of the loop's last barrier (or the one above it)
    if (tid == 0) {
        double score = (double)NAN;
        if (live) {
            int col = best[phi - (ps - search)];
            score = Tp[col] / (double)K;
            for (int p = prev; p >= 0;) {
                const size_t rp = rp0 + (size_t)p;
                pick[rp] = col;
                if (offsets) offsets[o0 + p] = p * patch - search + col;
                if (patch_nsim) patch_nsim[o0 + p] = cand[rp * (size_t)places + col];
                const int before = link[rp];
                if (before >= 0) col = back[rp * (size_t)places + col];
                p = before;
            }
        }
        nsim[r] = score;
    }
    if (!bands) return;
    if (!live) {
        if (tid < kGammatoneBands) bands[(size_t)r * kGammatoneBands + tid] = (double)NAN;
        return;
    }
    __syncthreads();   // pick, through memory
    double* Rdb = psel_lds;
    double* Ddb = Rdb + (size_t)kGammatoneBands * patch;
    double* pr = Ddb + (size_t)kGammatoneBands * patch;
    double* pd = pr + patch;
    double* Rw = pd + patch;
    double* Dw = Rw + (size_t)kGammatoneBands * patch;
    double* Mw = Dw + (size_t)kGammatoneBands * patch;
    double* bw = Mw + (size_t)kGammatoneBands * patch;
    double sum = 0.0;
    for (int p = 0; p < P; ++p) {
        const int col = pick[rp0 + (size_t)p];
        if (col < 0) continue;   // uniform over the workgroup
        const int s = p * patch, u = s - search + col;
        patch_stage(spec_ref + ((size_t)tb.fpref[b] + (size_t)s) * kGammatoneBands, patch, Rdb, pr, tid, 256);
        patch_stage(spec_deg + ((size_t)tb.dpref[r] + (size_t)u) * kGammatoneBands, patch, Ddb, pd, tid, 256);
        __syncthreads();
        (void)patch_candidate(wave == 0, Rdb, Ddb, pr, pd, patch, C1, C3, Rw, Dw, Mw, bw, lane);
        if (tid < kGammatoneBands) sum += bw[tid];   // ascending kept patches
    }
    if (tid < kGammatoneBands) bands[(size_t)r * kGammatoneBands + tid] = sum / (double)K;
}

}  // namespace nomad
