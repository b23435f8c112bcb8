// N_deg x N_ref Euclidean distance matrix + row mean = the NOMAD score (nomad.py:108-111:
// scipy.spatial.distance.cdist on float32 embeddings promoted to float64, then np.mean(axis=1)).
//
// Computed in float64 in the DIFFERENCE form sqrt(sum_k (a_k - b_k)^2), k ascending, exactly the
// loop SciPy runs - the expansion |a|^2+|b|^2-2a.b loses ~4e-5 absolute at d~0.01 in fp32 and is
// never used (and has no exact zero on the diagonal).
//
// Bound.  Per pair: 256 subtractions + 256 fused multiply-adds in fp64 and 8 bytes written.  At config C3
// (10 000 x 1 000) that is 5.1e9 fp64 lane-operations against 80 MB: 0.13 ms at the 78.6 TFLOP/s fp64 vector
// peak, 0.016 ms at the HBM write rate - the stage is fp64-VALU bound, not write bound.
//
// pairwise_tile_kernel: workgroup = 64 deg rows x 64 refs, thread (ty, tx) of a 16 x 16 layout owns the 4 x 4 pairs
// deg 4ty.. x ref 4tx.. (32 fp64 operations per k for 8 LDS doubles read).  Both operands are converted to float64
// once, when a 64-deep k-chunk is staged into LDS as [k][row] (two ds_read_b128 per operand and k).  The grid is
// (ref tiles, deg tiles) - 2 512 workgroups at C3 instead of the 313 of a one-dimensional grid - so a deg row's sum
// over the refs is taken per 64-ref tile (refs in order inside the thread, threads folded in tx order) into
// part[ref tile][deg], and pairwise_mean_kernel adds the tiles in order: deterministic, no atomics.
#pragma once
#include <hip/hip_runtime.h>

namespace nomad {

constexpr int kPairTile = 64;

// kD: the row width at compile time (256: nomad_pairwise, the shape the comment above describes), or 0: the width is the
// argument D, a positive multiple of 4 (nomad_cdist).  The arithmetic is one chain for every width - per pair one float64
// accumulator, e = a_k - b_k, acc = fma(e, e, acc), k ascending from 0 - so nomad_cdist at D = 256 returns the bits of
// nomad_pairwise.  A last k-chunk shorter than 64 is staged with zeros on both sides: e = 0 and fma(0, 0, acc) = acc, they add
// exactly nothing.  (D is a multiple of 4, so a staged float4 lies wholly inside or wholly outside the row.)
//
// pairwise_chain is that chain, once in the source: it leaves the thread's 4 x 4 sums of squares in acc and returns the 64 KB
// LDS image, free to reuse behind a barrier.  What becomes of the sums is the kernel's epilogue: distances and per-tile row sums
// in pairwise_tile_kernel (the forwards), the backward's weights in cdist_weights_kernel.
struct PairThread {
    int tid, tx, ty, r0, d0;
};
template <int kD>
__device__ __forceinline__ double* pairwise_chain(const float* __restrict__ deg, int Nd, const float* __restrict__ ref, int Nr, int Drt,
                                                  double (&acc)[4][4], PairThread& t) {
    const int D = kD ? kD : Drt;
    __shared__ __attribute__((aligned(16))) double As[64][kPairTile];  // [k][deg row]
    __shared__ __attribute__((aligned(16))) double Bs[64][kPairTile];  // [k][ref]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int r0 = blockIdx.x * kPairTile, d0 = blockIdx.y * kPairTile;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    // staging: lane -> row tid & 63 (consecutive lanes write consecutive doubles of one LDS row: conflict-free), the four
    // waves take k columns 4 * wave + 16 q .. + 3 of the chunk
    const int srow = tid & 63, skq = (tid >> 6) * 4;
    const float* ap = deg + (long long)min(d0 + srow, Nd - 1) * D + skq;
    const float* bp = ref + (long long)min(r0 + srow, Nr - 1) * D + skq;
    for (int k0 = 0; k0 < D; k0 += 64) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kk = skq + 16 * q;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if ((kD && kD % 64 == 0) || k0 + kk < D) {
                a = *reinterpret_cast<const float4*>(ap + k0 + 16 * q);
                b = *reinterpret_cast<const float4*>(bp + k0 + 16 * q);
            }
            As[kk][srow] = (double)a.x; As[kk + 1][srow] = (double)a.y; As[kk + 2][srow] = (double)a.z; As[kk + 3][srow] = (double)a.w;
            Bs[kk][srow] = (double)b.x; Bs[kk + 1][srow] = (double)b.y; Bs[kk + 2][srow] = (double)b.z; Bs[kk + 3][srow] = (double)b.w;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < 64; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = As[k][4 * ty + i];
                b[i] = Bs[k][4 * tx + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double e = a[i] - b[j];
                    acc[i][j] = fma(e, e, acc[i][j]);
                }
        }
    }
    t = PairThread{tid, tx, ty, r0, d0};
    return &As[0][0];
}

template <int kD>
__global__ __launch_bounds__(256) void pairwise_tile_kernel(const float* __restrict__ deg, int Nd, const float* __restrict__ ref,
                                                            int Nr, int Drt, double* __restrict__ dist, double* __restrict__ part) {
    double acc[4][4];
    PairThread t;
    double* rs = pairwise_chain<kD>(deg, Nd, ref, Nr, Drt, acc, t);  // [64 deg rows][16 tx] row sums of this tile, folded below in tx order
    const int tid = t.tid, tx = t.tx, ty = t.ty, r0 = t.r0, d0 = t.d0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int d = d0 + 4 * ty + i;
        double s = 0.0;
        double4 out;
        double* o = &out.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double dv = sqrt(acc[i][j]);
            o[j] = dv;
            if (r0 + 4 * tx + j < Nr) s += dv;
        }
        if (dist && d < Nd) {
            double* dst = dist + (long long)d * Nr + r0 + 4 * tx;
            if (r0 + 4 * tx + 3 < Nr && (Nr & 1) == 0) {  // 16-byte aligned pairs
                *reinterpret_cast<double2*>(dst) = make_double2(out.x, out.y);
                *reinterpret_cast<double2*>(dst + 2) = make_double2(out.z, out.w);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (r0 + 4 * tx + j < Nr) dst[j] = o[j];
            }
        }
        rs[(4 * ty + i) * 16 + tx] = s;
    }
    __syncthreads();
    if (tid < kPairTile && d0 + tid < Nd) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) s += rs[tid * 16 + j];
        part[(long long)blockIdx.x * Nd + d0 + tid] = s;
    }
}

// mean[d] = (sum over the ref tiles, in order) / Nr.  grid: ceil(Nd / 256) blocks of 256 threads.
__global__ __launch_bounds__(256) void pairwise_mean_kernel(const double* __restrict__ part, int ntiles, int Nd, int Nr,
                                                            double* __restrict__ mean) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= Nd) return;
    double s = 0.0;
    for (int t = 0; t < ntiles; ++t) s += part[(long long)t * Nd + d];
    mean[d] = s / (double)Nr;
}

// ---- backward of the distance stage (nomad_cdist_backward) -----------------------------------------------------------------------
// With c_ij = gdist_ij + gmean_i / Nb (float64, a NULL upstream counts as 0) the gradient of sum_ij c_ij d_ij is
//   da_ik = sum_j W_ij (a_ik - b_jk),   db_jk = sum_i W_ij (b_jk - a_ik),   W_ij = c_ij / d_ij, 0 where d_ij == 0
// (torch.cdist's convention: a reference equal to the row contributes nothing, never NaN / Inf).  Two launches: the weights - the
// forward's chain with another epilogue, so d_ij has the forward's bits - into the caller's [Na][Nb] float64 scratch, then one
// reduction per requested output.
// grid (ceil(Nb / 64), ceil(Na / 64)) like pairwise_tile_kernel<0>; D: a positive multiple of 4; gdist [Na][Nb] or NULL, gmean [Na]
// or NULL, W [Na][Nb] (out).
__global__ __launch_bounds__(256) void cdist_weights_kernel(const float* __restrict__ a, int Na, const float* __restrict__ b, int Nb,
                                                            int D, const double* __restrict__ gdist, const double* __restrict__ gmean,
                                                            double* __restrict__ W) {
    double acc[4][4];
    PairThread t;
    pairwise_chain<0>(a, Na, b, Nb, D, acc, t);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int d = t.d0 + 4 * t.ty + i;
        if (d >= Na) continue;
        const double gm = gmean ? gmean[d] / (double)Nb : 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = t.r0 + 4 * t.tx + j;
            if (r >= Nb) continue;
            const long long at = (long long)d * Nb + r;
            const double c = (gdist ? gdist[at] : 0.0) + gm;
            const double dv = sqrt(acc[i][j]);
            W[at] = dv == 0.0 ? 0.0 : c / dv;
        }
    }
}

// out[r][k] = (float) sum_s fma(W(r, s), (double)x[r][k] - (double)y[s][k], acc), s ascending from 0, one float64 accumulator per
// element, rounded to fp32 once at the store.  kRowMajorW: W(r, s) = W[r * ldw + s] (da: x = a, y = b, ldw = Nb), else
// W(r, s) = W[s * ldw + r] (db: x = b, y = a, ldw = Nb).  grid (ceil(D / 64), ceil(R / 64)): a workgroup owns 64 rows x 64 columns
// k, thread (ty, tx) the 4 x 4 elements rows 4ty.. x columns 4tx.. with its 16 x values in registers as doubles.  Per 64-deep
// s-chunk W is staged as Ws[s][row] and y, converted once, as Ys[s][k]: the forward's 64 KB image and its fragment reads (two
// ds_read_b128 per operand and s: 8 LDS doubles for 16 subtractions and 16 fused multiply-adds).  Staging: lane -> tid & 63 is
// the LDS column (consecutive lanes write consecutive doubles of one LDS row: conflict-free), wave w takes the chunk's rows
// 4w + 16q .. + 3.  Whatever lies outside W, y or the row width is staged as 0: fma(0, x - 0, acc) = acc, a short last chunk adds
// exactly nothing - so an output row depends on its own x row, y and its own row of the upstreams only, whatever R is.
template <bool kRowMajorW>
__global__ __launch_bounds__(256) void cdist_reduce_kernel(const float* __restrict__ x, int R, const float* __restrict__ y, int S, int D,
                                                           const double* __restrict__ W, int ldw, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) double Ws[64][kPairTile];  // [s][row]
    __shared__ __attribute__((aligned(16))) double Ys[64][kPairTile];  // [s][k]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int k0 = blockIdx.x * kPairTile, r0 = blockIdx.y * kPairTile;
    const int kcol = k0 + 4 * tx;  // D is a multiple of 4: the thread's four columns lie inside the row together or not at all
    double xr[4][4], acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (kcol < D) v = *reinterpret_cast<const float4*>(x + (long long)min(r0 + 4 * ty + i, R - 1) * D + kcol);
        xr[i][0] = (double)v.x; xr[i][1] = (double)v.y; xr[i][2] = (double)v.z; xr[i][3] = (double)v.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    }
    const int scol = tid & 63, sq = (tid >> 6) * 4;
    for (int s0 = 0; s0 < S; s0 += 64) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ss = sq + 16 * q + u, s = s0 + ss;
                double w = 0.0, yv = 0.0;
                if (s < S) {
                    if (r0 + scol < R) w = kRowMajorW ? W[(long long)(r0 + scol) * ldw + s] : W[(long long)s * ldw + r0 + scol];
                    if (k0 + scol < D) yv = (double)y[(long long)s * D + k0 + scol];
                }
                Ws[ss][scol] = w;
                Ys[ss][scol] = yv;
            }
        __syncthreads();
#pragma unroll 8
        for (int s = 0; s < 64; ++s) {
            double w[4], yv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w[i] = Ws[s][4 * ty + i];
                yv[i] = Ys[s][4 * tx + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(w[i], xr[i][j] - yv[j], acc[i][j]);
        }
    }
    if (kcol >= D) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + 4 * ty + i;
        if (r < R)
            *reinterpret_cast<float4*>(out + (long long)r * D + kcol) =
                make_float4((float)acc[i][0], (float)acc[i][1], (float)acc[i][2], (float)acc[i][3]);
    }
}

// ---- nearest references (nomad_knn, nomad_knn_backward) --------------------------------------------------------------------------
// Per row of a the k <= 64 columns smallest under the key (d_ij, j), a NaN distance ordered as +infinity: the forward's chain with a
// selection epilogue, then a merge of the 64-column tiles in tile order.  The matrix is never formed (it is written only on request).
//
// Bound.  The chain is the forward's: 512 fp64 operations per pair at D = 256.  The selection is rank counting: an element's rank
// in its row of the tile is the number of the row's 64 keys that precede it, 64 comparisons (two compares, a select and an add each:
// ~4 lane-operations) per pair - ~256 next to the chain's 512, whatever k.  At C3 (10 000 x 1 000) that is 7.7e9 lane-operations,
// ~0.2 ms at the fp64 vector rate, against 16 x 10 000 x k candidates of 12 bytes written and read once: 15 MB at k = 8 (0.004 ms
// of HBM time), 123 MB at k = 64 (0.03 ms) - VALU bound like the forward, and at k <= 42 less memory traffic than the 80 MB matrix.
//
// knn_tile_kernel: grid and chain of pairwise_tile_kernel.  Behind the chain's last barrier the thread's 4 x 4 keys go into the LDS
// image's first half as T[row][quad ^ ty][4] (the quads of a row swizzled by the owner's ty: the four ty of a wave read four different
// quads of their rows - no bank conflict at a row stride of 512 bytes - and the 16 tx lanes of one ty read one address),
// and every thread counts, for each of its 16 elements, the keys of the element's row that precede it - (key', c') < (key, c), the
// column order decided at compile time but for the thread's own quad.  Ranks in a row are a permutation of 0 .. 63, so the elements
// of rank < k fill the row's k candidate slots exactly once: cand_d / cand_i [tile][row][k], ascending.  Columns beyond Nb (the
// chain's clones of the last row) take the key +infinity behind every real column of their tile - they are the tile's last columns -
// and leave the sentinel (inf, INT_MAX) in their slot: excluded by index, whatever their value.
constexpr int kKnnMax = 64;
constexpr int kKnnNone = 0x7fffffff;

template <int kD>
__global__ __launch_bounds__(256) void knn_tile_kernel(const float* __restrict__ a, int Na, const float* __restrict__ b, int Nb, int Drt,
                                                       int k, double* __restrict__ dist, double* __restrict__ cand_d,
                                                       int* __restrict__ cand_i) {
    double acc[4][4];
    PairThread t;
    double* T = pairwise_chain<kD>(a, Na, b, Nb, Drt, acc, t);
    const int tx = t.tx, ty = t.ty, r0 = t.r0, d0 = t.d0;
    const double inf = __builtin_inf();
    double key[4][4];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int d = d0 + 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[i][j] = sqrt(acc[i][j]);   // from here on acc is the distance, as the forwards store it
            key[i][j] = (r0 + 4 * tx + j < Nb && acc[i][j] == acc[i][j]) ? acc[i][j] : inf;
        }
        if (dist && d < Na) {
            double* dst = dist + (long long)d * Nb + r0 + 4 * tx;
            if (r0 + 4 * tx + 3 < Nb && (Nb & 1) == 0) {  // 16-byte aligned pairs
                *reinterpret_cast<double2*>(dst) = make_double2(acc[i][0], acc[i][1]);
                *reinterpret_cast<double2*>(dst + 2) = make_double2(acc[i][2], acc[i][3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (r0 + 4 * tx + j < Nb) dst[j] = acc[i][j];
            }
        }
        double* row = T + (4 * ty + i) * kPairTile + 4 * (tx ^ ty);
        *reinterpret_cast<double2*>(row) = make_double2(key[i][0], key[i][1]);
        *reinterpret_cast<double2*>(row + 2) = make_double2(key[i][2], key[i][3]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int rank[4] = {0, 0, 0, 0};
        const double* row = T + (4 * ty + i) * kPairTile;
#pragma unroll 4
        for (int q = 0; q < 16; ++q) {
            const double* quad = row + 4 * (q ^ ty);
            const double2 lo = *reinterpret_cast<const double2*>(quad), hi = *reinterpret_cast<const double2*>(quad + 2);
            const double kp[4] = {lo.x, lo.y, hi.x, hi.y};
            const bool qlt = q < tx, qle = q <= tx;   // column 4q + p precedes column 4tx + j: q < tx, or q == tx and p < j
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const bool before = p < j ? qle : qlt;
                    rank[j] += (before ? kp[p] <= key[i][j] : kp[p] < key[i][j]) ? 1 : 0;
                }
        }
        const int d = d0 + 4 * ty + i;
        if (d >= Na) continue;
        const long long slot = ((long long)blockIdx.x * Na + d) * k;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (rank[j] < k) {
                const bool real = r0 + 4 * tx + j < Nb;
                cand_d[slot + rank[j]] = real ? acc[i][j] : inf;
                cand_i[slot + rank[j]] = real ? r0 + 4 * tx + j : kKnnNone;
            }
    }
}

// (d1, i1) precedes (d2, i2) under the contract's key: NaN as +infinity, equal keys by index.
__device__ __forceinline__ bool knn_before(double d1, int i1, double d2, int i2) {
    const double k1 = d1 == d1 ? d1 : __builtin_inf(), k2 = d2 == d2 ? d2 : __builtin_inf();
    return k1 < k2 || (k1 == k2 && i1 < i2);
}
// the number of the 64 ascending entries (ld, li) that precede (d, i), or - orEqual - that do not follow it
__device__ __forceinline__ int knn_count(const double* ld, const int* li, double d, int i, bool orEqual) {
    int n = 0;
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
        const int at = n + step - 1;
        if (orEqual ? !knn_before(d, i, ld[at], li[at]) : knn_before(ld[at], li[at], d, i)) n += step;
    }
    if (orEqual ? !knn_before(d, i, ld[n], li[n]) : knn_before(ld[n], li[n], d, i)) n += 1;
    return n;
}

// knn_merge_kernel: one wave per row of a, four rows per workgroup (grid ceil(Na / 4)), lane r = slot r of the row's running best
// 64 in LDS (sentinels behind the real entries).  The tiles are merged in order, a stable two-way merge per tile: lane c holds the
// tile's candidate c (a sentinel from c = k on) and both lists are ascending, so an entry's place in the union is its own position
// plus the number of entries of the other list in front of it - a 7-step binary search -, running entries before equal candidates.
// The 128 places are distinct; those below 64 are the new running list, written to the other half of a double buffer.  Fixed order,
// no atomics: a row's result depends on its own candidates only.  Then knn_dist / knn_idx [Na][k] from slots 0 .. k - 1 and
// score_i = (sum of the k distances, r ascending, one float64 accumulator from 0.0) / (double)k by lane 0.
__global__ __launch_bounds__(256) void knn_merge_kernel(const double* __restrict__ cand_d, const int* __restrict__ cand_i, int ntiles,
                                                        int Na, int k, double* __restrict__ knn_dist, int* __restrict__ knn_idx,
                                                        double* __restrict__ score) {
    __shared__ double run_d[2][4][kKnnMax];
    __shared__ int run_i[2][4][kKnnMax];
    __shared__ double new_d[4][kKnnMax];
    __shared__ int new_i[4][kKnnMax];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row = min(blockIdx.x * 4 + w, Na - 1);   // a wave behind the last row repeats it and stores nothing: barriers stay uniform
    const bool live = blockIdx.x * 4 + w < Na;
    run_d[0][w][lane] = __builtin_inf();
    run_i[0][w][lane] = kKnnNone;
    int cur = 0;
    double next_d = __builtin_inf();
    int next_i = kKnnNone;
    if (lane < k) {
        next_d = cand_d[(long long)row * k + lane];
        next_i = cand_i[(long long)row * k + lane];
    }
    for (int tile = 0; tile < ntiles; ++tile) {
        const double cd = next_d;
        const int ci = next_i;
        if (tile + 1 < ntiles && lane < k) {   // the next tile's candidates are on their way while this tile is merged
            const long long slot = ((long long)(tile + 1) * Na + row) * k;
            next_d = cand_d[slot + lane];
            next_i = cand_i[slot + lane];
        }
        new_d[w][lane] = cd;
        new_i[w][lane] = ci;
        __syncthreads();
        const double rd = run_d[cur][w][lane];
        const int ri = run_i[cur][w][lane];
        const int rpos = lane + knn_count(new_d[w], new_i[w], rd, ri, false);
        const int cpos = lane + knn_count(run_d[cur][w], run_i[cur][w], cd, ci, true);
        if (rpos < kKnnMax) {
            run_d[cur ^ 1][w][rpos] = rd;
            run_i[cur ^ 1][w][rpos] = ri;
        }
        if (cpos < kKnnMax) {
            run_d[cur ^ 1][w][cpos] = cd;
            run_i[cur ^ 1][w][cpos] = ci;
        }
        cur ^= 1;
        __syncthreads();
    }
    if (!live) return;
    if (lane < k) {
        knn_dist[(long long)row * k + lane] = run_d[cur][w][lane];
        knn_idx[(long long)row * k + lane] = run_i[cur][w][lane];
    }
    if (lane == 0) {
        double s = 0.0;
        for (int r = 0; r < k; ++r) s += run_d[cur][w][r];
        score[row] = s / (double)k;
    }
}

// The dense upstream of nomad_knn_backward in the caller's scratch: row i of G [Na][Nb] is zero but for
// G[i][knn_idx[i][r]] = g_knn[i][r] + g_score[i] / k (a NULL upstream counts as 0); an index outside 0 .. Nb - 1 is skipped.
// grid: Na workgroups of 256 threads, one per row - zero, barrier, scatter (the indices of a row are distinct: no collisions).
__global__ __launch_bounds__(256) void knn_scatter_kernel(const int* __restrict__ knn_idx, const double* __restrict__ g_knn,
                                                          const double* __restrict__ g_score, int Nb, int k, double* __restrict__ G) {
    const long long i = blockIdx.x;
    double* g = G + i * Nb;
    for (int j = threadIdx.x; j < Nb; j += 256) g[j] = 0.0;
    __syncthreads();
    if (threadIdx.x < k) {
        const int j = knn_idx[i * k + threadIdx.x];
        if (j >= 0 && j < Nb) g[j] = (g_knn ? g_knn[i * k + threadIdx.x] : 0.0) + (g_score ? g_score[i] / (double)k : 0.0);
    }
}

// paired_distance_kernel: out[i] = ||a_i - b_i||, the chain of pairwise_tile_kernel for the pair (i, i) - bit-identical to the
// diagonal of the matrix, without the other N - 1 columns (10 000 pairs: 8 x 10^4 bytes written instead of 8 x 10^8).
// grid: ceil(N / 64) workgroups of 256 threads, one per 64 pairs.  A 64-deep k-chunk of both operands is staged through LDS as
// fp32 [k][row]: in a wave 16 lanes read 256 contiguous bytes of each of 4 rows (a thread walking its own row would read 4
// bytes of 64 different cache lines per instruction), and the rows are 65 floats apart, so the staging writes (lane (row r,
// quad q) -> bank 4q + r + j) and the reads of the chain (lane = row) both touch 64 different banks.  Wave 0 then runs the 64
// chains, one pair per lane; the other three waves only stage (a chain is sequential by contract: the kernel is bound by the
// latency of D dependent fp64 fused multiply-adds, ~10 us at D = 768, whatever N up to one workgroup per CU).
constexpr int kPairedLd = kPairTile + 1;
__global__ __launch_bounds__(256) void paired_distance_kernel(const float* __restrict__ a, const float* __restrict__ b, int N,
                                                              int D, double* __restrict__ out) {
    __shared__ float As[64][kPairedLd];  // [k][pair]
    __shared__ float Bs[64][kPairedLd];
    const int tid = threadIdx.x, kq = (tid & 15) * 4, rr = tid >> 4;
    const int p0 = blockIdx.x * kPairTile;
    double acc = 0.0;
    for (int k0 = 0; k0 < D; k0 += 64) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = rr + 16 * q;
            const long long row = min(p0 + r, N - 1);
            float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
            if (k0 + kq < D) {
                va = *reinterpret_cast<const float4*>(a + row * D + k0 + kq);
                vb = *reinterpret_cast<const float4*>(b + row * D + k0 + kq);
            }
            As[kq][r] = va.x; As[kq + 1][r] = va.y; As[kq + 2][r] = va.z; As[kq + 3][r] = va.w;
            Bs[kq][r] = vb.x; Bs[kq + 1][r] = vb.y; Bs[kq + 2][r] = vb.z; Bs[kq + 3][r] = vb.w;
        }
        __syncthreads();
        if (tid < kPairTile) {
#pragma unroll 8
            for (int k = 0; k < 64; ++k) {
                const double e = (double)As[k][tid] - (double)Bs[k][tid];
                acc = fma(e, e, acc);
            }
        }
    }
    if (tid < kPairTile && p0 + tid < N) out[p0 + tid] = sqrt(acc);
}

}  // namespace nomad
