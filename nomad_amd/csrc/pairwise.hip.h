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
template <int kD>
__global__ __launch_bounds__(256) void pairwise_tile_kernel(const float* __restrict__ deg, int Nd, const float* __restrict__ ref,
                                                            int Nr, int Drt, double* __restrict__ dist, double* __restrict__ part) {
    const int D = kD ? kD : Drt;
    __shared__ __attribute__((aligned(16))) double As[64][kPairTile];  // [k][deg row]
    __shared__ __attribute__((aligned(16))) double Bs[64][kPairTile];  // [k][ref]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int r0 = blockIdx.x * kPairTile, d0 = blockIdx.y * kPairTile;
    double acc[4][4];
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
    __syncthreads();
    double* rs = &As[0][0];  // [64 deg rows][16 tx] row sums of this tile, folded below in tx order
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
