// fp32 pos-conv in the frequency domain: 512-point transforms around one small complex product per bin.
//
// One group of the positional convolution is the 128-tap stride-1 correlation C[t] = sum_k A[t + k] V[k] (A: the zero-padded
// input frames of a clip, 48 channels; V[k]: the 48 x 48 tap matrix).  Overlap-save with N = kPfN = 512: a UNIT is one (clip,
// block of kPfBlk = 385 output frames); block j reads padded frames 385 j .. 385 j + 511 of the clip (frames behind T_c + 128
// stand for zeros) and, as t + k <= 511 for t < 385, the circular correlation of length 512 equals the linear one there:
//     C[t] = IDFT( DFT(A)[f] . conj(DFT(V)[f]) )[t],   t = 0 .. 384.
// Per bin f = 0 .. 256 (the inputs are real: the other bins are conjugates) that is one [units x 48] . [48 x 48] complex product,
// run in real arithmetic on the matrix cores with the embedding [[Wr, -Wi], [Wi, Wr]], W = conj(DFT(V)) / 512:
//     posconv_fft_forward_kernel  xpad [16][frames][48]              -> X [16][257][units][96]
//     posconv_fft_bins_kernel     X x Wf [16][257][96][96]           -> Y [16][257][units][96]
//     posconv_fft_inverse_kernel  Y -> IDFT, first min(385, rest) frames, + bias, (Upre), GELU, + residual -> y [sum_c T_c][768]
// N is 512 for every clip and the products' contraction order is fixed, so a clip's values depend on the clip alone.
//
// The 96 columns of a row of X / Y: two real channels are packed into one complex transform, and a workgroup of the transform
// kernels owns 16 channels (8 transforms, 32 KB of LDS).  Column = chunk * 32 + part * 16 + i for channel chunk * 16 + i, part 0
// the real and 1 the imaginary component: a workgroup's 32 values of a bin are 128 contiguous bytes.  The weight transform lays
// the rows and columns of Wf out the same way; a bin product does not care in which order it contracts.
//
// Transform: in-place radix-8 decimation in frequency, three stages; bin k ends at position pf_rev(k) (octal digits reversed).
// The inverse is the same transform read at index (512 - t) mod 512; its 1 / 512 is in the weights (a power of two: exact).
#pragma once
#include "gemm_f32.hip.h"

namespace nomad {

constexpr int kPfN = 512;              // transform length
constexpr int kPfBlk = kPfN - 127;     // output frames per unit: 385
constexpr int kPfBins = kPfN / 2 + 1;  // 257
constexpr int kPfCols = 96;            // real + imaginary parts of a group's 48 channels

// Where the clips of a batch sit.  Uniform batch (tpref == nullptr): B clips of T frames.  Ragged: prefix sums (device) of the
// clips' frames (tpref), padded frames (ppref) and units (upref: ceil(T_c / 385) each, from posconv_fft_prefix_kernel).
struct PosFftGeom {
    int B, T;
    const int *tpref, *ppref, *upref;
    long long pad_rows;   // padded frames of one group of xpad
    int units;            // sum_c ceil(T_c / 385)
    int max_blocks;       // the longest clip's units
};

__host__ __device__ constexpr int pos_fft_blocks(int T) { return (T + kPfBlk - 1) / kPfBlk; }
inline size_t pos_fft_spec_bytes(long long units) { return sizeof(float) * 16 * kPfBins * kPfCols * (size_t)units; }   // X or Y
constexpr size_t kPfWeightFloats = (size_t)16 * kPfBins * kPfCols * kPfCols;

// A ragged batch's unit prefix sums from its frame prefix sums: umeta[0 .. B].  One workgroup; B is a batch size.
__global__ __launch_bounds__(64) void posconv_fft_prefix_kernel(const int* __restrict__ tpref, int B, int* __restrict__ umeta) {
    if (threadIdx.x != 0) return;
    int units = 0;
    for (int b = 0; b < B; ++b) {
        umeta[b] = units;
        units += pos_fft_blocks(tpref[b + 1] - tpref[b]);
    }
    umeta[B] = units;
}

struct PosFftClip {
    int T;            // frames
    long long pad0;   // first padded frame in a group of xpad
    long long row0;   // first output row (of [sum T][768])
    int unit0;        // first unit
};

__device__ __forceinline__ PosFftClip pos_fft_clip(const PosFftGeom& g, int b) {
    PosFftClip c;
    if (g.tpref) {
        c.T = g.tpref[b + 1] - g.tpref[b];
        c.pad0 = g.ppref[b];
        c.row0 = g.tpref[b];
        c.unit0 = g.upref[b];
    } else {
        c.T = g.T;
        c.pad0 = (long long)b * (g.T + 128);
        c.row0 = (long long)b * g.T;
        c.unit0 = b * pos_fft_blocks(g.T);
    }
    return c;
}

// exp(-2 pi i m / 512), m = 0 .. 511, in float64: the transforms read it rounded to fp32, the weight transform as it is
__global__ __launch_bounds__(256) void posconv_fft_twiddle_kernel(double2* __restrict__ tw64, float2* __restrict__ tw32) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= kPfN) return;
    double s, c;
    sincospi(-(double)m / (kPfN / 2), &s, &c);
    tw64[m] = make_double2(c, s);
    tw32[m] = make_float2((float)c, (float)s);
}

// Weight transform, once per weight version: pos_w [16][64][6144] (k = tap * 48 + ci, rows 48 .. 63 zero) -> wf [16][257][96][96]
// ([output column][input column], both in the layout above).  W[f] = conj(DFT(V)[f]) / 512 = sum_k V[k] exp(+2 pi i f k / 512) / 512
// per (n, ci), summed in float64 and rounded once; rows of the real embedding: Yre = Xre Wr - Xim Wi, Yim = Xre Wi + Xim Wr.
// grid: (257, 16), 256 threads.
__global__ __launch_bounds__(256) void posconv_fft_weight_kernel(const float* __restrict__ pos_w, const double2* __restrict__ tw64,
                                                                 float* __restrict__ wf) {
    __shared__ double2 tw[kPfN];
    const int f = blockIdx.x, g = blockIdx.y;
    for (int m = threadIdx.x; m < kPfN; m += 256) tw[m] = tw64[m];
    __syncthreads();
    float* o = wf + ((long long)g * kPfBins + f) * kPfCols * kPfCols;
    for (int e = threadIdx.x; e < 48 * 48; e += 256) {
        const int n = e / 48, ci = e - n * 48;
        const float* w = pos_w + ((long long)g * 64 + n) * 6144 + ci;
        double wr = 0.0, wi = 0.0;
        for (int k = 0; k < 128; ++k) {
            const double v = (double)w[k * 48];
            const double2 t = tw[(f * k) & (kPfN - 1)];   // exp(-2 pi i f k / 512): conjugate it
            wr += v * t.x;
            wi -= v * t.y;
        }
        wr *= 1.0 / kPfN;
        wi *= 1.0 / kPfN;
        const int nre = (n >> 4) * 32 + (n & 15), cre = (ci >> 4) * 32 + (ci & 15);
        o[nre * kPfCols + cre] = (float)wr;
        o[nre * kPfCols + cre + 16] = (float)-wi;
        o[(nre + 16) * kPfCols + cre] = (float)wi;
        o[(nre + 16) * kPfCols + cre + 16] = (float)wr;
    }
}

// position of bin k after the in-place transform (and of input k for a transform that is to come out in natural order)
__host__ __device__ __forceinline__ int pf_rev(int k) { return ((k & 7) << 6) | (k & 0x38) | (k >> 6); }

struct pf_cpx {
    float x, y;
};
__host__ __device__ __forceinline__ pf_cpx pf_add(pf_cpx a, pf_cpx b) { return {a.x + b.x, a.y + b.y}; }
__host__ __device__ __forceinline__ pf_cpx pf_sub(pf_cpx a, pf_cpx b) { return {a.x - b.x, a.y - b.y}; }
__host__ __device__ __forceinline__ pf_cpx pf_mul(pf_cpx a, pf_cpx b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__host__ __device__ __forceinline__ pf_cpx pf_mul_mi(pf_cpx a) { return {a.y, -a.x}; }   // a * (-i)

// 8-point DFT in registers, v[m] = sum_r v[r] exp(-2 pi i r m / 8), natural order in and out
__host__ __device__ __forceinline__ void pf_dft8(pf_cpx (&v)[8]) {
    constexpr float h = 0.70710678118654752440f;
    pf_cpx a[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a[i] = pf_add(v[i], v[i + 4]);
        a[i + 4] = pf_sub(v[i], v[i + 4]);
    }
    a[5] = {h * (a[5].x + a[5].y), h * (a[5].y - a[5].x)};     // * exp(-i pi / 4)
    a[6] = pf_mul_mi(a[6]);
    a[7] = {h * (a[7].y - a[7].x), -h * (a[7].x + a[7].y)};    // * exp(-3 i pi / 4)
    pf_cpx b[8];
#pragma unroll
    for (int q = 0; q < 8; q += 4) {
        b[q] = pf_add(a[q], a[q + 2]);
        b[q + 1] = pf_add(a[q + 1], a[q + 3]);
        b[q + 2] = pf_sub(a[q], a[q + 2]);
        b[q + 3] = pf_mul_mi(pf_sub(a[q + 1], a[q + 3]));
    }
    v[0] = pf_add(b[0], b[1]);
    v[4] = pf_sub(b[0], b[1]);
    v[2] = pf_add(b[2], b[3]);
    v[6] = pf_sub(b[2], b[3]);
    v[1] = pf_add(b[4], b[5]);
    v[5] = pf_sub(b[4], b[5]);
    v[3] = pf_add(b[6], b[7]);
    v[7] = pf_sub(b[6], b[7]);
}

// One radix-8 butterfly of stage `stage` (0 .. 2) of the in-place 512-point transform: butterfly `bf` (0 .. 63) of the transform
// whose element p sits at buf[p * stride].  tw: exp(-2 pi i m / 512).
template <typename Buf, typename Tw>
__host__ __device__ __forceinline__ void pf_butterfly(Buf buf, int stride, int stage, int bf, Tw tw) {
    const int span = kPfN >> (3 * stage), step = span >> 3;   // the sub-transform's length, the distance of a butterfly's inputs
    const int blk = bf / step, j = bf - blk * step;
    const int base = blk * span + j;
    pf_cpx v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = buf[(base + r * step) * stride];
    pf_dft8(v);
    const int tstep = j * (kPfN / span);   // output m takes exp(-2 pi i j m / span)
#pragma unroll
    for (int m = 1; m < 8; ++m)
        if (stage < 2) v[m] = pf_mul(v[m], tw[tstep * m]);
#pragma unroll
    for (int m = 0; m < 8; ++m) buf[(base + m * step) * stride] = v[m];
}

// The 8 transforms of a workgroup, in place in LDS: buf [512][8] (transform minor), 256 threads.  Barriers in front and behind.
__device__ __forceinline__ void pf_transform8(pf_cpx* buf, const pf_cpx* tw) {
    const int p = threadIdx.x & 7, b0 = threadIdx.x >> 3;
#pragma unroll
    for (int stage = 0; stage < 3; ++stage) {
        __syncthreads();
        pf_butterfly(buf + p, 8, stage, b0, tw);
        pf_butterfly(buf + p, 8, stage, b0 + 32, tw);
    }
    __syncthreads();
}

// Forward transform.  grid: (3 * max_blocks, 16 * B), 256 threads; a workgroup owns (unit, group, 16 channels).
__global__ __launch_bounds__(256) void posconv_fft_forward_kernel(const float* __restrict__ xpad, const float2* __restrict__ tw32,
                                                                  float* __restrict__ X, const PosFftGeom geo) {
    __shared__ __attribute__((aligned(16))) pf_cpx buf[kPfN * 8];
    __shared__ pf_cpx tw[kPfN];
    const int g = blockIdx.y / geo.B, b = blockIdx.y - g * geo.B;
    const int j = blockIdx.x / 3, chunk = blockIdx.x - j * 3;
    const PosFftClip c = pos_fft_clip(geo, b);
    if (j >= pos_fft_blocks(c.T)) return;
    const int tid = threadIdx.x;
    for (int m = tid; m < kPfN; m += 256) tw[m] = {tw32[m].x, tw32[m].y};
    // frames 385 j .. 385 j + 511 of the clip, channels 16 chunk .. + 15: channel pair (2 p, 2 p + 1) is transform p
    const int nf = c.T + 128 - kPfBlk * j;   // frames of the clip from this unit's first on (the rest stand for zeros)
    const float* src = xpad + ((long long)g * geo.pad_rows + c.pad0 + (long long)kPfBlk * j) * 48 + chunk * 16;
    f32x4* b4 = reinterpret_cast<f32x4*>(buf);
    for (int e = tid; e < kPfN * 4; e += 256) {
        const int f = e >> 2, q = e & 3;
        b4[e] = f < nf ? *reinterpret_cast<const f32x4*>(src + (long long)f * 48 + q * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    pf_transform8(buf, tw);
    // the two channels' spectra from the packed one: A[k] = (Z[k] + conj Z[N - k]) / 2, B[k] = (Z[k] - conj Z[N - k]) / 2i
    const int p = tid & 7;
    float* dst = X + ((long long)g * kPfBins * geo.units + c.unit0 + j) * kPfCols + chunk * 32 + 2 * p;
    for (int k = tid >> 3; k < kPfBins; k += 32) {
        const pf_cpx z = buf[pf_rev(k) * 8 + p], zn = buf[pf_rev((kPfN - k) & (kPfN - 1)) * 8 + p];
        float* o = dst + (long long)k * geo.units * kPfCols;
        *reinterpret_cast<float2*>(o) = make_float2(0.5f * (z.x + zn.x), 0.5f * (z.y + zn.y));          // re: channels 2 p, 2 p + 1
        *reinterpret_cast<float2*>(o + 16) = make_float2(0.5f * (z.y - zn.y), 0.5f * (zn.x - z.x));     // im
    }
}

// Bin products: Y[g][f] = X[g][f] [units x 96] . Wf[g][f]^T.  grid: (257, 16), 256 threads.  A wave keeps the whole 96 x 96
// weight matrix in registers as MFMA operands and walks over tiles of 16 units; the product is computed transposed (weights as
// the row operand) so that a lane ends with four consecutive columns of one unit: 16-byte stores.  Lane (i = l & 15, q = l >> 4)
// loads columns 16 s + 4 q .. + 3 of row i, and MFMA (s, e) contracts columns {16 s + 4 q' + e}: the same order for every tile.
__global__ __launch_bounds__(256) void posconv_fft_bins_kernel(const float* __restrict__ X, const float* __restrict__ wf,
                                                               float* __restrict__ Y, int units) {
    const int f = blockIdx.x, g = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const long long mat = (long long)g * kPfBins + f;
    const float* w = wf + mat * kPfCols * kPfCols + i * kPfCols + q * 4;
    f32x4 wr[6][6];   // [output tile][k step]
#pragma unroll
    for (int nt = 0; nt < 6; ++nt)
#pragma unroll
        for (int s = 0; s < 6; ++s) wr[nt][s] = *reinterpret_cast<const f32x4*>(w + nt * 16 * kPfCols + s * 16);
    const float* x = X + mat * units * kPfCols + q * 4;
    float* y = Y + mat * units * kPfCols + q * 4;
    for (int m0 = wave * 16; m0 < units; m0 += 64) {
        const int m = m0 + i;
        f32x4 xa[6];
#pragma unroll
        for (int s = 0; s < 6; ++s)
            xa[s] = m < units ? *reinterpret_cast<const f32x4*>(x + (long long)m * kPfCols + s * 16) : (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 acc[6];
#pragma unroll
        for (int nt = 0; nt < 6; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 6; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int nt = 0; nt < 6; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[nt][s][e], xa[s][e], acc[nt], 0, 0, 0);
        // D[row = 4 q + r][col = i]: unit m, output columns 16 nt + 4 q .. + 3
        if (m < units) {
#pragma unroll
            for (int nt = 0; nt < 6; ++nt) *reinterpret_cast<f32x4*>(y + (long long)m * kPfCols + nt * 16) = acc[nt];
        }
    }
}

// Inverse transform and the pos-conv's epilogue: + bias, the optional pre-activation store, GELU and the residual from xpad, in
// the order of the other two forms.  y / upre: [sum T][768].  grid: (3 * max_blocks, 16 * B), 256 threads.
__global__ __launch_bounds__(256) void posconv_fft_inverse_kernel(const float* __restrict__ Y, const float2* __restrict__ tw32,
                                                                  const float* __restrict__ bias, const float* __restrict__ xpad,
                                                                  float* __restrict__ y, float* __restrict__ upre, const PosFftGeom geo) {
    __shared__ __attribute__((aligned(16))) pf_cpx buf[kPfN * 8];
    __shared__ pf_cpx tw[kPfN];
    const int g = blockIdx.y / geo.B, b = blockIdx.y - g * geo.B;
    const int j = blockIdx.x / 3, chunk = blockIdx.x - j * 3;
    const PosFftClip c = pos_fft_clip(geo, b);
    if (j >= pos_fft_blocks(c.T)) return;
    const int tid = threadIdx.x;
    for (int m = tid; m < kPfN; m += 256) tw[m] = {tw32[m].x, tw32[m].y};
    // the packed spectrum Z = A + i B of the channel pair from the two real channels' half spectra (the other half: conjugates)
    const int p = tid & 7;
    const float* src = Y + ((long long)g * kPfBins * geo.units + c.unit0 + j) * kPfCols + chunk * 32 + 2 * p;
    for (int k = tid >> 3; k < kPfBins; k += 32) {
        const float* in = src + (long long)k * geo.units * kPfCols;
        const float2 re = *reinterpret_cast<const float2*>(in), im = *reinterpret_cast<const float2*>(in + 16);
        buf[k * 8 + p] = {re.x - im.y, im.x + re.y};
        if (k != 0 && k != kPfN / 2) buf[(kPfN - k) * 8 + p] = {re.x + im.y, re.y - im.x};
    }
    pf_transform8(buf, tw);
    // output frame t = DFT(Z)[(512 - t) mod 512] (the 1 / 512 is in the weights): channels 16 chunk + 4 q .. + 3 of frame t
    const int nt = min(kPfBlk, c.T - kPfBlk * j);
    const int col = g * 48 + chunk * 16;
    const float* res = xpad + ((long long)g * geo.pad_rows + c.pad0 + (long long)kPfBlk * j + 64) * 48 + chunk * 16;
    const f32x4* b4 = reinterpret_cast<const f32x4*>(buf);
    for (int e = tid; e < nt * 4; e += 256) {
        const int t = e >> 2, q = e & 3;
        f32x4 val = b4[pf_rev((kPfN - t) & (kPfN - 1)) * 4 + q];
        if (bias) val += *reinterpret_cast<const f32x4*>(bias + col + q * 4);
        const long long idx = (c.row0 + (long long)kPfBlk * j + t) * 768 + col + q * 4;
        if (upre) *reinterpret_cast<f32x4*>(upre + idx) = val;
#pragma unroll
        for (int k = 0; k < 4; ++k) val[k] = gelu_erf(val[k]);
        val += *reinterpret_cast<const f32x4*>(res + (long long)t * 48 + q * 4);
        *reinterpret_cast<f32x4*>(y + idx) = val;
    }
}

}  // namespace nomad
