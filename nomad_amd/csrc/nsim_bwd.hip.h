// The whole-clip NSIM as a loss: the backward of nomad_nsim down to the degraded spectrogram and of nomad_gammatone down to the
// samples.  include/nomad_hip.h ("NSIM as a loss") states the gradient conventions and every order; this file follows it.
//
// gammatone_adjoint_kernel - the hot path, gammatone_frames_kernel's lane mapping and LDS staging (a lane per (frame, band), 3 x 21
// lanes a wave, 12 frames a workgroup, the span staged as fp32 rows of H + 1 floats: the same bytes of LDS, so the 48 kHz budget of
// 57 660 bytes holds unchanged).  S = sqrt(sum y^2 / W) gives q[n] = dS y[n] / (S W), and a section from the zero state is a lower
// triangular Toeplitz map whose transpose is the same section over the time-reversed sequence, so the frame's gradient is
// rev(sec0(sec1(sec2(sec3(rev(q)))))).  q is needed last sample first and the recurrence cannot be run backwards in time (it grows
// by 1 / a2 per step), so y is STORED: pass 1 runs the forward cascade and writes y[n] to the workspace as [frame][n][21] float64
// (the 21 lanes of a frame write 168 contiguous bytes per step) and keeps S; pass 2, in the same lane, reads y[n] from n = W - 1
// down, runs the sections in the order 3, 2, 1, 0 from the zero state and writes each result over the y it has consumed three
// steps before (a lane reads back only what it wrote itself, so no barrier or second launch stands between the passes).  Both
// passes are skewed as the forward is; their fill and drain steps run every section on zeros, which from the zero state put out
// zeros, so they need no code of their own.  Pass 2 loads four steps ahead of the one it computes.
// The store is F 21 W 8 bytes: 215 KB per frame at 16 kHz, 10.7 MB per second of audio and row.  A variant with state checkpoints
// would save memory at the price of a third cascade pass; Engine bounds the workspace by grouping rows instead.
//
// gammatone_gather_kernel - one thread per sample: the up to four frames that cover it in ascending order, each frame's 21 band
// values (contiguous) added in ascending order into the frame's sum, the frames' sums added in ascending order, rounded to fp32
// once.  No atomics.  Samples behind the whole frames, up to the stride, are written as 0.
//
// nsim_backward_kernel - one workgroup per degraded row, like nsim_kernel, whose phases it repeats with nsim.hip.h's own device
// functions so that every comparison sees the forward's bits; then the map partials per cell (five planes: d / d mu_R, mu_D,
// w*R^2, w*D^2, w*RD), the window's adjoint as a gather (no atomics), least, the per-frame floors and dB -> dS.
#pragma once
#include <hip/hip_runtime.h>

#include "nsim.hip.h"

namespace nomad {

constexpr int kNsimBwdPlanes = 9;   // R, D, five partials, dR, dD: [G total][21] float64 each

// Grid (ceil(max F / 12), R), 256 threads, dynamic LDS as gammatone_frames_kernel.  Y: [sum F][W][21] float64; on return slot
// [fpref[r] + t][n][band] holds d (sum dspec S) / d x[t H + n] through that frame and band alone.
__global__ __launch_bounds__(256) void gammatone_adjoint_kernel(const float* __restrict__ x, int stride, const int* __restrict__ lens,
                                                                const long long* __restrict__ fpref, const double* __restrict__ coef, int H,
                                                                const double* __restrict__ dspec, double* Y) {
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
    const size_t cell = (size_t)fpref[r] + (size_t)(t0 + f);
    double* yl = Y + cell * (size_t)W * kGammatoneBands + band;   // slot n: yl[n * 21]
    double z10 = 0.0, z20 = 0.0, z11 = 0.0, z21 = 0.0, z12 = 0.0, z22 = 0.0, z13 = 0.0, z23 = 0.0;
    double y0 = 0.0, y1 = 0.0, y2 = 0.0, acc = 0.0;
    float chk = 0.0f;   // 0 * x summed: NaN once a sample is not finite
    const float* p = gt_span + f * (H + 1);
    // ---- pass 1: the cascade of the forward, its outputs stored.  At step i section j works on sample i - j.
    for (int q = 0; q < 4; ++q) {
        const float* pq = p + q * (H + 1);
        for (int i = 0; i < H; ++i) {
            const float v = pq[i];
            chk = fmaf(0.0f, v, chk);
            const double y3 = gammatone_section(b03, b13, a1, a2, y2, z13, z23);
            y2 = gammatone_section(b02, b12, a1, a2, y1, z12, z22);
            y1 = gammatone_section(b01, b11, a1, a2, y0, z11, z21);
            y0 = gammatone_section(b00, b10, a1, a2, (double)v, z10, z20);
            const int s = q * H + i - 3;
            if (s >= 0) {
                yl[(size_t)s * kGammatoneBands] = y3;
                acc += y3 * y3;
            }
        }
    }
    for (int s = W - 3; s < W; ++s) {   // the pipe drains; what section 0 makes of the zeros reaches no sample below W
        const double y3 = gammatone_section(b03, b13, a1, a2, y2, z13, z23);
        y2 = gammatone_section(b02, b12, a1, a2, y1, z12, z22);
        y1 = gammatone_section(b01, b11, a1, a2, y0, z11, z21);
        y0 = gammatone_section(b00, b10, a1, a2, 0.0, z10, z20);
        yl[(size_t)s * kGammatoneBands] = y3;
        acc += y3 * y3;
    }
    const double S = chk != chk ? (double)NAN : sqrt(acc / (double)W);
    const double dS = dspec[cell * kGammatoneBands + band];
    // sqrt has gradient 0 at 0; a NaN from above stays a NaN
    const double c = (acc == 0.0 && chk == chk) ? (dS != dS ? (double)NAN : 0.0) : dS / (S * (double)W);
    // ---- pass 2: sections 3, 2, 1, 0 over q[n] = c y[n], n from W - 1 down; step i reads slot W - 1 - i and writes slot W + 2 - i.
    z10 = z20 = z11 = z21 = z12 = z22 = z13 = z23 = 0.0;
    y0 = y1 = y2 = 0.0;
    double nxt0 = yl[(size_t)(W - 1) * kGammatoneBands], nxt1 = yl[(size_t)(W - 2) * kGammatoneBands],
           nxt2 = yl[(size_t)(W - 3) * kGammatoneBands], nxt3 = yl[(size_t)(W - 4) * kGammatoneBands];
    for (int i = 0; i < W; i += 4) {
        const double cur[4] = {nxt0, nxt1, nxt2, nxt3};
        if (i + 4 < W) {   // the next four, ahead of the stores below (their slots lie above these)
            nxt0 = yl[(size_t)(W - 5 - i) * kGammatoneBands];
            nxt1 = yl[(size_t)(W - 6 - i) * kGammatoneBands];
            nxt2 = yl[(size_t)(W - 7 - i) * kGammatoneBands];
            nxt3 = yl[(size_t)(W - 8 - i) * kGammatoneBands];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double o = gammatone_section(b00, b10, a1, a2, y2, z10, z20);
            y2 = gammatone_section(b01, b11, a1, a2, y1, z11, z21);
            y1 = gammatone_section(b02, b12, a1, a2, y0, z12, z22);
            y0 = gammatone_section(b03, b13, a1, a2, c * cur[u], z13, z23);
            const int s = W + 2 - i - u;
            if (s < W) yl[(size_t)s * kGammatoneBands] = o;
        }
    }
    for (int s = 2; s >= 0; --s) {
        const double o = gammatone_section(b00, b10, a1, a2, y2, z10, z20);
        y2 = gammatone_section(b01, b11, a1, a2, y1, z11, z21);
        y1 = gammatone_section(b02, b12, a1, a2, y0, z12, z22);
        y0 = gammatone_section(b03, b13, a1, a2, 0.0, z13, z23);
        yl[(size_t)s * kGammatoneBands] = o;
    }
}

// Grid (ceil(stride / 256), R), 256 threads.  dx[r][s] for every s < stride.
__global__ __launch_bounds__(256) void gammatone_gather_kernel(const double* __restrict__ Y, int stride, const int* __restrict__ lens,
                                                               const long long* __restrict__ fpref, int H, float* __restrict__ dx) {
    const int r = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    if (s >= stride) return;
    const int W = 4 * H, n = lens[r];
    const int F = (n - W) / H + 1;
    double acc = 0.0;
    if (s < (F - 1) * H + W) {
        const int lo = s < W ? 0 : (s - W) / H + 1, top = s / H, hi = top < F - 1 ? top : F - 1;
        for (int t = lo; t <= hi; ++t) {
            const double* v = Y + (((size_t)fpref[r] + (size_t)t) * (size_t)W + (size_t)(s - t * H)) * kGammatoneBands;
            double fsum = 0.0;
            for (int b = 0; b < kGammatoneBands; ++b) fsum += v[b];
            acc += fsum;
        }
    }
    dx[(size_t)r * (size_t)stride + (size_t)s] = (float)acc;
}

// ---- NSIM backward ----
// dB of a spectrogram value and whether a gradient passes through both of its floors (value > floor strictly).
__device__ __forceinline__ bool nsim_db_passes(double s) {
    const double eps = 2.220446049250313e-16;
    return s > eps && 10.0 * log10(s) > -45.0;
}

// The five partials of gm * map(t, band): with respect to mu_R, mu_D, w*R^2, w*D^2 and w*(R D).
__device__ __forceinline__ void nsim_cell_partials(const double* __restrict__ R, const double* __restrict__ D, int F, int t, int band, double C1,
                                                   double C3, double gm, double& gmr, double& gmd, double& grr, double& gdd, double& grd) {
    double mr, md, rr, dd, rd;
    nsim_window(R, D, F, t, band, mr, md, rr, dd, rd);
    const double vr = rr - mr * mr, vd = dd - md * md;
    const bool pr = vr > 0.0, pd = vd > 0.0;   // sigma = sqrt(var) has gradient 0 where var <= 0
    const double sr = pr ? sqrt(vr) : 0.0, sd = pd ? sqrt(vd) : 0.0;
    const double cov = rd - mr * md;
    const double Dl = mr * mr + md * md + C1, l = (2.0 * mr * md + C1) / Dl;
    const double Ds = sr * sd + C3, s = (cov + C3) / Ds;
    const double gl = gm * s, gs = gm * l;
    const double gsig = -(gs * s) / Ds;   // with respect to the product sigma_R sigma_D
    grd = gs / Ds;
    grr = pr ? gsig * sd / (2.0 * sr) : 0.0;
    gdd = pd ? gsig * sr / (2.0 * sd) : 0.0;
    gmr = gl * (2.0 * md - 2.0 * l * mr) / Dl - grd * md - 2.0 * grr * mr;
    gmd = gl * (2.0 * mr - 2.0 * l * md) / Dl - grd * mr - 2.0 * gdd * md;
}

// Grid B G, 256 threads.  Row j = b G + g as nsim_kernel; planes: [9][G total][21] float64 at the row's own offset;
// dspec[G fpref[b] + g F_b ..][21] <- grad[j] d nsim[j] / d spec_deg.
__global__ __launch_bounds__(256) void nsim_backward_kernel(const double* __restrict__ spec_ref, const double* __restrict__ spec_deg, int G,
                                                            const int* __restrict__ frames, const long long* __restrict__ fpref, long long total,
                                                            double C1, double C3, const double* __restrict__ grad, double* planes,
                                                            double* __restrict__ dspec) {
    __shared__ double red[256];
    __shared__ long long key[256];
    __shared__ int bad[256];
    const int j = blockIdx.x, b = j / G, g = j % G, tid = threadIdx.x;
    const int F = frames[b];
    const size_t at = (size_t)G * (size_t)fpref[b] + (size_t)g * (size_t)F, plane = (size_t)G * (size_t)total * kGammatoneBands;
    const double* sr = spec_ref + (size_t)fpref[b] * kGammatoneBands;
    const double* sd = spec_deg + at * kGammatoneBands;
    double* out = dspec + at * kGammatoneBands;
    double* R = planes + at * kGammatoneBands;
    double* D = R + plane;
    double* P = D + plane;               // five planes
    double* dR = P + 5 * plane;
    double* dD = dR + plane;
    const int n = F * kGammatoneBands;
    // ---- the forward's planes, by the forward's own steps
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
            rt[k] = nsim_max(floor_t, rt[k]);
            dt[k] = nsim_max(floor_t, dt[k]);
        }
    }
    __syncthreads();
    // least and the cell that attains it first: flat index ascending, clean before degraded (key = 2 i + plane)
    double lo = INFINITY;
    long long lk = 0;
    int nan = 0;
    for (int i = tid; i < n; i += 256) {
        const double a = R[i], d = D[i];
        nan |= (a != a) | (d != d);
        if (a < lo) {
            lo = a;
            lk = 2ll * i;
        }
        if (d < lo) {
            lo = d;
            lk = 2ll * i + 1;
        }
    }
    red[tid] = lo;
    key[tid] = lk;
    bad[tid] = nan;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) {
            const double o = red[tid + h];
            if (o < red[tid] || (o == red[tid] && key[tid + h] < key[tid])) {
                red[tid] = o;
                key[tid] = key[tid + h];
            }
            bad[tid] |= bad[tid + h];
        }
        __syncthreads();
    }
    if (bad[0]) {   // the row's NSIM is NaN: so is its gradient, all of it
        for (int i = tid; i < n; i += 256) out[i] = (double)NAN;
        return;
    }
    const double least = red[0];
    const long long least_key = key[0];
    __syncthreads();   // red is used again below
    for (int i = tid; i < n; i += 256) {
        R[i] -= least;
        D[i] -= least;
    }
    __syncthreads();
    // ---- the map's partials per cell
    const double gm = grad[j] / (21.0 * (double)F);
    for (int i = tid; i < n; i += 256) {
        const int t = i / kGammatoneBands, band = i % kGammatoneBands;
        double p0, p1, p2, p3, p4;
        nsim_cell_partials(R, D, F, t, band, C1, C3, gm, p0, p1, p2, p3, p4);
        P[i] = p0;
        P[plane + i] = p1;
        P[2 * plane + i] = p2;
        P[3 * plane + i] = p3;
        P[4 * plane + i] = p4;
    }
    __syncthreads();
    // ---- the window's adjoint: cell (tt, bb) receives every term whose clamped index lands on it; source frames ascending, the
    // window's row offsets ascending inside, source bands ascending inside that, the window's column offsets ascending innermost
    const double w[3][3] = {{0.0113, 0.0838, 0.0113}, {0.0838, 0.6193, 0.0838}, {0.0113, 0.0838, 0.0113}};
    double part = 0.0;
    for (int i = tid; i < n; i += 256) {
        const int tt = i / kGammatoneBands, bb = i % kGammatoneBands;
        const double a = R[i], d = D[i];
        double ar = 0.0, ad = 0.0;
        for (int t = tt - 1; t <= tt + 1; ++t) {
            if (t < 0 || t >= F) continue;
            for (int dt = -1; dt <= 1; ++dt) {
                const int tc = t + dt < 0 ? 0 : t + dt >= F ? F - 1 : t + dt;
                if (tc != tt) continue;
                for (int bs = bb - 1; bs <= bb + 1; ++bs) {
                    if (bs < 0 || bs >= kGammatoneBands) continue;
                    for (int db = -1; db <= 1; ++db) {
                        const int bc = bs + db < 0 ? 0 : bs + db >= kGammatoneBands ? kGammatoneBands - 1 : bs + db;
                        if (bc != bb) continue;
                        const size_t src = (size_t)t * kGammatoneBands + bs;
                        const double ww = w[dt + 1][db + 1], grd = P[4 * plane + src];
                        ar += ww * (P[src] + 2.0 * a * P[2 * plane + src] + d * grd);
                        ad += ww * (P[plane + src] + 2.0 * d * P[3 * plane + src] + a * grd);
                    }
                }
            }
        }
        dR[i] = ar;
        dD[i] = ad;
        part += ar + ad;
    }
    // ---- least takes minus the sum over both planes: per-thread sums in index order, folded by halves (an order F alone decides)
    red[tid] = part;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        double* to = (least_key & 1) ? dD : dR;
        to[least_key >> 1] += -red[0];
    }
    __syncthreads();
    // ---- the per-frame floors, the peak, and dB -> dS: one thread per frame, clean bands ascending, then degraded bands ascending
    const double db_scale = 10.0 / 2.302585092994046;   // d (10 log10 s) / d s = db_scale / s
    for (int t = tid; t < F; t += 256) {
        const double* srt = sr + (size_t)t * kGammatoneBands;
        const double* sdt = sd + (size_t)t * kGammatoneBands;
        double* grt = dR + (size_t)t * kGammatoneBands;
        double* gdt = dD + (size_t)t * kGammatoneBands;
        double peak = nsim_db(srt[0]);
        int arg = 0;   // the first cell that attains the peak, in the forward's walk: 0 .. 20 clean, 21 .. 41 degraded
        for (int k = 1; k < kGammatoneBands; ++k) {
            const double v = nsim_db(srt[k]);
            if (v > peak) {
                peak = v;
                arg = k;
            }
        }
        for (int k = 0; k < kGammatoneBands; ++k) {
            const double v = nsim_db(sdt[k]);
            if (v > peak) {
                peak = v;
                arg = kGammatoneBands + k;
            }
        }
        const double floor_t = peak - 45.0;
        double gp = 0.0;
        for (int k = 0; k < kGammatoneBands; ++k)
            if (!(nsim_db(srt[k]) > floor_t)) gp += grt[k];   // a clean cell on the frame's floor hands its gradient to the peak
        for (int k = 0; k < kGammatoneBands; ++k)
            if (!(nsim_db(sdt[k]) > floor_t)) {
                gp += gdt[k];
                gdt[k] = 0.0;
            }
        if (arg >= kGammatoneBands) gdt[arg - kGammatoneBands] += gp;   // a clean peak: the gradient ends there
        for (int k = 0; k < kGammatoneBands; ++k) out[(size_t)t * kGammatoneBands + k] = nsim_db_passes(sdt[k]) ? gdt[k] * db_scale / sdt[k] : 0.0;
    }
}

}  // namespace nomad
