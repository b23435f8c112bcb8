"""The gammatone-spectrogram NSIM of include/nomad_hip.h restated in torch with autograd, the gradient conventions of the header
("NSIM as a loss") written with ``torch.where``; imported by the tests like ``nsim_ref``, not a test module itself.  The recurrence
is ``nsim_ref.spectrogram``'s sample loop, vectorised over frames and bands.  float64 is the restatement; float32 (``dtype=``) exists
only for the bound the GPU tests derive from it (``tau``).

The conventions, as the header states them: sqrt has gradient 0 at 0; ``max(value, floor)`` hands its gradient to ``value`` only
where ``value > floor`` strictly, else to the floor (eps and -45 take nothing, the per-frame floor hands it to the peak p_t); p_t
hands it to the FIRST cell that attains it, clean bands ascending then degraded bands ascending; ``least`` to the attaining cell with
the lowest flat index, clean before degraded at the same index; the window's adjoint honours the replicated edges (index clamping
under autograd does exactly that)."""
import numpy as np
import torch

import nsim_ref as N

BANDS = N.BANDS


def _sqrt0(v):
    """sqrt with gradient 0 where v <= 0 (and value 0 there)."""
    pos = v > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, v, torch.ones_like(v))), torch.zeros_like(v))


def _floor(value, floor):
    """max(value, floor): the gradient goes to ``value`` only where value > floor strictly."""
    return torch.where(value > floor, value, floor)


def spectrogram(x, fs: int = 16000, dtype=torch.float64):
    """x: one row, a torch tensor of n samples (its gradient is followed) -> S [F][21] in ``dtype``."""
    H = fs // 50
    W = 4 * H
    F = N.frames_of(x.shape[0], fs)
    assert F >= 1, "shorter than one frame"
    b0, b1, a1, a2 = (torch.from_numpy(np.asarray(v)).to(dtype) for v in N.bank(fs))
    idx = torch.arange(F)[:, None] * H + torch.arange(W)[None, :]
    seg = x.to(dtype)[idx]                                                  # [F][W]
    zero = torch.zeros(F, BANDS, dtype=dtype)
    z1, z2 = [zero] * 4, [zero] * 4
    acc = zero
    for i in range(W):
        v = seg[:, i, None].expand(F, BANDS)
        for k in range(4):
            y = b0[None, :, k] * v + z1[k]
            z1[k] = b1[None, :, k] * v - a1[None, :] * y + z2[k]
            z2[k] = -a2[None, :] * y
            v = y
        acc = acc + v * v
    return _sqrt0(acc / W)


def _window(X):
    """w * X with the edges replicated, the nine terms row by row as ``nsim_ref._window`` adds them."""
    F, Nb = X.shape
    out = torch.zeros_like(X)
    for dt in (-1, 0, 1):
        ti = (torch.arange(F) + dt).clamp(0, F - 1)
        for db in (-1, 0, 1):
            bi = (torch.arange(Nb) + db).clamp(0, Nb - 1)
            out = out + N.WINDOW[dt + 1][db + 1] * X[ti][:, bi]
    return out


def nsim_map(R, D, intensity_range: float = 1.0):
    """Clean spectrogram R and degraded D, [F][21] torch tensors of one dtype -> (nsim, counters).  Counters: ``abs_floor_deg``
    degraded cells on the absolute floor (-45 or eps); ``frame_floor_clean`` / ``frame_floor_deg`` cells on the per-frame floor;
    ``frame_floor_clean_deg_peak`` clean cells on a per-frame floor set by a degraded peak; ``deg_peak_frames`` frames whose peak
    is a degraded cell; ``zero_var`` cells with var <= 0 in either plane."""
    dtype = R.dtype
    F = R.shape[0]
    eps = torch.tensor(2.0 ** -52, dtype=dtype)
    lo = torch.tensor(-45.0, dtype=dtype)
    X, on_abs = [], []
    for S in (R, D):
        v = _floor(S, eps)
        x10 = 10.0 * torch.log10(v)
        X.append(_floor(x10, lo))
        on_abs.append(~((S > eps) & (x10 > lo)))
    both = torch.cat(X, dim=1)                                              # clean bands, then degraded bands
    top = both.detach().max(dim=1).values
    first = (both.detach() == top[:, None]).to(torch.int64).argmax(dim=1)   # the first of several maxima
    peak = both.gather(1, first[:, None])                                   # [F][1]
    fl = peak - 45.0
    on_frame = [~(V > fl) for V in X]
    X = [_floor(V, fl.expand(F, BANDS)) for V in X]
    flat = torch.stack(X, dim=-1).reshape(-1)                               # cell by cell, clean before degraded
    at = (flat.detach() == flat.detach().min()).to(torch.int64).argmax()
    least = flat[at]
    r, d = X[0] - least, X[1] - least
    mr, md = _window(r), _window(d)
    vr_raw, vd_raw = _window(r * r) - mr * mr, _window(d * d) - md * md
    sr, sd = _sqrt0(vr_raw), _sqrt0(vd_raw)
    cov = _window(r * d) - mr * md
    C1, C3 = (0.01 * intensity_range) ** 2, (0.03 * intensity_range) ** 2 / 2.0
    m = (2.0 * mr * md + C1) / (mr * mr + md * md + C1) * ((cov + C3) / (sr * sd + C3))
    bands = torch.zeros(BANDS, dtype=dtype)
    for f in range(F):
        bands = bands + m[f]
    bands = bands / F
    total = torch.zeros((), dtype=dtype)
    for b in range(BANDS):
        total = total + bands[b]
    deg_peak = first >= BANDS
    counters = {"abs_floor_deg": int(on_abs[1].sum()), "frame_floor_clean": int(on_frame[0].sum()), "frame_floor_deg": int(on_frame[1].sum()),
                "frame_floor_clean_deg_peak": int((on_frame[0] & deg_peak[:, None]).sum()), "deg_peak_frames": int(deg_peak.sum()),
                "zero_var": int((vr_raw <= 0).sum() + (vd_raw <= 0).sum())}
    return total / BANDS, counters


def nsim(clean, degraded, fs: int = 16000, intensity_range: float = 1.0, dtype=torch.float64):
    """The whole measure for one pair of rows (torch tensors; ``degraded``'s gradient is followed) -> (nsim, counters)."""
    return nsim_map(spectrogram(clean, fs, dtype), spectrogram(degraded, fs, dtype), intensity_range)


def map_grad(R, D, intensity_range: float = 1.0, upstream: float = 1.0, dtype=torch.float64):
    """d (upstream nsim) / d D for spectrograms given as numpy arrays -> (nsim, gradient [F][21] numpy, counters)."""
    Rt = torch.from_numpy(np.asarray(R, dtype=np.float64)).to(dtype)
    Dt = torch.from_numpy(np.asarray(D, dtype=np.float64)).to(dtype).requires_grad_(True)
    score, counters = nsim_map(Rt, Dt, intensity_range)
    g, = torch.autograd.grad(score * upstream, Dt)
    return float(score.detach()), g.to(torch.float64).numpy(), counters


def spectrogram_grad(x, dspec, fs: int = 16000, dtype=torch.float64):
    """sum(dspec S(x)) differentiated with respect to the samples: the adjoint ``nomad_gammatone_backward`` computes.  x: n samples
    (numpy), dspec [F][21] -> gradient [n] float64 numpy (0 behind the whole frames)."""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dtype).requires_grad_(True)
    S = spectrogram(xt, fs, dtype)
    g, = torch.autograd.grad((S * torch.from_numpy(np.asarray(dspec, dtype=np.float64)).to(dtype)).sum(), xt)
    return g.to(torch.float64).numpy()


def loss_grad(clean, estimate, fs: int = 16000, intensity_range: float = 1.0, upstream: float = 1.0, dtype=torch.float64):
    """d (upstream (1 - nsim)) / d estimate -> (nsim, gradient [n] float64 numpy, counters)."""
    c = torch.from_numpy(np.asarray(clean, dtype=np.float32)).to(dtype)
    e = torch.from_numpy(np.asarray(estimate, dtype=np.float32)).to(dtype).requires_grad_(True)
    score, counters = nsim(c, e, fs, intensity_range, dtype)
    g, = torch.autograd.grad((1.0 - score) * upstream, e)
    return float(score.detach()), g.to(torch.float64).numpy(), counters


def tau(g64, g32) -> float:
    """The tolerance the GPU tests hold a float64 result to, relative to max|g|: the restatement's own float32 run against its
    float64 one on the same inputs, relative to max|g|, times 2^-25 (the ratio of the formats' rounding units, 2^-29, times a
    margin of 16 for order differences)."""
    g64, g32 = np.asarray(g64, dtype=np.float64), np.asarray(g32, dtype=np.float64)
    return float(np.abs(g32 - g64).max() / np.abs(g64).max()) * 2.0 ** -25


# ---- the five cuts the host and GPU tests share (tests/golden/wavs/nmr-data/FI53_04.wav, samples 8000 .. 12800) ---------------------
def cases(clip):
    """clip: the golden file's samples -> {name: (clean, degraded)} fp32 rows of 4800 samples."""
    x = np.asarray(clip, dtype=np.float32)[8000:12800].copy()
    noise = N.pcm_noise(4800, 3)
    a = N.add_noise(x, noise, 10.0)
    b = N.clip(x, 20.0)
    c = N.add_noise(x, noise, 5.0)
    c[1600:3400] = 0.0
    d_clean = x * np.float32(1000.0)
    d = N.add_noise(x, noise, 15.0)
    d[0:1500] *= np.float32(1e-4)
    return {"a": (x, a), "b": (x, b), "c": (x, c), "d": (d_clean, d), "e": (d, d_clean)}
