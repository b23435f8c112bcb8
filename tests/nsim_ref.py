"""The gammatone-spectrogram NSIM of include/nomad_hip.h restated in numpy; imported by the tests like ``loudness_ref``, not a test
module itself.  The recurrence is an explicit per-sample loop, vectorised over frames and bands, in ``np.longdouble`` (or any
other dtype, for the bounds the GPU tests derive); the floors and the map run in float64 (or, for the same purpose, long double).
Nothing here is ViSQOL: the header's text is the definition, and this file follows it line by line."""
import numpy as np

BANDS = 21
EARQ, MINBW, LO, HI = 9.26449, 24.7, 50.0, 8000.0
WINDOW = ((0.0113, 0.0838, 0.0113), (0.0838, 0.6193, 0.0838), (0.0113, 0.0838, 0.0113))
_BANK = {}


def centres():
    """Band centres in Hz, band 0 the lowest (Slaney's i = N)."""
    i = np.arange(BANDS, 0, -1, dtype=np.float64)
    return -(EARQ * MINBW) + np.exp(i * (np.log(LO + EARQ * MINBW) - np.log(HI + EARQ * MINBW)) / BANDS) * (HI + EARQ * MINBW)


def bank(fs: int):
    """-> (b0 [21][4], b1 [21][4], a1 [21], a2 [21]) float64: the four sections' numerators (the gain divided into the first
    section's) and the common denominator."""
    if fs not in _BANK:
        cf = centres()
        T = 1.0 / fs
        B = 1.019 * 2.0 * np.pi * (cf / EARQ + MINBW)
        c, s, e = np.cos(2.0 * np.pi * cf * T), np.sin(2.0 * np.pi * cf * T), np.exp(B * T)
        a1, a2 = -2.0 * c / e, np.exp(-2.0 * B * T)
        rp, rm = np.sqrt(3.0 + 2.0 ** 1.5), np.sqrt(3.0 - 2.0 ** 1.5)
        A1 = np.stack([-(2.0 * T * c / e + 2.0 * rp * T * s / e) / 2.0, -(2.0 * T * c / e - 2.0 * rp * T * s / e) / 2.0,
                       -(2.0 * T * c / e + 2.0 * rm * T * s / e) / 2.0, -(2.0 * T * c / e - 2.0 * rm * T * s / e) / 2.0], axis=1)
        u = np.exp(-2j * np.pi * cf * T)                                    # 1 / z at the centre
        resp = np.prod((T + A1 * u[:, None]) / (1.0 + a1 * u + a2 * u * u)[:, None], axis=1)
        g = np.abs(resp)
        b0 = np.full((BANDS, 4), T)
        b1 = A1.copy()
        b0[:, 0] /= g
        b1[:, 0] /= g
        _BANK[fs] = (b0, b1, a1, a2)
    return _BANK[fs]


def response_at_centre(fs: int):
    """|H(exp(j 2 pi cf T))| of every band's cascade with the gain divided in: 1 by construction."""
    b0, b1, a1, a2 = bank(fs)
    u = np.exp(-2j * np.pi * centres() / fs)
    return np.abs(np.prod((b0 + b1 * u[:, None]) / (1.0 + a1 * u + a2 * u * u)[:, None], axis=1))


def frames_of(n: int, fs: int = 16000) -> int:
    H = fs // 50
    return 0 if n < 4 * H else (n - 4 * H) // H + 1


def spectrogram(x, fs: int = 16000, dtype=np.longdouble):
    """x: one row, fp32 -> S [F][21] in ``dtype``: per frame and band the four sections from the zero state over the frame's W
    samples, section k fed by section k - 1, sqrt(sum y^2 / W) in time order.  A non-finite sample makes its frames NaN."""
    x = np.asarray(x, dtype=np.float32)
    H = fs // 50
    W = 4 * H
    F = frames_of(x.shape[0], fs)
    assert F >= 1, "shorter than one frame"
    b0, b1, a1, a2 = (np.asarray(v, dtype=dtype) for v in bank(fs))
    idx = np.arange(F)[:, None] * H + np.arange(W)[None, :]
    seg = x[idx]                                                           # [F][W] fp32
    bad = ~np.isfinite(seg).all(axis=1)
    seg = np.where(np.isfinite(seg), seg, np.float32(0.0)).astype(dtype)
    z1 = np.zeros((4, F, BANDS), dtype=dtype)
    z2 = np.zeros((4, F, BANDS), dtype=dtype)
    acc = np.zeros((F, BANDS), dtype=dtype)
    for i in range(W):
        v = np.broadcast_to(seg[:, i, None], (F, BANDS))
        for k in range(4):
            y = b0[None, :, k] * v + z1[k]
            z1[k] = b1[None, :, k] * v - a1[None, :] * y + z2[k]
            z2[k] = -a2[None, :] * y
            v = y
        acc += v * v
    S = np.sqrt(acc / dtype(W))
    S[bad] = np.nan
    return S


def _sticky_max(a, b):
    """Element-wise maximum that a NaN in either enters (numpy's ``maximum`` does exactly that)."""
    return np.maximum(a, b)


def _window(X):
    """w * X with the edges replicated, the nine terms row by row: frames t - 1, t, t + 1 outside, bands b - 1, b, b + 1 inside."""
    F, Nb = X.shape
    P = np.pad(X, 1, mode="edge")
    out = np.zeros_like(X)
    for dt in range(3):
        for db in range(3):
            out = out + X.dtype.type(WINDOW[dt][db]) * P[dt:dt + F, db:db + Nb]
    return out


def nsim_map(R, D, intensity_range: float = 1.0, dtype=np.float64):
    """Clean spectrogram R and degraded D, both [F][21] -> (nsim, bands [21], map [F][21]) in ``dtype``."""
    R, D = np.asarray(R, dtype=dtype), np.asarray(D, dtype=dtype)
    assert R.shape == D.shape and R.shape[1] == BANDS
    t = dtype
    eps = t(2.0) ** -52
    with np.errstate(invalid="ignore", divide="ignore"):
        X = [_sticky_max(t(-45.0), t(10.0) * np.log10(_sticky_max(S, eps))) for S in (R, D)]
        peak = _sticky_max(X[0].max(axis=1), X[1].max(axis=1))            # numpy's max carries a NaN
        X = [_sticky_max(V, (peak - t(45.0))[:, None]) for V in X]
        least = np.minimum(X[0].min(), X[1].min())
        r, d = X[0] - least, X[1] - least
        mr, md = _window(r), _window(d)
        vr = np.maximum(_window(r * r) - mr * mr, t(0.0))
        vd = np.maximum(_window(d * d) - md * md, t(0.0))
        cov = _window(r * d) - mr * md
        L = t(intensity_range)
        C1, C3 = (t(0.01) * L) ** 2, (t(0.03) * L) ** 2 / t(2.0)
        m = (t(2.0) * mr * md + C1) / (mr * mr + md * md + C1) * ((cov + C3) / (np.sqrt(vr) * np.sqrt(vd) + C3))
    F = m.shape[0]
    bands = np.zeros(BANDS, dtype=dtype)
    for f in range(F):                                                      # ascending frames
        bands = bands + m[f]
    bands = bands / t(F)
    total = t(0.0)
    for b in range(BANDS):                                                  # ascending bands
        total = total + bands[b]
    return total / t(BANDS), bands, m


def nsim(clean, degraded, fs: int = 16000, intensity_range: float = 1.0):
    """The whole measure for one pair of rows -> (nsim, bands [21]) float64."""
    R = spectrogram(clean, fs).astype(np.float64)
    D = spectrogram(degraded, fs).astype(np.float64)
    score, bands, _ = nsim_map(R, D, intensity_range)
    return float(score), bands


# ---- test signals and the reference's degradations on the host (utils/degradations.py) ------------------------------------------
def pcm_noise(n: int, seed: int, scale: float = 0.25):
    """16-bit PCM white noise."""
    return (np.random.RandomState(seed).randint(-32768, 32768, size=n) / 32768.0 * scale).astype(np.float32)


def add_noise(x, noise, snr_db: float):
    """x + alpha s with alpha = (rms(x) / 10^(snr / 10)) / rms(s): the reference's formula as it stands, s tiled or cut to x."""
    x = np.asarray(x, dtype=np.float64)
    s = np.resize(np.asarray(noise, dtype=np.float64), x.shape[0])
    alpha = (np.sqrt(np.mean(x * x)) / 10.0 ** (snr_db / 10.0)) / np.sqrt(np.mean(s * s))
    return (x + alpha * s).astype(np.float32)


def clip(x, clip_factor: float):
    """Samples clamped to the clip's own percentiles cf / 2 and 100 - cf / 2."""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = np.percentile(x, [clip_factor / 2.0, 100.0 - clip_factor / 2.0])
    return np.clip(x, lo, hi).astype(np.float32)
