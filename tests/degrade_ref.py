"""Float64 numpy restatement of the two degradations of ``nomad_degrade_noise`` / ``nomad_degrade_clip`` (include/nomad_hip.h),
written from those formulas.  Imported by the tests like ``ref64`` / ``knn_ref``; not a test module itself.

One clip at a time: x is a 1-D float32 array, the levels a sequence of floats; every function returns one row per level."""
import numpy as np


def clip_thresholds(x, clip_factor):
    """-> (G, 2) float64: (v_lo, v_hi) per level - numpy's default linear percentile rule at cf / 2 and 100 - cf / 2 on the clip's
    own samples: h = (n - 1) (p / 100), lo = floor(h), hi = min(lo + 1, n - 1), t = h - lo, v = a + (b - a) t, with a and b the
    lo-th and hi-th order statistics (numpy's sort order: NaN last) in float64."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = x.shape[0]
    s = np.sort(x).astype(np.float64)
    out = np.empty((len(clip_factor), 2), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for g, cf in enumerate(clip_factor):
            cf = np.float64(cf)
            for j, p in enumerate((cf / 2, 100 - cf / 2)):
                h = np.float64(n - 1) * (p / 100.0)
                lo = int(np.floor(h))
                hi = min(lo + 1, n - 1)
                t = h - lo
                a, b = s[lo], s[hi]
                out[g, j] = a + (b - a) * t
    return out


def clip_apply(x, thresholds):
    """-> (G, n) float32: x > v_hi ? (float)v_hi : x < v_lo ? (float)v_lo : x, compared in float64 (NaN compares false)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    xd = x.astype(np.float64)
    out = np.empty((thresholds.shape[0], x.shape[0]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for g, (vlo, vhi) in enumerate(thresholds):
            out[g] = np.where(xd > vhi, np.float32(vhi), np.where(xd < vlo, np.float32(vlo), x))
    return out


def clip(x, clip_factor):
    """-> (rows (G, n) float32, thresholds (G, 2) float64)."""
    thr = clip_thresholds(x, clip_factor)
    return clip_apply(x, thr), thr


def noise(x, s, snr_db):
    """-> (rows (G, n) float32, alpha (G,) float64, rows (G, n) float64 before the rounding to float32):
    xp = sqrt(mean x^2), sp = sqrt(mean s[i mod Ls]^2) over the clip's n samples, alpha = (xp / 10^(snr / 10)) / sp,
    out = (float)(x + alpha s[i mod Ls]), everything in float64.  No special cases."""
    x = np.asarray(x, dtype=np.float32).reshape(-1).astype(np.float64)
    s = np.asarray(s, dtype=np.float32).reshape(-1).astype(np.float64)
    n = x.shape[0]
    st = s[np.arange(n) % s.shape[0]]
    with np.errstate(all="ignore"):
        xp = np.sqrt(np.mean(x * x))
        sp = np.sqrt(np.mean(st * st))
        alpha = np.array([(xp / 10.0 ** (np.float64(v) / 10.0)) / sp for v in snr_db], dtype=np.float64)
        exact = x[None, :] + alpha[:, None] * st[None, :]
        return exact.astype(np.float32), alpha, exact
