"""Float64 numpy restatement of the time alignment of include/nomad_hip.h (``nomad_align_delay`` / ``nomad_align_shift``): the
cross-correlation over the lags -D .. D, the sum of magnitudes the error bound of the fp32 chains is stated in, the selection rule
and the shift.  Nothing here runs on the GPU; tests/test_align_host.py holds it to scipy and to hand-made tables."""
import numpy as np

SLICE = 4096      # time steps of one fp32 chain (kAlignSlice)


def corr(x, y, D):
    """c[d + D] = sum over i with 0 <= i < n and 0 <= i + d < m of x[i] y[i + d] for d = -D .. D, in float64 (one dot product per
    lag, so integer-valued inputs give exact sums)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.shape[0]
    pad = np.zeros(n + 2 * D, dtype=np.float64)      # pad[j] = y[j - D]
    m = min(y.shape[0], n + D)
    pad[D:D + m] = y[:m]
    return np.correlate(pad, x, mode="valid")


def magnitude(x, y, D):
    """sum |x[i]| |y[i + d]| over the same terms: what the bound scales with."""
    return corr(np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(y, dtype=np.float64)), D)


def bound(x, y, D):
    """|c_gpu[d] - c[d]| <= (SLICE + 8) 2^-24 (sum |x| |y|)[d] + 1e-37 n: the running-error bound of an fp32 multiply-add chain of at most
    SLICE terms (each step rounds a partial sum that is at most the sum of magnitudes, once, by at most 2^-24 relatively), + 8 for
    what the merging of accumulators could add, the last term for products that underflow.  The float64 sum of the slices adds
    nothing at this scale."""
    return (SLICE + 8) * 2.0 ** -24 * magnitude(x, y, D) + 1e-37 * len(x)


def select(c, D):
    """(delay, peak) of one row's table c[0 .. 2 D]: the lag of the largest value - ties to the smaller |d|, then to d >= 0; any NaN
    gives (0, NaN)."""
    c = np.asarray(c, dtype=np.float64)
    assert c.shape == (2 * D + 1,)
    if np.isnan(c).any():
        return 0, float("nan")
    lags = np.flatnonzero(c == c.max()) - D
    best = int(min(lags, key=lambda d: (abs(d), -d)))
    return best, float(c[best + D])


def shift(y, delay, n, stride=None):
    """out[i] = y[i + delay] for 0 <= i < n and 0 <= i + delay < m, 0 otherwise and up to ``stride``; the samples keep their bits."""
    y = np.asarray(y, dtype=np.float32)
    out = np.zeros(n if stride is None else stride, dtype=np.float32)
    i = np.arange(n, dtype=np.int64)
    j = i + int(delay)
    ok = (j >= 0) & (j < y.shape[0])
    out[i[ok]] = y[j[ok]]
    return out
