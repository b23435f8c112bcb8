"""ITU-R BS.1770-4 loudness of one mono clip, restated in float64 with ``scipy.signal.lfilter`` and numpy: what
``nomad_degrade_normalize`` is held to (include/nomad_hip.h states the same).  Imported by the tests like ``degrade_ref``; not a
test module itself."""
from __future__ import annotations

import math

import numpy as np
from scipy.signal import lfilter

MODES = ("ebu", "rms", "peak")


def k_weighting(fs: int):
    """((b, a) of the shelf, (b, a) of the high-pass) for the sample rate ``fs``: the standard's two stages re-derived from
    their analogue parameters (at 48 kHz its table)."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = (np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]),
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    high = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    return shelf, high


def _lufs(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def measure(x, fs: int = 16000, kind: str = "ebu") -> dict:
    """-> {"level": LUFS (ebu) or dBFS (rms, peak), "peak": max|x| (the sample peak), "blocks": blocks past both gates (0 for rms
    and peak), "absolute": blocks past the absolute gate, "total": whole blocks, "margin": the smallest distance in dB of any
    block from either gate (inf where there is none)}."""
    if kind not in MODES:
        raise ValueError(f"kind must be one of {MODES}, got {kind!r}")
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.shape[0]
    peak = float(np.abs(x).max())
    res = {"peak": peak, "blocks": 0, "absolute": 0, "total": 0, "margin": math.inf}
    with np.errstate(divide="ignore"):
        if kind == "rms":
            res["level"] = float(20.0 * np.log10(np.sqrt(np.mean(x * x))))
            return res
        if kind == "peak":
            res["level"] = float(20.0 * np.log10(peak))
            return res
    (b1, a1), (b2, a2) = k_weighting(fs)
    y = lfilter(b2, a2, lfilter(b1, a1, x))
    hop = fs // 10
    nb = (n - 4 * hop) // hop + 1 if n >= 4 * hop else 0
    res["total"] = nb
    res["level"] = -math.inf
    if nb == 0:
        return res
    z = np.array([np.mean(y[j * hop:j * hop + 4 * hop] ** 2) for j in range(nb)])
    lj = _lufs(z)
    absolute = lj > -70.0
    margin = float(np.min(np.abs(lj + 70.0)))
    res["absolute"] = int(absolute.sum())
    if absolute.any():
        gamma = float(_lufs(np.mean(z[absolute]))) - 10.0
        both = absolute & (lj > gamma)
        margin = min(margin, float(np.min(np.abs(lj[absolute] - gamma))))
        res["blocks"] = int(both.sum())
        res["level"] = float(_lufs(np.mean(z[both])))
    res["margin"] = margin
    return res


def gain(level: float, peak: float, target: float, peak_db=None) -> float:
    """The linear gain to ``target``: 1 for a level of -inf, capped so that the sample peak stays at ``peak_db`` dBFS."""
    if level == -math.inf:
        return 1.0
    g = 10.0 ** ((target - level) / 20.0)
    if peak_db is not None:
        g = min(g, 10.0 ** (peak_db / 20.0) / peak)
    return g


def apply(x, g: float):
    """``float32(float64(x) g)``: the device's output row for the gain it reports."""
    return (np.asarray(x, dtype=np.float32).astype(np.float64) * np.float64(g)).astype(np.float32)


# ---- the test signals (tests/test_loudness_host.py pins what they show; tests/test_gpu_loudness.py runs them on the device) ----
def pcm_noise(n: int, seed: int, scale: float = 0.25):
    """16-bit PCM white noise."""
    return (np.random.RandomState(seed).randint(-32768, 32768, size=n) / 32768.0 * scale).astype(np.float32)


def sine(n: int, fs: int, freq: float = 997.0, amp: float = 1.0):
    return (amp * np.sin(2.0 * np.pi * freq * np.arange(n) / fs)).astype(np.float32)


def silent_second(n: int, fs: int, seed: int):
    """Noise with one digital-silent second in the middle: those blocks fall to the absolute gate."""
    x = pcm_noise(n, seed)
    lo = (n - fs) // 2
    x[lo:lo + fs] = 0.0
    return x


def quiet_passage(n: int, fs: int, seed: int, drop_db: float = 15.0):
    """Noise whose last third is ``drop_db`` quieter: those blocks pass the absolute gate and fall to the relative one."""
    x = pcm_noise(n, seed).astype(np.float64)
    x[2 * n // 3:] *= 10.0 ** (-drop_db / 20.0)
    return x.astype(np.float32)


def dc_offset(n: int, seed: int, offset: float = 0.5):
    """Noise on a constant: the high-pass removes the constant, the rms and peak levels keep it."""
    return (pcm_noise(n, seed, 0.1) + np.float32(offset)).astype(np.float32)
