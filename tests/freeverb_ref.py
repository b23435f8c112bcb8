"""The sox-style reverb of ``nomad_degrade_reverb`` restated sample by sample in float64 (include/nomad_hip.h has the text this
follows, line by line).  Imported by the tests like ``loudness_ref``; not a test module itself.

Plain Python floats - IEEE double, every operation rounded once, nothing fused, nothing reordered - so this IS the recurrence as
written: one comb after the other from 7 down to 0, then the all-passes from 3 down to 0, one sample at a time.  Like the
kernel's header it is written from the project's own statement of the algorithm (itself from memory of sox 14.4 reverb.c); whether
that statement matches the sox binary has not been measured anywhere."""
from __future__ import annotations

import math

import numpy as np

COMB_LENGTHS = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS_LENGTHS = (225, 341, 441, 556)
STEREO_ADJUST = 12
DEFAULTS = dict(hf_damping=50.0, room_scale=100.0, stereo_depth=100.0, pre_delay_ms=0.0, wet_gain_db=0.0, wet_only=False, clamp=True,
                sample_rate=16000)


def feedback(reverberance: float) -> float:
    a = -1.0 / math.log(1.0 - 0.3)
    b = 100.0 / (math.log(1.0 - 0.98) * a + 1.0)
    return 1.0 - math.exp((reverberance - b) / (a * b))


def delays(sample_rate: int = 16000, room_scale: float = 100.0, stereo_depth: float = 100.0):
    """[(comb delays, all-pass delays)] per channel, channels 0 .. ceil(stereo_depth / 100)."""
    scale = room_scale / 100.0 * 0.9 + 0.1
    depth = stereo_depth / 100.0
    r = sample_rate * (1 / 44100.)
    out = []
    for c in range(int(math.ceil(depth)) + 1):
        off = c * depth
        combs, allpasses = [], []
        for n in COMB_LENGTHS:
            combs.append(int(scale * r * (n + STEREO_ADJUST * off) + 0.5))
            off = -off
        for n in ALLPASS_LENGTHS:
            allpasses.append(int(r * (n + STEREO_ADJUST * off) + 0.5))
            off = -off
        out.append((combs, allpasses))
    return out


def wet(x, reverberance, hf_damping=50.0, room_scale=100.0, stereo_depth=100.0, pre_delay_ms=0.0, wet_gain_db=0.0, sample_rate=16000):
    """x: float32 (n,) -> float64 (channels, n): wet_c[t] of every channel."""
    xs = [float(v) for v in np.asarray(x, dtype=np.float32).astype(np.float64)]
    n = len(xs)
    fb = feedback(float(reverberance))
    damp = hf_damping / 100.0 * 0.3 + 0.2
    gain = 10.0 ** (wet_gain_db / 20.0) * 0.015
    pre = int(pre_delay_ms / 1000.0 * sample_rate + 0.5)
    chans = delays(sample_rate, room_scale, stereo_depth)
    out = np.zeros((len(chans), n), dtype=np.float64)
    for c, (combs, allpasses) in enumerate(chans):
        lines = [[0.0] * d for d in combs]
        stores = [0.0] * 8
        aps = [[0.0] * d for d in allpasses]
        row = out[c]
        for t in range(n):
            src = xs[t - pre] if t >= pre else 0.0
            acc = 0.0
            for i in range(7, -1, -1):
                line = lines[i]
                at = t % combs[i]                      # a ring of D entries: the slot of t - D is the slot of t
                o = line[at]
                st = o + (stores[i] - o) * damp
                stores[i] = st
                line[at] = src + st * fb
                acc += o
            for j in range(3, -1, -1):
                ap = aps[j]
                at = t % allpasses[j]
                o = ap[at]
                ap[at] = acc + o * 0.5
                acc = o - acc
            row[t] = acc * gain
    return out


def mix(x, wet_planes, wet_only=False, clamp=True, as_float32=True):
    """y = (1 - wet_only) x + mean_c wet_c, the limit, one rounding to float32 (as_float32=False: the float64 value before it)."""
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    m = 0.5 * (wet_planes[0] + wet_planes[1]) if wet_planes.shape[0] == 2 else wet_planes[0]
    with np.errstate(invalid="ignore"):
        y = (1.0 - float(bool(wet_only))) * xd + m
    if clamp:
        y = np.where(y > 1.0, 1.0, np.where(y < -1.0, -1.0, y))      # both comparisons fail for a NaN: it stays
    return y.astype(np.float32) if as_float32 else y


def reverb(x, reverberance, hf_damping=50.0, room_scale=100.0, stereo_depth=100.0, pre_delay_ms=0.0, wet_gain_db=0.0, wet_only=False,
           clamp=True, sample_rate=16000, as_float32=True):
    w = wet(x, reverberance, hf_damping, room_scale, stereo_depth, pre_delay_ms, wet_gain_db, sample_rate)
    return mix(x, w, wet_only, clamp, as_float32)


def noise(n: int, seed: int, amp: float = 0.1) -> np.ndarray:
    """Seeded uniform noise in [-amp, amp) as float32."""
    return ((np.random.default_rng(seed).random(n) * 2.0 - 1.0) * amp).astype(np.float32)
