#!/usr/bin/env python3
"""Time alignment on the device (nomad_align_delay + nomad_align_shift): what the delay search over +-max_delay costs on the fp32
matrix cores, what the shift costs, and what alignment adds to ``Nomad.nsim``.  A record, not a threshold.

Workload: --clips clean clips of --seconds s (64 x 10 s), each with noise at the reference's 25 test SNRs (G = 25): 1600 rows, every
row then made late or early by its own known delay within +-700 samples and lengthened by 2000 samples.  Legs, alternating in ONE
process, median and fastest - slowest of --rounds rounds (a round times every leg once, so drift hits all alike):

  align_delay@S      ``Engine.align_delay`` at max_delay_s = S for S in 0.05 / 0.25 / 1.0 (801 / 4000 / 16000 samples each way); the
                     delays it returns are checked against the known ones before anything is timed
  align_shift        ``Engine.align_shift`` of the 1600 rows by those delays
  nsim_aligned       ``Nomad.nsim(max_delay_s=0.25)`` of the delayed rows: delay search, shift, both spectrograms, NSIM
  nsim_plain         ``Nomad.nsim()`` of the same rows already aligned: what the call cost before
  scipy              ``scipy.signal.correlate(method="fft")`` of ONE pair on the host, float64, for context

``align_delay`` also reports useful TFLOP/s - 2 x overlap FLOP per lag, the overlap being the terms the definition sums - and its
share of the 157.3 TFLOP/s fp32 matrix peak.  One JSON line; --out appends it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nomad_amd.nomad import Nomad, check_max_delay  # noqa: E402

REFERENCE_TEST_SNRS = [1, 3, 4, 6, 9, 10, 12, 14, 16, 19, 20, 22, 24, 26, 28, 30, 32, 33, 35, 37, 39, 42, 44, 46, 50]
FP32_MATRIX_PEAK = 157.3e12
EXTRA, SPREAD = 2000, 700


def _time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _stats(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def useful_flop(n, m, D, rows):
    d = np.arange(-D, D + 1, dtype=np.int64)
    overlap = np.maximum(0, np.minimum(n, m - d) - np.maximum(0, -d))
    return 2.0 * float(overlap.sum()) * rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--levels", type=lambda t: [float(v) for v in t.split(",")], default=REFERENCE_TEST_SNRS)
    ap.add_argument("--max-delays", type=lambda t: [float(v) for v in t.split(",")], default=[0.05, 0.25, 1.0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align.py needs a GPU: nomad_amd has no CPU path")
    nmd = Nomad(weights="seeded")
    eng = nmd.engine
    G = len(a.levels)
    n = int(a.seconds * 16000) // 4 * 4
    m = n + EXTRA
    R = a.clips * G
    rng = np.random.RandomState(0)
    env = 0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * np.arange(n) / 16000.0)
    host = (0.1 * env[None, :] * rng.uniform(-1.0, 1.0, size=(a.clips, n))).astype(np.float32)
    x = torch.from_numpy(host).cuda()
    noise = torch.from_numpy((0.1 * rng.randn(n)).astype(np.float32)).cuda()
    lens, dlens = [n] * a.clips, [m] * R
    rows, lens_rep, _ = eng.degrade_noise(x, noise, a.levels, lengths=lens)
    known = rng.randint(-SPREAD, SPREAD + 1, size=R).astype(np.int32)
    # row r late by known[r]: y[i + d] = row[i], which is the shift by -d
    late, _ = eng.align_shift((rows, lens_rep), torch.from_numpy(-known).cuda(), dlens)
    late = late.clone()
    clean, deg = (x, lens), (late, dlens)

    delays = {s: check_max_delay(s) for s in a.max_delays}
    for s, D in delays.items():
        found = eng.align_delay(clean, deg, G, D)[0].cpu().numpy()
        inside = np.abs(known) <= D
        assert np.array_equal(found[inside], known[inside]), f"max_delay_s {s}: {int((found[inside] != known[inside]).sum())} delays missed"
    found = eng.align_delay(clean, deg, G, max(delays.values()))[0]
    aligned = eng.align_shift(deg, found, lens_rep, out_stride=n)
    aligned = (aligned[0].clone(), aligned[1])
    late_rows = torch.from_numpy(known >= 0).cuda()      # (a row made early lost its first samples for good)
    assert torch.equal(aligned[0][late_rows], rows[late_rows]), "the late rows moved back are the rows before they were delayed"

    from scipy.signal import correlate
    pair = (late[0].cpu().numpy().astype(np.float64), host[0].astype(np.float64))
    correlate(pair[0][:4096], pair[1][:4096], mode="full", method="fft")      # (scipy's own first-call set-up is not the pair's time)
    t0 = time.perf_counter()
    c = correlate(pair[0], pair[1], mode="full", method="fft")
    scipy_ms = 1e3 * (time.perf_counter() - t0)
    assert int(np.argmax(c)) - (n - 1) == int(known[0])

    legs = {f"align_delay@{s:g}": (lambda D=D: eng.align_delay(clean, deg, G, D)) for s, D in delays.items()}
    legs["align_shift"] = lambda: eng.align_shift(deg, found, lens_rep, out_stride=n)
    legs["nsim_aligned"] = lambda: nmd.nsim(deg, x, lengths=lens, max_delay_s=0.25)
    legs["nsim_plain"] = lambda: nmd.nsim(aligned, x, lengths=lens)
    for fn in legs.values():
        fn()
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, fn in legs.items():
            times[name].append(_time(fn))

    out = {"config": f"{a.clips} clips x {a.seconds:g} s x {G} SNRs = {R} rows of {m} samples against clips of {n}, 16 kHz, 1 GPU",
           "rounds": a.rounds}
    out.update({name: _stats(t) for name, t in times.items()})
    for s, D in delays.items():
        flop = useful_flop(n, m, D, R)
        rate = flop / (out[f"align_delay@{s:g}"]["median_ms"] * 1e-3)
        out[f"align_delay@{s:g}_useful_tflops"] = round(rate / 1e12, 2)
        out[f"align_delay@{s:g}_share_of_fp32_matrix_peak"] = round(rate / FP32_MATRIX_PEAK, 3)
        out[f"align_delay@{s:g}_ms_per_row"] = round(out[f"align_delay@{s:g}"]["median_ms"] / R, 4)
    out["align_shift_gb_per_s"] = round(4.0 * R * (n + n) / (out["align_shift"]["median_ms"] * 1e-3) / 1e9, 1)
    out["nsim_aligned_over_plain"] = round(out["nsim_aligned"]["median_ms"] / out["nsim_plain"]["median_ms"], 2)
    out["scipy_fft_ms_per_pair"] = round(scipy_ms, 1)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(out) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
