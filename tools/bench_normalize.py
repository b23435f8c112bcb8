#!/usr/bin/env python3
"""Loudness normalisation on the device (nomad_degrade_normalize): what it costs next to the degradations that make its rows and
next to the sweep that consumes them.

Workload: --clips clean clips of --seconds s (64 x 10 s) clipped at G levels into R = clips x G packed rows, for every R of --rows
(1344 and 1600: 21 and 25 levels).  Legs, alternating in ONE process, median and fastest - slowest of --rounds rounds (a round
times every leg once, so drift hits all alike):

  measure_R / normalize_R        ``Engine.degrade_normalize`` on the R rows: statistics alone, and in place (the second and later
                                 rounds normalise rows that already sit at the target: the same work)
  degrade_clip_R / degrade_noise_R  the calls that make R rows from the clean clips, for scale
  sweep / sweep_normalized       ``Nomad.intensity_sweep`` end to end (--snr-db and --clip levels), without and with normalize=-23
  numpy_lfilter                  the host's way to the same levels and rows, float64 ``scipy.signal.lfilter`` + numpy, over
                                 --host-rows rows (per-row time reported; it takes seconds)

Traffic floor of a normalising call: the rows read twice (the two chunk walks) and read and written once by the gain pass, 16 bytes
per sample at --hbm-gbs (the measured streaming rate of the part); measuring alone reads them twice.  One JSON line; --out appends it."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nomad_amd.nomad import Nomad  # noqa: E402


def _levels(text):
    return [float(v) for v in text.split(",") if v.strip()]


def _time(fn, sync=True):
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    if sync:
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _stats(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def numpy_normalize(rows, target=-23.0, fs=16000):
    """BS.1770-4 level and gain per row on the host -> (rows, levels)."""
    from scipy.signal import lfilter
    K = np.tan(np.pi * 1681.974450955533 / fs)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb, Q = Vh ** 0.4996667741545416, 0.7071752369554196
    a0 = 1.0 + K / Q + K * K
    b1, a1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    K, Q = np.tan(np.pi * 38.13547087602444 / fs), 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    b2, a2 = [1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    hop = fs // 10
    out, levels = np.empty_like(rows), np.empty(rows.shape[0])
    for r, row in enumerate(rows):
        xd = row.astype(np.float64)
        y = lfilter(b2, a2, lfilter(b1, a1, xd))
        c = np.add.reduceat(y * y, np.arange(0, y.shape[0] // hop * hop, hop))
        z = (c[:-3] + c[1:-2] + c[2:-1] + c[3:]) / (4.0 * hop)
        with np.errstate(divide="ignore"):
            lj = -0.691 + 10.0 * np.log10(z)
            keep = lj > -70.0
            keep &= lj > -0.691 + 10.0 * np.log10(z[keep].mean()) - 10.0
            levels[r] = -0.691 + 10.0 * np.log10(z[keep].mean())
        out[r] = xd * 10.0 ** ((target - levels[r]) / 20.0)
    return out, levels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rows", type=lambda t: [int(v) for v in t.split(",")], default=[1344, 1600])
    ap.add_argument("--noise-seconds", type=float, default=7.3)
    ap.add_argument("--clip", type=_levels, default=[5, 10, 25, 40, 60])
    ap.add_argument("--snr-db", type=_levels, default=[0, 8, 15, 25, 40])
    ap.add_argument("--references", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rows", type=int, default=32)
    ap.add_argument("--hbm-gbs", type=float, default=6290.0, help="streaming rate the traffic floor is taken at, GB/s")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_normalize.py needs a GPU: nomad_amd has no CPU path")
    nmd = Nomad(weights="seeded")
    eng = nmd.engine
    rs = np.random.RandomState(0)
    n = int(a.seconds * 16000) // 4 * 4
    host = (rs.randint(-32768, 32768, size=(a.clips, n)) * rs.uniform(0.05, 1.0, size=(a.clips, 1)) / 32768.0).astype(np.float32)
    noise_host = (0.1 * rs.randn(int(a.noise_seconds * 16000))).astype(np.float32)
    x, noise = torch.from_numpy(host).cuda(), torch.from_numpy(noise_host).cuda()
    lens = [n] * a.clips
    refs = torch.randn(a.references, 256, generator=torch.Generator().manual_seed(0))
    refs = (refs / refs.norm(dim=1, keepdim=True)).cuda()

    legs, rows_of = {}, {}
    for R in a.rows:
        G = R // a.clips
        if G * a.clips != R or not 1 <= G <= 64:
            raise SystemExit(f"--rows {R}: a multiple of --clips {a.clips} with 1 .. 64 levels per clip")
        cf, snr = list(np.linspace(1.0, 60.0, G)), list(np.linspace(0.0, 40.0, G))
        rows, row_lens, _ = eng.degrade_clip(x, cf, lengths=lens)
        rows_of[R] = (rows, row_lens)
        legs[f"measure_{R}"] = lambda p=(rows, row_lens): eng.degrade_normalize(packed=p, measure_only=True)
        legs[f"normalize_{R}"] = lambda p=(rows, row_lens): eng.degrade_normalize(packed=p, inplace=True)
        legs[f"degrade_clip_{R}"] = lambda cf=cf: eng.degrade_clip(x, cf, lengths=lens)
        legs[f"degrade_noise_{R}"] = lambda snr=snr: eng.degrade_noise(x, noise, snr, lengths=lens)
    legs["sweep"] = lambda: nmd.intensity_sweep(x, refs, noise=noise, snr_db=a.snr_db, clip_factor=a.clip)
    legs["sweep_normalized"] = lambda: nmd.intensity_sweep(x, refs, noise=noise, snr_db=a.snr_db, clip_factor=a.clip, normalize=-23.0)
    # the rows the legs time are the rows the host makes
    rows, row_lens = rows_of[a.rows[0]]
    small, small_levels = numpy_normalize(rows[:2].cpu().numpy())
    got, _, stats = eng.degrade_normalize(packed=(rows[:2].contiguous(), row_lens[:2]))
    assert np.abs(stats[:, 0].cpu().numpy() - small_levels).max() <= 1e-9 and np.allclose(got.cpu().numpy(), small, rtol=1e-6, atol=1e-7)
    with contextlib.redirect_stdout(io.StringIO()):      # intensity_stats prints per degradation
        for fn in legs.values():
            fn()
        times = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                times[name].append(_time(fn))
    host_rows = rows[:a.host_rows].cpu().numpy()
    host_time = _time(lambda: numpy_normalize(host_rows), sync=False)
    out = {"config": f"{a.clips} clips x {a.seconds:g} s, rows {a.rows}, sweep of {len(a.snr_db)} SNRs + {len(a.clip)} clip factors, fp32, 1 GPU",
           "rounds": a.rounds, "hbm_gbs": a.hbm_gbs}
    out.update({name: _stats(t) for name, t in times.items()})
    out["numpy_lfilter_ms_per_row"] = round(host_time / host_rows.shape[0], 3)
    for R in a.rows:
        floor_ms = 16.0 * R * n / (a.hbm_gbs * 1e9) * 1e3
        out[f"normalize_{R}_floor_ms"] = round(floor_ms, 3)
        out[f"normalize_{R}_fraction_of_floor"] = round(floor_ms / out[f"normalize_{R}"]["median_ms"], 4)
        out[f"measure_{R}_fraction_of_floor"] = round(floor_ms / 2 / out[f"measure_{R}"]["median_ms"], 4)
        out[f"numpy_over_normalize_{R}"] = round(out["numpy_lfilter_ms_per_row"] * R / out[f"normalize_{R}"]["median_ms"], 1)
    out["sweep_normalized_over_sweep"] = round(out["sweep_normalized"]["median_ms"] / out["sweep"]["median_ms"], 4)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(out) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
