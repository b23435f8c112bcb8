#!/usr/bin/env python3
"""Degradations on the device (nomad_degrade_noise / nomad_degrade_clip): what a sweep costs next to the forward that consumes it.

Workload: --clips clean clips of --seconds s (64 x 10 s), --clip clip factors and --snr-db SNRs (pass the lists of the sweep you
mean to run; the defaults are the five levels of the CLI's example), one noise recording of --noise-seconds s.  Legs, alternating
in ONE process, median and fastest - slowest of --rounds rounds (a round times every leg once, so drift hits all alike):

  degrade_clip / degrade_noise   ``Engine.degrade_*`` alone on the packed device batch: all clips, all levels, one call
  forward_clip / forward_noise   the fp32 ragged forward of the same B G rows, in parts of at most --max-batch-samples samples
  sweep                          ``Nomad.intensity_sweep`` end to end on the device-resident clips (both degradations)
  numpy_clip / numpy_noise       the host's way to the same rows, timed without file I/O: ``np.percentile`` + clamp, and the float64
                                 mix (--host-rounds rounds; they take seconds)

One JSON line: the legs, each degrade leg as a share of the forward of its rows and as a ratio to its numpy leg; --out appends it."""
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


def numpy_clip(x, factors):
    out = np.empty((x.shape[0] * len(factors), x.shape[1]), dtype=np.float32)
    for b, row in enumerate(x):
        xd = row.astype(np.float64)
        ps = [p for cf in factors for p in (cf / 2, 100 - cf / 2)]
        thr = np.percentile(xd, ps)
        for g in range(len(factors)):
            out[b * len(factors) + g] = np.clip(xd, thr[2 * g], thr[2 * g + 1])
    return out


def numpy_noise(x, noise, snrs):
    out = np.empty((x.shape[0] * len(snrs), x.shape[1]), dtype=np.float32)
    s = np.resize(noise.astype(np.float64), x.shape[1])
    sp = np.sqrt(np.mean(s ** 2))
    for b, row in enumerate(x):
        xd = row.astype(np.float64)
        xp = np.sqrt(np.mean(xd ** 2))
        for g, snr in enumerate(snrs):
            out[b * len(snrs) + g] = xd + (xp / 10 ** (snr / 10)) / sp * s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--noise-seconds", type=float, default=7.3)
    ap.add_argument("--clip", type=_levels, default=[5, 10, 25, 40, 60])
    ap.add_argument("--snr-db", type=_levels, default=[0, 8, 15, 25, 40])
    ap.add_argument("--references", type=int, default=100)
    ap.add_argument("--max-batch-samples", type=int, default=256 * 64000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_degrade.py needs a GPU: nomad_amd has no CPU path")
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

    def forward(rows, row_lens):
        step = max(1, a.max_batch_samples // n)
        for lo in range(0, rows.shape[0], step):
            eng.embed_ragged(None, packed=(rows[lo:lo + step], row_lens[lo:lo + step]))

    rows_c, lens_c, _ = eng.degrade_clip(x, a.clip, lengths=lens)
    rows_n, lens_n, _ = eng.degrade_noise(x, noise, a.snr_db, lengths=lens)
    legs = {"degrade_clip": lambda: eng.degrade_clip(x, a.clip, lengths=lens),
            "degrade_noise": lambda: eng.degrade_noise(x, noise, a.snr_db, lengths=lens),
            "forward_clip": lambda: forward(rows_c, lens_c),
            "forward_noise": lambda: forward(rows_n, lens_n),
            "sweep": lambda: nmd.intensity_sweep(x, refs, noise=noise, snr_db=a.snr_db, clip_factor=a.clip,
                                                 max_batch_samples=a.max_batch_samples)}
    # the rows the legs time are the rows numpy makes (thresholds one float64 rounding apart, see tests/test_degrade_host.py)
    small = numpy_clip(host[:2], a.clip)
    assert np.abs(rows_c[:2 * len(a.clip)].cpu().numpy() - small).max() <= 2.0 ** -23
    small = numpy_noise(host[:2], noise_host, a.snr_db)
    assert np.allclose(rows_n[:2 * len(a.snr_db)].cpu().numpy(), small, rtol=1e-6, atol=1e-7)
    with contextlib.redirect_stdout(io.StringIO()):      # intensity_stats prints per degradation
        for fn in legs.values():
            fn()
        times = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                times[name].append(_time(fn))
    host_legs = {"numpy_clip": lambda: numpy_clip(host, a.clip), "numpy_noise": lambda: numpy_noise(host, noise_host, a.snr_db)}
    host_times = {name: [_time(fn, sync=False) for _ in range(a.host_rounds)] for name, fn in host_legs.items()}
    out = {"config": f"{a.clips} clips x {a.seconds:g} s, {len(a.clip)} clip factors, {len(a.snr_db)} SNRs, fp32, 1 GPU",
           "clip": a.clip, "snr_db": a.snr_db, "rounds": a.rounds, "host_rounds": a.host_rounds}
    out.update({name: _stats(t) for name, t in {**times, **host_times}.items()})
    med = {name: out[name]["median_ms"] for name in list(times) + list(host_times)}
    for kind in ("clip", "noise"):
        out[f"degrade_{kind}_share_of_forward"] = round(med[f"degrade_{kind}"] / med[f"forward_{kind}"], 5)
        out[f"numpy_{kind}_over_degrade_{kind}"] = round(med[f"numpy_{kind}"] / med[f"degrade_{kind}"], 1)
    out["sweep_over_forwards"] = round(med["sweep"] / (med["forward_clip"] + med["forward_noise"]), 4)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(out) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
