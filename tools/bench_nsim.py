#!/usr/bin/env python3
"""NSIM on the device (nomad_gammatone + nomad_nsim) and the triplets mined from it: what the gammatone recurrences, the similarity
map and the whole of ``Nomad.mine_triplets`` cost, next to the forward that consumes the rows.  A record, not a threshold.

Workload: --clips clean clips of --seconds s (64 x 10 s) with noise at the reference's 25 test SNRs (config_audio_degrader.yaml:
``noise_test``) in ONE call (G = 25 <= 64): 1600 packed rows.  Legs, alternating in ONE process, median and fastest - slowest of
--rounds rounds (a round times every leg once, so drift hits all alike):

  gammatone          ``Engine.gammatone`` of the 1600 degraded rows: 497 frames x 21 bands x 1280 steps each
  nsim               ``Engine.nsim_of_spectrograms`` on those spectrograms and the clean clips' (B = 64, G = 25)
  mine_triplets      ``Nomad.mine_triplets`` end to end: degrade, normalise to -23 LUFS, both spectrograms, NSIM, the table's round
                     trip, sampling (N = 3 per clip) and the gather of the three branches
  forward_fp32       ``Engine.embed_ragged`` (fp32) of the degraded rows of --context-clips clips x 25 SNRs, for scale
  numpy              ``tests/nsim_ref.py``, the long-double restatement, on --host-seconds s of one pair (it takes seconds per row)

``gammatone`` also reports its share of the float64 vector rate: 16 multiply-adds = 32 FLOP per sample, band and frame, against
78.6 TFLOP/s (the figure the ``pairwise`` rows of profiles/NOTEBOOK.md and README.md use).  Every leg is also reported per row of
--seconds s.  One JSON line; --out appends it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import nsim_ref  # noqa: E402
from nomad_amd.nomad import Nomad  # noqa: E402

REFERENCE_TEST_SNRS = [1, 3, 4, 6, 9, 10, 12, 14, 16, 19, 20, 22, 24, 26, 28, 30, 32, 33, 35, 37, 39, 42, 44, 46, 50]
FP64_VECTOR_PEAK = 78.6e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--levels", type=lambda t: [float(v) for v in t.split(",")], default=REFERENCE_TEST_SNRS)
    ap.add_argument("--context-clips", type=int, default=8)
    ap.add_argument("--host-seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nsim.py needs a GPU: nomad_amd has no CPU path")
    nmd = Nomad(weights="seeded")
    eng = nmd.engine
    G = len(a.levels)
    n = int(a.seconds * 16000) // 4 * 4
    rng = np.random.RandomState(0)
    env = 0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * np.arange(n) / 16000.0)
    host = (0.1 * env[None, :] * rng.uniform(-1.0, 1.0, size=(a.clips, n))).astype(np.float32)
    noise_host = (0.1 * rng.randn(n)).astype(np.float32)
    x = torch.from_numpy(host).cuda()
    noise = torch.from_numpy(noise_host).cuda()
    lens = [n] * a.clips

    rows, lens_rep, _ = eng.degrade_noise(x, noise, a.levels, lengths=lens)
    spec_ref, frames = eng.gammatone(packed=(x, lens))
    spec_deg, _ = eng.gammatone(packed=(rows, lens_rep))
    spec_ref, spec_deg = spec_ref.clone(), spec_deg.clone()
    xc = x[:a.context_clips].contiguous()
    rows_f = eng.degrade_noise(xc, noise, a.levels, lengths=lens[:a.context_clips])
    rows_f = (rows_f[0].clone(), rows_f[1])

    # the numbers the legs time are the numbers the restatement gives
    hn = int(a.host_seconds * 16000)
    t0 = time.perf_counter()
    want = nsim_ref.nsim(host[0, :hn], rows[G // 2, :hn].cpu().numpy())[0]
    host_ms = 1e3 * (time.perf_counter() - t0)
    got = float(eng.nsim((x[:1, :hn].contiguous(), [hn]), (rows[G // 2:G // 2 + 1, :hn].contiguous(), [hn]), 1)[0][0, 0])
    assert abs(got - want) <= 1e-10, (got, want)

    mined = {}

    def mine():
        mined["out"] = nmd.mine_triplets(x, noise=noise, snr_db=a.levels, normalize=-23.0, lengths=lens, N=3, seed=0)

    legs = {
        "gammatone": lambda: eng.gammatone(packed=(rows, lens_rep)),
        "nsim": lambda: eng.nsim_of_spectrograms(spec_ref, spec_deg, frames, G),
        "mine_triplets": mine,
        "forward_fp32": lambda: eng.embed_ragged(None, precision="fp32", packed=rows_f),
    }
    rows_of = {"gammatone": a.clips * G, "nsim": a.clips * G, "mine_triplets": a.clips * G, "forward_fp32": a.context_clips * G}
    for fn in legs.values():
        fn()
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, fn in legs.items():
            times[name].append(_time(fn))

    info = mined["out"][3]
    out = {"config": f"{a.clips} clips x {a.seconds:g} s x {G} SNRs = {a.clips * G} rows, 16 kHz, {frames[0]} frames per row, 1 GPU",
           "rounds": a.rounds, "rows": rows_of, "triplets_mined": int(len(info["triplets"]["clip"])), "draws_dropped": int(info["dropped"]),
           "nsim_at_snr": {str(v): round(float(s), 4) for v, s in zip(a.levels, info["nsim"].mean(axis=0))}}
    out.update({name: _stats(t) for name, t in times.items()})
    for name in legs:
        out[f"{name}_ms_per_row"] = round(out[name]["median_ms"] / rows_of[name], 4)
    flop = 32.0 * a.clips * G * frames[0] * 21 * 1280
    out["gammatone_tflops_fp64"] = round(flop / (out["gammatone"]["median_ms"] * 1e-3) / 1e12, 2)
    out["gammatone_share_of_fp64_vector_peak"] = round(flop / (out["gammatone"]["median_ms"] * 1e-3) / FP64_VECTOR_PEAK, 3)
    out["gammatone_audio_seconds_per_s"] = round(a.clips * G * a.seconds / (out["gammatone"]["median_ms"] * 1e-3), 0)
    out["numpy_ms_per_row"] = round(host_ms * n / hn / 2.0, 1)       # (the pair is two spectrograms: per row, one)
    out["forward_over_gammatone_per_row"] = round(out["forward_fp32_ms_per_row"] / out["gammatone_ms_per_row"], 2)
    out["numpy_over_gammatone_per_row"] = round(out["numpy_ms_per_row"] / out["gammatone_ms_per_row"], 0)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(out) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
