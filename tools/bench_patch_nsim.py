#!/usr/bin/env python3
"""Patch-wise NSIM on the device (nomad_nsim_patches): what the activity gate, the patch search and the selection cost next to the
whole-clip map and next to the spectrograms they all read.  A record, not a threshold: no target was fixed in advance.

Workload: --clips clean clips of --seconds s (64 x 10 s, 497 frames each), each with noise at the reference's 25 test SNRs (G = 25):
1600 rows, at --patch / --search frames (20 / 60: 0.4 s patches searched within 1.2 s, 24 patches of up to 121 candidates per row).
The spectrograms are made once, ahead of the timing.  Legs, alternating in ONE process, median and fastest - slowest of --rounds
rounds (a round times every leg once, so drift hits all alike):

  nsim_patches       ``Engine.nsim_patches_of_spectrograms``: activity, candidates, selection and the band values
  nsim               ``Engine.nsim_of_spectrograms`` of the same rows: the whole-clip map, one cell per (frame, band)
  gammatone          ``Engine.gammatone`` of the 1600 degraded rows: what either measure needs first

The patch stage also reports its float64 rate counted as cells x candidates - every candidate evaluates patch x 21 map cells - in
G cells / s, the same count for the whole-clip map (frames x 21 cells per row), and the ratio of the two times.  One JSON line;
--out appends it."""
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

from nomad_amd.nomad import Nomad  # noqa: E402

REFERENCE_TEST_SNRS = [1, 3, 4, 6, 9, 10, 12, 14, 16, 19, 20, 22, 24, 26, 28, 30, 32, 33, 35, 37, 39, 42, 44, 46, 50]


def _time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _stats(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--levels", type=lambda t: [float(v) for v in t.split(",")], default=REFERENCE_TEST_SNRS)
    ap.add_argument("--patch", type=int, default=20)
    ap.add_argument("--search", type=int, default=60)
    ap.add_argument("--vad-db", dest="vad_db", type=float, default=40.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_patch_nsim.py needs a GPU: nomad_amd has no CPU path")
    nmd = Nomad(weights="seeded")
    eng = nmd.engine
    G = len(a.levels)
    n = int(a.seconds * 16000) // 4 * 4
    R = a.clips * G
    rng = np.random.RandomState(0)
    env = 0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * np.arange(n) / 16000.0)
    x = torch.from_numpy((0.1 * env[None, :] * rng.uniform(-1.0, 1.0, size=(a.clips, n))).astype(np.float32)).cuda()
    noise = torch.from_numpy((0.1 * rng.randn(n)).astype(np.float32)).cuda()
    lens = [n] * a.clips
    rows, lens_rep, _ = eng.degrade_noise(x, noise, a.levels, lengths=lens)
    spec_ref, frames = eng.gammatone(packed=(x, lens))
    spec_deg, dframes = eng.gammatone(packed=(rows, lens_rep))
    spec_ref, spec_deg = spec_ref.clone(), spec_deg.clone()
    ratio, need = 10.0 ** (-a.vad_db / 10.0), a.patch

    res = eng.nsim_patches_of_spectrograms(spec_ref, spec_deg, frames, dframes, G, a.patch, a.search, ratio, need, want_cand=True)
    whole = eng.nsim_of_spectrograms(spec_ref, spec_deg, frames, G)[0]
    torch.cuda.synchronize()
    kept = int((res["offsets"] >= 0).sum())
    candidates = int(torch.isfinite(res["cand"]).sum())
    assert kept > 0 and bool(torch.isfinite(res["nsim"]).all()), "the workload keeps no patch"
    patch_mean, whole_mean = float(res["nsim"].mean()), float(whole.mean())
    del res

    legs = {"nsim_patches": lambda: eng.nsim_patches_of_spectrograms(spec_ref, spec_deg, frames, dframes, G, a.patch, a.search, ratio, need),
            "nsim": lambda: eng.nsim_of_spectrograms(spec_ref, spec_deg, frames, G),
            "gammatone": lambda: eng.gammatone(packed=(rows, lens_rep))}
    for fn in legs.values():
        fn()
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, fn in legs.items():
            times[name].append(_time(fn))

    out = {"config": f"{a.clips} clips x {a.seconds:g} s x {G} SNRs = {R} rows of {frames[0]} frames, patch {a.patch} / search {a.search} frames, "
                     f"vad {a.vad_db:g} dB, 16 kHz, 1 GPU", "rounds": a.rounds}
    out.update({name: _stats(t) for name, t in times.items()})
    cells = candidates * a.patch * 21
    out["kept_patches"], out["candidates"] = kept, candidates
    out["nsim_patches_gcells_per_s"] = round(cells / (out["nsim_patches"]["median_ms"] * 1e-3) / 1e9, 2)
    out["nsim_gcells_per_s"] = round(sum(dframes) * 21 / (out["nsim"]["median_ms"] * 1e-3) / 1e9, 3)
    out["nsim_patches_over_nsim"] = round(out["nsim_patches"]["median_ms"] / out["nsim"]["median_ms"], 2)
    out["nsim_patches_over_gammatone"] = round(out["nsim_patches"]["median_ms"] / out["gammatone"]["median_ms"], 2)
    out["nsim_patches_ms_per_row"] = round(out["nsim_patches"]["median_ms"] / R, 4)
    out["mean_nsim_patches"], out["mean_nsim"] = round(patch_mean, 4), round(whole_mean, 4)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(out) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
