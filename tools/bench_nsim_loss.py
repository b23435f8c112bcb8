#!/usr/bin/env python3
"""NSIM as a loss (``Nomad.nsim_loss``): what a forward + backward of the gammatone-spectrogram NSIM costs, next to the number alone
and to the feature loss it is meant to be added to.  A record, not a threshold: nobody had measured it, and by operation count the
backward is two to three gammatone passes plus the traffic of the stored cascade outputs (168 W bytes per frame).

Workloads: (32, 1, 16384), a training batch, and 8 x 10 s.  Legs, alternating in ONE process, median and fastest - slowest of
--rounds rounds (a round times every leg once, so drift hits all alike):

  nsim_loss            ``nomad.nsim_loss(est, clean).backward()``: two spectrograms, the map, both backward calls
  nsim                 ``nomad.nsim(est, clean)``: the number alone
  gammatone            ``Engine.gammatone`` of the estimate's rows alone: the unit the README's table counts in
  gammatone_backward   ``Engine.gammatone_backward`` alone on those rows
  forward              ``nomad.forward(est, clean).backward()``: the feature loss with its gradient

No hardware counters are collected: wall-clock times between device synchronisations only.  One JSON line per workload; --out
appends them."""
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


def _time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _stats(t):
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def run(nmd, B, n, rounds):
    eng = nmd.engine
    rng = np.random.RandomState(0)
    env = 0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * np.arange(n) / 16000.0)
    clean = torch.from_numpy((0.1 * env[None, :] * rng.uniform(-1.0, 1.0, size=(B, n))).astype(np.float32)).cuda()[:, None, :]
    est = (clean + 0.02 * torch.from_numpy(rng.randn(B, 1, n).astype(np.float32)).cuda()).requires_grad_(True)
    rows = est.detach().squeeze(1).contiguous()
    lens = [n] * B
    spec, frames = eng.gammatone(packed=(rows, lens))
    dspec = torch.ones_like(spec)

    def with_grad(loss):
        def leg():
            est.grad = None
            loss().backward()
        return leg

    legs = {
        "nsim_loss": with_grad(lambda: nmd.nsim_loss(est, clean)),
        "nsim": lambda: nmd.nsim(est.detach(), clean),
        "gammatone": lambda: eng.gammatone(packed=(rows, lens)),
        "gammatone_backward": lambda: eng.gammatone_backward(dspec, packed=(rows, lens)),
        "forward": with_grad(lambda: nmd.forward(est, clean)),
    }
    for fn in legs.values():
        fn()
    assert torch.isfinite(est.grad).all()
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(_time(fn))
    out = {"config": f"({B}, 1, {n}) fp32, 16 kHz, {frames[0]} frames per row, 1 GPU", "rounds": rounds, "counters_collected": False,
           "backward_workspace_mib": round(eng.lib.nomad_gammatone_backward_scratch_bytes(B, rows.shape[1], 16000) / 2 ** 20, 1)}
    out.update({name: _stats(t) for name, t in times.items()})
    out["nsim_loss_over_gammatone"] = round(out["nsim_loss"]["median_ms"] / out["gammatone"]["median_ms"], 2)
    out["nsim_loss_over_forward"] = round(out["nsim_loss"]["median_ms"] / out["forward"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nsim_loss_bench.jsonl"), help="append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nsim_loss.py needs a GPU: nomad_amd has no CPU path")
    nmd = Nomad(weights="seeded")
    for B, n in ((32, 16384), (8, 160000)):
        out = run(nmd, B, n, a.rounds)
        print(json.dumps(out))
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(out) + "\n")
    nmd.engine.close()


if __name__ == "__main__":
    main()
