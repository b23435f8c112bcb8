#!/usr/bin/env python3
"""The nearest-reference score (nomad_knn): two legs, alternating in ONE process, median and fastest - slowest of --rounds rounds.

Leg (a)  the distance stage at C3's shape, --rows x --references embeddings (10 000 x 1 000, D = 256), for k = 1, 8, 64:
         ``Engine.knn`` (matrix-free) against what the library could do for the same answer before it - ``Engine.pairwise(
         want_matrix=True)``, then ``torch.topk(k, largest=False)`` and ``.mean(1)`` on the 80 MB matrix - with
         ``Engine.pairwise(want_matrix=False)``, the mean over all references, printed next to them as the floor.
Leg (b)  ``Nomad.score(k=8)`` forward + backward at C4's shape, (32,1,16384) x --references, against ``Nomad.score()``, for fp32
         and bf16x3.

A round times every variant once, one after the other (so drift of the box hits all of them alike): --steps calls between two
device synchronisations, after --warmup calls of that variant.  One JSON line per leg; --out appends them to a file."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nomad_amd.nomad import Nomad  # noqa: E402


def _unit(n, d, gen):
    x = torch.randn(n, d, generator=gen)
    return (x / x.norm(dim=1, keepdim=True)).cuda()


def _time(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def _alternate(variants, rounds, steps, warmup):
    """{name: fn} -> {name: {"median_ms", "min_ms", "max_ms"}}: every round runs every variant once, in order."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(_time(fn, steps))
    return {name: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
            for name, t in times.items()}


def leg_a(eng, a, rounds, steps, warmup):
    gen = torch.Generator().manual_seed(0)
    deg, ref = _unit(a.rows, 256, gen), _unit(a.references, 256, gen)
    variants = {"pairwise_mean_floor": lambda: eng.pairwise(deg, ref, want_matrix=False)}
    for k in (1, 8, 64):
        kd, ki, sc = eng.knn(deg, ref, k)
        top = torch.topk(eng.pairwise(deg, ref, want_matrix=True)[0], k, dim=1, largest=False)
        assert torch.equal(top.values, kd), f"k={k}: the fused call and matrix + topk disagree on the distances"
        assert float((top.values.mean(1) - sc).abs().max()) < 1e-12
        variants[f"knn_k{k}"] = lambda k=k: eng.knn(deg, ref, k)
        variants[f"matrix_topk_k{k}"] = lambda k=k: torch.topk(eng.pairwise(deg, ref, want_matrix=True)[0], k, dim=1,
                                                              largest=False).values.mean(1)
    out = {"leg": "a", "config": f"Engine.knn vs pairwise(want_matrix=True) + topk + mean, {a.rows} x {a.references} x 256, 1 GPU",
           "rounds": rounds, "steps": steps}
    out.update(_alternate(variants, rounds, steps, warmup))
    return out


def leg_b(a, rounds, steps, warmup):
    out = {"leg": "b", "config": f"Nomad.score(k=8) vs Nomad.score(), forward+backward, ({a.batch},1,{a.samples}) x {a.references} "
                                 "references, 1 GPU", "rounds": rounds, "steps": steps}
    for precision in ("fp32", "bf16x3"):
        nmd = Nomad(weights="seeded", precision=precision)
        gen = torch.Generator().manual_seed(0)
        est0 = (0.1 * torch.randn(a.batch, 1, a.samples, generator=gen)).clamp(-1, 1).cuda()
        refs = _unit(a.references, 256, gen)

        def step(k):
            est = est0.clone().requires_grad_(True)
            nmd.score(est, refs, reduction="mean", k=k).backward()
            return est.grad

        assert torch.isfinite(step(8)).all()
        res = _alternate({"score": lambda: step(None), "score_k8": lambda: step(8)}, rounds, steps, warmup)
        out.update({f"{precision}_{name}": v for name, v in res.items()})
        nmd.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--references", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="ab")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn.py needs a GPU: nomad_amd has no CPU path")
    lines = []
    if "a" in a.legs:
        nmd = Nomad(weights="seeded")
        lines.append(leg_a(nmd.engine, a, a.rounds, a.steps, a.warmup))
        nmd.engine.close()
    if "b" in a.legs:
        lines.append(leg_b(a, a.rounds, a.steps, a.warmup))
    for line in lines:
        print(json.dumps(line))
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
