#!/usr/bin/env python3
"""Timings of the evaluation experiments' GPU stages (reported in profiles/NOTEBOOK.md, not gated by anything):

* ``paired_distance(a, b)`` against ``cdist(a, b)[0].diagonal()`` at N = 10 000, D = 256 and 768 (what quality_fr needs against
  what the reference computes: the whole N x N float64 matrix);
* ``cdist`` at 10 000 x 1 000 x 768 against ``pairwise`` at 10 000 x 1 000 x 256 - the stage is fp64-VALU bound, so the model is
  3 x the D = 256 time;
* the feature forward (``embed_features``) against the embedding forward (``embed``) on bench.py's batch (256 clips of 4 s), per
  precision, alternating the two in one process.

Device time per call from events on the launch stream, every shape warmed up first; each figure is the median of
``--repeats`` windows of ``--iters`` calls, with the spread (min .. max) next to it.  Prints one JSON line.
Usage: python tools/bench_eval.py [--clips 256] [--seconds 4] [--iters 20] [--repeats 5] [--skip-forward]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nomad_amd.engine import Engine  # noqa: E402
from nomad_amd.weights import seeded_state_dict  # noqa: E402


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(fns, iters, repeats, warmup=3):
    """{name: {ms, min, max}} for several callables, their windows alternating (A B A B ...)."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(window(fn, iters))
    return {k: {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-forward", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_eval.py needs an MI355X: there is nothing to time without one")
    eng = Engine(seeded_state_dict(0), 0)
    g = torch.Generator().manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats}

    N = 10000
    for D in (256, 768):
        a, b = torch.randn(N, D, generator=g).cuda(), torch.randn(N, D, generator=g).cuda()
        same = bool(torch.equal(eng.paired_distance(a, b), eng.cdist(a, b)[0].diagonal()))
        r = measure({"paired_distance": lambda: eng.paired_distance(a, b),
                     "cdist_diagonal": lambda: eng.cdist(a, b)[0].diagonal()}, args.iters, args.repeats)
        r["same_bits"] = same
        r["matrix_bytes_avoided"] = N * N * 8
        out[f"paired_N{N}_D{D}"] = r
        del a, b

    deg256, ref256 = torch.randn(N, 256, generator=g).cuda(), torch.randn(1000, 256, generator=g).cuda()
    deg768, ref768 = torch.randn(N, 768, generator=g).cuda(), torch.randn(1000, 768, generator=g).cuda()
    r = measure({"pairwise_256": lambda: eng.pairwise(deg256, ref256), "cdist_256": lambda: eng.cdist(deg256, ref256),
                 "cdist_768": lambda: eng.cdist(deg768, ref768)}, args.iters, args.repeats)
    r["model_768_ms"] = round(3 * r["pairwise_256"]["ms"], 4)     # fp64-VALU bound: three times the k loop
    r["fp64_lane_ops_per_s_768"] = round(N * 1000 * 768 * 2 / r["cdist_768"]["ms"] * 1e3, 1)
    out["cdist_10000x1000"] = r
    del deg256, ref256, deg768, ref768

    if not args.skip_forward:
        n = int(args.seconds * 16000)
        wav = (0.1 * torch.randn(args.clips, n, generator=g)).clamp(-1, 1).cuda()
        fwd = {"fp32": eng.embed, "bf16x3": eng.embed_bf16x3, "bf16": eng.embed_bf16}
        for precision, embed in fwd.items():
            r = measure({"embed": lambda: embed(wav), "embed_features": lambda: eng.embed_features(wav, precision=precision)},
                        max(2, args.iters // 4), args.repeats, warmup=2)
            r["clips"], r["samples"] = args.clips, n
            r["features_over_embed"] = round(r["embed_features"]["ms"] / r["embed"]["ms"], 4)
            out[f"forward_{precision}"] = r
    torch.cuda.synchronize()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
