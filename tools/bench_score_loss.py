#!/usr/bin/env python3
"""Nomad.score() as a training loss: per-step latency of the score forward and forward+backward at config C4's shape -
a (32,1,16384) batch of estimates (T = 50) against a bank of 1000 reference embeddings - and, on their own, the two launches
of the distance stage's backward (nomad_cdist_backward: weights + the da reduction) through the library's hipEvent classes.

One line of JSON.  tools/bench_c4.py at the same --batch / --samples is the step to read it against: forward() runs two
branches (estimate and clean) where score() runs one."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nomad_amd.nomad import Nomad  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--references", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp32", help="fp32 or bf16x3 (the differentiated forward stays on fp32 buffers, its products "
                                                        "follow Engine.gemm_precision)")
    ap.add_argument("--reference-grad", action="store_true", help="differentiate the references too (adds the db reduction)")
    a = ap.parse_args()
    nmd = Nomad(weights="seeded", precision=a.precision)
    eng = nmd.engine
    g = torch.Generator().manual_seed(0)
    est0 = (0.1 * torch.randn(a.batch, 1, a.samples, generator=g)).clamp(-1, 1).cuda()
    refs = torch.randn(a.references, 256, generator=g)
    refs = (refs / refs.norm(dim=1, keepdim=True)).cuda().requires_grad_(a.reference_grad)

    def fwd():
        with torch.no_grad():
            return nmd.score(est0, refs)

    def fwd_bwd():
        est = est0.clone().requires_grad_(True)
        refs.grad = None
        nmd.score(est, refs, reduction="mean").backward()
        return est.grad

    out = {"config": f"Nomad.score() on ({a.batch},1,{a.samples}) x {a.references} references, {a.precision}, 1 GPU", "steps": a.steps,
           "reference_grad": a.reference_grad}
    for name, fn in (("forward_ms", fwd), ("forward_backward_ms", fwd_bwd)):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            r = fn()
        torch.cuda.synchronize()
        out[name] = round(1e3 * (time.perf_counter() - t0) / a.steps, 3)
        assert torch.isfinite(r).all()

    # the distance stage on its own: hipEvents around each call's launches (class pairwise_f64), nothing else on the stream
    emb = nmd.model(est0)
    up = torch.full((a.batch,), 1.0 / a.batch, dtype=torch.float64, device=emb.device)
    rd = refs.detach()
    stages = {"cdist_backward_ms": lambda: eng.cdist_backward(emb, rd, g_mean=up, want_a=True, want_b=a.reference_grad),
              "pairwise_forward_ms": lambda: eng.pairwise(emb, rd, want_matrix=False)}
    for name, fn in stages.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        eng.profile_enable(True)
        eng.profile_reset()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        prof = eng.profile_read()["pairwise_f64"]
        eng.profile_enable(False)
        assert prof["launches"] == a.steps, prof
        out[name] = round(prof["ms"] / a.steps, 4)
    out["cdist_backward_share_of_step"] = round(out["cdist_backward_ms"] / out["forward_backward_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
