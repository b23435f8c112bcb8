#!/usr/bin/env python3
"""Config C4 (BASELINE.json configs[3]): nomad.forward() as an auxiliary loss inside a training step -
per-step latency of loss forward and forward+backward at the reference example's shapes
(nomad_loss_test.py: batch 32, clips zero-padded/cropped to 16384 samples, T = 50)."""
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp32", help="bf16x3: the no-gradient branch(es) run the split-bf16 forward")
    ap.add_argument("--lengths", default="", help="utterance lengths in seconds: a,b,... (one per clip) or uniform:lo:hi:seed; --samples is "
                                                  "then the padded width (at least the longest)")
    ap.add_argument("--pad-mode", choices=("batch", "exact"), default="exact",
                    help="with --lengths: 'exact' passes them to nomad.forward, 'batch' runs the zero-padded equal-length loss")
    ap.add_argument("--layers", type=int, default=13, help="nomad_loss.L: the first K of the 13 terms (12 transformer layers + the embedding); "
                                                           "below 13 the encoder stops behind layer K, forward and backward")
    ap.add_argument("--reduction", choices=("mean", "none"), default="mean", help="'none': one loss per utterance (summed for the backward)")
    a = ap.parse_args()
    lens = None
    if a.lengths:
        if a.lengths.startswith("uniform:"):
            lo, hi, seed = a.lengths.split(":")[1:]
            rng = torch.Generator().manual_seed(int(seed))
            secs = (float(lo) + (float(hi) - float(lo)) * torch.rand(a.batch, generator=rng)).tolist()
        else:
            secs = [float(x) for x in a.lengths.split(",")]
        assert len(secs) == a.batch, "--lengths: one value per clip"
        lens = [int(x * 16000) for x in secs]
        a.samples = max(a.samples, max(lens))
    nmd = Nomad(weights="seeded", precision=a.precision)
    nmd.nomad_loss.L = a.layers
    g = torch.Generator().manual_seed(0)
    clean = (0.1 * torch.randn(a.batch, 1, a.samples, generator=g)).clamp(-1, 1).cuda()
    est0 = (clean + 0.02 * torch.randn(a.batch, 1, a.samples, generator=g).cuda()).clamp(-1, 1)
    kw = {}
    if lens is not None:
        for i, n in enumerate(lens):   # zero padding behind every utterance (what a caller without lengths has to feed)
            clean[i, 0, n:] = 0.0
            est0[i, 0, n:] = 0.0
        if a.pad_mode == "exact":
            kw = {"lengths": lens}
    if a.reduction != "mean":   # (the default call keeps the signature every earlier commit has: A/B runs against them)
        kw["reduction"] = a.reduction

    def fwd():
        return nmd.forward(est0, clean, **kw)

    def fwd_bwd():
        est = est0.clone().requires_grad_(True)
        loss = nmd.forward(est, clean, **kw)
        loss.sum().backward() if loss.dim() else loss.backward()
        return est.grad

    out = {"config": f"C4: nomad.forward() on 2x({a.batch},1,{a.samples}), {a.precision}, 1 GPU", "steps": a.steps,
           "layers": a.layers, "reduction": a.reduction}
    if lens is not None:
        from nomad_amd.weights import num_frames
        Ts, Tp = [num_frames(n) for n in lens], num_frames(a.samples)
        out.update(lengths=a.lengths, pad_mode=a.pad_mode, frames_exact_over_padded=sum(Ts) / (Tp * len(Ts)),
                   frames2_exact_over_padded=sum(t * t for t in Ts) / (Tp * Tp * len(Ts)))
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
