#!/usr/bin/env python3
"""Nomad.score_windows() as a training loss: per-step latency of its forward and forward+backward next to Nomad.score() on the
same batch, the two ALTERNATING round by round in one process so that both see the same clocks and the same neighbours - and,
on their own, the two backwards over one set of saved activations (``embed_windows_backward`` against ``embed_backward``),
whose difference is what the windowed head's two launches cost over ``head_bwd_kernel``.

Shapes (--shape): "c4" = a (32,1,16384) batch against 1000 references with windows of 0.5 s every 0.25 s (3 windows per clip);
"10s" = 8 clips of 10 s with windows of 1 s every 0.5 s (18 windows per clip).  Every figure is the median over --rounds rounds
of --steps steps each, with the rounds' minimum and maximum next to it.  One line of JSON, printed and appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nomad_amd.nomad import Nomad, window_frames  # noqa: E402
from nomad_amd.weights import num_frames, num_windows  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"c4": (32, 16384, 0.5, 0.25), "10s": (8, 160000, 1.0, 0.5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c4", choices=sorted(SHAPES))
    ap.add_argument("--references", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp32", help="fp32 or bf16x3 (the differentiated forward stays on fp32 buffers, its products "
                                                        "follow Engine.gemm_precision)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_loss_bench.jsonl"))
    a = ap.parse_args()
    B, N, window_s, hop_s = SHAPES[a.shape]
    win, hop = window_frames(window_s, hop_s)
    nmd = Nomad(weights="seeded", precision=a.precision)
    eng = nmd.engine
    g = torch.Generator().manual_seed(0)
    est0 = (0.1 * torch.randn(B, 1, N, generator=g)).clamp(-1, 1).cuda()
    refs = torch.randn(a.references, 256, generator=g)
    refs = (refs / refs.norm(dim=1, keepdim=True)).cuda()

    def score_fwd():
        with torch.no_grad():
            return nmd.score(est0, refs)

    def windows_fwd():
        with torch.no_grad():
            return nmd.score_windows(est0, refs, window_s, hop_s)[0]

    def score_step():
        est = est0.clone().requires_grad_(True)
        nmd.score(est, refs, reduction="mean").backward()
        return est.grad

    def windows_step():
        est = est0.clone().requires_grad_(True)
        nmd.score_windows(est, refs, window_s, hop_s, reduction="mean")[0].backward()
        return est.grad

    # the backwards on their own, over the activations of one training-mode forward each
    x = est0[:, 0].contiguous()
    emb, layers, saved = eng.embed_train(x)
    emb_w, counts, layers_w, saved_w = eng.embed_train_windows(x, win, hop)
    demb, demb_w = torch.randn_like(emb), torch.randn_like(emb_w)

    timed = {"score_forward_ms": score_fwd, "windows_forward_ms": windows_fwd, "score_forward_backward_ms": score_step,
             "windows_forward_backward_ms": windows_step,
             "score_backward_ms": lambda: eng.embed_backward(x, layers, saved, None, demb),
             "windows_backward_ms": lambda: eng.embed_windows_backward(x, layers_w, saved_w, demb_w, win, hop)}
    for fn in timed.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in timed}
    for _ in range(a.rounds):                    # alternating: every round times each of them once, in turn
        for name, fn in timed.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                r = fn()
            torch.cuda.synchronize()
            samples[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
            assert torch.isfinite(r).all()

    T = num_frames(N)
    out = {"config": f"Nomad.score_windows() next to Nomad.score() on ({B},1,{N}) x {a.references} references, windows of {window_s} s every "
                     f"{hop_s} s ({win} / {hop} frames of {T}: {num_windows(T, win, hop)} per clip, {sum(counts)} in all), {a.precision}, 1 GPU",
           "steps": a.steps, "rounds": a.rounds}
    for name, v in samples.items():
        out[name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    med = {k: statistics.median(v) for k, v in samples.items()}
    out["windows_over_score_forward_backward"] = round(med["windows_forward_backward_ms"] / med["score_forward_backward_ms"], 4)
    out["windowed_head_backward_extra_ms"] = round(med["windows_backward_ms"] - med["score_backward_ms"], 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
