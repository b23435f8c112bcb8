#!/usr/bin/env python3
"""Scores over time on one batch: what the windowed head costs on top of the plain forward, and what the same windows cost as
separate clips.

  (a) ``embed_ragged``           one embedding per clip (the plain forward and head)
  (b) ``embed_windows_ragged``   one embedding per window of ``--win`` frames every ``--hop``, pooled from ONE forward
  (c) ``embed_ragged`` over the same windows cut out as clips of their own: excerpts of ``win * 320 + 80`` samples every
      ``hop * 320`` (gathered once, outside the timed region), about win / hop forwards' worth of audio

Prints one JSON line: the three times (ms, mean of ``--reps`` alternating rounds after a warm-up round of every shape, and
the fastest / slowest round), and the largest |difference| between the embeddings of (b) and (c).  That difference is a
semantic number, not an error: in (b) attention and the first conv layer's GroupNorm statistics saw the whole clip, in (c)
only the excerpt.

    python tools/bench_windows.py --clips 32 --seconds 30 --precision bf16
    python tools/bench_windows.py --clips 32 --seconds 4 --precision fp32
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nomad_amd.engine import Engine  # noqa: E402
from nomad_amd.weights import num_frames, num_windows, seeded_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--precision", default="bf16", choices=("fp32", "bf16x3", "bf16"))
    ap.add_argument("--win", type=int, default=200, help="frames per window (200 = 4 s)")
    ap.add_argument("--hop", type=int, default=100, help="frames between window starts")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_windows.py needs a GPU: there is no CPU path")

    n = int(round(a.seconds * 16000))
    T = num_frames(n)
    W = num_windows(T, a.win, a.hop)
    eng = Engine(seeded_state_dict(0), 0)
    g = torch.Generator().manual_seed(0)
    wav = (0.1 * torch.randn(a.clips, n, generator=g)).clamp(-1, 1).cuda()
    waves = [w for w in wav]
    span = min(a.win, T) * 320 + 80                       # the samples a window's frames see
    cut = wav.unfold(1, span, a.hop * 320)[:, :W].contiguous().view(a.clips * W, span) if T > a.win else wav
    assert cut.shape[0] == a.clips * W and num_frames(span) == min(a.win, T)
    lens_c = [cut.shape[1]] * cut.shape[0]

    runs = {"a_embed_ragged": lambda: eng.embed_ragged(waves, precision=a.precision),
            "b_embed_windows_ragged": lambda: eng.embed_windows_ragged(waves, a.win, a.hop, precision=a.precision)[0],
            "c_windows_as_clips": lambda: eng.embed_ragged(None, precision=a.precision, packed=(cut, lens_c))}
    last = {}
    for name, fn in runs.items():                         # warm-up: every shape once
        last[name] = fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(a.reps):                               # alternating, so that drift hits the three alike
        for name, fn in runs.items():
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    b, c = last["b_embed_windows_ragged"], last["c_windows_as_clips"]
    assert b.shape == c.shape == (a.clips * W, 256)
    out = {"tool": "bench_windows", "clips": a.clips, "seconds": a.seconds, "precision": a.precision, "frames": T, "win": a.win,
           "hop": a.hop, "windows": a.clips * W, "reps": a.reps}
    for name, ts in times.items():
        out[name + "_ms"] = round(sum(ts) / len(ts), 3)
        out[name + "_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
    out["b_minus_a_ms"] = round(out["b_embed_windows_ragged_ms"] - out["a_embed_ragged_ms"], 3)
    out["c_over_a"] = round(out["c_windows_as_clips_ms"] / out["a_embed_ragged_ms"], 2)
    out["max_abs_diff_b_vs_c"] = float((b - c).abs().max())
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
