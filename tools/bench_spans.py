#!/usr/bin/env python3
"""Scores over spans: what the span head costs next to the windowed head it generalises, on the same box in the same process.

Legs, ALTERNATING round by round (median, fastest and slowest of ``--rounds`` rounds of ``--steps`` steps after a warm-up):

  embed_ragged            --clips clips of --seconds s in --precision, the plain forward and head
  embed_windows_ragged    the windowed head at --win / --hop frames (4 s / 2 s)
  embed_spans_windows     ``embed_spans_ragged`` with the identical rows, one span each: the same loads plus the table lookup
  embed_spans_active      ``embed_spans_ragged`` with ONE row per clip over its active spans (every other second of the clip is
                          attenuated by 80 dB; the table comes from ``Nomad.active_spans``, outside the timed region)
  frame_energy            ``Engine.frame_energy`` alone
  active_spans            energies, their trip to the host and the rule: what ``predict_spans(active_db=...)`` adds per batch
  score_windows_fb /      ``Nomad.score_windows`` and ``Nomad.score_spans`` with the same rows, forward + backward, on a
  score_spans_fb          (32,1,16384) batch against --references references (windows of 0.5 s every 0.25 s)
  predict_segments /      the two file pipelines over the same folders (--nmr / --deg, default: the golden wavs), 1 s windows
  predict_spans_active    against one active-speech row per file

One line of JSON, printed and appended to --out.

    python tools/bench_spans.py
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nomad_amd.nomad import Nomad, span_table, window_frames  # noqa: E402
from nomad_amd.weights import num_frames, num_windows  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--precision", default="bf16", choices=("fp32", "bf16x3", "bf16"))
    ap.add_argument("--win", type=int, default=200, help="frames per window (200 = 4 s)")
    ap.add_argument("--hop", type=int, default=100, help="frames between window starts")
    ap.add_argument("--references", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nmr", default=os.path.join(ROOT, "tests", "golden", "wavs", "nmr-data"))
    ap.add_argument("--deg", default=os.path.join(ROOT, "tests", "golden", "wavs", "test-data"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spans_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spans.py needs a GPU: there is no CPU path")

    nmd = Nomad(weights="seeded", precision=a.precision)
    eng = nmd.engine
    g = torch.Generator().manual_seed(0)
    n = int(round(a.seconds * 16000))
    T = num_frames(n)
    wav = (0.1 * torch.randn(a.clips, n, generator=g)).clamp(-1, 1)
    for s in range(1, int(a.seconds), 2):                       # every other second: 80 dB down
        wav[:, s * 16000:(s + 1) * 16000] *= 1e-4
    wav = wav.cuda()
    waves = [w for w in wav]
    W = num_windows(T, a.win, a.hop)
    nw = min(a.win, T)
    win_table, _ = span_table([[[(k * a.hop, k * a.hop + nw)] for k in range(W)] for _ in waves], [T] * a.clips, unit="frames")
    active = nmd.active_spans(wav)
    act_table, _ = span_table([[s] for s in active], [T] * a.clips, unit="frames")

    # the loss legs
    B, N, window_s, hop_s = 32, 16384, 0.5, 0.25
    lwin, lhop = window_frames(window_s, hop_s)
    LT = num_frames(N)
    lrows = [[[(k * lhop, k * lhop + min(lwin, LT))] for k in range(num_windows(LT, lwin, lhop))] for _ in range(B)]
    est0 = (0.1 * torch.randn(B, 1, N, generator=g)).clamp(-1, 1).cuda()
    refs = torch.randn(a.references, 256, generator=g)
    refs = (refs / refs.norm(dim=1, keepdim=True)).cuda()
    loss_nmd = Nomad.from_engine(eng, "fp32")

    def windows_step():
        est = est0.clone().requires_grad_(True)
        loss_nmd.score_windows(est, refs, window_s, hop_s, lengths=[N] * B, reduction="mean")[0].backward()
        return est.grad

    def spans_step():
        est = est0.clone().requires_grad_(True)
        loss_nmd.score_spans(est, refs, lrows, lengths=[N] * B, reduction="mean", unit="frames")[0].backward()
        return est.grad

    timed = {"embed_ragged_ms": lambda: eng.embed_ragged(waves, precision=a.precision),
             "embed_windows_ragged_ms": lambda: eng.embed_windows_ragged(waves, a.win, a.hop, precision=a.precision)[0],
             "embed_spans_windows_ms": lambda: eng.embed_spans_ragged(waves, win_table, precision=a.precision),
             "embed_spans_active_ms": lambda: eng.embed_spans_ragged(waves, act_table, precision=a.precision),
             "frame_energy_ms": lambda: eng.frame_energy(waves),
             "active_spans_ms": lambda: (nmd.active_spans(wav), wav)[1],
             "score_windows_fb_ms": windows_step, "score_spans_fb_ms": spans_step}
    files = os.path.isdir(a.nmr) and os.path.isdir(a.deg)
    if files:
        def quiet(fn):
            def run():
                with contextlib.redirect_stdout(io.StringIO()):
                    fn()
                return wav
            return run
        timed["predict_segments_ms"] = quiet(lambda: nmd.predict_segments("dir", a.nmr, a.deg, window_s=1.0, hop_s=0.5))
        timed["predict_spans_active_ms"] = quiet(lambda: nmd.predict_spans("dir", a.nmr, a.deg, active_db=40.0))

    same = torch.equal(timed["embed_windows_ragged_ms"](), timed["embed_spans_windows_ms"]())
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

    out = {"tool": "bench_spans",
           "config": f"{a.clips} x {a.seconds:g} s in {a.precision} ({T} frames each), windows of {a.win} / {a.hop} frames ({a.clips * W} rows), "
                     f"one active row per clip over {sum(len(s) for s in active)} spans; loss legs ({B},1,{N}) x {a.references} references, "
                     f"{sum(len(r) for r in lrows)} rows, fp32; 1 GPU",
           "steps": a.steps, "rounds": a.rounds, "span_rows_equal_window_rows_bitwise": same}
    for name, v in samples.items():
        out[name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    med = {k: statistics.median(v) for k, v in samples.items()}
    out["spans_minus_windows_forward_ms"] = round(med["embed_spans_windows_ms"] - med["embed_windows_ragged_ms"], 4)
    out["spans_over_windows_forward_backward"] = round(med["score_spans_fb_ms"] / med["score_windows_fb_ms"], 4)
    if files:
        out["predict_spans_active_minus_predict_segments_ms"] = round(med["predict_spans_active_ms"] - med["predict_segments_ms"], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
