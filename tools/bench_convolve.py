#!/usr/bin/env python3
"""Reverberation on the device (nomad_degrade_convolve): what convolving a batch with a room costs next to the forward that consumes it.

Workload: --clips clean clips of --seconds s (64 x 10 s), one ``synthetic_rir`` room per entry of --rt60 (0.1, 0.25, 0.5, 1.0 s: 1600
to 16000 taps).  Legs per room, alternating in ONE process, median and fastest - slowest of --rounds rounds (a round times every leg
of every room once, so drift hits all alike):

  degrade_convolve   ``Engine.degrade_convolve`` alone on the packed device batch (the response already uploaded): all clips, one call
  forward            the fp32 ragged forward of the same rows, in parts of at most --max-batch-samples samples
  fftconvolve        ``scipy.signal.fftconvolve`` per clip on the host, cut to the clip's length, timed without file I/O or upload
                     (--host-rounds rounds) - for context: another algorithm (n log n, float64 transforms), not the same arithmetic

One JSON line per room: the legs, the useful TFLOP/s of the convolution counting 2 sum_i min(L, i + 1) per row, its share of the
forward and the host's time over it; --out appends the lines."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nomad_amd.nomad import Nomad, synthetic_rir  # noqa: E402


def _levels(text):
    return [float(v) for v in text.split(",") if v.strip()]


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


def useful_flop(n: int, L: int) -> float:
    """2 sum_{i < n} min(L, i + 1): the multiply-adds the formula asks for, for one row."""
    m = min(n, L)
    return 2.0 * (m * (m + 1) / 2 + (n - m) * L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rt60", type=_levels, default=[0.1, 0.25, 0.5, 1.0])
    ap.add_argument("--max-batch-samples", type=int, default=256 * 64000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_convolve.py needs a GPU: nomad_amd has no CPU path")
    from scipy.signal import fftconvolve
    nmd = Nomad(weights="seeded")
    eng = nmd.engine
    rs = np.random.RandomState(0)
    n = int(a.seconds * 16000) // 4 * 4
    host = (rs.randint(-32768, 32768, size=(a.clips, n)) * rs.uniform(0.05, 1.0, size=(a.clips, 1)) / 32768.0).astype(np.float32)
    x = torch.from_numpy(host).cuda()
    lens = [n] * a.clips

    def forward(rows, row_lens):
        step = max(1, a.max_batch_samples // n)
        for lo in range(0, rows.shape[0], step):
            eng.embed_ragged(None, packed=(rows[lo:lo + step], row_lens[lo:lo + step]))

    rooms = {rt: synthetic_rir(rt) for rt in a.rt60}
    legs, host_legs = {}, {}
    for rt, h in rooms.items():
        packed = eng.pack_responses([h])
        rows, row_lens = eng.degrade_convolve(x, packed, lengths=lens)
        # the rows the legs time are the rows the host makes: an fp32 chain of L terms against float64 transforms
        ref = fftconvolve(host[0].astype(np.float64), h.astype(np.float64))[:n]
        assert np.abs(rows[0].cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()
        legs[("degrade_convolve", rt)] = lambda packed=packed: eng.degrade_convolve(x, packed, lengths=lens)
        legs[("forward", rt)] = lambda rows=rows, row_lens=row_lens: forward(rows, row_lens)
        host_legs[rt] = lambda h=h: [fftconvolve(row, h)[:n] for row in host]
    for fn in legs.values():
        fn()
    times = {key: [] for key in legs}
    for _ in range(a.rounds):
        for key, fn in legs.items():
            times[key].append(_time(fn))
    lines = []
    for rt, h in rooms.items():
        L = int(h.shape[0])
        host_t = [_time(host_legs[rt], sync=False) for _ in range(a.host_rounds)]
        out = {"config": f"{a.clips} clips x {a.seconds:g} s, RT60 {rt:g} s ({L} taps), fp32, 1 GPU", "rt60_s": rt, "taps": L,
               "rounds": a.rounds, "host_rounds": a.host_rounds, "degrade_convolve": _stats(times[("degrade_convolve", rt)]),
               "forward": _stats(times[("forward", rt)]), "fftconvolve": _stats(host_t)}
        conv = out["degrade_convolve"]["median_ms"]
        out["useful_tflops"] = round(a.clips * useful_flop(n, L) / (conv * 1e-3) / 1e12, 2)
        out["degrade_convolve_share_of_forward"] = round(conv / out["forward"]["median_ms"], 5)
        out["fftconvolve_over_degrade_convolve"] = round(out["fftconvolve"]["median_ms"] / conv, 1)
        print(json.dumps(out))
        lines.append(json.dumps(out))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
