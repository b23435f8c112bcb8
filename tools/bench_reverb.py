#!/usr/bin/env python3
"""Sox-style reverb on the device (nomad_degrade_reverb): what the comb and all-pass recurrences cost, next to the other ways to
the same rows and next to the forward that consumes them.  A record, not a threshold.

Workload: --clips clean clips of --seconds s (64 x 10 s) at the reference's 30 reverberance conditions (config_audio_degrader.yaml:
`reverb:` 1, 3, 6, 7, ... 95, 100) in ONE call (G = 30 <= 64): 1920 packed rows.  Legs, alternating in ONE process, median and fastest - slowest
of --rounds rounds (a round times every leg once, so drift hits all alike):

  reverb             ``Engine.degrade_reverb`` on all clips at the 30 conditions
  convolve_65536     ``Engine.degrade_convolve`` with the same reverberator's impulse responses cut at 65 536 taps (what the FIR
                     path accepts; at reverberance 100 the response has fallen by only some 25 dB there - the line reports it -
                     so these rows are NOT the reverb's) - on --context-clips clips x 30 conditions: direct form costs
                     2 x 65 536 FLOP per output sample.  The responses are the device reverb's own output for a unit impulse.
  forward_fp32       ``Engine.embed_ragged`` (fp32) of the reverberant rows of --context-clips clips x 30 conditions
  numpy              ``tests/freeverb_ref.py``, the sample-by-sample float64 restatement, on --host-seconds s of one clip at one
                     condition (it takes seconds per row)

Every leg is also reported per row of --seconds s, the unit in which they compare.  One JSON line; --out appends it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import freeverb_ref  # noqa: E402
from nomad_amd.nomad import Nomad  # noqa: E402

REFERENCE_CONDITIONS = [1, 3, 6, 7, 9, 10, 12, 14, 16, 19, 20, 22, 24, 26, 28, 32, 36, 40, 45, 50, 55, 60, 65, 70, 75, 80, 85, 90, 95, 100]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--levels", type=lambda t: [float(v) for v in t.split(",")], default=REFERENCE_CONDITIONS)
    ap.add_argument("--context-clips", type=int, default=8)
    ap.add_argument("--host-seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reverb.py needs a GPU: nomad_amd has no CPU path")
    nmd = Nomad(weights="seeded")
    eng = nmd.engine
    G = len(a.levels)
    n = int(a.seconds * 16000) // 4 * 4
    host = (0.1 * np.random.RandomState(0).uniform(-1.0, 1.0, size=(a.clips, n))).astype(np.float32)
    x = torch.from_numpy(host).cuda()
    lens = [n] * a.clips

    # the rows the legs time are the rows the restatement makes
    k = min(n, 2000)
    got = eng.degrade_reverb(x[:1, :k].contiguous(), a.levels[-1:], lengths=[k])[0][0, :k].cpu().numpy()
    want = freeverb_ref.reverb(host[0, :k], a.levels[-1], as_float32=False)
    assert (np.abs(got - want) <= 2.0 ** -24 * np.abs(want) + 1e-12 * np.abs(host[0, :k]).max()).all()

    impulse = torch.zeros(1, 65536, device=x.device)
    impulse[0, 0] = 1.0
    irs = eng.degrade_reverb(impulse, a.levels, lengths=[65536], clamp=False)[0].clone()
    packed_irs = (irs, [65536] * G)
    top = int(np.argmax(a.levels))      # the longest tail: its level over the last 4096 taps against taps 4096 .. 8191
    decay_db = float(10.0 * torch.log10((irs[top, -4096:] ** 2).mean() / (irs[top, 4096:8192] ** 2).mean()))
    xc = x[:a.context_clips].contiguous()
    rows_f = eng.degrade_reverb(xc, a.levels, lengths=lens[:a.context_clips])
    rows_f = (rows_f[0].clone(), rows_f[1])

    legs = {
        "reverb": lambda: eng.degrade_reverb(x, a.levels, lengths=lens),
        "convolve_65536": lambda: eng.degrade_convolve(xc, packed_irs, lengths=lens[:a.context_clips]),
        "forward_fp32": lambda: eng.embed_ragged(None, precision="fp32", packed=rows_f),
    }
    rows_of = {"reverb": a.clips * G, "convolve_65536": a.context_clips * G, "forward_fp32": a.context_clips * G}
    for fn in legs.values():
        fn()
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, fn in legs.items():
            times[name].append(_time(fn))
    hn = int(a.host_seconds * 16000)
    host_ms = _time(lambda: freeverb_ref.reverb(host[0, :hn], a.levels[-1]), sync=False)

    out = {"config": f"{a.clips} clips x {a.seconds:g} s x {G} reverberance conditions = {a.clips * G} rows, 16 kHz, sox defaults, 1 GPU",
           "rounds": a.rounds, "rows": rows_of,
           "response_decay_db_at_65536_taps_reverberance_%g" % a.levels[top]: round(decay_db, 1)}
    out.update({name: _stats(t) for name, t in times.items()})
    for name in legs:
        out[f"{name}_ms_per_row"] = round(out[name]["median_ms"] / rows_of[name], 4)
    out["numpy_ms_per_row"] = round(host_ms * n / hn, 1)
    out["reverb_output_samples_per_s"] = round(a.clips * G * n / (out["reverb"]["median_ms"] * 1e-3), 0)
    out["reverb_audio_seconds_per_s"] = round(a.clips * G * a.seconds / (out["reverb"]["median_ms"] * 1e-3), 0)
    out["convolve_over_reverb_per_row"] = round(out["convolve_65536_ms_per_row"] / out["reverb_ms_per_row"], 1)
    out["forward_over_reverb_per_row"] = round(out["forward_fp32_ms_per_row"] / out["reverb_ms_per_row"], 2)
    out["numpy_over_reverb_per_row"] = round(out["numpy_ms_per_row"] / out["reverb_ms_per_row"], 0)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(out) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
