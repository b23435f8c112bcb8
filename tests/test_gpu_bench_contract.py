"""GPU: bench.py prints exactly one JSON line with the driver's contract fields (small sizes; the numbers are not checked)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, launcher=()):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run([sys.executable, *launcher, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), res.stdout      # ONE JSON line and nothing else on stdout (RCCL's banner too)
    return json.loads(lines[0])


def test_bench_line_contract():
    out = _run(["--steps", "2", "--warmup", "1", "--batch", "16", "--refs", "4", "--no-cpu-baseline", "--full"])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in out, key
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1 and out["unit"] == "clips/s"
    assert out["dtype"] == "f32" and out["higher_is_better"] is True and out["scaling"] == "weak" and out["vs_baseline"] is None
    assert "workload" in out["config"] and "model" not in out["config"]
    r = out["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] == "mfma" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert abs(out["value"] - 16 * 2 / (out["ms_per_step"] * 2e-3)) / out["value"] < 1e-3
    assert out["config"]["collective"].startswith("none") and out["config"]["workload"].startswith("custom")
    assert out["roofline"]["traffic"] is None and out["roofline"]["traffic_source"] is None   # only known for the full config
    assert "also_measured_c5" not in out                                                     # only next to the headline workload
    also = out["also_measured"]
    assert also["unit"] == "clips/s" and also["value"] > 0 and also["max_abs_score_diff_vs_f32"] < 1e-4


def test_bench_plain_line_is_lean():
    """Without --full the run times its steps and nothing else: the same contract fields, no extra legs, no CPU baseline,
    and no roofline where that would take a profiled pass of its own (the default two-stream split).  With the split off
    the kernels are timed inside the timed steps, so --single-stream still reports them."""
    args = ["--steps", "2", "--warmup", "1", "--batch", "16", "--refs", "4"]
    out = _run(args)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "ranks_seen"):
        assert key in out, key
    assert out["steps"] == 2 and out["warmup"] == 1 and out["dtype"] == "f32" and out["higher_is_better"] is True
    assert abs(out["value"] - 16 * 2 / (out["ms_per_step"] * 2e-3)) / out["value"] < 1e-3
    extra = [k for k in out if k.startswith("also_measured") or k in ("cpu_baseline", "roofline", "kernel_time_ms_per_step")]
    assert extra == [], extra
    one = _run(args + ["--single-stream"])
    assert one["roofline"]["achieved"] > 0 and "kernel_time_ms_per_step" in one
    assert not [k for k in one if k.startswith("also_measured") or k == "cpu_baseline"]


def test_bench_dump_outputs_repeat_run_to_run(tmp_path):
    """--dump-outputs DIR: the last timed step's scores, distance matrix and reference embeddings, the same from two runs
    with the same arguments (seeded inputs), and consistent with each other."""
    import numpy as np
    args = ["--steps", "3", "--warmup", "1", "--batch", "16", "--refs", "4", "--no-cpu-baseline", "--no-also", "--no-profile"]
    for run in ("a", "b"):
        out = _run(args + ["--dump-outputs", str(tmp_path / run)])
        assert out["steps"] == 3 and out["ms_per_step"] > 0
    got = {run: {k: np.load(tmp_path / run / f"{k}.npy") for k in ("scores", "distances", "ref_embeddings")} for run in "ab"}
    a = got["a"]
    assert a["scores"].shape == (12,) and a["distances"].shape == (12, 4) and a["ref_embeddings"].shape == (4, 256)
    assert a["scores"].dtype == a["distances"].dtype == np.float64 and a["ref_embeddings"].dtype == np.float32
    assert np.abs(a["distances"].mean(1) - a["scores"]).max() < 1e-12
    assert np.abs(np.linalg.norm(a["ref_embeddings"], axis=1) - 1).max() < 1e-5
    for k in a:
        assert np.array_equal(a[k], got["b"][k]), k


def test_bench_under_the_distributed_launcher():
    """The way the driver starts it for N > 1, with N = 1 (one GPU on the box)."""
    out = _run(["--gpus", "1", "--steps", "1", "--warmup", "1", "--batch", "8", "--refs", "2", "--no-cpu-baseline", "--no-also"],
               launcher=("-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                         "--master-port", "29541"))
    assert out["n_gpus"] == 1 and out["steps"] == 1 and "also_measured" not in out
    # under the launcher the RCCL process group exists at world size 1 too and the all-gather is really issued
    assert out["config"]["collective"].startswith("RCCL all_gather_into_tensor executed")
    # the line verifies itself: ranks counted by an all-reduce, one distinct device per rank, the all-gathered reference rows
    c = out["rank_census"]
    assert out["ranks_seen"] == 1 == c["ranks_seen"] == c["distinct_devices"] and c["consistent"]
    assert c["ref_rows_all_gathered"] == 2 == c["ref_rows_contributed_sum"] and c["ranks"][0]["device"]
    assert c["rank_ms_per_step"]["min"] <= c["rank_ms_per_step"]["max"]


def test_bench_spawns_its_own_ranks():
    """`python bench.py --gpus N` from a plain shell (no launcher): the parent starts the ranks under torch.distributed.run
    and relays rank 0's line - exercised here with one rank (--spawn), and N = 2 on this one-GPU box must fail cleanly."""
    out = _run(["--gpus", "1", "--spawn", "--steps", "1", "--warmup", "1", "--batch", "8", "--refs", "2", "--no-cpu-baseline", "--no-also"])
    assert out["n_gpus"] == 1 and out["config"]["collective"].startswith("RCCL all_gather_into_tensor executed")
    assert out["ranks_seen"] == 1 and out["rank_census"]["consistent"]
    import torch
    if torch.cuda.device_count() < 2:
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                              "--no-cpu-baseline", "--no-also"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode != 0 and res.stdout.strip() == "" and "2-rank run failed" in res.stderr


def test_bench_headline_extras_small():
    """The extra legs of the default line (configs[2] / configs[3] / peaky weights) through their helper functions at
    reduced sizes: keys and sanity only."""
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from nomad_amd.engine import Engine
    from nomad_amd.weights import seeded_state_dict
    sd = seeded_state_dict(0)
    eng = Engine(sd, 0)
    c3 = bench.time_c3(eng, 1, 0, False, torch.cuda.synchronize, n_deg=40, n_ref=8, batch=16)
    assert c3["finite"] and c3["pairs"] == 320 and c3["scaling"] == "strong" and c3["value"] > 0
    c4 = bench.time_c4(sd, 0, steps=2, warmup=1, batch=4)
    assert c4["finite"] and c4["forward_ms"] > 0 and c4["forward_backward_ms"] > 0     # two timed steps: no ordering claims
    x3 = c4["precision_bf16x3"]
    assert x3["forward_ms"] > 0 and x3["forward_backward_ms"] > 0 and x3["loss_rel_diff_vs_f32"] < 1e-4
    eng.close()


def test_bench_line_bf16_long_form():
    """configs[4] (bf16, 30 s clips) through the same contract, small batch."""
    out = _run(["--dtype", "bf16", "--seconds", "30", "--batch", "4", "--refs", "1", "--steps", "2", "--warmup", "1",
                "--no-cpu-baseline", "--full"])
    assert out["dtype"] == "bf16" and out["config"]["workload"].startswith("configs[4]")
    assert out["roofline"]["peak"] == 2500.0 and out["roofline"]["achieved"] > 0
    assert "also_measured" not in out and out["value"] > 0


def test_live_pmc_traffic(tmp_path):
    """roofline.traffic of a 1-GPU headline run is measured inside that run: the two rocprofv3 --pmc passes bench.py starts as
    child processes (tools/pmc_traffic.py:collect) produce HBM-side bytes per launch of the dominant GEMM close to the
    algorithmic A + W + C (+ residual) bytes."""
    import shutil
    if not (shutil.which("rocprofv3") or os.path.exists("/opt/rocm/bin/rocprofv3")):
        pytest.skip("rocprofv3 not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_traffic
    tab = pmc_traffic.collect(str(tmp_path))
    big = tab["gemm_256x128"]
    assert big["launches"] >= 40
    ratio = big["hbm_bytes_per_launch"] / big["algorithmic_bytes_per_launch"]
    assert 0.9 < ratio < 1.6, ratio                       # 1.16-1.19 measured: no wasted re-reads
    assert 0.9 < tab["gemm_all_launches"]["ratio"] < 1.6
