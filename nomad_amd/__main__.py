"""``python -m nomad_amd --mode dir --nmr P --deg P`` - CLI of the reference
(/root/reference/src/nomad_audio/__main__.py:4-18); ``--device`` is honoured here (the reference
parses it and ignores it).

Several GPUs: ``python -m torch.distributed.run --nproc-per-node N -m nomad_amd --mode dir ...`` - one process per GPU,
the files shard across the ranks (RCCL all-gather of the embeddings, ``Nomad.predict``), rank 0 writes the CSV files."""
import argparse
import os

from .nomad import Nomad


def main():
    ap = argparse.ArgumentParser(prog="nomad_amd")
    ap.add_argument("--mode", type=str, default="dir", help="Choose mode dir or csv")
    ap.add_argument("--nmr", "--nmr_path", dest="nmr", type=str, help="Path to non-matching reference files")
    ap.add_argument("--deg", "--test_path", dest="deg", type=str, help="Path to test files")
    ap.add_argument("--results_path", type=str, default=None)
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--weights", type=str, default=None, help="checkpoint path, or 'seeded'")
    ap.add_argument("--precision", type=str, default="fp32", choices=("fp32", "bf16x3", "bf16"),
                    help="bf16x3: split-operand bf16 MFMA, scores within ~1e-6 of fp32 at over twice the speed; "
                         "bf16: fastest, for long recordings (scores within ~5e-4 of fp32)")
    ap.add_argument("--window", type=float, default=None, metavar="S",
                    help="scores over time: one NOMAD score per window of S seconds of every test file (predict_segments)")
    ap.add_argument("--hop", type=float, default=None, metavar="S", help="seconds between window starts (default: half the window)")
    ap.add_argument("--knn", type=int, default=None, metavar="K",
                    help="score every file (or window) by the mean distance to its K nearest references (1 .. 64) instead of all "
                         "of them; without --window the neighbours go to nomad_nearest.csv")
    a = ap.parse_args()
    if a.hop is not None and a.window is None:
        ap.error("--hop goes with --window")
    if a.knn is not None and not 1 <= a.knn <= 64:
        ap.error(f"--knn takes a number of references from 1 to 64, got {a.knn}")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = 0
    if world > 1 or "LOCAL_RANK" in os.environ:      # started by torch.distributed.run: one process per GPU
        import torch
        import torch.distributed as dist
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local_rank)
        a.device = f"cuda:{local_rank}"
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        rank = dist.get_rank()
    nomad = Nomad(device=a.device, weights=a.weights, precision=a.precision)
    if a.window is not None:
        segments, nomad_avg = nomad.predict_segments(a.mode, a.nmr, a.deg, a.window, a.window / 2 if a.hop is None else a.hop,
                                                     a.results_path, k=a.knn)
        print("Nomad scores over time, printing the first 5 windows")
        print(segments.head())
    else:
        nomad_avg = nomad.predict(a.mode, a.nmr, a.deg, a.results_path, k=a.knn)[0]
    if rank == 0:
        print("Nomad average scores, printing top 5 test files")
        print(nomad_avg.head())
    if world > 1 or "LOCAL_RANK" in os.environ:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
