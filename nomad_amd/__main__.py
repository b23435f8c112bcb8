"""``python -m nomad_amd --mode dir --nmr P --deg P`` - CLI of the reference
(/root/reference/src/nomad_audio/__main__.py:4-18); ``--device`` is honoured here (the reference
parses it and ignores it).

Several GPUs: ``python -m torch.distributed.run --nproc-per-node N -m nomad_amd --mode dir ...`` - one process per GPU,
the files shard across the ranks (RCCL all-gather of the embeddings, ``Nomad.predict``), rank 0 writes the CSV files.

``--spans CSV`` / ``--active-db DB`` (one process): one score per caller-given row of spans, or per file over its non-silent frames
(``Nomad.predict_spans``, ``spans.csv``).

``--sweep`` (one process): ``--deg`` holds CLEAN files, which are degraded on the GPU at every level of ``--snr-db`` (with ``--noise
FILE``), ``--clip`` and / or ``--rt60`` (synthetic rooms, ``nomad_amd.nomad.synthetic_rir``) or ``--reverb`` (sox's reverb at its reverberance
levels, ``Nomad.reverb``) and scored against ``--nmr``: ``nomad_intensity.csv`` and the rank correlation of score and level.  ``--normalize [LUFS]`` brings every
degraded clip to one BS.1770 loudness first (bare: -23), as the reference's ``ffmpeg-normalize`` step does.  ``--nsim`` adds an ``NSIM``
column: the mean gammatone NSIM (``Nomad.nsim``) of the same rows with their clean clips, the similarity the model was trained to
order, next to the score.

``--nsim-pairs CSV [--max-delay S]`` (one process): the NSIM of every (``filepath_ref``, ``filepath_deg``) pair of CSV, the degraded
file moved by its delay against the clean one first (``Nomad.nsim_files``, ``nsim_pairs.csv``).  With ``--patch S [--search S]
[--vad-db DB]`` the NSIM is the patch-wise one (``Nomad.nsim_patches``): the clean file's active patches of S seconds, each searched
for within ``--search`` seconds of its own place, and the table gains ``patches_kept``, ``offset_min_frames`` and ``offset_max_frames``."""
import argparse
import os

from .nomad import Nomad


def _levels(text):
    """'0,8,15' -> [0.0, 8.0, 15.0]."""
    try:
        levels = [float(v) for v in text.split(",") if v.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected numbers separated by commas, got {text!r}")
    if not levels or not all(v == v and abs(v) != float("inf") for v in levels):
        raise argparse.ArgumentTypeError(f"expected finite numbers separated by commas, got {text!r}")
    return levels


def sweep(nomad, a):
    """--sweep: ``Nomad.intensity_sweep`` over the clean files of --deg against the references of --nmr; writes
    ``nomad_intensity.csv`` (Degradation, Condition, NOMAD) and prints the rank correlation per degradation.  -> the table."""
    import pandas as pd
    import torch
    from .nomad import _check_predict_paths
    _check_predict_paths(a.mode, a.nmr, a.deg)
    print(f"Compute non-matching reference embeddings from {a.nmr}")
    refs = nomad.get_embeddings(a.nmr).set_index("filename")
    refs = torch.from_numpy(refs.to_numpy(dtype="float32").copy())
    noise = nomad.load_processing(a.noise).reshape(-1) if a.noise is not None else None
    reverb = {"rt60_s": a.rt60} if a.rt60 is not None else {"reverberance": a.reverb} if a.reverb is not None else {}
    if a.normalize is not None:
        reverb["normalize"] = a.normalize
    if a.nsim:
        reverb["nsim"] = True
    results = nomad.intensity_sweep(a.deg, refs, noise=noise, snr_db=a.snr_db, clip_factor=a.clip, k=a.knn, **reverb)
    parts = []
    for name, res in results.items():
        t = res["table"].sort_values(by="Condition")
        part = pd.DataFrame({"Degradation": name, "Condition": t["Condition"].to_numpy(), "NOMAD": t["Distance"].to_numpy()})
        if a.nsim:     # the rows' mean per level, in the table's order
            mean = pd.DataFrame({"Condition": res["conditions"], "NSIM": res["nsim"]}).groupby("Condition")["NSIM"].mean()
            part["NSIM"] = mean.reindex(part["Condition"]).to_numpy()
        parts.append(part)
        print(f"{name}: SRCC of the mean NOMAD score with the level = {res['SRCC']:.3f}")
    table = pd.concat(parts, ignore_index=True)
    if a.results_path is None:      # as predict names its files
        from datetime import datetime
        stamp = datetime.now().strftime("%d-%m-%Y_%H-%M-%S")
        path = os.path.join("results-csv", stamp, f"{stamp}_nomad_intensity.csv")
    else:
        path = os.path.join(a.results_path, "nomad_intensity.csv")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    table.to_csv(path, index=False)
    return table


def main(argv=None):
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
    ap.add_argument("--spans", type=str, default=None, metavar="CSV",
                    help="scores over spans: one NOMAD score per row of CSV (columns Test File, start_s, end_s and optionally Row; lines "
                         "that share a Row label pool into one score), each pooled from one forward over the whole file (predict_spans)")
    ap.add_argument("--active-db", dest="active_db", type=float, default=None, metavar="DB",
                    help="score what is not silent: one score per test file over the frames within DB dB of its loudest frame (an "
                         "energy gate, not a speech detector; predict_spans)")
    ap.add_argument("--sweep", action="store_true",
                    help="--deg holds CLEAN files: degrade them on the GPU at every level of --snr-db / --clip / --rt60 / --reverb, score the result against "
                         "--nmr and report how well the score ranks the levels (nomad_intensity.csv, Nomad.intensity_sweep)")
    ap.add_argument("--noise", type=str, default=None, metavar="FILE", help="--sweep: the noise recording mixed in at --snr-db")
    ap.add_argument("--snr-db", dest="snr_db", type=_levels, default=None, metavar="A,B,...", help="--sweep: target SNRs in dB")
    ap.add_argument("--clip", type=_levels, default=None, metavar="A,B,...", help="--sweep: clip factors, percent of samples clipped")
    ap.add_argument("--rt60", type=_levels, default=None, metavar="A,B,...",
                    help="--sweep: reverberation times in seconds (synthetic diffuse rooms, not sox's reverb: that is --reverb), each in "
                         "(0, 4.096]")
    ap.add_argument("--reverb", type=_levels, default=None, metavar="A,B,...",
                    help="--sweep: sox's reverb (its comb and all-pass reverberator, the reference's REVERB degradation) at these "
                         "reverberance levels, each in 0 .. 100, sox's defaults otherwise; excludes --rt60")
    ap.add_argument("--normalize", type=float, nargs="?", const=-23.0, default=None, metavar="LUFS",
                    help="--sweep: bring every degraded clip to this BS.1770 integrated loudness before it is scored (bare: -23, EBU R128, "
                         "what the reference's ffmpeg-normalize step does), so that the score ranks the degradation at equal loudness")
    ap.add_argument("--nsim", action="store_true",
                    help="--sweep: add an NSIM column, the mean gammatone NSIM of the same degraded rows with their clean clips (Nomad.nsim; "
                         "this project's measure, not ViSQOL's); every clean file then needs 80 ms")
    ap.add_argument("--nsim-pairs", dest="nsim_pairs", type=str, default=None, metavar="CSV",
                    help="NSIM of rendered files with their clean files, each pair time-aligned first: CSV has the columns filepath_ref and "
                         "filepath_deg (the reference's degraded_data_visqol_format.csv); writes nsim_pairs.csv under --results_path "
                         "(Nomad.nsim_files; this project's measure and delay search, not ViSQOL's).  Needs neither --nmr nor --deg")
    ap.add_argument("--max-delay", dest="max_delay", type=float, default=None, metavar="S",
                    help="--nsim-pairs: the largest delay searched, in seconds (default 0.25, at most 1.024)")
    ap.add_argument("--patch", type=float, default=None, metavar="S",
                    help="--nsim-pairs: the patch-wise NSIM (Nomad.nsim_patches) with patches of S seconds (0.02 .. 1.28; ViSQOL's speech "
                         "mode is remembered to use 0.4): the clean file's active patches, each searched for in the degraded file")
    ap.add_argument("--search", type=float, default=None, metavar="S",
                    help="--patch: how far from its own place a patch is searched for, in seconds (default 1.2, at most 2.56)")
    ap.add_argument("--vad-db", dest="vad_db", type=float, default=None, metavar="DB",
                    help="--patch: a clean frame is active within DB decibels of the file's loudest frame (default 40)")
    a = ap.parse_args(argv)
    if a.max_delay is not None and a.nsim_pairs is None:
        ap.error("--max-delay goes with --nsim-pairs")
    if a.patch is not None and a.nsim_pairs is None:
        ap.error("--patch goes with --nsim-pairs")
    if (a.search is not None or a.vad_db is not None) and a.patch is None:
        ap.error("--search and --vad-db go with --patch")
    if a.nsim_pairs is not None:
        if a.sweep or a.window is not None or a.spans is not None or a.active_db is not None or a.knn is not None:
            ap.error("--nsim-pairs scores file pairs on its own: it does not go with --sweep, --window, --spans, --active-db or --knn")
        if a.max_delay is not None and not 0.0 <= a.max_delay <= 1.024:
            ap.error(f"--max-delay takes seconds from 0 to 1.024, got {a.max_delay}")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--nsim-pairs runs in one process")
        nomad = Nomad(device=a.device, weights=a.weights, precision=a.precision)
        patches = {}
        if a.patch is not None:
            patches = {"patch_s": a.patch, "search_s": 1.2 if a.search is None else a.search, "vad_db": 40.0 if a.vad_db is None else a.vad_db}
        table = nomad.nsim_files(a.nsim_pairs, max_delay_s=0.25 if a.max_delay is None else a.max_delay, results_path=a.results_path, **patches)
        print("NSIM of the aligned pairs, printing the first 5 rows")
        print(table.head())
        return
    if a.hop is not None and a.window is None:
        ap.error("--hop goes with --window")
    if not a.sweep and (a.noise is not None or a.snr_db is not None or a.clip is not None):
        ap.error("--noise, --snr-db and --clip go with --sweep")
    if not a.sweep and a.rt60 is not None:
        ap.error("--rt60 goes with --sweep")
    if not a.sweep and a.reverb is not None:
        ap.error("--reverb goes with --sweep")
    if a.reverb is not None and a.rt60 is not None:
        ap.error("--reverb and --rt60 exclude each other: both fill the REVERB rows")
    if a.nsim and not a.sweep:
        ap.error("--nsim goes with --sweep")
    if a.normalize is not None:
        if not a.sweep:
            ap.error("--normalize goes with --sweep")
        if not (a.normalize == a.normalize and abs(a.normalize) != float("inf")):
            ap.error(f"--normalize takes a finite level in LUFS, got {a.normalize}")
    if a.spans is not None and a.active_db is not None:
        ap.error("--spans and --active-db exclude each other: the rows come from the csv or from the energy gate")
    if a.spans is not None or a.active_db is not None:
        which = "--spans" if a.spans is not None else "--active-db"
        if a.window is not None:
            ap.error(f"{which} names its own frames: it does not go with --window")
        if a.sweep:
            ap.error(f"{which} does not go with --sweep")
        if a.active_db is not None and not (a.active_db == a.active_db and abs(a.active_db) != float("inf")):
            ap.error(f"--active-db takes a finite number of dB, got {a.active_db}")
    if a.sweep:
        if a.window is not None:
            ap.error("--sweep scores whole clips: it does not go with --window")
        if a.snr_db is None and a.clip is None and a.rt60 is None and a.reverb is None:
            ap.error("--sweep needs levels: --snr-db (with --noise), --clip or both, or --rt60, or --reverb")
        if (a.snr_db is None) != (a.noise is None):
            ap.error("--noise and --snr-db go together")
        for name, levels in (("--snr-db", a.snr_db), ("--clip", a.clip), ("--rt60", a.rt60), ("--reverb", a.reverb)):
            if levels is not None and not 1 <= len(levels) <= 64:
                ap.error(f"{name} takes 1 to 64 levels, got {len(levels)}")
        if a.clip is not None and not all(0.0 <= v <= 100.0 for v in a.clip):
            ap.error(f"--clip takes percentages from 0 to 100, got {a.clip}")
        if a.rt60 is not None and not all(0.0 < v <= 4.096 for v in a.rt60):
            ap.error(f"--rt60 takes seconds above 0 up to 4.096, got {a.rt60}")
        if a.reverb is not None and not all(0.0 <= v <= 100.0 for v in a.reverb):
            ap.error(f"--reverb takes reverberance levels from 0 to 100, got {a.reverb}")
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
    if a.sweep:
        if world > 1:
            raise SystemExit("--sweep runs in one process")
        print(sweep(nomad, a))
        return
    if a.spans is not None or a.active_db is not None:
        if world > 1:
            raise SystemExit("--spans and --active-db run in one process")
        rows, nomad_avg = nomad.predict_spans(a.mode, a.nmr, a.deg, spans=a.spans, active_db=a.active_db, results_path=a.results_path,
                                              k=a.knn)
        print("Nomad scores over spans, printing the first 5 rows")
        print(rows.head())
    elif a.window is not None:
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
