"""Triplet fine-tuning step on the reference's training shape (src/config/train_triplet.yaml: train_bs 8, clips
trimmed to 10 s): three forwards + TripletMarginLoss + backward to every trainable parameter + Adam, timed on the GPU.
Usage: python tools/bench_train.py [--bs 8] [--seconds 10] [--steps 5] [--eval-mode]
       python tools/bench_train.py --lengths uniform:1:10:0 [--pad-mode exact]     # clips of different lengths (seconds): the padded step
                                                                                   # ("batch", the default) or the exact-length one
(the CPU-autograd timing of the same step lives with the other oracle users: tests/manual/train_step_cpu_baseline.py)"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--eval-mode", action="store_true", help="no dropout / LayerDrop")
    ap.add_argument("--separate", action="store_true", help="three separate forward/backward calls (no merged batch)")
    ap.add_argument("--train-convnet", action="store_true", help="freeze_convnet: False - the conv feature extractor trains too")
    ap.add_argument("--gemm-precision", choices=("fp32", "bf16x3"), default="fp32",
                    help="bf16x3: every GEMM of the step as three bf16 MFMA products over hi / lo halves (Engine.gemm_precision)")
    ap.add_argument("--lengths", type=str, default="",
                    help="clip lengths in seconds: a,b,... (bs values, reused per branch, or 3*bs) or uniform:lo:hi:seed (3*bs draws)")
    ap.add_argument("--pad-mode", choices=("batch", "exact"), default="batch",
                    help="with --lengths: zero-pad every branch to its maximum (the reference's collate) or run the exact lengths")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    from nomad_amd.train import Training
    from nomad_amd.weights import num_frames, seeded_state_dict
    from nomad_amd.engine import Engine
    n = int(args.seconds * 16000)
    g = torch.Generator().manual_seed(0)
    A, P, N = [(0.1 * torch.randn(args.bs, 1, n, generator=g)).clamp(-1, 1).cuda() for _ in range(3)]
    lens = None
    if args.lengths:
        if args.lengths.startswith("uniform:"):
            lo, hi, seed = args.lengths.split(":")[1:]
            rng = torch.Generator().manual_seed(int(seed))
            secs = (float(lo) + (float(hi) - float(lo)) * torch.rand(3 * args.bs, generator=rng)).tolist()
        else:
            secs = [float(x) for x in args.lengths.split(",")]
            secs = secs * 3 if len(secs) == args.bs else secs
        assert len(secs) == 3 * args.bs, "--lengths: bs or 3*bs values"
        lens = [int(x * 16000) for x in secs]
        br = [lens[i * args.bs:(i + 1) * args.bs] for i in range(3)]
        if args.pad_mode == "exact":   # (rows (B,1,Nmax), lengths) per branch, one Nmax: TripletDataset.collate_exact's layout
            nmax = max(lens)
            mk = lambda l: ((0.1 * torch.randn(args.bs, 1, nmax, generator=g)).clamp(-1, 1).cuda(), torch.tensor(l, dtype=torch.int32))
            A, P, N = mk(br[0]), mk(br[1]), mk(br[2])
        else:                          # every branch zero-padded to its own maximum, no mask
            def mk(l):
                w = (0.1 * torch.randn(args.bs, 1, max(l), generator=g)).clamp(-1, 1)
                for i, k in enumerate(l):
                    w[i, 0, k:] = 0.0
                return w.cuda()
            A, P, N = mk(br[0]), mk(br[1]), mk(br[2])
    cfg = dict(experiment_name="bench", checkpoint_path="seeded", margin=0.2, lr=1e-4, lr_decay_factor=0.99,
               gemm_precision=args.gemm_precision)
    reg = dict(dropout=0.0, attention_dropout=0.0, dropout_input=0.0, encoder_layerdrop=0.0) if args.eval_mode else None
    sd = seeded_state_dict(0)
    tr = Training(cfg, engine=Engine(sd, 0), regularisation=reg, merge_branches=not args.separate)
    from nomad_amd.train import ExponentialLR
    tr.margin, tr.lr_scheduler = 0.2, ExponentialLR([1e-5, 1e-4], 0.99)
    eng = tr.engine
    eng.train_set_convnet(args.train_convnet)
    for _ in range(args.warmup):
        loss = tr.train_step(A, P, N)
    torch.cuda.synchronize()
    eng.profile_enable(True)
    eng.profile_reset()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = tr.train_step(A, P, N)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    prof = eng.profile_read()
    eng.profile_enable(False)
    T = num_frames(n)
    fwd_flop = 3 * args.bs * (56.925e9 * T / 199.0)  # ~linear in T except the T^2 attention term (small)
    extra = {}
    if lens is not None:
        Ts = [num_frames(k) for k in lens]
        pad = [max(Ts[i * args.bs:(i + 1) * args.bs]) for i in range(3) for _ in range(args.bs)]   # frames each row runs at when padded
        fwd_flop = 56.925e9 * (sum(Ts) if args.pad_mode == "exact" else sum(pad)) / 199.0
        extra = {"lengths": args.lengths, "pad_mode": args.pad_mode, "frames_exact_over_padded": sum(Ts) / sum(pad),
                 "frames2_exact_over_padded": sum(t * t for t in Ts) / sum(t * t for t in pad)}
    res = {**extra, "workload": f"triplet step 3x({args.bs},1,{n}) T={T}" if lens is None else f"triplet step 3x{args.bs} clips, {args.lengths}", "mode": "eval-arith" if args.eval_mode else "train (dropout+layerdrop)",
           "branches": "separate calls" if args.separate else "merged 3B batch",
           "conv_feature_extractor": "trainable" if args.train_convnet else "frozen", "gemm_precision": args.gemm_precision,
           "ms_per_step": dt * 1e3, "triplets_per_s": args.bs / dt, "loss": loss.item(),
           "approx_model_tflops": 3 * fwd_flop / dt / 1e12,
           "classes_ms_per_step": {k: v["ms"] / args.steps for k, v in prof.items()},
           "classes_launches_per_step": {k: v["launches"] / args.steps for k, v in prof.items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
