"""Triplet fine-tuning on the HIP engine: the host-side mirror of the reference's training script
(/root/reference/src/training/train_triplet.py, config /root/reference/src/config/train_triplet.yaml,
data set /root/reference/src/dataloader/triplet_dataloader.py).

Same names, same config keys, same control flow:

    train_obj = Training("src/config/train_triplet.yaml")     # train_triplet.py:44-110
    train_obj.training_loop()                                  # :161-205

and its evaluation experiments (``quality_nmr``, ``valid_rank``, ``intensity``, ``quality_fr``: train_triplet.py:203-489,
dispatched by ``main`` like the reference's main.py:26-44):

    Training("eval.yaml").eval_audio_quality(config["nomad_model_path"])

Every FLOP of a step - three forwards, nn.TripletMarginLoss, backward to every trainable parameter, Adam - runs in
libnomad_hip.so (nomad_embed_train / nomad_triplet_loss / nomad_train_backward / nomad_train_adam_step); this file
is data loading, the epoch loop, the learning-rate schedule and checkpoint writing.  The evaluation experiments embed their
files through ``Nomad.get_embeddings_csv`` (nomad_embed_ragged / nomad_embed_features_ragged), take their distances from
nomad_cdist / nomad_paired_distance, and leave the pandas / SciPy statistics of the reference as they are.

Differences, on purpose:
* none in the freeze switches: ``freeze_convnet: True`` (the shipped config; backbone at 1e-5, head at ``lr``),
  ``freeze_convnet: False`` (the conv feature extractor trains too, and - as in train_triplet.py:96 - ONE Adam group at
  ``lr`` for every parameter) and ``freeze_all: True`` are all supported.
* ``checkpoint_path`` may be a NOMAD-layout state dict (keys of nomad_best_model.pt), a fairseq ``wav2vec_small.pt``
  ({'model': state_dict}; the head is then initialised like ``nn.Linear`` under ``torch.manual_seed(0)``), or the word
  ``seeded`` (random weights, for tests).  fairseq itself is not needed.
* evaluation: ``nomad_model_path`` is a NOMAD-layout checkpoint (what ``Training.save`` writes) or ``seeded``; the config key
  ``precision`` (``fp32`` default, ``bf16x3``, ``bf16``; not a reference key) picks the forward of the embeddings; each
  ``eval_*`` method returns what it printed from (the reference returns nothing); figures are drawn with matplotlib alone
  (no seaborn) and skipped with one printed line when matplotlib is missing; the dead PCA block (``pca_plot = False``) is not
  built; no optimiser state is allocated.
* ``pad_mode`` (not a reference key): ``"batch"`` (default) zero-pads each of A / P / N to its own batch maximum with no mask, as
  the reference's collate does - a clip's training embedding then depends on the longest clip that happens to share its batch.
  ``"exact"`` departs from the reference on purpose: the collate keeps the lengths, a step is ALWAYS one merged launch sequence
  over the 3B clips at their exact lengths (nomad_embed_train_ragged / nomad_train_backward_ragged, LayerDrop per branch) and
  validation embeds through nomad_embed_ragged - the arithmetic ``predict`` and the evaluation experiments score the model
  with, and no time spent on padded frames.  ``freeze_convnet: False`` is refused with it (the conv extractor's parameter
  gradients need equal-length batches).
* ``triplets_on_device`` (not a reference key): ``{clean: <dir|csv>, valid_clean: <dir|csv>, noise: <wav>, snr_db: [...], clip:
  [...], reverb: [...], normalize: -23, N: 3, hard_sampling: false, sampling_margin: 0.05, patch_s: null, vad_db: 40, min_active: 1.0}``
  (``patch_s``: the table comes from the patch-wise NSIM, ``Nomad.nsim_patches``, so that silence does not count).  With it ``train_df`` / ``valid_df``
  are not read: a step takes ``train_bs // N`` clean clips, degrades them on the GPU at every listed level, takes each degraded
  row's NSIM with its clean clip, samples up to ``train_bs`` triplets by the reference's rule (``Nomad.mine_triplets``: the
  reference's offline ffmpeg / sox / ViSQOL / pandas preparation with nothing rendered to disk; the NSIM is this project's
  gammatone measure, not ViSQOL's) and runs the exact-length step on them.  It requires ``pad_mode: exact``.  Validation mines with
  one fixed seed per batch, the same in every epoch, so successive epochs are comparable.
* model.train() regularisation (fairseq BASE config: dropout 0.1, attention_dropout 0.1, dropout_input 0.1,
  encoder_layerdrop 0.05) uses the engine's counter-based masks; torch's RNG stream of the reference's device cannot
  be reproduced on any other device, so runs are statistically, not bit-wise, equivalent to the reference's.
"""
from __future__ import annotations

import os
import random
from datetime import datetime
from typing import Dict, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import wavio
from .engine import Engine
from .nomad import Nomad, Origw2v, TripletModel
from .weights import EMB_DIM, EMBED_DIM, check_state_dict, expected_shapes, load_checkpoint, seeded_state_dict

SEED = 0  # train_triplet.py:29-33
PAD_MODES = ("batch", "exact")   # config key pad_mode (module docstring)


def check_pad_mode(config) -> str:
    """The config's ``pad_mode`` (default "batch"), validated together with the switches it excludes."""
    mode = config.get("pad_mode", "batch")
    if mode not in PAD_MODES:
        raise ValueError(f"pad_mode must be one of {PAD_MODES}, got {mode!r}")
    if mode == "exact" and not config.get("freeze_convnet", True) and not config.get("freeze_all"):
        raise ValueError("pad_mode 'exact' needs freeze_convnet: True: the conv feature extractor's parameter gradients are built for "
                         "equal-length batches only")
    return mode

MINING_DEFAULTS = dict(clean=None, valid_clean=None, noise=None, snr_db=None, clip=None, reverb=None, normalize=-23.0, N=3,
                       hard_sampling=False, sampling_margin=0.05, patch_s=None, vad_db=40.0, min_active=1.0)


def check_triplets_on_device(config, pad_mode: str) -> Optional[dict]:
    """The config's ``triplets_on_device`` (module docstring) with its defaults filled in, or None without the key.  Needs no GPU."""
    raw = config.get("triplets_on_device")
    if raw is None:
        return None
    if not isinstance(raw, dict):
        raise ValueError("triplets_on_device must be a mapping (clean, valid_clean, noise, snr_db, clip, reverb, normalize, N, ...)")
    unknown = sorted(set(raw) - set(MINING_DEFAULTS))
    if unknown:
        raise ValueError(f"triplets_on_device: unknown keys {unknown}; known: {sorted(MINING_DEFAULTS)}")
    if pad_mode != "exact":
        raise ValueError("triplets_on_device requires pad_mode: exact (mined triplets are packed rows with their exact lengths; "
                         f"the config has pad_mode: {pad_mode})")
    m = dict(MINING_DEFAULTS, **raw)
    if not m["clean"] or not m["valid_clean"]:
        raise ValueError("triplets_on_device needs clean and valid_clean: a directory of wav files or a csv with a filename column")
    if m["snr_db"] is None and m["clip"] is None and m["reverb"] is None:
        raise ValueError("triplets_on_device needs at least one of snr_db, clip and reverb (lists of levels)")
    if m["snr_db"] is not None and not m["noise"]:
        raise ValueError("triplets_on_device: snr_db needs noise: <wav>")
    if m["patch_s"] is not None:
        from .nomad import check_patch_params
        check_patch_params(m["patch_s"], m["patch_s"], m["vad_db"], m["min_active"])
    m["N"] = int(m["N"])
    if m["N"] < 1 or int(config.get("train_bs", m["N"])) < m["N"] or int(config.get("val_bs", m["N"])) < m["N"]:
        raise ValueError(f"triplets_on_device: N = {m['N']} must be at least 1 and at most train_bs and val_bs")
    return m


class MinedTriplets:
    """What ``Training`` iterates in place of a DataLoader with ``triplets_on_device``: batches of ``batch_size // N`` clean files,
    each turned into up to ``batch_size`` triplets on the GPU (``Nomad.mine_triplets``) -> (A, P, N) as ``_step_exact`` takes them.
    shuffle: a new order of the files and new draws in every pass; otherwise file order and one fixed seed per batch, the same in
    every pass.  A batch whose draws all dropped is passed over."""

    def __init__(self, nomad: Nomad, files, mining: dict, batch_size: int, shuffle: bool, seed: int = SEED, trim: bool = False):
        self.nomad, self.mining, self.shuffle, self.trim = nomad, mining, shuffle, trim
        self.files = sorted(str(f) for f in files)     # (a directory lists in no fixed order)
        if not self.files:
            raise ValueError("triplets_on_device: no clean file to mine from")
        self.clips = max(1, int(batch_size) // mining["N"])
        self.noise = load_processing(mining["noise"])[0] if mining["noise"] else None
        self._rng = np.random.RandomState(seed)
        self._seed = seed
        self.last_info = None

    def __len__(self):
        return (len(self.files) + self.clips - 1) // self.clips

    def mine(self, paths, seed):
        """The clean files ``paths`` -> (A, P, N, info) of ``Nomad.mine_triplets``."""
        wavs = [load_processing(p, trim=self.trim)[0] for p in paths]
        lens = [int(w.shape[0]) for w in wavs]
        rows = torch.zeros(len(wavs), max(lens), dtype=torch.float32)
        for i, w in enumerate(wavs):
            rows[i, :lens[i]] = w
        m = self.mining
        return self.nomad.mine_triplets(rows, noise=self.noise, snr_db=m["snr_db"], clip_factor=m["clip"], reverberance=m["reverb"],
                                        normalize=m["normalize"], lengths=lens, N=m["N"], hard_sampling=bool(m["hard_sampling"]),
                                        margin=float(m["sampling_margin"]), seed=seed,
                                        **({} if m.get("patch_s") is None else
                                           {"patch_s": m["patch_s"], "vad_db": m["vad_db"], "min_active": m["min_active"]}))

    def __iter__(self):
        order = self._rng.permutation(len(self.files)) if self.shuffle else np.arange(len(self.files))
        for k, lo in enumerate(range(0, len(order), self.clips)):
            seed = int(self._rng.randint(0, 2 ** 31 - 1)) if self.shuffle else self._seed + k
            A, P, N, info = self.mine([self.files[i] for i in order[lo:lo + self.clips]], seed)
            self.last_info = info
            if len(A[1]):
                yield A, P, N


# fairseq wav2vec 2.0 BASE pre-training config (what wav2vec_small.pt carries in its cfg)
W2V_BASE_REGULARISATION = dict(dropout=0.1, attention_dropout=0.1, dropout_input=0.1, encoder_layerdrop=0.05)


def load_processing(filepath, target_sr: int = 16000, trim: bool = False) -> torch.Tensor:
    """triplet_dataloader.py:8-29: load, mono mix, resample to 16 kHz, optionally trim to 10 s.  -> (1, N) fp32."""
    return torch.from_numpy(wavio.load_processing(filepath, target_sr, trim))


class TripletDataset(torch.utils.data.Dataset):
    """triplet_dataloader.py:31-83: csv with Anchor / Positive / Negative (and db) columns under ``root``."""

    def __init__(self, config, data_mode="train_df", level=None):
        super().__init__()
        import pandas as pd
        self.config = config
        self.root = self.config["root"]
        self.dataset = pd.read_csv(self.config[data_mode])
        if level is not None:
            self.dataset = self.dataset[self.dataset["db"].isin(level)]
        self.dataset = self.dataset.drop_duplicates()
        self.pad_mode = check_pad_mode(self.config)

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, index):
        row = self.dataset.iloc[index]
        trim = self.config["trim"]
        return tuple(load_processing(os.path.join(self.root + row[c]), trim=trim) for c in ("Anchor", "Positive", "Negative"))

    def collate_fn(self, batch):  # zero padding at batch level
        A, P, N = zip(*batch)
        if getattr(self, "pad_mode", "batch") == "exact":
            return self.collate_exact(A, P, N)
        return self.zero_pad_wav(A), self.zero_pad_wav(P), self.zero_pad_wav(N)

    @staticmethod
    def collate_exact(A, P, N):
        """pad_mode "exact": every branch as (rows (B,1,Nmax), lengths (B,) int32) with ONE Nmax for the 3B clips, so that the step
        stacks them without a copy per clip; the samples behind a length are storage only - the engine never reads them."""
        max_len = max(w.shape[1] for w in A + P + N)
        def rows(wavs):
            out = torch.zeros(len(wavs), 1, max_len, dtype=torch.float32)
            for i, w in enumerate(wavs):
                out[i, 0, :w.shape[1]] = w[0]
            return out, torch.tensor([w.shape[1] for w in wavs], dtype=torch.int32)
        return rows(A), rows(P), rows(N)

    @staticmethod
    def zero_pad_wav(wavs):
        max_len = max(w.shape[1] for w in wavs)
        return torch.stack([torch.nn.functional.pad(w, (0, max_len - w.shape[1]), "constant", 0) for w in wavs], dim=0)


def load_pretrained(path: str, allow_unsafe_pickle: bool = None) -> Dict[str, torch.Tensor]:
    """State dict in the NOMAD checkpoint layout from ``checkpoint_path`` (see module docstring).

    The file is read with the tensors-only unpickler.  A fairseq checkpoint that pickles its config objects needs the full
    unpickler - which executes whatever the file contains - so that is used only when the caller asks for it
    (``allow_unsafe_pickle=True``, config key ``allow_unsafe_pickle``, or ``NOMAD_ALLOW_UNSAFE_PICKLE=1``); otherwise the
    restricted loader's error is re-raised with that hint.  (The reference always uses the full one: nomad.py:58.)"""
    if path == "seeded":
        return seeded_state_dict(0)
    if allow_unsafe_pickle is None:
        allow_unsafe_pickle = os.environ.get("NOMAD_ALLOW_UNSAFE_PICKLE", "0") == "1"
    try:
        obj = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:
        if not allow_unsafe_pickle:
            raise RuntimeError(f"{path}: not loadable with torch.load(weights_only=True) ({type(e).__name__}: {str(e)[:200]}).  If this is a "
                               "trusted fairseq checkpoint with pickled config objects, pass allow_unsafe_pickle=True (config key "
                               "'allow_unsafe_pickle', or NOMAD_ALLOW_UNSAFE_PICKLE=1) to load it with the full unpickler.") from e
        obj = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(obj, dict) and "model" in obj and isinstance(obj["model"], dict):  # fairseq checkpoint
        want = expected_shapes()
        sd = {}
        for k, v in obj["model"].items():
            k2 = "ssl_model." + k
            if k2 in want:
                sd[k2] = v.detach().to(torch.float32).contiguous()
        g = torch.Generator().manual_seed(SEED)  # nn.Linear default init (kaiming_uniform a=sqrt(5)): U(-1/sqrt(in), +)
        bound = 1.0 / np.sqrt(EMBED_DIM)
        sd["embedding_layer.1.weight"] = (torch.rand(EMB_DIM, EMBED_DIM, generator=g) * 2 - 1) * bound
        sd["embedding_layer.1.bias"] = (torch.rand(EMB_DIM, generator=g) * 2 - 1) * bound
        sd.setdefault("ssl_model.mask_emb", torch.zeros(EMBED_DIM))
        check_state_dict(sd)
        return sd
    return load_checkpoint(path)


def allreduce_mean_gradients(engine, group=None) -> None:
    """Data-parallel fine-tuning (not in the reference, which is single-GPU): average the flat gradient vector over
    the ranks - ONE all-reduce of 85 M floats (RCCL over xGMI; gloo in the CPU test) between backward and Adam.
    One process per GPU; each rank's DataLoader must yield its own shard (DistributedSampler)."""
    world = dist.get_world_size(group)
    if world == 1:
        return
    g = engine.train_read(1)
    dist.all_reduce(g, op=dist.ReduceOp.SUM, group=group)
    g.div_(world)
    engine.train_write(1, g)


class ExponentialLR:
    """torch.optim.lr_scheduler.ExponentialLR over the two learning rates (train_triplet.py:110)."""

    def __init__(self, lrs: Sequence[float], gamma: float):
        self.lrs, self.gamma = list(lrs), gamma

    def step(self):
        self.lrs = [lr * self.gamma for lr in self.lrs]

    def get_last_lr(self):
        return list(self.lrs)


EVAL_EXPERIMENTS = ("quality_nmr", "valid_rank", "intensity", "quality_fr")


def order_three(x, a, b, c, d):
    """train_triplet.py:227-228: the third-order map from distance to MOS."""
    return a * x + b * x ** 2 + c * x ** 3 + d


def filter_test_data(test_data, db=None, conds=None):
    """train_triplet.py:240-249: the databases (``db``: a list, None = all) and conditions (``conds``: substrings joined into
    one regular expression, None = all) under test."""
    if db is not None:
        test_data = test_data[test_data["db"].isin(db)]
    if conds is not None:
        print(f"Testing DB: {db}, conds: {conds}")
        test_data = test_data[test_data["condition"].str.contains("|".join(conds))]
    return test_data


def _emb_values(df) -> np.ndarray:
    """The embedding columns of a table whose index is the file name, as the fp32 values they were computed in."""
    return np.ascontiguousarray(df.to_numpy(dtype=np.float32))


def mos_statistics(df_dist) -> dict:
    """train_triplet.py:276-303 / :447-474 on a per-condition table with ``Distance`` and ``mos``: the cubic map (``curve_fit``,
    default arguments), ``Distance_map``, Spearman and Pearson with and without the map, printed as the reference prints
    them.  -> {table, popt, SRCC, SRCC_map, PCC, PCC_map}."""
    from scipy.optimize import curve_fit
    from scipy.stats import pearsonr, spearmanr
    popt3, _ = curve_fit(order_three, df_dist["Distance"].values, df_dist["mos"].values)
    a3, b3, c3, d3 = popt3
    df_dist["Distance_map"] = df_dist["Distance"].apply(lambda x: order_three(x, a3, b3, c3, d3))
    SRCC, _ = spearmanr(df_dist["Distance"], df_dist["mos"])
    print(f"SRCC: {np.round(SRCC, 2)}")
    SRCC_map, _ = spearmanr(df_dist["Distance_map"], df_dist["mos"])
    print(f"SRCC 3rd map: {np.round(SRCC_map, 2)}")
    PCC, _ = pearsonr(df_dist["Distance"], df_dist["mos"])
    print(f"PCC: {np.round(PCC, 2)}")
    PCC_map, _ = pearsonr(df_dist["Distance_map"], df_dist["mos"])
    print(f"PCC 3rd map: {np.round(PCC_map, 2)}")
    return dict(table=df_dist, popt=np.asarray(popt3), SRCC=float(SRCC), SRCC_map=float(SRCC_map), PCC=float(PCC),
                PCC_map=float(PCC_map))


def quality_nmr_stats(df_emb, db, ref_embeddings, nmr_mean) -> dict:
    """One database of ``eval_audio_quality`` (train_triplet.py:262-303).  df_emb: ``get_embeddings_csv`` of
    ``db['filepath_deg']``; ref_embeddings: the non-matching references, indexed by ``reference``;
    nmr_mean(test, ref) -> (N,) float64: the mean over the references of the Euclidean distances (cdist + np.mean(axis=1))."""
    import pandas as pd
    test_embeddings = df_emb.set_index("filepath_deg")
    test_names = df_emb.merge(db, on="filepath_deg")[["filepath_deg", "condition", "mos"]]
    avg_dist_nmr = nmr_mean(_emb_values(test_embeddings), _emb_values(ref_embeddings))
    df_dist = pd.DataFrame({"filepath_deg": test_embeddings.index, "Distance": avg_dist_nmr})
    df_dist = df_dist.merge(test_names, on="filepath_deg").set_index("filepath_deg")
    df_dist = df_dist.groupby("condition").mean()
    out = mos_statistics(df_dist)
    out["embeddings"] = df_emb
    return out


def valid_rank_labels(anchors):
    """train_triplet.py:332: the condition of a validation anchor, from its file name."""
    return [x.split("_")[1] + " " + x.split("_")[2].split(".")[0] for x in anchors]


def valid_rank_stats(df_emb, ref_embeddings, nmr_mean) -> dict:
    """``eval_degr_level`` (train_triplet.py:317-333).  df_emb: ``get_embeddings_csv`` of the validation anchors (column
    ``Anchor`` first); ref_embeddings: ``get_nmr_embeddings()`` (column ``reference`` first).
    -> {table (per file, sorted by Distance, with ``condition``), order (conditions by mean distance)}."""
    import pandas as pd
    test_embeddings = np.ascontiguousarray(df_emb.iloc[:, 1:].to_numpy(dtype=np.float32))
    avg_dist_nmr = nmr_mean(test_embeddings, np.ascontiguousarray(ref_embeddings.iloc[:, 1:].to_numpy(dtype=np.float32)))
    df_dist = pd.DataFrame({"Anchor": df_emb["Anchor"], "Distance": avg_dist_nmr})
    df_dist.sort_values(by="Distance", inplace=True)
    df_dist["condition"] = valid_rank_labels(df_dist["Anchor"])
    order = df_dist.groupby("condition")["Distance"].mean().sort_values().index
    return dict(table=df_dist, order=list(order), embeddings=df_emb)


def intensity_stats(df_emb, deg_data, ref_embeddings, nmr_mean, deg_name="") -> dict:
    """One degradation of ``eval_degradation_intensity`` (train_triplet.py:369-393): mean distance per ``Condition`` (the
    degradation's level) and its rank correlation with the level.  -> {table, SRCC}."""
    import pandas as pd
    from scipy.stats import spearmanr
    test_embeddings = df_emb.set_index("filepath_deg")
    test_names = df_emb.merge(deg_data, on="filepath_deg")[["filepath_deg", "Condition"]]
    avg_dist_nmr = nmr_mean(_emb_values(test_embeddings), _emb_values(ref_embeddings))
    df_dist = pd.DataFrame({"filepath_deg": test_embeddings.index, "Distance": avg_dist_nmr})
    df_dist = df_dist.merge(test_names, on="filepath_deg")
    df_dist.set_index("filepath_deg", inplace=True)
    df_dist = df_dist.groupby("Condition").mean().reset_index()
    df_dist.sort_values(by="Distance", inplace=True)
    SRCC, _ = spearmanr(df_dist["Distance"], df_dist["Condition"])
    print(f"Degradation: {deg_name}")
    print(f"SRCC: {np.round(SRCC, 2)}")
    return dict(table=df_dist, SRCC=float(SRCC), embeddings=df_emb)


def quality_fr_stats(df_emb_test, df_emb_ref, db, paired) -> dict:
    """One database of ``eval_full_reference`` (train_triplet.py:433-474).  df_emb_test / df_emb_ref: ``get_embeddings_csv`` of
    ``db['filepath_deg']`` / ``db['filepath_ref']``, row i of one matching row i of the other;
    paired(test, ref) -> (N,) float64: the distance of each file to ITS reference (np.diag(cdist(test, ref)))."""
    import pandas as pd
    test = df_emb_test.set_index("filepath_deg")
    ref = df_emb_ref.set_index("filepath_ref")
    test_names = df_emb_test.merge(db, on="filepath_deg")[["filepath_deg", "condition", "mos"]]
    fr_distance = paired(_emb_values(test), _emb_values(ref))
    df_dist = pd.DataFrame({"filepath_deg": test.index, "Distance": fr_distance})
    df_dist = df_dist.merge(test_names, on="filepath_deg")
    # (the reference leaves the file-name column in the frame here; pandas 2 no longer drops it silently from a mean)
    df_dist = df_dist.groupby("condition").mean(numeric_only=True)
    out = mos_statistics(df_dist)
    out["embeddings"], out["ref_embeddings"] = df_emb_test, df_emb_ref
    return out


def _figure():
    """(Figure, FigureCanvasAgg) or None with one printed line: matplotlib alone, no pyplot state, no display."""
    try:
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
    except Exception as e:  # noqa: BLE001 - an absent or broken matplotlib only costs the picture
        print(f"matplotlib is not available ({type(e).__name__}): figure skipped")
        return None
    return Figure, FigureCanvasAgg


def save_mos_scatter(df_dist, path: str, ylabel: str) -> Optional[str]:
    """train_triplet.py:282-291: MOS against the mapped distance, both axes 1 .. 5."""
    mpl = _figure()
    if mpl is None:
        return None
    fig = mpl[0]()
    mpl[1](fig)
    ax = fig.add_subplot(111)
    ax.scatter(df_dist["mos"], df_dist["Distance_map"])
    ax.set_xlabel("Actual MOS")
    ax.set_ylabel(ylabel)
    ax.set_xlim([1, 5])
    ax.set_ylim([1, 5])
    fig.tight_layout()
    fig.savefig(path)
    return path


def save_rank_boxplot(df_dist, order, path: str) -> Optional[str]:
    """train_triplet.py:329-342: one box per condition, conditions ordered by their mean distance, means marked."""
    mpl = _figure()
    if mpl is None:
        return None
    fig = mpl[0](figsize=(50, 20))
    mpl[1](fig)
    ax = fig.add_subplot(111)
    ax.boxplot([df_dist.loc[df_dist["condition"] == c, "Distance"].to_numpy() for c in order], showmeans=True, widths=0.8,
               meanprops={"markerfacecolor": "white", "markeredgecolor": "blue", "markersize": 50},
               boxprops={"linewidth": 6}, whiskerprops={"linewidth": 6}, capprops={"linewidth": 6}, medianprops={"linewidth": 6})
    ax.set_xticks(range(1, len(order) + 1))
    ax.set_xticklabels(list(order), rotation=65)
    ax.tick_params(labelsize=60)
    ax.set_ylabel("NOMAD", fontsize=80)
    ax.set_xlabel("Condition", fontsize=80)
    fig.tight_layout()
    fig.savefig(path)
    return path


class Training:
    def __init__(self, config_file, device: int = 0, engine: Optional[Engine] = None,
                 regularisation: Optional[dict] = None, merge_branches: bool = True, group=None):
        import yaml
        if isinstance(config_file, dict):
            self.config = dict(config_file)
        else:
            with open(config_file) as file:
                self.config = yaml.load(file, Loader=yaml.FullLoader)
        self.pad_mode = check_pad_mode(self.config)   # (a config error is reported as one, with or without a GPU)
        self.mining = check_triplets_on_device(self.config, self.pad_mode)
        if not torch.cuda.is_available():
            raise RuntimeError("nomad_amd.train needs an MI355X: the engine has no CPU path")
        self.DEVICE = torch.device("cuda", device)
        print(f"Device: {self.DEVICE}")
        random.seed(SEED)
        np.random.seed(SEED)
        torch.manual_seed(SEED)
        self.group = group                       # torch.distributed group (None: the default group, if any)
        self.precision = self.config.get("precision", "fp32")   # not a reference key: the forward of the evaluation embeddings
        if self.precision not in ("fp32", "bf16x3", "bf16"):
            raise ValueError("precision must be 'fp32', 'bf16x3' or 'bf16'")
        self._device_index = device
        if self.config["experiment_name"] in EVAL_EXPERIMENTS:
            # The evaluation experiments need no optimiser state (no train_enable).  eval_w2v: the model is an Origw2v over the
            # weights of checkpoint_path (train_triplet.py:67-68).  Otherwise the reference builds a TripletModel over
            # checkpoint_path and then overwrites every one of its parameters from `model_path` (load_state_dict of a NOMAD
            # checkpoint, :234): the engine is created from `model_path` itself, when the experiment names it (_load_model).
            self.engine = engine
            self._loaded_from = None if engine is None else "engine"
            if self.config.get("eval_w2v") and engine is None:
                self.engine = Engine(load_pretrained(self.config["checkpoint_path"], self.config.get("allow_unsafe_pickle")), device)
                self._loaded_from = self.config["checkpoint_path"]
            self.model = None
            self._bind_model()
            return
        if self.config.get("eval_w2v"):
            raise NotImplementedError("eval_w2v (raw wav2vec features) is for the evaluation experiments quality_nmr and intensity; "
                                      "'Training' fine-tunes the TripletModel")
        self.engine = engine if engine is not None else Engine(
            load_pretrained(self.config["checkpoint_path"], self.config.get("allow_unsafe_pickle")), device)
        # gemm_precision (not a reference key): "bf16x3" forms the products of every GEMM of the step - forward, dX and the
        # split-K dW - as three bf16 MFMA products over hi / lo halves, accumulated in fp32 (Engine.gemm_precision).  Only set
        # when the config names it: an engine handed in by the caller (shared with a Nomad(precision="bf16x3"), say) keeps its mode
        if "gemm_precision" in self.config:
            self.engine.gemm_precision = self.config["gemm_precision"]
        self.engine.train_enable()
        # freeze_all (train_triplet.py:76-79): feature extractor and encoder frozen; what is left trainable is
        # post_extract_proj, the feature LayerNorm and the embedding layer
        training = self.config["experiment_name"] == "Training"
        self.engine.train_set_frozen(bool(training and self.config.get("freeze_all")))
        # freeze_convnet: False (train_triplet.py:71-73): the conv feature extractor gets gradients too (unless freeze_all
        # froze it again, :76-78)
        self.train_convnet = bool(training and not self.config.get("freeze_convnet", True) and not self.config.get("freeze_all"))
        self.engine.train_set_convnet(self.train_convnet)
        self.reg = dict(W2V_BASE_REGULARISATION)
        self.reg.update(regularisation or {})
        self._rng = np.random.RandomState(SEED)  # LayerDrop draws + per-call dropout seeds
        self.merge_branches = merge_branches     # A/P/N as one 3B-clip launch sequence when their padded lengths agree
        if self.config["experiment_name"] == "Training":
            self.current_level = self.config.get("current_level")
            if self.mining is not None:
                # triplets mined on the GPU from clean files (module docstring): train_df / valid_df are not read
                from .nomad import _file_table
                miner = Nomad.from_engine(self.engine)
                trim = bool(self.config.get("trim", False))
                self.train_sampler = None
                self.train_loader = MinedTriplets(miner, _file_table(str(self.mining["clean"]))["filename"], self.mining,
                                                  self.config["train_bs"], shuffle=True, trim=trim)
                self.valid_loader = MinedTriplets(miner, _file_table(str(self.mining["valid_clean"]))["filename"], self.mining,
                                                  self.config["val_bs"], shuffle=False, trim=trim)
            else:
                g = torch.Generator()
                g.manual_seed(SEED)
                self.train_set = TripletDataset(self.config, data_mode="train_df", level=self.current_level)
                self.train_sampler = None
                if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
                    self.train_sampler = torch.utils.data.distributed.DistributedSampler(
                        self.train_set, num_replicas=dist.get_world_size(group), rank=dist.get_rank(group), shuffle=True, seed=SEED)
                self.train_loader = torch.utils.data.DataLoader(
                    self.train_set, batch_size=self.config["train_bs"], shuffle=self.train_sampler is None,
                    sampler=self.train_sampler, num_workers=self.config["num_workers"],
                    collate_fn=self.train_set.collate_fn, generator=g, pin_memory=True)
                self.valid_set = TripletDataset(self.config, data_mode="valid_df", level=self.current_level)
                self.valid_loader = torch.utils.data.DataLoader(
                    self.valid_set, batch_size=self.config["val_bs"], shuffle=False, num_workers=self.config["num_workers"],
                    collate_fn=self.valid_set.collate_fn, pin_memory=True)
            self.margin = float(self.config["margin"])
            # train_triplet.py:96-107: Adam; with freeze_convnet the pretrained parameters at 1e-5 and embedding_layer at
            # `lr`, otherwise the optimiser is not overwritten and every parameter runs at `lr`
            lr = float(self.config["lr"])
            body_lr = 1e-5 if self.config.get("freeze_convnet", True) else lr
            self.lr_scheduler = ExponentialLR([body_lr, lr], float(self.config["lr_decay_factor"]))

    # ---- one optimisation step (train_triplet.py:117-131) ---------------------------------------------
    def _draw(self) -> dict:
        """model.train() randomness of ONE forward call: LayerDrop mask (np.random.random() > layerdrop keeps the
        layer, fairseq TransformerEncoder.extract_features) and the seed of its dropout masks."""
        mask = 0
        for l in range(12):
            if self.reg["encoder_layerdrop"] <= 0 or self._rng.random_sample() > self.reg["encoder_layerdrop"]:
                mask |= 1 << l
        return dict(dropout=self.reg["dropout"], attention_dropout=self.reg["attention_dropout"],
                    dropout_input=self.reg["dropout_input"], seed=int(self._rng.randint(0, 2 ** 62)), layer_mask=mask)

    def train_step(self, A: torch.Tensor, P: torch.Tensor, N: torch.Tensor, training: bool = True) -> torch.Tensor:
        """A_embs = model(A); P_embs = model(P); N_embs = model(N); loss = criterion(...); zero_grad; backward; step.
        Returns the loss as a 1-element device tensor (no host sync here)."""
        eng = self.engine
        if isinstance(A, (tuple, list)):   # pad_mode "exact": (rows, lengths) per branch
            return self._step_exact(A, P, N, training)
        wavs = [w.to(self.DEVICE, torch.float32, non_blocking=True).squeeze(1).contiguous() for w in (A, P, N)]
        if not training:
            # model.eval(): clips are independent and the engine is batch invariant bit for bit, so the three
            # forwards of train_triplet.py:146-148 run as ONE batch of 3B clips when the lengths agree
            if wavs[0].shape == wavs[1].shape == wavs[2].shape:
                B = wavs[0].shape[0]
                e = eng.embed(torch.cat(wavs, dim=0))
                embs = [e[:B], e[B:2 * B], e[2 * B:]]
            else:
                embs = [eng.embed(w) for w in wavs]
            return eng.triplet_loss(embs[0].contiguous(), embs[1].contiguous(), embs[2].contiguous(), self.margin,
                                    want_grad=False)[0]
        draws = [self._draw() for _ in wavs]
        if self.merge_branches and wavs[0].shape == wavs[1].shape == wavs[2].shape:
            # The three forwards as ONE batch of 3B clips: every clip goes through the same arithmetic as in its own
            # call, LayerDrop stays per branch (the engine runs a layer per branch where the draws disagree), and
            # the dropout masks of the three branches are disjoint slices of one counter-based stream.
            B = wavs[0].shape[0]
            d = dict(draws[0], layer_mask=0xFFF)
            eng.train_set_stochastic(**d)
            eng.train_set_branches([x["layer_mask"] for x in draws])
            w = torch.cat(wavs, dim=0)
            emb, layers, saved = eng.embed_train(w)
            loss, da, dp, dn = eng.triplet_loss(emb[:B].contiguous(), emb[B:2 * B].contiguous(), emb[2 * B:].contiguous(),
                                                self.margin)
            eng.train_zero_grad()
            eng.train_backward(w, layers, saved, torch.cat([da, dp, dn], dim=0))
            eng.train_set_branches(None)
        else:
            outs = []
            for w, d in zip(wavs, draws):
                eng.train_set_stochastic(**d)
                outs.append(eng.embed_train(w))
            loss, da, dp, dn = eng.triplet_loss(outs[0][0], outs[1][0], outs[2][0], self.margin)
            eng.train_zero_grad()
            for w, (_, layers, saved), g, d in zip(wavs, outs, (da, dp, dn), draws):
                eng.train_set_stochastic(**d)
                eng.train_backward(w, layers, saved, g)
        eng.train_set_stochastic()
        if self.group is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            allreduce_mean_gradients(eng, self.group)  # data parallel: every rank saw its own triplets
        lr_body, lr_head = self.lr_scheduler.get_last_lr()
        eng.adam_step(lr_body, lr_head)
        return loss

    def _step_exact(self, A, P, N, training: bool) -> torch.Tensor:
        """``train_step`` for pad_mode "exact": A / P / N are (rows (B,1,Nmax) or (B,Nmax), lengths (B,)) with one Nmax.  Always ONE
        launch sequence over the 3B clips at their exact lengths; validation (training=False) embeds through ``embed_ragged``."""
        eng = self.engine
        rows = [w.to(self.DEVICE, torch.float32, non_blocking=True) for w, _ in (A, P, N)]
        rows = [w.squeeze(1) if w.dim() == 3 else w for w in rows]
        if not (rows[0].shape == rows[1].shape == rows[2].shape):
            raise ValueError("pad_mode 'exact': the three branches must share one (B, Nmax) storage shape (TripletDataset.collate_exact)")
        lens = [int(n) for _, l in (A, P, N) for n in (l.tolist() if torch.is_tensor(l) else l)]
        B = rows[0].shape[0]
        w = torch.cat(rows, dim=0).contiguous()
        if not training:
            e = eng.embed_ragged(None, packed=(w, lens))
            return eng.triplet_loss(e[:B].contiguous(), e[B:2 * B].contiguous(), e[2 * B:].contiguous(), self.margin,
                                    want_grad=False)[0]
        draws = [self._draw() for _ in range(3)]
        eng.train_set_stochastic(**dict(draws[0], layer_mask=0xFFF))
        eng.train_set_branches([x["layer_mask"] for x in draws])
        emb, layers, saved, batch = eng.embed_train_ragged(w, lens)
        loss, da, dp, dn = eng.triplet_loss(emb[:B].contiguous(), emb[B:2 * B].contiguous(), emb[2 * B:].contiguous(), self.margin)
        eng.train_zero_grad()
        eng.train_backward_ragged(batch, layers, saved, torch.cat([da, dp, dn], dim=0))
        eng.train_set_branches(None)
        eng.train_set_stochastic()
        if self.group is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            allreduce_mean_gradients(eng, self.group)
        lr_body, lr_head = self.lr_scheduler.get_last_lr()
        eng.adam_step(lr_body, lr_head)
        return loss

    def train(self, model=None, dataloader=None, optimizer=None, criterion=None) -> float:
        dataloader = dataloader if dataloader is not None else self.train_loader
        total = torch.zeros(1, device=self.DEVICE)
        for A, P, N in dataloader:
            total += self.train_step(A, P, N, training=True)
        return total.item() / max(len(dataloader), 1)

    def eval(self, model=None, dataloader=None, criterion=None) -> float:
        dataloader = dataloader if dataloader is not None else self.valid_loader
        total = torch.zeros(1, device=self.DEVICE)
        for A, P, N in dataloader:
            total += self.train_step(A, P, N, training=False)
        return total.item() / max(len(dataloader), 1)

    def save(self, path: str):
        torch.save(self.engine.train_state_dict(), path)

    # ---- train_triplet.py:161-205 --------------------------------------------------------------------------
    def training_loop(self):
        import yaml
        dt_string = datetime.now().strftime("%d-%m-%Y_%H-%M-%S")
        self.PATH_DIR = os.path.join("out-models", self.config["out_dir"], dt_string)
        os.makedirs(self.PATH_DIR, exist_ok=True)
        with open(os.path.join(self.PATH_DIR, "config.yaml"), "w") as file:
            yaml.dump(self.config, file)
        best_valid_loss = np.inf
        counter = 0
        rank0 = not (dist.is_available() and dist.is_initialized()) or dist.get_rank(self.group) == 0
        for i in range(self.config["num_epochs"]):
            if getattr(self, "train_sampler", None) is not None:
                self.train_sampler.set_epoch(i)
            train_loss = self.train()
            valid_loss = self.eval()  # every rank evaluates the whole validation set: identical numbers, no exchange
            if valid_loss < best_valid_loss:
                if rank0:
                    self.save(os.path.join(self.PATH_DIR, "best_model.pt"))
                best_valid_loss = valid_loss
                print("Saved Weights Success")
                counter = 0
            else:
                counter += 1
            if (counter + 1) % self.config["lr_decay_step"] == 0:
                self.lr_scheduler.step()
            print(f"COUNTER:  {counter}/{self.config['patience']}")
            print(f"LR: {self.lr_scheduler.get_last_lr()}")
            if counter > self.config["patience"]:
                print("Stop training, counter greater than patience")
                break
            print(f"EPOCHS: {i + 1} train_loss : {train_loss}")
            print(f"EPOCHS: {i + 1} valid_loss : {valid_loss}")
            print("\n")
        return best_valid_loss


    # ---- evaluation (train_triplet.py:201-489) -----------------------------------------------------------------------
    def _bind_model(self):
        """self.model / self.nomad over the current engine: an Origw2v with eval_w2v, a TripletModel otherwise."""
        if self.engine is None:
            return
        if self.precision == "bf16x3":
            # as Nomad(precision="bf16x3"): the few files that stay on fp32 buffers form their GEMM products the bf16x3 way too
            self.engine.gemm_precision = "bf16x3"
        self.nomad = Nomad.from_engine(self.engine, precision=self.precision, group=self.group)
        self.model = Origw2v(self.engine, self.precision) if self.config.get("eval_w2v") else self.nomad.model

    def _load_model(self, model_path: str, allow_w2v: bool):
        """``self.model.load_state_dict(torch.load(model_path))`` of the evaluation experiments.  With eval_w2v the reference
        skips the load in quality_nmr and intensity (train_triplet.py:233, :345); in valid_rank and quality_fr it loads
        unconditionally, which fails on an Origw2v (no embedding layer to load into): refused here with that explanation."""
        if self.config.get("eval_w2v"):
            if not allow_w2v:
                raise ValueError(f"experiment {self.config['experiment_name']!r} loads nomad_model_path into the model "
                                 "unconditionally (train_triplet.py:307, :422), which an Origw2v (eval_w2v: True) cannot take; "
                                 "the raw wav2vec 2.0 baseline is evaluated by quality_nmr and intensity only")
            return
        if self._loaded_from in ("engine", model_path):   # the caller's engine is the model; or loaded already
            return
        if self.engine is not None:
            torch.cuda.synchronize(self.DEVICE)
            self.engine.close()
        self.engine = Engine(load_pretrained(model_path, self.config.get("allow_unsafe_pickle")), self._device_index)
        self._loaded_from = model_path
        self._bind_model()

    def _figure_dir(self) -> str:
        """train_triplet.py:289: next to nomad_model_path; under ``out_dir`` when that is the word ``seeded``."""
        path = self.config["nomad_model_path"]
        out_dir = self.config.get("out_dir", ".") if path == "seeded" else "/".join(path.split("/")[:-1])
        out_dir = out_dir or "."
        os.makedirs(out_dir, exist_ok=True)
        return out_dir

    def get_embeddings_csv(self, model, file_names, root=False):
        """train_triplet.py:203-225, through the file pipeline of ``Nomad.get_embeddings_csv`` (ragged batches, bit-identical to
        one call per file; 768 feature columns for an Origw2v, 256 embedding columns otherwise)."""
        return self.nomad.get_embeddings_csv(model, file_names, root=root)

    def order_three(self, x, a, b, c, d):
        return order_three(x, a, b, c, d)

    def get_nmr_embeddings(self):
        """train_triplet.py:476-484: the embeddings of every file of ``non_match_dir``, column ``reference`` first."""
        import pandas as pd
        ref_files = pd.DataFrame(os.listdir(self.config["non_match_dir"]))
        ref_files.columns = ["reference"]
        ref_files["reference"] = [os.path.join(self.config["non_match_dir"], x) for x in ref_files["reference"]]
        return self.get_embeddings_csv(self.model, ref_files)

    def euclidean_dist(self, emb_a, emb_b):
        """train_triplet.py:487-489 (the reference's own cross-check of cdist)."""
        return np.sqrt(np.dot(emb_a - emb_b, (emb_a - emb_b).T))

    def _nmr_mean(self, test: np.ndarray, ref: np.ndarray) -> np.ndarray:
        """cdist(test, ref) + np.mean(axis=1) on the GPU (nomad_cdist: float64, difference form; the matrix is not stored)."""
        dev = self.engine.device
        _, mean = self.engine.cdist(torch.from_numpy(test).to(dev), torch.from_numpy(ref).to(dev), want_matrix=False)
        return mean.cpu().numpy()

    def _paired(self, test: np.ndarray, ref: np.ndarray) -> np.ndarray:
        """np.diag(cdist(test, ref)) on the GPU without the N x N matrix (nomad_paired_distance)."""
        dev = self.engine.device
        return self.engine.paired_distance(torch.from_numpy(test).to(dev), torch.from_numpy(ref).to(dev)).cpu().numpy()

    def eval_audio_quality(self, model_path):
        """``quality_nmr`` (train_triplet.py:231-303): per database, the mean distance to the non-matching references per
        condition against MOS.  -> {db: {table, popt, SRCC, SRCC_map, PCC, PCC_map, embeddings, ref_embeddings, figure}}."""
        import pandas as pd
        self._load_model(model_path, allow_w2v=True)
        test_data = filter_test_data(pd.read_csv(self.config["test_db_file"]), self.config.get("db"), self.config.get("conds"))
        ref_embeddings = self.get_nmr_embeddings()
        ref_embeddings.set_index("reference", inplace=True)
        results = {}
        for db_name, db in test_data.groupby("db"):
            print(db_name)
            df_emb = self.get_embeddings_csv(self.model, db["filepath_deg"], root=self.config["test_root_wav"])
            res = quality_nmr_stats(df_emb, db, ref_embeddings, self._nmr_mean)
            res["ref_embeddings"] = ref_embeddings
            res["figure"] = save_mos_scatter(res["table"], os.path.join(self._figure_dir(), f"{db_name}_embeddings.png"),
                                             "Dist w.r.t. clean embeddings")
            results[db_name] = res
        return results

    def eval_degr_level(self, model_path):
        """``valid_rank`` (train_triplet.py:305-342): the validation anchors ranked by their mean distance to the non-matching
        references.  -> {table, order, embeddings, ref_embeddings, figure}."""
        self._load_model(model_path, allow_w2v=False)
        valid_set = TripletDataset(self.config, data_mode="valid_df", level=self.config.get("current_level"))
        df_emb = self.get_embeddings_csv(self.model, valid_set.dataset["Anchor"], root=self.config["root"])
        ref_embeddings = self.get_nmr_embeddings()
        res = valid_rank_stats(df_emb, ref_embeddings, self._nmr_mean)
        res["ref_embeddings"] = ref_embeddings
        res["figure"] = save_rank_boxplot(res["table"], res["order"], os.path.join(self._figure_dir(), "validset_embeddings.png"))
        return res

    def eval_degradation_intensity(self, model_path):
        """``intensity`` (train_triplet.py:344-401): per degradation, the rank correlation of the mean distance with the
        degradation's level.  -> {degradation: {table, SRCC, embeddings, ref_embeddings}}.

        With the config key ``degrade_on_device: {clean: <dir|csv>, noise: <wav>, snr_db: [...], clip: [...], rt60: [...], reverb: [...]}`` (not a
        reference key) no rendered files and no ``test_mono_data`` are needed: the clean files are degraded on the GPU at the listed levels
        (``Nomad.intensity_sweep``: additive noise at an SNR, percentile clipping and - ``rt60``, in seconds - convolution with
        ``synthetic_rir`` rooms, which is NOT sox's reverb - or ``reverb``, the reference's own condition values: sox's reverb at these
        reverberance levels, 0 .. 100, ``Nomad.reverb``; one of the two) and the result has the same shape, with the degradations
        ``NOISE``, ``CLIP`` and ``REVERB``.  A
        further key ``normalize: -23`` brings every degraded row to that BS.1770 loudness in LUFS before it is scored, as the
        ``ffmpeg-normalize`` step of the reference's rendering scripts does (its linear gain only; no codecs); without the key the
        rows keep the level the degradation left them."""
        import pandas as pd
        on_device = self.config.get("degrade_on_device")
        if on_device and self.config.get("eval_w2v"):
            raise ValueError("degrade_on_device scores NOMAD embeddings (Nomad.intensity_sweep); the raw wav2vec 2.0 baseline "
                             "(eval_w2v: True) takes rendered files (test_mono_data)")
        self._load_model(model_path, allow_w2v=True)
        ref_embeddings = self.get_nmr_embeddings()
        ref_embeddings.set_index("reference", inplace=True)
        if on_device:
            noise = on_device.get("noise")
            results = self.nomad.intensity_sweep(
                on_device["clean"], torch.from_numpy(_emb_values(ref_embeddings)),
                noise=self.nomad.load_processing(noise).reshape(-1) if noise is not None else None,
                snr_db=on_device.get("snr_db"), clip_factor=on_device.get("clip"),
                **({"rt60_s": on_device["rt60"]} if on_device.get("rt60") is not None else {}),
                **({"reverberance": on_device["reverb"]} if on_device.get("reverb") is not None else {}),
                **({"normalize": on_device["normalize"]} if on_device.get("normalize") is not None else {}))
            for res in results.values():
                res["ref_embeddings"] = ref_embeddings
            return results
        test_data = pd.read_csv(self.config["test_mono_data"])
        results = {}
        for deg_name, deg_data in test_data.groupby("Degradation"):
            df_emb = self.get_embeddings_csv(self.model, deg_data["filepath_deg"], root=self.config["test_mono_wav"])
            res = intensity_stats(df_emb, deg_data, ref_embeddings, self._nmr_mean, deg_name)
            res["ref_embeddings"] = ref_embeddings
            results[deg_name] = res
        return results

    def eval_full_reference(self, model_path):
        """``quality_fr`` (train_triplet.py:421-474): per database, the distance of each file to its own clean reference per
        condition against MOS.  -> {db: {table, popt, SRCC, SRCC_map, PCC, PCC_map, embeddings, ref_embeddings, figure}}."""
        import pandas as pd
        self._load_model(model_path, allow_w2v=False)
        test_data = pd.read_csv(self.config["test_db_file_fr"])
        results = {}
        for db_name, db in test_data.groupby("db"):
            print(db_name)
            df_emb_ref = self.get_embeddings_csv(self.model, db["filepath_ref"], root=self.config["test_root_wav"])
            df_emb_test = self.get_embeddings_csv(self.model, db["filepath_deg"], root=self.config["test_root_wav"])
            res = quality_fr_stats(df_emb_test, df_emb_ref, db, self._paired)
            res["figure"] = save_mos_scatter(res["table"], os.path.join(self._figure_dir(), f"fr_{db_name}_embeddings.png"),
                                             "Dist w.r.t Reference")
            results[db_name] = res
        return results


def main(argv=None):
    """``python -m nomad_amd.train --config_file cfg.yaml``: the experiment choice of /root/reference/main.py:7-46 -
    ``Training``, ``quality_nmr``, ``valid_rank``, ``intensity``, ``quality_fr``."""
    import argparse
    import yaml
    ap = argparse.ArgumentParser(prog="python -m nomad_amd.train")
    ap.add_argument("--config_file", type=str, required=True)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    with open(args.config_file) as file:
        config = yaml.load(file, Loader=yaml.FullLoader)
    name = config["experiment_name"]
    if name != "Training" and name not in EVAL_EXPERIMENTS:
        raise SystemExit(f"experiment_name {name!r}: expected one of {('Training',) + EVAL_EXPERIMENTS}")
    train_obj = Training(args.config_file, device=args.device)
    if name == "Training":
        return train_obj.training_loop()
    if name == "quality_nmr":       # non-matching-reference audio quality
        return train_obj.eval_audio_quality(config["nomad_model_path"])
    if name == "valid_rank":        # ranking of the validation set's conditions
        return train_obj.eval_degr_level(config["nomad_model_path"])
    if name == "intensity":         # ranking of degradation intensities
        return train_obj.eval_degradation_intensity(config["nomad_model_path"])
    return train_obj.eval_full_reference(config["nomad_model_path"])   # quality_fr: full-reference audio quality


if __name__ == "__main__":
    main()
