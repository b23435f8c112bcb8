"""Drop-in ``Nomad`` surface over the MI355X HIP engine.

Mirrors /root/reference/src/nomad_audio/nomad.py: same class and method names, argument meaning,
return values, CSV side effects and exception messages -

* ``Nomad(device=None)``                 nomad.py:36-80
* ``predict(mode, nmr, deg, results_path) -> (df_avg_nomad, df_dm)``   nomad.py:82-140
* ``forward(estimate, clean) -> loss``   nomad.py:142-146
* ``get_embeddings(path)`` / ``get_embeddings_csv(model, file_names)``  nomad.py:148-189
* ``load_processing(filepath, target_sr, trim)``                       nomad.py:192-212
* ``TripletModel`` / ``LossNetLayers`` / ``NomadLoss``                 nomad.py:214-282

What differs, deliberately:

* all arithmetic (wav2vec 2.0 BASE backbone, head, distances, L1 loss) runs in libnomad_hip.so on
  a gfx950 GPU; there is NO CPU path - ``device='cpu'`` raises.
* nothing is downloaded at import time (no network in production clusters); the checkpoint is read
  from ``pt-models/nomad_best_model.pt`` (the reference's location, nomad.py:28) or from
  ``$NOMAD_CHECKPOINT``; ``Nomad(weights=...)`` accepts a state dict or ``'seeded'``.
* ``get_embeddings_csv`` packs clips of ANY lengths into ragged batches (one launch sequence, no
  padding in the arithmetic) instead of the reference's batch-1 loop with a device sync per clip
  (nomad.py:171-183); every clip sees exactly the arithmetic it sees at batch 1 (bit-identical).
* the distance matrix is computed on the GPU (float64, difference form) instead of SciPy.
"""
from __future__ import annotations

import contextlib
import math
import os
from datetime import datetime
from typing import Dict, List, Union

import numpy as np
import pandas as pd
import torch

from . import wavio
from .dist import partition
from .engine import Engine
from .weights import find_checkpoint, find_feature_grad_mult, load_checkpoint, num_frames, num_windows, seeded_state_dict

SSL_OUT_DIM = 768
EMB_DIM = 256


def _resolve_device(device) -> int:
    if device is None:
        # the reference falls back to the CPU here (nomad.py:40-43); this build has no CPU path, so a host without a GPU gets the
        # same clear message an explicit device='cpu' gets, not a failure somewhere inside nomad_create
        if not torch.cuda.is_available():
            raise RuntimeError("NOMAD (MI355X build) runs on a HIP GPU only and no GPU is visible to PyTorch "
                               "(device=None resolves to 'cuda'; there is no CPU path)")
        device = "cuda"
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"NOMAD (MI355X build) runs on a HIP GPU only; device={device!r} is not supported "
                           "(there is no CPU path)")
    return dev.index if dev.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)


class TripletModel:
    """``TripletModel.forward(wav, lengths=None)`` (nomad.py:224-231) on the engine."""

    def __init__(self, engine: Engine):
        self.engine = engine

    def eval(self):
        return self

    def __call__(self, wav: torch.Tensor, lengths=None) -> torch.Tensor:
        return self.forward(wav, lengths)

    def forward(self, wav: torch.Tensor, lengths=None) -> torch.Tensor:
        return self.engine.embed(wav.to(self.engine.device, torch.float32).contiguous())


class Origw2v:
    """``Origw2v.forward(wav)`` (src/models/networks.py:23-34) on the engine: the wav2vec 2.0 backbone's output averaged
    over time, (B, 768) - the baseline the evaluation experiments compare NOMAD with (``eval_w2v: True``).  Handed to
    ``get_embeddings_csv`` as ``model`` it makes the file pipeline produce these 768 columns."""

    def __init__(self, engine: Engine, precision: str = "fp32"):
        self.engine = engine
        self.precision = precision

    def eval(self):
        return self

    def __call__(self, wav: torch.Tensor) -> torch.Tensor:
        return self.forward(wav)

    def forward(self, wav: torch.Tensor) -> torch.Tensor:
        return self.engine.embed_features(wav.to(self.engine.device, torch.float32).contiguous(), precision=self.precision)


def _takes_bf16x3(precision: str, wav: torch.Tensor) -> bool:
    return precision == "bf16x3" and wav.numel() >= BF16X3_MIN_SAMPLES


class LossNetLayers:
    """``LossNetLayers.forward(wav)`` (nomad.py:243-258): 12 layer outputs (B,T,768) + embedding.

    Owns its own ``Linear(768,256)`` like the reference (nomad.py:238-241) - freshly initialised and
    never loaded from the checkpoint - exposed as ``embedding_weight`` / ``embedding_bias`` so callers
    that need reproducibility can set it.
    """

    def __init__(self, engine: Engine, ssl_out_dim: int = SSL_OUT_DIM, emb_dim: int = EMB_DIM, precision: str = "fp32"):
        self.engine = engine
        self.precision = precision     # "bf16x3": batches of at least BF16X3_MIN_SAMPLES samples take the split-bf16 forward
        lin = torch.nn.Linear(ssl_out_dim, emb_dim)
        self.embedding_weight = lin.weight.detach().to(engine.device).contiguous()
        self.embedding_bias = lin.bias.detach().to(engine.device).contiguous()

    def __call__(self, wav, lengths=None):
        return self.forward(wav, lengths)

    def forward(self, wav: torch.Tensor, lengths=None) -> List[torch.Tensor]:
        """lengths (B ints, tensor or list; ``wav`` (B,1,N) or (B,N), samples behind a length are never read): the clips at their
        exact lengths in one launch sequence - 12 PACKED layer outputs (M,768), M = the sum of the clips' frames, clip after
        clip, + the (B,256) embedding.  fp32 buffers whatever ``precision`` says (products follow ``Engine.gemm_precision``):
        there is no ragged layer-output forward on split bf16 storage."""
        wav = wav.to(self.engine.device, torch.float32).contiguous()
        if lengths is not None:
            lens = check_lengths(wav, lengths)
            emb, layers, _, _ = self.engine.embed_train_ragged(wav, lens, head=(self.embedding_weight, self.embedding_bias), save=False)
            return [layers[i] for i in range(12)] + [emb]
        fwd = self.engine.embed_bf16x3 if _takes_bf16x3(self.precision, wav) else self.engine.embed
        emb, layers = fwd(wav, head=(self.embedding_weight, self.embedding_bias), want_layers=True)
        return [layers[i] for i in range(12)] + [emb]


def loss_selection(L, layer_weights=None):
    """(``NomadLoss.L``, ``layer_weights``) -> (13 weights, encoder depth): which terms of the loss count, and how many encoder
    layers they need.  Pure host arithmetic.

    layer_weights None: the reference's ``for i in range(self.L)`` (nomad.py:276) - weights ``[1] * L + [0] * (13 - L)`` for an
    integer L in 1 .. 13.  The reference returns the float 0.0 at L = 0 (nothing to call ``backward`` on) and raises IndexError
    above 13 (``LossNetLayers`` returns 13 entries); both are a ValueError here.  Otherwise 13 finite numbers >= 0, not all 0:
    the 12 layers' weights, then the embedding's.  depth: 12 when the embedding counts (it is computed from the last layer), else
    1 + the deepest layer with a weight."""
    if layer_weights is None:
        if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or not 1 <= int(L) <= 13:
            raise ValueError(f"nomad_loss.L must be an integer in 1 .. 13 (12 transformer layers + the embedding), got {L!r}")
        weights = [1.0] * int(L) + [0.0] * (13 - int(L))
    else:
        if torch.is_tensor(layer_weights):
            layer_weights = layer_weights.detach().reshape(-1).tolist()
        weights = [float(w) for w in layer_weights]
        if len(weights) != 13:
            raise ValueError(f"layer_weights needs 13 numbers (12 transformer layers + the embedding), got {len(weights)}")
        if any(not math.isfinite(w) or w < 0.0 for w in weights):
            raise ValueError("layer_weights must be finite and >= 0")
        if not any(w != 0.0 for w in weights):
            raise ValueError("layer_weights are all zero: the loss would have no term")
    depth = 12 if weights[12] != 0.0 else 1 + max(i for i in range(12) if weights[i] != 0.0)
    return weights, depth


NSIM_FRAME_SAMPLES = 1280   # one 80 ms gammatone frame at 16 kHz


def check_reduction(reduction) -> str:
    if reduction not in ("mean", "none"):
        raise ValueError(f"reduction must be 'mean' or 'none', got {reduction!r}")
    return reduction


class NomadLoss:
    """``NomadLoss.forward(nomad_ref, nomad_test)`` (nomad.py:267-282): sum of the first ``L`` of 13 L1 means (``L = 13``)."""

    def __init__(self, engine: Engine):
        self.engine = engine
        self.L = 13   # read by Nomad.forward (loss_selection) and by forward below, like the reference's `for i in range(self.L)`
        self.only_embedding = False

    def eval(self):
        return self

    def __call__(self, nomad_ref, nomad_test):
        return self.forward(nomad_ref, nomad_test)

    def forward(self, nomad_ref, nomad_test) -> torch.Tensor:
        if self.only_embedding:
            # the reference's other branch (nomad.py:270-273) reads element 13 of the lists - one past what LossNetLayers
            # returns, an IndexError there and here; with longer lists it is the L1 distance of that entry alone
            ref, test = nomad_ref[13], nomad_test[13]
            return (test - ref).abs().mean()
        ref_layers = _stack_layers(nomad_ref[:12])
        test_layers = _stack_layers(nomad_test[:12])
        if self.L != 13:
            if test_layers.dim() != 4:
                raise ValueError("NomadLoss.L below 13 over packed (exact-length) layer outputs needs the clips' lengths: use "
                                 "Nomad.forward(estimate, clean, lengths)")
            weights, _ = loss_selection(self.L)
            return self.engine.l1_loss_weighted(test_layers, ref_layers, nomad_test[12].contiguous(), nomad_ref[12].contiguous(),
                                                weights, want_terms=False)[0]
        return self.engine.l1_loss(test_layers, ref_layers, nomad_test[12].contiguous(), nomad_ref[12].contiguous())


MIN_SAMPLES = 400   # one encoder frame (the conv stack's receptive field)


def check_lengths(wav: torch.Tensor, lengths) -> List[int]:
    """The ``lengths`` argument of ``Nomad.forward`` / ``LossNetLayers.forward`` as a list of ints, checked against ``wav``
    ((B,1,N) or (B,N)): one entry per clip, each at least one encoder frame (400 samples) and at most N."""
    if wav.dim() not in (2, 3) or (wav.dim() == 3 and wav.shape[1] != 1):
        raise ValueError(f"with lengths the waveforms must be (B,1,N) or (B,N), got {tuple(wav.shape)}")
    if torch.is_tensor(lengths):
        if lengths.dim() != 1 or lengths.is_floating_point():
            raise ValueError("lengths must be a 1-D integer tensor or a list of ints")
        lengths = lengths.tolist()
    lens = [int(n) for n in lengths]
    if len(lens) != wav.shape[0]:
        raise ValueError(f"lengths has {len(lens)} entries for a batch of {wav.shape[0]} clips")
    for i, n in enumerate(lens):
        if n < MIN_SAMPLES or n > wav.shape[-1]:
            raise ValueError(f"lengths[{i}] = {n} is outside [{MIN_SAMPLES}, {wav.shape[-1]}]")
    return lens


def _stack_layers(layers) -> torch.Tensor:
    """The 12 tensors LossNetLayers returns are views of one (12,B,T,768) buffer (a ragged batch: (12,M,768)): reuse it."""
    base = layers[0]._base if layers[0]._base is not None else None
    if base is not None and base.dim() == layers[0].dim() + 1 and base.shape[0] == 12 and all(
            l._base is base and l.data_ptr() == base[i].data_ptr() for i, l in enumerate(layers)):
        return base
    return torch.stack([l.contiguous() for l in layers])


@contextlib.contextmanager
def _encoder_cut(eng: Engine, selection):
    """The engine's ``encoder_depth`` set to the selection's around the engine calls of a pass and restored behind them: nothing else
    that uses the engine ever sees a cut encoder.  The plain loss (selection None) neither reads nor sets it."""
    if selection is None:
        yield
        return
    prev = eng.encoder_depth
    eng.encoder_depth = selection[1]
    try:
        yield
    finally:
        eng.encoder_depth = prev


class _NomadLossFn(torch.autograd.Function):
    """loss = NomadLoss(LossNetLayers(clean), LossNetLayers(estimate)); backward = d loss / d estimate and, when ``clean`` requires a
    gradient too, d loss / d clean - the reference's ``forward`` (nomad.py:142-146) is differentiable in both arguments.

    lens: None, or the clips' exact lengths (``Nomad.forward(estimate, clean, lengths)``) - both branches then run the ragged forward
    on fp32 buffers (no padding in the arithmetic, packed layer outputs), the loss terms are means over the valid frames, and the
    gradient is zero behind every length.  selection: None - the 13-term mean, ``l1_loss`` and its backward - or (13 weights,
    encoder depth, reduction) from ``loss_selection``: a weight per term, a loss per clip (reduction "none") and the encoder cut
    behind the deepest layer with a weight (``l1_loss_weighted``, whose kernels fold in another order: other bits than ``l1_loss``
    where both apply)."""

    @staticmethod
    def forward(ctx, estimate, clean, nomad, lens, selection):
        eng = nomad.engine
        head = (nomad.lossnet_layers.embedding_weight, nomad.lossnet_layers.embedding_bias)
        est = estimate.detach().to(eng.device, torch.float32).contiguous()
        cln = clean.detach().to(eng.device, torch.float32).contiguous()
        need_grad = estimate.requires_grad
        need_clean_grad = clean.requires_grad
        frames = None if lens is None else [num_frames(n) for n in lens]
        # precision="bf16x3": the branches that carry no gradient (always `clean`; `estimate` too under no_grad) run
        # the split-bf16 forward (layer outputs within ~1e-5 of fp32); the branch that is differentiated stays on fp32 BUFFERS
        # (embed_train), its GEMM products in whatever Engine.gemm_precision says - "bf16x3" when the Nomad was made with
        # precision="bf16x3", exact fp32 otherwise.  A cut encoder exists on fp32 buffers only: no embed_bf16x3 below depth 12
        x3 = (selection is None or selection[1] == 12) and _takes_bf16x3(nomad.precision, cln)

        def branch(wav, save, side):
            """One LossNetLayers forward -> (emb, layers, saved block or None, the waveform buffer its backward takes)."""
            if lens is not None:
                emb, layers, saved, batch = eng.embed_train_ragged(wav, lens, head, save=save, side=side)
                return emb, layers, saved, batch[0]
            if save:
                return (*eng.embed_train(wav, head), wav)
            emb, layers = (eng.embed_bf16x3 if x3 else eng.embed)(wav, head=head, want_layers=True, side=side)
            return emb, layers, None, wav

        with _encoder_cut(eng, selection):
            if need_clean_grad:
                # the uncommon case (the speech-enhancement example differentiates `estimate` only, nomad_loss_test.py:69): the clean
                # branch keeps its activations too, on the caller's stream - the training-mode forward has one workspace per context
                c_emb, c_layers, saved_c, cln = branch(cln, True, False)
            else:
                # the two forwards are independent: at training batch sizes (32 x 1 s) one of them fills less than half
                # of the chip, so the clean branch runs concurrently on a side stream with its own workspace
                cur, side = torch.cuda.current_stream(eng.device), eng.side_stream()
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    c_emb, c_layers, saved_c, cln = branch(cln, False, True)
            e_emb, e_layers, saved, est = branch(est, need_grad, False)
            if not need_clean_grad:
                cur.wait_stream(side)
                for t in (c_emb, c_layers, cln):
                    t.record_stream(cur)
            if selection is None:
                loss = eng.l1_loss(e_layers, c_layers, e_emb, c_emb)
            else:
                loss, _ = eng.l1_loss_weighted(e_layers, c_layers, e_emb, c_emb, selection[0], selection[2], frames, want_terms=False)
        if need_grad or need_clean_grad:
            ctx.nomad = nomad
            ctx.sel = (lens, frames, selection)
            ctx.shapes = (estimate.shape, clean.shape)
            ctx.save_for_backward(est, e_layers, e_emb, cln, c_layers, c_emb, saved, saved_c)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        est, e_layers, e_emb, cln, c_layers, c_emb, saved, saved_c = ctx.saved_tensors
        eng = ctx.nomad.engine
        lens, frames, selection = ctx.sel
        head = (ctx.nomad.lossnet_layers.embedding_weight, ctx.nomad.lossnet_layers.embedding_bias)

        # Per utterance, clip b's rows are linear in upstream[b]: the chain runs with upstream 1 - every clip's own gradient, the
        # bits of its B = 1 call - and row b is scaled once at the end.  (Scaled at the start, v_b * gradient would carry the
        # rounding of the whole chain again, ~2e-6 of it for a v_b that is no power of two.)
        per_clip = selection is not None and selection[2] == "none"
        up = torch.ones(grad_out.numel(), dtype=torch.float32, device=eng.device) if per_clip else grad_out

        def branch(wav, layers, emb, o_layers, o_emb, sv):   # |e - c| is symmetric: the clean side is the same call, arguments swapped
            if selection is None:
                dl, de = eng.l1_loss_backward(layers, o_layers, emb, o_emb, up)
            else:
                weights, depth, reduction = selection
                dl, de = eng.l1_loss_weighted_backward(layers, o_layers, emb, o_emb, up, weights, reduction, frames, depth)
                if de is None and depth == 12:   # the whole encoder, no embedding term: its head backward gets zeros
                    de = torch.zeros_like(emb)
            if lens is None:
                d = eng.embed_backward(wav, layers, sv, dl, de, head)
            else:
                d = eng.embed_backward_ragged((wav, lens), layers, sv, dl, de, head)
            return d * grad_out.to(d.device, torch.float32).reshape(-1, 1) if per_clip else d

        dwav = dcln = None
        with _encoder_cut(eng, selection):
            if saved is not None and ctx.needs_input_grad[0]:
                dwav = branch(est, e_layers, e_emb, c_layers, c_emb, saved).reshape(ctx.shapes[0])
            if saved_c is not None and ctx.needs_input_grad[1]:
                dcln = branch(cln, c_layers, c_emb, e_layers, e_emb, saved_c).reshape(ctx.shapes[1])
        return dwav, dcln, None, None, None


def check_references(references) -> None:
    """The ``references`` argument of ``Nomad.score``: a 2-D floating-point tensor of at least one 256-dimensional embedding, as
    ``nomad.model(wav)`` or ``get_embeddings`` make them.  Pure: looks at type, dtype and shape only."""
    if not torch.is_tensor(references):
        raise TypeError(f"references must be a tensor of embeddings, got {type(references).__name__}")
    if not references.is_floating_point():
        raise TypeError(f"references must be a floating-point tensor, got {references.dtype}")
    if references.dim() != 2 or references.shape[1] != EMB_DIM:
        raise ValueError(f"references must be (Nr, {EMB_DIM}) embeddings, got {tuple(references.shape)}")
    if references.shape[0] < 1:
        raise ValueError("references holds no embedding: the score is a mean over at least one reference")


KNN_MAX = 64   # nomad_knn's widest neighbourhood


def check_k(k, Nr: int) -> int:
    """The ``k`` of the nearest-reference scores against a bank of ``Nr`` references: an integer (not a bool) from 1 to
    ``min(64, Nr)``.  Pure; raises before any engine call."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"k must be an integer from 1 to min({KNN_MAX}, the number of references = {Nr}), got {k!r}")
    if k < 1 or k > KNN_MAX or k > Nr:
        raise ValueError(f"k = {int(k)} is outside 1 .. min({KNN_MAX}, the number of references = {Nr})")
    return int(k)


FRAMES_PER_SECOND = 50   # one encoder frame is 320 samples at 16 kHz; its receptive field is 400 samples


def window_frames(window_s, hop_s):
    """Window length and hop in seconds -> (win, hop) in encoder frames: ``max(1, round(s * 50))`` each.  Pure."""
    out = []
    for name, s in (("window_s", window_s), ("hop_s", hop_s)):
        if isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)) or not math.isfinite(s) or s <= 0:
            raise ValueError(f"{name} must be a positive number of seconds, got {s!r}")
        out.append(max(1, int(round(float(s) * FRAMES_PER_SECOND))))
    return out[0], out[1]


def window_times(T: int, win: int, hop: int):
    """(start_s, end_s) float64 arrays of the ``num_windows(T, win, hop)`` windows of a clip of T frames: window k of n =
    min(win, T) frames starts at ``k * hop * 0.02`` s and ends ``(n * 320 + 80) / 16000`` s later - the samples its frames
    see.  Both are formed as integer milliseconds / 1000, so they sit on the 3-decimal grid of the CSV writer."""
    k = np.arange(num_windows(T, win, hop), dtype=np.int64)
    n = min(int(win), int(T))
    return (k * hop * 20) / 1000.0, ((k * hop + n) * 20 + 5) / 1000.0


def segments_tables(test_files, frames, scores, win: int, hop: int):
    """The tables of ``Nomad.predict_segments``: file labels, the files' frame counts and the window scores (files in order,
    each file's windows in order) -> (one row per window: ``Test File``, ``start_s``, ``end_s``, ``NOMAD`` rounded to 3
    decimals; one row per file, indexed by ``Test File``: ``NOMAD`` = the mean of the file's window scores, rounded)."""
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    counts = [num_windows(t, win, hop) for t in frames]
    if len(test_files) != len(counts) or sum(counts) != scores.shape[0]:
        raise ValueError(f"{scores.shape[0]} window scores for {len(test_files)} files with {sum(counts)} windows")
    times = [window_times(t, win, hop) for t in frames]
    df = pd.DataFrame({"Test File": np.repeat(np.asarray(test_files, dtype=object), counts),
                       "start_s": np.concatenate([t[0] for t in times]) if times else np.zeros(0),
                       "end_s": np.concatenate([t[1] for t in times]) if times else np.zeros(0),
                       "NOMAD": scores}).round({"NOMAD": 3})
    ends = np.cumsum(counts)
    means = [scores[e - c:e].mean() for c, e in zip(counts, ends)]
    df_mean = pd.DataFrame({"Test File": list(test_files), "NOMAD": np.asarray(means, dtype=np.float64)}).set_index("Test File").round(3)
    return df, df_mean


def span_frames(start_s, end_s, T: int):
    """A span in seconds -> (t0, t1), encoder frames [t0, t1) of a clip of T frames: ``t0 = round(start_s * 50)``, ``t1 =
    round((end_s - 0.005) * 50)``, both clamped to [0, T].  The inverse of ``window_times``: a window's (start_s, end_s) gives that
    window's frames back (its end is the last sample its frames SEE, 80 samples = 5 ms past their 20 ms grid).  Pure; a span that
    is empty after clamping raises a ValueError that names it."""
    for name, s in (("start_s", start_s), ("end_s", end_s)):
        if isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)) or not math.isfinite(s):
            raise ValueError(f"{name} must be a finite number of seconds, got {s!r}")
    T = int(T)
    t0 = min(max(int(round(float(start_s) * FRAMES_PER_SECOND)), 0), T)
    t1 = min(max(int(round((float(end_s) - 0.005) * FRAMES_PER_SECOND)), 0), T)
    if t1 <= t0:
        raise ValueError(f"the span ({start_s!r} s, {end_s!r} s) holds no frame of a clip of {T} frames (frames [{t0}, {t1}))")
    return t0, t1


def span_times(t0: int, t1: int):
    """Frames [t0, t1) -> (start_s, end_s) on ``window_times``' 3-decimal grid: ``span_frames`` gives (t0, t1) back."""
    return (int(t0) * 20) / 1000.0, (int(t1) * 20 + 5) / 1000.0


def active_frames(energy, floor_db: float = 40.0, min_speech_frames: int = 5, min_gap_frames: int = 15):
    """The rule of ``Nomad.active_spans`` on one clip's frame energies (a 1-D array) -> a list of (t0, t1) in frames.  Pure.
    1. a frame is active when ``e[t] >= max(e) * 10 ** (-floor_db / 10)``; 2. inactive runs of at most ``min_gap_frames`` frames
    between two active frames become active; 3. active runs shorter than ``min_speech_frames`` frames are dropped; 4. if nothing is
    left, or ``max(e)`` is 0 or not finite, the whole clip [0, T) is returned.  An energy gate, not a speech detector."""
    e = np.asarray(energy, dtype=np.float64).reshape(-1)
    T = int(e.shape[0])
    if T < 1:
        raise ValueError("a clip has at least one frame")
    top = float(np.max(e))
    if not math.isfinite(top) or top <= 0.0:
        return [(0, T)]
    active = e >= top * 10.0 ** (-float(floor_db) / 10.0)

    def runs(mask):
        edge = np.flatnonzero(np.diff(np.concatenate(([False], mask, [False])).astype(np.int8)))
        return list(zip(edge[0::2].tolist(), edge[1::2].tolist()))

    on = runs(active)
    for (_, a), (b, _) in zip(on[:-1], on[1:]):      # the gap [a, b) lies between two active frames
        if b - a <= int(min_gap_frames):
            active[a:b] = True
    kept = [(a, b) for a, b in runs(active) if b - a >= int(min_speech_frames)]
    return kept if kept else [(0, T)]


def span_table(rows, frames, unit: str = "s"):
    """The Python form of the spans -> the table ``Engine.embed_spans_ragged`` takes, ``(row_clip, row_ptr, spans)``, and the rows
    per clip.  ``rows[c]`` is the list of rows of clip c (empty: the clip has none); a row is one ``(start, end)`` pair or a list
    of them, in seconds (``span_frames``) or, with unit="frames", frames [t0, t1) as they are.  frames[c]: the clip's frame count.
    Spans inside a row must be ascending and must not overlap; the error names clip, row and span.  Pure."""
    if unit not in ("s", "frames"):
        raise ValueError(f"unit must be 's' or 'frames', got {unit!r}")
    if len(rows) != len(frames):
        raise ValueError(f"spans holds the rows of {len(rows)} clips for a batch of {len(frames)}")
    row_clip, row_ptr, spans, counts = [], [0], [], []
    for c, clip_rows in enumerate(rows):
        counts.append(len(clip_rows))
        for r, row in enumerate(clip_rows):
            row = list(row)
            if len(row) == 2 and not isinstance(row[0], (list, tuple, np.ndarray)):
                row = [tuple(row)]
            if not row:
                raise ValueError(f"clip {c}, row {r} has no span")
            for s, pair in enumerate(row):
                if len(pair) != 2:
                    raise ValueError(f"clip {c}, row {r}, span {s}: expected a (start, end) pair, got {pair!r}")
                if unit == "s":
                    try:
                        t0, t1 = span_frames(pair[0], pair[1], frames[c])
                    except ValueError as err:
                        raise ValueError(f"clip {c}, row {r}, span {s}: {err}") from None
                else:
                    t0, t1 = int(pair[0]), int(pair[1])
                    if t0 < 0 or t1 > frames[c] or t0 >= t1:
                        raise ValueError(f"clip {c}, row {r}, span {s} is [{t0}, {t1}): not inside the clip's {frames[c]} frames")
                if s and t0 < spans[-1][1]:
                    raise ValueError(f"clip {c}, row {r}, span {s} [{t0}, {t1}) overlaps or precedes the span before it")
                spans.append((t0, t1))
            row_clip.append(c)
            row_ptr.append(len(spans))
    if not row_clip:
        raise ValueError("spans holds no row")
    return (row_clip, row_ptr, spans), counts


def spans_from_csv(spans, test_files):
    """The csv form of ``Nomad.predict_spans``: a DataFrame or a csv path with the columns ``Test File``, ``start_s``, ``end_s`` and
    optionally ``Row`` -> {test file: [(row label, [(start_s, end_s), ...]), ...]}, rows in the order their first line appears,
    a row's spans ascending by start.  Lines that share a ``Row`` label (of the same file) pool into one row; without the column
    every line is a row of its own, labelled by its position among the file's lines.  A file that ``test_files`` does not list is
    an error; a listed file without a line gets no row."""
    df = pd.read_csv(spans) if isinstance(spans, (str, os.PathLike)) else spans
    if not isinstance(df, pd.DataFrame):
        raise TypeError(f"spans must be a DataFrame or the path of a csv file, got {type(spans).__name__}")
    missing = [c for c in ("Test File", "start_s", "end_s") if c not in df.columns]
    if missing:
        raise ValueError(f"the span table lacks the column(s) {missing}: it needs Test File, start_s, end_s (and optionally Row)")
    known = set(test_files)
    out = {}
    for i, (f, a, b) in enumerate(zip(df["Test File"], df["start_s"], df["end_s"])):
        f = str(f)
        if f not in known:
            raise ValueError(f"the span table names the test file {f!r} (line {i}), which is not among the test files")
        rows = out.setdefault(f, [])
        if "Row" in df.columns:
            label = df["Row"].iloc[i]
            row = next((r for r in rows if r[0] == label), None)
            if row is None:
                rows.append((label, [(float(a), float(b))]))
            else:
                row[1].append((float(a), float(b)))
        else:
            rows.append((len(rows), [(float(a), float(b))]))
    for rows in out.values():
        for _, pairs in rows:
            pairs.sort()
    return out


def nearest_table(test_files, ref_names, knn_dist, knn_idx) -> pd.DataFrame:
    """The third table of ``Nomad.predict(k=...)``: one row per test file, indexed by ``Test File``, with the columns ``Ref 1``,
    ``Dist 1``, ... ``Ref k``, ``Dist k`` - the names of the file's nearest references (as the matrix's columns are named), nearest
    first, and the distances rounded to 3 decimals.  knn_dist (N,k) float64, knn_idx (N,k) integers into ``ref_names``."""
    knn_dist = np.asarray(knn_dist, dtype=np.float64)
    knn_idx = np.asarray(knn_idx, dtype=np.int64)
    names = np.asarray(list(ref_names), dtype=object)
    cols = {"Test File": list(test_files)}
    for r in range(knn_idx.shape[1]):
        cols[f"Ref {r + 1}"] = names[knn_idx[:, r]] if len(names) else np.zeros(0, dtype=object)
        cols[f"Dist {r + 1}"] = np.round(knn_dist[:, r], 3)
    return pd.DataFrame(cols).set_index("Test File")


def _check_predict_paths(mode, nmr, deg) -> None:
    """The argument checks of ``predict`` (same conditions, same messages)."""
    if nmr is None:
        raise Exception("nmr_path not specified, you need to pass a valid value to nmr_path")
    if deg is None:
        raise Exception("test_path not specified, you need to pass a valide value to test_path")
    if mode == "dir":
        if not os.path.isdir(nmr):
            raise Exception(f"Path to the non-matching reference files {nmr} does not exist")
        if not os.path.isdir(deg):
            raise Exception(f"Path to the test files {deg} does not exist")
    elif mode == "csv":
        if not os.path.isfile(nmr):
            raise Exception(f"File {nmr} does not exist")
        if not os.path.isfile(deg):
            raise Exception(f"File {deg} does not exist")
    else:
        raise Exception(f"Mode value {mode} is not valid. Valid values are dir and csv")


def _file_table(path) -> pd.DataFrame:
    """The file listing of ``get_embeddings``: a directory's entries, or a csv file's ``filename`` column."""
    if os.path.isdir(path):
        return pd.DataFrame({"filename": [os.path.join(path, x) for x in os.listdir(path)]})
    if os.path.isfile(path):
        data = pd.read_csv(path)
        if "filename" not in data.columns:
            raise Exception(f"File {path} not including a column called filename. Please pass a csv file with a "
                            "column called filename that includes the absolute filpaths of the waveforms.")
        return data
    raise Exception(f"Path {path} does not exist")


def pairs_from_csv(table):
    """The (clean, degraded) file pairs of ``nsim_files`` -> (clean paths, degraded paths): a csv path or a DataFrame with the
    columns ``filepath_ref`` and ``filepath_deg`` - what the reference's data preparation writes as
    ``degraded_data_visqol_format.csv``.  Other columns are ignored; the rows keep their order."""
    if isinstance(table, (str, os.PathLike)):
        if not os.path.isfile(table):
            raise ValueError(f"File {table} does not exist")
        table = pd.read_csv(table)
    if not isinstance(table, pd.DataFrame):
        raise ValueError("the pairs are a csv path or a DataFrame with the columns filepath_ref and filepath_deg")
    missing = [c for c in ("filepath_ref", "filepath_deg") if c not in table.columns]
    if missing:
        raise ValueError(f"the pairs table lacks the column(s) {', '.join(missing)}: filepath_ref and filepath_deg are needed")
    if len(table) == 0:
        raise ValueError("the pairs table has no rows")
    if table[["filepath_ref", "filepath_deg"]].isna().any().any():
        raise ValueError("the pairs table has an empty filepath_ref or filepath_deg")
    return [str(p) for p in table["filepath_ref"]], [str(p) for p in table["filepath_deg"]]


def check_patch_params(patch_s, search_s=1.2, vad_db=40.0, min_active=1.0):
    """The patch parameters of ``nsim_patches`` / ``nsim`` / ``nsim_files`` / ``mine_triplets`` -> (patch, search, vad_ratio,
    min_active_frames) as ``nomad_nsim_patches`` takes them: seconds to frames of 20 ms (patch 1 .. 64, search 0 .. 128),
    ``vad_ratio = 10 ** (-vad_db / 10)`` formed here and handed down as that double, ``max(1, ceil(min_active * patch))``."""
    for name, v in (("patch_s", patch_s), ("search_s", search_s), ("vad_db", vad_db), ("min_active", min_active)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    patch, search = int(round(float(patch_s) * 50.0)), int(round(float(search_s) * 50.0))
    if not 1 <= patch <= Engine.NSIM_PATCH_MAX:
        raise ValueError(f"patch_s must lie in 0.02 .. {Engine.NSIM_PATCH_MAX / 50.0} s (1 .. {Engine.NSIM_PATCH_MAX} frames of 20 ms), got {patch_s}")
    if search_s < 0 or search > Engine.NSIM_SEARCH_MAX:
        raise ValueError(f"search_s must lie in 0 .. {Engine.NSIM_SEARCH_MAX / 50.0} s (0 .. {Engine.NSIM_SEARCH_MAX} frames of 20 ms), got {search_s}")
    vad_ratio = 10.0 ** (-float(vad_db) / 10.0)
    if vad_db < 0 or not vad_ratio > 0.0:
        raise ValueError(f"vad_db must lie in 0 .. 3000 dB under the clip's loudest frame, got {vad_db}")
    if not 0.0 < min_active <= 1.0:
        raise ValueError(f"min_active must be a share of a patch's frames in (0, 1], got {min_active}")
    return patch, search, vad_ratio, max(1, int(math.ceil(float(min_active) * patch)))


def check_max_delay(max_delay_s, sample_rate: int = 16000) -> int:
    """``max_delay_s`` of ``align`` / ``nsim`` / ``nsim_files`` -> whole samples: a finite number of seconds from 0 up to 16384
    samples (1.024 s at 16 kHz), rounded to the nearest sample."""
    if isinstance(max_delay_s, bool) or not isinstance(max_delay_s, (int, float, np.integer, np.floating)) or not math.isfinite(max_delay_s):
        raise ValueError(f"max_delay_s must be a finite number of seconds, got {max_delay_s!r}")
    samples = int(round(float(max_delay_s) * sample_rate))
    if max_delay_s < 0 or samples > Engine.ALIGN_MAX_DELAY:
        raise ValueError(f"max_delay_s must lie in 0 .. {Engine.ALIGN_MAX_DELAY / sample_rate} s ({Engine.ALIGN_MAX_DELAY} samples), got {max_delay_s}")
    return samples


class _CdistFn(torch.autograd.Function):
    """``Engine.cdist`` with a backward: (dist, mean) -> d / d a and d / d b through ``Engine.cdist_backward``."""

    @staticmethod
    def forward(ctx, a, b, engine):
        ctx.set_materialize_grads(False)
        a, b = a.detach(), b.detach()
        dist, mean = engine.cdist(a, b)
        ctx.engine = engine
        ctx.save_for_backward(a, b)
        return dist, mean

    @staticmethod
    def backward(ctx, g_dist, g_mean):
        a, b = ctx.saved_tensors
        want_a, want_b = ctx.needs_input_grad[:2]
        if (g_dist is None and g_mean is None) or not (want_a or want_b):
            return None, None, None
        up = [None if g is None else g.to(a.device, torch.float64).contiguous() for g in (g_dist, g_mean)]
        da, db = ctx.engine.cdist_backward(a, b, up[0], up[1], want_a=want_a, want_b=want_b)
        return da, db, None


def cdist(engine: Engine, a: torch.Tensor, b: torch.Tensor):
    """a (Na,D), b (Nb,D) contiguous fp32 on the GPU -> (dist (Na,Nb), mean (Na,)) float64 with the values of ``Engine.cdist``,
    differentiable in ``a`` and ``b``: float64 sums in a fixed order, rounded to fp32 once; a pair at distance 0 contributes
    nothing to either gradient (``torch.cdist``'s convention)."""
    return _CdistFn.apply(a, b, engine)


class _ClipRows:
    """What ``_ScoreFn`` scores: one row per clip (``Nomad.score``)."""

    def embed(self, nomad, est, lens):
        return nomad._score_embed(est, lens)

    def embed_train(self, eng, est, lens):
        if lens is None:
            return (*eng.embed_train(est), est)
        emb, layers, saved, (est, _) = eng.embed_train_ragged(est, lens)
        return emb, layers, saved, est

    def backward(self, eng, est, lens, layers, saved, demb):
        if lens is None:
            return eng.embed_backward(est, layers, saved, None, demb)
        return eng.embed_backward_ragged((est, lens), layers, saved, None, demb)


class _WindowRows:
    """... one row per window of ``win`` frames every ``hop`` (``Nomad.score_windows``)."""

    def __init__(self, win, hop):
        self.win, self.hop = win, hop

    def embed(self, nomad, est, lens):
        if lens is None:
            return nomad.engine.embed_windows(est, self.win, self.hop, precision=nomad._window_precision(est.numel()))[0]
        return nomad.engine.embed_windows_ragged([est[i, :n] for i, n in enumerate(lens)], self.win, self.hop,
                                                 precision=nomad._window_precision(sum(lens)))[0]

    def embed_train(self, eng, est, lens):
        if lens is None:
            emb, _, layers, saved = eng.embed_train_windows(est, self.win, self.hop)
        else:
            emb, _, layers, saved, (est, _) = eng.embed_train_windows_ragged(est, self.win, self.hop, lens)
        return emb, layers, saved, est

    def backward(self, eng, est, lens, layers, saved, demb):
        if lens is None:
            return eng.embed_windows_backward(est, layers, saved, demb, self.win, self.hop)
        return eng.embed_windows_backward_ragged((est, lens), layers, saved, demb, self.win, self.hop)


class _TableRows:
    """... one row per row of a span table (``Nomad.score_spans``: always with ``lens``)."""

    def __init__(self, table):
        self.table = table

    def embed(self, nomad, est, lens):
        return nomad.engine.embed_spans_ragged([est[i, :n] for i, n in enumerate(lens)], self.table,
                                               precision=nomad._window_precision(sum(lens)))

    def embed_train(self, eng, est, lens):
        emb, layers, saved, (est, _) = eng.embed_train_spans_ragged(est, self.table, lens)
        return emb, layers, saved, est

    def backward(self, eng, est, lens, layers, saved, demb):
        return eng.embed_spans_backward_ragged((est, lens), layers, saved, demb, self.table)


class _ScoreFn(torch.autograd.Function):
    """score[r] = mean_j ||emb_r - references_j|| with the checkpoint's head, over the rows ``rows`` names: clips, windows or the rows
    of a span table (above).  backward = d / d estimate through ``cdist_backward`` over the rows and the rows' own ``backward`` -
    ``embed_backward[_ragged]`` with layer gradients NULL, ``embed_windows_backward[_ragged]`` or ``embed_spans_backward_ragged``: the
    head's backward and the backbone down to the waveform - and, when asked for, d / d references.  With ``k`` the mean runs over the
    k nearest references (``Engine.knn``; the backward is ``Engine.knn_backward`` on the saved selection)."""

    @staticmethod
    def forward(ctx, estimate, references, nomad, lens, rows, k):
        eng = nomad.engine
        est = estimate.detach().to(eng.device, torch.float32).contiguous()
        est = est.squeeze(1) if est.dim() == 3 else est
        refs = references.detach().to(eng.device, torch.float32).contiguous()
        ctx.nomad, ctx.lens, ctx.rows = nomad, lens, rows
        ctx.meta = (estimate.shape, references.device, references.dtype)
        if not estimate.requires_grad:   # only the references are differentiated: the scoring forward will do
            emb, layers, saved = rows.embed(nomad, est, lens), None, None
        else:
            emb, layers, saved, est = rows.embed_train(eng, est, lens)
        idx = None
        if k is None:
            _, mean = eng.pairwise(emb, refs, want_matrix=False)
        else:
            _, idx, mean = eng.knn(emb, refs, k)
        ctx.save_for_backward(est, refs, emb, layers, saved, idx)
        return mean

    @staticmethod
    def backward(ctx, grad_out):
        est, refs, emb, layers, saved, idx = ctx.saved_tensors
        eng = ctx.nomad.engine
        shape, ref_device, ref_dtype = ctx.meta
        want_a = ctx.needs_input_grad[0] and saved is not None
        want_b = ctx.needs_input_grad[1]
        if not (want_a or want_b):
            return None, None, None, None, None, None
        g = grad_out.to(eng.device, torch.float64).contiguous()
        if idx is None:
            demb, dref = eng.cdist_backward(emb, refs, g_mean=g, want_a=want_a, want_b=want_b)
        else:
            demb, dref = eng.knn_backward(emb, refs, idx, g_score=g, want_a=want_a, want_b=want_b)
        dwav = None
        if want_a:
            Nomad._need_whole_encoder(eng)
            dwav = ctx.rows.backward(eng, est, ctx.lens, layers, saved, demb).reshape(shape)
        if dref is not None:
            dref = dref.to(ref_device, ref_dtype)
        return dwav, dref, None, None, None, None


class _NsimLossFn(torch.autograd.Function):
    """loss[b] = 1 - NSIM(estimate_b, clean_b): ``Engine.gammatone`` twice and ``nsim_of_spectrograms`` forward, ``Engine.nsim_backward``
    and ``gammatone_backward`` backward, both float64 down to the fp32 samples.  ``clean`` gets no gradient."""

    @staticmethod
    def forward(ctx, estimate, clean, nomad, lens, intensity_range):
        eng = nomad.engine
        est, _ = eng._rows(_loss_rows(estimate, eng), lens, None)
        cln, _ = eng._rows(_loss_rows(clean, eng), lens, None)
        spec_ref, frames = eng.gammatone(packed=(cln, lens))
        spec_deg, _ = eng.gammatone(packed=(est, lens))
        score, _ = eng.nsim_of_spectrograms(spec_ref, spec_deg, frames, 1, intensity_range, want_bands=False)
        ctx.nomad, ctx.lens, ctx.frames, ctx.intensity_range, ctx.meta = nomad, lens, frames, intensity_range, (estimate.shape, estimate.shape[-1])
        ctx.save_for_backward(est, spec_ref, spec_deg)
        return 1.0 - score.view(-1)

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        est, spec_ref, spec_deg = ctx.saved_tensors
        eng = ctx.nomad.engine
        shape, width = ctx.meta
        g = (-grad_out.to(eng.device, torch.float64)).reshape(len(ctx.lens), 1).contiguous()
        dspec = eng.nsim_backward(spec_ref, spec_deg, ctx.frames, 1, g, ctx.intensity_range)
        dx = eng.gammatone_backward(dspec, packed=(est, ctx.lens))
        return dx[:, :width].reshape(shape), None, None, None, None


def _loss_rows(wav, eng):
    x = wav.detach().to(eng.device, torch.float32)
    return (x.squeeze(1) if x.dim() == 3 else x).contiguous()


class GraphedLoss:
    """``nomad.forward`` + its backward to ``estimate`` for ONE input shape, captured once as a HIP graph and replayed per step.

    A configs[3] training step (2 x (32,1,16384)) is ~440 kernel launches of 5-90 us: issued one by one, the host is still launching
    when the first two thirds of the step's GPU work are done (profiles/r04_c4_posconv_splitk_ab.txt).  A training loop with a fixed
    batch shape can capture the launch sequence once (``torch.cuda.graph``; every entry point on the path is capture-safe: the
    library allocates nothing and queries no event after the first call of a shape) and replay it - same kernels, same order,
    same bits (``tests/test_gpu_backward.py::test_graphed_loss_replays_bit_identically``).

    ``loss = graphed(estimate, clean)`` is differentiable with respect to ``estimate`` like ``nomad.forward``: the replay computes the
    loss AND d loss / d estimate; the autograd node hands the stored gradient (times the incoming one) on.

    Restrictions (checked): a captured graph holds its kernel arguments BY VALUE - the dropout / LayerDrop masks, the step counter and
    the addresses of ``lossnet_layers.embedding_weight`` / ``embedding_bias`` of the moment of capture.  So capture is refused while the
    engine has dropout or LayerDrop switched on (``Engine.train_set_stochastic`` / ``train_set_branches``: every replay would reuse one
    set of masks), and ``step`` raises when the head tensors have been replaced since (the graph would read freed memory) or
    stochastic mode has been switched on; "same bits as eager" is a statement about the frozen, eval-mode loss path only."""

    def _state(self):
        ll = self.nomad.lossnet_layers
        return (ll.embedding_weight.data_ptr(), ll.embedding_bias.data_ptr())

    def _check_not_stochastic(self, what: str):
        eng = self.nomad.engine
        if getattr(eng, "stochastic", False) or getattr(eng, "stochastic_branches", False):
            raise RuntimeError(f"GraphedLoss: {what} while the engine has dropout / LayerDrop switched on - a HIP graph replays the masks "
                               "and the step counter of its capture; use nomad.forward() for stochastic passes")

    def __init__(self, nomad: "Nomad", estimate: torch.Tensor, clean: torch.Tensor, warmup: int = 3):
        self.nomad = nomad
        if nomad.nomad_loss.L != 13:
            raise ValueError(f"GraphedLoss captures the 13-term mean only (nomad_loss.L is {nomad.nomad_loss.L!r}): layer selections and "
                             "per-utterance losses go through nomad.forward()")
        self._check_not_stochastic("capture")
        # the graph reads the head through these addresses: keep the tensors alive and notice a replacement
        self._head = (nomad.lossnet_layers.embedding_weight, nomad.lossnet_layers.embedding_bias)
        self._head_ptrs = self._state()
        dev = nomad.engine.device
        self._est = estimate.detach().to(dev, torch.float32).clone().requires_grad_(True)
        self._cln = clean.detach().to(dev, torch.float32).clone()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):           # warm-up off the capture: workspaces, kernel attributes, autograd buffers
            for _ in range(max(1, warmup)):
                self._est.grad = None
                nomad.forward(self._est, self._cln).backward()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self._graph = torch.cuda.CUDAGraph()
        self._est.grad = None
        with torch.cuda.graph(self._graph):
            self._loss = nomad.forward(self._est, self._cln)
            self._loss.backward()
        self._grad = self._est.grad

    def step(self, estimate: torch.Tensor, clean: torch.Tensor):
        """-> (loss, d loss / d estimate): views of the graph's static outputs, valid until the next step."""
        if estimate.shape != self._est.shape or clean.shape != self._cln.shape:
            raise ValueError(f"GraphedLoss was captured for {tuple(self._est.shape)} / {tuple(self._cln.shape)}")
        self._check_not_stochastic("replay")
        if self._state() != self._head_ptrs:
            raise RuntimeError("GraphedLoss: lossnet_layers.embedding_weight / embedding_bias were replaced after capture (the graph holds "
                               "their old addresses); update them in place (copy_) or capture a new graph with nomad.graphed_loss()")
        with torch.no_grad():
            self._est.copy_(estimate)
            self._cln.copy_(clean)
        self._graph.replay()
        return self._loss, self._grad

    def __call__(self, estimate: torch.Tensor, clean: torch.Tensor) -> torch.Tensor:
        return _GraphedLossFn.apply(estimate, clean, self)


class _GraphedLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, estimate, clean, graphed):
        loss, grad = graphed.step(estimate.detach(), clean.detach())
        ctx.save_for_backward(grad.clone())
        ctx.shape = estimate.shape
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return (g * grad_out).reshape(ctx.shape), None, None


# precision="bf16x3": from about 2 500 frames per batch (12 clips of 4 s, 50 of 1 s) the split-storage forward (256 x 256 tiles,
# embed_bf16x3) is the fastest; below that the batch stays on fp32 buffers with the same three-product arithmetic in its
# small-tile GEMMs (Engine.gemm_precision = "bf16x3").  Measured on MI355X (tools/bench_small_batch.py,
# profiles/r03_small_batch.jsonl; fp32 / x3 products on fp32 buffers / split storage, ms): 8 clips of 4 s 5.96 / 4.33 / 5.32,
# 16 clips 9.44 / 6.64 / 5.84, 32 clips of 1 s (config C4's branch) 5.75 / 4.18 / 5.22, 64 clips of 1 s 9.15 / 6.38 / 5.77.
BF16X3_MIN_SAMPLES = 800_000


def _write_rounded_csv(df: pd.DataFrame, path: str) -> None:
    """``df.to_csv(path, index=False)`` for the scores table (first column = labels, the rest 3-decimal floats), byte for
    byte, without pandas' per-cell float formatting: 10 000 x 1 000 scores take pandas 6-9 s to write and this 1 s.
    A value rounded to 3 decimals is k / 1000 for an integer k, and pandas prints a float by its shortest round-trip
    repr, so a table of ``repr(k / 1000.0)`` covers every cell.  Anything else (NaN, values off the grid, huge
    values, labels that need CSV quoting) goes through pandas itself."""
    vals = df.iloc[:, 1:].to_numpy(dtype=np.float64, copy=False) if df.shape[1] > 1 else np.zeros((len(df), 0))
    labels = [str(x) for x in df.iloc[:, 0].tolist()]
    header = [str(c) for c in df.columns]
    special = set(',"\r\n')
    ok = (vals.size > 0 and bool(np.isfinite(vals).all()) and not any(special & set(x) for x in labels + header)
          and all(isinstance(x, str) for x in df.iloc[:, 0].tolist()))
    if ok:
        idx = np.rint(vals * 1000.0)
        ok = bool(idx.min() >= 0 and idx.max() <= 100000 and np.array_equal(idx / 1000.0, vals))
    if not ok:
        df.to_csv(path, index=False)
        return
    lut = np.array([repr(k / 1000.0) for k in range(int(idx.max()) + 1)], dtype=object)
    cells = lut[idx.astype(np.int64)]
    with open(path, "w", newline="") as f:
        f.write(",".join(header) + "\n")
        f.write("\n".join(labels[i] + "," + ",".join(cells[i]) for i in range(len(labels))))
        f.write("\n")


class _StagingRing:
    """``slots`` pinned host buffers reused round-robin by the packer thread (grown on demand, never per batch).

    A slot is rewritten only after the H2D copy that read it last has completed: the consumer records an event right
    after it enqueued the copy (``uploaded``), ``take`` waits for it.  With ``max_alive`` staged batches in flight and
    ``max_alive + 1`` slots that wait is already over in practice (the batch three back has had its results fetched)."""

    def __init__(self, slots: int, device=None):
        self.bufs = [None] * slots
        self.events = [None] * slots
        self.taken = 0
        self.device = device   # the engine's device: the H2D copy runs on ITS current stream, whatever device is current

    def take(self, rows: int, stride: int):
        slot = self.taken % len(self.bufs)
        self.taken += 1
        ev, self.events[slot] = self.events[slot], None
        if ev is not None:
            ev.synchronize()
        need = rows * stride
        if self.bufs[slot] is None or self.bufs[slot].numel() < need:
            self.bufs[slot] = None
            self.bufs[slot] = torch.empty(need, dtype=torch.float32, pin_memory=torch.cuda.is_available())
        return slot, self.bufs[slot][:need].view(rows, stride)

    def uploaded(self, slot: int) -> None:
        if torch.cuda.is_available():
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self.events[slot] = ev


def _dist_info(group=None):
    """(world size, rank, use collectives) of the torch.distributed job this process belongs to - (1, 0, False) outside one.
    NOMAD_FORCE_COLLECTIVE=1 runs the collectives in a group of one rank too (how the RCCL path is exercised on a
    single-GPU box)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 1, 0, False
    world = dist.get_world_size(group)
    return world, dist.get_rank(group), world > 1 or os.environ.get("NOMAD_FORCE_COLLECTIVE") == "1"


def _staged_batches(paths, load, pack, max_batch_samples: int, decode_threads: int, max_alive: int, native_threads: int = 0,
                    target_sr: int = 16000, device=None):
    """Generator of (row indices, (staging buffer, lengths), uploaded) batches over ``paths`` in order, built ahead of
    the consumer; the consumer calls ``uploaded()`` once it has enqueued the H2D copy of the staging buffer.

    A packer thread groups consecutive files into batches of at most ``max_batch_samples`` samples (a longer file is a
    batch of its own; a batch also closes before rows x longest row would exceed twice that, which bounds the
    staging buffer when one long file sits among short ones).

    * ``native_threads > 0``: file headers are probed through the C ABI (``nomad_wav_probe``); the files it can decode are
      converted - and, at another sample rate, resampled to ``target_sr`` - by ``nomad_wav_read_rows`` on that many plain
      host threads, straight into a slot of a ring of pinned staging buffers - no per-file Python, no GIL, no second copy.
    * every other file (an encoding or a header the native reader does not take, an unreadable file) goes through
      ``load(path) -> (1, N) array`` on ``decode_threads`` Python worker threads with a bounded look-ahead, so results
      and exceptions are those of ``load``.  A batch without native files is packed by ``pack(list of 1-D arrays)``.

    At most ``max_alive`` packed batches exist between the packer and the consumer: the packer takes a token before
    it starts a batch, and the token returns when the consumer asks for the batch AFTER the next one (by then the
    consumer has fetched that batch's results).  Exceptions raised by ``load`` / ``pack`` re-raise in the consumer."""
    import queue
    import threading
    from concurrent.futures import ThreadPoolExecutor

    if not paths:
        return
    tokens = threading.Semaphore(max_alive)
    out: "queue.Queue" = queue.Queue()
    stop = threading.Event()
    lookahead = max(4 * decode_threads, 16)
    ring = _StagingRing(max_alive + 1, device) if native_threads > 0 else None
    probe_chunk = 2048

    def packer():
        try:
            with ThreadPoolExecutor(max_workers=max(1, decode_threads)) as pool:
                infos, fast = {}, {}          # index -> WavInfo / frames of the files the native reader takes
                probed = 0
                futs, scan = {}, 0            # index -> future of load(path); next file to look at for submission

                def probe_upto(upto):
                    nonlocal probed
                    while ring is not None and probed < min(upto, len(paths)):
                        chunk = [str(p) for p in paths[probed:probed + probe_chunk]]
                        inf, status = wavio.probe(chunk, native_threads)
                        for k in range(len(chunk)):
                            if status[k] == 0 and inf[k].sample_rate > 0 and inf[k].frames > 0:
                                infos[probed + k] = inf[k]
                                fast[probed + k] = (int(inf[k].frames) if inf[k].sample_rate == target_sr
                                                    else wavio.frames_at(inf[k], target_sr))
                        probed += len(chunk)

                def top_up(i):                 # keep up to `lookahead` Python decodes in flight, in file order
                    nonlocal scan
                    scan = max(scan, i)
                    while scan < len(paths) and len(futs) < lookahead and scan < i + probe_chunk:
                        probe_upto(scan + 1)
                        if scan not in fast:
                            futs[scan] = pool.submit(load, paths[scan])
                        scan += 1

                def flush(idxs, items, lens):
                    if not any(isinstance(it, int) for it in items):
                        return idxs, pack(items), (lambda: None)
                    stride = (max(lens) + 3) // 4 * 4
                    slot, host = ring.take(len(idxs), stride)
                    rows = [r for r, it in enumerate(items) if isinstance(it, int)]
                    wavio.read_rows([str(paths[items[r]]) for r in rows], [infos.pop(items[r]) for r in rows], rows, host,
                                    native_threads, target_sr)
                    for r, it in enumerate(items):
                        if not isinstance(it, int):
                            host[r, :lens[r]] = torch.as_tensor(it, dtype=torch.float32).reshape(-1)
                    return idxs, (host, lens), (lambda: ring.uploaded(slot))

                idxs, items, lens, total = [], [], [], 0
                tokens.acquire()
                for i in range(len(paths)):
                    if stop.is_set():
                        return
                    top_up(i)
                    if i in fast:
                        item, n = i, fast.pop(i)                  # native: converted when the batch is flushed
                    else:
                        w = futs.pop(i).result()
                        item = w[0] if getattr(w, "ndim", 1) == 2 else w
                        n = int(item.shape[0])
                    if idxs and (total + n > max_batch_samples or (len(idxs) + 1) * max(max(lens), n) > 2 * max_batch_samples):
                        out.put(flush(idxs, items, lens))
                        idxs, items, lens, total = [], [], [], 0
                        tokens.acquire()
                    idxs.append(i)
                    items.append(item)
                    lens.append(n)
                    total += n
                out.put(flush(idxs, items, lens))
            out.put(None)
        except BaseException as e:  # noqa: BLE001 - handed to the consumer
            out.put(e)

    th = threading.Thread(target=packer, name="nomad-packer", daemon=True)
    th.start()
    handed = 0
    try:
        while True:
            item = out.get()
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            handed += 1
            if handed >= max_alive:      # the consumer is done with batch (handed - max_alive + 1): its slot is free again
                tokens.release()
            yield item
    finally:
        stop.set()
        for _ in range(max_alive + 1):   # unblock a packer waiting for a slot
            tokens.release()
        th.join(timeout=30)


def synthetic_rir(rt60_s, seed: int = 0, drr_db: float = 0.0) -> np.ndarray:
    """A synthetic diffuse room at 16 kHz for ``Nomad.convolve`` -> float32 (L,), L = min(ceil(rt60_s 16000), 65536): a direct path
    ``h[0] = 1`` and, from tap 1 on, Gaussian noise (``np.random.RandomState(seed).standard_normal(L)``; its first value is not used)
    under an envelope that has fallen by 60 dB at ``rt60_s``, ``10^(-3 k / (rt60_s 16000))``, scaled so that the tail's energy is
    ``10^(-drr_db / 10)`` - ``drr_db`` is the direct-to-reverberant ratio.  rt60_s: finite, in (0, 4.096] seconds.  This is NOT
    sox's reverb (Freeverb: comb and all-pass filters with its own parameters), which the reference's renderings use - that one is
    ``Nomad.reverb``: it is a stand-in with a stated RT60 for sweeps and augmentation; measured responses go into ``convolve`` as
    they are."""
    rt60_s, drr_db = float(rt60_s), float(drr_db)
    if not (math.isfinite(rt60_s) and 0.0 < rt60_s <= 4.096):
        raise ValueError(f"rt60_s must be finite and in (0, 4.096] seconds, got {rt60_s}")
    if not math.isfinite(drr_db):
        raise ValueError(f"drr_db must be finite, got {drr_db}")
    L = min(int(math.ceil(rt60_s * 16000)), 65536)
    r = np.random.RandomState(seed).standard_normal(L)
    tail = r * 10.0 ** (-3.0 * np.arange(L, dtype=np.float64) / (rt60_s * 16000))
    tail[0] = 0.0
    energy = float(np.sum(tail ** 2))
    if energy > 0.0:          # a room of one tap (or a tail of zeros) has no tail to scale
        tail *= math.sqrt(10.0 ** (-drr_db / 10.0) / energy)
    h = tail
    h[0] = 1.0
    return h.astype(np.float32)


class Nomad:
    def __init__(self, device=None, weights: Union[None, str, Dict[str, torch.Tensor]] = None, precision: str = "fp32",
                 feature_grad_mult: Union[None, float] = None, group=None):
        """feature_grad_mult: fairseq's ``Wav2Vec2Model.feature_grad_mult`` - ``forward()``'s gradient w.r.t. ``estimate``
        passes through ``GradMultiply(features, feature_grad_mult)`` at the conv feature extractor's output, exactly as
        in the reference's backbone (built from wav2vec_small.pt, whose config says 0.1; nomad.py:58).  None = 0.1, or
        the value in the fairseq checkpoint ``$NOMAD_W2V_CHECKPOINT`` names (read with ``weights_only=True``; nothing is
        unpickled that the caller did not name); 1.0 = plain chain rule.

        precision of the embeddings of ``predict`` / ``get_embeddings*``:
        "fp32"   the reference's arithmetic (fp32 MFMA), scores within 1e-4 of the reference;
        "bf16x3" GEMM operands split into hi + lo bf16 planes, three bf16 MFMA products per fp32 product, fp32
                 accumulation / softmax / norms: scores within ~1e-6 of the fp32 path, 2.7x as fast on full batches
                 (batches of fewer than BF16X3_MIN_SAMPLES samples stay on fp32 buffers, with the same three-product
                 arithmetic in their GEMMs: ``Engine.gemm_precision``); ``forward()``'s differentiated branch and its
                 backward run that way too;
        "bf16"   bf16 storage, fp32 accumulation: scores within ~5e-4 of fp32, fastest on long recordings.
        ``forward()`` (the training loss) is fp32 unless precision is "bf16x3"."""
        if precision not in ("fp32", "bf16x3", "bf16"):
            raise ValueError("precision must be 'fp32', 'bf16x3' or 'bf16'")
        self.precision = precision
        dev_index = _resolve_device(device)
        self.DEVICE = f"cuda:{dev_index}"
        print(f"NOMAD running on: {self.DEVICE}")
        if weights is None:
            path = find_checkpoint()
            if path is None:
                raise FileNotFoundError(
                    "NOMAD weights not found: place nomad_best_model.pt under ./pt-models/ (the reference "
                    "downloads it there, nomad.py:27-33) or set $NOMAD_CHECKPOINT; for synthetic benchmarks "
                    "pass weights='seeded'")
            sd = load_checkpoint(path)
        elif isinstance(weights, str) and weights == "seeded":
            sd = seeded_state_dict(0)
        elif isinstance(weights, str):
            sd = load_checkpoint(weights)
        else:
            sd = weights
        self.group = group   # torch.distributed group predict() shards its files over (None: the default group, if any)
        self.engine = Engine(sd, dev_index)
        self.engine.feature_grad_mult = find_feature_grad_mult() if feature_grad_mult is None else float(feature_grad_mult)
        if precision == "bf16x3":
            # everything that stays on fp32 buffers in this mode - batches too small for the split-storage path, and the
            # differentiated branch of forward() with its backward - forms its GEMM products as three bf16 MFMA products
            # as well (hi / lo halves split in registers): ~1e-6 on scores, ~5x shorter K loops on the small-M problems
            self.engine.gemm_precision = "bf16x3"
        self.model = TripletModel(self.engine)
        self.lossnet_layers = LossNetLayers(self.engine, SSL_OUT_DIM, EMB_DIM, precision)
        self.nomad_loss = NomadLoss(self.engine)

    @classmethod
    def from_engine(cls, engine: Engine, precision: str = "fp32", group=None) -> "Nomad":
        """A ``Nomad`` over an engine that exists already (``nomad_amd.train.Training`` shares its own with the file pipeline)."""
        if precision not in ("fp32", "bf16x3", "bf16"):
            raise ValueError("precision must be 'fp32', 'bf16x3' or 'bf16'")
        self = cls.__new__(cls)
        self.precision, self.group, self.engine = precision, group, engine
        self.DEVICE = f"cuda:{engine.device_index}"
        self.model = TripletModel(engine)
        self.lossnet_layers = LossNetLayers(engine, SSL_OUT_DIM, EMB_DIM, precision)
        self.nomad_loss = NomadLoss(engine)
        return self

    # ------------------------------------------------------------------------------------------
    def predict(self, mode="dir", nmr="data/nmr-data", deg="data/test-data", results_path=None, k=None):
        """The reference's ``predict`` -> (df_avg, df_scores).  With ``k`` (1 .. min(64, references)) the ``NOMAD`` column is the mean
        distance to the file's ``k`` NEAREST references instead of all of them, the score matrix (``nomad_scores.csv``) is unchanged,
        and a third table comes back - ``nearest_table``, written to ``nomad_nearest.csv`` -: -> (df_avg, df_scores, df_nearest)."""
        if k is not None:
            check_k(k, KNN_MAX)   # the type and 1 .. 64 before any file is read; against the bank's size once it is known
        if nmr is None:
            raise Exception("nmr_path not specified, you need to pass a valid value to nmr_path")
        if deg is None:
            raise Exception("test_path not specified, you need to pass a valide value to test_path")

        if mode == "dir":
            if os.path.isdir(nmr) == False:  # noqa: E712 (message parity with the reference)
                raise Exception(f"Path to the non-matching reference files {nmr} does not exist")
            if os.path.isdir(deg) == False:  # noqa: E712
                raise Exception(f"Path to the test files {deg} does not exist")
        elif mode == "csv":
            if os.path.isfile(nmr) == False:  # noqa: E712
                raise Exception(f"File {nmr} does not exist")
            if os.path.isfile(deg) == False:  # noqa: E712
                raise Exception(f"File {deg} does not exist")
        else:
            raise Exception(f"Mode value {mode} is not valid. Valid values are dir and csv")

        print(f"Compute non-matching reference embeddings from {nmr}")
        nmr_embeddings = self.get_embeddings(nmr).set_index("filename")

        print(f"Compute degraded embeddings from {deg}")
        test_embeddings = self.get_embeddings(deg).set_index("filename")

        # Pairwise distance matrix + average NOMAD score, on the GPU (cdist + np.mean, nomad.py:108-111)
        deg_t = torch.from_numpy(np.ascontiguousarray(test_embeddings.to_numpy(dtype=np.float32))).to(self.engine.device)
        ref_t = torch.from_numpy(np.ascontiguousarray(nmr_embeddings.to_numpy(dtype=np.float32))).to(self.engine.device)
        world, rank, collective = _dist_info(getattr(self, "group", None))
        if k is not None:
            k = check_k(k, ref_t.shape[0])
            knn_d, knn_i = torch.zeros(0, k, dtype=torch.float64), torch.zeros(0, k, dtype=torch.int32)
        if deg_t.shape[0] == 0 or ref_t.shape[0] == 0:
            # an empty directory: what cdist + np.mean(axis=1) give the reference - an empty matrix, and NaN means when
            # there is no reference to average over (the engine's kernels take no empty operands)
            collective = False
            dist = torch.zeros(deg_t.shape[0], ref_t.shape[0], dtype=torch.float64)
            mean = torch.full((deg_t.shape[0],), float("nan"), dtype=torch.float64)
        elif collective:   # this rank's slab of the matrix (its slice of the degraded files x all references), then one gather
            lo, hi = partition(deg_t.shape[0], world, rank)
            if hi > lo and k is not None:   # the neighbours of this rank's rows: gathered as the means are
                knn_d, knn_i, mean, dist = self.engine.knn(deg_t[lo:hi].contiguous(), ref_t, k, want_matrix=True)
            elif hi > lo:
                dist, mean = self.engine.pairwise(deg_t[lo:hi].contiguous(), ref_t, want_matrix=True)
            else:
                dist = torch.zeros(0, ref_t.shape[0], dtype=torch.float64, device=deg_t.device)
                mean = torch.zeros(0, dtype=torch.float64, device=deg_t.device)
                if k is not None:
                    knn_d, knn_i = knn_d.to(deg_t.device), knn_i.to(deg_t.device)
            dist, mean = self._all_gather_rows(dist), self._all_gather_rows(mean)
            if k is not None:
                knn_d, knn_i = self._all_gather_rows(knn_d), self._all_gather_rows(knn_i)
        elif k is not None:
            knn_d, knn_i, mean, dist = self.engine.knn(deg_t, ref_t, k, want_matrix=True)
        else:
            dist, mean = self.engine.pairwise(deg_t, ref_t, want_matrix=True)
        distance_matrix = dist.cpu().numpy()
        avg_nomad = mean.cpu().numpy()

        test_files = [x.split("/")[-1].split(".")[0] for x in test_embeddings.index]
        df_avg_nomad = pd.DataFrame({"Test File": test_files, "NOMAD": avg_nomad}).set_index("Test File").round(3)

        df_dm = pd.DataFrame(distance_matrix).round(3)
        df_dm["Test File"] = test_files
        df_dm.set_index("Test File", inplace=True)
        df_dm.columns = [x.split("/")[-1].split(".")[0] for x in nmr_embeddings.index]
        if k is not None:
            df_nearest = nearest_table(test_files, df_dm.columns, knn_d.cpu().numpy(), knn_i.cpu().numpy())

        if results_path is None:
            dt_string = datetime.now().strftime("%d-%m-%Y_%H-%M-%S")
            out_dir = os.path.join("results-csv", dt_string)
            if rank == 0:
                os.makedirs(out_dir, exist_ok=True)
            results_avg_path = os.path.join(out_dir, f"{dt_string}_nomad_avg.csv")
            results_scores_path = os.path.join(out_dir, f"{dt_string}_nomad_scores.csv")
            results_nearest_path = os.path.join(out_dir, f"{dt_string}_nomad_nearest.csv")
        else:
            results_avg_path = os.path.join(results_path, "nomad_avg.csv")
            results_scores_path = os.path.join(results_path, "nomad_scores.csv")
            results_nearest_path = os.path.join(results_path, "nomad_nearest.csv")

        if rank == 0:   # every rank returns the tables, one writes the files
            df_avg_nomad.reset_index().to_csv(results_avg_path, index=False)
            _write_rounded_csv(df_dm.reset_index(), results_scores_path)
            if k is not None:
                df_nearest.reset_index().to_csv(results_nearest_path, index=False)
        return (df_avg_nomad, df_dm) if k is None else (df_avg_nomad, df_dm, df_nearest)

    def forward(self, estimate, clean, lengths=None, *, layer_weights=None, reduction="mean"):
        """NOMAD loss (nomad.py:142-146), differentiable w.r.t. ``estimate`` - and w.r.t. ``clean`` when it requires a gradient:
        that branch then keeps its activations too (the fp32 ``embed_train`` on the caller's stream: no side-stream overlap, no
        split-bf16 forward), about the cost of a second ``estimate`` branch.

        Which terms count: ``self.nomad_loss.L`` as in the reference (``for i in range(self.L)``, nomad.py:276) - the first L of the
        12 transformer layers + the embedding, L in 1 .. 13 - or ``layer_weights``, 13 numbers >= 0 (the layers' weights, then the
        embedding's; see ``loss_selection``, which also says what the reference does at L = 0 and above 13: a ValueError here).  The
        encoder stops behind the deepest layer with a weight, forward and backward, in both branches; a term with weight 0 costs
        nothing.  reduction="none": a (B,) tensor, one loss per utterance - every term the mean over the utterance's own frames
        (with ``lengths``: bit-identical to the utterance's own call at B = 1) - whose backward takes the (B,) upstream;
        "mean" (default): every term the mean over the batch.  ``L == 13`` without weights and "mean" is the path, the kernels
        and the bits of before.  Below depth 12 the no-gradient branch stays on fp32 buffers whatever ``precision`` says (products
        follow ``Engine.gemm_precision``).

        lengths (B ints, tensor or list; ``estimate`` and ``clean`` (B,1,N) or (B,N)): the exact-length loss - utterance b is the
        first ``lengths[b]`` samples of its row, the samples behind are never read, and nothing is padded in the arithmetic
        (zero padding would change GroupNorm statistics, attention and the time mean, hence the loss).  Every layer term is the
        mean over the valid frames of all clips, as ``F.l1_loss`` on their concatenation; the gradient is zero behind each
        length.  Differentiable in ``estimate`` (and in ``clean`` when it requires a gradient); the no-gradient branch runs on the
        side stream.  With ``precision="bf16x3"`` both branches stay on fp32 buffers with bf16x3 products: there is no ragged
        layer-output forward on split bf16 storage.  ``lengths=None`` is the equal-length path, unchanged.

        The whole forward and backward run in the HIP engine (``torch.autograd.Function`` glue only).  As in the
        reference, the gradient that reaches ``estimate`` carries fairseq's ``feature_grad_mult`` (0.1 for wav2vec 2.0
        BASE; ``Nomad(feature_grad_mult=...)`` / ``self.engine.feature_grad_mult``).  The backbone is frozen: the reference would also accumulate parameter gradients nobody reads
        (the freeze is commented out at nomad.py:74-76)."""
        check_reduction(reduction)
        lens = None
        if lengths is not None:
            if estimate.shape != clean.shape:
                raise ValueError(f"estimate {tuple(estimate.shape)} and clean {tuple(clean.shape)} must have one shape")
            lens = check_lengths(estimate, lengths)
        weights, depth = loss_selection(self.nomad_loss.L, layer_weights)
        if layer_weights is None and self.nomad_loss.L == 13 and reduction == "mean":
            return _NomadLossFn.apply(estimate, clean, self, lens, None)
        return _NomadLossFn.apply(estimate, clean, self, lens, (weights, depth, reduction))

    @staticmethod
    def _need_whole_encoder(eng: Engine):
        depth = eng.encoder_depth
        if depth != 12:
            raise RuntimeError(f"Nomad.score needs the whole encoder: the embedding is computed from the last layer and encoder_depth "
                               f"is {depth} (a cut encoder is a property of forward()'s layer selections)")

    def _score_embed(self, wav: torch.Tensor, lens) -> torch.Tensor:
        """The scoring forward of ``precision`` over a (B,N) device batch -> (B,256): what ``self.model`` / ``get_embeddings*`` run."""
        eng = self.engine
        if lens is not None:
            prec = self.precision
            if prec == "bf16x3" and sum(lens) < BF16X3_MIN_SAMPLES:
                prec = "fp32"   # as in the file pipeline: fp32 buffers, products by Engine.gemm_precision
            return eng.embed_ragged([wav[i, :n] for i, n in enumerate(lens)], precision=prec)
        if self.precision == "bf16":
            return eng.embed_bf16(wav)
        return eng.embed_bf16x3(wav) if _takes_bf16x3(self.precision, wav) else eng.embed(wav)

    def _reference_mean(self, emb: torch.Tensor, refs: torch.Tensor, k) -> torch.Tensor:
        """(N,) float64: the mean distance of every embedding to all references (``Engine.pairwise``), or to its k nearest."""
        if k is None:
            return self.engine.pairwise(emb, refs, want_matrix=False)[1]
        return self.engine.knn(emb, refs, k)[2]

    def nearest_references(self, wav_or_embeddings, references, k, lengths=None):
        """-> (knn_dist (N,k) float64, knn_idx (N,k) int32) on the GPU: for every clip the distances to and the rows of its ``k``
        nearest ``references`` ((Nr,256), as ``score`` takes them), ascending by (distance, row).  A (N,256) tensor is taken as
        embeddings; a (B,1,N) or (B,N) tensor as waveforms, embedded by the scoring forward of ``precision`` (``lengths`` as in
        ``score``).  No gradient."""
        check_references(references)
        k = check_k(k, references.shape[0])
        x = wav_or_embeddings
        if not torch.is_tensor(x) or x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[1] != 1):
            raise ValueError(f"expected (N,{EMB_DIM}) embeddings or (B,1,N) / (B,N) waveforms, got {tuple(getattr(x, 'shape', ()))}")
        eng = self.engine
        refs = references.detach().to(eng.device, torch.float32).contiguous()
        x = x.detach().to(eng.device, torch.float32).contiguous()
        if x.dim() == 2 and x.shape[1] == EMB_DIM:
            if lengths is not None:
                raise ValueError("lengths go with waveforms: a (N,256) tensor is taken as embeddings")
            emb = x
        else:
            lens = check_lengths(wav_or_embeddings, lengths) if lengths is not None else None
            self._need_whole_encoder(eng)
            emb = self._score_embed(x.squeeze(1) if x.dim() == 3 else x, lens)
        knn_dist, knn_idx, _ = eng.knn(emb, refs, k)
        return knn_dist, knn_idx

    def score(self, estimate, references, lengths=None, reduction="none", k=None):
        """The NOMAD score as a differentiable quantity: ``score[b] = mean_j ||emb(estimate_b) - references_j||`` in float64, the
        number ``predict`` reports for a file - no matching clean signal is needed, only a bank of reference embeddings.

        estimate (B,1,N) or (B,N); references (Nr,256) embeddings as ``self.model(wav)`` / ``get_embeddings`` make them (the
        checkpoint's ``embedding_layer``, not ``lossnet_layers``' head); lengths: the clips' exact lengths as in ``forward``.
        -> (B,) float64, or with reduction="mean" their mean (plain torch on that tensor).

        Under ``torch.no_grad()``, or when nothing requires a gradient, the embeddings come from the scoring forward of
        ``precision`` and the distances from ``Engine.pairwise``: at fp32 with ``lengths`` the bits ``predict`` gives the file.  With
        a gradient the forward is ``embed_train[_ragged]`` (fp32 buffers, products by ``Engine.gemm_precision``), and the backward
        runs ``cdist_backward`` - float64, a reference equal to the embedding contributes nothing - then the head, the
        normalisation and the backbone down to the waveform; the gradient carries ``feature_grad_mult`` exactly as
        ``forward()``'s does and is zero behind every length.  ``references`` gets a gradient too when it requires one.

        k (1 .. min(64, Nr)): the mean over the ``k`` NEAREST references instead of all of them - for a bank that mixes speakers,
        rooms and microphones the distance to the closest clean speech known, and as a loss a pull towards clean speech that is
        like the estimate rather than towards the bank's centroid.  ``Engine.knn`` takes ``Engine.pairwise``'s place (the same
        distances, ties to the lower row) and ``Engine.knn_backward`` ``cdist_backward``'s, with the forward's selection held fixed;
        ``k=None`` is the mean over the whole bank, unchanged."""
        check_reduction(reduction)
        check_references(references)
        k = check_k(k, references.shape[0]) if k is not None else None
        if not torch.is_tensor(estimate) or estimate.dim() not in (2, 3) or (estimate.dim() == 3 and estimate.shape[1] != 1):
            raise ValueError(f"estimate must be (B,1,N) or (B,N), got {tuple(getattr(estimate, 'shape', ()))}")
        lens = check_lengths(estimate, lengths) if lengths is not None else None
        self._need_whole_encoder(self.engine)
        if torch.is_grad_enabled() and (estimate.requires_grad or references.requires_grad):
            scores = _ScoreFn.apply(estimate, references, self, lens, _ClipRows(), k)
        else:
            eng = self.engine
            est = estimate.detach().to(eng.device, torch.float32).contiguous()
            est = est.squeeze(1) if est.dim() == 3 else est
            refs = references.detach().to(eng.device, torch.float32).contiguous()
            scores = self._reference_mean(self._score_embed(est, lens), refs, k)
        return scores.mean() if reduction == "mean" else scores

    def _window_precision(self, n_samples: int) -> str:
        """The forward the windows of a batch of ``n_samples`` samples take: ``precision``, with the file pipeline's rule for bf16x3."""
        return "fp32" if self.precision == "bf16x3" and n_samples < BF16X3_MIN_SAMPLES else self.precision

    def score_over_time(self, wav, references, window_s=4.0, hop_s=2.0, lengths=None, k=None):
        """NOMAD scores over time: -> (scores (W_total,) float64 on the GPU, counts) - for every window of ``window_s`` seconds
        every ``hop_s`` seconds the mean distance of the window's embedding to ``references`` ((Nr,256), as ``score`` takes
        them); clip 0's windows in order, then clip 1's, ...; counts[c] = windows of clip c.  wav (B,1,N) or (B,N) on the GPU;
        lengths: the clips' exact lengths as in ``score``.

        Seconds become encoder frames, ``max(1, round(s * 50))`` (one frame is 320 samples, its receptive field 400); the
        windows are those of ``weights.num_windows``: a clip shorter than the window gets one window over all of it - then
        the bits of ``score`` -, frames behind the last full window belong to no window.  All windows come from ONE forward
        of ``precision`` (``Engine.embed_windows*``): attention and the first conv layer's GroupNorm statistics saw the whole
        clip, so a window's score is not the score of the excerpt on its own.  No gradient is produced: ``score_windows`` is the
        differentiable form of this call.  k: every window's mean over its ``k`` nearest references, as in ``score``."""
        win, hop = window_frames(window_s, hop_s)
        check_references(references)
        k = check_k(k, references.shape[0]) if k is not None else None
        if not torch.is_tensor(wav) or wav.dim() not in (2, 3) or (wav.dim() == 3 and wav.shape[1] != 1):
            raise ValueError(f"wav must be (B,1,N) or (B,N), got {tuple(getattr(wav, 'shape', ()))}")
        if wav.requires_grad or references.requires_grad:
            raise ValueError("score_over_time produces no gradient (the windowed head has no backward): pass tensors that do not "
                             "require one, or use score() for a differentiable whole-clip score")
        lens = check_lengths(wav, lengths) if lengths is not None else None
        self._need_whole_encoder(self.engine)
        eng = self.engine
        x = wav.detach().to(eng.device, torch.float32).contiguous()
        x = x.squeeze(1) if x.dim() == 3 else x
        refs = references.detach().to(eng.device, torch.float32).contiguous()
        if lens is not None:
            emb, counts = eng.embed_windows_ragged([x[i, :n] for i, n in enumerate(lens)], win, hop,
                                                   precision=self._window_precision(sum(lens)))
        else:
            emb, counts = eng.embed_windows(x, win, hop, precision=self._window_precision(x.numel()))
        return self._reference_mean(emb, refs, k), counts

    def score_windows(self, estimate, references, window_s=4.0, hop_s=2.0, lengths=None, reduction="none", k=None):
        """``score_over_time`` as a differentiable quantity: -> (scores (W_total,) float64, counts), the windows, their order and
        ``counts`` exactly those of ``score_over_time`` (``window_frames``, ``weights.num_windows``); with reduction="mean" the
        0-dim mean over all windows in place of ``scores``.  A loss on where a recording is bad is plain torch on that tensor -
        the worst window of every clip::

            scores, counts = nomad.score_windows(estimate, references, window_s=4.0, hop_s=2.0)
            loss = torch.stack([s.max() for s in scores.split(counts)]).mean()

        and per-window weights are ``(scores * weights).sum()``.

        estimate (B,1,N) or (B,N); references (Nr,256) as ``score`` takes them; lengths: the clips' exact lengths.  Under
        ``torch.no_grad()``, or when nothing requires a gradient, this is ``score_over_time``: the scoring forward of
        ``precision``, then ``Engine.pairwise``, the same bits.  With a gradient the forward is ``embed_train_windows[_ragged]``
        (fp32 buffers, products by ``Engine.gemm_precision``; a window over a whole clip then has ``score``'s value), and the
        backward runs ``cdist_backward`` over the window rows, the windowed head's backward - a frame receives the sum of the
        gradients of the windows that cover it, exact zeros where none does - and the backbone down to the waveform.  The
        encoder saw the whole clip: a window's gradient reaches every sample of its clip through attention, not only the
        window's own samples.  It carries ``feature_grad_mult`` as ``score``'s does and is zero behind every length;
        ``references`` gets a gradient too when it requires one.  k: every window's mean over its ``k`` nearest references, as
        in ``score`` (``Engine.knn`` / ``Engine.knn_backward`` over the window rows)."""
        win, hop = window_frames(window_s, hop_s)
        check_reduction(reduction)
        check_references(references)
        k = check_k(k, references.shape[0]) if k is not None else None
        if not torch.is_tensor(estimate) or estimate.dim() not in (2, 3) or (estimate.dim() == 3 and estimate.shape[1] != 1):
            raise ValueError(f"estimate must be (B,1,N) or (B,N), got {tuple(getattr(estimate, 'shape', ()))}")
        lens = check_lengths(estimate, lengths) if lengths is not None else None
        if not (torch.is_grad_enabled() and (estimate.requires_grad or references.requires_grad)):
            scores, counts = self.score_over_time(estimate.detach(), references.detach(), window_s, hop_s, lengths, k)
        else:
            self._need_whole_encoder(self.engine)
            scores = _ScoreFn.apply(estimate, references, self, lens, _WindowRows(win, hop), k)
            samples = lens if lens is not None else [estimate.shape[-1]] * estimate.shape[0]
            counts = [num_windows(num_frames(n), win, hop) for n in samples]
        return (scores.mean() if reduction == "mean" else scores), counts

    def _score_file_windows(self, paths, ref_t, win: int, hop: int, max_batch_samples: int, k=None):
        """The file pipeline of ``get_embeddings_csv`` with the windowed head: -> (frames per file, window scores float64, files
        in order).  Each staged ragged batch is embedded in windows and scored against ``ref_t`` on the GPU; only the scores
        come back, one batch late."""
        frames, scores = [0] * len(paths), [None] * len(paths)
        pending = None

        def collect(item):
            idxs, counts, fetch = item
            vals = fetch.result() if fetch is not None else np.full(sum(counts), np.nan)
            at = 0
            for i, c in zip(idxs, counts):
                scores[i] = np.array(vals[at:at + c], dtype=np.float64)
                at += c

        for idxs, packed, uploaded in _staged_batches(paths, lambda p: self.load_processing(p, trim=False),
                                                      self.engine.pack_ragged_host, max_batch_samples, self.DECODE_THREADS,
                                                      self.PIPELINE_BATCHES, self.NATIVE_WAV_THREADS,
                                                      device=getattr(self.engine, "device", None)):
            for i, n in zip(idxs, packed[1]):
                frames[i] = num_frames(n)
            emb, counts = self.engine.embed_windows_ragged(None, win, hop, precision=self._window_precision(sum(packed[1])),
                                                           packed=packed)
            uploaded()
            # (no reference to average over: NaN, what predict reports then - the distance kernels take no empty operand)
            fetch = self.engine.fetch_async(self._reference_mean(emb, ref_t, k)) if ref_t.shape[0] else None
            if pending is not None:
                collect(pending)
            pending = (idxs, counts, fetch)
        if pending is not None:
            collect(pending)
        return frames, (np.concatenate(scores) if scores else np.zeros(0))

    def predict_segments(self, mode="dir", nmr="data/nmr-data", deg="data/test-data", window_s=4.0, hop_s=2.0, results_path=None,
                         max_batch_samples: int = 256 * 64000, k=None):
        """``predict`` over time: -> (df_segments, df_avg).  df_segments has one row per window of every test file, files in
        listing order: ``Test File``, ``start_s``, ``end_s`` (``window_times``) and ``NOMAD``, the window's mean distance to the
        reference embeddings, rounded to 3 decimals; df_avg, indexed by ``Test File``, the mean of each file's window scores.

        Arguments, checks and file listing as in ``predict``.  The reference files are embedded whole; the test files go through
        the staged ragged batches of ``get_embeddings_csv`` with the windowed head (``score_over_time`` says what a window
        is: pooled from one forward over the whole file).  With ``results_path`` the segment table is written to
        ``segments.csv`` there.  One process only: inside a torch.distributed job of several ranks it raises.  k: a window's
        ``NOMAD`` is its mean distance to its ``k`` nearest references (``score_over_time(k=...)``)."""
        win, hop = window_frames(window_s, hop_s)
        if k is not None:
            check_k(k, KNN_MAX)
        _check_predict_paths(mode, nmr, deg)
        world, _, _ = _dist_info(getattr(self, "group", None))
        if world > 1:
            raise RuntimeError(f"predict_segments runs in one process: this one belongs to a torch.distributed job of {world} ranks "
                               "(sharding the windows is not implemented; predict() shards whole-file scores)")
        print(f"Compute non-matching reference embeddings from {nmr}")
        nmr_embeddings = self.get_embeddings(nmr).set_index("filename")
        print(f"Compute degraded embeddings over windows of {win} frames every {hop} from {deg}")
        paths = [str(p) for p in _file_table(deg)["filename"]]
        ref_t = torch.from_numpy(np.ascontiguousarray(nmr_embeddings.to_numpy(dtype=np.float32))).to(self.engine.device)
        if k is not None:
            k = check_k(k, ref_t.shape[0])
        frames, scores = self._score_file_windows(paths, ref_t, win, hop, max_batch_samples, k)
        test_files = [x.split("/")[-1].split(".")[0] for x in paths]
        df, df_mean = segments_tables(test_files, frames, scores, win, hop)
        if results_path is not None:
            _write_rounded_csv(df, os.path.join(results_path, "segments.csv"))
        return df, df_mean

    # ---- scores over caller-given spans: speech only, per utterance, per speaker turn ------------------------------------
    span_frames = staticmethod(span_frames)

    def score_spans(self, wav, references, spans, lengths=None, reduction="none", k=None, unit="s"):
        """NOMAD scores over spans the CALLER names: -> (scores (R,) float64 on the GPU, counts) - for every row the mean distance
        of the row's embedding to ``references`` ((Nr,256), as ``score`` takes them); clip 0's rows in order, then clip 1's, ...;
        counts[c] = rows of clip c.  wav (B,1,N) or (B,N); lengths: the clips' exact lengths as in ``score``.

        ``spans[c]`` is the list of rows of clip c (an empty list: no row).  A row is one ``(start, end)`` pair or a list of
        them - ascending, not overlapping - in seconds (``span_frames``: ``t0 = round(start * 50)``, ``t1 = round((end - 0.005)
        * 50)``, the inverse of ``window_times``) or, with unit="frames", encoder frames [t0, t1) as they are.  A row's embedding
        is the plain head applied to the concatenation of its spans' frames as if they were a clip of their own: one time mean
        over all of them, ReLU, Linear, L2 norm - "the score of what is speech" is ONE row over the union of the speech spans,
        which per-window scores cannot give.  All rows come from ONE forward (``Engine.embed_spans_ragged``): the encoder saw
        the whole clip, so a row's score is not the score of the excerpt on its own.  A row ``[(0, T)]`` has the bits of
        ``score``, a row of one span the bits of ``score_over_time``'s window over those frames.

        Under ``torch.no_grad()``, or when nothing requires a gradient, the embeddings come from the scoring forward of
        ``precision``, then ``Engine.pairwise`` (k: ``Engine.knn``).  With a gradient the forward is
        ``embed_train_spans_ragged`` (fp32 buffers, products by ``Engine.gemm_precision``) and the backward runs
        ``cdist_backward`` / ``knn_backward`` over the rows, the span head's backward - a frame receives the sum of the gradients
        of the rows that contain it, exact zeros where none does - and the backbone down to the waveform; it carries
        ``feature_grad_mult`` as ``score``'s does and is zero behind every length.  ``references`` gets a gradient too when it
        requires one.  With reduction="mean" the 0-dim mean over all rows takes the place of ``scores``; weights per turn are
        plain torch, ``(scores * weights).sum()``."""
        check_reduction(reduction)
        check_references(references)
        k = check_k(k, references.shape[0]) if k is not None else None
        if not torch.is_tensor(wav) or wav.dim() not in (2, 3) or (wav.dim() == 3 and wav.shape[1] != 1):
            raise ValueError(f"wav must be (B,1,N) or (B,N), got {tuple(getattr(wav, 'shape', ()))}")
        lens = check_lengths(wav, lengths) if lengths is not None else [int(wav.shape[-1])] * int(wav.shape[0])
        if min(lens) < MIN_SAMPLES:
            raise ValueError(f"a clip of {min(lens)} samples is shorter than one encoder frame ({MIN_SAMPLES} samples)")
        table, counts = span_table(spans, [num_frames(n) for n in lens], unit)
        self._need_whole_encoder(self.engine)
        if torch.is_grad_enabled() and (wav.requires_grad or references.requires_grad):
            scores = _ScoreFn.apply(wav, references, self, lens, _TableRows(table), k)
        else:
            eng = self.engine
            x = wav.detach().to(eng.device, torch.float32).contiguous()
            x = x.squeeze(1) if x.dim() == 3 else x
            refs = references.detach().to(eng.device, torch.float32).contiguous()
            emb = eng.embed_spans_ragged([x[i, :n] for i, n in enumerate(lens)], table, precision=self._window_precision(sum(lens)))
            scores = self._reference_mean(emb, refs, k)
        return (scores.mean() if reduction == "mean" else scores), counts

    @staticmethod
    def _active_frame_counts(min_speech_s, min_gap_s):
        for name, s in (("min_speech_s", min_speech_s), ("min_gap_s", min_gap_s)):
            if isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)) or not math.isfinite(s) or s < 0:
                raise ValueError(f"{name} must be a non-negative number of seconds, got {s!r}")
        return int(round(float(min_speech_s) * FRAMES_PER_SECOND)), int(round(float(min_gap_s) * FRAMES_PER_SECOND))

    def _active_from_packed(self, packed, floor_db, min_speech, min_gap):
        """Frame energies of a packed batch (``Engine.frame_energy``), down to the host, through ``active_frames`` per clip."""
        frames = [num_frames(n) for n in packed[1]]
        e = self.engine.frame_energy(None, packed=packed)
        e = e.cpu().numpy() if torch.is_tensor(e) else np.asarray(e)
        out, at = [], 0
        for t in frames:
            out.append(active_frames(e[at:at + t], floor_db, min_speech, min_gap))
            at += t
        return out

    def active_spans(self, wav, lengths=None, floor_db=40.0, min_speech_s=0.1, min_gap_s=0.3):
        """Where a recording is not silent: -> per clip a list of ``(t0, t1)`` in encoder frames, ascending and not overlapping -
        what ``score_spans(..., spans=[[s] for s in active], unit="frames")`` takes as one row per clip.  wav (B,1,N) or (B,N);
        lengths as in ``score``.  The energy of a frame is the mean square of the 400 samples it sees (``Engine.frame_energy``,
        float64 on the GPU); the rule on them runs on the host (``active_frames``): a frame is active within ``floor_db`` dB of
        the clip's loudest frame, gaps of at most ``min_gap_s`` between active frames are closed, runs shorter than
        ``min_speech_s`` dropped; a clip where nothing is left (or that is all zeros, or not finite) gets its whole length.
        Deliberately simple: an energy gate, not a speech detector - music, noise and a slammed door are "active" too."""
        if not isinstance(floor_db, (int, float, np.integer, np.floating)) or isinstance(floor_db, bool) or not math.isfinite(floor_db):
            raise ValueError(f"floor_db must be a finite number of dB, got {floor_db!r}")
        min_speech, min_gap = self._active_frame_counts(min_speech_s, min_gap_s)
        if not torch.is_tensor(wav) or wav.dim() not in (2, 3) or (wav.dim() == 3 and wav.shape[1] != 1):
            raise ValueError(f"wav must be (B,1,N) or (B,N), got {tuple(getattr(wav, 'shape', ()))}")
        lens = check_lengths(wav, lengths) if lengths is not None else [int(wav.shape[-1])] * int(wav.shape[0])
        if min(lens) < MIN_SAMPLES:
            raise ValueError(f"a clip of {min(lens)} samples is shorter than one encoder frame ({MIN_SAMPLES} samples)")
        x = wav.detach().to(self.engine.device, torch.float32).contiguous()
        x = x.squeeze(1) if x.dim() == 3 else x
        return self._active_from_packed((x, lens), floor_db, min_speech, min_gap)

    def _score_file_spans(self, paths, test_files, ref_t, rows_of, active, max_batch_samples: int, k=None):
        """The file pipeline of ``_score_file_windows`` with the span head: -> one record per row, files in order: (file index,
        row label, spans in frames, score).  rows_of: ``spans_from_csv``'s result, or None with ``active`` = (floor_db, min speech
        frames, min gap frames): one row per file over its active spans, which costs a host round trip per staged batch (the
        energies come down, the table goes up)."""
        records = [[] for _ in paths]
        pending = None

        def collect(item):
            meta, fetch = item
            vals = fetch.result() if fetch is not None else np.full(len(meta), np.nan)
            for (i, label, spans), v in zip(meta, vals):
                records[i].append((i, label, spans, float(v)))

        for idxs, packed, uploaded in _staged_batches(paths, lambda p: self.load_processing(p, trim=False),
                                                      self.engine.pack_ragged_host, max_batch_samples, self.DECODE_THREADS,
                                                      self.PIPELINE_BATCHES, self.NATIVE_WAV_THREADS,
                                                      device=getattr(self.engine, "device", None)):
            frames = [num_frames(n) for n in packed[1]]
            if torch.is_tensor(packed[0]):   # one upload serves the energies and the forward
                packed = (packed[0].to(self.engine.device, non_blocking=True), packed[1])
            if rows_of is None:
                act = self._active_from_packed(packed, *active)
                rows, labels = [[a] for a in act], [["active"] for _ in act]
                unit = "frames"
            else:
                per_file = [rows_of.get(test_files[i], []) for i in idxs]
                rows, labels = [[p for _, p in r] for r in per_file], [[lab for lab, _ in r] for r in per_file]
                unit = "s"
            if not any(rows):
                uploaded()
                continue
            try:
                table, _ = span_table(rows, frames, unit)
            except ValueError as err:
                raise ValueError(f"{err} (clips of this batch: {[test_files[i] for i in idxs]})") from None
            emb = self.engine.embed_spans_ragged(None, table, precision=self._window_precision(sum(packed[1])), packed=packed)
            uploaded()
            meta = [(idxs[c], labels[c][r - table[0].index(c)], table[2][table[1][r]:table[1][r + 1]]) for r, c in enumerate(table[0])]
            fetch = self.engine.fetch_async(self._reference_mean(emb, ref_t, k)) if ref_t.shape[0] else None
            if pending is not None:
                collect(pending)
            pending = (meta, fetch)
        if pending is not None:
            collect(pending)
        return [r for rec in records for r in rec]

    def predict_spans(self, mode="dir", nmr="data/nmr-data", deg="data/test-data", spans=None, active_db=None, results_path=None,
                      max_batch_samples: int = 256 * 64000, k=None):
        """``predict`` over spans the caller names: -> (df_spans, df_avg).  Exactly one of:

        spans      a DataFrame or a csv path with the columns ``Test File`` (the label ``predict`` prints: the file's name without
                   directory and extension), ``start_s``, ``end_s`` and optionally ``Row``.  Lines of a file that share a ``Row``
                   label pool into ONE row (a speaker's turns, the speech of a call); without the column every line is its own row.
                   A file the csv names but ``deg`` does not list is an error; a test file without a line produces no row.
        active_db  one row per file over its active spans: ``active_spans(floor_db=active_db)`` with its default times.

        df_spans has one row per row, files in listing order: ``Test File``, ``Row``, ``start_s`` / ``end_s`` (the first span's
        start and the last span's end, ``span_times``), ``active_s`` (the seconds the row's frames cover, 0.02 s each) and
        ``NOMAD``, the row's mean distance to the reference embeddings rounded to 3 decimals; df_avg, indexed by ``Test File``,
        the mean of each file's rows.  Seconds become frames by ``span_frames``.  The test files go through the staged ragged
        batches of ``predict_segments`` with the span head (``score_spans`` says what a row is: pooled from one forward over the
        whole file, as if its spans' frames were a clip of their own).  With ``results_path`` the table is written to
        ``spans.csv`` there.  One process only, like ``predict_segments``.  k: as in ``predict_segments``."""
        if (spans is None) == (active_db is None):
            raise ValueError("predict_spans takes exactly one of spans= (a DataFrame or csv path) and active_db= (a floor in dB)")
        if active_db is not None and (isinstance(active_db, bool) or not isinstance(active_db, (int, float, np.integer, np.floating))
                                      or not math.isfinite(active_db)):
            raise ValueError(f"active_db must be a finite number of dB, got {active_db!r}")
        if k is not None:
            check_k(k, KNN_MAX)
        _check_predict_paths(mode, nmr, deg)
        world, _, _ = _dist_info(getattr(self, "group", None))
        if world > 1:
            raise RuntimeError(f"predict_spans runs in one process: this one belongs to a torch.distributed job of {world} ranks "
                               "(sharding the rows is not implemented; predict() shards whole-file scores)")
        paths = [str(p) for p in _file_table(deg)["filename"]]
        test_files = [x.split("/")[-1].split(".")[0] for x in paths]
        rows_of = spans_from_csv(spans, test_files) if spans is not None else None
        active = (float(active_db),) + self._active_frame_counts(0.1, 0.3) if active_db is not None else None
        print(f"Compute non-matching reference embeddings from {nmr}")
        nmr_embeddings = self.get_embeddings(nmr).set_index("filename")
        print(f"Compute degraded embeddings over spans from {deg}")
        ref_t = torch.from_numpy(np.ascontiguousarray(nmr_embeddings.to_numpy(dtype=np.float32))).to(self.engine.device)
        if k is not None:
            k = check_k(k, ref_t.shape[0])
        recs = self._score_file_spans(paths, test_files, ref_t, rows_of, active, max_batch_samples, k)
        times = [(span_times(s[0][0], s[-1][1]), sum(b - a for a, b in s) * 20 / 1000.0) for _, _, s, _ in recs]
        df = pd.DataFrame({"Test File": np.asarray([test_files[i] for i, _, _, _ in recs], dtype=object),
                           "Row": np.asarray([lab for _, lab, _, _ in recs], dtype=object),
                           "start_s": np.asarray([t[0][0] for t in times], dtype=np.float64),
                           "end_s": np.asarray([t[0][1] for t in times], dtype=np.float64),
                           "active_s": np.asarray([t[1] for t in times], dtype=np.float64),
                           "NOMAD": np.asarray([v for _, _, _, v in recs], dtype=np.float64)}).round({"NOMAD": 3})
        raw = pd.DataFrame({"Test File": [test_files[i] for i, _, _, _ in recs], "NOMAD": [v for _, _, _, v in recs]})
        df_mean = raw.groupby("Test File", sort=False)["NOMAD"].mean().to_frame().round(3)
        if results_path is not None:
            df.to_csv(os.path.join(results_path, "spans.csv"), index=False)   # (two label columns: not _write_rounded_csv's table)
        return df, df_mean

    # ---- degradations on the device ----------------------------------------------------------------------------------
    def _degrade_packed(self, buf, lens, kind: str, levels, noise):
        """One degradation of a packed device batch -> (rows (B G, stride), lengths repeated G times, alpha or thresholds or None);
        kind "reverb": ``noise`` holds the responses; kind "freeverb" (sox's reverb at ``levels``): the shared parameters, a dict."""
        if kind == "reverb":
            return self.engine.degrade_convolve(buf, noise, lengths=lens) + (None,)
        if kind == "freeverb":
            return self.engine.degrade_reverb(buf, levels, lengths=lens, **(noise or {})) + (None,)
        if kind == "noise":
            return self.engine.degrade_noise(buf, noise, levels, lengths=lens)
        return self.engine.degrade_clip(buf, levels, lengths=lens)

    def degrade(self, wav, kind, levels, noise=None, lengths=None):
        """Degraded copies of clean clips, made on the GPU: -> (clips (B G, stride) fp32 on the GPU, lengths): row ``b G + g`` is
        clip ``b`` at ``levels[g]`` with length ``lengths[b]`` (``lengths`` comes back repeated G times; every row is zero behind
        its length).  wav (B,1,N) or (B,N); lengths: the clips' exact lengths (any length from 1 sample); 1 .. 64 levels.

        kind "noise": ``levels`` are target SNRs in dB and ``noise`` a 1-D signal, tiled or cut to each clip:
        ``x + alpha s`` with ``alpha = (rms(x) / 10^(snr / 10)) / rms(s)`` - the reference's ``utils/degradations.py`` formula as it
        stands.  kind "clip": ``levels`` are clip factors in percent (0 .. 100): samples are clamped to the clip's own percentiles
        ``cf / 2`` and ``100 - cf / 2`` (numpy's linear rule, exact order statistics).  Both change the level with the
        degradation; the loudness normalisation the reference's rendering scripts apply afterwards is ``normalize`` (or
        ``intensity_sweep(normalize=...)``).  Codecs are not offered; reverberation is ``convolve`` (impulse responses) or ``reverb``
        (sox's reverberator).  No gradient."""
        if kind not in ("noise", "clip"):
            raise ValueError(f"kind must be 'noise' or 'clip', got {kind!r}")
        if not torch.is_tensor(wav) or wav.dim() not in (2, 3) or (wav.dim() == 3 and wav.shape[1] != 1):
            raise ValueError(f"wav must be (B,1,N) or (B,N), got {tuple(getattr(wav, 'shape', ()))}")
        if wav.requires_grad or (torch.is_tensor(noise) and noise.requires_grad):
            raise ValueError("degrade produces no gradient (the degradations have no backward): pass tensors that do not require one")
        if kind == "noise" and noise is None:
            raise ValueError("kind 'noise' needs a noise signal")
        if kind == "clip" and noise is not None:
            raise ValueError("noise goes with kind 'noise'")
        x = wav.detach().to(self.engine.device, torch.float32)
        x = (x.squeeze(1) if x.dim() == 3 else x).contiguous()
        lens = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)] if lengths is not None else [x.shape[1]] * x.shape[0]
        out, lens_rep, _ = self._degrade_packed(x, lens, kind, levels, noise)
        return out, lens_rep

    def convolve(self, wav, irs, lengths=None, ir_lengths=None):
        """Reverberant copies of clean clips, made on the GPU: every clip convolved with each of G impulse responses -> (clips
        (B G, stride) fp32 on the GPU, lengths): row ``b G + g`` is clip ``b`` through response ``g``, causal and cut to the clip's
        length (``lengths`` comes back repeated G times; every row is zero behind its length).  wav (B,1,N) or (B,N); lengths: the
        clips' exact lengths (any length from 1 sample); irs: a list of 1 .. 64 1-D responses of 1 .. 65536 taps each, or a (G,L)
        tensor with optional ``ir_lengths`` - measured rooms, or ``synthetic_rir``.  For a fixed setting a reverberator is this
        filter; sox's parameters are ``reverb``'s, codecs are not offered, the loudness normalisation of the reference's rendering scripts is
        ``normalize`` (a room adds its tail's energy).  fp32
        products and sums (``nomad_degrade_convolve``); a row does not depend on the batch it is made in.  No gradient."""
        if not torch.is_tensor(wav) or wav.dim() not in (2, 3) or (wav.dim() == 3 and wav.shape[1] != 1):
            raise ValueError(f"wav must be (B,1,N) or (B,N), got {tuple(getattr(wav, 'shape', ()))}")
        rows = [irs] if torch.is_tensor(irs) else list(irs)
        if wav.requires_grad or any(torch.is_tensor(h) and h.requires_grad for h in rows):
            raise ValueError("convolve produces no gradient (the degradations have no backward): pass tensors that do not require one")
        G = int(irs.shape[0]) if torch.is_tensor(irs) and irs.dim() == 2 else len(rows)
        if (torch.is_tensor(irs) and irs.dim() != 2) or not 1 <= G <= 64:
            raise ValueError(f"irs must be a list of 1 .. 64 1-D responses or a (G,L) tensor, got {tuple(irs.shape) if torch.is_tensor(irs) else G}")
        x = wav.detach().to(self.engine.device, torch.float32)
        x = (x.squeeze(1) if x.dim() == 3 else x).contiguous()
        lens = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)] if lengths is not None else [x.shape[1]] * x.shape[0]
        return self.engine.degrade_convolve(x, irs, lengths=lens, ir_lengths=ir_lengths)

    def reverb(self, wav, reverberance, lengths=None, **params):
        """Sox-style reverberant copies of clean clips, made on the GPU - the reference's REVERB degradation (``sox ... reverb P``,
        ``utils/degradations.py``) at its own condition values: -> (clips (B G, stride) fp32 on the GPU, lengths): row ``b G + g``
        is clip ``b`` at ``reverberance[g]`` (0 .. 100, 1 .. 64 levels), the reverberator's two channels averaged, cut to the clip's
        length (``lengths`` comes back repeated G times; every row is zero behind its length).  wav (B,1,N) or (B,N); lengths: the
        clips' exact lengths.  params, shared by the levels, are sox's: ``hf_damping=50, room_scale=100, stereo_depth=100,
        pre_delay_ms=0, wet_gain_db=0, wet_only=False`` plus ``clamp=True`` (limit to [-1, 1] as sox's sample conversion does) and
        ``sample_rate=16000``.  The comb and all-pass recurrences run in float64 (``nomad_degrade_reverb``); a row does not depend on
        the batch it is made in.  The algorithm is restated from memory of sox 14.4 and has NOT been checked against the sox binary.
        No gradient."""
        Engine.check_reverb(reverberance, **params)
        x, lens = self._rows_for_normalize(wav, lengths, "reverb")
        return self.engine.degrade_reverb(x, reverberance, lengths=lens, **params)

    def _rows_for_normalize(self, wav, lengths, what: str):
        """(B,1,N) / (B,N) clips and their lengths as a device tensor and a list, for ``loudness`` and ``normalize``."""
        if not torch.is_tensor(wav) or wav.dim() not in (2, 3) or (wav.dim() == 3 and wav.shape[1] != 1):
            raise ValueError(f"wav must be (B,1,N) or (B,N), got {tuple(getattr(wav, 'shape', ()))}")
        if wav.requires_grad:
            raise ValueError(f"{what} produces no gradient (the degradations have no backward): pass tensors that do not require one")
        x = wav.detach().to(self.engine.device, torch.float32)
        x = (x.squeeze(1) if x.dim() == 3 else x).contiguous()
        lens = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)] if lengths is not None else [x.shape[1]] * x.shape[0]
        return x, lens

    def loudness(self, wav, lengths=None, kind: str = "ebu"):
        """The level of every clip, measured on the GPU -> (R,) float64 on the device.  kind "ebu": ITU-R BS.1770-4 integrated
        loudness in LUFS at 16 kHz, one channel (K-weighting, 400 ms blocks, absolute gate at -70 LUFS, relative gate 10 LU under
        the gated mean); -inf for silence and for clips under 400 ms.  "rms" / "peak": dBFS of the clip's rms and of its SAMPLE peak
        (not the oversampled true peak).  wav (B,1,N) or (B,N), lengths: the clips' exact lengths."""
        Engine.check_normalize(0.0, kind, None, 16000)
        x, lens = self._rows_for_normalize(wav, lengths, "loudness")
        return self.engine.degrade_normalize(x, lengths=lens, kind=kind, measure_only=True)[2][:, 0]

    def normalize(self, wav, target: float = -23.0, kind: str = "ebu", lengths=None, peak_db=None):
        """Clips brought to one level on the GPU, as ``ffmpeg-normalize -nt <kind> -t <target>`` does to the reference's rendered
        files (its default: EBU R128, -23 LUFS) -> (rows (R, stride) fp32 on the GPU, lengths, stats (R, 4) float64 on the GPU =
        measured level, sample peak, applied gain, blocks past both gates).  The rows are packed as ``degrade`` returns them (zero
        behind each length) and go into ``score`` / ``embed_ragged(packed=...)``.  Each clip is scaled by ONE gain
        ``10^((target - level) / 20)``, lowered where needed so that the sample peak stays at ``peak_db`` dBFS; a clip without a
        level (silence; under 400 ms for "ebu") is returned unchanged.  This is the linear mode of ffmpeg's ``loudnorm``: its
        dynamic mode, loudness-range target and true-peak limiter are not offered.  No gradient."""
        Engine.check_normalize(target, kind, peak_db, 16000)
        x, lens = self._rows_for_normalize(wav, lengths, "normalize")
        return self.engine.degrade_normalize(x, lengths=lens, target=target, kind=kind, peak_db=peak_db)

    def _align_inputs(self, degraded, clean, lengths, degraded_lengths, max_delay_s, what: str):
        """The arguments of ``align`` checked on the host -> (clean tensor, its lengths, degraded tensor, its lengths, G, max delay
        in samples).  degraded: a (R,1,M) / (R,M) tensor of any width with ``degraded_lengths``, or a packed ``(rows, lengths)``."""
        max_delay = check_max_delay(max_delay_s)
        x, lens = self._rows_for_normalize(clean, lengths, what)
        if isinstance(degraded, tuple):
            if degraded_lengths is not None:
                raise ValueError("degraded_lengths go with a tensor: packed (rows, lengths) have their own")
            if len(degraded) != 2 or not torch.is_tensor(degraded[0]) or degraded[0].dim() != 2:
                raise ValueError("degraded must be a (R,1,M) or (R,M) tensor, or packed (rows (R, stride), lengths)")
            if degraded[0].requires_grad:
                raise ValueError(f"{what} produces no gradient (the degradations have no backward): pass tensors that do not require one")
            d, dlens = degraded[0].detach(), [int(n) for n in degraded[1]]
        else:
            d, dlens = self._rows_for_normalize(degraded, degraded_lengths, what)
        if len(lens) != x.shape[0] or len(dlens) != d.shape[0]:
            raise ValueError("lengths must hold one entry per clean clip, degraded_lengths one per degraded row")
        if not dlens or len(dlens) % len(lens) or len(dlens) // len(lens) > 64:
            raise ValueError(f"degraded must hold G rows per clean clip, G = 1 .. 64 (row b G + g belongs to clip b), got {len(dlens)} rows "
                             f"for {len(lens)} clips")
        if min(lens) < 1 or max(lens) > x.shape[1] or min(dlens) < 1 or max(dlens) > d.shape[1]:
            raise ValueError("every length must lie in 1 .. the width of its tensor")
        return x, lens, d, dlens, len(dlens) // len(lens), max_delay

    def align(self, degraded, clean, lengths=None, degraded_lengths=None, max_delay_s: float = 0.25):
        """Degraded clips brought into line with their clean clips on the GPU -> ((rows (B G, stride) fp32 on the GPU, lengths),
        delay (B G,) int32 on the GPU, peak (B G,) float64): row ``b G + g`` is degraded row ``b G + g`` moved by its delay, cut or
        zero-filled to clip ``b``'s length, so the pair goes straight into ``nsim``, ``score`` and ``embed_ragged(packed=...)``.
        clean (B,1,N) or (B,N) with ``lengths``; degraded a tensor of ANY width with ``degraded_lengths`` (its own exact lengths),
        or packed ``(rows, lengths)``; B G rows, G = 1 .. 64.  The delay is the lag, within ``max_delay_s`` (up to 1.024 s), of the
        largest cross-correlation ``sum_i clean[i] degraded[i + d]`` - positive where the degraded clip is late - and ONE whole
        number of samples per row: no sub-sample delays, no clock drift, no per-patch re-alignment, no polarity search; ``peak`` is
        the correlation there (NaN, with a delay of 0, where a row or its clip holds a NaN).  include/nomad_hip.h states the
        arithmetic (``nomad_align_delay``); agreement with ViSQOL's aligner has not been measured.  No gradient."""
        x, lens, d, dlens, G, max_delay = self._align_inputs(degraded, clean, lengths, degraded_lengths, max_delay_s, "align")
        eng = self.engine
        return eng.align(eng._rows(x, lens, None), self._packed_rows(d, dlens), G, max_delay)

    def _packed_rows(self, d, dlens):
        """A checked (R, M) tensor and its lengths as a packed device pair (no copy where it already is one)."""
        eng = self.engine
        d = d.to(eng.device, torch.float32)
        if d.shape[1] % 4 or not d.is_contiguous():
            return eng._pack([d[i, :n] for i, n in enumerate(dlens)])
        return eng._rows(None, None, (d, dlens))

    def nsim_patches(self, degraded, clean, lengths=None, degraded_lengths=None, patch_s: float = 0.4, search_s: float = 1.2,
                     vad_db: float = 40.0, min_active: float = 1.0, max_delay_s=None, intensity_range: float = 1.0):
        """The patch-wise NSIM of degraded clips with their clean clips, on the GPU: the clean clip's spectrogram is cut into
        patches of ``patch_s`` seconds, the ACTIVE ones are kept (a frame is active within ``vad_db`` dB of the clip's loudest
        frame; a patch needs the share ``min_active`` of its frames active), each is searched for within ``search_s`` seconds of
        its own place in the degraded spectrogram - the places of a row never going back -, and the patches' similarities are
        averaged.  A delay that changes inside a file (dropped or inserted frames, a drifting clock) so costs one patch instead of
        the whole score, and silence does not count.  -> a dict of device tensors: ``nsim`` (B, G) float64, ``bands`` (B, G, 21),
        ``offsets`` (B, G, P) int32 (the degraded frame every patch was found at, -1 where it is not kept; patch p starts at clean
        frame ``p * round(50 patch_s)``), ``patch_nsim`` (B, G, P) (NaN where not kept), ``kept`` (B, G) (the kept patches; a row
        with none has NaN), and ``delay`` (B, G) int32 with ``max_delay_s``: the global alignment of ``align`` first, then the
        patch search.  clean and degraded as ``align`` takes them; without ``max_delay_s`` a degraded row may be shorter or longer
        than its clip (``degraded_lengths``, or packed rows).  Whole frames of 20 ms only: no fine alignment per patch, no
        sub-sample delays, no polarity search, no MOS mapping, no gradient.  Modelled on ViSQOL's speech mode from memory and NOT
        checked against the ViSQOL binary; include/nomad_hip.h states the measure (``nomad_nsim_patches``)."""
        patch, search, vad_ratio, need = check_patch_params(patch_s, search_s, vad_db, min_active)
        eng = self.engine
        x, lens, d, dlens, G, max_delay = self._align_inputs(degraded, clean, lengths, degraded_lengths,
                                                             0.0 if max_delay_s is None else max_delay_s, "nsim_patches")
        one = 4 * (16000 // 50)
        if min(lens) < one or min(dlens) < one:
            raise ValueError(f"every clean clip and every degraded row needs one frame of {one} samples (80 ms)")
        crows = eng._rows(x, lens, None)
        drows = self._packed_rows(d, dlens)
        delay = None
        if max_delay_s is not None:
            drows, delay, _ = eng.align(crows, drows, G, max_delay)
        res = eng.nsim_patches(crows, drows, G, patch, search, vad_ratio, need, intensity_range=intensity_range)
        out = {"nsim": res["nsim"], "bands": res["bands"], "offsets": res["offsets"], "patch_nsim": res["patch_nsim"],
               "kept": (res["offsets"] >= 0).sum(dim=2)}
        if delay is not None:
            out["delay"] = delay.view(len(lens), G)
        return out

    def nsim(self, degraded, clean, lengths=None, bands: bool = False, intensity_range: float = 1.0, max_delay_s=None,
             degraded_lengths=None, patch_s=None, search_s: float = 1.2, vad_db: float = 40.0, min_active: float = 1.0):
        """The gammatone-spectrogram NSIM of degraded clips with their clean clips, computed on the GPU: the similarity the
        reference takes from ViSQOL before it samples triplets -> (B, G) float64 on the GPU, 1 for identical clips and falling with
        the degradation (with ``bands``: also the (B, G, 21) per-band values whose mean it is).  clean (B,1,N) or (B,N) with
        ``lengths``, the clips' exact lengths (at least 80 ms each); degraded: a tensor of clean's shape (G = 1), or the packed
        ``(rows, lengths)`` that ``degrade`` / ``convolve`` / ``reverb`` / ``normalize`` return for these clips - row ``b G + g``
        belongs to clip ``b`` - which is used without a copy.  21 ERB bands from 50 Hz to 8 kHz, 80 ms frames every 20 ms, dB
        floors, a 3 x 3 window over one similarity map of the whole clip (no patch search, no voice-activity gate, no MOS
        mapping).  Time alignment: with ``max_delay_s=None`` there is none and the rows must be sample-aligned with their clean
        clip, as everything the degradations make is.  With ``max_delay_s`` (seconds, up to 1.024) every row is first moved by its
        delay against its clip (``align``: one whole-sample delay per row); the degraded rows may then have any lengths - a tensor
        of another width takes ``degraded_lengths`` - and the (B, G) int32 delays are returned as one more, last result.
        Modelled on ViSQOL's speech mode from memory and NOT checked against the ViSQOL binary, neither the measure nor the
        delays; include/nomad_hip.h states both.  No gradient (``nsim_loss`` is the whole-clip measure's differentiable form).  With ``patch_s`` (seconds; ``search_s``, ``vad_db``, ``min_active``
        as ``nsim_patches`` takes them) the score and the band values are the patch-wise ones of ``nsim_patches``, in the same
        tuple; ``patch_s=None`` is every call as it was."""
        if patch_s is not None:
            res = self.nsim_patches(degraded, clean, lengths, degraded_lengths, patch_s, search_s, vad_db, min_active, max_delay_s,
                                    intensity_range)
            out = (res["nsim"],) + ((res["bands"],) if bands else ()) + ((res["delay"],) if max_delay_s is not None else ())
            return out if len(out) > 1 else out[0]
        if max_delay_s is not None:
            x, lens, d, dlens, G, max_delay = self._align_inputs(degraded, clean, lengths, degraded_lengths, max_delay_s, "nsim")
            eng = self.engine
            crows = eng._rows(x, lens, None)
            rows, delay, _ = eng.align(crows, self._packed_rows(d, dlens), G, max_delay)
            score, per_band = eng.nsim(crows, rows, G, intensity_range=intensity_range, want_bands=bands)
            delay = delay.view(len(lens), G)
            return (score, per_band, delay) if bands else (score, delay)
        if degraded_lengths is not None:
            raise ValueError("degraded_lengths go with max_delay_s: without alignment a degraded row has its clean clip's length")
        x, lens = self._rows_for_normalize(clean, lengths, "nsim")
        eng = self.engine
        cbuf, clens = eng._rows(x, lens, None)
        if isinstance(degraded, tuple):
            dbuf, dlens = degraded
            dlens = [int(n) for n in dlens]
            if not torch.is_tensor(dbuf) or dbuf.dim() != 2 or len(dlens) != dbuf.shape[0] or len(dlens) % len(clens) or not dlens:
                raise ValueError("degraded must be (rows (B G, stride), lengths) as degrade returns them, G rows per clean clip")
            G = len(dlens) // len(clens)
        else:
            if not torch.is_tensor(degraded) or tuple(degraded.shape) != tuple(clean.shape):
                raise ValueError("degraded must have clean's shape, or be the (rows, lengths) a degradation returned")
            d, _ = self._rows_for_normalize(degraded, lengths, "nsim")
            dbuf, dlens = eng._rows(d, lens, None)
            G = 1
        score, per_band = eng.nsim((cbuf, clens), (dbuf, dlens), G, intensity_range=intensity_range, want_bands=bands)
        return (score, per_band) if bands else score

    def nsim_loss(self, estimate, clean, lengths=None, reduction: str = "mean", intensity_range: float = 1.0):
        """The gammatone-spectrogram NSIM as a loss: ``1 - nsim(estimate, clean)`` per clip in float64, the number ``nsim`` reports,
        with a gradient down to ``estimate`` computed on the GPU in the same float64 arithmetic (``nomad_nsim_backward``,
        ``nomad_gammatone_backward``).  estimate and clean (B,1,N) or (B,N) of one shape, fp32; lengths: the clips' exact lengths as
        in ``forward`` (every clip at least 80 ms); -> (B,) float64, or with reduction="mean" their mean.  The gradient has
        estimate's shape and dtype and is 0 behind every clip's whole frames; ``clean`` gets none and must not require one.  A
        full-reference spectral term to add to the feature loss: ``nomad.forward(est, clean) + lam * nomad.nsim_loss(est, clean)``.
        The whole-clip measure only (no alignment, no patch search), and this project's measure, not ViSQOL's: neither the number
        nor the gradient has been checked against ViSQOL or any differentiable form of it.  include/nomad_hip.h ("NSIM as a
        loss") states the conventions that keep the gradient finite on silence."""
        check_reduction(reduction)
        for t, name in ((estimate, "estimate"), (clean, "clean")):
            if not torch.is_tensor(t) or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[1] != 1):
                raise ValueError(f"{name} must be (B,1,N) or (B,N), got {tuple(getattr(t, 'shape', ()))}")
        if tuple(clean.shape) != tuple(estimate.shape):
            raise ValueError(f"clean must have estimate's shape {tuple(estimate.shape)}, got {tuple(clean.shape)}")
        if clean.requires_grad:
            raise ValueError("nsim_loss differentiates with respect to estimate only: clean must not require a gradient")
        intensity_range = float(intensity_range)
        if not (math.isfinite(intensity_range) and intensity_range > 0.0):
            raise ValueError(f"intensity_range must be finite and positive, got {intensity_range}")
        lens = check_lengths(estimate, lengths) if lengths is not None else [int(estimate.shape[-1])] * estimate.shape[0]
        if not lens:
            raise ValueError("nsim_loss needs at least one clip")
        if min(lens) < NSIM_FRAME_SAMPLES:
            raise ValueError(f"a clip of {min(lens)} samples is shorter than one frame of {NSIM_FRAME_SAMPLES}")
        loss = _NsimLossFn.apply(estimate, clean, self, lens, intensity_range)
        return loss.mean() if reduction == "mean" else loss

    def nsim_files(self, degraded, clean=None, max_delay_s: float = 0.25, results_path=None, max_batch_samples: int = 64 * 160000,
                   patch_s=None, search_s: float = 1.2, vad_db: float = 40.0, min_active: float = 1.0):
        """The NSIM of rendered files with their clean files, each pair aligned first: files a codec, a device or another program
        made, which are not sample-aligned with their source.  ``degraded`` and ``clean``: two lists of paths of one length; or
        ``degraded`` alone: a csv path (or DataFrame) with the columns ``filepath_ref`` and ``filepath_deg``, the reference's
        ``degraded_data_visqol_format.csv``.  -> a DataFrame ``filepath_ref, filepath_deg, delay_samples, delay_s, NSIM`` in the
        pairs' order, written to ``nsim_pairs.csv`` under ``results_path`` if given.  The files go through the staged reader of
        ``predict`` (mono, resampled to 16 kHz), pairs are batched up to ``max_batch_samples`` samples, and every pair is
        ``nsim(max_delay_s=...)`` of its two files: the degraded file moved by ONE delay of whole samples (positive: it is late)
        and cut or zero-filled to the clean file's length.  A pair whose clean file is under 80 ms gets NaN.  The NSIM is this
        project's (``nsim``) and the delay search is not ViSQOL's either: neither has been checked against that binary.  With
        ``patch_s`` the NSIM is the patch-wise one (``nsim_patches`` after the same alignment) and the table gains ``patches_kept``,
        ``offset_min_frames`` and ``offset_max_frames``: the kept patches of the pair, and the smallest and largest distance, in
        frames of 20 ms, of a patch's found place from its own start (NaN where no patch is kept); without it the file is what it was."""
        patches = check_patch_params(patch_s, search_s, vad_db, min_active) if patch_s is not None else None
        if clean is None:
            ref_paths, deg_paths = pairs_from_csv(degraded)
        else:
            if isinstance(degraded, (str, os.PathLike)) or isinstance(clean, (str, os.PathLike)):
                raise ValueError("nsim_files takes two lists of paths, or one csv with the columns filepath_ref and filepath_deg")
            ref_paths, deg_paths = [str(p) for p in clean], [str(p) for p in degraded]
            if len(ref_paths) != len(deg_paths) or not ref_paths:
                raise ValueError(f"nsim_files needs as many clean files as degraded ones and at least one, got {len(ref_paths)} and {len(deg_paths)}")
        max_delay = check_max_delay(max_delay_s)
        eng = self.engine
        paths = [p for pair in zip(ref_paths, deg_paths) for p in pair]      # file 2 k is pair k's clean file, 2 k + 1 its degraded one
        delays, scores = np.zeros(len(ref_paths), dtype=np.int64), np.full(len(ref_paths), np.nan)
        kept, off_lo, off_hi = np.zeros(len(ref_paths), dtype=np.int64), np.full(len(ref_paths), np.nan), np.full(len(ref_paths), np.nan)
        held, fetches = {}, []

        def run(ks):
            cbuf, clens = eng._pack([held[2 * k] for k in ks])
            rows, delay, _ = eng.align((cbuf, clens), eng._pack([held[2 * k + 1] for k in ks]), 1, max_delay)
            ok = [i for i, n in enumerate(clens) if Engine.gammatone_frames(n) >= 1]
            sims = offs = None
            if ok:
                pick = torch.as_tensor(ok, device=eng.device)
                lens_ok = [clens[i] for i in ok]
                if patches is None:
                    sims = eng.nsim((cbuf[pick], lens_ok), (rows[0][pick], lens_ok), 1, want_bands=False)[0].reshape(-1)
                else:
                    res = eng.nsim_patches((cbuf[pick], lens_ok), (rows[0][pick], lens_ok), 1, *patches, want_bands=False)
                    sims, offs = res["nsim"].reshape(-1), eng.fetch_async(res["offsets"][:, 0, :].contiguous())
            fetches.append((ks, ok, eng.fetch_async(delay), eng.fetch_async(sims) if ok else None, offs))
            for k in ks:
                del held[2 * k], held[2 * k + 1]

        for idxs, packed, uploaded in _staged_batches(paths, lambda p: self.load_processing(p, trim=False), eng.pack_ragged_host,
                                                      max_batch_samples, self.DECODE_THREADS, self.PIPELINE_BATCHES, self.NATIVE_WAV_THREADS,
                                                      device=getattr(eng, "device", None)):
            buf, lens = eng._pack(None, packed)
            uploaded()
            for r, i in enumerate(idxs):
                held[i] = buf[r, :lens[r]]
            ks = sorted(i // 2 for i in idxs if i % 2 and i - 1 in held)      # a pair is whole once its degraded file is here
            if ks:
                run(ks)
        for ks, ok, delay, sims, offs in fetches:
            delays[ks] = delay.result()
            if ok:
                scores[[ks[i] for i in ok]] = sims.result()
            if offs is not None:
                table = np.asarray(offs.result())
                rel = table - np.arange(table.shape[1])[None, :] * patches[0]      # from the patch's own start
                for i, row in zip(ok, range(table.shape[0])):
                    on = table[row] >= 0
                    kept[ks[i]] = int(on.sum())
                    if on.any():
                        off_lo[ks[i]], off_hi[ks[i]] = rel[row][on].min(), rel[row][on].max()
        df = pd.DataFrame({"filepath_ref": ref_paths, "filepath_deg": deg_paths, "delay_samples": delays, "delay_s": delays / 16000.0,
                           "NSIM": scores})
        if patches is not None:
            df["patches_kept"], df["offset_min_frames"], df["offset_max_frames"] = kept, off_lo, off_hi
        if results_path is not None:
            os.makedirs(results_path, exist_ok=True)
            df.to_csv(os.path.join(results_path, "nsim_pairs.csv"), index=False)
        return df

    def mine_triplets(self, clean, noise=None, snr_db=None, clip_factor=None, reverberance=None, normalize=-23.0, lengths=None,
                      N: int = 3, hard_sampling: bool = False, margin: float = 0.05, seed=0, patch_s=None, vad_db: float = 40.0,
                      min_active: float = 1.0):
        """From clean clips to (Anchor, Positive, Negative) batches with nothing rendered to disk - the reference's data
        preparation (degrade, ``ffmpeg-normalize``, ViSQOL's NSIM, ``nsim_triplet_sampling.py``) on the GPU.  The clips are
        degraded at every given level (``snr_db`` with ``noise``, ``clip_factor``, ``reverberance``: the C conditions, in that
        order); with ``normalize`` (LUFS, None: not at all) every degraded row and a copy of the clean clip are brought to that
        loudness; the NSIM of every degraded row is taken against the UN-normalised clean clip, as the reference hands ViSQOL
        its original wav; the (B, C) table makes one round trip to the host, where ``triplets.create_triplets`` samples up to N
        triplets per clip (``hard_sampling``, ``margin``, ``seed``: its arguments); the three branches are gathered on the GPU.

        -> (anchor, positive, negative, info): each branch a ``(rows (K, stride) fp32 on the GPU, lengths)`` pair as
        ``forward_triplet`` / ``embed_ragged(packed=...)`` take them, K <= B N; ``info`` = {"nsim": the (B, C) float64 table,
        "conditions": [(kind, level)] per column, "triplets": ``create_triplets``' index table (member C is the clean clip),
        "dropped": its count of draws that gave no row}.  The NSIM is this project's (``nsim``), not ViSQOL's.  No gradient.
        With ``patch_s`` the table is the patch-wise measure (``nsim_patches`` with ``vad_db`` and ``min_active``; the rows are
        sample-aligned by construction, so a patch is searched for within one patch length of its place): silence then does not
        count.  Clips one of whose rows has no kept patch (too short, nothing active enough) are left out of the sampling and
        listed in ``info["no_patches"]``; ``info["triplets"]["clip"]`` keeps the clips' own indices."""
        from .triplets import create_triplets
        patches = check_patch_params(patch_s, patch_s, vad_db, min_active) if patch_s is not None else None
        x, lens = self._rows_for_normalize(clean, lengths, "mine_triplets")
        if snr_db is not None and noise is None:
            raise ValueError("snr_db needs a noise signal: pass noise=")
        if torch.is_tensor(noise) and noise.requires_grad:
            raise ValueError("mine_triplets produces no gradient: pass tensors that do not require one")
        sweeps = [(kind, [float(v) for v in np.asarray(levels, dtype=np.float64).reshape(-1)])
                  for kind, levels in (("noise", snr_db), ("clip", clip_factor), ("freeverb", reverberance)) if levels is not None]
        if not sweeps:
            raise ValueError("mine_triplets needs snr_db, clip_factor or reverberance")
        for kind, levels in sweeps:
            if not 1 <= len(levels) <= 64:
                raise ValueError(f"{kind}: 1 .. 64 levels, got {len(levels)}")
        if normalize is not None:
            Engine.check_normalize(normalize, "ebu", None, 16000)
        eng = self.engine
        buf, lens = eng._rows(x, lens, None)
        B, stride = buf.shape
        if noise is not None:
            noise = torch.as_tensor(noise, dtype=torch.float32).reshape(-1).to(eng.device)
        spec_ref, frames = eng.gammatone(packed=(buf, lens))
        members, scores = [], []
        for kind, levels in sweeps:
            out, lens_rep, _ = self._degrade_packed(buf, lens, kind, levels, noise if kind == "noise" else None)
            if normalize is not None:
                eng.degrade_normalize(packed=(out, lens_rep), target=normalize, inplace=True)
            spec_deg, _ = eng.gammatone(packed=(out, lens_rep))
            if patches is None:
                scores.append(eng.nsim_of_spectrograms(spec_ref, spec_deg, frames, len(levels), want_bands=False)[0])
            else:
                scores.append(eng.nsim_patches_of_spectrograms(spec_ref, spec_deg, frames, [f for f in frames for _ in levels], len(levels),
                                                               *patches, want_bands=False)["nsim"])
            members.append(out.view(B, len(levels), stride))
        if normalize is not None:
            clean_member = eng.degrade_normalize(packed=(buf, lens), target=normalize)[0]
        else:                     # the clean member is zero behind its length like every other row
            clean_member = buf.clone()
            for b, n in enumerate(lens):
                clean_member[b, n:] = 0.0
        members.append(clean_member.view(B, 1, stride))
        table = torch.cat(scores, dim=1).cpu().numpy()        # the one round trip
        no_patches = []
        if patches is None:
            triplets, dropped = create_triplets(table, N=N, hard_sampling=hard_sampling, margin=margin, rng=seed)
        else:                     # a row without a kept patch has NaN: its clip is not sampled from
            no_patches = [int(b) for b in np.nonzero(np.isnan(table).any(axis=1))[0]]
            sampled = np.asarray([b for b in range(B) if b not in no_patches], dtype=np.int64)
            if sampled.size == 0:
                raise ValueError("mine_triplets: no clip has a kept patch in all of its rows (patch_s too long, or nothing active)")
            triplets, dropped = create_triplets(table[sampled], N=N, hard_sampling=hard_sampling, margin=margin, rng=seed)
            triplets = dict(triplets)
            triplets["clip"] = sampled[triplets["clip"]]
        bank = torch.cat(members, dim=1)
        C1 = bank.shape[1]
        bank = bank.view(B * C1, stride)
        branch_lens = [lens[b] for b in triplets["clip"]]
        branches = []
        for key in ("anchor", "positive", "negative"):
            idx = torch.from_numpy(triplets["clip"] * C1 + triplets[key]).to(eng.device)
            branches.append((bank.index_select(0, idx), list(branch_lens)))
        info = {"nsim": table, "conditions": [(kind, v) for kind, levels in sweeps for v in levels], "triplets": triplets, "dropped": dropped}
        if patches is not None:
            info["no_patches"] = no_patches
        return branches[0], branches[1], branches[2], info

    def _clean_batches(self, clean, lengths, budget: int):
        """The clean clips of ``intensity_sweep`` as packed device batches of at most ``budget`` samples each (one clip at least):
        yields (names, buffer, lengths)."""
        eng = self.engine
        if isinstance(clean, (str, os.PathLike)):
            if lengths is not None:
                raise ValueError("lengths go with tensors: files have their own")
            paths = [str(p) for p in _file_table(str(clean))["filename"]]
            for idxs, packed, uploaded in _staged_batches(paths, lambda p: self.load_processing(p, trim=False), eng.pack_ragged_host,
                                                          budget, self.DECODE_THREADS, self.PIPELINE_BATCHES, self.NATIVE_WAV_THREADS,
                                                          device=getattr(eng, "device", None)):
                buf, lens = eng._pack(None, packed)
                uploaded()
                yield [paths[i] for i in idxs], buf, lens
            return
        if torch.is_tensor(clean):
            if clean.dim() not in (2, 3) or (clean.dim() == 3 and clean.shape[1] != 1):
                raise ValueError(f"clean must be (B,1,N) or (B,N), a list of clips, a directory or a csv file, got {tuple(clean.shape)}")
            x = clean.squeeze(1) if clean.dim() == 3 else clean
            lens = check_lengths(x, lengths) if lengths is not None else [x.shape[1]] * x.shape[0]
            clips = [x[i, :n] for i, n in enumerate(lens)]
        else:
            if lengths is not None:
                raise ValueError("lengths go with a padded tensor: a list of clips has its own")
            clips = [torch.as_tensor(w).reshape(-1) for w in clean]
        if any(torch.is_tensor(w) and w.requires_grad for w in clips):
            raise ValueError("intensity_sweep produces no gradient (the degradations have no backward): pass tensors that do not require one")
        lo = 0
        while lo < len(clips):
            hi, total = lo + 1, int(clips[lo].numel())
            while hi < len(clips) and total + int(clips[hi].numel()) <= budget:
                total += int(clips[hi].numel())
                hi += 1
            buf, lens = eng.pack_ragged([w.detach() for w in clips[lo:hi]])
            yield [f"clip{i}" for i in range(lo, hi)], buf, lens
            lo = hi

    def intensity_sweep(self, clean, references, noise=None, snr_db=None, clip_factor=None, lengths=None, k=None,
                        max_batch_samples: int = 256 * 64000, rt60_s=None, rir_seed: int = 0, drr_db: float = 0.0,
                        normalize=None, normalize_kind: str = "ebu", reverberance=None, reverb_params=None, nsim: bool = False):
        """Does the score rank the strength of a degradation?  The reference's ``intensity`` experiment without rendered files: the
        clean clips are degraded on the GPU (``degrade``) at every level, embedded and scored against ``references`` ((Nr,256), as
        ``score`` takes them); -> {"NOISE": {...}, "CLIP": {...}, "REVERB": {...}}, a degradation whose levels are None being left out.  Each entry is
        ``train.intensity_stats``'s result - ``table`` (``Condition`` = the level, ``Distance`` = the mean score of the clips at that
        level, sorted by Distance), ``SRCC`` = spearmanr(Distance, Condition), ``embeddings`` - plus ``scores``, the (N G,) float64
        scores in row order (clip b at level g in row b G + g; at fp32 the bits of ``score`` on ``degrade``'s rows).

        clean: a (B,1,N) / (B,N) tensor (with ``lengths``), a list of 1-D clips, a directory of wav files or a csv file with a
        ``filename`` column (the file pipeline of ``get_embeddings``).  snr_db needs ``noise``, a 1-D signal at 16 kHz.  k: the
        nearest-reference score of ``score(k=...)``.  rt60_s: reverberation times in seconds, each in (0, 4.096]: the clips are
        convolved (``convolve``) with ``synthetic_rir(rt60, rir_seed, drr_db)`` - a synthetic diffuse room, NOT sox's reverb (that is ``reverberance``) -
        and ``Condition`` is the RT60; whether the score ranks it is not claimed.  reverberance: sox's reverb itself (``reverb``)
        at these levels, 0 .. 100 - the reference's REVERB conditions - with ``reverb_params`` (a dict of ``reverb``'s shared
        parameters, or None) and ``Condition`` the reverberance; it fills the same ``REVERB`` entry, so it goes without rt60_s.  The clean audio is uploaded once per batch; batches are cut so that the
        G-fold degraded rows stay within ``max_batch_samples`` samples.

        normalize: None - the degraded rows are scored at whatever level the degradation left them (noise at 0 dB SNR is 3 dB
        louder than the clip, a 40 % clip factor several dB quieter).  A number: every degraded row is brought to that level in
        place before it is embedded (``normalize``; ``normalize_kind`` "ebu" = LUFS as the reference's ``ffmpeg-normalize`` step,
        -23 being its default, or "rms" / "peak" in dBFS), so that the score ranks the degradation at equal loudness; each entry
        then also has ``gain_db``, the (N G,) float64 gains applied, in row order.

        nsim: each entry also gets ``nsim``, the (N G,) float64 NSIM of every scored row with its clean clip (``nsim``: this
        project's gammatone measure, one more call over the same rows; the clean clip is taken as it is, the degraded row as it
        is scored), in row order - the similarity the model was trained to order, next to the score.  Every clip then needs 80 ms."""
        from .train import intensity_stats
        check_references(references)
        if normalize is not None:
            Engine.check_normalize(normalize, normalize_kind, None, 16000)
        k = check_k(k, references.shape[0]) if k is not None else None
        if rt60_s is not None and reverberance is not None:
            raise ValueError("rt60_s and reverberance both fill the REVERB entry: pass one of them")
        if reverb_params is not None and reverberance is None:
            raise ValueError("reverb_params go with reverberance")
        if reverberance is not None:
            Engine.check_reverb(np.asarray(reverberance, dtype=np.float64).reshape(-1), **(reverb_params or {}))
        if snr_db is None and clip_factor is None and rt60_s is None and reverberance is None:
            raise ValueError("intensity_sweep needs snr_db, clip_factor or both, or rt60_s, or reverberance")
        if snr_db is not None and noise is None:
            raise ValueError("snr_db needs a noise signal: pass noise=")
        if references.requires_grad or (torch.is_tensor(noise) and noise.requires_grad):
            raise ValueError("intensity_sweep produces no gradient (the degradations have no backward): pass tensors that do not require one")
        sweeps = [(name, kind, [float(v) for v in np.asarray(levels, dtype=np.float64).reshape(-1)])
                  for name, kind, levels in (("NOISE", "noise", snr_db), ("CLIP", "clip", clip_factor), ("REVERB", "reverb", rt60_s),
                                             ("REVERB", "freeverb", reverberance))
                  if levels is not None]
        for name, _, levels in sweeps:
            if not 1 <= len(levels) <= 64:
                raise ValueError(f"{name}: 1 .. 64 levels per sweep, got {len(levels)}")
        rirs = [torch.from_numpy(synthetic_rir(v, rir_seed, drr_db)) for v in sweeps[-1][2]] if rt60_s is not None else None
        sox_params = dict(reverb_params or {})
        self._need_whole_encoder(self.engine)
        eng = self.engine
        refs = references.detach().to(eng.device, torch.float32).contiguous()
        if noise is not None:
            noise = torch.as_tensor(noise, dtype=torch.float32).reshape(-1).to(eng.device)
        rows = {name: ([], [], [], [], []) for name, _, _ in sweeps}  # row names, levels, embeddings, gains and NSIM in flight
        budget = max(1, int(max_batch_samples) // max(len(levels) for _, _, levels in sweeps))
        for names, buf, lens in self._clean_batches(clean, lengths, budget):
            spec_ref, frames = eng.gammatone(packed=(buf, lens)) if nsim else (None, None)
            for name, kind, levels in sweeps:
                if kind == "reverb" and isinstance(rirs, list):
                    rirs = eng.pack_responses(rirs)      # packed and uploaded once, with the first batch
                out, lens_rep, _ = self._degrade_packed(buf, lens, kind, levels,
                                                        rirs if kind == "reverb" else sox_params if kind == "freeverb" else noise)
                if normalize is not None:
                    _, _, stats = eng.degrade_normalize(packed=(out, lens_rep), target=normalize, kind=normalize_kind, inplace=True)
                    rows[name][3].append(eng.fetch_async(stats))
                if nsim:
                    spec_deg, _ = eng.gammatone(packed=(out, lens_rep))
                    rows[name][4].append(eng.fetch_async(eng.nsim_of_spectrograms(spec_ref, spec_deg, frames, len(levels),
                                                                                  want_bands=False)[0].reshape(-1)))
                emb = eng.embed_ragged(None, precision=self._window_precision(sum(lens_rep)), packed=(out, lens_rep))
                rows[name][0].extend(f"{n}|{name}_{g}" for n in names for g in range(len(levels)))
                rows[name][1].extend(levels * len(names))
                rows[name][2].append(eng.fetch_async(emb))
        ref_df = pd.DataFrame(refs.cpu().numpy())
        results = {}
        for name, _, _ in sweeps:
            row_names, conds, fetches, gains, sims = rows[name]
            if not row_names:
                raise ValueError("intensity_sweep: no clean clip to degrade")
            df_emb = pd.concat([pd.DataFrame({"filepath_deg": row_names}),
                                pd.DataFrame(np.concatenate([f.result() for f in fetches]))], axis=1)
            deg_data = pd.DataFrame({"filepath_deg": row_names, "Condition": conds})
            scores = {}

            def nmr_mean(test, ref):
                dev = eng.device
                scores["rows"] = self._reference_mean(torch.from_numpy(test).to(dev), torch.from_numpy(ref).to(dev), k).cpu().numpy()
                return scores["rows"]

            results[name] = intensity_stats(df_emb, deg_data, ref_df, nmr_mean, name)
            results[name]["scores"] = scores["rows"]
            if normalize is not None:
                with np.errstate(divide="ignore"):
                    results[name]["gain_db"] = 20.0 * np.log10(np.concatenate([f.result() for f in gains])[:, 2])
            if nsim:
                results[name]["nsim"] = np.concatenate([f.result() for f in sims])
                results[name]["conditions"] = np.asarray(conds, dtype=np.float64)
        return results

    def graphed_loss(self, estimate: torch.Tensor, clean: torch.Tensor, lengths=None) -> "GraphedLoss":
        """``forward`` + backward for inputs of this shape, captured as one HIP graph (see ``GraphedLoss``): for training loops with
        a fixed batch shape - the per-step launch overhead of ~440 small kernels disappears, the bits do not change."""
        if lengths is not None:
            raise ValueError("GraphedLoss captures ONE batch shape: exact lengths (a different geometry every step) are not captured; "
                             "use nomad.forward(estimate, clean, lengths)")
        return GraphedLoss(self, estimate, clean)

    def _all_gather_rows(self, x: torch.Tensor) -> torch.Tensor:
        """Rows of every rank, in rank order, on every rank (nccl = RCCL needs device tensors, gloo takes host ones)."""
        import torch.distributed as dist
        from .dist import all_gather_rows
        if dist.get_backend(getattr(self, "group", None)) == "nccl":
            x = x.to(self.engine.device)
        return all_gather_rows(x.contiguous(), getattr(self, "group", None), force_collective=True)

    def get_embeddings(self, path):
        if os.path.isdir(path):
            data = pd.DataFrame(os.listdir(path))
            data.columns = ["filename"]
            data["filename"] = [os.path.join(path, x) for x in data["filename"]]
        elif os.path.isfile(path):
            data = pd.read_csv(path)
            if "filename" not in data.columns:
                raise Exception("File {path} not including a column called filename. Please pass a csv file with a "
                                "column called filename that includes the absolute filpaths of the waveforms.")
        else:
            raise Exception(f"Path {path} does not exist")
        return self.get_embeddings_csv(self.model, data)

    def _embed_files_into(self, paths, embeddings: np.ndarray, max_batch_samples: int, features: bool = False) -> None:
        """The file pipeline over ``paths`` -> rows of ``embeddings`` (same order).  features: the 768 pooled backbone
        features of ``Origw2v`` instead of the 256-dimensional embeddings."""
        pending = None                                   # (row indices, host copy in flight) of the previous batch
        for idxs, packed, uploaded in _staged_batches(paths, lambda p: self.load_processing(p, trim=False),
                                                      self.engine.pack_ragged_host, max_batch_samples, self.DECODE_THREADS,
                                                      self.PIPELINE_BATCHES, self.NATIVE_WAV_THREADS,
                                                      device=getattr(self.engine, "device", None)):
            prec = self.precision
            if prec == "bf16x3" and sum(packed[1]) < BF16X3_MIN_SAMPLES:
                # a handful of files does not fill the 256 x 256 tiles of the split-storage path: they take the fp32-buffer forward,
                # which is the faster one there.  Its GEMM products follow Engine.gemm_precision, and Nomad(precision="bf16x3") has
                # set that to "bf16x3" - so these embeddings are bf16x3-class (~1e-6 from fp32) too, not exact fp32
                prec = "fp32"
            embed = self.engine.embed_features_ragged if features else self.engine.embed_ragged
            emb = embed(None, precision=prec, packed=packed)                       # asynchronous
            uploaded()                                                             # the staging slot is free once the copy is done
            fetch = self.engine.fetch_async(emb)                                   # D2H enqueued right behind it
            if pending is not None:
                embeddings[pending[0]] = pending[1].result()                        # waits for the PREVIOUS batch only
            pending = (idxs, fetch)
        if pending is not None:
            embeddings[pending[0]] = pending[1].result()

    def get_embeddings_csv(self, model, file_names, root=False, max_batch_samples: int = 256 * 64000):
        """Embeddings for every row of ``file_names`` (a DataFrame with the path in column 0).

        The reference embeds one file per iteration with a device sync each time (nomad.py:171-183).  Here files
        of arbitrary lengths are packed into ragged batches (``nomad_embed_ragged``: no padding enters the
        arithmetic, results are bit-identical to per-file calls) of at most ``max_batch_samples`` samples, as a
        pipeline (``_staged_batches``): a packer thread has the C ABI's reader decode (and resample) each batch on native
        host threads straight into a pinned staging buffer, and this thread only enqueues GPU work - batch k+1 is
        built and launched while the GPU still runs batch k, and results are fetched one batch late.
        Like the reference, which holds one clip at a time, memory does not grow with the size of the directory:
        never more than ``PIPELINE_BATCHES`` staged batches (plus the decode look-ahead) are alive.
        Inside a ``torch.distributed`` job (one process per GPU) every rank embeds its contiguous slice of the list
        and one all-gather gives every rank the whole table.
        ``model``: an ``Origw2v`` yields its 768 feature columns (the raw wav2vec 2.0 baseline) through the same pipeline;
        anything else (the reference passes ``self.model``) the 256-dimensional NOMAD embeddings."""
        features = isinstance(model, Origw2v)
        file_names_arr = np.array(file_names)
        paths = []
        for row in file_names_arr:
            name = row[0] if isinstance(row, np.ndarray) else row
            paths.append(os.path.join(root, name) if root else name)
        # one process per GPU under torch.distributed: every rank embeds a contiguous slice of the file list, one
        # all-gather (RCCL over xGMI; gloo on CPU) hands every rank all embeddings in listing order
        world, rank, collective = _dist_info(getattr(self, "group", None))
        lo, hi = partition(len(paths), world, rank) if collective else (0, len(paths))
        mine = paths[lo:hi]
        embeddings = np.zeros((len(mine), SSL_OUT_DIM if features else EMB_DIM), dtype=np.float32)
        failure = None
        try:
            if features:
                self._embed_files_into(mine, embeddings, max_batch_samples, features=True)
            else:
                self._embed_files_into(mine, embeddings, max_batch_samples)
        except Exception as e:  # noqa: BLE001 - inside a job the other ranks must hear about it before anybody raises
            if not collective:
                raise
            failure = e
        if collective:
            # a rank that failed (an unreadable file in its slice) must not leave the others waiting in the all-gather
            flags = self._all_gather_rows(torch.tensor([0 if failure is None else 1], dtype=torch.int32)).cpu().tolist()
            if any(flags):
                if failure is not None:
                    raise failure
                raise RuntimeError(f"get_embeddings_csv: rank(s) {[r for r, f in enumerate(flags) if f]} failed on their files")
        if collective:
            embeddings = self._all_gather_rows(torch.from_numpy(embeddings)).cpu().numpy()
        emb_df = pd.DataFrame(embeddings)
        df_emb = pd.concat([file_names.reset_index(), emb_df], axis=1).drop("index", axis=1)
        return df_emb

    # files are decoded (and resampled) by the C ABI's reader on plain host threads (0: everything through load_processing);
    # files it does not take (unusual headers / encodings) are decoded on a few Python threads - more than two of those
    # only fight over the interpreter lock
    NATIVE_WAV_THREADS = int(os.environ.get("NOMAD_WAV_THREADS", min(8, os.cpu_count() or 1)))
    DECODE_THREADS = int(os.environ.get("NOMAD_DECODE_THREADS", min(2, os.cpu_count() or 1)))
    PIPELINE_BATCHES = 2      # staged batches alive at any time: one on the GPU, one being built / waiting

    def load_processing(self, filepath, target_sr=16000, trim=False):
        """file -> (1, N) fp32 mono tensor at 16 kHz, like the reference (nomad.py:192-212) but without torchaudio."""
        return torch.from_numpy(wavio.load_processing(filepath, target_sr, trim))
