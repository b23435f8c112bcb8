"""Host-side handle on the HIP engine: owns a nomad_ctx, hands it device buffers that PyTorch-ROCm
allocates, and launches on torch's current HIP stream.  PyTorch is plumbing here (memory, streams,
torch.distributed); every FLOP of the NOMAD path runs in libnomad_hip.so."""
from __future__ import annotations

import math
import os

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from .weights import check_state_dict, num_frames, num_windows

P = "ssl_model."
_SUFFIX = {"fp32": "", "bf16": "_bf16", "bf16x3": "_bf16x3"}   # of the C ABI's per-precision entry points
# the largest workspace ``gammatone_backward`` / ``nsim_backward`` ask for in one call: rows beyond it go into further calls
NSIM_BACKWARD_WORKSPACE_BYTES = 1 << 30


def _ptr(t: Optional[torch.Tensor]):
    """An optional tensor's device pointer: None (a NULL argument) where the tensor is left out."""
    return None if t is None else t.data_ptr()


def _weights_struct(sd: Dict[str, torch.Tensor]):
    """Build the nomad_weights struct of HOST pointers; returns (struct, keepalive list)."""
    keep = []

    def ptr(key):
        t = sd[key].detach().to(device="cpu", dtype=torch.float32).contiguous()
        keep.append(t)
        return t.data_ptr()

    w = _lib.Weights()
    for i in range(7):
        w.conv_w[i] = ptr(P + f"feature_extractor.conv_layers.{i}.0.weight")
    w.gn_w = ptr(P + "feature_extractor.conv_layers.0.2.weight")
    w.gn_b = ptr(P + "feature_extractor.conv_layers.0.2.bias")
    w.feat_ln_w = ptr(P + "layer_norm.weight")
    w.feat_ln_b = ptr(P + "layer_norm.bias")
    w.proj_w = ptr(P + "post_extract_proj.weight")
    w.proj_b = ptr(P + "post_extract_proj.bias")
    w.pos_v = ptr(P + "encoder.pos_conv.0.weight_v")
    w.pos_g = ptr(P + "encoder.pos_conv.0.weight_g")
    w.pos_b = ptr(P + "encoder.pos_conv.0.bias")
    w.enc_ln_w = ptr(P + "encoder.layer_norm.weight")
    w.enc_ln_b = ptr(P + "encoder.layer_norm.bias")
    for l in range(_lib.NUM_LAYERS):
        q = P + f"encoder.layers.{l}."
        lw = w.layers[l]
        for short, name in (("q", "self_attn.q_proj"), ("k", "self_attn.k_proj"), ("v", "self_attn.v_proj"),
                            ("o", "self_attn.out_proj"), ("ln1", "self_attn_layer_norm"), ("fc1", "fc1"),
                            ("fc2", "fc2"), ("ln2", "final_layer_norm")):
            setattr(lw, short + "_w", ptr(q + name + ".weight"))
            setattr(lw, short + "_b", ptr(q + name + ".bias"))
    w.emb_w = ptr("embedding_layer.1.weight")
    w.emb_b = ptr("embedding_layer.1.bias")
    return w, keep


class _AsyncFetch:
    """Device tensor -> pinned host copy enqueued behind the work that produces it; ``result()`` waits for THAT copy
    only (an event), not for whatever has been enqueued on the stream since."""

    def __init__(self, dev: torch.Tensor):
        self.host = torch.empty(dev.shape, dtype=dev.dtype, pin_memory=True)
        self.host.copy_(dev, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(dev.device))

    def result(self):
        self.event.synchronize()
        return self.host.numpy()


class Engine:
    """One engine per (process, GPU).  Not thread-safe; asynchronous on torch's current stream."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device: int = 0, diag=None):
        """diag=True: run on libnomad_diag.so (same path + the experimental kernel instantiations the measurement tools and
        the kernel tests select by tile id); None: ``NOMAD_DIAG_LIB=1`` decides; the product never passes it."""
        self.lib = _lib.load(diag)
        check_state_dict(state_dict)
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        w, keep = _weights_struct(state_dict)
        handle = C.c_void_p()
        _lib.check(self.lib.nomad_create(C.byref(handle), self.device_index, C.byref(w)), "nomad_create")
        del keep
        self.ctx = handle
        self._state_dict = state_dict     # host copy: nomad_train_enable re-reads it for the master parameters
        self._train_segments = None
        self._ws: Optional[torch.Tensor] = None
        self._ws_side: Dict[int, torch.Tensor] = {}     # further workspaces for concurrent forwards on side streams
        self._side_streams: Dict[int, "torch.cuda.Stream"] = {}
        self._l1_scratch: Optional[torch.Tensor] = None
        self._l1w_scratch: Optional[torch.Tensor] = None
        self._cdist_scratch: Optional[torch.Tensor] = None   # cdist_backward's W, grown on demand
        # A library built WITH packed-FP32 instructions (NOMAD_PACKED_FP32=1 / the _pk A/B variants) must not run two of its
        # forwards concurrently: v_pk_fma_f32 can lose a product next to the other forward's bf16 128 x 128 GEMM (DESIGN.md
        # "The packed-FP32 hazard").  The shipped build reports 0 here; with the bit set every two-stream batch split is off.
        self.build_flags = int(self.lib.nomad_build_flags())
        self.stochastic = self.stochastic_branches = False   # train_set_stochastic / train_set_branches: dropout or LayerDrop is on
        if self.build_flags & 1:
            import warnings
            warnings.warn("nomad_amd: this library was built with packed-FP32 instructions; the two-stream batch splits are switched "
                          "off (results of concurrent forwards would not be reproducible)", RuntimeWarning, stacklevel=2)
            self.F32_SPLIT_ROWS = self.BF16_SPLIT_ROWS = self.X3_SPLIT_ROWS = 0

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.nomad_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers -----------------------------------------------------------------------------
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _size(self, fn, B, n_samples, what):
        n = C.c_size_t()
        _lib.check(fn(self.ctx, B, n_samples, C.byref(n)), what)
        return n.value

    def _size_ragged(self, fn, lens, what):
        n = C.c_size_t()
        _lib.check(fn(self.ctx, len(lens), (C.c_int * len(lens))(*lens), C.byref(n)), what)
        return n.value

    def _forward_size(self, precision: str, B: int, n_samples: int) -> int:
        """Workspace bytes of the forward of ``precision`` over B clips of n_samples."""
        name = "nomad_workspace_bytes" + _SUFFIX[precision]
        return self._size(getattr(self.lib, name), B, n_samples, name)

    def _forward_size_ragged(self, precision: str, lens) -> int:
        name = "nomad_workspace_bytes_ragged" + _SUFFIX[precision]
        return self._size_ragged(getattr(self.lib, name), lens, name)

    def workspace_bytes(self, B: int, n_samples: int) -> int:
        return self._forward_size("fp32", B, n_samples)

    def _workspace(self, nbytes: int, side=False) -> torch.Tensor:
        """side: False / 0 = the main workspace, True / k >= 1 = the workspace of side stream k."""
        k = int(side)
        if k:
            ws = self._ws_side.get(k)
            if ws is None or ws.numel() < nbytes:
                self._ws_side.pop(k, None)
                ws = self._ws_side[k] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        else:
            if self._ws is None or self._ws.numel() < nbytes:
                self._ws = None
                self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            ws = self._ws
        if ws.is_cuda:
            # the caller's stream may differ from the one the block was allocated on: when the block is replaced by a larger one
            # the caching allocator must not hand it out again before this stream's kernels are done with it
            ws.record_stream(torch.cuda.current_stream(self.device))
        return ws

    def side_stream(self, k: int = 1) -> "torch.cuda.Stream":
        if k not in self._side_streams:
            self._side_streams[k] = torch.cuda.Stream(device=self.device)
        return self._side_streams[k]

    def _check_dev(self, t: torch.Tensor, name: str):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous fp32 tensor on {self.device}")

    def _check_wav(self, wav: torch.Tensor):
        """Equal-length waveforms (B,N) or (B,1,N) -> ((B,N) tensor, B, N, frames per clip)."""
        if wav.dim() == 3:
            wav = wav.squeeze(1)
        self._check_dev(wav, "wav")
        B, N = wav.shape
        T = num_frames(N)
        if T < 1:
            raise ValueError(f"clip of {N} samples is shorter than the conv stack's receptive field")
        return wav, B, N, T

    def _check_head(self, head):
        hw, hb = head if head is not None else (None, None)
        for t, name in ((hw, "head weight"), (hb, "head bias")):
            if t is not None:
                self._check_dev(t, name)
        return hw, hb

    def enable(self, precision: str) -> int:
        """Have the context allocate what the forward of ``precision`` needs ("fp32": nothing) -> the precision's code in the C ABI."""
        if precision not in _lib.PRECISION:
            raise ValueError("precision must be 'fp32', 'bf16x3' or 'bf16'")
        if precision != "fp32":
            _lib.check(getattr(self.lib, "nomad_enable_" + precision)(self.ctx), "nomad_enable_" + precision)
        return _lib.PRECISION[precision]

    # ---- two-stream batch splits -------------------------------------------------------------------------------------------------
    # A scoring batch with at least *_SPLIT_ROWS frames (rows of the encoder GEMMs) runs as two parts on two streams, each with
    # its own workspace: one part's kernels fill the CUs that the partial last round of the other's tiles leaves idle.  Every
    # GEMM instantiation contracts k in the same order and a clip's bits do not depend on the batch it is in, so the split
    # changes no result (tests/test_gpu_race_screen.py holds every precision to bit-identical results with the split on).
    # Equal-length batches are cut at B // 2, ragged ones where half of the audio is reached; two parts and equal halves are
    # what the measurements left (profiles/r01_f32_two_streams.txt, profiles/r02_c5_split_and_threshold_ab.txt).  The three
    # thresholds are read from the instance at call time: bench.py zeroes them for its per-kernel (roofline) pass, where kernels
    # have to run alone, and the constructor does for a packed-FP32 build.  NOMAD_*_SPLIT_ROWS override; 0 disables.
    #
    # fp32: +7.6 % at 32 clips of 4 s, +4 % at 64, +5 % at 128 (profiles/r01_f32_two_streams.txt), +0.7 % at 256 (the bench
    # workload, 50 944 frames: 2253-2260 vs 2238-2245 clips/s alternating in one run).
    F32_SPLIT_ROWS = int(os.environ.get("NOMAD_F32_SPLIT_ROWS", 4000))
    # bf16 (long-form clips, config C5): every GEMM of the path runs one 256 x 256 workgroup per CU, so the partial last round of
    # one half's tiles (the N = 768 GEMMs of 32 clips x 30 s are 2.2 rounds) and its per-tile prologue / epilogue are filled by
    # the other half's kernels.  (Round 2 switched this off because embed_bf16 then differed run to run in ~1 % of the calls.
    # Round 3 found the cause - not the split: v_pk_fma_f32 in conv0 lost products while the other half's 128 x 128 bf16 GEMM
    # shared its SIMD, DESIGN.md "The packed-FP32 hazard" - and the library is now built without packed-FP32 instructions.)
    BF16_SPLIT_ROWS = int(os.environ.get("NOMAD_BF16_SPLIT_ROWS", 4000))
    # bf16x3: one 256 x 256 workgroup per CU as well; e.g. the N = 768 GEMMs of a 256-clip batch are 2.33 rounds of the 256 CUs
    # and the other half's kernels fill the idle third round: +4 % at 256 clips of 4 s, +14 % at 128, break-even at 16
    # (profiles/r01_bf16x3_two_streams.txt).
    X3_SPLIT_ROWS = int(os.environ.get("NOMAD_X3_SPLIT_ROWS", 4000))

    def _split_rows(self, precision: str) -> int:
        return {"fp32": self.F32_SPLIT_ROWS, "bf16": self.BF16_SPLIT_ROWS, "bf16x3": self.X3_SPLIT_ROWS}[precision]

    def _splits(self, precision: str, B: int, rows: int) -> bool:
        threshold = self._split_rows(precision)
        return B >= 2 and bool(threshold) and rows >= threshold

    @staticmethod
    def _audio_cut(lens) -> int:
        """Where a ragged batch of at least two clips is cut: behind the clip in which half of the audio is reached, never behind
        the last one."""
        acc = 0
        for i, n in enumerate(lens[:-1]):
            acc += n
            if 2 * acc >= sum(lens):
                return i + 1
        return len(lens) - 1

    def _dispatch(self, B: int, cut: int, run, hint: bool = False):
        """``run(lo, hi, side)`` over clips 0 .. B-1: in one call (cut 0), or clips cut .. B-1 on the side stream with the side
        workspace and clips 0 .. cut-1 on the current stream, which then waits for the side stream.  hint: tell the library how
        many parts run concurrently (``nomad_set_concurrent_parts``: it selects tile shapes, results never depend on it).  Which
        entry points announce their parts is historical - DESIGN.md, "Known wart: the concurrent-parts hint"."""
        if hint:
            self.lib.nomad_set_concurrent_parts(self.ctx, 2 if cut else 1)
        if not cut:
            run(0, B, False)
            return
        cur, ss = torch.cuda.current_stream(self.device), self.side_stream()
        ss.wait_stream(cur)                        # the waveform (and anything queued before) is ready
        with torch.cuda.stream(ss):                # _workspace records the side workspace on the stream current inside run
            run(cut, B, True)
        run(0, cut, False)
        cur.wait_stream(ss)

    # ---- hot path ------------------------------------------------------------------------------
    def embed(self, wav: torch.Tensor, head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
              want_layers: bool = False, side: bool = False):
        """wav (B,N) or (B,1,N) fp32 on the GPU -> emb (B,256) [, layers (12,B,T,768)].
        side=True uses a second workspace so the call may run concurrently with another forward on a
        different stream (the launch stream is always torch's current stream)."""
        wav, B, N, T = self._check_wav(wav)
        emb = torch.empty(B, 256, dtype=torch.float32, device=self.device)
        layers = torch.empty(12, B, T, 768, dtype=torch.float32, device=self.device) if want_layers else None
        hw, hb = self._check_head(head)

        def run(lo, hi, use_side):
            ws = self._workspace(self.workspace_bytes(hi - lo, N), use_side)
            _lib.check(self.lib.nomad_embed(self.ctx, wav[lo:hi].data_ptr(), hi - lo, N, _ptr(hw), _ptr(hb), emb[lo:hi].data_ptr(),
                                            _ptr(layers), ws.data_ptr(), ws.numel(), self._stream()), "nomad_embed")

        if side:
            run(0, B, side)   # the caller's own concurrency: its stream, the side workspace it names, no split
        else:
            self._dispatch(B, B // 2 if not want_layers and self._splits("fp32", B, B * T) else 0, run, hint=True)
        return (emb, layers) if want_layers else emb

    def fetch_async(self, dev: torch.Tensor) -> _AsyncFetch:
        """Start copying a result to the host; ``.result()`` (numpy) later waits for this copy alone."""
        return _AsyncFetch(dev)

    def pack_ragged_host(self, waves):
        """Host-side half of ``embed_ragged`` for host inputs: clips -> ONE pinned (B, stride) fp32 staging tensor
        (rows are only read up to their length: no zero fill) + lengths.  Touches no GPU state, so a worker thread
        can build the next batch's staging buffer while the GPU runs the current one (``Nomad.get_embeddings_csv``)."""
        flat = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in waves]
        lens = [int(w.numel()) for w in flat]
        stride = (max(lens) + 3) // 4 * 4
        host = torch.empty(len(flat), stride, dtype=torch.float32, pin_memory=True)
        for i, w in enumerate(flat):
            host[i, :lens[i]] = w
        return host, lens

    def _pack(self, waves, packed=None):
        """Clips -> (device (B, stride) fp32 buffer, lengths), stride a multiple of 4.  Rows are only read up to their length, so the
        buffer needs no zero fill; device clips are packed on the device, host clips in one pinned staging buffer
        (``pack_ragged_host``; packed: its result, made ahead) and ONE asynchronous copy."""
        if packed is None:
            flat = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in waves]
            if all(w.is_cuda for w in flat):
                lens = [int(w.numel()) for w in flat]
                buf = torch.empty(len(flat), (max(lens) + 3) // 4 * 4, dtype=torch.float32, device=self.device)
                for i, w in enumerate(flat):
                    buf[i, :lens[i]] = w
                return buf, lens
            packed = self.pack_ragged_host(flat)
        host, lens = packed
        return host.to(self.device, non_blocking=True), lens

    def _forward_ragged(self, waves, packed, precision: str, width: int, launch) -> torch.Tensor:
        """The ragged forwards: pack, then ``launch(source, clips, stride, lengths array, destination, workspace)`` over the whole
        batch or, where that pays, over two halves by audio length on two streams, each with its own length array and workspace
        size -> the (B, width) result."""
        buf, lens = self._pack(waves, packed)
        B, stride = buf.shape
        out = torch.empty(B, width, dtype=torch.float32, device=self.device)

        def run(lo, hi, side):
            ws = self._workspace(self._forward_size_ragged(precision, lens[lo:hi]), side)
            launch(buf[lo:hi].data_ptr(), hi - lo, stride, (C.c_int * (hi - lo))(*lens[lo:hi]), out[lo:hi].data_ptr(), ws)

        split = self._splits(precision, B, sum(num_frames(n) for n in lens))
        self._dispatch(B, self._audio_cut(lens) if split else 0, run)
        return out

    def embed_ragged(self, waves, head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, bf16: bool = False,
                     precision: Optional[str] = None, packed: Optional[Tuple[torch.Tensor, list]] = None) -> torch.Tensor:
        """Embed clips of different lengths in ONE launch sequence (no padding in the arithmetic).

        waves: list of 1-D (or (1,N)) fp32 tensors / numpy arrays (host or device).  Returns (B,256) fp32 on the
        GPU, bit-identical to embedding every clip on its own.  precision: "fp32" (default), "bf16x3" (fp32-class
        scores from split bf16 operands) or "bf16" (also bf16=True); the last two take no head override.
        packed: instead of ``waves``, the (staging tensor, lengths) pair ``pack_ragged_host`` made."""
        precision = precision or ("bf16" if bf16 else "fp32")
        if precision not in ("fp32", "bf16", "bf16x3"):
            raise ValueError("precision must be 'fp32', 'bf16x3' or 'bf16'")
        if precision != "fp32" and head is not None:
            raise ValueError(f"the {precision} path has no head override")
        hw, hb = head if head is not None else (None, None)
        self.enable(precision)

        def launch(src, n, stride, arr, dst, ws):
            if precision == "fp32":
                _lib.check(self.lib.nomad_embed_ragged(self.ctx, src, n, stride, arr, _ptr(hw), _ptr(hb), dst, ws.data_ptr(), ws.numel(),
                                                       self._stream()), "nomad_embed_ragged")
                return
            fwd = self.lib.nomad_embed_ragged_bf16 if precision == "bf16" else self.lib.nomad_embed_ragged_bf16x3
            _lib.check(fwd(self.ctx, src, n, stride, arr, dst, ws.data_ptr(), ws.numel(), self._stream()), f"nomad_embed_ragged_{precision}")

        return self._forward_ragged(waves, packed, precision, 256, launch)

    # ---- pooled backbone features (the raw wav2vec 2.0 baseline, Origw2v) ----------------------------------------------
    def embed_features(self, wav: torch.Tensor, precision: str = "fp32") -> torch.Tensor:
        """wav (B,N) or (B,1,N) fp32 on the GPU -> (B,768) fp32: the backbone's output averaged over time
        (``Origw2v.forward``), by the forward of ``precision``.  Batches split over two streams by the rule of that
        precision's ``embed*``; a clip's values do not depend on the batch it is in, so the split changes no bit."""
        wav, B, N, T = self._check_wav(wav)
        prec = self.enable(precision)
        feat = torch.empty(B, 768, dtype=torch.float32, device=self.device)

        def run(lo, hi, side):
            ws = self._workspace(self._forward_size(precision, hi - lo, N), side)
            _lib.check(self.lib.nomad_embed_features(self.ctx, wav[lo:hi].data_ptr(), hi - lo, N, prec, feat[lo:hi].data_ptr(),
                                                     ws.data_ptr(), ws.numel(), self._stream()), "nomad_embed_features")

        self._dispatch(B, B // 2 if self._splits(precision, B, B * T) else 0, run, hint=True)
        return feat

    def embed_features_ragged(self, waves=None, precision: str = "fp32",
                              packed: Optional[Tuple[torch.Tensor, list]] = None) -> torch.Tensor:
        """``embed_features`` for clips of different lengths in ONE launch sequence: (B,768) fp32, bit-identical to one
        ``embed_features`` call per clip.  waves / packed, the staging and the two-stream split: as in ``embed_ragged``."""
        prec = self.enable(precision)

        def launch(src, n, stride, arr, dst, ws):
            _lib.check(self.lib.nomad_embed_features_ragged(self.ctx, src, n, stride, arr, prec, dst, ws.data_ptr(), ws.numel(),
                                                            self._stream()), "nomad_embed_features_ragged")

        return self._forward_ragged(waves, packed, precision, 768, launch)

    # ---- embeddings over windows of frames (scores over time) ------------------------------------------------------------
    def _check_windows(self, win, hop, precision: str, head):
        """Checked window geometry (frames), precision code and head override of ``embed_windows*`` -> (win, hop, code, hw, hb)."""
        win, hop = int(win), int(hop)
        if win < 1 or hop < 1:
            raise ValueError(f"win and hop must be at least 1 frame, got win={win}, hop={hop}")
        if precision not in _lib.PRECISION:
            raise ValueError("precision must be 'fp32', 'bf16x3' or 'bf16'")
        if precision != "fp32" and head is not None:
            raise ValueError(f"the {precision} path has no head override")
        hw, hb = self._check_head(head)
        return win, hop, self.enable(precision), hw, hb

    def embed_windows(self, wav: torch.Tensor, win: int, hop: int, precision: str = "fp32",
                      head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """wav (B,N) or (B,1,N) fp32 on the GPU -> (emb (W_total,256) fp32, counts): ONE forward of ``precision``, then the head
        over windows of ``win`` encoder frames every ``hop`` frames (``weights.num_windows``; one frame = 320 samples) instead
        of over the whole clip.  Rows: clip 0's windows in order, then clip 1's, ...; counts[c] = windows of clip c.  A window
        that covers a whole clip has the bits of that clip's ``embed*``; the encoder saw the whole clip, so a window is not the
        embedding of the excerpt alone.  Split over two streams by the rule of ``embed``; head: fp32 only."""
        win, hop, prec, hw, hb = self._check_windows(win, hop, precision, head)
        wav, B, N, T = self._check_wav(wav)
        W = num_windows(T, win, hop)
        emb = torch.empty(B * W, 256, dtype=torch.float32, device=self.device)

        def run(lo, hi, side):
            ws = self._workspace(self._forward_size(precision, hi - lo, N), side)
            _lib.check(self.lib.nomad_embed_windows(self.ctx, wav[lo:hi].data_ptr(), hi - lo, N, prec, win, hop, _ptr(hw), _ptr(hb),
                                                    emb[lo * W:hi * W].data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                       "nomad_embed_windows")

        self._dispatch(B, B // 2 if self._splits(precision, B, B * T) else 0, run, hint=True)
        return emb, [W] * B

    def embed_windows_ragged(self, waves=None, win: int = 0, hop: int = 0, precision: str = "fp32",
                             packed: Optional[Tuple[torch.Tensor, list]] = None,
                             head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """``embed_windows`` for clips of different lengths in ONE launch sequence -> (emb (W_total,256), counts); a clip's
        windows are bit-identical to those of its own call.  waves / packed, the staging and the two-stream split: as in
        ``embed_ragged``; a part [lo, hi) of the batch writes the rows of its own clips' windows."""
        win, hop, prec, hw, hb = self._check_windows(win, hop, precision, head)
        buf, lens = self._pack(waves, packed)
        B, stride = buf.shape
        frames = [num_frames(n) for n in lens]
        if min(frames) < 1:
            raise ValueError(f"a clip of {min(lens)} samples is shorter than the conv stack's receptive field")
        counts = [num_windows(t, win, hop) for t in frames]
        wpref = [0]
        for w in counts:
            wpref.append(wpref[-1] + w)
        emb = torch.empty(wpref[-1], 256, dtype=torch.float32, device=self.device)

        def run(lo, hi, side):
            ws = self._workspace(self._forward_size_ragged(precision, lens[lo:hi]), side)
            _lib.check(self.lib.nomad_embed_windows_ragged(self.ctx, buf[lo:hi].data_ptr(), hi - lo, stride,
                                                           (C.c_int * (hi - lo))(*lens[lo:hi]), prec, win, hop, _ptr(hw), _ptr(hb),
                                                           emb[wpref[lo]:wpref[hi]].data_ptr(), ws.data_ptr(), ws.numel(),
                                                           self._stream()), "nomad_embed_windows_ragged")

        self._dispatch(B, self._audio_cut(lens) if self._splits(precision, B, sum(frames)) else 0, run)
        return emb, counts

    # ---- embeddings over caller-given spans of frames (speech-only and per-turn scores) ------------------------------------------
    @staticmethod
    def _check_table(table, frames):
        """A span table ``(row_clip, row_ptr, spans)`` - the clip of each row (not decreasing), row r's span range
        ``row_ptr[r]:row_ptr[r + 1]`` and the ``(t0, t1)`` frame pairs - checked against the clips' frame counts -> the three as
        lists of ints.  The library checks the same again: these messages come before anything is packed or enabled."""
        row_clip, row_ptr, spans = table
        row_clip, row_ptr = [int(c) for c in row_clip], [int(p) for p in row_ptr]
        spans = [(int(a), int(b)) for a, b in spans]
        R = len(row_clip)
        if R < 1:
            raise ValueError("a span table needs at least one row")
        if len(row_ptr) != R + 1 or row_ptr[0] != 0 or row_ptr[-1] != len(spans):
            raise ValueError(f"row_ptr must hold {R + 1} entries from 0 to the number of spans ({len(spans)})")
        for r, c in enumerate(row_clip):
            if not 0 <= c < len(frames):
                raise ValueError(f"row {r} names clip {c}, outside [0, {len(frames)})")
            if r and c < row_clip[r - 1]:
                raise ValueError(f"row {r} names clip {c} behind row {r - 1}'s clip {row_clip[r - 1]}: the rows of a clip are contiguous")
            if row_ptr[r + 1] <= row_ptr[r]:
                raise ValueError(f"row {r} has no span")
            for k, (t0, t1) in enumerate(spans[row_ptr[r]:row_ptr[r + 1]]):
                if t0 < 0 or t1 > frames[c] or t0 >= t1:
                    raise ValueError(f"row {r}, span {k} is [{t0}, {t1}): not inside clip {c}'s {frames[c]} frames")
                if k and t0 < spans[row_ptr[r] + k - 1][1]:
                    raise ValueError(f"row {r}, span {k} [{t0}, {t1}) overlaps or precedes span {k - 1}")
        return row_clip, row_ptr, spans

    @staticmethod
    def _table_part(table, lo: int, hi: int):
        """The rows of clips lo .. hi - 1 as a table of their own (clips renumbered from 0) -> (first row, table or None)."""
        row_clip, row_ptr, spans = table
        rows = [r for r, c in enumerate(row_clip) if lo <= c < hi]
        if not rows:
            return 0, None
        r0, r1 = rows[0], rows[-1] + 1
        s0 = row_ptr[r0]
        return r0, ([c - lo for c in row_clip[r0:r1]], [p - s0 for p in row_ptr[r0:r1 + 1]], spans[s0:row_ptr[r1]])

    @staticmethod
    def _table_args(table):
        """The table as the C ABI takes it: R, row_clip, row_ptr, spans (host arrays that may die on return)."""
        row_clip, row_ptr, spans = table
        flat = [t for s in spans for t in s]
        return len(row_clip), (C.c_int * len(row_clip))(*row_clip), (C.c_int * len(row_ptr))(*row_ptr), (C.c_int * len(flat))(*flat)

    def _spans_scratch(self, B: int, table, backward: bool) -> torch.Tensor:
        """The span calls' scratch - the table's device copy, plus the per-row gradient rows of the backward: a fresh block per
        call, like the outputs."""
        n = C.c_size_t()
        _lib.check(self.lib.nomad_spans_scratch_bytes(B, len(table[0]), len(table[2]), int(backward), C.byref(n)), "nomad_spans_scratch_bytes")
        return torch.empty(n.value, dtype=torch.uint8, device=self.device)

    def embed_spans_ragged(self, waves=None, table=None, precision: str = "fp32",
                           head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                           packed: Optional[Tuple[torch.Tensor, list]] = None) -> torch.Tensor:
        """Clips of different lengths in ONE launch sequence -> emb (R,256) fp32: ONE forward of ``precision``, then the head over
        the R rows of ``table = (row_clip, row_ptr, spans)`` (``_check_table``) instead of over whole clips.  A row is an ordered
        list of spans ``[t0, t1)`` of encoder frames of one clip (one frame = 320 samples), ascending and not overlapping; its
        embedding is the plain head applied to the concatenation of its spans' frames as if they were a clip of their own (time
        mean over all of them, ReLU, Linear, L2 norm).  The encoder saw the whole clip, so a row is not the embedding of the
        excerpt alone.  A row of one span has the bits of ``embed_windows*``' window over those frames, a row that covers the
        whole clip the bits of ``embed_ragged``, and a clip's rows do not depend on the batch.  waves / packed, the staging and
        the two-stream split: as in ``embed_ragged`` (a part without a row is not run); head: fp32 only."""
        if precision not in _lib.PRECISION:
            raise ValueError("precision must be 'fp32', 'bf16x3' or 'bf16'")
        if precision != "fp32" and head is not None:
            raise ValueError(f"the {precision} path has no head override")
        hw, hb = self._check_head(head)
        buf, lens = self._pack(waves, packed)
        B, stride = buf.shape
        frames = [num_frames(n) for n in lens]
        if min(frames) < 1:
            raise ValueError(f"a clip of {min(lens)} samples is shorter than the conv stack's receptive field")
        table = self._check_table(table, frames)
        prec = self.enable(precision)
        emb = torch.empty(len(table[0]), 256, dtype=torch.float32, device=self.device)

        def run(lo, hi, side):
            r0, part = self._table_part(table, lo, hi)
            if part is None:
                return
            R, row_clip, row_ptr, spans = self._table_args(part)
            ws = self._workspace(self._forward_size_ragged(precision, lens[lo:hi]), side)
            scratch = self._spans_scratch(hi - lo, part, False)
            _lib.check(self.lib.nomad_embed_spans_ragged(self.ctx, buf[lo:hi].data_ptr(), hi - lo, stride,
                                                         (C.c_int * (hi - lo))(*lens[lo:hi]), prec, R, row_clip, row_ptr, spans,
                                                         _ptr(hw), _ptr(hb), emb[r0:r0 + R].data_ptr(), scratch.data_ptr(),
                                                         scratch.numel(), ws.data_ptr(), ws.numel(), self._stream()),
                       "nomad_embed_spans_ragged")

        self._dispatch(B, self._audio_cut(lens) if self._splits(precision, B, sum(frames)) else 0, run)
        return emb

    def frame_energy(self, waves=None, packed: Optional[Tuple[torch.Tensor, list]] = None):
        """Mean square of the 400 samples every encoder frame sees -> float64 (sum of the clips' frames,) on the GPU: clip 0's
        ``num_frames`` values, then clip 1's, ...  Every product and sum is in float64 in a fixed order; a frame's value depends on its own
        samples only.  waves / packed: as in ``embed_ragged``."""
        buf, lens = self._pack(waves, packed)
        B, stride = buf.shape
        frames = [num_frames(n) for n in lens]
        if min(frames) < 1:
            raise ValueError(f"a clip of {min(lens)} samples is shorter than the conv stack's receptive field")
        e = torch.empty(sum(frames), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.nomad_frame_energy(self.ctx, buf.data_ptr(), B, stride, (C.c_int * B)(*lens), e.data_ptr(), self._stream()),
                   "nomad_frame_energy")
        return e

    # ---- degradations on packed clips (nomad_degrade_noise / nomad_degrade_clip) ------------------------------------------------
    def _degrade(self, waves, lengths, levels, what: str):
        """The shared front of the two degradations: pack, check the levels -> (buffer, lengths, level array, G, output, workspace)."""
        if lengths is not None:
            buf, lens = self.pack_ragged(waves, lengths)
            if buf.shape[1] % 4:     # a padded tensor whose row stride is no multiple of 4: through the packer after all
                buf, lens = self._pack([buf[i, :n] for i, n in enumerate(lens)])
        else:
            buf, lens = self._pack(waves)
        levels = [float(v) for v in (levels.tolist() if hasattr(levels, "tolist") else levels)]
        G = len(levels)
        if not 1 <= G <= 64:
            raise ValueError(f"{what} takes 1 .. 64 levels per call, got {G}")
        B, stride = buf.shape
        out = torch.empty(B * G, stride, dtype=torch.float32, device=self.device)
        ws = self._workspace(int(self.lib.nomad_degrade_scratch_bytes(B, stride, G)))
        return buf, lens, (C.c_double * G)(*levels), G, out, ws

    def degrade_noise(self, waves, noise, snr_db, lengths=None):
        """Additive noise at G target SNRs: waves as ``pack_ragged`` takes them (a list of clips, or a padded device tensor plus
        ``lengths``), noise a 1-D signal (tiled or cut to each clip's length), snr_db G levels in dB -> (out (B G, stride) fp32 on the
        device, lengths repeated G times, alpha (B, G) float64): row b G + g is clip b at snr_db[g], zero behind its length, and
        ``(out, lengths)`` is what ``embed_ragged`` / ``embed_windows_ragged`` take as ``packed=`` without another copy.  The
        formula, the reference's own, is stated in include/nomad_hip.h (``nomad_degrade_noise``)."""
        noise = torch.as_tensor(noise, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
        if noise.numel() < 1:
            raise ValueError("the noise signal is empty")
        buf, lens, arr, G, out, ws = self._degrade(waves, lengths, snr_db, "degrade_noise")
        B, stride = buf.shape
        alpha = torch.empty(B, G, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.nomad_degrade_noise(self.ctx, buf.data_ptr(), B, stride, (C.c_int * B)(*lens), noise.data_ptr(), noise.numel(),
                                                arr, G, out.data_ptr(), alpha.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                   "nomad_degrade_noise")
        return out, [n for n in lens for _ in range(G)], alpha

    def degrade_clip(self, waves, clip_factor, lengths=None):
        """Percentile clipping at G clip factors (percent of the samples clipped, 0 .. 100): -> (out (B G, stride) fp32 on the device,
        lengths repeated G times, thresholds (B, G, 2) float64 = (v_lo, v_hi)), rows and layout as ``degrade_noise``.  The thresholds
        are numpy's linear percentiles cf / 2 and 100 - cf / 2 of the clip's own samples, from exact order statistics
        (``nomad_degrade_clip``)."""
        buf, lens, arr, G, out, ws = self._degrade(waves, lengths, clip_factor, "degrade_clip")
        B, stride = buf.shape
        thr = torch.empty(B, G, 2, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.nomad_degrade_clip(self.ctx, buf.data_ptr(), B, stride, (C.c_int * B)(*lens), arr, G, out.data_ptr(),
                                               thr.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), "nomad_degrade_clip")
        return out, [n for n in lens for _ in range(G)], thr

    def pack_responses(self, irs, ir_lengths=None):
        """Impulse responses -> (device (G, ir_stride) fp32 buffer, tap counts): a list of 1-D responses (tensors or arrays), or a
        (G, L) tensor with optional ``ir_lengths``; packed on the host and uploaded once (taps behind a length are never read)."""
        if torch.is_tensor(irs) and irs.dim() == 2:
            lens = [int(n) for n in (ir_lengths.tolist() if torch.is_tensor(ir_lengths) else ir_lengths)] if ir_lengths is not None \
                else [int(irs.shape[1])] * int(irs.shape[0])
            if len(lens) != irs.shape[0] or any(n > irs.shape[1] for n in lens):
                raise ValueError("ir_lengths must hold one entry per row of the (G,L) responses, none above L")
            rows = [irs[g, :n] for g, n in enumerate(lens)]
        else:
            if ir_lengths is not None:
                raise ValueError("ir_lengths go with a (G,L) tensor: a list of responses has its own")
            rows = list(irs)
        flat = [torch.as_tensor(h, dtype=torch.float32).reshape(-1).detach().cpu() for h in rows]
        G = len(flat)
        if not 1 <= G <= 64:
            raise ValueError(f"degrade_convolve takes 1 .. 64 responses per call, got {G}")
        lens = [int(h.numel()) for h in flat]
        if min(lens) < 1 or max(lens) > 65536:
            raise ValueError(f"a response has {min(lens) if min(lens) < 1 else max(lens)} taps, 1 .. 65536 are supported")
        host = torch.zeros(G, (max(lens) + 3) // 4 * 4, dtype=torch.float32)
        for g, h in enumerate(flat):
            host[g, :lens[g]] = h
        return host.to(self.device), lens

    def degrade_convolve(self, waves, irs, lengths=None, ir_lengths=None):
        """Every clip convolved with each of G impulse responses (reverberation as a causal FIR filter, cut to the clip's length):
        waves as ``degrade_noise`` takes them, irs as ``pack_responses`` takes them (or its result, to reuse one upload) -> (out
        (B G, stride) fp32 on the device, lengths repeated G times): row b G + g is clip b through response g, zero behind its
        length, and ``(out, lengths)`` goes into ``embed_ragged(packed=...)`` without another copy.  fp32 products and sums on the
        matrix cores in an order that depends on the clip's and the response's length only (``nomad_degrade_convolve``)."""
        if lengths is not None:
            buf, lens = self.pack_ragged(waves, lengths)
            if buf.shape[1] % 4:     # a padded tensor whose row stride is no multiple of 4: through the packer after all
                buf, lens = self._pack([buf[i, :n] for i, n in enumerate(lens)])
        else:
            buf, lens = self._pack(waves)
        packed_ir = isinstance(irs, tuple) and len(irs) == 2 and torch.is_tensor(irs[0]) and irs[0].dim() == 2 and isinstance(irs[1], list)
        ir, ir_lens = irs if packed_ir else self.pack_responses(irs, ir_lengths)
        B, stride = buf.shape
        G = len(ir_lens)
        out = torch.empty(B * G, stride, dtype=torch.float32, device=self.device)
        ws = self._workspace(int(self.lib.nomad_degrade_convolve_scratch_bytes(B, G)))
        _lib.check(self.lib.nomad_degrade_convolve(self.ctx, buf.data_ptr(), B, stride, (C.c_int * B)(*lens), ir.data_ptr(), G,
                                                   ir.shape[1], (C.c_int * G)(*ir_lens), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   self._stream()), "nomad_degrade_convolve")
        return out, [n for n in lens for _ in range(G)]

    REVERB_RANGES = {"reverberance": (0.0, 100.0), "hf_damping": (0.0, 100.0), "room_scale": (0.0, 100.0), "stereo_depth": (0.0, 100.0),
                     "pre_delay_ms": (0.0, 500.0), "wet_gain_db": (-10.0, 10.0)}

    @staticmethod
    def check_reverb(reverberance, hf_damping=50, room_scale=100, stereo_depth=100, pre_delay_ms=0, wet_gain_db=0, wet_only=False,
                     clamp=True, sample_rate=16000):
        """The arguments of ``degrade_reverb`` that need no GPU -> the ``nomad_reverb_params`` struct the C ABI takes."""
        levels = [float(v) for v in (reverberance.tolist() if hasattr(reverberance, "tolist") else
                                     reverberance if isinstance(reverberance, (list, tuple)) else [reverberance])]
        if not 1 <= len(levels) <= 64:
            raise ValueError(f"degrade_reverb takes 1 .. 64 reverberance levels per call, got {len(levels)}")
        shared = dict(hf_damping=float(hf_damping), room_scale=float(room_scale), stereo_depth=float(stereo_depth),
                      pre_delay_ms=float(pre_delay_ms), wet_gain_db=float(wet_gain_db))
        for name, values in [("reverberance", levels)] + [(k, [v]) for k, v in shared.items()]:
            lo, hi = Engine.REVERB_RANGES[name]
            for v in values:
                if not (math.isfinite(v) and lo <= v <= hi):
                    raise ValueError(f"{name} must be finite and in {lo:g} .. {hi:g}, got {v}")
        sample_rate = int(sample_rate)
        if not 8000 <= sample_rate <= 48000:
            raise ValueError(f"sample_rate must be in 8000 .. 48000, got {sample_rate}")
        params = _lib.ReverbParams(G=len(levels), wet_only=int(bool(wet_only)), clamp=int(bool(clamp)), sample_rate=sample_rate, **shared)
        params.reverberance[:len(levels)] = levels
        return params

    def degrade_reverb(self, waves, reverberance, lengths=None, hf_damping=50, room_scale=100, stereo_depth=100, pre_delay_ms=0,
                       wet_gain_db=0, wet_only=False, clamp=True, sample_rate=16000):
        """Sox-style reverb (``sox ... reverb P``: Freeverb's eight combs and four all-passes per channel) at G reverberance levels,
        0 .. 100, the other parameters - sox's names, ranges and defaults - shared: waves as ``degrade_noise`` takes them -> (out
        (B G, stride) fp32 on the device, lengths repeated G times): row b G + g is clip b at reverberance[g], the two output
        channels averaged, cut to the clip's length and zero behind it; ``(out, lengths)`` goes into ``embed_ragged(packed=...)``
        without another copy.  The recurrences run in float64 with one rounding to fp32 (``nomad_degrade_reverb``; include/nomad_hip.h
        states the algorithm, which is restated from memory of sox 14.4 and has not been checked against the sox binary)."""
        params = self.check_reverb(reverberance, hf_damping, room_scale, stereo_depth, pre_delay_ms, wet_gain_db, wet_only, clamp, sample_rate)
        if lengths is not None:
            buf, lens = self.pack_ragged(waves, lengths)
            if buf.shape[1] % 4:     # a padded tensor whose row stride is no multiple of 4: through the packer after all
                buf, lens = self._pack([buf[i, :n] for i, n in enumerate(lens)])
        else:
            buf, lens = self._pack(waves)
        B, stride = buf.shape
        G = params.G
        out = torch.empty(B * G, stride, dtype=torch.float32, device=self.device)
        ws = self._workspace(int(self.lib.nomad_degrade_reverb_scratch_bytes(B, stride, G, params.sample_rate)))
        _lib.check(self.lib.nomad_degrade_reverb(self.ctx, buf.data_ptr(), B, stride, (C.c_int * B)(*lens), C.byref(params), out.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), self._stream()), "nomad_degrade_reverb")
        return out, [n for n in lens for _ in range(G)]

    @staticmethod
    def check_normalize(target, kind, peak_db, sample_rate):
        """The arguments of ``degrade_normalize`` that need no GPU -> (mode, target, peak_db as the C ABI takes them)."""
        if kind not in _lib.LOUDNESS_MODE:
            raise ValueError(f"kind must be 'ebu', 'rms' or 'peak', got {kind!r}")
        target = float(target)
        if not math.isfinite(target):
            raise ValueError(f"the target level must be finite, got {target}")
        peak = float("nan") if peak_db is None else float(peak_db)
        if peak_db is not None and not math.isfinite(peak):
            raise ValueError(f"peak_db must be finite or None, got {peak_db}")
        sample_rate = int(sample_rate)
        if not 8000 <= sample_rate <= 192000 or sample_rate % 10:
            raise ValueError(f"sample_rate must be a multiple of 10 in 8000 .. 192000, got {sample_rate}")
        return _lib.LOUDNESS_MODE[kind], target, peak, sample_rate

    def degrade_normalize(self, waves=None, lengths=None, packed: Optional[Tuple[torch.Tensor, list]] = None, target: float = -23.0,
                          kind: str = "ebu", peak_db: Optional[float] = None, sample_rate: int = 16000, inplace: bool = False,
                          measure_only: bool = False):
        """Loudness of every row and the linear gain that brings it to ``target`` -> (rows (R, stride) fp32 on the device or None,
        lengths, stats (R, 4) float64 on the device = level, sample peak, applied gain, blocks past both gates).  kind "ebu": the
        level is the BS.1770-4 integrated loudness in LUFS (K-weighting in float64, 400 ms blocks every 100 ms, the -70 LUFS and
        -10 LU gates); "rms" / "peak": dBFS - ffmpeg-normalize's three.  peak_db: a ceiling for the SAMPLE peak after the gain.  A
        row without a level (silence, under 400 ms for "ebu") is copied unchanged.  waves / lengths as ``degrade_noise`` takes
        them, or packed = (device buffer, lengths) as the degradations return it; inplace: write into that buffer (what feeds
        ``embed_ragged(packed=...)`` is then normalised with no copy); measure_only: statistics alone, rows None.  The linear gain of
        ffmpeg's loudnorm: no dynamic mode, loudness range or true-peak limiter (``nomad_degrade_normalize``)."""
        mode, target, peak, sample_rate = self.check_normalize(target, kind, peak_db, sample_rate)
        if packed is not None:
            if waves is not None or lengths is not None:
                raise ValueError("packed goes without waves and lengths")
            buf, lens = packed
            self._check_dev(buf, "packed rows")
            if buf.dim() != 2 or buf.dtype != torch.float32 or not buf.is_contiguous() or buf.shape[1] % 4 or len(lens) != buf.shape[0]:
                raise ValueError("packed must be a contiguous (R, stride) fp32 device buffer, stride a multiple of 4, with R lengths")
        elif lengths is not None:
            buf, lens = self.pack_ragged(waves, lengths)
            if buf.shape[1] % 4 or not buf.is_contiguous() or buf.dtype != torch.float32:
                buf, lens = self._pack([buf[i, :n] for i, n in enumerate(lens)])
        else:
            buf, lens = self._pack(waves)
        lens = [int(n) for n in lens]
        R, stride = buf.shape
        if measure_only and inplace:
            raise ValueError("measure_only writes no rows: it goes without inplace")
        out = None if measure_only else buf if inplace else torch.empty(R, stride, dtype=torch.float32, device=self.device)
        stats = torch.empty(R, 4, dtype=torch.float64, device=self.device)
        ws = self._workspace(int(self.lib.nomad_degrade_normalize_scratch_bytes(R, stride, sample_rate)))
        _lib.check(self.lib.nomad_degrade_normalize(self.ctx, buf.data_ptr(), R, stride, (C.c_int * R)(*lens), sample_rate, mode, target, peak,
                                                    _ptr(out), stats.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                   "nomad_degrade_normalize")
        return out, lens, stats

    def _scratch_size(self, fn, what, *args) -> int:
        """Bytes from a ``*_scratch_bytes`` helper that returns the size itself: 0 is its refusal, raised as ``_size`` raises one."""
        n = int(fn(*args))
        if n == 0:
            _lib.check(_lib.NOMAD_ERR_INVALID, what)
        return n

    def _rows(self, waves, lengths, packed):
        """``packed`` = (device (R, stride) fp32 buffer, lengths) as the degradations return it, used as it is; or waves / lengths
        as ``degrade_noise`` takes them -> (buffer, lengths)."""
        if packed is not None:
            if waves is not None or lengths is not None:
                raise ValueError("packed goes without waves and lengths")
            buf, lens = packed
            self._check_dev(buf, "packed rows")
            if buf.dim() != 2 or buf.shape[1] % 4 or len(lens) != buf.shape[0]:
                raise ValueError("packed must be a contiguous (R, stride) fp32 device buffer, stride a multiple of 4, with R lengths")
        elif lengths is not None:
            buf, lens = self.pack_ragged(waves, lengths)
            if buf.shape[1] % 4 or not buf.is_contiguous() or buf.dtype != torch.float32:
                buf, lens = self._pack([buf[i, :n] for i, n in enumerate(lens)])
        else:
            buf, lens = self._pack(waves)
        return buf, [int(n) for n in lens]

    NSIM_BANDS = 21

    @staticmethod
    def gammatone_frames(n_samples: int, sample_rate: int = 16000) -> int:
        """Whole 80 ms frames every 20 ms of a row of n_samples (``nomad_gammatone_frames``), 0 for a shorter row."""
        H = int(sample_rate) // 50
        return 0 if n_samples < 4 * H else (int(n_samples) - 4 * H) // H + 1

    @staticmethod
    def check_gammatone(sample_rate):
        sample_rate = int(sample_rate)
        if not 16000 <= sample_rate <= 48000 or sample_rate % 50:
            raise ValueError(f"sample_rate must be a multiple of 50 in 16000 .. 48000, got {sample_rate}")
        return sample_rate

    def gammatone(self, waves=None, lengths=None, packed: Optional[Tuple[torch.Tensor, list]] = None, sample_rate: int = 16000):
        """Gammatone spectrogram of every row: 21 ERB bands from 50 Hz to 8 kHz, 80 ms frames every 20 ms with the filter state
        reset per frame, float64 -> (spec (sum F_r, 21) float64 on the device, frames [F_r]): the rows' frames packed row after
        row, S[t][b] = the band's RMS over the frame.  waves / lengths as ``degrade_noise`` takes them, or packed = (device
        buffer, lengths) as the degradations return it (no copy).  Every row needs one whole frame.  Modelled on ViSQOL's
        speech mode from memory, not checked against it; include/nomad_hip.h states the measure (``nomad_gammatone``)."""
        sample_rate = self.check_gammatone(sample_rate)
        buf, lens = self._rows(waves, lengths, packed)
        R, stride = buf.shape
        frames = [self.gammatone_frames(n, sample_rate) for n in lens]
        if min(frames) < 1:
            raise ValueError(f"a row of {min(lens)} samples is shorter than one frame of {sample_rate // 50 * 4}")
        spec = torch.empty(sum(frames), self.NSIM_BANDS, dtype=torch.float64, device=self.device)
        ws = self._workspace(self._scratch_size(self.lib.nomad_gammatone_scratch_bytes, "nomad_gammatone_scratch_bytes", R, stride, sample_rate))
        _lib.check(self.lib.nomad_gammatone(self.ctx, buf.data_ptr(), R, stride, (C.c_int * R)(*lens), sample_rate, spec.data_ptr(),
                                            ws.data_ptr(), ws.numel(), self._stream()), "nomad_gammatone")
        return spec, frames

    def nsim_of_spectrograms(self, spec_ref: torch.Tensor, spec_deg: torch.Tensor, frames, G: int, intensity_range: float = 1.0,
                             want_bands: bool = True):
        """``nomad_nsim`` on spectrograms ``gammatone`` made: spec_ref (sum F_b, 21) of B clean clips, spec_deg (G sum F_b, 21) of
        their B G degraded rows (row b G + g belongs to clip b), frames [F_b] -> (nsim (B, G) float64, bands (B, G, 21) or None)."""
        frames = [int(f) for f in frames]
        B, G, total = len(frames), int(G), sum(frames)
        intensity_range = float(intensity_range)
        if not (math.isfinite(intensity_range) and intensity_range > 0.0):
            raise ValueError(f"intensity_range must be finite and positive, got {intensity_range}")
        for t, rows, name in ((spec_ref, total, "spec_ref"), (spec_deg, G * total, "spec_deg")):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
                    and tuple(t.shape) == (rows, self.NSIM_BANDS)):
                raise ValueError(f"{name} must be a contiguous float64 tensor of shape ({rows}, {self.NSIM_BANDS}) on {self.device}")
        nsim = torch.empty(B, G, dtype=torch.float64, device=self.device)
        bands = torch.empty(B, G, self.NSIM_BANDS, dtype=torch.float64, device=self.device) if want_bands else None
        ws = self._workspace(self._scratch_size(self.lib.nomad_nsim_scratch_bytes, "nomad_nsim_scratch_bytes", B, G, total))
        _lib.check(self.lib.nomad_nsim(self.ctx, spec_ref.data_ptr(), spec_deg.data_ptr(), B, G, (C.c_int * B)(*frames), intensity_range,
                                       nsim.data_ptr(), _ptr(bands), ws.data_ptr(), ws.numel(), self._stream()), "nomad_nsim")
        return nsim, bands

    def nsim(self, clean, degraded, G: int, intensity_range: float = 1.0, sample_rate: int = 16000, want_bands: bool = True):
        """NSIM of every degraded row with its clean clip -> (nsim (B, G) float64 on the device, bands (B, G, 21) or None): clean
        and degraded are (device buffer, lengths) pairs as ``degrade_normalize`` takes ``packed`` - B clean rows, and B G degraded
        rows of which row b G + g belongs to clip b and has its length, i.e. what any ``degrade_*`` call returns, without a copy.
        1 for identical rows, falling with the degradation; the clean spectrograms are computed once (``gammatone`` twice, then
        ``nomad_nsim``).  Not ViSQOL's number: include/nomad_hip.h states the measure."""
        cbuf, clens = self._rows(None, None, clean)
        dbuf, dlens = self._rows(None, None, degraded)
        G = int(G)
        if not 1 <= G <= 64:
            raise ValueError(f"nsim takes 1 .. 64 degraded rows per clean clip, got {G}")
        if dlens != [n for n in clens for _ in range(G)]:
            raise ValueError("degraded must hold G rows per clean clip, row b G + g with the length of clip b")
        spec_ref, frames = self.gammatone(packed=(cbuf, clens), sample_rate=sample_rate)
        spec_deg, _ = self.gammatone(packed=(dbuf, dlens), sample_rate=sample_rate)
        return self.nsim_of_spectrograms(spec_ref, spec_deg, frames, G, intensity_range, want_bands)

    @staticmethod
    def _groups(costs, fixed, what: str):
        """Consecutive groups [lo, hi) of items whose workspace ``fixed(count) + sum(costs)`` stays within
        ``NSIM_BACKWARD_WORKSPACE_BYTES``; an item that alone exceeds it raises."""
        cap, out, lo, acc = int(NSIM_BACKWARD_WORKSPACE_BYTES), [], 0, 0
        for i, c in enumerate(costs):
            if fixed(1) + c > cap:
                raise ValueError(f"{what} {i} alone needs a workspace of {fixed(1) + c} bytes, more than NSIM_BACKWARD_WORKSPACE_BYTES = {cap}")
            if i > lo and fixed(i - lo + 1) + acc + c > cap:
                out.append((lo, i))
                lo, acc = i, 0
            acc += c
        out.append((lo, len(costs)))
        return out

    def gammatone_backward(self, dspec: torch.Tensor, waves=None, lengths=None, packed: Optional[Tuple[torch.Tensor, list]] = None,
                           sample_rate: int = 16000):
        """The gradient of ``gammatone`` with respect to the samples: dspec (sum F_r, 21) float64, the gradient with respect to the
        spectrogram ``gammatone`` makes of these rows -> (R, stride) fp32 on the device, 0 behind every row's whole frames
        (``nomad_gammatone_backward``; include/nomad_hip.h, "NSIM as a loss", states the conventions).  The rows are processed in
        groups whose workspace - 168 W bytes per frame of a row as long as the stride - stays within
        ``NSIM_BACKWARD_WORKSPACE_BYTES``; rows are independent, so the grouping changes no bit."""
        sample_rate = self.check_gammatone(sample_rate)
        buf, lens = self._rows(waves, lengths, packed)
        self._check_dev(buf, "the rows")
        R, stride = buf.shape
        frames = [self.gammatone_frames(n, sample_rate) for n in lens]
        if min(frames) < 1:
            raise ValueError(f"a row of {min(lens)} samples is shorter than one frame of {sample_rate // 50 * 4}")
        if not (torch.is_tensor(dspec) and dspec.is_cuda and dspec.dtype == torch.float64 and dspec.is_contiguous()
                and tuple(dspec.shape) == (sum(frames), self.NSIM_BANDS)):
            raise ValueError(f"dspec must be a contiguous float64 tensor of shape ({sum(frames)}, {self.NSIM_BANDS}) on {self.device}")
        size = lambda k: self._scratch_size(self.lib.nomad_gammatone_backward_scratch_bytes, "nomad_gammatone_backward_scratch_bytes", k,
                                            stride, sample_rate)
        per_row = size(2) - size(1)
        dx = torch.empty(R, stride, dtype=torch.float32, device=self.device)
        at = 0
        for lo, hi in self._groups([per_row] * R, lambda k: size(k) - k * per_row, "row"):
            n = hi - lo
            ws = self._workspace(size(n))
            _lib.check(self.lib.nomad_gammatone_backward(self.ctx, buf[lo:hi].data_ptr(), n, stride, (C.c_int * n)(*lens[lo:hi]), sample_rate,
                                                         dspec[at:].data_ptr(), dx[lo:hi].data_ptr(), ws.data_ptr(), ws.numel(),
                                                         self._stream()), "nomad_gammatone_backward")
            at += sum(frames[lo:hi])
        return dx

    def nsim_backward(self, spec_ref: torch.Tensor, spec_deg: torch.Tensor, frames, G: int, grad_nsim: torch.Tensor,
                      intensity_range: float = 1.0):
        """The gradient of ``nsim_of_spectrograms`` with respect to spec_deg: grad_nsim (B, G) float64, the gradient with respect to
        the scores -> (G sum F_b, 21) float64, packed as spec_deg (``nomad_nsim_backward``; a row whose NSIM is NaN gets NaN).  The
        clips are processed in groups as ``gammatone_backward`` processes rows."""
        frames = [int(f) for f in frames]
        B, G, total = len(frames), int(G), sum(frames)
        intensity_range = float(intensity_range)
        if not (math.isfinite(intensity_range) and intensity_range > 0.0):
            raise ValueError(f"intensity_range must be finite and positive, got {intensity_range}")
        for t, shape, name in ((spec_ref, (total, self.NSIM_BANDS), "spec_ref"), (spec_deg, (G * total, self.NSIM_BANDS), "spec_deg"),
                               (grad_nsim, (B, G), "grad_nsim")):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError(f"{name} must be a contiguous float64 tensor of shape {shape} on {self.device}")
        size = lambda k, f: self._scratch_size(self.lib.nomad_nsim_backward_scratch_bytes, "nomad_nsim_backward_scratch_bytes", k, G, f)
        per_frame = size(1, 2) - size(1, 1)
        out = torch.empty(G * total, self.NSIM_BANDS, dtype=torch.float64, device=self.device)
        at = 0
        for lo, hi in self._groups([per_frame * f for f in frames], lambda k: size(k, k) - k * per_frame, "clip"):
            n, f = hi - lo, sum(frames[lo:hi])
            ws = self._workspace(size(n, f))
            _lib.check(self.lib.nomad_nsim_backward(self.ctx, spec_ref[at:].data_ptr(), spec_deg[G * at:].data_ptr(), n, G,
                                                    (C.c_int * n)(*frames[lo:hi]), intensity_range, grad_nsim[lo:hi].data_ptr(),
                                                    out[G * at:].data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), "nomad_nsim_backward")
            at += f
        return out

    NSIM_PATCH_MAX, NSIM_SEARCH_MAX = 64, 128

    @classmethod
    def check_patches(cls, patch, search, vad_ratio, min_active_frames):
        """The parameters of ``nsim_patches`` -> (patch, search, vad_ratio, min_active_frames) as the library takes them."""
        patch, search, vad_ratio, min_active_frames = int(patch), int(search), float(vad_ratio), int(min_active_frames)
        if not 1 <= patch <= cls.NSIM_PATCH_MAX:
            raise ValueError(f"patch must be 1 .. {cls.NSIM_PATCH_MAX} frames, got {patch}")
        if not 0 <= search <= cls.NSIM_SEARCH_MAX:
            raise ValueError(f"search must be 0 .. {cls.NSIM_SEARCH_MAX} frames, got {search}")
        if not 0.0 < vad_ratio <= 1.0:
            raise ValueError(f"vad_ratio must lie in (0, 1], got {vad_ratio}")
        if not 1 <= min_active_frames <= patch:
            raise ValueError(f"min_active_frames must be 1 .. patch = {patch}, got {min_active_frames}")
        return patch, search, vad_ratio, min_active_frames

    def nsim_patches_of_spectrograms(self, spec_ref: torch.Tensor, spec_deg: torch.Tensor, frames, deg_frames, G: int, patch: int,
                                     search: int, vad_ratio: float, min_active_frames: int, intensity_range: float = 1.0,
                                     want_bands: bool = True, want_cand: bool = False):
        """``nomad_nsim_patches`` on spectrograms ``gammatone`` made: spec_ref (sum F_b, 21) of B clean clips, spec_deg (sum Fd_r, 21)
        of their B G degraded rows, row b G + g belonging to clip b and having its OWN frame count deg_frames[b G + g] -> a dict of
        device tensors: nsim (B, G) float64, bands (B, G, 21) or None, offsets (B, G, P) int32 (the chosen place of every patch, -1
        where it is not kept), patch_nsim (B, G, P) (NaN where not kept), cand (B, G, P, 2 search + 1) or None; P = the patches of
        the longest clip, at least 1.  The clean clip's active patches (frame energy within vad_ratio of the clip's largest, at
        least min_active_frames per patch of ``patch`` frames) are each searched for within ``search`` frames of their own place,
        the places of a row never going back.  include/nomad_hip.h states the measure."""
        frames, deg_frames = [int(f) for f in frames], [int(f) for f in deg_frames]
        B, G = len(frames), int(G)
        patch, search, vad_ratio, min_active_frames = self.check_patches(patch, search, vad_ratio, min_active_frames)
        intensity_range = float(intensity_range)
        if not (math.isfinite(intensity_range) and intensity_range > 0.0):
            raise ValueError(f"intensity_range must be finite and positive, got {intensity_range}")
        if not 1 <= G <= 64 or len(deg_frames) != B * G or not frames:
            raise ValueError("deg_frames must hold G = 1 .. 64 entries per clean clip, row b G + g belonging to clip b")
        if min(frames) < 1 or min(deg_frames) < 1:
            raise ValueError("every clean clip and every degraded row needs at least one frame")
        total, dtotal = sum(frames), sum(deg_frames)
        for t, rows, name in ((spec_ref, total, "spec_ref"), (spec_deg, dtotal, "spec_deg")):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
                    and tuple(t.shape) == (rows, self.NSIM_BANDS)):
                raise ValueError(f"{name} must be a contiguous float64 tensor of shape ({rows}, {self.NSIM_BANDS}) on {self.device}")
        P = max(1, max(frames) // patch)
        nsim = torch.empty(B, G, dtype=torch.float64, device=self.device)
        bands = torch.empty(B, G, self.NSIM_BANDS, dtype=torch.float64, device=self.device) if want_bands else None
        offsets = torch.empty(B, G, P, dtype=torch.int32, device=self.device)
        patch_nsim = torch.empty(B, G, P, dtype=torch.float64, device=self.device)
        cand = torch.empty(B, G, P, 2 * search + 1, dtype=torch.float64, device=self.device) if want_cand else None
        ws = self._workspace(self._scratch_size(self.lib.nomad_nsim_patches_scratch_bytes, "nomad_nsim_patches_scratch_bytes", B, G, total,
                                                dtotal, patch, search))
        _lib.check(self.lib.nomad_nsim_patches(self.ctx, spec_ref.data_ptr(), spec_deg.data_ptr(), B, G, (C.c_int * B)(*frames),
                                               (C.c_int * (B * G))(*deg_frames), patch, search, vad_ratio, min_active_frames, intensity_range,
                                               P, nsim.data_ptr(), _ptr(bands), offsets.data_ptr(), patch_nsim.data_ptr(), _ptr(cand),
                                               ws.data_ptr(), ws.numel(), self._stream()), "nomad_nsim_patches")
        return {"nsim": nsim, "bands": bands, "offsets": offsets, "patch_nsim": patch_nsim, "cand": cand}

    def nsim_patches(self, clean, degraded, G: int, patch: int, search: int, vad_ratio: float, min_active_frames: int,
                     intensity_range: float = 1.0, sample_rate: int = 16000, want_bands: bool = True, want_cand: bool = False):
        """Patch-wise NSIM of every degraded row with its clean clip: clean and degraded are (device buffer, lengths) pairs as
        ``nsim`` takes them, but a degraded row may have any length of at least one frame (``gammatone`` twice, then
        ``nsim_patches_of_spectrograms``, whose dict it returns with "frames" and "deg_frames" added)."""
        cbuf, clens = self._rows(None, None, clean)
        dbuf, dlens = self._rows(None, None, degraded)
        G = int(G)
        if not 1 <= G <= 64 or len(dlens) != G * len(clens) or not clens:
            raise ValueError("degraded must hold G = 1 .. 64 rows per clean clip, row b G + g belonging to clip b")
        self.check_patches(patch, search, vad_ratio, min_active_frames)
        spec_ref, frames = self.gammatone(packed=(cbuf, clens), sample_rate=sample_rate)
        spec_deg, dframes = self.gammatone(packed=(dbuf, dlens), sample_rate=sample_rate)
        res = self.nsim_patches_of_spectrograms(spec_ref, spec_deg, frames, dframes, G, patch, search, vad_ratio, min_active_frames,
                                                intensity_range, want_bands, want_cand)
        res["frames"], res["deg_frames"] = frames, dframes
        return res

    ALIGN_MAX_DELAY = 16384

    def _align_rows(self, clean, degraded, G, max_delay):
        cbuf, clens = self._rows(None, None, clean)
        dbuf, dlens = self._rows(None, None, degraded)
        G, max_delay = int(G), int(max_delay)
        if not 1 <= G <= 64:
            raise ValueError(f"align takes 1 .. 64 degraded rows per clean clip, got {G}")
        if not 0 <= max_delay <= self.ALIGN_MAX_DELAY:
            raise ValueError(f"max_delay must be 0 .. {self.ALIGN_MAX_DELAY} samples, got {max_delay}")
        if len(dlens) != G * len(clens) or not clens:
            raise ValueError("degraded must hold G rows per clean clip, row b G + g belonging to clip b")
        if min(clens) < 1 or min(dlens) < 1:
            raise ValueError("every clean clip and every degraded row needs at least one sample")
        return cbuf, clens, dbuf, dlens, G, max_delay

    def align_delay(self, clean, degraded, G: int, max_delay: int, want_corr: bool = False):
        """The delay of every degraded row against its clean clip -> (delay (B G,) int32, peak (B G,) float64, corr (B G, 2
        max_delay + 1) float64 or None), all on the device: clean and degraded are (device buffer, lengths) pairs as ``nsim``
        takes them, but the degraded lengths may be any positive values.  ``corr[r][d + max_delay]`` is the cross-correlation
        ``sum_i x[i] y[i + d]``, the delay the lag of its largest value (d > 0: the row is late; ties to the smaller ``|d|``, then
        to d >= 0; any NaN: delay 0, peak NaN).  fp32 products on the matrix cores, 4096 steps per chain, the chains added in
        float64: include/nomad_hip.h states the order (``nomad_align_delay``)."""
        cbuf, clens, dbuf, dlens, G, max_delay = self._align_rows(clean, degraded, G, max_delay)
        B, R = len(clens), len(dlens)
        delay = torch.empty(R, dtype=torch.int32, device=self.device)
        peak = torch.empty(R, dtype=torch.float64, device=self.device)
        corr = torch.empty(R, 2 * max_delay + 1, dtype=torch.float64, device=self.device) if want_corr else None
        ws = self._workspace(self._scratch_size(self.lib.nomad_align_scratch_bytes, "nomad_align_scratch_bytes", B, G, cbuf.shape[1],
                                                dbuf.shape[1], max_delay))
        _lib.check(self.lib.nomad_align_delay(self.ctx, cbuf.data_ptr(), B, cbuf.shape[1], (C.c_int * B)(*clens), dbuf.data_ptr(), G,
                                              dbuf.shape[1], (C.c_int * R)(*dlens), max_delay, delay.data_ptr(), peak.data_ptr(), _ptr(corr),
                                              ws.data_ptr(), ws.numel(), self._stream()), "nomad_align_delay")
        return delay, peak, corr

    def align_shift(self, degraded, delay: torch.Tensor, out_lengths, out_stride: Optional[int] = None):
        """Every degraded row moved by its delay: ``out[r][i] = y[r][i + delay[r]]`` inside the row, 0 outside and behind
        ``out_lengths[r]`` -> (rows (R, out_stride) fp32 on the device, out_lengths).  ``delay`` is an int32 device tensor and is
        read on the device (``nomad_align_shift``)."""
        dbuf, dlens = self._rows(None, None, degraded)
        R = len(dlens)
        olens = [int(n) for n in out_lengths]
        if not (torch.is_tensor(delay) and delay.is_cuda and delay.dtype == torch.int32 and delay.is_contiguous() and delay.numel() == R):
            raise ValueError(f"delay must be a contiguous int32 tensor of {R} entries on {self.device}")
        if len(olens) != R or min(olens) < 1 or min(dlens) < 1:
            raise ValueError("out_lengths must hold one positive entry per degraded row")
        stride = (max(olens) + 3) // 4 * 4 if out_stride is None else int(out_stride)
        out = torch.empty(R, stride, dtype=torch.float32, device=self.device)
        ws = self._workspace(2 * ((4 * R + 255) // 256 * 256))
        _lib.check(self.lib.nomad_align_shift(self.ctx, dbuf.data_ptr(), R, dbuf.shape[1], (C.c_int * R)(*dlens), delay.data_ptr(),
                                              (C.c_int * R)(*olens), out.data_ptr(), stride, ws.data_ptr(), ws.numel(), self._stream()),
                   "nomad_align_shift")
        return out, olens

    def align(self, clean, degraded, G: int, max_delay: int):
        """``align_delay`` then ``align_shift`` with no host round trip -> ((rows (B G, stride) fp32, clean lengths repeated G
        times), delay (B G,) int32 on the device, peak (B G,) float64): row b G + g has clip b's length and stride, so the pair
        goes into ``nsim`` / ``embed_ragged(packed=...)`` as a degradation's result does."""
        cbuf, clens, dbuf, dlens, G, max_delay = self._align_rows(clean, degraded, G, max_delay)
        delay, peak, _ = self.align_delay((cbuf, clens), (dbuf, dlens), G, max_delay)
        rows = self.align_shift((dbuf, dlens), delay, [n for n in clens for _ in range(G)], out_stride=cbuf.shape[1])
        return rows, delay, peak

    def cdist(self, a: torch.Tensor, b: torch.Tensor, want_matrix: bool = True):
        """a (Na,D), b (Nb,D) fp32 on the GPU, D a multiple of 4 up to 4096 -> (dist (Na,Nb) float64 or None, mean (Na,)
        float64): ``pairwise`` for rows of any width (the same bits at D = 256)."""
        self._check_dev(a, "a")
        self._check_dev(b, "b")
        if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
            raise ValueError("a and b must be matrices with rows of one width")
        Na, Nb, D = a.shape[0], b.shape[0], a.shape[1]
        dist = torch.empty(Na, Nb, dtype=torch.float64, device=self.device) if want_matrix else None
        mean = torch.empty(Na, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.nomad_cdist(self.ctx, a.data_ptr(), Na, b.data_ptr(), Nb, D,
                                        _ptr(dist), mean.data_ptr(), self._stream()),
                   "nomad_cdist")
        return dist, mean

    def cdist_backward(self, a: torch.Tensor, b: torch.Tensor, g_dist: Optional[torch.Tensor] = None,
                       g_mean: Optional[torch.Tensor] = None, want_a: bool = True, want_b: bool = False):
        """The backward of ``cdist(a, b)``: g_dist (Na,Nb) and / or g_mean (Na,) float64, the upstreams of its matrix and of its row
        means -> (da (Na,D) or None, db (Nb,D) or None), fp32.  Float64 sums in a fixed order, rounded once; a pair at distance 0
        contributes nothing (``nomad_cdist_backward``)."""
        self._check_dev(a, "a")
        self._check_dev(b, "b")
        if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
            raise ValueError("a and b must be matrices with rows of one width")
        Na, Nb, D = a.shape[0], b.shape[0], a.shape[1]
        if g_dist is None and g_mean is None:
            raise ValueError("cdist_backward needs g_dist, g_mean or both")
        if not (want_a or want_b):
            raise ValueError("cdist_backward needs want_a, want_b or both")
        for g, shape, name in ((g_dist, (Na, Nb), "g_dist"), (g_mean, (Na,), "g_mean")):
            if g is not None and not (g.is_cuda and g.dtype == torch.float64 and g.is_contiguous() and tuple(g.shape) == shape):
                raise ValueError(f"{name} must be a contiguous float64 tensor of shape {shape} on {self.device}")
        n = C.c_size_t()
        _lib.check(self.lib.nomad_cdist_backward_scratch_bytes(Na, Nb, C.byref(n)), "nomad_cdist_backward_scratch_bytes")
        scratch = self._distance_scratch(n.value)
        da = torch.empty(Na, D, dtype=torch.float32, device=self.device) if want_a else None
        db = torch.empty(Nb, D, dtype=torch.float32, device=self.device) if want_b else None
        _lib.check(self.lib.nomad_cdist_backward(self.ctx, a.data_ptr(), Na, b.data_ptr(), Nb, D, _ptr(g_dist), _ptr(g_mean), _ptr(da),
                                                 _ptr(db), scratch.data_ptr(), scratch.numel(),
                                                 self._stream()), "nomad_cdist_backward")
        return da, db

    def _distance_scratch(self, nbytes: int) -> torch.Tensor:
        """The cached scratch of ``cdist_backward`` / ``knn`` / ``knn_backward``, grown on demand (calls on one stream are ordered)."""
        if self._cdist_scratch is None or self._cdist_scratch.numel() < nbytes:
            self._cdist_scratch = None
            self._cdist_scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device)
        self._cdist_scratch.record_stream(torch.cuda.current_stream(self.device))
        return self._cdist_scratch

    def _check_knn(self, a: torch.Tensor, b: torch.Tensor, k):
        self._check_dev(a, "a")
        self._check_dev(b, "b")
        if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
            raise ValueError("a and b must be matrices with rows of one width")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(64, b.shape[0]):
            raise ValueError(f"k must be an integer from 1 to min(64, rows of b = {b.shape[0]}), got {k!r}")
        return a.shape[0], b.shape[0], a.shape[1]

    def knn(self, a: torch.Tensor, b: torch.Tensor, k: int, want_matrix: bool = False):
        """a (Na,D), b (Nb,D) fp32 on the GPU as ``cdist`` takes them, 1 <= k <= min(64, Nb) -> (knn_dist (Na,k) float64, knn_idx
        (Na,k) int32, score (Na,) float64[, dist (Na,Nb) float64]): per row of a the k rows of b at the smallest distance, ascending
        under (distance, index) with NaN as +infinity, and their mean.  The distances are ``cdist``'s bits; without ``want_matrix``
        the matrix is never formed (``nomad_knn``)."""
        Na, Nb, D = self._check_knn(a, b, k)
        n = C.c_size_t()
        _lib.check(self.lib.nomad_knn_scratch_bytes(Na, Nb, k, C.byref(n)), "nomad_knn_scratch_bytes")
        scratch = self._distance_scratch(n.value)
        dist = torch.empty(Na, Nb, dtype=torch.float64, device=self.device) if want_matrix else None
        knn_dist = torch.empty(Na, k, dtype=torch.float64, device=self.device)
        knn_idx = torch.empty(Na, k, dtype=torch.int32, device=self.device)
        score = torch.empty(Na, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.nomad_knn(self.ctx, a.data_ptr(), Na, b.data_ptr(), Nb, D, k, _ptr(dist), knn_dist.data_ptr(),
                                      knn_idx.data_ptr(), score.data_ptr(), scratch.data_ptr(), scratch.numel(), self._stream()),
                   "nomad_knn")
        return (knn_dist, knn_idx, score, dist) if want_matrix else (knn_dist, knn_idx, score)

    def knn_backward(self, a: torch.Tensor, b: torch.Tensor, knn_idx: torch.Tensor, g_knn: Optional[torch.Tensor] = None,
                     g_score: Optional[torch.Tensor] = None, want_a: bool = True, want_b: bool = True):
        """The backward of ``knn(a, b, k)`` with the selection ``knn_idx`` (Na,k) int32 held fixed: g_knn (Na,k) and / or g_score
        (Na,) float64, the upstreams of the neighbour distances and of their mean -> (da (Na,D) or None, db (Nb,D) or None), fp32:
        the bits of ``cdist_backward`` fed the dense upstream of the selected pairs (``nomad_knn_backward``)."""
        if not (torch.is_tensor(knn_idx) and knn_idx.is_cuda and knn_idx.dtype == torch.int32 and knn_idx.dim() == 2
                and knn_idx.is_contiguous() and knn_idx.shape[0] == a.shape[0]):
            raise ValueError(f"knn_idx must be a contiguous int32 tensor of shape (rows of a, k) on {self.device}")
        k = int(knn_idx.shape[1])
        Na, Nb, D = self._check_knn(a, b, k)
        if g_knn is None and g_score is None:
            raise ValueError("knn_backward needs g_knn, g_score or both")
        if not (want_a or want_b):
            raise ValueError("knn_backward needs want_a, want_b or both")
        for g, shape, name in ((g_knn, (Na, k), "g_knn"), (g_score, (Na,), "g_score")):
            if g is not None and not (g.is_cuda and g.dtype == torch.float64 and g.is_contiguous() and tuple(g.shape) == shape):
                raise ValueError(f"{name} must be a contiguous float64 tensor of shape {shape} on {self.device}")
        n = C.c_size_t()
        _lib.check(self.lib.nomad_knn_backward_scratch_bytes(Na, Nb, k, C.byref(n)), "nomad_knn_backward_scratch_bytes")
        scratch = self._distance_scratch(n.value)
        da = torch.empty(Na, D, dtype=torch.float32, device=self.device) if want_a else None
        db = torch.empty(Nb, D, dtype=torch.float32, device=self.device) if want_b else None
        _lib.check(self.lib.nomad_knn_backward(self.ctx, a.data_ptr(), Na, b.data_ptr(), Nb, D, k, knn_idx.data_ptr(), _ptr(g_knn),
                                               _ptr(g_score), _ptr(da), _ptr(db), scratch.data_ptr(), scratch.numel(),
                                               self._stream()), "nomad_knn_backward")
        return da, db

    def paired_distance(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """a, b (N,D) fp32 on the GPU -> (N,) float64, out[i] = ||a_i - b_i||: the diagonal of ``cdist(a, b)`` bit for bit,
        without the matrix."""
        self._check_dev(a, "a")
        self._check_dev(b, "b")
        if a.dim() != 2 or a.shape != b.shape:
            raise ValueError("a and b must be matrices of one shape")
        out = torch.empty(a.shape[0], dtype=torch.float64, device=self.device)
        _lib.check(self.lib.nomad_paired_distance(self.ctx, a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], out.data_ptr(),
                                                  self._stream()), "nomad_paired_distance")
        return out

    def pairwise(self, deg: torch.Tensor, ref: torch.Tensor, want_matrix: bool = True):
        """deg (Nd,256), ref (Nr,256) fp32 on GPU -> (dist (Nd,Nr) float64 or None, mean (Nd,) float64)."""
        self._check_dev(deg, "deg")
        self._check_dev(ref, "ref")
        if deg.shape[1] != 256 or ref.shape[1] != 256:
            raise ValueError("embeddings must be 256-dimensional")
        Nd, Nr = deg.shape[0], ref.shape[0]
        dist = torch.empty(Nd, Nr, dtype=torch.float64, device=self.device) if want_matrix else None
        mean = torch.empty(Nd, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.nomad_pairwise(self.ctx, deg.data_ptr(), Nd, ref.data_ptr(), Nr,
                                           _ptr(dist), mean.data_ptr(),
                                           self._stream()), "nomad_pairwise")
        return dist, mean

    def l1_loss(self, a_layers, b_layers, a_emb, b_emb) -> torch.Tensor:
        for t, n in ((a_layers, "a_layers"), (b_layers, "b_layers"), (a_emb, "a_emb"), (b_emb, "b_emb")):
            self._check_dev(t, n)
        if self._l1_scratch is None:
            self._l1_scratch = torch.empty(self.lib.nomad_l1_scratch_bytes(), dtype=torch.uint8, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        if a_layers.dim() == 3:   # packed layers (12, M, 768) of a ragged batch: means over the valid frames
            _lib.check(self.lib.nomad_l1_loss_ragged(self.ctx, a_layers.data_ptr(), b_layers.data_ptr(), a_emb.data_ptr(),
                                                     b_emb.data_ptr(), a_layers.shape[1], a_emb.shape[0], loss.data_ptr(),
                                                     self._l1_scratch.data_ptr(), self._stream()), "nomad_l1_loss_ragged")
            return loss[0]
        _, B, T, _ = a_layers.shape
        _lib.check(self.lib.nomad_l1_loss(self.ctx, a_layers.data_ptr(), b_layers.data_ptr(), a_emb.data_ptr(),
                                          b_emb.data_ptr(), B, T, loss.data_ptr(), self._l1_scratch.data_ptr(),
                                          self._stream()), "nomad_l1_loss")
        return loss[0]

    def _l1w_call(self, a_layers, b_layers, a_emb, b_emb, weights, reduction, frames):
        """Checked arguments of ``nomad_l1_loss_weighted*``: (M, B, frames array or None, weights array, reduction code, scratch)."""
        if reduction not in _lib.L1_REDUCTION:
            raise ValueError(f"reduction must be 'mean' or 'none', got {reduction!r}")
        w = [float(x) for x in weights]
        if len(w) != 13:
            raise ValueError(f"13 weights (12 layers + the embedding) are needed, got {len(w)}")
        if a_layers.shape != b_layers.shape or a_layers.dim() not in (3, 4) or a_layers.shape[0] != 12 or a_layers.shape[-1] != 768:
            raise ValueError(f"layer tensors must both be (12,B,T,768) or (12,M,768), got {tuple(a_layers.shape)} and {tuple(b_layers.shape)}")
        for t, n in ((a_layers, "a_layers"), (b_layers, "b_layers")):
            self._check_dev(t, n)
        if w[12] != 0.0:   # (a cut encoder leaves the embeddings unwritten: unread, so unchecked, when their weight is 0)
            self._check_dev(a_emb, "a_emb")
            self._check_dev(b_emb, "b_emb")
            if a_emb.shape != b_emb.shape:
                raise ValueError(f"embeddings must have one shape, got {tuple(a_emb.shape)} and {tuple(b_emb.shape)}")
        if a_layers.dim() == 4:
            B, M = a_layers.shape[1], a_layers.shape[1] * a_layers.shape[2]
            if frames is not None:
                raise ValueError("frames goes with packed (12,M,768) layers")
        else:
            M = a_layers.shape[1]
            if frames is None:
                raise ValueError("packed (12,M,768) layers need the clips' frame counts")
            B = len(frames)
        if w[12] != 0.0 and a_emb.shape[0] != B:
            raise ValueError(f"{a_emb.shape[0]} embeddings for {B} clips")
        arr = (C.c_int * B)(*[int(t) for t in frames]) if frames is not None else None
        n = C.c_size_t()
        _lib.check(self.lib.nomad_l1_weighted_scratch_bytes(M, B, C.byref(n)), "nomad_l1_weighted_scratch_bytes")
        if self._l1w_scratch is None or self._l1w_scratch.numel() < n.value:
            self._l1w_scratch = None
            self._l1w_scratch = torch.empty(n.value, dtype=torch.uint8, device=self.device)
        self._l1w_scratch.record_stream(torch.cuda.current_stream(self.device))
        return M, B, arr, (C.c_float * 13)(*w), _lib.L1_REDUCTION[reduction], self._l1w_scratch

    def l1_loss_weighted(self, a_layers, b_layers, a_emb, b_emb, weights, reduction: str = "mean", frames=None,
                         want_terms: bool = True):
        """NomadLoss with a weight per term and, with reduction="none", one loss per clip -> (loss, terms).

        a_layers / b_layers (12,B,T,768), or packed (12,M,768) with ``frames`` (the clips' frame counts); weights: 13 numbers >= 0
        (index 12 = the embedding) - a term with weight 0 is not read, so behind a cut encoder (``encoder_depth``) its tensors may
        hold anything.  "mean": a 0-dim loss, every term the mean over the batch's valid elements (``l1_loss`` with weights);
        "none": (B,), every term the mean over the clip's own elements.  terms: (13,B) float64 per-clip means (0 where the
        weight is 0), or None with want_terms=False."""
        M, B, arr, w, red, scratch = self._l1w_call(a_layers, b_layers, a_emb, b_emb, weights, reduction, frames)
        loss = torch.empty(B if reduction == "none" else 1, dtype=torch.float32, device=self.device)
        terms = torch.empty(13, B, dtype=torch.float64, device=self.device) if want_terms else None
        _lib.check(self.lib.nomad_l1_loss_weighted(self.ctx, a_layers.data_ptr(), b_layers.data_ptr(), _ptr(a_emb), _ptr(b_emb), M,
                                                   B, arr, w, red, loss.data_ptr(), _ptr(terms), scratch.data_ptr(),
                                                   scratch.numel(), self._stream()), "nomad_l1_loss_weighted")
        return (loss if reduction == "none" else loss[0]), terms

    def l1_loss_weighted_backward(self, a_layers, b_layers, a_emb, b_emb, upstream: torch.Tensor, weights,
                                  reduction: str = "mean", frames=None, depth: Optional[int] = None, dlayers=None, demb=None):
        """(d loss / d a_layers, d loss / d a_emb or None) of ``l1_loss_weighted``; upstream: 0-dim ("mean") or (B,) ("none").
        depth (default: ``encoder_depth``): layers below it with weight 0 are written as zeros, layers from it on are left
        untouched (``dlayers``: a buffer to write into, else a fresh uninitialised one); the embedding gradient is None when its
        weight is 0."""
        M, B, arr, w, red, scratch = self._l1w_call(a_layers, b_layers, a_emb, b_emb, weights, reduction, frames)
        depth = self.encoder_depth if depth is None else int(depth)
        dl = torch.empty_like(a_layers) if dlayers is None else dlayers
        self._check_dev(dl, "dlayers")
        if dl.shape != a_layers.shape:
            raise ValueError("dlayers must have the layers' shape")
        de = None
        if w[12] != 0.0:
            de = torch.empty_like(a_emb) if demb is None else demb
        up = upstream.to(self.device, torch.float32).reshape(-1).contiguous()
        if up.numel() != (B if reduction == "none" else 1):
            raise ValueError(f"upstream has {up.numel()} values for reduction={reduction!r} over {B} clips")
        _lib.check(self.lib.nomad_l1_loss_weighted_backward(self.ctx, a_layers.data_ptr(), b_layers.data_ptr(), _ptr(a_emb),
                                                            _ptr(b_emb), M, B, arr, w, red, depth, up.data_ptr(), dl.data_ptr(),
                                                            _ptr(de), scratch.data_ptr(), scratch.numel(),
                                                            self._stream()), "nomad_l1_loss_weighted_backward")
        return dl, de

    # ---- bf16 path (long-form clips, config C5) and bf16x3 path (fp32-class scores on the bf16 matrix cores) --------------------
    def _embed_into(self, precision: str, wav: torch.Tensor, emb: torch.Tensor, side):
        """``nomad_embed_bf16`` / ``nomad_embed_bf16x3`` over the whole of ``wav`` (B,N) into ``emb`` on the current stream."""
        B, N = wav.shape
        ws = self._workspace(self._forward_size(precision, B, N), side)
        _lib.check(getattr(self.lib, "nomad_embed_" + precision)(self.ctx, wav.data_ptr(), B, N, emb.data_ptr(), ws.data_ptr(), ws.numel(),
                                                                 self._stream()), "nomad_embed_" + precision)

    def _embed_bf16_into(self, wav: torch.Tensor, emb: torch.Tensor, side):
        """(What the stage tests and the race-hunt tools drive directly: one bf16 forward, no split, on the workspace they name.)"""
        self._embed_into("bf16", wav, emb, side)

    def embed_bf16(self, wav: torch.Tensor) -> torch.Tensor:
        """Scoring forward with bf16 activations/weights (fp32 accumulation and statistics)."""
        wav, B, N, T = self._check_wav(wav)
        self.enable("bf16")
        emb = torch.empty(B, 256, dtype=torch.float32, device=self.device)
        self._dispatch(B, B // 2 if self._splits("bf16", B, B * T) else 0,
                       lambda lo, hi, side: self._embed_into("bf16", wav[lo:hi], emb[lo:hi], side), hint=True)
        return emb

    def embed_bf16x3(self, wav: torch.Tensor, head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                     want_layers: bool = False, side: bool = False):
        """Forward whose GEMMs run as three bf16 MFMA products over hi/lo-split operands (fp32 accumulation,
        fp32 softmax / LayerNorm / head): NOMAD scores agree with the fp32 path to ~1e-6.
        want_layers / head: as in ``embed`` -> (emb, layers (12,B,T,768)), the LossNetLayers outputs (no gradient:
        the branch of ``forward()`` that needs one stays on ``embed_train``)."""
        wav, B, N, T = self._check_wav(wav)
        self.enable("bf16x3")
        emb = torch.empty(B, 256, dtype=torch.float32, device=self.device)
        if want_layers or head is not None:
            hw, hb = self._check_head(head)
            layers = torch.empty(12, B, T, 768, dtype=torch.float32, device=self.device)
            ws = self._workspace(self._forward_size("bf16x3", B, N), side)
            _lib.check(self.lib.nomad_embed_layers_bf16x3(self.ctx, wav.data_ptr(), B, N, _ptr(hw), _ptr(hb), emb.data_ptr(),
                                                          layers.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                       "nomad_embed_layers_bf16x3")
            return (emb, layers) if want_layers else emb

        def run(lo, hi, use_side):
            self._embed_into("bf16x3", wav[lo:hi], emb[lo:hi], use_side)

        if side:
            run(0, B, side)   # the caller's own concurrency: its stream, the side workspace it names, no split
        else:
            self._dispatch(B, B // 2 if self._splits("bf16x3", B, B * T) else 0, run)
        return emb

    def diag_split_bf16(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 tensor -> split buffer (bf16 tensor of shape (2, *x.shape): plane 0 = hi, plane 1 = lo)."""
        x = x.contiguous()
        out = torch.empty((2,) + tuple(x.shape), dtype=torch.bfloat16, device=self.device)
        _lib.check(self.lib.nomad_diag_split_bf16(self.ctx, x.data_ptr(), out.data_ptr(), x.numel(), x.numel(), 0,
                                                  self._stream()), "nomad_diag_split_bf16")
        return out

    def diag_unsplit_bf16(self, xs: torch.Tensor) -> torch.Tensor:
        out = torch.empty(tuple(xs.shape[1:]), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nomad_diag_split_bf16(self.ctx, xs.data_ptr(), out.data_ptr(), out.numel(), out.numel(), 1,
                                                  self._stream()), "nomad_diag_split_bf16")
        return out

    def diag_gemm_bf16x3(self, A, W, bias=None, R=None, gelu=False, out_f32=True, out=None, variant=None):
        """A (2,M,K), W (2,N,K), R (2,M,N) split buffers (diag_split_bf16); returns fp32 (M,N) or a split (2,M,N).
        variant (int, optional): kernel selector of nomad_diag_gemm_bf16x3 - 0/1 K-concatenated kernel (split / fp32 out),
        7/8 staged-once kernel (split / fp32 out), 12/13 the same with three A buffers (K % 192 == 0), others are timing
        probes with fp32 output."""
        if variant is None:
            variant = 8 if out_f32 else 7
        out_f32 = variant % 100 not in (0, 7, 12)
        _, M, K = A.shape
        N = W.shape[1]
        if out is None:
            out = (torch.zeros(M, N, dtype=torch.float32, device=self.device) if out_f32
                   else torch.zeros(2, M, N, dtype=torch.bfloat16, device=self.device))
        _lib.check(self.lib.nomad_diag_gemm_bf16x3(self.ctx, A.data_ptr(), W.data_ptr(), _ptr(bias), _ptr(R), out.data_ptr(), M, N,
                                                   K, int(gelu), int(variant), self._stream()), "nomad_diag_gemm_bf16x3")
        return out

    def diag_attention_bf16x3(self, qkv_split, B, T, waves: int = -1):
        """qkv_split (2, B*T, 2304) split buffer -> split (2, B*T, 768).  waves: -1 the forward's choice, 0 the tiled
        kernel, 4 / 8 the K/V-resident kernel (T <= 256)."""
        out = torch.empty(2, B * T, 768, dtype=torch.bfloat16, device=self.device)
        _lib.check(self.lib.nomad_diag_attention_bf16x3(self.ctx, qkv_split.data_ptr(), out.data_ptr(), B, T, waves, self._stream()),
                   "nomad_diag_attention_bf16x3")
        return out

    def diag_attention_bf16(self, qkv, B, T, q_has_log2e: bool = True):
        """qkv (B*T, 2304) bf16 -> (B*T, 768) bf16.  q_has_log2e: the q columns already carry log2(e) (what the bf16
        forward's QKV projection produces); False is an error (the kernel that scaled q itself was removed)."""
        out = torch.empty(B * T, 768, dtype=torch.bfloat16, device=self.device)
        _lib.check(self.lib.nomad_diag_attention_bf16(self.ctx, qkv.data_ptr(), out.data_ptr(), B, T, int(q_has_log2e), self._stream()),
                   "nomad_diag_attention_bf16")
        return out

    def diag_gemm_bf16(self, A, W, bias=None, R=None, gelu=False, tile=0, out=None):
        M, K = A.shape
        N = W.shape[0]
        if out is None:
            out = torch.zeros(M, N, dtype=torch.bfloat16, device=self.device)  # zeros: a kernel that writes nothing shows
        _lib.check(self.lib.nomad_diag_gemm_bf16(self.ctx, A.data_ptr(), W.data_ptr(), _ptr(bias), _ptr(R), out.data_ptr(), M, N, K,
                                                 int(gelu), tile, self._stream()), "nomad_diag_gemm_bf16")
        return out

    # ---- training (differentiable forward) ---------------------------------------------------------
    @property
    def feature_grad_mult(self) -> float:
        """fairseq ``feature_grad_mult``: scale of the gradient entering the conv feature extractor in
        ``embed_backward`` (0.1 = wav2vec 2.0 BASE / wav2vec_small.pt; 1.0 = plain chain rule)."""
        v = C.c_float()
        _lib.check(self.lib.nomad_get_feature_grad_mult(self.ctx, C.byref(v)), "nomad_get_feature_grad_mult")
        return float(v.value)

    @feature_grad_mult.setter
    def feature_grad_mult(self, mult: float):
        _lib.check(self.lib.nomad_set_feature_grad_mult(self.ctx, float(mult)), "nomad_set_feature_grad_mult")

    @property
    def encoder_depth(self) -> int:
        """How many encoder layers the loss's layer-output forwards (``embed(want_layers=True)``, ``embed_train``,
        ``embed_train_ragged``) and ``embed_backward[_ragged]`` run: 1 .. 12, default 12.  Below 12 the forwards stop behind layer
        depth - 1 (layer outputs from ``depth`` on and the embedding stay unwritten) and every scoring / bf16 / fine-tuning entry
        point raises (``nomad_set_encoder_depth``)."""
        v = C.c_int()
        _lib.check(self.lib.nomad_get_encoder_depth(self.ctx, C.byref(v)), "nomad_get_encoder_depth")
        return int(v.value)

    @encoder_depth.setter
    def encoder_depth(self, depth: int):
        _lib.check(self.lib.nomad_set_encoder_depth(self.ctx, int(depth)), "nomad_set_encoder_depth")

    @property
    def gemm_precision(self) -> str:
        """"fp32" (exact fp32 MFMA, the default) or "bf16x3" (three bf16 MFMA products over hi / lo halves split in
        registers, fp32 accumulation) for the GEMMs of ``embed`` / ``embed_ragged`` / ``embed_train`` / the backward passes;
        buffers and every other kernel stay fp32 (``nomad_set_gemm_precision``)."""
        v = C.c_int()
        _lib.check(self.lib.nomad_get_gemm_precision(self.ctx, C.byref(v)), "nomad_get_gemm_precision")
        return "bf16x3" if v.value else "fp32"

    @gemm_precision.setter
    def gemm_precision(self, mode: str):
        if mode not in ("fp32", "bf16x3"):
            raise ValueError("gemm_precision must be 'fp32' or 'bf16x3'")
        _lib.check(self.lib.nomad_set_gemm_precision(self.ctx, int(mode == "bf16x3")), "nomad_set_gemm_precision")

    def enable_backward(self):
        _lib.check(self.lib.nomad_enable_backward(self.ctx), "nomad_enable_backward")

    def embed_train(self, wav: torch.Tensor, head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """Training-mode forward: -> (emb (B,256), layers (12,B,T,768), saved block for embed_backward)."""
        if wav.dim() == 3:
            wav = wav.squeeze(1)
        self._check_dev(wav, "wav")
        self.enable_backward()   # also allocates the split-K scratch: the first call must run the same kernels as later ones
        B, N = wav.shape
        T = num_frames(N)
        emb = torch.empty(B, 256, dtype=torch.float32, device=self.device)
        layers = torch.empty(12, B, T, 768, dtype=torch.float32, device=self.device)
        saved = torch.empty(self._size(self.lib.nomad_saved_bytes, B, N, "nomad_saved_bytes"), dtype=torch.uint8,
                            device=self.device)
        hw, hb = head if head is not None else (None, None)
        ws = self._workspace(self.workspace_bytes(B, N))
        _lib.check(self.lib.nomad_embed_train(self.ctx, wav.data_ptr(), B, N, _ptr(hw), _ptr(hb), emb.data_ptr(), layers.data_ptr(),
                                              saved.data_ptr(), saved.numel(), ws.data_ptr(), ws.numel(),
                                              self._stream()), "nomad_embed_train")
        return emb, layers, saved

    def embed_backward(self, wav, layers, saved, dlayers, demb, head=None) -> torch.Tensor:
        """d loss / d wav (B,N) from d loss / d layers (12,B,T,768 or None) and d loss / d emb (B,256; None only while
        ``encoder_depth`` is below 12, where it is ignored)."""
        if wav.dim() == 3:
            wav = wav.squeeze(1)
        B, N = wav.shape
        self.enable_backward()
        nb = self._size(self.lib.nomad_backward_workspace_bytes, B, N, "nomad_backward_workspace_bytes")
        ws = self._workspace(nb)
        dwav = torch.empty(B, N, dtype=torch.float32, device=self.device)
        hw, hb = head if head is not None else (None, None)
        _lib.check(self.lib.nomad_embed_backward(self.ctx, wav.data_ptr(), B, N, _ptr(hw), _ptr(hb), layers.data_ptr(),
                                                 saved.data_ptr(), saved.numel(), _ptr(dlayers), _ptr(demb), dwav.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), self._stream()), "nomad_embed_backward")
        return dwav

    def l1_loss_backward(self, a_layers, b_layers, a_emb, b_emb, upstream: torch.Tensor):
        """(d loss/d a_layers, d loss/d a_emb) for NomadLoss, scaled by the 0-dim device tensor `upstream`."""
        dl = torch.empty_like(a_layers)
        de = torch.empty_like(a_emb)
        up = upstream.to(self.device, torch.float32).reshape(1).contiguous()
        if a_layers.dim() == 3:   # packed layers (12, M, 768) of a ragged batch
            _lib.check(self.lib.nomad_l1_loss_backward_ragged(self.ctx, a_layers.data_ptr(), b_layers.data_ptr(), a_emb.data_ptr(),
                                                              b_emb.data_ptr(), a_layers.shape[1], a_emb.shape[0], up.data_ptr(),
                                                              dl.data_ptr(), de.data_ptr(), self._stream()),
                       "nomad_l1_loss_backward_ragged")
            return dl, de
        _, B, T, _ = a_layers.shape
        _lib.check(self.lib.nomad_l1_loss_backward(self.ctx, a_layers.data_ptr(), b_layers.data_ptr(), a_emb.data_ptr(),
                                                   b_emb.data_ptr(), B, T, up.data_ptr(), dl.data_ptr(), de.data_ptr(),
                                                   self._stream()), "nomad_l1_loss_backward")
        return dl, de

    # ---- exact-length (ragged) batches on the gradient paths ------------------------------------------
    def pack_ragged(self, waves, lengths=None):
        """Clips -> (device (B, stride) fp32 buffer, lengths): what the ragged gradient calls take.  waves: a list of 1-D (or
        (1,N)) tensors / arrays as ``embed_ragged`` takes them, or a padded (B,N) / (B,1,N) device tensor plus ``lengths``
        (used as it is, no copy: samples behind a length are never read)."""
        if lengths is not None:
            wav = waves.squeeze(1) if waves.dim() == 3 else waves
            self._check_dev(wav, "wav")
            lens = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
            if wav.dim() != 2 or len(lens) != wav.shape[0]:
                raise ValueError("lengths must hold one entry per row of the (B,N) waveform tensor")
            if any(n > wav.shape[1] for n in lens):
                raise ValueError("a length exceeds the padded waveform tensor")
            return wav, lens
        return self._pack(waves)

    def embed_train_ragged(self, waves, lengths=None, head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                           save: bool = True, side: bool = False):
        """``embed_train`` over clips of different lengths in ONE launch sequence, no padding in the arithmetic:
        -> (emb (B,256), packed layers (12,M,768) with M = sum of the clips' frames, saved block, (buffer, lengths)).
        save=False: layer outputs only (no saved block - None -, no regularisation): the ragged ``LossNetLayers`` forward.
        The last item is what ``embed_backward_ragged`` / ``train_backward_ragged`` take as their batch."""
        buf, lens = self.pack_ragged(waves, lengths)
        if save:
            self.enable_backward()
        B, stride = buf.shape
        M = sum(num_frames(n) for n in lens)
        arr = (C.c_int * B)(*lens)
        emb = torch.empty(B, 256, dtype=torch.float32, device=self.device)
        layers = torch.empty(12, M, 768, dtype=torch.float32, device=self.device)
        saved = torch.empty(self._size_ragged(self.lib.nomad_saved_bytes_ragged, lens, "nomad_saved_bytes_ragged"),
                            dtype=torch.uint8, device=self.device) if save else None
        hw, hb = head if head is not None else (None, None)
        ws = self._workspace(self._size_ragged(self.lib.nomad_workspace_bytes_ragged, lens, "nomad_workspace_bytes_ragged"), side)
        _lib.check(self.lib.nomad_embed_train_ragged(self.ctx, buf.data_ptr(), B, stride, arr, _ptr(hw), _ptr(hb), emb.data_ptr(),
                                                     layers.data_ptr(), _ptr(saved), saved.numel() if save else 0, ws.data_ptr(),
                                                     ws.numel(), self._stream()), "nomad_embed_train_ragged")
        return emb, layers, saved, (buf, lens)

    def embed_backward_ragged(self, batch, layers, saved, dlayers, demb, head=None) -> torch.Tensor:
        """d loss / d wav (B, stride) of an ``embed_train_ragged`` call (``batch``: its last result) from d loss / d layers
        (12,M,768 or None) and d loss / d emb (B,256); zero behind every clip's length."""
        buf, lens = batch
        B, stride = buf.shape
        self.enable_backward()
        ws = self._workspace(self._size_ragged(self.lib.nomad_backward_workspace_bytes_ragged, lens,
                                               "nomad_backward_workspace_bytes_ragged"))
        dwav = torch.empty(B, stride, dtype=torch.float32, device=self.device)
        hw, hb = head if head is not None else (None, None)
        _lib.check(self.lib.nomad_embed_backward_ragged(self.ctx, buf.data_ptr(), B, stride, (C.c_int * B)(*lens), _ptr(hw),
                                                        _ptr(hb), layers.data_ptr(), saved.data_ptr(), saved.numel(), _ptr(dlayers),
                                                        _ptr(demb), dwav.data_ptr(), ws.data_ptr(), ws.numel(),
                                                        self._stream()), "nomad_embed_backward_ragged")
        return dwav

    # ---- the windowed head on the gradient path (differentiable scores over time) ----------------------------------------
    def _check_grad_windows(self, win, hop, head):
        win, hop = int(win), int(hop)
        if win < 1 or hop < 1:
            raise ValueError(f"win and hop must be at least 1 frame, got win={win}, hop={hop}")
        hw, hb = self._check_head(head)
        return win, hop, hw, hb

    def embed_train_windows(self, wav: torch.Tensor, win: int, hop: int, head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """``embed_train`` with the windowed head of ``embed_windows`` as its last stage: -> (emb_w (W_total,256), counts,
        layers (12,B,T,768), saved block for ``embed_windows_backward``).  Rows and counts as in ``embed_windows``."""
        win, hop, hw, hb = self._check_grad_windows(win, hop, head)
        wav, B, N, T = self._check_wav(wav)
        self.enable_backward()
        W = num_windows(T, win, hop)
        emb = torch.empty(B * W, 256, dtype=torch.float32, device=self.device)
        layers = torch.empty(12, B, T, 768, dtype=torch.float32, device=self.device)
        saved = torch.empty(self._size(self.lib.nomad_saved_bytes, B, N, "nomad_saved_bytes"), dtype=torch.uint8,
                            device=self.device)
        ws = self._workspace(self.workspace_bytes(B, N))
        _lib.check(self.lib.nomad_embed_train_windows(self.ctx, wav.data_ptr(), B, N, win, hop, _ptr(hw), _ptr(hb), emb.data_ptr(),
                                                      layers.data_ptr(), saved.data_ptr(), saved.numel(), ws.data_ptr(), ws.numel(),
                                                      self._stream()), "nomad_embed_train_windows")
        return emb, [W] * B, layers, saved

    def embed_train_windows_ragged(self, waves, win: int, hop: int, lengths=None,
                                   head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """``embed_train_ragged`` with the windowed head: -> (emb_w (W_total,256), counts, packed layers (12,M,768), saved block,
        (buffer, lengths)); the last item is the batch ``embed_windows_backward_ragged`` takes."""
        win, hop, hw, hb = self._check_grad_windows(win, hop, head)
        buf, lens = self.pack_ragged(waves, lengths)
        frames = [num_frames(n) for n in lens]
        if min(frames) < 1:
            raise ValueError(f"a clip of {min(lens)} samples is shorter than the conv stack's receptive field")
        self.enable_backward()
        B, stride = buf.shape
        counts = [num_windows(t, win, hop) for t in frames]
        emb = torch.empty(sum(counts), 256, dtype=torch.float32, device=self.device)
        layers = torch.empty(12, sum(frames), 768, dtype=torch.float32, device=self.device)
        saved = torch.empty(self._size_ragged(self.lib.nomad_saved_bytes_ragged, lens, "nomad_saved_bytes_ragged"),
                            dtype=torch.uint8, device=self.device)
        ws = self._workspace(self._size_ragged(self.lib.nomad_workspace_bytes_ragged, lens, "nomad_workspace_bytes_ragged"))
        _lib.check(self.lib.nomad_embed_train_windows_ragged(self.ctx, buf.data_ptr(), B, stride, (C.c_int * B)(*lens), win, hop,
                                                             _ptr(hw), _ptr(hb), emb.data_ptr(), layers.data_ptr(), saved.data_ptr(),
                                                             saved.numel(), ws.data_ptr(), ws.numel(), self._stream()),
                   "nomad_embed_train_windows_ragged")
        return emb, counts, layers, saved, (buf, lens)

    def _windows_scratch(self, n_windows: int) -> torch.Tensor:
        """The per-window gradient rows of the windowed head's backward: a fresh block per call, like the outputs."""
        n = C.c_size_t()
        _lib.check(self.lib.nomad_windows_backward_scratch_bytes(n_windows, C.byref(n)), "nomad_windows_backward_scratch_bytes")
        return torch.empty(n.value, dtype=torch.uint8, device=self.device)

    def _check_demb_w(self, demb_w: torch.Tensor, n_windows: int):
        self._check_dev(demb_w, "demb_w")
        if tuple(demb_w.shape) != (n_windows, 256):
            raise ValueError(f"demb_w must be ({n_windows}, 256): one row per window, got {tuple(demb_w.shape)}")

    def embed_windows_backward(self, wav, layers, saved, demb_w, win: int, hop: int, head=None) -> torch.Tensor:
        """d loss / d wav (B,N) of an ``embed_train_windows`` call from d loss / d emb_w (W_total,256)."""
        win, hop, hw, hb = self._check_grad_windows(win, hop, head)
        wav, B, N, T = self._check_wav(wav)
        self._check_demb_w(demb_w, B * num_windows(T, win, hop))
        self.enable_backward()
        ws = self._workspace(self._size(self.lib.nomad_backward_workspace_bytes, B, N, "nomad_backward_workspace_bytes"))
        scratch = self._windows_scratch(demb_w.shape[0])
        dwav = torch.empty(B, N, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nomad_embed_windows_backward(self.ctx, wav.data_ptr(), B, N, win, hop, _ptr(hw), _ptr(hb), layers.data_ptr(),
                                                         saved.data_ptr(), saved.numel(), demb_w.data_ptr(), dwav.data_ptr(),
                                                         scratch.data_ptr(), scratch.numel(), ws.data_ptr(), ws.numel(),
                                                         self._stream()), "nomad_embed_windows_backward")
        return dwav

    def embed_windows_backward_ragged(self, batch, layers, saved, demb_w, win: int, hop: int, head=None) -> torch.Tensor:
        """d loss / d wav (B, stride) of an ``embed_train_windows_ragged`` call (``batch``: its last result) from d loss / d emb_w
        (W_total,256); zero behind every clip's length."""
        win, hop, hw, hb = self._check_grad_windows(win, hop, head)
        buf, lens = batch
        B, stride = buf.shape
        self._check_demb_w(demb_w, sum(num_windows(num_frames(n), win, hop) for n in lens))
        self.enable_backward()
        ws = self._workspace(self._size_ragged(self.lib.nomad_backward_workspace_bytes_ragged, lens,
                                               "nomad_backward_workspace_bytes_ragged"))
        scratch = self._windows_scratch(demb_w.shape[0])
        dwav = torch.empty(B, stride, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nomad_embed_windows_backward_ragged(self.ctx, buf.data_ptr(), B, stride, (C.c_int * B)(*lens), win, hop,
                                                                _ptr(hw), _ptr(hb), layers.data_ptr(), saved.data_ptr(),
                                                                saved.numel(), demb_w.data_ptr(), dwav.data_ptr(), scratch.data_ptr(),
                                                                scratch.numel(), ws.data_ptr(), ws.numel(), self._stream()),
                   "nomad_embed_windows_backward_ragged")
        return dwav

    # ---- the span head on the gradient path ------------------------------------------------------------------------------------
    def embed_train_spans_ragged(self, waves, table, lengths=None, head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """``embed_train_ragged`` with the span head of ``embed_spans_ragged`` as its last stage: -> (emb (R,256), packed layers
        (12,M,768), saved block, (buffer, lengths)); the last item is the batch ``embed_spans_backward_ragged`` takes.  Rows, spans
        and the table as in ``embed_spans_ragged``: a row pools the concatenation of its spans' frames as if they were a clip of
        their own, and the encoder saw the whole clip."""
        hw, hb = self._check_head(head)
        buf, lens = self.pack_ragged(waves, lengths)
        frames = [num_frames(n) for n in lens]
        if min(frames) < 1:
            raise ValueError(f"a clip of {min(lens)} samples is shorter than the conv stack's receptive field")
        table = self._check_table(table, frames)
        self.enable_backward()
        B, stride = buf.shape
        R, row_clip, row_ptr, spans = self._table_args(table)
        emb = torch.empty(R, 256, dtype=torch.float32, device=self.device)
        layers = torch.empty(12, sum(frames), 768, dtype=torch.float32, device=self.device)
        saved = torch.empty(self._size_ragged(self.lib.nomad_saved_bytes_ragged, lens, "nomad_saved_bytes_ragged"),
                            dtype=torch.uint8, device=self.device)
        ws = self._workspace(self._size_ragged(self.lib.nomad_workspace_bytes_ragged, lens, "nomad_workspace_bytes_ragged"))
        scratch = self._spans_scratch(B, table, False)
        _lib.check(self.lib.nomad_embed_train_spans_ragged(self.ctx, buf.data_ptr(), B, stride, (C.c_int * B)(*lens), R, row_clip,
                                                           row_ptr, spans, _ptr(hw), _ptr(hb), emb.data_ptr(), layers.data_ptr(),
                                                           saved.data_ptr(), saved.numel(), scratch.data_ptr(), scratch.numel(),
                                                           ws.data_ptr(), ws.numel(), self._stream()),
                   "nomad_embed_train_spans_ragged")
        return emb, layers, saved, (buf, lens)

    def embed_spans_backward_ragged(self, batch, layers, saved, demb_r, table, head=None) -> torch.Tensor:
        """d loss / d wav (B, stride) of an ``embed_train_spans_ragged`` call (``batch``: its last result, ``table``: its table) from
        d loss / d emb (R,256); zero behind every clip's length, and all zero for a clip without a row."""
        hw, hb = self._check_head(head)
        buf, lens = batch
        B, stride = buf.shape
        table = self._check_table(table, [num_frames(n) for n in lens])
        R, row_clip, row_ptr, spans = self._table_args(table)
        self._check_dev(demb_r, "demb_r")
        if tuple(demb_r.shape) != (R, 256):
            raise ValueError(f"demb_r must be ({R}, 256): one row per row of the table, got {tuple(demb_r.shape)}")
        self.enable_backward()
        ws = self._workspace(self._size_ragged(self.lib.nomad_backward_workspace_bytes_ragged, lens,
                                               "nomad_backward_workspace_bytes_ragged"))
        scratch = self._spans_scratch(B, table, True)
        dwav = torch.empty(B, stride, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nomad_embed_spans_backward_ragged(self.ctx, buf.data_ptr(), B, stride, (C.c_int * B)(*lens), R, row_clip,
                                                              row_ptr, spans, _ptr(hw), _ptr(hb), layers.data_ptr(), saved.data_ptr(),
                                                              saved.numel(), demb_r.data_ptr(), dwav.data_ptr(), scratch.data_ptr(),
                                                              scratch.numel(), ws.data_ptr(), ws.numel(), self._stream()),
                   "nomad_embed_spans_backward_ragged")
        return dwav

    def train_backward_ragged(self, batch, layers: torch.Tensor, saved: torch.Tensor, demb: torch.Tensor):
        """Accumulate d loss / d parameters for one ``embed_train_ragged`` call, given d loss / d emb (B,256)."""
        buf, lens = batch
        self._check_dev(demb, "demb")
        B, stride = buf.shape
        ws = self._workspace(self._size_ragged(self.lib.nomad_train_workspace_bytes_ragged, lens,
                                               "nomad_train_workspace_bytes_ragged"))
        _lib.check(self.lib.nomad_train_backward_ragged(self.ctx, buf.data_ptr(), B, stride, (C.c_int * B)(*lens),
                                                        layers.data_ptr(), saved.data_ptr(), saved.numel(), demb.data_ptr(),
                                                        ws.data_ptr(), ws.numel(), self._stream()),
                   "nomad_train_backward_ragged")

    # ---- triplet fine-tuning step (train_triplet.py:112-133) ---------------------------------------
    @property
    def train_enabled(self) -> bool:
        """True once ``train_enable`` has allocated the master parameters, gradients and Adam moments (scoring and the
        evaluation experiments never do)."""
        return self._train_segments is not None

    def train_enable(self):
        """Allocate master parameters / gradients / Adam moments and re-point the engine at them."""
        if self._train_segments is not None:
            return
        w, keep = _weights_struct(self._state_dict)
        _lib.check(self.lib.nomad_train_enable(self.ctx, C.byref(w)), "nomad_train_enable")
        del keep
        segs = []
        name = C.create_string_buffer(128)
        off, cnt = C.c_size_t(), C.c_size_t()
        for i in range(self.lib.nomad_train_num_segments()):
            _lib.check(self.lib.nomad_train_segment(i, name, 128, C.byref(off), C.byref(cnt)), "nomad_train_segment")
            segs.append((name.value.decode(), off.value, cnt.value))
        self._train_segments = segs

    def train_segments(self):
        """[(checkpoint key, offset, count)] of the flat parameter vector."""
        self.train_enable()
        return list(self._train_segments)

    def train_param_count(self) -> Tuple[int, int]:
        total, head = C.c_size_t(), C.c_size_t()
        _lib.check(self.lib.nomad_train_param_count(C.byref(total), C.byref(head)), "nomad_train_param_count")
        return total.value, head.value

    def train_zero_grad(self):
        _lib.check(self.lib.nomad_train_zero_grad(self.ctx, self._stream()), "nomad_train_zero_grad")

    def train_backward(self, wav: torch.Tensor, layers: torch.Tensor, saved: torch.Tensor, demb: torch.Tensor):
        """Accumulate d loss / d parameters for one embed_train call, given d loss / d emb (B,256)."""
        if wav.dim() == 3:
            wav = wav.squeeze(1)
        self._check_dev(wav, "wav")
        self._check_dev(demb, "demb")
        B, N = wav.shape
        ws = self._workspace(self._size(self.lib.nomad_train_workspace_bytes, B, N, "nomad_train_workspace_bytes"))
        _lib.check(self.lib.nomad_train_backward(self.ctx, wav.data_ptr(), B, N, layers.data_ptr(), saved.data_ptr(),
                                                 saved.numel(), demb.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 self._stream()), "nomad_train_backward")

    def triplet_loss(self, a: torch.Tensor, p: torch.Tensor, n: torch.Tensor, margin: float, want_grad: bool = True):
        """nn.TripletMarginLoss(margin) -> (loss (1,), da, dp, dn) (gradients None when want_grad=False)."""
        for t, nm in ((a, "a"), (p, "p"), (n, "n")):
            self._check_dev(t, nm)
        B = a.shape[0]
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        da, dp, dn = (torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)) if want_grad else (None, None, None)
        _lib.check(self.lib.nomad_triplet_loss(self.ctx, a.data_ptr(), p.data_ptr(), n.data_ptr(), B, float(margin),
                                               loss.data_ptr(), _ptr(da), _ptr(dp), _ptr(dn), self._stream()), "nomad_triplet_loss")
        return loss, da, dp, dn

    def adam_step(self, lr_body: float, lr_head: float, betas=(0.9, 0.999), eps: float = 1e-8):
        _lib.check(self.lib.nomad_train_adam_step(self.ctx, float(lr_body), float(lr_head), float(betas[0]),
                                                  float(betas[1]), float(eps), self._stream()), "nomad_train_adam_step")

    def train_read(self, what: int = 0) -> torch.Tensor:
        """Flat copy of: 0 parameters, 1 gradients, 2 Adam exp_avg, 3 Adam exp_avg_sq."""
        total, _ = self.train_param_count()
        out = torch.empty(total, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nomad_train_read(self.ctx, what, out.data_ptr(), self._stream()), "nomad_train_read")
        return out

    def train_write(self, what: int, flat: torch.Tensor):
        self._check_dev(flat, "flat")
        total, _ = self.train_param_count()
        if flat.numel() != total:
            raise ValueError(f"expected {total} floats, got {flat.numel()}")
        _lib.check(self.lib.nomad_train_write(self.ctx, what, flat.data_ptr(), self._stream()), "nomad_train_write")

    def train_set_stochastic(self, dropout: float = 0.0, attention_dropout: float = 0.0, dropout_input: float = 0.0,
                             seed: int = 0, layer_mask: int = 0xFFF):
        """model.train() regularisation for the following embed_train / train_backward calls (defaults = eval)."""
        _lib.check(self.lib.nomad_train_set_stochastic(self.ctx, float(dropout), float(attention_dropout),
                                                       float(dropout_input), int(seed) & (2 ** 64 - 1),
                                                       int(layer_mask) & 0xFFF), "nomad_train_set_stochastic")
        # (what GraphedLoss asks: a captured graph freezes the dropout masks and the step counter of its capture)
        self.stochastic = bool(dropout > 0 or attention_dropout > 0 or dropout_input > 0 or (int(layer_mask) & 0xFFF) != 0xFFF)

    def train_set_branches(self, layer_masks=None):
        """The following training batches are len(layer_masks) equal groups of clips, each with its own LayerDrop
        mask (None: back to one group using train_set_stochastic's layer_mask)."""
        self.stochastic_branches = bool(layer_masks) and any((int(m) & 0xFFF) != 0xFFF for m in layer_masks)
        if not layer_masks:
            _lib.check(self.lib.nomad_train_set_branches(self.ctx, 1, None), "nomad_train_set_branches")
            return
        arr = (C.c_uint * len(layer_masks))(*[int(m) & 0xFFF for m in layer_masks])
        _lib.check(self.lib.nomad_train_set_branches(self.ctx, len(layer_masks), arr), "nomad_train_set_branches")

    def train_set_frozen(self, freeze_encoder: bool):
        """``freeze_all: True`` of the reference's config: no parameter gradients for the encoder (nor the extractor);
        post_extract_proj, the feature LayerNorm and the head keep training."""
        _lib.check(self.lib.nomad_train_set_frozen(self.ctx, int(bool(freeze_encoder))), "nomad_train_set_frozen")

    def train_set_convnet(self, trainable: bool):
        """``freeze_convnet: False`` of the reference's config: the conv feature extractor's weights and GroupNorm get
        gradients too (scaled by ``feature_grad_mult``, like everything that enters the extractor)."""
        _lib.check(self.lib.nomad_train_set_convnet(self.ctx, int(bool(trainable))), "nomad_train_set_convnet")

    def train_set_step(self, step: int):
        _lib.check(self.lib.nomad_train_set_step(self.ctx, int(step)), "nomad_train_set_step")

    def train_unflatten(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Flat vector -> {checkpoint key: CPU tensor in the checkpoint's shape}."""
        from .weights import expected_shapes
        shapes = expected_shapes()
        host = flat.detach().cpu()
        return {k: host[o:o + n].reshape(shapes[k]).clone() for k, o, n in self.train_segments()}

    def train_flatten(self, tensors: Dict[str, torch.Tensor], fill: Optional[float] = None) -> torch.Tensor:
        """{checkpoint key: tensor} -> flat device vector.  A key that is missing raises, unless ``fill`` gives the value
        its slice gets (e.g. 0.0 for gradient dicts that leave out frozen parameters)."""
        total, _ = self.train_param_count()
        host = torch.empty(total, dtype=torch.float32)
        for k, o, n in self.train_segments():
            if k not in tensors and fill is not None:
                host[o:o + n] = fill
            else:
                host[o:o + n] = tensors[k].detach().reshape(-1).to(torch.float32)
        return host.to(self.device)

    def train_state_dict(self) -> Dict[str, torch.Tensor]:
        """Full checkpoint-layout state dict with the current (fine-tuned) parameters (torch.save-able)."""
        sd = {k: v.detach().cpu().clone() for k, v in self._state_dict.items()}
        sd.update(self.train_unflatten(self.train_read(0)))
        return sd

    # ---- measurement -----------------------------------------------------------------------------
    def profile_enable(self, on: bool = True):
        _lib.check(self.lib.nomad_profile_enable(self.ctx, int(on)), "nomad_profile_enable")

    def profile_reset(self):
        _lib.check(self.lib.nomad_profile_reset(self.ctx), "nomad_profile_reset")

    def profile_read(self):
        ms = (C.c_double * _lib.K_COUNT)()
        n = (C.c_longlong * _lib.K_COUNT)()
        fl = (C.c_double * _lib.K_COUNT)()
        _lib.check(self.lib.nomad_profile_read(self.ctx, ms, n, fl), "nomad_profile_read")
        return {name: {"ms": ms[i], "launches": n[i], "flops": fl[i]}
                for i, name in enumerate(_lib.KERNEL_CLASS_NAMES)}

    # ---- diagnostics (tests) ---------------------------------------------------------------------
    def diag_clock_probe(self, ms: float, stream: "torch.cuda.Stream") -> torch.Tensor:
        """Launch the one-wave clock probe on `stream` for ~ms milliseconds; returns the (2,) int64 device tensor
        [shader cycles, 100 MHz ticks] (read it after synchronising)."""
        with torch.cuda.stream(stream):  # the zero fill must not queue behind the load on the main stream
            out = torch.zeros(2, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.nomad_diag_clock_probe(self.ctx, int(ms * 1e5), out.data_ptr(), stream.cuda_stream),
                   "nomad_diag_clock_probe")
        return out

    def diag_gemm(self, A, W, bias=None, R=None, gelu=False, tile=0):
        M, K = A.shape
        N = W.shape[0]
        out = torch.empty(M, N, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nomad_diag_gemm(self.ctx, A.data_ptr(), W.data_ptr(), _ptr(bias), _ptr(R), out.data_ptr(), M, N, K,
                                            int(gelu), tile, self._stream()), "nomad_diag_gemm")
        return out

    def diag_layernorm(self, x, gamma, beta):
        M, N = x.shape
        out = torch.empty_like(x)
        _lib.check(self.lib.nomad_diag_layernorm(self.ctx, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                 out.data_ptr(), M, N, self._stream()), "nomad_diag_layernorm")
        return out

    def diag_attention(self, qkv, B, T):
        out = torch.empty(B * T, 768, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nomad_diag_attention(self.ctx, qkv.data_ptr(), out.data_ptr(), B, T, self._stream()),
                   "nomad_diag_attention")
        return out

    def diag_layernorm_bwd(self, x, g, gamma):
        M, N = x.shape
        dx = torch.empty_like(x)
        _lib.check(self.lib.nomad_diag_layernorm_bwd(self.ctx, x.data_ptr(), g.data_ptr(), gamma.data_ptr(),
                                                     dx.data_ptr(), M, N, self._stream()), "nomad_diag_layernorm_bwd")
        return dx

    def diag_attention_bwd(self, qkv, dctx, B, T):
        out = torch.empty(B * T, 768, dtype=torch.float32, device=self.device)
        lse = torch.empty(B * 12, T, dtype=torch.float32, device=self.device)
        dqkv = torch.empty(B * T, 2304, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nomad_diag_attention_bwd(self.ctx, qkv.data_ptr(), dctx.data_ptr(), out.data_ptr(),
                                                     lse.data_ptr(), dqkv.data_ptr(), B, T, self._stream()),
                   "nomad_diag_attention_bwd")
        return out, lse, dqkv

    def diag_keep_intermediates(self, on: bool):
        _lib.check(self.lib.nomad_diag_keep_intermediates(self.ctx, int(on)), "nomad_diag_keep_intermediates")
        self._ws = None

    def diag_region(self, B: int, n_samples: int, name: str) -> torch.Tensor:
        """View (fp32, flat) of a named intermediate of the LAST embed() call with this (B, n_samples)."""
        off, nb = C.c_size_t(), C.c_size_t()
        _lib.check(self.lib.nomad_diag_workspace_region(self.ctx, B, n_samples, name.encode(), C.byref(off), C.byref(nb)),
                   "nomad_diag_workspace_region")
        return self._ws[off.value:off.value + nb.value].view(torch.float32)

    def diag_poison_scratch(self, byte: int = 0xFF):
        """Fill the context's own per-call scratch (split-K partials, pairwise blocks, weight-norm backward temporaries) with
        `byte` on the current stream (libnomad_diag.so only; nomad_diag_poison_scratch lists the buffers)."""
        fn = self.lib.nomad_diag_poison_scratch
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.check(fn(self.ctx, int(byte), self._stream()), "nomad_diag_poison_scratch")
