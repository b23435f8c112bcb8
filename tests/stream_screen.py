"""The stream-order screen: does a call do ALL of its device work on the caller's stream, in order, and is it done with the
caller's host arrays when it returns?  Imported by the tests like ``guard``; not a test module itself.

Nearly every GPU test runs on torch's default stream and reads its results through ``.cpu()``: a launch or a copy that strayed
onto another stream, or a missing ``wait_stream`` on the way to or from the engine's side stream, would pass all of them.  On a
caller's own stream - torch's pool streams do not synchronise with the legacy default stream - such a slip is a silent race.

``screen(eng, S, make, call, spin_ms)`` runs one call ``E = call(eng, inputs)`` like this:

1. Quiet, on the default stream: ``ref = E(real)`` and ``stale = E(decoy)`` - ``real`` and ``decoy`` are ``make(seed)`` for two
   seeds: dicts of device tensors of the same shapes, both valid input.  Synchronise.
2. On the stream ``S``, with no host synchronisation until the end: fill the input buffers with ``decoy``; hold ``S`` with
   ``Engine.diag_clock_probe`` (one wave that sleeps and polls the wall clock); BEHIND the spin copy ``real`` over the decoy and
   record an event; hold the engine's side stream with a longer probe of its own (``side="late"``: a part dispatched there
   finishes late, so a consumer that does not wait for it reads memory it has not written) or leave it free (``side="free"``: a
   part dispatched there without waiting for ``S`` starts at once and reads the decoy); call ``E``; note whether the event has
   completed (``held``: it has not - the whole of ``E`` was enqueued while its input was still the decoy); on ``S`` clone every
   output and overwrite the inputs with the decoy again; overwrite every host array that went through the C ABI during the call
   (``HostArrays``: the ctypes arrays Engine builds from the caller's lists) with other valid values.
3. Synchronise.  The clones, and the tensors ``E`` returned, must equal ``ref`` bit for bit - every path is documented as
   bit-reproducible, so there is no tolerance.  A mismatch that equals ``stale`` means the call read its input too early (ahead of
   the producer on ``S``) or the output was read before the call had written it (the memory still held an earlier call's
   result for the decoy); any other mismatch is a torn read, or a read after the caller had the buffer back.

Nothing here can fault: every buffer a mis-ordered read could touch holds valid waveforms, every replacement length is the shortest
legal clip, every replacement table is valid for such a clip, and nothing is poisoned.  A violation shows as wrong bits."""
from __future__ import annotations

import ctypes as C
import time
from typing import Callable, Dict, List, Optional, Sequence

import torch

from nomad_amd import _lib

MIN_CLIP = 400      # samples: one encoder frame, the shortest clip any entry point accepts

# Host arrays by entry point, in the order of their pointer arguments (include/nomad_hip.h); every other entry point that takes
# one takes the clips' lengths alone.
_ROLES = {
    "nomad_embed_spans_ragged": ("lens", "row_clip", "row_ptr", "spans"),
    "nomad_embed_train_spans_ragged": ("lens", "row_clip", "row_ptr", "spans"),
    "nomad_embed_spans_backward_ragged": ("lens", "row_clip", "row_ptr", "spans"),
    "nomad_degrade_noise": ("lens", "levels"),
    "nomad_degrade_clip": ("lens", "levels"),
    "nomad_degrade_convolve": ("lens", "ir_lens"),
    "nomad_l1_loss_weighted": ("frames", "weights"),
    "nomad_l1_loss_weighted_backward": ("frames", "weights"),
}
_HOST_ELEMENTS = (C.c_int, C.c_uint, C.c_float, C.c_double)


def _replacement(role: str, n: int) -> list:
    """Other VALID values for a host array of ``n`` entries: what a kernel may read, were it to read them, without leaving a buffer
    that was sized for the real ones (lengths and tap counts only shrink, tables name frame 0 of clip 0)."""
    return {"lens": [MIN_CLIP] * n, "frames": [1] * n, "ir_lens": [1] * n, "row_clip": [0] * n, "row_ptr": list(range(n)),
            "spans": [0, 1] * (n // 2) + [0] * (n % 2), "levels": [7.0] * n, "weights": [0.25] * n}[role]


class HostArrays:
    """Stands in for ``Engine.lib`` during a screened call: passes every call through and keeps each ctypes array that went into
    the C ABI, with its role, so that the screen can overwrite it once the call has returned."""

    def __init__(self, lib):
        self._lib = lib
        self.taken: List[tuple] = []      # (entry point, role, array)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        sig = _lib.SIGNATURES.get(name)
        if sig is None:
            return fn
        slots = [i for i, t in enumerate(sig[1]) if isinstance(t, type) and issubclass(t, C._Pointer) and t._type_ in _HOST_ELEMENTS]
        if not slots:
            return fn
        roles = _ROLES.get(name, ("lens",))

        def call(*args):
            for k, i in enumerate(slots):
                if i < len(args) and k < len(roles) and isinstance(args[i], C.Array):
                    self.taken.append((name, roles[k], args[i]))
            return fn(*args)

        return call

    def overwrite(self) -> int:
        """Every array taken so far gets its replacement values; -> how many were overwritten."""
        for _, role, arr in self.taken:
            arr[:] = _replacement(role, len(arr))
        return len(self.taken)


def _flat(outs) -> List[torch.Tensor]:
    if torch.is_tensor(outs):
        return [outs]
    return [t for t in outs if t is not None]


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8),
                                                                     b.contiguous().view(-1).view(torch.uint8))


def _row_bytes(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bytes, one row per entry of its first dimension (a 0-dim tensor: one row)."""
    t = t.contiguous()
    return t.view(t.shape[0] if t.dim() else 1, -1).view(torch.uint8)


def _rows_that_differ(a: torch.Tensor, b: torch.Tensor) -> list:
    return torch.nonzero((_row_bytes(a) != _row_bytes(b)).any(dim=1)).flatten().tolist()


class Report:
    """What one screened call showed.  ``held``: S was still held when the call returned; ``enqueue_ms``: host time of the call
    while S was held; ``host_arrays``: how many were overwritten after the return; ``problems``: one line per output that differs."""

    def __init__(self, name: str):
        self.name, self.held, self.enqueue_ms, self.quiet_ms, self.host_arrays = name, False, 0.0, 0.0, 0
        self.problems: List[str] = []

    def line(self) -> str:
        return (f"{self.name}: held={self.held} enqueue={self.enqueue_ms:.2f} ms (quiet {self.quiet_ms:.2f} ms) host arrays={self.host_arrays} "
                + ("ok" if not self.problems else "; ".join(self.problems)))


def _compare(rep: Report, what: str, got: Sequence[torch.Tensor], ref: Sequence[torch.Tensor], stale: Sequence[torch.Tensor], names):
    for i, (g, r, s) in enumerate(zip(got, ref, stale)):
        if _same_bits(g, r):
            continue
        rows = _rows_that_differ(g, r)
        idx = torch.tensor(rows, device=g.device)
        early = torch.equal(_row_bytes(g)[idx], _row_bytes(s)[idx])      # judged on the rows that differ: a split batch goes stale by halves
        kind = ("its rows that differ equal their STALE value: they were computed from the input of before the caller's copy, or are what "
                "an earlier call left in memory the call had not written yet" if early
                else "its rows that differ equal neither the reference nor the stale value: torn, or read too late")
        rep.problems.append(f"{what} output {names[i] if names else i} {tuple(g.shape)}: {kind}; rows {rows[:12]}{' ...' if len(rows) > 12 else ''} "
                            f"({len(rows)} of {g.shape[0] if g.dim() else 1})")


def screen(eng, S: "torch.cuda.Stream", make: Callable[[int], Dict[str, torch.Tensor]], call: Callable, spin_ms: float,
           name: str = "", side: Optional[str] = "late", names: Optional[Sequence[str]] = None, seeds=(101, 202),
           watch_abi: bool = True, held_call: Optional[Callable] = None) -> Report:
    """Screen ``call(eng, inputs) -> tensor or tuple of tensors`` (None entries are skipped) on the stream ``S`` as the module's
    docstring says.  eng: the engine whose clock probe holds S, whose side stream is held and whose C ABI calls are watched
    (watch_abi=False: a call that goes through another engine, or through none - the positive controls).
    side: "late" (the side stream is held for 1.5 spins) or "free" (it is not held).  held_call: what runs in step 2 in place of
    ``call`` (a variant of it that is broken on purpose: the quiet runs need the sound one)."""
    rep = Report(name)
    dev = S.device
    real, decoy = make(seeds[0]), make(seeds[1])
    assert sorted(real) == sorted(decoy) and all(real[k].shape == decoy[k].shape and real[k].dtype == decoy[k].dtype for k in real)
    bufs = {k: torch.empty_like(v) for k, v in real.items()}

    def load(src, quiet=False):
        for k in bufs:
            bufs[k].copy_(src[k])
        if quiet:      # (a quiet call sees its input whatever stream it reads it on)
            torch.cuda.synchronize(dev)

    # 1. quiet, on the default stream
    load(real, True)
    ref = [t.clone() for t in _flat(call(eng, bufs))]
    torch.cuda.synchronize(dev)
    load(decoy, True)
    stale = [t.clone() for t in _flat(call(eng, bufs))]
    torch.cuda.synchronize(dev)
    # once on S with nothing held: what the library binds to a launch stream at its first call there (the pairwise scratch) exists
    # before the held run, and the screen's premise - the same bits on every call - is checked on S itself.  On the DECOY: the
    # blocks this run frees are the ones the allocator hands to the held run's outputs, and what a consumer that does not wait
    # for its producer finds in them must not be the right answer.
    with torch.cuda.stream(S):
        load(decoy, True)
        t0 = time.perf_counter()
        again = _flat(call(eng, bufs))
        rep.quiet_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize(dev)
    for i, (a, r) in enumerate(zip(again, stale)):
        assert _same_bits(a, r), f"{name}: output {i} of a quiet call on S differs from the default stream's: the screen needs bit-identical calls"
    del again

    # 2. on S, behind a spin, with no host synchronisation
    watch = None
    if watch_abi:
        watch = HostArrays(eng.lib)
        eng.lib = watch
    try:
        with torch.cuda.stream(S):
            load(decoy)
            eng.diag_clock_probe(spin_ms, S)
            load(real)
            released = torch.cuda.Event()
            released.record(S)
            if side == "late":
                eng.diag_clock_probe(1.5 * spin_ms, eng.side_stream())
            t0 = time.perf_counter()
            outs = _flat((held_call or call)(eng, bufs))
            rep.enqueue_ms = (time.perf_counter() - t0) * 1e3
            rep.held = not released.query()
            clones = [t.clone() for t in outs]
            aliased = {v.data_ptr() for v in bufs.values()}
            load(decoy)
            if watch is not None:
                rep.host_arrays = watch.overwrite()
    finally:
        if watch is not None:
            eng.lib = watch._lib
    # 3.
    torch.cuda.synchronize(dev)
    assert len(clones) == len(ref) == len(stale)
    _compare(rep, "clone of", clones, ref, stale, names)
    keep = [i for i, t in enumerate(outs) if t.data_ptr() not in aliased]      # (an in-place output IS an input: it holds the decoy now)
    _compare(rep, "returned", [outs[i] for i in keep], [ref[i] for i in keep], [stale[i] for i in keep],
             [names[i] for i in keep] if names else keep)
    return rep
