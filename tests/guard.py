"""Guarded buffers: every Engine call inside ``guarded()`` writes into allocations of exactly the size it asked for, with a
fixed byte pattern in front of and behind each, and the patterns are checked afterwards.  Imported by the tests like
``ref64``; not a test module itself.

* Workspaces: ``Engine._workspace`` is replaced, so every call gets a fresh block of exactly ``workspace_bytes`` (no cached
  block of an earlier, larger call whose slack would absorb an overflow), between two guards of ``WS_GUARD`` bytes each,
  4 x kSplitKPartFloats (4 x 512 x 64 x 64 floats) = 32 MiB: a split-K block written with partial products of the largest
  problem any split-K check admits still lands inside the allocation.  ``_ws`` / ``_ws_side[k]`` are set to the block as
  before, so ``diag_region`` reads the call's intermediates.
* Outputs: ``torch`` inside ``nomad_amd.engine`` is replaced by a stand-in (the mechanism of ``test_gpu_poison.py``) whose
  ``empty`` / ``empty_like`` put ``OUT_GUARD`` bytes on each side of every device tensor Engine allocates: emb, layers,
  saved, dwav, staging buffers, the l1 scratch.

The guards are filled on the current stream when they are allocated, so they are in place before any kernel of the call
runs.  ``check()`` synchronises and reports every guard whose bytes changed: which buffer, which side, how many bytes and the
first offset."""
from __future__ import annotations

import contextlib
from typing import List

import torch

PATTERN = 0xA7                     # a float32 of 0xA7A7A7A7 is -4.6e-15, a bfloat16 -4.6e-15: no kernel writes it by chance
WS_GUARD = 4 * (4 * 512 * 64 * 64)  # bytes: 4 x kSplitKPartFloats
OUT_GUARD = 1 << 16


class _Guarded:
    __slots__ = ("name", "buf", "pre", "nbytes", "post")

    def __init__(self, name, buf, pre, nbytes, post):
        self.name, self.buf, self.pre, self.nbytes, self.post = name, buf, pre, nbytes, post


class Guards:
    """The guarded allocations made so far; ``empty`` makes one, ``check`` verifies all of them."""

    def __init__(self):
        self.items: List[_Guarded] = []

    def empty_bytes(self, nbytes: int, device, guard: int, name: str) -> torch.Tensor:
        """A uint8 view of exactly ``nbytes`` bytes with ``guard`` pattern bytes on each side (guard: a multiple of 256, so
        the view keeps the allocation's alignment)."""
        assert guard % 256 == 0
        buf = torch.empty(guard + nbytes + guard, dtype=torch.uint8, device=device)
        buf[:guard].fill_(PATTERN)
        buf[guard + nbytes:].fill_(PATTERN)
        self.items.append(_Guarded(name, buf, guard, nbytes, guard))
        return buf[guard:guard + nbytes]

    def empty(self, shape, dtype=torch.float32, device=None, guard: int = OUT_GUARD, name: str = "tensor") -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        item = torch.empty((), dtype=dtype).element_size()
        return self.empty_bytes(n * item, device, guard, name).view(dtype).view(shape)

    def empty_at(self, shape, offset: int, dtype=torch.float32, device=None, guard: int = OUT_GUARD, name: str = "tensor") -> torch.Tensor:
        """``empty`` whose first element lies ``offset`` elements (0 .. 3) behind the allocation's own (at least 64-byte) boundary:
        with an offset of 1 or 3 floats the address is aligned to 4 bytes and nothing wider, with 2 to 8 bytes.  The ``offset``
        elements in front of it and the ``4 - offset`` behind it carry the pattern and are checked as part of the two guards."""
        assert 0 <= offset <= 3 and guard % 256 == 0
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        item = torch.empty((), dtype=dtype).element_size()
        pre, nbytes, post = guard + offset * item, n * item, guard + (4 - offset) * item
        buf = torch.empty(pre + nbytes + post, dtype=torch.uint8, device=device)
        buf[:pre].fill_(PATTERN)
        buf[pre + nbytes:].fill_(PATTERN)
        self.items.append(_Guarded(name, buf, pre, nbytes, post))
        out = buf[pre:pre + nbytes].view(dtype).view(shape)
        assert out.data_ptr() % 16 == offset * item % 16
        return out

    def damaged(self):
        """[(name, side, bytes changed, first changed offset within the guard)] over every guarded allocation."""
        if any(g.buf.is_cuda for g in self.items):
            torch.cuda.synchronize()
        out = []
        for g in self.items:
            for side, lo, hi in (("before", 0, g.pre), ("after", g.pre + g.nbytes, g.pre + g.nbytes + g.post)):
                bad = (g.buf[lo:hi] != PATTERN).nonzero()
                if bad.numel():
                    out.append((g.name, side, int(bad.numel()), int(bad[0])))
        return out

    def check(self, case: str = ""):
        bad = self.damaged()
        assert not bad, f"{case}: guard bytes overwritten: " + "; ".join(
            f"{name} {side} ({n} bytes, first at +{off})" for name, side, n, off in bad[:6])


class _GuardedTorch:
    """``torch`` as nomad_amd.engine sees it inside ``guarded()``: every device tensor it allocates sits between guards."""

    def __init__(self, guards: Guards):
        self._g = guards

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None, **kw):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        if device is None or torch.device(device).type != "cuda":
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._g.empty(size, dtype or torch.get_default_dtype(), device, name=f"empty{tuple(size)}")

    def empty_like(self, t, **kw):
        if kw or not t.is_cuda:
            return torch.empty_like(t, **kw)
        return self._g.empty(t.shape, t.dtype, t.device, name=f"empty_like{tuple(t.shape)}")


@contextlib.contextmanager
def guarded(check: bool = True, case: str = ""):
    """Run the body with guarded workspaces and outputs; yields the Guards (checked at the end unless check=False).

    Engines keep the last guarded workspace in ``_ws`` after the block (diag_region may read it); they allocate exact
    blocks again only inside another ``guarded()``."""
    from nomad_amd import engine as engine_mod
    guards = Guards()
    Engine = engine_mod.Engine
    real_ws, real_torch = Engine._workspace, engine_mod.torch

    def _workspace(self, nbytes: int, side=False):
        k = int(side)
        ws = guards.empty_bytes(int(nbytes), self.device, WS_GUARD, f"workspace[{k}] {nbytes} B")
        if k:
            self._ws_side[k] = ws
        else:
            self._ws = ws
        if ws.is_cuda:
            ws.record_stream(torch.cuda.current_stream(self.device))
        return ws

    Engine._workspace = _workspace
    engine_mod.torch = _GuardedTorch(guards)
    try:
        yield guards
    finally:
        Engine._workspace = real_ws
        engine_mod.torch = real_torch
    if check:
        guards.check(case)
