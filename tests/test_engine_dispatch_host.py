"""CPU: the call sequence ``Engine`` issues for every dispatching entry point, pinned without a GPU.

``nomad_amd.engine.torch`` is replaced by a stand-in (the mechanism of ``guard.py`` / ``test_gpu_poison.py``) whose ``cuda``
namespace hands out fake streams, and the engine's ``lib`` by a fake that records every call: (function, the stream that was
current, arguments).  In the arguments ctypes int arrays are lists, and pointers are what they point at: ``ws_main`` /
``ws_side<k>``, a stream's name, or (tensor name, byte offset) - the offset shows which slice a part got.  A tensor the test
registered has the name it was registered under; one the engine allocated is ``new<shape>``.  Size queries (every ``*_bytes*``
function) are not recorded: they answer ``fake_size``, which depends on the function and on every integer argument, so the
workspace size in the recorded call shows which query was made with which geometry.  Besides the library calls the trace holds
``("wait", waiter, waited)``, ``("enter" / "exit", stream)`` of a ``torch.cuda.stream`` block and ``("alloc", stream, bytes)``
for every uint8 block (workspaces, saved activations) - the caching allocator ties a block to the stream current when it is
allocated, so the side part's workspace has to be made inside the side stream's block.

The expected traces below are written from the documented behaviour (who splits, where, who announces it through
``nomad_set_concurrent_parts``), not recorded from the code.
"""
import contextlib
import ctypes as C

import pytest
import torch

from nomad_amd import _lib
from nomad_amd import engine as engine_mod
from nomad_amd.weights import num_frames

MAIN_ID, F4 = 0x57000000, 4
N4S = 64000      # 4 s: T = 199


def fake_size(fn: str, *ints) -> int:
    return 1000 * len(fn) + sum(int(i) for i in ints)


class _Stream:
    def __init__(self, h, name, ident):
        self._h, self.name, self.cuda_stream = h, name, ident

    def wait_stream(self, other):
        self._h.trace.append(("wait", self.name, other.name))


class _Cuda:
    def __init__(self, h):
        self._h = h

    def __getattr__(self, name):
        return getattr(torch.cuda, name)

    def Stream(self, device=None):
        k = len(self._h.streams)
        st = _Stream(self._h, f"side{k}", MAIN_ID + k)
        self._h.streams.append(st)
        return st

    def current_stream(self, device=None):
        return self._h.current

    @contextlib.contextmanager
    def stream(self, st):
        prev, self._h.current = self._h.current, st
        self._h.trace.append(("enter", st.name))
        try:
            yield
        finally:
            self._h.current = prev
            self._h.trace.append(("exit", st.name))


class _Harness:
    """The stand-in ``torch``: trace, streams, named tensors.  Everything it does not define is the real ``torch``."""

    def __init__(self):
        self.trace, self.named = [], []
        self.streams = [_Stream(self, "main", MAIN_ID)]
        self.current = self.streams[0]
        self.cuda = _Cuda(self)

    def __getattr__(self, name):
        return getattr(torch, name)

    def reg(self, name, t):
        self.named.append((name, t))
        return t

    def empty(self, *size, **kw):
        kw.pop("pin_memory", None)
        t = torch.empty(*size, **kw)
        if t.dtype == torch.uint8:
            self.trace.append(("alloc", self.current.name, t.numel()))
        return self.reg(f"new{tuple(t.shape)}", t)

    def empty_like(self, t, **kw):
        return self.reg(f"new{tuple(t.shape)}", torch.empty_like(t, **kw))


class _FakeLib:
    def __init__(self, h, eng):
        self._h, self._eng = h, eng

    def _arg(self, a):
        if isinstance(a, C.Array):
            return list(a)
        if not isinstance(a, int) or isinstance(a, bool):
            return a
        for st in self._h.streams:
            if a == st.cuda_stream:
                return st.name
        blocks = [("ws_main", self._eng._ws)] + [(f"ws_side{k}", t) for k, t in self._eng._ws_side.items()] + self._h.named
        for name, t in blocks:
            if t is not None and t.data_ptr() <= a < t.data_ptr() + max(1, t.numel() * t.element_size()):
                off = a - t.data_ptr()
                return name if name.startswith("ws_") and off == 0 else (name, off)
        return a

    def __getattr__(self, fn):
        def call(*args):
            if fn == "nomad_num_frames":
                return num_frames(args[0])
            args = [a for a in args if a is not self._eng.ctx]
            if "_bytes" in fn:
                ints = [x for a in args[:-1] for x in (list(a) if isinstance(a, C.Array) else [a])]
                args[-1]._obj.value = fake_size(fn, *ints)
                return 0
            self._h.trace.append((fn, self._h.current.name, [self._arg(a) for a in args]))
            return 0
        return call


class _TraceEngine(engine_mod.Engine):
    def __init__(self, h):
        self.device, self.device_index = torch.device("cpu"), 0
        self.ctx = object()
        self._ws, self._ws_side, self._side_streams = None, {}, {}
        self._l1_scratch = self._l1w_scratch = self._train_segments = None
        self.lib = _FakeLib(h, self)

    def close(self):
        pass

    def _check_dev(self, t, name):
        if not (t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous fp32 tensor")


@pytest.fixture
def rig(monkeypatch):
    h = _Harness()
    monkeypatch.setattr(engine_mod, "torch", h)
    return h, _TraceEngine(h)


# ---- the rows of the expected tables ----------------------------------------------------------------------------------------
def _st(side):
    return "side1" if side else "main"


def _ws(side):
    return "ws_side1" if side else "ws_main"


def two_streams(side_rows, main_rows):
    """wait, the second part inside the side stream's block, the first part on the caller's stream, wait."""
    return [("wait", "side1", "main"), ("enter", "side1"), *side_rows, ("exit", "side1"), *main_rows, ("wait", "main", "side1")]


def hint(n):
    return [("nomad_set_concurrent_parts", "main", [n])]


def enable(what):
    return [(f"nomad_enable_{what}", "main", [])]


def ws_rows(size, on_side_stream):
    return [("alloc", _st(on_side_stream), size)]


SIZE_FN = {"fp32": "nomad_workspace_bytes", "bf16": "nomad_workspace_bytes_bf16", "bf16x3": "nomad_workspace_bytes_bf16x3"}
SIZE_FN_RAGGED = {p: f.replace("bytes", "bytes_ragged") for p, f in SIZE_FN.items()}


def embed_part(B, N, lo, hi, side=False, stream_side=None, head=(None, None), layers=None):
    """Rows lo..hi-1 of a (B,N) batch through nomad_embed; side: the workspace, stream_side: the stream (default: the same)."""
    ss = side if stream_side is None else stream_side
    size = fake_size("nomad_workspace_bytes", hi - lo, N)
    return ws_rows(size, ss) + [("nomad_embed", _st(ss), [("wav", lo * N * F4), hi - lo, N, *head, (f"new({B}, 256)", lo * 256 * F4), layers,
                                                      _ws(side), size, _st(ss)])]


def plain_part(fn, precision, B, N, lo, hi, side=False, stream_side=None):
    """nomad_embed_bf16 / nomad_embed_bf16x3: (wav, b, N, emb, ws, bytes, stream)."""
    ss = side if stream_side is None else stream_side
    size = fake_size(SIZE_FN[precision], hi - lo, N)
    return ws_rows(size, ss) + [(fn, _st(ss), [("wav", lo * N * F4), hi - lo, N, (f"new({B}, 256)", lo * 256 * F4), _ws(side), size, _st(ss)])]


def features_part(precision, B, N, lo, hi, side=False):
    size = fake_size(SIZE_FN[precision], hi - lo, N)
    return ws_rows(size, side) + [("nomad_embed_features", _st(side), [("wav", lo * N * F4), hi - lo, N, _lib.PRECISION[precision],
                                                                       (f"new({B}, 768)", lo * 768 * F4), _ws(side), size, _st(side)])]


def ragged_part(kind, precision, buf, lens, lo, hi, side=False):
    """Clips lo..hi-1 of a packed batch: their own length array, their own size query."""
    B, stride, part = len(lens), (max(lens) + 3) // 4 * 4, lens[lo:hi]
    size = fake_size(SIZE_FN_RAGGED[precision], hi - lo, *part)
    src, tail = (buf, lo * stride * F4), [_ws(side), size, _st(side)]
    if kind == "features":
        args = [src, hi - lo, stride, part, _lib.PRECISION[precision], (f"new({B}, 768)", lo * 768 * F4), *tail]
        return ws_rows(size, side) + [("nomad_embed_features_ragged", _st(side), args)]
    dst = (f"new({B}, 256)", lo * 256 * F4)
    if precision == "fp32":
        return ws_rows(size, side) + [("nomad_embed_ragged", _st(side), [src, hi - lo, stride, part, None, None, dst, *tail])]
    return ws_rows(size, side) + [(f"nomad_embed_ragged_{precision}", _st(side), [src, hi - lo, stride, part, dst, *tail])]


def _wav(h, B, N):
    return h.reg("wav", torch.zeros(B, N))


def _zero_thresholds(eng):
    eng.F32_SPLIT_ROWS = eng.BF16_SPLIT_ROWS = eng.X3_SPLIT_ROWS = 0   # as bench.py's roofline pass sets them


# ---- embed ------------------------------------------------------------------------------------------------------------------
def test_embed_small_batch_is_one_call_with_hint_1(rig):
    h, eng = rig
    eng.embed(_wav(h, 3, N4S))
    assert h.trace == hint(1) + embed_part(3, N4S, 0, 3)


def test_embed_splits_from_4000_frames(rig):
    h, eng = rig
    assert 21 * num_frames(N4S) >= 4000 > 20 * num_frames(N4S)
    eng.embed(_wav(h, 21, N4S))
    assert h.trace == hint(2) + two_streams(embed_part(21, N4S, 10, 21, side=True), embed_part(21, N4S, 0, 10))


def test_embed_below_the_threshold_and_with_thresholds_zero(rig):
    h, eng = rig
    eng.embed(_wav(h, 20, N4S))
    assert h.trace == hint(1) + embed_part(20, N4S, 0, 20)
    h2 = _Harness()
    engine_mod.torch = h2          # (monkeypatch restores the module's torch at the end of the test)
    eng2 = _TraceEngine(h2)
    _zero_thresholds(eng2)
    eng2.embed(_wav(h2, 21, N4S))
    assert h2.trace == hint(1) + embed_part(21, N4S, 0, 21)


def test_embed_want_layers_never_splits(rig):
    h, eng = rig
    hw, hb = h.reg("hw", torch.zeros(256, 768)), h.reg("hb", torch.zeros(256))
    emb, layers = eng.embed(_wav(h, 21, N4S), head=(hw, hb), want_layers=True)
    assert layers.shape == (12, 21, 199, 768)
    assert h.trace == hint(1) + embed_part(21, N4S, 0, 21, head=(("hw", 0), ("hb", 0)), layers=("new(12, 21, 199, 768)", 0))


def test_embed_side_has_no_hint_and_the_side_workspace(rig):
    h, eng = rig
    eng.embed(_wav(h, 21, N4S), side=True)
    assert h.trace == embed_part(21, N4S, 0, 21, side=True, stream_side=False)


def test_embed_side_k_names_the_workspace_of_side_stream_k(rig):
    """(tests/test_gpu_race_screen.py runs three layer-output forwards on three streams with side = 0, 1, 2)"""
    h, eng = rig
    eng.embed(_wav(h, 3, N4S), want_layers=True, side=2)
    size = fake_size("nomad_workspace_bytes", 3, N4S)
    assert h.trace == [("alloc", "main", size),
                       ("nomad_embed", "main", [("wav", 0), 3, N4S, None, None, ("new(3, 256)", 0), ("new(12, 3, 199, 768)", 0),
                                                "ws_side2", size, "main"])]


# ---- embed_bf16 / embed_bf16x3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,split", [(3, False), (21, True), (21, None)], ids=["small", "split", "thresholds0"])
def test_embed_bf16(rig, B, split):
    h, eng = rig
    if split is None:
        _zero_thresholds(eng)
    eng.embed_bf16(_wav(h, B, N4S))
    part = lambda lo, hi, side=False: plain_part("nomad_embed_bf16", "bf16", B, N4S, lo, hi, side)   # noqa: E731
    if split:
        assert h.trace == enable("bf16") + hint(2) + two_streams(part(10, 21, True), part(0, 10))
    else:
        assert h.trace == enable("bf16") + hint(1) + part(0, B)


@pytest.mark.parametrize("B,split", [(3, False), (21, True), (21, None)], ids=["small", "split", "thresholds0"])
def test_embed_bf16x3_never_touches_the_hint(rig, B, split):
    h, eng = rig
    if split is None:
        _zero_thresholds(eng)
    eng.embed_bf16x3(_wav(h, B, N4S))
    part = lambda lo, hi, side=False: plain_part("nomad_embed_bf16x3", "bf16x3", B, N4S, lo, hi, side)   # noqa: E731
    if split:
        assert h.trace == enable("bf16x3") + two_streams(part(10, 21, True), part(0, 10))
    else:
        assert h.trace == enable("bf16x3") + part(0, B)


def test_embed_bf16x3_side(rig):
    h, eng = rig
    eng.embed_bf16x3(_wav(h, 21, N4S), side=True)
    assert h.trace == enable("bf16x3") + plain_part("nomad_embed_bf16x3", "bf16x3", 21, N4S, 0, 21, side=True, stream_side=False)


@pytest.mark.parametrize("side", [False, True], ids=["main", "side"])
def test_embed_bf16x3_layers_and_head_never_split(rig, side):
    h, eng = rig
    hw, hb = h.reg("hw", torch.zeros(256, 768)), h.reg("hb", torch.zeros(256))
    eng.embed_bf16x3(_wav(h, 21, N4S), head=(hw, hb), want_layers=True, side=side)
    size = fake_size("nomad_workspace_bytes_bf16x3", 21, N4S)
    assert h.trace == enable("bf16x3") + ws_rows(size, False) + [
        ("nomad_embed_layers_bf16x3", "main", [("wav", 0), 21, N4S, ("hw", 0), ("hb", 0), ("new(21, 256)", 0),
                                               ("new(12, 21, 199, 768)", 0), _ws(side), size, "main"])]


# ---- embed_features -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,split", [(3, False), (21, True), (21, None)], ids=["small", "split", "thresholds0"])
@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_embed_features(rig, precision, B, split):
    h, eng = rig
    if split is None:
        _zero_thresholds(eng)
    eng.embed_features(_wav(h, B, N4S), precision=precision)
    pre = enable(precision) if precision != "fp32" else []
    if split:
        assert h.trace == pre + hint(2) + two_streams(features_part(precision, B, N4S, B // 2, B, True),
                                                      features_part(precision, B, N4S, 0, B // 2))
    else:
        assert h.trace == pre + hint(1) + features_part(precision, B, N4S, 0, B)


# ---- ragged forwards ----------------------------------------------------------------------------------------------------------
# 4169 frames; half of the 1 344 401 samples is passed inside clip 11, so clips 0..11 are the first part and 12..32 the second
RAGGED_LENS = [N4S] * 10 + [32000] * 22 + [401]
SMALL_LENS = [401, 720, 20560]


def _call_ragged(eng, kind, waves, precision, packed=None):
    if kind == "features":
        return eng.embed_features_ragged(waves, precision=precision, packed=packed)
    return eng.embed_ragged(waves, precision=precision, packed=packed)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("kind", ["embed", "features"])
def test_ragged_splits_by_audio_length_without_a_hint(rig, kind, precision):
    h, eng = rig
    assert sum(num_frames(n) for n in RAGGED_LENS) == 4169
    _call_ragged(eng, kind, [torch.zeros(n) for n in RAGGED_LENS], precision)
    pre = enable(precision) if precision != "fp32" else []
    buf = "new(33, 64000)"
    assert h.trace == pre + two_streams(ragged_part(kind, precision, buf, RAGGED_LENS, 12, 33, True),
                                        ragged_part(kind, precision, buf, RAGGED_LENS, 0, 12))


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("kind", ["embed", "features"])
def test_ragged_small_list_and_thresholds_zero(rig, kind, precision):
    h, eng = rig
    _call_ragged(eng, kind, [torch.zeros(1, n) for n in SMALL_LENS], precision)
    pre = enable(precision) if precision != "fp32" else []
    assert h.trace == pre + ragged_part(kind, precision, "new(3, 20560)", SMALL_LENS, 0, 3)
    del h.trace[:]
    _zero_thresholds(eng)
    eng._ws = None
    _call_ragged(eng, kind, [torch.zeros(n) for n in RAGGED_LENS], precision)
    assert h.trace == pre + ragged_part(kind, precision, "new(33, 64000)", RAGGED_LENS, 0, 33)


@pytest.mark.parametrize("kind", ["embed", "features"])
def test_ragged_packed_staging_is_used_as_it_is(rig, kind):
    h, eng = rig
    host, lens = eng.pack_ragged_host([torch.full((n,), float(i)) for i, n in enumerate(RAGGED_LENS)])
    assert lens == RAGGED_LENS and host.shape == (33, 64000) and float(host[32, 400]) == 32.0 and float(host[11, 31999]) == 11.0
    del h.named[:]
    h.reg("staged", host)
    _call_ragged(eng, kind, None, "fp32", packed=(host, lens))
    assert h.trace == two_streams(ragged_part(kind, "fp32", "staged", RAGGED_LENS, 12, 33, True),
                                  ragged_part(kind, "fp32", "staged", RAGGED_LENS, 0, 12))


def test_ragged_stride_is_rounded_to_4_and_one_long_clip_leads(rig):
    """The cut never leaves a part empty: a first clip longer than all the rest is a part of its own."""
    h, eng = rig
    eng.X3_SPLIT_ROWS = 100
    lens = [N4S + 1, 401, 402]
    eng.embed_ragged([torch.zeros(n) for n in lens], precision="bf16x3")
    buf = "new(3, 64004)"
    assert h.trace == enable("bf16x3") + two_streams(ragged_part("embed", "bf16x3", buf, lens, 1, 3, True),
                                                     ragged_part("embed", "bf16x3", buf, lens, 0, 1))


def test_ragged_head_override(rig):
    h, eng = rig
    hw, hb = h.reg("hw", torch.zeros(256, 768)), h.reg("hb", torch.zeros(256))
    eng.embed_ragged([torch.zeros(n) for n in SMALL_LENS], head=(hw, hb))
    size = fake_size("nomad_workspace_bytes_ragged", 3, *SMALL_LENS)
    assert h.trace == ws_rows(size, False) + [("nomad_embed_ragged", "main", [("new(3, 20560)", 0), 3, 20560, SMALL_LENS, ("hw", 0), ("hb", 0),
                                                                              ("new(3, 256)", 0), "ws_main", size, "main"])]
    with pytest.raises(ValueError):
        eng.embed_ragged([torch.zeros(400)], head=(hw, hb), precision="bf16")


# ---- the gradient paths ---------------------------------------------------------------------------------------------------------
def test_pack_ragged_both_inputs(rig):
    h, eng = rig
    clips = [torch.full((1, n), float(i + 1)) for i, n in enumerate(SMALL_LENS)]
    buf, lens = eng.pack_ragged(clips)
    assert lens == SMALL_LENS and buf.shape == (3, 20560) and buf.dtype == torch.float32
    assert all(bool((buf[i, :n] == i + 1).all()) for i, n in enumerate(SMALL_LENS))
    buf, lens = eng.pack_ragged([torch.zeros(401), torch.zeros(402)])
    assert buf.shape == (2, 404)
    padded = torch.zeros(3, 1, 20560)
    buf, lens = eng.pack_ragged(padded, torch.tensor(SMALL_LENS))
    assert lens == SMALL_LENS and buf.shape == (3, 20560) and buf.data_ptr() == padded.data_ptr()
    with pytest.raises(ValueError):
        eng.pack_ragged(padded, [401, 720])
    with pytest.raises(ValueError):
        eng.pack_ragged(padded, [401, 720, 20561])
    assert h.trace == []


def _ragged_batch(h):
    return h.reg("wav", torch.zeros(3, 20560)), SMALL_LENS


def test_embed_train_ragged(rig):
    h, eng = rig
    wav, lens = _ragged_batch(h)
    M = sum(num_frames(n) for n in lens)
    emb, layers, saved, batch = eng.embed_train_ragged(wav, lens)
    assert layers.shape == (12, M, 768) and batch[0] is wav and batch[1] == lens
    nsaved, size = fake_size("nomad_saved_bytes_ragged", 3, *lens), fake_size("nomad_workspace_bytes_ragged", 3, *lens)
    assert h.trace == enable("backward") + [("alloc", "main", nsaved), ("alloc", "main", size)] + [
        ("nomad_embed_train_ragged", "main", [("wav", 0), 3, 20560, lens, None, None, ("new(3, 256)", 0), (f"new(12, {M}, 768)", 0),
                                              (f"new({nsaved},)", 0), nsaved, "ws_main", size, "main"])]


def test_embed_train_ragged_layer_outputs_only_on_the_side_workspace(rig):
    h, eng = rig
    wav, lens = _ragged_batch(h)
    hw, hb = h.reg("hw", torch.zeros(256, 768)), h.reg("hb", torch.zeros(256))
    M = sum(num_frames(n) for n in lens)
    _, _, saved, _ = eng.embed_train_ragged(wav, lens, head=(hw, hb), save=False, side=True)
    assert saved is None
    size = fake_size("nomad_workspace_bytes_ragged", 3, *lens)
    assert h.trace == [("alloc", "main", size),
                       ("nomad_embed_train_ragged", "main", [("wav", 0), 3, 20560, lens, ("hw", 0), ("hb", 0), ("new(3, 256)", 0),
                                                             (f"new(12, {M}, 768)", 0), None, 0, "ws_side1", size, "main"])]


def test_backward_ragged_calls(rig):
    h, eng = rig
    wav, lens = _ragged_batch(h)
    M = sum(num_frames(n) for n in lens)
    layers, saved = h.reg("layers", torch.zeros(12, M, 768)), h.reg("saved", torch.zeros(77, dtype=torch.uint8))
    dl, de = h.reg("dl", torch.zeros(12, M, 768)), h.reg("de", torch.zeros(3, 256))
    dwav = eng.embed_backward_ragged((wav, lens), layers, saved, dl, None)
    assert dwav.shape == (3, 20560)
    size = fake_size("nomad_backward_workspace_bytes_ragged", 3, *lens)
    assert h.trace == enable("backward") + [("alloc", "main", size)] + [
        ("nomad_embed_backward_ragged", "main", [("wav", 0), 3, 20560, lens, None, None, ("layers", 0), ("saved", 0), 77, ("dl", 0), None,
                                                 ("new(3, 20560)", 0), "ws_main", size, "main"])]
    del h.trace[:]
    eng._ws = None
    eng.train_backward_ragged((wav, lens), layers, saved, de)
    size = fake_size("nomad_train_workspace_bytes_ragged", 3, *lens)
    assert h.trace == [("alloc", "main", size),
                       ("nomad_train_backward_ragged", "main", [("wav", 0), 3, 20560, lens, ("layers", 0), ("saved", 0), 77, ("de", 0),
                                                                "ws_main", size, "main"])]


def test_equal_length_train_and_backward_calls(rig):
    """embed_train / embed_backward / train_backward: one call each on the main workspace, each with its own size query."""
    h, eng = rig
    B, N, T = 2, 16384, num_frames(16384)
    wav = h.reg("wav", torch.zeros(B, 1, N))
    emb, layers, saved = eng.embed_train(wav)
    nsaved, size = fake_size("nomad_saved_bytes", B, N), fake_size("nomad_workspace_bytes", B, N)
    assert h.trace == enable("backward") + [("alloc", "main", nsaved), ("alloc", "main", size)] + [
        ("nomad_embed_train", "main", [("wav", 0), B, N, None, None, ("new(2, 256)", 0), (f"new(12, 2, {T}, 768)", 0),
                                       (f"new({nsaved},)", 0), nsaved, "ws_main", size, "main"])]
    del h.trace[:], h.named[1:]
    eng._ws = None
    h.reg("layers", layers), h.reg("saved", saved)
    dl, de = h.reg("dl", torch.zeros_like(layers)), h.reg("de", torch.zeros(B, 256))
    hw, hb = h.reg("hw", torch.zeros(256, 768)), h.reg("hb", torch.zeros(256))
    eng.embed_backward(wav, layers, saved, dl, de, head=(hw, hb))
    size = fake_size("nomad_backward_workspace_bytes", B, N)
    assert h.trace == enable("backward") + [("alloc", "main", size)] + [
        ("nomad_embed_backward", "main", [("wav", 0), B, N, ("hw", 0), ("hb", 0), ("layers", 0), ("saved", 0), nsaved, ("dl", 0), ("de", 0),
                                          (f"new({B}, {N})", 0), "ws_main", size, "main"])]
    del h.trace[:]
    eng._ws = None
    eng.train_backward(wav, layers, saved, de)
    size = fake_size("nomad_train_workspace_bytes", B, N)
    assert h.trace == [("alloc", "main", size),
                       ("nomad_train_backward", "main", [("wav", 0), B, N, ("layers", 0), ("saved", 0), nsaved, ("de", 0), "ws_main", size, "main"])]


# ---- what every equal-length forward refuses --------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["embed", "embed_bf16", "embed_bf16x3", "embed_features"])
def test_short_clip_and_wrong_dtype_are_refused_before_any_call(rig, call):
    h, eng = rig
    with pytest.raises(ValueError, match="receptive field"):
        getattr(eng, call)(torch.zeros(2, 1, 399))
    with pytest.raises(ValueError, match="contiguous fp32"):
        getattr(eng, call)(torch.zeros(2, 400, dtype=torch.float64))
    assert h.trace == []
