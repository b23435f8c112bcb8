"""CPU: the host side of differentiable scores over time (``nomad_embed_train_windows*``, ``nomad_embed_windows_backward*``,
``Engine.embed_*windows*``, ``Nomad.score_windows``) - everything that needs no GPU.

* ``nomad_window_cover`` through the built library - the helper the backward's scatter kernel itself calls - against a brute
  force over every T <= 40, win <= 12, hop <= 12 and every frame: the windows that contain a frame are exactly k_lo .. k_hi,
  and there is none exactly when k_lo > k_hi;
* header prototypes, ``_lib`` bindings and the exported symbols of the new entry points;
* ``nomad_windows_backward_scratch_bytes``;
* the refusals of ``score_windows`` and of the engine methods, each before anything touches an engine, for tensors with and
  without ``requires_grad``.
"""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from conftest import ROOT
from nomad_amd import _lib
from nomad_amd.nomad import Nomad
from nomad_amd.weights import num_windows

nomad_mod = sys.modules["nomad_amd.nomad"]     # (the package attribute `nomad` is the lazy singleton, not the module)
NEW = ("nomad_window_cover", "nomad_windows_backward_scratch_bytes", "nomad_embed_train_windows", "nomad_embed_train_windows_ragged",
       "nomad_embed_windows_backward", "nomad_embed_windows_backward_ragged")


def _cover(lib, T, win, hop, t):
    lo, hi = C.c_int(-7), C.c_int(-7)
    rc = lib.nomad_window_cover(T, win, hop, t, C.byref(lo), C.byref(hi))
    return rc, lo.value, hi.value


def test_window_cover_against_enumeration(built_lib):
    lib = _lib.load()
    gaps = tails = overlaps = 0
    for T in range(1, 41):
        for win in range(1, 13):
            for hop in range(1, 13):
                W, n = num_windows(T, win, hop), min(win, T)
                for t in range(T):
                    rc, lo, hi = _cover(lib, T, win, hop, t)
                    assert rc == 0, (T, win, hop, t)
                    want = [k for k in range(W) if k * hop <= t < k * hop + n]
                    assert want == list(range(lo, hi + 1)), (T, win, hop, t, lo, hi, want)
                    assert (not want) == (lo > hi), (T, win, hop, t, lo, hi)
                    overlaps += len(want) > 1
                    if not want:
                        tails += t >= (W - 1) * hop + n
                        gaps += t < (W - 1) * hop + n
    assert gaps and tails and overlaps        # the enumeration reached every kind of frame


def test_window_cover_refusals(built_lib):
    lib = _lib.load()
    for bad in ((0, 4, 2, 0), (-1, 4, 2, 0), (10, 0, 2, 0), (10, 4, 0, 0), (10, -3, 2, 0), (10, 4, -1, 0), (10, 4, 2, -1), (10, 4, 2, 10)):
        rc, lo, hi = _cover(lib, *bad)
        assert rc == _lib.NOMAD_ERR_INVALID and (lo, hi) == (-7, -7), bad      # outputs untouched
        assert b"nomad_window_cover" in lib.nomad_last_error()
    k = C.c_int()
    assert lib.nomad_window_cover(10, 4, 2, 3, None, C.byref(k)) == _lib.NOMAD_ERR_INVALID
    assert lib.nomad_window_cover(10, 4, 2, 3, C.byref(k), None) == _lib.NOMAD_ERR_INVALID


def test_scratch_bytes(built_lib):
    lib = _lib.load()
    n = C.c_size_t()
    for w in (1, 2, 3, 85, 416, 1 << 20, 3_000_000):      # the last: more than 2^31 floats
        assert lib.nomad_windows_backward_scratch_bytes(w, C.byref(n)) == 0
        assert n.value == (w * 768 * 4 + 255) // 256 * 256 == w * 768 * 4
    for w in (0, -1, -(1 << 40)):
        n.value = 12345
        assert lib.nomad_windows_backward_scratch_bytes(w, C.byref(n)) == _lib.NOMAD_ERR_INVALID and n.value == 12345
        assert b"nomad_windows_backward_scratch_bytes" in lib.nomad_last_error()
    assert lib.nomad_windows_backward_scratch_bytes(4, None) == _lib.NOMAD_ERR_INVALID


def _prototype(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in include/nomad_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype_of(arg):
    if arg.endswith("*") or "*" in arg or arg.startswith("nomad_stream_t"):
        if arg.startswith("const int*") or arg.startswith("int*"):
            return C.POINTER(C.c_int)
        if arg.startswith("size_t*"):
            return C.POINTER(C.c_size_t)
        return C.c_void_p
    return {"int": C.c_int, "size_t": C.c_size_t, "long long": C.c_longlong}[arg.rsplit(" ", 1)[0]]


def test_header_binding_and_exports_agree(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nomad_hip.h")).read(), flags=re.S)
    lib = C.CDLL(built_lib)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = _lib.SIGNATURES[name]
        proto = _prototype(text, name)
        assert res is C.c_int and len(args) == len(proto), (name, len(args), len(proto))
        for i, (a, p) in enumerate(zip(args, proto)):
            assert a == _ctype_of(p), (name, i, p, a)
    # the train forwards are nomad_embed_train[_ragged] plus (win, hop); the backwards nomad_embed_backward[_ragged] plus (win, hop)
    # and (scratch, scratch_bytes), minus dlayers
    assert len(_lib.SIGNATURES["nomad_embed_train_windows"][1]) == len(_lib.SIGNATURES["nomad_embed_train"][1]) + 2
    assert len(_lib.SIGNATURES["nomad_embed_train_windows_ragged"][1]) == len(_lib.SIGNATURES["nomad_embed_train_ragged"][1]) + 2
    assert len(_lib.SIGNATURES["nomad_embed_windows_backward"][1]) == len(_lib.SIGNATURES["nomad_embed_backward"][1]) + 3
    assert len(_lib.SIGNATURES["nomad_embed_windows_backward_ragged"][1]) == len(_lib.SIGNATURES["nomad_embed_backward_ragged"][1]) + 3
    # entry points were added, none changed: the binary-interface number stays
    assert int(re.search(r"#define NOMAD_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 3


# ---- refusals decided on the host ----------------------------------------------------------------------------------------------
class _NoEngine:
    """An engine nothing may be asked of: the refusals below come before the first engine call."""
    device = torch.device("cpu")

    def __getattr__(self, name):
        raise AssertionError(f"the engine was asked for {name}")


def _nomad(engine, precision="fp32"):
    n = Nomad.__new__(Nomad)            # no GPU: only the host side is under test
    n.engine, n.precision, n.group = engine, precision, None
    return n


@pytest.mark.parametrize("grad", [False, True], ids=["no_grad", "requires_grad"])
def test_score_windows_refusals(grad):
    n = _nomad(_NoEngine())
    wav, refs = torch.zeros(2, 1, 4000, requires_grad=grad), torch.zeros(3, 256, requires_grad=grad)
    for kw in (dict(window_s=0), dict(hop_s=-1.0), dict(window_s=float("nan")), dict(hop_s=None), dict(window_s=True)):
        with pytest.raises(ValueError, match="positive number of seconds"):
            n.score_windows(wav, refs, **kw)
    for bad in (torch.zeros(3, 255), torch.zeros(256), torch.zeros(2, 3, 256)):
        with pytest.raises(ValueError, match=r"\(Nr, 256\)"):
            n.score_windows(wav, bad.requires_grad_(grad))
    with pytest.raises(ValueError, match="at least one reference"):
        n.score_windows(wav, torch.zeros(0, 256, requires_grad=grad))
    with pytest.raises(TypeError, match="floating-point"):
        n.score_windows(wav, torch.zeros(3, 256, dtype=torch.int32))
    with pytest.raises(TypeError, match="tensor of embeddings"):
        n.score_windows(wav, [[0.0] * 256])
    for bad in (torch.zeros(2, 2, 4000), torch.zeros(4000), torch.zeros(1, 2, 1, 4000)):
        with pytest.raises(ValueError, match=r"\(B,1,N\) or \(B,N\)"):
            n.score_windows(bad.requires_grad_(grad), refs)
    with pytest.raises(ValueError, match=r"\(B,1,N\) or \(B,N\)"):
        n.score_windows([0.0] * 4000, refs)
    with pytest.raises(ValueError, match=r"lengths\[1\]"):
        n.score_windows(wav, refs, lengths=[4000, 399])
    with pytest.raises(ValueError, match=r"lengths\[0\]"):
        n.score_windows(wav, refs, lengths=[4001, 4000])
    with pytest.raises(ValueError, match="3 entries"):
        n.score_windows(wav, refs, lengths=[4000, 4000, 4000])
    with pytest.raises(ValueError, match="1-D integer tensor"):
        n.score_windows(wav, refs, lengths=torch.tensor([4000.0, 4000.0]))
    for bad in ("sum", None, "Mean"):
        with pytest.raises(ValueError, match="reduction"):
            n.score_windows(wav, refs, reduction=bad)


def test_score_over_time_still_refuses_a_gradient():
    """``score_windows`` is the differentiable form; ``score_over_time`` keeps its refusal and names the alternative."""
    n = _nomad(_NoEngine())
    with pytest.raises(ValueError, match="no gradient"):
        n.score_over_time(torch.zeros(2, 4000, requires_grad=True), torch.zeros(3, 256))
    assert "score_windows" in Nomad.score_over_time.__doc__


class _CheckOnlyEngine(nomad_mod.Engine):
    """The argument checks of the engine's windowed gradient calls without a context: only the device check answers."""

    def __init__(self):
        self.device = torch.device("cpu")

    def _check_dev(self, t, name):
        if not (t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous fp32 tensor")

    def enable_backward(self):
        raise AssertionError("the context was touched")

    def close(self):
        pass


def test_engine_refusals_come_before_the_context_is_touched():
    eng = _CheckOnlyEngine()
    wav = torch.zeros(2, 4000)
    for win, hop in ((0, 1), (1, 0), (-5, 2), (4, -2)):
        for call in (lambda: eng.embed_train_windows(wav, win, hop),
                     lambda: eng.embed_train_windows_ragged(wav, win, hop, lengths=[4000, 4000]),
                     lambda: eng.embed_windows_backward(wav, None, None, torch.zeros(2, 256), win, hop),
                     lambda: eng.embed_windows_backward_ragged((wav, [4000, 4000]), None, None, torch.zeros(2, 256), win, hop)):
            with pytest.raises(ValueError, match="at least 1 frame"):
                call()
    with pytest.raises(ValueError, match="head weight"):
        eng.embed_train_windows(wav, 4, 2, head=(torch.zeros(256, 768, dtype=torch.float64), torch.zeros(256)))
    with pytest.raises(ValueError, match="receptive field"):
        eng.embed_train_windows(torch.zeros(2, 399), 4, 2)
    with pytest.raises(ValueError, match="receptive field"):
        eng.embed_train_windows_ragged(torch.zeros(2, 4000), 4, 2, lengths=[4000, 399])
    # 4000 samples are 12 frames: 5 windows of 4 frames every 2 per clip - one row of demb_w per window
    assert num_windows(12, 4, 2) == 5
    for bad in (torch.zeros(2, 256), torch.zeros(10, 255), torch.zeros(11, 256)):
        with pytest.raises(ValueError, match=r"\(10, 256\)"):
            eng.embed_windows_backward(wav, None, None, bad, 4, 2)
        with pytest.raises(ValueError, match=r"\(10, 256\)"):
            eng.embed_windows_backward_ragged((wav, [4000, 4000]), None, None, bad, 4, 2)
    with pytest.raises(ValueError, match="demb_w must be a contiguous fp32"):
        eng.embed_windows_backward(wav, None, None, torch.zeros(10, 256, dtype=torch.float64), 4, 2)
