"""CPU: the host side of scores over spans (``nomad_embed_spans*``, ``nomad_frame_energy``; ``Engine.embed_spans_ragged`` and its
gradient siblings; ``Nomad.span_frames`` / ``score_spans`` / ``active_spans`` / ``predict_spans``; the CLI) - everything that needs
no GPU.

* header, binding and exports of the new names;
* ``span_frames``: the inverse of ``window_times``, clamping, refusals;
* the activity rule on hand-made energies: gap closing, short-run dropping, the silent clip, a NaN;
* table building from the Python and the csv forms, shared ``Row`` labels, the error cases; the engine's own table check and its
  cut into the parts of a two-stream split;
* ``score_spans`` / ``predict_spans`` over a recorder engine: call sequences with and without a gradient, with and without ``k``;
* the CLI routes and exclusions.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import ROOT
from nomad_amd import _lib
from nomad_amd.nomad import Nomad, active_frames, span_frames, span_table, span_times, spans_from_csv, window_times
from nomad_amd.weights import num_frames, num_windows

nomad_mod = sys.modules["nomad_amd.nomad"]
NEW = ("nomad_spans_scratch_bytes", "nomad_embed_spans_ragged", "nomad_embed_train_spans_ragged", "nomad_embed_spans_backward_ragged",
       "nomad_frame_energy")


def test_binding_header_and_library_carry_the_new_entry_points(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nomad_hip.h")).read(), flags=re.S)
    lib = C.CDLL(built_lib)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} is not declared in include/nomad_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        # the binding takes as many arguments as the header declares
        decl = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(decl.split(",")), name
    res, args = _lib.SIGNATURES["nomad_embed_spans_ragged"]
    # ctx, wav, B, stride, lengths, precision, R, row_clip, row_ptr, spans, head_w, head_b, emb, scratch, bytes, workspace, bytes, stream
    assert res is C.c_int and len(args) == 18 and [i for i, t in enumerate(args) if t is C.c_int] == [2, 3, 5, 6]
    assert [i for i, t in enumerate(args) if t == C.POINTER(C.c_int)] == [4, 7, 8, 9] and args[14] is args[16] is C.c_size_t
    assert len(_lib.SIGNATURES["nomad_embed_train_spans_ragged"][1]) == 20
    assert len(_lib.SIGNATURES["nomad_embed_spans_backward_ragged"][1]) == 21
    assert len(_lib.SIGNATURES["nomad_frame_energy"][1]) == 7
    # entry points were added, none changed: the binary-interface number stays
    assert int(re.search(r"#define NOMAD_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 3


def test_scratch_size_is_host_arithmetic(built_lib):
    lib = _lib.load()
    n0, n1 = C.c_size_t(), C.c_size_t()
    for B, R, S in ((1, 1, 1), (3, 8, 14), (32, 448, 448), (5, 1, 1000)):
        assert lib.nomad_spans_scratch_bytes(B, R, S, 0, C.byref(n0)) == 0 and lib.nomad_spans_scratch_bytes(B, R, S, 1, C.byref(n1)) == 0
        ints = 2 * R + 1 + 2 * S + B + 1                   # row_clip, row_ptr, spans, the per-clip row ranges
        assert 4 * ints <= n0.value < 4 * ints + 256 and n0.value % 256 == 0
        assert 4 * 768 * R <= n1.value - n0.value < 4 * 768 * R + 256
    for bad in ((0, 1, 1), (1, 0, 1), (1, 2, 1), (-1, 1, 1)):
        assert lib.nomad_spans_scratch_bytes(*bad, 0, C.byref(n0)) == _lib.NOMAD_ERR_INVALID
        assert b"nomad_spans_scratch_bytes" in lib.nomad_last_error()
    assert lib.nomad_spans_scratch_bytes(1, 1, 1, 0, None) == _lib.NOMAD_ERR_INVALID


# ---- seconds <-> frames ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T, win, hop", [(1, 1, 1), (65, 64, 1), (130, 65, 65), (40, 3, 2), (40, 4, 9), (7, 200, 100), (1499, 200, 100),
                                         (1499, 1, 7)])
def test_span_frames_inverts_window_times(T, win, hop):
    start, end = window_times(T, win, hop)
    n = min(win, T)
    for k in range(num_windows(T, win, hop)):
        assert span_frames(start[k], end[k], T) == (k * hop, k * hop + n)
        assert span_times(k * hop, k * hop + n) == (start[k], end[k])
    assert Nomad.span_frames(start[0], end[0], T) == (0, n)       # also reachable from the class


def test_span_frames_rounds_and_clamps():
    assert span_frames(0.0, 1.005, 100) == (0, 50) and span_frames(0.0, 1.0, 100) == (0, 50)      # 49.75 rounds to 50
    assert span_frames(0.011, 0.049, 100) == (1, 2)
    assert span_frames(-3.0, 0.5, 100) == (0, 25) and span_frames(1.0, 99.0, 100) == (50, 100)
    assert span_frames(np.float32(0.5), np.float64(0.705), 40) == (25, 35) and span_frames(0, 1, 60) == (0, 50)


@pytest.mark.parametrize("start, end, T", [(1.0, 1.0, 100), (2.0, 1.0, 100), (5.0, 6.0, 100), (-2.0, -1.0, 100), (0.0, 0.01, 100)])
def test_an_empty_span_is_refused_by_name(start, end, T):
    with pytest.raises(ValueError, match=re.escape(f"({start!r} s, {end!r} s)")):
        span_frames(start, end, T)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), None, "1", True])
def test_bad_seconds_are_refused(bad):
    with pytest.raises(ValueError, match="start_s"):
        span_frames(bad, 1.0, 10)
    with pytest.raises(ValueError, match="end_s"):
        span_frames(0.0, bad, 10)


# ---- the activity rule ----------------------------------------------------------------------------------------------------------
def _e(T, *runs, level=1.0):
    e = np.full(T, 1e-9)
    for a, b in runs:
        e[a:b] = level
    return e


def test_active_frames_threshold_gaps_and_short_runs():
    assert active_frames(_e(100, (10, 30), (60, 90))) == [(10, 30), (60, 90)]                      # a gap of 30 > 15 stays
    assert active_frames(_e(100, (10, 30), (45, 90))) == [(10, 90)]                                # a gap of exactly 15 closes
    assert active_frames(_e(100, (10, 30), (46, 90))) == [(10, 30), (46, 90)]                      # 16 does not
    assert active_frames(_e(100, (10, 14), (60, 90))) == [(60, 90)]                                # a run of 4 < 5 is dropped
    assert active_frames(_e(100, (10, 15), (60, 90))) == [(10, 15), (60, 90)]                      # 5 stays
    assert active_frames(_e(100, (10, 12), (14, 16), (60, 90))) == [(10, 16), (60, 90)]            # gaps close BEFORE short runs drop
    assert active_frames(_e(100, (0, 10), (95, 100))) == [(0, 10), (95, 100)]                      # the clip's edges are not gaps
    assert active_frames(_e(100, (10, 30), (60, 90)), min_speech_frames=25, min_gap_frames=0) == [(60, 90)]
    # the floor is relative to the loudest frame: -30 dB is active at 40 dB, not at 20 dB
    e = _e(100, (0, 10))
    e[40:60] = 1e-3
    assert active_frames(e, 40.0) == [(0, 10), (40, 60)] and active_frames(e, 20.0) == [(0, 10)]
    assert active_frames(e, 30.0) == [(0, 10), (40, 60)]                                           # the floor itself is active (>=)


def test_active_frames_falls_back_to_the_whole_clip():
    assert active_frames(np.zeros(7)) == [(0, 7)]                                                  # silence
    assert active_frames([1.0, np.nan, 2.0, 1.0]) == [(0, 4)] and active_frames([1.0, np.inf]) == [(0, 2)]
    assert active_frames(_e(100, (10, 13))) == [(0, 100)]                                          # nothing survives rule 3
    assert active_frames([0.5]) == [(0, 1)] or active_frames([0.5], min_speech_frames=1) == [(0, 1)]
    with pytest.raises(ValueError, match="at least one frame"):
        active_frames([])


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def test_span_table_from_the_python_form():
    rows = [[(0.0, 0.505), [(0.1, 0.205), (0.2, 0.405)]], [], [[(0.0, 0.025)]]]
    table, counts = span_table(rows, [50, 10, 30])
    assert table == ([0, 0, 2], [0, 1, 3, 4], [(0, 25), (5, 10), (10, 20), (0, 1)]) and counts == [2, 0, 1]
    table, counts = span_table([[[(3, 40), (50, 120)], (129, 130)]], [130], unit="frames")
    assert table == ([0, 0], [0, 2, 3], [(3, 40), (50, 120), (129, 130)]) and counts == [2]
    assert span_table([[np.array([[0, 1], [1, 2]])]], [5], unit="frames")[0] == ([0], [0, 2], [(0, 1), (1, 2)])   # touching is allowed


@pytest.mark.parametrize("rows, frames, unit, msg", [
    ([[(0, 5)]], [5, 5], "frames", "rows of 1 clips for a batch of 2"),
    ([[], []], [5, 5], "frames", "no row"),
    ([[[]]], [5], "frames", "clip 0, row 0 has no span"),
    ([[(0, 6)]], [5], "frames", r"clip 0, row 0, span 0 is \[0, 6\)"),
    ([[(-1, 2)]], [5], "frames", r"span 0 is \[-1, 2\)"),
    ([[(2, 2)]], [5], "frames", r"span 0 is \[2, 2\)"),
    ([[], [[(0, 3), (2, 4)]]], [5, 5], "frames", "clip 1, row 0, span 1 .* overlaps or precedes"),
    ([[[(3, 4), (0, 1)]]], [5], "frames", "span 1 .* overlaps or precedes"),
    ([[(1.0, 1.0)]], [100], "s", "clip 0, row 0, span 0: the span"),
    ([[[(0, 1, 2)]]], [5], "frames", "expected a .start, end. pair"),
    ([[(0, 1)]], [5], "samples", "unit must be"),
])
def test_span_table_refusals(rows, frames, unit, msg):
    with pytest.raises(ValueError, match=msg):
        span_table(rows, frames, unit)


def test_spans_from_csv(tmp_path):
    df = pd.DataFrame({"Test File": ["b", "a", "b", "a", "b"], "start_s": [2.0, 0.0, 0.5, 3.0, 4.0], "end_s": [3.0, 1.0, 1.0, 4.0, 5.0]})
    out = spans_from_csv(df, ["a", "b", "c"])
    assert out == {"b": [(0, [(2.0, 3.0)]), (1, [(0.5, 1.0)]), (2, [(4.0, 5.0)])], "a": [(0, [(0.0, 1.0)]), (1, [(3.0, 4.0)])]}
    df["Row"] = ["spk1", "x", "spk2", "x", "spk1"]
    path = tmp_path / "spans.csv"
    df.to_csv(path, index=False)
    for src in (df, str(path), path):
        out = spans_from_csv(src, ["a", "b", "c"])
        assert out == {"b": [("spk1", [(2.0, 3.0), (4.0, 5.0)]), ("spk2", [(0.5, 1.0)])], "a": [("x", [(0.0, 1.0), (3.0, 4.0)])]}
    assert "c" not in out
    with pytest.raises(ValueError, match="'b'.*not among the test files"):
        spans_from_csv(df, ["a", "c"])
    with pytest.raises(ValueError, match="lacks the column"):
        spans_from_csv(df.drop(columns=["end_s"]), ["a", "b"])
    with pytest.raises(TypeError, match="DataFrame or the path"):
        spans_from_csv([("a", 0, 1)], ["a"])


def test_engine_table_check_and_parts():
    from nomad_amd.engine import Engine
    table = ([0, 0, 2, 3], [0, 1, 3, 4, 6], [(0, 5), (1, 2), (2, 9), (0, 1), (3, 4), (6, 7)])
    assert Engine._check_table(table, [10, 10, 10, 10]) == ([0, 0, 2, 3], [0, 1, 3, 4, 6], list(table[2]))
    assert Engine._table_part(table, 0, 2) == (0, ([0, 0], [0, 1, 3], [(0, 5), (1, 2), (2, 9)]))
    assert Engine._table_part(table, 2, 4) == (2, ([0, 1], [0, 1, 3], [(0, 1), (3, 4), (6, 7)]))
    assert Engine._table_part(table, 1, 2) == (0, None) and Engine._table_part(table, 0, 4) == (0, table)
    R, row_clip, row_ptr, spans = Engine._table_args(table)
    assert R == 4 and list(row_clip) == table[0] and list(row_ptr) == table[1] and list(spans) == [0, 5, 1, 2, 2, 9, 0, 1, 3, 4, 6, 7]
    for bad, msg in ((([], [0], []), "at least one row"), (([0], [0, 1], [(0, 11)]), r"row 0, span 0 is \[0, 11\)"),
                     (([1, 0], [0, 1, 2], [(0, 1), (0, 1)]), "row 1 names clip 0 behind"), (([4], [0, 1], [(0, 1)]), "outside"),
                     (([0, 0], [0, 1, 1], [(0, 1)]), "row 1 has no span"), (([0], [0, 2], [(0, 5), (4, 6)]), "row 0, span 1"),
                     (([0], [0, 2], [(0, 5)]), "row_ptr must hold"), (([0], [1, 2], [(0, 5), (5, 6)]), "row_ptr must hold")):
        with pytest.raises(ValueError, match=msg):
            Engine._check_table(bad, [10, 10, 10, 10])


# ---- score_spans over a recorder engine -----------------------------------------------------------------------------------------
def _nomad(engine, precision="fp32"):
    n = Nomad.__new__(Nomad)
    n.engine, n.precision, n.group = engine, precision, None
    return n


class _Recorder:
    """Records every engine call; row r's embedding is [r + 1, 0, ...], a distance |emb_0 - ref_0|, backwards return zeros."""
    device = torch.device("cpu")
    encoder_depth = 12

    def __init__(self):
        self.calls = []

    @staticmethod
    def _emb(rows):
        emb = torch.zeros(rows, 256)
        emb[:, 0] = torch.arange(1, rows + 1)
        return emb

    def embed_spans_ragged(self, waves, table, precision="fp32", packed=None):
        self.calls.append(("embed_spans_ragged", [int(w.shape[0]) for w in waves], table, precision))
        return self._emb(len(table[0]))

    def embed_train_spans_ragged(self, wav, table, lens):
        self.calls.append(("embed_train_spans_ragged", tuple(wav.shape), table, list(lens)))
        return self._emb(len(table[0])), torch.zeros(1), torch.zeros(1), (wav, lens)

    def embed_spans_backward_ragged(self, batch, layers, saved, demb, table):
        self.calls.append(("embed_spans_backward_ragged", list(batch[1]), tuple(demb.shape), table))
        return torch.zeros_like(batch[0])

    @staticmethod
    def _dist(emb, ref):
        return (emb[:, :1].double() - ref[:, 0].double()[None, :]).abs()

    def pairwise(self, emb, ref, want_matrix=True):
        self.calls.append(("pairwise", want_matrix))
        return None, self._dist(emb, ref).mean(1)

    def knn(self, a, b, k, want_matrix=False):
        self.calls.append(("knn", k, want_matrix))
        d, idx = self._dist(a, b).sort(dim=1, stable=True)
        return d[:, :k], idx[:, :k].to(torch.int32), d[:, :k].mean(1)

    def cdist_backward(self, a, b, g_dist=None, g_mean=None, want_a=True, want_b=False):
        self.calls.append(("cdist_backward", tuple(g_mean.shape), want_a, want_b))
        return (torch.zeros_like(a) if want_a else None), (torch.zeros_like(b) if want_b else None)

    def knn_backward(self, a, b, knn_idx, g_knn=None, g_score=None, want_a=True, want_b=True):
        self.calls.append(("knn_backward", int(knn_idx.shape[1]), tuple(g_score.shape), want_a, want_b))
        return (torch.zeros_like(a) if want_a else None), (torch.zeros_like(b) if want_b else None)


REFS = torch.zeros(5, 256)
REFS[:, 0] = torch.tensor([10.0, 2.5, 7.0, 1.0, 3.0])
N = 320 * 49 + 400                                              # 50 frames
SPANS = [[(0.0, 0.505), [(0.1, 0.205), (0.3, 0.405)]], [(0.5, 1.005)]]
TABLE = ([0, 0, 1], [0, 1, 3, 4], [(0, 25), (5, 10), (15, 20), (25, 50)])


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("lengths", [None, [N, N - 320]])
def test_score_spans_call_sequences(k, lengths):
    table = TABLE if lengths is None else (TABLE[0], TABLE[1], TABLE[2][:3] + [(25, 49)])
    lens = lengths or [N, N]
    mean = ("pairwise", False) if k is None else ("knn", k, False)
    d = (torch.arange(1, 4).double()[:, None] - REFS[:, 0].double()[None, :]).abs()
    want = d.mean(1) if k is None else d.sort(dim=1)[0][:, :k].mean(1)
    # no gradient
    eng = _Recorder()
    scores, counts = _nomad(eng).score_spans(torch.zeros(2, 1, N), REFS, SPANS, lengths=lengths, k=k)
    assert eng.calls == [("embed_spans_ragged", lens, table, "fp32"), mean]
    assert counts == [2, 1] and torch.equal(scores, want) and not scores.requires_grad
    # bf16 stays bf16; bf16x3 takes fp32 buffers for so short a batch, as score_over_time does
    for precision, runs in (("bf16", "bf16"), ("bf16x3", "fp32")):
        eng = _Recorder()
        _nomad(eng, precision).score_spans(torch.zeros(2, N), REFS, SPANS, lengths=lengths, k=k)
        assert eng.calls[0][3] == runs
    # under no_grad nothing is differentiated, whatever the leaves ask for
    eng = _Recorder()
    with torch.no_grad():
        _nomad(eng).score_spans(torch.zeros(2, 1, N, requires_grad=True), REFS.clone().requires_grad_(True), SPANS, lengths=lengths, k=k)
    assert [c[0] for c in eng.calls] == ["embed_spans_ragged", mean[0]]
    # a gradient to the waveform
    eng = _Recorder()
    wav = torch.zeros(2, 1, N, requires_grad=True)
    scores, counts = _nomad(eng).score_spans(wav, REFS, SPANS, lengths=lengths, k=k)
    scores.sum().backward()
    back = ("cdist_backward", (3,), True, False) if k is None else ("knn_backward", k, (3,), True, False)
    assert eng.calls == [("embed_train_spans_ragged", (2, N), table, lens), mean, back,
                         ("embed_spans_backward_ragged", lens, (3, 256), table)]
    assert wav.grad.shape == wav.shape and torch.equal(scores.detach(), want)
    # a gradient to the references only: the scoring forward, no backbone backward
    eng = _Recorder()
    refs = REFS.clone().requires_grad_(True)
    _nomad(eng).score_spans(torch.zeros(2, 1, N), refs, SPANS, lengths=lengths, k=k, reduction="mean")[0].backward()
    back = ("cdist_backward", (3,), False, True) if k is None else ("knn_backward", k, (3,), False, True)
    assert eng.calls == [("embed_spans_ragged", lens, table, "fp32"), mean, back] and refs.grad is not None


class _NoEngine:
    device = torch.device("cpu")

    def __getattr__(self, name):
        raise AssertionError(f"the engine was asked for {name}")


def test_score_spans_refusals_come_before_any_engine_call():
    n = _nomad(_NoEngine())
    wav = torch.zeros(2, 1, N)
    with pytest.raises(ValueError, match="clip 1, row 0, span 0"):
        n.score_spans(wav, REFS, [[(0.0, 0.5)], [(2.0, 3.0)]])
    with pytest.raises(ValueError, match="rows of 1 clips for a batch of 2"):
        n.score_spans(wav, REFS, [[(0.0, 0.5)]])
    with pytest.raises(ValueError, match="no row"):
        n.score_spans(wav, REFS, [[], []])
    with pytest.raises(ValueError, match="unit must be"):
        n.score_spans(wav, REFS, SPANS, unit="ms")
    with pytest.raises(ValueError, match=r"\(Nr, 256\)"):
        n.score_spans(wav, torch.zeros(3, 255), SPANS)
    with pytest.raises(ValueError, match="k = 9"):
        n.score_spans(wav, REFS, SPANS, k=9)
    with pytest.raises(ValueError, match=r"\(B,1,N\) or \(B,N\)"):
        n.score_spans(torch.zeros(2, 2, N), REFS, SPANS)
    with pytest.raises(ValueError, match=r"lengths\[1\]"):
        n.score_spans(wav, REFS, SPANS, lengths=[N, 399])
    with pytest.raises(ValueError, match="shorter than one encoder frame"):
        n.score_spans(torch.zeros(2, 399), REFS, SPANS)
    with pytest.raises(ValueError, match="reduction"):
        n.score_spans(wav, REFS, SPANS, reduction="sum")
    for kw in (dict(floor_db=float("nan")), dict(min_speech_s=-1.0), dict(min_gap_s=float("inf"))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            n.active_spans(wav, **kw)


def test_active_spans_runs_the_rule_on_the_engines_energies():
    class _Energy:
        device = torch.device("cpu")

        def frame_energy(self, waves, packed=None):
            assert waves is None
            self.lens = list(packed[1])
            e = np.concatenate([np.full(num_frames(n), 1e-9) for n in packed[1]])
            e[10:30] = 1.0                                      # clip 0: one run; clip 1 (frames 50 ..): silent next to it
            return torch.from_numpy(e)
    eng = _Energy()
    assert _nomad(eng).active_spans(torch.zeros(2, 1, N), lengths=[N, N - 640]) == [[(10, 30)], [(0, 48)]]
    assert eng.lens == [N, N - 640]
    assert _nomad(eng).active_spans(torch.zeros(2, N), min_speech_s=0.5) == [[(0, 50)], [(0, 50)]]


# ---- predict_spans through a fake engine --------------------------------------------------------------------------------------------
class _FileEngine:
    """A row -> the embedding [clip length, first frame, frames pooled, 0, ...]; its "distance" is length / 1e5 + first frame / 1e3 +
    frames pooled / 1e6 (+ the number of references), so every score names its row."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def pack_ragged_host(self, waves):
        lens = [int(w.shape[0]) for w in waves]
        host = np.zeros((len(waves), max(lens)), dtype=np.float32)
        for i, w in enumerate(waves):
            host[i, :lens[i]] = w
        return host, lens

    def embed_ragged(self, waves, precision=None, packed=None):
        self.calls.append(("embed_ragged", list(packed[1])))
        out = np.zeros((len(packed[1]), 256), dtype=np.float32)
        out[:, 0] = packed[1]
        return out

    def frame_energy(self, waves, packed=None):
        self.calls.append(("frame_energy", list(packed[1])))
        e = np.concatenate([np.full(num_frames(n), 1e-9) for n in packed[1]])
        at = 0
        for n in packed[1]:                                      # every clip: active in frames [2, 8) and from frame 30 on
            t = num_frames(n)
            e[at + 2:at + min(8, t)] = 1.0
            e[at + 30:at + t] = 1.0
            at += t
        return torch.from_numpy(e)

    def embed_spans_ragged(self, waves, table, precision="fp32", packed=None):
        assert waves is None
        self.calls.append(("embed_spans_ragged", list(packed[1]), table))
        row_clip, row_ptr, spans = table
        emb = torch.zeros(len(row_clip), 256)
        for r, c in enumerate(row_clip):
            mine = spans[row_ptr[r]:row_ptr[r + 1]]
            emb[r, :3] = torch.tensor([packed[1][c], mine[0][0], sum(b - a for a, b in mine)], dtype=torch.float32)
        return emb

    def pairwise(self, emb, ref, want_matrix=True):
        assert not want_matrix and ref.shape[1] == 256
        return None, (emb[:, 0].double() / 1e5 + emb[:, 1].double() / 1e3 + emb[:, 2].double() / 1e6 + ref.shape[0])

    def fetch_async(self, t):
        class F:
            def result(self_inner):
                return t.numpy() if torch.is_tensor(t) else t
        return F()


LENS = {name: 320 * (T - 1) + 400 for name, T in (("long", 450), ("short", 12), ("exact", 200), ("mid", 300))}


@pytest.fixture
def folders(tmp_path):
    nmr, deg = tmp_path / "nmr", tmp_path / "deg"
    nmr.mkdir()
    deg.mkdir()
    for name in ("r0", "r1", "r2"):
        (nmr / f"{name}.wav").write_bytes(b"")
    for name in LENS:
        (deg / f"{name}.wav").write_bytes(b"")
    return str(nmr), str(deg), tmp_path


def _pipeline_nomad(eng):
    n = _nomad(eng)
    n.model = None

    def load(p, trim=False):
        return np.zeros((1, LENS.get(os.path.basename(p)[:-4], 16000)), dtype=np.float32)
    n.load_processing = load
    n.NATIVE_WAV_THREADS = 0
    return n


def _score(name, t0, frames):
    return LENS[name] / 1e5 + t0 / 1e3 + frames / 1e6 + 3


def test_predict_spans_from_a_csv(folders):
    nmr, deg, tmp = folders
    listed = [f[:-4] for f in os.listdir(deg)]
    csv = pd.DataFrame({"Test File": ["long", "mid", "long", "long", "short"], "Row": ["A", "turn", "B", "A", "all"],
                        "start_s": [4.0, 0.0, 1.0, 0.0, 0.0], "end_s": [6.005, 2.005, 2.005, 1.005, 99.0]})
    eng = _FileEngine()
    out = tmp / "out"
    out.mkdir()
    df, avg = _pipeline_nomad(eng).predict_spans("dir", nmr, deg, spans=csv, results_path=str(out), max_batch_samples=150000)
    want = {"long": [("A", 0.0, 6.005, 3.0, _score("long", 0, 150)), ("B", 1.0, 2.005, 1.0, _score("long", 50, 50))],
            "mid": [("turn", 0.0, 2.005, 2.0, _score("mid", 0, 100))], "short": [("all", 0.0, 0.245, 0.24, _score("short", 0, 12))]}
    assert list(df.columns) == ["Test File", "Row", "start_s", "end_s", "active_s", "NOMAD"]
    files = [f for f in listed if f in want]                       # listing order; "exact" has no line and no row
    assert list(df["Test File"]) == [f for f in files for _ in want[f]]
    got = [tuple(r) for r in df[["Row", "start_s", "end_s", "active_s", "NOMAD"]].itertuples(index=False)]
    assert got == [(lab, a, b, act, round(s, 3)) for f in files for lab, a, b, act, s in want[f]]
    assert avg.index.name == "Test File" and list(avg.index) == files and list(avg.columns) == ["NOMAD"]
    for f in files:
        assert avg.loc[f, "NOMAD"] == round(float(np.mean([s for *_, s in want[f]])), 3)
    # the references were embedded whole, the test files through the span head in more than one staged batch; no energies were asked for
    names = [c[0] for c in eng.calls]
    assert "frame_energy" not in names and names.count("embed_spans_ragged") >= 2 and "embed_ragged" in names
    back = pd.read_csv(out / "spans.csv")
    assert list(back.columns) == list(df.columns) and list(back["Row"]) == list(df["Row"])
    for col in ("start_s", "end_s", "active_s", "NOMAD"):
        assert np.array_equal(back[col].to_numpy(dtype=np.float64), df[col].to_numpy(dtype=np.float64)), col
    assert sorted(os.listdir(out)) == ["spans.csv"]
    # without the Row column every line is a row of its own
    df2, _ = _pipeline_nomad(_FileEngine()).predict_spans("dir", nmr, deg, spans=csv.drop(columns=["Row"]))
    assert len(df2) == 5 and list(df2[df2["Test File"] == "long"]["Row"]) == [0, 1, 2]


def test_predict_spans_with_the_energy_gate(folders):
    nmr, deg, _ = folders
    listed = [f[:-4] for f in os.listdir(deg)]
    eng = _FileEngine()
    df, avg = _pipeline_nomad(eng).predict_spans("dir", nmr, deg, active_db=40.0, max_batch_samples=150000)
    assert list(df["Test File"]) == listed and list(df["Row"]) == ["active"] * 4 and list(avg.index) == listed
    for f, (_, row) in zip(listed, df.iterrows()):
        T = num_frames(LENS[f])
        spans = [(2, 8), (30, T)] if T > 34 else [(2, 8)]          # "short": 12 frames, nothing behind frame 30
        n = sum(b - a for a, b in spans)
        assert (row["start_s"], row["end_s"], row["active_s"]) == (0.04, (spans[-1][1] * 20 + 5) / 1000.0, n * 20 / 1000.0)
        assert row["NOMAD"] == round(_score(f, 2, n), 3)
    # one energy call per staged batch, ahead of that batch's forward, on the same clips
    pipe = [c for c in eng.calls if c[0] in ("frame_energy", "embed_spans_ragged")]
    assert len(pipe) >= 4 and all(a[0] == "frame_energy" and b[0] == "embed_spans_ragged" and a[1] == b[1] for a, b in zip(pipe[::2], pipe[1::2]))


def test_predict_spans_refusals(folders, monkeypatch):
    nmr, deg, _ = folders
    n = _pipeline_nomad(_NoEngine())
    csv = pd.DataFrame({"Test File": ["long"], "start_s": [0.0], "end_s": [1.0]})
    with pytest.raises(ValueError, match="exactly one of"):
        n.predict_spans("dir", nmr, deg)
    with pytest.raises(ValueError, match="exactly one of"):
        n.predict_spans("dir", nmr, deg, spans=csv, active_db=40.0)
    with pytest.raises(ValueError, match="active_db"):
        n.predict_spans("dir", nmr, deg, active_db=float("nan"))
    with pytest.raises(ValueError, match="not among the test files"):
        n.predict_spans("dir", nmr, deg, spans=pd.DataFrame({"Test File": ["nobody"], "start_s": [0.0], "end_s": [1.0]}))
    with pytest.raises(Exception, match="Path to the test files"):
        n.predict_spans("dir", nmr, deg + "x", spans=csv)
    with pytest.raises(ValueError, match="k = 65"):
        n.predict_spans("dir", nmr, deg, spans=csv, k=65)
    # a span outside its file: refused with the file's name when its batch is reached
    with pytest.raises(ValueError, match=r"clip 0, row 0, span 0.*short"):
        _pipeline_nomad(_FileEngine()).predict_spans("dir", nmr, deg, max_batch_samples=1,
                                                     spans=pd.DataFrame({"Test File": ["short"], "start_s": [5.0], "end_s": [6.0]}))
    monkeypatch.setattr(nomad_mod, "_dist_info", lambda group=None: (2, 0, True))
    with pytest.raises(RuntimeError, match="2 ranks"):
        n.predict_spans("dir", nmr, deg, spans=csv)


# ---- CLI -------------------------------------------------------------------------------------------------------------------------
def test_cli_routes(monkeypatch):
    from nomad_amd import __main__ as cli
    seen = []

    class _Fake:
        def __init__(self, **kw):
            pass

        def predict(self, mode, nmr, deg, results_path, k=None):
            seen.append(("predict", mode, nmr, deg, results_path, k))
            return pd.DataFrame(), pd.DataFrame()

        def predict_segments(self, mode, nmr, deg, window_s, hop_s, results_path, k=None):
            seen.append(("predict_segments", window_s, hop_s, k))
            return pd.DataFrame(), pd.DataFrame()

        def predict_spans(self, mode, nmr, deg, spans=None, active_db=None, results_path=None, k=None):
            seen.append(("predict_spans", mode, nmr, deg, spans, active_db, results_path, k))
            return pd.DataFrame(), pd.DataFrame()

    monkeypatch.setattr(cli, "Nomad", _Fake)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    monkeypatch.setenv("WORLD_SIZE", "1")
    for extra in ([], ["--window", "2"], ["--spans", "turns.csv", "--knn", "3"], ["--active-db", "35", "--results_path", "out"]):
        monkeypatch.setattr(sys, "argv", ["nomad_amd", "--nmr", "a", "--deg", "b"] + extra)
        cli.main()
    assert seen == [("predict", "dir", "a", "b", None, None), ("predict_segments", 2.0, 1.0, None),
                    ("predict_spans", "dir", "a", "b", "turns.csv", None, None, 3), ("predict_spans", "dir", "a", "b", None, 35.0, "out", None)]


@pytest.mark.parametrize("extra, msg", [(["--spans", "t.csv", "--active-db", "40"], "exclude each other"),
                                        (["--spans", "t.csv", "--window", "2"], "--window"),
                                        (["--active-db", "40", "--window", "2"], "--window"),
                                        (["--spans", "t.csv", "--sweep", "--clip", "1"], "--sweep"),
                                        (["--active-db", "40", "--sweep", "--clip", "1"], "--sweep"),
                                        (["--active-db", "nan"], "finite"), (["--active-db", "loud"], "--active-db")])
def test_cli_exclusions(extra, msg, monkeypatch, capsys):
    from nomad_amd import __main__ as cli
    monkeypatch.setattr(cli, "Nomad", lambda **kw: pytest.fail("the CLI built a Nomad"))
    monkeypatch.setattr(sys, "argv", ["nomad_amd", "--nmr", "a", "--deg", "b"] + extra)
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert e.value.code == 2 and msg in capsys.readouterr().err
