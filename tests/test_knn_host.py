"""CPU: the host side of the nearest-reference NOMAD score (``nomad_knn*``, ``Engine.knn*``, ``Nomad.score*(k=...)``,
``predict(k=...)``) - everything that needs no GPU.

* ``knn_ref`` (the contract of include/nomad_hip.h in plain torch) against a brute-force selection, under ties, zeros and NaN;
* the new entry points in the header, in the binding and in the built library;
* ``check_k``, and that every refusal comes before an engine sees a call;
* the engine calls of ``score`` / ``score_over_time`` / ``score_windows``: with ``k=None`` the sequence of before, with ``k`` the same
  sequence with ``knn`` in ``pairwise``'s place and ``knn_backward`` in ``cdist_backward``'s - on an engine that only records;
* the three tables of ``predict(k=2)`` on a fake engine that "embeds" a file as its length;
* the CLI's refusal of ``--knn 0``."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import ROOT
from knn_ref import knn_ref, same
from nomad_amd import _lib
from nomad_amd.nomad import Nomad, check_k, nearest_table
from nomad_amd.weights import num_frames, num_windows

NEW = ("nomad_knn_scratch_bytes", "nomad_knn", "nomad_knn_backward_scratch_bytes", "nomad_knn_backward")
NAN, INF = float("nan"), float("inf")


# ---- the helper ------------------------------------------------------------------------------------------------------------------
def _brute(row, k):
    """Selection by repeated minimum under the key (d with NaN as +inf, column): -> (values, columns, score)."""
    left = list(range(len(row)))
    vals, cols = [], []
    for _ in range(k):
        best = min(left, key=lambda j: (INF if math.isnan(row[j]) else row[j], j))
        left.remove(best)
        vals.append(row[best])
        cols.append(best)
    s = 0.0
    for v in vals:
        s += v
    return vals, cols, s / k


@pytest.mark.parametrize("k", [1, 2, 3, 7])
def test_helper_agrees_with_brute_force_under_ties_zeros_and_nan(k):
    rows = [[3.0, 1.0, 2.0, 1.0, 0.0, 5.0, 1.0],            # a triple tie
            [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],            # all equal: the identity permutation
            [2.0, NAN, 1.0, INF, NAN, 1.0, 0.5],            # NaN as +inf: column 1 before the real +inf of column 3, then column 4
            [NAN, NAN, NAN, NAN, NAN, NAN, NAN],
            [7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0]]
    gen = torch.Generator().manual_seed(5)
    rows += torch.randint(0, 4, (20, 7), generator=gen).double().tolist()   # many ties
    dist = torch.tensor(rows, dtype=torch.float64)
    kd, ki, sc = knn_ref(dist, k)
    assert kd.dtype == torch.float64 and ki.dtype == torch.int32 and sc.dtype == torch.float64
    for i, row in enumerate(rows):
        vals, cols, s = _brute(row, k)
        assert ki[i].tolist() == cols, (i, k)
        assert same(kd[i], torch.tensor(vals, dtype=torch.float64)), (i, k)
        assert same(sc[i:i + 1], torch.tensor([s], dtype=torch.float64)), (i, k)
    if k == 7:   # k = Nb: the stable argsort
        assert ki[0].tolist() == [4, 1, 3, 6, 2, 0, 5] and ki[1].tolist() == list(range(7)) and ki[2].tolist() == [6, 2, 5, 0, 1, 3, 4]


# ---- header, binding, library ----------------------------------------------------------------------------------------------------
def test_binding_header_and_library_carry_the_new_entry_points(built_lib):
    text = open(os.path.join(ROOT, "include", "nomad_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = C.CDLL(built_lib)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/nomad_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
    for name in ("nomad_knn_scratch_bytes", "nomad_knn_backward_scratch_bytes"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    # ctx, a, Na, b, Nb, D, k, dist, knn_dist, knn_idx, score, scratch, scratch_bytes, stream
    res, args = _lib.SIGNATURES["nomad_knn"]
    assert res is C.c_int and len(args) == 14 and [i for i, t in enumerate(args) if t is C.c_int] == [2, 4, 5, 6] and args[12] is C.c_size_t
    # ctx, a, Na, b, Nb, D, k, knn_idx, g_knn, g_score, da, db, scratch, scratch_bytes, stream
    res, args = _lib.SIGNATURES["nomad_knn_backward"]
    assert res is C.c_int and len(args) == 15 and [i for i, t in enumerate(args) if t is C.c_int] == [2, 4, 5, 6] and args[13] is C.c_size_t
    # entry points were added, none changed: the binary-interface number and the version prefix stay, and there is no new profile class
    assert int(re.search(r"#define NOMAD_ABI_VERSION (\d+)", code).group(1)) == _lib.ABI_VERSION == 3
    assert _lib.load().nomad_version().startswith(b"nomad_hip 0.3")
    assert "NOMAD_K_KNN" not in text and "NOMAD_K_SELECT" not in text
    # the sizes are host arithmetic: no context, no GPU
    n = C.c_size_t(123)
    real = _lib.load()
    assert real.nomad_knn_scratch_bytes(10000, 1000, 8, C.byref(n)) == 0 and n.value == 16 * 10000 * 8 * 12
    assert real.nomad_knn_backward_scratch_bytes(65, 130, 7, C.byref(n)) == 0 and n.value == 2 * 8 * 65 * 130
    n = C.c_size_t(123)
    for fn in (real.nomad_knn_scratch_bytes, real.nomad_knn_backward_scratch_bytes):
        for Na, Nb, k, p in ((0, 5, 1, C.byref(n)), (5, 0, 1, C.byref(n)), (5, 5, 0, C.byref(n)), (5, 5, 6, C.byref(n)),
                             (5, 100, 65, C.byref(n)), (65535 * 64 + 1, 5, 1, C.byref(n)), (5, 5, 1, None)):
            assert fn(Na, Nb, k, p) == _lib.NOMAD_ERR_INVALID, (Na, Nb, k)
    assert n.value == 123


# ---- check_k ---------------------------------------------------------------------------------------------------------------------
class _NoEngine:
    """An engine nothing may be asked of: the refusals below come before the first engine call."""
    device = torch.device("cpu")

    def __getattr__(self, name):
        raise AssertionError(f"the engine was asked for {name}")


def _nomad(engine, precision="fp32"):
    n = Nomad.__new__(Nomad)            # no GPU: only the host side is under test
    n.engine, n.precision, n.group = engine, precision, None
    return n


BAD_K = [0, -1, 65, 4, 2.0, "2", True, False, [2]]   # against 3 references


def test_check_k():
    for k, Nr in ((1, 1), (3, 3), (64, 64), (64, 1000), (np.int64(2), 5)):
        out = check_k(k, Nr)
        assert out == k and type(out) is int
    for k in BAD_K + [None]:
        with pytest.raises(ValueError):
            check_k(k, 3)
    with pytest.raises(ValueError, match=r"k = 70 .*64.* 1000"):      # the message names both numbers
        check_k(70, 1000)
    with pytest.raises(ValueError, match=r"k = 4 .* 3\b"):
        check_k(4, 3)


@pytest.mark.parametrize("grad", [False, True], ids=["no_grad", "requires_grad"])
def test_a_bad_k_is_refused_before_any_engine_call(grad, tmp_path):
    n = _nomad(_NoEngine())
    wav = torch.zeros(2, 1, 4000, requires_grad=grad)
    refs = torch.zeros(3, 256, requires_grad=grad)
    for k in BAD_K:
        with pytest.raises(ValueError, match="k"):
            n.score(wav, refs, k=k)
        with pytest.raises(ValueError, match="k"):
            n.score_windows(wav, refs, k=k)
        with pytest.raises(ValueError, match="k"):
            n.score_over_time(wav.detach(), refs.detach(), k=k)
        with pytest.raises(ValueError, match="k"):
            n.nearest_references(torch.zeros(2, 256), refs, k)
    (tmp_path / "a").mkdir()
    for k in (0, 65, 1.5, True):      # before a file is listed or read
        with pytest.raises(ValueError, match="k"):
            n.predict("dir", str(tmp_path / "a"), str(tmp_path / "a"), k=k)
        with pytest.raises(ValueError, match="k"):
            n.predict_segments("dir", str(tmp_path / "a"), str(tmp_path / "a"), k=k)
    # score_over_time still produces no gradient, with or without k
    with pytest.raises(ValueError, match="no gradient"):
        n.score_over_time(torch.zeros(2, 1, 4000, requires_grad=True), torch.zeros(3, 256), k=2)


# ---- the engine calls of the score family ----------------------------------------------------------------------------------------
class _Recorder:
    """Records the name of every engine call; embeddings are [row number + 1, 0, ...], the distance of an embedding to a reference
    |emb_0 - ref_0|, and every backward returns zeros of the right shape."""
    device = torch.device("cpu")
    encoder_depth = 12

    def __init__(self):
        self.calls = []

    @staticmethod
    def _emb(rows):
        emb = torch.zeros(rows, 256)
        emb[:, 0] = torch.arange(1, rows + 1)
        return emb

    def embed(self, wav):
        self.calls.append("embed")
        return self._emb(wav.shape[0])

    def embed_ragged(self, waves, precision=None, packed=None):
        self.calls.append("embed_ragged")
        return self._emb(len(waves))

    def embed_train(self, wav):
        self.calls.append("embed_train")
        return self._emb(wav.shape[0]), torch.zeros(1), torch.zeros(1)

    def embed_train_ragged(self, wav, lens):
        self.calls.append("embed_train_ragged")
        return self._emb(wav.shape[0]), torch.zeros(1), torch.zeros(1), (wav, lens)

    def _counts(self, samples, win, hop):
        return [num_windows(num_frames(n), win, hop) for n in samples]

    def embed_windows(self, wav, win, hop, precision="fp32"):
        self.calls.append("embed_windows")
        counts = self._counts([wav.shape[1]] * wav.shape[0], win, hop)
        return self._emb(sum(counts)), counts

    def embed_windows_ragged(self, waves, win, hop, precision="fp32", packed=None):
        self.calls.append("embed_windows_ragged")
        counts = self._counts([int(w.shape[0]) for w in waves], win, hop)
        return self._emb(sum(counts)), counts

    def embed_train_windows(self, wav, win, hop):
        self.calls.append("embed_train_windows")
        counts = self._counts([wav.shape[1]] * wav.shape[0], win, hop)
        return self._emb(sum(counts)), counts, torch.zeros(1), torch.zeros(1)

    def embed_train_windows_ragged(self, wav, win, hop, lens):
        self.calls.append("embed_train_windows_ragged")
        counts = self._counts(lens, win, hop)
        return self._emb(sum(counts)), counts, torch.zeros(1), torch.zeros(1), (wav, lens)

    @staticmethod
    def _dist(emb, ref):
        return (emb[:, :1].double() - ref[:, 0].double()[None, :]).abs()

    def pairwise(self, emb, ref, want_matrix=True):
        self.calls.append(("pairwise", want_matrix))
        d = self._dist(emb, ref)
        return (d if want_matrix else None), d.mean(1)

    def knn(self, a, b, k, want_matrix=False):
        self.calls.append(("knn", k, want_matrix))
        d = self._dist(a, b)
        out = knn_ref(d, k)
        return out + (d,) if want_matrix else out

    def cdist_backward(self, a, b, g_dist=None, g_mean=None, want_a=True, want_b=False):
        self.calls.append(("cdist_backward", g_dist is None, tuple(g_mean.shape), want_a, want_b))
        return (torch.zeros_like(a) if want_a else None), (torch.zeros_like(b) if want_b else None)

    def knn_backward(self, a, b, knn_idx, g_knn=None, g_score=None, want_a=True, want_b=True):
        assert knn_idx.dtype == torch.int32 and knn_idx.shape[0] == a.shape[0]
        self.calls.append(("knn_backward", int(knn_idx.shape[1]), g_knn is None, tuple(g_score.shape), want_a, want_b))
        return (torch.zeros_like(a) if want_a else None), (torch.zeros_like(b) if want_b else None)

    def embed_backward(self, est, layers, saved, dlayers, demb):
        self.calls.append("embed_backward")
        return torch.zeros_like(est)

    def embed_backward_ragged(self, packed, layers, saved, dlayers, demb):
        self.calls.append("embed_backward_ragged")
        return torch.zeros_like(packed[0])

    def embed_windows_backward(self, est, layers, saved, demb, win, hop):
        self.calls.append("embed_windows_backward")
        return torch.zeros_like(est)

    def embed_windows_backward_ragged(self, packed, layers, saved, demb, win, hop):
        self.calls.append("embed_windows_backward_ragged")
        return torch.zeros_like(packed[0])


REFS = torch.zeros(5, 256)
REFS[:, 0] = torch.tensor([10.0, 2.5, 7.0, 1.0, 3.0])
LENS = [4000, 3000]


def _swap(calls, k):
    """Today's sequence with knn / knn_backward in the places of pairwise / cdist_backward."""
    out = []
    for c in calls:
        if isinstance(c, tuple) and c[0] == "pairwise":
            c = ("knn", k, c[1])
        elif isinstance(c, tuple) and c[0] == "cdist_backward":
            c = ("knn_backward", k, True) + c[2:]
        out.append(c)
    return out


def _run(method, k, grad, lengths, ref_grad=False):
    eng = _Recorder()
    n = _nomad(eng)
    wav = torch.zeros(2, 1, 4000, requires_grad=grad)
    refs = REFS.clone().requires_grad_(ref_grad)
    kw = {} if k is None else {"k": k}
    if method == "score":
        out = n.score(wav, refs, lengths=lengths, **kw)
    elif method == "score_over_time":
        out = n.score_over_time(wav, refs, window_s=0.1, hop_s=0.06, lengths=lengths, **kw)[0]
    else:
        out = n.score_windows(wav, refs, window_s=0.1, hop_s=0.06, lengths=lengths, **kw)[0]
    if grad or ref_grad:
        out.sum().backward()
        assert (wav.grad is not None) == grad and (refs.grad is not None) == ref_grad
    return eng.calls, out.detach()


TODAY = {   # the engine calls of the parent commit (k does not exist there): (method, gradient, lengths) -> sequence
    ("score", False, False): ["embed", ("pairwise", False)],
    ("score", False, True): ["embed_ragged", ("pairwise", False)],
    ("score", True, False): ["embed_train", ("pairwise", False), ("cdist_backward", True, (2,), True, False), "embed_backward"],
    ("score", True, True): ["embed_train_ragged", ("pairwise", False), ("cdist_backward", True, (2,), True, False),
                            "embed_backward_ragged"],
    ("score_over_time", False, False): ["embed_windows", ("pairwise", False)],
    ("score_over_time", False, True): ["embed_windows_ragged", ("pairwise", False)],
    ("score_windows", False, False): ["embed_windows", ("pairwise", False)],
    ("score_windows", False, True): ["embed_windows_ragged", ("pairwise", False)],
    ("score_windows", True, False): ["embed_train_windows", ("pairwise", False), ("cdist_backward", True, (6,), True, False),
                                     "embed_windows_backward"],
    ("score_windows", True, True): ["embed_train_windows_ragged", ("pairwise", False), ("cdist_backward", True, (5,), True, False),
                                    "embed_windows_backward_ragged"],
}


@pytest.mark.parametrize("method,grad,ragged", sorted(TODAY))
def test_engine_calls_without_k_are_todays_and_with_k_take_knn(method, grad, ragged):
    lengths = LENS if ragged else None
    calls, out = _run(method, None, grad, lengths)
    assert calls == TODAY[(method, grad, ragged)]
    calls3, out3 = _run(method, 3, grad, lengths)
    assert calls3 == _swap(TODAY[(method, grad, ragged)], 3)
    # the values: the mean over all five references, and over the three nearest
    rows = out.shape[0]
    d = (torch.arange(1, rows + 1).double()[:, None] - REFS[:, 0].double()[None, :]).abs()
    assert torch.equal(out, d.mean(1)) and torch.equal(out3, knn_ref(d, 3)[2])


def test_references_get_their_gradient_through_knn_backward():
    calls, _ = _run("score", 2, False, None, ref_grad=True)
    assert calls == ["embed", ("knn", 2, False), ("knn_backward", 2, True, (2,), False, True)]
    calls, _ = _run("score_windows", 2, True, None, ref_grad=True)
    assert calls == ["embed_train_windows", ("knn", 2, False), ("knn_backward", 2, True, (6,), True, True), "embed_windows_backward"]
    calls, _ = _run("score", None, False, None, ref_grad=True)
    assert calls == ["embed", ("pairwise", False), ("cdist_backward", True, (2,), False, True)]


def test_nearest_references_takes_embeddings_or_waveforms():
    eng = _Recorder()
    n = _nomad(eng)
    emb = _Recorder._emb(4)
    kd, ki = n.nearest_references(emb, REFS, 2)
    assert eng.calls == [("knn", 2, False)]
    assert ki.tolist() == [[3, 1], [1, 3], [4, 1], [4, 1]]           # row 1: references 3 and 4 are both at 1.0 - the lower row
    assert kd.tolist() == [[0.0, 1.5], [0.5, 1.0], [0.0, 0.5], [1.0, 1.5]]
    eng.calls.clear()
    kd2, ki2 = n.nearest_references(torch.zeros(4, 1, 4000), REFS, 2)
    assert eng.calls == ["embed", ("knn", 2, False)] and torch.equal(ki2, ki) and torch.equal(kd2, kd)
    eng.calls.clear()
    n.nearest_references(torch.zeros(2, 4000), REFS, 1, lengths=LENS)
    assert eng.calls == ["embed_ragged", ("knn", 1, False)]
    with pytest.raises(ValueError, match="lengths"):
        n.nearest_references(emb, REFS, 2, lengths=[1, 2, 3, 4])


# ---- predict(k) on a fake engine -------------------------------------------------------------------------------------------------
class _FileEngine:
    """A file is "embedded" as [its length, 0, ...]; the distance of two files is |length - length| / 1e4."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def pack_ragged_host(self, waves):
        lens = [int(w.shape[0]) for w in waves]
        host = np.zeros((len(waves), max(lens)), dtype=np.float32)
        return host, lens

    def embed_ragged(self, waves, precision=None, packed=None):
        out = np.zeros((len(packed[1]), 256), dtype=np.float32)
        out[:, 0] = packed[1]
        return out

    def fetch_async(self, t):
        class F:
            def result(self_inner):
                return t.numpy() if torch.is_tensor(t) else t
        return F()

    @staticmethod
    def _dist(a, b):
        return (a[:, :1].double() - b[:, 0].double()[None, :]).abs() / 1e4

    def pairwise(self, deg, ref, want_matrix=True):
        self.calls.append(("pairwise", want_matrix))
        d = self._dist(deg, ref)
        return d, d.mean(1)

    def knn(self, a, b, k, want_matrix=False):
        self.calls.append(("knn", k, want_matrix))
        d = self._dist(a, b)
        return knn_ref(d, k) + ((d,) if want_matrix else ())


FILES = {"r0": 16000, "r1": 26004, "r2": 21000, "r3": 40000, "near": 21500, "far": 60000, "tie": 18500}


def _folders(tmp_path, refs=("r0", "r1", "r2", "r3"), degs=("near", "far", "tie")):
    nmr, deg = tmp_path / "nmr", tmp_path / "deg"
    nmr.mkdir()
    deg.mkdir()
    for name in refs:
        (nmr / f"{name}.wav").write_bytes(b"")
    for name in degs:
        (deg / f"{name}.wav").write_bytes(b"")
    return str(nmr), str(deg)


def _file_nomad(eng):
    n = _nomad(eng)
    n.model = None
    n.load_processing = lambda p, trim=False: np.zeros((1, FILES[os.path.basename(p)[:-4]]), dtype=np.float32)
    n.NATIVE_WAV_THREADS = 0            # the files are empty: everything goes through load_processing
    return n


def test_predict_with_k_yields_three_tables(tmp_path):
    nmr, deg = _folders(tmp_path)
    out0, out2 = tmp_path / "out0", tmp_path / "out2"
    out0.mkdir()
    out2.mkdir()
    eng0, eng2 = _FileEngine(), _FileEngine()
    res0 = _file_nomad(eng0).predict("dir", nmr, deg, results_path=str(out0))
    res2 = _file_nomad(eng2).predict("dir", nmr, deg, results_path=str(out2), k=2)
    assert len(res0) == 2 and eng0.calls == [("pairwise", True)]                 # the drop-in surface: untouched
    assert len(res2) == 3 and eng2.calls == [("knn", 2, True)]                   # one call in pairwise's place
    avg, dm, near = res2
    assert dm.equals(res0[1])
    assert sorted(os.listdir(out0)) == ["nomad_avg.csv", "nomad_scores.csv"]
    assert sorted(os.listdir(out2)) == ["nomad_avg.csv", "nomad_nearest.csv", "nomad_scores.csv"]
    assert (out2 / "nomad_scores.csv").read_bytes() == (out0 / "nomad_scores.csv").read_bytes()
    refs = [f[:-4] for f in os.listdir(nmr)]
    tests = [f[:-4] for f in os.listdir(deg)]
    assert list(near.index) == tests == list(avg.index) and near.index.name == "Test File"
    assert list(near.columns) == ["Ref 1", "Dist 1", "Ref 2", "Dist 2"]
    for t in tests:
        d = {r: abs(FILES[t] - FILES[r]) / 1e4 for r in refs}
        order = sorted(refs, key=lambda r: (d[r], refs.index(r)))                # ties (r0 and r2 for "tie") by column order
        assert [near.loc[t, "Ref 1"], near.loc[t, "Ref 2"]] == order[:2], t
        assert [near.loc[t, "Dist 1"], near.loc[t, "Dist 2"]] == [round(d[order[0]], 3), round(d[order[1]], 3)], t
        assert avg.loc[t, "NOMAD"] == round((d[order[0]] + d[order[1]]) / 2, 3), t
        assert res0[0].loc[t, "NOMAD"] == round(sum(d.values()) / 4, 3), t
    assert near.loc["near", "Dist 2"] == 0.45                                    # 0.4504 rounded to 3 decimals
    back = pd.read_csv(out2 / "nomad_nearest.csv")
    assert list(back.columns) == ["Test File"] + list(near.columns) and list(back["Test File"]) == tests
    assert list(back["Ref 1"]) == list(near["Ref 1"]) and list(back["Dist 2"]) == list(near["Dist 2"])


def test_predict_with_k_on_an_empty_file_list_and_a_small_bank(tmp_path):
    """csv mode with no test rows (an empty directory already fails in get_embeddings, as in the reference): empty tables, no
    engine call; a bank smaller than k is check_k's error, before the distance stage."""
    nmr, deg = _folders(tmp_path)
    pd.DataFrame({"filename": [os.path.join(nmr, f) for f in os.listdir(nmr)]}).to_csv(tmp_path / "nmr.csv", index=False)
    pd.DataFrame({"filename": [os.path.join(deg, f) for f in os.listdir(deg)]}).to_csv(tmp_path / "deg.csv", index=False)
    pd.DataFrame({"filename": []}).to_csv(tmp_path / "none.csv", index=False)
    out = tmp_path / "out"
    out.mkdir()
    eng = _FileEngine()
    avg, dm, near = _file_nomad(eng).predict("csv", str(tmp_path / "nmr.csv"), str(tmp_path / "none.csv"), results_path=str(out), k=2)
    assert eng.calls == [] and avg.shape == (0, 1) and dm.shape == (0, 4) and len(near) == 0
    assert list(near.columns) == ["Ref 1", "Dist 1", "Ref 2", "Dist 2"]
    assert (out / "nomad_nearest.csv").read_text().strip() == "Test File,Ref 1,Dist 1,Ref 2,Dist 2"
    for nmr_csv, Nr in (("nmr.csv", 4), ("none.csv", 0)):
        with pytest.raises(ValueError, match=r"k = 5 .* %d\b" % Nr):
            _file_nomad(eng).predict("csv", str(tmp_path / nmr_csv), str(tmp_path / "deg.csv"), results_path=str(out), k=5)
    assert eng.calls == []


def test_nearest_table():
    t = nearest_table(["x", "y"], ["a", "b", "c"], [[0.12345, 0.5], [1.0, 2.00049]], [[2, 0], [1, 1]])
    assert t.index.name == "Test File" and list(t.index) == ["x", "y"]
    assert t.to_dict("list") == {"Ref 1": ["c", "b"], "Dist 1": [0.123, 1.0], "Ref 2": ["a", "b"], "Dist 2": [0.5, 2.0]}


# ---- CLI -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", ["0", "65", "-3", "two"])
def test_cli_rejects_a_bad_knn(value, monkeypatch, capsys):
    from nomad_amd import __main__ as cli
    monkeypatch.setattr(cli, "Nomad", lambda **kw: pytest.fail("the CLI built a Nomad"))
    monkeypatch.setattr(sys, "argv", ["nomad_amd", "--nmr", "a", "--deg", "b", "--knn", value])
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert e.value.code == 2 and "--knn" in capsys.readouterr().err


def test_cli_passes_knn_with_and_without_window(monkeypatch):
    from nomad_amd import __main__ as cli
    seen = []

    class _Fake:
        def __init__(self, **kw):
            pass

        def predict(self, mode, nmr, deg, results_path, k=None):
            seen.append(("predict", k))
            return pd.DataFrame(), pd.DataFrame(), pd.DataFrame()

        def predict_segments(self, mode, nmr, deg, window_s, hop_s, results_path, k=None):
            seen.append(("predict_segments", window_s, hop_s, k))
            return pd.DataFrame(), pd.DataFrame()

    monkeypatch.setattr(cli, "Nomad", _Fake)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    monkeypatch.setenv("WORLD_SIZE", "1")
    for extra in (["--knn", "3"], ["--knn", "3", "--window", "2"]):
        monkeypatch.setattr(sys, "argv", ["nomad_amd", "--nmr", "a", "--deg", "b"] + extra)
        cli.main()
    assert seen == [("predict", 3), ("predict_segments", 2.0, 1.0, 3)]
