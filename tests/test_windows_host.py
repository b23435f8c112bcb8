"""CPU: the host side of scores over time (``nomad_embed_windows*``, ``Engine.embed_windows*``, ``Nomad.score_over_time`` /
``predict_segments``) - everything that needs no GPU.

* the window geometry, ``weights.num_windows`` and the library's ``nomad_num_windows`` (host arithmetic, no context), against a
  brute-force enumeration of the window starts for every T, win, hop in 1 .. 40;
* seconds <-> frames and the ``start_s`` / ``end_s`` columns;
* the refusals that are decided on the host, each before anything touches an engine;
* the tables and the CSV of ``predict_segments``, driven through a fake engine (the mechanism of
  ``test_eval_host.py::test_get_embeddings_csv_takes_the_model_it_is_given``) that "embeds" a window as its clip's length, its
  first frame and its frame count, so that every row of the table can be traced to the window it came from.
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
from nomad_amd.nomad import Nomad, segments_tables, window_frames, window_times
from nomad_amd.weights import num_frames, num_windows

nomad_mod = sys.modules["nomad_amd.nomad"]     # (the package attribute `nomad` is the lazy singleton, not the module)
RANGE = range(1, 41)
NEW = ("nomad_num_windows", "nomad_embed_windows", "nomad_embed_windows_ragged")


def _starts(T, win, hop):
    """Brute force: a clip no longer than the window is one window; otherwise every start k * hop whose window fits."""
    if T <= win:
        return [0]
    return [t for t in range(0, T, hop) if t + win <= T]


def test_num_windows_against_enumeration():
    for T in RANGE:
        for win in RANGE:
            for hop in RANGE:
                starts = _starts(T, win, hop)
                assert num_windows(T, win, hop) == len(starts), (T, win, hop)
                assert starts == [k * hop for k in range(len(starts))]


def test_window_rows_never_reach_past_the_clip():
    for T in RANGE:
        for win in RANGE:
            for hop in RANGE:
                W, n = num_windows(T, win, hop), min(win, T)
                assert W >= 1 and (W - 1) * hop + n <= T, (T, win, hop)
                # ... and the next window would: the count is the largest that fits
                assert T <= win or W * hop + win > T, (T, win, hop)


def test_library_agrees_with_python(built_lib):
    lib = _lib.load()
    for T in RANGE:
        for win in RANGE:
            for hop in RANGE:
                assert lib.nomad_num_windows(T, win, hop) == num_windows(T, win, hop), (T, win, hop)
    for bad in ((0, 4, 2), (-1, 4, 2), (10, 0, 2), (10, 4, 0), (10, -3, 2), (10, 4, -1)):
        assert lib.nomad_num_windows(*bad) <= 0, bad
        with pytest.raises(ValueError, match="num_windows"):
            num_windows(*bad)


def test_binding_and_header_carry_the_new_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nomad_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} is not declared in include/nomad_hip.h"
    assert _lib.SIGNATURES["nomad_num_windows"] == (C.c_int, [C.c_int] * 3)
    # ctx, wav, B, n_samples, precision, win, hop, head_w, head_b, emb, workspace, workspace_bytes, stream
    res, args = _lib.SIGNATURES["nomad_embed_windows"]
    assert res is C.c_int and len(args) == 13 and [i for i, t in enumerate(args) if t is C.c_int] == [2, 3, 4, 5, 6]
    assert args[11] is C.c_size_t
    # ctx, wav, B, stride, lengths, precision, win, hop, head_w, head_b, emb, workspace, workspace_bytes, stream
    res, args = _lib.SIGNATURES["nomad_embed_windows_ragged"]
    assert res is C.c_int and len(args) == 14 and [i for i, t in enumerate(args) if t is C.c_int] == [2, 3, 5, 6, 7]
    assert args[4] == C.POINTER(C.c_int) and args[12] is C.c_size_t
    # entry points were added, none changed: the binary-interface number stays
    assert int(re.search(r"#define NOMAD_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 3


# ---- seconds <-> frames ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seconds, frames", [(4.0, 200), (2.0, 100), (0.02, 1), (0.001, 1), (0.03, 2), (0.07, 4), (1, 50), (0.5, 25),
                                             (np.float32(0.5), 25), (30.0, 1500)])
def test_seconds_to_frames(seconds, frames):
    assert window_frames(seconds, seconds) == (frames, frames)
    assert frames == max(1, round(float(seconds) * 50))


def test_window_and_hop_convert_on_their_own():
    assert window_frames(4.0, 2.0) == (200, 100) and window_frames(0.1, 3) == (5, 150)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), None, "4", True])
def test_bad_seconds_are_refused(bad):
    with pytest.raises(ValueError, match="window_s"):
        window_frames(bad, 1.0)
    with pytest.raises(ValueError, match="hop_s"):
        window_frames(1.0, bad)


@pytest.mark.parametrize("T, win, hop", [(1, 1, 1), (65, 64, 1), (130, 65, 65), (40, 3, 2), (40, 4, 9), (7, 200, 100), (1499, 200, 100)])
def test_window_times(T, win, hop):
    start, end = window_times(T, win, hop)
    W, n = num_windows(T, win, hop), min(win, T)
    assert start.shape == end.shape == (W,) and start.dtype == end.dtype == np.float64
    for k in range(W):
        assert start[k] == pytest.approx(k * hop * 0.02, abs=1e-12)
        assert end[k] == pytest.approx(start[k] + (n * 320 + 80) / 16000, abs=1e-12)
        # the samples the window's frames see: frame t reads samples [320 t, 320 t + 400)
        assert end[k] * 16000 == pytest.approx(320 * (k * hop + n - 1) + 400, abs=1e-6)
    # on the 3-decimal grid the CSV writer prints exactly
    assert np.array_equal(np.rint(start * 1000) / 1000.0, start) and np.array_equal(np.rint(end * 1000) / 1000.0, end)
    assert end[-1] * 16000 <= 320 * (T - 1) + 400 + 1e-6        # never past the clip's last frame


def test_one_frame_of_receptive_field():
    """T frames need 320 (T - 1) + 400 samples: the end of a whole-clip window is the clip's length."""
    for T in (1, 2, 65, 200):
        assert num_frames(320 * (T - 1) + 400) == T
        assert window_times(T, T, 1)[1][0] == pytest.approx((320 * (T - 1) + 400) / 16000)


# ---- segments_tables --------------------------------------------------------------------------------------------------------
def test_segments_tables():
    frames, win, hop = [450, 30, 199], 200, 100
    counts = [num_windows(t, win, hop) for t in frames]
    assert counts == [3, 1, 1]
    scores = np.array([0.12345, 0.5, 0.7006, 1.0, 0.25])
    df, avg = segments_tables(["a", "b", "c"], frames, scores, win, hop)
    assert list(df.columns) == ["Test File", "start_s", "end_s", "NOMAD"]
    assert list(df["Test File"]) == ["a", "a", "a", "b", "c"]
    assert list(df["start_s"]) == [0.0, 2.0, 4.0, 0.0, 0.0]
    assert list(df["end_s"]) == [4.005, 6.005, 8.005, 0.605, 3.985]
    assert list(df["NOMAD"]) == [0.123, 0.5, 0.701, 1.0, 0.25]
    assert avg.index.name == "Test File" and list(avg.index) == ["a", "b", "c"] and list(avg.columns) == ["NOMAD"]
    assert list(avg["NOMAD"]) == [round(float(scores[:3].mean()), 3), 1.0, 0.25]
    with pytest.raises(ValueError, match="window scores"):
        segments_tables(["a", "b", "c"], frames, scores[:-1], win, hop)
    with pytest.raises(ValueError, match="window scores"):
        segments_tables(["a", "b"], frames, scores, win, hop)
    empty, empty_avg = segments_tables([], [], np.zeros(0), win, hop)
    assert len(empty) == 0 and len(empty_avg) == 0 and list(empty.columns) == ["Test File", "start_s", "end_s", "NOMAD"]


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


def test_score_over_time_refusals():
    n = _nomad(_NoEngine())
    wav, refs = torch.zeros(2, 1, 4000), torch.zeros(3, 256)
    for kw in (dict(window_s=0), dict(hop_s=-1.0), dict(window_s=float("nan"))):
        with pytest.raises(ValueError, match="positive number of seconds"):
            n.score_over_time(wav, refs, **kw)
    for bad in (torch.zeros(3, 255), torch.zeros(256), torch.zeros(2, 3, 256)):
        with pytest.raises(ValueError, match=r"\(Nr, 256\)"):
            n.score_over_time(wav, bad)
    with pytest.raises(ValueError, match="at least one reference"):
        n.score_over_time(wav, torch.zeros(0, 256))
    with pytest.raises(TypeError, match="floating-point"):
        n.score_over_time(wav, torch.zeros(3, 256, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\(B,1,N\) or \(B,N\)"):
        n.score_over_time(torch.zeros(2, 2, 4000), refs)
    with pytest.raises(ValueError, match="no gradient"):
        n.score_over_time(wav.clone().requires_grad_(True), refs)
    with pytest.raises(ValueError, match="no gradient"):
        n.score_over_time(wav, refs.clone().requires_grad_(True))
    with pytest.raises(ValueError, match=r"lengths\[1\]"):
        n.score_over_time(wav, refs, lengths=[4000, 399])


class _CheckOnlyEngine(nomad_mod.Engine):
    """``Engine._check_windows`` without a context: ``enable`` and the device check answer, nothing else exists."""

    def __init__(self):
        self.device, self.enabled = torch.device("cpu"), []

    def enable(self, precision):
        if precision not in _lib.PRECISION:
            raise ValueError("precision must be 'fp32', 'bf16x3' or 'bf16'")
        self.enabled.append(precision)
        return _lib.PRECISION[precision]

    def _check_dev(self, t, name):
        if not (t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous fp32 tensor")

    def close(self):
        pass


def test_engine_refusals_come_before_anything_is_enabled():
    eng = _CheckOnlyEngine()
    wav, head = torch.zeros(2, 4000), (torch.zeros(256, 768), torch.zeros(256))
    for win, hop in ((0, 1), (1, 0), (-5, 2), (4, -2)):
        with pytest.raises(ValueError, match="at least 1 frame"):
            eng.embed_windows(wav, win, hop)
        with pytest.raises(ValueError, match="at least 1 frame"):
            eng.embed_windows_ragged([wav[0]], win, hop)
    with pytest.raises(ValueError, match="at least 1 frame"):
        eng.embed_windows_ragged([wav[0]])                      # win and hop have no default worth guessing
    for precision in ("bf16", "bf16x3"):
        with pytest.raises(ValueError, match=f"the {precision} path has no head override"):
            eng.embed_windows(wav, 4, 2, precision=precision, head=head)
        with pytest.raises(ValueError, match=f"the {precision} path has no head override"):
            eng.embed_windows_ragged([wav[0]], 4, 2, precision=precision, head=head)
    with pytest.raises(ValueError, match="precision must be"):
        eng.embed_windows(wav, 4, 2, precision="fp16")
    with pytest.raises(ValueError, match="head weight must be"):
        eng.embed_windows(wav, 4, 2, head=(head[0].double(), head[1]))
    assert eng.enabled == []
    assert eng._check_windows(4, 2, "bf16", None) == (4, 2, _lib.PRECISION["bf16"], None, None) and eng.enabled == ["bf16"]


# ---- predict_segments through a fake engine --------------------------------------------------------------------------------------
class _FakeEngine:
    """Window k of a clip -> the embedding [clip length, first frame, frames, 0, ...]; a whole file -> [length, 0, ...].  The
    "distance" of a window to the references is length / 1e5 + first frame / 1e3 (+ the number of references), so every score
    names its window."""
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
        assert waves is None
        self.calls.append(("embed_ragged", precision, list(packed[1])))
        out = np.zeros((len(packed[1]), 256), dtype=np.float32)
        out[:, 0] = packed[1]
        return out

    def embed_windows_ragged(self, waves, win, hop, precision="fp32", packed=None):
        assert waves is None
        self.calls.append(("embed_windows_ragged", precision, list(packed[1]), win, hop))
        counts = [num_windows(num_frames(n), win, hop) for n in packed[1]]
        rows = [[n, k * hop, min(win, num_frames(n))] for n, c in zip(packed[1], counts) for k in range(c)]
        emb = torch.zeros(len(rows), 256)
        emb[:, :3] = torch.tensor(rows, dtype=torch.float32)
        return emb, counts

    def pairwise(self, emb, ref, want_matrix=True):
        assert not want_matrix and ref.shape[1] == 256
        return None, (emb[:, 0].double() / 1e5 + emb[:, 1].double() / 1e3 + ref.shape[0])

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
        name = os.path.basename(p)[:-4]
        return np.zeros((1, LENS.get(name, 16000)), dtype=np.float32)
    n.load_processing = load
    n.NATIVE_WAV_THREADS = 0            # the files are empty: everything goes through load_processing
    return n


def test_predict_segments_tables_and_csv(folders):
    nmr, deg, tmp = folders
    assert [num_frames(n) for n in LENS.values()] == [450, 12, 200, 300]
    eng = _FakeEngine()
    n = _pipeline_nomad(eng)
    out = tmp / "out"
    out.mkdir()
    df, avg = n.predict_segments("dir", nmr, deg, window_s=4.0, hop_s=2.0, results_path=str(out), max_batch_samples=150000)
    listed = [f[:-4] for f in os.listdir(deg)]                              # one row per window, files in listing order
    counts = {"long": 3, "short": 1, "exact": 1, "mid": 2}
    assert list(df.columns) == ["Test File", "start_s", "end_s", "NOMAD"]
    assert list(df["Test File"]) == [f for f in listed for _ in range(counts[f])]
    for f in listed:
        rows = df[df["Test File"] == f].reset_index(drop=True)
        T = num_frames(LENS[f])
        start, end = window_times(T, 200, 100)
        assert list(rows["start_s"]) == list(start) and list(rows["end_s"]) == list(end)
        want = [round(LENS[f] / 1e5 + k * 100 / 1e3 + 3, 3) for k in range(counts[f])]       # 3 references
        assert list(rows["NOMAD"]) == want, f
        assert avg.loc[f, "NOMAD"] == pytest.approx(np.mean([LENS[f] / 1e5 + k * 100 / 1e3 + 3 for k in range(counts[f])]), abs=5.01e-4)
    assert list(avg.index) == listed
    # the references were embedded whole, the test files in windows, in more than one staged batch
    assert [c[0] for c in eng.calls if c[0] == "embed_ragged"] and all(c[3:] == (200, 100) for c in eng.calls if c[0] == "embed_windows_ragged")
    assert sorted(l for c in eng.calls if c[0] == "embed_ragged" for l in c[2]) == [16000] * 3
    assert [l for c in eng.calls if c[0] == "embed_windows_ragged" for l in c[2]] == [LENS[f] for f in listed]
    assert sum(c[0] == "embed_windows_ragged" for c in eng.calls) >= 2
    # segments.csv is the table
    back = pd.read_csv(out / "segments.csv")
    assert list(back.columns) == list(df.columns) and len(back) == len(df)
    assert list(back["Test File"]) == list(df["Test File"])
    for col in ("start_s", "end_s", "NOMAD"):
        assert np.array_equal(back[col].to_numpy(dtype=np.float64), df[col].to_numpy(dtype=np.float64)), col
    assert sorted(os.listdir(out)) == ["segments.csv"]


def test_predict_segments_without_results_path_writes_nothing(folders, monkeypatch):
    nmr, deg, tmp = folders
    monkeypatch.chdir(tmp)
    before = sorted(os.listdir(tmp))
    df, avg = _pipeline_nomad(_FakeEngine()).predict_segments("dir", nmr, deg, window_s=1.0, hop_s=0.5)
    assert len(df) == sum(num_windows(num_frames(n), 50, 25) for n in LENS.values()) and len(avg) == len(LENS)
    assert sorted(os.listdir(tmp)) == before


def test_predict_segments_argument_checks_are_those_of_predict(folders):
    nmr, deg, _ = folders
    n = _pipeline_nomad(_NoEngine())
    for kw, msg in ((dict(nmr=None), "nmr_path not specified"), (dict(deg=None), "test_path not specified"),
                    (dict(mode="file"), "Mode value file is not valid"), (dict(nmr=nmr + "x"), "non-matching reference files"),
                    (dict(deg=deg + "x"), "Path to the test files"), (dict(mode="csv"), "File .* does not exist")):
        args = dict(mode="dir", nmr=nmr, deg=deg)
        args.update(kw)
        with pytest.raises(Exception, match=msg):
            n.predict_segments(**args)
    with pytest.raises(ValueError, match="window_s"):
        n.predict_segments("dir", nmr, deg, window_s=0.0)


def test_predict_segments_refuses_a_process_group_of_several_ranks(folders, monkeypatch):
    nmr, deg, _ = folders
    n = _pipeline_nomad(_NoEngine())
    monkeypatch.setattr(nomad_mod, "_dist_info", lambda group=None: (2, 0, True))
    with pytest.raises(RuntimeError, match="2 ranks"):
        n.predict_segments("dir", nmr, deg)


def test_cli_has_the_window_flags():
    text = open(os.path.join(ROOT, "nomad_amd", "__main__.py")).read()
    assert '"--window"' in text and '"--hop"' in text and "predict_segments" in text and ".predict(a.mode" in text
