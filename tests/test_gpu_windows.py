"""GPU: embeddings and scores over windows of frames (``nomad_embed_windows*``, ``head_rows_kernel<TIn, WindowRows>``; ``Engine.embed_windows*``,
``Nomad.score_over_time`` / ``predict_segments``).

Every engine call runs inside ``guard.guarded()``: the output between guards, the workspace at exactly the size of the plain
forward of the same precision and geometry (the windows take no scratch of their own).

* Bits.  A window that covers a whole clip has the bits of that clip's plain embedding (fp32, bf16x3, bf16; uniform and ragged;
  a custom head on fp32).  A clip's windows do not depend on the batch it is in: inside a ragged batch of three, in its own
  B = 1 call, in the uniform call, and with the batch split over two streams.
* Values, the head on its own input (fp32, bf16x3).  The GPU's own last-layer output (``embed(want_layers=True)`` /
  ``embed_bf16x3(want_layers=True)``, ``layers[11]``) goes through ``O.head`` window by window on the CPU, once in float64 and once
  in fp32: ``err_gpu <= ref64.C * e32 + ref64.FLOOR * top`` (C = 8, FLOOR = 1e-7).
* Values, end to end (all three precisions): ``O.backbone`` in float64 and fp32, ``O.head`` on each window's rows, with the path
  constants of tests/test_gpu_forward_f64.py (C_F32 = 8, C_X3S = 90, C_BF16 = 50 000).
* Scores, ``predict_segments`` on the golden wavs, refusals.

Geometries (clips of T = 1, 65 and 130 frames, ``ref64.n_for``): T = 65 with win 64 hop 1 (window 1 starts at frame 1: chunks of
64 frames count from the window, not the clip); T = 130 with win 65 hop 65 (two chunks, 64 + 1); win 3 hop 2 (fewer frames than
waves); win 1 hop 1 (W = T); win 4 hop 9 (gaps between windows, tail frames dropped); the three clips as one ragged batch.

Worst err_gpu / e32 measured on one MI355X (``ref64.check`` prints it per case):

  check                 path                 worst err_gpu / e32 (where)                                        c
  head on own input     fp32                 6.11 (T 1+65+130, win 64 hop 1: the T = 1 clip's window)            ref64.C = 8
                        fp32-ragged-layers   0.73 (the same case)                                                ref64.C = 8
                        bf16x3               0.60 (T = 65, win 4 hop 9)                                          ref64.C = 8
  end to end            fp32                 3.61 (T = 65, win 1 hop 1); whole clip of the same input 1.67       C_F32 = 8
                        bf16x3               41.15 (T = 65, win 64 hop 1); whole clip 30.84                      C_X3S = 90
                        bf16                 23 959 (T = 65, win 64 hop 1); whole clip 18 255                    C_BF16 = 50 000

The fp32 head check runs on two inputs.  ``embed(want_layers=True)`` is the loss path's forward, which may split K: its
``layers[11]`` is up to 1e-5 away from the last-layer output the scoring forward hands its head, and the CPU reference carries
that difference as if it were the kernel's error - 6.11, and 8.00 (0.95 of the bound) for the T = 1 clip in a case of its own,
which the geometries above do not hold.  ``fp32-ragged-layers`` takes ``layers[11]`` from ``embed_train_ragged(save=False)``,
which never splits K and so has the scoring path's bits: there the kernel is at 0.42 .. 0.73 of fp32's own error, like bf16x3
(whose layer-output forward is its scoring forward).  End to end, windows of one frame have no time mean to average the
forward's error away (err_gpu 6.2e-7 against 9.2e-8 for the whole clip in fp32), and e32 grows with them: no window case
exceeds its path's constant, and none comes closer to it than 0.48 of the bound (bf16, 64 of 65 frames).
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import guard
import ref64
from conftest import GOLD
from nomad_amd import _lib
from nomad_amd.weights import num_frames, num_windows
from oracle import nomad_oracle as O
from test_gpu_forward_f64 import C_BF16, C_F32, C_X3S

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "bf16x3", "bf16"]
C_OF = {"fp32": C_F32, "bf16x3": C_X3S, "bf16": C_BF16}
T_CLIPS = (1, 65, 130)
# (clips of T_CLIPS by index, win, hop)
GEOMETRIES = [((1,), 64, 1), ((2,), 65, 65), ((1,), 3, 2), ((1,), 1, 1), ((1,), 4, 9), ((0, 1, 2), 64, 1), ((0, 1, 2), 4, 9),
              ((0, 1, 2), 65, 65)]
THRESHOLDS = ("F32_SPLIT_ROWS", "BF16_SPLIT_ROWS", "X3_SPLIT_ROWS")


def _gid(g):
    return "T" + "+".join(str(T_CLIPS[i]) for i in g[0]) + f"-win{g[1]}-hop{g[2]}"


def _wav(n, seed):
    g = torch.Generator().manual_seed(seed * 1000003 + n)
    return (0.1 * torch.randn(n, generator=g)).clamp(-1, 1)


def _custom_head(seed=5):
    g = torch.Generator().manual_seed(seed)
    return 0.02 * torch.randn(256, 768, generator=g), 0.01 * torch.randn(256, generator=g)


def _plain(engine, wav, precision, head=None):
    if precision == "fp32":
        return engine.embed(wav, head=head)
    return engine.embed_bf16x3(wav) if precision == "bf16x3" else engine.embed_bf16(wav)


def _windows(engine, waves, win, hop, precision):
    """One clip: the uniform call; several: the ragged one."""
    if len(waves) == 1:
        return engine.embed_windows(waves[0][None].cuda(), win, hop, precision=precision)
    return engine.embed_windows_ragged([w.cuda() for w in waves], win, hop, precision=precision)


def _oracle_windows(xs, w, b, win, hop):
    """``O.head`` on every window's rows of every clip's last-layer output (T,768), in the dtype of the arguments."""
    rows = []
    with torch.no_grad():
        for x in xs:
            T = x.shape[0]
            n = min(win, T)
            rows += [O.head(x[None, k * hop:k * hop + n], w, b) for k in range(num_windows(T, win, hop))]
    return torch.cat(rows)


@pytest.fixture(scope="module")
def clips(sd0):
    """The three clips and, computed once, the oracle's last-layer output of each in float64 and in fp32."""
    waves = [_wav(ref64.n_for(T), 70 + i) for i, T in enumerate(T_CLIPS)]
    assert [num_frames(w.numel()) for w in waves] == list(T_CLIPS)
    x = {}
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            sd = ref64.cast(sd0, dt)
            x[dt] = [O.backbone(sd, w[None].to(dt))[0][0] for w in waves]
    return waves, x


@contextlib.contextmanager
def _thresholds(eng, rows):
    """The three split thresholds set on the instance, and the instance left as it was (tests/test_gpu_split_dispatch.py)."""
    before = {k: eng.__dict__[k] for k in THRESHOLDS if k in eng.__dict__}
    for k in THRESHOLDS:
        setattr(eng, k, rows)
    try:
        yield
    finally:
        for k in THRESHOLDS:
            if k in before:
                setattr(eng, k, before[k])
            else:
                delattr(eng, k)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))


# ---- bits: a window over a whole clip ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_whole_clip_window_has_the_clips_bits(engine, clips, precision):
    waves, _ = clips
    one = waves[0][None].cuda()                                                   # T = 1
    three = torch.stack([_wav(ref64.n_for(65), 80 + i) for i in range(3)]).cuda()     # B = 3, T = 65
    rag = [waves[0].cuda(), waves[2].cuda()]                                      # T = 1 next to T = 130
    with guard.guarded(case=f"whole-clip windows [{precision}]"):
        got = [engine.embed_windows(one, 1, 1, precision=precision), engine.embed_windows(one, 200, 100, precision=precision),
               engine.embed_windows(three, 65, 7, precision=precision), engine.embed_windows(three, 66, 1, precision=precision),
               engine.embed_windows_ragged(rag, 130, 3, precision=precision), engine.embed_windows_ragged(rag, 200, 100, precision=precision)]
        want = [_plain(engine, one, precision), _plain(engine, three, precision), engine.embed_ragged(rag, precision=precision)]
        torch.cuda.synchronize()
    for (emb, counts), ref in zip(got, (want[0], want[0], want[1], want[1], want[2], want[2])):
        assert counts == [1] * ref.shape[0] and emb.dtype == torch.float32
        assert torch.equal(emb, ref), f"{int((emb != ref).any(1).sum())} of {ref.shape[0]} whole-clip windows differ from the clip's embedding"


def test_whole_clip_window_with_a_custom_head(engine):
    hw, hb = (t.cuda() for t in _custom_head())
    wav = torch.stack([_wav(ref64.n_for(65), 90 + i) for i in range(3)]).cuda()
    with guard.guarded(case="whole-clip windows, custom head"):
        emb, counts = engine.embed_windows(wav, 65, 1, head=(hw, hb))
        rag, rcounts = engine.embed_windows_ragged([w for w in wav], 70, 2, head=(hw, hb))
        ref = engine.embed(wav, head=(hw, hb))
        other = engine.embed(wav)
        torch.cuda.synchronize()
    assert counts == rcounts == [1, 1, 1]
    assert torch.equal(emb, ref) and torch.equal(rag, ref) and not torch.equal(ref, other)


# ---- bits: batch invariance -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win, hop", [(4, 3), (64, 1), (1, 1)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_clips_windows_do_not_depend_on_its_batch(engine, clips, precision, win, hop):
    waves = [w.cuda() for w in clips[0]]
    with guard.guarded(case=f"batch invariance [{precision}] win={win} hop={hop}"):
        emb, counts = engine.embed_windows_ragged(waves, win, hop, precision=precision)
        again, _ = engine.embed_windows_ragged(waves, win, hop, precision=precision)
        own = [engine.embed_windows_ragged([w], win, hop, precision=precision) for w in waves]
        uni = [engine.embed_windows(w[None], win, hop, precision=precision) for w in waves]
        torch.cuda.synchronize()
    assert counts == [num_windows(T, win, hop) for T in T_CLIPS] and emb.shape == (sum(counts), 256)
    assert bool(torch.isfinite(emb).all()) and torch.equal(emb, again)
    at = 0
    for i, c in enumerate(counts):
        assert own[i][1] == uni[i][1] == [c]
        assert torch.equal(emb[at:at + c], own[i][0]), f"clip {i} (T = {T_CLIPS[i]}) differs from its own ragged call"
        assert torch.equal(emb[at:at + c], uni[i][0]), f"clip {i} (T = {T_CLIPS[i]}) differs from its own uniform call"
        at += c


@pytest.mark.parametrize("precision", PRECISIONS)
def test_uniform_equals_ragged_and_a_split_changes_no_bit(engine, precision):
    """Three clips of T = 65: the uniform call, the ragged call, and both again with the thresholds at 1 (the uniform batch is cut
    1 + 2, so a wrong output offset shows), against the calls with no split."""
    wav = torch.stack([_wav(ref64.n_for(65), 100 + i) for i in range(3)]).cuda()
    rag_waves = [_wav(ref64.n_for(T), 110 + i).cuda() for i, T in enumerate((1, 2, 64))]   # the cut by audio length: 2 + 1
    with guard.guarded(case=f"split [{precision}]"):
        with _thresholds(engine, 0):
            uni, counts = engine.embed_windows(wav, 4, 9, precision=precision)
            rag, rcounts = engine.embed_windows_ragged([w for w in wav], 4, 9, precision=precision)
            mixed, mcounts = engine.embed_windows_ragged(rag_waves, 2, 1, precision=precision)
        torch.cuda.synchronize()
        engine._ws_side.clear()
        with _thresholds(engine, 1):
            uni2, _ = engine.embed_windows(wav, 4, 9, precision=precision)
            assert engine._ws_side, "the uniform call was expected to split (no side workspace was made)"
            engine._ws_side.clear()
            mixed2, mcounts2 = engine.embed_windows_ragged(rag_waves, 2, 1, precision=precision)
            assert engine._ws_side, "the ragged call was expected to split (no side workspace was made)"
        torch.cuda.synchronize()
    assert counts == rcounts == [7, 7, 7] and mcounts == mcounts2 == [1, 1, 63]
    assert torch.equal(uni, rag), "the uniform call differs from the ragged call on the same clips"
    assert _same(uni, uni2), "the split uniform call differs from the unsplit one"
    assert _same(mixed, mixed2), "the split ragged call differs from the unsplit one"


# ---- values: the head on its own input --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def own_layers(engine, clips):
    """The GPU's own last-layer output of every clip, per precision: (T,768) fp32 on the host."""
    out = {}
    for precision, fwd in (("fp32", engine.embed), ("bf16x3", engine.embed_bf16x3)):
        out[precision] = [fwd(w[None].cuda(), want_layers=True)[1][11][0].cpu() for w in clips[0]]
    # fp32 once more, from the ragged layer-output forward: it never splits K, so its layers[11] has the bits the scoring
    # forward hands its head, where embed(want_layers=True) - the loss path's forward, which may split K - is up to 1e-5 away
    out["fp32-ragged-layers"] = [engine.embed_train_ragged([w.cuda()], save=False)[1][11].cpu() for w in clips[0]]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=_gid)
@pytest.mark.parametrize("precision", ["fp32", "fp32-ragged-layers", "bf16x3"])
def test_head_on_its_own_input_against_float64(engine, sd0, clips, own_layers, precision, geometry):
    idx, win, hop = geometry
    case = f"windows head[{precision}] {_gid(geometry)}"
    with guard.guarded(case=case):
        emb, counts = _windows(engine, [clips[0][i] for i in idx], win, hop, precision.split("-")[0])
        torch.cuda.synchronize()
    assert counts == [num_windows(T_CLIPS[i], win, hop) for i in idx]
    w, b = sd0["embedding_layer.1.weight"], sd0["embedding_layer.1.bias"]
    xs = [own_layers[precision][i] for i in idx]
    r64 = _oracle_windows([x.double() for x in xs], w.double(), b.double(), win, hop)
    r32 = _oracle_windows(xs, w.float(), b.float(), win, hop)
    ref64.check(case, emb.cpu(), r64, r32)


# ---- values: end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=_gid)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_windows_against_float64(engine, sd0, clips, precision, geometry):
    idx, win, hop = geometry
    case = f"windows[{precision}] {_gid(geometry)}"
    with guard.guarded(case=case):
        emb, _ = _windows(engine, [clips[0][i] for i in idx], win, hop, precision)
        whole = torch.cat([_plain(engine, clips[0][i][None].cuda(), precision) for i in idx])
        torch.cuda.synchronize()
    w, b = sd0["embedding_layer.1.weight"], sd0["embedding_layer.1.bias"]
    r = {dt: _oracle_windows([clips[1][dt][i] for i in idx], w.to(dt), b.to(dt), win, hop) for dt in (torch.float64, torch.float32)}
    # the whole-clip embedding of the same input, for comparison: the constants were measured on these
    big = 1 << 20
    r_whole = {dt: _oracle_windows([clips[1][dt][i] for i in idx], w.to(dt), b.to(dt), big, big) for dt in (torch.float64, torch.float32)}
    ref64.check(case + " (whole clip)", whole.cpu(), r_whole[torch.float64], r_whole[torch.float32], c=C_OF[precision])
    ref64.check(case, emb.cpu(), r[torch.float64], r[torch.float32], c=C_OF[precision])


# ---- scores --------------------------------------------------------------------------------------------------------------------
def _references(n=5, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, 256, generator=g), dim=1)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_score_over_time(engine, clips, precision):
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine, precision)
    # a batch of fewer than BF16X3_MIN_SAMPLES samples stays on fp32 buffers under precision="bf16x3", in score_over_time as in
    # score and in the file pipeline
    precision = "fp32" if precision == "bf16x3" else precision
    refs = _references().cuda()
    wav = torch.stack([_wav(ref64.n_for(65), 120 + i) for i in range(3)]).cuda()
    lens = [ref64.n_for(T) for T in (65, 1, 30)]
    with guard.guarded(case=f"score_over_time [{precision}]"):
        scores, counts = nomad.score_over_time(wav[:, None, :], refs, window_s=0.4, hop_s=0.1)          # win 20, hop 5
        emb, ecounts = engine.embed_windows(wav, 20, 5, precision=precision)
        want = engine.pairwise(emb, refs, want_matrix=False)[1]
        rag_scores, rag_counts = nomad.score_over_time(wav, refs, window_s=0.08, hop_s=0.06, lengths=lens)   # win 4, hop 3
        rag_emb, _ = engine.embed_windows_ragged([wav[i, :n] for i, n in enumerate(lens)], 4, 3, precision=precision)
        rag_want = engine.pairwise(rag_emb, refs, want_matrix=False)[1]
        # a window at least as long as the clip: the score of the clip
        whole, wcounts = nomad.score_over_time(wav, refs, window_s=1.3, hop_s=0.5)                     # win 65
        whole_len, _ = nomad.score_over_time(wav, refs, window_s=4.0, hop_s=2.0, lengths=lens)
        with torch.no_grad():
            plain, plain_len = nomad.score(wav, refs), nomad.score(wav, refs, lengths=lens)
        torch.cuda.synchronize()
    assert counts == ecounts == [10, 10, 10] and scores.dtype == torch.float64 and scores.shape == (30,)
    assert torch.equal(scores, want)
    assert rag_counts == [num_windows(T, 4, 3) for T in (65, 1, 30)] and torch.equal(rag_scores, rag_want)
    assert wcounts == [1, 1, 1] and torch.equal(whole, plain) and torch.equal(whole_len, plain_len)
    assert not scores.requires_grad


def test_predict_segments_on_the_golden_wavs(engine, tmp_path):
    from nomad_amd.nomad import Nomad, window_times
    nomad = Nomad.from_engine(engine)
    nmr, deg = os.path.join(GOLD, "wavs", "nmr-data"), os.path.join(GOLD, "wavs", "test-data")
    with guard.guarded(case="predict_segments"):
        df, avg = nomad.predict_segments("dir", nmr, deg, window_s=1.0, hop_s=0.5, results_path=str(tmp_path))
        refs = torch.cat([engine.embed(nomad.load_processing(os.path.join(nmr, f)).cuda()) for f in os.listdir(nmr)])
        files = os.listdir(deg)
        own = [nomad.score_over_time(nomad.load_processing(os.path.join(deg, f)).cuda(), refs, 1.0, 0.5) for f in files]
        torch.cuda.synchronize()
    assert list(df.columns) == ["Test File", "start_s", "end_s", "NOMAD"] and list(avg.index) == [f.split(".")[0] for f in files]
    assert list(df["Test File"]) == [f.split(".")[0] for f, (_, c) in zip(files, own) for _ in range(c[0])]     # one row per window, in file order
    at = 0
    for f, (scores, counts) in zip(files, own):
        T = num_frames(nomad.load_processing(os.path.join(deg, f)).shape[1])
        rows = df.iloc[at:at + counts[0]]
        at += counts[0]
        assert counts == [num_windows(T, 50, 25)] and counts[0] > 1
        start, end = window_times(T, 50, 25)
        assert list(rows["start_s"]) == list(start) and list(rows["end_s"]) == list(end)
        # the table's rows are the file's own scores, rounded to 3 decimals; the per-file mean is the mean of its rows
        assert np.abs(rows["NOMAD"].to_numpy() - scores.cpu().numpy()).max() <= 5.01e-4, f
        assert abs(avg.loc[f.split(".")[0], "NOMAD"] - rows["NOMAD"].mean()) <= 1.001e-3, f
        assert avg.loc[f.split(".")[0], "NOMAD"] == pytest.approx(round(float(scores.mean()), 3), abs=1e-9), f
    assert at == len(df) and os.path.isfile(tmp_path / "segments.csv")


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    lib = engine.lib
    n = ref64.n_for(65)
    wav = _wav(2 * n, 130).reshape(2, n).cuda()
    good, counts = engine.embed_windows(wav, 4, 9)
    good = good.clone()
    emb = torch.full((sum(counts), 256), 7.0, device="cuda")
    need = engine.workspace_bytes(2, n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    hw, hb = (t.cuda() for t in _custom_head())
    engine.enable("bf16x3")

    def call(B=2, w=wav.data_ptr(), ns=n, p=0, win=4, hop=9, head=(None, None), e=emb.data_ptr(), wsp=ws.data_ptr(), nb=need):
        return lib.nomad_embed_windows(engine.ctx, w, B, ns, p, win, hop, head[0], head[1], e, wsp, nb, None)

    def call_ragged(win=4, hop=9, p=0, lens=(n, n), head=(None, None), nb=need):
        return lib.nomad_embed_windows_ragged(engine.ctx, wav.data_ptr(), 2, n, (C.c_int * 2)(*lens), p, win, hop, head[0], head[1],
                                              emb.data_ptr(), ws.data_ptr(), nb, None)
    for kw in (dict(win=0), dict(hop=0), dict(win=-1), dict(B=0), dict(w=None), dict(e=None), dict(wsp=None), dict(ns=399), dict(p=3),
               dict(head=(hw.data_ptr(), None)), dict(head=(None, hb.data_ptr())), dict(p=1, head=(hw.data_ptr(), hb.data_ptr()))):
        assert call(**kw) == _lib.NOMAD_ERR_INVALID, kw
        assert b"nomad_embed_windows" in lib.nomad_last_error(), kw
    for kw in (dict(win=0), dict(hop=0), dict(p=7), dict(lens=(n, 399)), dict(p=1, head=(hw.data_ptr(), hb.data_ptr()))):
        assert call_ragged(**kw) == _lib.NOMAD_ERR_INVALID, kw
        assert b"nomad_embed_windows_ragged" in lib.nomad_last_error(), kw
    assert call(nb=need - 1) == _lib.NOMAD_ERR_WORKSPACE and b"nomad_embed_windows: workspace" in lib.nomad_last_error()
    need_r = engine._forward_size_ragged("fp32", [n, n])
    assert need_r <= need or call_ragged(nb=need) == _lib.NOMAD_ERR_WORKSPACE
    assert call_ragged(nb=min(need, need_r) - 1) == _lib.NOMAD_ERR_WORKSPACE
    engine.encoder_depth = 5
    try:
        assert call() == _lib.NOMAD_ERR_INVALID and b"depth is 5" in lib.nomad_last_error()
        assert call_ragged() == _lib.NOMAD_ERR_INVALID and b"depth is 5" in lib.nomad_last_error()
        with pytest.raises(_lib.NomadHipError, match="depth is 5"):
            engine.embed_windows(wav, 4, 9)
    finally:
        engine.encoder_depth = 12
    with pytest.raises(ValueError, match="at least 1 frame"):
        engine.embed_windows(wav, 0, 1)
    torch.cuda.synchronize()
    assert bool((emb == 7.0).all())                                               # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(emb, good)
