"""GPU: embeddings over caller-given spans of frames (``nomad_embed_spans_ragged``, ``head_rows_kernel<TIn, SpanRows>``;
``Engine.embed_spans_ragged``, ``Nomad.score_spans`` / ``active_spans`` / ``predict_spans``) and ``nomad_frame_energy``.

Every engine call runs inside ``guard.guarded()``: outputs and the span scratch between guards, the workspace at exactly the size
of the plain forward of the same precision.  Clips are those of tests/test_gpu_windows.py: T = 1, 65, 130 frames.

* Bits against merged code (fp32, bf16x3, bf16).  One row per window of a window geometry has the bits of
  ``embed_windows_ragged``; the rows ``[(0, T)]`` and ``[(0, 64), (64, 130)]`` have the bits of ``embed_ragged``; a clip's rows do
  not depend on its batch, and a clip without a row changes nothing for the others.
* Values against float64, for rows that windows cannot express (ROWS).  The head on its own input - ``layers[11]`` of
  ``embed_train_ragged(save=False)``, the "fp32-ragged-layers" path of the window tests - with ``ref64.C = 8``; end to end
  (``O.backbone`` + ``O.head`` on the concatenated rows) with the path constants of tests/test_gpu_forward_f64.py.
* ``nomad_frame_energy`` against numpy float64 within 402 * 2**-53 of each value, exact zeros, batch invariance.
* Refusals through ctypes, one per item of the header's list; a poison run (NaN, then 0, in scratch, workspace and output).

Worst err_gpu / e32 measured on one MI355X (``ref64.check`` prints it per case), over the eight rows of ROWS:

  check                 path                 worst err_gpu / e32                            c
  head on own input     fp32-ragged-layers   0.69                                           ref64.C = 8
  end to end            fp32                 1.38                                           C_F32 = 8
                        bf16x3               10.32                                          C_X3S = 90
                        bf16                 7 126                                          C_BF16 = 50 000

No case uses more than 0.18 of its bound.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import guard
import ref64
from nomad_amd import _lib
from nomad_amd.nomad import span_table
from nomad_amd.weights import num_frames, num_windows
from oracle import nomad_oracle as O
from test_gpu_forward_f64 import C_BF16, C_F32, C_X3S

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "bf16x3", "bf16"]
C_OF = {"fp32": C_F32, "bf16x3": C_X3S, "bf16": C_BF16}
T_CLIPS = (1, 65, 130)
# (clips of T_CLIPS by index, win, hop): the window geometries the one-span rows reproduce
GEOMETRIES = [((1,), 64, 1), ((2,), 65, 65), ((1,), 3, 2), ((1,), 4, 9), ((0, 1, 2), 20, 5)]
# rows windows cannot express, per clip of T_CLIPS
ROWS = [[[(0, 1)]],
        [[(0, 1), (2, 3), (4, 5)], [(20, 40), (41, 42)], [(10, 30)], [(25, 35)]],
        [[(3, 40), (50, 120)], [(0, 63), (64, 65), (66, 130)], [(129, 130)]]]


def _gid(g):
    return "T" + "+".join(str(T_CLIPS[i]) for i in g[0]) + f"-win{g[1]}-hop{g[2]}"


def _wav(n, seed):
    g = torch.Generator().manual_seed(seed * 1000003 + n)
    return (0.1 * torch.randn(n, generator=g)).clamp(-1, 1)


def _window_rows(T, win, hop):
    n = min(win, T)
    return [[(k * hop, k * hop + n)] for k in range(num_windows(T, win, hop))]


def _table(rows, idx=(0, 1, 2)):
    return span_table(rows, [T_CLIPS[i] for i in idx], unit="frames")[0]


def _oracle_rows(xs, rows, w, b):
    """``O.head`` on the concatenation of every row's spans of its clip's last-layer output (T,768), in the dtype of the arguments."""
    out = []
    with torch.no_grad():
        for x, clip_rows in zip(xs, rows):
            out += [O.head(torch.cat([x[a:b_] for a, b_ in row])[None], w, b) for row in clip_rows]
    return torch.cat(out)


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


# ---- bits against merged code ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=_gid)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_span_rows_have_the_windows_bits(engine, clips, precision, geometry):
    idx, win, hop = geometry
    waves = [clips[0][i].cuda() for i in idx]
    table = _table([_window_rows(T_CLIPS[i], win, hop) for i in idx], idx)
    with guard.guarded(case=f"spans = windows [{precision}] {_gid(geometry)}"):
        got = engine.embed_spans_ragged(waves, table, precision=precision)
        want, counts = engine.embed_windows_ragged(waves, win, hop, precision=precision)
        torch.cuda.synchronize()
    assert got.shape == want.shape == (sum(counts), 256) and got.dtype == torch.float32
    assert torch.equal(got, want), f"{int((got != want).any(1).sum())} of {want.shape[0]} one-span rows differ from their windows"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_whole_clip_rows_have_the_clips_bits(engine, clips, precision):
    waves = [w.cuda() for w in clips[0]]
    rows = [[[(0, 1)]], [[(0, 65)], [(0, 64), (64, 65)]], [[(0, 130)], [(0, 64), (64, 130)], [(0, 1), (1, 129), (129, 130)]]]
    with guard.guarded(case=f"whole-clip rows [{precision}]"):
        got = engine.embed_spans_ragged(waves, _table(rows), precision=precision)
        want = engine.embed_ragged(waves, precision=precision)
        torch.cuda.synchronize()
    for r, c in enumerate((0, 1, 1, 2, 2, 2)):
        assert torch.equal(got[r], want[c]), f"row {r} (clip {c}, T = {T_CLIPS[c]}) differs from the clip's embedding"


def test_whole_clip_row_with_a_custom_head(engine, clips):
    g = torch.Generator().manual_seed(5)
    head = ((0.02 * torch.randn(256, 768, generator=g)).cuda(), (0.01 * torch.randn(256, generator=g)).cuda())
    waves = [w.cuda() for w in clips[0]]
    with guard.guarded(case="whole-clip rows, custom head"):
        got = engine.embed_spans_ragged(waves, _table([[[(0, T)]] for T in T_CLIPS]), head=head)
        want, other = engine.embed_ragged(waves, head=head), engine.embed_ragged(waves)
        torch.cuda.synchronize()
    assert torch.equal(got, want) and not torch.equal(want, other)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_clips_rows_do_not_depend_on_its_batch(engine, clips, precision):
    waves = [w.cuda() for w in clips[0]]
    with guard.guarded(case=f"batch invariance [{precision}]"):
        emb = engine.embed_spans_ragged(waves, _table(ROWS), precision=precision)
        again = engine.embed_spans_ragged(waves, _table(ROWS), precision=precision)
        own = [engine.embed_spans_ragged([w], _table([ROWS[i]], (i,)), precision=precision) for i, w in enumerate(waves)]
        # the middle clip without a row: the others keep their bits; so do they with the batch split over two streams
        holes = engine.embed_spans_ragged(waves, _table([ROWS[0], [], ROWS[2]]), precision=precision)
        before = {k: engine.__dict__[k] for k in ("F32_SPLIT_ROWS", "BF16_SPLIT_ROWS", "X3_SPLIT_ROWS") if k in engine.__dict__}
        try:
            engine.F32_SPLIT_ROWS = engine.BF16_SPLIT_ROWS = engine.X3_SPLIT_ROWS = 1
            engine._ws_side.clear()
            split = engine.embed_spans_ragged(waves, _table(ROWS), precision=precision)
            assert engine._ws_side, "the call was expected to split (no side workspace was made)"
        finally:
            for k in ("F32_SPLIT_ROWS", "BF16_SPLIT_ROWS", "X3_SPLIT_ROWS"):
                if k in before:
                    setattr(engine, k, before[k])
                else:
                    delattr(engine, k)
        torch.cuda.synchronize()
    counts = [len(r) for r in ROWS]
    assert emb.shape == (sum(counts), 256) and bool(torch.isfinite(emb).all()) and torch.equal(emb, again) and torch.equal(emb, split)
    at = 0
    for i, c in enumerate(counts):
        assert torch.equal(emb[at:at + c], own[i]), f"clip {i} (T = {T_CLIPS[i]}) differs from its own B = 1 call"
        at += c
    assert torch.equal(holes, torch.cat([emb[:counts[0]], emb[counts[0] + counts[1]:]]))


# ---- values against float64 ---------------------------------------------------------------------------------------------------
def test_head_on_its_own_input_against_float64(engine, sd0, clips):
    waves = [w.cuda() for w in clips[0]]
    case = "spans head[fp32-ragged-layers]"
    with guard.guarded(case=case):
        emb = engine.embed_spans_ragged(waves, _table(ROWS))
        xs = [engine.embed_train_ragged([w], save=False)[1][11].cpu() for w in waves]
        torch.cuda.synchronize()
    w, b = sd0["embedding_layer.1.weight"], sd0["embedding_layer.1.bias"]
    r64 = _oracle_rows([x.double() for x in xs], ROWS, w.double(), b.double())
    r32 = _oracle_rows(xs, ROWS, w.float(), b.float())
    ref64.check(case, emb.cpu(), r64, r32)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_spans_against_float64(engine, sd0, clips, precision):
    waves = [w.cuda() for w in clips[0]]
    case = f"spans[{precision}]"
    with guard.guarded(case=case):
        emb = engine.embed_spans_ragged(waves, _table(ROWS), precision=precision)
        torch.cuda.synchronize()
    w, b = sd0["embedding_layer.1.weight"], sd0["embedding_layer.1.bias"]
    r = {dt: _oracle_rows(clips[1][dt], ROWS, w.to(dt), b.to(dt)) for dt in (torch.float64, torch.float32)}
    ref64.check(case, emb.cpu(), r[torch.float64], r[torch.float32], c=C_OF[precision])


# ---- frame energies -------------------------------------------------------------------------------------------------------------
def _energy64(w):
    x = w.double().numpy()
    return np.array([(x[320 * t:320 * t + 400] ** 2).sum() / 400.0 for t in range(num_frames(x.shape[0]))])


def test_frame_energy(engine, clips):
    waves = list(clips[0]) + [torch.zeros(ref64.n_for(7))]
    stride = max(w.numel() for w in waves) + 8
    padded = torch.full((len(waves), stride), 0.5)          # 0.5 stored behind every length
    for i, w in enumerate(waves):
        padded[i, :w.numel()] = w
    lens = [w.numel() for w in waves]
    with guard.guarded(case="frame_energy"):
        e = engine.frame_energy([w.cuda() for w in waves])
        own = [engine.frame_energy([w.cuda()]) for w in waves]
        buf = padded.cuda()
        e_pad = torch.empty(e.shape[0], dtype=torch.float64, device="cuda")
        _lib.check(engine.lib.nomad_frame_energy(engine.ctx, buf.data_ptr(), len(waves), stride, (C.c_int * len(lens))(*lens),
                                                 e_pad.data_ptr(), None), "nomad_frame_energy")
        torch.cuda.synchronize()
    assert e.dtype == torch.float64 and e.shape == (sum(T_CLIPS) + 7,)
    want = np.concatenate([_energy64(w) for w in waves])
    got = e.cpu().numpy()
    assert np.all(np.abs(got - want) <= 402 * 2.0 ** -53 * want), float(np.max(np.abs(got - want) / np.maximum(want, 1e-300)))
    assert np.all(got[-7:] == 0.0) and np.all(got[:-7] > 0.0)
    assert torch.equal(e, torch.cat(own)), "a clip's energies depend on its batch"
    assert torch.equal(e, e_pad), "samples behind a length were read"


def test_active_spans_and_the_speech_only_score(engine, clips):
    from nomad_amd.nomad import Nomad, active_frames
    nomad = Nomad.from_engine(engine)
    wav = _wav(ref64.n_for(130), 77).clone()
    wav[320 * 40:320 * 100] *= 1e-4                             # 60 quiet frames in the middle
    refs = torch.nn.functional.normalize(torch.randn(5, 256, generator=torch.Generator().manual_seed(3)), dim=1).cuda()
    with guard.guarded(case="active_spans"):
        act = nomad.active_spans(wav[None].cuda())
        e = engine.frame_energy([wav.cuda()]).cpu().numpy()
        scores, counts = nomad.score_spans(wav[None].cuda(), refs, [[s] for s in act], unit="frames")
        emb = engine.embed_spans_ragged([wav.cuda()], _table([[act[0]]], (2,)))
        want = engine.pairwise(emb, refs, want_matrix=False)[1]
        torch.cuda.synchronize()
    assert act == [active_frames(e, 40.0, 5, 15)] and len(act[0]) == 2
    assert act[0][0][0] == 0 and 38 <= act[0][0][1] <= 41 and 98 <= act[0][1][0] <= 100 and act[0][1][1] == 130
    assert counts == [1] and scores.dtype == torch.float64 and torch.equal(scores, want)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _ints(v):
    return (C.c_int * len(v))(*v)


def test_refusals(engine):
    lib = engine.lib
    n = ref64.n_for(65)
    wav = _wav(2 * n, 130).reshape(2, n).cuda()
    table = span_table([[[(0, 10), (20, 30)]], [[(5, 65)], [(0, 1)]]], [65, 65], unit="frames")[0]
    good = engine.embed_spans_ragged([w for w in wav], table).clone()
    emb = torch.full((3, 256), 7.0, device="cuda")
    need = engine._forward_size_ragged("fp32", [n, n])
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    sb = C.c_size_t()
    assert lib.nomad_spans_scratch_bytes(2, 3, 4, 0, C.byref(sb)) == 0 and sb.value >= 4 * (2 * 3 + 1 + 2 * 4 + 3)
    sb1 = C.c_size_t()
    assert lib.nomad_spans_scratch_bytes(2, 3, 4, 1, C.byref(sb1)) == 0 and sb1.value >= sb.value + 4 * 768 * 3
    for bad in ((0, 3, 4), (2, 0, 4), (2, 3, 2)):
        assert lib.nomad_spans_scratch_bytes(*bad, 0, C.byref(sb1)) == _lib.NOMAD_ERR_INVALID
    assert lib.nomad_spans_scratch_bytes(2, 3, 4, 0, None) == _lib.NOMAD_ERR_INVALID
    scratch = torch.empty(sb.value, dtype=torch.uint8, device="cuda")
    hw = torch.zeros(256, 768, device="cuda")
    hb = torch.zeros(256, device="cuda")
    engine.enable("bf16x3")

    def call(R=3, row_clip=(0, 1, 1), row_ptr=(0, 2, 3, 4), spans=(0, 10, 20, 30, 5, 65, 0, 1), p=0, head=(None, None), lens=(n, n),
             nb=need, snb=sb.value, null=None):
        args = [_ints(row_clip), _ints(row_ptr), _ints(spans)]
        if null is not None:
            args[null] = None
        return lib.nomad_embed_spans_ragged(engine.ctx, wav.data_ptr(), 2, n, _ints(lens), p, R, args[0], args[1], args[2], head[0],
                                            head[1], emb.data_ptr(), scratch.data_ptr(), snb, ws.data_ptr(), nb, None)

    refused = [(dict(R=0), b"at least one row"), (dict(null=0), b"NULL span table"), (dict(null=1), b"NULL span table"),
               (dict(null=2), b"NULL span table"), (dict(row_clip=(1, 0, 1)), b"row 1 names clip 0 behind"),
               (dict(row_clip=(0, 1, 2)), b"row 2 names clip 2, outside"), (dict(row_clip=(-1, 1, 1)), b"row 0 names clip -1"),
               (dict(row_ptr=(0, 2, 2, 4)), b"row 1 has no span"), (dict(row_ptr=(1, 2, 3, 4)), b"row_ptr[0]"),
               (dict(spans=(-1, 10, 20, 30, 5, 65, 0, 1)), b"row 0, span 0 is [-1, 10)"),
               (dict(spans=(0, 10, 20, 30, 5, 66, 0, 1)), b"row 1, span 0 is [5, 66)"),
               (dict(spans=(0, 10, 20, 30, 5, 65, 1, 1)), b"row 2, span 0 is [1, 1)"),
               (dict(spans=(0, 10, 9, 30, 5, 65, 0, 1)), b"row 0, span 1 [9, 30) overlaps"),
               (dict(spans=(20, 30, 0, 10, 5, 65, 0, 1)), b"row 0, span 1 [0, 10) overlaps or precedes"),
               (dict(lens=(n, 399)), b"row 1, span 0"), (dict(p=7), b"unknown precision"),
               (dict(head=(hw.data_ptr(), None)), b"both be set"), (dict(p=1, head=(hw.data_ptr(), hb.data_ptr())), b"head override")]
    for kw, msg in refused:
        assert call(**kw) == _lib.NOMAD_ERR_INVALID, kw
        err = lib.nomad_last_error()
        assert b"nomad_embed_spans_ragged" in err and msg in err, (kw, err)
    assert call(snb=sb.value - 256) == _lib.NOMAD_ERR_WORKSPACE and b"nomad_embed_spans_ragged: scratch" in lib.nomad_last_error()
    assert call(nb=need - 1) == _lib.NOMAD_ERR_WORKSPACE and b"nomad_embed_spans_ragged: workspace" in lib.nomad_last_error()
    engine.encoder_depth = 5
    try:
        assert call() == _lib.NOMAD_ERR_INVALID and b"depth is 5" in lib.nomad_last_error()
    finally:
        engine.encoder_depth = 12
    with pytest.raises(ValueError, match="row 0, span 1"):
        engine.embed_spans_ragged([w for w in wav], ([0], [0, 2], [(0, 10), (5, 12)]))
    e = torch.full((130,), 7.0, dtype=torch.float64, device="cuda")
    for kw in (dict(B=0), dict(w=None), dict(out=None), dict(lens=(n, 399)), dict(lens=(n, n + 1))):
        rc = lib.nomad_frame_energy(engine.ctx, kw.get("w", wav.data_ptr()), kw.get("B", 2), n, _ints(kw.get("lens", (n, n))),
                                    kw.get("out", e.data_ptr()), None)
        assert rc == _lib.NOMAD_ERR_INVALID and b"nomad_frame_energy" in lib.nomad_last_error(), kw
    torch.cuda.synchronize()
    assert bool((emb == 7.0).all()) and bool((e == 7.0).all())                    # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(emb, good)


# ---- poison ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_poisoned_buffers_change_nothing(engine, clips, precision):
    """Scratch, workspace and output filled with NaN, then with 0: identical, finite results - everything read was written."""
    waves = [w.cuda() for w in clips[0]]
    prec = engine.enable(precision)
    buf, lens = engine._pack(waves)
    row_clip, row_ptr, spans = _table(ROWS)
    flat = [t for s in spans for t in s]
    R = len(row_clip)
    sb = C.c_size_t()
    _lib.check(engine.lib.nomad_spans_scratch_bytes(3, R, len(spans), 0, C.byref(sb)), "nomad_spans_scratch_bytes")
    need = engine._forward_size_ragged(precision, lens)
    out = []
    for byte in (0xFF, 0x00):
        scratch = torch.full((sb.value,), byte, dtype=torch.uint8, device="cuda")
        ws = torch.full((need,), byte, dtype=torch.uint8, device="cuda")
        emb = torch.full((R * 256 * 4,), byte, dtype=torch.uint8, device="cuda")
        _lib.check(engine.lib.nomad_embed_spans_ragged(engine.ctx, buf.data_ptr(), 3, buf.shape[1], _ints(lens), prec, R, _ints(row_clip),
                                                       _ints(row_ptr), _ints(flat), None, None, emb.data_ptr(), scratch.data_ptr(),
                                                       sb.value, ws.data_ptr(), need, None), "nomad_embed_spans_ragged")
        torch.cuda.synchronize()
        out.append(emb.view(torch.float32).view(R, 256).clone())
    assert bool(torch.isfinite(out[0]).all()) and torch.equal(out[0], out[1])
