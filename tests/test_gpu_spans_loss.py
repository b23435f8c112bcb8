"""GPU: ``Nomad.score_spans`` as a differentiable quantity and what carries it: ``head_rows_bwd_kernel<SpanRows>`` +
``head_spans_scatter_kernel`` (the span head's backward), ``nomad_embed_train_spans_ragged`` / ``nomad_embed_spans_backward_ragged``,
``Engine.embed_train_spans_ragged`` / ``embed_spans_backward_ragged``.  Every engine call runs inside ``guard.guarded()``: outputs,
the span scratch and the workspaces at exactly the size asked for, between guards.

Clips are those of tests/test_gpu_windows.py (T = 1, 65 and 130 frames), as one ragged batch with 0.5 stored behind every length.

Bits.  With one row per window of the geometries win 4 hop 9, win 65 hop 65 and win 20 hop 5 and the same ``demb``, the embeddings
and ``dwav`` are ``embed_train_windows_ragged``'s and ``embed_windows_backward_ragged``'s, bit for bit; two identical calls give
the same bits; a clip's row of ``dwav`` is that of its own B = 1 call; a clip without a row gets an all-zero, finite row; samples
behind a length are zero.  ``references.grad`` is ``cdist_backward``'s, ``k=2`` goes through ``knn`` / ``knn_backward``; without
a gradient ``score_spans`` has the bits of the scoring forward.

Gradient and value against float64 for rows windows cannot express (ROWS, those of tests/test_gpu_spans.py), by the method of
tests/test_gpu_windows_loss.py: the oracle runs every clip at its exact length (``O.backbone`` with feature_grad_mult, ``O.head``
with the checkpoint's ``embedding_layer`` on the concatenation of each row's spans, the float64 mean distance to 5 unit-norm
references, a random float64 upstream per row, ``torch.autograd.grad``), once in float64 and once in fp32; ``ref64.check`` with
``ref64.C`` = 8 for fp32 and ``C_X3P`` = 80 for ``Nomad(precision="bf16x3")``.  A column of ``embedding_layer.1.weight`` is zeroed
when any row's mean of that channel lies within ``ref64.KINK`` of 0 in float64 (at most 64 of 768, asserted; 0 for these rows).

Worst err_gpu / e32 measured on one MI355X (``ref64.check`` prints it per case):

  fgm   fp32 gradient  fp32 value   bf16x3 gradient  bf16x3 value
  0.1   2.33           1.47         16.62            5.06
  1.0   2.13           1.47         13.93            5.06
  constant in front of e32: ref64.C = 8             C_X3P = 80

No case uses more than 0.29 of its bound; ``score_windows``' own gradient sits at 1.4 - 2.5 and 11 - 15 (tests/test_gpu_windows_loss.py).
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

pytestmark = pytest.mark.gpu

NR = 5
T_CLIPS = (1, 65, 130)
ROWS = [[[(0, 1)]],
        [[(0, 1), (2, 3), (4, 5)], [(20, 40), (41, 42)], [(10, 30)], [(25, 35)]],
        [[(3, 40), (50, 120)], [(0, 63), (64, 65), (66, 130)], [(129, 130)]]]
WINDOWS = [(4, 9), (65, 65), (20, 5)]


def _wav(n, seed):
    g = torch.Generator().manual_seed(seed * 1000003 + n)
    return (0.1 * torch.randn(n, generator=g)).clamp(-1, 1)


def _padded(clips):
    """(B,1,N) with 0.5 behind every length: samples that are never read."""
    n = max(c.numel() for c in clips)
    out = torch.full((len(clips), 1, n), 0.5)
    for i, c in enumerate(clips):
        out[i, 0, :c.numel()] = c
    return out


def _table(rows, idx=(0, 1, 2)):
    return span_table(rows, [T_CLIPS[i] for i in idx], unit="frames")[0]


def _window_rows(T, win, hop):
    n = min(win, T)
    return [[(k * hop, k * hop + n)] for k in range(num_windows(T, win, hop))]


@pytest.fixture(scope="module")
def data(sd0):
    gen = torch.Generator().manual_seed(177)
    refs = torch.randn(NR, 256, generator=gen, dtype=torch.float64)
    refs = (refs / refs.norm(dim=1, keepdim=True)).float()
    clips = [_wav(ref64.n_for(T), 70 + i) for i, T in enumerate(T_CLIPS)]
    assert [num_frames(c.numel()) for c in clips] == list(T_CLIPS)
    sd64 = ref64.cast(sd0, torch.float64)
    undecided = torch.zeros(768, dtype=torch.bool)
    with torch.no_grad():
        x64 = [O.backbone(sd64, c[None].double(), required_seq_len_multiple=2)[0][0] for c in clips]
    for x, clip_rows in zip(x64, ROWS):
        for row in clip_rows:
            undecided |= torch.cat([x[a:b] for a, b in row]).mean(0).abs() < ref64.KINK
    assert int(undecided.sum()) <= 64, int(undecided.sum())
    print(f"SPANS LOSS {int(undecided.sum())} head columns zeroed")
    sd = {k: v.clone() for k, v in sd0.items()}
    sd["embedding_layer.1.weight"][:, undecided] = 0.0
    up = torch.randn(sum(len(r) for r in ROWS), generator=gen, dtype=torch.float64)
    yield {"sd": sd, "refs": refs, "clips": clips, "up": up}
    for cache in (_oracle_cache, _sd_cache):
        cache.clear()


def _nomad(data, precision):
    from nomad_amd.nomad import Nomad
    return Nomad(weights=data["sd"], precision=precision)


@pytest.fixture(scope="module")
def nmd_f32(built_lib, data):
    nmd = _nomad(data, "fp32")
    yield nmd
    nmd.engine.close()


@pytest.fixture(scope="module")
def nmd_x3(built_lib, data):
    nmd = _nomad(data, "bf16x3")
    yield nmd
    nmd.engine.close()


# ---- the oracle: computed once per feature_grad_mult, never changed ------------------------------------------------------------
_oracle_cache, _sd_cache = {}, {}


def _oracle(data, mult):
    """-> {dtype: (row scores (R,) float64, [d <up, scores> / d clip])}: the clips' rows in the engine's order."""
    if mult not in _oracle_cache:
        out = {}
        for dt in (torch.float64, torch.float32):
            if dt not in _sd_cache:
                _sd_cache[dt] = ref64.cast(data["sd"], dt)
            hw, hb = _sd_cache[dt]["embedding_layer.1.weight"], _sd_cache[dt]["embedding_layer.1.bias"]
            scores, grads, at = [], [], 0
            for clip, clip_rows in zip(data["clips"], ROWS):
                w = clip[None].to(dt).requires_grad_(True)
                x = O.backbone(_sd_cache[dt], w, feature_grad_mult=mult, required_seq_len_multiple=2)[0][0]
                e = torch.cat([O.head(torch.cat([x[a:b] for a, b in row])[None], hw, hb) for row in clip_rows])
                s = (e.double()[:, None, :] - data["refs"].double()[None]).norm(dim=-1).mean(1)   # the distance in float64, as the engine takes it
                (g,) = torch.autograd.grad((s * data["up"][at:at + s.numel()]).sum(), w)
                at += s.numel()
                scores.append(s.detach())
                grads.append(g[0])
            out[dt] = (torch.cat(scores), grads)
        _oracle_cache[mult] = out
    return _oracle_cache[mult]


def _backward(nmd, data, rows=ROWS, mult=0.1, idx=(0, 1, 2), up=None, k=None):
    """``score_spans`` with a gradient on the clips ``idx`` (``lengths``, 0.5 behind them) and its backward -> (scores, counts,
    gradient (B,1,N), lengths)."""
    clips = [data["clips"][i] for i in idx]
    lens = [c.numel() for c in clips]
    eng = nmd.engine
    prev = eng.feature_grad_mult
    eng.feature_grad_mult = mult
    try:
        x = _padded(clips).cuda().requires_grad_(True)
        s, counts = nmd.score_spans(x, data["refs"].cuda(), rows, lengths=lens, unit="frames", k=k)
        s.backward((data["up"] if up is None else up).cuda())
    finally:
        eng.feature_grad_mult = prev
    return s.detach(), counts, x.grad, lens


def _gradient_case(nmd, data, mult, c):
    case = f"score_spans {nmd.precision} fgm={mult:g}"
    ref = _oracle(data, mult)
    (s64, g64), (s32, g32) = ref[torch.float64], ref[torch.float32]
    with guard.guarded(case=case):
        s, counts, grad, lens = _backward(nmd, data, mult=mult)
        torch.cuda.synchronize()
    assert counts == [len(r) for r in ROWS] and s.shape == (sum(counts),) and s.dtype == torch.float64
    assert grad.shape == (3, 1, max(lens)) and bool(torch.isfinite(grad).all())
    for i, n in enumerate(lens):
        assert not grad[i, 0, n:].any(), f"clip {i}: a gradient behind its length"
    ref64.check(case + " gradient", {f"d{i}": grad[i, 0, :n].cpu() for i, n in enumerate(lens)},
                {f"d{i}": g for i, g in enumerate(g64)}, {f"d{i}": g for i, g in enumerate(g32)}, c=c)
    half_ulp = float(np.spacing(np.float32(s64.abs().max().item()))) / 2
    ref64.check(case + " value", s.cpu(), s64, s32, e32_min={"": half_ulp}, c=c)


@pytest.mark.parametrize("mult", [0.1, 1.0])
def test_gradient_vs_float64(nmd_f32, data, mult):
    _gradient_case(nmd_f32, data, mult, ref64.C)


@pytest.mark.parametrize("mult", [0.1, 1.0])
def test_gradient_bf16x3_vs_float64(nmd_x3, data, mult):
    from test_gpu_forward_f64 import C_X3P
    assert nmd_x3.engine.gemm_precision == "bf16x3"
    _gradient_case(nmd_x3, data, mult, C_X3P)


# ---- bits against merged code ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win, hop", WINDOWS)
def test_one_span_rows_have_the_windows_gradient_bits(nmd_f32, data, win, hop):
    eng = nmd_f32.engine
    lens = [c.numel() for c in data["clips"]]
    table = _table([_window_rows(T, win, hop) for T in T_CLIPS])
    g = torch.Generator().manual_seed(win * 100 + hop)
    with guard.guarded(case=f"spans backward = windows backward, win={win} hop={hop}"):
        x = _padded(data["clips"]).cuda()
        emb_w, counts, layers_w, saved_w, batch_w = eng.embed_train_windows_ragged(x, win, hop, lens)
        demb = torch.randn(sum(counts), 256, generator=g).cuda()
        want = eng.embed_windows_backward_ragged(batch_w, layers_w, saved_w, demb, win, hop)
        emb_s, layers_s, saved_s, batch_s = eng.embed_train_spans_ragged(x, table, lens)
        got = eng.embed_spans_backward_ragged(batch_s, layers_s, saved_s, demb, table)
        torch.cuda.synchronize()
    assert torch.equal(emb_s, emb_w) and torch.equal(layers_s, layers_w)
    assert got.shape == want.shape and bool(torch.isfinite(got).all()) and got.abs().max() > 0
    assert torch.equal(got, want), f"{int((got != want).any(1).sum())} of 3 clips differ from the windowed backward"
    for i, n in enumerate(lens):
        assert not got[i, n:].any(), f"clip {i}: a gradient behind its length"


def test_repeatable_batch_invariant_and_zero_for_a_clip_without_a_row(nmd_f32, data):
    counts = [len(r) for r in ROWS]
    with guard.guarded(case="score_spans batch invariance"):
        s, c, grad, lens = _backward(nmd_f32, data)
        s2, _, grad2, _ = _backward(nmd_f32, data)
        own, at = [], 0
        for i in range(3):
            own.append(_backward(nmd_f32, data, rows=[ROWS[i]], idx=(i,), up=data["up"][at:at + counts[i]]))
            at += counts[i]
        up_holes = torch.cat([data["up"][:counts[0]], data["up"][counts[0] + counts[1]:]])
        sh, ch, gh, _ = _backward(nmd_f32, data, rows=[ROWS[0], [], ROWS[2]], up=up_holes)
        torch.cuda.synchronize()
    assert c == counts and torch.equal(s, s2) and torch.equal(grad, grad2), "two identical calls differ"
    at = 0
    for i, (so, co, go, _) in enumerate(own):
        assert co == [counts[i]] and torch.equal(so, s[at:at + counts[i]]), f"clip {i}: the scores differ from its own call"
        assert go.abs().max() > 0 and torch.equal(go[0, 0], grad[i, 0, :lens[i]]), f"clip {i}: the gradient differs from its own B = 1 call"
        at += counts[i]
    assert ch == [counts[0], 0, counts[2]] and torch.equal(sh, torch.cat([s[:counts[0]], s[counts[0] + counts[1]:]]))
    assert bool(torch.isfinite(gh).all()) and not gh[1].any(), "a clip without a row must get exact zeros"
    assert torch.equal(gh[0], grad[0]) and torch.equal(gh[2], grad[2])


def test_references_gradient_knn_and_the_no_grad_path(nmd_f32, data):
    nmd, eng = nmd_f32, nmd_f32.engine
    refs, up = data["refs"].cuda(), data["up"].cuda()
    lens = [c.numel() for c in data["clips"]]
    table = _table(ROWS)
    with guard.guarded(case="score_spans d / d references, k, no gradient"):
        x = _padded(data["clips"]).cuda()
        waves = [x[i, 0, :n] for i, n in enumerate(lens)]
        # nothing requires a gradient: the scoring forward's rows and Engine.pairwise, also under no_grad with leaves that ask
        plain, counts = nmd.score_spans(x, refs, ROWS, lengths=lens, unit="frames")
        emb = eng.embed_spans_ragged(waves, table)
        want = eng.pairwise(emb, refs, want_matrix=False)[1]
        with torch.no_grad():
            req, _ = nmd.score_spans(x.clone().requires_grad_(True), refs.clone().requires_grad_(True), ROWS, lengths=lens, unit="frames")
            mean, _ = nmd.score_spans(x, refs, ROWS, lengths=lens, unit="frames", reduction="mean")
            k2, _ = nmd.score_spans(x, refs, ROWS, lengths=lens, unit="frames", k=2)
        want_k2 = eng.knn(emb, refs, 2)[2]
        # only the references: the scoring forward's rows, cdist_backward's gradient
        r = refs.clone().requires_grad_(True)
        nmd.score_spans(x, r, ROWS, lengths=lens, unit="frames")[0].backward(up)
        want_r = eng.cdist_backward(emb, refs, g_mean=up, want_a=False, want_b=True)[1]
        # both, with k = 2: the rows are embed_train_spans_ragged's, selection and gradients are knn's / knn_backward's
        xg, r2 = x.clone().requires_grad_(True), refs.clone().requires_grad_(True)
        sk, _ = nmd.score_spans(xg, r2, ROWS, lengths=lens, unit="frames", k=2)
        sk.backward(up)
        emb_t, layers, saved, batch = eng.embed_train_spans_ragged(x, table, lens)
        _, idx, mean_k = eng.knn(emb_t, refs, 2)
        demb, dref = eng.knn_backward(emb_t, refs, idx, g_score=up, want_a=True, want_b=True)
        dwav = eng.embed_spans_backward_ragged(batch, layers, saved, demb, table)
        torch.cuda.synchronize()
    assert counts == [len(r_) for r_ in ROWS] and plain.dtype == torch.float64 and not plain.requires_grad
    assert torch.equal(plain, want) and torch.equal(req, want) and not req.requires_grad
    assert mean.dim() == 0 and torch.equal(mean, want.mean()) and torch.equal(k2, want_k2)
    assert r.grad.dtype == torch.float32 and torch.equal(r.grad, want_r)
    assert torch.equal(sk.detach(), mean_k) and torch.equal(r2.grad, dref)
    assert torch.equal(xg.grad.reshape(dwav.shape), dwav) and xg.grad.abs().max() > 0


# ---- buffers and refusals at the C ABI ------------------------------------------------------------------------------------------
def _ints(v):
    return (C.c_int * len(v))(*v)


class _Call:
    """``nomad_embed_spans_backward_ragged`` for the three clips and ROWS, with every buffer the test's own."""

    def __init__(self, eng, data):
        self.eng, self.lib = eng, eng.lib
        self.lens = [c.numel() for c in data["clips"]]
        self.table = _table(ROWS)
        self.wav = _padded(data["clips"]).cuda()[:, 0].contiguous()
        self.emb, self.layers, self.saved, _ = eng.embed_train_spans_ragged(self.wav, self.table, self.lens)
        self.R, self.S = len(self.table[0]), len(self.table[2])
        self.demb = torch.randn(self.R, 256, generator=torch.Generator().manual_seed(9)).cuda()
        nb, ns = C.c_size_t(), C.c_size_t()
        assert self.lib.nomad_backward_workspace_bytes_ragged(eng.ctx, 3, _ints(self.lens), C.byref(nb)) == 0
        assert self.lib.nomad_spans_scratch_bytes(3, self.R, self.S, 1, C.byref(ns)) == 0
        self.ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
        self.scratch = torch.empty(ns.value, dtype=torch.uint8, device="cuda")
        self.dwav = torch.empty_like(self.wav)

    def fill(self, value):
        for t in (self.ws.view(torch.float32), self.scratch.view(torch.float32), self.dwav):
            t.fill_(value)

    def __call__(self, **kw):
        a = dict(ctx=self.eng.ctx, R=self.R, row_clip=self.table[0], row_ptr=self.table[1], spans=[t for s in self.table[2] for t in s],
                 hw=None, hb=None, demb=self.demb.data_ptr(), dwav=self.dwav.data_ptr(), scratch=self.scratch.data_ptr(),
                 scratch_bytes=self.scratch.numel(), ws_bytes=self.ws.numel(), saved_bytes=self.saved.numel())
        a.update(kw)
        return self.lib.nomad_embed_spans_backward_ragged(a["ctx"], self.wav.data_ptr(), 3, self.wav.shape[1], _ints(self.lens), a["R"],
                                                          _ints(a["row_clip"]), _ints(a["row_ptr"]), _ints(a["spans"]), a["hw"], a["hb"],
                                                          self.layers.data_ptr(), self.saved.data_ptr(), a["saved_bytes"], a["demb"],
                                                          a["dwav"], a["scratch"], a["scratch_bytes"], self.ws.data_ptr(), a["ws_bytes"], None)


def test_nothing_relies_on_cleared_buffers_and_refusals(nmd_f32, data, sd0):
    """Frames 42 .. 64 of the T = 65 clip lie in no row of ROWS: their rows of the frame gradient exist only because the scatter
    writes zeros there.  NaN, then 0, in scratch, workspace and output: finite and identical."""
    from nomad_amd.engine import Engine
    eng, lib = nmd_f32.engine, nmd_f32.engine.lib
    with guard.guarded(case="spans backward, poisoned buffers: the forward"):
        call = _Call(eng, data)
        torch.cuda.synchronize()
    out = []
    for value in (float("nan"), 0.0):
        call.fill(value)
        assert call() == 0, lib.nomad_last_error()
        torch.cuda.synchronize()
        out.append(call.dwav.clone())
    assert bool(torch.isfinite(out[0]).all()) and out[0].abs().max() > 0 and torch.equal(out[0], out[1])
    with guard.guarded(case="spans backward, poisoned buffers: the engine's call"):
        own = eng.embed_spans_backward_ragged((call.wav, call.lens), call.layers, call.saved, call.demb, call.table)
        torch.cuda.synchronize()
    assert torch.equal(out[0], own)
    # refusals: status, the entry point named, the output untouched
    good = out[0]
    call.dwav.fill_(7.0)
    who = b"nomad_embed_spans_backward_ragged"
    hw = torch.zeros(256, 768, device="cuda")
    spans = [t for s in call.table[2] for t in s]
    for kw in (dict(R=0), dict(hw=hw.data_ptr()), dict(demb=None), dict(dwav=None), dict(scratch=None), dict(ctx=None),
               dict(row_clip=[0, 1, 1, 1, 0, 2, 2, 2]), dict(row_ptr=[0, 1, 1] + call.table[1][3:]), dict(spans=[0, 2] + spans[2:])):
        assert call(**kw) == _lib.NOMAD_ERR_INVALID, kw
        assert lib.nomad_last_error().startswith(who + b":"), (kw, lib.nomad_last_error())
    for kw in (dict(scratch_bytes=call.scratch.numel() - 256), dict(ws_bytes=1), dict(saved_bytes=1)):
        assert call(**kw) == _lib.NOMAD_ERR_WORKSPACE, kw
        assert lib.nomad_last_error().startswith(who + b":"), (kw, lib.nomad_last_error())
    eng.encoder_depth = 5
    try:
        assert call() == _lib.NOMAD_ERR_INVALID and b"depth is 5" in lib.nomad_last_error()
        with pytest.raises(_lib.NomadHipError, match="depth is 5"):
            eng.embed_train_spans_ragged(call.wav, call.table, call.lens)
        for x in (call.wav, call.wav.clone().requires_grad_(True)):
            with pytest.raises(RuntimeError, match="whole encoder"):
                nmd_f32.score_spans(x, data["refs"].cuda(), ROWS, lengths=call.lens, unit="frames")
    finally:
        eng.encoder_depth = 12
    tuned = Engine(sd0, 0)      # fine-tuning mode: its training-mode forward draws masks this backward does not replay
    try:
        tuned.enable_backward()
        tuned.train_enable()
        assert call(ctx=tuned.ctx) == _lib.NOMAD_ERR_INVALID
        assert lib.nomad_last_error().startswith(who + b":") and b"fine-tuning" in lib.nomad_last_error()
        with pytest.raises(_lib.NomadHipError, match="fine-tuning"):
            tuned.embed_train_spans_ragged(call.wav, call.table, call.lens)
    finally:
        tuned.close()
    torch.cuda.synchronize()
    assert bool((call.dwav == 7.0).all())                                          # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(call.dwav, good)
