"""GPU: ``Nomad.score_windows`` - scores over time as a differentiable quantity - and what carries it: ``head_rows_bwd_kernel<WindowRows>`` +
``head_windows_scatter_kernel`` (the windowed head's backward), ``nomad_embed_train_windows*`` / ``nomad_embed_windows_backward*``,
``Engine.embed_train_windows*`` / ``embed_windows_backward*``.  Every engine call runs inside ``guard.guarded()``: outputs, the
per-window scratch and the workspaces at exactly the size asked for, between guards.

Clips and geometries are those of tests/test_gpu_windows.py (T = 1, 65 and 130 frames): T = 65 with win 64 hop 1; T = 130 with
win 65 hop 65 (the chunk loop of the time sum runs twice); win 3 hop 2 (overlap); win 4 hop 9 (gaps between windows and a tail
no window covers: frames whose gradient row is exact zeros); the three clips as one ragged batch (``lengths``, 0.5 stored behind
every length) with win 4 hop 9 (a one-frame clip), win 65 hop 65 (whole-clip windows next to split ones) and win 20 hop 5 (up
to four windows on a frame).

Gradient and value against float64, by the method and constants of tests/ref64.py (``check``: err_gpu <= C e32 + FLOOR top,
C = 8, FLOOR = 1e-7; ``test_gpu_forward_f64.C_X3P`` = 80 in front of e32 for ``Nomad(precision="bf16x3")``, whose gradient path
runs bf16x3 products on fp32 buffers).  The oracle runs every clip at its exact length: ``O.backbone`` (feature_grad_mult, frames
padded to a multiple of 2 as fairseq does), ``O.head`` with the checkpoint's ``embedding_layer`` on each window's rows, the
float64 mean distance to 5 unit-norm references, a random float64 upstream per window, ``torch.autograd.grad`` - once in float64
and once in fp32.  feature_grad_mult is 0.1 everywhere and 1.0 on the win 20 hop 5 ragged geometry.  The head's ReLU kink is
taken out as the score tests do it, but per window: a column of ``embedding_layer.1.weight`` is zeroed when ANY window's mean of
that channel, over all geometries, lies within ``ref64.KINK`` of 0 in float64 (at most 64 of 768 columns, asserted; the CPU
oracle gives 6 for these clips and geometries).  The values of the differentiated forward are held to the same bound with e32
at least half an fp32 ulp of the largest score.

Bits: without a gradient ``score_windows`` is ``score_over_time``; with every clip inside one window and a gradient required its
values are ``score``'s; two identical calls give the same gradient; a clip's row of the ragged call's gradient is that of its own
B = 1 call; 260 clips in one batch - more than the scatter has threads to count the earlier clips' windows with - give the rows and
the gradient of the same clips as two batches of 130; ``references.grad`` is ``cdist_backward``'s.  Buffers: ``nomad_embed_windows_backward`` through ctypes with scratch,
workspace and output filled with NaN, then with 0 - finite and identical.  Refusals: status, ``nomad_last_error`` naming the
entry point, a poisoned output left untouched.

Worst err_gpu / e32 measured on one MI355X (``ref64.check`` prints it per case; gradient = d <up, scores> / d waveform over the
case's clips, value = the window scores of the differentiated forward, e32 at least half an fp32 ulp):

  geometry                     fgm   fp32 gradient  fp32 value   bf16x3 gradient  bf16x3 value
  T65 win64 hop1               0.1   1.88           0.59         13.68            0.64
  T130 win65 hop65             0.1   1.73           0.11         12.03            1.96
  T65 win3 hop2                0.1   2.07           1.11         13.38            5.21
  T65 win4 hop9                0.1   1.40           1.27         13.46            2.56
  T1+65+130 win4 hop9          0.1   2.46           2.18         14.49            6.96
  T1+65+130 win65 hop65        0.1   1.86           2.16         11.09            4.40
  T1+65+130 win20 hop5         0.1   2.10           1.95         12.15            3.97
  T1+65+130 win20 hop5         1.0   2.44           1.95         14.63            3.97
  constant in front of e32           ref64.C = 8                 C_X3P = 80

No case uses more than 0.31 of its bound.  ``score``'s own gradient sits at 1.8 - 2.7 and 12 - 16 (tests/test_gpu_score_loss.py):
the windowed head's backward adds nothing that shows next to the backbone's.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import guard
import ref64
from nomad_amd import _lib
from nomad_amd.weights import num_frames, num_windows
from oracle import nomad_oracle as O

pytestmark = pytest.mark.gpu

NR = 5
T_CLIPS = (1, 65, 130)
# (clips of T_CLIPS by index, win, hop)
GEOMETRIES = [((1,), 64, 1), ((2,), 65, 65), ((1,), 3, 2), ((1,), 4, 9), ((0, 1, 2), 4, 9), ((0, 1, 2), 65, 65), ((0, 1, 2), 20, 5)]
FGM1 = GEOMETRIES[-1]      # the geometry that also runs with feature_grad_mult = 1.0


def _gid(g):
    return "T" + "+".join(str(T_CLIPS[i]) for i in g[0]) + f"-win{g[1]}-hop{g[2]}"


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


def _seconds(win, hop):
    from nomad_amd.nomad import window_frames
    window_s, hop_s = win / 50, hop / 50
    assert window_frames(window_s, hop_s) == (win, hop)
    return window_s, hop_s


def _window_means(x, win, hop):
    """x (T,768) -> (W,768): the time mean of every window's rows."""
    T = x.shape[0]
    n = min(win, T)
    return torch.stack([x[k * hop:k * hop + n].mean(0) for k in range(num_windows(T, win, hop))])


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
    for idx, win, hop in GEOMETRIES:
        for i in idx:
            undecided |= (_window_means(x64[i], win, hop).abs() < ref64.KINK).any(0)
    assert int(undecided.sum()) <= 64, int(undecided.sum())
    print(f"WINDOWS LOSS {int(undecided.sum())} head columns zeroed")
    sd = {k: v.clone() for k, v in sd0.items()}
    sd["embedding_layer.1.weight"][:, undecided] = 0.0
    up = {g: torch.randn(sum(num_windows(T_CLIPS[i], g[1], g[2]) for i in g[0]), generator=gen, dtype=torch.float64) for g in GEOMETRIES}
    yield {"sd": sd, "refs": refs, "clips": clips, "up": up}
    for cache in (_backbone_cache, _oracle_cache, _sd_cache):     # the graphs and the float64 copy of the weights go with the module
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


# ---- the oracle: computed once per (clip, feature_grad_mult, dtype) and per (geometry, feature_grad_mult), never changed ----------
_backbone_cache, _oracle_cache, _sd_cache = {}, {}, {}


def _backbone(data, i, mult, dt):
    """Clip i through ``O.backbone`` at its exact length, in ``dt``, with the graph kept -> (leaf (1,N), x (T,768))."""
    key = (i, mult, dt)
    if key not in _backbone_cache:
        w = data["clips"][i][None].to(dt).requires_grad_(True)
        if dt not in _sd_cache:
            _sd_cache[dt] = ref64.cast(data["sd"], dt)
        x, _ = O.backbone(_sd_cache[dt], w, feature_grad_mult=mult, required_seq_len_multiple=2)
        _backbone_cache[key] = (w, x[0])
    return _backbone_cache[key]


def _oracle(data, geometry, mult):
    """-> {dtype: (window scores (W_total,) float64, [d <up, scores> / d clip])}: the clips' windows in the engine's order."""
    key = (geometry, mult)
    if key not in _oracle_cache:
        idx, win, hop = geometry
        out = {}
        for dt in (torch.float64, torch.float32):
            hw, hb = data["sd"]["embedding_layer.1.weight"].to(dt), data["sd"]["embedding_layer.1.bias"].to(dt)
            scores, grads, at = [], [], 0
            for i in idx:
                w, x = _backbone(data, i, mult, dt)
                T = x.shape[0]
                n = min(win, T)
                e = torch.cat([O.head(x[None, k * hop:k * hop + n], hw, hb) for k in range(num_windows(T, win, hop))])
                s = (e.double()[:, None, :] - data["refs"].double()[None]).norm(dim=-1).mean(1)   # the distance in float64, as the engine takes it
                (g,) = torch.autograd.grad((s * data["up"][geometry][at:at + s.numel()]).sum(), w, retain_graph=True)
                at += s.numel()
                scores.append(s.detach())
                grads.append(g[0])
            out[dt] = (torch.cat(scores), grads)
        _oracle_cache[key] = out
    return _oracle_cache[key]


def _backward(nmd, data, geometry, mult=0.1, clips=None, up=None):
    """``score_windows`` with a gradient on the geometry's clips (one clip: the uniform call; several: ``lengths``) and its
    backward with the geometry's upstream -> (scores, counts, gradient (B,1,N), lengths)."""
    idx, win, hop = geometry
    clips = [data["clips"][i] for i in idx] if clips is None else clips
    up = data["up"][geometry] if up is None else up
    lens = [k.numel() for k in clips]
    eng = nmd.engine
    prev = eng.feature_grad_mult
    eng.feature_grad_mult = mult
    try:
        x = _padded(clips).cuda().requires_grad_(True)
        s, counts = nmd.score_windows(x, data["refs"].cuda(), *_seconds(win, hop), lengths=lens if len(clips) > 1 else None)
        s.backward(up.cuda())
    finally:
        eng.feature_grad_mult = prev
    return s.detach(), counts, x.grad, lens


def _gradient_case(nmd, data, geometry, mult, c):
    idx, win, hop = geometry
    case = f"score_windows {nmd.precision} {_gid(geometry)} fgm={mult:g}"
    ref = _oracle(data, geometry, mult)
    (s64, g64), (s32, g32) = ref[torch.float64], ref[torch.float32]
    with guard.guarded(case=case):
        s, counts, grad, lens = _backward(nmd, data, geometry, mult)
        torch.cuda.synchronize()
    assert counts == [num_windows(T_CLIPS[i], win, hop) for i in idx]
    assert s.shape == (sum(counts),) and s.dtype == torch.float64
    assert grad.shape == (len(idx), 1, max(lens)) and bool(torch.isfinite(grad).all())
    for i, n in enumerate(lens):
        assert not grad[i, 0, n:].any(), f"clip {i}: a gradient behind its length"
    ref64.check(case + " gradient", {f"d{i}": grad[i, 0, :n].cpu() for i, n in enumerate(lens)},
                {f"d{i}": g for i, g in enumerate(g64)}, {f"d{i}": g for i, g in enumerate(g32)}, c=c)
    half_ulp = float(np.spacing(np.float32(s64.abs().max().item()))) / 2
    ref64.check(case + " value", s.cpu(), s64, s32, e32_min={"": half_ulp}, c=c)


CASES = [(g, 0.1) for g in GEOMETRIES] + [(FGM1, 1.0)]


@pytest.mark.parametrize("geometry, mult", CASES, ids=[f"{_gid(g)}-fgm{m:g}" for g, m in CASES])
def test_gradient_vs_float64(nmd_f32, data, geometry, mult):
    _gradient_case(nmd_f32, data, geometry, mult, ref64.C)


@pytest.mark.parametrize("geometry, mult", CASES, ids=[f"{_gid(g)}-fgm{m:g}" for g, m in CASES])
def test_gradient_bf16x3_vs_float64(nmd_x3, data, geometry, mult):
    from test_gpu_forward_f64 import C_X3P
    assert nmd_x3.engine.gemm_precision == "bf16x3"
    _gradient_case(nmd_x3, data, geometry, mult, C_X3P)


# ---- bits ------------------------------------------------------------------------------------------------------------------
def test_without_a_gradient_it_is_score_over_time(nmd_f32, data):
    nmd, refs = nmd_f32, data["refs"].cuda()
    clips = data["clips"]
    uni = torch.stack([_wav(ref64.n_for(65), 120 + i) for i in range(3)]).cuda()        # (B,N)
    rag, lens = _padded(clips).cuda(), [c.numel() for c in clips]                       # (B,1,N) with lengths
    with guard.guarded(case="score_windows without a gradient"):
        for x, ln in ((uni, None), (uni[:, None, :], None), (rag, lens), (rag[:, 0].contiguous(), lens)):
            want, wcounts = nmd.score_over_time(x, refs, 0.4, 0.1, lengths=ln)             # win 20, hop 5
            got, counts = nmd.score_windows(x, refs, 0.4, 0.1, lengths=ln)              # grad mode on, nothing requires a gradient
            with torch.no_grad():
                req, _ = nmd.score_windows(x.clone().requires_grad_(True), refs.clone().requires_grad_(True), 0.4, 0.1, lengths=ln)
                mean, mcounts = nmd.score_windows(x, refs, 0.4, 0.1, lengths=ln, reduction="mean")
            assert counts == wcounts == mcounts and got.dtype == torch.float64 and got.shape == (sum(counts),)
            assert torch.equal(got, want) and torch.equal(req, want) and not got.requires_grad and not req.requires_grad
            assert mean.dim() == 0 and torch.equal(mean, want.mean())
        torch.cuda.synchronize()


def test_one_window_per_clip_has_the_values_of_score(nmd_f32, data):
    nmd, refs = nmd_f32, data["refs"].cuda()
    uni = torch.stack([_wav(ref64.n_for(65), 120 + i) for i in range(3)]).cuda()
    rag, lens = _padded(data["clips"]).cuda(), [c.numel() for c in data["clips"]]
    with guard.guarded(case="score_windows, one window per clip"):
        for x, ln in ((uni, None), (rag, lens)):
            xs = x.clone().requires_grad_(True)
            got, counts = nmd.score_windows(xs, refs, window_s=4.0, hop_s=2.0, lengths=ln)
            want = nmd.score(x.clone().requires_grad_(True), refs, lengths=ln)
            assert counts == [1, 1, 1] and got.requires_grad and want.requires_grad
            assert torch.equal(got.detach(), want.detach())
            mean, _ = nmd.score_windows(xs, refs, window_s=4.0, hop_s=2.0, lengths=ln, reduction="mean")
            assert mean.dim() == 0 and torch.equal(mean.detach(), want.detach().mean())
        torch.cuda.synchronize()


@pytest.mark.parametrize("geometry", [GEOMETRIES[4], GEOMETRIES[6]], ids=_gid)
def test_repeatable_and_a_clips_gradient_does_not_depend_on_its_batch(nmd_f32, data, geometry):
    idx, win, hop = geometry
    with guard.guarded(case=f"score_windows batch invariance {_gid(geometry)}"):
        s, counts, grad, lens = _backward(nmd_f32, data, geometry)
        s2, _, grad2, _ = _backward(nmd_f32, data, geometry)
        own, at = [], 0
        for b, i in enumerate(idx):     # the clip on its own, at B = 1 with its length (the ragged path), with its rows of the upstream
            clip = data["clips"][i]
            x = clip[None, None].cuda().requires_grad_(True)
            so, co = nmd_f32.score_windows(x, data["refs"].cuda(), *_seconds(win, hop), lengths=[clip.numel()])
            so.backward(data["up"][geometry][at:at + counts[b]].cuda())
            own.append((so.detach(), co, x.grad))
            at += counts[b]
        torch.cuda.synchronize()
    assert torch.equal(s, s2) and torch.equal(grad, grad2), "two identical calls differ"
    assert grad.abs().max() > 0
    at = 0
    for b, (so, co, g) in enumerate(own):
        assert co == [counts[b]] and torch.equal(so, s[at:at + counts[b]]), f"clip {b}: the scores differ from its own call"
        assert torch.equal(g[0, 0], grad[b, 0, :lens[b]]), f"clip {b}: the gradient differs from its own B = 1 call"
        at += counts[b]


def test_references_get_the_gradient_of_cdist_backward(nmd_f32, data):
    nmd, eng = nmd_f32, nmd_f32.engine
    geometry = GEOMETRIES[3]                                       # T = 65, win 4, hop 9
    refs, up = data["refs"].cuda(), data["up"][geometry].cuda()
    x = data["clips"][1][None].cuda()
    with guard.guarded(case="score_windows d / d references"):
        r = refs.clone().requires_grad_(True)
        s, counts = nmd.score_windows(x, r, *_seconds(4, 9))        # only the references: the scoring forward's windows
        s.backward(up)
        emb_w, _ = eng.embed_windows(x, 4, 9)
        want = eng.cdist_backward(emb_w, refs, g_mean=up, want_a=False, want_b=True)[1]
        # both differentiated: the windows are embed_train_windows', the references' gradient is still cdist_backward's
        xg, r2 = x.clone().requires_grad_(True), refs.clone().requires_grad_(True)
        nmd.score_windows(xg, r2, *_seconds(4, 9))[0].backward(up)
        emb_t = eng.embed_train_windows(x, 4, 9)[0]
        want_t = eng.cdist_backward(emb_t, refs, g_mean=up, want_a=False, want_b=True)[1]
        # a float64 bank on the host gets its gradient where and as it lives
        r3 = data["refs"].double().requires_grad_(True)
        nmd.score_windows(x, r3, *_seconds(4, 9))[0].backward(up)
        torch.cuda.synchronize()
    assert counts == [7] and r.grad.dtype == torch.float32 and torch.equal(r.grad, want)
    assert torch.equal(r2.grad, want_t) and xg.grad is not None and xg.grad.abs().max() > 0
    assert r3.grad.dtype == torch.float64 and r3.grad.device.type == "cpu" and torch.equal(r3.grad, want.cpu().double())


def test_more_clips_than_the_scatter_has_threads(nmd_f32):
    """B = 260 clips of 1, 2, 3 frames (cycled), win 2 hop 1 - 1, 1, 2 windows: a clip's first output row is the sum of the earlier
    clips' window counts, which every workgroup forms for itself with a stride of its own size (1024 threads in the two head
    kernels, 256 in the scatter).  260 clips make the scatter's count loop take a second trip.  Rows and gradient of the one batch
    against clips 0..129 and 130..259 run as two batches, bit for bit: the batch-invariance contract."""
    eng = nmd_f32.engine
    lens = [(400, 720, 1040)[i % 3] for i in range(260)]
    assert [num_frames(n) for n in lens[:3]] == [1, 2, 3]
    clips = [_wav(n, 300 + i).cuda() for i, n in enumerate(lens)]
    counts = [num_windows(num_frames(n), 2, 1) for n in lens]
    demb_w = torch.randn(sum(counts), 256, generator=torch.Generator().manual_seed(260)).cuda()

    def run(lo, hi):
        emb, cnt, layers, saved, batch = eng.embed_train_windows_ragged(clips[lo:hi], 2, 1)
        assert cnt == counts[lo:hi]
        at = sum(counts[:lo])
        return emb, eng.embed_windows_backward_ragged(batch, layers, saved, demb_w[at:at + sum(cnt)], 2, 1)

    with guard.guarded(case="windows of 260 clips"):
        emb, dwav = run(0, 260)
        (emb_a, dwav_a), (emb_b, dwav_b) = run(0, 130), run(130, 260)
        torch.cuda.synchronize()
    assert emb.shape == (sum(counts), 256) and bool(torch.isfinite(emb).all()) and dwav.abs().max() > 0
    assert torch.equal(emb, torch.cat([emb_a, emb_b])), "a window's row depends on the clips ahead of it"
    assert torch.equal(dwav, torch.cat([dwav_a, dwav_b])), "a clip's gradient depends on the clips ahead of it"


# ---- buffers and refusals at the C ABI ------------------------------------------------------------------------------------------
class _Call:
    """``nomad_embed_windows_backward`` for one (2, n) batch of T = 65 clips, win 4 hop 9, with every buffer the test's own."""

    def __init__(self, eng, seed=140):
        self.eng, self.lib = eng, eng.lib
        self.n = ref64.n_for(65)
        self.wav = _wav(2 * self.n, seed).reshape(2, self.n).cuda()
        self.emb, counts, self.layers, self.saved = eng.embed_train_windows(self.wav, 4, 9)
        self.W = sum(counts)
        g = torch.Generator().manual_seed(seed)
        self.demb = torch.randn(self.W, 256, generator=g).cuda()
        nb, ns = C.c_size_t(), C.c_size_t()
        assert self.lib.nomad_backward_workspace_bytes(eng.ctx, 2, self.n, C.byref(nb)) == 0
        assert self.lib.nomad_windows_backward_scratch_bytes(self.W, C.byref(ns)) == 0
        self.ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
        self.scratch = torch.empty(ns.value, dtype=torch.uint8, device="cuda")
        self.dwav = torch.empty(2, self.n, device="cuda")

    def fill(self, value):
        for t in (self.ws.view(torch.float32), self.scratch.view(torch.float32), self.dwav):
            t.fill_(value)

    def __call__(self, **kw):
        a = dict(ctx=self.eng.ctx, wav=self.wav.data_ptr(), B=2, n=self.n, win=4, hop=9, hw=None, hb=None, layers=self.layers.data_ptr(),
                 saved=self.saved.data_ptr(), saved_bytes=self.saved.numel(), demb=self.demb.data_ptr(), dwav=self.dwav.data_ptr(),
                 scratch=self.scratch.data_ptr(), scratch_bytes=self.scratch.numel(), ws=self.ws.data_ptr(), ws_bytes=self.ws.numel())
        a.update(kw)
        return self.lib.nomad_embed_windows_backward(a["ctx"], a["wav"], a["B"], a["n"], a["win"], a["hop"], a["hw"], a["hb"], a["layers"],
                                                     a["saved"], a["saved_bytes"], a["demb"], a["dwav"], a["scratch"], a["scratch_bytes"],
                                                     a["ws"], a["ws_bytes"], None)

    def ragged(self, **kw):
        a = dict(lens=(self.n, self.n), win=4, hop=9, hw=None, hb=None, demb=self.demb.data_ptr(), dwav=self.dwav.data_ptr(),
                 scratch=self.scratch.data_ptr(), scratch_bytes=self.scratch.numel(), ws_bytes=self.ws.numel(), saved_bytes=self.saved.numel())
        a.update(kw)
        lens = (C.c_int * 2)(*a["lens"]) if a["lens"] is not None else None
        return self.lib.nomad_embed_windows_backward_ragged(self.eng.ctx, self.wav.data_ptr(), 2, self.n, lens, a["win"], a["hop"], a["hw"],
                                                            a["hb"], self.layers.data_ptr(), self.saved.data_ptr(), a["saved_bytes"],
                                                            a["demb"], a["dwav"], a["scratch"], a["scratch_bytes"], self.ws.data_ptr(),
                                                            a["ws_bytes"], None)


def test_nothing_relies_on_cleared_buffers(nmd_f32):
    """T = 65, win 4, hop 9: frames 4 .. 8 of every hop lie between windows and frames 58 .. 64 behind the last one - their rows of
    the frame gradient exist only because the scatter writes zeros there."""
    with guard.guarded(case="windows backward, poisoned buffers: the forward"):
        call = _Call(nmd_f32.engine)
        torch.cuda.synchronize()
    out = []
    for value in (float("nan"), 0.0):
        call.fill(value)
        assert call() == 0, call.lib.nomad_last_error()
        torch.cuda.synchronize()
        out.append(call.dwav.clone())
    assert bool(torch.isfinite(out[0]).all()) and out[0].abs().max() > 0
    assert torch.equal(out[0], out[1])
    with guard.guarded(case="windows backward, poisoned buffers: the engine's call"):
        own = nmd_f32.engine.embed_windows_backward(call.wav, call.layers, call.saved, call.demb, 4, 9)
        torch.cuda.synchronize()
    assert torch.equal(out[0], own)


def test_refusals_at_the_abi(nmd_f32, sd0):
    from nomad_amd.engine import Engine
    eng, lib = nmd_f32.engine, nmd_f32.engine.lib
    with guard.guarded(case="windows backward refusals: the forward"):
        call = _Call(eng, seed=141)
        torch.cuda.synchronize()
    call.fill(0.0)
    assert call() == 0
    torch.cuda.synchronize()
    good = call.dwav.clone()
    call.dwav.fill_(7.0)
    hw, hb = torch.zeros(256, 768, device="cuda"), torch.zeros(256, device="cuda")
    who = b"nomad_embed_windows_backward"
    for kw in (dict(win=0), dict(hop=0), dict(win=-1), dict(hop=-3), dict(hw=hw.data_ptr()), dict(hb=hb.data_ptr()), dict(ctx=None),
               dict(wav=None), dict(layers=None), dict(saved=None), dict(demb=None), dict(dwav=None), dict(scratch=None), dict(ws=None),
               dict(B=0), dict(n=399)):
        assert call(**kw) == _lib.NOMAD_ERR_INVALID, kw
        assert lib.nomad_last_error().startswith(who + b":"), (kw, lib.nomad_last_error())
    for kw in (dict(scratch_bytes=call.scratch.numel() - 1), dict(ws_bytes=call.ws.numel() - 1), dict(saved_bytes=call.saved.numel() - 1)):
        assert call(**kw) == _lib.NOMAD_ERR_WORKSPACE, kw
        assert lib.nomad_last_error().startswith(who + b":"), (kw, lib.nomad_last_error())
    who = b"nomad_embed_windows_backward_ragged"
    for kw in (dict(win=0), dict(hop=0), dict(hw=hw.data_ptr()), dict(hb=hb.data_ptr()), dict(demb=None), dict(dwav=None),
               dict(scratch=None), dict(lens=None), dict(lens=(call.n, 399)), dict(lens=(call.n, call.n + 1))):
        assert call.ragged(**kw) == _lib.NOMAD_ERR_INVALID, kw
        assert lib.nomad_last_error().startswith(who + b":"), (kw, lib.nomad_last_error())
    assert call.ragged(scratch_bytes=call.scratch.numel() - 1) == _lib.NOMAD_ERR_WORKSPACE and lib.nomad_last_error().startswith(who + b":")
    assert call.ragged(saved_bytes=1) == _lib.NOMAD_ERR_WORKSPACE and lib.nomad_last_error().startswith(who + b":")
    assert call.ragged(ws_bytes=1) == _lib.NOMAD_ERR_WORKSPACE and lib.nomad_last_error().startswith(who + b":")
    # the training-mode forwards: the same refusals, and their outputs untouched
    emb = torch.full((call.W, 256), 7.0, device="cuda")
    fws = torch.empty(eng.workspace_bytes(2, call.n), dtype=torch.uint8, device="cuda")

    def train(win=4, hop=9, hw=None, hb=None, emb_p=emb.data_ptr(), layers=call.layers.data_ptr(), saved=call.saved.data_ptr(),
              saved_bytes=call.saved.numel(), ws_bytes=fws.numel()):
        return lib.nomad_embed_train_windows(eng.ctx, call.wav.data_ptr(), 2, call.n, win, hop, hw, hb, emb_p, layers, saved, saved_bytes,
                                             fws.data_ptr(), ws_bytes, None)

    def train_ragged(win=4, hop=9, hw=None, saved=call.saved.data_ptr(), lens=(call.n, call.n), saved_bytes=call.saved.numel()):
        return lib.nomad_embed_train_windows_ragged(eng.ctx, call.wav.data_ptr(), 2, call.n, (C.c_int * 2)(*lens), win, hop, hw, None,
                                                    emb.data_ptr(), call.layers.data_ptr(), saved, saved_bytes, fws.data_ptr(),
                                                    fws.numel(), None)
    for fn, who, kws in ((train, b"nomad_embed_train_windows", (dict(win=0), dict(hop=0), dict(hw=hw.data_ptr()), dict(hb=hb.data_ptr()),
                                                                dict(emb_p=None), dict(layers=None), dict(saved=None))),
                         (train_ragged, b"nomad_embed_train_windows_ragged", (dict(win=0), dict(hop=-1), dict(hw=hw.data_ptr()),
                                                                              dict(saved=None), dict(lens=(call.n, 399))))):
        for kw in kws:
            assert fn(**kw) == _lib.NOMAD_ERR_INVALID, (who, kw)
            assert lib.nomad_last_error().startswith(who + b":"), (kw, lib.nomad_last_error())
    assert train(saved_bytes=call.saved.numel() - 1) == _lib.NOMAD_ERR_WORKSPACE and b"nomad_embed_train_windows:" in lib.nomad_last_error()
    assert train(ws_bytes=fws.numel() - 1) == _lib.NOMAD_ERR_WORKSPACE and b"nomad_embed_train_windows:" in lib.nomad_last_error()
    assert train_ragged(saved_bytes=1) == _lib.NOMAD_ERR_WORKSPACE and b"nomad_embed_train_windows_ragged:" in lib.nomad_last_error()
    # a cut encoder: at the ABI, in the engine and in score_windows, with and without a gradient
    refs = torch.nn.functional.normalize(torch.ones(2, 256), dim=1).cuda()
    eng.encoder_depth = 5
    try:
        for fn in (call, call.ragged, train, train_ragged):
            assert fn() == _lib.NOMAD_ERR_INVALID and b"depth is 5" in lib.nomad_last_error()
        with pytest.raises(_lib.NomadHipError, match="depth is 5"):
            eng.embed_train_windows(call.wav, 4, 9)
        for x in (call.wav, call.wav.clone().requires_grad_(True)):
            with pytest.raises(RuntimeError, match="whole encoder"):
                nmd_f32.score_windows(x, refs, 0.08, 0.18)
    finally:
        eng.encoder_depth = 12
    # fine-tuning mode: its training-mode forward draws masks this backward does not replay
    tuned = Engine(sd0, 0)
    try:
        tuned.enable_backward()
        tuned.train_enable()
        assert call(ctx=tuned.ctx) == _lib.NOMAD_ERR_INVALID
        assert lib.nomad_last_error().startswith(b"nomad_embed_windows_backward:") and b"fine-tuning" in lib.nomad_last_error()
        assert lib.nomad_embed_train_windows(tuned.ctx, call.wav.data_ptr(), 2, call.n, 4, 9, None, None, emb.data_ptr(),
                                             call.layers.data_ptr(), call.saved.data_ptr(), call.saved.numel(), fws.data_ptr(),
                                             fws.numel(), None) == _lib.NOMAD_ERR_INVALID
        assert lib.nomad_last_error().startswith(b"nomad_embed_train_windows:") and b"fine-tuning" in lib.nomad_last_error()
    finally:
        tuned.close()
    torch.cuda.synchronize()
    assert bool((call.dwav == 7.0).all()) and bool((emb == 7.0).all())            # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(call.dwav, good)
