"""GPU: every entry point reads only what it wrote.

The kernels write exactly the elements they own and zero only the pads something later reads (the conv backward's pad rows, the
pos-conv buffers' padding frames, the dW operands' tails, split-K partial slices ...).  A fresh allocation is usually zero, which
is what a forgotten pad needs, and the rest of the suite runs on such buffers or on the previous call's data of the same shape.
Here each case runs once on a fresh engine (the reference), then again after everything it reads from or writes to has been
filled with 0xFF bytes - a NaN in fp32, bf16 and fp64, which survives multiplication by zero and masking by multiply:

  * the engine's cached workspaces (``_ws``, every ``_ws_side[k]``) and the l1 scratch,
  * the context's own scratch (``nomad_diag_poison_scratch``: split-K partials, pairwise blocks, weight-norm temporaries),
  * the gradient vector, before ``train_zero_grad`` (``train_write(1, NaN)``),
  * every tensor an Engine method allocates during the call - outputs (emb, layers, saved, dwav, the distance matrix and
    means, ...), staging buffers and new workspaces: ``torch`` inside ``nomad_amd.engine`` is replaced by a stand-in whose
    ``empty`` / ``empty_like`` fill on the current stream, so the outputs are poisoned on the very code path users take
    (two-stream splits and side workspaces included).

The poisoned run must be bit-identical to the reference and finite.  The last test runs the production pattern without poison:
one engine serving calls of different shapes must give what a fresh engine gives.
"""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = 0xFF
N_T1 = 400       # the smallest clip with T = 1 (conv lengths 79/39/19/9/4/2/1)
N_T64 = 20560    # T = 64: 4111/2055/1027/513/256/128/64
N_T65 = 20887    # T = 65: 4176/2087/1043/521/260/130/65
N_T199 = 64000   # T = 199
# (B, n): conv lengths 1799/899/449/224/111/55/27 at n = 9001 (odd at most layers), T = 50 at 16384 (the loss path)
SHAPES = [(1, 9001), (3, 9001), (2, 16384), (1, N_T199), (2, N_T64), (1, N_T65), (3, N_T1)]
RAGGED_N = [N_T1, 720, N_T64, N_T65, N_T199]   # one clip each of T = 1, 2, 64, 65, 199


def _fill(t):
    if t is not None and t.numel():
        t.reshape(-1).view(torch.uint8).fill_(POISON)
    return t


class _PoisonTorch:
    """``torch`` as nomad_amd.engine sees it during a poisoned run: every tensor it allocates starts as 0xFF bytes."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*args, **kw):
        return _fill(torch.empty(*args, **kw))

    @staticmethod
    def empty_like(*args, **kw):
        return _fill(torch.empty_like(*args, **kw))


@contextlib.contextmanager
def _poisoned(*engines):
    """Poison every engine's workspaces and context scratch (synchronised before the call), then run the body with every
    Engine-allocated tensor poisoned too."""
    from nomad_amd import engine as engine_mod
    for eng in engines:
        for ws in [eng._ws, eng._l1_scratch, *eng._ws_side.values()]:
            _fill(ws)
        eng.diag_poison_scratch(POISON)
        if eng._train_segments is not None:
            total, _ = eng.train_param_count()
            eng.train_write(1, torch.full((total,), float("nan"), device=eng.device))
    torch.cuda.synchronize()
    real = engine_mod.torch
    engine_mod.torch = _PoisonTorch()
    try:
        yield
    finally:
        engine_mod.torch = real


def _host(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().clone()
    if isinstance(x, (tuple, list)):
        return [_host(v) for v in x]
    if isinstance(x, dict):
        return {k: _host(v) for k, v in x.items()}
    return x


def _flat(x, prefix="out"):
    if x is None:
        return []
    if isinstance(x, torch.Tensor):
        return [(prefix, x.reshape(-1))]
    if isinstance(x, dict):
        return [p for k, v in x.items() for p in _flat(v, f"{prefix}.{k}")]
    return [p for i, v in enumerate(x) for p in _flat(v, f"{prefix}[{i}]")]


def _assert_same_bits(ref, got):
    for (name, r), (_, g) in zip(_flat(ref), _flat(got)):
        assert r.shape == g.shape, name
        bad = ~torch.isfinite(g) if g.is_floating_point() else torch.zeros_like(g, dtype=torch.bool)
        assert not bad.any(), f"{name}: {int(bad.sum())} non-finite of {g.numel()}, first at {np.argwhere(bad.numpy())[0].tolist()}"
        same = np.array_equal(r.numpy().view(np.uint8), g.numpy().view(np.uint8))
        if not same:
            diff = (r.double() - g.double()).abs()
            pytest.fail(f"{name}: {int((diff > 0).sum())} of {g.numel()} elements differ, max |diff| {diff.max().item():.3e}, "
                        f"first at {np.argwhere((diff > 0).numpy())[0].tolist()}")


def _screen(eng, call):
    """call() on the fresh engine, then on the poisoned one: bit-identical and finite."""
    ref = _host(call())
    torch.cuda.synchronize()
    with _poisoned(eng):
        got = _host(call())
    _assert_same_bits(ref, got)
    return ref


@pytest.fixture
def fresh(built_lib, sd0):
    """Fresh engines on libnomad_diag.so (the poison hook), closed at the end of the test."""
    from nomad_amd.engine import Engine
    made = []

    def make(train=False):
        eng = Engine(sd0, 0, diag=True)
        if train:
            eng.train_enable()
        made.append(eng)
        return eng

    yield make
    torch.cuda.synchronize()
    for eng in made:
        eng.close()


def _wav(B, n, seed=0):
    g = torch.Generator().manual_seed(seed * 1000003 + B * 7919 + n)
    return (0.1 * torch.randn(B, n, generator=g)).clamp(-1, 1).cuda()


def _head(seed=5):
    g = torch.Generator().manual_seed(seed)
    return ((0.02 * torch.randn(256, 768, generator=g)).cuda(), (0.01 * torch.randn(256, generator=g)).cuda())


# ---- forwards -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [False, True], ids=["emb", "layers"])
@pytest.mark.parametrize("B,n", SHAPES)
def test_embed_fp32(fresh, B, n, layers):
    """Layer-output forwards of fewer than 4096 frames take the split-K GEMMs (Layout::splitk)."""
    eng = fresh()
    w, head = _wav(B, n), _head()
    _screen(eng, lambda: eng.embed(w, head=head if layers else None, want_layers=layers))


@pytest.mark.parametrize("B,n", SHAPES)
def test_embed_bf16(fresh, B, n):
    eng = fresh()
    w = _wav(B, n)
    _screen(eng, lambda: eng.embed_bf16(w))


@pytest.mark.parametrize("layers", [False, True], ids=["emb", "layers"])
@pytest.mark.parametrize("B,n", SHAPES)
def test_embed_bf16x3(fresh, B, n, layers):
    eng = fresh()
    w = _wav(B, n)
    _screen(eng, lambda: eng.embed_bf16x3(w, head=_head() if layers else None, want_layers=layers))


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_embed_ragged(fresh, precision):
    """Every ragged entry point copies its metadata into the workspace (hipMemcpyAsync) before any kernel reads it, so the
    poisoned metadata region is overwritten before use."""
    eng = fresh()
    waves = [_wav(1, n, seed=i)[0] for i, n in enumerate(RAGGED_N[::-1] + RAGGED_N[:2])]
    _screen(eng, lambda: eng.embed_ragged(waves, precision=precision))


@pytest.mark.parametrize("layers", [False, True], ids=["emb", "layers"])
def test_embed_fp32_buffers_bf16x3_products(fresh, layers):
    eng = fresh()
    eng.gemm_precision = "bf16x3"
    w = _wav(3, 9001)
    _screen(eng, lambda: eng.embed(w, head=_head() if layers else None, want_layers=layers))


@pytest.mark.parametrize("path", ["fp32", "bf16", "bf16x3", "ragged"])
def test_two_stream_split(fresh, path):
    """21 clips of T = 199 (4179 frames): the batch is split over the main and a side stream, each with its own workspace
    (the halves are 10 and 11 clips, so the two workspaces differ in size)."""
    from nomad_amd.engine import Engine
    from nomad_amd.weights import num_frames
    eng = fresh()
    w = _wav(21, N_T199)
    assert 21 * num_frames(N_T199) >= max(Engine.F32_SPLIT_ROWS, Engine.BF16_SPLIT_ROWS, Engine.X3_SPLIT_ROWS)
    if path == "ragged":
        waves = [w[i, :N_T199 - 97 * i] for i in range(21)]
        call = lambda: eng.embed_ragged(waves)   # noqa: E731
    else:
        call = {"fp32": lambda: eng.embed(w), "bf16": lambda: eng.embed_bf16(w), "bf16x3": lambda: eng.embed_bf16x3(w)}[path]
    _screen(eng, call)
    assert eng._ws_side, "the batch was expected to use a side workspace"


# ---- Nomad.forward (the loss) and its backward ------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n", [(2, 16384), (1, 9001)])
def test_loss_forward_backward(built_lib, sd0, monkeypatch, B, n):
    """The loss path: clean branch (layer-output forward on the side stream), embed_train, l1 loss, its backward and
    embed_backward, whose input is the saved block embed_train wrote."""
    from nomad_amd.nomad import Nomad
    monkeypatch.setenv("NOMAD_DIAG_LIB", "1")   # the poison hook is in libnomad_diag.so
    nmd = Nomad(weights=sd0)
    eng = nmd.engine
    try:
        assert eng.lib.nomad_build_flags() & 2, "expected the diagnostics library"
        est0, cln = _wav(B, n, seed=1), _wav(B, n, seed=2)

        def call():
            est = est0.clone().requires_grad_(True)
            loss = nmd.forward(est, cln)
            loss.backward()
            return [loss, est.grad]

        _screen(eng, call)
    finally:
        torch.cuda.synchronize()
        eng.close()


# ---- training step ----------------------------------------------------------------------------------------------------------
def _train_step(eng, clips, masks=None):
    """train_zero_grad -> embed_train per branch -> triplet loss -> train_backward -> (loss, embeddings, gradient)."""
    eng.train_zero_grad()
    if masks is None:
        outs = [eng.embed_train(w) for w in clips]
        loss, da, dp, dn = eng.triplet_loss(outs[0][0], outs[1][0], outs[2][0], 0.5)
        for w, (_, layers, saved), d in zip(clips, outs, (da, dp, dn)):
            eng.train_backward(w, layers, saved, d)
        embs = [o[0] for o in outs]
    else:
        B = clips[0].shape[0]
        w = torch.cat(clips)
        eng.train_set_branches(list(masks))
        try:
            emb, layers, saved = eng.embed_train(w)
            loss, da, dp, dn = eng.triplet_loss(emb[:B].contiguous(), emb[B:2 * B].contiguous(), emb[2 * B:].contiguous(), 0.5)
            eng.train_backward(w, layers, saved, torch.cat([da, dp, dn]))
        finally:
            eng.train_set_branches(None)
        embs = [emb]
    return [loss, embs, eng.train_read(1)]


TRAIN_CASES = {
    # three branches of different lengths, each its own embed_train / train_backward on the one training workspace
    "separate_frozen": dict(convnet=False, lens=(9001, 16384, 12000)),
    "separate_convnet": dict(convnet=True, lens=(9001, 16384, 12000)),
    # one merged batch of three branches, each with its own LayerDrop mask
    "merged_convnet": dict(convnet=True, lens=(9001,) * 3, masks=(0xFFF, 0xFFE, 0x7FF)),
    "merged_frozen": dict(convnet=False, lens=(16384,) * 3, masks=(0xFFF, 0xFFF, 0xFFF)),
    "dropout_convnet": dict(convnet=True, lens=(9001, 16384, 12000), dropout=True),
}


@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_train_step(fresh, case):
    cfg = TRAIN_CASES[case]
    eng = fresh(train=True)
    eng.train_set_convnet(cfg["convnet"])
    clips = [_wav(2, n, seed=10 + i) for i, n in enumerate(cfg["lens"])]

    def call():
        if cfg.get("dropout"):
            eng.train_set_stochastic(0.1, 0.1, 0.1, seed=(7 << 33) + 3)
        try:
            return _train_step(eng, clips, cfg.get("masks"))
        finally:
            eng.train_set_stochastic()

    ref = _screen(eng, call)
    if not cfg["convnet"]:   # the frozen extractor's slices: exactly zero (NaN before train_zero_grad in the poisoned run)
        got = eng.train_unflatten(eng.train_read(1))
        conv = [k for k in got if ".feature_extractor." in k]
        assert conv and all(float(got[k].abs().max()) == 0.0 for k in conv)
        assert all(float(v.abs().max()) == 0.0 for k, v in eng.train_unflatten(ref[2]).items() if k in conv)


# ---- scoring -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix", [True, False], ids=["matrix", "means"])
@pytest.mark.parametrize("Nd,Nr", [(33, 70), (1, 1000), (300, 129)])
def test_pairwise(fresh, Nd, Nr, matrix):
    eng = fresh()
    g = torch.Generator().manual_seed(Nd * 1000 + Nr)
    deg, ref = torch.randn(Nd, 256, generator=g).cuda(), torch.randn(Nr, 256, generator=g).cuda()
    _screen(eng, lambda: eng.pairwise(deg, ref, want_matrix=matrix))


@pytest.mark.parametrize("B,T", [(2, 50), (1, 27), (3, 1)])
def test_l1_loss(fresh, B, T):
    eng = fresh()
    g = torch.Generator().manual_seed(B * 100 + T)
    a, b = torch.randn(12, B, T, 768, generator=g).cuda(), torch.randn(12, B, T, 768, generator=g).cuda()
    ea, eb = torch.randn(B, 256, generator=g).cuda(), torch.randn(B, 256, generator=g).cuda()
    _screen(eng, lambda: eng.l1_loss(a, b, ea, eb))


# ---- the production pattern, without poison ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_one_engine_across_shapes(fresh, precision):
    """One engine (and its cached workspaces) serving calls of different shapes - predict over a directory, ragged batches of
    varying lengths, training steps of varying length - gives what a fresh engine gives for each call, bit for bit."""
    from nomad_amd.weights import num_frames
    long_ragged = [_wav(1, n, seed=30 + i)[0] for i, n in enumerate((N_T199, 48000, 31111, N_T65, 9001))]
    short_ragged = [_wav(1, n, seed=40 + i)[0] for i, n in enumerate((5000, 720, N_T1))]
    uniform = _wav(4, 16384, seed=50)
    embed = (lambda e, w: e.embed(w)) if precision == "fp32" else (lambda e, w: e.embed_bf16(w))
    calls = [lambda e: e.embed_ragged(long_ragged, precision=precision),
             lambda e: e.embed_ragged(short_ragged, precision=precision),
             lambda e: embed(e, uniform)]
    shared = fresh()
    for call in calls:
        got = _host(call(shared))
        _assert_same_bits(_host(call(fresh())), got)
    # training steps at n = 48000, then 5000 (on fp32 buffers; "bf16": their GEMM products as bf16x3)
    steps = [[_wav(1, n, seed=60 + i) for i in range(3)] for n in (48000, 5000)]
    assert num_frames(5000) < num_frames(48000)
    shared = fresh(train=True)
    shared.train_set_convnet(True)
    for clips in steps:
        if precision == "bf16":
            shared.gemm_precision = "bf16x3"
        got = _host(_train_step(shared, clips))
        ref_eng = fresh(train=True)
        ref_eng.train_set_convnet(True)
        if precision == "bf16":
            ref_eng.gemm_precision = "bf16x3"
        _assert_same_bits(_host(_train_step(ref_eng, clips)), got)
