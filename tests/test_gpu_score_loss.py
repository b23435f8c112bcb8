"""GPU: ``Nomad.score`` - the NOMAD score of ``predict`` (mean float64 distance to a bank of reference embeddings) as a
differentiable quantity.

Value: without a gradient the score is the scoring forward + ``Engine.pairwise``, bit for bit, for uniform batches and with
``lengths`` (where a clip's score is that of its own B = 1 call).

Gradient against float64, by the method and constants of tests/ref64.py (``check``: err_gpu <= C e32 + FLOOR top, C = 8,
FLOOR = 1e-7; ``test_gpu_forward_f64.C_X3P`` in front of e32 for bf16x3 products): the oracle's ``triplet_forward`` (the checkpoint's
head), the float64 mean distance to the references, ``torch.autograd.grad`` - every clip at its exact length, once in float64
and once in fp32.  The head's ReLU kink is taken out the way the loss path's tests do (``ref64.head_relu_undecided``): the
``Nomad`` is built from a copy of the seeded state dict whose ``embedding_layer.1.weight`` has zero columns for the undecided
channels of every clip used here, and the oracle runs on the same copy."""
import numpy as np
import pytest
import torch

import ref64
from nomad_amd.weights import num_frames
from oracle import nomad_oracle as O

pytestmark = pytest.mark.gpu

B, NR = 3, 5
CASES = {"T5": (5, 5, 5), "T9": (9, 9, 9), "ragged": (5, 7, 9)}


def _clips(Ts, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(0.1 * torch.randn(ref64.n_for(T), generator=gen)).clamp(-1, 1) for T in Ts]


def _padded(clips):
    """(B,1,N) with 0.5 behind every length: samples that are never read."""
    n = max(c.numel() for c in clips)
    out = torch.full((len(clips), 1, n), 0.5)
    for i, c in enumerate(clips):
        out[i, 0, :c.numel()] = c
    return out


@pytest.fixture(scope="module")
def data(sd0):
    gen = torch.Generator().manual_seed(77)
    refs = torch.randn(NR, 256, generator=gen, dtype=torch.float64)
    refs = (refs / refs.norm(dim=1, keepdim=True)).float()
    clips = {name: _clips(Ts, 100 + i) for i, (name, Ts) in enumerate(CASES.items())}
    for name, Ts in CASES.items():
        assert [num_frames(c.numel()) for c in clips[name]] == list(Ts)
    undecided = torch.zeros(768, dtype=torch.bool)
    for cs in clips.values():
        for c in cs:
            undecided |= ref64.head_relu_undecided(sd0, c[None])
    sd = {k: v.clone() for k, v in sd0.items()}
    sd["embedding_layer.1.weight"][:, undecided] = 0.0
    print(f"SCORE {int(undecided.sum())} head columns zeroed")
    return {"sd": sd, "refs": refs, "clips": clips, "up": torch.randn(B, generator=gen, dtype=torch.float64)}


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


def _score_oracle(sd, clips, refs, up, mult):
    """Every clip through the oracle at its exact length -> (scores (B,), [d (up_b score_b) / d clip_b]), in the dtype of the
    arguments; the distance itself is taken in float64 in both runs, as the engine does.  up: Python floats."""
    scores, grads = [], []
    for w, u in zip(clips, up):
        x = w[None].clone().requires_grad_(True)
        e = O.triplet_forward(sd, x, None, mult)
        s = (e.double()[:, None, :] - refs.double()[None]).norm(dim=-1).mean(1)[0]
        (g,) = torch.autograd.grad(s * u, x)
        scores.append(s.detach())
        grads.append(g[0])
    return torch.stack(scores), grads


_oracle_cache = {}


def _oracle(data, name, reduction, mult):
    """Computed once per (clips, upstream, feature_grad_mult), shared by the precisions."""
    key = (name, reduction, mult)
    if key not in _oracle_cache:
        up = data["up"].tolist() if reduction == "none" else [1.0 / B] * B
        _oracle_cache[key] = ref64.both(_score_oracle, data["sd"], data["clips"][name], data["refs"], up=up, mult=mult)
    return _oracle_cache[key]


def _gradient_case(nmd, data, name, reduction, mult, c):
    eng = nmd.engine
    clips = data["clips"][name]
    lens = [k.numel() for k in clips]
    ragged = len(set(lens)) > 1
    (s64, g64), (s32, g32) = _oracle(data, name, reduction, mult)
    prev = eng.feature_grad_mult
    eng.feature_grad_mult = mult
    try:
        x = _padded(clips).cuda().requires_grad_(True)
        s = nmd.score(x, data["refs"].cuda(), lengths=lens if ragged else None, reduction=reduction)
        if reduction == "none":
            assert s.shape == (B,) and s.dtype == torch.float64
            s.backward(data["up"].cuda())
        else:
            assert s.dim() == 0 and s.dtype == torch.float64
            s.backward()
    finally:
        eng.feature_grad_mult = prev
    assert x.grad.shape == x.shape and torch.isfinite(x.grad).all()
    for i, n in enumerate(lens):
        assert not x.grad[i, 0, n:].any(), i
    case = f"score {nmd.precision} {name} {reduction} fgm={mult:g}"
    ref64.check(case + " gradient", {f"d{i}": x.grad[i, 0, :n].cpu() for i, n in enumerate(lens)},
                {f"d{i}": g for i, g in enumerate(g64)}, {f"d{i}": g for i, g in enumerate(g32)}, c=c)
    # the value of the differentiated forward (embed_train): one number per clip, e32 at least half an fp32 ulp of it
    want64, want32 = (s64, s32) if reduction == "none" else (s64.mean(), s32.mean())
    half_ulp = float(np.spacing(np.float32(want64.abs().max().item()))) / 2
    ref64.check(case + " value", s.detach().cpu(), want64, want32, e32_min={"": half_ulp}, c=c)


@pytest.mark.parametrize("mult", [0.1, 1.0])
@pytest.mark.parametrize("reduction", ["none", "mean"])
@pytest.mark.parametrize("name", list(CASES))
def test_score_gradient_vs_float64(nmd_f32, data, name, reduction, mult):
    _gradient_case(nmd_f32, data, name, reduction, mult, ref64.C)


@pytest.mark.parametrize("mult", [0.1, 1.0])
@pytest.mark.parametrize("reduction", ["none", "mean"])
@pytest.mark.parametrize("name", list(CASES))
def test_score_gradient_bf16x3_vs_float64(nmd_x3, data, name, reduction, mult):
    from test_gpu_forward_f64 import C_X3P
    assert nmd_x3.engine.gemm_precision == "bf16x3"
    _gradient_case(nmd_x3, data, name, reduction, mult, C_X3P)


def test_score_without_a_gradient_is_the_scoring_forward_and_pairwise(nmd_f32, data):
    nmd, eng, refs = nmd_f32, nmd_f32.engine, data["refs"].cuda()
    x = _padded(data["clips"]["T9"]).cuda()
    want = eng.pairwise(nmd.model(x), refs)[1]
    with torch.no_grad():
        s = nmd.score(x, refs)
        s_req = nmd.score(x.clone().requires_grad_(True), refs.clone().requires_grad_(True))
        s_mean = nmd.score(x, refs, reduction="mean")
    s_plain = nmd.score(x, refs)                         # grad mode on, nothing requires a gradient
    s_2d = nmd.score(x[:, 0].contiguous(), refs)         # (B,N)
    assert s.shape == (B,) and s.dtype == torch.float64 and not s.requires_grad and not s_req.requires_grad
    for got in (s, s_req, s_plain, s_2d):
        assert torch.equal(got, want)
    assert torch.equal(s_mean, want.mean())
    # exact lengths: the clips' own embeddings, and every clip its own B = 1 call
    clips = data["clips"]["ragged"]
    lens = [c.numel() for c in clips]
    xr = _padded(clips).cuda()
    with torch.no_grad():
        sl = nmd.score(xr, refs, lengths=lens)
        own = torch.cat([nmd.model(xr[b:b + 1, :, :n].contiguous()) for b, n in enumerate(lens)])
        assert torch.equal(sl, eng.pairwise(own, refs)[1])
        assert torch.equal(sl, nmd.score(xr, refs, lengths=torch.tensor(lens)))
        for b, n in enumerate(lens):
            one = xr[b:b + 1, :, :n].contiguous()
            assert torch.equal(nmd.score(one, refs, lengths=[n])[0], sl[b]), b
            assert torch.equal(nmd.score(one, refs)[0], sl[b]), b
        padded = nmd.score(xr, refs)                     # the argument is honoured: the padded clips score differently
    assert not torch.equal(padded[:2], sl[:2])


def test_references_get_the_gradient_of_cdist_backward(nmd_f32, data):
    nmd, eng = nmd_f32, nmd_f32.engine
    refs, up = data["refs"].cuda(), data["up"].cuda()
    x = _padded(data["clips"]["T9"]).cuda()
    r = refs.clone().requires_grad_(True)
    nmd.score(x, r).backward(up)
    emb = nmd.model(x)
    _, db = eng.cdist_backward(emb, refs, g_mean=up, want_a=False, want_b=True)
    assert r.grad.dtype == torch.float32 and torch.equal(r.grad, db)
    # within the kernel test's bound of float64: 2^-24 |ref64| + 1e-12 sum_i |c_ij|, c_ij = up_i / Nr
    e64, r64 = emb.cpu().double().numpy(), refs.cpu().double().numpy()
    diff = e64[:, None, :] - r64[None]
    d = np.sqrt((diff * diff).sum(-1))
    c = np.broadcast_to((up.cpu().numpy() / NR)[:, None], d.shape)
    want = -np.einsum("ij,ijk->jk", c / d, diff)
    err = np.abs(r.grad.cpu().double().numpy() - want)
    bound = 2.0 ** -24 * np.abs(want) + 1e-12 * np.abs(c).sum(0)[:, None]
    print(f"SCORE d / d references: max err {err.max():.3e}, worst share of the bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    # both arguments differentiated: the embeddings are embed_train's, the references' gradient is still cdist_backward's
    xg, r2 = x.clone().requires_grad_(True), refs.clone().requires_grad_(True)
    nmd.score(xg, r2, reduction="mean").backward()
    emb_t = eng.embed_train(x)[0]
    g = torch.full((B,), 1.0 / B, dtype=torch.float64, device="cuda")
    assert torch.equal(r2.grad, eng.cdist_backward(emb_t, refs, g_mean=g, want_a=False, want_b=True)[1])
    assert xg.grad is not None and xg.grad.abs().max() > 0
    # a float64 bank on the host gets its gradient where and as it lives
    r3 = data["refs"].double().requires_grad_(True)
    nmd.score(x, r3).backward(up)
    assert r3.grad.dtype == torch.float64 and r3.grad.device.type == "cpu" and torch.equal(r3.grad, db.cpu().double())


def test_refusals_come_before_any_launch(nmd_f32, data, monkeypatch):
    nmd, eng, refs = nmd_f32, nmd_f32.engine, data["refs"].cuda()
    x = _padded(data["clips"]["T5"]).cuda()

    def launched(*a, **k):
        raise AssertionError("an engine call was made")
    for name in ("embed", "embed_ragged", "embed_train", "embed_train_ragged", "pairwise", "cdist_backward", "embed_bf16x3", "embed_bf16"):
        monkeypatch.setattr(eng, name, launched)
    for xs in (x, x.clone().requires_grad_(True)):
        for bad, exc in ((refs[:, :128], ValueError), (refs[0], ValueError), (refs[:0], ValueError), (refs[None], ValueError),
                         (refs.long(), TypeError), (refs.cpu().numpy(), TypeError)):
            with pytest.raises(exc):
                nmd.score(xs, bad)
        with pytest.raises(ValueError, match="reduction"):
            nmd.score(xs, refs, reduction="sum")
        with pytest.raises(ValueError):
            nmd.score(xs, refs, lengths=[400, 400])
        with pytest.raises(ValueError):
            nmd.score(xs[:, :, None], refs)
        try:
            eng.encoder_depth = 6
            with pytest.raises(RuntimeError, match="whole encoder"):
                nmd.score(xs, refs)
        finally:
            eng.encoder_depth = 12
    assert eng.encoder_depth == 12
    monkeypatch.undo()
    assert nmd.score(x, refs).shape == (B,)
