"""GPU: the pooled backbone features (``Engine.embed_features`` / ``embed_features_ragged``, nomad_embed_features*:
``Origw2v.forward``, the time mean of the backbone's output) against float64, against the reference's own ``Origw2v``, bit for
bit between the ragged and the per-clip calls, and on poisoned buffers.

Method of tests/test_gpu_forward_f64.py (tests/ref64.py): ``O.backbone(sd, wav)[0].mean(1)`` runs once in float64 and once in
fp32; per case the GPU must satisfy ``err_gpu <= c * e32 + FLOOR * top`` inside ``guard.guarded()``.  The constants start from
the ones that file gives the layer outputs these features average: C_F32 = 8, C_X3S = 90, C_BF16 = 50 000.

Worst err_gpu / e32 measured on one MI355X over every case of this file (``check`` prints it per case), and the constant each
path has here:

  path     worst err_gpu / e32 (where)                                              c
  fp32     3.68 (peaky B=1 T=257; sd0: 3.67 at T=64; ragged 1.43)                   C_F32 = ref64.C = 8
  bf16x3   88.41 (sd0 B=1 T=1499; 68.3 at T=257, 56.4 at T=64, 11.1 at T=1)        C_X3S = 90 (the layer outputs' constant)
  bf16     60 940 (sd0 B=1 T=1499; 48 599 at T=257, 41 779 at T=64, 9 206 at T=1)  C_BF16 = 125 000 (was 50 000)

The ratio of a time MEAN grows with the clip's length: the fp32 oracle's error averages away over the frames (e32 6.0e-6 at
T = 1, 3.9e-7 at T = 64, 2.6e-7 at T = 1499) while the reduced-precision forwards' error is systematic per clip and does not
(bf16: err_gpu 1.6e-2 at T = 64, 1.7e-2 at T = 257, 1.6e-2 at T = 1499 - what bf16 storage costs on values of rms 0.9; bf16x3:
2.2e-5 .. 2.9e-5 from T = 63 to T = 1499).  bf16x3 stays inside the layer outputs' constant, with 2 % to spare at T = 1499, and
keeps it.  bf16 exceeded its 50 000 at T = 1499 (ratio 60 940) with a correct kernel - the new stage, ``head_mean_kernel``,
is the one the fp32 and bf16x3 cases hold to 3.7 and 88 times fp32's own error, the forward in front of it is the one
tests/test_gpu_forward_f64.py holds to 50 000 on embeddings, and err_gpu is the same 1.6e-2 as at T = 64 - so by that file's
rule (about 2x, at most 3x, the worst ratio measured) the constant for bf16 time means is 125 000 = 2.05 x 60 940.  As there,
bf16 is the weaker gate: it says that nothing is wrong by more than about twice what bf16 storage already costs.

Geometries: T = 1, 2, 63, 64, 65, 257 and 1499; B = 1 and B > 1; B x T = 4000 (the two-stream split); two cases with the
peaky-attention weights; a ragged batch with a T = 1 clip next to a 30 s clip.

The fixture test pins the kernel to reference code: tests/golden/ref_networks.npz holds ``pooled_seed0`` / ``pooled_peaky``, outputs
of the reference's ``Origw2v`` class (oracle/make_golden.py), and the fp32 features must lie within 2e-5 / 2e-4 of them - the
tolerances tests/test_oracle.py holds the oracle to.  The fixtures sit 1.1e-6 / 1.1e-5 from the float64 oracle and fp32's own
error is 1.2e-6 / 1.1e-5, so a result inside the float64 bound is inside these with a factor of two to spare."""
import contextlib
import os

import numpy as np
import pytest
import torch

import guard
import ref64
from conftest import GOLD
from nomad_amd.weights import num_frames
from oracle import nomad_oracle as O

pytestmark = pytest.mark.gpu

C_F32 = ref64.C
C_X3S = 90.0
C_BF16 = 125000.0      # time means in bf16: 2.05 x the worst ratio measured (docstring); the layer outputs' 50 000 was exceeded at T = 1499
C_OF = {"fp32": C_F32, "bf16x3": C_X3S, "bf16": C_BF16}
PRECISIONS = ["fp32", "bf16x3", "bf16"]

# a subset of tests/test_gpu_forward_f64.py's UNIFORM: T = 1, 2, 63 (B = 2), 64, 65 (B = 3), 257, 1499, B x T = 4000, two peaky
UNIFORM = [
    ("sd0", 1, 400), ("sd0", 1, 720), ("sd0", 2, 20240), ("sd0", 1, 20560), ("sd0", 3, 20880), ("sd0", 1, 82320),
    ("sd0", 1, 479760), ("sd0", 32, 40080),
    ("peaky", 2, 20240), ("peaky", 1, 82320),
]
RAGGED_N = [400, 479760, 9001, 20880, 720, 30080]      # T = 1 next to a 30 s clip
BITS_N = [16384, 400, 27225, 9001, 64000, 30267, 5000, 12345, 48000]   # the list of tests/test_gpu_bf16.py


def _wav(B, n, seed=0):
    g = torch.Generator().manual_seed(seed * 1000003 + B * 7919 + n)
    return (0.1 * torch.randn(B, n, generator=g)).clamp(-1, 1)


def _pooled(sd, wav):
    with torch.no_grad():
        return O.backbone(sd, wav)[0].mean(1)


@pytest.fixture(scope="module")
def weights(sd0, sd_peaky):
    return {"sd0": sd0, "peaky": sd_peaky}


@pytest.fixture(scope="module")
def engines(engine, engine_peaky):
    return {"sd0": engine, "peaky": engine_peaky}


@pytest.fixture(scope="module", params=UNIFORM, ids=lambda c: f"{c[0]}-B{c[1]}-n{c[2]}")
def uniform(request, weights):
    name, B, n = request.param
    wav = _wav(B, n)
    return name, wav, ref64.both(_pooled, weights[name], wav)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_embed_features_against_float64(engines, uniform, precision):
    name, wav, (r64, r32) = uniform
    B, n = wav.shape
    case = f"embed_features[{precision}] {name} B={B} n={n} T={num_frames(n)}"
    with guard.guarded(case=case):
        feat = engines[name].embed_features(wav.cuda(), precision=precision)
        torch.cuda.synchronize()
    assert feat.shape == (B, 768) and feat.dtype == torch.float32
    ref64.check(case, feat.cpu(), r64, r32, c=C_OF[precision])


@pytest.fixture(scope="module")
def ragged(weights):
    waves = [_wav(1, n, seed=20 + i)[0] for i, n in enumerate(RAGGED_N)]
    per = [ref64.both(_pooled, weights["sd0"], w[None]) for w in waves]      # the oracle runs per clip
    return waves, torch.cat([p[0] for p in per]), torch.cat([p[1] for p in per])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_embed_features_ragged_against_float64(engine, ragged, precision):
    waves, r64, r32 = ragged
    case = f"embed_features_ragged[{precision}] {len(waves)} clips"
    with guard.guarded(case=case):
        feat = engine.embed_features_ragged([w.cuda() for w in waves], precision=precision)
        torch.cuda.synchronize()
    ref64.check(case, feat.cpu(), r64, r32, c=C_OF[precision])


def test_against_the_reference_networks_fixture(engine, engine_peaky):
    g = np.load(os.path.join(GOLD, "ref_networks.npz"))
    wav = torch.from_numpy(g["wav"]).cuda()
    for tag, eng, tol in (("seed0", engine, 2e-5), ("peaky", engine_peaky, 2e-4)):
        feat = eng.embed_features(wav).cpu()
        feat3 = eng.embed_features(wav[:, None, :]).cpu()                    # (B, 1, N) as the reference takes it
        err = float((feat - torch.from_numpy(g[f"pooled_{tag}"])).abs().max())
        print(f"REFNET pooled_{tag}: max |diff| {err:.3e} (tolerance {tol:.0e})")
        assert err < tol, tag
        assert torch.equal(feat, feat3)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_equals_per_clip_calls_bit_for_bit(engine, precision):
    waves = [_wav(1, n, seed=40 + i)[0].cuda() for i, n in enumerate(BITS_N)]
    emb_before = engine.embed_ragged(waves, precision=precision).clone()
    one_before = engine.embed(waves[0][None]).clone()
    rag = engine.embed_features_ragged(waves, precision=precision)
    per = torch.cat([engine.embed_features(w[None], precision=precision) for w in waves])
    again = engine.embed_features_ragged(waves, precision=precision)
    host = engine.embed_features_ragged([w.cpu().numpy() for w in waves], precision=precision)   # host inputs: the staging path
    torch.cuda.synchronize()
    assert rag.shape == (len(waves), 768)
    assert torch.equal(rag, per), f"{int((rag != per).any(1).sum())} clips differ from their own call"
    assert torch.equal(rag, again) and torch.equal(rag, host)
    assert torch.equal(engine.embed_ragged(waves, precision=precision), emb_before)
    assert torch.equal(engine.embed(waves[0][None]), one_before)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_split_batch_changes_no_bit(engine, precision):
    """32 clips of 40080 samples are 4000 frames: two halves on two streams.  Each clip equals its own call."""
    wav = _wav(32, 40080, seed=3).cuda()
    whole = engine.embed_features(wav, precision=precision)
    rag = engine.embed_features_ragged([w for w in wav], precision=precision)
    per = torch.cat([engine.embed_features(wav[i:i + 1], precision=precision) for i in (0, 15, 16, 31)])
    torch.cuda.synchronize()
    assert torch.equal(whole[[0, 15, 16, 31]], per) and torch.equal(rag, whole)


# ---- poison (the mechanism of tests/test_gpu_poison.py) -------------------------------------------------------------------
POISON = 0xFF


def _fill(t):
    if t is not None and t.numel():
        t.reshape(-1).view(torch.uint8).fill_(POISON)
    return t


class _PoisonTorch:
    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*args, **kw):
        return _fill(torch.empty(*args, **kw))

    @staticmethod
    def empty_like(*args, **kw):
        return _fill(torch.empty_like(*args, **kw))


@contextlib.contextmanager
def _poisoned(eng):
    from nomad_amd import engine as engine_mod
    for ws in [eng._ws, eng._l1_scratch, *eng._ws_side.values()]:
        _fill(ws)
    eng.diag_poison_scratch(POISON)
    torch.cuda.synchronize()
    real = engine_mod.torch
    engine_mod.torch = _PoisonTorch()
    try:
        yield
    finally:
        engine_mod.torch = real


@pytest.mark.parametrize("precision", PRECISIONS)
def test_poisoned_workspace_and_output(built_lib, sd0, precision):
    """Workspaces, the context's scratch and every tensor the call allocates (the output included) start as NaN bytes: the
    result is finite and equal to the unpoisoned run's, uniform and ragged."""
    from nomad_amd.engine import Engine
    eng = Engine(sd0, 0, diag=True)
    try:
        wav = _wav(3, 20887, seed=9).cuda()                                   # T = 65
        clips = [_wav(1, n, seed=60 + i)[0].cuda() for i, n in enumerate([400, 720, 20560, 20887, 64000])]
        ref_u = eng.embed_features(wav, precision=precision).cpu()
        ref_r = eng.embed_features_ragged(clips, precision=precision).cpu()
        torch.cuda.synchronize()
        with _poisoned(eng):
            got_u = eng.embed_features(wav, precision=precision).cpu()
        with _poisoned(eng):
            got_r = eng.embed_features_ragged(clips, precision=precision).cpu()
        for ref, got in ((ref_u, got_u), (ref_r, got_r)):
            assert bool(torch.isfinite(got).all())
            assert np.array_equal(ref.numpy().view(np.uint8), got.numpy().view(np.uint8))
    finally:
        torch.cuda.synchronize()
        eng.close()


def test_bad_arguments_name_the_function(engine):
    """The statuses of the embedding entry points, with a nomad_last_error() text that names the feature function."""
    import ctypes as C
    from nomad_amd import _lib
    lib = engine.lib
    wav = _wav(2, 4000).cuda()
    good = engine.embed_features(wav).clone()
    feat = torch.full((2, 768), 7.0, device="cuda")
    need = engine.workspace_bytes(2, 4000)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(B=2, w=wav.data_ptr(), n=4000, p=0, f=feat.data_ptr(), wsp=ws.data_ptr(), nb=need):
        return lib.nomad_embed_features(engine.ctx, w, B, n, p, f, wsp, nb, None)
    for kw in (dict(B=0), dict(w=None), dict(f=None), dict(wsp=None), dict(n=399), dict(p=3), dict(p=-1)):
        assert call(**kw) == _lib.NOMAD_ERR_INVALID, kw
        assert b"nomad_embed_features" in lib.nomad_last_error(), kw
    assert call(nb=need - 1) == _lib.NOMAD_ERR_WORKSPACE and b"nomad_embed_features: workspace" in lib.nomad_last_error()
    lens = (C.c_int * 2)(4000, 399)
    rc = lib.nomad_embed_features_ragged(engine.ctx, wav.data_ptr(), 2, 4000, lens, 0, feat.data_ptr(), ws.data_ptr(), need, None)
    assert rc == _lib.NOMAD_ERR_INVALID and b"nomad_embed_features_ragged" in lib.nomad_last_error()
    lens = (C.c_int * 2)(4000, 4000)
    rc = lib.nomad_embed_features_ragged(engine.ctx, wav.data_ptr(), 2, 4000, lens, 7, feat.data_ptr(), ws.data_ptr(), need, None)
    assert rc == _lib.NOMAD_ERR_INVALID and b"nomad_embed_features_ragged" in lib.nomad_last_error()
    with pytest.raises(ValueError, match="shorter than"):
        engine.embed_features(_wav(2, 399).cuda())
    with pytest.raises(ValueError, match="precision"):
        engine.embed_features(wav, precision="fp16")
    torch.cuda.synchronize()
    assert bool((feat == 7.0).all())                                          # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(feat, good)
