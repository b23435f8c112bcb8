"""GPU: every forward entry point against float64, inside guarded buffers.

Method: tests/ref64.py.  The CPU oracle (``O.backbone`` with taps, ``O.head``, ``O.nomad_loss``, ``O.pairwise``) runs once in
float64 and once in fp32 on the same input; per tensor the GPU must satisfy ``err_gpu <= c * e32 + FLOOR * top``.  Every
call runs inside ``guard.guarded()``: workspaces of exactly ``workspace_bytes`` between 32 MiB guards, every output between
64 KiB guards, all checked after the case.

Compared: conv0 .. conv6 and the projection / zero pad frames of ``xpad`` (``diag_keep_intermediates``), the 12 layer
outputs, embeddings (the checkpoint's head and a custom one), distances of the GPU embeddings (``pairwise``) against float64
distances of float64 embeddings, and ``Nomad.forward``'s loss.  Entry points: ``embed`` with fp32 and with bf16x3 products
(``gemm_precision``), with and without layer outputs; ``embed_bf16``; ``embed_bf16x3`` with and without layer outputs;
``embed_ragged`` in fp32 / bf16 / bf16x3; ``embed_train``'s forward; ``Nomad(precision=...).forward()`` at B = 1, 2, 32.
Geometries: T = 1, 2, 63, 64, 65, 93 (conv1 .. conv4 all odd), 149, 199, 256, 257 (kAttnResidentMaxT + 1) and 1499 (one 30 s
clip); B x T = 3999 / 4000 (Engine.F32_SPLIT_ROWS, the two-stream split) and 4095 / 4096 (kSplitKLayersMaxM, the split-K
layer-output forward); B = 1 for every entry point, including the one-clip layer-output forwards whose conv GEMMs used to
write partial products past the split-K block (test_one_clip_layer_output_forward_*); a ragged batch of a T = 1 clip next to
a 30 s clip; the peaky-attention weights (``seeded_state_dict(1, qk_gain=6)``).

Bounds: err_gpu <= c * e32 + 1e-7 * top (ref64.FLOOR), c per path.  Worst err_gpu / e32 measured on one MI355X over every
case of this file (``check`` prints it per group), and the constant each path gets (fp32 keeps ref64's C; every other
constant is about 2x, at most 3x, its path's worst):

  path                              worst err_gpu / e32 (where)                                c
  fp32 products                     7.05 conv1 (B=2, T=63); layers 5.11; embeddings 4.67       C_F32 = ref64.C = 8
                                    (peaky T=257); loss 1.00
    distances from fp32 embeddings  8.88 (B=3, T=65; inside C_F32 only through the floor)      C_F32_DIST = 20
  bf16x3 products on fp32 buffers   38.95 emb (embed_train, T=1499); conv4 30.0; layers 29.3   C_X3P = 80
  split-storage bf16x3              42.20 layers (B=32, T=128); emb 37.75; distances 35.4      C_X3S = 90
  Nomad(precision="bf16x3") loss    81.8 (B=2 x 16384: err_gpu 5.8e-6, e32 7.1e-8; the loss     C_X3_LOSS = 200
                                    averages 13 means of |differences|, fp32's e32 is tiny)
  bf16                              23 948 emb (T=257); distances 17 549                      C_BF16 = 50 000

bf16 is the weaker gate: its error is set by bf16 rounding (~3e-3 on a unit-norm embedding), so the bound says only that
nothing is wrong by more than about twice what bf16 storage already costs.  The fp32-class constants come from products
that keep 16 to 24 mantissa bits: bf16x3 drops the lo x lo term and rounds each operand's low half to bf16.

The file takes about 80 s on one MI355X, most of it the CPU oracle (float64 and fp32) of its ~400 s of audio."""
import os
import subprocess
import sys

import pytest
import torch

import guard
import ref64
from nomad_amd.weights import num_frames
from oracle import nomad_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_F32 = ref64.C         # fp32 products
C_F32_DIST = 20.0       # distances of fp32 embeddings
C_X3P = 80.0            # bf16x3 products on fp32 buffers (Engine.gemm_precision = "bf16x3")
C_X3S = 90.0            # split-storage bf16x3 (embed_bf16x3, embed_ragged precision="bf16x3")
C_X3_LOSS = 200.0       # Nomad(precision="bf16x3").forward()'s loss
C_BF16 = 50000.0        # bf16
C_PRODUCTS = {"fp32": C_F32, "x3": C_X3P}
C_DIST = {"fp32": C_F32_DIST, "x3": C_X3P}

# (weights, B, n): n = ref64.n_for(T) gives conv1 .. conv4 odd lengths wherever they can be (Winograd drops the last output)
UNIFORM = [
    ("sd0", 1, 400), ("sd0", 1, 720), ("sd0", 1, 9001), ("sd0", 1, 16384), ("sd0", 1, 30080), ("sd0", 1, 48000),
    ("sd0", 2, 20240), ("sd0", 1, 20560), ("sd0", 3, 20880), ("sd0", 1, 82000), ("sd0", 1, 82320), ("sd0", 2, 64000),
    ("sd0", 1, 479760),
    ("sd0", 31, 41360), ("sd0", 32, 40080), ("sd0", 21, 62480), ("sd0", 32, 41040),   # B x T = 3999, 4000, 4095, 4096
    ("peaky", 1, 400), ("peaky", 2, 20240), ("peaky", 1, 82320),
]
FAULT_N = [400, 9001, 16384, 48000]   # one clip: conv GEMM partials of 39 936 .. 2 456 576 floats against a block of S x 6144 x T


def _wav(B, n, seed=0):
    g = torch.Generator().manual_seed(seed * 1000003 + B * 7919 + n)
    return (0.1 * torch.randn(B, n, generator=g)).clamp(-1, 1)


def _custom_head(seed=5):
    g = torch.Generator().manual_seed(seed)
    return 0.02 * torch.randn(256, 768, generator=g), 0.01 * torch.randn(256, generator=g)


@pytest.fixture(scope="module")
def weights(sd0, sd_peaky):
    return {"sd0": sd0, "peaky": sd_peaky}


_SD = {}


def _sd(weights, name, dtype):
    key = (name, dtype)
    if key not in _SD:
        _SD[key] = ref64.cast(weights[name], dtype)
    return _SD[key]


def _oracle(weights, name, wav, taps=False):
    """{64: ..., 32: ...}: layers {l: (B,T,768)}, emb (checkpoint head), emb_c (custom head), and with taps conv0..6 / proj."""
    hw, hb = _custom_head()
    out = {}
    for bits, dt in ((64, torch.float64), (32, torch.float32)):
        sd = _sd(weights, name, dt)
        t = {} if taps else None
        with torch.no_grad():
            x, layers = O.backbone(sd, wav.to(dt), t)
            r = {"layers": {str(l): y for l, y in enumerate(layers)},
                 "emb": O.head(x, sd["embedding_layer.1.weight"], sd["embedding_layer.1.bias"]),
                 "emb_c": O.head(x, hw.to(dt), hb.to(dt))}
        if taps:
            r.update({k: v for k, v in t.items() if k.startswith("conv") or k == "proj"})
        out[bits] = r
    return out


def _check(case, got, ref, key, c=ref64.C):
    """ref64.check of one group (the 12 layers, or one embedding) of an oracle result."""
    return ref64.check(case, got, ref[64][key], ref[32][key], c=c)


def _layers(layers):
    return {str(l): layers[l].cpu() for l in range(12)}


def _pair_check(case, emb, ref, key, eng, c):
    """pairwise(emb[:h], emb[h:]) on the GPU against O.pairwise of the float64 / fp32 oracle embeddings."""
    h = emb.shape[0] // 2
    dist, mean = eng.pairwise(emb[:h].contiguous(), emb[h:].contiguous())
    r = {bits: O.pairwise(ref[bits][key][:h].double().numpy(), ref[bits][key][h:].double().numpy()) for bits in (64, 32)}
    ref64.check(case + " pairwise", {"dist": dist.cpu(), "mean": mean.cpu()},
                {"dist": torch.from_numpy(r[64][0]), "mean": torch.from_numpy(r[64][1])},
                {"dist": torch.from_numpy(r[32][0]), "mean": torch.from_numpy(r[32][1])}, c=c)


def _engine(sd, x3_products=False):
    from nomad_amd.engine import Engine
    eng = Engine(sd, 0)
    if x3_products:
        eng.gemm_precision = "bf16x3"
    return eng


@pytest.fixture(scope="module")
def engines(built_lib, weights):
    """{(weights name, "fp32" | "x3"): Engine}: fp32 products, and bf16x3 products on fp32 buffers."""
    made = {(w, p): _engine(weights[w], p == "x3") for w in weights for p in ("fp32", "x3")}
    yield made
    torch.cuda.synchronize()
    for eng in made.values():
        eng.close()


@pytest.fixture(scope="module", params=UNIFORM, ids=lambda c: f"{c[0]}-B{c[1]}-n{c[2]}")
def uniform(request, weights):
    """(name, wav on the CPU, oracle): one input per geometry, shared by every entry point that runs it."""
    name, B, n = request.param
    wav = _wav(B, n)
    return name, wav, _oracle(weights, name, wav)


def _id(name, wav):
    B, n = wav.shape
    return f"{name} B={B} n={n} T={num_frames(n)}"


# ---- embed: fp32 products, and bf16x3 products on fp32 buffers ---------------------------------------------------------------
@pytest.mark.parametrize("products", ["fp32", "x3"])
def test_embed(engines, uniform, products):
    """Without layer outputs (scoring: the two-stream split from B x T = 4000), with them (split-K below 4096 frames), each with
    the checkpoint's head and a custom one."""
    name, wav, ref = uniform
    eng = engines[(name, products)]
    w = wav.cuda()
    hw, hb = (t.cuda() for t in _custom_head())
    case, c = f"embed[{products}] {_id(name, wav)}", C_PRODUCTS[products]
    with guard.guarded(case=case):
        emb = eng.embed(w)
        emb_c = eng.embed(w, head=(hw, hb))
        emb_l, layers = eng.embed(w, want_layers=True)
        emb_lc, layers_c = eng.embed(w, head=(hw, hb), want_layers=True)
        torch.cuda.synchronize()
    _check(case + " emb", emb.cpu(), ref, "emb", c)
    _check(case + " emb head", emb_c.cpu(), ref, "emb_c", c)
    _check(case + " layers", _layers(layers), ref, "layers", c)
    _check(case + " layers emb", emb_l.cpu(), ref, "emb", c)
    _check(case + " layers emb head", emb_lc.cpu(), ref, "emb_c", c)
    assert torch.equal(layers, layers_c), "the head changed the layer outputs"
    if wav.shape[0] >= 2:
        with guard.guarded(case=case + " pairwise"):
            _pair_check(case, emb, ref, "emb", eng, C_DIST[products])


def test_embed_bf16(engines, uniform):
    name, wav, ref = uniform
    eng = engines[(name, "fp32")]
    case = f"embed_bf16 {_id(name, wav)}"
    with guard.guarded(case=case):
        emb = eng.embed_bf16(wav.cuda())
        torch.cuda.synchronize()
    _check(case + " emb", emb.cpu(), ref, "emb", C_BF16)
    if wav.shape[0] >= 2:
        with guard.guarded(case=case + " pairwise"):
            _pair_check(case, emb, ref, "emb", eng, C_BF16)


def test_embed_bf16x3(engines, uniform):
    """Split-storage bf16x3: scoring (two streams from X3_SPLIT_ROWS) and the layer-output form with a custom head."""
    name, wav, ref = uniform
    eng = engines[(name, "fp32")]
    w = wav.cuda()
    hw, hb = (t.cuda() for t in _custom_head())
    case = f"embed_bf16x3 {_id(name, wav)}"
    with guard.guarded(case=case):
        emb = eng.embed_bf16x3(w)
        emb_c, layers = eng.embed_bf16x3(w, head=(hw, hb), want_layers=True)
        torch.cuda.synchronize()
    _check(case + " emb", emb.cpu(), ref, "emb", C_X3S)
    _check(case + " layers", _layers(layers), ref, "layers", C_X3S)
    _check(case + " layers emb head", emb_c.cpu(), ref, "emb_c", C_X3S)
    if wav.shape[0] >= 2:
        with guard.guarded(case=case + " pairwise"):
            _pair_check(case, emb, ref, "emb", eng, C_X3S)


@pytest.mark.parametrize("products", ["fp32", "x3"])
def test_embed_train_forward(engines, uniform, products):
    """The training-mode forward (Nomad.forward's differentiated branch; stochastic settings off): its emb and layers."""
    name, wav, ref = uniform
    eng = engines[(name, products)]
    case = f"embed_train[{products}] {_id(name, wav)}"
    with guard.guarded(case=case):
        emb, layers, _saved = eng.embed_train(wav.cuda())
        torch.cuda.synchronize()
    _check(case + " layers", _layers(layers), ref, "layers", C_PRODUCTS[products])
    _check(case + " emb", emb.cpu(), ref, "emb", C_PRODUCTS[products])


# ---- every stage of the fp32-buffer forward ----------------------------------------------------------------------------------
STAGES = [("sd0", 1, 400), ("sd0", 1, 720), ("sd0", 1, 9001), ("sd0", 1, 30080), ("sd0", 2, 20240), ("sd0", 3, 20880),
          ("sd0", 2, 64000), ("sd0", 1, 82320), ("peaky", 2, 9001)]


@pytest.mark.parametrize("products", ["fp32", "x3"])
@pytest.mark.parametrize("name,B,n", STAGES)
def test_stages(engines, weights, name, B, n, products):
    """conv0 .. conv6 (Winograd conv1 .. conv4 with fp32 products, implicit GEMMs with bf16x3 products) and the projection in
    the pos-conv input buffer xpad, whose 64 pad frames on each side must be exactly zero."""
    wav = _wav(B, n, seed=3)
    ref = _oracle(weights, name, wav, taps=True)
    eng = engines[(name, products)]
    case = f"stages[{products}] {_id(name, wav)}"
    T = num_frames(n)
    eng.diag_keep_intermediates(True)
    try:
        with guard.guarded(case=case):
            eng.embed(wav.cuda())
            torch.cuda.synchronize()
            got = {f"conv{i}": eng.diag_region(B, n, f"conv{i}").cpu().view(B, -1, 512) for i in range(7)}
            xg = eng.diag_region(B, n, "xpad").cpu().view(16, B, T + 128, 48)
    finally:
        eng.diag_keep_intermediates(False)
    for i in range(7):
        _check(f"{case} conv{i}", got[f"conv{i}"], ref, f"conv{i}", C_PRODUCTS[products])
    assert xg[:, :, :64].abs().max().item() == 0.0 and xg[:, :, 64 + T:].abs().max().item() == 0.0, "xpad pad frames"
    _check(case + " proj", xg[:, :, 64:64 + T].permute(1, 2, 0, 3).reshape(B, T, 768), ref, "proj", C_PRODUCTS[products])


# ---- ragged ------------------------------------------------------------------------------------------------------------------
RAGGED_N = {"mixed": [400, 479760, 9001, 20880, 720, 30080],   # T = 1 next to a 30 s clip, odd conv lengths, T = 65, 2, 93
            "one": [9001]}


@pytest.fixture(scope="module", params=list(RAGGED_N))
def ragged(request, weights):
    waves = [_wav(1, n, seed=20 + i)[0] for i, n in enumerate(RAGGED_N[request.param])]
    per = [_oracle(weights, "sd0", w[None]) for w in waves]     # the oracle runs per clip
    return waves, {bits: {"emb": torch.cat([r[bits]["emb"] for r in per])} for bits in (64, 32)}


@pytest.mark.parametrize("precision,products", [("fp32", "fp32"), ("fp32", "x3"), ("bf16", "fp32"), ("bf16x3", "fp32")])
def test_embed_ragged(engines, ragged, precision, products):
    waves, ref = ragged
    eng = engines[("sd0", products)]
    case = f"embed_ragged[{precision}/{products}] {len(waves)} clips"
    c, cd = {"fp32": (C_PRODUCTS[products], C_DIST[products]), "bf16": (C_BF16, C_BF16), "bf16x3": (C_X3S, C_X3S)}[precision]
    with guard.guarded(case=case):
        emb = eng.embed_ragged([w.cuda() for w in waves], precision=precision)
        torch.cuda.synchronize()
    _check(case + " emb", emb.cpu(), ref, "emb", c)
    if len(waves) >= 2:
        with guard.guarded(case=case + " pairwise"):
            _pair_check(case, emb, ref, "emb", eng, cd)


# ---- Nomad.forward: the loss -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad", [True, False], ids=["grad", "no_grad"])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("B,n", [(1, 16384), (2, 16384), (32, 25000)])
def test_nomad_forward_loss(built_lib, sd0, weights, B, n, precision, grad):
    """The clean branch is a layer-output forward on the side stream (B = 1, bf16x3: fp32 buffers with bf16x3 products, the
    one-clip case that used to overflow its split-K block; B = 32 x 25000 samples: the split-storage forward); the estimate
    branch is embed_train with a gradient, the clean branch's forward without."""
    from nomad_amd.nomad import Nomad
    est, cln = _wav(B, n, seed=1), _wav(B, n, seed=2)
    nmd = Nomad(weights=sd0, precision=precision)
    eng = nmd.engine
    try:
        hw, hb = nmd.lossnet_layers.embedding_weight.cpu(), nmd.lossnet_layers.embedding_bias.cpu()
        ref = {}
        for bits, dt in ((64, torch.float64), (32, torch.float32)):
            sd = _sd(weights, "sd0", dt)
            with torch.no_grad():
                outs = [O.lossnet_forward(sd, w.to(dt), hw.to(dt), hb.to(dt)) for w in (cln, est)]
            ref[bits] = O.nomad_loss(outs[0], outs[1]).reshape(1)
        case = f"Nomad[{precision}].forward B={B} n={n} {'grad' if grad else 'no_grad'}"
        with guard.guarded(case=case):
            e = est.cuda().requires_grad_(grad)
            with torch.set_grad_enabled(grad):
                loss = nmd.forward(e, cln.cuda())
            torch.cuda.synchronize()
        c = C_F32 if precision == "fp32" else C_X3_LOSS
        ref64.check(case + " loss", loss.detach().cpu().reshape(1), ref[64], ref[32], c=c)
    finally:
        torch.cuda.synchronize()
        eng.close()


# ---- one-clip layer-output forwards: the split-K block --------------------------------------------------------------------
@pytest.mark.parametrize("n", FAULT_N)
def test_one_clip_layer_output_forward_bf16x3_products(engines, weights, n):
    """B = 1 with bf16x3 products on fp32 buffers: conv1 .. conv4 run as implicit GEMMs of M = L[i] rows (several times the
    frames), which must not split K into a block sized for the frames.  Guards intact, layers within the bound, the same
    bits from a repeated call on the same engine (the embedding is NOT compared with the call without layer outputs: on fp32
    buffers the layer-output forward takes the loss path's split-K bits by design)."""
    wav = _wav(1, n, seed=7)
    ref = _oracle(weights, "sd0", wav)
    eng = engines[("sd0", "x3")]
    case = f"one-clip layers[x3] n={n}"
    with guard.guarded(case=case):
        e1, l1 = eng.embed(wav.cuda(), want_layers=True)
        e1, l1 = e1.cpu(), l1.cpu()
        e2, l2 = eng.embed(wav.cuda(), want_layers=True)
        torch.cuda.synchronize()
    assert torch.equal(e1, e2.cpu()) and torch.equal(l1, l2.cpu()), "a repeated call changed the bits"
    _check(case + " layers", _layers(l1), ref, "layers", C_X3P)
    _check(case + " emb", e1, ref, "emb", C_X3P)


_CHILD = r"""
import sys, torch
sys.path[:0] = [{root!r}, {tests!r}]
import guard
from nomad_amd.engine import Engine
from nomad_amd.weights import seeded_state_dict
eng = Engine(seeded_state_dict(0), 0, diag=True)
out = {{}}
for n in {ns!r}:
    g = torch.Generator().manual_seed(7 * 1000003 + 7919 + n)
    wav = (0.1 * torch.randn(1, n, generator=g)).clamp(-1, 1).cuda()
    with guard.guarded(check=False) as gd:
        e1, l1 = eng.embed(wav, want_layers=True)
        e1, l1 = e1.cpu(), l1.cpu()
        e2, l2 = eng.embed(wav, want_layers=True)
        torch.cuda.synchronize()
    out[n] = dict(emb=e1, layers=l1, same=bool(torch.equal(e1, e2.cpu()) and torch.equal(l1, l2.cpu())), damaged=gd.damaged())
torch.save(out, {path!r})
eng.close()
"""


def test_one_clip_layer_output_forward_direct_conv(built_lib, weights, tmp_path):
    """The same with fp32 products and conv1 .. conv4 as implicit GEMMs (NOMAD_F32_CONV_WINO=0, libnomad_diag.so), in a child
    process: the switch is read when a context is created."""
    path = str(tmp_path / "out.pt")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), ns=FAULT_N, path=path)
    env = dict(os.environ, NOMAD_F32_CONV_WINO="0")
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = torch.load(path)
    for n in FAULT_N:
        res, case = got[n], f"one-clip layers[direct conv] n={n}"
        assert not res["damaged"], f"{case}: guard bytes overwritten: {res['damaged'][:6]}"
        assert res["same"], f"{case}: a repeated call changed the bits"
        ref = _oracle(weights, "sd0", _wav(1, n, seed=7))
        _check(case + " layers", _layers(res["layers"]), ref, "layers", C_F32)
        _check(case + " emb", res["emb"], ref, "emb", C_F32)
