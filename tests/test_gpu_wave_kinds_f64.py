"""GPU: every path against float64 on degenerate and product-like waveforms (tests/wave_kinds.py: silence, a constant, a DC offset,
a faint signal, an impulse, a square wave, full-scale noise, int16-quantised, hard-clipped, noise at -20 dB SNR, half-silent).

Every other float64-held file feeds the network ``0.1 * randn``: zero-mean and white, where a wrong ``L0``, a chunk slot that was
never written, a statistic shared between clips or an fp32 cancellation in the GroupNorm statistics (frontend.hip.h), in the conv0 +
GroupNorm backward (backward.hip.h) or in the parameter gradients that read the same folds (train.hip.h) makes an error below the
bounds, or none.  tests/test_wave_kinds_host.py shows on the CPU that the references are usable on these inputs.

Method: tests/ref64.py, ``err_gpu <= c * e32 + FLOOR * top`` with the oracle in float64 and in fp32, the constants imported from
tests/test_gpu_forward_f64.py (C_F32 = ref64.C = 8, C_X3P = 80, C_X3S = 90, C_BF16 = 50 000), none enlarged.  Every call runs inside
``guard.guarded()``, on workspaces filled with 0xFF bytes first (the statistics chunk slots behind a clip's own chunks are never
written: a short clip beside a long one, or any clip above 8192 frames, whose batch keeps eight slots per clip).

ONE RULE for every case: the kinds run as ONE batch and each clip is checked on its own, with its own ``top`` - max |d loss / d wav|
spans 6e-7 (noisy_m20db) to 1.5e-2 (silence) because rstd amplifies the quiet clips, and a batch-wide floor would hide a 1e-3 relative
error on the loud ones.  A case collects every clip that misses before it fails.

Cases: the forward of the uniform batch at N_SHORT (T = 65, L0 = 4175: five statistics chunks) through ``embed`` with every stage
tapped, ``embed`` with bf16x3 products, ``embed_bf16x3``, ``embed_bf16`` and ``embed_train``; at N_LONG (L0 = 8193: the 8192-frame
chunk fold with a one-frame second chunk) for dc_offset, constant and half_silent; ragged (every kind its own length, T = 1 .. 65) in
fp32 / bf16 / bf16x3; the loss path's d loss / d wav, uniform and ragged, feature_grad_mult 0.1 and 1.0, fp32 and bf16x3 products,
and at N_LONG for dc_offset (129 chunks of the GroupNorm backward's fp32 sums); the triplet step's parameter gradients with the conv
feature extractor trainable; windowed embeddings and their backward over silence; cdist and its backward of the batch against itself.

Bitwise batch invariance is asserted for the entry points for which an existing test already states it: ``embed``
(test_gpu_parity.py::test_batch_invariance_is_bit_exact), ``embed_bf16`` (test_gpu_bf16.py), ``embed_bf16x3``
(test_gpu_bf16x3.py::test_embed_bf16x3_batch_invariance_and_repeat) - every row equals its own B = 1 call, so no statistic leaks
between a silent clip and a loud neighbour - and ``embed_ragged`` in all three precisions against the same B = 1 calls.

Parameter gradients sum over clips, so the clips with rstd = 1 / sqrt(eps) would drown the rest: two steps, a quiet group (silence,
constant, dc_offset, faint, impulse) and a loud one (the others).  Anchors are the kinds, positives the kinds plus 1e-3 randn,
negatives the kinds rotated by one.  With margin 1.0 every hinge is active and at least 0.48 away from its switch point in float64
(tests/test_wave_kinds_host.py asserts 1e-3, as does the case itself), so the margin of test_gpu_train_f64.py is kept.

Worst err_gpu / e32 per path and kind, measured on one MI355X (``check`` prints every figure), 2026-10-20, on the kernels of commit
ec30425 (this change adds tests only).  Rows: the worst tensor of the path; columns: the kind (const = constant, dc_off = dc_offset,
full_sc = full_scale, clipped = hard_clipped, noisy = noisy_m20db, half_s = half_silent); the loss-path rows take the larger of
feature_grad_mult 0.1 and 1.0; "long" is N_LONG; c is the constant the path is held to.

  path                                  silence   const  dc_off   faint impulse  square full_sc   int16 clipped   noisy  half_s     c
  embed[fp32] conv0                        3.93    3.97    1.00    1.59    0.36    1.00    0.62    0.78    0.65    0.76    0.66     8
  embed[fp32] conv1-6, proj                5.65    4.17    1.10    7.33    4.51    5.65    6.82    6.60    6.60    6.01    5.68     8
  embed[fp32] layers                       3.93    3.20    1.31    3.51    3.95    4.67    4.62    4.01    3.75    4.52    4.11     8
  embed[fp32] emb                          4.00    2.53    0.93    1.12    5.30    2.71    2.14    1.69    1.76    1.58    3.58     8
  embed-x3-products emb                   27.26    2.60    0.95   24.22   32.45   20.38   31.26   29.61   29.78   28.79   23.06    80
  embed-x3-products layers                40.42    3.13    1.41   26.16   29.81   26.32   25.42   30.72   22.40   28.66   30.03    80
  embed_bf16x3 emb                        24.61    2.52    0.96   24.48   35.66   16.92   35.03   27.82   27.72   30.59   24.07    90
  embed_bf16x3 layers                     42.56    3.18    1.39   32.21   34.02   31.37   36.81   38.32   36.50   35.12   37.87    90
  embed_bf16 emb                          20415  230.55  247.41   21124   23142   11779   22925   16839   17154   21783   19853 50000
  embed_train emb                          3.92    2.53    0.93    1.12    5.12    2.63    1.80    1.69    1.76    1.50    3.58     8
  embed_train layers                       3.93    3.20    1.31    3.51    3.95    4.67    4.62    4.01    3.75    4.52    4.11     8
  embed_train-x3-products emb             27.26    2.60    0.95   24.22   32.45   20.38   31.26   29.61   29.78   28.79   23.06    80
  embed_train-x3-products layers          40.42    3.13    1.41   26.16   29.81   26.32   25.42   30.72   22.40   28.66   30.03    80
  long embed conv0                            -    3.97    0.92       -       -       -       -       -       -       -    0.81     8
  long embed emb                              -    2.85    0.98       -       -       -       -       -       -       -    2.19     8
  long embed layers                           -    3.26    1.04       -       -       -       -       -       -       -    4.57     8
  long embed_bf16x3 emb                       -    2.82    1.09       -       -       -       -       -       -       -   21.74    90
  long embed_bf16x3 layers                    -    3.22    1.45       -       -       -       -       -       -       -   31.97    90
  embed_ragged[fp32]                       1.41    2.71    0.67    1.43    3.01    3.03    1.66    1.99    2.15    2.30    2.65     8
  embed_ragged[bf16]                       8676  305.15  184.31   26536   19945   17678   15522   20482   14435   21787   22818 50000
  embed_ragged[bf16x3]                    11.50    2.76    0.73   22.90   33.48   19.25   24.95   35.64   21.41   25.47   33.30    90
  fp32 loss path short                     1.16    2.78    1.24    0.96    1.24    1.38    2.07    2.04    2.07    2.46    1.16     8
  x3 loss path short                       9.35    2.60    1.31    7.74    9.82   11.42   13.79   12.86   13.99   13.59   10.32    80
  fp32 loss path ragged                    1.14    2.36    1.04    2.08    1.69    2.08    2.25    2.69    2.20    2.43    1.41     8
  x3 loss path ragged                      8.56    2.55    1.07   12.19   14.65   14.70   15.92   14.32   13.94   13.84    8.92    80
  fp32 loss path long                         -       -    0.91       -       -       -       -       -       -       -       -     8
  windows embed_windows                    3.04       -       -       -       -       -       -       -       -       -    3.60     8
  windows embed_train_windows              2.94       -       -       -       -       -       -       -       -       -    3.12     8
  windows gradient                         1.06       -       -       -       -       -       -       -       -       -    0.87     8
  windows embed_windows, windows 5-7          -       -       -       -       -       -       -       -       -       -    3.60     8

  train convnet quiet conv0 + GroupNorm: 2.95 (feature_extractor.conv_layers.0.2.bias), 0.37 of the bound
  train convnet quiet: 3.44 (encoder.layer_norm.weight), 0.43 of the bound
  train convnet loud conv0 + GroupNorm: 3.92 (feature_extractor.conv_layers.0.2.bias), 0.49 of the bound
  train convnet loud: 6.81 (encoder.layers.4.self_attn_layer_norm.weight), 0.83 of the bound

The largest share of a bound is 0.88 (fp32, faint, conv1: 7.33 e32); bf16x3 stays below 0.51 of its bound and bf16 below 0.54.  Where
fp32 arithmetic cancels the yardstick grows by itself (constant and dc_offset: e32 of the last layer 2.8e-4 and 2.6e-4 against 5e-6 for
the other kinds), so the bf16x3 and bf16 ratios there are small.  No e32_min was needed for any kind.

That the cases bite was checked with four temporary edits of the kernels (never committed), each run under this file: (a) gn_fold_kernel
forming mean and var from s1, s2 cast to float - 18 of the 24 cases fail (every forward but bf16, every loss path, the quiet parameter
gradients); (b) conv0_bwd_kernel without its ``yhat * q[15]`` term - 11 fail (every loss path, the windows); (c) gn_bwd_fold_kernel's
ragged branch dividing by the batch's longest L0 - the 4 ragged loss-path cases fail; (d) wav_stats_fold_kernel looping to nchunk_max -
10 fail (N_LONG, the ragged forwards and loss paths).
"""
import contextlib

import numpy as np
import pytest
import torch

import guard
import ref64
import wave_kinds as K
from nomad_amd.weights import num_frames, num_windows
from oracle import nomad_oracle as O
from test_gpu_backward_f64 import grad_mult  # noqa: F401  (the fixture)
from test_gpu_cdist_backward import _Ref, _within
from test_gpu_forward_f64 import C_BF16, C_F32, C_X3P, C_X3S, _engine
from test_gpu_train_f64 import MARGIN, _step_separate

pytestmark = pytest.mark.gpu

WIN, HOP = 8, 8      # T = 65: windows over frames 0-7, 8-15, .. 56-63; half_silent's last three lie wholly in its silent half


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
class _Checks:
    """ref64.check per clip, every miss collected; ``done`` fails the case with all of them."""

    def __init__(self):
        self.bad = []

    def __call__(self, case, got, r64, r32, c=ref64.C, e32_min=None):
        try:
            ref64.check(case, got, r64, r32, e32_min, c)
        except AssertionError as e:
            self.bad.append(str(e))

    def done(self):
        assert not self.bad, f"{len(self.bad)} checks missed their bound:\n" + "\n".join(self.bad)


def _clip(x, i):
    """Clip i of a (B, ...) tensor or of a dict of them."""
    return {k: v[i] for k, v in x.items()} if isinstance(x, dict) else x[i]


def _layers(layers):
    return {str(l): layers[l].cpu() for l in range(12)}


@contextlib.contextmanager
def _guarded(case):
    """guard.guarded() with every workspace block starting as 0xFF bytes (NaN), so a slot read that was never written shows."""
    with guard.guarded(case=case):
        from nomad_amd.engine import Engine
        inner = Engine._workspace

        def _workspace(self, nbytes, side=False):
            ws = inner(self, nbytes, side)
            ws.fill_(0xFF)
            return ws
        Engine._workspace = _workspace
        try:
            yield
        finally:
            Engine._workspace = inner


@pytest.fixture(scope="module")
def x3(built_lib, sd0):
    """bf16x3 products on fp32 buffers."""
    eng = _engine(sd0, True)
    yield eng
    torch.cuda.synchronize()
    eng.close()


# ---- oracles: once per (batch, dtype), never changed ------------------------------------------------------------------------
_SD, _FWD, _LOSS = {}, {}, {}


def _sd(sd0, dt):
    if dt not in _SD:
        _SD[dt] = ref64.cast(sd0, dt)
    return _SD[dt]


def _forward_oracle(sd0, key, wav, taps=False):
    """{64 | 32: {"layers": {l: (B,T,768)}, "emb": (B,256), and with taps "conv0" .. "conv6", "proj"}} of a (B, n) batch."""
    if key not in _FWD:
        out = {}
        for bits, dt in ((64, torch.float64), (32, torch.float32)):
            sd = _sd(sd0, dt)
            t = {} if taps else None
            with torch.no_grad():
                x, layers = O.backbone(sd, wav.to(dt), t)
                r = {"layers": {str(l): y for l, y in enumerate(layers)},
                     "emb": O.head(x, sd["embedding_layer.1.weight"], sd["embedding_layer.1.bias"])}
            if taps:
                r.update({k: v for k, v in t.items() if k.startswith("conv") or k == "proj"})
            out[bits] = r
        _FWD[key] = out
    return _FWD[key]


def _ragged_oracle(sd0):
    """The ragged clips, each through the oracle at its own length: {64 | 32: {"emb": (B,256)}}."""
    if "ragged" not in _FWD:
        names, clips = K.ragged()
        per = [_forward_oracle(sd0, ("ragged", i), w[None]) for i, w in enumerate(clips)]
        _FWD["ragged"] = {bits: {"emb": torch.cat([r[bits]["emb"] for r in per])} for bits in (64, 32)}
    return _FWD["ragged"]


@pytest.fixture(scope="module")
def short(sd0):
    names, wav = K.batch(K.N_SHORT)
    yield names, wav, _forward_oracle(sd0, "short", wav, taps=True)
    for cache in (_SD, _FWD, _LOSS):
        cache.clear()


# ---- forward, uniform batch at N_SHORT --------------------------------------------------------------------------------------
def _rows_equal_their_own_call(names, wav, emb, fn, what):
    for i, name in enumerate(names):
        one = fn(wav[i:i + 1].contiguous())
        assert torch.equal(one[0], emb[i]), f"{what}: {name} in the batch differs from its own B = 1 call by {(one[0] - emb[i]).abs().max().item():.3e}"


def test_embed_every_stage(engine, short):
    """fp32: conv0 .. conv6 and the projection (diag_keep_intermediates), the 12 layers, the embedding; batch invariance."""
    names, wav, ref = short
    B, n, T = wav.shape[0], wav.shape[1], num_frames(wav.shape[1])
    w = wav.cuda()
    engine.diag_keep_intermediates(True)
    try:
        with _guarded("kinds embed stages"):
            emb = engine.embed(w)
            torch.cuda.synchronize()
            got = {f"conv{i}": engine.diag_region(B, n, f"conv{i}").cpu().view(B, -1, 512) for i in range(7)}
            xg = engine.diag_region(B, n, "xpad").cpu().view(16, B, T + 128, 48)
    finally:
        engine.diag_keep_intermediates(False)
    got["proj"] = xg[:, :, 64:64 + T].permute(1, 2, 0, 3).reshape(B, T, 768)
    assert xg[:, :, :64].abs().max().item() == 0.0 and xg[:, :, 64 + T:].abs().max().item() == 0.0, "xpad pad frames"
    with _guarded("kinds embed layers"):
        emb_l, layers = engine.embed(w, want_layers=True)
        _rows_equal_their_own_call(names, w, emb, engine.embed, "embed")
        torch.cuda.synchronize()
    assert torch.isfinite(emb).all() and torch.isfinite(layers).all()
    chk = _Checks()
    for i, name in enumerate(names):
        for stage in [f"conv{j}" for j in range(7)] + ["proj"]:
            chk(f"kinds embed[fp32] {name} {stage}", got[stage][i], ref[64][stage][i], ref[32][stage][i], C_F32)
        chk(f"kinds embed[fp32] {name} layers", _clip(_layers(layers), i), _clip(ref[64]["layers"], i), _clip(ref[32]["layers"], i), C_F32)
        chk(f"kinds embed[fp32] {name} emb", emb[i].cpu(), ref[64]["emb"][i], ref[32]["emb"][i], C_F32)
        chk(f"kinds embed[fp32] {name} layers emb", emb_l[i].cpu(), ref[64]["emb"][i], ref[32]["emb"][i], C_F32)
    chk.done()


@pytest.mark.parametrize("entry", ["embed-x3-products", "embed_bf16x3", "embed_bf16", "embed_train", "embed_train-x3-products"])
def test_forward_entry_points(engine, x3, short, entry):
    names, wav, ref = short
    w = wav.cuda()
    layers = None
    with _guarded(f"kinds {entry}"):
        if entry == "embed-x3-products":
            c = C_X3P
            emb, layers = x3.embed(w, want_layers=True)
        elif entry == "embed_bf16x3":
            c = C_X3S
            emb = engine.embed_bf16x3(w)
            emb_l, layers = engine.embed_bf16x3(w, want_layers=True)
            _rows_equal_their_own_call(names, w, emb, engine.embed_bf16x3, entry)
        elif entry == "embed_bf16":
            c = C_BF16
            emb = engine.embed_bf16(w)
            _rows_equal_their_own_call(names, w, emb, engine.embed_bf16, entry)
        else:
            eng, c = (x3, C_X3P) if entry.endswith("x3-products") else (engine, C_F32)
            emb, layers, _saved = eng.embed_train(w)
        torch.cuda.synchronize()
    assert torch.isfinite(emb).all()
    chk = _Checks()
    for i, name in enumerate(names):
        chk(f"kinds {entry} {name} emb", emb[i].cpu(), ref[64]["emb"][i], ref[32]["emb"][i], c)
        if layers is not None:
            chk(f"kinds {entry} {name} layers", _clip(_layers(layers), i), _clip(ref[64]["layers"], i), _clip(ref[32]["layers"], i), c)
        if entry == "embed_bf16x3":
            chk(f"kinds {entry} {name} layers emb", emb_l[i].cpu(), ref[64]["emb"][i], ref[32]["emb"][i], c)
    chk.done()


# ---- forward at N_LONG ------------------------------------------------------------------------------------------------------
def test_forward_across_the_8192_frame_statistics_chunk(engine, sd0):
    """L0 = 8193: the clip's 65 waveform sums are taken in chunks of 8192 frames, the second of ONE frame (a shorter clip takes
    chunks of 1024).  conv0 is tapped: it is the stage the statistics enter."""
    names, wav = K.batch(K.N_LONG, K.LONG_KINDS)
    ref = _forward_oracle(sd0, "long", wav, taps=True)
    B, n = wav.shape
    w = wav.cuda()
    engine.diag_keep_intermediates(True)
    try:
        with _guarded("kinds long embed"):
            emb = engine.embed(w)
            torch.cuda.synchronize()
            conv0 = engine.diag_region(B, n, "conv0").cpu().view(B, -1, 512)
    finally:
        engine.diag_keep_intermediates(False)
    with _guarded("kinds long layers, bf16x3"):
        emb_l, layers = engine.embed(w, want_layers=True)
        emb3 = engine.embed_bf16x3(w)
        emb3_l, layers3 = engine.embed_bf16x3(w, want_layers=True)
        torch.cuda.synchronize()
    assert conv0.shape[1] == 8193
    chk = _Checks()
    for i, name in enumerate(names):
        case = f"kinds long {name}"
        chk(case + " embed conv0", conv0[i], ref[64]["conv0"][i], ref[32]["conv0"][i], C_F32)
        chk(case + " embed emb", emb[i].cpu(), ref[64]["emb"][i], ref[32]["emb"][i], C_F32)
        chk(case + " embed layers", _clip(_layers(layers), i), _clip(ref[64]["layers"], i), _clip(ref[32]["layers"], i), C_F32)
        chk(case + " embed layers emb", emb_l[i].cpu(), ref[64]["emb"][i], ref[32]["emb"][i], C_F32)
        chk(case + " embed_bf16x3 emb", emb3[i].cpu(), ref[64]["emb"][i], ref[32]["emb"][i], C_X3S)
        chk(case + " embed_bf16x3 layers", _clip(_layers(layers3), i), _clip(ref[64]["layers"], i), _clip(ref[32]["layers"], i), C_X3S)
        chk(case + " embed_bf16x3 layers emb", emb3_l[i].cpu(), ref[64]["emb"][i], ref[32]["emb"][i], C_X3S)
    chk.done()


# ---- forward, ragged ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_embed_ragged(engine, sd0, precision):
    """Every kind at its own length (400 samples, T = 1, for silence .. N_SHORT) in one launch sequence, on a workspace of NaN:
    each clip against the oracle at its own length, and bit for bit its own B = 1 call."""
    names, clips = K.ragged()
    ref = _ragged_oracle(sd0)
    own = {"fp32": engine.embed, "bf16": engine.embed_bf16, "bf16x3": engine.embed_bf16x3}[precision]
    c = {"fp32": C_F32, "bf16": C_BF16, "bf16x3": C_X3S}[precision]
    with _guarded(f"kinds embed_ragged[{precision}]"):
        emb = engine.embed_ragged([w.cuda() for w in clips], precision=precision)
        torch.cuda.synchronize()
    with _guarded(f"kinds embed_ragged[{precision}] own calls"):
        ones = torch.cat([own(w[None].cuda()) for w in clips])
        torch.cuda.synchronize()
    assert torch.isfinite(emb).all()
    chk = _Checks()
    for i, name in enumerate(names):
        chk(f"kinds embed_ragged[{precision}] {name} n={clips[i].numel()}", emb[i].cpu(), ref[64]["emb"][i], ref[32]["emb"][i], c)
        assert torch.equal(emb[i], ones[i]), f"{name}: the ragged batch differs from its own call by {(emb[i] - ones[i]).abs().max().item():.3e}"
    chk.done()


# ---- the loss path: d loss / d wav -------------------------------------------------------------------------------------------
def _rows(clips):
    return np.concatenate([[0], np.cumsum([num_frames(c.numel()) for c in clips])]).tolist()


def _loss_setup(sd0, key, clips, mult):
    """Head (its ``head_relu_undecided`` columns zeroed), upstreams and the float64 / fp32 d <outputs, G> / d clip of every clip
    at its own length, as test_gpu_backward_f64._loss_path_case builds them; clips of one length run as one oracle batch."""
    key = (key, mult)
    if key in _LOSS:
        return _LOSS[key]
    B, r = len(clips), _rows(clips)
    M = r[-1]
    gen = torch.Generator().manual_seed(K.SEED + B)
    hw = (torch.rand(256, 768, generator=gen) * 2 - 1) / 768 ** 0.5
    hb = (torch.rand(256, generator=gen) * 2 - 1) / 768 ** 0.5
    uniform = len({c.numel() for c in clips}) == 1
    if uniform:
        undecided = ref64.head_relu_undecided(sd0, torch.stack(clips))
    else:
        undecided = torch.zeros(768, dtype=torch.bool)
        for w in clips:
            undecided |= ref64.head_relu_undecided(sd0, w[None])
    assert int(undecided.sum()) <= 64, int(undecided.sum())
    hw[:, undecided] = 0.0
    Gl = torch.randn(12, M, 768, generator=gen) / (M * 768)            # packed rows: clip c's frames at r[c] .. r[c + 1]
    Ge = torch.randn(B, 256, generator=gen) / (B * 256)
    if uniform:
        T = M // B
        r64, r32 = ref64.both(ref64.lossnet_dwav, sd0, torch.stack(clips), hw, hb, Gl.view(12, B, T, 768), Ge, feature_grad_mult=mult)
        r64, r32 = list(r64), list(r32)
    else:
        per = [ref64.both(ref64.lossnet_dwav, sd0, w[None], hw, hb, Gl[:, r[i]:r[i + 1]][:, None], Ge[i:i + 1], feature_grad_mult=mult)
               for i, w in enumerate(clips)]
        r64, r32 = [p[0][0] for p in per], [p[1][0] for p in per]
    _LOSS[key] = (hw, hb, Gl, Ge, r64, r32)
    return _LOSS[key]


def _loss_case(eng, sd0, key, names, clips, mult, c, ragged, tag):
    hw, hb, Gl, Ge, r64, r32 = _loss_setup(sd0, key, clips, mult)
    B = len(clips)
    head = (hw.cuda(), hb.cuda())
    old = eng.feature_grad_mult
    eng.feature_grad_mult = mult
    try:
        with _guarded(f"kinds {tag} loss path {key} fgm={mult:g}"):
            if ragged:
                emb, layers, saved, batch = eng.embed_train_ragged([w.cuda() for w in clips], head=head)
                dwav = eng.embed_backward_ragged(batch, layers, saved, Gl.cuda(), Ge.cuda(), head)
            else:
                wav = torch.stack(clips).cuda()
                emb, layers, saved = eng.embed_train(wav, head)
                dwav = eng.embed_backward(wav, layers, saved, Gl.view(12, B, -1, 768).cuda(), Ge.cuda(), head)
            torch.cuda.synchronize()
    finally:
        eng.feature_grad_mult = old
    assert torch.isfinite(dwav).all()
    dwav = dwav.cpu()
    chk = _Checks()
    for i, name in enumerate(names):
        n = clips[i].numel()
        chk(f"kinds {tag} loss path {key} {name} n={n} fgm={mult:g}", dwav[i, :n], r64[i], r32[i], c)
        assert not dwav[i, n:].any(), f"{name}: a gradient behind the clip's length"
        unused = r64[i] == 0                                   # samples no frame depends on: exactly zero in float64, and on the GPU
        assert not dwav[i, :n][unused].any(), f"{name}: {int((dwav[i, :n][unused] != 0).sum())} unused samples with a gradient"
    chk.done()


def _engine_of(products, engine, x3):
    return (engine, ref64.C, "fp32") if products == "fp32" else (x3, C_X3P, "x3")


@pytest.mark.parametrize("products", ["fp32", "x3"])
@pytest.mark.parametrize("mult", [0.1, 1.0])
def test_loss_path_uniform(engine, x3, sd0, grad_mult, mult, products):
    eng, c, tag = _engine_of(products, engine, x3)
    names, wav = K.batch(K.N_SHORT)
    _loss_case(eng, sd0, "short", names, list(wav), mult, c, False, tag)


@pytest.mark.parametrize("products", ["fp32", "x3"])
@pytest.mark.parametrize("mult", [0.1, 1.0])
def test_loss_path_ragged(engine, x3, sd0, grad_mult, mult, products):
    """Each clip's a1 / L0, a2 / L0 take the clip's own L0, and its fold its own chunks (the slots behind them hold NaN here)."""
    eng, c, tag = _engine_of(products, engine, x3)
    names, clips = K.ragged()
    _loss_case(eng, sd0, "ragged", names, clips, mult, c, True, tag)


@pytest.mark.parametrize("mult", [0.1, 1.0])
def test_loss_path_across_129_chunks_of_fp32_sums(engine, sd0, grad_mult, mult):
    """dc_offset at N_LONG: s1, s2 of the GroupNorm backward are fp32 sums over 129 chunks of 64 frames, the last of one frame."""
    names, wav = K.batch(K.N_LONG, ["dc_offset"])
    _loss_case(engine, sd0, "long", names, list(wav), mult, ref64.C, False, "fp32")


# ---- parameter gradients -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd_train():
    from nomad_amd.weights import seeded_state_dict
    return seeded_state_dict(3, qk_gain=3.0)


@pytest.fixture(scope="module")
def teng(built_lib, sd_train):
    from nomad_amd.engine import Engine
    eng = Engine({k: v.clone() for k, v in sd_train.items()}, 0)
    eng.train_enable()
    yield eng
    eng.close()


@pytest.mark.parametrize("group", ["quiet", "loud"])
def test_parameter_gradients_with_the_convnet_trainable(teng, sd_train, group):
    """The triplet step of test_gpu_train_f64.py (three calls, freeze_convnet False, feature_grad_mult 0.1): the GroupNorm gamma /
    beta and conv0 weight gradients read the folds of the degenerate clips."""
    names = K.QUIET if group == "quiet" else K.LOUD
    A, P, N = K.triplet_group(names)
    with torch.no_grad():
        ea, ep, en = (O.triplet_forward(ref64.cast(sd_train, torch.float64), w.double()) for w in (A, P, N))
    pd = torch.nn.functional.pairwise_distance
    hinge = pd(ea, ep) - pd(ea, en) + MARGIN
    assert hinge.abs().min().item() >= 1e-3 and (hinge > 0).any(), hinge.tolist()       # no hinge at its switch point
    (loss64, g64), (loss32, g32) = ref64.both(ref64.triplet_grads, sd_train, A, P, N, MARGIN, freeze_convnet=False, feature_grad_mult=0.1)
    old = teng.feature_grad_mult
    teng.train_set_convnet(True)
    teng.feature_grad_mult = 0.1
    try:
        with _guarded(f"kinds train {group}"):
            loss, got = _step_separate(teng, A, P, N)
            torch.cuda.synchronize()
    finally:
        teng.train_set_convnet(False)
        teng.feature_grad_mult = old
    assert loss64.item() > 0 and all(torch.isfinite(v).all() for v in got.values())
    conv0 = [k for k in g64 if "feature_extractor.conv_layers.0." in k]
    assert len(conv0) == 3 and all(g64[k].abs().max() > 0 for k in conv0)
    assert abs(loss - loss64.item()) <= ref64.C * abs(loss32.item() - loss64.item()) + 1e-6, (loss, loss64.item(), loss32.item())
    ref64.check(f"kinds train convnet {group} conv0 + GroupNorm", {k: got[k] for k in conv0}, {k: g64[k] for k in conv0},
                {k: g32[k] for k in conv0})
    ref64.check(f"kinds train convnet {group}", {k: got[k] for k in g64}, g64, g32)


# ---- windows -----------------------------------------------------------------------------------------------------------------
def _windows_oracle(sd, clips, hw, hb, demb, mult, dt):
    """-> (window embeddings (W_total, 256), [d <emb_w, demb> / d clip]) in ``dt``: O.backbone at each clip's length, O.head on
    every window's rows (the float64 reference of test_gpu_windows.py / test_gpu_windows_loss.py)."""
    embs, grads, at = [], [], 0
    for w in clips:
        w = w[None].to(dt).requires_grad_(True)
        x, _ = O.backbone(sd, w, feature_grad_mult=mult, required_seq_len_multiple=2)
        T = x.shape[1]
        n = min(WIN, T)
        e = torch.cat([O.head(x[:, k * HOP:k * HOP + n], hw.to(dt), hb.to(dt)) for k in range(num_windows(T, WIN, HOP))])
        (g,) = torch.autograd.grad((e * demb[at:at + e.shape[0]].to(dt)).sum(), w)
        at += e.shape[0]
        embs.append(e.detach())
        grads.append(g[0])
    return torch.cat(embs), grads


def test_windows_over_silence(engine, sd0):
    """half_silent and silence as one batch, win 8 hop 8 at T = 65: half_silent's windows 5 .. 7 cover silent frames only (the
    frames of silence still differ from each other: the pos-conv sees its zero padding from the clip's ends).  ``embed_windows``, then
    ``embed_train_windows`` + ``embed_windows_backward``."""
    names = ["half_silent", "silence"]
    _, wav = K.batch(K.N_SHORT, names)
    clips = list(wav)
    assert not wav[0, 5 * HOP * 320:].any()                      # window 5 starts at sample 12800, behind n // 2 = 10440
    W = num_windows(65, WIN, HOP)
    gen = torch.Generator().manual_seed(K.SEED + 2)
    demb = torch.randn(2 * W, 256, generator=gen) / (2 * W * 256)
    sd64 = _sd(sd0, torch.float64)
    undecided = torch.zeros(768, dtype=torch.bool)
    with torch.no_grad():
        x64, _ = O.backbone(sd64, wav.double(), required_seq_len_multiple=2)
    for k in range(W):                                           # the head's ReLU kink, per window (test_gpu_windows_loss.py)
        undecided |= (x64[:, k * HOP:k * HOP + WIN].mean(1).abs() < ref64.KINK).any(0)
    assert int(undecided.sum()) <= 64, int(undecided.sum())
    hw, hb = sd0["embedding_layer.1.weight"].clone(), sd0["embedding_layer.1.bias"].clone()
    hw[:, undecided] = 0.0
    mult = engine.feature_grad_mult
    (e64, g64), (e32, g32) = (_windows_oracle(_sd(sd0, dt), clips, hw, hb, demb, mult, dt) for dt in (torch.float64, torch.float32))
    head = (hw.cuda(), hb.cuda())
    w = wav.cuda()
    with _guarded("kinds windows"):
        emb, counts = engine.embed_windows(w, WIN, HOP, head=head)
        emb_t, counts_t, layers, saved = engine.embed_train_windows(w, WIN, HOP, head)
        dwav = engine.embed_windows_backward(w, layers, saved, demb.cuda(), WIN, HOP, head)
        torch.cuda.synchronize()
    assert counts == counts_t == [W, W] and torch.isfinite(emb).all() and torch.isfinite(dwav).all()
    chk = _Checks()
    for i, name in enumerate(names):
        rows = slice(i * W, (i + 1) * W)
        chk(f"kinds windows {name} embed_windows", emb[rows].cpu(), e64[rows], e32[rows], C_F32)
        chk(f"kinds windows {name} embed_train_windows", emb_t[rows].cpu(), e64[rows], e32[rows], C_F32)
        chk(f"kinds windows {name} gradient", dwav[i].cpu(), g64[i], g32[i], ref64.C)
    chk(f"kinds windows half_silent, the silent windows", emb[5:W].cpu(), e64[5:W], e32[5:W], C_F32)
    chk.done()


# ---- scores on equal clips -----------------------------------------------------------------------------------------------------
def test_cdist_of_the_batch_against_itself(engine, short):
    names, wav, _ = short
    B = len(names)
    gen = torch.Generator().manual_seed(K.SEED + 3)
    g_dist = torch.randn(B, B, generator=gen, dtype=torch.float64)
    g_mean = torch.randn(B, generator=gen, dtype=torch.float64)
    with _guarded("kinds cdist"):
        emb = engine.embed(wav.cuda())
        other = emb.clone()
        dist, mean = engine.cdist(emb, other)
        da, db = engine.cdist_backward(emb, other, g_dist.cuda(), g_mean.cuda(), want_a=True, want_b=True)
        torch.cuda.synchronize()
    assert not dist.diagonal().any(), "a clip is not at distance 0 from itself"
    assert torch.isfinite(dist).all() and torch.isfinite(mean).all() and torch.isfinite(da).all() and torch.isfinite(db).all()
    ref = _Ref(emb.cpu(), emb.cpu())
    assert np.abs(dist.cpu().numpy() - ref.d).max() <= 1e-13 and np.abs(mean.cpu().numpy() - ref.d.mean(1)).max() <= 1e-13
    rda, rdb, row_slack, col_slack = ref.grads(g_dist, g_mean)
    _within("kinds cdist_backward da", da, rda, row_slack)
    _within("kinds cdist_backward db", db, rdb, col_slack)
