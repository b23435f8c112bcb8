"""GPU: the fp32 positional convolution in the frequency domain (nomad_amd/csrc/posconv_fft_f32.hip.h).

One group of the pos-conv is the 128-tap correlation C[t] = sum_k A[t + k] V[k] over the zero-padded frames of a clip.  The engine
runs it as overlap-save with 512-point transforms: units of 385 output frames, one 48 x 48 complex product per bin (tests/
test_posconv_fft_identity.py restates the algebra on the CPU).  The form is not exact on integers, so the layout tests hold it to
the float64 direct correlation within a quarter of the smallest change a misplaced frame, tap, channel or block can make.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_posconv_wino import _pad_group_major, _posconv_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "posconv_fft_switch_off.npz")


@pytest.fixture(scope="module")
def diag_posconv_fft(engine):
    from nomad_amd import _lib
    fn = engine.lib.nomad_diag_posconv_fft

    def run(xpad, w, bias, lens, ragged):
        rows = sum(lens)
        guard = 64   # rows behind the output that nothing may touch
        y = torch.full((rows + guard, 768), 1234.5, device="cuda")
        u = torch.full((rows + guard, 768), 1234.5, device="cuda")
        arr = (C.c_int * len(lens))(*lens)
        _lib.check(fn(engine.ctx, xpad.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), u.data_ptr(), len(lens), arr,
                      int(ragged), engine._stream()), "nomad_diag_posconv_fft")
        torch.cuda.synchronize()
        assert (y[rows:] == 1234.5).all() and (u[rows:] == 1234.5).all(), "stores beyond the last output row"
        return y[:rows].cpu(), u[:rows].cpu()

    return run


# below one frame pair, a short clip, the 4 s clip, exactly one unit, one frame into a second unit, one frame into a third;
# ragged: clips of one, two and three units next to clips of a few frames, a unit that is one frame short of full
CASES = [([T] * 2, False) for T in (1, 2, 63, 199, 385, 386, 771)]
CASES += [([199, 1, 386, 64, 770, 7], True)]


@pytest.mark.parametrize("lens,ragged", CASES)
def test_integer_layout(diag_posconv_fft, lens, ragged):
    """Operands as in test_gpu_posconv_wino.py::test_exact_integer_layout: integers |x| <= 3, |w| <= 2, sums of 6144 products below
    2^24.  A misplaced frame, tap, channel or block moves such a sum by at least 1; the form's own rounding error on them was at
    most 2.4e-4 on the first green run (7.6e-6 at T = 1, 1.5e-4 at T = 199, 2.4e-4 from T = 385 on and in the ragged batch) - below
    0.05, so the bound of 0.25 stays, a factor of 4 below the smallest misplacement."""
    gen = torch.Generator().manual_seed(sum(lens) + 17 * len(lens) + ragged)
    x = torch.randint(-3, 4, (sum(lens), 768), generator=gen).float()
    w = torch.zeros(16, 64, 6144)
    w[:, :48] = torch.randint(-2, 3, (16, 48, 6144), generator=gen).float()
    xpad = _pad_group_major(x, lens)
    y, u = diag_posconv_fft(xpad.cuda(), w.cuda(), torch.zeros(768, device="cuda"), lens, ragged)
    ref = _posconv_ref(xpad.double(), w.double(), lens)
    assert ref.abs().max().item() < 2 ** 24
    err = (u.double() - ref).abs().max().item()
    print("pos-conv in the frequency domain, integer operands", lens, ": max |u - ref| =", err)
    assert err <= 0.25, err
    want = x.double() + torch.nn.functional.gelu(u.double())   # the epilogue on the form's own pre-activation
    assert ((y.double() - want).abs() <= 1e-6 * want.abs().clamp(min=1.0)).all()


def _stage_errors(form, peaky):
    """Max |engine pos-conv - float64 pos-conv| of the pre-activation and of the stage's output, on the engine's own pos-conv
    input (2 clips of 9000 samples) and the model's folded fp32 weights, in a child process: form "direct" is the 128-tap GEMM
    (NOMAD_F32_POSCONV_WINO=0 is read when a context is created, by libnomad_diag.so), "fft" the frequency domain."""
    code = f"""
import ctypes as C, sys, torch
sys.path.insert(0, {ROOT!r})
sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
from nomad_amd import _lib
from nomad_amd.engine import Engine
from nomad_amd.weights import seeded_state_dict
from test_gpu_posconv_wino import _hook, _posconv_ref
sd = seeded_state_dict(1, qk_gain=6.0) if {peaky} else seeded_state_dict(0)
eng = Engine(sd, 0, diag=True)
gen = torch.Generator().manual_seed(7)
B, N = 2, 9000
wav = (0.1 * torch.randn(B, N, generator=gen)).clamp(-1, 1)
eng.embed(wav.cuda())
torch.cuda.synchronize()
xpad = eng.diag_region(B, N, "xpad").clone().view(16, -1, 48)
T = xpad.shape[1] // B - 128
v = sd["ssl_model.encoder.pos_conv.0.weight_v"].double()                     # [768][48][128]
g = sd["ssl_model.encoder.pos_conv.0.weight_g"].double().view(128)
wn = (v * (g / v.pow(2).sum(dim=(0, 1)).sqrt())).float()                     # weight_norm(dim=2), folded, in fp32 as the engine holds it
w = torch.zeros(16, 64, 6144)
w[:, :48] = wn.view(16, 48, 48, 128).permute(0, 1, 3, 2).reshape(16, 48, 6144)
bias = sd["ssl_model.encoder.pos_conv.0.bias"].float()
y = torch.empty(B * T, 768, device="cuda")
u = torch.empty(B * T, 768, device="cuda")
lens = (C.c_int * B)(*([T] * B))
fn = eng.lib.nomad_diag_posconv_fft if {form == "fft"} else _hook(eng)
_lib.check(fn(eng.ctx, xpad.data_ptr(), w.cuda().data_ptr(), bias.cuda().data_ptr(), y.data_ptr(), u.data_ptr(), B, lens, 0,
              eng._stream()), "pos-conv hook")
torch.cuda.synchronize()
xp = xpad.cpu().double()
ref_u = _posconv_ref(xp, w.double(), [T] * B) + bias.double()
x = torch.cat([xp[:, b * (T + 128) + 64:b * (T + 128) + 64 + T] for b in range(B)], dim=1).transpose(0, 1).reshape(B * T, 768)
ref_y = x + torch.nn.functional.gelu(ref_u)
print(repr((u.cpu().double() - ref_u).abs().max().item()), repr((y.cpu().double() - ref_y).abs().max().item()))
eng.close()
"""
    env = dict(os.environ, NOMAD_F32_POSCONV_WINO="0")
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return [float(v) for v in r.stdout.split()[-2:]]


@pytest.mark.parametrize("peaky", [False, True])
def test_accuracy_vs_direct_form(built_lib, peaky):
    """Below 2e-5 against float64, and no worse than the direct fp32 form (+ 1e-7)."""
    old = _stage_errors("direct", peaky)
    new = _stage_errors("fft", peaky)
    print("pos-conv stage, max error against float64 (pre-activation, output): direct", old, "frequency domain", new)
    for eo, en in zip(old, new):
        assert en < 2e-5, (eo, en)
        assert en <= eo + 1e-7, (eo, en)


def test_five_clip_batch_equals_single_clips(engine):
    gen = torch.Generator().manual_seed(11)
    wav = (0.1 * torch.randn(5, 9001, generator=gen)).clamp(-1, 1).cuda()
    batch = engine.embed(wav)
    for i in range(5):
        assert torch.equal(batch[i:i + 1], engine.embed(wav[i:i + 1])), i


def test_ragged_batch_equals_per_clip_calls(engine):
    from nomad_amd.weights import num_frames
    gen = torch.Generator().manual_seed(12)
    lens = [400, 9001, 400 + 385 * 320, 480000]   # one, two and four units; a clip of one frame
    assert [num_frames(n) for n in lens] == [1, 27, 386, 1499]
    waves = [(0.1 * torch.randn(n, generator=gen)).clamp(-1, 1) for n in lens]
    batch = engine.embed_ragged(waves)
    for i, w in enumerate(waves):
        assert torch.equal(batch[i:i + 1], engine.embed_ragged([w])), i


def test_transformed_weights_follow_a_training_step(built_lib):
    """After an optimiser step, embed() on the trained engine equals embed() on a fresh engine made from the updated weights, bit
    for bit: the pos-conv weights' spectrum was rebuilt together with the folded weights."""
    from nomad_amd.engine import Engine
    from nomad_amd.weights import seeded_state_dict
    sd = seeded_state_dict(3, qk_gain=3.0)
    eng = Engine({k: v.clone() for k, v in sd.items()}, 0)
    fresh = None
    try:
        eng.train_enable()
        g = torch.Generator().manual_seed(5)
        total, _ = eng.train_param_count()
        eng.train_write(1, (torch.randn(total, generator=g) * 1e-3).cuda())
        eng.adam_step(1e-3, 1e-2)   # large steps: stale derived weights would be obvious
        new_sd = eng.train_state_dict()
        moved = (new_sd["ssl_model.encoder.pos_conv.0.weight_v"] - sd["ssl_model.encoder.pos_conv.0.weight_v"]).abs().max().item()
        assert moved > 1e-4
        wav = (0.1 * torch.randn(2, 6000, generator=g)).clamp(-1, 1).cuda()
        have = eng.embed(wav).clone()
        fresh = Engine(new_sd, 0)
        want = fresh.embed(wav)
        torch.cuda.synchronize()
        assert torch.equal(have, want), (have - want).abs().max().item()
    finally:
        eng.close()
        if fresh is not None:
            fresh.close()


def test_switch_off_is_the_previous_forward(built_lib, sd0):
    """NOMAD_F32_POSCONV_FFT=0 (read when a context is created, by libnomad_diag.so): embed() gives the bits it gave before the form
    existed: tests/golden/posconv_fft_switch_off.npz holds them, written by the parent commit's embed() on the same input."""
    from nomad_amd.engine import Engine
    gen = torch.Generator().manual_seed(7)
    wav = (0.1 * torch.randn(2, 9000, generator=gen)).clamp(-1, 1).cuda()
    want = torch.from_numpy(np.load(GOLDEN)["emb"])
    old = os.environ.get("NOMAD_F32_POSCONV_FFT")
    os.environ["NOMAD_F32_POSCONV_FFT"] = "0"
    try:
        eng = Engine(sd0, 0, diag=True)
    finally:
        if old is None:
            del os.environ["NOMAD_F32_POSCONV_FFT"]
        else:
            os.environ["NOMAD_F32_POSCONV_FFT"] = old
    try:
        assert torch.equal(eng.embed(wav).cpu(), want)
    finally:
        eng.close()
