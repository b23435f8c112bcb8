"""GPU: conv1 .. conv4 in polyphase Winograd form (nomad_amd/csrc/conv_s2_f32.hip.h).

Per output pair s of a clip the kernel computes
    P = (w0 + w2) x[4s+2],  y[2s] = w0 (x[4s] - x[4s+2]) + w1 x[4s+1] + P,  y[2s+1] = w2 (x[4s+4] - x[4s+2]) + w1 x[4s+3] + P
(GELU after).  The layout tests use small-integer operands, where every fp32 sum is exact, so the kernel must match the float64
direct convolution bit for bit: any wrong row, column, tap, channel chunk, clip boundary or pair parity shows.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conv_ref(x, w, lins):
    """float64 direct conv (k = 3, stride 2) per clip: x [sum lin][512], w [512][1536] ([out][tap*512 + in])."""
    outs, o = [], 0
    w3 = w.view(512, 3, 512)
    for lin in lins:
        L = (lin - 3) // 2 + 1
        xc = x[o:o + lin]
        cols = torch.stack([xc[2 * t:2 * t + 3].reshape(-1) for t in range(L)])   # [L][3*512], tap-major
        outs.append(cols @ w3.reshape(512, -1).T)
        o += lin
    return torch.cat(outs)


@pytest.fixture(scope="module")
def diag_conv(built_lib):
    from nomad_amd import _lib
    from nomad_amd.engine import Engine
    from nomad_amd.weights import seeded_state_dict
    eng = Engine(seeded_state_dict(0), 0, diag=True)
    fn = eng.lib.nomad_diag_conv_s2
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_void_p]

    def run(x, w, lins, ragged):
        Ls = [(l - 3) // 2 + 1 for l in lins]
        rows = sum(Ls)
        guard = 64   # rows behind the output that nothing may touch
        y = torch.full((rows + guard, 512), 1234.5, device="cuda")
        u = torch.full((rows + guard, 512), 1234.5, device="cuda")
        arr = (C.c_int * len(lins))(*lins)
        _lib.check(fn(eng.ctx, x.data_ptr(), w.data_ptr(), y.data_ptr(), u.data_ptr(), len(lins), arr, int(ragged),
                      eng._stream()), "nomad_diag_conv_s2")
        torch.cuda.synchronize()
        assert (y[rows:] == 1234.5).all() and (u[rows:] == 1234.5).all(), "stores beyond the last output row"
        return y[:rows].cpu(), u[:rows].cpu()

    yield run
    eng.close()


CASES = [
    ([603, 603, 603], False),          # L = 301 (odd): the last pair has no odd output; 151 pairs per clip, partial last tile
    ([604, 604], False),               # L = 301 with the longer input (lin = 2L + 2)
    ([600] * 4, False),                # L = 299
    ([5] * 5, False),                  # L = 2: one pair per clip
    ([3] * 7, False),                  # L = 1: one pair per clip, no odd output at all
    ([1601, 1601], False),             # conv4-shaped at a 4 s clip: L = 800, 400 pairs
    ([6401], False),                   # conv1-shaped single clip: L = 3200
    ([603, 4, 3, 900, 257, 1000, 6], True),   # ragged: clip boundaries inside tiles, L = 1 / 2 / odd / even
    ([1601, 1601], True),              # ragged launch of a uniform batch
]


@pytest.mark.parametrize("lins,ragged", CASES)
def test_exact_integer_layout(diag_conv, lins, ragged):
    gen = torch.Generator().manual_seed(sum(lins) + ragged)
    x = torch.randint(-3, 4, (sum(lins), 512), generator=gen).float()
    w = torch.randint(-2, 3, (512, 1536), generator=gen).float()
    y, u = diag_conv(x.cuda(), w.cuda(), lins, ragged)
    ref = _conv_ref(x.double(), w.double(), lins)
    assert ref.abs().max().item() < 2 ** 24   # every partial sum is exact in fp32
    assert torch.equal(u.double(), ref), (u.double() - ref).abs().max().item()
    g = torch.nn.functional.gelu(ref)
    assert ((y.double() - g).abs() <= 1e-6 * g.abs().clamp(min=1.0)).all()


def _layer_errors(wino, peaky):
    """Max |engine conv_i - float64 conv_i(engine conv_{i-1})| for i = 1 .. 4, in a child process (the switch is read when a
    context is created, by libnomad_diag.so)."""
    code = f"""
import torch, sys
sys.path.insert(0, {ROOT!r})
from nomad_amd.engine import Engine
from nomad_amd.weights import seeded_state_dict
sd = seeded_state_dict(1, qk_gain=6.0) if {peaky} else seeded_state_dict(0)
eng = Engine(sd, 0, diag=True)
gen = torch.Generator().manual_seed(7)
B, N = 2, 9000
wav = (0.1 * torch.randn(B, N, generator=gen)).clamp(-1, 1)
eng.diag_keep_intermediates(True)
eng.embed(wav.cuda())
torch.cuda.synchronize()
errs = []
for i in range(1, 5):
    w = sd[f"ssl_model.feature_extractor.conv_layers.{{i}}.0.weight"].double()        # [out][in][k]
    xin = eng.diag_region(B, N, f"conv{{i-1}}").cpu().view(B, -1, 512).double()
    got = eng.diag_region(B, N, f"conv{{i}}").cpu().view(B, -1, 512).double()
    ref = torch.nn.functional.gelu(torch.nn.functional.conv1d(xin.transpose(1, 2), w, stride=2)).transpose(1, 2)
    errs.append((got - ref).abs().max().item())
print(" ".join(repr(e) for e in errs))
eng.close()
"""
    env = dict(os.environ, NOMAD_F32_CONV_WINO=str(int(wino)))
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return [float(v) for v in r.stdout.split()[-4:]]


@pytest.mark.parametrize("peaky", [False, True])
def test_accuracy_vs_direct_form(built_lib, peaky):
    old = _layer_errors(False, peaky)
    new = _layer_errors(True, peaky)
    for i, (eo, en) in enumerate(zip(old, new), start=1):
        assert en < 2e-5 and eo < 2e-5, (i, eo, en)
        assert en <= 2 * eo + 1e-7, (i, eo, en)


def test_full_bench_batch_is_bit_identical_across_calls(engine):
    gen = torch.Generator().manual_seed(3)
    wav = (0.1 * torch.randn(256, 64000, generator=gen)).clamp(-1, 1).cuda()
    a = engine.embed(wav).clone()
    b = engine.embed(wav)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_five_clip_batch_equals_single_clips(engine):
    gen = torch.Generator().manual_seed(11)
    wav = (0.1 * torch.randn(5, 9001, generator=gen)).clamp(-1, 1).cuda()   # conv1 .. conv4 lengths 899 / 449 / 224 / 111
    batch = engine.embed(wav)
    for i in range(5):
        assert torch.equal(batch[i:i + 1], engine.embed(wav[i:i + 1])), i
