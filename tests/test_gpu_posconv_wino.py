"""GPU: the fp32 positional convolution in nested F(2,2) form (nomad_amd/csrc/posconv_wino_f32.hip.h).

One group of the pos-conv is the 128-tap correlation C[t] = sum_k A[t + k] V[k] over the zero-padded frames of a clip.  The engine
runs it as 9 quarter-rate 32-tap correlations per group (input differences, weight sums, output sums: tests/
test_posconv_wino_identity.py restates the algebra on the CPU).  The layout tests use small-integer operands, where every
transformed operand and every partial sum is exact in fp32, so the pre-activation must equal the float64 direct correlation bit
for bit: any wrong frame, tap, channel, operand, clip boundary or output parity shows.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pad_group_major(x, lens):
    """x [sum T][768] -> the engine's padded group-major buffer [16][sum (T + 128)][48] (64 zero frames around every clip)."""
    clips, o = [], 0
    for T in lens:
        xc = torch.zeros(T + 128, 768, dtype=x.dtype)
        xc[64:64 + T] = x[o:o + T]
        clips.append(xc)
        o += T
    return torch.cat(clips).view(-1, 16, 48).transpose(0, 1).contiguous()


def _posconv_ref(xpad, w, lens):
    """float64 direct correlation per clip and group.  xpad [16][sum (T + 128)][48], w [16][64][6144] ([out][tap * 48 + in])."""
    outs, o = [], 0
    for T in lens:
        xc = xpad[:, o:o + T + 128]                                          # [16][T + 128][48]
        cols = torch.stack([xc[:, t:t + 128].reshape(16, -1) for t in range(T)], dim=1)   # [16][T][6144], tap-major
        y = torch.einsum("gtk,gnk->tgn", cols, w[:, :48])                    # [T][16][48]
        outs.append(y.reshape(T, 768))
        o += T + 128
    return torch.cat(outs)


def _hook(eng):
    fn = eng.lib.nomad_diag_posconv
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int,
                   C.c_void_p]
    return fn


@pytest.fixture(scope="module")
def diag_posconv(built_lib):
    from nomad_amd import _lib
    from nomad_amd.engine import Engine
    from nomad_amd.weights import seeded_state_dict
    old = os.environ.get("NOMAD_F32_POSCONV_WINO")
    os.environ["NOMAD_F32_POSCONV_WINO"] = "1"   # read when the context is created: the hook runs the form under test
    try:
        eng = Engine(seeded_state_dict(0), 0, diag=True)
    finally:
        if old is None:
            del os.environ["NOMAD_F32_POSCONV_WINO"]
        else:
            os.environ["NOMAD_F32_POSCONV_WINO"] = old
    fn = _hook(eng)

    def run(xpad, w, bias, lens, ragged):
        rows = sum(lens)
        guard = 64   # rows behind the output that nothing may touch
        y = torch.full((rows + guard, 768), 1234.5, device="cuda")
        u = torch.full((rows + guard, 768), 1234.5, device="cuda")
        arr = (C.c_int * len(lens))(*lens)
        _lib.check(fn(eng.ctx, xpad.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), u.data_ptr(), len(lens), arr,
                      int(ragged), eng._stream()), "nomad_diag_posconv")
        torch.cuda.synchronize()
        assert (y[rows:] == 1234.5).all() and (u[rows:] == 1234.5).all(), "stores beyond the last output row"
        return y[:rows].cpu(), u[:rows].cpu()

    yield run
    eng.close()


# every remainder of T modulo 4 at one and at several operand rows, clips shorter than one row, partial and full 16-row blocks of
# the transform kernels (T = 63 / 64 / 65: 16 / 16 / 17 rows), the 4 s clip's 199 frames and an even neighbour; ragged: clip
# boundaries inside a GEMM tile and inside a transform block, all four remainders
CASES = [([T] * n, False) for T, n in ((1, 3), (2, 2), (3, 3), (4, 2), (5, 3), (63, 2), (64, 2), (65, 3), (199, 2), (200, 2))]
CASES += [([199, 1, 4, 130, 7, 64], True), ([65, 65], True)]


@pytest.mark.parametrize("lens,ragged", CASES)
def test_exact_integer_layout(diag_posconv, lens, ragged):
    gen = torch.Generator().manual_seed(sum(lens) + 17 * len(lens) + ragged)
    x = torch.randint(-3, 4, (sum(lens), 768), generator=gen).float()
    w = torch.zeros(16, 64, 6144)
    w[:, :48] = torch.randint(-2, 3, (16, 48, 6144), generator=gen).float()
    xpad = _pad_group_major(x, lens)
    y, u = diag_posconv(xpad.cuda(), w.cuda(), torch.zeros(768, device="cuda"), lens, ragged)
    ref = _posconv_ref(xpad.double(), w.double(), lens)
    # operands |x| <= 12, weights |w| <= 8, 1536 products per sum: every operand and partial sum is an integer below 2^24
    assert 12 * 8 * 1536 < 2 ** 24 and ref.abs().max().item() < 2 ** 24
    assert torch.equal(u.double(), ref), (u.double() - ref).abs().max().item()
    want = x.double() + torch.nn.functional.gelu(ref)
    assert ((y.double() - want).abs() <= 1e-6 * want.abs().clamp(min=1.0)).all()


def _stage_errors(wino, peaky):
    """Max |engine pos-conv - float64 pos-conv| of the pre-activation and of the stage's output, on the engine's own pos-conv
    input (2 clips of 9000 samples) and the model's folded fp32 weights, in a child process (the switch is read when a context is
    created, by libnomad_diag.so)."""
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
_lib.check(_hook(eng)(eng.ctx, xpad.data_ptr(), w.cuda().data_ptr(), bias.cuda().data_ptr(), y.data_ptr(), u.data_ptr(), B, lens, 0,
                      eng._stream()), "nomad_diag_posconv")
torch.cuda.synchronize()
xp = xpad.cpu().double()
ref_u = _posconv_ref(xp, w.double(), [T] * B) + bias.double()
x = torch.cat([xp[:, b * (T + 128) + 64:b * (T + 128) + 64 + T] for b in range(B)], dim=1).transpose(0, 1).reshape(B * T, 768)
ref_y = x + torch.nn.functional.gelu(ref_u)
print(repr((u.cpu().double() - ref_u).abs().max().item()), repr((y.cpu().double() - ref_y).abs().max().item()))
eng.close()
"""
    env = dict(os.environ, NOMAD_F32_POSCONV_WINO=str(int(wino)))
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return [float(v) for v in r.stdout.split()[-2:]]


@pytest.mark.parametrize("peaky", [False, True])
def test_accuracy_vs_direct_form(built_lib, peaky):
    """The bar of the conv1 .. conv4 change (tests/test_gpu_conv_s2.py): below 2e-5, and at most twice the direct form's error."""
    old = _stage_errors(False, peaky)
    new = _stage_errors(True, peaky)
    print("pos-conv stage, max error against float64 (pre-activation, output): direct", old, "nested F(2,2)", new)
    for eo, en in zip(old, new):
        assert en < 2e-5 and eo < 2e-5, (eo, en)
        assert en <= 2 * eo + 1e-7, (eo, en)


def test_five_clip_batch_equals_single_clips(engine):
    gen = torch.Generator().manual_seed(11)
    wav = (0.1 * torch.randn(5, 9001, generator=gen)).clamp(-1, 1).cuda()   # 27 frames per clip: 7 operand rows, the last of 3 frames
    batch = engine.embed(wav)
    for i in range(5):
        assert torch.equal(batch[i:i + 1], engine.embed(wav[i:i + 1])), i


def test_ragged_batch_equals_per_clip_calls(engine):
    gen = torch.Generator().manual_seed(12)
    lens = [9001, 400, 1300, 5000, 2210, 800]   # 27 / 1 / 3 / 15 / 6 / 2 frames: every remainder modulo 4, clips below one operand row
    waves = [(0.1 * torch.randn(n, generator=gen)).clamp(-1, 1) for n in lens]
    batch = engine.embed_ragged(waves)
    for i, w in enumerate(waves):
        assert torch.equal(batch[i:i + 1], engine.embed_ragged([w])), i
        assert torch.equal(batch[i:i + 1], engine.embed(w.view(1, -1).cuda())), i


def test_transformed_weights_follow_a_training_step(built_lib):
    """After an optimiser step, embed() on the trained engine equals embed() on a fresh engine made from the updated weights, bit
    for bit: the transformed pos-conv weights were rebuilt together with the folded ones."""
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
