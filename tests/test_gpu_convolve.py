"""GPU: ``nomad_degrade_convolve`` through the C ABI in guarded buffers - input rows and response rows padded with NaN behind their
lengths, output NaN-poisoned, workspace filled with 0xFF - against ``np.convolve`` in float64; then ``Engine.degrade_convolve`` /
``Nomad.convolve`` / ``Nomad.intensity_sweep(rt60_s=...)`` end to end.

Shapes.  The kernel as built (nomad_amd/csrc/degrade_convolve.hip.h) gives a workgroup an output tile of TILE = 4096 samples and
walks the taps in chunks of CHUNK = 241.  Clip lengths: 1, 2, 15, 16, 17, 255, 257, 1025, 4099, 9001 and TILE - 1, TILE, TILE + 1;
response lengths: 1, 2, 3, 16, 17, 63, 65, 1000, 4097, 6000 and CHUNK - 1, CHUNK, CHUNK + 1.  Every clip meets every response in one
call (13 x 13 rows), so responses longer than the clip are in it; one more call has G = 64.

Bounds.
* integer-valued inputs (x in [-8, 8], h in [-4, 4]: every partial sum is below 6000 x 32 < 2^24) and pure delays: the BITS of the
  float64 result - an fp32 multiply-add chain makes no rounding on them in any order.
* real values: ``|out - ref64| <= (L + 8) 2^-24 (|h| * |x|)[i] + 1e-37 L``: the running-error bound of an fp32 multiply-add chain of
  at most L terms (each step rounds a partial sum that is at most (|h| * |x|)[i] in magnitude, once, by at most 2^-24 relatively),
  + 8 for the merging of partial accumulators, the last term for products that underflow.  It holds for any order of the terms."""
import ctypes as C

import numpy as np
import pytest
import torch

import guard
from nomad_amd import _lib
from nomad_amd.nomad import synthetic_rir

pytestmark = pytest.mark.gpu

TILE, CHUNK = 4096, 241
CLIP_LENS = [1, 2, 15, 16, 17, 255, 257, 1025, 4099, 9001, TILE - 1, TILE, TILE + 1]
IR_LENS = [1, 2, 3, 16, 17, 63, 65, 1000, 4097, 6000, CHUNK - 1, CHUNK, CHUNK + 1]


def _pcm(n, seed):
    return (np.random.RandomState(seed).randint(-32768, 32768, size=n) / 32768.0).astype(np.float32)


def _ints(n, bound, seed):
    return np.random.RandomState(seed).randint(-bound, bound + 1, size=n).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows(arrays, stride):
    host = np.full((len(arrays), stride), np.nan, dtype=np.float32)
    for i, a in enumerate(arrays):
        host[i, :min(a.shape[0], stride)] = a[:stride]
    return host


class _Call:
    """One ABI call in guarded buffers; the arguments can be overridden one by one (the refusals)."""

    def __init__(self, engine, clips, irs, stride=None, x_off=0, ir_off=0, out_off=0):
        """x_off / ir_off / out_off: the rows begin that many floats (0 .. 3) behind a 256-byte boundary (``guard.Guards.empty_at``):
        base addresses aligned to 4 or 8 bytes only.  The workspace stays aligned."""
        self.engine, self.B, self.G = engine, len(clips), len(irs)
        self.lens, self.ir_lens = [int(c.shape[0]) for c in clips], [int(h.shape[0]) for h in irs]
        self.stride, self.ir_stride = stride or (max(self.lens) + 3) // 4 * 4, (max(self.ir_lens) + 3) // 4 * 4
        dev = engine.device
        self.guards = g = guard.Guards()
        self.x = g.empty_at((self.B, self.stride), x_off, device=dev, name="x")
        self.x.copy_(torch.from_numpy(_rows(clips, self.stride)))
        self.ir = g.empty_at((self.G, self.ir_stride), ir_off, device=dev, name="ir")
        self.ir.copy_(torch.from_numpy(_rows(irs, self.ir_stride)))
        self.out = g.empty_at((self.B * self.G, self.stride), out_off, device=dev, name="out")
        self.out.fill_(float("nan"))
        self.ws_bytes = int(engine.lib.nomad_degrade_convolve_scratch_bytes(self.B, self.G))
        self.ws = g.empty_bytes(max(self.ws_bytes, 256), dev, 1 << 16, "workspace")
        self.ws.fill_(0xFF)

    def run(self, **kw):
        a = dict(ctx=self.engine.ctx, x=self.x.data_ptr(), B=self.B, stride=self.stride, lens=self.lens, ir=self.ir.data_ptr(), G=self.G,
                 ir_stride=self.ir_stride, ir_lens=self.ir_lens, out=self.out.data_ptr(), ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(kw)
        lens = (C.c_int * len(a["lens"]))(*a["lens"]) if a["lens"] is not None else None
        ir_lens = (C.c_int * len(a["ir_lens"]))(*a["ir_lens"]) if a["ir_lens"] is not None else None
        rc = self.engine.lib.nomad_degrade_convolve(a["ctx"], a["x"], a["B"], a["stride"], lens, a["ir"], a["G"], a["ir_stride"], ir_lens,
                                                    a["out"], a["ws"], a["ws_bytes"], self.engine._stream())
        torch.cuda.synchronize()
        return rc

    def results(self):
        """(B, G, stride) after the guards and the zeros behind every length have been checked."""
        self.guards.check()
        out = self.out.cpu().numpy().reshape(self.B, self.G, self.stride)
        for b, n in enumerate(self.lens):
            assert not np.isnan(out[b, :, n:]).any() and not out[b, :, n:].any(), f"clip {b}: rows are zero behind the length {n}"
        return out


def _convolve(engine, clips, irs, **kw):
    call = _Call(engine, clips, irs, **kw)
    rc = call.run()
    assert rc == 0, engine.lib.nomad_last_error()
    return call.results()


def _ref64(x, h):
    return np.convolve(x.astype(np.float64), h.astype(np.float64))[:x.shape[0]]


_CACHE = {}


def _batch(engine, kind):
    """The 13 x 13 call on integer-valued ('int') or real ('real') inputs -> (clips, responses, out), made once."""
    if kind not in _CACHE:
        if kind == "int":
            clips = [_ints(n, 8, 10 + n) for n in CLIP_LENS]
            irs = [_ints(L, 4, 20 + L) for L in IR_LENS]
        else:
            clips = [_pcm(n, 30 + n) for n in CLIP_LENS]
            irs = [synthetic_rir((L - 0.5) / 16000.0, seed=L) for L in IR_LENS]
            assert [h.shape[0] for h in irs] == IR_LENS
        _CACHE[kind] = (clips, irs, _convolve(engine, clips, irs))
    return _CACHE[kind]


def test_integer_inputs_give_the_bits_of_float64(engine):
    clips, irs, out = _batch(engine, "int")
    for b, x in enumerate(clips):
        for g, h in enumerate(irs):
            want = _ref64(x, h)
            assert np.abs(want).max() < 2 ** 24
            got = out[b, g, :x.shape[0]]
            assert np.array_equal(got.astype(np.float64), want) and not np.signbit(got[want == 0]).any(), (x.shape[0], h.shape[0])


def test_sixty_four_responses_in_one_call(engine):
    clips = [_ints(257, 8, 1), _ints(4099, 8, 2)]
    irs = [_ints(IR_LENS[g % len(IR_LENS)] + g // len(IR_LENS), 4, 300 + g) for g in range(64)]
    out = _convolve(engine, clips, irs)
    for b, x in enumerate(clips):
        for g, h in enumerate(irs):
            assert np.array_equal(out[b, g, :x.shape[0]].astype(np.float64), _ref64(x, h)), (b, g, h.shape[0])


def test_pure_delays_move_the_samples_bit_for_bit(engine):
    L = 6000
    delays = [0, 1, 15, 16, 17, TILE - 1, TILE, CHUNK - 1, CHUNK, L - 1]
    irs = []
    for d in delays:
        h = np.zeros(L, dtype=np.float32)
        h[d] = 1.0
        irs.append(h)
    clips = [_pcm(n, 40 + n) for n in (257, 4099, 9001)]
    out = _convolve(engine, clips, irs)
    for b, x in enumerate(clips):
        n = x.shape[0]
        for g, d in enumerate(delays):
            want = np.zeros(n, dtype=np.float32)
            want[d:] = x[:max(n - d, 0)]
            want = want + np.float32(0.0)          # a sample of -0.0 comes out as +0.0 (it is added to the accumulator's +0.0)
            assert np.array_equal(_bits(out[b, g, :n]), _bits(want)), (n, d)


def test_real_values_within_the_running_error_bound(engine):
    clips, irs, out = _batch(engine, "real")
    worst = 0.0
    for b, x in enumerate(clips):
        for g, h in enumerate(irs):
            n, L = x.shape[0], h.shape[0]
            ref = _ref64(x, h)
            mag = _ref64(np.abs(x), np.abs(h))
            bound = (L + 8) * 2.0 ** -24 * mag + 1e-37 * L
            err = np.abs(out[b, g, :n].astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (n, L, float((err / bound).max()))
    print(f"largest error / bound over the 169 rows: {worst:.4f}")


def test_every_row_has_the_bits_of_its_own_call(engine):
    clips, irs, out = _batch(engine, "real")
    for b, x in enumerate(clips):
        for g, h in enumerate(irs):
            one = _convolve(engine, [x], [h])
            assert np.array_equal(_bits(one[0, 0, :x.shape[0]]), _bits(out[b, g, :x.shape[0]])), (x.shape[0], h.shape[0])
    again = _convolve(engine, clips, irs)
    assert np.array_equal(_bits(again), _bits(out)), "run to run"


def test_non_finite_values_stay_in_their_rows(engine):
    clips = [_pcm(4099, 1), _pcm(9001, 2)]
    irs = [synthetic_rir(1000 / 16000.0 - 1e-5, seed=3), synthetic_rir(65 / 16000.0 - 1e-5, seed=4)]
    assert [h.shape[0] for h in irs] == [1000, 65]
    clean = _convolve(engine, clips, irs)
    p = 5000
    bad = [clips[0], clips[1].copy()]
    bad[1][p] = np.nan
    out = _convolve(engine, bad, irs)
    for g, h in enumerate(irs):
        assert not np.isfinite(out[1, g, p:min(p + h.shape[0], 9001)]).any(), f"response {g}: the NaN reaches every tap"
        assert np.isfinite(out[1, g, :p - 255]).all() and np.isfinite(out[1, g, p + h.shape[0] + 255:9001]).all()
    assert np.array_equal(_bits(out[0]), _bits(clean[0])), "the other clip's rows are those of the clean call"
    k = 40
    bad_ir = [irs[0], irs[1].copy()]
    bad_ir[1][k] = np.inf
    out = _convolve(engine, clips, bad_ir)
    for b, n in enumerate((4099, 9001)):
        assert not np.isfinite(out[b, 1, k:n]).any(), f"clip {b}: an infinite tap reaches every output from its index on"
        assert np.array_equal(_bits(out[b, 0]), _bits(clean[b, 0])), "the other response's rows are those of the clean call"


# (x offset, out offset, response offset) in floats: together, separately, and every residue of 16 bytes on each pointer
OFFSETS = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 0, 0), (0, 3, 0), (0, 0, 2), (2, 1, 3)]


@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: "x%d-out%d-ir%d" % o)
def test_rows_at_unaligned_addresses_have_the_bits_of_the_aligned_call(engine, offs):
    """The kernel stores four outputs at once only where the output's base is 16-byte aligned and the four lie inside the length,
    else one by one; it reads samples and taps one by one.  Rows whose base is aligned to a float and nothing wider therefore give
    the aligned call's bits.  Lengths 4093 / 4096 / 4099 at a stride of 4100: the last vector store of a row ends 1 / 0 samples
    in front of the length or the row ends in the second tile (3 outputs of it), and the zeros behind a length reach up to the
    guard, which begins at the very next float.  The reference is np.convolve in float64 on integers (exact in any order)."""
    xo, oo, io = offs
    clips = [_ints(n, 8, 60 + n) for n in (4093, 4096, 4099)]
    irs = [_ints(L, 4, 70 + L) for L in (1, 17, CHUNK + 1, 1000)]
    if "aligned" not in _CACHE:
        _CACHE["aligned"] = _convolve(engine, clips, irs, stride=4100)
    want = _CACHE["aligned"]
    call = _Call(engine, clips, irs, stride=4100, x_off=xo, ir_off=io, out_off=oo)
    assert call.x.data_ptr() % 16 == 4 * xo and call.out.data_ptr() % 16 == 4 * oo and call.ir.data_ptr() % 16 == 4 * io
    assert call.run() == 0, engine.lib.nomad_last_error()
    out = call.results()      # guards, zeros behind every length
    assert out.shape == (3, 4, 4100) and np.array_equal(_bits(out), _bits(want)), "the bits of the aligned call"
    for b, x in enumerate(clips):
        for g, h in enumerate(irs):
            assert np.array_equal(out[b, g, :x.shape[0]].astype(np.float64), _ref64(x, h)), (x.shape[0], h.shape[0])


def test_invalid_arguments_return_a_status_and_a_message_and_touch_nothing(engine):
    lib = engine.lib
    clips, irs = [_pcm(1025, 1), _pcm(300, 2)], [_pcm(65, 3), _pcm(17, 4)]

    def refused(status, what, **kw):
        c = _Call(engine, clips, irs)
        rc = c.run(**kw)
        assert rc == status, (what, rc)
        assert lib.nomad_last_error(), what
        c.guards.check(what)
        assert bool(torch.isnan(c.out).all()), f"{what}: the output was written"
        assert bool((c.ws == 0xFF).all()), f"{what}: the workspace was written"

    inv = _lib.NOMAD_ERR_INVALID
    for name in ("ctx", "x", "lens", "ir", "ir_lens", "out", "ws"):
        refused(inv, f"NULL {name}", **{name: None})
    refused(inv, "G = 0", G=0)
    refused(inv, "G = 65", G=65)
    refused(inv, "B = 0", B=0)
    refused(inv, "B = 65536", B=65536)
    refused(inv, "stride no multiple of 4", stride=1026)
    refused(inv, "stride = 0", stride=0)
    refused(inv, "stride shorter than a length", stride=1024)
    refused(inv, "ir_stride no multiple of 4", ir_stride=66)
    refused(inv, "ir_stride = 0", ir_stride=0)
    refused(inv, "ir_stride shorter than a length", ir_stride=64)
    refused(inv, "a clip length of 0", lens=[1025, 0])
    refused(inv, "a response length of 0", ir_lens=[65, 0])
    refused(inv, "a response of 65537 taps", ir_lens=[65, 65537], ir_stride=65540)
    refused(_lib.NOMAD_ERR_WORKSPACE, "a short workspace", ws_bytes=256)
    assert lib.nomad_degrade_convolve_scratch_bytes(0, 1) == 0 and lib.nomad_degrade_convolve_scratch_bytes(65536, 1) == 0
    assert lib.nomad_degrade_convolve_scratch_bytes(2, 0) == 0 and lib.nomad_degrade_convolve_scratch_bytes(2, 65) == 0
    assert lib.nomad_degrade_convolve_scratch_bytes(2, 64) >= 4 * (2 + 64)
    # a response of the largest length is accepted: 65536 taps on a clip of 300 samples
    out = _convolve(engine, [_ints(300, 8, 5)], [_ints(65536, 4, 6)])
    assert np.array_equal(out[0, 0, :300].astype(np.float64), _ref64(_ints(300, 8, 5), _ints(65536, 4, 6)))


# ---- the host layers -------------------------------------------------------------------------------------------------------------
def test_engine_rows_feed_the_ragged_forward_without_a_copy(engine):
    clips = [torch.from_numpy(_pcm(n, 50 + n)) for n in (6400, 7001, 9600)]
    irs = [np.ones(1, dtype=np.float32), synthetic_rir(0.05, seed=1)]
    with guard.guarded(case="Engine.degrade_convolve"):
        rows, lens = engine.degrade_convolve(clips, irs)
        emb = engine.embed_ragged(None, packed=(rows, lens))
    assert rows.shape == (6, 9600) and lens == [6400] * 2 + [7001] * 2 + [9600] * 2
    plain = engine.embed_ragged(clips)
    assert torch.equal(emb[0::2], plain), "a response of [1] gives the input's embedding bits"
    for b, x in enumerate(clips):
        n = x.numel()
        assert torch.equal(rows[2 * b, :n].cpu(), x)
        ref, mag = _ref64(x.numpy(), irs[1]), _ref64(np.abs(x.numpy()), np.abs(irs[1]))
        err = np.abs(rows[2 * b + 1, :n].cpu().numpy().astype(np.float64) - ref)
        assert (err <= (irs[1].shape[0] + 8) * 2.0 ** -24 * mag + 1e-37 * irs[1].shape[0]).all()
    stacked = torch.zeros(2, 800)
    stacked[0, :1] = 1.0
    stacked[1] = torch.from_numpy(irs[1])
    again, lens2 = engine.degrade_convolve(clips, stacked, ir_lengths=[1, 800])
    assert lens2 == lens and torch.equal(again, rows), "a (G,L) tensor with ir_lengths is the list of responses"


@pytest.mark.parametrize("k", [None, 2])
def test_sweep_scores_are_score_on_the_convolved_rows(engine, k):
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    lens = [6400, 8000, 9600]
    clean = torch.zeros(3, 9600)
    for b, n in enumerate(lens):
        clean[b, :n] = torch.from_numpy(_pcm(n, 70 + b))
    refs = torch.randn(5, 256, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    refs = (refs / refs.norm(dim=1, keepdim=True)).float()
    rt60 = [0.2, 0.05]
    with guard.guarded(case="intensity_sweep(rt60_s)"):
        res = nomad.intensity_sweep(clean, refs, lengths=lens, k=k, rt60_s=rt60, rir_seed=3, drr_db=2.0)
    assert sorted(res) == ["REVERB"]
    rows, lens_rep = nomad.convolve(clean, [torch.from_numpy(synthetic_rir(v, 3, 2.0)) for v in rt60], lengths=lens)
    assert rows.shape == (6, 9600) and lens_rep == [n for n in lens for _ in rt60]
    want = nomad.score(rows, refs, lengths=lens_rep, k=k).cpu().numpy()
    got = res["REVERB"]["scores"]
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
    table = res["REVERB"]["table"].sort_values(by="Condition")
    assert list(table.columns) == ["Condition", "Distance"] and table["Condition"].tolist() == [0.05, 0.2]
    assert np.allclose(table["Distance"].to_numpy(), [want[1::2].mean(), want[0::2].mean()], rtol=1e-12, atol=0)
