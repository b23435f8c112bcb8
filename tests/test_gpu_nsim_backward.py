"""GPU: ``nomad_nsim_backward`` and ``nomad_gammatone_backward`` through the C ABI in guarded, NaN-poisoned buffers, and
``Nomad.nsim_loss`` end to end, against the torch float64 restatement ``nsim_grad_ref`` (the conventions of include/nomad_hip.h,
"NSIM as a loss").

Bound per value: ``2^-23 |g_ref| + tau max|g_ref|`` for the fp32 samples' gradient, ``tau max|g_ref|`` for the float64 planes.  tau is
derived per case, at run time, from the restatement alone: the restatement run in float32 on the same inputs against its float64
run, relative to max|g|, times 2^-25 - the ratio of the two formats' rounding units, 2^-29, times a margin of 16 for the order of
the operations (``nsim_grad_ref.tau``).  Every case prints its tau and the device's distance in the same unit.
MEASURED tau (CPU) and device distance relative to max|g| (MI355X), per case:
  map, B = 4 x G = 2 (F = 1, 2, 3, 13): tau 9.6e-13 .. 2.5e-11, device 2.5e-14 .. 6.2e-13 (each 10 x or more under its tau)
  map, host cases a .. e (F = 12):        tau 1.0e-12, 8.4e-13, 8.3e-13, 5.3e-12, 3.8e-12; device 6.8e-14, 3.7e-14, 1.3e-13, 2.5e-13, 1.3e-13
  gammatone, dense dspec:                 tau 5.9e-13 (1280), 8.2e-13 (1600), 7.1e-13 (5120), 9.4e-13 (5220), 1.4e-12 (48 kHz)
  gammatone, one cell of the 5120 row:    tau 7.4e-12 (frame 0, band 0), 1.7e-14 (frame 12, band 20)
  nsim_loss end to end, cases a .. e:     tau 2.9e-12, 5.0e-12, 2.6e-12, 5.6e-12, 1.9e-12
  every fp32 output (gammatone, nsim_loss): device 2.3e-8 .. 4.7e-8 of max|g|, which is the output's own rounding to fp32 (2^-24 = 6.0e-8 of
  a value): the float64 part of the bound cannot be told apart from it in these figures, the map's rows above show it alone.

Cases.  Map alone: spectrograms the restatement makes (numpy float64) of cuts of tests/golden/wavs/nmr-data/FI53_04.wav: one call of
B = 4 clips with F = 1, 2, 3 and 13 frames and G = 2 rows each (noise at 10 dB and at 5 dB) with a different upstream value per row,
and one call of the five host cases a .. e (tests/test_nsim_grad_host.py: absolute floor and zero variance, per-frame floor in the
degraded plane, clean cells on a floor set by a degraded peak) whose counters are asserted again here.  Gammatone alone: rows of
1280 (F = 1), 1600 (F = 2), 5120 (F = 13: across the 12-frame workgroup) and 5220 samples (a trailing partial frame) at 16 kHz and one
48 kHz row of 4800 samples (F = 2), a dense dspec each, and on the 5120 row dspec with ONE non-zero cell (the adjoint's impulse
response).  The references are computed once per case and shared."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import guard
import nsim_grad_ref as GR
import nsim_ref as N
from conftest import ROOT
from nomad_amd import _lib, wavio

pytestmark = pytest.mark.gpu

NAN = float("nan")
U23 = 2.0 ** -23
FORWARD_BOUND = 9.8e-12      # tests/test_gpu_nsim.py's MAP_BOUND: the forward is not this module's subject


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


_CLIP = []


def golden_clip():
    if not _CLIP:
        x, fs = wavio.read_wav(os.path.join(ROOT, "tests", "golden", "wavs", "nmr-data", "FI53_04.wav"))
        assert fs == 16000
        _CLIP.append(np.asarray(x, dtype=np.float32).reshape(-1))
    return _CLIP[0]


def _held(name, got, want, t, fp32):
    """Assert the bound on every value; print tau and the device's distance relative to max|g|."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    top = float(np.abs(want).max())
    err = np.abs(got - want)
    bound = t * top + (U23 * np.abs(want) if fp32 else 0.0)
    print(f"{name}: tau {t:.3g}, device distance / max|g| {float(err.max()) / top if top else 0.0:.3g}, max|g| {top:.3g}")
    assert np.isfinite(got).all(), name
    assert (err <= bound).all(), (name, float(err.max()), float(np.max(err - bound)))


# ---- the map alone --------------------------------------------------------------------------------------------------------------
_MAP = {}


def map_cases():
    """{"frames": (R list, D list, frames, G, upstream (B, G)), "host": ...}: spectrograms by the restatement, made once."""
    if not _MAP:
        clip = golden_clip()
        x = clip[8000:13120].copy()                              # 13 frames
        noise = N.pcm_noise(5120, 5)
        S = [N.spectrogram(v, dtype=np.float64) for v in (x, N.add_noise(x, noise, 10.0), N.add_noise(x, noise, 5.0))]
        Fs = [1, 2, 3, 13]
        up = np.random.RandomState(17).randn(len(Fs), 2)
        _MAP["frames"] = ([S[0][:F] for F in Fs], [[S[1][:F], S[2][:F]] for F in Fs], Fs, 2, up)
        cuts = GR.cases(clip)
        names = sorted(cuts)
        _MAP["host"] = ([N.spectrogram(cuts[k][0], dtype=np.float64) for k in names],
                        [[N.spectrogram(cuts[k][1], dtype=np.float64)] for k in names], [12] * len(names), 1, np.ones((len(names), 1)))
    return _MAP


class NsCall:
    """One ``nomad_nsim_backward`` call in guarded buffers: output NaN-filled, workspace 0xFF (NaN as float64)."""

    def __init__(self, engine, R, D, frames, g, up):
        self.engine, self.frames, self.G, self.B = engine, [int(f) for f in frames], g, len(frames)
        dev = engine.device
        self.guards = gd = guard.Guards()
        ref = np.concatenate(R)
        deg = np.concatenate([d for rows in D for d in rows])
        self.ref = gd.empty(ref.shape, dtype=torch.float64, device=dev, name="spec_ref")
        self.ref.copy_(torch.from_numpy(ref))
        self.deg = gd.empty(deg.shape, dtype=torch.float64, device=dev, name="spec_deg")
        self.deg.copy_(torch.from_numpy(deg))
        self.grad = gd.empty((self.B, g), dtype=torch.float64, device=dev, name="grad_nsim")
        self.grad.copy_(torch.from_numpy(np.asarray(up, dtype=np.float64)))
        self.out = gd.empty(deg.shape, dtype=torch.float64, device=dev, name="dspec")
        self.out.fill_(NAN)
        need = int(engine.lib.nomad_nsim_backward_scratch_bytes(self.B, g, sum(self.frames)))
        self.ws = gd.empty_bytes(max(need, 256), dev, 1 << 16, "workspace")
        self.ws.fill_(0xFF)
        self.ws_bytes = need

    def run(self, **over):
        a = dict(ref=self.ref.data_ptr(), deg=self.deg.data_ptr(), B=self.B, G=self.G, frames=self.frames, L=1.0, grad=self.grad.data_ptr(),
                 out=self.out.data_ptr(), ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(over)
        rc = self.engine.lib.nomad_nsim_backward(self.engine.ctx, a["ref"], a["deg"], a["B"], a["G"], (C.c_int * len(a["frames"]))(*a["frames"]),
                                                 a["L"], a["grad"], a["out"], a["ws"], a["ws_bytes"], self.engine._stream())
        torch.cuda.synchronize()
        return rc

    def rows(self):
        """-> dspec of row (b, g) as [b][g] arrays [F_b][21], guards checked."""
        self.guards.check()
        flat = self.out.cpu().numpy()
        out, at = [], 0
        for F in self.frames:
            out.append([flat[at + k * F:at + (k + 1) * F] for k in range(self.G)])
            at += self.G * F
        return out


@pytest.mark.parametrize("which", ["frames", "host"])
def test_map_gradient_is_held_to_the_restatement(engine, which):
    R, D, frames, g, up = map_cases()[which]
    call = NsCall(engine, R, D, frames, g, up)
    assert call.run() == 0, engine.lib.nomad_last_error()
    got = call.rows()
    again = NsCall(engine, R, D, frames, g, up)
    assert again.run() == 0
    got2 = again.rows()
    seen = {}
    for b, F in enumerate(frames):
        for k in range(g):
            _, want, counters = GR.map_grad(R[b], D[b][k], upstream=float(up[b, k]))
            _, g32, _ = GR.map_grad(R[b], D[b][k], upstream=float(up[b, k]), dtype=torch.float32)
            _held(f"map {which} clip {b} (F={F}) row {k}", got[b][k], want, GR.tau(want, g32), fp32=False)
            assert np.array_equal(_bits(got2[b][k]), _bits(got[b][k])), "run to run"
            one = NsCall(engine, [R[b]], [[D[b][k]]], [F], 1, [[up[b, k]]])
            assert one.run() == 0
            assert np.array_equal(_bits(one.rows()[0][0]), _bits(got[b][k])), f"clip {b} row {k}: the bits of its own B = 1, G = 1 call"
            seen[b] = counters
    if which == "host":                                       # a .. e in sorted order
        assert seen[2]["abs_floor_deg"] >= 1 and seen[2]["zero_var"] >= 1, seen[2]
        assert seen[3]["frame_floor_deg"] >= 1, seen[3]
        assert seen[4]["frame_floor_clean_deg_peak"] >= 1 and seen[4]["deg_peak_frames"] >= 1, seen[4]
        assert np.abs(got[4][0]).max() > 0.0


def test_a_nan_row_of_the_map_is_nan_and_no_other_changes(engine):
    R, D, frames, g, up = map_cases()["frames"]
    base = NsCall(engine, R, D, frames, g, up)
    assert base.run() == 0
    want = base.rows()
    bad = [[d.copy() for d in rows] for rows in D]
    bad[3][1][7, 4] = NAN
    call = NsCall(engine, R, bad, frames, g, up)
    assert call.run() == 0
    got = call.rows()
    for b in range(len(frames)):
        for k in range(g):
            if (b, k) == (3, 1):
                assert np.isnan(got[b][k]).all()
            else:
                assert np.array_equal(_bits(got[b][k]), _bits(want[b][k])), (b, k)


# ---- the gammatone adjoint alone ------------------------------------------------------------------------------------------------
def _row(name):
    clip = golden_clip()
    return {"n1280": (clip[8000:9280], 16000), "n1600": (clip[8000:9600], 16000), "n5120": (clip[8000:13120], 16000),
            "n5220": (clip[8000:13220], 16000), "48k": (clip[8000:12800], 48000)}[name]


def _dspec(name, kind):
    x, fs = _row(name)
    F = N.frames_of(x.shape[0], fs)
    if kind == "dense":
        return np.random.RandomState(x.shape[0]).randn(F, 21)
    t, b = kind
    d = np.zeros((F, 21))
    d[t, b] = 1.0
    return d


_GT = {}


def gt_ref(name, kind):
    """(gradient [n] float64 by the restatement, tau), computed once per case."""
    if (name, kind) not in _GT:
        x, fs = _row(name)
        d = _dspec(name, kind)
        g64 = GR.spectrogram_grad(x, d, fs)
        g32 = GR.spectrogram_grad(x, d, fs, dtype=torch.float32)
        g64.setflags(write=False)
        _GT[(name, kind)] = (g64, GR.tau(g64, g32))
    return _GT[(name, kind)]


class GtCall:
    """One ``nomad_gammatone_backward`` call in guarded buffers: the rows NaN behind each length, output NaN-filled, workspace 0xFF."""

    def __init__(self, engine, rows, dspecs, fs=16000, stride=None, x_off=0):
        self.engine, self.fs, self.R = engine, fs, len(rows)
        self.lens = [int(r.shape[0]) for r in rows]
        self.stride = stride if stride is not None else (max(self.lens) + 3) // 4 * 4
        dev = engine.device
        self.guards = g = guard.Guards()
        host = np.full((self.R, self.stride), np.nan, dtype=np.float32)
        for r, x in enumerate(rows):
            host[r, :self.lens[r]] = x
        self.x = g.empty_at((self.R, self.stride), x_off, device=dev, name="x")
        self.x.copy_(torch.from_numpy(host))
        d = np.concatenate(dspecs)
        self.dspec = g.empty(d.shape, dtype=torch.float64, device=dev, name="dspec")
        self.dspec.copy_(torch.from_numpy(d))
        self.dx = g.empty_at((self.R, self.stride), x_off, device=dev, name="dx")
        self.dx.fill_(NAN)
        need = int(engine.lib.nomad_gammatone_backward_scratch_bytes(self.R, self.stride, fs))
        self.ws = g.empty_bytes(max(need, 256), dev, 1 << 16, "workspace")
        self.ws.fill_(0xFF)
        self.ws_bytes = need

    def run(self, **over):
        a = dict(x=self.x.data_ptr(), R=self.R, stride=self.stride, lens=self.lens, fs=self.fs, dspec=self.dspec.data_ptr(), dx=self.dx.data_ptr(),
                 ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(over)
        rc = self.engine.lib.nomad_gammatone_backward(self.engine.ctx, a["x"], a["R"], a["stride"], (C.c_int * len(a["lens"]))(*a["lens"]),
                                                      a["fs"], a["dspec"], a["dx"], a["ws"], a["ws_bytes"], self.engine._stream())
        torch.cuda.synchronize()
        return rc

    def results(self):
        """-> dx [R][stride] fp32, guards checked."""
        self.guards.check()
        return self.dx.cpu().numpy()


def _whole(n, fs):
    H = fs // 50
    return (N.frames_of(n, fs) - 1) * H + 4 * H


@pytest.mark.parametrize("name", ["n1280", "n1600", "n5120", "n5220", "48k"])
def test_gammatone_gradient_is_held_to_the_restatement(engine, name):
    x, fs = _row(name)
    want, t = gt_ref(name, "dense")
    call = GtCall(engine, [x], [_dspec(name, "dense")], fs, stride=(x.shape[0] + 3) // 4 * 4 + 8)
    assert call.run() == 0, engine.lib.nomad_last_error()
    got = call.results()[0]
    n, covered = x.shape[0], _whole(x.shape[0], fs)
    _held(f"gammatone {name} dense", got[:n], want, t, fp32=True)
    assert not got[covered:].any() and not np.isnan(got).any(), "0 behind the whole frames, every element written"
    assert not want[covered:].any()


@pytest.mark.parametrize("cell", [(0, 0), (12, 20)])
def test_a_single_cell_gives_the_adjoints_impulse_response(engine, cell):
    x, fs = _row("n5120")
    want, t = gt_ref("n5120", cell)
    call = GtCall(engine, [x], [_dspec("n5120", cell)], fs)
    assert call.run() == 0, engine.lib.nomad_last_error()
    got = call.results()[0]
    _held(f"gammatone n5120 cell {cell}", got, want, t, fp32=True)
    lo = cell[0] * 320
    assert not got[:lo].any() and not got[lo + 1280:].any() and got[lo:lo + 1280].any(), "one frame's samples and no other"


def test_a_row_keeps_its_bits_in_any_batch_stride_and_alignment(engine):
    names = ["n1280", "n1600", "n5120", "n5220"]
    rows = [_row(k)[0] for k in names]
    ds = [_dspec(k, "dense") for k in names]
    batch = GtCall(engine, rows, ds)
    assert batch.run() == 0, engine.lib.nomad_last_error()
    got = batch.results()
    again = GtCall(engine, rows, ds)
    assert again.run() == 0
    assert np.array_equal(_bits(again.results()), _bits(got)), "run to run"
    for r, x in enumerate(rows):
        n = x.shape[0]
        _held(f"gammatone batch row {names[r]}", got[r, :n], gt_ref(names[r], "dense")[0], gt_ref(names[r], "dense")[1], fp32=True)
        assert not got[r, _whole(n, 16000):].any()
        one = GtCall(engine, [x], [ds[r]], stride=(n + 3) // 4 * 4 + 8 * (r % 2), x_off=1)
        assert one.x.data_ptr() % 16 == 4
        assert one.run() == 0
        assert np.array_equal(_bits(one.results()[0, :n]), _bits(got[r, :n])), f"row {names[r]}: the bits of its own R = 1 call"


def test_engine_grouping_changes_no_bit(engine, monkeypatch):
    from nomad_amd import engine as engine_mod
    names = ["n1600", "n5120", "n5220", "n1280"]
    rows = [torch.from_numpy(_row(k)[0].copy()) for k in names]
    buf, lens = engine._pack([r.cuda() for r in rows])
    frames = [engine.gammatone_frames(n) for n in lens]
    dspec = torch.from_numpy(np.concatenate([_dspec(k, "dense") for k in names])).cuda()
    with guard.guarded(case="Engine.gammatone_backward"):
        whole = engine.gammatone_backward(dspec, packed=(buf, lens))
    lib = engine.lib
    two = int(lib.nomad_gammatone_backward_scratch_bytes(2, buf.shape[1], 16000))
    monkeypatch.setattr(engine_mod, "NSIM_BACKWARD_WORKSPACE_BYTES", two)
    assert engine._groups([1] * 4, lambda k: two - 2, "row") == [(0, 2), (2, 4)]
    with guard.guarded(case="Engine.gammatone_backward in two groups"):
        split = engine.gammatone_backward(dspec, packed=(buf, lens))
    assert torch.equal(split.view(torch.int32), whole.view(torch.int32))
    # the map's backward, grouped by clips
    spec, _ = engine.gammatone(packed=(buf, lens))
    deg = (spec * 1.25).contiguous()
    up = torch.from_numpy(np.random.RandomState(2).randn(4, 1)).cuda()
    monkeypatch.setattr(engine_mod, "NSIM_BACKWARD_WORKSPACE_BYTES", 1 << 30)
    whole = engine.nsim_backward(spec, deg, frames, 1, up)
    monkeypatch.setattr(engine_mod, "NSIM_BACKWARD_WORKSPACE_BYTES", int(lib.nomad_nsim_backward_scratch_bytes(2, 1, frames[0] + frames[1])))
    with guard.guarded(case="Engine.nsim_backward in groups"):
        split = engine.nsim_backward(spec, deg, frames, 1, up)
    assert torch.equal(split.view(torch.int64), whole.view(torch.int64))
    monkeypatch.setattr(engine_mod, "NSIM_BACKWARD_WORKSPACE_BYTES", 1 << 20)
    with pytest.raises(ValueError, match="NSIM_BACKWARD_WORKSPACE_BYTES"):
        engine.gammatone_backward(dspec, packed=(buf, lens))


def test_a_nan_sample_voids_its_row_and_no_other(engine):
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    clip = golden_clip()
    lens = [5220, 5220, 4800]
    clean = torch.zeros(3, 5220)
    est = torch.zeros(3, 5220)
    for b, n in enumerate(lens):
        x = clip[8000 + 1000 * b:8000 + 1000 * b + n]
        clean[b, :n] = torch.from_numpy(x)
        est[b, :n] = torch.from_numpy(N.add_noise(x, N.pcm_noise(n, 30 + b), 10.0))

    def grad(e):
        e = e.clone().cuda().requires_grad_(True)
        with guard.guarded(case="nsim_loss with a NaN row"):
            loss = nomad.nsim_loss(e, clean.cuda(), lengths=lens, reduction="none")
            loss.sum().backward()
        return loss.detach().cpu().numpy(), e.grad.cpu().numpy()

    loss0, g0 = grad(est)
    bad = est.clone()
    bad[1, 2000] = NAN
    loss, g = grad(bad)
    assert np.isnan(loss[1]) and np.isfinite(loss[[0, 2]]).all()
    covered = _whole(5220, 16000)
    assert covered == 5120 and np.isnan(g[1, :covered]).all() and not g[1, covered:].any(), "NaN on the whole frames, 0 behind"
    assert np.array_equal(_bits(g[[0, 2]]), _bits(g0[[0, 2]])) and np.array_equal(_bits(loss[[0, 2]]), _bits(loss0[[0, 2]]))
    assert np.isfinite(g0).all() and not g0[2, 4800:].any()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
_E2E = {}


def e2e_ref(name):
    """(nsim, d (1 - nsim) / d estimate by the restatement, tau, counters) of a host case, computed once."""
    if name not in _E2E:
        clean, est = GR.cases(golden_clip())[name]
        score, g64, counters = GR.loss_grad(clean, est)
        _, g32, _ = GR.loss_grad(clean, est, dtype=torch.float32)
        g64.setflags(write=False)
        _E2E[name] = (score, g64, GR.tau(g64, g32), counters)
    return _E2E[name]


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_nsim_loss_end_to_end_is_held_to_the_restatement(engine, name):
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    clean, est = GR.cases(golden_clip())[name]
    score, want, t, counters = e2e_ref(name)
    c = torch.from_numpy(clean.copy())[None, None, :].cuda()
    e = torch.from_numpy(est.copy())[None, None, :].cuda().requires_grad_(True)
    with guard.guarded(case=f"nsim_loss {name}"):
        loss = nomad.nsim_loss(e, c, reduction="none")
        up = 0.75
        grads = torch.autograd.grad(loss, [e], grad_outputs=torch.full_like(loss, up))
    assert loss.shape == (1,) and loss.dtype == torch.float64 and grads[0].shape == e.shape and grads[0].dtype == torch.float32
    assert abs(float(loss[0].detach()) - (1.0 - score)) <= FORWARD_BOUND, (float(loss[0].detach()), 1.0 - score)
    assert np.array_equal(_bits(loss.detach().cpu().numpy()), _bits(1.0 - nomad.nsim(e.detach(), c).cpu().numpy().reshape(-1))), "1 - nsim's bits"
    _held(f"nsim_loss {name} ({counters})", grads[0].cpu().numpy().reshape(-1), up * want, t, fp32=True)


def test_nsim_loss_reductions_lengths_and_the_clean_side(engine):
    from nomad_amd.nomad import Nomad
    nomad = Nomad.from_engine(engine)
    cuts = GR.cases(golden_clip())
    clean = torch.from_numpy(np.stack([cuts["a"][0], cuts["c"][0]])).cuda()
    est = torch.from_numpy(np.stack([cuts["a"][1], cuts["c"][1]])).cuda()

    def grad(e, c, up=None, **kw):
        e = e.clone().requires_grad_(True)
        loss = nomad.nsim_loss(e, c, **kw)
        loss.backward(up) if up is not None else loss.backward()
        return loss.detach(), e.grad

    up = torch.tensor([0.5, -2.0], dtype=torch.float64).cuda()
    loss, g = grad(est, clean, up, reduction="none")
    for b, k in enumerate("ac"):
        _held(f"reduction none row {k}", g[b].cpu().numpy(), float(up[b]) * e2e_ref(k)[1], e2e_ref(k)[2], fp32=True)
    mean, gm = grad(est, clean)
    assert mean.dim() == 0 and abs(float(mean) - float(loss.mean())) <= 1e-15
    for b, k in enumerate("ac"):
        _held(f"reduction mean row {k}", gm[b].cpu().numpy(), 0.5 * e2e_ref(k)[1], e2e_ref(k)[2], fp32=True)
    # two lengths: each row has the bits of its own call, and 0 behind its whole frames
    lens = [4800, 3333]
    _, gl = grad(est, clean, torch.ones(2, dtype=torch.float64).cuda(), lengths=lens, reduction="none")
    for b, n in enumerate(lens):
        _, own = grad(est[b:b + 1, :n], clean[b:b + 1, :n], torch.ones(1, dtype=torch.float64).cuda(), reduction="none")
        assert torch.equal(gl[b, :n].view(torch.int32), own[0].view(torch.int32)), f"row {b}: the bits of its own call"
        assert not gl[b, _whole(n, 16000):].any()
    # clean gets None; (B, N) and (B, 1, N) alike
    e = est.clone().requires_grad_(True)
    c = clean.clone()
    loss = nomad.nsim_loss(e[:, None, :], c[:, None, :])
    assert torch.autograd.grad(loss, [e, c.requires_grad_(True)], allow_unused=True)[1] is None
    with pytest.raises(ValueError, match="clean must not require a gradient"):
        nomad.nsim_loss(e, c)
    same = nomad.nsim_loss(clean.clone().requires_grad_(True), clean, reduction="none")
    assert bool((same.abs() <= FORWARD_BOUND).all())


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_anything_is_queued(engine):
    lib = engine.lib
    inv, wsp = _lib.NOMAD_ERR_INVALID, _lib.NOMAD_ERR_WORKSPACE
    rows = [N.pcm_noise(1920, 41), N.pcm_noise(1280, 42)]
    ds = [np.ones((3, 21)), np.ones((1, 21))]

    def refused_gt(status, what, **over):
        call = GtCall(engine, rows, ds)
        rc = call.run(**over)
        assert rc == status, (what, rc)
        assert lib.nomad_last_error(), what
        call.guards.check(what)
        assert bool(torch.isnan(call.dx).all()), f"{what}: the output was written"
        assert bool((call.ws == 0xFF).all()), f"{what}: the workspace was written"

    refused_gt(inv, "a length of 1279: below one frame", lens=[1920, 1279])
    refused_gt(inv, "NULL x_dev", x=None)
    refused_gt(inv, "NULL dspec_dev", dspec=None)
    refused_gt(inv, "NULL output", dx=None)
    refused_gt(inv, "NULL workspace", ws=None)
    refused_gt(inv, "R = 0", R=0, lens=[1920])
    refused_gt(inv, "stride no multiple of 4", stride=1922)
    refused_gt(inv, "stride shorter than a length", stride=1916)
    refused_gt(inv, "a rate below 16000", fs=15950)
    refused_gt(inv, "a rate above 48000", fs=48050)
    refused_gt(inv, "a rate that is no multiple of 50", fs=16010)
    refused_gt(wsp, "ws_bytes - 1", ws_bytes=GtCall(engine, rows, ds).ws_bytes - 1)
    size = lib.nomad_gammatone_backward_scratch_bytes
    assert size(0, 1920, 16000) == 0 and size(2, 1922, 16000) == 0 and size(2, 1920, 16010) == 0 and size(2, 1276, 16000) == 0
    assert size(2, 1920, 16000) - lib.nomad_gammatone_scratch_bytes(2, 1920, 16000) == 2 * 3 * 1280 * 21 * 8

    R, D, frames, g, up = map_cases()["frames"]

    def refused_ns(status, what, **over):
        call = NsCall(engine, R, D, frames, g, up)
        rc = call.run(**over)
        assert rc == status, (what, rc)
        assert lib.nomad_last_error(), what
        call.guards.check(what)
        assert bool(torch.isnan(call.out).all()), f"{what}: the output was written"
        assert bool((call.ws == 0xFF).all()), f"{what}: the workspace was written"

    refused_ns(inv, "NULL spec_ref_dev", ref=None)
    refused_ns(inv, "NULL spec_deg_dev", deg=None)
    refused_ns(inv, "NULL grad_nsim_dev", grad=None)
    refused_ns(inv, "NULL output", out=None)
    refused_ns(inv, "NULL workspace", ws=None)
    refused_ns(inv, "B = 0", B=0)
    refused_ns(inv, "G = 65", G=65)
    refused_ns(inv, "a frame count of 0", frames=[1, 0, 3, 13])
    refused_ns(inv, "an intensity range of 0", L=0.0)
    refused_ns(wsp, "ws_bytes - 1", ws_bytes=NsCall(engine, R, D, frames, g, up).ws_bytes - 1)
    size = lib.nomad_nsim_backward_scratch_bytes
    assert size(0, 2, 19) == 0 and size(4, 65, 19) == 0 and size(4, 2, 3) == 0
    assert size(4, 2, 19) - lib.nomad_nsim_scratch_bytes(4, 2, 19) == 6 * 2 * 19 * 21 * 8
