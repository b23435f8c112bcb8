"""GPU: ``nomad_cdist_backward`` / ``Engine.cdist_backward`` / ``nomad_amd.nomad.cdist`` - the backward of the distance stage.

The contract of include/nomad_hip.h: with d_ij the forward's value and c_ij = gdist_ij + gmean_i / Nb in float64,
W_ij = c_ij / d_ij (exactly 0 where d_ij == 0), da_ik = (float) sum_j fma(W_ij, a_ik - b_jk, acc) with j ascending and one float64
accumulator, db_jk likewise over i; one rounding to fp32, at the store.

Against float64 (numpy, the difference form, zero-distance terms dropped) the bound per element is
``|got - ref64| <= 2^-24 |ref64| + 1e-12 * sum_j |c_ij|`` (db: the sum over i).  The first term is the one fp32 rounding of the
output.  The second is float64 accumulation slack: every term is at most |c_ij| in size (|a_ik - b_jk| <= d_ij), and on the CPU two
float64 summation orders of these very inputs (numpy's einsum; a plain loop, last index first) differ by at most 2.1e-14, never
more than 6e-4 of the slack term of their element, and the fp32-rounded result of one order meets the bound against the other
in every case.  On the GPU the worst share of the bound is 0.997, for a single pair at D = 4: the output's own fp32 rounding.

The rest are conditions on bits: the sums have one order, whatever the grid, so a call repeats itself, a row of da is its own
Na = 1 call, a row of db its own Nb = 1 call, and g_mean is g_dist filled with g_mean_i / Nb.  (For db the Nb = 1 call takes
c's column as g_dist: g_mean_i / Nb depends on Nb.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import guard
from nomad_amd import _lib
from nomad_amd.nomad import cdist as autograd_cdist   # (the package attribute `nomad` is the lazy singleton, not the module)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (63, 65), (65, 130), (130, 63)]
WIDTHS = [4, 36, 256, 768]
UPSTREAMS = ["mean", "dist", "both"]


def _unit(n, d, gen):
    x = torch.randn(n, d, generator=gen, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float()


def _inputs(Na, Nb, D, seed=0, copy=True, near=True):
    """Unit-norm random rows; the last row of b copied bit for bit from the last row of a (d = 0); b_0 about 1e-3 from a_0 (where
    b has a row left for it).  -> a, b, g_dist, g_mean (CPU) and the (i, j) of the copy (or None)."""
    gen = torch.Generator().manual_seed(1000 * seed + 7919 * Na + 31 * Nb + D)
    a, b = _unit(Na, D, gen), _unit(Nb, D, gen)
    zero = None
    if copy:
        b[Nb - 1] = a[Na - 1]
        zero = (Na - 1, Nb - 1)
    if near and (Nb >= 2 or not copy):
        b[0] = a[0] + 1e-3 * _unit(1, D, gen)[0]
    g_dist = torch.randn(Na, Nb, generator=gen, dtype=torch.float64)
    g_mean = torch.randn(Na, generator=gen, dtype=torch.float64)
    return a, b, g_dist, g_mean, zero


def _pick(kind, g_dist, g_mean):
    return (g_dist if kind in ("dist", "both") else None), (g_mean if kind in ("mean", "both") else None)


class _Ref:
    """float64 from the definition: diff and d once per (a, b), then (da, db, row slack, column slack) per upstream."""

    def __init__(self, a, b):
        a, b = a.double().numpy(), b.double().numpy()
        self.diff = a[:, None, :] - b[None, :, :]
        self.d = np.sqrt((self.diff * self.diff).sum(-1))

    def grads(self, g_dist, g_mean):
        Na, Nb = self.d.shape
        c = np.zeros((Na, Nb))
        if g_dist is not None:
            c = c + g_dist.numpy()
        if g_mean is not None:
            c = c + (g_mean.numpy() / Nb)[:, None]
        W = np.divide(c, self.d, out=np.zeros_like(c), where=self.d != 0)
        da = np.einsum("ij,ijk->ik", W, self.diff)
        db = -np.einsum("ij,ijk->jk", W, self.diff)
        return da, db, np.abs(c).sum(1), np.abs(c).sum(0)


def _within(case, got, ref, slack):
    got = got.cpu().double().numpy()
    assert np.isfinite(got).all(), case
    err = np.abs(got - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 1e-12 * slack[:, None]
    print(f"CDIST-BWD {case}: max |got - ref64| {err.max():.3e}, worst share of the bound {(err / bound).max():.3f}, "
          f"smallest slack {1e-12 * slack.min():.1e}")
    assert (err <= bound).all(), f"{case}: {int((err > bound).sum())} of {err.size} elements outside the bound, worst {err.max():.3e}"


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _against_float64(engine, Na, Nb, D, **kw):
    a, b, g_dist, g_mean, zero = _inputs(Na, Nb, D, **kw)
    ref = _Ref(a, b)
    assert zero is None or ref.d[zero] == 0.0
    ad, bd = _cuda(a, b)
    for kind in UPSTREAMS:
        gd, gm = _pick(kind, g_dist, g_mean)
        da, db = engine.cdist_backward(ad, bd, *_cuda(gd, gm), want_a=True, want_b=True)
        assert da.shape == (Na, D) and db.shape == (Nb, D) and da.dtype == db.dtype == torch.float32
        rda, rdb, row_slack, col_slack = ref.grads(gd, gm)
        case = f"{Na} x {Nb} x {D} {kind} {kw or ''}"
        _within(case + " da", da, rda, row_slack)
        _within(case + " db", db, rdb, col_slack)
        if zero is not None and gd is not None:
            # the d = 0 pair contributes exactly nothing: whatever its upstream is, no bit of either output moves
            gd2 = gd.clone()
            gd2[zero] = 1e300
            da2, db2 = engine.cdist_backward(ad, bd, *_cuda(gd2, gm), want_a=True, want_b=True)
            assert torch.equal(da2, da) and torch.equal(db2, db), case


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("Na,Nb", SHAPES)
def test_cdist_backward_against_float64(engine, Na, Nb, D):
    if (Na, Nb) == (1, 1):   # one pair: random, the bit-for-bit copy (every gradient exactly 0) and the near row, each on its own
        _against_float64(engine, 1, 1, D, copy=False, near=False)
        _against_float64(engine, 1, 1, D, copy=True, near=False)
        _against_float64(engine, 1, 1, D, copy=False, near=True)
        a, _, g_dist, g_mean, _ = _inputs(1, 1, D)
        da, db = engine.cdist_backward(*_cuda(a, a.clone(), g_dist, g_mean), want_a=True, want_b=True)
        assert not da.any() and not db.any()
    else:
        _against_float64(engine, Na, Nb, D)


@pytest.mark.parametrize("want_a,want_b", [(True, False), (False, True)])
def test_one_output_alone_has_the_bits_of_both(engine, want_a, want_b):
    a, b, g_dist, g_mean = _cuda(*_inputs(65, 130, 36)[:4])
    da, db = engine.cdist_backward(a, b, g_dist, g_mean, want_a=True, want_b=True)
    oa, ob = engine.cdist_backward(a, b, g_dist, g_mean, want_a=want_a, want_b=want_b)
    assert (oa is None) == (not want_a) and (ob is None) == (not want_b)
    assert torch.equal(oa if want_a else ob, da if want_a else db)


@pytest.mark.parametrize("Na,Nb,D", [(65, 130, 36), (130, 63, 256), (3, 5, 768)])
def test_bits_do_not_depend_on_the_grid(engine, Na, Nb, D):
    a, b, g_dist, g_mean = _cuda(*_inputs(Na, Nb, D)[:4])
    da, db = engine.cdist_backward(a, b, g_dist, g_mean, want_a=True, want_b=True)
    da2, db2 = engine.cdist_backward(a, b, g_dist, g_mean, want_a=True, want_b=True)
    assert torch.equal(da, da2) and torch.equal(db, db2)                      # run to run
    c = g_dist + (g_mean / Nb)[:, None]                                       # float64, the kernel's own two operations
    for i in sorted({0, 1, 62, 63, 64, Na - 1} & set(range(Na))):            # a row of da is the row's own Na = 1 call
        for gd, gm in ((g_dist[i:i + 1].contiguous(), g_mean[i:i + 1].contiguous()), (None, g_mean[i:i + 1].contiguous())):
            whole = da if gd is not None else engine.cdist_backward(a, b, None, g_mean)[0]
            one, _ = engine.cdist_backward(a[i:i + 1].contiguous(), b, gd, gm)
            assert torch.equal(one[0], whole[i]), (i, gd is None)
    db_dist = engine.cdist_backward(a, b, g_dist, None, want_a=False, want_b=True)[1]
    for j in sorted({0, 1, 62, 63, 64, Nb - 1} & set(range(Nb))):            # a row of db is the row's own Nb = 1 call
        bj = b[j:j + 1].contiguous()
        one = engine.cdist_backward(a, bj, g_dist[:, j:j + 1].contiguous(), None, want_a=False, want_b=True)[1]
        assert torch.equal(one[0], db_dist[j]), j
        one = engine.cdist_backward(a, bj, c[:, j:j + 1].contiguous(), None, want_a=False, want_b=True)[1]
        assert torch.equal(one[0], db[j]), j
    # g_mean alone is g_dist filled with g_mean_i / Nb (the division in float64)
    ma, mb = engine.cdist_backward(a, b, None, g_mean, want_a=True, want_b=True)
    fill = (g_mean / Nb)[:, None].expand(Na, Nb).contiguous()
    fa, fb = engine.cdist_backward(a, b, fill, None, want_a=True, want_b=True)
    assert torch.equal(ma, fa) and torch.equal(mb, fb)


@pytest.mark.parametrize("D", WIDTHS)
def test_the_forward_keeps_its_bits(engine, D):
    """The forward shares its chain with the weights kernel; ``paired_distance`` has a kernel of its own: the diagonal still agrees,
    and at D = 256 ``cdist`` is still ``pairwise``."""
    a, b = _cuda(*_inputs(130, 130, D)[:2])
    dist, mean = engine.cdist(a, b)
    assert torch.equal(dist.diagonal(), engine.paired_distance(a, b))
    assert torch.equal(mean, engine.cdist(a, b, want_matrix=False)[1])
    if D == 256:
        dp, mp = engine.pairwise(a, b)
        assert torch.equal(dp, dist) and torch.equal(mp, mean)


def _abi_call(engine, a, b, D, gd, gm, da, db, scratch, nbytes=None, Na=None, Nb=None):
    return engine.lib.nomad_cdist_backward(engine.ctx, a if a is None else a.data_ptr(), a.shape[0] if Na is None else Na,
                                           b if b is None else b.data_ptr(), b.shape[0] if Nb is None else Nb, D,
                                           gd if gd is None else gd.data_ptr(), gm if gm is None else gm.data_ptr(),
                                           da if da is None else da.data_ptr(), db if db is None else db.data_ptr(),
                                           scratch if scratch is None else scratch.data_ptr(),
                                           scratch.numel() if nbytes is None else nbytes, None)


def _scratch_bytes(engine, Na, Nb):
    n = C.c_size_t()
    assert engine.lib.nomad_cdist_backward_scratch_bytes(Na, Nb, C.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("Na,Nb,D", [(65, 130, 36), (3, 5, 768), (130, 63, 256)])
def test_nothing_is_read_that_was_not_written(engine, Na, Nb, D):
    """Outputs and a scratch of exactly nomad_cdist_backward_scratch_bytes between guards, pre-filled with 0xFF bytes and with zeros:
    the same bits, the guards intact."""
    a, b, g_dist, g_mean = _cuda(*_inputs(Na, Nb, D)[:4])
    need = _scratch_bytes(engine, Na, Nb)
    assert need == 8 * Na * Nb
    results = []
    for fill in (0xFF, 0x00):
        guards = guard.Guards()
        da = guards.empty((Na, D), torch.float32, "cuda", name="da")
        db = guards.empty((Nb, D), torch.float32, "cuda", name="db")
        scratch = guards.empty_bytes(need, "cuda", guard.OUT_GUARD, "scratch")
        for t in (da, db, scratch):
            t.view(torch.uint8).fill_(fill)
        assert _abi_call(engine, a, b, D, g_dist, g_mean, da, db, scratch) == 0
        guards.check(f"cdist_backward {Na} x {Nb} x {D} fill {fill:#x}")
        results.append((da.clone(), db.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    ea, eb = engine.cdist_backward(a, b, g_dist, g_mean, want_a=True, want_b=True)
    assert torch.equal(ea, results[0][0]) and torch.equal(eb, results[0][1])


def test_argument_errors_return_their_status_and_write_nothing(engine):
    Na, Nb, D = 5, 7, 36
    a, b, g_dist, g_mean = _cuda(*_inputs(Na, Nb, D)[:4])
    need = _scratch_bytes(engine, Na, Nb)
    da = torch.full((Na, D), 7.0, device="cuda")
    db = torch.full((Nb, D), 7.0, device="cuda")
    scratch = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    base = dict(a=a, b=b, D=D, gd=g_dist, gm=g_mean, da=da, db=db, scratch=scratch)
    INVALID, WORKSPACE = _lib.NOMAD_ERR_INVALID, _lib.NOMAD_ERR_WORKSPACE
    refusals = [("a NULL", dict(a=None, Na=Na), INVALID), ("b NULL", dict(b=None, Nb=Nb), INVALID),
                ("scratch NULL", dict(scratch=None, nbytes=need), INVALID), ("both upstreams NULL", dict(gd=None, gm=None), INVALID),
                ("both outputs NULL", dict(da=None, db=None), INVALID), ("Na = 0", dict(Na=0), INVALID), ("Na < 0", dict(Na=-1), INVALID),
                ("Nb = 0", dict(Nb=0), INVALID), ("Nb < 0", dict(Nb=-3), INVALID), ("D = 0", dict(D=0), INVALID),
                ("D < 0", dict(D=-4), INVALID), ("D % 4", dict(D=6), INVALID), ("D > 4096", dict(D=4100), INVALID),
                ("scratch one byte short", dict(nbytes=need - 1), WORKSPACE), ("no scratch bytes", dict(nbytes=0), WORKSPACE)]
    for what, over, status in refusals:
        assert _abi_call(engine, **{**base, **over}) == status, what
        assert engine.lib.nomad_last_error(), what
    torch.cuda.synchronize()
    assert bool((da == 7.0).all()) and bool((db == 7.0).all()) and bool((scratch == 0x5A).all())
    n = C.c_size_t(123)
    for Na_, Nb_, p in ((0, 5, C.byref(n)), (5, 0, C.byref(n)), (-1, 5, C.byref(n)), (5, 7, None)):
        assert engine.lib.nomad_cdist_backward_scratch_bytes(Na_, Nb_, p) == INVALID
    assert n.value == 123
    # the context is usable afterwards, and the wrapper's own refusals are ValueErrors
    assert _abi_call(engine, **base) == 0
    ea, eb = engine.cdist_backward(a, b, g_dist, g_mean, want_a=True, want_b=True)
    assert torch.equal(ea, da) and torch.equal(eb, db)
    with pytest.raises(ValueError):
        engine.cdist_backward(a, b)
    with pytest.raises(ValueError):
        engine.cdist_backward(a, b, g_dist, want_a=False, want_b=False)
    with pytest.raises(ValueError):
        engine.cdist_backward(a, b, g_dist.float())
    with pytest.raises(ValueError):
        engine.cdist_backward(a, b, None, g_mean[:-1].contiguous())
    with pytest.raises(ValueError):
        engine.cdist_backward(a, b[:, :32].contiguous(), g_dist)


def test_autograd_cdist_is_cdist_and_cdist_backward(engine):
    """``nomad_amd.nomad.cdist``: the values of ``Engine.cdist``; autograd's gradients are ``Engine.cdist_backward``'s, bit for bit."""
    Na, Nb, D = 65, 130, 36
    a, b, g_dist, g_mean = _cuda(*_inputs(Na, Nb, D)[:4])
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    dist, mean = autograd_cdist(engine, ar, br)
    d0, m0 = engine.cdist(a, b)
    assert torch.equal(dist, d0) and torch.equal(mean, m0)
    ((dist * g_dist).sum() + (mean * g_mean).sum()).backward()
    da, db = engine.cdist_backward(a, b, g_dist, g_mean, want_a=True, want_b=True)
    assert torch.equal(ar.grad, da) and torch.equal(br.grad, db)
    # one output used, one input differentiated
    ar2 = a.clone().requires_grad_(True)
    autograd_cdist(engine, ar2, b)[1].sum().backward()
    assert torch.equal(ar2.grad, engine.cdist_backward(a, b, None, torch.ones(Na, dtype=torch.float64, device="cuda"))[0])
