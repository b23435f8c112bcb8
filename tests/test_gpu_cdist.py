"""GPU: ``Engine.cdist`` / ``Engine.paired_distance`` (nomad_cdist, nomad_paired_distance): distances for rows of any width.

The arithmetic contract of include/nomad_hip.h - per pair ONE float64 accumulator, e = a_k - b_k, acc = fma(e, e, acc), k
ascending, sqrt; row sums per 64-column tile in column order, tiles in order - makes two of the checks conditions on bits, not
measurements: at D = 256 ``cdist`` is ``pairwise``, and ``paired_distance`` is the diagonal of ``cdist``.

Against numpy float64 in the difference form (``O.pairwise``) the bound is ``rel * max(1, want)`` with rel = 1e-13 up to
D = 768 (the bound tests/test_gpu_parity.py uses at D = 256) and (D + 2) * 2^-53 at D = 1000 and 4096 (1.1e-13, 4.5e-13): each
side's squared sum carries at most (D + 2) * 2^-53 relative error, the square root halves it, and the two sides together stay
below that figure."""
import ctypes as C

import numpy as np
import pytest
import torch

import guard
from nomad_amd import _lib
from oracle import nomad_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (64, 64), (65, 130), (1000, 257)]
WIDTHS = [4, 60, 256, 768, 1000, 4096]


def _rows(n, d, seed):
    g = torch.Generator().manual_seed(seed * 7919 + n * 31 + d)
    return torch.randn(n, d, generator=g)


def _rel(d):
    return 1e-13 if d <= 768 else (d + 2) * 2.0 ** -53


def _oracle(a, b):
    """O.pairwise in slabs of rows of ``a`` (its broadcast difference is Na x Nb x D doubles)."""
    a, b = a.double().numpy(), b.double().numpy()
    step = max(1, (1 << 25) // (b.shape[0] * b.shape[1]))
    parts = [O.pairwise(a[i:i + step], b) for i in range(0, a.shape[0], step)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _close(case, got, want, rel):
    err = np.abs(got - want)
    bound = rel * np.maximum(1.0, want)
    print(f"CDIST {case}: max |got - want| {err.max():.3e}, worst share of the bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), f"{case}: {int((err > bound).sum())} of {err.size} outside {rel:.2e} * max(1, want), worst {err.max():.3e}"


@pytest.mark.parametrize("Na,Nb", SHAPES)
def test_cdist_at_256_is_pairwise(engine, Na, Nb):
    a, b = _rows(Na, 256, 1).cuda(), _rows(Nb, 256, 2).cuda()
    dp, mp = engine.pairwise(a, b)
    dc, mc = engine.cdist(a, b)
    _, mo = engine.cdist(a, b, want_matrix=False)
    torch.cuda.synchronize()
    assert torch.equal(dc, dp) and torch.equal(mc, mp) and torch.equal(mo, mp)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("Na,Nb", SHAPES)
def test_cdist_against_float64(engine, Na, Nb, D):
    a, b = _rows(Na, D, 3), _rows(Nb, D, 4)
    dist, mean = engine.cdist(a.cuda(), b.cuda())
    want_d, want_m = _oracle(a, b)
    case = f"cdist {Na} x {Nb} x {D}"
    _close(case + " dist", dist.cpu().numpy(), want_d, _rel(D))
    _close(case + " mean", mean.cpu().numpy(), want_m, _rel(D))


@pytest.mark.parametrize("D", [256, 768])
def test_cdist_of_equal_and_of_near_rows(engine, D):
    """b = a: exact zeros on the diagonal.  Rows 1e-3 apart: what the difference form exists for (the expansion
    |a|^2 + |b|^2 - 2 a.b loses ~4e-5 absolute there in fp32)."""
    a = _rows(130, D, 5)
    dist, mean = engine.cdist(a.cuda(), a.cuda())
    want_d, want_m = _oracle(a, a)
    assert bool((dist.diagonal() == 0).all())
    _close(f"cdist b = a D={D} dist", dist.cpu().numpy(), want_d, _rel(D))
    _close(f"cdist b = a D={D} mean", mean.cpu().numpy(), want_m, _rel(D))
    near = (a + 1e-3 * _rows(130, D, 6) / D ** 0.5).float()
    dist, mean = engine.cdist(near.cuda(), a.cuda())
    want_d, want_m = _oracle(near, a)
    assert want_d.diagonal().max() < 2e-3
    _close(f"cdist near rows D={D} dist", dist.cpu().numpy(), want_d, _rel(D))
    _close(f"cdist near rows D={D} mean", mean.cpu().numpy(), want_m, _rel(D))
    assert torch.equal(engine.paired_distance(near.cuda(), a.cuda()), dist.diagonal())


@pytest.mark.parametrize("D", [256, 768])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_paired_distance_is_the_diagonal(engine, N, D):
    a, b = _rows(N, D, 7).cuda(), _rows(N, D, 8).cuda()
    got = engine.paired_distance(a, b)
    diag = engine.cdist(a, b)[0].diagonal()
    torch.cuda.synchronize()
    assert torch.equal(got, diag)


def test_bad_arguments_return_status_and_leave_the_context_usable(engine):
    lib, inv = engine.lib, _lib.NOMAD_ERR_INVALID
    a, b = _rows(8, 256, 9).cuda(), _rows(8, 256, 10).cuda()
    before = [t.clone() for t in engine.pairwise(a, b)]
    wide = torch.zeros(8, 4100, device="cuda")
    dist = torch.full((8, 8), 7.0, dtype=torch.float64, device="cuda")
    mean = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    pa, pb, pw, pd, pm = a.data_ptr(), b.data_ptr(), wide.data_ptr(), dist.data_ptr(), mean.data_ptr()
    for D in (6, 0, 4100, -4):
        assert lib.nomad_cdist(engine.ctx, pw, 8, pw, 8, D, pd, pm, None) == inv, D
        assert b"nomad_cdist" in lib.nomad_last_error()
        assert lib.nomad_paired_distance(engine.ctx, pw, pw, 8, D, pm, None) == inv, D
        assert b"nomad_paired_distance" in lib.nomad_last_error()
    assert lib.nomad_cdist(engine.ctx, pa, 0, pb, 8, 256, pd, pm, None) == inv
    assert lib.nomad_cdist(engine.ctx, pa, 8, pb, 0, 256, pd, pm, None) == inv
    assert lib.nomad_cdist(engine.ctx, None, 8, pb, 8, 256, pd, pm, None) == inv
    assert lib.nomad_cdist(engine.ctx, pa, 8, None, 8, 256, pd, pm, None) == inv
    assert lib.nomad_cdist(engine.ctx, pa, 8, pb, 8, 256, pd, None, None) == inv
    assert lib.nomad_cdist(None, pa, 8, pb, 8, 256, pd, pm, None) == inv
    assert lib.nomad_paired_distance(engine.ctx, pa, pb, 0, 256, pm, None) == inv
    assert lib.nomad_paired_distance(engine.ctx, None, pb, 8, 256, pm, None) == inv
    assert lib.nomad_paired_distance(engine.ctx, pa, None, 8, 256, pm, None) == inv
    assert lib.nomad_paired_distance(engine.ctx, pa, pb, 8, 256, None, None) == inv
    with pytest.raises(_lib.NomadHipError, match="nomad_cdist"):
        engine.cdist(torch.zeros(4, 6, device="cuda"), torch.zeros(4, 6, device="cuda"))
    torch.cuda.synchronize()
    assert bool((dist == 7.0).all()) and bool((mean == 7.0).all())      # nothing was launched
    after = engine.pairwise(a, b)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    # a NULL matrix is legal: means only
    assert lib.nomad_cdist(engine.ctx, pa, 8, pb, 8, 256, None, pm, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(mean, before[1])


@pytest.mark.parametrize("D", [256, 768, 60])
@pytest.mark.parametrize("Na,Nb", [(5, 3), (65, 131), (130, 257)])
def test_inside_guards_with_odd_widths(engine, Na, Nb, D):
    """Odd Nb: the tile kernel's unaligned store path.  Outputs of exactly their size between guard bytes."""
    a, b = _rows(Na, D, 11), _rows(Nb, D, 12)
    c = _rows(Na, D, 13)
    case = f"guarded cdist {Na} x {Nb} x {D}"
    with guard.guarded(case=case):
        dist, mean = engine.cdist(a.cuda(), b.cuda())
        _, mean_only = engine.cdist(a.cuda(), b.cuda(), want_matrix=False)
        pd = engine.paired_distance(a.cuda(), c.cuda())
        torch.cuda.synchronize()
    want_d, want_m = _oracle(a, b)
    _close(case + " dist", dist.cpu().numpy(), want_d, _rel(D))
    _close(case + " mean", mean.cpu().numpy(), want_m, _rel(D))
    assert torch.equal(mean_only, mean)
    _close(case + " paired", pd.cpu().numpy(), np.sqrt(((a.double() - c.double()) ** 2).sum(1).numpy()), _rel(D))
