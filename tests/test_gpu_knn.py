"""GPU: ``nomad_knn`` / ``nomad_knn_backward`` (``Engine.knn`` / ``Engine.knn_backward``) and the nearest-reference scores built on
them (``Nomad.score*(k=...)``, ``predict(k=...)``).

The forward's contract (include/nomad_hip.h) is held bit for bit: the distances are ``Engine.cdist``'s, the selection, its order and
the score are those of ``knn_ref`` on that matrix (stable sort with NaN as +inf, sequential float64 sum) - so the reference of the
forward tests is ``Engine.cdist`` + ``knn_ref``, computed once per shape.  The backward is BY DEFINITION ``Engine.cdist_backward`` fed
the dense upstream of the selected pairs, so that is its bitwise reference; one check is independent of the engine - float64
autograd through ``torch.cdist`` -> ``topk`` -> ``mean`` on inputs without ties - under the bound of
``test_gpu_cdist_backward.py``, restated here:

    |got - ref64| <= 2^-24 |ref64| + 1e-12 * (sum of |c| over the element's row of the dense upstream; db: its column)

The first term is the output's one rounding to fp32, the second float64 accumulation slack: every term of an output element is at
most |c_ij| in size (|a_ik - b_jk| <= d_ij), and two float64 summation orders of such sums differ by far less than 1e-12 of it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import guard
from conftest import GOLD
from knn_ref import knn_ref, same
from nomad_amd import _lib

pytestmark = pytest.mark.gpu

FORWARD_SHAPES = [(1, 1, 256, 1), (3, 5, 768, 5), (65, 130, 36, 7), (130, 63, 256, 63), (5, 64, 256, 64), (4, 200, 256, 64)]
BACKWARD_SHAPES = [(65, 130, 36, 7), (3, 5, 768, 5), (130, 63, 256, 3)]


def _unit(n, d, gen):
    x = torch.randn(n, d, generator=gen, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float()


def _inputs(Na, Nb, D, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + 7919 * Na + 31 * Nb + D)
    return _unit(Na, D, gen).cuda(), _unit(Nb, D, gen).cuda()


def _check_forward(engine, a, b, k, case):
    """``Engine.knn`` against ``Engine.cdist`` + ``knn_ref``; -> (knn_dist, knn_idx, score)."""
    dist, _ = engine.cdist(a, b)
    rd, ri, rs = knn_ref(dist, k)
    kd, ki, sc = engine.knn(a, b, k)
    assert kd.shape == (a.shape[0], k) and kd.dtype == torch.float64 and ki.shape == kd.shape and ki.dtype == torch.int32
    assert sc.shape == (a.shape[0],) and sc.dtype == torch.float64
    assert int(ki.min()) >= 0 and int(ki.max()) < b.shape[0], case
    srt = ki.sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), f"{case}: an index appears twice in a row"
    assert torch.equal(ki, ri), f"{case}: {int((ki != ri).sum())} indices differ"
    assert same(kd, rd) and same(sc, rs), case
    return kd, ki, sc


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Na,Nb,D,k", FORWARD_SHAPES)
def test_forward_is_cdist_and_the_helper(engine, Na, Nb, D, k):
    a, b = _inputs(Na, Nb, D)
    _check_forward(engine, a, b, k, f"{Na} x {Nb} x {D} k={k}")
    if k > 1:
        _check_forward(engine, a, b, 1, f"{Na} x {Nb} x {D} k=1")


def test_the_last_tile_holds_one_real_column_and_63_clones(engine):
    """Nb = 65: the chain stages columns 65 .. 127 as copies of row 64 - of the nearest reference of every row.  Excluded by index:
    column 64 comes first and exactly once."""
    Na, Nb, D, k = 7, 65, 256, 3
    gen = torch.Generator().manual_seed(65)
    centre = _unit(1, D, gen)
    a = centre + 0.05 * _unit(Na, D, gen)
    a = (a / a.norm(dim=1, keepdim=True)).cuda()
    b = _unit(Nb, D, gen)
    b[64] = centre[0]
    b = b.cuda()
    _, ki, _ = _check_forward(engine, a, b, k, "7 x 65 planted")
    assert bool((ki[:, 0] == 64).all()) and bool(((ki == 64).sum(1) == 1).all())
    _, ki, _ = _check_forward(engine, a, b, 64, "7 x 65 planted, k = 64")
    assert bool((ki[:, 0] == 64).all()) and bool(((ki == 64).sum(1) == 1).all())


# ---- 2. ties and zeros -----------------------------------------------------------------------------------------------------------
def test_ties_resolve_to_the_lower_index_and_a_copy_is_at_distance_zero(engine):
    Na, Nb, D = 9, 130, 256
    a, b = _inputs(Na, Nb, D, seed=2)
    b[5] = b[3]        # inside one tile
    b[70] = b[3]       # across tiles
    b[129] = b[64]     # across tiles, into the short last tile
    a[0] = b[10]       # a row of a equal to a reference
    a[8] = b[3]        # ... to a duplicated one: three zeros
    for k in (1, 4, 64):
        kd, ki, sc = _check_forward(engine, a, b, k, f"ties k={k}")
        assert int(ki[0, 0]) == 10 and float(kd[0, 0]) == 0.0
        assert int(ki[8, 0]) == 3 and float(kd[8, 0]) == 0.0
        if k >= 4:
            assert ki[8, :3].tolist() == [3, 5, 70] and kd[8, :3].tolist() == [0.0, 0.0, 0.0] and float(kd[8, 3]) > 0.0
    _, ki, _ = engine.knn(a, b, 64)
    full = engine.knn(a, b[:64].contiguous(), 64)[1]                  # k = Nb: the stable argsort of the matrix row
    assert torch.equal(full, torch.sort(engine.cdist(a, b[:64].contiguous())[0], dim=1, stable=True).indices.int())
    for i in range(1, 8):                                              # wherever 3 is selected, 5 and 70 follow it directly
        row = ki[i].tolist()
        if 3 in row and row.index(3) + 2 < 64:
            at = row.index(3)
            assert row[at:at + 3] == [3, 5, 70], (i, row)


# ---- 3. NaN ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Na,Nb,D,k", [(5, 66, 36, 64), (5, 40, 256, 40), (67, 130, 256, 5)])
def test_nan_and_inf_rows_are_ordered_as_the_helper_orders_them(engine, Na, Nb, D, k):
    a, b = _inputs(Na, Nb, D, seed=3)
    a[2] = float("nan")                # every distance of row 2 is NaN: its neighbours are columns 0 .. k - 1
    b[7] = float("nan")                # column 7 is NaN for every row: behind every finite column
    b[Nb - 1, 0] = float("nan")        # ... and so is the last column, in the short last tile
    a[1, 0] = float("inf")             # row 1: +inf against finite rows, NaN against the NaN rows - ties of the key, by index
    kd, ki, sc = _check_forward(engine, a, b, k, f"NaN {Na} x {Nb} x {D} k={k}")
    assert ki[2].tolist() == list(range(k)) and bool(torch.isnan(kd[2]).all()) and bool(torch.isnan(sc[2]))
    assert ki[1].tolist() == list(range(k)) and bool(torch.isinf(kd[1, 0]))
    if k == Nb:
        assert ki[0, -2:].tolist() == [7, Nb - 1] and bool(torch.isnan(kd[0, -2:]).all())
    else:
        assert not bool(torch.isnan(kd[0]).any())


# ---- 4. grid independence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,k", [(256, 7), (36, 64)])
def test_a_row_has_the_bits_of_its_own_call_with_and_without_the_matrix(engine, D, k):
    Na, Nb = 130, 200
    a, b = _inputs(Na, Nb, D, seed=4)
    kd, ki, sc = engine.knn(a, b, k)
    kd2, ki2, sc2 = engine.knn(a, b, k)
    assert torch.equal(kd, kd2) and torch.equal(ki, ki2) and torch.equal(sc, sc2)                 # run to run
    for lo, hi in ((0, 1), (129, 130), (60, 71)):
        sd_, si_, ss_ = engine.knn(a[lo:hi].contiguous(), b, k)
        assert torch.equal(sd_, kd[lo:hi]) and torch.equal(si_, ki[lo:hi]) and torch.equal(ss_, sc[lo:hi]), (lo, hi)
    md, mi, ms, dist = engine.knn(a, b, k, want_matrix=True)
    assert torch.equal(md, kd) and torch.equal(mi, ki) and torch.equal(ms, sc)
    assert torch.equal(dist, engine.cdist(a, b)[0])
    if D == 256:
        assert torch.equal(dist, engine.pairwise(a, b)[0])


# ---- 5. nothing is read that was not written -------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def _knn_call(engine, a, b, D, k, dist, kd, ki, sc, scratch, nbytes=None, Na=None, Nb=None):
    return engine.lib.nomad_knn(engine.ctx, _ptr(a), a.shape[0] if Na is None else Na, _ptr(b), b.shape[0] if Nb is None else Nb, D, k,
                                _ptr(dist), _ptr(kd), _ptr(ki), _ptr(sc), _ptr(scratch), scratch.numel() if nbytes is None else nbytes, None)


def _bwd_call(engine, a, b, D, k, ki, gk, gs, da, db, scratch, nbytes=None, Na=None, Nb=None):
    return engine.lib.nomad_knn_backward(engine.ctx, _ptr(a), a.shape[0] if Na is None else Na, _ptr(b), b.shape[0] if Nb is None else Nb,
                                         D, k, _ptr(ki), _ptr(gk), _ptr(gs), _ptr(da), _ptr(db), _ptr(scratch),
                                         scratch.numel() if nbytes is None else nbytes, None)


def _bytes(fn, Na, Nb, k):
    n = C.c_size_t()
    assert fn(Na, Nb, k, C.byref(n)) == 0
    return n.value


def _upstreams(Na, k, seed=0):
    gen = torch.Generator().manual_seed(99 + seed)
    return (torch.randn(Na, k, generator=gen, dtype=torch.float64).cuda(), torch.randn(Na, generator=gen, dtype=torch.float64).cuda())


@pytest.mark.parametrize("Na,Nb,D,k", [(65, 130, 36, 7), (3, 5, 768, 5), (4, 200, 256, 64)])
def test_nothing_is_read_that_was_not_written(engine, Na, Nb, D, k):
    """Outputs and scratch of exactly the reported sizes between guards, pre-filled with 0xFF bytes (NaN) and with zeros: the same
    bits as ``Engine.knn`` / ``Engine.knn_backward``, the guards intact."""
    a, b = _inputs(Na, Nb, D, seed=5)
    ekd, eki, esc, edist = engine.knn(a, b, k, want_matrix=True)
    gk, gs = _upstreams(Na, k)
    eda, edb = engine.knn_backward(a, b, eki, gk, gs)
    need = _bytes(engine.lib.nomad_knn_scratch_bytes, Na, Nb, k)
    need_b = _bytes(engine.lib.nomad_knn_backward_scratch_bytes, Na, Nb, k)
    assert need == ((Nb + 63) // 64) * Na * k * 12 and need_b == 2 * 8 * Na * Nb
    for fill in (0xFF, 0x00):
        for with_matrix in (False, True):
            guards = guard.Guards()
            kd = guards.empty((Na, k), torch.float64, "cuda", name="knn_dist")
            ki = guards.empty((Na, k), torch.int32, "cuda", name="knn_idx")
            sc = guards.empty((Na,), torch.float64, "cuda", name="score")
            dist = guards.empty((Na, Nb), torch.float64, "cuda", name="dist") if with_matrix else None
            scratch = guards.empty_bytes(need, "cuda", guard.OUT_GUARD, "scratch")
            for t in (kd, ki, sc, dist, scratch):
                if t is not None:
                    t.view(torch.uint8).fill_(fill)
            assert _knn_call(engine, a, b, D, k, dist, kd, ki, sc, scratch) == 0
            guards.check(f"knn {Na} x {Nb} x {D} k={k} fill {fill:#x}")
            assert torch.equal(kd, ekd) and torch.equal(ki, eki) and torch.equal(sc, esc)
            assert dist is None or torch.equal(dist, edist)
        guards = guard.Guards()
        da = guards.empty((Na, D), torch.float32, "cuda", name="da")
        db = guards.empty((Nb, D), torch.float32, "cuda", name="db")
        scratch = guards.empty_bytes(need_b, "cuda", guard.OUT_GUARD, "scratch")
        for t in (da, db, scratch):
            t.view(torch.uint8).fill_(fill)
        assert _bwd_call(engine, a, b, D, k, eki, gk, gs, da, db, scratch) == 0
        guards.check(f"knn_backward {Na} x {Nb} x {D} k={k} fill {fill:#x}")
        assert torch.equal(da, eda) and torch.equal(db, edb)


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors_return_their_status_and_write_nothing(engine):
    Na, Nb, D, k = 5, 7, 36, 3
    a, b = _inputs(Na, Nb, D, seed=6)
    gk, gs = _upstreams(Na, k)
    need = _bytes(engine.lib.nomad_knn_scratch_bytes, Na, Nb, k)
    need_b = _bytes(engine.lib.nomad_knn_backward_scratch_bytes, Na, Nb, k)
    kd = torch.full((Na, k), 7.0, dtype=torch.float64, device="cuda")
    ki = torch.full((Na, k), 7, dtype=torch.int32, device="cuda")
    sc = torch.full((Na,), 7.0, dtype=torch.float64, device="cuda")
    dist = torch.full((Na, Nb), 7.0, dtype=torch.float64, device="cuda")
    da = torch.full((Na, D), 7.0, device="cuda")
    db = torch.full((Nb, D), 7.0, device="cuda")
    scratch = torch.full((max(need, need_b),), 0x5A, dtype=torch.uint8, device="cuda")
    INVALID, WORKSPACE = _lib.NOMAD_ERR_INVALID, _lib.NOMAD_ERR_WORKSPACE
    sizes = [("Na = 0", dict(Na=0)), ("Na < 0", dict(Na=-1)), ("Na above the limit", dict(Na=65535 * 64 + 1)), ("Nb = 0", dict(Nb=0)),
             ("Nb < 0", dict(Nb=-3)), ("Nb above the limit", dict(Nb=65535 * 64 + 1)), ("D = 0", dict(D=0)), ("D < 0", dict(D=-4)),
             ("D % 4", dict(D=6)), ("D > 4096", dict(D=4100)), ("k = 0", dict(k=0)), ("k < 0", dict(k=-1)), ("k > 64", dict(k=65, Nb=100)),
             ("k > Nb", dict(k=8))]
    base = dict(a=a, b=b, D=D, k=k, dist=dist, kd=kd, ki=ki, sc=sc, scratch=scratch, nbytes=need)
    refusals = [("a NULL", dict(a=None, Na=Na), INVALID), ("b NULL", dict(b=None, Nb=Nb), INVALID), ("knn_dist NULL", dict(kd=None), INVALID),
                ("knn_idx NULL", dict(ki=None), INVALID), ("score NULL", dict(sc=None), INVALID),
                ("scratch NULL", dict(scratch=None), INVALID)] + [(w, o, INVALID) for w, o in sizes] + [
                ("scratch one byte short", dict(nbytes=need - 1), WORKSPACE), ("no scratch bytes", dict(nbytes=0), WORKSPACE)]
    for what, over, status in refusals:
        assert _knn_call(engine, **{**base, **over}) == status, what
        assert engine.lib.nomad_last_error(), what
    idx = engine.knn(a, b, k)[1]
    base_b = dict(a=a, b=b, D=D, k=k, ki=idx, gk=gk, gs=gs, da=da, db=db, scratch=scratch, nbytes=need_b)
    refusals = [("a NULL", dict(a=None, Na=Na), INVALID), ("b NULL", dict(b=None, Nb=Nb), INVALID), ("knn_idx NULL", dict(ki=None), INVALID),
                ("scratch NULL", dict(scratch=None), INVALID), ("both upstreams NULL", dict(gk=None, gs=None), INVALID),
                ("both outputs NULL", dict(da=None, db=None), INVALID)] + [(w, o, INVALID) for w, o in sizes] + [
                ("scratch one byte short", dict(nbytes=need_b - 1), WORKSPACE), ("no scratch bytes", dict(nbytes=0), WORKSPACE)]
    for what, over, status in refusals:
        assert _bwd_call(engine, **{**base_b, **over}) == status, what
        assert engine.lib.nomad_last_error(), what
    torch.cuda.synchronize()
    for t in (kd, sc, dist, da, db):
        assert bool((t == 7.0).all())
    assert bool((ki == 7).all()) and bool((scratch == 0x5A).all())
    # the context is usable afterwards, and the wrapper's own refusals are ValueErrors
    assert _knn_call(engine, **base) == 0 and _bwd_call(engine, **base_b) == 0
    ekd, eki, esc, edist = engine.knn(a, b, k, want_matrix=True)
    assert torch.equal(kd, ekd) and torch.equal(ki, eki) and torch.equal(sc, esc) and torch.equal(dist, edist)
    eda, edb = engine.knn_backward(a, b, idx, gk, gs)
    assert torch.equal(da, eda) and torch.equal(db, edb)
    for bad_k in (0, 8, 65, 2.0, True):
        with pytest.raises(ValueError):
            engine.knn(a, b, bad_k)
    with pytest.raises(ValueError):
        engine.knn(a, b[:, :32].contiguous(), k)
    for bad_idx in (idx.long(), idx.cpu(), idx.t(), idx[:-1].contiguous(), idx.flatten()):
        with pytest.raises(ValueError):
            engine.knn_backward(a, b, bad_idx, gk, gs)
    with pytest.raises(ValueError):
        engine.knn_backward(a, b, idx)
    with pytest.raises(ValueError):
        engine.knn_backward(a, b, idx, gk, gs, want_a=False, want_b=False)
    with pytest.raises(ValueError):
        engine.knn_backward(a, b, idx, gk.float(), gs)
    with pytest.raises(ValueError):
        engine.knn_backward(a, b, idx, None, gs[:-1].contiguous())


# ---- 7. backward -----------------------------------------------------------------------------------------------------------------
def _dense(idx, Nb, gk, gs):
    """The dense upstream of the definition: c_ir = g_knn_ir + g_score_i / k at (i, knn_idx[i][r]), 0 elsewhere; float64."""
    Na, k = idx.shape
    c = torch.zeros(Na, k, dtype=torch.float64, device=idx.device)
    if gk is not None:
        c = c + gk
    if gs is not None:
        c = c + (gs / torch.full_like(gs, float(k)))[:, None]      # the quotient (a Python divisor becomes a product on the GPU)
    return torch.zeros(Na, Nb, dtype=torch.float64, device=idx.device).scatter_(1, idx.long(), c)


@pytest.mark.parametrize("Na,Nb,D,k", BACKWARD_SHAPES)
def test_backward_is_cdist_backward_of_the_dense_upstream(engine, Na, Nb, D, k):
    a, b = _inputs(Na, Nb, D, seed=7)
    if Nb > 10:
        a[0] = b[10]                   # a neighbour at distance 0
    kd, idx, _ = engine.knn(a, b, k)
    assert Nb <= 10 or (int(idx[0, 0]) == 10 and float(kd[0, 0]) == 0.0)
    gk, gs = _upstreams(Na, k, seed=Na)
    for ugk, ugs in ((gk, None), (None, gs), (gk, gs)):
        dense = _dense(idx, Nb, ugk, ugs)
        rda, rdb = engine.cdist_backward(a, b, dense, None, want_a=True, want_b=True)
        da, db = engine.knn_backward(a, b, idx, ugk, ugs)
        assert da.dtype == db.dtype == torch.float32 and da.shape == a.shape and db.shape == b.shape
        assert torch.equal(da, rda) and torch.equal(db, rdb), (ugk is None, ugs is None)
        assert bool(torch.isfinite(da).all()) and bool(torch.isfinite(db).all())
        oa, none = engine.knn_backward(a, b, idx, ugk, ugs, want_a=True, want_b=False)        # one output alone
        assert none is None and torch.equal(oa, da)
        none, ob = engine.knn_backward(a, b, idx, ugk, ugs, want_a=False, want_b=True)
        assert none is None and torch.equal(ob, db)
    if Nb > 10:   # the pair at distance 0 adds nothing: whatever its upstream is, no bit of either output moves
        gk2 = gk.clone()
        gk2[0, 0] = 1e300
        da2, db2 = engine.knn_backward(a, b, idx, gk2, gs)
        assert torch.equal(da2, da) and torch.equal(db2, db)
    # an index outside 0 .. Nb - 1 is skipped: the gradients of the remaining pairs
    bad = idx.clone()
    bad[0, 0], bad[-1, -1] = -1, Nb
    dense = _dense(idx, Nb, gk, None)
    dense[0, idx[0, 0]] = 0.0
    dense[-1, idx[-1, -1]] = 0.0
    rda, rdb = engine.cdist_backward(a, b, dense, None, want_a=True, want_b=True)
    da, db = engine.knn_backward(a, b, bad, gk, None)
    assert torch.equal(da, rda) and torch.equal(db, rdb)


@pytest.mark.parametrize("Na,Nb,D,k", BACKWARD_SHAPES)
def test_score_gradient_against_float64_autograd(engine, Na, Nb, D, k):
    """Independent of the engine: d (sum_i up_i score_i) / d a and / d b through torch.cdist (float64, difference form) -> topk ->
    mean, on random unit rows (no ties: the selection is the same set, in the same order)."""
    a, b = _inputs(Na, Nb, D, seed=8)
    up = _upstreams(Na, k, seed=8)[1]
    _, idx, sc = engine.knn(a, b, k)
    da, db = engine.knn_backward(a, b, idx, g_score=up)
    a64 = a.cpu().double().requires_grad_(True)
    b64 = b.cpu().double().requires_grad_(True)
    d64 = torch.cdist(a64, b64, compute_mode="donot_use_mm_for_euclid_dist")
    top = torch.topk(d64, k, dim=1, largest=False, sorted=True)
    assert torch.equal(top.indices, idx.cpu().long()), "the float64 selection differs: the inputs have a near tie"
    score64 = top.values.mean(1)
    assert float((sc.cpu() - score64.detach()).abs().max()) <= 1e-14
    (score64 * up.cpu()).sum().backward()
    c = torch.zeros(Na, Nb, dtype=torch.float64).scatter_(1, idx.cpu().long(), (up.cpu().abs() / k)[:, None].expand(Na, k).contiguous())
    for name, got, ref, slack in (("da", da, a64.grad, c.sum(1)), ("db", db, b64.grad, c.sum(0))):
        err = (got.cpu().double() - ref).abs()
        bound = 2.0 ** -24 * ref.abs() + 1e-12 * slack[:, None]
        share = float((err / bound.clamp_min(1e-300)).max())
        print(f"KNN-BWD {Na} x {Nb} x {D} k={k} {name}: max |got - ref64| {float(err.max()):.3e}, worst share of the bound {share:.3f}")
        assert bool((err <= bound).all()), f"{name}: {int((err > bound).sum())} of {err.numel()} elements outside the bound"


# ---- 8. through Nomad ------------------------------------------------------------------------------------------------------------
K, NR = 3, 70
LENGTHS = [4000, 6000, 5000]


@pytest.fixture(scope="module")
def nmd(engine):
    from nomad_amd.nomad import Nomad
    return Nomad.from_engine(engine)


@pytest.fixture(scope="module")
def clips():
    gen = torch.Generator().manual_seed(31)
    wav = (0.1 * torch.randn(3, 1, 6000, generator=gen)).clamp(-1, 1).cuda()
    refs = _unit(NR, 256, gen).cuda()
    up = torch.randn(3, generator=gen, dtype=torch.float64).cuda()
    return wav, refs, up


@pytest.mark.parametrize("lengths", [None, LENGTHS], ids=["uniform", "lengths"])
def test_score_with_k_is_its_composition(engine, nmd, clips, lengths):
    wav, refs, up = clips
    est = wav.squeeze(1)
    with torch.no_grad():
        got = nmd.score(wav, refs, lengths=lengths, k=K)
        all_refs = nmd.score(wav, refs, lengths=lengths)
    emb = nmd._score_embed(est, lengths)
    assert torch.equal(got, engine.knn(emb, refs, K)[2])
    assert torch.equal(all_refs, engine.pairwise(emb, refs, want_matrix=False)[1])               # k=None: the bits of before
    assert bool((got < all_refs).all())
    kd, ki = nmd.nearest_references(wav, refs, K, lengths=lengths)
    ed, ei, _ = engine.knn(emb, refs, K)
    assert torch.equal(kd, ed) and torch.equal(ki, ei)
    kd, ki = nmd.nearest_references(emb, refs, K)
    assert torch.equal(kd, ed) and torch.equal(ki, ei)
    # with a gradient: the training forward's value, and the gradients of the composition, bit for bit
    w = wav.clone().requires_grad_(True)
    r = refs.clone().requires_grad_(True)
    s = nmd.score(w, r, lengths=lengths, k=K)
    (s * up).sum().backward()
    if lengths is None:
        temb, layers, saved = engine.embed_train(est)
    else:
        temb, layers, saved, batch = engine.embed_train_ragged(est, lengths)
    _, idx, ts = engine.knn(temb, refs, K)
    assert torch.equal(s.detach(), ts)
    demb, dref = engine.knn_backward(temb, refs, idx, g_score=up, want_a=True, want_b=True)
    if lengths is None:
        dwav = engine.embed_backward(est, layers, saved, None, demb)
    else:
        dwav = engine.embed_backward_ragged(batch, layers, saved, None, demb)
    assert torch.equal(w.grad, dwav.reshape(w.shape)) and torch.equal(r.grad, dref)
    assert bool(w.grad.abs().sum() > 0) and int((r.grad.abs().sum(1) > 0).sum()) <= 3 * K
    if lengths is not None:
        for i, n in enumerate(lengths):
            assert not bool(w.grad[i, 0, n:].any())
    # only the references differentiated: the scoring forward, then knn_backward's db alone
    r2 = refs.clone().requires_grad_(True)
    s2 = nmd.score(wav, r2, lengths=lengths, k=K)
    (s2 * up).sum().backward()
    assert torch.equal(s2.detach(), got)
    assert torch.equal(r2.grad, engine.knn_backward(emb, refs, engine.knn(emb, refs, K)[1], g_score=up, want_a=False, want_b=True)[1])


@pytest.mark.parametrize("lengths", [None, LENGTHS], ids=["uniform", "lengths"])
def test_window_scores_with_k_are_their_compositions(engine, nmd, clips, lengths):
    from nomad_amd.nomad import window_frames
    wav, refs, up = clips
    est = wav.squeeze(1)
    win, hop = window_frames(0.1, 0.06)
    with torch.no_grad():
        got, counts = nmd.score_over_time(wav, refs, 0.1, 0.06, lengths=lengths, k=K)
        got_w, counts_w = nmd.score_windows(wav, refs, 0.1, 0.06, lengths=lengths, k=K)
    if lengths is None:
        emb, ecounts = engine.embed_windows(est, win, hop)
    else:
        emb, ecounts = engine.embed_windows_ragged([est[i, :n] for i, n in enumerate(lengths)], win, hop)
    assert counts == ecounts == counts_w and torch.equal(got, engine.knn(emb, refs, K)[2]) and torch.equal(got_w, got)
    with pytest.raises(ValueError, match="no gradient"):
        nmd.score_over_time(wav.clone().requires_grad_(True), refs, 0.1, 0.06, k=K)
    gen = torch.Generator().manual_seed(5)
    upw = torch.randn(sum(counts), generator=gen, dtype=torch.float64).cuda()
    w = wav.clone().requires_grad_(True)
    r = refs.clone().requires_grad_(True)
    s, scounts = nmd.score_windows(w, r, 0.1, 0.06, lengths=lengths, k=K)
    (s * upw).sum().backward()
    if lengths is None:
        temb, tcounts, layers, saved = engine.embed_train_windows(est, win, hop)
    else:
        temb, tcounts, layers, saved, batch = engine.embed_train_windows_ragged(est, win, hop, lengths)
    _, idx, ts = engine.knn(temb, refs, K)
    assert scounts == tcounts == counts and torch.equal(s.detach(), ts)
    demb, dref = engine.knn_backward(temb, refs, idx, g_score=upw, want_a=True, want_b=True)
    if lengths is None:
        dwav = engine.embed_windows_backward(est, layers, saved, demb, win, hop)
    else:
        dwav = engine.embed_windows_backward_ragged(batch, layers, saved, demb, win, hop)
    assert torch.equal(w.grad, dwav.reshape(w.shape)) and torch.equal(r.grad, dref)
    # a window over a whole clip has score(k)'s value, without and with a gradient
    with torch.no_grad():
        whole, wc = nmd.score_over_time(wav, refs, 10.0, 5.0, lengths=lengths, k=K)
        assert wc == [1, 1, 1] and torch.equal(whole, nmd.score(wav, refs, lengths=lengths, k=K))
    w2 = wav.clone().requires_grad_(True)
    whole_g, _ = nmd.score_windows(w2, refs, 10.0, 5.0, lengths=lengths, k=K)
    assert torch.equal(whole_g.detach(), nmd.score(wav.clone().requires_grad_(True), refs, lengths=lengths, k=K).detach())


# ---- 9. predict ------------------------------------------------------------------------------------------------------------------
def test_predict_with_k_on_the_example_wavs(engine, nmd, tmp_path):
    nmr, deg = os.path.join(GOLD, "wavs", "nmr-data"), os.path.join(GOLD, "wavs", "test-data")
    out0, out2 = tmp_path / "k_none", tmp_path / "k2"
    out0.mkdir()
    out2.mkdir()
    avg0, dm0 = nmd.predict("dir", nmr, deg, results_path=str(out0))
    avg, dm, near = nmd.predict("dir", nmr, deg, results_path=str(out2), k=2)
    assert (out2 / "nomad_scores.csv").read_bytes() == (out0 / "nomad_scores.csv").read_bytes() and dm.equals(dm0)
    assert sorted(os.listdir(out2)) == ["nomad_avg.csv", "nomad_nearest.csv", "nomad_scores.csv"]
    assert sorted(os.listdir(out0)) == ["nomad_avg.csv", "nomad_scores.csv"]
    ref_emb = nmd.get_embeddings(nmr).set_index("filename")
    deg_emb = nmd.get_embeddings(deg).set_index("filename")
    names = [x.split("/")[-1].split(".")[0] for x in ref_emb.index]
    tests = [x.split("/")[-1].split(".")[0] for x in deg_emb.index]
    dist = engine.pairwise(torch.from_numpy(np.ascontiguousarray(deg_emb.to_numpy(dtype=np.float32))).cuda(),
                           torch.from_numpy(np.ascontiguousarray(ref_emb.to_numpy(dtype=np.float32))).cuda())[0]
    rd, ri, rs = knn_ref(dist, 2)
    assert list(avg.index) == tests == list(near.index) and list(dm.columns) == names
    assert np.array_equal(avg["NOMAD"].to_numpy(), np.round(rs.cpu().numpy(), 3))
    assert bool((avg["NOMAD"] <= avg0["NOMAD"]).all())
    assert list(near.columns) == ["Ref 1", "Dist 1", "Ref 2", "Dist 2"]
    for r in range(2):
        assert list(near[f"Ref {r + 1}"]) == [names[j] for j in ri[:, r].tolist()]
        assert np.array_equal(near[f"Dist {r + 1}"].to_numpy(), np.round(rd[:, r].cpu().numpy(), 3))
        assert np.array_equal(near[f"Dist {r + 1}"].to_numpy(), np.array([dm.loc[t, near.loc[t, f"Ref {r + 1}"]] for t in tests]))
