"""GPU: a non-finite clip stays non-finite and inside its own rows.

Every other file feeds the engine finite audio (and NaN only into memory that must not be read), where a select done by multiplying
with zero, a ``fmaxf`` or a row loaded for a neighbour's tile gives the bits of the right code.  ``Nomad.predict*`` packs whatever files
a folder holds into one batch and a float WAV may hold a NaN; ``Nomad.forward`` is a training loss, and the network under training is
what produces non-finite estimates.  tests/test_nonfinite_host.py pins the contract on the reference arithmetic; tests/nonfinite.py
holds the poison values and positions, the geometries and the comparison.

Every case makes THREE calls on the same engine with the same shapes - a clean batch, the batch with clip j poisoned, the clean batch
again - and asserts

  A  containment: every output element of a clip other than j is ``torch.equal`` between call 1 and call 2, and call 3 is
     ``torch.equal`` to call 1 everywhere (same shapes, same dispatch: bit identity, no tolerance);
  B  visibility: every output element of clip j is NaN - layers, features, embedding, window rows, span rows, loss term, score.
     Gradients follow the CPU oracle's autograd on the same poisoned clip (``nonfinite.same_mask``).  Which rule applied where:
       d loss / d estimate, d score / d estimate (whole clip, windows, spans): every length here leaves three or more samples
         behind the last conv0 frame, whose gradient is an exact zero in the oracle, so its mask is not all-NaN: the any / none
         answer per clip - and, on top of that, elementwise on the samples conv0 reads, where the oracle's mask IS all-NaN;
       cdist_backward: da and db elementwise against float64 autograd;
       train_backward: every parameter segment elementwise (the oracle makes every element of every trainable tensor NaN).

The kernels that had to change: the ReLU of the head - then seven copies, now three sites in head.hip.h: head_kernel,
head_pooled_from_sum (head_rows_kernel, head_rows_bwd_kernel) and head_pooled_one_pass (head_bwd_kernel) - and the hinge of triplet_loss_kernel computed
``fmaxf(x, 0.f)``, which is 0 for a NaN: an all-NaN clip got the finite embedding normalize(bias) and a finite score, a NaN triplet
added 0 to the loss.  They now run ``relu_keep_nan`` (rowops.hip.h), two true selects.  No GEMM, conv, attention, pos-conv,
LayerNorm or split-K kernel failed containment or visibility in any case below: none was changed.

What bites, measured with libraries built for the purpose (never committed): on the parent commit's kernels 95 of the 181 cases
run there fail - every case that reads an embedding, a window or span row, a score, the triplet loss, the files - and the layers / features /
frame-energy / distance cases pass.  With ONLY the three backward sites put back to ``fmaxf`` exactly one case fails,
test_train_backward_with_a_finite_upstream (its docstring says why nothing else can see them).

What reaches what (tests/test_nonfinite_host.py restates the thresholds):
  small   fp32: the 64-row tile edge (195 rows); bf16: 64 x 64 GEMM tiles, the 128-query attention with partial key and query blocks,
          pos-conv in 128-frame mode, a last LayerNorm wave of 3 rows
  mid     bf16 pos-conv in 256-frame mode with clips 2 and 3 in one workgroup, 128 x 128 / 256 x 256 tiles, the three-kernel
          attention backward (also at small: T > 64)
  ragged  T = 1, 64, 2, 65, 130, 35 with clip 0, 3 or 5 poisoned: clamped and padded rows at clip boundaries of the packed layout, both
          attention backward kernels in one batch
  large   bf16 44 x 160000: the persistent GEMM, the 256-query attention, pos-conv in 512-frame mode; fp32 25 x 160000: fc1 on
          gemm_f32_mixed_kernel, the poisoned clip inside its 256 x 128 part

Worst case per test function, seconds on one MI355X (2026-10-20, call phase; no case above 1 s, the file 16 s in all):
  0.74 test_train_backward_with_a_poisoned_anchor      0.47 test_train_backward_with_a_finite_upstream
  0.39 test_fp32_forward_every_value_at_every_position  (the first case: first launches)
  0.27 test_loss_per_utterance[small-all_terms]         0.25 test_forward_large_fp32      0.21 test_scores_with_a_poisoned_estimate[small-score]
  0.14 test_head_backward_with_a_finite_upstream[ragged3-spans]    0.06 test_forward_large_bf16    0.06 test_predict_with_a_nan_file
  every other function below 0.05
"""
import contextlib
import os
import shutil
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nonfinite as NF
import ref64
from conftest import GOLD
from nomad_amd.weights import num_frames, num_windows
from oracle import nomad_oracle as O

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "bf16x3", "bf16")
WIN, HOP = 16, 8                 # frames; T = 65: 7 windows per clip, the window rows of neighbouring clips adjacent in the output
UNIFORM = {"small": NF.SMALL, "mid": NF.MID}
LAYER_WEIGHTS = [0, 0.5, 0, 0, 2.0, 0, 0, 0, 0, 0, 0, 0, 0]          # depth 5, no embedding term
EMBEDDING_ONLY = [0] * 12 + [1.0]   # d |e - c| / d e is sign(e - c) = 0 at a NaN: a FINITE upstream reaches the head's backward, whose own
#                                     recomputation of the pooled ReLU then has to carry the NaN (the oracle's gradient is NaN on every read sample)
MARGIN = 1.0


def _poisoned(n, poison):
    """(sample index, value) of a (value name, position name) pair, or of ("nan", "tail")."""
    value, where = poison
    return (NF.tail_position(n) if where == "tail" else NF.position(n, where)), NF.VALUES[value]


def _three(fn, clean_in, bad_in):
    out = [fn(clean_in), fn(bad_in), fn(clean_in)]
    torch.cuda.synchronize()
    return out


def _check(case, outs, own, dims=None, want_nan=True):
    """outs: the three calls' results, each a dict {name: tensor}.  own: {name: row mask} or one mask for all (None: tail)."""
    for k in outs[0]:
        o = own[k] if isinstance(own, dict) else own
        NF.contained(f"{case} {k}", outs[0][k], outs[1][k], outs[2][k], o, dim=(dims or {}).get(k, 0), want_nan=want_nan)


# ---- forward, equal lengths ----------------------------------------------------------------------------------------------------
def _uniform_entry(engine, entry, T):
    if entry == "embed":
        def fn(w):
            emb, layers = engine.embed(w, want_layers=True)
            return {"emb": emb, "layers": layers, "emb alone": engine.embed(w)}
        return fn, {"layers": 1}
    if entry == "embed_bf16x3":
        def fn(w):
            emb, layers = engine.embed_bf16x3(w, want_layers=True)
            return {"emb": emb, "layers": layers, "emb alone": engine.embed_bf16x3(w)}
        return fn, {"layers": 1}
    if entry == "embed_bf16":
        return (lambda w: {"emb": engine.embed_bf16(w)}), {}
    if entry == "features":
        return (lambda w: {p: engine.embed_features(w, precision=p) for p in PRECISIONS}), {}
    assert entry == "windows"
    return (lambda w: {p: engine.embed_windows(w, WIN, HOP, precision=p)[0] for p in PRECISIONS}), {}


def _uniform_case(engine, geom, entry, poison):
    g = UNIFORM[geom]
    wav = NF.waves(g["B"], g["n"])
    at, value = _poisoned(g["n"], poison)
    fn, dims = _uniform_entry(engine, entry, g["T"])
    outs = _three(fn, wav.cuda(), NF.poison_batch(wav, g["j"], at, value).cuda())
    if poison[1] == "tail":
        own = None
    elif entry == "windows":
        own = NF.rows_of([num_windows(g["T"], WIN, HOP)] * g["B"], g["j"])
        assert int(own.sum()) == {65: 7, 130: 15}[g["T"]]
    else:
        own = NF.rows_of([1] * g["B"], g["j"])
    _check(f"{geom} {entry} {poison}", outs, own, dims)


ENTRIES = ["embed", "embed_bf16x3", "embed_bf16", "features", "windows"]


@pytest.mark.parametrize("value, where", NF.FULL)
def test_fp32_forward_every_value_at_every_position(engine, value, where):
    _uniform_case(engine, "small", "embed", (value, where))


@pytest.mark.parametrize("poison", NF.REDUCED, ids=lambda p: "-".join(p))
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("geom", ["small", "mid"])
def test_forward_equal_lengths(engine, geom, entry, poison):
    _uniform_case(engine, geom, entry, poison)


@pytest.mark.parametrize("entry", ENTRIES)
def test_forward_equal_lengths_unread_tail(engine, entry):
    _uniform_case(engine, "small", entry, ("nan", "tail"))


def test_bf16_attention_with_peaked_scores(engine_peaky):
    """qk_gain 6: softmax rows dominated by one key, the running-maximum rescale taken - with a NaN clip beside."""
    _uniform_case(engine_peaky, "small", "embed_bf16", ("nan", "middle"))
    _uniform_case(engine_peaky, "small", "embed_bf16x3", ("+inf", "first"))


# ---- forward, ragged -------------------------------------------------------------------------------------------------------------
def _span_rows(T):
    """Rows of one clip: the whole clip, and where it is long enough its first half and a row of two spans."""
    rows = [[(0, T)]]
    if T >= 4:
        rows += [[(0, T // 2)], [(1, 2), (T - 2, T)]]
    return rows


SPAN_ROWS = [_span_rows(T) for T in NF.RAGGED_T]
SPAN_COUNTS = [len(r) for r in SPAN_ROWS]


def _span_table():
    from nomad_amd.nomad import span_table
    table, counts = span_table(SPAN_ROWS, NF.RAGGED_T, "frames")
    assert counts == SPAN_COUNTS == [1, 3, 1, 3, 3, 3]
    return table


def _ragged_entry(engine, entry):
    """-> (fn(clips) -> {name: tensor}, rows per clip)."""
    if entry == "embed_ragged":
        return (lambda c: {p: engine.embed_ragged(c, precision=p) for p in PRECISIONS}), [1] * 6
    if entry == "features_ragged":
        return (lambda c: {p: engine.embed_features_ragged(c, precision=p) for p in PRECISIONS}), [1] * 6
    if entry == "windows_ragged":
        return (lambda c: {p: engine.embed_windows_ragged(c, WIN, HOP, precision=p)[0] for p in PRECISIONS}), [num_windows(T, WIN, HOP) for T in NF.RAGGED_T]
    assert entry == "spans_ragged"
    table = _span_table()
    return (lambda c: {p: engine.embed_spans_ragged(c, table, precision=p) for p in PRECISIONS}), SPAN_COUNTS


RAGGED_ENTRIES = ["embed_ragged", "features_ragged", "windows_ragged", "spans_ragged"]


def _ragged_case(engine, entry, j, poison):
    clips = NF.ragged_waves()
    at, value = _poisoned(NF.RAGGED_N[j], poison)
    bad = [NF.poison(c, at, value) if i == j else c for i, c in enumerate(clips)]
    fn, counts = _ragged_entry(engine, entry)
    outs = _three(fn, [c.cuda() for c in clips], [c.cuda() for c in bad])
    assert outs[0]["fp32"].shape[0] == sum(counts)
    _check(f"ragged {entry} clip {j} {poison}", outs, None if poison[1] == "tail" else NF.rows_of(counts, j))


@pytest.mark.parametrize("poison", NF.REDUCED + [("nan", "tail")], ids=lambda p: "-".join(p))
@pytest.mark.parametrize("j", NF.RAGGED_J)
@pytest.mark.parametrize("entry", RAGGED_ENTRIES)
def test_forward_ragged(engine, entry, j, poison):
    _ragged_case(engine, entry, j, poison)


@pytest.mark.parametrize("poison", NF.FULL + [("nan", "tail")], ids=lambda p: "-".join(p))
@pytest.mark.parametrize("j", NF.RAGGED_J)
def test_frame_energy(engine, j, poison):
    """Exactly the frames t with 320 t <= i < 320 t + 400 are NaN (+-Inf squared is +Inf: non-finite, checked as such); all others,
    of this clip too, keep the clean bits."""
    clips = NF.ragged_waves()
    at, value = _poisoned(NF.RAGGED_N[j], poison)
    bad = [NF.poison(c, at, value) if i == j else c for i, c in enumerate(clips)]
    e0, e1, e2 = _three(engine.frame_energy, [c.cuda() for c in clips], [c.cuda() for c in bad])
    want = torch.cat([c.double().unfold(0, 400, 320).pow(2).mean(1) for c in bad])            # torch, float64
    hit = torch.zeros(sum(NF.RAGGED_T), dtype=torch.bool)
    hit[[sum(NF.RAGGED_T[:j]) + t for t in NF.frames_reading(at, NF.RAGGED_T[j])]] = True
    assert torch.equal(~torch.isfinite(want), hit)
    assert torch.equal(e2, e0) and torch.isfinite(e0).all()
    assert torch.equal(~torch.isfinite(e1.cpu()), hit) and torch.equal(torch.isnan(e1.cpu()), torch.isnan(want))
    assert torch.equal(e1.cpu()[~hit], e0.cpu()[~hit])


# ---- forward, large --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", NF.REDUCED, ids=lambda p: "-".join(p))
def test_forward_large_bf16(engine, poison):
    B, j = NF.BF16_LARGE_B, NF.BF16_LARGE_B // 2
    wav = NF.waves(B, NF.N_10S).cuda()
    bad = wav.clone()
    at, value = _poisoned(NF.N_10S, poison)
    bad[j, at] = value
    outs = _three(lambda w: {"emb": engine.embed_bf16(w)}, wav, bad)
    _check(f"large bf16 {poison}", outs, NF.rows_of([1] * B, j))


@pytest.mark.parametrize("poison", NF.REDUCED, ids=lambda p: "-".join(p))
def test_forward_large_fp32(engine, poison):
    """25 clips of 10 s in one unsplit forward (want_layers): fc1 runs on gemm_f32_mixed_kernel.  Compared on the device."""
    assert torch.cuda.get_device_properties(0).multi_processor_count == NF.CUS
    B = NF.F32_LARGE_B
    j = (B - 1) // 2
    wav = NF.waves(B, NF.N_10S).cuda()
    bad = wav.clone()
    at, value = _poisoned(NF.N_10S, poison)
    bad[j, at] = value
    own = NF.rows_of([1] * B, j)
    ref = None
    for k, w in enumerate((wav, bad, wav)):              # one call's layers alive beside the first's: 0.46 GB each
        emb, layers = engine.embed(w, want_layers=True)
        torch.cuda.synchronize()
        if k == 0:
            ref = (emb, layers)
        elif k == 1:
            NF.contained(f"large fp32 {poison} emb", ref[0], emb, ref[0], own)
            NF.contained(f"large fp32 {poison} layers", ref[1], layers, ref[1], own, dim=1)
        else:
            assert torch.equal(emb, ref[0]) and torch.equal(layers, ref[1]), "the clean call after the poisoned one"
        del emb, layers


# ---- distances -------------------------------------------------------------------------------------------------------------------
def _embeddings(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    return F.normalize(torch.randn(n, D, generator=g), dim=1)


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("call, D", [("cdist", 256), ("cdist", 68), ("pairwise", 256)])
def test_distance_matrix_with_a_nan_row(engine, call, D, side):
    """Na = 70, Nb = 67: more than one 64-row tile each way, partial tiles.  Exactly that row (column) of the matrix is NaN, the means
    are NaN exactly where torch's are, everything else has the clean bits."""
    a, b = _embeddings(70, D, 1), _embeddings(67, D, 2)
    an, bn = a.clone(), b.clone()
    an[65, D - 1], bn[3, 0] = NF.NAN, NF.NAN
    bad = (an, b) if side == "a" else (a, bn)
    fn = getattr(engine, call)
    outs = _three(lambda ab: dict(zip(("dist", "mean"), fn(ab[0].cuda(), ab[1].cuda()))), (a, b), bad)
    want = torch.cdist(bad[0].double(), bad[1].double())
    d0, d1 = outs[0]["dist"].cpu(), outs[1]["dist"].cpu()
    assert torch.equal(torch.isnan(d1), torch.isnan(want)) and torch.equal(torch.isnan(outs[1]["mean"].cpu()), torch.isnan(want.mean(1)))
    assert int(torch.isnan(d1).sum()) == (67 if side == "a" else 70)
    keep = ~torch.isnan(want)
    assert torch.equal(d1[keep], d0[keep])
    km = ~torch.isnan(want.mean(1))
    assert torch.equal(outs[1]["mean"].cpu()[km], outs[0]["mean"].cpu()[km]) and int(km.sum()) == (69 if side == "a" else 0)
    assert torch.equal(outs[2]["dist"], outs[0]["dist"]) and torch.equal(outs[2]["mean"], outs[0]["mean"])
    # the means without the matrix are the same bits
    assert torch.equal(torch.nan_to_num(fn(bad[0].cuda(), bad[1].cuda(), want_matrix=False)[1]), torch.nan_to_num(outs[1]["mean"]))


@pytest.mark.parametrize("side", ["a", "b"])
def test_paired_distance_with_a_nan_row(engine, side):
    a, b = _embeddings(70, 256, 1), _embeddings(70, 256, 2)
    an, bn = a.clone(), b.clone()
    an[65, 255], bn[65, 0] = NF.NAN, NF.NAN
    bad = (an, b) if side == "a" else (a, bn)
    outs = _three(lambda ab: {"d": engine.paired_distance(ab[0].cuda(), ab[1].cuda())}, (a, b), bad)
    want = (bad[0].double() - bad[1].double()).pow(2).sum(1).sqrt()
    assert torch.isnan(want).nonzero().flatten().tolist() == [65]
    _check(f"paired_distance {side}", outs, NF.rows_of([1] * 70, 65))


@pytest.mark.parametrize("side", ["a", "b"])
def test_cdist_backward_masks(engine, side):
    """The non-finite masks of da and db equal float64 autograd's, elementwise."""
    a, b = _embeddings(70, 256, 1), _embeddings(67, 256, 2)
    an, bn = a.clone(), b.clone()
    an[65, 255], bn[3, 0] = NF.NAN, NF.NAN
    bad = (an, b) if side == "a" else (a, bn)
    g = torch.Generator().manual_seed(3)
    g_dist, g_mean = torch.randn(70, 67, generator=g, dtype=torch.float64), torch.randn(70, generator=g, dtype=torch.float64)

    def fn(ab):
        da, db = engine.cdist_backward(ab[0].cuda(), ab[1].cuda(), g_dist.cuda(), g_mean.cuda(), want_a=True, want_b=True)
        return {"da": da, "db": db}
    outs = _three(fn, (a, b), bad)
    x, y = bad[0].double().requires_grad_(True), bad[1].double().requires_grad_(True)
    d = (x[:, None] - y[None]).pow(2).sum(-1).sqrt()
    ((d * g_dist).sum() + (d.mean(1) * g_mean).sum()).backward()
    for k, ref in (("da", x.grad), ("db", y.grad)):
        got = outs[1][k].cpu()
        assert torch.equal(~torch.isfinite(got), ~torch.isfinite(ref)), f"{k}: {int((~torch.isfinite(got)).sum())} vs {int((~torch.isfinite(ref)).sum())}"
        keep = torch.isfinite(ref)
        assert torch.equal(got[keep], outs[0][k].cpu()[keep])
        assert torch.equal(outs[2][k], outs[0][k])
    assert (~torch.isfinite(x.grad)).sum() == (256 if side == "a" else 70 * 256)


# ---- loss and scores with gradients ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nomad(engine):
    from nomad_amd.nomad import Nomad
    n = Nomad.from_engine(engine)
    g = torch.Generator().manual_seed(NF.SEED)
    n.lossnet_layers.embedding_weight = ((torch.rand(256, 768, generator=g) * 2 - 1) / 768 ** 0.5).cuda()
    n.lossnet_layers.embedding_bias = ((torch.rand(256, generator=g) * 2 - 1) / 768 ** 0.5).cuda()
    return n


def _batch(geom, j, seed=NF.SEED):
    """-> (padded (B, Nmax) fp32, lengths or None, j, lengths as a list)."""
    if geom == "ragged":
        clips = NF.ragged_waves(seed)
        wav = torch.zeros(len(clips), max(NF.RAGGED_N))
        for i, c in enumerate(clips):
            wav[i, :c.numel()] = c
        return wav, list(NF.RAGGED_N), j, list(NF.RAGGED_N)
    g = UNIFORM[geom]
    return NF.waves(g["B"], g["n"], seed), None, g["j"], [g["n"]] * g["B"]


GRAD_GEOMS = [("small", None)] + [("ragged", j) for j in NF.RAGGED_J]


def _gid(p):
    return p[0] if p[1] is None else f"ragged{p[1]}"


def _grad_calls(fn, est, bad):
    """fn(estimate requiring a gradient) -> per-row values; three calls -> [{"values", "grad"}]."""
    outs = []
    for w in (est, bad, est):
        e = w.cuda().requires_grad_(True)
        v = fn(e)
        v.sum().backward()
        outs.append({"values": v.detach(), "grad": e.grad})
    torch.cuda.synchronize()
    return outs


def _check_grad(case, outs, counts, j, n_j, oracle_grad):
    B = len(counts)
    NF.contained(f"{case} values", outs[0]["values"], outs[1]["values"], outs[2]["values"], NF.rows_of(counts, j))
    NF.contained(f"{case} grad", outs[0]["grad"], outs[1]["grad"], outs[2]["grad"], NF.rows_of([1] * B, j), want_nan=False)
    got = outs[1]["grad"][j, :n_j].cpu()
    read = NF.position(n_j, "last_read") + 1
    assert NF.same_mask(f"{case} grad of clip {j}", got, oracle_grad) == "any"              # the unread tail: zeros in the oracle
    assert NF.same_mask(f"{case} grad of clip {j}, the samples conv0 reads", got[:read], oracle_grad[:read]) == "elementwise"
    assert torch.equal(~torch.isfinite(got[read:]), ~torch.isfinite(oracle_grad[read:]))


def _loss_oracle(sd0, nomad, est_j, clean_j, weights, mult):
    hw, hb = nomad.lossnet_layers.embedding_weight.cpu(), nomad.lossnet_layers.embedding_bias.cpu()
    e = est_j[None].clone().requires_grad_(True)
    oe = O.lossnet_forward(sd0, e, hw, hb, feature_grad_mult=mult, required_seq_len_multiple=2)
    with torch.no_grad():
        oc = O.lossnet_forward(sd0, clean_j[None], hw, hb, required_seq_len_multiple=2)
    w = weights if weights is not None else [1.0] * 13
    term = sum(w[i] * (oe[i] - oc[i]).abs().mean() for i in range(13) if w[i])
    (g,) = torch.autograd.grad(term, e)
    return term.detach(), g[0]


@pytest.mark.parametrize("poison", NF.REDUCED, ids=lambda p: "-".join(p))
@pytest.mark.parametrize("weights", [None, LAYER_WEIGHTS, EMBEDDING_ONLY], ids=["all_terms", "layer_weights", "embedding_only"])
@pytest.mark.parametrize("geom", GRAD_GEOMS, ids=_gid)
def test_loss_per_utterance(engine, nomad, sd0, geom, weights, poison):
    """``Nomad.forward(..., reduction="none")`` and the backward of the sum: term j is NaN, the other terms and the other clips' rows
    of d loss / d estimate keep the clean bits, clip j's rows follow the oracle's mask."""
    est, lengths, j, lens = _batch(*geom)
    clean = _batch(*geom, seed=NF.SEED + 50)[0].cuda()
    at, value = _poisoned(lens[j], poison)
    bad = NF.poison_batch(est, j, at, value)
    outs = _grad_calls(lambda e: nomad.forward(e, clean, lengths, layer_weights=weights, reduction="none"), est, bad)
    term, g = _loss_oracle(sd0, nomad, bad[j, :lens[j]], clean[j, :lens[j]].cpu(), weights, engine.feature_grad_mult)
    assert torch.isnan(term)
    _check_grad(f"loss {_gid(geom)} {poison}", outs, [1] * len(lens), j, lens[j], g)


def _refs(n=5, seed=3):
    return _embeddings(n, 256, seed)


def _rows_oracle(sd0, wav_j, mult, refs, rows_of_x):
    """Scores of the rows ``rows_of_x(x)`` makes of one clip's last layer (checkpoint head), and d sum / d clip."""
    e = wav_j[None].clone().requires_grad_(True)
    x, _ = O.backbone(sd0, e, feature_grad_mult=mult, required_seq_len_multiple=2)
    w, b = sd0["embedding_layer.1.weight"], sd0["embedding_layer.1.bias"]
    emb = torch.cat([O.head(r, w, b) for r in rows_of_x(x)])
    d = (emb.double()[:, None] - refs.double()[None]).pow(2).sum(-1).sqrt().mean(1)
    (g,) = torch.autograd.grad(d.sum(), e)
    return d.detach(), g[0]


def _score_kinds(nomad, refs, lengths, T):
    """{kind: (fn(estimate) -> scores, rows per clip, rows_of_x for the oracle of a clip of T frames)}."""
    def windows(x):
        n = min(WIN, x.shape[1])
        return [x[:, k * HOP:k * HOP + n] for k in range(num_windows(x.shape[1], WIN, HOP))]
    rows = [_span_rows(t) for t in T]
    return {
        "score": (lambda e: nomad.score(e, refs, lengths=lengths), [1] * len(T), lambda x: [x]),
        "score_windows": (lambda e: nomad.score_windows(e, refs, WIN / 50, HOP / 50, lengths=lengths)[0],
                          [num_windows(t, WIN, HOP) for t in T], windows),
        "score_spans": (lambda e: nomad.score_spans(e, refs, rows, lengths=lengths, unit="frames")[0], [len(r) for r in rows],
                        lambda x: [torch.cat([x[:, a:b] for a, b in row], 1) for row in _span_rows(x.shape[1])]),
    }


@pytest.mark.parametrize("poison", NF.REDUCED, ids=lambda p: "-".join(p))
@pytest.mark.parametrize("kind", ["score", "score_windows", "score_spans"])
@pytest.mark.parametrize("geom", GRAD_GEOMS, ids=_gid)
def test_scores_with_a_poisoned_estimate(engine, nomad, sd0, geom, kind, poison):
    """A poisoned estimate clip makes only its own scores NaN - with a gradient (``embed_train*``, ``cdist_backward``, the heads'
    backward) and without one (the scoring forward, ``pairwise``)."""
    est, lengths, j, lens = _batch(*geom)
    T = [num_frames(n) for n in lens]
    refs = _refs()
    fn, counts, rows_of_x = _score_kinds(nomad, refs.cuda(), lengths, T)[kind]
    at, value = _poisoned(lens[j], poison)
    bad = NF.poison_batch(est, j, at, value)
    outs = _grad_calls(fn, est, bad)
    d, g = _rows_oracle(sd0, bad[j, :lens[j]], engine.feature_grad_mult, refs, rows_of_x)
    assert torch.isnan(d).all() and d.shape == (counts[j],)
    _check_grad(f"{kind} {_gid(geom)} {poison}", outs, counts, j, lens[j], g)
    with torch.no_grad():
        plain = _three(lambda w: {"scores": fn(w)}, est.cuda(), bad.cuda())
    assert not plain[0]["scores"].requires_grad
    _check(f"{kind} {_gid(geom)} {poison} no gradient", plain, NF.rows_of(counts, j))


@pytest.mark.parametrize("kind", ["score", "score_windows", "score_spans"])
def test_scores_with_a_poisoned_reference(engine, nomad, kind):
    """One NaN element in one reference: every score is NaN, as the float64 composition ``cdist(emb, refs).mean(1)`` makes it
    (tests/test_nonfinite_host.py::test_torch_distances_with_a_nan_row); the clean call afterwards has the clean bits."""
    est, lengths, j, lens = _batch("ragged", 0)
    T = [num_frames(n) for n in lens]
    refs = _refs()
    bad_refs = refs.clone()
    bad_refs[1, 7] = NF.NAN
    assert torch.isnan(torch.cdist(_embeddings(4, 256, 9).double(), bad_refs.double()).mean(1)).all()
    for grad in (False, True):
        outs = []
        for r in (refs, bad_refs, refs):
            fn, counts, _ = _score_kinds(nomad, r.cuda(), lengths, T)[kind]
            if grad:
                e = est.cuda().requires_grad_(True)
                v = fn(e)
                v.sum().backward()
                outs.append((v.detach(), e.grad))
            else:
                with torch.no_grad():
                    outs.append((fn(est.cuda()), None))
        torch.cuda.synchronize()
        assert outs[0][0].shape == (sum(counts),) and torch.isfinite(outs[0][0]).all()
        assert torch.isnan(outs[1][0]).all(), f"{kind} grad={grad}: {int((~torch.isnan(outs[1][0])).sum())} finite scores"
        assert torch.equal(outs[2][0], outs[0][0])
        if grad:
            assert torch.isfinite(outs[0][1]).all() and torch.equal(outs[2][1], outs[0][1])
            read = [NF.position(n, "last_read") + 1 for n in lens]
            assert all(bool((~torch.isfinite(outs[1][1][i, :read[i]])).all()) for i in range(len(lens))), "d score / d estimate: NaN on every read sample"


# ---- the heads' backward on a finite upstream ----------------------------------------------------------------------------------------
def _upstream_oracle(sd0, wav_j, mult, G, rows_of_x):
    """d <rows, G> / d clip for the rows ``rows_of_x`` makes of one clip's last layer (checkpoint head)."""
    e = wav_j[None].clone().requires_grad_(True)
    x, _ = O.backbone(sd0, e, feature_grad_mult=mult, required_seq_len_multiple=2)
    w, b = sd0["embedding_layer.1.weight"], sd0["embedding_layer.1.bias"]
    emb = torch.cat([O.head(r, w, b) for r in rows_of_x(x)])
    (g,) = torch.autograd.grad((emb * G).sum(), e)
    return emb.detach(), g[0]


@pytest.mark.parametrize("poison", NF.REDUCED, ids=lambda p: "-".join(p))
@pytest.mark.parametrize("geom, kind", [("small", "whole"), ("small", "windows"), ("ragged3", "whole"), ("ragged3", "windows"),
                                        ("ragged3", "spans")])           # (the span head takes ragged batches only)
def test_head_backward_with_a_finite_upstream(engine, sd0, geom, kind, poison):
    """``embed_train*`` then ``embed*_backward*`` with a finite, random d loss / d embedding rows and no layer upstream, so that no NaN
    enters the backward from above (the scores' own backward is fed NaN by ``cdist_backward`` already): the rows are NaN, the other
    clips' gradients keep the clean bits, and clip j's gradient follows the oracle's mask.  The head kernels' zero for a masked
    column meets the NaN activations in the next backward kernel, so these cases hold the whole chain, not the head sites alone
    (test_train_backward_with_a_finite_upstream does that)."""
    ragged = geom != "small"
    est, lengths, j, lens = _batch("ragged", 3) if ragged else _batch("small", None)
    T = [num_frames(n) for n in lens]
    _, counts, rows_of_x = _score_kinds(None, None, None, T)[{"whole": "score", "windows": "score_windows", "spans": "score_spans"}[kind]]
    G = torch.randn(sum(counts), 256, generator=torch.Generator().manual_seed(NF.SEED + 7)) / 256
    Gd = G.cuda()
    from nomad_amd.nomad import span_table
    table = span_table([_span_rows(t) for t in T], T, "frames")[0]
    at, value = _poisoned(lens[j], poison)
    bad = NF.poison_batch(est, j, at, value)

    def fn(wav):
        w = wav.cuda()
        if ragged and kind == "whole":
            emb, layers, saved, batch = engine.embed_train_ragged(w, lengths)
            dwav = engine.embed_backward_ragged(batch, layers, saved, None, Gd)
        elif ragged and kind == "windows":
            emb, _, layers, saved, batch = engine.embed_train_windows_ragged(w, WIN, HOP, lengths)
            dwav = engine.embed_windows_backward_ragged(batch, layers, saved, Gd, WIN, HOP)
        elif ragged:
            emb, layers, saved, batch = engine.embed_train_spans_ragged(w, table, lengths)
            dwav = engine.embed_spans_backward_ragged(batch, layers, saved, Gd, table)
        elif kind == "whole":
            emb, layers, saved = engine.embed_train(w)
            dwav = engine.embed_backward(w, layers, saved, None, Gd)
        else:
            emb, _, layers, saved = engine.embed_train_windows(w, WIN, HOP)
            dwav = engine.embed_windows_backward(w, layers, saved, Gd, WIN, HOP)
        return {"values": emb, "grad": dwav}
    outs = _three(fn, est, bad)
    at_row = sum(counts[:j])
    emb_ref, g = _upstream_oracle(sd0, bad[j, :lens[j]], engine.feature_grad_mult, G[at_row:at_row + counts[j]], rows_of_x)
    assert torch.isnan(emb_ref).all()
    _check_grad(f"head backward {geom} {kind} {poison}", outs, counts, j, lens[j], g)


# ---- training ------------------------------------------------------------------------------------------------------------------------
def test_triplet_loss_with_a_nan_anchor(engine):
    """The loss is NaN (``F.triplet_margin_loss`` is); the other rows of da / dp / dn keep the clean bits.  6 rows: waves take
    rows w, w + 4, so a wave holds the NaN row and a clean one."""
    a, p, n = (_embeddings(6, 256, s) for s in (11, 12, 13))
    bad = a.clone()
    bad[2, 100] = NF.NAN
    assert torch.isnan(F.triplet_margin_loss(bad, p, n, margin=MARGIN)) and torch.isfinite(F.triplet_margin_loss(a, p, n, margin=MARGIN))

    def fn(anchors):
        loss, da, dp, dn = engine.triplet_loss(anchors.cuda(), p.cuda(), n.cuda(), MARGIN)
        return {"loss": loss, "da": da, "dp": dp, "dn": dn}
    outs = _three(fn, a, bad)
    assert torch.isnan(outs[1]["loss"]).all() and torch.isfinite(outs[0]["loss"]).all() and torch.equal(outs[2]["loss"], outs[0]["loss"])
    assert abs(outs[0]["loss"].item() - F.triplet_margin_loss(a, p, n, margin=MARGIN).item()) < 1e-5
    own = NF.rows_of([1] * 6, 2)
    for k in ("da", "dp", "dn"):
        NF.contained(f"triplet_loss {k}", outs[0][k], outs[1][k], outs[2][k], own, want_nan=False)
    loss_only = engine.triplet_loss(bad.cuda(), p.cuda(), n.cuda(), MARGIN, want_grad=False)[0]
    assert torch.isnan(loss_only).all()


@contextlib.contextmanager
def _training_engine(sd0):
    """An engine of its own with the master parameters allocated (the session's engine stays a scoring engine)."""
    from nomad_amd.engine import Engine
    eng = Engine({k: v.clone() for k, v in sd0.items()}, 0)
    try:
        eng.train_enable()
        yield eng
        torch.cuda.synchronize()
    finally:
        eng.close()


def _segments_follow_the_oracle(case, eng, steps, g_ref):
    """steps: three {key: gradient} (clean, poisoned, clean).  Every segment elementwise against the oracle's mask."""
    segments = [name for name, _, _ in eng.train_segments()]
    assert set(g_ref) <= set(segments) and len(g_ref) > 100
    how = set()
    for k in segments:
        c, b, a = (s[k].cpu() for s in steps)
        assert torch.isfinite(c).all() and torch.equal(a, c), k
        if k in g_ref:
            how.add(NF.same_mask(f"{case} {k}", b, g_ref[k]))
        else:                                             # frozen (the conv feature extractor): no gradient in the oracle, zeros here
            assert torch.equal(b, c), k
    assert how == {"elementwise"}


def test_train_backward_with_a_poisoned_anchor(built_lib, sd0):
    """B = 2 per branch, T = 18, a NaN in the middle of anchor 1: every parameter segment is non-finite exactly where the CPU oracle's
    autograd makes it so (everywhere: the gradients sum over clips), and a clean step afterwards has the clean step's bits."""
    from test_gpu_train_f64 import _step_separate
    A, P, N = ref64.triplet_batch(2, 18, 5)
    bad = NF.poison_batch(A, 1, A.shape[1] // 2, NF.NAN)
    loss_ref, g_ref = ref64.triplet_grads(sd0, bad, P, N, MARGIN)
    assert torch.isnan(loss_ref)
    with _training_engine(sd0) as eng:
        steps = [_step_separate(eng, a, P, N) for a in (A, bad, A)]
        assert np.isfinite(steps[0][0]) and np.isnan(steps[1][0]) and steps[2][0] == steps[0][0]
        _segments_follow_the_oracle("train_backward", eng, [s[1] for s in steps], g_ref)


def test_train_backward_with_a_finite_upstream(built_lib, sd0):
    """``train_backward`` given a finite d loss / d embedding for a batch with one NaN clip.  This is the one place where the pooled
    ReLU that head_bwd_kernel recomputes is visible on its own: with ``fmaxf`` the NaN clip's pooled row is 0, its ``dz`` finite, and
    the head's weight and bias gradients (dz x pooled, summed over clips) come out FINITE, where the oracle's are NaN.  (Everywhere
    else the kernel's zero gradient meets NaN activations one kernel later - a build with only the backward sites reverted passes
    every other case of this file, and for the windowed and span heads, which have no parameter-gradient path, every case.)"""
    A, _, _ = ref64.triplet_batch(2, 18, 5)
    bad = NF.poison_batch(A, 1, A.shape[1] // 2, NF.NAN)
    G = torch.randn(2, 256, generator=torch.Generator().manual_seed(NF.SEED + 9)) / 256
    sd, keys = ref64._live(sd0, True)
    emb = O.triplet_forward(sd, bad)
    g_ref = dict(zip(keys, torch.autograd.grad((emb * G).sum(), [sd[k] for k in keys])))
    assert torch.isnan(emb[1]).all() and torch.isfinite(emb[0]).all()
    assert all(torch.isnan(g_ref[k]).all() for k in ("embedding_layer.1.weight", "embedding_layer.1.bias"))

    def step(eng, wav):
        w = wav.cuda()
        eng.train_zero_grad()
        e, layers, saved = eng.embed_train(w)
        eng.train_backward(w, layers, saved, G.cuda())
        return eng.train_unflatten(eng.train_read(1))
    with _training_engine(sd0) as eng:
        _segments_follow_the_oracle("train_backward, finite upstream", eng, [step(eng, w) for w in (A, bad, A)], g_ref)


# ---- files ---------------------------------------------------------------------------------------------------------------------------
def _write_float_wav(path, x, sr=16000):
    body = np.asarray(x, dtype="<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, sr, sr * 4, 4, 32)
    riff = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(riff)) + riff)


@pytest.fixture
def folders(tmp_path):
    """The golden example folder, its test files copied beside one 16 kHz float32 WAV (``broken``) that the test rewrites."""
    nmr, src = os.path.join(GOLD, "wavs", "nmr-data"), os.path.join(GOLD, "wavs", "test-data")
    deg = tmp_path / "deg"
    deg.mkdir()
    for f in os.listdir(src):
        shutil.copy(os.path.join(src, f), deg / f)
    x = NF.waves(1, 16000 * 2 + 163)[0].numpy()

    def write(poisoned):
        y = x.copy()
        if poisoned:
            y[len(y) // 2] = np.nan
        _write_float_wav(str(deg / "broken.wav"), y)
    return nmr, str(deg), write, tmp_path


@pytest.mark.parametrize("native_threads", [4, 0], ids=["native_reader", "python_front_end"])
def test_predict_with_a_nan_file(engine, folders, native_threads):
    from nomad_amd.nomad import Nomad
    nmr, deg, write, tmp = folders
    n = Nomad.from_engine(engine)
    n.NATIVE_WAV_THREADS = native_threads
    tables = []
    for k, poisoned in enumerate((False, True, False)):
        write(poisoned)
        out = tmp / f"out{k}"
        out.mkdir()
        tables.append(n.predict("dir", nmr, deg, results_path=str(out)))
    (avg0, dm0), (avg1, dm1), (avg2, dm2) = tables
    assert "broken" in avg0.index and len(avg0) == 3 and np.isfinite(avg0.to_numpy()).all() and np.isfinite(dm0.to_numpy()).all()
    assert avg2.equals(avg0) and dm2.equals(dm0)
    assert np.isnan(avg1.loc["broken", "NOMAD"]) and np.isnan(dm1.loc["broken"].to_numpy()).all()
    others = [f for f in avg0.index if f != "broken"]
    assert avg1.loc[others].equals(avg0.loc[others]) and dm1.loc[others].equals(dm0.loc[others])
    # unrounded: the embeddings of the other files are the clean run's bits
    write(False)
    e0 = n.get_embeddings(deg).set_index("filename")
    write(True)
    e1 = n.get_embeddings(deg).set_index("filename")
    for f in e0.index:
        if f.endswith("broken.wav"):
            assert np.isnan(e1.loc[f].to_numpy(dtype=np.float32)).all()
        else:
            assert np.array_equal(e1.loc[f].to_numpy(dtype=np.float32), e0.loc[f].to_numpy(dtype=np.float32)), f


def test_predict_segments_with_a_nan_file(engine, folders):
    from nomad_amd.nomad import Nomad
    nmr, deg, write, tmp = folders
    n = Nomad.from_engine(engine)
    tables = []
    for poisoned in (False, True, False):
        write(poisoned)
        tables.append(n.predict_segments("dir", nmr, deg, window_s=1.0, hop_s=0.5))
    (df0, avg0), (df1, avg1), (df2, avg2) = tables
    assert df2.equals(df0) and avg2.equals(avg0) and np.isfinite(df0["NOMAD"].to_numpy()).all()
    own = (df0["Test File"] == "broken").to_numpy()
    assert own.sum() == num_windows(num_frames(16000 * 2 + 163), 50, 25) > 1 and (~own).sum() > 2
    assert np.isnan(df1["NOMAD"].to_numpy()[own]).all() and np.isnan(avg1.loc["broken", "NOMAD"])
    assert df1[~own].equals(df0[~own]) and avg1.drop("broken").equals(avg0.drop("broken"))
