"""GPU: every entry point keeps to its caller's stream and is done with the caller's host arrays on return.

include/nomad_hip.h promises "the launch stream is always the caller's stream" and "host arrays may die on return"; the rest of the
suite runs on torch's default stream and reads results through ``.cpu()``, where neither promise can be broken visibly.  Here every
call runs through ``stream_screen.screen`` (its docstring has the procedure): on a pool stream S whose input is still a decoy when
the call is enqueued - the real input is copied in behind a sleeping one-wave spin -, with the engine's side stream held longer
still (side="late") or not at all (side="free"), with every output cloned and every input and host array overwritten right behind
the call.  The result must be the quiet call's, bit for bit.

The module owns its engines (the session ``engine``'s side stream and workspaces belong to other modules).  The three split
thresholds are set to 100 rows on the instance, so that B = 4 clips of 16384 samples (200 rows) and the ragged batch 720 / 9001 /
16384 / 30267 samples (173 rows, cut by audio length behind the third clip) run as two parts on two streams.

Positive controls: the same screen on a toy call that is mis-ordered on purpose (``y = x * 2`` under another stream, no
``wait_stream``) must report that y equals its stale value - against a second pool stream, and against the legacy default stream,
where a stray ``hipLaunchKernelGGL(..., 0, 0, ...)`` would land.  The module picks as S the first of up to four fresh pool streams
on which both controls are seen (two streams that share a hardware queue serialise, and the screen is blind between them) and fails
with "the screen is blind here" if there is none.

Held-stream condition: a case shows producer ordering only if S was still held when the call returned.  Every case must meet it
except those marked ``host_waits`` in the table below, with the observation that earned the mark; such a case is held to the
side-stream, consumer and host-array parts.

MEASURED on an MI355X (4 hardware queues per process), host time of enqueueing each case while S was held, in ms: the three
``embed*`` 0.31 - 0.35 single and 0.57 - 0.66 split; ``embed(want_layers, side)`` 0.40; ``embed_ragged`` 0.68 - 0.72 in the
three precisions; ``embed_features`` 0.67, ``_ragged`` 0.70; ``embed_windows`` 0.64, ``_ragged`` 0.70; ``embed_spans_ragged``
0.77; ``frame_energy`` 0.06; ``pairwise`` 0.02, ``cdist`` 0.02, ``knn`` 0.14, ``paired_distance`` 0.01, ``cdist_backward`` 0.03,
``knn_backward`` 0.04; ``l1_loss`` 0.02, its backward 0.02, ``l1_loss_weighted`` 0.04, its backward 0.04; ``embed_train`` +
``embed_backward`` 0.76, ragged 0.68, windows 0.73, ragged windows 0.67, spans 0.71; the training step 2.22; ``degrade_noise``
0.09, ``_clip`` 0.08, ``_convolve`` 0.07, ``_normalize`` 0.11, in place 0.06; ``Nomad.forward`` + backward 1.63, ``Nomad.score`` +
backward 1.18, with k 1.24, without a gradient 0.81; two ``GraphedLoss`` replays 2.40; the toy calls 0.02 - 0.17.  The slowest is
2.40 ms; SPIN_MS = 100 is 40 x that (4 x is the least that shows anything; the rest is room for a host that stalls on a shared
machine).  S was still held at the return of EVERY case, those that upload host metadata included: the runtime stages a small
pageable ``hipMemcpyAsync`` without making the host wait for the stream, so the HOST_WAITS table below is empty.  Both positive
controls were seen on the first pair of pool streams tried."""
import pytest
import torch

from stream_screen import HostArrays, screen
from nomad_amd.weights import num_frames, num_windows

pytestmark = pytest.mark.gpu

SPIN_MS = 100.0
SPLIT_ROWS = 100

B, N = 4, 16384
LENS = [720, 9001, 16384, 30267]
STRIDE = 30268
FRAMES = [num_frames(n) for n in LENS]                   # 2, 27, 50, 94
WIN, HOP = 10, 5
TABLE = ([0, 1, 2, 3, 3], [0, 1, 3, 4, 5, 6], [(0, 2), (0, 10), (15, 27), (5, 50), (0, 40), (50, 94)])
GB, GN = 2, 8000                                         # the gradient pairs: 2 clips of 0.5 s
GLENS = [720, 5001, 8000]
GSTRIDE = 8000
GFRAMES = [num_frames(n) for n in GLENS]
GTABLE = ([0, 1, 1, 2], [0, 1, 2, 3, 5], [(0, 2), (0, 7), (9, 15), (0, 10), (12, 24)])
WEIGHTS = [1.0, 0.5, 0.0, 2.0, 1.0, 1.0, 0.25, 1.0, 1.0, 3.0, 1.0, 1.0, 1.5]


def _wav(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(*shape, generator=g)).clamp(-1, 1).cuda()


def _randn(seed, *shape, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g, dtype=torch.float64)).to(dtype).cuda()


def _unit(seed, n, d=256):
    x = _randn(seed, n, d, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float().contiguous()


def _clips(buf, lens):
    return [buf[i, :n] for i, n in enumerate(lens)]


# ---- the module's engines ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(built_lib, sd0):
    from nomad_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test running without a GPU")
    e = Engine(sd0, 0)
    assert not e.build_flags & 1
    yield e
    e.close()


@pytest.fixture(scope="module")
def teng(built_lib):
    from nomad_amd.engine import Engine
    from nomad_amd.weights import seeded_state_dict
    e = Engine(seeded_state_dict(3, qk_gain=3.0), 0)
    e.train_enable()
    e.theta0 = e.train_read(0).clone()
    e.zeros = torch.zeros_like(e.theta0)
    torch.cuda.synchronize()
    yield e
    e.close()


@pytest.fixture(scope="module")
def nomad(eng):
    from nomad_amd.nomad import Nomad
    torch.manual_seed(7)          # LossNetLayers draws its own head
    return Nomad.from_engine(eng)


def _split(eng, on):
    eng.F32_SPLIT_ROWS = eng.BF16_SPLIT_ROWS = eng.X3_SPLIT_ROWS = SPLIT_ROWS if on else 0


# ---- the positive controls and the choice of S ---------------------------------------------------------------------------------------
def _toy(target, ordered=False):
    """``y = x * 2`` under ``target``: mis-ordered on purpose (no wait_stream in either direction) unless ``ordered``."""
    def call(_, bufs):
        cur = torch.cuda.current_stream()
        if ordered:
            target.wait_stream(cur)
        with torch.cuda.stream(target):
            y = bufs["x"] * 2
        if ordered:
            cur.wait_stream(target)
        return y
    return call


def _control(eng, S, target, ordered=False):
    return screen(eng, S, lambda seed: {"x": _wav(seed, 1 << 16)}, _toy(target, ordered), SPIN_MS, name="toy", side=None, watch_abi=False)


def _seen(rep):
    return rep.held and any("clone of output 0" in p and "STALE" in p for p in rep.problems)


_OTHER = []     # the second pool stream of the controls on the chosen S


@pytest.fixture(scope="module")
def S(eng):
    """The stream the module screens on: the first fresh pool stream on which both controls are seen."""
    notes = []
    for attempt in range(4):
        s, other = torch.cuda.Stream(), torch.cuda.Stream()
        reps = [_control(eng, s, other), _control(eng, s, torch.cuda.default_stream())]
        notes.append(f"attempt {attempt}: second stream seen={_seen(reps[0])} [{reps[0].line()}], legacy default stream seen={_seen(reps[1])} [{reps[1].line()}]")
        print(notes[-1])
        if all(_seen(r) for r in reps):
            _OTHER[:] = [other]
            return s
    pytest.fail("the screen is blind here: a call mis-ordered on purpose was not seen on any of four pool streams - " + " | ".join(notes))


def test_positive_controls_are_seen_and_an_ordered_toy_passes(eng, S):
    for what, target in (("a second pool stream", _OTHER[0]), ("the legacy default stream", torch.cuda.default_stream())):
        rep = _control(eng, S, target)
        print(what, "->", rep.line())
        assert rep.held, f"the screen is blind here: S was released before the toy call under {what} returned"
        assert _seen(rep), f"the screen is blind here: y = x * 2 under {what} without wait_stream was not reported stale: {rep.line()}"
        assert any("returned output 0" in p and "STALE" in p for p in rep.problems), rep.line()
    rep = _control(eng, S, _OTHER[0], ordered=True)
    print("ordered toy ->", rep.line())
    assert rep.held and not rep.problems, rep.line()


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# Cases exempt from the held-stream condition: name -> the observation that earned the mark.  Only a call that uploads host
# metadata may be listed.
HOST_WAITS = {}


class Case:
    """make(seed) -> inputs; call(eng, inputs) -> outputs; sides: the side-stream modes to run; split: thresholds at 100 rows or off;
    on: which fixture drives it; uploads: the call hands host arrays to the C ABI (they must have been seen and overwritten)."""

    def __init__(self, name, make, call, names, sides=("late",), split=False, on="eng", uploads=False):
        self.name, self.make, self.call, self.names, self.sides, self.split, self.on, self.uploads = \
            name, make, call, names, sides, split, on, uploads

    @property
    def host_waits(self):
        return HOST_WAITS.get(self.name)


BOTH = ("late", "free")


def _equal_wav(seed):
    return {"wav": _wav(seed, B, N)}


def _ragged_wav(seed):
    return {"wav": _wav(seed, len(LENS), STRIDE)}


def _forward_cases():
    cases = []
    for split in (True, False):
        tag = "split" if split else "single"
        sides = BOTH if split else ("late",)
        cases += [
            Case(f"embed/{tag}", _equal_wav, lambda e, x: e.embed(x["wav"]), ["emb"], sides, split),
            Case(f"embed_bf16/{tag}", _equal_wav, lambda e, x: e.embed_bf16(x["wav"]), ["emb"], sides, split),
            Case(f"embed_bf16x3/{tag}", _equal_wav, lambda e, x: e.embed_bf16x3(x["wav"]), ["emb"], sides, split),
        ]
    cases.append(Case("embed/layers-side", _equal_wav, lambda e, x: e.embed(x["wav"], want_layers=True, side=True), ["emb", "layers"]))
    for prec in ("fp32", "bf16", "bf16x3"):
        cases.append(Case(f"embed_ragged/{prec}", _ragged_wav,
                          lambda e, x, prec=prec: e.embed_ragged(_clips(x["wav"], LENS), precision=prec), ["emb"], BOTH, True, uploads=True))
    cases += [
        Case("embed_features", _equal_wav, lambda e, x: e.embed_features(x["wav"]), ["feat"], BOTH, True),
        Case("embed_features_ragged", _ragged_wav, lambda e, x: e.embed_features_ragged(_clips(x["wav"], LENS)), ["feat"], BOTH, True,
             uploads=True),
        Case("embed_windows", _equal_wav, lambda e, x: e.embed_windows(x["wav"], WIN, HOP)[0], ["emb_w"], BOTH, True),
        Case("embed_windows_ragged", _ragged_wav, lambda e, x: e.embed_windows_ragged(_clips(x["wav"], LENS), WIN, HOP)[0], ["emb_w"], BOTH,
             True, uploads=True),
        Case("embed_spans_ragged", _ragged_wav, lambda e, x: e.embed_spans_ragged(_clips(x["wav"], LENS), TABLE), ["emb_r"], BOTH, True,
             uploads=True),
        Case("frame_energy", _ragged_wav, lambda e, x: e.frame_energy(_clips(x["wav"], LENS)), ["energy"], uploads=True),
    ]
    return cases


def _distance_cases():
    def ab(seed, d=132):
        return {"a": _randn(seed, 37, d), "b": _randn(seed + 1, 21, d)}

    def emb(seed):
        return {"a": _unit(seed, 37), "b": _unit(seed + 1, 21)}

    def cdist_bwd(seed):
        return dict(ab(seed), g_dist=_randn(seed + 2, 37, 21, dtype=torch.float64), g_mean=_randn(seed + 3, 37, dtype=torch.float64))

    def knn_bwd(seed):
        x = ab(seed)
        # the selection is an input like any other: that of the seed's own operands, so that every index is in range
        x["idx"] = torch.cdist(x["a"].double(), x["b"].double()).topk(5, dim=1, largest=False).indices.to(torch.int32).contiguous()
        x["g_knn"] = _randn(seed + 2, 37, 5, dtype=torch.float64)
        x["g_score"] = _randn(seed + 3, 37, dtype=torch.float64)
        return x

    return [
        Case("pairwise", emb, lambda e, x: e.pairwise(x["a"], x["b"]), ["dist", "mean"]),
        Case("cdist", ab, lambda e, x: e.cdist(x["a"], x["b"]), ["dist", "mean"]),
        Case("knn", ab, lambda e, x: e.knn(x["a"], x["b"], 5, want_matrix=True), ["knn_dist", "knn_idx", "score", "dist"]),
        Case("paired_distance", lambda seed: {"a": _randn(seed, 37, 132), "b": _randn(seed + 1, 37, 132)},
             lambda e, x: e.paired_distance(x["a"], x["b"]), ["dist"]),
        Case("cdist_backward", cdist_bwd, lambda e, x: e.cdist_backward(x["a"], x["b"], x["g_dist"], x["g_mean"], True, True), ["da", "db"]),
        Case("knn_backward", knn_bwd, lambda e, x: e.knn_backward(x["a"], x["b"], x["idx"], x["g_knn"], x["g_score"]), ["da", "db"]),
    ]


def _loss_cases():
    T = 25

    def dense(seed):
        return {"a_layers": _randn(seed, 12, 2, T, 768), "b_layers": _randn(seed + 1, 12, 2, T, 768), "a_emb": _unit(seed + 2, 2),
                "b_emb": _unit(seed + 3, 2), "up": _randn(seed + 4, 1).abs().reshape(())}

    frames = [10, 15, 25]

    def packed(seed):
        M = sum(frames)
        return {"a_layers": _randn(seed, 12, M, 768), "b_layers": _randn(seed + 1, 12, M, 768), "a_emb": _unit(seed + 2, 3),
                "b_emb": _unit(seed + 3, 3), "up": _randn(seed + 4, 3).abs()}

    return [
        Case("l1_loss", dense, lambda e, x: e.l1_loss(x["a_layers"], x["b_layers"], x["a_emb"], x["b_emb"]), ["loss"]),
        Case("l1_loss_backward", dense, lambda e, x: e.l1_loss_backward(x["a_layers"], x["b_layers"], x["a_emb"], x["b_emb"], x["up"]),
             ["dlayers", "demb"]),
        Case("l1_loss_weighted", packed,
             lambda e, x: e.l1_loss_weighted(x["a_layers"], x["b_layers"], x["a_emb"], x["b_emb"], list(WEIGHTS), "none", list(frames)),
             ["loss", "terms"], uploads=True),
        Case("l1_loss_weighted_backward", packed,
             lambda e, x: e.l1_loss_weighted_backward(x["a_layers"], x["b_layers"], x["a_emb"], x["b_emb"], x["up"], list(WEIGHTS), "none",
                                                      list(frames)),
             ["dlayers", "demb"], uploads=True),
    ]


def _gradient_cases():
    T = num_frames(GN)
    W = num_windows(T, WIN, HOP)
    M = sum(GFRAMES)
    Wr = sum(num_windows(t, WIN, HOP) for t in GFRAMES)

    def equal(seed):
        return {"wav": _wav(seed, GB, GN), "dlayers": _randn(seed + 1, 12, GB, T, 768, scale=1e-3), "demb": _randn(seed + 2, GB, 256, scale=1e-2),
                "demb_w": _randn(seed + 3, GB * W, 256, scale=1e-2)}

    def ragged(seed):
        return {"wav": _wav(seed, len(GLENS), GSTRIDE), "dlayers": _randn(seed + 1, 12, M, 768, scale=1e-3),
                "demb": _randn(seed + 2, len(GLENS), 256, scale=1e-2), "demb_w": _randn(seed + 3, Wr, 256, scale=1e-2),
                "demb_r": _randn(seed + 4, len(GTABLE[0]), 256, scale=1e-2)}

    def pair(e, x):
        emb, layers, saved = e.embed_train(x["wav"])
        return emb, layers, e.embed_backward(x["wav"], layers, saved, x["dlayers"], x["demb"])

    def pair_ragged(e, x):
        emb, layers, saved, batch = e.embed_train_ragged(x["wav"], list(GLENS))
        return emb, layers, e.embed_backward_ragged(batch, layers, saved, x["dlayers"], x["demb"])

    def pair_windows(e, x):
        emb, _, layers, saved = e.embed_train_windows(x["wav"], WIN, HOP)
        return emb, layers, e.embed_windows_backward(x["wav"], layers, saved, x["demb_w"], WIN, HOP)

    def pair_windows_ragged(e, x):
        emb, _, layers, saved, batch = e.embed_train_windows_ragged(x["wav"], WIN, HOP, list(GLENS))
        return emb, layers, e.embed_windows_backward_ragged(batch, layers, saved, x["demb_w"], WIN, HOP)

    def pair_spans(e, x):
        emb, layers, saved, batch = e.embed_train_spans_ragged(x["wav"], GTABLE, list(GLENS))
        return emb, layers, e.embed_spans_backward_ragged(batch, layers, saved, x["demb_r"], GTABLE)

    def step(t, x):
        """One fine-tuning step from a fixed state: parameters, moments and the step counter are reset first, on the same stream."""
        t.train_write(0, t.theta0)
        t.train_write(2, t.zeros)
        t.train_write(3, t.zeros)
        t.train_set_step(0)
        t.train_zero_grad()
        emb, layers, saved = t.embed_train(x["wav"])
        loss, da, dp, dn = t.triplet_loss(emb[0:2].contiguous(), emb[2:4].contiguous(), emb[4:6].contiguous(), 0.2)
        t.train_backward(x["wav"], layers, saved, torch.cat([da, dp, dn]))
        t.adam_step(1e-4, 1e-3)
        return loss, t.train_read(1), t.train_read(0), t.train_read(2), t.train_read(3)

    names = ["emb", "layers", "dwav"]
    return [
        Case("embed_train+embed_backward", equal, pair, names),
        Case("embed_train_ragged+embed_backward_ragged", ragged, pair_ragged, names, uploads=True),
        Case("embed_train_windows+embed_windows_backward", equal, pair_windows, names),
        Case("embed_train_windows_ragged+embed_windows_backward_ragged", ragged, pair_windows_ragged, names, uploads=True),
        Case("embed_train_spans_ragged+embed_spans_backward_ragged", ragged, pair_spans, names, uploads=True),
        Case("training step", lambda seed: {"wav": _wav(seed, 6, 6000)}, step, ["loss", "gradient", "parameters", "exp_avg", "exp_avg_sq"],
             on="teng"),
    ]


def _degradation_cases():
    def rows(seed):
        return {"wav": _wav(seed, len(LENS), STRIDE), "noise": _wav(seed + 1, 5000), "ir": _randn(seed + 2, 2, 300, scale=0.05)}

    ir_lens = [300, 65]
    return [
        Case("degrade_noise", rows, lambda e, x: (lambda r: (r[0], r[2]))(e.degrade_noise(_clips(x["wav"], LENS), x["noise"], [0.0, 15.0])),
             ["rows", "alpha"], uploads=True),
        Case("degrade_clip", rows, lambda e, x: (lambda r: (r[0], r[2]))(e.degrade_clip(_clips(x["wav"], LENS), [5.0, 40.0])),
             ["rows", "thresholds"], uploads=True),
        Case("degrade_convolve", rows, lambda e, x: e.degrade_convolve(_clips(x["wav"], LENS), (x["ir"], list(ir_lens)))[0], ["rows"],
             uploads=True),
        Case("degrade_normalize", rows, lambda e, x: (lambda r: (r[0], r[2]))(e.degrade_normalize(_clips(x["wav"], LENS))), ["rows", "stats"],
             uploads=True),
        Case("degrade_normalize/inplace", rows,
             lambda e, x: (lambda r: (r[0], r[2]))(e.degrade_normalize(packed=(x["wav"], list(LENS)), inplace=True)), ["rows", "stats"],
             uploads=True),
    ]


def _nomad_cases():
    def pair(seed):
        clean = _wav(seed, B, 1, N)
        return {"est": (clean + 0.02 * _randn(seed + 1, B, 1, N)).clamp(-1, 1), "clean": clean, "refs": _unit(seed + 2, 9)}

    def forward(nmd, x):
        est = x["est"].clone().requires_grad_(True)
        loss = nmd.forward(est, x["clean"])
        loss.backward()
        return loss.detach(), est.grad

    def score(k):
        def call(nmd, x):
            est = x["est"].clone().requires_grad_(True)
            s = nmd.score(est, x["refs"], k=k)
            s.sum().backward()
            return s.detach(), est.grad
        return call

    return [
        Case("Nomad.forward+backward", pair, forward, ["loss", "d estimate"], BOTH, on="nomad"),
        Case("Nomad.score+backward", pair, score(None), ["score", "d estimate"], on="nomad"),
        Case("Nomad.score(k=3)+backward", pair, score(3), ["score", "d estimate"], on="nomad"),
        Case("Nomad.score/no_grad", pair, lambda nmd, x: nmd.score(x["est"], x["refs"]), ["score"], BOTH, True, on="nomad"),
    ]


CASES = _forward_cases() + _distance_cases() + _loss_cases() + _gradient_cases() + _degradation_cases() + _nomad_cases()
RUNS = [(c, side) for c in CASES for side in c.sides]


def _judge(case, rep):
    print(rep.line())
    assert not rep.problems, rep.line()
    assert (rep.host_arrays > 0) == case.uploads, f"{rep.name}: {rep.host_arrays} host arrays went through the C ABI"
    assert case.host_waits is None or case.uploads, f"{case.name}: only a call that uploads host metadata may carry a host_waits mark"
    if case.host_waits is None:
        assert rep.held, (f"{rep.name}: S was found released when the call returned, so the case shows nothing about producer ordering, and "
                          f"it carries no host_waits mark ({rep.line()})")


@pytest.mark.parametrize("case,side", RUNS, ids=[f"{c.name}-{s}" for c, s in RUNS])
def test_call_keeps_to_the_callers_stream(request, eng, S, case, side):
    _split(eng, case.split)
    try:
        if case.on == "nomad":
            nmd = request.getfixturevalue("nomad")
            rep = screen(eng, S, case.make, lambda _, x: case.call(nmd, x), SPIN_MS, f"{case.name} [{side}]", side, case.names)
        else:
            e = request.getfixturevalue(case.on)
            rep = screen(e, S, case.make, case.call, SPIN_MS, f"{case.name} [{side}]", side, case.names)
    finally:
        _split(eng, False)
    _judge(case, rep)


@pytest.mark.parametrize("missing,side,rows", [("fork", "free", [2, 3]), ("join", "late", [2, 3])])
def test_a_dispatch_without_one_of_its_waits_is_seen(eng, S, missing, side, rows):
    """The screen against the engine's own dispatcher with one ``wait_stream`` taken out for the held run (the quiet runs keep
    both): without ``side.wait_stream(cur)`` the second half of the batch is embedded from the decoy while S is still held
    (side="free"); without ``cur.wait_stream(side)`` the clone on S reads the second half's rows before the held side stream has
    written them (side="late") and finds whatever the allocator left there - as a rule what the quiet call on the decoy wrote.
    Either way rows 2 and 3 are reported and rows 0 and 1 are not: both directions are directions the screen can see."""
    def broken(e, x):
        real, ss = torch.cuda.Stream.wait_stream, e.side_stream()

        def wait(self, other):
            if (self is ss or self == ss) == (missing == "fork"):
                return None
            return real(self, other)

        torch.cuda.Stream.wait_stream = wait
        try:
            return e.embed(x["wav"])
        finally:
            torch.cuda.Stream.wait_stream = real

    _split(eng, True)
    try:
        rep = screen(eng, S, _equal_wav, lambda e, x: e.embed(x["wav"]), SPIN_MS, f"embed without its {missing} wait [{side}]", side, ["emb"],
                     held_call=broken)
    finally:
        _split(eng, False)
    print(rep.line())
    assert rep.held
    # (what an unwritten row holds is up to the allocator: usually the decoy's result, which the quiet run on S left there)
    seen = [p for p in rep.problems if p.startswith("clone of output emb") and ("STALE" in p or missing == "join") and f"rows {rows} " in p]
    assert seen, f"the screen is blind here: {rep.line()}"


def test_graphed_loss_replays_on_the_callers_stream(eng, nomad, S):
    """Capture under S, then two replays as one screened call: ``step`` copies the inputs into the graph's static tensors and
    replays on the current stream; both replays' loss and gradient are the eager call's bits."""
    def pair(seed):
        clean = _wav(seed, B, 1, N)
        return {"est": (clean + 0.02 * _randn(seed + 1, B, 1, N)).clamp(-1, 1), "clean": clean}

    first = pair(11)
    est = first["est"].clone().requires_grad_(True)
    loss = nomad.forward(est, first["clean"])
    loss.backward()
    eager = (loss.detach().clone(), est.grad.clone())
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        graphed = nomad.graphed_loss(first["est"], first["clean"])
        l0, g0 = graphed.step(first["est"], first["clean"])
        l0, g0 = l0.detach().clone(), g0.clone()
    torch.cuda.synchronize()
    assert torch.equal(l0, eager[0]) and torch.equal(g0, eager[1]), "a replay on S gives the eager call's bits"

    def replays(_, x):
        l1, g1 = graphed.step(x["est"], x["clean"])
        l1, g1 = l1.detach().clone(), g1.clone()
        l2, g2 = graphed.step(x["est"], x["clean"])
        return l1, g1, l2.detach().clone(), g2.clone()

    for side in BOTH:
        rep = screen(eng, S, pair, replays, SPIN_MS, f"GraphedLoss replays [{side}]", side, ["loss 1", "grad 1", "loss 2", "grad 2"])
        print(rep.line())
        assert not rep.problems, rep.line()
        assert rep.held, rep.line()


def test_twelve_ragged_forwards_in_flight_keep_their_own_lengths(eng, S):
    """Ring depth: the library stages each call's host metadata in a ring of 16 vectors.  Twelve ragged forwards of twelve length
    sets are enqueued back to back on the held S (single-part: one ring slot each), each length array overwritten as soon as its
    call has returned; every result equals its own quiet call.  Twelve stays inside the ring: its depth is a stated limit."""
    _split(eng, False)
    sets = [[720 + 37 * i, 9001 - 113 * i, 16384 - 64 * i, 30267 - 1000 * i] for i in range(12)]
    real, decoy = _wav(31, 4, STRIDE), _wav(32, 4, STRIDE)
    buf = real.clone()
    refs = [eng.embed_ragged(_clips(buf, lens)).clone() for lens in sets]
    torch.cuda.synchronize()
    watch = HostArrays(eng.lib)
    eng.lib = watch
    try:
        with torch.cuda.stream(S):
            buf.copy_(decoy)
            eng.diag_clock_probe(SPIN_MS, S)
            buf.copy_(real)
            released = torch.cuda.Event()
            released.record(S)
            outs, taken = [], 0
            for lens in sets:
                outs.append(eng.embed_ragged(_clips(buf, lens)))
                taken = watch.overwrite()
            held = not released.query()
            clones = [o.clone() for o in outs]
            buf.copy_(decoy)
    finally:
        eng.lib = watch._lib
    torch.cuda.synchronize()
    print(f"12 ragged forwards: held={held}, host arrays overwritten={taken}")
    assert taken >= 12
    bad = [i for i in range(12) if not (torch.equal(clones[i], refs[i]) and torch.equal(outs[i], refs[i]))]
    assert not bad, f"forwards {bad} of 12 differ from their own quiet call (lengths {[sets[i] for i in bad]})"
    assert held or "embed_ragged/fp32" in HOST_WAITS, "S was found released when the twelfth call returned"
