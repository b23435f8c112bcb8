"""GPU: ``nomad_gammatone`` and ``nomad_nsim`` keep to their caller's stream and are done with the caller's host arrays on return,
held to it with ``stream_screen.screen`` as tests/test_gpu_stream_order.py holds the other entry points (that module's docstring has
the procedure and the reasons for SPIN_MS): each call runs on a pool stream S whose input is still a decoy when the call is
enqueued, every output is cloned and every input and host array overwritten right behind it, and the result must be the quiet
call's bit for bit.  The module owns its engine and picks S with the same positive control: a toy call mis-ordered on purpose
must be seen as stale, or the screen is blind here and the module fails."""
import pytest
import torch

from stream_screen import screen

pytestmark = pytest.mark.gpu

SPIN_MS = 100.0
LENS = [1280, 9001, 16384, 30267]      # 1, 25, 48 and 91 frames
STRIDE = 30268
G = 2


@pytest.fixture(scope="module")
def eng(built_lib, sd0):
    from nomad_amd.engine import Engine
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test running without a GPU")
    e = Engine(sd0, 0)
    yield e
    e.close()


def _wav(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(*shape, generator=g)).clamp(-1, 1).cuda()


def _toy(target):
    """``y = x * 2`` under ``target`` with no wait_stream in either direction: mis-ordered on purpose."""
    def call(_, bufs):
        with torch.cuda.stream(target):
            return bufs["x"] * 2
    return call


def _seen(rep):
    return rep.held and any("clone of output 0" in p and "STALE" in p for p in rep.problems)


@pytest.fixture(scope="module")
def S(eng):
    notes = []
    for attempt in range(4):
        s, other = torch.cuda.Stream(), torch.cuda.Stream()
        rep = screen(eng, s, lambda seed: {"x": _wav(seed, 1 << 16)}, _toy(other), SPIN_MS, name="toy", side=None, watch_abi=False)
        notes.append(f"attempt {attempt}: seen={_seen(rep)} [{rep.line()}]")
        print(notes[-1])
        if _seen(rep):
            return s
    pytest.fail("the screen is blind here: a call mis-ordered on purpose was not seen on any of four pool streams - " + " | ".join(notes))


def _judge(rep):
    print(rep.line())
    assert not rep.problems, rep.line()
    assert rep.host_arrays > 0, f"{rep.name}: no host array went through the C ABI"
    assert rep.held, f"{rep.name}: S was found released when the call returned, so the case shows nothing about producer ordering ({rep.line()})"


def test_gammatone_keeps_to_the_callers_stream(eng, S):
    rep = screen(eng, S, lambda seed: {"wav": _wav(seed, len(LENS), STRIDE)},
                 lambda e, x: e.gammatone(packed=(x["wav"], list(LENS)))[0], SPIN_MS, "gammatone", "late", ["spec"])
    _judge(rep)


def test_nsim_keeps_to_the_callers_stream(eng, S):
    def make(seed):
        clean = _wav(seed, len(LENS), STRIDE)
        deg = clean.repeat_interleave(G, dim=0) + _wav(seed + 1, len(LENS) * G, STRIDE) * 0.3
        return {"clean": clean, "deg": deg.contiguous()}

    def call(e, x):
        return e.nsim((x["clean"], list(LENS)), (x["deg"], [n for n in LENS for _ in range(G)]), G)

    rep = screen(eng, S, make, call, SPIN_MS, "nsim", "late", ["nsim", "bands"])
    _judge(rep)


def test_nsim_of_spectrograms_keeps_to_the_callers_stream(eng, S):
    """``nomad_nsim`` alone, its spectrograms being the screened inputs."""
    frames = [eng.gammatone_frames(n) for n in LENS]

    def make(seed):
        g = torch.Generator().manual_seed(seed)
        total = sum(frames)
        return {"ref": torch.rand(total, 21, generator=g, dtype=torch.float64).cuda() * 0.1,
                "deg": torch.rand(G * total, 21, generator=g, dtype=torch.float64).cuda() * 0.1}

    rep = screen(eng, S, make, lambda e, x: e.nsim_of_spectrograms(x["ref"], x["deg"], frames, G), SPIN_MS, "nsim_of_spectrograms", "late",
                 ["nsim", "bands"])
    _judge(rep)
