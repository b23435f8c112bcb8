"""GPU: ``nomad_nsim_backward`` and ``nomad_gammatone_backward`` keep to their caller's stream and are done with the caller's host
arrays on return, held to it with ``stream_screen.screen`` the way tests/test_gpu_nsim_stream.py holds the forward calls (that
module and tests/test_gpu_stream_order.py have the procedure and the reasons for SPIN_MS).  The module owns its engine and picks S
with the same positive control: a toy call mis-ordered on purpose must be seen as stale, or the screen is blind here and the module
fails."""
import pytest
import torch

from stream_screen import screen

pytestmark = pytest.mark.gpu

SPIN_MS = 100.0
LENS = [1280, 5001, 8192]      # 1, 12 and 22 frames
STRIDE = 8192
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


def test_gammatone_backward_keeps_to_the_callers_stream(eng, S):
    frames = [eng.gammatone_frames(n) for n in LENS]

    def make(seed):
        g = torch.Generator().manual_seed(seed + 7)
        return {"wav": _wav(seed, len(LENS), STRIDE), "dspec": torch.randn(sum(frames), 21, generator=g, dtype=torch.float64).cuda()}

    rep = screen(eng, S, make, lambda e, x: e.gammatone_backward(x["dspec"], packed=(x["wav"], list(LENS))), SPIN_MS, "gammatone_backward",
                 "late", ["dx"])
    _judge(rep)


def test_nsim_backward_keeps_to_the_callers_stream(eng, S):
    frames = [eng.gammatone_frames(n) for n in LENS]
    total = sum(frames)

    def make(seed):
        g = torch.Generator().manual_seed(seed)
        return {"ref": torch.rand(total, 21, generator=g, dtype=torch.float64).cuda() * 0.1,
                "deg": torch.rand(G * total, 21, generator=g, dtype=torch.float64).cuda() * 0.1,
                "grad": torch.randn(len(LENS), G, generator=g, dtype=torch.float64).cuda()}

    rep = screen(eng, S, make, lambda e, x: e.nsim_backward(x["ref"], x["deg"], frames, G, x["grad"]), SPIN_MS, "nsim_backward", "late",
                 ["dspec"])
    _judge(rep)
