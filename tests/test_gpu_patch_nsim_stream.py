"""GPU: ``nomad_nsim_patches`` keeps to its caller's stream and is done with BOTH host tables on return, held to it with
``stream_screen.screen`` as tests/test_gpu_nsim_stream.py holds ``nomad_nsim`` (tests/test_gpu_stream_order.py has the procedure and
the reasons for SPIN_MS): the call runs on a pool stream S whose input is still a decoy when it is enqueued, every output is cloned
and every input overwritten right behind it, and the result must be the quiet call's bit for bit.  The screen sees the first host
table of an entry point it does not list; the second one (the degraded rows' frame counts, bound as a plain address) is overwritten
here, with the first, as soon as the entry point has returned - while S is still held, so ahead of the kernels - as
tests/test_gpu_align.py does it for ``nomad_align_delay``.  The module owns its engine and picks S with the same positive control."""
import ctypes as C

import pytest
import torch

from stream_screen import screen

pytestmark = pytest.mark.gpu

SPIN_MS = 100.0
LENS = [1280, 9001, 16384, 30267]      # 1, 25, 48 and 91 frames
DLENS = [n + 640 * (g + 1) for n in LENS for g in range(2)]      # every row 2 or 4 frames longer than its clip
STRIDE, DSTRIDE = 30268, 31548
G = 2
PATCH, SEARCH, RATIO, NEED = 8, 6, 1e-4, 4


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


class _Tables:
    """Stands between the engine and its library for one call: both ctypes arrays that go into ``nomad_nsim_patches`` are
    overwritten with other valid frame counts as soon as the entry point has returned."""

    def __init__(self, lib):
        self._lib = lib
        self.seen = 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "nomad_nsim_patches":
            return fn

        def call(*args):
            rc = fn(*args)
            tables = [a for a in args if isinstance(a, C.Array)]
            assert len(tables) == 2, name
            for t in tables:
                t[:] = [9] * len(t)
            self.seen += 1
            return rc

        return call


def _with_tables_overwritten(fn):
    def call(e, x):
        lib = e.lib
        e.lib = tables = _Tables(lib)
        try:
            out = fn(e, x)
        finally:
            e.lib = lib
        assert tables.seen == 1
        return out
    return call


def _outputs(res):
    return res["nsim"], res["bands"], res["offsets"], res["patch_nsim"], res["cand"]


NAMES = ["nsim", "bands", "offsets", "patch_nsim", "cand"]


def test_nsim_patches_keeps_to_the_callers_stream(eng, S):
    """Both ``gammatone`` calls and the three launches of ``nomad_nsim_patches``, from the waveforms."""
    def make(seed):
        clean = _wav(seed, len(LENS), STRIDE)
        deg = torch.zeros(len(LENS) * G, DSTRIDE, device="cuda")
        for r in range(len(LENS) * G):
            d = 640 * (r % G + 1)
            deg[r, d:d + STRIDE] = clean[r // G]
        return {"clean": clean, "deg": (deg + 0.02 * _wav(seed + 1, len(LENS) * G, DSTRIDE)).contiguous()}

    def call(e, x):
        return _outputs(e.nsim_patches((x["clean"], list(LENS)), (x["deg"], list(DLENS)), G, PATCH, SEARCH, RATIO, NEED, want_cand=True))

    rep = screen(eng, S, make, _with_tables_overwritten(call), SPIN_MS, "nsim_patches", "late", NAMES)
    _judge(rep)


def test_nsim_patches_of_spectrograms_keeps_to_the_callers_stream(eng, S):
    """``nomad_nsim_patches`` alone, its spectrograms being the screened inputs."""
    frames = [eng.gammatone_frames(n) for n in LENS]
    dframes = [eng.gammatone_frames(n) for n in DLENS]

    def make(seed):
        g = torch.Generator().manual_seed(seed)
        return {"ref": torch.rand(sum(frames), 21, generator=g, dtype=torch.float64).cuda() * 0.1,
                "deg": torch.rand(sum(dframes), 21, generator=g, dtype=torch.float64).cuda() * 0.1}

    def call(e, x):
        return _outputs(e.nsim_patches_of_spectrograms(x["ref"], x["deg"], frames, dframes, G, PATCH, SEARCH, RATIO, NEED, want_cand=True))

    rep = screen(eng, S, make, _with_tables_overwritten(call), SPIN_MS, "nsim_patches_of_spectrograms", "late", NAMES)
    _judge(rep)
