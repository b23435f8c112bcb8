"""Non-finite clips for ``test_nonfinite_host.py`` and ``test_gpu_nonfinite.py``: poison values and positions, the geometries, the
three-call comparison.  Imported by the tests like ``wave_kinds``; not a test module itself.

The contract (pinned for the reference arithmetic by tests/test_nonfinite_host.py): one NaN, +Inf or -Inf sample that conv0 reads makes
EVERY output element of its clip NaN and changes no bit of any other clip of the batch; a sample behind the last conv0 frame is never
read and changes nothing.

  A  containment   outputs of the other clips are ``torch.equal`` between a clean call and the call with clip j poisoned, and a third,
                   clean call is ``torch.equal`` to the first everywhere (nothing non-finite survives in the engine)
  B  visibility    every output element of clip j is NaN (forward); gradients follow the CPU oracle's autograd mask (``same_mask``)

Positions: sample 0, sample n // 2, and the last sample conv0 reads, 5 (L0 - 1) + 9; separately the unread tail (``tail_position``).
Every length here has ``(n - 10) % 5 != 0``, so one length serves the read and the unread cases.

Geometries (``ref64.n_for(T)`` plus an offset below 320 that is no multiple of 5):
  small   B = 3, T = 65, clip 1     the 64-row tile edge; bf16: 64 x 64 tiles, 128-query attention with partial blocks, pos-conv in
                                    128-frame mode, a last LayerNorm wave of 3 rows
  mid     B = 5, T = 130, clip 2    bf16 pos-conv in 256-frame mode, two clips per workgroup (clip 2 shares one with clip 3);
                                    128 x 128 / 256 x 256 tiles; the three-kernel attention backward
  ragged  T = 1, 64, 2, 65, 130, 35, poisoned in turn: clip 0 (T = 1, a boundary), clip 3 (T = 65, finite clips on both sides),
                                    clip 5 (the last)
  large   forward only, the middle clip: bf16 44 x 160000 (persistent GEMM, 256-query attention, pos-conv in 512-frame mode) and fp32
          ``F32_LARGE_B`` x 160000, the smallest batch of 10 s clips with a GEMM on ``gemm_f32_mixed_kernel`` (``f32_mixed_gemms``)
"""
import math
import os
import re

import torch

import ref64
from nomad_amd.weights import num_frames

NAN, INF = float("nan"), float("inf")
VALUES = {"nan": NAN, "+inf": INF, "-inf": -INF}
POSITIONS = ("first", "middle", "last_read")
FULL = [(v, p) for v in VALUES for p in POSITIONS]                 # the fp32 forward at ``small``
REDUCED = [("nan", "middle"), ("+inf", "first")]                   # everywhere else
SEED = 23


def conv0_frames(n: int) -> int:
    return (n - 10) // 5 + 1


def position(n: int, where: str) -> int:
    return {"first": 0, "middle": n // 2, "last_read": 5 * (conv0_frames(n) - 1) + 9}[where]


def tail_position(n: int) -> int:
    """The last sample of a clip whose length leaves samples behind the last conv0 frame."""
    assert (n - 10) % 5 != 0 and n - 1 > position(n, "last_read")
    return n - 1


def frames_reading(i: int, T: int):
    """The encoder frames t whose 400 samples [320 t, 320 t + 400) contain sample i."""
    return [t for t in range(T) if 320 * t <= i < 320 * t + 400]


def _n(T: int, extra: int) -> int:
    n = ref64.n_for(T) + extra
    assert 0 < extra < 320 and extra % 5 and num_frames(n) == T and (n - 10) % 5 != 0
    return n


N_TINY = _n(5, 3)                                                  # the oracle experiment of the host file
SMALL = dict(B=3, T=65, n=_n(65, 163), j=1)
MID = dict(B=5, T=130, n=_n(130, 83), j=2)
RAGGED_T = [1, 64, 2, 65, 130, 35]
RAGGED_N = [_n(T, e) for T, e in zip(RAGGED_T, (3, 111, 37, 163, 83, 7))]
RAGGED_J = [0, 3, 5]
N_10S = 160000
BF16_LARGE_B = 44
assert num_frames(N_10S) == 499 and (N_10S - 10) % 5 == 0           # the large geometry has no unread tail: read positions only


def waves(B: int, n: int, seed: int = SEED) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed + 1000 * B + n)
    return (0.1 * torch.randn(B, n, generator=g)).clamp(-1, 1)


def ragged_waves(seed: int = SEED):
    return [waves(1, n, seed + i)[0] for i, n in enumerate(RAGGED_N)]


def poison(x: torch.Tensor, at: int, value: float) -> torch.Tensor:
    """A copy of the 1-D clip x with sample ``at`` replaced."""
    y = x.clone()
    y[at] = value
    return y


def poison_batch(wav: torch.Tensor, j: int, at: int, value: float) -> torch.Tensor:
    y = wav.clone()
    y[j, at] = value
    return y


def rows_of(counts, j: int) -> torch.Tensor:
    """Boolean mask over the rows of a packed output (clip 0's ``counts[0]`` rows, then clip 1's, ...): the rows of clip j."""
    m = torch.zeros(sum(counts), dtype=torch.bool)
    at = sum(counts[:j])
    m[at:at + counts[j]] = True
    return m


def contained(case: str, clean: torch.Tensor, bad: torch.Tensor, again: torch.Tensor, own, dim: int = 0, want_nan: bool = True):
    """Properties A and B of one output tensor.  own: boolean mask over ``dim`` of the entries that belong to the poisoned clip
    (None: the poison is in the unread tail, every entry keeps the clean bits).  Works on the device the tensors are on."""
    c, b, a = (t.movedim(dim, 0) for t in (clean, bad, again))
    assert c.shape == b.shape == a.shape, (case, c.shape, b.shape, a.shape)
    assert bool(torch.isfinite(c).all()), f"{case}: the clean call is not finite"
    assert torch.equal(a, c), f"{case}: the clean call after the poisoned one differs from the clean call before it"
    if own is None:
        assert torch.equal(b, c), f"{case}: a sample that no frame reads changed {int((b != c).sum())} output elements"
        return
    own = own.to(c.device)
    assert own.shape == (c.shape[0],) and bool(own.any()), (case, own.shape, c.shape)
    other = ~own
    if bool(other.any()):
        diff = (b[other] != c[other]) | torch.isnan(b[other])
        assert not bool(diff.any()), f"{case}: {int(diff.sum())} elements of OTHER clips changed ({int(torch.isnan(b[other]).sum())} of them NaN)"
    if want_nan:
        fin = ~torch.isnan(b[own])
        assert not bool(fin.any()), f"{case}: {int(fin.sum())} of {fin.numel()} elements of the poisoned clip are not NaN"


def same_mask(case: str, got: torch.Tensor, oracle: torch.Tensor) -> str:
    """Property B for a gradient: ``oracle`` is the CPU oracle's autograd result on the same poisoned input.  Where every element of
    the oracle's tensor is non-finite the masks must agree elementwise (-> "elementwise"); otherwise the any / none answer must
    (-> "any")."""
    g, o = ~torch.isfinite(got.cpu()), ~torch.isfinite(oracle)
    assert g.shape == o.shape, (case, g.shape, o.shape)
    if bool(o.all()):
        assert bool(g.all()), f"{case}: the oracle's gradient is non-finite everywhere, {int((~g).sum())} of {g.numel()} elements here are finite"
        return "elementwise"
    assert bool(g.any()) == bool(o.any()), f"{case}: oracle non-finite: {bool(o.any())}, here: {bool(g.any())}"
    return "any"


# ---- the fp32 GEMM dispatch, restated (nomad_amd/csrc/nomad_gemm_f32.hip: pick_tile, mixed_split_rows) --------------------------------
CUS = 256
MIXED_MIN_FILL, MIXED_MAX_FILL = 0.05, 0.70
ENCODER_GEMMS = {"projection": (768, 512), "qkv": (2304, 768), "out_proj": (768, 768), "fc1": (3072, 768), "fc2": (768, 3072)}


def pick_tile_f32(M: int, N: int, parts: int = 1, cus: int = CUS) -> int:
    tiles256 = -(-M // 256) * (N // 128)
    if N % 128 == 0 and tiles256 >= 4 * cus:
        per_cu_256 = -(-tiles256 // cus)
        tiles128 = -(-M // 128) * (N // 128)
        cost128 = -(-tiles128 // cus) * 0.5 * (1.08 if parts >= 2 else 1.03)
        return 31 if cost128 < per_cu_256 else 33
    if N % 128 == 0 and tiles256 >= 1500:
        return 33
    if tiles256 < 512:
        return 37
    if N >= 2048 and N % 128 == 0 and tiles256 < 2048:
        return 20
    return 31 if N % 128 == 0 else 34


def mixed_split_rows(M: int, N: int, cus: int = CUS) -> int:
    if N % 128:
        return 0
    tn, slots = N // 128, 2 * cus
    tiles = -(-M // 256) * tn
    rounds = tiles // slots
    frac = (tiles - rounds * slots) / slots
    if rounds < 1 or frac < MIXED_MIN_FILL or frac > MIXED_MAX_FILL:
        return 0
    m1 = rounds * slots // tn * 256
    return m1 if 0 < m1 < M else 0


def f32_mixed_gemms(B: int, T: int = 499):
    """The encoder GEMMs of one unsplit fp32 forward of B clips of T frames that run on ``gemm_f32_mixed_kernel``."""
    return [k for k, (N, K) in ENCODER_GEMMS.items() if pick_tile_f32(B * T, N) == 33 and mixed_split_rows(B * T, N) > 0]


F32_LARGE_B = next(B for B in range(1, 200) if f32_mixed_gemms(B))


def dispatch_constants():
    """The constants of the restatement above as the source states them today."""
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "nomad_amd", "csrc", "nomad_gemm_f32.hip")).read()
    fills = re.search(r"kMixedMinFill = ([0-9.]+), kMixedMaxFill = ([0-9.]+);", text)
    pen = re.search(r"concurrent_parts >= 2 \? ([0-9.]+) : ([0-9.]+);", text)
    return dict(min_fill=float(fills.group(1)), max_fill=float(fills.group(2)), penalty=(float(pen.group(1)), float(pen.group(2))),
                big=bool(re.search(r"tiles256 >= 4LL \* cus\)", text)), rounds1500=bool(re.search(r"tiles256 >= 1500\) return 33;", text)),
                small=bool(re.search(r"if \(tiles256 < 512\) return 37;", text)),
                slots=bool(re.search(r"slots = 2 \* c->num_cus;", text)),
                mixed_on_33=bool(re.search(r"if \(lean && tile == 33\)", text)))


assert not math.isfinite(NAN) and not math.isfinite(INF)
