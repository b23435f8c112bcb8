"""GPU: the two-stream split of every dispatching entry point, on the smallest batches that can take it.

The other split tests need 4000 frames.  Here the thresholds are lowered on the instance (``*_SPLIT_ROWS = 1``) so that three clips
split, and each entry point is held bit-identical to the same call with the thresholds at 0 (no split).  A clip's bits do not
depend on the batch it is in on these paths, so equality is exact.

* Equal-length: B = 3, N = 720 (T = 2): the cut at B // 2 gives 1 + 2 clips, so a wrong slice or output offset shows.
* Ragged: clips of 400, 720 and 20560 samples (T = 1, 2, 64) in this order: half of the audio is reached only in the last clip, so
  the cut by audio length puts two clips in the first part and one in the second.

Every clip holds its own random data, so swapped parts cannot cancel.  That the split happened is asserted through the side
workspace, which only a split (or ``side=True``) allocates.
"""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

THRESHOLDS = ("F32_SPLIT_ROWS", "BF16_SPLIT_ROWS", "X3_SPLIT_ROWS")
RAGGED_N = (400, 720, 20560)
PRECISIONS = ("fp32", "bf16", "bf16x3")


@contextlib.contextmanager
def _thresholds(eng, rows):
    """The three split thresholds set on the instance, and the instance left as it was."""
    before = {k: eng.__dict__[k] for k in THRESHOLDS if k in eng.__dict__}
    for k in THRESHOLDS:
        setattr(eng, k, rows)
    try:
        yield
    finally:
        for k in THRESHOLDS:
            if k in before:
                setattr(eng, k, before[k])
            else:
                delattr(eng, k)


def _wav(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(*shape, generator=g)).clamp(-1, 1)


def _split_equals_whole(eng, call):
    with _thresholds(eng, 0):
        whole = call().cpu()
    torch.cuda.synchronize()
    eng._ws_side.clear()
    with _thresholds(eng, 1):
        parts = call().cpu()
    assert eng._ws_side, "the call was expected to split (no side workspace was made)"
    assert whole.shape == parts.shape and bool(torch.isfinite(parts).all())
    same = np.array_equal(whole.numpy().view(np.uint8), parts.numpy().view(np.uint8))
    if not same:
        diff = (whole.double() - parts.double()).abs()
        pytest.fail(f"{int((diff > 0).sum())} of {diff.numel()} elements differ, max |diff| {diff.max().item():.3e}, "
                    f"rows {sorted(set(np.argwhere((diff > 0).numpy())[:, 0].tolist()))}")


@pytest.mark.parametrize("path", ["embed", "embed_bf16", "embed_bf16x3", "features_fp32", "features_bf16", "features_bf16x3"])
def test_equal_length_split_is_bit_identical(engine, path):
    wav = _wav((3, 720), 11).cuda()
    call = {"embed": lambda: engine.embed(wav), "embed_bf16": lambda: engine.embed_bf16(wav),
            "embed_bf16x3": lambda: engine.embed_bf16x3(wav)}.get(path)
    if call is None:
        call = lambda: engine.embed_features(wav, precision=path[len("features_"):])   # noqa: E731
    _split_equals_whole(engine, call)


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["embed", "features"])
def test_ragged_split_is_bit_identical(engine, kind, precision, where):
    waves = [_wav((n,), 20 + i) for i, n in enumerate(RAGGED_N)]
    assert 2 * sum(RAGGED_N[:2]) < sum(RAGGED_N)   # half of the audio lies in the last clip: the cut is behind clip 1
    if where == "device":
        waves = [w.cuda() for w in waves]
    fwd = engine.embed_ragged if kind == "embed" else engine.embed_features_ragged
    _split_equals_whole(engine, lambda: fwd(waves, precision=precision))


def test_thresholds_are_left_as_they_were(engine):
    before = {k: getattr(engine, k) for k in THRESHOLDS}
    with _thresholds(engine, 1):
        assert all(getattr(engine, k) == 1 for k in THRESHOLDS)
    assert {k: getattr(engine, k) for k in THRESHOLDS} == before
