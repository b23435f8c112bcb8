"""CPU: the guarded-buffer helper (tests/guard.py) reports a write one element outside a guarded view, on either side, and
nothing for writes inside it; the same for the exact-size workspaces that ``guarded()`` gives an Engine."""
import pytest
import torch

import guard


def _outside(t: torch.Tensor, offset: int) -> torch.Tensor:
    """A one-element view at ``offset`` elements from t's first element (negative: in front of it), in t's storage."""
    return t.as_strided((1,), (1,), t.storage_offset() + offset)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64, torch.uint8])
def test_write_one_past_is_reported(dtype):
    g = guard.Guards()
    t = g.empty((5, 7), dtype, "cpu", name="out")
    t.fill_(3)                                    # every element of the view itself: not a guard
    assert g.damaged() == []
    _outside(t, t.numel()).fill_(1)
    assert g.damaged() == [("out", "after", t.element_size(), 0)]    # every byte of a 1 differs from the pattern
    with pytest.raises(AssertionError, match="out after"):
        g.check("case")


def test_write_one_before_is_reported():
    g = guard.Guards()
    t = g.empty((3, 4), torch.float32, "cpu", name="emb")
    _outside(t, -1).fill_(0.5)
    bad = g.damaged()
    assert len(bad) == 1 and bad[0][:2] == ("emb", "before") and bad[0][3] >= guard.OUT_GUARD - 4


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_a_view_at_an_element_offset_is_guarded_from_the_very_next_element(offset):
    """``empty_at``: the tensor begins ``offset`` floats behind an aligned address, and the float in front of it and the float
    behind it already belong to the guards."""
    g = guard.Guards()
    t = g.empty_at((3, 5), offset, torch.float32, "cpu", name="rows")
    assert t.shape == (3, 5) and t.is_contiguous() and t.data_ptr() % 16 == 4 * offset
    t.fill_(2.0)
    assert g.damaged() == []
    _outside(t, -1).fill_(0.0)
    assert [b[:3] for b in g.damaged()] == [("rows", "before", 4)] and g.damaged()[0][3] == guard.OUT_GUARD + 4 * offset - 4
    _outside(t, -1).view(torch.uint8).fill_(guard.PATTERN)
    _outside(t, t.numel()).fill_(0.0)
    assert g.damaged() == [("rows", "after", 4, 0)]


def test_bytes_equal_to_the_pattern_are_invisible_only_if_they_match():
    """The check compares bytes with the pattern: a float whose bytes are the pattern's (the one value that escapes) is not
    something a kernel produces; 0, NaN and any ordinary value are seen."""
    g = guard.Guards()
    t = g.empty((8,), torch.float32, "cpu")
    for v in (0.0, float("nan"), 1.0):
        _outside(t, 8).fill_(v)
        assert g.damaged(), v
    _outside(t, 8).view(torch.uint8).fill_(guard.PATTERN)     # restore
    assert g.damaged() == []


def test_engine_workspace_is_exact_and_guarded():
    """Inside guarded(): Engine._workspace hands out a fresh block of exactly the bytes asked for (no cached slack), records it
    in _ws / _ws_side, and an overflow past its end fails the check at the end of the block."""
    from nomad_amd.engine import Engine

    class _Fake:
        device = torch.device("cpu")
        _ws = None
        _ws_side = {}

    fake = _Fake()
    with pytest.raises(AssertionError, match=r"workspace\[0\] 1000 B after"):
        with guard.guarded(case="fake"):
            big = Engine._workspace(fake, 4096)
            ws = Engine._workspace(fake, 1000)
            assert ws.numel() == 1000 and fake._ws is ws and ws.data_ptr() != big.data_ptr()
            side = Engine._workspace(fake, 300, side=1)
            assert side.numel() == 300 and fake._ws_side[1] is side
            ws.fill_(0)
            side.fill_(0)
            _outside(ws, 1000).fill_(0)
    assert Engine._workspace is not None and "guard" not in Engine._workspace.__qualname__
    with guard.guarded(case="clean") as g:
        Engine._workspace(fake, 64).fill_(1)
    assert len(g.items) == 1


def test_engine_torch_stand_in_guards_device_tensors_only():
    from nomad_amd import engine as engine_mod
    real = engine_mod.torch
    with guard.guarded() as g:
        assert engine_mod.torch is not real
        host = engine_mod.torch.empty(4, 5, dtype=torch.float32)
        assert host.shape == (4, 5) and not g.items          # host tensors (pinned staging) pass through
    assert engine_mod.torch is real
