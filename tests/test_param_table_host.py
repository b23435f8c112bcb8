"""CPU: the layout of the flat parameter vector is pinned by a recorded table, independently of the code that produces it.

Offsets into the master vector are observable - nomad_train_segment, nomad_train_read / nomad_train_write, saved optimiser
state - so the order (encoder front, layers, conv extractor, head last; q / k / v fused and reported as three segments) must
not move.  tests/golden/train_segments.json is what the library returned before the parameter inventory became one table."""
import ctypes as C
import json
import os

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "train_segments.json")) as f:
        return json.load(f)


def _table(lib):
    name = C.create_string_buffer(128)
    off, cnt = C.c_size_t(), C.c_size_t()
    segs = []
    for i in range(lib.nomad_train_num_segments()):
        assert lib.nomad_train_segment(i, name, 128, C.byref(off), C.byref(cnt)) == 0, lib.nomad_last_error()
        segs.append([name.value.decode(), off.value, cnt.value])
    total, head = C.c_size_t(), C.c_size_t()
    assert lib.nomad_train_param_count(C.byref(total), C.byref(head)) == 0, lib.nomad_last_error()
    return segs, total.value, head.value


@pytest.mark.parametrize("diag", [False, True], ids=["product", "diag"])
def test_segment_table_is_the_recorded_one(built_lib, golden, diag):
    from nomad_amd import _lib
    segs, total, head = _table(_lib.load(diag=diag))
    assert len(segs) == len(golden["segments"])
    for i, (got, want) in enumerate(zip(segs, golden["segments"])):
        assert got == want, i
    assert (total, head) == (golden["total"], golden["head_begin"])


def test_recorded_table_is_a_partition_with_the_head_last(golden):
    """The fixture itself: contiguous from 0 to total in the recorded order, and head_begin splits body from head."""
    off = 0
    for name, o, n in golden["segments"]:
        assert o == off and n > 0 and n % 4 == 0, name
        off += n
    assert off == golden["total"]
    head = [name for name, o, _ in golden["segments"] if o >= golden["head_begin"]]
    assert head == ["embedding_layer.1.weight", "embedding_layer.1.bias"]
