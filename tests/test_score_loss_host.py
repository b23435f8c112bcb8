"""CPU: the host-side pieces of the differentiable NOMAD score (``Nomad.score``, ``nomad_cdist_backward``) that need no GPU -
the pure check of the ``references`` argument, and the two new entry points in the header and in the binding
(``test_abi.py::test_header_and_binding_agree`` holds the two lists, and the library's exports, to each other)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from nomad_amd import _lib
from nomad_amd.nomad import check_references

NEW = ("nomad_cdist_backward_scratch_bytes", "nomad_cdist_backward")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows", [1, 5, 1000])
def test_references_that_are_embeddings_pass(rows, dtype):
    assert check_references(torch.zeros(rows, 256, dtype=dtype)) is None
    assert check_references(torch.zeros(rows, 256, dtype=dtype, requires_grad=True)) is None


@pytest.mark.parametrize("shape", [(256,), (5, 128), (5, 257), (5, 768), (2, 5, 256), (5, 256, 1), ()])
def test_references_of_another_shape_are_refused(shape):
    with pytest.raises(ValueError, match=r"\(Nr, 256\)"):
        check_references(torch.zeros(shape))


def test_references_without_a_row_are_refused():
    with pytest.raises(ValueError, match="at least one reference"):
        check_references(torch.zeros(0, 256))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.uint8, torch.bool])
def test_references_of_a_non_floating_type_are_refused(dtype):
    with pytest.raises(TypeError, match="floating-point"):
        check_references(torch.zeros(5, 256, dtype=dtype))


@pytest.mark.parametrize("value", [None, [[0.0] * 256], "refs.csv"])
def test_references_that_are_no_tensor_are_refused(value):
    with pytest.raises(TypeError, match="must be a tensor"):
        check_references(value)


def test_the_check_of_references_reads_no_value():
    """Pure: type, dtype and shape only - a tensor without storage (the meta device) passes or fails like a real one."""
    assert check_references(torch.empty(3, 256, device="meta")) is None
    with pytest.raises(ValueError):
        check_references(torch.empty(3, 255, device="meta"))


def test_binding_and_header_carry_the_backward_of_cdist():
    text = open(os.path.join(ROOT, "include", "nomad_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} is not declared in include/nomad_hip.h"
    res, args = _lib.SIGNATURES["nomad_cdist_backward_scratch_bytes"]
    assert res is C.c_int and args == [C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    # ctx, a, Na, b, Nb, D, gdist, gmean, da, db, scratch, scratch_bytes, stream
    res, args = _lib.SIGNATURES["nomad_cdist_backward"]
    assert res is C.c_int and len(args) == 13
    assert [i for i, t in enumerate(args) if t is C.c_int] == [2, 4, 5] and args[11] is C.c_size_t
    # entry points were added, none changed: the binary-interface number stays
    assert int(re.search(r"#define NOMAD_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 3
