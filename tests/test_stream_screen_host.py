"""CPU: the parts of the stream-order screen (tests/stream_screen.py) that need no GPU - which host arrays it sees on their way
into the C ABI, and that what it overwrites them with is valid input."""
import ctypes as C

import torch

import stream_screen
from nomad_amd import _lib
from nomad_amd.engine import Engine


class _FakeLib:
    """Records what reaches the library; every entry point returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_every_host_array_slot_of_the_abi_has_a_role():
    """An entry point that takes more host arrays than the clips' lengths is listed with one role per array, and every role has
    replacement values."""
    host_only = {"nomad_wav_probe", "nomad_wav_frames_at", "nomad_wav_read_rows", "nomad_window_cover", "nomad_ragged_metadata",
                 "nomad_profile_read"}      # no stream argument: nothing of theirs is in flight after the return
    for name, (_, argtypes) in _lib.SIGNATURES.items():
        slots = [t for t in argtypes if isinstance(t, type) and issubclass(t, C._Pointer) and t._type_ in stream_screen._HOST_ELEMENTS]
        if len(slots) > 1 and name not in host_only:
            assert name in stream_screen._ROLES and len(stream_screen._ROLES[name]) == len(slots), name
    for roles in stream_screen._ROLES.values():
        for role in roles:
            assert len(stream_screen._replacement(role, 5)) == 5


def test_arrays_are_taken_by_role_and_overwritten_in_place():
    fake = _FakeLib()
    watch = stream_screen.HostArrays(fake)
    lens, levels = (C.c_int * 3)(720, 9001, 16384), (C.c_double * 2)(0.0, 15.0)
    assert watch.nomad_degrade_noise(None, 1, 3, 16384, lens, 2, 5000, levels, 2, 3, 4, 5, 6, None) == 0
    assert watch.nomad_embed(None, 1, 3, 16384, None, None, 2, None, 3, 4, None) == 0          # no host array: passed straight through
    assert watch.nomad_l1_loss_weighted(None, 1, 2, 3, 4, 50, 3, None, (C.c_float * 13)(*[1.0] * 13), 1, 5, 6, 7, 8, None) == 0
    assert [(n, r) for n, r, _ in watch.taken] == [("nomad_degrade_noise", "lens"), ("nomad_degrade_noise", "levels"),
                                                   ("nomad_l1_loss_weighted", "weights")]
    assert [c[0] for c in fake.calls] == ["nomad_degrade_noise", "nomad_embed", "nomad_l1_loss_weighted"]
    assert fake.calls[0][1][4] is lens, "the library got the caller's own array"
    assert watch.overwrite() == 3
    assert list(lens) == [stream_screen.MIN_CLIP] * 3 and list(levels) == [7.0, 7.0] and list(watch.taken[2][2]) == [0.25] * 13


def test_the_replacement_span_table_is_valid_for_the_shortest_clip():
    """Whatever the real table was, the arrays that replace it form a table ``Engine._check_table`` accepts for clips of one frame:
    a kernel that read them would stay inside every buffer."""
    R, S = 5, 7
    row_clip, row_ptr = stream_screen._replacement("row_clip", R), stream_screen._replacement("row_ptr", R + 1)
    flat = stream_screen._replacement("spans", 2 * S)
    spans = list(zip(flat[0::2], flat[1::2]))
    assert max(row_ptr) < S      # every row's range lies inside the spans the real table had (it has at least one span per row)
    table = (row_clip, row_ptr[:-1] + [row_ptr[-1]], spans[:row_ptr[-1]])
    Engine._check_table(table, [1] * 4)
    assert stream_screen._replacement("lens", 3) == [400] * 3 and torch.tensor(stream_screen._replacement("levels", 2)).isfinite().all()
