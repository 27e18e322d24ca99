"""CPU (no GPU needed): framed members written on the device — zh_stitch_scan with room for headers and trailers, zh_frame_clear and zh_frame_members
of zultra_amd/csrc/zh_frame.h, zultra_hip_frame_members, zultra_memory_compress_bgzf and zultra_memory_compress_batch — in the lock-step emulator
build of the product's sources, against the reference's members and Python's gzip / zlib (tests/frame_member_cases.py).
tests/test_frame_members_gpu.py runs the same cases on the MI355X, with the larger counts and the command-line tool."""
import os
import sys

import pytest

import frame_member_cases as M
import inflate_file_cases as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    L = Lib(build_emu.build())
    L.is_emulator = True    # (verify_cases.DeviceCopy: device memory is host memory)
    return L


def test_parity_per_framing(emu, checker):
    assert M.check_parity(emu, checker) == 10


def test_many_small_inputs_capped_lanes(emu):
    """40 inputs with eight lanes in zh_frame_members: every lane frames five members or six. In a process of its own (the cap is read when a context is created)."""
    F.run_child(emu.path, True, "__import__('frame_member_cases').check_many_small(L, None, 40)", dict(ZULTRA_HIP_GRID_CAP="8"))


def test_many_small_inputs(emu, checker):
    assert M.check_many_small(emu, checker, 40) == 40


def test_both_kinds_of_context_and_the_plain_layout(emu, checker):
    M.check_both_contexts(emu, checker)


def test_round_trip_on_the_device(emu, checker):
    M.check_round_trip(emu, checker)


def test_refusals(emu):
    M.check_refusals(emu)


def test_oversize_member_of_an_input_that_fits(emu):
    M.check_oversize_member(emu)


def test_a_batch_after_framing_verifies(emu, checker):
    M.check_batch_after_framing(emu, checker)


def test_host_api_bgzf(emu, checker):
    assert M.check_bgzf_api(emu, checker) == 5
    M.check_bgzf_api_verifies(emu)


def test_host_api_batch(emu, checker):
    M.check_batch_api(emu, checker)
