"""CPU (no GPU needed): ZIP archives written on the device — zh_zip_scan, zh_zip_records and zh_zip_copy of zultra_amd/csrc/zh_zip.h,
zultra_hip_zip_members, zultra_zip_end_records and zultra_memory_compress_zip — in the lock-step emulator build of the product's sources, against
archives put together with struct.pack around the reference's streams, and Python's zipfile (tests/zip_cases.py).
tests/test_zip_gpu.py runs the same cases on the MI355X, with the larger counts, the ZIP64 end records and the command-line tool."""
import os
import sys

import pytest

import inflate_file_cases as F
import zip_cases as Z

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    L = Lib(build_emu.build())
    L.is_emulator = True    # (verify_cases.DeviceCopy: device memory is host memory)
    return L


def test_every_source_and_destination_alignment(emu, checker):
    assert Z.check_alignment_grid(emu, checker) >= 40


def test_many_entries(emu, checker):
    assert Z.check_many(emu, checker, 40) == 40


def test_many_entries_capped_grid(emu):
    """40 entries with eight lanes in zh_zip_records and eight workgroups in zh_zip_copy. In a process of its own (the cap is read when a context is created)."""
    F.run_child(emu.path, True, "__import__('zip_cases').check_many(L, None, 40)", dict(ZULTRA_HIP_GRID_CAP="8"))


def test_large_entries_in_slices(emu, checker):
    """(40 000 bytes of noise are five slices of zh_zip_copy; the emulator is too slow for 200 KiB of text, whose stream here is part of one slice)"""
    comp = Z.check_large(emu, checker, 40000, 6000)
    assert comp[0] > 4 * 8192, comp


def test_large_entries_capped_grid(emu):
    F.run_child(emu.path, True, "__import__('zip_cases').check_large(L, __import__('frame_member_cases').make_checker(), 40000, 3000)", dict(ZULTRA_HIP_GRID_CAP="4"))


def test_host_api_both_kinds_of_context(emu, checker):
    assert Z.check_api_mixed(emu, checker, 9000, 3000) == 7


def test_host_api_empty_entries(emu, checker):
    Z.check_api_empty_entries(emu, checker)


def test_host_api_refusals(emu):
    Z.check_api_refusals(emu)


def test_round_trip_on_the_device_and_the_stream_buffer(emu, checker):
    Z.check_round_trip(emu, checker, 2)


def test_refusals(emu, checker):
    Z.check_refusals(emu, checker)


def test_end_records(emu):
    Z.check_end_records(emu)
