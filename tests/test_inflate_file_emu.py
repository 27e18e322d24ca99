"""CPU (no GPU needed): the member index of a BGZF / multi-member gzip file — zh_ix_tiles, zh_ix_resolve and zh_ix_items of
zultra_amd/csrc/zh_inflate_index.h —, zultra_hip_index_members, zultra_hip_inflate_file and zultra_memory_decompress_members in the lock-step emulator
build of the product's sources, against the serial walk of tests/inflate_file_cases.py, Python's gzip and zultra_hip_inflate_members.
tests/test_inflate_file_gpu.py runs the same cases on the MI355X, with the larger sizes."""
import os
import sys

import pytest

import inflate_file_cases as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    L = Lib(build_emu.build())
    L.is_emulator = True    # (verify_cases.DeviceCopy: device memory is host memory)
    return L


def test_index_of_every_file_default_tile(emu):
    """Headers, boundaries, decoys and stops (cases 1 to 4) with the default tile."""
    assert F.check_index_files(emu) >= 300


@pytest.mark.parametrize("tile", F.TILES)
def test_index_of_every_file_small_tiles(emu, tile):
    F.run_child(emu.path, True, "F.check_index_files(L)", dict(ZULTRA_HIP_INDEX_TILE=str(tile)))


def test_index_with_a_capped_grid(emu):
    F.run_child(emu.path, True, "F.check_index_files(L)", dict(ZULTRA_HIP_INDEX_TILE="100", ZULTRA_HIP_GRID_CAP="8"))


def test_whole_files(emu):
    assert F.check_whole_files(emu, big=False) == 18


def test_whole_files_small_tiles_capped_grid(emu):
    F.run_child(emu.path, True, "F.check_whole_files(L, False)", dict(ZULTRA_HIP_INDEX_TILE="256", ZULTRA_HIP_GRID_CAP="8"))


def test_damaged_members_and_too_little_room(emu):
    F.check_damage(emu)


def test_own_files_batch_framed_as_bgzf(emu):
    F.check_own_files(emu, 18)   # (the emulator spends its time compressing them)


def test_host_api(emu):
    F.check_host_api(emu)


def test_bad_arguments(emu):
    F.check_bad_arguments(emu)
