"""CPU (no GPU needed): ZIP archives read on the device — the directory index (zh_uz_tiles, zh_uz_resolve, zh_uz_entries), zh_uz_locals, zh_uz_copy and
the ZIP form of zh_check_members (zultra_amd/csrc/zh_unzip.h, zh_inflate_check.h), zultra_hip_zip_index, zultra_hip_unzip, zultra_zip_find_end and
zultra_memory_decompress_zip — in the lock-step emulator build of the product's sources, against the serial walk, Python's zipfile / zlib and hand-made
archives (tests/unzip_cases.py). tests/test_unzip_gpu.py runs the same cases on the MI355X, with the larger counts, the ZIP64 archive and the tool."""
import os
import sys

import pytest

import inflate_file_cases as F
import unzip_cases as U

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    L = Lib(build_emu.build())
    L.is_emulator = True    # (verify_cases.DeviceCopy: device memory is host memory)
    return L


def test_index_equals_the_serial_walk(emu):
    assert U.check_index_tiles(emu) == 34


@pytest.mark.parametrize("tile", U.TILES)
def test_index_at_small_tiles(emu, tile):
    F.run_child(emu.path, True, "__import__('unzip_cases').check_index_tiles(L)", dict(ZULTRA_HIP_INDEX_TILE=str(tile)))


def test_stops_and_caps(emu):
    assert U.check_stops(emu) == 10


def test_stops_at_tile_32(emu):
    F.run_child(emu.path, True, "__import__('unzip_cases').check_stops(L)", dict(ZULTRA_HIP_INDEX_TILE="32"))


def test_what_other_producers_write(emu):
    assert U.check_foreign(emu, 40000, 30) == 42 + 41


@pytest.mark.parametrize("cap", (4, 8))
def test_what_other_producers_write_capped_grid(emu, cap):
    F.run_child(emu.path, True, "__import__('unzip_cases').check_foreign(L, 40000, 30, full=False)", dict(ZULTRA_HIP_GRID_CAP=str(cap)))


def test_stored_copy_at_every_alignment(emu):
    assert U.check_copy_alignment(emu) >= 256


def test_reasons(emu):
    assert U.check_reasons(emu) == 20


def test_round_trip_without_leaving_the_device(emu, checker):
    U.check_device_round_trip(emu, checker, 1)


def test_host_api(emu):
    U.check_host_api(emu, 8200, 1000)


def test_end_records(emu):
    U.check_find_end(emu)
