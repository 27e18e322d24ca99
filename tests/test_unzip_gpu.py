"""MI355X: ZIP archives read on the device (zultra_hip_zip_index, zultra_hip_unzip, zultra_memory_decompress_zip, the tool's -x -a) in the product
library, against the serial walk of the central directory, Python's zipfile / zlib and hand-made archives. The cases are those of
tests/test_unzip_emu.py (tests/unzip_cases.py), with about 1100 entries — more than one workgroup of every per-entry kernel —, a stored entry of
200 KiB, the 65 537-entry archive with its ZIP64 end records and a directory of several default tiles, and the command-line tool."""
import pytest

import inflate_file_cases as F
import unzip_cases as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    L.is_emulator = False   # (verify_cases.DeviceCopy: device memory comes from hipMalloc)
    return L


def test_index_equals_the_serial_walk(gpu):
    assert U.check_index_tiles(gpu) == 34


@pytest.mark.parametrize("tile", U.TILES)
def test_index_at_small_tiles(gpu, tile):
    F.run_child(gpu.path, False, "__import__('unzip_cases').check_index_tiles(L)", dict(ZULTRA_HIP_INDEX_TILE=str(tile)))


def test_stops_and_caps(gpu):
    assert U.check_stops(gpu) == 10


def test_stops_at_tile_32(gpu):
    F.run_child(gpu.path, False, "__import__('unzip_cases').check_stops(L)", dict(ZULTRA_HIP_INDEX_TILE="32"))


def test_what_other_producers_write(gpu):
    assert U.check_foreign(gpu, 204800, 1100) == 1112 + 1111


@pytest.mark.parametrize("cap", (4, 8))
def test_what_other_producers_write_capped_grid(gpu, cap):
    F.run_child(gpu.path, False, "__import__('unzip_cases').check_foreign(L, 204800, 1100, full=False)", dict(ZULTRA_HIP_GRID_CAP=str(cap)))


def test_stored_copy_at_every_alignment(gpu):
    assert U.check_copy_alignment(gpu) >= 256


def test_reasons(gpu):
    assert U.check_reasons(gpu) == 20


def test_round_trip_without_leaving_the_device(gpu, checker):
    U.check_device_round_trip(gpu, checker, 4)


def test_host_api(gpu):
    U.check_host_api(gpu, 70000, 8191)


def test_end_records(gpu):
    U.check_find_end(gpu)


def test_zip64_archive_of_65537_entries(gpu):
    U.check_zip64_archive(gpu)


def test_cli_extracts_archives(gpu, tmp_path):
    import zultra_amd.build
    U.check_cli(zultra_amd.build.CLI, tmp_path)
