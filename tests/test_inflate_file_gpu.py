"""GPU (MI355X): the member index of a BGZF / multi-member gzip file — zh_ix_tiles, zh_ix_resolve and zh_ix_items of
zultra_amd/csrc/zh_inflate_index.h —, zultra_hip_index_members, zultra_hip_inflate_file, zultra_memory_decompress_members and the command-line tool's
-m in the product library. The cases are those of tests/test_inflate_file_emu.py (tests/inflate_file_cases.py), with the larger sizes."""
import pytest

import inflate_file_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    L.is_emulator = False   # (verify_cases.DeviceCopy: device memory comes from hipMalloc)
    return L


def test_index_of_every_file_default_tile(gpu):
    """Headers, boundaries, decoys and stops (cases 1 to 4) with the default tile."""
    assert F.check_index_files(gpu) >= 300


@pytest.mark.parametrize("tile", F.TILES)
def test_index_of_every_file_small_tiles(gpu, tile):
    import zultra_amd
    F.run_child(zultra_amd.LIB_PATH, False, "F.check_index_files(L)", dict(ZULTRA_HIP_INDEX_TILE=str(tile)))


def test_index_with_a_capped_grid(gpu):
    import zultra_amd
    F.run_child(zultra_amd.LIB_PATH, False, "F.check_index_files(L)", dict(ZULTRA_HIP_INDEX_TILE="100", ZULTRA_HIP_GRID_CAP="8"))


def test_whole_files(gpu):
    assert F.check_whole_files(gpu, big=True) == 18


def test_whole_files_small_tiles_capped_grid(gpu):
    import zultra_amd
    F.run_child(zultra_amd.LIB_PATH, False, "F.check_whole_files(L, True)", dict(ZULTRA_HIP_INDEX_TILE="256", ZULTRA_HIP_GRID_CAP="8"))


def test_eight_mebibytes_across_the_default_tile(gpu):
    F.check_large_file(gpu)


def test_damaged_members_and_too_little_room(gpu):
    F.check_damage(gpu)


def test_own_files_batch_framed_as_bgzf(gpu):
    F.check_own_files(gpu, 200)


def test_host_api(gpu):
    F.check_host_api(gpu)


def test_command_line_tool(gpu, tmp_path):
    import zultra_amd.build
    F.check_cli(zultra_amd.build.CLI, tmp_path)


def test_bad_arguments(gpu):
    F.check_bad_arguments(gpu)
