"""GPU (MI355X): a byte range of a BGZF / multi-member gzip file — zh_rg_select, zh_rg_items and zh_rg_edges of zultra_amd/csrc/zh_inflate_range.h under
zultra_hip_inflate_range —, zultra_memory_index_gzi, zultra_memory_decompress_range and the command-line tool's -r and -i in the product library. The
cases are those of tests/test_inflate_range_emu.py (tests/inflate_range_cases.py), with the larger sizes."""
import pytest

import inflate_file_cases as F
import inflate_range_cases as R

pytestmark = pytest.mark.gpu

CHILD = "__import__('inflate_range_cases').check_tiles(L)"


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    L.is_emulator = False   # (verify_cases.DeviceCopy: device memory comes from hipMalloc)
    return L


def test_every_range_of_a_tiny_file(gpu):
    assert R.check_tiny(gpu) == 2 * (15 * 16 + 6)


def test_edges_at_real_sizes(gpu):
    """Every boundary point to every later one."""
    assert R.check_sizes(gpu) >= 150


@pytest.mark.parametrize("tile", (32, 100, 256))
def test_small_tiles(gpu, tile):
    import zultra_amd
    F.run_child(zultra_amd.LIB_PATH, False, CHILD, dict(ZULTRA_HIP_INDEX_TILE=str(tile)))


def test_small_tiles_with_a_capped_grid(gpu):
    import zultra_amd
    F.run_child(zultra_amd.LIB_PATH, False, CHILD, dict(ZULTRA_HIP_INDEX_TILE="100", ZULTRA_HIP_GRID_CAP="8"))


def test_placement(gpu):
    assert R.check_placement(gpu) == 96


def test_only_the_covered_members(gpu):
    R.check_only_covered(gpu)


def test_stops(gpu):
    R.check_stops(gpu)


def test_room(gpu):
    R.check_room(gpu)


def test_bad_arguments(gpu):
    R.check_bad_arguments(gpu)


def test_gzi_index(gpu):
    R.check_gzi(gpu, big=True)


def test_eight_mebibytes_across_the_default_tile(gpu):
    R.check_large_file(gpu)


def test_own_files_batch_framed_as_bgzf(gpu):
    R.check_own_files(gpu, 200)


def test_command_line_tool(gpu, tmp_path):
    import zultra_amd.build
    R.check_cli(zultra_amd.build.CLI, tmp_path)
