"""MI355X: ZIP archives written on the device (zultra_hip_zip_members, zultra_memory_compress_zip, the tool's -a) in the product library, against
archives put together with struct.pack around the reference's streams, and Python's zipfile. The cases are those of tests/test_zip_emu.py
(tests/zip_cases.py), with 1100 entries — more than zh_zip_scan has threads —, entries of 200 KiB, the ZIP64 end records and the command-line tool."""
import pytest

import inflate_file_cases as F
import zip_cases as Z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    L.is_emulator = False   # (verify_cases.DeviceCopy: device memory comes from hipMalloc)
    return L


def test_every_source_and_destination_alignment(gpu, checker):
    assert Z.check_alignment_grid(gpu, checker) >= 40


def test_many_entries(gpu, checker):
    assert Z.check_many(gpu, checker, 1100) == 1100


def test_many_entries_capped_grid(gpu):
    F.run_child(gpu.path, False, "__import__('zip_cases').check_many(L, None, 1100)", dict(ZULTRA_HIP_GRID_CAP="8"))


def test_large_entries_in_slices(gpu, checker):
    comp = Z.check_large(gpu, checker, 204800, 204800)
    assert comp[0] > 24 * 8192 and comp[1] > 4 * 8192, comp


def test_large_entries_capped_grid(gpu):
    F.run_child(gpu.path, False, "__import__('zip_cases').check_large(L, __import__('frame_member_cases').make_checker(), 204800, 204800)", dict(ZULTRA_HIP_GRID_CAP="4"))


def test_host_api_both_kinds_of_context(gpu, checker):
    assert Z.check_api_mixed(gpu, checker, 70000, 8191) == 7


def test_host_api_empty_entries(gpu, checker):
    Z.check_api_empty_entries(gpu, checker)


def test_host_api_refusals(gpu):
    Z.check_api_refusals(gpu)


def test_round_trip_on_the_device_and_the_stream_buffer(gpu, checker):
    Z.check_round_trip(gpu, checker, 12)


def test_refusals(gpu, checker):
    Z.check_refusals(gpu, checker)


def test_end_records(gpu):
    Z.check_end_records(gpu)


def test_zip64_end_records_of_65537_entries(gpu):
    Z.check_zip64_end(gpu)


def test_cli_archive(gpu, checker, tmp_path):
    import zultra_amd.build
    Z.check_cli(zultra_amd.build.CLI, gpu, tmp_path, checker)
