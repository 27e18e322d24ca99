"""MI355X: framed members written on the device (zultra_hip_frame_members, zultra_memory_compress_bgzf, zultra_memory_compress_batch, the tool's
-f bgzf) in the product library, against the reference's members and Python's gzip / zlib. The cases are those of tests/test_frame_members_emu.py
(tests/frame_member_cases.py), with 1100 small inputs — more max-blocks than zh_stitch_scan has threads — and the command-line tool."""
import pytest

import frame_member_cases as M
import inflate_file_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    L.is_emulator = False   # (verify_cases.DeviceCopy: device memory comes from hipMalloc)
    return L


def test_parity_per_framing(gpu, checker):
    assert M.check_parity(gpu, checker) == 10


def test_many_small_inputs(gpu, checker):
    assert M.check_many_small(gpu, checker, 1100) == 1100


def test_many_small_inputs_capped_lanes(gpu):
    F.run_child(gpu.path, False, "__import__('frame_member_cases').check_many_small(L, None, 200)", dict(ZULTRA_HIP_GRID_CAP="8"))


def test_both_kinds_of_context_and_the_plain_layout(gpu, checker):
    M.check_both_contexts(gpu, checker)


def test_round_trip_on_the_device(gpu, checker):
    M.check_round_trip(gpu, checker)


def test_refusals(gpu):
    M.check_refusals(gpu)


def test_oversize_member_of_an_input_that_fits(gpu):
    M.check_oversize_member(gpu)


def test_a_batch_after_framing_verifies(gpu, checker):
    M.check_batch_after_framing(gpu, checker)


def test_host_api_bgzf(gpu, checker):
    assert M.check_bgzf_api(gpu, checker) == 5
    M.check_bgzf_api_verifies(gpu)


def test_host_api_batch(gpu, checker):
    M.check_batch_api(gpu, checker)


def test_cli_bgzf(gpu, checker, tmp_path):
    import zultra_amd.build
    M.check_cli(zultra_amd.build.CLI, tmp_path, checker)
