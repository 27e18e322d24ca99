"""GPU (MI355X): zultra_hip_inflate_members — zh_frame_heads and zh_check_members of zultra_amd/csrc/zh_inflate_check.h around the inflate kernels — and
zultra_memory_decompress_batch in the product library, against Python's zlib. The cases are those of tests/test_inflate_members_emu.py
(tests/inflate_member_cases.py), with the larger sizes."""
import pytest

import inflate_member_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    L.is_emulator = False   # (verify_cases.DeviceCopy: device memory comes from hipMalloc)
    return L


def test_hand_built_gzip_headers(gpu):
    assert M.check_gzip_headers(gpu) >= 70


def test_every_header_bit_flipped(gpu):
    """Every accept case, those with XLEN 300 included."""
    n, benign = M.check_header_flips(gpu, big=True)
    assert n >= 30000 and benign > 0


def test_zlib_headers(gpu):
    assert M.check_zlib_headers(gpu) >= 150


@pytest.mark.parametrize("dict_size", [1, 32768, 70000])
def test_zlib_fdict_and_dictionaries(gpu, dict_size):
    M.check_zlib_fdict(gpu, dict_size, leads=(0, 1, 2, 3))


def test_cut_at_every_byte(gpu):
    assert M.check_cuts(gpu, big=True) >= 51 * 75   # (48 gzip and 3 zlib accept cases, each of at least 75 bytes)


def test_trailers(gpu):
    M.check_trailers(gpu)


@pytest.mark.parametrize("framing", [M.GZIP, M.ZLIB])
def test_checksum_edges(gpu, framing):
    assert M.check_checksum_edges(gpu, framing) == 36


def test_both_forms_in_one_batch(gpu):
    assert M.check_mixed(gpu) >= 90


def test_both_forms_with_a_capped_grid(gpu):
    import zultra_amd
    M.check_mixed_strided(zultra_amd.LIB_PATH, False)


def test_alignment(gpu):
    M.check_alignment(gpu)


def test_concatenated_gzip_members(gpu):
    M.check_concatenated(gpu)


def test_equivalence_with_the_raw_calls(gpu):
    assert M.check_equivalence(gpu) >= 80


def test_own_files_batch_framed(gpu):
    M.check_own_files(gpu, 200)


def test_host_api(gpu):
    M.check_host_api(gpu, 100000)


def test_bad_arguments(gpu):
    M.check_bad_arguments(gpu)
