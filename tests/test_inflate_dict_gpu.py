"""GPU (MI355X): zultra_hip_inflate_streams_dict — the dictionary form of the batched inflate kernel, zh_inflate_streams_dict of
zultra_amd/csrc/zh_inflate_out.h —, zultra_memory_decompress_dict and zultra_amd_cli -D in the product library, against Python's zlib with zdict.
The cases are those of tests/test_inflate_dict_emu.py (tests/inflate_dict_cases.py), with the larger sizes."""
import os

import pytest

import inflate_dict_cases as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    L.is_emulator = False   # (verify_cases.DeviceCopy: device memory comes from hipMalloc)
    return L


@pytest.mark.parametrize("k", range(len(D.DICT_SIZES)))
def test_zlib_streams_with_zdict(gpu, k):
    """The device dictionary at every offset into a dword."""
    assert D.check_zlib_streams(gpu, D.DICT_SIZES[k], (0, 1, 2, 3)) >= 1


def test_hand_written_matches_into_the_history(gpu):
    assert D.check_hand(gpu) >= 24


def test_distance_one_byte_too_far_is_reason_4(gpu):
    assert D.check_too_far(gpu) >= 8


def test_plain_call_rejects_every_dictionary_stream(gpu):
    assert D.check_plain_call_rejects(gpu) >= 24


def test_dst_cap_on_a_straddling_match(gpu):
    D.check_dst_cap(gpu)


def test_equivalence_with_the_plain_call(gpu):
    assert D.check_equivalence(gpu) >= 65


def test_token_stream_fuzz(gpu, tmp_path):
    """512 items of about 400 tokens in flight: 128 generated streams, each four times; then the same batch with eight waves striding."""
    import zultra_amd
    made = D.check_token_fuzz(gpu, 20261019, 128, 400, copies=4)
    D.check_token_fuzz_strided(zultra_amd.LIB_PATH, False, made, 4, tmp_path)


def test_every_bit_flipped(gpu):
    n, benign = D.check_flips(gpu)
    assert n >= 2000 and benign > 0


def test_cut_at_every_byte(gpu):
    assert D.check_cuts(gpu) >= 300


def test_bad_arguments(gpu):
    D.check_bad_arguments(gpu)


@pytest.mark.parametrize("dict_size", [1, 258, 32768, 70000])
def test_host_api_round_trip(gpu, dict_size):
    D.check_host_round_trip(gpu, 100000, dict_size)


def test_host_api_zlib_framing(gpu):
    D.check_host_zlib_framing(gpu, 100000)


def test_cli_dictionary(gpu, tmp_path):
    import zultra_amd
    D.check_cli(os.path.join(os.path.dirname(zultra_amd.LIB_PATH), "zultra_amd_cli"), tmp_path)
