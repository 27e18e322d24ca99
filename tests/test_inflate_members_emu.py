"""CPU (no GPU needed): zultra_hip_inflate_members — zh_frame_heads and zh_check_members of zultra_amd/csrc/zh_inflate_check.h around the inflate kernels
— and zultra_memory_decompress_batch in the lock-step emulator build of the product's sources, against Python's zlib: hand-built gzip and zlib
headers, every header bit flipped and every byte cut, trailers, the checksum at the sizes where the kernel's slices and rounds change, alignment,
concatenated members, equivalence with the raw calls, the library's own output, the host API, bad arguments.
tests/test_inflate_members_gpu.py runs the same cases (tests/inflate_member_cases.py) on the MI355X, with the larger sizes."""
import os
import sys

import pytest

import inflate_member_cases as M

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    L = Lib(build_emu.build())
    L.is_emulator = True    # (verify_cases.DeviceCopy: device memory is host memory)
    return L


def test_hand_built_gzip_headers(emu):
    assert M.check_gzip_headers(emu) >= 70


def test_every_header_bit_flipped(emu):
    """The headers of up to 60 bytes and one with XLEN 300."""
    n, benign = M.check_header_flips(emu, big=False)
    assert n >= 4000 and benign > 0


def test_zlib_headers(emu):
    assert M.check_zlib_headers(emu) >= 150


@pytest.mark.parametrize("dict_size", [1, 32768, 70000])
def test_zlib_fdict_and_dictionaries(emu, dict_size):
    M.check_zlib_fdict(emu, dict_size, leads=(1 + dict_size % 3,))


def test_cut_at_every_byte(emu):
    assert M.check_cuts(emu, big=False) >= 2000


def test_trailers(emu):
    M.check_trailers(emu)


@pytest.mark.parametrize("framing", [M.GZIP, M.ZLIB])
def test_checksum_edges(emu, framing):
    assert M.check_checksum_edges(emu, framing) == 36


def test_both_forms_in_one_batch(emu):
    assert M.check_mixed(emu) >= 90


def test_both_forms_with_a_capped_grid(emu):
    M.check_mixed_strided(emu.path, True)


def test_alignment(emu):
    M.check_alignment(emu)


def test_concatenated_gzip_members(emu):
    M.check_concatenated(emu)


def test_equivalence_with_the_raw_calls(emu):
    assert M.check_equivalence(emu) >= 80


def test_own_files_batch_framed(emu):
    M.check_own_files(emu, 18)   # (the emulator spends its time compressing them)


def test_host_api(emu):
    M.check_host_api(emu, 3000)


def test_bad_arguments(emu):
    M.check_bad_arguments(emu)
