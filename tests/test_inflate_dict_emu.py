"""CPU (no GPU needed): zultra_hip_inflate_streams_dict — the dictionary form of the batched inflate kernel, zh_inflate_streams_dict of
zultra_amd/csrc/zh_inflate_out.h — and zultra_memory_decompress_dict in the lock-step emulator build of the product's sources, against Python's zlib
with zdict: zlib's own streams against dictionaries of 1 .. 70000 bytes, hand-written token streams at the edges of the history, rejects held to
their reason, equivalence with the plain call, a seeded token fuzz, every bit flipped and every byte cut, bad arguments, the host API.
tests/test_inflate_dict_gpu.py runs the same cases (tests/inflate_dict_cases.py) on the MI355X, with the larger sizes."""
import os
import sys

import pytest

import inflate_dict_cases as D

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    L = Lib(build_emu.build())
    L.is_emulator = True    # (verify_cases.DeviceCopy: device memory is host memory)
    return L


@pytest.mark.parametrize("k", range(len(D.DICT_SIZES)))
def test_zlib_streams_with_zdict(emu, k):
    """The device dictionary at every offset into a dword for two of the sizes, at one (taking turns) for the others."""
    size = D.DICT_SIZES[k]
    assert D.check_zlib_streams(emu, size, (0, 1, 2, 3) if size in (259, 32769) else (k & 3,)) >= 1


def test_hand_written_matches_into_the_history(emu):
    assert D.check_hand(emu) >= 24


def test_distance_one_byte_too_far_is_reason_4(emu):
    assert D.check_too_far(emu) >= 8


def test_plain_call_rejects_every_dictionary_stream(emu):
    assert D.check_plain_call_rejects(emu) >= 24


def test_dst_cap_on_a_straddling_match(emu):
    D.check_dst_cap(emu)


def test_equivalence_with_the_plain_call(emu):
    assert D.check_equivalence(emu) >= 65


def test_token_stream_fuzz(emu):
    D.check_token_fuzz(emu, 20261019, 16, 150)


def test_every_bit_flipped(emu):
    n, benign = D.check_flips(emu)
    assert n >= 2000 and benign > 0


def test_cut_at_every_byte(emu):
    assert D.check_cuts(emu) >= 300


def test_bad_arguments(emu):
    D.check_bad_arguments(emu)


def test_host_api_round_trip(emu):
    D.check_host_round_trip(emu, 3000, 258)


def test_host_api_zlib_framing(emu):
    D.check_host_zlib_framing(emu, 3000)
