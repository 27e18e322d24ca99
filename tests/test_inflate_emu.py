"""CPU (no GPU needed): zultra_hip_inflate_streams — the batched inflate kernel of zultra_amd/csrc/zh_inflate_out.h — and zultra_memory_decompress
in the lock-step emulator build of the product's sources, against Python's zlib: foreign streams, hand-written token streams, the library's own
streams device to device, bounds, corrupted streams, the host API, dynamic-Huffman headers written by hand (cut at every byte, every bit flipped), seeded token streams, buffers
that start inside a dword, stored-block edges. tests/test_inflate_gpu.py runs the same cases (tests/inflate_cases.py), larger,
on the MI355X."""
import ctypes
import os
import sys

import pytest

import inflate_cases as I

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    L = Lib(build_emu.build())
    L.is_emulator = True    # (verify_cases.DeviceCopy: device memory is host memory)
    return L


@pytest.mark.parametrize("name", sorted(I.FOREIGN))
def test_foreign_streams(emu, name):
    I.check_foreign(emu, I.FOREIGN[name])


def test_sync_flushes_give_empty_stored_blocks(emu):
    I.check_sync_flushes(emu)


def test_stored_pieces_of_a_long_level_0_stream(emu):
    I.check_stored_pieces(emu)


def test_hand_written_matches(emu):
    I.check_hand_good(emu)


def test_hand_written_bad_streams(emu):
    I.check_hand_bad(emu)


def test_own_files_batch_device_to_device(emu):
    I.check_own_files(emu, 200)


def test_own_files_batch_with_a_capped_grid(emu):
    I.check_own_files_strided(emu.path, True, 200)


def test_own_blocks_stream(emu):
    I.check_own_blocks(emu, 40000, 32768)


def test_bounds(emu):
    I.check_bounds(emu)


def test_bad_arguments(emu):
    I.check_bad_arguments(emu)


def test_single_bit_flips_get_zlibs_verdict(emu):
    n, benign = I.check_flips(emu, 40, seed=20261017)
    assert n == 40


def test_truncated_streams_end_with_reason_12(emu):
    assert I.check_truncations(emu, seed=20261017) >= 21 * 5


def test_host_api(emu):
    I.check_host_api(emu, 9000)


def test_hand_written_dynamic_headers(emu):
    assert I.check_dynamic_good(emu) >= 13


def test_hand_written_bad_dynamic_headers(emu):
    assert I.check_dynamic_bad(emu) >= 20


def test_dynamic_headers_cut_at_every_byte(emu):
    assert I.check_dynamic_cuts(emu) >= 1000


def test_dynamic_headers_with_every_bit_flipped(emu):
    n, benign = I.check_dynamic_flips(emu)
    assert n >= 900 and benign > 0


def test_token_stream_fuzz(emu):
    I.check_token_fuzz(emu, 20261018, 64, 300)


def test_unaligned_source_and_destination_pointers(emu):
    I.check_unaligned(emu)


def test_stored_block_edges(emu):
    I.check_stored_edges(emu)


def test_no_device_means_loud_failure():
    """On a machine without a GPU the product library refuses to decompress, and does not crash."""
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    from zultra_amd import build
    from zultra_amd._ffi import Lib
    so = build.build(verbose=False)
    L = ctypes.CDLL(so)
    L.zultra_hip_device_count.restype = ctypes.c_int
    if L.zultra_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    lib = Lib(so)
    s = I.zlib_raw(b"hello hello hello hello", 6, I.zlib.Z_DEFAULT_STRATEGY)
    assert lib.memory_decompress(s, 0, 100) is None
    import numpy as np
    src, dst = np.frombuffer(s, dtype=np.uint8).copy(), np.zeros(100, dtype=np.uint8)
    assert lib.inflate_streams(src, len(src), dst, 100, [(0, len(src), 0, 100)])[0] == -1
    assert not dst.any()
