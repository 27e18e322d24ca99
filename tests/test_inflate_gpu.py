"""GPU (MI355X): zultra_hip_inflate_streams — the batched inflate kernel of zultra_amd/csrc/zh_inflate_out.h — and zultra_memory_decompress in the
product library, against Python's zlib. The cases are those of tests/test_inflate_emu.py (tests/inflate_cases.py), with the larger sizes."""
import os
import subprocess
import zlib

import pytest

import corpus
import inflate_cases as I

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    L.is_emulator = False   # (verify_cases.DeviceCopy: device memory comes from hipMalloc)
    return L


@pytest.mark.parametrize("name", sorted(I.FOREIGN) + sorted(I.FOREIGN_GPU_ONLY))
def test_foreign_streams(gpu, name):
    I.check_foreign(gpu, dict(I.FOREIGN, **I.FOREIGN_GPU_ONLY)[name])


def test_sync_flushes_give_empty_stored_blocks(gpu):
    I.check_sync_flushes(gpu)


def test_stored_pieces_of_a_long_level_0_stream(gpu):
    I.check_stored_pieces(gpu)


def test_hand_written_matches(gpu):
    I.check_hand_good(gpu)


def test_hand_written_bad_streams(gpu):
    I.check_hand_bad(gpu)


def test_own_files_batch_device_to_device(gpu):
    I.check_own_files(gpu, 5000)


def test_own_files_batch_with_a_capped_grid(gpu):
    import zultra_amd
    I.check_own_files_strided(zultra_amd.LIB_PATH, False, 5000)


def test_own_blocks_stream(gpu):
    I.check_own_blocks(gpu, 200000, 65536)


def test_bounds(gpu):
    I.check_bounds(gpu)


def test_bad_arguments(gpu):
    I.check_bad_arguments(gpu)


def test_single_bit_flips_get_zlibs_verdict(gpu):
    n, benign = I.check_flips(gpu, 200, seed=20261017)
    assert n == 200


def test_truncated_streams_end_with_reason_12(gpu):
    assert I.check_truncations(gpu, seed=20261017) >= 21 * 5


def test_host_api(gpu):
    I.check_host_api(gpu, 100000)


def test_hand_written_dynamic_headers(gpu):
    assert I.check_dynamic_good(gpu) >= 13


def test_hand_written_bad_dynamic_headers(gpu):
    assert I.check_dynamic_bad(gpu) >= 20


def test_dynamic_headers_cut_at_every_byte(gpu):
    assert I.check_dynamic_cuts(gpu) >= 1000


def test_dynamic_headers_with_every_bit_flipped(gpu):
    n, benign = I.check_dynamic_flips(gpu)
    assert n >= 900 and benign > 0


def test_token_stream_fuzz(gpu, tmp_path):
    """512 items of about 600 tokens in flight: 128 generated streams, each four times (generating 512 takes Python ten seconds)."""
    import zultra_amd
    made = I.check_token_fuzz(gpu, 20261018, 128, 600, copies=4)
    I.check_token_fuzz_strided(zultra_amd.LIB_PATH, False, made, 4, tmp_path)


def test_unaligned_source_and_destination_pointers(gpu):
    I.check_unaligned(gpu)


def test_stored_block_edges(gpu):
    I.check_stored_edges(gpu)


def test_cli_extracts(gpu, tmp_path):
    import zultra_amd
    cli = os.path.join(os.path.dirname(zultra_amd.LIB_PATH), "zultra_amd_cli")
    d = corpus.text_like(100000, 9).tobytes()
    src, packed, back = tmp_path / "in.bin", tmp_path / "out.gz", tmp_path / "back.bin"
    src.write_bytes(d)
    r = subprocess.run([cli, "-b", "65536", str(src), str(packed)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([cli, "-x", str(packed), str(back)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert back.read_bytes() == d
    raw = tmp_path / "out.deflate"
    raw.write_bytes(zlib.compress(d, 6)[2:-4])
    r = subprocess.run([cli, "-x", "-f", "deflate", str(raw), str(back)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and back.read_bytes() == d, r.stdout + r.stderr
    r = subprocess.run([cli, "-x", "-f", "zlib", str(raw), str(back)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
