"""MI355X: streams of several max-blocks in one batch (zultra_hip_frame_streams, zultra_hip_zip_streams, zultra_memory_compress_streams,
zultra_memory_compress_zip_streams, the tool's -a with -b) in the product library, against the reference's members and streams, Python's gzip, zlib and
zipfile. The cases are those of tests/stream_group_cases.py at their full sizes; tests/test_stream_groups_emu.py runs the ones the emulator has time for."""
import pytest

import inflate_file_cases as F
import stream_group_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    L.is_emulator = False   # (verify_cases.DeviceCopy: device memory comes from hipMalloc)
    return L


@pytest.fixture(scope="module")
def batch(gpu):
    """The parity batch: eight streams, fifteen max-blocks, stored ones among them."""
    b = S.Batch(gpu, S.parity_parts())
    yield b
    b.close()


@pytest.fixture(scope="module")
def small(gpu):
    b = S.Batch(gpu, S.small_parts())
    yield b
    b.close()


def test_parity_per_framing(batch, checker):
    assert S.check_parity(batch, checker) == 8


def test_every_phase_is_carried(gpu, batch, checker):
    """All eight bit phases occur at the interior max-block boundaries of the parity batch and the phase batch, and both are held to the reference."""
    more = S.Batch(gpu, S.phase_parts())
    try:
        S.check_parity(more, checker)
        seen = S.carried_phases(batch) + S.carried_phases(more)
    finally:
        more.close()
    assert set(seen) == set(range(8)), sorted(seen)


def test_single_block_streams_are_frame_members(gpu, checker):
    S.check_single_blocks(gpu, checker)


def test_one_stream_over_the_batch_is_stitch_device(gpu, checker):
    S.check_one_stream(gpu, checker, 2 * S.MB + 100)


def test_device_scan_equals_host_planner(batch):
    S.check_scan_equals_planner(batch)


def test_more_blocks_than_scan_threads(gpu, checker):
    assert S.check_many(gpu, checker, *S.MANY_GPU, chunk=2) == 1103


def test_more_blocks_than_scan_threads_capped_grid(gpu):
    """The strided forms: eight lanes in zh_frame_members and zh_zip_records, eight waves in zh_fold_streams. In a process of its own (the cap is read when
    a context is created)."""
    F.run_child(gpu.path, False, "__import__('stream_group_cases').check_many(L, None, *__import__('stream_group_cases').MANY_GPU, chunk=2)", dict(ZULTRA_HIP_GRID_CAP="8"))


def test_fold_across_lanes(gpu):
    S.check_fold(gpu, 70)


def test_flipped_bits(batch, checker):
    S.check_flipped_bits(batch, checker)


def test_refused_groupings(small):
    S.check_refused_groupings(small)


def test_refused_descriptors_and_the_reference_s_failure(gpu, checker):
    S.check_refused_descriptors(gpu, checker)


def test_next_to_the_other_assemblies(batch, checker):
    S.check_next_to_the_others(batch, checker)


def test_zip_of_streams(gpu, checker):
    """5000 B, empty, 70000 B, 3 x 32768 + 1, a directory, noise of 40000."""
    b = S.Batch(gpu, S.zip_parts())
    try:
        S.check_zip(b, checker, empty_at=(1, 4))
    finally:
        b.close()


@pytest.mark.parametrize("max_block", [32768, 0])
def test_host_api(gpu, checker, max_block):
    assert S.check_api(gpu, checker, max_block, S.api_parts(True)) == 5


def test_host_api_small_batches(gpu):
    F.run_child(gpu.path, False, "__import__('stream_group_cases').check_api_small_batches(L, None)", dict(ZULTRA_HIP_BATCH_BLOCKS="4"))


def test_cli_archive_of_large_files(gpu, checker, tmp_path):
    import zultra_amd.build
    S.check_cli(zultra_amd.build.CLI, gpu, tmp_path, checker)
