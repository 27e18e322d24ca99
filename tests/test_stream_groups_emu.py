"""CPU (no GPU needed): streams of several max-blocks in one batch — zh_stitch_scan_streams and zh_fold_streams of zultra_amd/csrc/zh_streams.h,
zultra_hip_frame_streams, zultra_hip_zip_streams, zultra_memory_compress_streams and zultra_memory_compress_zip_streams — in the lock-step emulator build
of the product's sources, against the reference's members and streams (tests/stream_group_cases.py).

The emulator compresses about a kilobyte per second and the smallest max-block is 32768 bytes, so a stream of two max-blocks costs half a minute. The
checks here therefore share ONE batch — streams of 1, 2 and 1 max-blocks — that is compressed once per module. GPU only (tests/test_stream_groups_gpu.py),
because they need several full max-blocks each: the parity batch of eight streams with its stored max-blocks (1), all eight carried phases (2), the whole
batch as one stream of three max-blocks (3), 1100 max-blocks and the capped grids (5), the fold across lanes over 70 max-blocks (6), max-blocks that do not
continue their predecessor and the stream the reference fails on (8), the archive of six entries (10), the host API with 1 MiB max-blocks, with
ZULTRA_HIP_BATCH_BLOCKS=4 and with the input of 2097153 bytes (11), the tool (12)."""
import os
import subprocess
import sys

import pytest

import stream_group_cases as S

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
SLOW = os.environ.get("ZULTRA_SLOW_TESTS") == "1"


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    L = Lib(build_emu.build())
    L.is_emulator = True    # (verify_cases.DeviceCopy: device memory is host memory)
    return L


@pytest.fixture(scope="module")
def batch(emu):
    b = S.Batch(emu, S.small_parts())
    yield b
    b.close()


def test_parity_per_framing(batch, checker):
    assert S.check_parity(batch, checker) == 3


def test_a_phase_is_carried(batch):
    """(that all eight occur is the GPU suite's to assert: here the one boundary of the batch, against the host stitcher)"""
    phases = S.carried_phases(batch)
    assert len(phases) == 1 and 0 <= phases[0] <= 7


def test_single_block_streams_are_frame_members(emu, checker):
    S.check_single_blocks(emu, checker)


def test_device_scan_equals_host_planner(batch):
    S.check_scan_equals_planner(batch, stored=False)


def test_flipped_bits(batch, checker):
    S.check_flipped_bits(batch, checker)


def test_refused_groupings(batch):
    S.check_refused_groupings(batch)


def test_next_to_the_other_assemblies(batch, checker):
    S.check_next_to_the_others(batch, checker)


def test_zip_of_streams(batch, checker):
    S.check_zip(batch, checker, empty_at=(1, 4))


def test_host_api(emu, checker):
    """(one framing and the archive: every call compresses its 33 KB again)"""
    assert S.check_api(emu, checker, S.MB, [S.F.text(100, 1000), S.F.text(S.MB + 5, 1001)], framings=(S.GZIP,), short_caps=False) == 2


def test_stand_alone_program_under_the_sanitizers(tmp_path, checker):
    """tests/emu/stream_groups_main.cpp — the grouped assembly in an executable of its own, AddressSanitizer and UBSan built in — over the shared batch's
    inputs: parity per framing against the reference's members, and the refused groupings with both buffers marked: exit status 0, nothing on stderr."""
    if not SLOW:
        pytest.skip("slow (a minute to build, minutes to run under the sanitizers): set ZULTRA_SLOW_TESTS=1")
    import build_emu
    main = os.path.join(os.path.dirname(build_emu.__file__), "stream_groups_main.cpp")
    prog = build_emu._build_program(main, os.path.join(os.path.dirname(build_emu.OUT), "stream_groups_main"), False)
    env = dict(os.environ)
    env["LSAN_OPTIONS"] = "suppressions=%s:print_suppressions=0" % build_emu.LSAN_SUPPRESSIONS
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    path = tmp_path / "streams.case"
    path.write_bytes(S.sanitizer_case(checker, S.small_parts()))
    p = subprocess.run([prog, str(path)], env=env, capture_output=True, timeout=3000)
    # (AddressSanitizer's one line at start-up about the emulator's fibres — "doesn't fully support makecontext/swapcontext" — is no report)
    report = [ln for ln in p.stderr.decode(errors="replace").splitlines() if ln.strip() and "makecontext/swapcontext" not in ln]
    assert p.returncode == 0 and not report, (p.returncode, "\n".join(report[:40]))
    assert p.stdout.decode().strip() == "3 framings, 6 refusals, 0 failed", p.stdout
