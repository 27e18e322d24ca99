"""CPU (no GPU needed): a byte range of a BGZF / multi-member gzip file — zh_rg_select, zh_rg_items and zh_rg_edges of
zultra_amd/csrc/zh_inflate_range.h under zultra_hip_inflate_range —, zultra_memory_index_gzi and zultra_memory_decompress_range in the lock-step emulator
build of the product's sources, against Python's gzip, the serial walk of tests/inflate_file_cases.py and zultra_hip_inflate_file.
tests/test_inflate_range_gpu.py runs the same cases on the MI355X, with the larger sizes."""
import os
import subprocess
import sys

import pytest

import inflate_file_cases as F
import inflate_range_cases as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

CHILD = "__import__('inflate_range_cases').check_tiles(L)"
SLOW = os.environ.get("ZULTRA_SLOW_TESTS") == "1"


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    L = Lib(build_emu.build())
    L.is_emulator = True    # (verify_cases.DeviceCopy: device memory is host memory)
    return L


def test_every_range_of_a_tiny_file(emu):
    assert R.check_tiny(emu) == 2 * (15 * 16 + 6)


def test_edges_at_real_sizes(emu):
    """Every boundary point to the next one and to the last (the GPU test: to every later one)."""
    assert R.check_sizes(emu, reach=1) >= 40


@pytest.mark.parametrize("tile", (32, 100, 256))
def test_small_tiles(emu, tile):
    F.run_child(emu.path, True, CHILD, dict(ZULTRA_HIP_INDEX_TILE=str(tile)))


def test_small_tiles_with_a_capped_grid(emu):
    F.run_child(emu.path, True, CHILD, dict(ZULTRA_HIP_INDEX_TILE="100", ZULTRA_HIP_GRID_CAP="8"))


def test_placement(emu):
    assert R.check_placement(emu) == 96


def test_only_the_covered_members(emu):
    R.check_only_covered(emu)


def test_stops(emu):
    R.check_stops(emu)


def test_room(emu):
    R.check_room(emu)


def test_bad_arguments(emu):
    R.check_bad_arguments(emu)


def test_gzi_index(emu):
    R.check_gzi(emu, big=False)


def sanitizer_case(case, ranges):
    """The case file of tests/emu/inflate_range_main.cpp."""
    u64 = lambda v: int(v).to_bytes(8, "little")
    return u64(len(case.buf)) + case.buf + u64(case.out) + case.want + u64(len(ranges)) + b"".join(u64(a) + u64(b) for a, b in ranges)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/emu/inflate_range_main.cpp — zultra_hip_inflate_range in an executable of its own, AddressSanitizer and UBSan built in — over the tiny file's
    sweep and the boundary ranges of the file of real sizes, under tiles of 32, 100, 256 bytes and the default, each with and without ZULTRA_HIP_GRID_CAP=8,
    source, destination and results in exact-size heap blocks used in place: exit status 0, nothing on stderr."""
    if not SLOW:
        pytest.skip("slow (a minute to build, minutes to run under the sanitizers): set ZULTRA_SLOW_TESTS=1")
    import build_emu
    main = os.path.join(os.path.dirname(build_emu.__file__), "inflate_range_main.cpp")
    prog = build_emu._build_program(main, os.path.join(os.path.dirname(build_emu.OUT), "inflate_range_main"), False)
    env = dict(os.environ)
    env["LSAN_OPTIONS"] = "suppressions=%s:print_suppressions=0" % build_emu.LSAN_SUPPRESSIONS
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    tiny, sizes = R.tiny_case(), R.sizes_case()
    jobs = (("tiny", tiny, [(a, b) for a in range(15) for b in range(16)] + [(5, R.U64), (R.U64, R.U64)]), ("sizes", sizes, R.boundary_ranges(sizes, reach=1)))
    running = []
    for name, case, ranges in jobs:   # (the two processes side by side)
        path = tmp_path / (name + ".case")
        path.write_bytes(sanitizer_case(case, ranges))
        running.append((name, len(ranges), subprocess.Popen([prog, str(path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)))
    try:
        for name, n, p in running:
            out, err = p.communicate(timeout=3000)
            # (AddressSanitizer's one line at start-up about the emulator's fibres — "doesn't fully support makecontext/swapcontext" — is no report)
            report = [ln for ln in err.decode(errors="replace").splitlines() if ln.strip() and "makecontext/swapcontext" not in ln]
            assert p.returncode == 0 and not report, (name, p.returncode, "\n".join(report[:40]))
            assert out.decode().strip() == "%d runs, 0 failed" % (8 * n), (name, out)
    finally:
        for _, _, p in running:
            if p.poll() is None:
                p.kill()
                p.wait()
