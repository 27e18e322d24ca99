"""CPU (no GPU needed): the one list of a context's buffers (zultra_amd/csrc/zh_device.hip, ZH_CTX_BUFFERS) in the lock-step emulator build — the size
estimate that the host layer budgets its batches with is the sum the creation allocates, for every shape and every switch that sizes a buffer; a files
context stays below the block estimate; the sets of first use are added once. tests/emu/ctx_lifecycle_main.cpp walks the same list's releases under
LeakSanitizer."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

SWITCHES = ("ZULTRA_HIP_STREAMS", "ZULTRA_HIP_MF_CAP", "ZULTRA_HIP_CHAIN_TRACE")
# 65536 is the largest block of one matchfinder segment (98304 - 32768), 65537 the first of two; 100000 is no multiple of 64
BLOCK_SHAPES = [(32768, 1), (65536, 3), (100000, 5), (65537, 2), (200000, 3), (1048576, 2)]
ENVIRONMENTS = [{}, {"ZULTRA_HIP_STREAMS": "1"}, {"ZULTRA_HIP_STREAMS": "8"}, {"ZULTRA_HIP_MF_CAP": "16"}, {"ZULTRA_HIP_CHAIN_TRACE": "1"}]


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    lib = Lib(build_emu.build())
    lib.L.zultra_hip_context_bytes_on.argtypes = [C.c_int, C.c_uint32, C.c_uint32]
    lib.L.zultra_hip_context_bytes_on.restype = C.c_size_t
    lib.L.zultra_hip_ctx_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]
    return lib


def device_bytes(lib, ctx):
    n = C.c_size_t()
    lib.L.zultra_hip_ctx_info(ctx.h, None, None, None, C.byref(n))
    return n.value


def set_switches(monkeypatch, env):
    for name in SWITCHES:   # (read when a context is created, and when the estimate is asked for)
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


@pytest.mark.parametrize("env", ENVIRONMENTS, ids=lambda e: "-".join("%s=%s" % (k[11:].lower(), v) for k, v in e.items()) or "default")
@pytest.mark.parametrize("max_block,max_blocks", BLOCK_SHAPES)
def test_estimate_is_what_a_block_context_allocates(emu, monkeypatch, max_block, max_blocks, env):
    set_switches(monkeypatch, env)
    est = emu.L.zultra_hip_context_bytes_on(0, max_block, max_blocks)
    ctx = emu.context(max_block, max_blocks)
    try:
        real = device_bytes(emu, ctx)
    finally:
        ctx.close()
    print("estimate %d, allocated %d, ratio %.6f" % (est, real, est / real))
    assert est == real


@pytest.mark.parametrize("max_file,max_files", [(100, 1), (4096, 7), (8191, 3)])
def test_files_context_stays_below_the_block_estimate(emu, monkeypatch, max_file, max_files):
    set_switches(monkeypatch, {})
    ctx = emu.files_context(max_file, max_files)
    try:
        real = device_bytes(emu, ctx)
    finally:
        ctx.close()
    est = emu.L.zultra_hip_context_bytes_on(0, (max_file + 63) & ~63, max_files)
    print("allocated %d, block estimate %d" % (real, est))
    assert 0 < real <= est


def test_sets_of_first_use_are_added_once(emu, monkeypatch):
    """verify, the files form's offsets, framed members and the zip report: each appears in device_bytes with the first call that needs it and never again."""
    set_switches(monkeypatch, {})
    data = np.frombuffer((b"one list of a context's buffers, stated once. " * 8)[:300], dtype=np.uint8)
    ctx = emu.context(32768, 1)
    try:
        ctx.compress_blocks(data, [(0, 0, len(data))])
        ctx.stitch_device(0)
        calls = [("verify_device", lambda: ctx.verify()["rc"]), ("stitch_files", lambda: 0 if len(ctx.stitch_files()) == 2 else -1),   # (raises where the call fails)
                 ("frame_members", lambda: ctx.frame_members(2)[0]), ("zip_members", lambda: ctx.zip_members(["a.txt"])[0])]
        seen = [device_bytes(emu, ctx)]
        for name, call in calls:
            assert call() == 0, name
            seen.append(device_bytes(emu, ctx))
            assert seen[-1] > seen[-2], (name, seen)
        for name, call in calls:
            if name == "verify_device":
                ctx.stitch_device(0)   # (the stream form again: what the first verify looked at)
            assert call() == 0, name
            assert device_bytes(emu, ctx) == seen[-1], (name, seen)
    finally:
        ctx.close()


def test_lifecycle_program_under_the_sanitizers():
    """tests/emu/ctx_lifecycle_main.cpp — contexts of both kinds created, used through every call that allocates on first use or grows a buffer, and
    destroyed, twice over, in an executable of its own with AddressSanitizer, UBSan and LeakSanitizer built in: exit status 0 and nothing on stderr. In the
    emulator every device allocation is a malloc, so a buffer that zultra_hip_destroy's walk of the list misses is reported where it was allocated."""
    if os.environ.get("ZULTRA_SLOW_TESTS", "0") != "1":
        pytest.skip("slow (a minute to build under the sanitizers): set ZULTRA_SLOW_TESTS=1")
    import build_emu
    prog = build_emu.build_lifecycle_program()
    env = dict(os.environ)
    for name in SWITCHES:
        env.pop(name, None)
    env["LSAN_OPTIONS"] = "suppressions=%s:print_suppressions=0" % build_emu.LSAN_SUPPRESSIONS
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    p = subprocess.run([prog], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    # (AddressSanitizer's one line at start-up about the emulator's fibres — "doesn't fully support makecontext/swapcontext" — is no report)
    report = [ln for ln in p.stderr.decode(errors="replace").splitlines() if ln.strip() and "makecontext/swapcontext" not in ln]
    assert p.returncode == 0 and not report, (p.returncode, "\n".join(report[:40]))
