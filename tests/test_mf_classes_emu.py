"""CPU (no GPU needed): the bigram classes zh_mf_group notes for zh_mf_group_big (zultra_amd/csrc/zh_mf_group_lds.h) under the lock-step emulator — more of
them than the 29 notes the table held whatever the chunk size — and the same inputs through a stand-alone program built with AddressSanitizer and UBSan.
The cases: tests/mf_class_cases.py; tests/test_mf_classes_gpu.py repeats them on the MI355X build."""
import os
import subprocess
import sys

import pytest

import mf_class_cases as cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

SLOW = os.environ.get("ZULTRA_SLOW_TESTS", "0") == "1"


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    return Lib(build_emu.build())


@pytest.mark.parametrize("name", cases.TABLE_IDS)
def test_every_class_above_the_chunk_size_is_noted(emu, oracle, monkeypatch, name):
    cases.table_case(emu, oracle, monkeypatch, name)


def test_noted_classes_at_the_end_of_a_window(emu, oracle, monkeypatch):
    cases.window_end_tail0(emu, oracle, monkeypatch)


def test_noted_classes_in_front_of_a_look_ahead_tail(emu, oracle, monkeypatch):
    if not SLOW:
        pytest.skip("slow (two segments with windows of 64 KiB: nine minutes under the emulator; the GPU suite runs it): set ZULTRA_SLOW_TESTS=1")
    cases.window_end_lookahead(emu, oracle, monkeypatch)


def test_compiled_chunk_size_with_more_classes_than_the_old_table(emu, oracle, monkeypatch):
    cases.default_cap_sibling(emu, oracle, monkeypatch)


def test_recorded_phrase_input_as_a_stream(emu, oracle, monkeypatch):
    if not SLOW:
        pytest.skip("slow (six minutes under the emulator): set ZULTRA_SLOW_TESTS=1")
    cases.recorded_shape(emu, oracle, monkeypatch)


def test_helping_workgroups_on_deep_classes(emu, oracle, monkeypatch):
    if not SLOW:
        pytest.skip("slow (four max-blocks of 32 KiB: thirteen minutes under the emulator; the GPU suite runs it): set ZULTRA_SLOW_TESTS=1")
    cases.helpers(emu, oracle, monkeypatch, None, 48)


def test_stand_alone_program_under_the_sanitizers(oracle, tmp_path):
    """notes_30 and notes_64 through tests/emu/mf_notes_main.cpp — zultra_memory_compress in an executable of its own, AddressSanitizer and UBSan built
    in: exit status 0, nothing on stderr, the oracle's stream on stdout. (Before the note table was sized by the chunk size both inputs ended in
    zh_mf_frontier reading far outside the window: the 30th class and those after it had no note and left their part of the order unwritten.)"""
    if not SLOW:
        pytest.skip("slow (a minute to build, three for the two inputs side by side under the sanitizers): set ZULTRA_SLOW_TESTS=1")
    import build_emu
    prog = build_emu.build_notes_program()
    env = dict(os.environ)
    env.pop("ZULTRA_HIP_MF_CAP", None)
    env["ZULTRA_HIP_CACHE"] = "0"
    env["LSAN_OPTIONS"] = "suppressions=%s:print_suppressions=0" % build_emu.LSAN_SUPPRESSIONS
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    running = []
    for name in ("notes_30", "notes_64"):   # (the two processes side by side)
        gen, prev, n, cap, expect, at_least = cases.TABLE[name]
        d = gen()
        assert prev == 0 and n == len(d)
        cases.expect_noted(d, prev, n, cap, expect, at_least)
        path = tmp_path / (name + ".bin")
        path.write_bytes(d.tobytes())
        running.append((name, d, subprocess.Popen([prog, str(path), "32768", "2", str(cap)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)))
    try:
        for name, d, p in running:
            out, err = p.communicate(timeout=900)
            # (AddressSanitizer's one line at start-up about the emulator's fibres — "doesn't fully support makecontext/swapcontext" — is no report)
            report = [ln for ln in err.decode(errors="replace").splitlines() if ln.strip() and "makecontext/swapcontext" not in ln]
            assert p.returncode == 0 and not report, (name, p.returncode, "\n".join(report[:40]))
            assert out == oracle.memory_compress(d, 2, 32768), name
    finally:
        for _, _, p in running:
            if p.poll() is None:
                p.kill()
                p.wait()
