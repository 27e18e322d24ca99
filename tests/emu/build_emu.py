"""TEST INFRASTRUCTURE: build tests/emu/_build/libzultra_amd_emu.so — the product's own sources (zultra_amd/csrc)
compiled for the CPU against tests/emu/zh_platform.h, a lock-step emulator of the HIP subset they use.
Lets the `-m "not gpu"` suite run the kernel logic against the oracle on a machine without a GPU.
The product package never loads this file; its loader only accepts zultra_amd/libzultra_amd.so."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "zultra_amd", "csrc")
OUT = os.path.join(HERE, "_build", "libzultra_amd_emu.so")
NOTES_MAIN = os.path.join(HERE, "mf_notes_main.cpp")
NOTES_OUT = os.path.join(HERE, "_build", "mf_notes_main")
LIFECYCLE_MAIN = os.path.join(HERE, "ctx_lifecycle_main.cpp")
LIFECYCLE_OUT = os.path.join(HERE, "_build", "ctx_lifecycle_main")
LSAN_SUPPRESSIONS = os.path.join(HERE, "lsan_suppressions.txt")

# the emulator configuration: small chunks, cuts and matchfinder chunks, so that windows of a few KB take every path
DEFINES = ["-DZH_TOK_CHUNK=1024u", "-DZH_CUT_LEN=512u", "-DZH_CUT_WARM=288u", "-DZH_MFL_CAP_LIMIT=512u"]
WARNINGS = ["-Wall", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unknown-pragmas"]


def _sources():
    return ["-I", HERE, "-I", CSRC, "-x", "c++", "-DZH_EMU_INFLATE_TU", os.path.join(CSRC, "zh_device.hip"), os.path.join(CSRC, "zh_inflate.hip"),
            os.path.join(CSRC, "libzultra.cpp")]


def _fresh(out, more=()):
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "zh_platform.h")] + list(more)
    return os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps)


def build(force=False):
    if not force and _fresh(OUT):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    cmd = ["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared"] + WARNINGS + DEFINES + _sources() + ["-o"]
    cmd[1:1] = os.environ.get("ZH_EMU_DEFINES", "").split()   # extra -D switches (A/B of compile-time variants under the emulator)
    tmp = "%s.%d.tmp" % (OUT, os.getpid())   # several test processes may build at once: each writes its own file, the rename is atomic
    subprocess.run(cmd + [tmp], check=True)
    os.replace(tmp, OUT)
    return OUT


def _build_program(main, out, force):
    """main and the three emulator sources as ONE EXECUTABLE with AddressSanitizer and UBSan — run as a process of its own, never loaded into Python.
    LeakSanitizer is told to pass over the emulator's fibre stacks, which live as long as the process (lsan_suppressions.txt)."""
    if not force and _fresh(out, (main,)):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # (the sanitizers' runtimes linked into the executable: it runs whatever else the process loads)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"] + WARNINGS + DEFINES + _sources() + [main, "-lpthread", "-o"]
    tmp = "%s.%d.tmp" % (out, os.getpid())
    subprocess.run(cmd + [tmp], check=True)
    os.replace(tmp, out)
    return out


def build_notes_program(force=False):
    """tests/emu/_build/mf_notes_main: zultra_memory_compress on a file (tests/test_mf_classes_emu.py)."""
    return _build_program(NOTES_MAIN, NOTES_OUT, force)


def build_lifecycle_program(force=False):
    """tests/emu/_build/ctx_lifecycle_main: contexts created, used and destroyed (tests/test_context_layout_emu.py)."""
    return _build_program(LIFECYCLE_MAIN, LIFECYCLE_OUT, force)


if __name__ == "__main__":
    print(build(force=True))
