"""CPU (no GPU needed): the code-building kernels zh_sb_init and zh_sb_build on chosen histograms, under the lock-step emulator, against the `checker`
(the compiled reference where it is built, its pinned restatement otherwise). The kernels run unchanged on made-up sub-blocks (zultra_hip_entropy_probe); every
comparison is exact equality of the whole coder state and of the block header. Cases and what they reach: tests/entropy_cases.py; the coverage is asserted in
tests/test_oracle_vs_ref.py; tests/test_entropy_gpu.py runs more of the random cases on the MI355X build. Times: profiles/entropy_probe.txt.

Do the suite's older "deep tree" inputs reach the limiter? Run once through the restatement with a counter in its code build (every sub-block, every build: the
greedy one, the four passes, the alternative, the twenty-one code-length tables), longest UNLIMITED code per alphabet:
  * the `deep_huffman` window of tests/test_emu_parity.py, corpus.fibonacci_bytes(19), 10 945 bytes: literal/length 12 bits, distance 10, code-length 7.
    No build is limited.
  * the `deep_huffman` window of tests/test_gpu_parity.py (and `fibonacci` of tests/verify_cases.py), corpus.fibonacci_bytes(22), 46 367 bytes, two sub-blocks:
    literal/length 13, distance 13, code-length 6. No build is limited.
  * the 2 MiB block of Python sources of tests/test_gpu_parity.py (GPU only, five sub-blocks; it is whatever sources the image holds): literal/length 17 bits —
    6 of its 30 builds go through the 15-bit repair —, distance 13 (never limited), code-length 8 (6 of 105 builds limited at 7).
So on the CPU nothing reached zh_limit_lengths before this file, and on the GPU only the literal/length and code-length alphabets of one input did."""
import os
import sys

import pytest

import entropy_cases as cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    return Lib(build_emu.build())


@pytest.mark.parametrize("grid", [None, 5], ids=["one_per_workgroup", "striding_from_5"])
@pytest.mark.parametrize("ntasks", [1, 3])
def test_build_matches_the_reference(emu, checker, ntasks, grid):
    cases.check_build(emu, checker, cases.EMU, ntasks, grid)


@pytest.mark.parametrize("grid", [None, 5], ids=["one_per_workgroup", "striding_from_5"])
def test_init_matches_the_reference(emu, checker, grid):
    cases.check_init(emu, checker, cases.EMU, grid)
