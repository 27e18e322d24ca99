"""GPU (MI355X): the code-building kernels zh_sb_init and zh_sb_build of the product library on chosen histograms, against the `checker` of tests/conftest.py
(the compiled reference where oracle/_ref travelled, its pinned restatement otherwise). The kernels run unchanged on made-up sub-blocks
(zultra_hip_entropy_probe); every family of tests/entropy_cases.py goes through in a handful of launches, once with every sub-block in the one-per-workgroup form
of the kernel and once with all but a few in the striding form. Every comparison is exact equality of the whole coder state and of the block header.
What the cases reach (length limiting at 15 and at 7 bits, the repair's last loop, the RLE-friendly alternative, the masks, HCLEN) is asserted from the
reference side in tests/test_oracle_vs_ref.py; tests/test_entropy_emu.py has the note on what the suite's older inputs reached."""
import pytest

import entropy_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    return L


@pytest.mark.parametrize("grid", [None, 7], ids=["one_per_workgroup", "striding_from_7"])
@pytest.mark.parametrize("ntasks", [1, 3])
def test_build_matches_the_reference(gpu, checker, ntasks, grid):
    cases.check_build(gpu, checker, cases.GPU, ntasks, grid)


@pytest.mark.parametrize("grid", [None, 7], ids=["one_per_workgroup", "striding_from_7"])
def test_init_matches_the_reference(gpu, checker, grid):
    cases.check_init(gpu, checker, cases.GPU, grid)
