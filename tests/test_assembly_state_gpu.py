"""MI355X: what the context remembers of the stream buffer between the calls that assemble the last batch, in the product library. The cases are
those of tests/test_assembly_state_emu.py (tests/assembly_state_cases.py)."""
import pytest

import assembly_state_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    L.is_emulator = False
    return L


@pytest.mark.parametrize("kind", A.KINDS)
def test_each_operation_alone_against_its_reference(gpu, checker, kind):
    assert A.check_solo(gpu, checker, kind) == (4 if kind == "files" else 7)


@pytest.mark.parametrize("kind,first", [(k, op) for k in A.KINDS for op in A.ops_of(k)])
def test_every_ordered_pair(gpu, checker, kind, first):
    assert A.check_pairs(gpu, checker, kind, first) == (4 if kind == "files" else 7)


@pytest.mark.parametrize("armed", [0, 3])
def test_stitch_armed_with_the_batch(gpu, checker, armed):
    A.check_armed_stitch(gpu, checker, armed)


def test_files_batch_brings_its_offsets(gpu, checker):
    A.check_files_batch_brings_its_offsets(gpu, checker)


def test_explicit_assembly_is_redone_over_an_overwritten_buffer(gpu, checker):
    A.check_explicit_assembly_is_redone(gpu, checker)


@pytest.mark.parametrize("kind", A.KINDS)
def test_zip_reuses_the_assembled_buffer(gpu, checker, kind):
    A.check_zip_reuses_the_assembled_buffer(gpu, checker, kind)
