"""CPU (no GPU needed): what the context remembers of the stream buffer between the calls that assemble the last batch — stitch_device, stitch_files,
frame_members, stitch_phase_table, zip_members, the assemblies a batch brings with it — in the lock-step emulator build of the product's sources
(tests/assembly_state_cases.py). tests/test_assembly_state_gpu.py runs the same cases on the MI355X."""
import os
import sys

import pytest

import assembly_state_cases as A

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    L = Lib(build_emu.build())
    L.is_emulator = True
    return L


@pytest.mark.parametrize("kind", A.KINDS)
def test_each_operation_alone_against_its_reference(emu, checker, kind):
    assert A.check_solo(emu, checker, kind) == (4 if kind == "files" else 7)


@pytest.mark.parametrize("kind,first", [(k, op) for k in A.KINDS for op in A.ops_of(k)])
def test_every_ordered_pair(emu, checker, kind, first):
    assert A.check_pairs(emu, checker, kind, first) == (4 if kind == "files" else 7)


@pytest.mark.parametrize("armed", [0, 3])
def test_stitch_armed_with_the_batch(emu, checker, armed):
    A.check_armed_stitch(emu, checker, armed)


def test_files_batch_brings_its_offsets(emu, checker):
    A.check_files_batch_brings_its_offsets(emu, checker)


def test_explicit_assembly_is_redone_over_an_overwritten_buffer(emu, checker):
    A.check_explicit_assembly_is_redone(emu, checker)


@pytest.mark.parametrize("kind", A.KINDS)
def test_zip_reuses_the_assembled_buffer(emu, checker, kind):
    A.check_zip_reuses_the_assembled_buffer(emu, checker, kind)
