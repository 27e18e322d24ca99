"""GPU (MI355X): the bigram classes zh_mf_group notes for zh_mf_group_big (zultra_amd/csrc/zh_mf_group_lds.h) on the product library, against the `checker`
of tests/conftest.py: ZULTRA_HIP_MF_CAP — a product knob — with more classes above the chunk size than the 29 notes the table held before it was sized by
the chunk size, and the default configuration at its edge, 24 such classes in the largest window. The cases: tests/mf_class_cases.py."""
import pytest

import mf_class_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    return L


@pytest.mark.parametrize("name", cases.TABLE_IDS)
def test_every_class_above_the_chunk_size_is_noted(gpu, checker, monkeypatch, name):
    cases.table_case(gpu, checker, monkeypatch, name)


def test_noted_classes_at_the_end_of_a_window(gpu, checker, monkeypatch):
    cases.window_end_tail0(gpu, checker, monkeypatch)


def test_noted_classes_in_front_of_a_look_ahead_tail(gpu, checker, monkeypatch):
    cases.window_end_lookahead(gpu, checker, monkeypatch)


def test_largest_window_with_the_default_chunk_size(gpu, checker, monkeypatch):
    cases.full_window_default_cap(gpu, checker, monkeypatch)


@pytest.mark.parametrize("cap,period", [(None, 6), (512, 48)], ids=["default_cap", "cap512"])
def test_helping_workgroups_on_deep_classes(gpu, checker, monkeypatch, cap, period):
    cases.helpers(gpu, checker, monkeypatch, cap, period)
