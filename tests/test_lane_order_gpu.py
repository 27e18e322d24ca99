"""GPU (MI355X): the bundles of zh_parse_lanes and their longest-first order (zh_parse.h) on the product library, with ZULTRA_HIP_LANE_ORDER 0 and 1 and
ZULTRA_HIP_LANE_TASKS 1, 2, 3 and 8, against the `checker` of tests/conftest.py. The cases: tests/lane_order_cases.py."""
import pytest

import lane_order_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import zultra_amd
    L = zultra_amd.lib()            # raises if the .so is missing: no fallback
    assert L.device_count() >= 1, "no HIP device visible"
    return L


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_bundles_of_one_and_a_last_bundle_of_one(gpu, checker, monkeypatch, combo):
    cases.bundle_sizes(gpu, checker, monkeypatch, combo, small=False)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_bundles_of_several_length_classes(gpu, checker, monkeypatch, combo):
    cases.mixed_classes(gpu, checker, monkeypatch, combo, small=False)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_every_bundle_in_one_class(gpu, checker, monkeypatch, combo):
    cases.single_class(gpu, checker, monkeypatch, combo, small=False)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_settled_subblocks_keep_their_parse_in_ordered_bundles(gpu, checker, monkeypatch, combo):
    cases.settled_subblocks(gpu, checker, monkeypatch, combo, small=False)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_overflow_form_of_the_listing_kernel_fills_the_lists(gpu, checker, monkeypatch, combo):
    cases.overflow_form(gpu, checker, monkeypatch, combo, small=False)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_staggered_runs_list_their_own_bundles(gpu, checker, monkeypatch, combo):
    cases.staggered_runs(gpu, checker, monkeypatch, combo, small=False)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_files_mode_keeps_its_hand_out(gpu, checker, monkeypatch, combo):
    cases.files_mode(gpu, checker, monkeypatch, combo, small=False)


@pytest.mark.parametrize("wide", ["1", "1000000"], ids=["segment_workgroups", "jobs_of_zh_parse_chain"])
@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_bundles_whose_tasks_are_listed_elsewhere(gpu, checker, monkeypatch, combo, wide):
    cases.listed_tasks(gpu, checker, monkeypatch, combo, small=False, wide=wide)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_hand_out_of_before_bundles_is_still_there(gpu, checker, monkeypatch, combo):
    cases.bundles_off(gpu, checker, monkeypatch, combo, small=False)
