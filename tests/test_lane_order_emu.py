"""CPU (no GPU needed): the bundles of zh_parse_lanes and their longest-first order (zh_parse.h) under the lock-step emulator, which runs the product's
own sources serially — no wave may wait for another one, or these tests would not end. The cases, at the emulator's sizes: tests/lane_order_cases.py;
tests/test_lane_order_gpu.py repeats them on the MI355X build."""
import os
import sys

import pytest

import lane_order_cases as cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from zultra_amd._ffi import Lib
    return Lib(build_emu.build())


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_bundles_of_one_and_a_last_bundle_of_one(emu, checker, monkeypatch, combo):
    cases.bundle_sizes(emu, checker, monkeypatch, combo, small=True)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_bundles_of_several_length_classes(emu, checker, monkeypatch, combo):
    cases.mixed_classes(emu, checker, monkeypatch, combo, small=True)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_every_bundle_in_one_class(emu, checker, monkeypatch, combo):
    cases.single_class(emu, checker, monkeypatch, combo, small=True)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_settled_subblocks_keep_their_parse_in_ordered_bundles(emu, checker, monkeypatch, combo):
    cases.settled_subblocks(emu, checker, monkeypatch, combo, small=True)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_overflow_form_of_the_listing_kernel_fills_the_lists(emu, checker, monkeypatch, combo):
    cases.overflow_form(emu, checker, monkeypatch, combo, small=True)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_staggered_runs_list_their_own_bundles(emu, checker, monkeypatch, combo):
    cases.staggered_runs(emu, checker, monkeypatch, combo, small=True)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_files_mode_keeps_its_hand_out(emu, checker, monkeypatch, combo):
    cases.files_mode(emu, checker, monkeypatch, combo, small=True)


@pytest.mark.parametrize("wide", ["1", "1000000"], ids=["segment_workgroups", "jobs_of_zh_parse_chain"])
@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_bundles_whose_tasks_are_listed_elsewhere(emu, checker, monkeypatch, combo, wide):
    cases.listed_tasks(emu, checker, monkeypatch, combo, small=True, wide=wide)


@pytest.mark.parametrize("combo", cases.COMBOS, ids=cases.COMBO_IDS)
def test_hand_out_of_before_bundles_is_still_there(emu, checker, monkeypatch, combo):
    cases.bundles_off(emu, checker, monkeypatch, combo, small=True)
