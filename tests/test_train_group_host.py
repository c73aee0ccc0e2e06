"""Training groups (K7g, specification TG-1) without a device: the library exports the entry points include/wsa.h declares, and the launch
count of a group epoch is TG-1's formula, restated here in Python and evaluated over member shapes taken from tests/train_cases.py."""
import ctypes
import os
import re

import pytest

from tests import train_cases as tc
from webspeechanalyzer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("wsa_train_group_create", "wsa_train_group_destroy", "wsa_train_group_epoch", "wsa_train_group_stats", "wsa_train_group_launches")


def shape(key):
    """(nl, n_train, batch, n_val) of a case"""
    c = tc.CASES[key]
    return len(c["units"]) - 1, c["n"] - c["n_val"], c["batch"], c["n_val"]


def formula(shapes):
    """TG-1: each step costs 3 . max nl over the members still stepping; then max nl + 1 over the members with validation rows, if any;
    then the finish"""
    steps = [-(-n_train // min(batch, n_train)) for _, n_train, batch, _ in shapes]
    total = 0
    for s in range(max(steps)):
        total += 3 * max(nl for (nl, _, _, _), k in zip(shapes, steps) if k > s)
    val = [nl for nl, _, _, n_val in shapes if n_val]
    return total + (max(val) + 1 if val else 0) + 1


def count(shapes):
    return capi.train_group_launch_count(*zip(*shapes))


def test_the_library_exports_what_the_header_declares():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "wsa.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS + ("wsa_train_group_launch_count",):
        assert hasattr(L, name), name
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in capi.ABI_SYMBOLS
    assert re.search(r"#define\s+WSA_TRAIN_GROUP_MAX\s+32\b", code) and capi.TRAIN_GROUP_MAX == 32
    assert "typedef struct wsa_train_group wsa_train_group;" in code


def test_one_member_costs_what_the_solo_epoch_enqueues():
    """3 nl per step, nl + 1 for the validation pass, 1 for the finish: wsa_trainer_epoch's own launches"""
    for key in tc.CASES:
        nl, n_train, batch, n_val = shape(key)
        steps = -(-n_train // batch)
        assert count([shape(key)]) == formula([shape(key)]) == 3 * nl * steps + (nl + 1 if n_val else 0) + 1, key


GROUPS = {
    "all_cases": list(tc.CASES),
    "reversed": list(tc.CASES)[::-1],
    "with_a_one_layer_member": ["one_layer", "eight_layers", "r_one_layer"],
    "one_layer_members_only": ["one_layer", "r_one_layer"],
    "batch_1_outlasts_the_rest": ["last_of_1", "batch_1", "big_batch", "eight_layers"],     # 300 steps beside 3, 3 and 4
    "no_validation_rows_at_all": ["width_edges", "r_width_edges"],
    "thirty_two": ["last_of_1", "r_one_layer"] * 16,
}


@pytest.mark.parametrize("name", list(GROUPS))
def test_launch_count_is_the_formula(name):
    shapes = [shape(k) for k in GROUPS[name]]
    assert count(shapes) == formula(shapes)


def test_the_long_member_pays_for_its_own_stack_only():
    """after the 3- and 4-step members have dropped out, the 300-step two-layer member steps alone: 6 launches a step, not 24"""
    shapes = [shape(k) for k in GROUPS["batch_1_outlasts_the_rest"]]
    assert shape("batch_1")[:3] == (2, 300, 1) and shape("eight_layers")[0] == 8
    steps8 = -(-shape("eight_layers")[1] // shape("eight_layers")[2])
    assert count(shapes) == 3 * 8 * steps8 + 3 * 2 * (300 - steps8) + (8 + 1) + 1


def test_a_batch_above_the_training_rows_is_one_step():
    assert count([(2, 10, 64, 0)]) == 3 * 2 + 1
    assert count([(2, 10, 64, 3), (1, 10, 5, 0)]) == 3 * 2 + 3 * 1 + (2 + 1) + 1


@pytest.mark.parametrize("shapes", [[], [(1, 10, 2, 0)] * 33, [(0, 10, 2, 0)], [(9, 10, 2, 0)], [(1, 0, 2, 0)], [(1, 10, 0, 0)]])
def test_shapes_outside_the_limits_are_refused(shapes):
    with pytest.raises((capi.WsaError, ValueError)):
        capi.train_group_launch_count(*(zip(*shapes) if shapes else ([], [], [], [])))


def test_null_arguments_are_refused():
    L = capi.lib()
    one = (ctypes.c_uint32 * 1)(1)
    out = ctypes.c_uint64()
    assert L.wsa_train_group_launch_count(None, one, one, one, 1, ctypes.byref(out)) != 0
    assert L.wsa_train_group_launch_count(one, one, one, one, 1, None) != 0
