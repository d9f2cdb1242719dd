"""The tick launchers without a GPU: for every case of tests/launch_plan_cases.py, launch_search, launch_belief_update and launch_reset of this
tree launch the kernels that tests/golden/launch_plan_expected.jsonl records -- the same instantiations in the same order, with the same
grid, block and dynamic LDS, and the same LDS limits raised in front of the same launches.  The record was taken from the launchers of
b672baa by scripts/record_launch_plan.py; nothing here is compared with a tolerance.

tests/launch_capture.cpp is built once (the launchers' translation units come with their kernels, so that takes a couple of minutes;
the cases themselves take microseconds) and runs all cases.

Not captured: the listed-slots path of for_each_chunk (budgeted searches) reads the number of listed slots back from the device, so it
cannot run here.  Its per-chunk launches are the same steps as the unlisted path's; the budgeted-search GPU tests cover it
(tests/test_gpu_history_table.py, tests/test_gpu_history_rejection.py, tests/test_gpu_parity.py)."""
import os
import re

import pytest

import launch_plan_cases as T
from fba_pomdp_amd import _native as N

CSRC = os.path.join(N.HERE, "csrc")
EXPECTED = T.expected()


@pytest.fixture(scope="module")
def captured(tmp_path_factory):
    exe = tmp_path_factory.mktemp("launch_capture") / "launch_capture"
    T.build_capture(exe)
    return T.capture(exe)


def normal(calls):
    """a kernel's name without spaces and without an outermost pair of parentheses: how a launch line is formatted is not compared"""
    out = []
    for call in calls:
        if call[0] == "L":
            name = call[1].replace(" ", "")
            if name.startswith("(") and name.endswith(")"):
                name = name[1:-1]
            call = [call[0], name] + call[2:]
        out.append(call)
    return out


def test_the_table_and_the_record_name_the_same_cases():
    assert [c["name"] for c in T.CASES] == list(EXPECTED)
    assert 100 <= len(T.CASES) <= 400
    for c in T.CASES:
        assert set(EXPECTED[c["name"]]) == set(c["launchers"]), c["name"]
        assert c["fields"].get("P_S", 1) >= 1 and c["fields"].get("P_E", 1) >= 1


@pytest.mark.parametrize("name", [c["name"] for c in T.CASES])
def test_the_launchers_launch_what_was_recorded(captured, name):
    seen, want = captured[name], EXPECTED[name]
    for launcher in want:
        assert normal(seen[launcher]) == normal(want[launcher]), (name, launcher)
    assert set(seen) == set(want)


def test_every_condition_has_a_case_on_each_side():
    """the kernels the record names: every instantiation family the launchers choose between is reached, and the thresholds on both sides"""
    kernels = {call[1] for rec in EXPECTED.values() for calls in rec.values() for call in calls if call[0] == "L"}
    for k in ("reject_tiger_lds_kernel<512>", "reject_tiger_once_kernel<512>", "reject_tiger_once_gather_kernel<512>", "reject_kernel<false, 2, 0, 512, false>",
              "reject_kernel<false, 1, 0, 256, false>", "reject_kernel<true, 0, 0, 256, false>", "reject_hist_kernel<8>", "reject_hist_kernel<12>",
              "reject_hist_kernel<0>", "reject_tab_hist_kernel", "is_multi_tab_step_kernel", "is_multi_ca_step_kernel", "is_multi_step_kernel<false, true, 8>",
              "is_multi_step_kernel<false, true, 12>", "is_multi_step_kernel<false, true, 0>", "is_multi_step_kernel<true, false, 0>", "mh_kernel",
              "cheat_kernel", "nested_update_kernel<true>", "nested_update_kernel<false>", "search_ca_hist_kernel<4>", "search_tabhist_kernel<true>",
              "search_tabhist_kernel<false>", "search_order_kernel", "lazy_reset_kernel", "reset_hist_flat_kernel", "nested_fill_kernel", "swap_buffers_kernel"):
        assert k in kernels, k
    for fam, variants in (("importance_kernel<", 9), ("search_hist_kernel<", 3), ("search_hist2_kernel<", 6), ("hist2_flat_search<", 6), ("search_kernel<", 40)):
        assert len({k for k in kernels if k.startswith(fam)}) >= variants, fam
    for fs in (2, 3, 4):
        assert f"reject_kernel<false, 0, {fs}, 256, true>" in kernels and f"reject_kernel<false, 0, {fs}, 256, false>" in kernels
    raised = {name for name, rec in EXPECTED.items() for calls in rec.values() for call in calls if call[0] == "A"}
    assert all(call[1] == 1 for rec in EXPECTED.values() for calls in rec.values() for call in calls if call[0] == "A")   # (always the kernel launched next)
    assert "search_grid_tab_bucket_importance_depth145" in raised and "search_grid_tab_bucket_importance_depth144" not in raised
    assert "importance_tiger_2049" in raised and "importance_tiger_small" not in raised


def test_the_decisions_have_one_home():
    """fba_launch_plan.h is built into the library, and the conditions it gathered are written nowhere else under csrc/"""
    assert os.path.join(CSRC, "fba_launch_plan.h") in N.HEADERS
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f))}
    count = lambda pattern, files: sum(len(re.findall(pattern, text[f])) for f in files)
    others = [f for f in text if f != "fba_launch_plan.h"]
    assert count(r"search_takes_compact", text) == 0
    assert count(r"__builtin_clz\(\(unsigned\)P\.S\)", others) == 0 and count(r"__builtin_clz\(\(unsigned\)P\.S\)", ["fba_launch_plan.h"]) == 1
    assert count(r"hist_row <= 8 \? 8", text) == 1 and count(r"hist_row <= 8 \? 8", ["fba_device.h"]) == 1        # hist_row_width, beside HistRow
    # the domain predicates themselves (fba_device.h: dom_is_tiger, dom_is_episodic) are the only places left that spell a tiger domain test out
    assert count(r"FBA_DOM_TIGER_EPISODIC \|\|", text) == 2 and count(r"FBA_DOM_TIGER_EPISODIC \|\|", ["fba_device.h"]) == 2
