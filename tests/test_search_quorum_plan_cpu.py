"""Which boundary quorum a search launch gets (fba_launch_plan.h: search_plan(P, D).quorum, which launch_search writes into the launch's
DeviceState), without a GPU.  The GPU tests cannot pin it -- results do not depend on the quorum, only speed does -- so it is pinned
here: 60 for the two instantiations it was measured for, 64 for every other kernel that the case table of tests/launch_plan_cases.py
reaches; DeviceState::search_quorum of 1..64 instead of either; anything else there, and anything but 1..64 in FBA_SEARCH_QUORUM, means
the default.  tests/search_quorum_plan.cpp calls search_plan and search_quorum_switch on the cases; host code only."""
import os
import subprocess

import pytest

import launch_plan_cases as T
from fba_pomdp_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = {"search_kernel<true,4,false,2,1,0,false,false,true>": 60,    # packed tabular tiger (C1, C2)
            "search_kernel<true,4,false,0,2,3,false,true,true>": 60}     # packed factored tiger of size 3 (C3)
LOCKSTEP = 64
SEARCHES = [c for c in T.CASES if "s" in c["launchers"]]
SWITCH = {"unset": (None, 0), "one": ("1", 1), "sixty": ("60", 60), "sixty_four": ("64", 64), "zero": ("0", 0), "sixty_five": ("65", 0),
          "negative": ("-3", 0), "word": ("all", 0), "empty": ("", 0), "huge": ("4096", 0)}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = tmp_path_factory.mktemp("search_quorum_plan") / "search_quorum_plan"
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O0", "-std=c++17", "-w", "-I" + os.path.join(N.ROOT, "include"),
                           "-I" + os.path.join(N.HERE, "csrc"), "-x", "hip", os.path.join(HERE, "search_quorum_plan.cpp"), "-o", str(exe)])
    lines = []
    for c in SEARCHES:
        fields = " ".join(f"{k[0]}.{k[2:]}={v}" for k, v in c["fields"].items())
        lines.append(f"plan {c['name']} {fields}")
        for q in (1, 33, 64, 0, 65, -1):
            lines.append(f"plan {c['name']}@{q} {fields} D.search_quorum={q}")
    lines += [f"switch {name}" + ("" if text is None else " " + text) for name, (text, _) in SWITCH.items()]
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60).stdout
    plans, switches = {}, {}
    for line in out.splitlines():
        what, name, *rest = line.split()
        if what == "plan":
            plans[name] = (rest[0], int(rest[1]))
        else:
            switches[name] = int(rest[0])
    return plans, switches


def test_the_case_table_reaches_both_measured_kernels_and_others(answers):
    kernels = {answers[0][c["name"]][0] for c in SEARCHES}
    assert set(MEASURED) <= kernels and len(kernels - set(MEASURED)) >= 20 and "other" in kernels


@pytest.mark.parametrize("name", [c["name"] for c in SEARCHES])
def test_default_and_override(name, answers):
    plans = answers[0]
    kernel, quorum = plans[name]
    default = MEASURED.get(kernel, LOCKSTEP)
    assert quorum == default, (kernel, quorum)
    for q in (1, 33, 64):   # (the history-record searches have no such schedule: their plan keeps saying 64)
        assert plans[f"{name}@{q}"] == (kernel, q if kernel != "other" else LOCKSTEP)
    for q in (0, 65, -1):
        assert plans[f"{name}@{q}"] == (kernel, default)


def test_the_switch_takes_1_to_64_and_nothing_else(answers):
    assert answers[1] == {name: value for name, (_, value) in SWITCH.items()}
