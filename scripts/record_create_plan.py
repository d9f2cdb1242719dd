#!/usr/bin/env python3
"""Prints what fba_create decides for every case of tests/create_plan_cases.py, and the device memory each made context takes.

    python scripts/record_create_plan.py                 the library of this tree
    FBA_LIB=/path/to/libfba_hip.so python scripts/...    another build of it (the A/B of profiles/r15_create_plan.txt)

The first block is one JSON line per case: the lines of tests/golden/create_plan_expected.jsonl, which are recorded at a commit whose
fba_create is trusted, never taken from the code a test is about to check.  The second block ("# " lines) lists, per made context,
hipMemGetInfo's free bytes before fba_create minus the free bytes while the context exists (the runtime is loaded and has made and
destroyed one context before the first case).  The script writes no file."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import create_plan_cases as T   # noqa: E402
import fba_pomdp_amd._native as N   # noqa: E402


def main():
    L = N.load()
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        free, total = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    T.observe(L, T.BY_NAME["tiger_table_packed"])
    seen, took = {}, {}
    for case in T.CASES:
        before = free_bytes()
        during = []
        seen[case["name"]] = T.observe(L, case, probe=lambda h: during.append(free_bytes()))
        if during:
            took[case["name"]] = before - during[0]
    for name, what in seen.items():
        print(json.dumps({"name": name, **what}))
    print("# device bytes per made context")
    for name, b in took.items():
        print(f"# {name:44s} {b:12d}")


if __name__ == "__main__":
    main()
