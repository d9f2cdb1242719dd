#!/usr/bin/env python3
"""Records what the tick launchers of a named commit launch for the cases of tests/launch_plan_cases.py.

    python scripts/record_launch_plan.py COMMIT                  prints one JSON line per case
    python scripts/record_launch_plan.py COMMIT --write          rewrites tests/golden/launch_plan_expected.jsonl
    python scripts/record_launch_plan.py COMMIT --write NAME...  re-records those cases only and keeps the other lines

The commit's sources are checked out into a temporary directory (git archive) and this tree's tests/launch_capture.cpp is built against
them, so the record comes from launchers that are trusted -- never from the code a test is about to check.  No GPU is needed."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import launch_plan_cases as T   # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if a != "--write"]
    if not args:
        sys.exit(__doc__)
    commit, names = args[0], args[1:]
    with tempfile.TemporaryDirectory() as tmp:
        archive = subprocess.run(["git", "-C", ROOT, "archive", commit, "fba_pomdp_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=archive, check=True)
        exe = os.path.join(tmp, "launch_capture")
        T.build_capture(exe, csrc=os.path.join(tmp, "fba_pomdp_amd", "csrc"), include=os.path.join(tmp, "include"))
        seen = T.capture(exe, [T.BY_NAME[n] for n in names] if names else None)
    table = T.expected() if names else {}
    table.update(seen)
    lines = [json.dumps({"name": c["name"], **table[c["name"]]}) + "\n" for c in T.CASES if c["name"] in table]
    if "--write" in sys.argv[1:]:
        with open(T.GOLDEN, "w") as f:
            f.writelines(lines)
    else:
        sys.stdout.writelines(lines)


if __name__ == "__main__":
    main()
