"""Resumed spans without a GPU: the built library exports fba_run_bapomdp_span and the header declares it under the unchanged ABI version,
the kernels of fba_restore.hip cross-compile for gfx950 without scratch or spills, the room rule of fba_snapshot_format.h -- header-only
and free of HIP -- holds at its edges when a stand-alone host program feeds it headers under the address and undefined-behaviour
sanitizers (the sanitizers see that program alone, never code loaded into Python), and the seeds of tests/resume_cases.py have the
properties tests/test_gpu_belief_resume.py relies on, established on the oracle."""
import inspect
import os
import re
import subprocess

import pytest

import fba_pomdp_amd as fba
import resume_cases as R
from fba_pomdp_amd import _native as N

CSRC = os.path.join(N.HERE, "csrc")
KERNELS = ("_ZN3fba14restore_kernelENS_7ProblemENS_11DeviceStateE", "_ZN3fba19restore_post_kernelENS_7ProblemENS_11DeviceStateE",
           "_ZN3fba22span_increments_kernelENS_7ProblemENS_18BeliefSnapshotArgsEi")


def test_the_library_exports_the_span_call():
    fba.build()
    lib = fba.load()
    assert "fba_run_bapomdp_span" in N.EXPORTS and hasattr(lib, "fba_run_bapomdp_span")
    assert os.path.join(CSRC, "fba_restore.hip") in N.SOURCES
    assert list(inspect.signature(fba.Engine.run_bapomdp).parameters) == ["self", "first_episode", "stop_episode", "beliefs"]
    sig = inspect.signature(fba.Engine.run_bapomdp).parameters
    assert (sig["first_episode"].default, sig["stop_episode"].default, sig["beliefs"].default) == (0, None, None)


def test_the_header_declares_the_call():
    header = open(os.path.join(N.ROOT, "include", "fba_hip.h")).read()
    assert re.search(r"int fba_run_bapomdp_span\(fba_ctx\* ctx, int32_t first_episode, int32_t stop_episode, const void\* blocks, int32_t nblocks, int64_t bytes,\s*"
                     r"fba_stat\* stats /\* \[episodes\] \*/\);", header)
    assert "#define FBA_ABI_VERSION 3 " in header and "#define FBA_SNAPSHOT_VERSION   1" in header
    assert "is not offered" not in header


def test_restore_kernels_use_no_scratch(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "fba_restore.s"
    subprocess.check_call(["hipcc"] + flags + ["-I" + os.path.join(N.ROOT, "include"), "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(CSRC, "fba_restore.hip")], stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        seen[name] = (get("private_segment_fixed_size"), get("vgpr_spill_count"), get("vgpr_count"))
    assert set(seen) == set(KERNELS)
    for name, (scratch, spills, vgprs) in seen.items():
        assert (scratch, spills) == (0, 0) and vgprs <= 64, (name, scratch, spills, vgprs)
    # restore_kernel moves its records in 16-byte pieces, four in flight per lane
    body = text[text.index(KERNELS[0] + ":"):text.index(".Lfunc_end0")]
    assert body.count("global_load_dwordx4") >= 4 and body.count("global_store_dwordx4") >= 4


def test_the_room_rule_under_sanitizers(tmp_path):
    exe = tmp_path / "span_room_check"
    src = os.path.join(N.ROOT, "tests", "span_room_check.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-I" + os.path.join(N.ROOT, "include"), "-I" + CSRC, src, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "span_room_check: ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.mark.parametrize("name", R.GRIDWORLD_HISTORY)
def test_the_history_seeds_reach_every_stride(name):
    """some run holds at least 15 entries after two episodes and at least 31 after four, and the first episode leaves 14 at most"""
    assert R.entries_after(name, 1).max() <= 14
    assert R.entries_after(name, 2).max() >= 15 and R.entries_after(name, 2).max() <= 30
    assert R.entries_after(name, 4).max() >= 31
    assert R.strides_met(name) == {64, 128, R.RECORD_BYTES}


def test_collision_avoidance_records_stay_short():
    """the plane's last step is terminal: 3 updates per episode at most, 12 entries after four episodes (resume_cases.py)"""
    name = "collision_avoidance_5x5x2_history"
    ref = R.oracle_whole(name)
    assert ref["lengths"].max() <= 4 and ref["updates"].max() <= 3 and R.strides_met(name) == {64}


@pytest.mark.parametrize("name", R.SPLIT_FORMATS)
def test_the_oracle_finishes_every_update(name):
    ref = R.oracle_whole(name)
    assert ref["refused"] is None, ref["refused"]
    assert ref["lengths"].min() >= 1 and len(ref["trace"]) == ref["lengths"].sum()


def test_the_room_rule_meets_the_refusal_cases():
    """the blocks of span [0, 2) cannot take episodes [1, 5): what test_refusals_leave_the_context_untouched asks to be refused"""
    assert int(R.entries_after("gridworld3_history_importance", 2)[0]) + 4 * R.HORIZON > R.EPISODES * R.HORIZON
    assert int(R.oracle_whole("packed_tiger")["lengths"][0, :2].sum()) + 4 * R.HORIZON > R.EPISODES * R.HORIZON
