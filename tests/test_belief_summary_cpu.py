"""fba_belief_summary without a GPU: the built library exports it, the header's fba_belief_summary_head and the ctypes mirror agree
field by field, and the kernels of fba_summary.hip cross-compile for gfx950 without scratch or spills, their VGPR counts pinned.
Read from the code-object metadata hipcc emits, as test_history_ca_resources.py does."""
import ctypes as C
import os
import re
import subprocess

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARGS = "ENS_7ProblemENS_11DeviceStateENS_17BeliefSummaryArgsE"
# (scratch bytes, VGPRs, spilled VGPRs)
PINNED = {
    "_ZN3fba19summary_head_kernel" + ARGS: (0, 27, 0),
    "_ZN3fba20summary_prior_kernel" + ARGS: (0, 18, 0),
    "_ZN3fba22summary_scatter_kernelILi1EEEv" + ARGS[1:]: (0, 39, 0),   # gridworld FBA-POMDP records
    "_ZN3fba22summary_scatter_kernelILi2EEEv" + ARGS[1:]: (0, 23, 0),   # tabular gridworld records
    "_ZN3fba22summary_scatter_kernelILi3EEEv" + ARGS[1:]: (0, 39, 0),   # collision-avoidance records
    "_ZN3fba19summary_cols_kernelILi0EEEv" + ARGS[1:]: (0, 25, 0),      # fp32 counts
    "_ZN3fba19summary_cols_kernelILi1EEEv" + ARGS[1:]: (0, 26, 0),      # packed tiger
    "_ZN3fba19summary_cols_kernelILi2EEEv" + ARGS[1:]: (0, 27, 0),      # packed factored tiger, 2 to 4 state features
    "_ZN3fba19summary_cols_kernelILi3EEEv" + ARGS[1:]: (0, 27, 0),
    "_ZN3fba19summary_cols_kernelILi4EEEv" + ARGS[1:]: (0, 27, 0),
}


def test_the_library_exports_the_summary():
    fba.build()
    lib = fba.load()
    assert "fba_belief_summary" in N.EXPORTS and hasattr(lib, "fba_belief_summary")
    assert os.path.join(N.HERE, "csrc", "fba_summary.hip") in N.SOURCES


def test_head_struct_matches_the_header():
    """sizes and offsets of fba_belief_summary_head as a C compiler lays the header's struct out, against the ctypes Structure and the numpy dtype"""
    header = open(os.path.join(ROOT, "include", "fba_hip.h")).read()
    body = re.search(r"typedef struct fba_belief_summary_head \{(.*?)\} fba_belief_summary_head;", header, re.S).group(1)
    fields = re.findall(r"^\s*(double|int32_t)\s+(\w+);", body, re.M)
    assert [n for _, n in fields] == ["weight_total", "weight_sq_total", "particles", "weighted"]
    size = {"double": 8, "int32_t": 4}
    off, expect = 0, {}
    for t, n in fields:                      # natural alignment, as the C ABI of x86-64 gives these two types
        off = (off + size[t] - 1) // size[t] * size[t]
        expect[n] = (off, size[t])
        off += size[t]
    total = (off + 7) // 8 * 8
    assert C.sizeof(N.BeliefSummaryHead) == N.SUMMARY_HEAD_DTYPE.itemsize == total == 24
    for n, (o, s) in expect.items():
        f = getattr(N.BeliefSummaryHead, n)
        assert (f.offset, f.size) == (o, s), n
        assert (N.SUMMARY_HEAD_DTYPE.fields[n][1], N.SUMMARY_HEAD_DTYPE.fields[n][0].itemsize) == (o, s), n
    assert [n for n, _ in N.BeliefSummaryHead._fields_] == [n for _, n in fields]


def test_summary_kernels_use_no_scratch(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "fba_summary.s"
    src = os.path.join(N.HERE, "csrc", "fba_summary.hip")
    subprocess.check_call(["hipcc"] + flags + ["-I" + os.path.join(N.ROOT, "include"), "-S", "--cuda-device-only", "-o", str(out), src],
                          stderr=subprocess.DEVNULL)
    meta = out.read_text()
    meta = meta[meta.index("amdhsa.kernels:"):]
    seen = {}
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        seen[name] = (get("private_segment_fixed_size"), get("vgpr_count"), get("vgpr_spill_count"))
    assert seen == PINNED
