"""fba_belief_predict without a GPU: the built library exports it and fba_predict_lens, and the kernels of fba_predict.hip
cross-compile for gfx950 without scratch or spills, their VGPR counts pinned.  Read from the code-object metadata hipcc emits, as
test_belief_summary_cpu.py does."""
import os
import re
import subprocess

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

ARGS = "ENS_7ProblemENS_11DeviceStateENS_17BeliefPredictArgsE"
# (scratch bytes, VGPRs, spilled VGPRs)
PINNED = {
    "_ZN3fba20predict_total_kernel" + ARGS: (0, 10, 0),
    "_ZN3fba26predict_hist_finish_kernelENS_7ProblemENS_17BeliefPredictArgsE": (0, 15, 0),
    "_ZN3fba19predict_hist_kernelILi1EEEv" + ARGS[1:]: (0, 90, 0),    # gridworld FBA-POMDP records
    "_ZN3fba19predict_hist_kernelILi2EEEv" + ARGS[1:]: (0, 52, 0),    # tabular gridworld records
    "_ZN3fba19predict_hist_kernelILi3EEEv" + ARGS[1:]: (0, 120, 0),   # collision-avoidance records
    "_ZN3fba19predict_rows_kernelILi0EEEv" + ARGS[1:]: (0, 84, 0),    # fp32 counts
    "_ZN3fba19predict_rows_kernelILi1EEEv" + ARGS[1:]: (0, 78, 0),    # packed tiger
    "_ZN3fba19predict_rows_kernelILi2EEEv" + ARGS[1:]: (0, 91, 0),    # packed factored tiger, 2 to 4 state features
    "_ZN3fba19predict_rows_kernelILi3EEEv" + ARGS[1:]: (0, 91, 0),
    "_ZN3fba19predict_rows_kernelILi4EEEv" + ARGS[1:]: (0, 91, 0),
}


def test_the_library_exports_the_prediction():
    fba.build()
    lib = fba.load()
    for name in ("fba_predict_lens", "fba_belief_predict"):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert os.path.join(N.HERE, "csrc", "fba_predict.hip") in N.SOURCES


def test_the_header_declares_both_calls():
    header = open(os.path.join(N.ROOT, "include", "fba_hip.h")).read()
    assert re.search(r"int fba_predict_lens\(const fba_ctx\* ctx, int32_t\* TL, int32_t\* OL\);", header)
    assert re.search(r"int fba_belief_predict\(fba_ctx\* ctx, int32_t first, int32_t count, int32_t nq,", header)
    assert "#define FBA_ABI_VERSION 3 " in header


def test_predict_kernels_use_no_scratch(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "fba_predict.s"
    src = os.path.join(N.HERE, "csrc", "fba_predict.hip")
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
