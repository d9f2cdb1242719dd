"""fba_belief_forecast without a GPU: the built library exports it, and the kernels of fba_forecast.hip cross-compile for gfx950
without scratch or spills, their VGPR counts pinned.  Read from the code-object metadata hipcc emits, as
test_belief_predict_cpu.py does."""
import os
import re
import subprocess

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

ARGS = "ENS_7ProblemENS_11DeviceStateENS_18BeliefForecastArgsE"
# (scratch bytes, VGPRs, spilled VGPRs).  Three counts moved when the factor phase became belief_factors (fba_belief_factors.h), a function
# the kernel inlines, where it had been statements of the kernel's own body (91, 87 and 104 then; the function's statements put back into
# a kernel's body give the old counts, so it is the function boundary that moves them).  None of them changes the waves a SIMD can
# hold, min(8, 512 // (ceil(count / 8) * 8)): 5 for any count from 86 to 96, 4 for 103 and 104.
PINNED = {
    "_ZN3fba22forecast_finish_kernel" + ARGS: (0, 24, 0),
    "_ZN3fba21forecast_chunk_kernelILi0EEEv" + ARGS[1:]: (0, 40, 0),    # fp32 counts
    "_ZN3fba21forecast_chunk_kernelILi1EEEv" + ARGS[1:]: (0, 40, 0),    # packed tiger
    "_ZN3fba21forecast_chunk_kernelILi2EEEv" + ARGS[1:]: (0, 41, 0),    # packed factored tiger, 2 to 4 state features
    "_ZN3fba21forecast_chunk_kernelILi3EEEv" + ARGS[1:]: (0, 41, 0),
    "_ZN3fba21forecast_chunk_kernelILi4EEEv" + ARGS[1:]: (0, 41, 0),
    "_ZN3fba21forecast_chunk_kernelILi5EEEv" + ARGS[1:]: (0, 95, 0),    # gridworld FBA-POMDP records (91 before: 5 waves as before)
    "_ZN3fba21forecast_chunk_kernelILi6EEEv" + ARGS[1:]: (0, 91, 0),    # tabular gridworld records (87 before: 5 waves as before)
    "_ZN3fba21forecast_chunk_kernelILi7EEEv" + ARGS[1:]: (0, 103, 0),   # collision-avoidance records (104 before: 4 waves as before)
}


def test_the_library_exports_the_forecast():
    fba.build()
    lib = fba.load()
    assert "fba_belief_forecast" in N.EXPORTS and hasattr(lib, "fba_belief_forecast")
    assert os.path.join(N.HERE, "csrc", "fba_forecast.hip") in N.SOURCES


def test_the_header_declares_the_call():
    header = open(os.path.join(N.ROOT, "include", "fba_hip.h")).read()
    assert re.search(r"int fba_belief_forecast\(fba_ctx\* ctx, int32_t first, int32_t count,", header)
    assert "#define FBA_ABI_VERSION 3 " in header


def test_forecast_kernels_use_no_scratch(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "fba_forecast.s"
    src = os.path.join(N.HERE, "csrc", "fba_forecast.hip")
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
