"""fba_probe without a GPU: the built library exports the three calls, the header declares them under the unchanged ABI version, and
the kernels of fba_probe.hip cross-compile for gfx950 without scratch or spills, their VGPR counts pinned.  Read from the code-object
metadata hipcc emits, as test_belief_forecast_cpu.py does."""
import os
import re
import subprocess

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

ARGS = "ENS_7ProblemENS_11DeviceStateENS_15BeliefProbeArgsE"
# (scratch bytes, VGPRs, spilled VGPRs).  Two counts moved when the factor phase became belief_factors (fba_belief_factors.h), a function
# the kernel inlines, where it had been statements of the kernel's own body (93 and 87 then; the function's statements put back into
# the kernel's body give those again, so it is the function boundary that moves them).  Neither changes the waves a SIMD can hold,
# min(8, 512 // (ceil(count / 8) * 8)): 5 for any count from 86 to 96.
PINNED = {
    "_ZN3fba19probe_finish_kernel" + ARGS: (0, 14, 0),
    "_ZN3fba18probe_chunk_kernelILi0EEEv" + ARGS[1:]: (0, 46, 0),    # fp32 counts
    "_ZN3fba18probe_chunk_kernelILi1EEEv" + ARGS[1:]: (0, 47, 0),    # packed tiger
    "_ZN3fba18probe_chunk_kernelILi2EEEv" + ARGS[1:]: (0, 47, 0),    # packed factored tiger, 2 to 4 state features
    "_ZN3fba18probe_chunk_kernelILi3EEEv" + ARGS[1:]: (0, 47, 0),
    "_ZN3fba18probe_chunk_kernelILi4EEEv" + ARGS[1:]: (0, 47, 0),
    "_ZN3fba18probe_chunk_kernelILi5EEEv" + ARGS[1:]: (0, 95, 0),    # gridworld FBA-POMDP records (93 before: 5 waves as before)
    "_ZN3fba18probe_chunk_kernelILi6EEEv" + ARGS[1:]: (0, 91, 0),    # tabular gridworld records (87 before: 5 waves as before)
    "_ZN3fba18probe_chunk_kernelILi7EEEv" + ARGS[1:]: (0, 104, 0),   # collision-avoidance records
}
CALLS = ("fba_probe_enable", "fba_probe_count", "fba_get_probe")


def test_the_library_exports_the_probe():
    fba.build()
    lib = fba.load()
    for name in CALLS:
        assert name in N.EXPORTS and hasattr(lib, name), name
    assert os.path.join(N.HERE, "csrc", "fba_probe.hip") in N.SOURCES


def test_the_header_declares_the_calls():
    header = open(os.path.join(N.ROOT, "include", "fba_hip.h")).read()
    assert re.search(r"int fba_probe_enable\(fba_ctx\* ctx, int32_t first, int32_t count, int32_t capacity\);", header)
    assert re.search(r"int fba_probe_count\(const fba_ctx\* ctx, int64_t\* seen\);", header)
    assert re.search(r"int fba_get_probe\(const fba_ctx\* ctx, fba_probe_rec\* out, int32_t cap\);", header)
    assert "#define FBA_ABI_VERSION 3 " in header
    # the record as the header lays it out: eight int32, three doubles
    assert N.PROBE_DTYPE.itemsize == 56
    assert N.PROBE_DTYPE.names == ("run", "episode", "t", "slot", "action", "obs", "state", "reserved", "evidence", "next_true", "post_true")


def test_probe_kernels_use_no_scratch(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "fba_probe.s"
    src = os.path.join(N.HERE, "csrc", "fba_probe.hip")
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
