"""The kernels of the collision-avoidance FBA-POMDP's history particles -- is_multi_ca_step_kernel (the importance filter's update pass) and
search_ca_hist_kernel (the lane-per-tree search over staged records) -- cross-compile for gfx950 and hold their values in registers: no
scratch, no spills, and the VGPR counts pinned below.  Checked on the code-object metadata hipcc emits (no GPU), as
test_kernel_resources.py does."""
import os
import re
import subprocess

from fba_pomdp_amd import _native as N

# (scratch bytes, VGPRs, spilled VGPRs)
PINNED = {
    "_ZN3fba23is_multi_ca_step_kernelENS_7ProblemENS_11DeviceStateE": (0, 59, 0),
    "_ZN3fba21search_ca_hist_kernelILi4EEEvNS_7ProblemENS_11DeviceStateE": (0, 145, 0),   # (its occupancy is set by the LDS of the staged records, not by these)
}


def test_collision_avoidance_history_kernels_use_no_scratch(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    jobs = []
    for base in ("fba_search", "fba_kernels"):
        out = tmp_path / (base + ".s")
        src = os.path.join(N.HERE, "csrc", base + ".hip")
        jobs.append((out, subprocess.Popen(["hipcc"] + flags + ["-I" + os.path.join(N.ROOT, "include"), "-S", "--cuda-device-only", "-o", str(out), src],
                                           stderr=subprocess.DEVNULL)))
    seen = {}
    for out, p in jobs:
        assert p.wait() == 0
        meta = out.read_text()
        meta = meta[meta.index("amdhsa.kernels:"):]
        for blk in meta.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
            seen[name] = (get("private_segment_fixed_size"), get("vgpr_count"), get("vgpr_spill_count"))
    assert {n: seen.get(n) for n in PINNED} == PINNED
