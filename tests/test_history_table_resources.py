"""The kernels of the tabular gridworld BA-POMDP's history particles -- reject_tab_hist_kernel and is_multi_tab_step_kernel (the two
filters' update passes), search_tabhist_kernel (the bucket-tree search, both root samples) -- hold their values in registers: no scratch,
no spills, and the VGPR counts pinned below (the search within FBA_HIST2_WAVES = 3 waves per SIMD, 168 registers).  Checked on the
code-object metadata hipcc emits (no GPU), as test_kernel_resources.py does."""
import os
import re
import subprocess

from fba_pomdp_amd import _native as N

# (scratch bytes, VGPRs, spilled VGPRs)
PINNED = {
    "_ZN3fba22reject_tab_hist_kernelENS_7ProblemENS_11DeviceStateE": (0, 58, 0),
    "_ZN3fba24is_multi_tab_step_kernelENS_7ProblemENS_11DeviceStateE": (0, 34, 0),
    "_ZN3fba21search_tabhist_kernelILb0EEEvNS_7ProblemENS_11DeviceStateE": (0, 157, 0),   # importance filter: the weighted root sample
    "_ZN3fba21search_tabhist_kernelILb1EEEvNS_7ProblemENS_11DeviceStateE": (0, 139, 0),   # rejection filter: uniform_int(N)
}


def test_tabular_history_kernels_use_no_scratch(tmp_path):
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
