"""The kernels of the rejection filter on history particles -- reject_hist_kernel (the update), reset_hist_flat_kernel (the reset),
hist2_flat_search (the bucket-tree search with FlatFilter's root sample) -- hold their values in registers: no scratch, no spills,
at most 168 VGPRs.  search_hist2_kernel, whose body hist2_flat_search shares, keeps the registers and spills it had before the flat
variant existed.  Checked on the code-object metadata hipcc emits (no GPU), as test_kernel_resources.py does."""
import os
import re
import subprocess

from fba_pomdp_amd import _native as N

# search_hist2_kernel<K, LROWS>: (scratch bytes, VGPRs, spilled VGPRs) before hist2_flat_search was added
HIST2_BEFORE = {
    (8, True): (12, 168, 2), (8, False): (12, 168, 2),
    (12, True): (12, 168, 2), (12, False): (12, 168, 2),
    (16, True): (32, 168, 7), (16, False): (28, 168, 6),
}


def _kernels(tmp_path):
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
    return seen


def test_history_rejection_kernels_use_no_scratch(tmp_path):
    seen = _kernels(tmp_path)
    update = {n: v for n, v in seen.items() if "reject_hist_kernel" in n}
    assert len(update) == 3, sorted(seen)        # the prior's rows from LDS (K = 8 / 12) or from L2 (K = 0)
    reset = {n: v for n, v in seen.items() if "reset_hist_flat_kernel" in n}
    assert len(reset) == 1, sorted(seen)
    flat = {n: v for n, v in seen.items() if "hist2_flat_search" in n}
    assert len(flat) == 6, sorted(seen)          # three row widths x {every row from LDS, transition rows from HBM}
    for name, (scratch, vgprs, spills) in {**update, **reset, **flat}.items():
        assert scratch == 0 and spills == 0 and vgprs <= 168, (name, scratch, vgprs, spills)
    hist2 = {}
    for name, v in seen.items():
        m = re.search(r"search_hist2_kernelILi(\d+)ELb([01])E", name)
        if m:
            hist2[(int(m.group(1)), m.group(2) == "1")] = v
    assert hist2 == HIST2_BEFORE
