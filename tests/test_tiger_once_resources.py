"""reject_tiger_once_kernel (the bench workload's belief update) and its FBA_TIGER_GATHER twin: no scratch, no spills, at most 128
registers, and LDS -- static plus the 17 N + 16 dynamic bytes of the largest filter -- that leaves two workgroups on a CU.
Checked on the code-object metadata hipcc emits (no GPU), like tests/test_kernel_resources.py for the kernels it names."""
import os
import re
import subprocess

from fba_pomdp_amd import _native as N

TIGER_LDS_MAX_N = 4096
LDS_PER_CU = 160 * 1024


def test_once_kernels_fit_two_workgroups_per_cu(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "fba_kernels.s"
    src = os.path.join(N.HERE, "csrc", "fba_kernels.hip")
    subprocess.check_call(["hipcc"] + flags + ["-I" + os.path.join(N.ROOT, "include"), "-S", "--cuda-device-only", "-o", str(out), src],
                          stderr=subprocess.DEVNULL)
    with open(os.path.join(N.HERE, "csrc", "fba_kernels.h")) as f:
        assert re.search(r"constexpr\s+int\s+TIGER_LDS_MAX_N\s*=\s*%d\s*;" % TIGER_LDS_MAX_N, f.read())
    with open(src) as f:      # the launcher's dynamic LDS of both entries, as the source states it
        assert len(re.findall(r"reject_tiger_once(?:_gather)?_kernel<512>\), dim3\(P\.E\), dim3\(512\), \(size_t\)P\.N \* 17 \+ 16,", f.read())) == 2
    meta = out.read_text()
    meta = meta[meta.index("amdhsa.kernels:"):]
    seen = {}
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        if "reject_tiger_once" in name:
            seen[name] = (get("private_segment_fixed_size"), get("vgpr_count"), get("vgpr_spill_count"), get("group_segment_fixed_size"))
    assert len(seen) == 2 and sum("gather" in n for n in seen) == 1, sorted(seen)
    for name, (scratch, vgprs, spills, lds) in seen.items():
        assert scratch == 0 and spills == 0 and vgprs <= 128, (name, scratch, vgprs, spills)
        assert 2 * (lds + 17 * TIGER_LDS_MAX_N + 16) <= LDS_PER_CU, (name, lds)
