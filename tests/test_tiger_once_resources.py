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
    with open(os.path.join(N.HERE, "csrc", "fba_launch_plan.h")) as f:      # the dynamic LDS and block of both entries, as update_plan states them ...
        assert len(re.findall(r"kernel_key\(D\.ab_tiger_gather \? K_REJECT_TIGER_ONCE_GATHER : K_REJECT_TIGER_ONCE\), 512, 0, 1, \(size_t\)P\.N \* 17 \+ 16\)",
                              f.read())) == 1
    with open(src) as f:      # ... and the two instantiations the launcher has behind those keys, launched with the step's LDS
        text = f.read()
        assert len(re.findall(r"case kernel_key\(K_REJECT_TIGER_ONCE(?:_GATHER)?\): FBA_STEP\(reject_tiger_once(?:_gather)?_kernel<512>\)", text)) == 2
        assert "#define FBA_STEP(...) { hipLaunchKernelGGL((__VA_ARGS__), grid, block, s.lds, st, P, D); return; }" in text
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
