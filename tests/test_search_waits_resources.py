"""The episodic-tiger instantiations of search_kernel (ETIGER: the last template argument): no scratch, no spills, the static LDS
they have always had, and no resident wave lost to registers -- the limits any change to that loop has to keep (the search answers
to its fourth wave per SIMD more than to anything else).  Checked on the code-object metadata hipcc emits
(no GPU), as test_kernel_resources.py does.

Four waves per SIMD need at most 128 VGPRs, three at most 168.  The instantiations over packed tabular tiger records (the
benchmark's: 125) and over the tiger POMDP (123) hold four; the ones over dense tabular records (129: their LDS allows three
waves anyway) and over packed factored-tiger records (145-149) hold three and must keep three."""
import os
import re
import subprocess

from fba_pomdp_amd import _native as N

ET = "_ZN3fba13search_kernelILb%dELi4ELb0ELi%dELi%dELi%dELb%dELb%dELb1EEEvNS_7ProblemENS_11DeviceStateE"
# instantiation -> (most VGPRs, static LDS bytes)
LIMITS = {
    ET % (1, 2, 1, 0, 0, 0): (128, 96),    # packed tabular tiger: the default benchmark (the 96 bytes are the prior's 24 floats)
    ET % (0, 0, 0, 0, 1, 0): (128, 0),     # tiger POMDP planning
    ET % (1, 1, 1, 0, 0, 0): (168, 0),     # dense tabular tiger
    ET % (1, 0, 2, 2, 0, 1): (168, 0),     # packed factored tiger, 2 / 3 / 4 state features
    ET % (1, 0, 2, 3, 0, 1): (168, 0),
    ET % (1, 0, 2, 4, 0, 1): (168, 0),
}


def test_episodic_tiger_search_keeps_its_registers_and_lds(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "fba_search.s"
    src = os.path.join(N.HERE, "csrc", "fba_search.hip")
    subprocess.check_call(["hipcc"] + flags + ["-I" + os.path.join(N.ROOT, "include"), "-S", "--cuda-device-only", "-o", str(out), src],
                          stderr=subprocess.DEVNULL)
    meta = out.read_text()
    meta = meta[meta.index("amdhsa.kernels:"):]
    seen = {}
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        seen[name] = (get("private_segment_fixed_size"), get("vgpr_count"), get("vgpr_spill_count"), get("group_segment_fixed_size"))
    etiger = {n for n in seen if re.search(r"search_kernelI.*Lb1EEEvNS_7Problem", n)}
    assert etiger == set(LIMITS), sorted(etiger ^ set(LIMITS))
    for name, (vgpr_max, lds) in LIMITS.items():
        scratch, vgprs, spills, static_lds = seen[name]
        assert scratch == 0 and spills == 0, (name, scratch, spills)
        assert vgprs <= vgpr_max, (name, vgprs)
        assert static_lds == lds, (name, static_lds)
