"""fba_step_stat without a GPU: the header's layout is the one the Python side reads, and the translation unit of its kernel compiles for
gfx950 without scratch memory or spilled registers (the code-object metadata hipcc emits, as test_kernel_resources.py reads it)."""
import os
import re
import subprocess

from fba_pomdp_amd import _native as N

MEMBERS = ["steps", "terminals", "action", "root_visits", "nodes_sum", "depth_sum", "attempts_steps", "attempts_sum", "nodes_max", "depth_max",
           "attempts_max", "reserved", "reward_sum", "reward_sq_sum", "value_sum", "value_sq_sum", "probed", "evidence_zero", "evidence_sum",
           "log_evidence_sum", "log_evidence_sq_sum", "next_true_sum", "post_ratio_sum"]


def test_the_header_and_the_dtype_agree(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    lines = "".join(f'    printf("{m} %zu\\n", offsetof(fba_step_stat, {m}));\n' for m in MEMBERS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fba_hip.h"\nint main(void)\n{\n'
                   '    printf("sizeof %zu\\n", sizeof(fba_step_stat));\n' + lines + "    return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(N.ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    dt = N.STEP_STAT_DTYPE
    assert int(got.pop("sizeof")) == dt.itemsize == 536
    assert list(dt.names) == MEMBERS
    assert {m: int(v) for m, v in got.items()} == {m: dt.fields[m][1] for m in MEMBERS}
    assert all(dt.fields[m][1] % 8 == 0 for m in MEMBERS if m not in ("depth_max", "reserved"))
    assert dt["action"].shape == dt["root_visits"].shape == (N.MAX_ACTIONS,)
    assert "fba_step_stats_enable" in N.EXPORTS and "fba_get_step_stats" in N.EXPORTS


def test_the_kernel_uses_no_scratch(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "fba_step_stats.s"
    src = os.path.join(N.HERE, "csrc", "fba_step_stats.hip")
    assert src in N.SOURCES
    subprocess.check_call(["hipcc"] + flags + ["-I" + os.path.join(N.ROOT, "include"), "-S", "--cuda-device-only", "-o", str(out), src],
                          stderr=subprocess.DEVNULL)
    meta = out.read_text()
    meta = meta[meta.index("amdhsa.kernels:"):]
    seen = {}
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        seen[name] = (get("private_segment_fixed_size"), get("vgpr_count"), get("vgpr_spill_count"), get("sgpr_spill_count"), get("group_segment_fixed_size"))
    assert len(seen) == 1 and "step_stats_kernel" in next(iter(seen)), sorted(seen)
    scratch, vgprs, vspills, sspills, lds = next(iter(seen.values()))
    assert scratch == 0 and vspills == 0 and sspills == 0, seen
    assert vgprs <= 128, seen      # 1 024 threads: sixteen waves on a CU, four per SIMD
    assert lds == 0, seen          # the table of partial rows is dynamic LDS, sized by the launcher
