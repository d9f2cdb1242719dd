"""fba_belief_structures without a GPU: the built library exports it, the header's fba_structure_head and the numpy mirror agree field
by field, fba_structures.hip cross-compiles for gfx950 without scratch, and the host-callable helpers of fba_structures.h (hash,
equality, the order of the top list) pass their stand-alone check under the host sanitizers."""
import os
import re
import subprocess

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(N.HERE, "csrc")


def _header():
    return open(os.path.join(ROOT, "include", "fba_hip.h")).read()


def test_the_library_exports_the_call():
    fba.build()
    lib = fba.load()
    for name in ("fba_structure_lens", "fba_belief_structures"):
        assert name in N.EXPORTS and hasattr(lib, name), name
    assert os.path.join(CSRC, "fba_structures.hip") in N.SOURCES
    assert os.path.join(CSRC, "fba_structures.h") in N.HEADERS
    assert lib.fba_abi_version() == 3


def test_the_header_declares_the_call():
    h = _header()
    assert re.search(r"#define FBA_ABI_VERSION 3\b", h)
    assert int(re.search(r"#define FBA_STRUCT_MAX_TOP (\d+)", h).group(1)) == N.STRUCT_MAX_TOP == 64
    table = int(re.search(r"#define FBA_STRUCT_TABLE (\d+)", h).group(1))
    assert table == N.STRUCT_TABLE and table >= 2048
    assert re.search(r"int fba_structure_lens\(const fba_ctx\* ctx, int32_t\* n_words, int32_t\* n_sets\);", h)
    decl = re.search(r"int fba_belief_structures\((.*?)\);", h, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["fba_ctx* ctx", "int32_t first", "int32_t count", "int32_t top_k", "int32_t nq", "const uint32_t* query", "fba_structure_head* head",
                    "double* set_mass", "uint32_t* top_words", "double* top_mass", "double* query_mass"]
    assert len(fba.load().fba_belief_structures.argtypes) == len(args)


def test_head_struct_matches_the_header():
    """sizes and offsets of fba_structure_head as a C compiler lays the header's struct out, against the numpy dtype"""
    body = re.search(r"typedef struct fba_structure_head \{(.*?)\} fba_structure_head;", _header(), re.S).group(1)
    fields = re.findall(r"^\s*(double|int32_t)\s+(\w+);", body, re.M)
    assert [n for _, n in fields] == ["weight_total", "unplaced_mass", "distinct", "overflow", "stored", "reserved"]
    size = {"double": 8, "int32_t": 4}
    off = 0
    for t, n in fields:                      # natural alignment, as the C ABI of x86-64 gives these two types
        off = (off + size[t] - 1) // size[t] * size[t]
        assert (N.STRUCTURE_HEAD_DTYPE.fields[n][1], N.STRUCTURE_HEAD_DTYPE.fields[n][0].itemsize) == (off, size[t]), n
        off += size[t]
    assert N.STRUCTURE_HEAD_DTYPE.itemsize == (off + 7) // 8 * 8 == 32
    assert list(N.STRUCTURE_HEAD_DTYPE.names) == [n for _, n in fields]


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "fba_hip.h"\n'
                   "_Static_assert(sizeof(fba_structure_head) == 32, \"fba_structure_head\");\n"
                   "int use(fba_ctx* c, fba_structure_head* h) { int32_t w, s; fba_structure_lens(c, &w, &s);\n"
                   "    return fba_belief_structures(c, 0, 1, FBA_STRUCT_MAX_TOP, 0, 0, h, 0, 0, 0, 0) + FBA_STRUCT_TABLE; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_structures_kernel_cross_compiles_without_scratch(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "fba_structures.s"
    subprocess.check_call(["hipcc"] + flags + ["-I" + os.path.join(N.ROOT, "include"), "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(CSRC, "fba_structures.hip")], stderr=subprocess.DEVNULL)
    meta = out.read_text()
    meta = meta[meta.index("amdhsa.kernels:"):]
    seen = {}
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        seen[name] = (get("private_segment_fixed_size"), get("vgpr_spill_count"), get("group_segment_fixed_size"))
    assert list(seen) == ["_ZN3fba17structures_kernelENS_7ProblemENS_11DeviceStateENS_20BeliefStructuresArgsE"]
    scratch, spills, static_lds = next(iter(seen.values()))
    assert scratch == 0 and spills == 0
    # two workgroups share a CU's 160 KB of LDS: the static part and the dynamic part of launch_belief_structures (fba_structures.hip)
    dynamic = (2 * N.STRUCT_TABLE + 1024 + 1024) * 8 + N.STRUCT_TABLE * 4
    assert 2 * (static_lds + dynamic) <= 160 * 1024 and static_lds + dynamic <= 64 * 1024


def test_hash_and_order_helpers_under_sanitizers(tmp_path):
    exe = tmp_path / "structure_order_check"
    src = os.path.join(N.ROOT, "tests", "structure_order_check.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-I" + os.path.join(N.ROOT, "include"), "-I" + CSRC, src, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "structure_order_check: ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
