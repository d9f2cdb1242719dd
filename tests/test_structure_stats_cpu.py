"""fba_structure_stats without a GPU: the header's fba_structure_stat is the numpy dtype field by field, the new symbols are declared,
exported and bound, the new translation unit compiles for gfx950 without scratch memory or spilled registers and leaves two workgroups
room on a CU (the code-object metadata, as test_structures_abi.py reads it), the size table of tests/structure_stats_cases.py straddles
every switch-over of the reduction as fba_kernels.h states it, and the host-side reference sums a hand-made example as the header
defines the bins."""
import os
import re
import subprocess

import numpy as np

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N
import structure_stats_cases as SS

MEMBERS = ["steps", "weightless", "overflowed", "collapsed", "distinct_sum", "distinct_max", "reserved"]
CSRC = os.path.join(N.HERE, "csrc")


def _header():
    return open(os.path.join(N.ROOT, "include", "fba_hip.h")).read()


def test_the_header_and_the_dtype_agree(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    lines = "".join(f'    printf("{m} %zu\\n", offsetof(fba_structure_stat, {m}));\n' for m in MEMBERS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fba_hip.h"\nint main(void)\n{\n'
                   '    printf("sizeof %zu\\n", sizeof(fba_structure_stat));\n' + lines + "    return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(N.ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    dt = N.STRUCTURE_STAT_DTYPE
    assert int(got.pop("sizeof")) == dt.itemsize == 48
    assert list(dt.names) == MEMBERS
    assert {m: int(v) for m, v in got.items()} == {m: dt.fields[m][1] for m in MEMBERS}
    assert all(dt.fields[m][1] % 8 == 0 for m in MEMBERS if m != "reserved")
    # ... and against the header's text: five uint64_t, then two int32_t
    body = re.search(r"typedef struct fba_structure_stat \{(.*?)\} fba_structure_stat;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n.strip()) for t, names in re.findall(r"^\s*(uint64_t|int32_t)\s+([\w, ]+);", body, re.M) for n in names.split(",")]
    assert [n for _, n in fields] == MEMBERS and [t for t, _ in fields] == ["uint64_t"] * 5 + ["int32_t"] * 2
    off = 0
    for t, n in fields:
        size = 8 if t == "uint64_t" else 4
        assert (dt.fields[n][1], dt.fields[n][0].itemsize) == (off, size), n
        off += size


def test_the_symbols_are_declared_exported_and_bound():
    h = _header()
    assert re.search(r"#define FBA_ABI_VERSION 3\b", h)
    assert int(re.search(r"#define FBA_STRUCT_STATS_MAX_QUERIES (\d+)", h).group(1)) == N.STRUCT_STATS_MAX_QUERIES == 16
    assert re.search(r"int fba_structure_stats_enable\(fba_ctx\* ctx, int32_t on, int32_t nq, const uint32_t\* query", h)
    decl = re.search(r"int fba_get_structure_stats\((.*?)\);", h, re.S).group(1)
    args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert args == ["fba_ctx* ctx", "int32_t cap_bins", "fba_structure_stat* head", "double* set_frac", "double* query_frac", "uint64_t* query_held",
                    "uint64_t* query_sole"]
    fba.build()
    lib = fba.load()
    for name in ("fba_structure_stats_enable", "fba_get_structure_stats"):
        assert name in N.EXPORTS and hasattr(lib, name), name
    assert len(lib.fba_get_structure_stats.argtypes) == len(args) and len(lib.fba_structure_stats_enable.argtypes) == 4
    assert lib.fba_abi_version() == 3
    assert os.path.join(CSRC, "fba_structure_stats.hip") in N.SOURCES
    assert os.path.join(CSRC, "fba_structures_table.h") in N.HEADERS
    assert hasattr(fba.Engine, "structure_stats_enable") and hasattr(fba.Engine, "structure_stats")
    # one definition of what the two kernels agree on: both include the header, neither restates it
    for unit in ("fba_structures.hip", "fba_structure_stats.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        assert '#include "fba_structures_table.h"' in text and "struct_table_rounds<STRUCT_TABLE>(" in text, unit
        assert "atomicCAS" not in text and "uint32_t record_key_word(" not in text, unit


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "fba_hip.h"\n'
                   "_Static_assert(sizeof(fba_structure_stat) == 48, \"fba_structure_stat\");\n"
                   "int use(fba_ctx* c, fba_structure_stat* h, const uint32_t* q) { if (fba_structure_stats_enable(c, 1, FBA_STRUCT_STATS_MAX_QUERIES, q)) return -1;\n"
                   "    return fba_get_structure_stats(c, 1, h, 0, 0, 0, 0); }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(N.ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_the_kernels_use_no_scratch_and_share_a_cu(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "fba_structure_stats.s"
    subprocess.check_call(["hipcc"] + flags + ["-I" + os.path.join(N.ROOT, "include"), "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(CSRC, "fba_structure_stats.hip")], stderr=subprocess.DEVNULL)
    meta = out.read_text()
    meta = meta[meta.index("amdhsa.kernels:"):]
    seen = {}
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        seen[name] = (get("private_segment_fixed_size"), get("vgpr_count"), get("vgpr_spill_count"), get("sgpr_spill_count"), get("group_segment_fixed_size"))
    assert len(seen) == 2, sorted(seen)
    slot = next(v for k, v in seen.items() if "struct_stats_slot_kernel" in k)
    bins = next(v for k, v in seen.items() if "struct_stats_bins_kernel" in k)
    for scratch, _, vspills, _, _ in (slot, bins):      # (as test_kernel_resources.py counts: no scratch memory, no spilled vector register;
        assert scratch == 0 and vspills == 0, seen      #  a scalar register parked in a vector register's lane touches no memory)
    assert bins[3] == 0, seen
    c = SS.constants()
    assert 2 * slot[4] <= 160 * 1024 and slot[4] <= 64 * 1024, seen      # stage one: static LDS only, two workgroups (and more) to a CU
    assert slot[4] >= N.STRUCT_TABLE * 12 + 1024 * 8      # ... the table's hashes and representatives and the histogram cells are in it
    assert bins[4] == 0 and c["LDS_WORDS"] * 8 <= 64 * 1024      # stage two: the window is dynamic LDS, sized by the launcher
    assert bins[1] <= 128, seen      # 1 024 threads: sixteen waves on a CU, four per SIMD


def test_the_size_cases_straddle_every_switch_over():
    """the thresholds as fba_kernels.h states them today: a changed constant fails here and names the cases to move"""
    c = SS.constants()
    assert (c["BIN_HEAD"] * 8, c["SLOT_HEAD"]) == (N.STRUCTURE_STAT_DTYPE.itemsize, 2)
    assert (c["GROUP_SLOTS"], c["CHUNK_SLOTS"], c["COLS"], c["LDS_WORDS"]) == (256, 32768, 96, 7680)
    text = open(os.path.join(CSRC, "fba_kernels.h")).read()
    assert "return STRUCT_STATS_BIN_HEAD + n_words * n_sets + 3 * nq;" in text
    assert "return row_words < STRUCT_STATS_COLS ? row_words : STRUCT_STATS_COLS;" in text
    assert "const int fit = STRUCT_STATS_LDS_WORDS / cols; return n_bins < fit ? n_bins : fit;" in text
    kernel = open(os.path.join(CSRC, "fba_structure_stats.hip")).read()
    assert "dim3(ceil_div(a.count, STRUCT_STATS_GROUP_SLOTS))" in kernel and "dim3(a.count), dim3(STRUCT_STATS_BLOCK)" in kernel
    assert set(SS.SIZE_CASES) == set(SS.SIZE_PLANS)
    plans = {}
    for name, (slots, episodes, horizon, nq, ticks) in SS.SIZE_CASES.items():
        plans[name] = SS.plan(slots, episodes * horizon, SS.GW_WORDS, SS.GW_SETS, nq, c)
        assert plans[name] == SS.SIZE_PLANS[name], name
        assert 0 < nq <= N.STRUCT_STATS_MAX_QUERIES and ticks <= 90, name
    size = {name: (v[0], v[1] * v[2], SS.row_words(SS.GW_WORDS, SS.GW_SETS, v[3], c)) for name, v in SS.SIZE_CASES.items()}
    # a case at each threshold and a case one step beyond it
    assert size["slots_one_workgroup"][0] == c["GROUP_SLOTS"] and size["slots_two_workgroups"][0] == c["GROUP_SLOTS"] + 1
    assert size["slots_one_chunk"][0] == c["CHUNK_SLOTS"] and size["slots_two_chunks"][0] == c["CHUNK_SLOTS"] + 1
    assert size["row_one_window"][2] <= c["COLS"] < size["row_two_windows"][2] == size["row_one_window"][2] + 3      # (a query is three words)
    fit = c["LDS_WORDS"] // c["COLS"]
    assert size["bins_one_window"][1] == fit and size["bins_two_windows"][1] == fit + 1 and size["bins_second_window_used"][1] > fit + 1
    # the row bound of a chunk is out of the built-in models' reach: the gridworld's row takes 64 MB only beyond CHUNK_SLOTS slots
    assert c["ROWS_BYTES"] // ((c["SLOT_HEAD"] + size["row_two_windows"][2] - c["BIN_HEAD"]) * 8) > c["CHUNK_SLOTS"]
    # 150 ragged slots: fewer than a workgroup's share, more than one wave
    assert 64 < size["ragged_150_slots"][0] < c["GROUP_SLOTS"]


def test_the_reference_sums_a_hand_made_example():
    """three steps in two bins: a weighted filter, a weightless one, an overflowed one"""
    sm = np.array([[1.0, 3.0], [4.0, 0.0]])
    vals = {
        (0, 0, 0): SS.step_value(4.0, sm, [1.0, 0.0], 2, 0, [1, 0], 4),
        (1, 0, 0): SS.step_value(0.0, 0 * sm, [0.0, 0.0], 1, 0, [4, 0], 4),
        (2, 1, 1): SS.step_value(8.0, 2 * sm, [0.0, 8.0], 2048, 1, [0, 3], 4),
        (7, 1, 1): SS.step_value(2.0, sm / 2, [2.0, 0.0], 1, 0, [4, 0], 4),
    }
    head, sf, qf, qh, qs = SS.bins_of(vals, 2, 2, 2, 2, 2)
    assert head["steps"].tolist() == [[2, 0], [0, 2]] and head["weightless"].tolist() == [[1, 0], [0, 0]]
    assert head["overflowed"].tolist() == [[0, 0], [0, 1]] and head["collapsed"].tolist() == [[1, 0], [0, 1]]
    assert head["distinct_sum"].tolist() == [[3, 0], [0, 2049]] and head["distinct_max"].tolist() == [[2, 0], [0, 2048]]
    assert sf[0, 0].tolist() == [[0.25, 0.75], [1.0, 0.0]] and sf[1, 1].tolist() == [[0.5, 1.5], [2.0, 0.0]] and not np.any(sf[0, 1]) and not np.any(sf[1, 0])
    assert qf[0, 0].tolist() == [0.25, 0.0] and qf[1, 1].tolist() == [1.0, 1.0]
    assert qh[0, 0].tolist() == [2, 0] and qh[1, 1].tolist() == [1, 1] and qs[0, 0].tolist() == [1, 0] and qs[1, 1].tolist() == [1, 0]
    # keep: the runs of an experiment
    head2 = SS.bins_of(vals, 2, 2, 2, 2, 2, keep=lambda key: key[0] < 3)[0]
    assert head2["steps"].tolist() == [[2, 0], [0, 1]]
    # compare() holds a device answer to it: equal passes, one count or one part in 2^40 off does not
    dev = fba.engine.StructureStats(head.copy(), sf.copy(), qf.copy(), qh.copy(), qs.copy())
    SS.compare(dev, (head, sf, qf, qh, qs), 4, "hand-made", exact=True)
    for spoil in ("steps", "set_frac", "query_held", "zero"):
        bad = fba.engine.StructureStats(head.copy(), sf.copy(), qf.copy(), qh.copy(), qs.copy())
        if spoil == "steps":
            bad.head["steps"][0, 0] += 1
        elif spoil == "set_frac":
            bad.set_frac[0, 0, 0, 0] *= 1 + 2.0 ** -40
        elif spoil == "query_held":
            bad.query_held[1, 1, 0] += 1
        else:
            bad.set_frac[0, 0, 1, 1] = 1e-300
        try:
            SS.compare(bad, (head, sf, qf, qh, qs), 4, "hand-made, spoilt " + spoil)
        except AssertionError:
            continue
        raise AssertionError("compare() passed a spoilt answer: " + spoil)
