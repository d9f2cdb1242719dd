"""fba_step_stat without a GPU: the header's layout is the one the Python side reads, and the translation unit of its kernel compiles for
gfx950 without scratch memory or spilled registers (the code-object metadata hipcc emits, as test_kernel_resources.py reads it); the size
table of tests/step_stats_size_cases.py straddles every switch-over of the kernel as the sources state it, row_word reaches every member
of a bin once, and the vectorised reference of that module is the per-record loop it replaced."""
import math
import os
import re
import subprocess
import time
import types

import numpy as np
import pytest

import step_stats_size_cases as S
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


# ---- the size table (tests/step_stats_size_cases.py) without a GPU
def test_the_size_cases_straddle_every_switch_over():
    """every family holds a case at or below and a case beyond each of its switch-overs, the thresholds as the sources state them today:
    a changed STEP_STATS_LDS, _BLOCK, _GROUPS or row layout fails here and names the cases to move"""
    k = S.constants()
    assert S.K == k and S.row_words(k["FBA_MAX_ACTIONS"]) * 8 == N.STEP_STAT_DTYPE.itemsize
    assert k["STEP_STATS_ROW_TAIL"] == (N.STEP_STAT_DTYPE.itemsize - N.STEP_STAT_DTYPE.fields["nodes_sum"][1]) // 8
    for family, switches in S.SWITCHES.items():
        cases = [c for c in S.CASES if c["family"] == family]
        assert cases and len({c["A"] for c in cases}) == 1, family
        for sw in switches:
            at, sizes = S.threshold(sw, cases[0]["A"]), sorted(S.measure(sw, c) for c in cases)
            assert any(n <= at for n in sizes) and any(n > at for n in sizes), f"{family}: no case on each side of {sw} = {at}: {sizes}"
            if sw != "TWO_FIT":     # ... and next to it: at the threshold or less than a horizon below it, less than a horizon beyond it
                step = 1 if sw in ("STEP_STATS_BLOCK", "STRIDE") or cases[0]["cfg"].get("episodes", 1) == 1 else max(c["cfg"]["horizon"] for c in cases)
                assert any(at - step < n <= at for n in sizes) and any(at < n <= at + step for n in sizes), f"{family}: {sw} = {at}, cases at {sizes}"
        for c in cases:
            for sw in c["past"]:
                assert S.measure(sw, c) > S.threshold(sw, c["A"]), f"{c['name']} is not beyond {sw}"
            assert switches or c["past"] or family == "fewest_actions", c["name"]
    # the three window counts, the slot counts and the largest and smallest rows are all there
    shapes = {(S.windows(c["n_bins"], c["A"]), S.workgroups(c["slots"])) for c in S.CASES}
    assert {(1, 1), (2, 1), (3, 1), (1, 2), (1, 3), (2, 2), (3, 2), (1, k["STEP_STATS_GROUPS"])} <= shapes, shapes
    assert any(c["slots"] > S.STRIDE for c in S.CASES) and any(c["slots"] == S.STRIDE for c in S.CASES)
    assert min(c["A"] for c in S.CASES) == 2 and max(c["A"] for c in S.CASES) == 16
    assert any(c["A"] >= 16 and S.windows(c["n_bins"], c["A"]) > 1 for c in S.CASES)
    assert any(c["probe"] == "full" and S.windows(c["n_bins"], c["A"]) == 3 for c in S.CASES)
    assert any(c["probe"] not in (None, "full") and S.workgroups(c["slots"]) > 1 and S.windows(c["n_bins"], c["A"]) > 1 for c in S.CASES)
    assert any(c["trace_off"] and S.workgroups(c["slots"]) > 1 and S.windows(c["n_bins"], c["A"]) > 1 for c in S.CASES)
    assert any(c["cfg"].get("search_budget", 0) > 0 and S.workgroups(c["slots"]) > 1 for c in S.CASES)
    for c in S.CASES:       # tiny searches and filters, a run within the trace, a horizon the engine takes
        cfg = c["cfg"]
        assert 4 <= cfg["sims"] <= 8 and cfg["particles"] == S.PARTICLES and cfg["runs"] == c["slots"] and cfg["horizon"] <= 255, c["name"]
        assert c["slots"] * c["n_bins"] < S.TRACE_CAP and c["n_bins"] == cfg.get("episodes", 1) * cfg["horizon"], c["name"]
        assert c["slots"] * min(c["n_bins"], 4 if c["ends"] else c["n_bins"]) * N.TRACE_DTYPE.itemsize < 300e6 or not c["ends"], c["name"]


def test_row_word_reaches_every_member_once():
    """row_word of fba_step_stats.hip restated: for every A the words 0 .. row_words(A) - 1 of an LDS row are distinct words of
    fba_step_stat, and together they are steps, terminals, action[:A], root_visits[:A] and every member from nodes_sum on"""
    dt, MAX = N.STEP_STAT_DTYPE, S.K["FBA_MAX_ACTIONS"]
    src = open(os.path.join(N.HERE, "csrc", "fba_step_stats.hip")).read()
    assert re.search(r"if \(c < 2 \+ A\) return c;\s*if \(c < 2 \+ 2 \* A\) return W_VISITS \+ \(c - 2 - A\);\s*return W_NODES \+ \(c - 2 - 2 \* A\);", src)
    assert re.search(r"W_ACTION = 2, W_VISITS = W_ACTION \+ FBA_MAX_ACTIONS, W_NODES = W_VISITS \+ FBA_MAX_ACTIONS", src)
    W_VISITS, W_NODES = 2 + MAX, 2 + 2 * MAX
    assert (dt.fields["action"][1], dt.fields["root_visits"][1], dt.fields["nodes_sum"][1]) == (16, W_VISITS * 8, W_NODES * 8)

    def row_word(c, A):
        if c < 2 + A:
            return c
        if c < 2 + 2 * A:
            return W_VISITS + (c - 2 - A)
        return W_NODES + (c - 2 - 2 * A)
    for A in range(1, MAX + 1):
        words = [row_word(c, A) for c in range(S.row_words(A))]
        want = {dt.fields["steps"][1], dt.fields["terminals"][1]}
        want |= {dt.fields[m][1] + 8 * a for m in ("action", "root_visits") for a in range(A)}
        want |= set(range(dt.fields["nodes_sum"][1], dt.itemsize, 8))
        assert len(set(words)) == len(words) == len(want) and {8 * w for w in words} == want, A
        # (every 8-byte member behind root_visits starts a word; the four int32 of the maxima share two)
        assert {dt.fields[m][1] // 8 * 8 for m in MEMBERS[MEMBERS.index("nodes_sum"):]} == set(range(W_NODES * 8, dt.itemsize, 8))


def _loop_ref(E, H, tr):
    """the reference as tests/test_gpu_step_stats.py first had it: one pass over the records"""
    ints = np.zeros((E, H), N.STEP_STAT_DTYPE)
    terms = {f: [[[] for _ in range(H)] for _ in range(E)] for f in S.DOUBLES}
    b = ints
    for r in tr:
        k = (int(r["episode"]), int(r["t"]))
        a, q, rew = int(r["action"]), float(r["root_q"][int(r["action"])]), float(r["reward"])
        b["steps"][k] += 1
        b["terminals"][k] += int(r["terminal"] != 0)
        b["action"][k][a] += 1
        b["root_visits"][k] += r["root_n"].astype(np.uint64)
        b["nodes_sum"][k] += int(r["n_nodes"])
        b["depth_sum"][k] += int(r["tree_depth"])
        b["nodes_max"][k] = max(b["nodes_max"][k], r["n_nodes"])
        b["depth_max"][k] = max(b["depth_max"][k], r["tree_depth"])
        if not r["terminal"] and r["update_count"] >= 0:
            b["attempts_steps"][k] += 1
            b["attempts_sum"][k] += int(r["update_count"])
            b["attempts_max"][k] = max(b["attempts_max"][k], r["update_count"])
        for f, v in (("reward_sum", rew), ("reward_sq_sum", rew * rew), ("value_sum", q), ("value_sq_sum", q * q)):
            terms[f][k[0]][k[1]].append(v)
    return ints, terms


def test_the_vectorised_reference_equals_the_loop():
    """a synthetic trace with ties in the three maxima, empty bins, terminal records whose update_count is stale and records without an
    update: the aggregation by np.add.at / np.maximum.at and a sort by bin gives what one pass over the records gave"""
    rng = np.random.default_rng(77)
    E, H, n = 5, 4, 600
    tr = np.zeros(n, N.TRACE_DTYPE)
    tr["episode"] = rng.choice([0, 1, 3, 4], n)         # (episode 2 has no record)
    tr["t"] = rng.choice([0, 1, 3], n)                  # (nor has t = 2)
    tr["run"] = np.arange(n)
    tr["action"] = rng.integers(0, N.MAX_ACTIONS, n)
    tr["terminal"] = rng.integers(0, 2, n) * rng.integers(1, 3, n)
    tr["n_nodes"] = rng.integers(1, 4, n)               # (few values: every bin's maximum is held by many records)
    tr["tree_depth"] = rng.integers(0, 3, n)
    tr["update_count"] = rng.choice([-1, 0, 5, 9, 9], n)
    tr["root_n"] = rng.integers(0, 7, (n, N.MAX_ACTIONS))
    tr["root_q"] = rng.normal(0, 30, (n, N.MAX_ACTIONS))
    tr["reward"] = rng.choice([-100.0, -1.0, -0.5, 10.0], n)
    eng = types.SimpleNamespace(cfg=types.SimpleNamespace(episodes=E, horizon=H))
    ref = S.Ref(eng, tr)
    ints, terms = _loop_ref(E, H, tr)
    assert ref.ints.tobytes() == ints.tobytes()
    assert not np.any(ints["steps"][2]) and not np.any(ints["steps"][:, 2]) and np.all(ints["steps"][[0, 1, 3, 4]][:, [0, 1, 3]] > 5)
    assert np.any((tr["terminal"] != 0) & (tr["update_count"] > int(ints["attempts_max"].max()) - 1))      # a stale count that must not be read
    for f in S.DOUBLES:
        for e in range(E):
            for t in range(H):
                x = terms[f][e][t]
                assert ref.terms[f][e][t].tolist() == x and ref.count[e, t] == len(x)
                assert ref.sums[f][e, t] == math.fsum(x) and ref.mags[f][e, t] == math.fsum(abs(v) for v in x)
                assert ref.bound(f)[e, t] == len(x) * 2.0 ** -52 * math.fsum(abs(v) for v in x)
    st = ref.ints.copy()
    for f in S.DOUBLES:
        st[f] = ref.sums[f]
    assert ref.check(st, "synthetic") == 0.0
    # ... and it bites: one count, one maximum, one ulp of a reward sum, a value sum beyond its bound
    for f, d in (("steps", 1), ("nodes_max", -1), ("attempts_max", 1)):
        bad = st.copy()
        bad[f][4, 3] += d
        with pytest.raises(AssertionError, match=f):
            ref.check(bad, "synthetic")
    bad = st.copy()
    bad["reward_sum"][0, 1] = np.nextafter(bad["reward_sum"][0, 1], np.inf)
    with pytest.raises(AssertionError, match="reward_sum"):
        ref.check(bad, "synthetic")
    bad = st.copy()
    bad["value_sum"][3, 0] += 1.5 * ref.bound("value_sum")[3, 0]
    with pytest.raises(AssertionError, match="value_sum"):
        ref.check(bad, "synthetic")
    bad["value_sum"][3, 0] = st["value_sum"][3, 0] + 0.5 * ref.bound("value_sum")[3, 0]
    assert 0.4 < ref.check(bad, "synthetic") < 0.6


def test_the_reference_aggregates_the_widest_case_in_seconds():
    """as many records as the 131 073-slot case writes, aggregated within a few seconds"""
    n = (S.STRIDE + 1) * 3
    rng = np.random.default_rng(5)
    tr = np.zeros(n, N.TRACE_DTYPE)
    tr["episode"], tr["t"] = rng.integers(0, 2, n), rng.integers(0, 2, n)
    tr["action"] = rng.integers(0, 3, n)
    tr["n_nodes"] = rng.integers(1, 4, n)
    tr["root_q"] = rng.normal(0, 30, (n, N.MAX_ACTIONS))
    t0 = time.time()
    ref = S.Ref(types.SimpleNamespace(cfg=types.SimpleNamespace(episodes=2, horizon=2)), tr)
    took = time.time() - t0
    print(f"{n} records aggregated in {took:.2f} s")
    assert int(ref.ints["steps"].sum()) == n and took < 10.0
