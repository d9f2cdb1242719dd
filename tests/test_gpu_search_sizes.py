"""Engine == oracle on both sides of every tree size at which the search changes.  The engine chooses its search kernel, its tree layout
and several packed bit-fields from sims, max_depth, A * O and the number of searches a slot has made (tests/search_size_cases.py: the table
of switch-overs), and nearly every other oracle comparison of the suite searches 8 to 300 simulations: a `<` for a `<=` at one of these
switches, a 12-, 15- or 16-bit field one bit too narrow, or a hash table that keeps stale entries over an epoch wrap would pass them all.
tests/test_launch_plan_cpu.py pins which kernel search_plan names on each side; here both sides run.  A small whole experiment runs at c
and at c + 1 of every switch (or at the nearest sizes real domains have), and every trace field -- n_nodes, tree_depth, root_n, root_q and
the belief hash among them --, statistic, counter and per-run return must be the oracle's, bit for bit.  Before anything runs,
Engine.device_arrays() is compared with the tree geometry the case states, which proves on which side it stands; and the oracle's trace
must show that the case loads the field its limit protects (search_size_cases.CONDITIONS).  The tests without a GPU keep the table honest:
the thresholds are read out of the sources, so a moved threshold fails the table instead of leaving it beside the switch.

Measured on the oracle (Philox, device arithmetic, 32 particles; deterministic, so these are what the conditions see):
    ETIGER by sims: `listen` gets 58 658 | 58 674 of 65 535 | 65 536 visits at some root (planning; 58 176 | 46 145 packed, 58 620 | 58 719
        dense tabular), trees of 124 to 127 of 129 nodes at depth 6
    ETIGER by node bound: 58 | 71 nodes at 4091 | 4092 simulations; 245 | 243 nodes at depth 8 of 2049 | 4097 records at max_depth 10 | 11
    int16 root children: n_nodes 32 766 | 32 767 at 32 765 | 32 766 simulations (exploration 1e5)
    bucket tree | records: 35 262 to 35 661 nodes at 65 536 | 65 537 simulations (exploration 1000, horizon 4; 13 000 at horizon 3)
    wide hash at its natural size: 28 597 | 27 984 nodes at 68 476 | 68 477 simulations
    epoch wipes: 86 and 110 (factored), 96 and 121 (tabular) records in 3 slots against 3 * 18; 255, 317 and 301 (planning) and 106
        (search_hist_kernel) records in 3 slots against 3 * 34"""
import functools
import os
import re

import pytest

import search_size_cases as S
import fba_pomdp_amd as fba
import wide_launch_cases as W

CSRC = os.path.join(os.path.dirname(os.path.abspath(fba.__file__)), "csrc")


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """the oracle's side of a case, computed once and shared (a one-slot twin is compared with its many-slot case's run)"""
    return W.oracle_side(S.BY_NAME[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in S.CASES])
def test_search_size_equals_the_oracle(name, monkeypatch):
    c = S.BY_NAME[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    ref = _oracle(S.oracle_case(c)["name"])
    print(f"{name}: {S.assert_conditions(c, ref['trace'])}")

    def check(eng):
        assert (eng.A, eng.O) == (c["geom"]["A"], c["geom"]["O"])
        S.assert_geometry(c, eng.device_arrays())

    W.assert_same_experiment(c, W.engine_side(c, fba, check), ref)


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(text, head):
    """the braces' content of the function whose head matches"""
    m = re.search(head + r"[^{;]*\{", text)
    assert m, head
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def _constants():
    """the thresholds as the sources state them"""
    plan, header, engine = _read("fba_launch_plan.h"), _read("fba_kernels.h"), _read("fba_engine.hip")
    search, hist2, common = _read("fba_search.hip"), _read("fba_search_hist2.inc"), _read("fba_kernels_common.h")
    k = {}
    et = _body(plan, r"inline bool etiger_ok\(")
    k["ETIGER_SIMS"] = int(_one(r"P\.sims <= (\d+)", et))
    k["ETIGER_NODES"] = int(_one(r"D\.max_nodes <= (\d+)", et))
    rc = _body(plan, r"bool root_children_in_lds\(")
    assert re.search(r"P\.A \* P\.O <= ROOT_CHILDREN\b", rc)
    k["ROOT_CHILDREN_NODES"] = int(_one(r"D\.max_nodes <= (\d+)", rc))
    k["ROOT_CHILDREN_AO"] = int(_one(r"constexpr\s+int\s+ROOT_CHILDREN\s*=\s*(\d+)\s*;", header))
    k["STAGE_WORDS"] = int(_one(r"constexpr\s+int\s+SEARCH_STAGE_WORDS\s*=\s*(\d+)\s*;", header))
    sp = _body(plan, r"inline SearchPlan search_plan\(")
    assert re.search(r"const bool stage = P\.model != FBA_MODEL_POMDP && P\.Cs <= SEARCH_STAGE_WORDS;", sp)
    k["AMAX"] = tuple(int(v) for v in _one(r"amax\s*=\s*P\.A <= (\d+) \? \1 : \(P\.A <= (\d+) \? \2 : \(P\.A <= (\d+) \? \3 : 24\)\)", sp))
    # the bucket-tree searches' LDS: the waves of a workgroup, its limit, a wave's bytes
    k["H2_WAVES"] = int(_one(r"constexpr\s+int\s+H2_WAVES\s*=\s*(\d+)\s*;", plan))
    assert re.search(r"while \(nw > 1 && shared \+ \(size_t\)nw \* h2_wave_bytes\(P\) > 64 \* 1024\) nw >>= 1;", sp)
    assert re.search(r"pl\.raise_lds = pl\.lds > 64 \* 1024 \?", sp)
    assert re.search(r"const size_t shared = tab \? 0 :", sp)
    # (a wave's bytes: W.h2_waves against what the launchers were recorded to launch, _recorded_geometries below)
    assert re.search(r"tree_k = \(blockIdx\.x \* \(int\)\(blockDim\.x >> 6\) \+ wave\) \* HIST_TREES \+ tl;", hist2)     # (DEEP_E: which wave holds tree k)
    # plan_tree and bucket_tree_search
    pt = _body(engine, r"int plan_tree\(")
    k["HASHED_AO"] = int(_one(r"t\.hashed = P\.A \* P\.O > (\d+);", pt))
    k["HASH_COMPACT"] = 1 << int(_one(r"D\.max_nodes \* P\.A \* P\.O < \(1ull << (\d+)\) && !sw\.wide_hash", pt))
    assert re.search(r"D\.max_nodes\s*=\s*P\.sims \+ 2;", pt)
    assert re.search(r"D\.max_nodes = std::min\(D\.max_nodes, \(1 << \(P\.max_depth \+ 1\)\) \+ 1\);", pt)
    assert re.search(r"while \(t\.hcap < 2u \* \(uint32_t\)\(D\.max_nodes - 2\)\) t\.hcap <<= 1;", pt)
    assert re.search(r's\.wide_hash\s*=\s*std::getenv\("FBA_WIDE_HASH"\) != nullptr;', engine)
    assert re.search(r's\.tree_records\s*=\s*says\(std::getenv\("FBA_HIST_TREE"\), "records"\);', engine)
    sims = {int(_one(r"cfg\.sims <= (\d+)", _body(engine, r"bool bucket_tree_search\("))),
            int(_one(r"bucket_records && P\.sims <= (\d+)", pt)),
            int(_one(r"const bool spec = carry && D\.max_nodes <= \d+ && P\.sims <= (\d+);", search))}
    assert len(sims) == 1, sims
    (k["BUCKET_SIMS"],) = sims
    assert int(_one(r"const bool spec = carry && D\.max_nodes <= (\d+) && P\.sims <= \d+;", search)) == k["BUCKET_SIMS"] + 2
    # the epochs
    k["BUCKET_EPOCH"] = int(_one(r"if \(epoch > (\d+)u\)", hist2))
    k["HASH_EPOCH"] = int(_one(r"if \(epoch > (\d+)u\)", _body(common, r"uint32_t hash_begin_search\(")))
    return k


def _recorded_geometries():
    """(max_depth, Cs) -> (waves per workgroup, LDS bytes, limit raised) of search_tabhist_kernel as tests/golden/launch_plan_expected.jsonl
    records the launchers (tests/test_launch_plan_cpu.py holds this tree's launchers to that record)"""
    import launch_plan_cases as T
    want, out = T.expected(), {}
    for c in T.CASES:
        m = re.fullmatch(r"search_grid_tab_bucket_importance_depth(\d+)", c["name"])
        if m:
            calls = want[c["name"]]["s"]
            (launch,) = [call for call in calls if call[0] == "L" and call[1].startswith("search_tabhist_kernel")]
            out[int(m.group(1)), c["fields"]["P_Cs"]] = (launch[5] // 64, launch[8], any(call[0] == "A" for call in calls))
    return out


def _values(family, key):
    return sorted({c["kw"][key] for c in S.of_family(family)})


def _both_sides(family, values, c, sw):
    assert c in values and c + 1 in values, f"{family}: no case at {c} and {c + 1}, the two sides of {sw}: {values}"


def test_search_size_cases_straddle_every_switch_over():
    """every family of cases holds c and c + 1 of every switch-over that its search has, c as the sources state it today -- or the nearest
    sizes on each side that a real domain has, as the table says"""
    k = _constants()
    assert (S.BUCKET_WRAP, S.HASH_WRAP) == (k["BUCKET_EPOCH"], k["HASH_EPOCH"])
    for family, switches in S.SWITCHES.items():
        cases = S.of_family(family)
        for sw in switches:
            if sw in ("ETIGER_SIMS", "BUCKET_SIMS"):
                _both_sides(family, _values(family, "sims"), k[sw], sw)
                if sw == "ETIGER_SIMS":      # (and the node bound does not decide there)
                    assert all(c["geom"]["max_nodes"] <= k["ETIGER_NODES"] and "episodic" in c["domain"] for c in cases)
            elif sw in ("ETIGER_NODES", "ROOT_CHILDREN_NODES"):       # max_nodes = sims + 2 where nothing else bounds the tree
                by_sims = [c for c in cases if c["geom"]["max_nodes"] == c["kw"]["sims"] + 2]
                _both_sides(family, sorted(c["geom"]["max_nodes"] for c in by_sims), k[sw], sw)
                if sw == "ETIGER_NODES":
                    assert all("episodic" in c["domain"] and (1 << c["kw"]["max_depth"] + 1) + 1 > k[sw] + 1 and
                               c["kw"]["sims"] <= k["ETIGER_SIMS"] for c in by_sims)
                else:
                    assert all("continuous" in c["domain"] and c["geom"]["A"] * c["geom"]["O"] <= k["ROOT_CHILDREN_AO"] for c in cases)
            elif sw == "ETIGER_DEPTH":       # one large sims, the episodic bound 2^(max_depth + 1) + 1 on each side of the node limit
                by_depth = [c for c in cases if c["geom"]["max_nodes"] == (1 << c["kw"]["max_depth"] + 1) + 1 < c["kw"]["sims"] + 2]
                assert len({c["kw"]["sims"] for c in by_depth}) == 1 and by_depth[0]["kw"]["sims"] <= k["ETIGER_SIMS"]
                depths = sorted(c["kw"]["max_depth"] for c in by_depth)
                assert len(depths) == 2 and depths[1] == depths[0] + 1, depths
                assert (1 << depths[0] + 1) + 1 <= k["ETIGER_NODES"] < (1 << depths[1] + 1) + 1
            elif sw == "ROOT_CHILDREN_AO":
                ao = sorted(c["geom"]["A"] * c["geom"]["O"] for c in cases)
                assert k[sw] in ao and min(v for v in ao if v > k[sw]) <= k[sw] * 3 // 2, (family, ao)
                assert all(c["geom"]["max_nodes"] <= k["ROOT_CHILDREN_NODES"] for c in cases)
            elif sw == "AMAX":               # A at every rung, and the next A a domain of this family has above each rung but the last
                a = sorted(c["geom"]["A"] for c in cases)
                assert all(rung in a for rung in k[sw]), (family, a)
                assert all(any(lo < v <= hi for v in a) for lo, hi in zip(k[sw], k[sw][1:])), (family, a)
            elif sw == "STAGE_WORDS":        # the nearest record sizes that the tabular model has: Cs of 2^n * 2n * (2^n + 2) counts and a state
                words = sorted(W.dense_bytes((1 << c["kw"]["size"]) * c["geom"]["A"] * ((1 << c["kw"]["size"]) + c["geom"]["O"])) // 4 for c in cases)
                assert len(words) == 2 and words[0] <= k[sw] < words[1], (family, words)
                assert sorted(c["kw"]["size"] for c in cases) == [2, 3]
            elif sw == "HASHED_AO":          # no domain at 64 | 65: two below, and above an odd and an even number of actions
                ao = [(c["geom"]["A"], c["geom"]["A"] * c["geom"]["O"], c["geom"]["hash_entry"]) for c in cases]
                assert sum(1 for a, v, h in ao if v <= k[sw] and not h) >= 2, ao
                assert any(v > k[sw] and h and a % 2 for a, v, h in ao) and any(v > k[sw] and h and a % 2 == 0 for a, v, h in ao), ao
            elif sw == "HASH_COMPACT":       # max_nodes * A * O on each side of 2^27, one simulation apart
                natural = sorted((c["geom"]["max_nodes"] * c["geom"]["A"] * c["geom"]["O"], c["geom"]["max_nodes"], c["geom"]["hash_entry"])
                                 for c in cases if not c["env"])
                below, above = [v for v in natural if v[0] < k[sw]][-1], [v for v in natural if v[0] >= k[sw]][0]
                assert above[1] == below[1] + 1 and (below[2], above[2]) == (8, 16), natural
            elif sw == "WIDE_HASH_ENV":      # one small tree on 16-byte entries next to its 8-byte twin
                wide = [c for c in cases if c["env"] == S.WIDE_ENV]
                assert len(wide) == 1 and wide[0]["geom"]["hash_entry"] == 16
                twin = [c for c in cases if not c["env"] and c["geom"]["max_nodes"] == wide[0]["geom"]["max_nodes"]]
                assert len(twin) == 1 and twin[0]["geom"]["hash_entry"] == 8
                assert wide[0]["geom"]["max_nodes"] * wide[0]["geom"]["A"] * wide[0]["geom"]["O"] < k["HASH_COMPACT"]
            elif sw in ("BUCKET_EPOCH", "HASH_EPOCH"):
                many = [c for c in cases if not c["oracle_of"]]
                assert all((c["geom"]["bkt_lines"] > 0) == (sw == "BUCKET_EPOCH") and c["runs"] > c["E"] for c in many)
                assert all(c["geom"]["hash_entry"] == 8 for c in many if sw == "HASH_EPOCH")          # (the 5-bit epoch: compact entries only)
                for c in cases:
                    if c["oracle_of"]:       # one slot makes every search of the twin's experiment in order
                        o = S.oracle_case(c)
                        assert c["E"] == 1 and (c["runs"], c["kw"], c["env"], c["geom"]) == (o["runs"], o["kw"], o["env"], o["geom"])
            elif sw == "H2_WAVES":           # max_depth on each side of each halving and of the 64 KB limit, from W.h2_waves
                assert k[sw] == 4
                recorded = _recorded_geometries()       # W.h2_waves is what the launchers do: at both sides of every edge they recorded
                assert {d for d, _ in recorded} >= {34, 35, 71, 72, 144, 145}
                for (d, cs), (nw, lds, raised) in recorded.items():
                    assert W.h2_waves(d, cs) == (nw, raised) and nw * W.h2_wave_bytes_at(d, cs) == lds, (d, cs)
                depths, want = _values(family, "max_depth"), []
                geo = {d: W.h2_waves(d, S.DEEP_CS) for d in range(1, 400)}
                for d in range(1, 399):
                    if geo[d] != geo[d + 1]:
                        want += [d, d + 1]
                assert len(want) == 6 and [geo[d] for d in want] == [(4, False), (2, False), (2, False), (1, False), (1, False), (1, True)]
                assert depths == want, (depths, want)
                assert all(c["model"] == W.TABLE and c["fmt"] == "history" and c["geom"]["bkt_lines"] for c in cases)     # (shared = 0)
                assert all(W.record_bytes(c["kw"]["episodes"], c["kw"]["horizon"]) == 4 * S.DEEP_CS for c in cases)
                assert all(c["E"] > 16 * (k[sw] - 1) for c in cases)       # (a tree in the last wave of the widest workgroup)
            elif sw == "H2_WAVES_SHARED":    # the factored searches: shared tables of 0 .. SHARED_MOST bytes in front of the waves' areas; the
                # nearest depths on each side of each halving at which the geometry is the same for every such size
                sure = {d: W.h2_waves(d, S.DEEP_CS) for d in range(1, 400)
                        if W.h2_waves(d, S.DEEP_CS) == W.h2_waves(d, S.DEEP_CS, shared=S.SHARED_MOST)}
                want, ds = [], sorted(sure)
                for lo, hi in zip(ds, ds[1:]):
                    if sure[lo] != sure[hi]:
                        want += [lo, hi]
                assert [sure[d] for d in want] == [(4, False), (2, False), (2, False), (1, False), (1, False), (1, True)]
                assert _values(family, "max_depth") == want == list(S.DEEP_FACTORED), (family, want)
                assert all(c["model"] == W.FACT and c["fmt"] == "history" and c["geom"]["bkt_lines"] and c["kw"]["size"] == 3 for c in cases)
                assert all(W.record_bytes(c["kw"]["episodes"], c["kw"]["horizon"]) == 4 * S.DEEP_CS and c["E"] > 16 * 3 for c in cases)
            else:
                raise AssertionError(sw)
    # what fba_create makes on each side of BUCKET_SIMS, as the cases expect it
    top = k["BUCKET_SIMS"]
    made = {(c["family"], c["kw"]["sims"]): (c["fmt"], c["geom"]["bkt_lines"], c["geom"]["hash_entry"]) for c in S.CASES}
    assert (made["bucket_sims_importance", top], made["bucket_sims_importance", top + 1]) == (("history", top + 2, 0), ("history", 0, 8))
    assert (made["bucket_sims_rejection", top], made["bucket_sims_rejection", top + 1]) == (("history", top + 2, 0), ("dense", 0, 8))
    assert (made["bucket_sims_table", top], made["bucket_sims_table", top + 1]) == (("history", top + 2, 0), ("dense", 0, 8))
    assert (made["records_sims_importance", top], made["records_sims_importance", top + 1]) == (("history", 0, 8), ("history", 0, 8))
    assert all(c["env"] == S.RECORDS_ENV for c in S.of_family("records_sims_importance"))
    # the shape of a case: small filters in few slots, one slot used again, short runs except where many searches or a deep LDS are the subject
    for c in S.CASES:
        kw, long_run = c["kw"], c["family"].startswith(("epoch_", "deep_lds_"))
        assert 32 <= kw["particles"] <= 64 and kw.get("episodes", 1) * kw["horizon"] <= 126
        if c["oracle_of"]:
            continue
        assert c["E"] == S.DEEP_E if c["family"].startswith("deep_lds_") else c["E"] in (2, 3), c["name"]
        assert c["runs"] == (c["E"] if c["name"] in S.CUT_RUNS else 9 if c["family"] == "epoch_hash" else c["E"] + 1), c["name"]
        assert long_run or (3 <= kw["horizon"] <= 8 and kw.get("episodes", 1) in (1, 2)), c["name"]


@pytest.mark.parametrize("family", sorted(S.SWITCHES))
def test_search_size_cases_load_the_field_their_limit_protects(family):
    """the cheapest case of every family on the oracle alone: two searches in a row in some slot, and the family's conditions"""
    c = S.cheapest_of(family)
    tr = _oracle(c["name"])["trace"]
    assert len(tr) > 0
    S.assert_conditions(c, tr)
