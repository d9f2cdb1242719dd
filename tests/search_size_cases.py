"""The case table of tests/test_gpu_search_sizes.py: one small whole experiment on each side of every tree size at which the engine takes
another search kernel, another tree layout or another packed bit-field -- with the oracle's side of it.

Every other oracle comparison of the suite fixes `sims` between 8 and 300 (one node-bound test at 3000; the full-size workloads at their
nominal 4096 and 65536).  Here the filters are 32 to 64 particles in E = 2 or 3 slots (49 where the waves of a workgroup are the subject), and sims, max_depth, A * O and the number of searches
a slot has made are the subject:

    switch-over                      where                                      what changes
    sims <= 65535                    etiger_ok                                  ETIGER layout (16-bit counts n0 | n1 << 16) or the general one
    max_nodes <= 4093                etiger_ok; plan_tree's episodic bound      the same two layouts, by min(sims + 2, 2^(max_depth + 1) + 1)
    max_nodes <= 32767               root_children_in_lds                       the root's children as int16 in LDS or in its record
    A * O <= ROOT_CHILDREN           root_children_in_lds                       the same
    A * O > 64                       plan_tree (hashed)                         children in the record or in the hash table; the visits word
    max_nodes * A * O < 2^27         plan_tree (hash_compact)                   8-byte entries with a 5-bit epoch, or 16-byte entries
    sims <= 65536                    bucket_tree_search, plan_tree; `spec`      bucket tree, or node records + hash table; count | hint << 16
    epoch > 15, epoch > 31           search_hist2 / hash_begin_search           the slot's table is wiped and the epoch restarts at 1
    4 -> 2 -> 1 waves, raise_lds     search_plan, h2_wave_bytes                 the LDS geometry of the bucket-tree searches, by max_depth
    A <= 4, 8, 16                    search_plan (amax)                         the instantiation, the width of the root's register arrays
    Cs <= SEARCH_STAGE_WORDS         search_plan (stage)                        the root particle staged in LDS or read from HBM

A case makes runs = E + 1 runs in E slots: one slot is used again, the others are inactive in the last round.  It states the tree geometry
it expects (`geom`: A, O, max_nodes, node_words, hash_entry, bkt_lines), which the GPU test compares with Engine.device_arrays() before
anything runs: that is what proves on which side of its switch the case stands.  SWITCHES names, for every family, the switch-overs of
its kernels; tests/test_gpu_search_sizes.py reads the thresholds out of the sources and asserts that the family has a case on each side.
CONDITIONS names what the oracle's trace of a family must show, so that the field a limit protects is really loaded (checked without a
GPU on the family's cheapest case that carries the condition, and on the GPU for every case that carries it)."""
import wide_launch_cases as W
from wide_launch_cases import FACT, IS, POMDP, REJ, TABLE

TIGER, CTIGER, GRID, CA, SYS = "episodic-tiger", "continuous-tiger", "gridworld", "random-collision-avoidance", "linear-sysadmin"
RECORDS_ENV = {"FBA_HIST_TREE": "records"}
WIDE_ENV = {"FBA_WIDE_HASH": "1"}
BUCKET_WRAP, HASH_WRAP = 15, 31           # searches of one slot between two wipes of its table (4-bit and 5-bit epochs)

# family -> the switch-overs its search has (the family's cases must hold both sides of each)
SWITCHES = {
    "etiger_sims_planning": ("ETIGER_SIMS",),
    "etiger_sims_table_packed": ("ETIGER_SIMS",),
    "etiger_sims_table_dense": ("ETIGER_SIMS",),
    "etiger_nodes_planning": ("ETIGER_NODES", "ETIGER_DEPTH"),
    "etiger_nodes_table_packed": ("ETIGER_NODES",),
    "root_children_planning": ("ROOT_CHILDREN_NODES",),
    "root_children_table": ("ROOT_CHILDREN_NODES",),
    "sysadmin_planning": ("ROOT_CHILDREN_AO", "AMAX"),
    "sysadmin_factored": ("ROOT_CHILDREN_AO", "AMAX"),
    "sysadmin_table": ("STAGE_WORDS",),
    "hashed_children": ("HASHED_AO",),
    "wide_hash": ("HASH_COMPACT", "WIDE_HASH_ENV"),
    "bucket_sims_importance": ("BUCKET_SIMS",),
    "bucket_sims_rejection": ("BUCKET_SIMS",),
    "bucket_sims_table": ("BUCKET_SIMS",),
    "records_sims_importance": ("BUCKET_SIMS",),
    "epoch_bucket": ("BUCKET_EPOCH",),
    "epoch_bucket_table": ("BUCKET_EPOCH",),
    "epoch_hash": ("HASH_EPOCH",),
    "epoch_records": ("HASH_EPOCH",),
    "deep_lds_table": ("H2_WAVES",),
    "deep_lds_importance": ("H2_WAVES_SHARED",),
    "deep_lds_rejection": ("H2_WAVES_SHARED",),
}

# family -> what the oracle's trace must show ("streak" holds for every case: two searches in a row in one slot within one run)
CONDITIONS = {
    "etiger_sims_planning": ("listen_count",),
    "etiger_sims_table_packed": ("listen_count",),
    "etiger_sims_table_dense": ("listen_count",),
    "etiger_nodes_planning": ("nodes_stated",),
    "root_children_planning": ("nodes_sims_minus_1",),
    "root_children_table": ("nodes_sims_minus_1",),
    "wide_hash": ("nodes_stated",),
    "bucket_sims_importance": ("nodes_32768",),
    "bucket_sims_rejection": ("nodes_32768",),
    "bucket_sims_table": ("nodes_32768",),
    "records_sims_importance": ("nodes_32768",),
    "epoch_bucket": ("wrap",),
    "epoch_bucket_table": ("wrap",),
    "epoch_hash": ("wrap",),
    "epoch_records": ("wrap",),
    "deep_lds_table": ("last_wave",),
    "deep_lds_importance": ("last_wave",),
    "deep_lds_rejection": ("last_wave",),
}

CASES = []


def node_words(A, O):
    """a node record (fba_state.h): [visits], the action counts, padded to two words; the Qs as doubles; the children unless hashed"""
    hashed = A * O > 64
    cn = 0 if hashed and A % 2 == 0 else 1
    cq = (cn + A + 1) // 2 * 2
    child = cq + 2 * A
    return child if hashed else (child + A * O + 1) // 2 * 2


def add(family, name, domain, model, belief, fmt, geom, E=2, runs=None, env=None, seed0=5000, oracle_of=None, **kw):
    """geom: A, O, max_nodes, and hash_entry (0: children in the record) or bkt_lines (the bucket tree); node_words follows from A and O"""
    kw.setdefault("particles", 32)
    kw.setdefault("horizon", 4)
    if model != POMDP:
        kw.setdefault("episodes", 2)
    g = dict(hash_entry=0, bkt_lines=0)
    g.update(geom)
    g["node_words"] = node_words(g["A"], g["O"])
    assert (g["hash_entry"] != 0) == (g["A"] * g["O"] > 64 and not g["bkt_lines"])
    kw.setdefault("seed", seed0 + len(CASES))
    c = W.case(f"{family}_{name}", domain, model, belief, fmt, E=E, runs=E + 1 if runs is None else runs, env=env, **kw)
    c.update(family=family, geom=g, oracle_of=oracle_of)
    CASES.append(c)
    return c


TG = dict(A=3, O=2)

# ---- the ETIGER layout by sims: 65535 | 65536 (the episodic bound keeps max_nodes at 2^(6 + 1) + 1; the loaded field is the 16-bit count)
for s in (65535, 65536):
    g = dict(TG, max_nodes=129)
    add("etiger_sims_planning", s, TIGER, POMDP, REJ, "dense", g, sims=s, horizon=6)
    add("etiger_sims_table_packed", s, TIGER, TABLE, REJ, "packed_tiger", g, sims=s, horizon=6)
    add("etiger_sims_table_dense", s, TIGER, TABLE, REJ, "dense", g, env=W.DENSE_ENV, sims=s, horizon=6)

# ---- the ETIGER layout by the node bound: max_depth = 11 allows 4097 records, so sims + 2 decides (4093 | 4094); and at 60000 simulations
# max_depth 10 | 11 (2049 | 4097 records; an even and an odd depth_cap: two path16 entries per word)
for s in (4091, 4092):
    g = dict(TG, max_nodes=s + 2)
    add("etiger_nodes_planning", f"sims{s}", TIGER, POMDP, REJ, "dense", g, sims=s, max_depth=11, horizon=8)
    add("etiger_nodes_table_packed", f"sims{s}", TIGER, TABLE, REJ, "packed_tiger", g, sims=s, max_depth=11, horizon=8)
for d in (10, 11):
    add("etiger_nodes_planning", f"depth{d}", TIGER, POMDP, REJ, "dense", dict(TG, max_nodes=(2 << d) + 1), sims=60000, max_depth=d,
        horizon=8)

# ---- the root's children as int16 in LDS: max_nodes 32767 | 32768 on continuous tiger (no episodic bound).  An exploration constant of
# 1e5 makes the search breadth-first, so nearly every simulation adds a node and child indices use bit 14
for s in (32765, 32766):
    g = dict(TG, max_nodes=s + 2)
    add("root_children_planning", s, CTIGER, POMDP, IS, "dense", g, sims=s, horizon=8, exploration=1e5)
    add("root_children_table", s, CTIGER, TABLE, IS, "packed_tiger", g, sims=s, horizon=8, episodes=1, exploration=1e5)

# ---- linear sysadmin, A = 2 * size and O = 2: A * O = 8 | 12 (ROOT_CHILDREN), A = 4 | 6, 8 | 10, 16 (the AMAX ladder); the tabular
# model's record of 2^size * A * (2^size + 2) counts is 97 | 481 words (SEARCH_STAGE_WORDS)
for n in (2, 3, 4, 5, 8):
    g = dict(A=2 * n, O=2, max_nodes=66)
    add("sysadmin_planning", f"size{n}", SYS, POMDP, REJ, "dense", g, size=n, sims=64, horizon=5)
    add("sysadmin_factored", f"size{n}", SYS, FACT, REJ, "dense", g, size=n, sims=64, horizon=5)
    if n <= 3:
        add("sysadmin_table", f"size{n}", SYS, TABLE, REJ, "dense", g, size=n, sims=64, horizon=5)

# ---- children in the record or in the hash table: no domain has A * O = 64 | 65; the nearest below are sysadmin 8 (32) and collision
# avoidance 5 x 3 x 2 (27), the nearest above collision avoidance 5 x 5 x 2 (75, odd A: the visits word stays) and gridworld 3 (108, even A)
add("hashed_children", "sysadmin8_ao32", SYS, POMDP, IS, "dense", dict(A=16, O=2, max_nodes=130), size=8, sims=128, horizon=5)
add("hashed_children", "ca_5x3x2_ao27", CA, POMDP, IS, "dense", dict(A=3, O=9, max_nodes=130), width=5, height=3, size=2, sims=128, horizon=6)
add("hashed_children", "ca_5x5x2_ao75", CA, POMDP, IS, "dense", dict(A=3, O=25, max_nodes=130, hash_entry=8), width=5, height=5, size=2,
    sims=128, horizon=6)
add("hashed_children", "gridworld3_ao108", GRID, POMDP, IS, "dense", dict(A=4, O=27, max_nodes=130, hash_entry=8), size=3, sims=128, horizon=6)

# ---- 8-byte or 16-byte hash entries: planning gridworld 7 (A * O = 1960), (sims + 2) * 1960 < 2^27 up to 68476 simulations; and a small
# tree made wide by FBA_WIDE_HASH, next to its compact twin
for s in (68476, 68477):
    add("wide_hash", f"gridworld7_{s}", GRID, POMDP, IS, "dense", dict(A=4, O=490, max_nodes=s + 2, hash_entry=8 if s == 68476 else 16),
        size=7, sims=s, horizon=3)
add("wide_hash", "gridworld3_compact", GRID, POMDP, IS, "dense", dict(A=4, O=27, max_nodes=258, hash_entry=8), size=3, sims=256, horizon=6,
    seed0=5500)
add("wide_hash", "gridworld3_env", GRID, POMDP, IS, "dense", dict(A=4, O=27, max_nodes=258, hash_entry=16), env=WIDE_ENV, size=3, sims=256,
    horizon=6, seed0=5499)

# ---- the bucket tree up to 65536 simulations, node records + hash table beyond (where the rejection filter and the tabular model keep
# dense records and search_kernel's hashed tree); under FBA_HIST_TREE=records search_hist_kernel on both sides, with and without its hints
GW3 = dict(A=4, O=27)
# Four steps deep at an exploration constant of 1000 a root's tree passes 32768 nodes (three steps: 13000), so a 16-bit hint uses its top bit.
# CUT_RUNS: the tabular model's dense records at 65537 simulations are 5833 words that search_kernel reads unstaged, the slowest search of
# the table by far; the case keeps its sims and makes one run per slot.
# (Beyond 65536 simulations plan_tree gives node records, 8-byte hash entries and spec == false with or without FBA_HIST_TREE=records, so
#  records_sims_importance_65537 runs the path of bucket_sims_importance_65537 from another seed: it is there so that the family under the
#  switch holds both sides, not as a second path.)
CUT_RUNS = ("bucket_sims_table_65537",)
BIG = dict(size=3, horizon=4, episodes=1, exploration=1000.0)
for s in (65536, 65537):
    bucket = s <= 65536
    g = dict(GW3, max_nodes=s + 2, bkt_lines=s + 2) if bucket else dict(GW3, max_nodes=s + 2, hash_entry=8)
    add("bucket_sims_importance", s, GRID, FACT, IS, "history", g, structure_prior=2, sims=s, **BIG)
    add("bucket_sims_rejection", s, GRID, FACT, REJ, "history" if bucket else "dense", g, structure_prior=2, sims=s, **BIG)
    add("bucket_sims_table", s, GRID, TABLE, IS, "history" if bucket else "dense", g, runs=3 if bucket else 2, sims=s, **BIG)
    add("records_sims_importance", s, GRID, FACT, IS, "history", dict(GW3, max_nodes=s + 2, hash_entry=8), env=RECORDS_ENV,
        structure_prior=2, sims=s, **BIG)

# ---- the epoch wipes: more searches in one slot than the epoch field counts (4 bits in a bucket's key, 5 in a compact hash entry).
# Long horizons, few simulations, more runs than slots; the `_one_slot` twins run the same experiment in one slot -- every search of the
# oracle's trace in order on one table -- and are compared with the same oracle run
twin = add("epoch_bucket", "gridworld3", GRID, FACT, IS, "history", dict(GW3, max_nodes=26, bkt_lines=26), E=3, size=3, structure_prior=2, sims=24,
    horizon=12, episodes=3)
add("epoch_bucket", "gridworld3_one_slot", GRID, FACT, IS, "history", dict(GW3, max_nodes=26, bkt_lines=26), E=1, runs=4,
    oracle_of="epoch_bucket_gridworld3", size=3, structure_prior=2, sims=24, horizon=12, episodes=3, seed=twin["kw"]["seed"])
tab = add("epoch_bucket_table", "gridworld3", GRID, TABLE, IS, "history", dict(GW3, max_nodes=26, bkt_lines=26), E=3, size=3, sims=24,
          horizon=12, episodes=3)
hsh = add("epoch_hash", "gridworld5", GRID, POMDP, IS, "dense", dict(A=4, O=150, max_nodes=26, hash_entry=8), E=3, runs=9, size=5, sims=24,
          horizon=40)
add("epoch_hash", "gridworld5_one_slot", GRID, POMDP, IS, "dense", dict(A=4, O=150, max_nodes=26, hash_entry=8), E=1, runs=9,
    oracle_of="epoch_hash_gridworld5", size=5, sims=24, horizon=40, seed=hsh["kw"]["seed"])
# A search that fills its table (24 new nodes in 64 entries) overwrites every entry of another epoch within a few searches, wipe or no wipe,
# so the cases above can hardly see a missing wipe.  What it leaves behind lasts where the trees saturate far below `sims` -- max_depth 1 or
# 2 -- so that most of a table is never written between two searches of the same epoch; then the first search after the wrap finds children
# that this search never made
SAT = dict(max_depth=2, horizon=12, episodes=3, size=3)
add("epoch_bucket", "gridworld3_depth2", GRID, FACT, IS, "history", dict(GW3, max_nodes=258, bkt_lines=258), E=3, structure_prior=2, sims=256,
    seed=twin["kw"]["seed"], **SAT)
add("epoch_bucket_table", "gridworld3_depth2", GRID, TABLE, IS, "history", dict(GW3, max_nodes=258, bkt_lines=258), E=3, sims=256,
    seed=tab["kw"]["seed"], **SAT)
# (search_hist_kernel: node records and compact hash entries, wiped by the four lanes of the tree's quad)
rec = add("epoch_records", "gridworld3_depth2", GRID, FACT, IS, "history", dict(GW3, max_nodes=1002, hash_entry=8), E=3, env=RECORDS_ENV,
          structure_prior=2, sims=1000, seed=twin["kw"]["seed"], **SAT)
add("epoch_records", "gridworld3_depth2_one_slot", GRID, FACT, IS, "history", dict(GW3, max_nodes=1002, hash_entry=8), E=1, runs=4,
    env=RECORDS_ENV, oracle_of=rec["name"], structure_prior=2, sims=1000, seed=twin["kw"]["seed"], **SAT)
GW5 = dict(A=4, O=150)
h1 = add("epoch_hash", "gridworld5_depth1", GRID, POMDP, IS, "dense", dict(GW5, max_nodes=66, hash_entry=8), E=3, runs=9, size=5, sims=64,
         max_depth=1, horizon=40, seed=hsh["kw"]["seed"])
add("epoch_hash", "gridworld5_depth1_one_slot", GRID, POMDP, IS, "dense", dict(GW5, max_nodes=66, hash_entry=8), E=1, runs=9,
    oracle_of=h1["name"], size=5, sims=64, max_depth=1, horizon=40, seed=hsh["kw"]["seed"])
add("epoch_hash", "gridworld5_depth2", GRID, POMDP, IS, "dense", dict(GW5, max_nodes=1002, hash_entry=8), E=3, runs=9, size=5, sims=1000,
    max_depth=2, horizon=40, seed=hsh["kw"]["seed"])


# ---- waves per workgroup of the bucket-tree searches: 64 KB hold the shared tables and nw areas of W.h2_wave_bytes_at(max_depth, Cs).
# max_depth sizes the LDS and horizon the real depth: a horizon of 3 keeps the deep geometries cheap.  Tree e sits in wave (e / 16) % nw of
# workgroup e / (16 nw), so DEEP_E = 49 slots put a tree into the last wave of every geometry (one wave: into a fourth workgroup) and a
# wrong stride between the waves' areas, or an allocation one area short, cannot pass.  Tabular records share no tables: both sides of
# every halving.  The factored searches keep their Dirichlet rows in front of the waves' areas, under SHARED_MOST bytes at size 3; their
# cases stand at the nearest depths whose side holds for every size of those tables from 0 to SHARED_MOST
DEEP_CS = 8                               # words of a history record of 2 episodes of 3 steps
DEEP_E = 49
SHARED_MOST = 8 * 1024
DEEP_FACTORED = (30, 35, 62, 72, 126, 145)
DEEP = dict(size=3, sims=32, horizon=3)
for d in (34, 35, 71, 72, 144, 145):
    add("deep_lds_table", f"depth{d}", GRID, TABLE, IS, "history", dict(GW3, max_nodes=34, bkt_lines=34), E=DEEP_E, max_depth=d, **DEEP)
for d in DEEP_FACTORED:
    add("deep_lds_importance", f"depth{d}", GRID, FACT, IS, "history", dict(GW3, max_nodes=34, bkt_lines=34), E=DEEP_E, structure_prior=2,
        max_depth=d, **DEEP)
    add("deep_lds_rejection", f"depth{d}", GRID, FACT, REJ, "history", dict(GW3, max_nodes=34, bkt_lines=34), E=DEEP_E, structure_prior=2,
        max_depth=d, **DEEP)

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert {c["family"] for c in CASES} == set(SWITCHES) and set(CONDITIONS) <= set(SWITCHES)


def of_family(family):
    return [c for c in CASES if c["family"] == family]


def cheapest_of(family):
    """the family's case of the fewest simulated steps that is compared with an oracle run of its own"""
    return min((c for c in of_family(family) if not c["oracle_of"]), key=lambda c: (c["kw"]["sims"] * c["runs"], c["name"]))


def oracle_case(c):
    """the case whose oracle run this case is compared with: itself, or the many-slot twin of a one-slot case"""
    return BY_NAME[c["oracle_of"]] if c["oracle_of"] else c


def hash_slot_elems(g):
    """16-byte elements of one slot's hash table: a power of two of entries, at least 64, at most half full"""
    hcap = 64
    while hcap < 2 * (g["max_nodes"] - 2):
        hcap <<= 1
    return hcap * g["hash_entry"] // 16


def assert_geometry(c, arrays):
    """Engine.device_arrays() holds the tree this case says it searches"""
    g = c["geom"]
    if g["bkt_lines"]:
        assert "hash" not in arrays and arrays["nodes"].slot_elems == 0, arrays.get("hash")
        assert (arrays["bkt"].slot_elems, arrays["bkt"].elem_bytes) == (g["bkt_lines"] * 8, 16), arrays["bkt"]
        return
    assert "bkt" not in arrays, arrays.get("bkt")
    assert (arrays["nodes"].slot_elems, arrays["nodes"].elem_bytes) == (g["max_nodes"] * g["node_words"], 4), (arrays["nodes"], g)
    if g["hash_entry"]:
        assert (arrays["hash"].slot_elems, arrays["hash"].elem_bytes) == (hash_slot_elems(g), 16), (arrays["hash"], g)
    else:
        assert "hash" not in arrays, arrays["hash"]


def longest_search_streak(trace):
    """the most searches that one slot made in a row: the real steps of one episode of one run (every step begins with a search, and the
    second one starts on the tree or table the first one used)"""
    best, run, key = 0, 0, None
    for r, ep in zip(trace["run"].tolist(), trace["episode"].tolist()):
        run = run + 1 if (r, ep) == key else 1
        key = (r, ep)
        best = max(best, run)
    return best


def measures(trace):
    return dict(records=len(trace), streak=longest_search_streak(trace), nodes=int(trace["n_nodes"].max()), depth=int(trace["tree_depth"].max()),
                listen=int(trace["root_n"][:, 0].max()), count=int(trace["root_n"].max()))


# the n_nodes that the oracle reaches in the cases that cannot load their tree's index field (episodic tiger ends an episode at `open`;
# the wide hash table at its natural size is a quarter full): stated, and asserted as the least the case must go on reaching
NODES_STATED = {
    "etiger_nodes_planning_sims4091": 58, "etiger_nodes_planning_sims4092": 71,       # (at depth 6)
    "etiger_nodes_planning_depth10": 245, "etiger_nodes_planning_depth11": 243,       # (at depth 8, of 2049 | 4097 records)
    "wide_hash_gridworld7_68476": 28597, "wide_hash_gridworld7_68477": 27984,         # (of 131072 entries)
}


def assert_conditions(c, trace):
    """what the oracle's trace of this case must show, so that the case loads the field its limit protects"""
    m = measures(trace)
    kw = c["kw"]
    assert m["streak"] >= 2, m
    for cond in CONDITIONS.get(c["family"], ()):
        if cond == "listen_count":            # action 0 is `listen`: a 16-bit count with its top bit set
            assert m["listen"] >= 32768, m
        elif cond == "nodes_sims_minus_1":    # child indices up to max_nodes - 3: bit 14 of an int16
            assert m["nodes"] >= kw["sims"] - 1, m
        elif cond == "nodes_32768":           # a 16-bit hint or count with its top bit set
            assert m["nodes"] >= 32768, m
        elif cond == "wrap":                  # some slot passes the wipe and searches three more times on the cleared table
            wrap = BUCKET_WRAP if c["geom"]["bkt_lines"] else HASH_WRAP
            assert m["records"] >= c["E"] * (wrap + 3), m
        elif cond == "last_wave":             # a tree in the last of the most waves a workgroup holds, on both sides of every halving
            assert c["E"] > 16 * (4 - 1) and c["runs"] > c["E"], (c["E"], c["runs"])
        elif cond == "nodes_stated":
            if c["name"] in NODES_STATED:
                assert m["nodes"] >= NODES_STATED[c["name"]], m
    return m
