"""The case table of tests/test_gpu_create_plan.py: what fba_create decides for a configuration, and what it refuses with which message.

A case is a creation only: a configuration, the environment switches it is made under, and what the context then answers -- the return code
and fba_last_error(NULL); for a context that is made its sizes, the bytes of a particle record (which says which record format fba_create
chose), the slots, the bytes of a snapshot block, and, where the belief allows snapshots, the header of slot 0 exported before
fba_belief_init.  Nothing runs, and the contexts that are made hold at most 256 particles in at most 4 slots, so the whole table takes a
few seconds.  Three refusals name a larger particle count (incubator_resample_1025, incubator_8193_particles, importance_above_2_26) and
allocate nothing; one made context is large on purpose: buckets_at_fit, a bucket table at the key fit bound, about 165 MB in one slot.

The expected side, tests/golden/create_plan_expected.jsonl, was recorded by scripts/record_create_plan.py at the commit before fba_create
was split into stages (ee2f841) and is compared without tolerance.  A new case is recorded the same way: at a commit whose fba_create is
trusted, never from the code under test.  The one machine-dependent text is the device count in "device 99 out of range (1 visible)": the
test reads the count of its own machine from the runtime."""
import contextlib
import ctypes as C
import json
import os

import numpy as np

import fba_pomdp_amd._native as N

POMDP, TABLE, FACT = N.MODEL_POMDP, N.MODEL_BA_TABLE, N.MODEL_BA_FACTORED
REJ, IS, POINT = "rejection_sampling", "importance_sampling", "point_estimate"
TIGER, CTIGER, FTIGER, GRID, CA = "episodic-tiger", "continuous-tiger", "episodic-factored-tiger", "gridworld", "random-collision-avoidance"
SYSADMIN, COFFEE, AGR = "independent-sysadmin", "coffee", "agr"
DENSE = {"FBA_DENSE_PARTICLES": "1"}
RECORDS = {"FBA_HIST_TREE": "records"}
MULTI = {"FBA_IS_MULTI_MIN": "1"}
CA431 = dict(width=4, height=3, size=1)
GRID_FIT = (1 << 28) // (4 * 27) - 2        # the most buckets whose keys fit 28 bits at the 27 observations of gridworld --size 3
HEAD_FIELDS = ("record_format", "weighted", "particle_bytes", "counts_len", "stride", "prior_hash")
SNAPSHOT_BELIEFS = (N.BELIEF_REJECTION, N.BELIEF_IMPORTANCE, N.BELIEF_POINT)

CASES = []


def add(name, domain, model, belief=REJ, planner="po-uct", env=None, null=None, **kw):
    """null: "cfg" or "out" -- fba_create is handed a null pointer in that argument"""
    kw.setdefault("particles", 16)
    kw.setdefault("sims", 8)
    kw.setdefault("horizon", 4)
    kw.setdefault("runs", 2)
    kw.setdefault("slots", 2)
    kw.setdefault("episodes", 1 if model == POMDP else 2)
    CASES.append(dict(name=name, domain=domain, model=model, belief=belief, planner=planner, env=dict(env or {}), null=null, kw=kw))


# ---- every record format and its nearest miss
add("tiger_table_packed", TIGER, TABLE)
add("tiger_table_packed_importance", TIGER, TABLE, IS)
add("tiger_table_dense_by_switch", TIGER, TABLE, env=DENSE)
add("tiger_table_dense_by_multi_min", TIGER, TABLE, IS, env=MULTI)
add("tiger_table_65535_steps", TIGER, TABLE, episodes=13107, horizon=5)
add("tiger_table_65540_steps", TIGER, TABLE, episodes=13108, horizon=5)
add("tiger_table_random_planner", TIGER, TABLE, planner="random")
add("tiger_table_regular_dirichlet", TIGER, TABLE, dirichlet_regular=1)
add("tiger_planning", TIGER, POMDP)
for size in (1, 2, 3, 4):
    add(f"ftiger_size{size}", FTIGER, FACT, size=size)
add("ftiger_point_estimate", FTIGER, FACT, POINT, size=3)
add("ftiger_importance", FTIGER, FACT, IS, size=3)
add("ftiger_dense_by_switch", FTIGER, FACT, size=3, env=DENSE)
add("ftiger_table", FTIGER, TABLE, size=2)
add("grid_fact_importance", GRID, FACT, IS, size=3)
add("grid_fact_rejection", GRID, FACT, size=3)
add("grid_fact_rejection_random", GRID, FACT, planner="random", size=3)
add("grid_fact_rejection_ts", GRID, FACT, planner="ts", size=3)
add("grid_fact_rejection_records", GRID, FACT, size=3, env=RECORDS)
add("grid_fact_importance_records", GRID, FACT, IS, size=3, env=RECORDS)
add("grid_fact_rejection_65536_sims", GRID, FACT, size=3, sims=65536, slots=1)
add("grid_fact_rejection_65537_sims", GRID, FACT, size=3, sims=65537, slots=1)
add("grid_fact_importance_65537_sims", GRID, FACT, IS, size=3, sims=65537, slots=1)
add("grid_fact_importance_full_stride", GRID, FACT, IS, size=3, env={"FBA_HIST_STRIDE": "full"})
add("grid_fact_dense_by_switch", GRID, FACT, IS, size=3, env=DENSE)
add("grid_fact_126_steps", GRID, FACT, IS, size=3, episodes=21, horizon=6)
add("grid_fact_126_steps_full_stride", GRID, FACT, IS, size=3, episodes=21, horizon=6, env={"FBA_HIST_STRIDE": "full"})
add("grid_fact_127_steps",GRID, FACT, IS, size=3, episodes=1, horizon=127)
add("grid_fact_point_estimate", GRID, FACT, POINT, size=3)
add("grid_fact_double_buffer", GRID, FACT, IS, size=3, env={"FBA_DOUBLE_BUFFER": "1"})
add("grid_fact_scratch_slots", GRID, FACT, IS, size=3, slots=4, runs=4, env={"FBA_SCRATCH_SLOTS": "2"})
add("grid_fact_search_budget", GRID, FACT, IS, size=3, search_budget=16)
add("grid_table_importance", GRID, TABLE, IS, size=3)
add("grid_table_rejection", GRID, TABLE, size=3)
add("grid_table_rejection_ts", GRID, TABLE, planner="ts", size=3)
add("grid_table_importance_records", GRID, TABLE, IS, size=3, env=RECORDS)
add("grid_planning_node_visits", GRID, POMDP, size=3, env={"FBA_NODE_VISITS": "1"})
add("grid_planning_wide_hash", GRID, POMDP, size=3, env={"FBA_WIDE_HASH": "1"})
add("ca_history_multi", CA, FACT, IS, env=MULTI, **CA431)
add("ca_dense_one_launch", CA, FACT, IS, **CA431)
add("ca_dense_width9", CA, FACT, IS, env=MULTI, width=9, height=3, size=1)
add("ca_dense_structure_prior", CA, FACT, IS, env=MULTI, structure_prior=1, **CA431)
add("ca_dense_ts", CA, FACT, IS, planner="ts", env=MULTI, **CA431)
add("ca_dense_multi_min_above", CA, FACT, IS, env={"FBA_IS_MULTI_MIN": "17"}, **CA431)
add("ca_history_multi_min_at", CA, FACT, IS, env={"FBA_IS_MULTI_MIN": "16"}, **CA431)
add("ca_table", CA, TABLE, IS, **CA431)
add("sysadmin_fact", SYSADMIN, FACT, size=2)
add("sysadmin_table", SYSADMIN, TABLE, IS, size=2)
add("coffee_planning", COFFEE, POMDP)
add("agr_planning", AGR, POMDP)

# ---- tree_buckets
add("buckets_explicit", GRID, FACT, size=3, tree_buckets=64)
add("buckets_below_eight", GRID, FACT, size=3, tree_buckets=3)
add("buckets_at_fit", GRID, FACT, IS, size=3, tree_buckets=GRID_FIT, slots=1)
add("buckets_above_fit_importance", GRID, FACT, IS, size=3, tree_buckets=GRID_FIT + 1)
add("buckets_above_fit_rejection", GRID, FACT, size=3, tree_buckets=GRID_FIT + 1)        # (no flat search: dense records, nothing to refuse)
add("buckets_negative", GRID, FACT, size=3, tree_buckets=-1)
add("buckets_negative_tiger", TIGER, TABLE, tree_buckets=-1)
add("buckets_unused_tiger", TIGER, TABLE, tree_buckets=64)
add("buckets_unused_records_tree", GRID, FACT, IS, size=3, tree_buckets=64, env=RECORDS)
add("buckets_unusable_65537_sims", GRID, FACT, IS, size=3, sims=65537, tree_buckets=64, slots=1)

# ---- one good context of each composite belief
add("reinvigoration", FTIGER, FACT, "reinvigoration", size=2, resample_amount=2)
add("cheating", FTIGER, FACT, "cheating-reinvigoration", size=2, resample_amount=2, threshold=-5.0)
add("incubator", FTIGER, FACT, "incubator", size=2, resample_amount=2, threshold=0.5)
add("nested", TIGER, TABLE, "nested", particles=4)
add("mh_within_gibbs", FTIGER, FACT, "mh-within-gibbs", size=2, threshold=-5.0)
add("mh_within_gibbs_option", FTIGER, FACT, "mh-within-gibbs", size=2, threshold=-5.0, belief_option=1)
add("mh_nips", FTIGER, FACT, "mh-nips", size=2, threshold=-5.0)
add("mh_collision_avoidance", CA, FACT, "mh-within-gibbs", threshold=-5.0, structure_prior=1, **CA431)
add("regular_dirichlet_fact", FTIGER, FACT, IS, size=2, dirichlet_regular=1)

# ---- slots
add("slots_from_runs", TIGER, TABLE, slots=0, runs=5)
add("slots_explicit_above_runs", TIGER, TABLE, slots=4, runs=2)

# ---- refusals: one case for every message fba_create can give on a machine with a device
add("null_config", TIGER, POMDP, null="cfg")
add("null_result", TIGER, POMDP, null="out")
add("no_sims", TIGER, POMDP, sims=0)
add("no_sims_random_planner", TIGER, POMDP, planner="random", sims=0)                     # (only po-uct asks for simulations)
add("no_horizon", TIGER, POMDP, horizon=0)
add("horizon_256", TIGER, POMDP, horizon=256)
add("no_particles", TIGER, POMDP, particles=0)
add("no_particles_point_estimate", TIGER, POMDP, POINT, particles=0)
add("discount_zero", TIGER, POMDP, discount=0.0)
add("discount_above_one", TIGER, POMDP, discount=1.5)
add("no_runs", TIGER, POMDP, runs=0)
add("no_episodes", TIGER, TABLE, episodes=0)
add("episodes_65536", TIGER, TABLE, episodes=65536)
add("planning_two_episodes", TIGER, POMDP, episodes=2)
add("device_out_of_range", TIGER, POMDP, device=99)
add("device_negative", TIGER, POMDP, device=-1)
add("cheating_table", TIGER, TABLE, "cheating-reinvigoration", resample_amount=2, threshold=-5.0)
add("cheating_no_resample", FTIGER, FACT, "cheating-reinvigoration", size=2, resample_amount=0, threshold=-5.0)
add("cheating_threshold", FTIGER, FACT, "cheating-reinvigoration", size=2, resample_amount=2, threshold=0.0)
add("mh_gibbs_table", TIGER, TABLE, "mh-within-gibbs", threshold=-5.0)
add("mh_nips_regular_dirichlet", FTIGER, FACT, "mh-nips", size=2, threshold=-5.0, dirichlet_regular=1)
add("mh_fully_connected_ca", CA, FACT, "mh-within-gibbs", threshold=-5.0, structure_prior=3, **CA431)
add("mh_nips_sysadmin", SYSADMIN, FACT, "mh-nips", size=2, threshold=-5.0)
add("mh_gibbs_threshold", FTIGER, FACT, "mh-within-gibbs", size=2, threshold=0.5)
add("mh_nips_threshold", FTIGER, FACT, "mh-nips", size=2, threshold=0.0)
add("incubator_gridworld", GRID, FACT, "incubator", size=3, resample_amount=2, threshold=0.5)
add("incubator_no_resample", FTIGER, FACT, "incubator", size=2, resample_amount=0, threshold=0.5)
add("incubator_threshold_zero", FTIGER, FACT, "incubator", size=2, resample_amount=2, threshold=0.0)
add("incubator_threshold_two", FTIGER, FACT, "incubator", size=2, resample_amount=2, threshold=2.0)
add("incubator_resample_all", FTIGER, FACT, "incubator", size=2, resample_amount=16, threshold=0.5)
add("incubator_resample_1025", FTIGER, FACT, "incubator", size=2, particles=2048, resample_amount=1025, threshold=0.5)
add("incubator_8193_particles", FTIGER, FACT, "incubator", size=2, particles=8193, resample_amount=2, threshold=0.5)
add("incubator_promotes_all", FTIGER, FACT, "incubator", size=2, resample_amount=2, threshold=0.01)
add("nested_planning", TIGER, POMDP, "nested", particles=4)
add("nested_257_particles", TIGER, TABLE, "nested", particles=257)
add("reinvigoration_gridworld", GRID, FACT, "reinvigoration", size=3, resample_amount=2)
add("reinvigoration_no_resample", FTIGER, FACT, "reinvigoration", size=2, resample_amount=0)
add("ftiger_size0", FTIGER, FACT, size=0)
add("ftiger_size13", FTIGER, FACT, size=13)
add("agr_table", AGR, TABLE)
add("agr_importance", AGR, POMDP, IS)
add("coffee_table", COFFEE, TABLE)
add("sysadmin_size0", SYSADMIN, FACT, size=0)
add("sysadmin_size9", SYSADMIN, FACT, size=9)
add("ca_width0", CA, FACT, IS, width=0, height=3, size=1)
add("ca_height2", CA, FACT, IS, width=4, height=2, size=1)
add("ca_height17", CA, FACT, IS, width=4, height=17, size=1)
add("ca_five_obstacles_four_columns", CA, FACT, IS, width=4, height=3, size=5)
add("ca_seven_obstacles", CA, FACT, IS, width=9, height=3, size=7)
add("grid_size2", GRID, FACT, size=2)
add("grid_size16", GRID, FACT, size=16)
add("unknown_domain", 99, POMDP)
add("unknown_model", TIGER, 7)
add("tiger_factored", TIGER, FACT)
add("ftiger_fact_size8", FTIGER, FACT, size=8)          # (the domain takes up to 12 features, the factored prior 7)
add("ftiger_fact_size12", FTIGER, FACT, size=12)
add("ftiger_fact_noise", FTIGER, FACT, size=2, noise=0.5)
add("grid_fact_noise", GRID, FACT, size=3, noise=-0.1)
add("grid_fact_structure_prior", GRID, FACT, size=3, structure_prior=1)
add("ca_fact_noise", CA, FACT, IS, noise=0.6, **CA431)
add("sysadmin_structure_prior", SYSADMIN, FACT, size=2, structure_prior=1)
add("tiger_table_noise", TIGER, TABLE, noise=0.5)
add("grid_table_noise", GRID, TABLE, size=3, noise=-0.1)
add("ca_table_noise", CA, TABLE, IS, noise=0.6, **CA431)
add("importance_above_2_26", TIGER, POMDP, IS, particles=(1 << 26) + 1)
add("mh_over_multi_limit", FTIGER, FACT, "mh-within-gibbs", size=2, threshold=-5.0, env=MULTI)
add("cheating_over_multi_limit", FTIGER, FACT, "cheating-reinvigoration", size=2, resample_amount=2, threshold=-5.0, env=MULTI)
add("regular_dirichlet_planning", TIGER, POMDP, dirichlet_regular=1)
add("regular_dirichlet_long_row", GRID, TABLE, size=3, dirichlet_regular=1)

# ---- precedence: two faults at once, which pin the order of the refusals
add("first_sims_then_domain", 99, POMDP, sims=0)
add("first_cheating_then_domain", FTIGER, TABLE, "cheating-reinvigoration", size=0, resample_amount=2, threshold=-5.0)
add("first_nested_model_then_count", TIGER, POMDP, "nested", particles=300)
add("first_buckets_then_mh_limit", FTIGER, FACT, "mh-within-gibbs", size=2, threshold=-5.0, tree_buckets=-1, env=MULTI)
add("first_buckets_then_regular_dirichlet", TIGER, POMDP, dirichlet_regular=1, tree_buckets=-1)
add("first_incubator_threshold_then_resample", FTIGER, FACT, "incubator", size=2, resample_amount=0, threshold=2.0)

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@contextlib.contextmanager
def environment(case):
    """the case's switches in the process environment (fba_create reads them at every call), and no other FBA_ switch"""
    saved = {k: v for k, v in os.environ.items() if k.startswith("FBA_") and k != "FBA_LIB"}
    for k in saved:
        del os.environ[k]
    os.environ.update(case["env"])
    try:
        yield
    finally:
        for k in case["env"]:
            os.environ.pop(k, None)
        os.environ.update(saved)


def config_of(L, case):
    cfg = N.Config()
    L.fba_default_config(C.byref(cfg))
    cfg.domain = N.DOMAIN_NAMES.get(case["domain"], case["domain"])
    cfg.model = case["model"]
    cfg.belief = N.BELIEF_NAMES[case["belief"]]
    cfg.planner = N.PLANNER_NAMES[case["planner"]]
    for k, v in case["kw"].items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return cfg


def observe(L, case, probe=None):
    """fba_create under the case's environment, and what the table records of the outcome.  probe(handle), if given, is called while the
    context exists (scripts/record_create_plan.py measures the device bytes there)."""
    cfg = config_of(L, case)
    h = C.c_void_p()
    with environment(case):
        rc = L.fba_create(None if case["null"] == "cfg" else C.byref(cfg), None if case["null"] == "out" else C.byref(h))
    if rc != N.OK:
        assert not h.value
        return {"rc": rc, "error": L.fba_last_error(None).decode()}
    try:
        S, A, O, per = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        assert L.fba_domain_sizes(h, C.byref(S), C.byref(A), C.byref(O)) == N.OK
        assert L.fba_belief_snapshot_bytes(h, C.byref(per)) == N.OK
        seen = {"rc": rc, "sizes": [S.value, A.value, O.value], "counts_len": L.fba_counts_len(h), "particle_bytes": L.fba_particle_bytes(h),
                "slots": L.fba_slots(h), "snapshot_bytes": per.value}
        if cfg.belief in SNAPSHOT_BELIEFS:
            block = np.zeros(per.value, np.uint8)
            assert L.fba_belief_export(h, 0, 1, block.ctypes.data, block.nbytes) == N.OK, L.fba_last_error(h).decode()
            head = block[:N.SNAPSHOT_HEAD_DTYPE.itemsize].view(N.SNAPSHOT_HEAD_DTYPE)[0]
            seen["head"] = {f: int(head[f]) for f in HEAD_FIELDS}
        if probe:
            probe(h)
        return seen
    finally:
        L.fba_destroy(h)


def expected():
    """name -> what observe() returned at the recording commit (tests/golden/create_plan_expected.jsonl)"""
    table = {}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_plan_expected.jsonl")) as f:
        for line in f:
            rec = json.loads(line)
            table[rec.pop("name")] = rec
    return table
