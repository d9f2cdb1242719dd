"""The case table of tests/test_gpu_wide_launch.py: one whole experiment per kernel family that launch_search, launch_belief_update,
launch_init and launch_reset choose between, in many ragged slots, with the oracle's side of it.

Every other oracle comparison of the suite runs in at most 24 slots: lanes 0..23 of workgroup 0.  Here a case runs in E slots, E neither a
multiple of 64 (SEARCH_BLOCK: one tree per lane) nor of 16 (HIST_TREES: sixteen trees per wave, four waves per workgroup in the bucket-tree
searches), and makes runs = 2 E + 37 of them: every slot is used again (need_init / need_reset on run roll-over), and in the last round
E - 37 slots are inactive while 37 keep going (the inactive-first key of search_order_kernel, the `active` exits, the n_active count).
E = 150 is two full waves of lanes and 22 more, or nine full waves of trees and 6 more (two workgroups of four waves and a partial one);
the expensive beliefs take E = 70 (one full wave of lanes and 6 more).

The oracle's side needs no GPU (oracle_side), so what a case costs there can be measured anywhere; the engine's side is engine_side."""
import numpy as np

from oracle import pyorc as orc

POMDP, TABLE, FACT = orc.MODEL_POMDP, orc.MODEL_BA_TABLE, orc.MODEL_BA_FACTORED
REJ, IS = "rejection_sampling", "importance_sampling"

DOM = {"random-collision-avoidance": orc.DOM_COLLISION_AVOID, "centered-collision-avoidance": orc.DOM_COLLISION_AVOID,
       "gridworld": orc.DOM_GRIDWORLD, "episodic-tiger": orc.DOM_TIGER_EPISODIC, "continuous-tiger": orc.DOM_TIGER_CONTINUOUS,
       "episodic-factored-tiger": orc.DOM_FTIGER_EPISODIC, "continuous-factored-tiger": orc.DOM_FTIGER_CONTINUOUS,
       "independent-sysadmin": orc.DOM_SYSADMIN_INDEPENDENT, "linear-sysadmin": orc.DOM_SYSADMIN_LINEAR,
       "coffee": orc.DOM_COFFEE, "boutilier-coffee": orc.DOM_COFFEE_BOUTILIER, "agr": orc.DOM_AGR}
BELIEF = {REJ: orc.BELIEF_REJECTION, IS: orc.BELIEF_IMPORTANCE, "reinvigoration": orc.BELIEF_REINVIGORATION,
          "cheating-reinvigoration": orc.BELIEF_CHEATING, "point_estimate": orc.BELIEF_POINT, "mh-within-gibbs": orc.BELIEF_MH_GIBBS,
          "mh-nips": orc.BELIEF_MH_NIPS, "nested": orc.BELIEF_NESTED, "incubator": orc.BELIEF_INCUBATOR}
PLANNER = {"po-uct": orc.PLANNER_POUCT, "random": orc.PLANNER_RANDOM, "ts": orc.PLANNER_TS}

# Domains whose episodes never end before the horizon (no terminal state in the domain): every length is the horizon there, so the
# "slots of one wave sit at different t" property comes from run roll-over alone and the spread of lengths is not asserted.
NEVER_TERMINAL = {"continuous-tiger", "continuous-factored-tiger", "independent-sysadmin", "linear-sysadmin", "coffee", "boutilier-coffee"}

ENGINE_ONLY = ("search_budget", "tree_buckets")     # schedules and table sizes of the engine, not parameters of the algorithm

WIDE, NARROW = 150, 70


def record_bytes(episodes, horizon):
    """a history record: state, a second word, one entry per real step"""
    return 4 * ((2 + episodes * horizon + 3) // 4 * 4)


def dense_bytes(ncnt):
    """fp32 counts and the state word: a power of two up to 64 words, a multiple of 4 words beyond (fba_create)"""
    need, cs = ncnt + 1, 4
    if need <= 64:
        while cs < need:
            cs <<= 1
    else:
        cs = (need + 3) // 4 * 4
    return 4 * cs


def packed_ftiger_bytes(size):
    fs = size + 1
    nc = 8 * fs + 4 + (2 << fs)
    return 4 * ((nc // 2 + 2 + 3) // 4 * 4)       # uint16 increments, structure word, state


def h2_wave_bytes_at(max_depth, cs):
    """fba_launch_plan.h h2_wave_bytes for records of cs words: a wave's paths, its staged records, the roots' statistics"""
    return max_depth * 16 * (8 + 4 + 4 + 4) + max(cs, 2 * max_depth) * 16 * 4 + 14 * 16 * 4


def h2_wave_bytes(horizon, episodes):
    """... at max_depth = horizon"""
    return h2_wave_bytes_at(horizon, (2 + episodes * horizon + 3) // 4 * 4)


def h2_waves(max_depth, cs, shared=0, most=4, lds=64 * 1024):
    """search_plan: (waves per workgroup of a bucket-tree search beside `shared` bytes of tables, whether the LDS limit has to be raised)"""
    nw = most
    while nw > 1 and shared + nw * h2_wave_bytes_at(max_depth, cs) > lds:
        nw >>= 1
    return nw, shared + nw * h2_wave_bytes_at(max_depth, cs) > lds


def case(name, domain, model, belief, fmt, E=WIDE, runs=None, env=None, sample=False, **kw):
    kw.setdefault("sims", 64)
    if model != POMDP:
        kw.setdefault("episodes", 2)
    return dict(name=name, domain=domain, model=model, belief=belief, fmt=fmt, E=E, runs=2 * E + 37 if runs is None else runs,
                env=env or {}, sample=sample, kw=kw)


DENSE_ENV = {"FBA_DENSE_PARTICLES": "1"}
MULTI_ENV = {"FBA_IS_MULTI_MIN": "1"}
GW = dict(structure_prior=2, horizon=7)
CA431 = dict(width=4, height=3, size=1, horizon=6)

CASES = [
    # 1. planning on tiger: the ETIGER tree layout; the weighted root sample
    case("planning_episodic_tiger_rejection", "episodic-tiger", POMDP, REJ, "dense", particles=64, horizon=8, seed=1101),
    case("planning_continuous_tiger_importance", "continuous-tiger", POMDP, IS, "dense", particles=100, horizon=6, seed=1102),
    case("planning_episodic_tiger_fewer_runs_than_slots", "episodic-tiger", POMDP, REJ, "dense", runs=97, particles=48, horizon=8, seed=1103),
    # 2. tabular tiger BA-POMDP: packed records (reject_tiger_lds_kernel, the packed importance filter) and dense ones
    case("bapomdp_tiger_packed_rejection", "episodic-tiger", TABLE, REJ, "packed_tiger", particles=64, horizon=8, seed=1201),
    case("bapomdp_tiger_packed_importance", "episodic-tiger", TABLE, IS, "packed_tiger", particles=130, horizon=8, seed=1202),
    case("bapomdp_tiger_dense_rejection", "episodic-tiger", TABLE, REJ, "dense", env=DENSE_ENV, particles=64, horizon=8, seed=1203),
    case("bapomdp_tiger_dense_importance", "episodic-tiger", TABLE, IS, "dense", env=DENSE_ENV, particles=130, horizon=8, seed=1204),
    # 3. factored tiger FBA-POMDP: the C3 kernel on packed records, the importance filter, dense records
    case("fbapomdp_factored_tiger3_match_uniform_rejection_packed", "episodic-factored-tiger", FACT, REJ, "packed_ftiger", size=3,
         structure_prior=2, particles=96, horizon=8, seed=1301),
    case("fbapomdp_factored_tiger2_importance", "episodic-factored-tiger", FACT, IS, "dense", size=2, structure_prior=2, particles=130,
         horizon=8, seed=1302),
    case("fbapomdp_factored_tiger3_rejection_dense", "episodic-factored-tiger", FACT, REJ, "dense", env=DENSE_ENV, size=3, structure_prior=2,
         particles=96, horizon=8, seed=1303),
    # 4. sysadmin: AM = 16 at eight computers; the factored and the tabular model
    case("planning_linear_sysadmin8_am16", "linear-sysadmin", POMDP, REJ, "dense", size=8, particles=64, horizon=6, seed=1401),
    case("fbapomdp_linear_sysadmin5", "linear-sysadmin", FACT, REJ, "dense", size=5, particles=80, horizon=6, seed=1402),
    case("bapomdp_independent_sysadmin3", "independent-sysadmin", TABLE, REJ, "dense", size=3, particles=80, horizon=6, seed=1403),
    # 5. agr (AM = 24) and coffee
    case("planning_agr_am24", "agr", POMDP, REJ, "dense", particles=300, horizon=8, seed=1501),
    case("planning_coffee", "coffee", POMDP, REJ, "dense", particles=130, horizon=8, seed=1502),
    case("planning_boutilier_coffee", "boutilier-coffee", POMDP, IS, "dense", particles=130, horizon=8, seed=1503),
    # 6. the hashed child table; collision avoidance's true dynamics
    # (a horizon of 12: at 8 hardly any episode on the 5 x 5 grid reaches its goal, and every slot would sit at the same t)
    case("planning_gridworld5_importance_hashed_children", "gridworld", POMDP, IS, "dense", size=5, particles=120, horizon=12, seed=1601),
    case("planning_random_collision_avoidance_5x3x2", "random-collision-avoidance", POMDP, IS, "dense", width=5, height=3, size=2,
         particles=100, horizon=8, seed=1602),
    # 7. gridworld FBA-POMDP history records, importance filter: search_hist2_kernel in lock-step
    case("fbapomdp_gridworld3_history_importance", "gridworld", FACT, IS, "history", size=3, particles=64, seed=1701, **GW),
    # (the oracle needs half a minute for the 337 runs at size 5 -- dense 5 x 5 count tables -- so SAMPLE_RUNS of them are compared)
    case("fbapomdp_gridworld5_history_importance", "gridworld", FACT, IS, "history", sample=True, size=5, particles=130, structure_prior=2,
         horizon=10, seed=1702),
    case("fbapomdp_gridworld3_history_importance_budget37", "gridworld", FACT, IS, "history", size=3, particles=96, search_budget=37,
         seed=1703, **GW),
    case("fbapomdp_gridworld3_history_importance_tight_buckets", "gridworld", FACT, IS, "history", size=3, particles=64, tree_buckets=66,
         seed=1704, **GW),
    case("fbapomdp_gridworld3_history_importance_no_lockstep", "gridworld", FACT, IS, "history", env={"FBA_HIST_LOCKSTEP": "0"}, size=3,
         particles=64, seed=1705, **GW),
    # (a horizon of 36: four waves' paths no longer fit 64 KB, so a workgroup holds two waves -- test_deep_horizon_geometry)
    case("fbapomdp_gridworld3_history_importance_two_waves_per_workgroup", "gridworld", FACT, IS, "history", size=3, particles=64, sims=4,
         structure_prior=2, horizon=36, seed=1706),
    # 8. the same records under the plain rejection filter: hist2_flat_search, reject_hist_kernel
    case("fbapomdp_gridworld3_history_rejection", "gridworld", FACT, REJ, "history", size=3, particles=64, seed=1801, **GW),
    case("fbapomdp_gridworld4_history_rejection", "gridworld", FACT, REJ, "history", size=4, particles=80, seed=1802, **GW),
    # 9. tabular gridworld BA-POMDP history records: search_tabhist_kernel under both filters
    case("bapomdp_gridworld3_table_history_importance", "gridworld", TABLE, IS, "history", size=3, particles=64, horizon=7, seed=1901),
    case("bapomdp_gridworld3_table_history_rejection", "gridworld", TABLE, REJ, "history", size=3, particles=64, horizon=7, seed=1902),
    # 10. collision avoidance on dense records: the factored prior with and without edge noise, the table prior
    case("fbapomdp_collision_avoidance_4x3x1_dense", "random-collision-avoidance", FACT, IS, "dense", structure_prior=0, particles=48,
         seed=2001, **CA431),
    case("fbapomdp_collision_avoidance_4x3x1_dense_uniform_structure", "random-collision-avoidance", FACT, IS, "dense", structure_prior=1,
         particles=48, seed=2002, **CA431),
    case("bapomdp_collision_avoidance_4x3x1_table_prior", "random-collision-avoidance", TABLE, IS, "dense", particles=48, noise=0.1,
         counts_total=500.0, seed=2003, **CA431),
    # 11. collision-avoidance history records: search_ca_hist_kernel, the multi-launch filter walking chunks of slots
    case("fbapomdp_collision_avoidance_4x3x1_history", "random-collision-avoidance", FACT, IS, "history", env=MULTI_ENV, particles=130,
         seed=2101, **CA431),
    case("fbapomdp_collision_avoidance_5x5x2_history", "random-collision-avoidance", FACT, IS, "history", env=MULTI_ENV, width=5, height=5,
         size=2, particles=64, horizon=7, seed=2102),
    # (chunks of 64, 64 and 22 slots)
    case("fbapomdp_collision_avoidance_4x3x1_history_scratch_slots_64", "random-collision-avoidance", FACT, IS, "history",
         env={**MULTI_ENV, "FBA_SCRATCH_SLOTS": "64"}, particles=96, seed=2103, **CA431),
    # 12. the expensive beliefs and the other planners, at the sizes of their small tests, in 70 slots
    case("fbapomdp_reinvigoration_factored_tiger", "episodic-factored-tiger", FACT, "reinvigoration", "dense", E=NARROW, size=3,
         structure_prior=2, resample_amount=8, particles=96, horizon=8, seed=2201),
    case("fbapomdp_cheating_reinvigoration", "episodic-factored-tiger", FACT, "cheating-reinvigoration", "dense", E=NARROW, size=3,
         structure_prior=1, threshold=-1.5, resample_amount=7, particles=48, horizon=8, seed=2202),
    case("fbapomdp_incubator", "episodic-factored-tiger", FACT, "incubator", "dense", E=NARROW, size=2, structure_prior=2, particles=48,
         resample_amount=6, threshold=0.5, horizon=8, seed=2203),
    case("fbapomdp_mh_within_gibbs", "episodic-factored-tiger", FACT, "mh-within-gibbs", "dense", E=NARROW, size=2, structure_prior=1,
         threshold=-0.5, belief_option=0, particles=48, horizon=8, seed=2204),
    case("bapomdp_nested", "episodic-tiger", TABLE, "nested", "dense", E=NARROW, particles=12, horizon=8, seed=2205),
    # (a point estimate is certain of the tiger's door and opens it at once, and elsewhere one wrong state may never reproduce an
    #  observation: sysadmin, as in the belief's small tests)
    case("fbapomdp_point_estimate", "linear-sysadmin", FACT, "point_estimate", "dense", E=NARROW, size=3, particles=50, horizon=6, seed=2206),
    # (the importance filter keeps history records under every planner)
    case("fbapomdp_thompson_sampling_planner", "gridworld", FACT, IS, "history", E=NARROW, planner="ts", size=3, structure_prior=2,
         particles=64, horizon=8, seed=2207),
    case("planning_random_planner", "episodic-tiger", POMDP, REJ, "dense", E=NARROW, planner="random", particles=48, sims=10, horizon=8,
         seed=2208),
    case("bapomdp_tiger_regular_dirichlet", "episodic-tiger", TABLE, REJ, "dense", E=NARROW, dirichlet_regular=1, particles=60, horizon=8,
         seed=2209),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def expected_particle_bytes(c, ncnt):
    kw = c["kw"]
    if c["fmt"] == "history":
        return record_bytes(kw["episodes"], kw["horizon"])
    if c["fmt"] == "packed_tiger":
        return 64
    if c["fmt"] == "packed_ftiger":
        return packed_ftiger_bytes(kw["size"])
    return dense_bytes(ncnt)


def sample_runs(c):
    """The runs compared where the whole experiment is too long for the oracle: the first slot, both sides of lane 23 | 24 (all that the
    other tests reach), of the wave boundary 63 | 64, the last slot and the first run of the second and third round, and the last run.
    (A case that brings its own list under "sample_runs" has those compared: tests/far_slot_cases.py.)"""
    if "sample_runs" in c:
        return sorted(set(c["sample_runs"]))
    E, runs = c["E"], c["runs"]
    return sorted({0, 23, 24, 63, 64, 65, E - 1, E, 2 * E - 1, 2 * E, runs - 1})


def min_distinct_lengths(c):
    """How many distinct episode lengths an experiment must show, so that the slots of a wave sit at different t.  Three, except where the
    domain fixes the length: no terminal state at all (NEVER_TERMINAL: every episode lasts the horizon), and collision avoidance, whose
    plane flies one column per step from column W - 1 and ends at column 0 or by a crash in one of the n obstacle columns before it --
    n possible lengths, W - n .. W - 1 (one for a single obstacle)."""
    if c["domain"] in NEVER_TERMINAL:
        return 1
    if "collision-avoidance" in c["domain"]:
        return min(3, c["kw"]["size"])
    return 3


def make_oracle(c, **over):
    kw = {k: v for k, v in c["kw"].items() if k not in ENGINE_ONLY and k != "seed"}
    if "planner" in kw:
        kw["planner"] = PLANNER[kw["planner"]]
    if c["domain"] == "centered-collision-avoidance":
        kw["ca_centered"] = 1
    kw.update(over)
    return orc.Oracle(domain=DOM[c["domain"]], model=c["model"], belief=BELIEF[c["belief"]], rng_mode=orc.RNG_PHILOX, arith=orc.ARITH_DEV,
                      philox_seed=c["kw"]["seed"], trace=1, **kw)


def _run(o, ba):
    if ba:
        stats, res = o.run_bapomdp()
    else:
        st, res = o.run_planning()
        stats = [st]
    return o.trace(res.n_trace), [(s.count, s.mean, s.m2) for s in stats], (res.sim_steps, res.belief_steps, res.env_steps)


def returns_of_trace(tr, runs, episodes, discount):
    """Per-run, per-episode return and length from trace records, with the operations of episode::run in their order
    (ret += r * disc; disc *= discount, in fp64): bit for bit what the experiment added to its statistics."""
    ret = np.zeros((runs, episodes), np.float64)
    ln = np.zeros((runs, episodes), np.int32)
    disc = np.ones((runs, episodes), np.float64)
    for run, ep, r in zip(tr["run"].tolist(), tr["episode"].tolist(), tr["reward"].tolist()):
        ret[run, ep] += r * disc[run, ep]
        disc[run, ep] *= discount
        ln[run, ep] += 1
    return ret, ln


def oracle_side(c, whole=False):
    """The experiment on the oracle: trace, per-run returns and lengths, and -- for a whole experiment -- per-episode (count, mean, m2)
    and counters.  A sampled case runs sample_runs(c) one by one (run_offset = r, runs = 1: the oracle's run r by offset is run r of the
    whole experiment, field for field) and has no statistics; `whole` runs everything all the same (for measuring, without a GPU)."""
    ba = c["model"] != POMDP
    if c["sample"] and not whole:
        traces = [_run(make_oracle(c, runs=1, run_offset=r), ba)[0] for r in sample_runs(c)]
        tr, stats, counters = np.concatenate(traces), None, None
    else:
        tr, stats, counters = _run(make_oracle(c, runs=c["runs"]), ba)
    cfg = orc.make_config(**{k: v for k, v in c["kw"].items() if k in ("episodes", "discount")})
    ret, ln = returns_of_trace(tr, c["runs"], cfg.episodes, cfg.discount)
    return dict(trace=tr, stats=stats, counters=counters, returns=ret, lengths=ln)


def engine_side(c, fba, check=None, after=None):
    """The same experiment on the engine, in E slots; the caller has set c["env"].  `check` sees the context before anything runs,
    `after` once everything has run and before the context is closed."""
    eng = fba.Engine(c["domain"], model=c["model"], belief=c["belief"], slots=c["E"], runs=c["runs"], trace=1, **c["kw"])
    assert eng.slots == c["E"]
    assert eng.particle_bytes == expected_particle_bytes(c, eng.ncnt), (eng.particle_bytes, eng.ncnt)
    if check:
        check(eng)
    stats = eng.run_bapomdp() if c["model"] != POMDP else [eng.run_planning()]
    cn = eng.counters()
    ret, ln = eng.returns()
    out = dict(trace=eng.trace(), stats=[(s.count, s.mean, s.m2) for s in stats], counters=(cn.sim_steps, cn.belief_steps, cn.env_steps),
               returns=ret, lengths=ln)
    if after:
        after(eng)
    eng.close()
    return out


def assert_same_experiment(c, got, ref):
    """every trace field, statistic, counter and per-run return and length of the engine's experiment is the oracle's, bit for bit"""
    tr, otr = got["trace"], ref["trace"]
    if c["sample"]:
        runs = sample_runs(c)
        tr = tr[np.isin(tr["run"], runs)]
    else:
        runs = np.arange(c["runs"])
    assert len(tr) == len(otr) > 0
    for name in tr.dtype.names:
        bad = np.nonzero(~np.all((tr[name] == otr[name]).reshape(len(tr), -1), axis=1))[0]
        assert bad.size == 0, f"{name}: first mismatch at record {bad[0]}: {tr[bad[0]]} vs {otr[bad[0]]}"
    if not c["sample"]:
        assert got["stats"] == ref["stats"]
        assert got["counters"] == ref["counters"]
    assert np.array_equal(got["lengths"][runs], ref["lengths"][runs])
    assert np.array_equal(got["returns"][runs].view(np.uint64), ref["returns"][runs].view(np.uint64))
