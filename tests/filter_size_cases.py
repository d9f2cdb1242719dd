"""The case table of tests/test_gpu_filter_sizes.py: one small whole experiment on each side of every particle count at which the engine
takes another belief-filter kernel, another branch of one, or another record format -- with the oracle's side of it.

Every other oracle comparison of the suite fixes the particle count at a few hundred (or runs 4096 / 16384 inside a full-size workload);
here the slots are few (E = 3, or 2 at the largest filters), the search is 8 simulations and the horizon 4 to 6, and N is the subject:

    switch-over                                   where                                        what changes
    IS_LDS_MAX_N = 8192                           plan_importance_single                       weights and prefix sums in LDS or in HBM
    hist_all_draws_first = 16384                  importance_kernel<HIST>                      all draws first (16-bit sources in LDS) or by rounds
    hist_update_multi = 4096 (N >= 4096)          launch_belief_update, history records        one launch or seven
    IS_MAX_CHUNKS * 256 = 65536                   fba_create, launch_uniform_scan              one workgroup per slot or seven launches; the format
    CARRY_TILE = 2048 chunks (524 288 particles)  scan_carry_kernel                            a second LDS tile of the carry chain; its remainder loop
    TIGER_LDS_MAX_N = 4096                        launch_belief_update, packed tiger rejection reject_tiger_lds_kernel or reject_kernel<false, 2, 0, 512>
    PARTICLE_TILE = 4096                          init / reset / materialize grids             a second workgroup per slot
    256-element chunks, 4 per lane, 4 per block   the multi-launch filter                      ragged last lane, ragged last chunk, nchunks % 4
    N a power of two                              the history search's root sample             ceil(u N) - 1 or a search of the prefix sums
    REJECT_BLOCK = 256                            reject_kernel                                a second chunk of attempts
    a wave = 64                                   nested_fill_kernel / nested_update_kernel    a second wave of count particles (256: the workgroup)

The composite beliefs (reinvigoration, incubator, cheating-reinvigoration, the Metropolis-Hastings ones, nested) run these kernels on a
second or third filter and with passes of their own around them; their families end at the largest filter fba_create makes of them (CAPS)
and have their final filters compared as well (FILTERS).

A case makes runs = E + 1 (or E + 2) runs in E slots: one slot (two) is initialised a second time at this N, the others are inactive in the
last round.  SWITCHES names, for every family of cases, the switch-overs that its kernels have; tests/test_gpu_filter_sizes.py reads the
thresholds out of the sources and asserts that the family has a case on each side of each."""
import numpy as np

import wide_launch_cases as W
from wide_launch_cases import FACT, IS, POMDP, REJ, TABLE

CTIGER, CFTIGER, GRID, CA = "continuous-tiger", "continuous-factored-tiger", "gridworld", "random-collision-avoidance"
ONE_LAUNCH_ENV = {"FBA_HIST_MULTI": "0"}        # history records: the one-launch importance_kernel<HIST> at every N
# (five columns: the plane flies one column per step and the step into column 0 ends the episode, so W - 2 updates follow each other --
#  two on the 4 x 3 grid of the suite's other collision-avoidance cases, which cannot show three in a row)
CA531 = dict(width=5, height=3, size=1)

# family -> the switch-overs its filter has (the family's cases must hold both sides of each)
SWITCHES = {
    "is_tiger_packed": ("IS_LDS_MAX_N", "IS_MAX_CHUNKS", "PARTICLE_TILE"),
    "is_tiger_dense": ("IS_LDS_MAX_N", "IS_MAX_CHUNKS"),
    "is_generic_dense": ("IS_LDS_MAX_N", "IS_MAX_CHUNKS", "PARTICLE_TILE"),
    "is_regular_dirichlet": ("IS_MAX_CHUNKS",),                       # (never in LDS: plan_importance_single)
    "is_planning": ("IS_LDS_MAX_N", "IS_MAX_CHUNKS", "CARRY_TILE", "PARTICLE_TILE"),
    "is_gridworld_history": ("hist_update_multi", "IS_MAX_CHUNKS", "PARTICLE_TILE", "power_of_two"),
    "is_gridworld_history_one_launch": ("IS_LDS_MAX_N", "hist_all_draws_first", "power_of_two"),
    "is_table_gridworld_history": ("PARTICLE_TILE", "ragged_chunks"),
    "is_collision_avoidance_multi": ("ragged_chunks",),
    "is_collision_avoidance": ("IS_MAX_CHUNKS",),
    "rej_tiger_packed": ("TIGER_LDS_MAX_N", "PARTICLE_TILE", "REJECT_512"),
    "rej_factored_tiger_packed": ("PARTICLE_TILE", "REJECT_BLOCK"),
    "rej_generic_dense": ("PARTICLE_TILE", "REJECT_BLOCK"),
    "rej_gridworld_history": ("PARTICLE_TILE", "REJECT_BLOCK"),
    "rej_table_gridworld_history": ("PARTICLE_TILE", "REJECT_BLOCK"),
    # the composite beliefs: the same kernels with further filters and passes around them (CAPS: N beyond which fba_create refuses)
    "reinvig_factored_tiger": ("REJECT_BLOCK", "PARTICLE_TILE"),
    "reinvig_generic": ("REJECT_BLOCK", "PARTICLE_TILE"),
    "incubator_factored_tiger": ("REJECT_BLOCK", "PARTICLE_TILE", "INCUBATOR_MAX"),
    "incubator_collision_avoidance": ("REJECT_BLOCK", "PARTICLE_TILE"),
    "cheating_factored_tiger": ("REJECT_BLOCK", "PARTICLE_TILE", "IS_LDS_MAX_N", "CHEATING_MAX"),
    "mh_gibbs_messages": ("PARTICLE_TILE", "IS_LDS_MAX_N"),           # (MH_MAX: no case, see below)
    "mh_gibbs_rejection": ("PARTICLE_TILE", "IS_LDS_MAX_N"),
    "mh_nips": ("PARTICLE_TILE", "IS_LDS_MAX_N"),
    "nested_table": ("wave", "NESTED_MAX"),
    "nested_factored": ("wave",),
}
# the largest filter fba_create makes of a belief: a family that names one has a case at exactly that N (there is no other side to run)
CAPS = ("INCUBATOR_MAX", "CHEATING_MAX", "MH_MAX", "NESTED_MAX")
WAVE = 64

# family -> the filters beside belief_get that the engine and the oracle are compared in after the experiment, and whether belief_get's
# weights are part of the belief (tests/test_gpu_filter_sizes.py: final_filters).  belief_hash covers the main filter alone, and a
# particle of the second filter reaches the main one only when a breeding draw lands on it.
FILTERS = {
    "reinvig_factored_tiger": ("fully_connected",), "reinvig_generic": ("fully_connected",),
    "incubator_factored_tiger": ("fully_connected", "shadow"), "incubator_collision_avoidance": ("fully_connected", "shadow"),
    "cheating_factored_tiger": ("weights", "fully_connected"),
    "mh_gibbs_messages": ("weights",), "mh_gibbs_rejection": ("weights",), "mh_nips": ("weights",),
    "nested_table": ("weights", "nested"), "nested_factored": ("weights", "nested"),
}

CASES = []


def add(family, counts, domain, model, belief, fmt, E=3, more=1, env=None, seed0=3000, tag="", **kw):
    """one case per particle count; fmt: the record format, or {N: format} where fba_create changes it with N; tag: what tells the
    family's cases of one N apart"""
    kw.setdefault("sims", 8)
    kw.setdefault("horizon", 4)
    if model != POMDP:
        kw.setdefault("episodes", 2)         # (the importance filter's reset_kernel and reset_hist_flat_kernel run between the two)
    for n in counts:
        f = fmt if isinstance(fmt, str) else fmt.get(n, fmt.get(None))
        c = W.case(f"{family}_{tag}{n}", domain, model, belief, f, E=E, runs=E + more, env=env, particles=n, seed=seed0 + len(CASES), **kw)
        c["family"] = family
        CASES.append(c)


# ---- the importance filter
# tabular tiger BA-POMDP: packed records up to 65536 particles (importance_kernel<false, 2, false, WLDS>), dense beyond (the seven launches)
add("is_tiger_packed", (4096, 4097, 8192, 8193, 65535, 65536, 65537), CTIGER, TABLE, IS, {None: "packed_tiger", 65537: "dense"})
add("is_tiger_dense", (8192, 8193, 65536, 65537), CTIGER, TABLE, IS, "dense", env=W.DENSE_ENV)
# generic dense records (importance_kernel<false, 0, false, WLDS>, is_multi_step_kernel<false, false>)
add("is_generic_dense", (4096, 4097, 8192, 8193, 65536, 65537), CFTIGER, FACT, IS, "dense", size=2, structure_prior=2)
add("is_regular_dirichlet", (8191, 65536, 65537), CFTIGER, FACT, IS, "dense", size=2, structure_prior=2, dirichlet_regular=1)
# planning: 16-byte records, so the filters of half a million particles that reach the carry chain's second tile are cheap
add("is_planning", (4096, 4097, 8192, 8193, 65536, 65537), CTIGER, POMDP, IS, "dense")
# (2048 chunks exactly; 2050 chunks: the second tile holds 2, so only its remainder loop runs)
add("is_planning", (524288, 524547), CTIGER, POMDP, IS, "dense", E=2)
# gridworld FBA-POMDP history records: one launch below 4096 particles, seven from there, dense records beyond 65536
add("is_gridworld_history", (4095, 4096, 4097, 8192, 8193, 16384, 16385), GRID, FACT, IS, "history", size=3, structure_prior=2, horizon=5)
# (one episode: the oracle needs 9 s for these twelve real steps)
add("is_gridworld_history", (65535, 65536, 65537), GRID, FACT, IS, {None: "history", 65537: "dense"}, E=2, episodes=1, size=3,
    structure_prior=2)
# (the one-launch kernel is what a context without the scratch pool runs at every N: its own two switch-overs)
add("is_gridworld_history_one_launch", (8192, 8193, 16384, 16385), GRID, FACT, IS, "history", env=ONE_LAUNCH_ENV, size=3, structure_prior=2,
    horizon=5)
# tabular gridworld history records: always the seven launches.  1021: four chunks, the last ragged; 1281: six chunks, one ragged
add("is_table_gridworld_history", (255, 257, 1021, 1281, 4096, 4097), GRID, TABLE, IS, "history", size=3, horizon=5)
# collision-avoidance history records: the seven launches from FBA_IS_MULTI_MIN up, and at the real switch-over (dense | history)
add("is_collision_avoidance_multi", (257, 1021, 1281), CA, FACT, IS, "history", env=W.MULTI_ENV, horizon=6, **CA531)
add("is_collision_avoidance", (65536, 65537), CA, FACT, IS, {65536: "dense", 65537: "history"}, horizon=6, **CA531)

# ---- the rejection filter
add("rej_tiger_packed", (511, 512, 513, 4096, 4097), CTIGER, TABLE, REJ, "packed_tiger")
add("rej_factored_tiger_packed", (255, 256, 257, 4096, 4097), CFTIGER, FACT, REJ, "packed_ftiger", size=3, structure_prior=2)
add("rej_generic_dense", (256, 257, 4096, 4097), CFTIGER, FACT, REJ, "dense", env=W.DENSE_ENV, size=3, structure_prior=2)
add("rej_gridworld_history", (256, 257, 4096, 4097), GRID, FACT, REJ, "history", size=3, structure_prior=2, horizon=5)
add("rej_table_gridworld_history", (256, 257), GRID, TABLE, REJ, "history", size=3, horizon=5)
add("rej_table_gridworld_history", (4096, 4097), GRID, TABLE, REJ, "history", E=2, episodes=1, seed0=3300, size=3)     # (the oracle's slowest filter)

# ---- the composite beliefs: dense records throughout.  [seconds]: the family's cases together as measured, the oracle's experiment and
# its one run for the final filters | the engine's experiment on an MI355X, reading the filters back included
FT2 = dict(size=2, structure_prior=2)           # continuous factored tiger, two irrelevant features, match-uniform
# reinvigoration: reinvigorate_kernel, reject_kernel(fc = 1) on the fully connected filter, then fc = 0; init / reset twice  [0.2 | 0.1 s]
add("reinvig_factored_tiger", (255, 256, 257, 4096, 4097), CFTIGER, FACT, "reinvigoration", "dense", resample_amount=8, **FT2)
# (the generic instantiation of reject_kernel; reinvigorate_kernel's mutate draws are the domain's)  [1.3 | 0.7 s]
add("reinvig_generic", (256, 257, 4096, 4097), CA, FACT, "reinvigoration", "dense", tag="collision_avoidance_", structure_prior=1,
    resample_amount=8, horizon=6, **CA531)
add("reinvig_generic", (256, 257, 4096, 4097), "linear-sysadmin", FACT, "reinvigoration", "dense", tag="sysadmin_", size=3, resample_amount=8)
# incubator: the same, and a shadow filter with its own reset pass, its breeding (mode 1 or 2) and the one-launch importance_kernel on it;
# 8192 is the largest (weights in LDS at their largest size)  [factored tiger 0.5 | 0.4 s, collision avoidance 1.0 | 2.2 s]
add("incubator_factored_tiger", (256, 257, 4096, 4097, 8192), CFTIGER, FACT, "incubator", "dense", resample_amount=6, threshold=0.5, **FT2)
add("incubator_collision_avoidance", (256, 257, 4096, 4097), CA, FACT, "incubator", "dense", structure_prior=1, resample_amount=6,
    threshold=0.5, horizon=6, **CA531)
# cheating: reject_kernel(fc = 1) on the correct-graph filter, the importance filter, cheat_kernel; 65536 is the largest  [2.0 | 0.4 s]
add("cheating_factored_tiger", (256, 257, 4096, 4097, 8192, 8193), CFTIGER, FACT, "cheating-reinvigoration", "dense", size=2,
    structure_prior=1, threshold=-1.5, resample_amount=7)
add("cheating_factored_tiger", (65536,), CFTIGER, FACT, "cheating-reinvigoration", "dense", E=2, size=2, structure_prior=1, threshold=-1.5,
    resample_amount=7)
# Metropolis-Hastings: the importance filter, then mh_kernel -- one wave walking a chain of N accepts, so the larger pair is cut to two
# slots and one episode.  The largest filter (65536) has no case: nobody has measured one re-draw of that many particles on one wave;
# test_composite_belief_caps creates a context there.  [messages 4.1 | 21.3 s, rejection 1.1 | 19.6 s, mh-nips 0.9 | 13.7 s; the slowest
# case is mh_gibbs_rejection_4097 with 7.9 s on the GPU, the collision-avoidance pair takes 6 s each]
for fam, belief, option in (("mh_gibbs_messages", "mh-within-gibbs", 0), ("mh_gibbs_rejection", "mh-within-gibbs", 1), ("mh_nips", "mh-nips", 0)):
    # (mh-nips at 4096 | 4097 took 10 s a case on the GPU with two episodes, a third of a second per update: one episode there, 2.4 and
    #  3.2 s, which leaves four updates in a row)
    add(fam, (4096, 4097), CFTIGER, FACT, belief, "dense", episodes=1 if fam == "mh_nips" else 2, threshold=-1.0, belief_option=option, **FT2)
    add(fam, (8192, 8193), CFTIGER, FACT, belief, "dense", E=2, episodes=1, threshold=-1.0, belief_option=option, **FT2)
add("mh_gibbs_messages", (8192, 8193), CA, FACT, "mh-within-gibbs", "dense", E=2, episodes=1, tag="collision_avoidance_", structure_prior=2,
    threshold=-2.0, belief_option=0, horizon=6, **CA531)
# nested: one lane per count particle in one workgroup of 256, block_device_scan over N weights, N^2 domain states per particle.
# 64 | 65: a second wave; 256: the workgroup is full (about 1e5 sequential steps per lane and update: two slots, one episode, which the
# oracle needs 22 s for and the GPU 2.4 s)  [table 36.9 | 5.0 s, factored 3.5 | 2.5 s]
add("nested_table", (64, 65, 128, 129), CTIGER, TABLE, "nested", "dense")
add("nested_table", (256,), CTIGER, TABLE, "nested", "dense", E=2, episodes=1)
add("nested_factored", (64, 65), CFTIGER, FACT, "nested", "dense", **FT2)

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert {c["family"] for c in CASES} == set(SWITCHES) and set(FILTERS) <= set(SWITCHES)


def counts_of(family):
    return sorted(c["kw"]["particles"] for c in CASES if c["family"] == family)


def cheapest_of(family):
    """the family's case of the fewest particles: what the oracle does there is cheapest"""
    return min((c for c in CASES if c["family"] == family), key=lambda c: c["kw"]["particles"])


def engine_final_filters(c, eng):
    """(run, filters): the filters of the slot that the engine initialised a second time, as the experiment left them, and the run that
    slot held last (last_step_info names it)"""
    info = eng.last_step_info()
    e = int(np.argmax(info["run"]))
    assert info["run"][e] >= c["E"]             # (runs = E + 1: one slot took a run after its first)
    what = FILTERS[c["family"]]
    s, w, cnt = eng.belief_get(e)
    out = {"states": s, "counts": cnt}
    if "weights" in what:
        out["weights"] = w
    if "fully_connected" in what:
        out["fully connected states"], out["fully connected counts"] = eng.belief_get_fully_connected(e)
    if "shadow" in what:
        out["shadow states"], out["shadow weights"], out["shadow counts"] = eng.belief_get_shadow(e)
    if "nested" in what:
        out["flat filters"] = eng.belief_get_nested(e)
    return int(info["run"][e]), out


def oracle_final_filters(c, run):
    """the same filters after that run alone on the oracle (run_offset = r, runs = 1: run r of the whole experiment)"""
    o = W.make_oracle(c, runs=1, run_offset=run)
    o.run_bapomdp()
    what = FILTERS[c["family"]]
    s, w, cnt = o.belief_get()
    out = {"states": s, "counts": cnt}
    if "weights" in what:
        out["weights"] = w
    if "fully_connected" in what:
        out["fully connected states"], out["fully connected counts"] = o.belief_get_fc()
    if "shadow" in what:
        out["shadow states"], out["shadow weights"], out["shadow counts"] = o.belief_get_shadow()
    if "nested" in what:
        out["flat filters"] = o.belief_get_nested()
    return out


def assert_same_filters(name, run, got, ref):
    """bit for bit: states as int32, weights as the 64 bits of a double, counts as the 32 bits of a float"""
    assert list(got) == list(ref)
    for key, g in got.items():
        r = ref[key]
        assert g.shape == r.shape and g.dtype == r.dtype and g.size > 0, (name, key)
        view = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}.get(g.dtype, g.dtype)
        bad = np.nonzero(g.view(view).reshape(len(g), -1) != r.view(view).reshape(len(r), -1))[0]
        assert bad.size == 0, f"{name}, run {run}: {key} differ from the oracle's in {len(set(bad.tolist()))} particles, first {bad[0]}"


def longest_update_streak(trace):
    """the most belief updates that one slot made in a row: real steps that did not end their episode (a terminal step has no update),
    consecutive within one episode of one run"""
    best, run, key = 0, 0, None
    for r, ep, t, term in zip(trace["run"].tolist(), trace["episode"].tolist(), trace["t"].tolist(), trace["terminal"].tolist()):
        if (r, ep) != key:
            key, run = (r, ep), 0
        run = run + 1 if term == 0 else 0
        best = max(best, run)
    return best
