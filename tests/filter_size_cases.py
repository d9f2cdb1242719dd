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

A case makes runs = E + 1 (or E + 2) runs in E slots: one slot (two) is initialised a second time at this N, the others are inactive in the
last round.  SWITCHES names, for every family of cases, the switch-overs that its kernels have; tests/test_gpu_filter_sizes.py reads the
thresholds out of the sources and asserts that the family has a case on each side of each."""
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
}

CASES = []


def add(family, counts, domain, model, belief, fmt, E=3, more=1, env=None, seed0=3000, **kw):
    """one case per particle count; fmt: the record format, or {N: format} where fba_create changes it with N"""
    kw.setdefault("sims", 8)
    kw.setdefault("horizon", 4)
    if model != POMDP:
        kw.setdefault("episodes", 2)         # (the importance filter's reset_kernel and reset_hist_flat_kernel run between the two)
    for n in counts:
        f = fmt if isinstance(fmt, str) else fmt.get(n, fmt.get(None))
        c = W.case(f"{family}_{n}", domain, model, belief, f, E=E, runs=E + more, env=env, particles=n, seed=seed0 + len(CASES), **kw)
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

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert {c["family"] for c in CASES} == set(SWITCHES)


def counts_of(family):
    return sorted(c["kw"]["particles"] for c in CASES if c["family"] == family)


def cheapest_of(family):
    """the family's case of the fewest particles: what the oracle does there is cheapest"""
    return min((c for c in CASES if c["family"] == family), key=lambda c: c["kw"]["particles"])


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
