"""The case table, the schedule and the oracle's side of tests/test_gpu_per_call_wide.py.

Part 1 drives the per-call half of the C-ABI -- fba_set_position, fba_select_action(hist_len, active), fba_belief_update(action, obs,
active), fba_belief_reset_domain_state, fba_belief_get*, fba_last_step_info -- in E = 70 slots (one full wave of lane-per-tree searches
and 6 more lanes; four waves of 16 four-lane trees and 6 more trees) against E independent oracles, with what no experiment gives a
kernel: masks chosen by the host, neighbouring slots at unrelated (run, episode, t), history records of different lengths side by side,
and actions the planner would not pick.  `drive(c)` makes the oracle's calls and, given an engine, the engine's beside them, comparing
after every call; without an engine it needs no GPU, so the schedule's own properties are checked on the CPU (its return value).

The schedule of a case is a function of the case alone (numpy's default_rng(seed) and the oracle), never of engine output:

* slot e sits at run RUN[e] -- distinct ids that are neither e nor monotone in e, some above 65 535, two exactly E apart --, at episode
  0 or 1 and starts at t0[e] in {0, 1, 2}; t moves per slot, by one with every belief update of that slot, and hist_len = t;
* a hidden true state per slot on the oracle's side (env_start / env_step on the streams of episode::run) supplies an observation the
  filter can produce; the update takes the planner's action in even rounds and an action the host draws uniformly in odd ones; a
  terminal hidden step is not followed by an update (Episode.cpp:47-50) and takes the slot out of every later mask until the reset;
* six rounds of set_position, select_action(search mask), belief_update(update mask).  The two masks of an odd round are drawn
  independently; in an even round they are one mask (none, the slots >= 64, all zero), since the update there takes the action the
  search of that round planned.  0 no mask (NULL), 1 random (about 60 %), 2 only slots >= 64 (the first wave of lanes and all four
  full waves of quads wholly inactive), 3 exactly one slot below 64 (in a random order of them, the first still in its episode and,
  for the update, the first whose hidden step with its host-drawn action does not end the episode, so that the update mask holds one
  slot and not none), 4 the all-zero mask, 5 random: every slot round 1 left out, and a third of the others -- so that every slot
  is drawn into two of the masks of rounds 0, 1 and 5, of either kind;
* between rounds 3 and 4 the episode index goes up by one, t returns to 0 and every slot is reset: fba_belief_reset_domain_state in
  the Bayes-adaptive cases (beliefs::resetDomainStateDistribution at the start of an episode, BAPOMDPExperiment.cpp:44-75), and
  fba_belief_init in the planning ones (whose experiment initiates the belief per run, PlanningExperiment.cpp:39-52), at run + E.

Initiation belongs to the run and draws at (run, 0, 0), a reset at t = 0 of its episode, on both sides (init_kernel and reset_state
take these positions whatever the slot's episode and t are; orc_run_planning and orc_run_bapomdp set them).

Part 2 (ticks_*) is the oracle's side of fba_run_ticks: which (run, episode, t) every slot has reached after T ticks."""
import functools

import numpy as np

import wide_launch_cases as W
from oracle import pyorc as orc
from wide_launch_cases import DENSE_ENV, FACT, IS, MULTI_ENV, POMDP, REJ, TABLE

E = 70
ROUNDS = 6
RESET_BEFORE = 4
WEIGHTED = ("importance_sampling", "cheating-reinvigoration", "mh-within-gibbs", "nested")


def case(name, domain, model, belief, fmt, env=None, **kw):
    return W.case(name, domain, model, belief, fmt, E=E, runs=1, env=env, **kw)


GW = dict(size=3, structure_prior=2, horizon=7)
CA431 = dict(width=4, height=3, size=1, horizon=6)

# The tiger cases but the first run on the continuous variants: on the episodic ones two of three host-drawn actions open a door and end
# the episode, so most slots would leave the masks after a single update.  The first case keeps the episodic planning problem and with
# it slots that stay out of every later mask; slots that end an episode and come back at the reset are collision avoidance's (the plane's
# third step is its last).  Every seed but the first case's is the first one tried: no case made an oracle refuse an update.
CASES = [
    # (seed 3110, the tenth tried: under 3101..3109 each of the slots >= 64 still in its episode opens a door in round 2, whose update
    #  mask is then empty; no seed made an oracle refuse)
    case("planning_episodic_tiger_rejection", "episodic-tiger", POMDP, REJ, "dense", particles=64, horizon=8, seed=3110),
    case("planning_continuous_tiger_importance", "continuous-tiger", POMDP, IS, "dense", particles=100, horizon=8, seed=3102),
    case("bapomdp_tiger_packed_rejection", "continuous-tiger", TABLE, REJ, "packed_tiger", particles=64, horizon=8, seed=3201),
    case("bapomdp_tiger_packed_importance", "continuous-tiger", TABLE, IS, "packed_tiger", particles=130, horizon=8, seed=3202),
    case("bapomdp_tiger_dense_rejection", "continuous-tiger", TABLE, REJ, "dense", env=DENSE_ENV, particles=64, horizon=8, seed=3203),
    case("fbapomdp_factored_tiger3_packed_rejection", "continuous-factored-tiger", FACT, REJ, "packed_ftiger", size=3, structure_prior=2,
         particles=96, horizon=8, seed=3301),
    case("fbapomdp_factored_tiger2_importance", "continuous-factored-tiger", FACT, IS, "dense", size=2, structure_prior=2, particles=130,
         horizon=8, seed=3302),
    case("fbapomdp_linear_sysadmin5_rejection", "linear-sysadmin", FACT, REJ, "dense", size=5, particles=80, horizon=8, seed=3401),
    case("fbapomdp_gridworld3_history_importance", "gridworld", FACT, IS, "history", particles=64, seed=3701, **GW),
    case("fbapomdp_gridworld3_history_importance_no_lockstep", "gridworld", FACT, IS, "history", env={"FBA_HIST_LOCKSTEP": "0"},
         particles=64, seed=3702, **GW),
    case("fbapomdp_gridworld3_history_rejection", "gridworld", FACT, REJ, "history", particles=64, seed=3801, **GW),
    case("bapomdp_gridworld3_table_history_importance", "gridworld", TABLE, IS, "history", size=3, particles=64, horizon=7, seed=3901),
    case("bapomdp_gridworld3_table_history_rejection", "gridworld", TABLE, REJ, "history", size=3, particles=64, horizon=7, seed=3902),
    case("fbapomdp_collision_avoidance_4x3x1_dense_importance", "random-collision-avoidance", FACT, IS, "dense", structure_prior=0,
         particles=64, seed=4001, **CA431),
    case("fbapomdp_collision_avoidance_4x3x1_history", "random-collision-avoidance", FACT, IS, "history", env=MULTI_ENV, particles=130,
         seed=4101, **CA431),
    # (chunks of 64 and 6 slots)
    case("fbapomdp_collision_avoidance_4x3x1_history_scratch_slots_64", "random-collision-avoidance", FACT, IS, "history",
         env={**MULTI_ENV, "FBA_SCRATCH_SLOTS": "64"}, particles=96, seed=4102, **CA431),
    case("fbapomdp_reinvigoration_factored_tiger", "continuous-factored-tiger", FACT, "reinvigoration", "dense", size=3, structure_prior=2,
         resample_amount=8, particles=96, horizon=8, seed=4201),
    case("fbapomdp_cheating_reinvigoration_factored_tiger", "continuous-factored-tiger", FACT, "cheating-reinvigoration", "dense", size=3,
         structure_prior=1, threshold=-1.5, resample_amount=7, particles=64, horizon=8, seed=4202),
    case("planning_random_planner", "continuous-tiger", POMDP, REJ, "dense", planner="random", particles=64, sims=10, horizon=8, seed=4301),
    case("fbapomdp_thompson_sampling_planner", "gridworld", FACT, IS, "history", planner="ts", size=3, structure_prior=2, particles=64,
         horizon=8, seed=4302),
    case("fbapomdp_incubator", "continuous-factored-tiger", FACT, "incubator", "dense", size=2, structure_prior=2, particles=64,
         resample_amount=6, threshold=0.5, horizon=8, seed=4401),
    case("bapomdp_nested", "continuous-tiger", TABLE, "nested", "dense", particles=12, horizon=8, seed=4402),
    case("fbapomdp_point_estimate", "linear-sysadmin", FACT, "point_estimate", "dense", size=3, particles=50, horizon=8, seed=4403),
    case("fbapomdp_mh_within_gibbs", "continuous-factored-tiger", FACT, "mh-within-gibbs", "dense", size=2, structure_prior=1,
         threshold=-0.5, belief_option=0, particles=64, horizon=8, seed=4404),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def _draws(seed):
    """everything the host draws for a case: positions, masks, the order in which round 3 looks for its one slot, actions (as u01)"""
    g = np.random.default_rng(seed)
    run = g.choice(200000, E, replace=False).astype(np.int64)
    hi, a, b = g.choice(E, 3, replace=False)
    if not np.any(run > 65535):
        run[hi] += 65536
    run[b] = run[a] + E                                        # two ids exactly E apart
    assert len(set(run.tolist())) == E
    d = dict(run=run.astype(np.int32), episode=g.integers(0, 2, E).astype(np.int32), t0=g.integers(0, 3, E).astype(np.int32))
    first = {k: g.random(E) < 0.6 for k in ("search", "update")}
    last = {k: ~first[k] | (g.random(E) < 1 / 3) for k in ("search", "update")}
    tail = np.arange(E) >= 64
    d["order3"] = {k: g.permutation(64) for k in ("search", "update")}
    d["masks"] = {k: [np.ones(E, bool), first[k], tail, None, np.zeros(E, bool), last[k]] for k in ("search", "update")}
    d["u_action"] = g.random((ROUNDS, E))
    return d


def positions(c):
    d = _draws(c["kw"]["seed"])
    return d["run"], d["episode"], d["t0"]


def _same_particles(got, ref, what, e):
    for name, g, r in zip(("states", "weights", "counts"), got, ref):
        if g is None or r is None:
            continue
        view = np.uint64 if g.dtype == np.float64 else np.uint32
        assert np.array_equal(g.view(view), r.view(view)), f"{what}: {name} of slot {e} differ from the oracle's"


class _Pair:
    """the E oracles of a case and, when there is one, the engine beside them"""

    def __init__(self, c, eng):
        self.c, self.eng, self.L = c, eng, orc.lib()
        self.orcs = [W.make_oracle(c) for _ in range(E)]
        self.ba = c["model"] != POMDP
        self.belief = c["belief"]
        self.A = self.orcs[0].A

    def position(self, run, episode, t):
        for o, r, ep, tt in zip(self.orcs, run, episode, t):
            self.L.orc_rng_episode(o.rng, int(r), int(ep), int(tt))
        if self.eng:
            self.eng.set_position(run=run, episode=episode, t=t)

    def start(self, run, episode, initiate):
        """the belief of a new run (initiate) or of a new episode, and a new hidden state; leaves both sides at (run, episode, 0)"""
        zero = np.zeros(E, np.int32)
        if initiate:
            self.position(run, zero, zero)
            for o in self.orcs:
                o.belief_initiate()
            if self.eng:
                self.eng.belief_init()
        self.position(run, episode, zero)
        hidden = np.zeros(E, np.int32)
        for e, o in enumerate(self.orcs):
            if self.ba:
                o.belief_reset_domain_state()
            self.L.orc_rng_stream(o.rng, orc.PH_START, 0)
            hidden[e] = o.env_start()
        if self.eng and self.ba:
            self.eng.belief_reset_domain_state()
        return hidden

    def refused(self):
        return [(e, o.L.orc_error(o.h).decode()) for e, o in enumerate(self.orcs) if o.L.orc_error(o.h)]

    def compare_beliefs(self, what):
        if not self.eng:
            return
        eng, weighted = self.eng, self.belief in WEIGHTED
        for e, o in enumerate(self.orcs):
            s, w, cnt = eng.belief_get(e)
            os_, ow, ocnt = o.belief_get()
            _same_particles((s, w if weighted else None, cnt), (os_, ow, ocnt if o.ncnt else None), what, e)
            if self.belief in ("reinvigoration", "cheating-reinvigoration"):
                fs, fcnt = eng.belief_get_fully_connected(e)
                ofs, ofcnt = o.belief_get_fc()
                _same_particles((fs, None, fcnt), (ofs, None, ofcnt), what + ", second filter", e)
            if self.belief == "incubator":
                _same_particles(eng.belief_get_shadow(e), o.belief_get_shadow(), what + ", shadow filter", e)
            if self.belief == "nested":
                assert np.array_equal(eng.belief_get_nested(e), o.belief_get_nested()), f"{what}: flat filters of slot {e}"


def _mask_arg(mask):
    return None if mask.all() else mask.astype(np.uint8)


def drive(c, eng=None):
    """The schedule on E oracles and, beside them, on `eng` (the caller has set c["env"]), every result compared after every call.
    Returns what the schedule did, for test_the_schedule_covers_what_it_says."""
    d = _draws(c["kw"]["seed"])
    p = _Pair(c, eng)
    run, episode = d["run"].copy(), d["episode"].copy()
    hidden = p.start(run, episode, initiate=True)
    p.compare_beliefs("after initiation")
    t = d["t0"].copy()
    alive = np.ones(E, bool)
    out = dict(searches=np.zeros(E, int), updates=np.zeros(E, int), steps=np.zeros(E, int), entries=np.zeros(E, int), host_differs=0,
               search_masks=[], update_masks=[], entries_after_round_3=None, refused=[], zero_weight=[], null_masks=[])
    for rnd in range(ROUNDS):
        if rnd == RESET_BEFORE:
            episode, t = episode + 1, np.zeros(E, np.int32)
            if not p.ba:      # a planning belief is initiated per run: the slot's next one, E further (advance_kernel)
                run = run + E
                out["entries"][:] = 0
            hidden = p.start(run, episode, initiate=not p.ba)
            alive[:] = True
            p.compare_beliefs("after the reset")
        masks = {}
        for k in ("search", "update"):
            m = d["masks"][k][rnd]
            if m is None:     # round 3: one slot
                m = np.zeros(E, bool)
                m[[e for e in d["order3"][k] if alive[e]][:1]] = True
            masks[k] = m & alive
        p.position(run, episode, t)
        # ---- Planner::selectAction in the search mask
        sm = masks["search"]
        planned = np.full(E, -1, np.int32)
        recs = {}
        for e in np.nonzero(sm)[0]:
            planned[e], recs[e] = p.orcs[e].select_action(int(t[e]))
        out["searches"] += sm
        out["search_masks"].append(int(sm.sum()))
        if eng:
            before = eng.last_step_info()
            acts = eng.select_action(hist_len=t, active=_mask_arg(sm))
            info = eng.last_step_info()
            for e in range(E):
                if not sm[e]:
                    assert info[e].tobytes() == before[e].tobytes(), f"round {rnd}: the search changed the record of slot {e}, which it leaves out"
                    continue
                what = f"round {rnd}, search of slot {e} at (run, episode, t) = ({run[e]}, {episode[e]}, {t[e]})"
                assert acts[e] == planned[e], f"{what}: action {acts[e]}, the oracle's {planned[e]}"
                for name in ("root_n", "root_q", "n_nodes", "tree_depth"):
                    assert np.array_equal(info[e][name], recs[e][name]), f"{what}: {name} {info[e][name]}, the oracle's {recs[e][name]}"
            p.compare_beliefs(f"after the search of round {rnd}")
        # ---- the hidden step, then Belief::updateEstimation in the update mask unless that step was terminal
        um = masks["update"].copy()
        action = np.zeros(E, np.int32)
        obs = np.zeros(E, np.int32)

        def hidden_step(e, a):      # (a function of the slot's position, state and action: trying it changes nothing)
            p.L.orc_rng_stream(p.orcs[e].rng, orc.PH_ENV, 0)
            return p.orcs[e].env_step(int(hidden[e]), int(a))

        host_action = np.minimum((d["u_action"][rnd] * p.A).astype(np.int32), p.A - 1)
        if d["masks"]["update"][rnd] is None:      # round 3: the one slot is one whose step leaves it in its episode
            um[:] = False
            um[[e for e in d["order3"]["update"] if alive[e] and not hidden_step(e, host_action[e])[3]][:1]] = True
        for e in np.nonzero(um)[0]:
            if rnd % 2 == 0:
                assert sm[e], "an even round updates with the planner's action: its two masks are one"
                action[e] = planned[e]
            else:
                action[e] = host_action[e]
                out["host_differs"] += int(sm[e] and action[e] != planned[e])
            hidden[e], obs[e], _, term = hidden_step(e, action[e])
            out["steps"][e] += 1
            if term:
                alive[e] = um[e] = False
                action[e] = obs[e] = 0
        tot = {}
        for e in np.nonzero(um)[0]:
            o = p.orcs[e]
            if p.belief == IS:      # (is_update and is_resample are belief_update's two calls for this filter; the first returns the total)
                tot[e] = o.is_update(int(action[e]), int(obs[e]))
                o.is_resample()
                if not tot[e] > 0:
                    out["zero_weight"].append((rnd, int(e)))
            else:
                o.belief_update(int(action[e]), int(obs[e]))
        out["refused"] += [(rnd,) + r for r in p.refused()]
        out["updates"] += um
        out["entries"] += um
        out["update_masks"].append(int(um.sum()))
        out["null_masks"].append((bool(sm.all()), bool(um.all())))
        if eng:
            before = eng.last_step_info()
            states_before = [eng.belief_get(e) for e in range(E)] if not um.any() else None
            eng.belief_update(action, obs, active=_mask_arg(um))
            info = eng.last_step_info()
            p.compare_beliefs(f"after the update of round {rnd}")
            for e in range(E):
                if not um[e]:
                    assert info[e].tobytes() == before[e].tobytes(), f"round {rnd}: the update changed the record of slot {e}, which it leaves out"
                elif p.belief == IS:
                    assert info[e]["weight_total"].view(np.uint64) == np.float64(tot[e]).view(np.uint64), \
                        f"round {rnd}: weight_total of slot {e} is {info[e]['weight_total']!r}, the oracle's {tot[e]!r}"
                elif p.belief in (REJ, "reinvigoration"):
                    assert info[e]["update_count"] == p.L.orc_last_update_count(p.orcs[e].h), f"round {rnd}: update_count of slot {e}"
            if states_before is not None:      # the all-zero mask: nothing at all has changed
                for e in range(E):
                    _same_particles(eng.belief_get(e), states_before[e], f"round {rnd}, the all-zero mask", e)
        t = t + um
        if rnd == 3:
            out["entries_after_round_3"] = out["entries"].copy()
    out["drawn_into"] = {k: sum(d["masks"][k][r].astype(int) for r in (0, 1, 5)) for k in ("search", "update")}
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Part 2: fba_run_ticks.  With runs_total = -1 slot e makes runs e, e + E, e + 2 E, ... (advance_kernel) and, without a search budget,
# every tick is one real step of every slot: the lengths of the oracle's episodes say where each slot is after T ticks.
# ---------------------------------------------------------------------------------------------------------------------------------
TICK_ROUNDS = 4     # runs per slot on the oracle (4 E in all): three cover T ticks in the longer domains, the tiger's shortest runs need a fourth
TICK_CASES = [
    case("ticks_bapomdp_tiger_packed_rejection", "episodic-tiger", TABLE, REJ, "packed_tiger", particles=64, horizon=8, seed=5101),
    case("ticks_fbapomdp_gridworld3_history_importance", "gridworld", FACT, IS, "history", particles=64, seed=5102, **GW),
    # (two obstacles: with one every episode of the plane lasts W - 1 steps and all slots would roll over at the same tick)
    case("ticks_fbapomdp_collision_avoidance_5x5x2_history", "random-collision-avoidance", FACT, IS, "history", env=MULTI_ENV, width=5,
         height=5, size=2, particles=64, horizon=7, seed=5103),
    case("ticks_fbapomdp_gridworld3_history_importance_budget37", "gridworld", FACT, IS, "history", particles=64, search_budget=37,
         seed=5104, **GW),
]
TICKS_BY_NAME = {c["name"]: c for c in TICK_CASES}
SECOND_RUNS = 3     # at least so many slots finish their second run within T ticks (5 and 10 in the gridworld and collision-avoidance
                    # cases; 37 of 70 on the tiger, whose T = 7 is its longest first run, and 2 of them a third as well)


@functools.lru_cache(maxsize=None)
def ticks_oracle(name):
    """The oracle's experiment of TICK_ROUNDS * E runs: its trace, each record's simulated steps, per-episode returns and lengths; T, the least
    number of ticks after which every slot has finished its first run and at least SECOND_RUNS slots their second; and per slot and tick the
    index of the trace record that tick makes."""
    c = TICKS_BY_NAME[name]
    runs = TICK_ROUNDS * E
    o = W.make_oracle(c, runs=runs)
    _, res = o.run_bapomdp()
    tr, steps = o.trace(res.n_trace), o.trace_steps(res.n_trace)
    cfg = orc.make_config(**{k: v for k, v in c["kw"].items() if k in ("episodes", "discount")})
    ret, ln = W.returns_of_trace(tr, runs, cfg.episodes, cfg.discount)
    run_len = ln.sum(axis=1).reshape(TICK_ROUNDS, E)               # [k][e]: the length of run e + k E
    T = int(max(run_len[0].max(), np.sort(run_len[0] + run_len[1])[SECOND_RUNS - 1]))
    first = np.zeros(runs + 1, np.int64)                           # the first trace record of every run (the trace is in run order)
    first[1:] = np.cumsum(ln.sum(axis=1))
    assert np.array_equal(tr["run"][first[:-1]], np.arange(runs)) and first[-1] == len(tr)
    return dict(trace=tr, steps=steps, returns=ret, lengths=ln, run_len=run_len, T=T, first=first, episodes=cfg.episodes)


def slot_records(ref, e):
    """the indices of the trace records slot e makes, in its order: runs e, e + E, e + 2 E, e + 3 E"""
    return np.concatenate([np.arange(ref["first"][e + k * E], ref["first"][e + k * E + 1]) for k in range(TICK_ROUNDS)])


def ticks_records(ref, ticks):
    """per slot, the indices of the trace records of its first `ticks` ticks"""
    out = [slot_records(ref, e)[:ticks] for e in range(E)]
    assert all(len(idx) == ticks for idx in out), "TICK_ROUNDS runs per slot do not fill the ticks"
    return out


def ticks_return_sums(ref, ticks):
    """{n, sum ret, sum ret^2} over the episodes finished within `ticks` ticks, added as the engine adds them: per slot in episode
    order (env_kernel), then over slots in slot order (fba_get_return_sums)"""
    total = np.zeros(3, np.float64)
    for e in range(E):
        mine, done = np.zeros(3, np.float64), 0
        for k in range(TICK_ROUNDS):
            for ep in range(ref["episodes"]):
                done += int(ref["lengths"][e + k * E, ep])
                if done <= ticks:
                    r = np.float64(ref["returns"][e + k * E, ep])
                    mine += np.array([1.0, r, r * r])
        total += mine
    return total
