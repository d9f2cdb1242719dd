"""The per-call half of the C-ABI and the timed driver against the oracle, in 70 slots (tests/per_call_cases.py: the cases, the schedule,
the oracle's side).

Part 1: fba_set_position / fba_select_action(hist_len, active) / fba_belief_update(action, obs, active) /
fba_belief_reset_domain_state under masks the host chooses -- none, random, a whole wave and four whole waves of quads inactive, one
slot, all zero --, with neighbouring slots at unrelated (run, episode, t), history records of different lengths side by side and actions
the planner would not pick.  After every call every slot, masked in or not, must hold what its own oracle holds, bit for bit, and a
slot left out must keep its last-step record byte for byte.

Part 2: fba_run_ticks (runs_total = -1: what bench.py times) must make the steps the oracle's experiment makes."""
import numpy as np
import pytest

import fba_pomdp_amd as fba
import per_call_cases as PC
import wide_launch_cases as W

# (the one case whose domain lets the host end an episode with two actions of three: see test_the_schedule_covers_what_it_says)
EPISODIC = "planning_episodic_tiger_rejection"


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in PC.CASES])
def test_per_call_interface_equals_the_oracle_in_masked_slots(name, monkeypatch):
    c = PC.BY_NAME[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    eng = fba.Engine(c["domain"], model=c["model"], belief=c["belief"], slots=PC.E, **c["kw"])
    assert eng.slots == PC.E
    assert eng.particle_bytes == W.expected_particle_bytes(c, eng.ncnt), (eng.particle_bytes, eng.ncnt)
    try:
        out = PC.drive(c, eng)
    finally:
        eng.close()
    assert not out["refused"] and not out["zero_weight"], (out["refused"], out["zero_weight"])
    print(f"{name}: searched {out['search_masks']}, updated {out['update_masks']} slots per round")


def test_the_schedule_covers_what_it_says():
    """The conditions on the schedule, from the oracle's side alone (no GPU).  Three of them hold in a narrower form than one would
    first write down, each for a reason the domain gives:

    * "every slot is updated at least twice" holds in every case but planning on the episodic tiger: there two of three host-drawn
      actions (and, at the flat prior and 64 simulations, a third of the planner's) open a door, a terminal step is not followed by an
      update (Episode.cpp:47-50) and a planning belief is never reset.  That case asserts that every slot is drawn into two update
      masks, takes a hidden step, and that 8 slots or more are updated twice; its slots that ended their episode stay out of every
      mask until the belief is initiated again, which is the property it is there for.
    * "every non-empty mask has at least 8 active slots" is asserted for rounds 0, 1 and 5; round 2 is the slots >= 64, six at most by
      its definition, and round 3 one slot.
    * "after round 3 the entry counts of history records span three values" holds for gridworld (1, 2, 3); on the 4 x 3 collision
      avoidance grid the plane's third step is its last, so a record has 1 or 2 entries before the reset and 2 or 3 after round 5:
      two lengths side by side are asserted there, at both points."""
    for c in PC.CASES:
        name = c["name"]
        run, episode, t0 = PC.positions(c)
        e = np.arange(PC.E)
        assert len(set(run.tolist())) == PC.E and not np.any(run == e) and np.any(np.diff(run) < 0) and np.any(np.diff(run) > 0), name
        assert np.any(run > 65535) and PC.E in (run[:, None] - run[None, :]), name
        assert set(episode.tolist()) == {0, 1} and set(t0.tolist()) == {0, 1, 2}, name
        out = PC.drive(c)
        assert not out["refused"] and not out["zero_weight"], (name, out["refused"], out["zero_weight"])
        assert out["drawn_into"]["search"].min() >= 2 and out["drawn_into"]["update"].min() >= 2, name
        assert out["steps"].min() >= 1, name
        if name == EPISODIC:
            assert np.sum(out["updates"] >= 2) >= 8 and np.sum(out["searches"] >= 2) >= 8, name
            assert out["updates"].min() == 0, "no slot ended its episode before its first update: the case no longer shows what it is for"
        else:
            assert out["searches"].min() >= 2 and out["updates"].min() >= 2, (name, out["searches"].min(), out["updates"].min())
            assert out["null_masks"][0] == (True, True), f"{name}: round 0 passes no mask"
        for k in ("search_masks", "update_masks"):
            sizes = out[k]
            assert len(sizes) == PC.ROUNDS and sizes[4] == 0 and sizes[3] == 1 and 1 <= sizes[2] <= PC.E - 64, (name, k, sizes)
            assert min(sizes[0], sizes[1], sizes[5]) >= 8, (name, k, sizes)
            assert sizes[1] < PC.E and sizes[5] < PC.E, (name, k, sizes)
        assert out["host_differs"] >= 1, name
        if c["fmt"] == "history":
            kw = c["kw"]
            assert W.expected_particle_bytes(c, 0) == W.record_bytes(kw["episodes"], kw["horizon"]), name
            assert max(out["updates"]) <= kw["episodes"] * kw["horizon"], name
            if "collision-avoidance" in c["domain"]:
                assert len(set(out["entries_after_round_3"].tolist())) >= 2 and len(set(out["entries"].tolist())) >= 2, name
            else:
                assert len(set(out["entries_after_round_3"].tolist())) >= 3, name
    names = set(PC.BY_NAME)
    assert {"fbapomdp_gridworld3_history_importance_no_lockstep", "fbapomdp_collision_avoidance_4x3x1_history_scratch_slots_64",
            "planning_random_planner", "fbapomdp_thompson_sampling_planner"} <= names


# ---------------------------------------------------------------------------------------------------------------------------------
# Part 2
# ---------------------------------------------------------------------------------------------------------------------------------
def _assert_ticks_property(ref):
    """every slot finishes its first run within T ticks, SECOND_RUNS slots or more (not all) a second one, none the fourth the oracle made"""
    T, run_len = ref["T"], ref["run_len"]
    second = int(np.sum(run_len[0] + run_len[1] <= T))
    assert np.all(run_len[0] <= T) and PC.SECOND_RUNS <= second < PC.E and np.all(run_len.sum(axis=0) > T), (T, second)
    assert np.any(run_len[0] < T), "every slot ends its first run at the same tick"


def _same_records(tr, otr, what):
    assert len(tr) == len(otr) > 0, f"{what}: {len(tr)} records, the oracle's {len(otr)}"
    for name in tr.dtype.names:
        bad = np.nonzero(~np.all((tr[name] == otr[name]).reshape(len(tr), -1), axis=1))[0]
        assert bad.size == 0, f"{what}, {name}: first mismatch at record {bad[0]}: {tr[bad[0]]} vs {otr[bad[0]]}"


def _by_key(tr):
    return tr[np.lexsort((tr["t"], tr["episode"], tr["run"]))]


def _engine(c):
    return fba.Engine(c["domain"], model=c["model"], belief=c["belief"], slots=PC.E, runs=1 << 20, trace=1, **c["kw"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in PC.TICK_CASES if "search_budget" not in c["kw"]])
def test_run_ticks_makes_the_oracles_steps(name, monkeypatch):
    c = PC.TICKS_BY_NAME[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    ref = PC.ticks_oracle(name)
    _assert_ticks_property(ref)
    T, kw = ref["T"], c["kw"]
    eng = _engine(c)
    assert eng.particle_bytes == W.expected_particle_bytes(c, eng.ncnt)
    eng.run_ticks(T)
    # the trace keeps room for one run's worth of records per slot (fba_run_ticks, ensure_trace), filled in tick order (flush_kernel):
    # every slot's first min(T, episodes * horizon) ticks, which cover its whole first run
    kept = min(T, kw["episodes"] * kw["horizon"])
    assert np.all(ref["run_len"][0] <= kept)
    tr = eng.trace()
    print(f"{name}: T = {T}, {len(tr)} records kept, first runs of {ref['run_len'][0].min()}..{ref['run_len'][0].max()} ticks, "
          f"{int(np.sum(ref['run_len'][0] + ref['run_len'][1] <= T))} slots finished a second run")
    assert len(tr) == PC.E * kept
    _same_records(tr, _by_key(ref["trace"][np.concatenate(PC.ticks_records(ref, kept))]), name)
    made = np.concatenate(PC.ticks_records(ref, T))
    cn = eng.counters()
    assert cn.env_steps == PC.E * T
    assert (cn.sim_steps, cn.belief_steps) == (int(ref["steps"][made, 0].sum()), int(ref["steps"][made, 1].sum()))
    assert np.array_equal(eng.return_sums().view(np.uint64), PC.ticks_return_sums(ref, T).view(np.uint64))
    assert eng.return_sums()[0] >= PC.E * kw["episodes"] + PC.SECOND_RUNS * kw["episodes"]
    # per-run returns exist for experiments of a known number of runs only: env_kernel skips returns[] when runs_total < 0, the driver
    # allocates none, and fba_get_returns refuses
    with pytest.raises(fba.FbaError, match="no experiment has been run on this ctx"):
        eng.returns()
    eng.close()


@pytest.mark.gpu
def test_run_ticks_with_a_search_budget_makes_the_oracles_steps():
    """slots advance on their own under a budget: the kept records -- the first E * episodes * horizon flushed -- are compared by key"""
    name = "ticks_fbapomdp_gridworld3_history_importance_budget37"
    c = PC.TICKS_BY_NAME[name]
    ref = PC.ticks_oracle(name)
    _assert_ticks_property(ref)
    T, kw = ref["T"], c["kw"]
    eng = _engine(c)
    eng.run_ticks(T)
    made = eng.counters().env_steps
    assert made >= PC.E * T
    tr = eng.trace()
    assert len(tr) == min(made, PC.E * kw["episodes"] * kw["horizon"])      # (every real step flushes one record)
    otr = ref["trace"]
    assert tr["run"].max() < PC.TICK_ROUNDS * PC.E
    key = lambda r: (r["run"].astype(np.int64) * 64 + r["episode"]) * 256 + r["t"]
    pos = np.searchsorted(key(otr), key(tr))          # (the oracle's trace is in key order)
    assert np.all(pos < len(otr)) and np.array_equal(key(otr)[pos], key(tr)), "a kept record is at a position the oracle never reaches"
    assert len(np.unique(key(tr))) == len(tr)
    _same_records(tr, otr[pos], name)
    for e in range(PC.E):                             # each slot's records are a prefix of its steps: nothing skipped
        mine = np.sort(pos[tr["run"] % PC.E == e])
        assert np.array_equal(mine, PC.slot_records(ref, e)[:len(mine)]), f"slot {e}"
    eng.close()


def test_the_tick_cases_reach_a_second_run():
    """T is derived from the oracle's episode lengths, not tuned: the property it is chosen for, on the CPU"""
    for c in PC.TICK_CASES:
        ref = PC.ticks_oracle(c["name"])
        _assert_ticks_property(ref)
        assert ref["steps"][:, 0].min() > 0 and ref["steps"][ref["trace"]["terminal"] == 0, 1].min() > 0
        n = PC.ticks_return_sums(ref, ref["T"])[0]
        assert n == sum(int(np.sum(np.cumsum(ref["lengths"][e::PC.E].ravel()) <= ref["T"])) for e in range(PC.E))
