"""fba_giveup_policy / Engine.giveup_policy / Engine.retired: a run whose rejection update gives up is retired, reported and replaced in its
slot by the slot's next run, and the experiment finishes.

The yardstick is the oracle, which never gives up: tests/giveup_cases.py predicts from its trace alone what the engine must report under a
limit of max_attempts -- the retired list, every surviving record, returns, lengths, statistics, counters, the steps per bin -- and the
engine is held to that bit for bit.  tests/test_giveup_cpu.py shows, without a GPU, that every case retires some runs and keeps some."""
import numpy as np
import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N
import giveup_cases as G

pytestmark = pytest.mark.gpu

UNSPECIFIED = ("update_count", "weight_total", "belief_hash")      # of the record at which a run was retired


def _engine(c, policy="retire", max_attempts=None, **over):
    eng = fba.Engine(c["domain"], model=c["model"], belief=c["belief"], slots=c["E"], **dict(dict(c["kw"], runs=c["runs"], trace=1), **over))
    assert eng.slots == c["E"]
    if policy is not None:
        eng.giveup_policy(policy, c["max_attempts"] if max_attempts is None else max_attempts)
    return eng


def _retired(eng):
    r = eng.retired()
    assert r.seen == len(r)
    assert np.all(r["slot"] == r["run"] % eng.slots) and np.all(r["reserved"] == 0)
    return [tuple(int(x[f]) for f in G.RETIRED_FIELDS) for x in r]


def _check_trace(tr, otr, p):
    """the engine's records are the oracle's kept ones: the surviving ones in every field, those that gave up in all but three"""
    want = otr[p["keep"]]
    gave = p["gave"][p["keep"]]
    assert len(tr) == len(want)
    G.same_records(tr[~gave], want[~gave])
    G.same_records(tr[gave], want[gave], skip=UNSPECIFIED)
    assert np.all(tr["update_count"][gave] == N.UPDATE_GAVE_UP) and not np.any(tr["update_count"][~gave] == N.UPDATE_GAVE_UP)


def _counters(eng):
    cn = eng.counters()
    return (cn.sim_steps, cn.belief_steps, cn.env_steps)


def _check_experiment(eng, stats, c, p, otr, before=(0, 0, 0)):
    """before: the context's counters in front of the experiment (they count since fba_create)"""
    assert _retired(eng) == p["retired"]
    _check_trace(eng.trace(), otr, p)
    ret, ln = eng.returns()
    assert np.array_equal(ln, p["lengths"])
    assert np.array_equal(ret.view(np.uint64), p["returns"].view(np.uint64))
    assert [(s.count, s.mean, s.m2) for s in stats] == p["stats"]
    assert tuple(a - b for a, b in zip(_counters(eng), before)) == p["counters"]


@pytest.mark.parametrize("name", list(G.CASES))
def test_retired_runs_and_survivors_equal_the_prediction(name):
    c = G.CASES[name]
    otr, steps = G.oracle_run(c)
    p = G.predict(c, otr, steps)
    G.mix_conditions(c, p)
    eng = _engine(c)
    plan = G.update_plan(eng)      # the launch plan of this very context
    print(f"{name}: {plan}, {len(p['retired'])} of {c['runs']} runs to retire at {c['max_attempts']} attempts")
    assert plan == [c["kernel"]]
    eng.step_stats_enable()
    stats = eng.run_bapomdp()
    _check_experiment(eng, stats, c, p, otr)
    few = np.zeros(5, N.RETIRED_DTYPE)      # a short buffer gets the first records by run, whatever the order they were appended in
    assert eng.L.fba_get_retired(eng.h, few.ctypes.data, len(few)) == len(few)
    assert few["run"].tolist() == [r[0] for r in p["retired"][:len(few)]]
    assert "retired" in eng.device_arrays() and "gave_up" in eng.device_arrays()
    st = eng.step_stats()
    assert np.array_equal(st["steps"], p["steps"])
    gave_bins = np.zeros_like(p["steps"])
    for _, ep, t, _, _, _ in p["retired"]:
        gave_bins[ep, t] += 1
    non_terminal = p["steps"] - st["terminals"]
    assert np.array_equal(st["attempts_steps"], non_terminal - gave_bins)      # a given-up update is a step without an update_count
    sums = eng.return_sums()
    assert sums[0] == float(np.sum(p["lengths"] > 0))                          # void episodes are in no sum
    eng.close()


def test_composite_belief_retires_on_either_filter():
    """reinvigoration: the fully connected filter's update runs first and may give up too; its attempts are not in the trace, so a run is
    retired AT OR BEFORE the step its main filter's counts predict, and a run that is not retired is the oracle's"""
    c = G.COMPOSITE
    otr, steps = G.oracle_run(c)
    p = G.predict(c, otr, steps)
    when = {r[0]: (r[1], r[2]) for r in p["retired"]}
    eng = _engine(c)
    assert G.update_plan(eng) == c["kernel"]
    eng.run_bapomdp()
    tr, rec = eng.trace(), eng.retired()
    ret, ln = eng.returns()
    oret, oln = G.W.returns_of_trace(otr, c["runs"], c["kw"]["episodes"], 0.95)
    gone = {int(r["run"]): (int(r["episode"]), int(r["t"])) for r in rec}
    assert len(gone) == len(rec) >= len(when) and len(gone) < c["runs"]
    earlier = 0
    for run in range(c["runs"]):
        mine, theirs = tr[tr["run"] == run], otr[otr["run"] == run]
        if run not in gone:
            assert run not in when
            G.same_records(mine, theirs)
            assert np.array_equal(ln[run], oln[run]) and np.array_equal(ret[run].view(np.uint64), oret[run].view(np.uint64))
            continue
        assert gone[run] <= when.get(run, (1 << 30, 0))
        earlier += gone[run] != when.get(run)
        assert (int(mine["episode"][-1]), int(mine["t"][-1])) == gone[run] and mine["update_count"][-1] == N.UPDATE_GAVE_UP
        G.same_records(mine[:-1], theirs[:len(mine) - 1])
        G.same_records(mine[-1:], theirs[len(mine) - 1:len(mine)], skip=UNSPECIFIED)
        assert not np.any(ln[run, gone[run][0] + 1:])
    print(f"composite: {len(gone)} retired, {earlier} of them by the fully connected filter before the main filter's step")
    # the give-up site of the fully connected launch is reached: some run is retired where its main filter would have gone on (the main
    # launch then skips the slot: its record holds no update_count), and the survivors above show that nothing else was disturbed
    assert earlier >= 1
    eng.close()


def test_budgeted_searches_retire_the_same_runs():
    c = G.CASES["gw3_fact"]
    otr, steps = G.oracle_run(c)
    p = G.predict(c, otr, steps)
    eng = _engine(c, search_budget=37)
    stats = eng.run_bapomdp()
    _check_experiment(eng, stats, c, p, otr)
    eng.close()


def test_stop_fails_the_experiment_with_the_limit_in_force():
    c = G.CASES["tiger_lds"]
    eng = _engine(c, policy="stop")
    with pytest.raises(fba.FbaError, match="accepted fewer than 512 particles in 1024 attempts"):
        eng.run_bapomdp()
    assert len(eng.retired()) == 0
    eng.giveup_policy("stop", 0)       # the context stays usable: at the default limit the experiment is the oracle's
    before = _counters(eng)
    stats = eng.run_bapomdp()
    otr, steps = G.oracle_run(c)
    q = G.predict(c, otr, steps, max_attempts=1 << 28)
    _check_experiment(eng, stats, c, q, otr, before)
    eng.close()


@pytest.mark.parametrize("policy", ["stop", "retire"])
def test_per_call_update_gives_up_at_the_limit(policy):
    """the impossible observation of test_gpu_parity.py: the per-call interface fails its call under either policy, now after 1024 attempts"""
    eng = fba.Engine("episodic-tiger", model=N.MODEL_BA_TABLE, particles=4, sims=4, slots=2, seed=3)
    eng.giveup_policy(policy, 1024)
    prior = eng.prior()
    prior[12 + 2 * 4 + 0 * 2 + 1] = 0      # psi(listen, left, hear right) = 0
    prior[12 + 2 * 4 + 1 * 2 + 1] = 0      # psi(listen, right, hear right) = 0: "hear right" cannot happen
    eng.set_model_tabular(prior[:12], prior[12:])
    eng.belief_init()
    eng.belief_reset_domain_state()
    with pytest.raises(fba.FbaError, match="accepted fewer than 4 particles in 1024 attempts"):
        eng.belief_update(2, 1, active=[0, 1])
    eng.belief_update(2, 0, active=[1, 1])   # the ctx stays usable
    for bad in (1000, -1024, 1):
        assert eng.L.fba_giveup_policy(eng.h, N.GIVEUP_STOP, bad) == N.EINVAL
        assert "FBA_REJECT_QUANTUM" in eng.L.fba_last_error(eng.h).decode()
    assert eng.L.fba_giveup_policy(eng.h, 2, 1024) == N.EINVAL and eng.L.fba_giveup_policy(None, 0, 0) == N.EINVAL
    with pytest.raises(ValueError):
        eng.giveup_policy("retire", 1000)
    with pytest.raises(fba.FbaError, match="accepted fewer than 4 particles in 1024 attempts"):      # the policy and the limit are as they were
        eng.belief_update(2, 1, active=[1, 0])
    assert len(eng.retired()) == 0
    eng.close()


@pytest.mark.parametrize("name", ["gw3_fact", "tiger_lds"])
def test_filters_left_behind_are_valid_and_the_list_accumulates(name):
    c = G.CASES[name]
    otr, steps = G.oracle_run(c)
    p = G.predict(c, otr, steps)
    assert any(r[0] >= c["runs"] - c["E"] for r in p["retired"])      # some slot's LAST run is retired: its filter is what the slot keeps
    eng = _engine(c)
    stats = eng.run_bapomdp()
    _check_experiment(eng, stats, c, p, otr)
    blocks = eng.belief_export()
    assert blocks.shape[0] == c["E"]
    eng.belief_import(0, blocks)
    assert eng.belief_export().tobytes() == blocks.tobytes()
    again = eng.run_bapomdp()      # the same experiment once more: the same results, and the list is not cleared
    assert [(s.count, s.mean, s.m2) for s in again] == p["stats"]
    _check_trace(eng.trace(), otr, p)
    ret, ln = eng.returns()
    assert np.array_equal(ln, p["lengths"]) and np.array_equal(ret.view(np.uint64), p["returns"].view(np.uint64))
    assert _retired(eng) == sorted(p["retired"] + p["retired"])
    eng.giveup_policy("retire", c["max_attempts"])
    assert len(eng.retired()) == 0 and eng.retired().seen == 0
    eng.belief_init()              # every later call works
    eng.belief_reset_domain_state()
    eng.select_action()
    eng.close()


def test_run_ticks_goes_on_behind_a_retirement():
    """run_ticks has no last run: 24 ticks are what three runs of two episodes of four steps need at most, so every slot has by then been
    through the 48 runs the oracle knows, and goes on"""
    c = G.CASES["tiger_lds"]
    otr, steps = G.oracle_run(c)
    p = G.predict(c, otr, steps)
    ticks = (c["runs"] // c["E"]) * c["kw"]["episodes"] * c["kw"]["horizon"]
    eng = _engine(c, runs=4 * c["runs"])      # (the list has room for max(runs, slots) records)
    eng.run_ticks(ticks)
    rec = eng.retired()
    assert rec.seen == len(rec)
    known = [tuple(int(x[f]) for f in G.RETIRED_FIELDS) for x in rec if x["run"] < c["runs"]]
    assert known == p["retired"]
    assert eng.counters().env_steps == ticks * c["E"]      # no slot stopped
    eng.close()


def test_off_is_off():
    """no policy call, and the call that names the defaults: the same experiment bit for bit"""
    c = G.CASES["tiger_lds"]
    seen = []
    for policy in (None, "stop"):
        eng = _engine(c, policy=policy, max_attempts=0)
        stats = eng.run_bapomdp()
        ret, ln = eng.returns()
        cn = eng.counters()
        seen.append([eng.trace().tobytes(), ret.tobytes(), ln.tobytes(), [(s.count, s.mean, s.m2) for s in stats],
                     (cn.sim_steps, cn.belief_steps, cn.env_steps), eng.belief_export().tobytes()])
        assert len(eng.retired()) == 0
        eng.close()
    assert seen[0] == seen[1]
    otr, _ = G.oracle_run(c)
    assert len(seen[0][0]) == len(otr) * N.TRACE_DTYPE.itemsize
