"""History particles under the plain rejection filter (gridworld FBA-POMDP, -B rejection_sampling): reject_hist_kernel updates the
records, hist2_flat_search samples the root with FlatFilter::sample.  Every result must be the dense path's and the oracle's."""
import os
import random
import sys

import numpy as np
import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N
from oracle import pyorc as orc

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

REJ = "rejection_sampling"
FACT = N.MODEL_BA_FACTORED


def _record_bytes(episodes, horizon):
    return 4 * ((2 + episodes * horizon + 3) // 4 * 4)   # state, structure bits, one entry per real step


def _pair(seed, slots=None, size=0, **kw):
    runs = kw.get("runs", 1)
    eng = fba.Engine("gridworld", model=FACT, belief=REJ, seed=seed, slots=slots or runs, trace=1, size=size, **kw)
    okw = dict(kw)
    okw.pop("search_budget", None)     # (a schedule of the engine, not a parameter of the algorithm)
    okw.pop("tree_buckets", None)
    if isinstance(okw.get("planner"), str):
        okw["planner"] = N.PLANNER_NAMES[okw["planner"]]
    o = orc.Oracle(domain=orc.DOM_GRIDWORLD, model=FACT, belief=N.BELIEF_NAMES[REJ], rng_mode=orc.RNG_PHILOX,
                   arith=orc.ARITH_DEV, philox_seed=seed, trace=1, size=size, **okw)
    return eng, o


def _assert_same_experiment(eng, o):
    stats = eng.run_bapomdp()
    ostats, res = o.run_bapomdp()
    tr, otr = eng.trace(), o.trace(res.n_trace)
    assert len(tr) == len(otr)
    for name in tr.dtype.names:
        bad = np.nonzero(~np.all((tr[name] == otr[name]).reshape(len(tr), -1), axis=1))[0]
        assert bad.size == 0, f"{name}: first mismatch at record {bad[0]}: {tr[bad[0]]} vs {otr[bad[0]]}"
    for a, b in zip(stats, ostats):
        assert (a.count, a.mean, a.m2) == (b.count, b.mean, b.m2)
    c = eng.counters()
    assert (c.sim_steps, c.belief_steps, c.env_steps) == (res.sim_steps, res.belief_steps, res.env_steps)


def _run(eng):
    stats = eng.run_bapomdp()
    c = eng.counters()
    return eng.trace(), [(s.count, s.mean, s.m2) for s in stats], (c.sim_steps, c.belief_steps, c.env_steps)


def test_rejection_contexts_store_history_particles():
    eng = fba.Engine("gridworld", model=FACT, belief=REJ, size=7, structure_prior=2, particles=1024, sims=64, episodes=2, horizon=9)
    assert eng.particle_bytes == 4 * ((2 + 18 + 3) // 4 * 4)


@pytest.mark.parametrize("size,sp,noise,particles,runs,slots,budget,planner", [
    (3, 0, 0.0, 64, 4, 4, 0, "po-uct"),       # power of two
    (3, 2, 0.1, 96, 3, 1, 0, "po-uct"),       # one slot for every run
    (4, 2, 0.0, 130, 4, 4, 0, "po-uct"),
    (4, 0, 0.1, 128, 3, 3, 0, "random"),
    (5, 2, 0.1, 256, 3, 3, 0, "po-uct"),
    (5, 0, 0.0, 96, 3, 1, 0, "po-uct"),
    (7, 2, 0.0, 128, 2, 2, 0, "po-uct"),
    (7, 0, 0.1, 130, 2, 1, 0, "po-uct"),
    (3, 2, 0.0, 64, 24, 20, 37, "po-uct"),    # lock-step waves of slots at mixed depths, budgeted searches parked and resumed
    (4, 2, 0.1, 130, 21, 21, 9, "po-uct"),
])
def test_history_rejection_equals_the_oracle(size, sp, noise, particles, runs, slots, budget, planner):
    eng, o = _pair(400 + size * 10 + sp, slots=slots, size=size, particles=particles, sims=96, runs=runs, episodes=2, horizon=7,
                   structure_prior=sp, noise=noise, planner=planner, search_budget=budget)
    assert eng.particle_bytes == _record_bytes(2, 7)
    _assert_same_experiment(eng, o)


@pytest.mark.parametrize("size,sp,noise,particles", [(3, 2, 0.0, 96), (5, 2, 0.1, 130), (4, 0, 0.05, 64), (7, 2, 0.0, 1024)])
def test_history_rejection_equals_dense_particles(size, sp, noise, particles, monkeypatch):
    """The same experiment on dense count tables (FBA_DENSE_PARTICLES=1): every trace field -- the checksum over every particle's whole
    count table included -- every statistic, every counter."""
    kw = dict(model=FACT, belief=REJ, seed=171 + size, size=size, particles=particles, sims=120, runs=4, slots=4, episodes=2, horizon=9,
              structure_prior=sp, noise=noise, trace=1)
    hist = fba.Engine("gridworld", **kw)
    assert hist.particle_bytes == _record_bytes(2, 9)
    monkeypatch.setenv("FBA_DENSE_PARTICLES", "1")
    dense = fba.Engine("gridworld", **kw)
    monkeypatch.delenv("FBA_DENSE_PARTICLES")
    assert dense.particle_bytes > 10 * hist.particle_bytes
    (th, sh, ch), (td, sd, cd) = _run(hist), _run(dense)
    assert len(th) == len(td) > 0
    for name in th.dtype.names:
        assert np.array_equal(th[name], td[name]), name
    assert sh == sd and ch == cd


def _real_steps(seed, **kw):
    """(action, observation) of run 0, episode 0 as an experiment took them: observations its filter can reproduce"""
    eng = fba.Engine("gridworld", model=FACT, belief=REJ, seed=seed, slots=1, runs=1, episodes=1, trace=1, **kw)
    eng.run_bapomdp()
    tr = eng.trace()
    eng.close()
    return [(int(r["action"]), int(r["obs"])) for r in tr if not r["terminal"]]


def test_per_call_updates_equal_the_oracle():
    kw = dict(size=4, particles=64, sims=100, structure_prior=2, horizon=6)
    steps = _real_steps(515, **kw)[:4]
    assert len(steps) >= 2
    eng = fba.Engine("gridworld", model=FACT, belief=REJ, seed=515, slots=1, episodes=1, **kw)
    assert eng.particle_bytes == _record_bytes(1, 6)
    o = orc.Oracle(domain=orc.DOM_GRIDWORLD, model=orc.MODEL_BA_FACTORED, belief=N.BELIEF_NAMES[REJ], rng_mode=orc.RNG_PHILOX,
                   arith=orc.ARITH_DEV, philox_seed=515, episodes=1, **kw)
    L = orc.lib()
    L.orc_rng_episode(o.rng, 0, 0, 0)
    o.belief_initiate()
    eng.belief_init()
    o.belief_reset_domain_state()
    eng.belief_reset_domain_state()
    for t, (a, ob) in enumerate(steps):
        L.orc_rng_episode(o.rng, 0, 0, t)
        eng.set_position(run=0, episode=0, t=t)
        a_ref, rec = o.select_action(t)
        assert eng.select_action(hist_len=t)[0] == a_ref == a
        info = eng.last_step_info()[0]
        assert np.array_equal(info["root_n"], rec["root_n"]) and np.array_equal(info["root_q"], rec["root_q"])
        o.belief_update(a, ob)
        eng.belief_update(a, ob)
        assert eng.last_step_info()[0]["update_count"] == L.orc_last_update_count(o.h)
        s, _, cnt = eng.belief_get(0)
        os_, _, ocnt = o.belief_get()
        assert np.array_equal(s, os_)
        assert np.array_equal(cnt.view(np.uint32), ocnt.view(np.uint32))


def test_full_records_and_belief_set_are_refused():
    steps = _real_steps(77, size=3, particles=32, sims=16, structure_prior=2, horizon=2)
    assert len(steps) == 2
    eng = fba.Engine("gridworld", model=FACT, belief=REJ, size=3, particles=32, sims=16, horizon=2, episodes=1, structure_prior=2, slots=1, seed=77)
    assert eng.particle_bytes == _record_bytes(1, 2)
    eng.belief_init()
    eng.belief_reset_domain_state()
    for t in range(2):                   # episodes * horizon = 2 entries: full
        eng.set_position(run=0, episode=0, t=t)
        eng.belief_update(*steps[t])
    eng.set_position(run=0, episode=0, t=2)
    with pytest.raises(fba.FbaError, match="FBA_DENSE_PARTICLES"):   # (refused before any attempt: the observation does not matter)
        eng.belief_update(*steps[0])
    with pytest.raises(ValueError, match="FBA_DENSE_PARTICLES"):
        eng.belief_set(0, state=np.zeros(32, np.int32))


def test_an_impossible_observation_fails_instead_of_spinning():
    """No particle can observe x = N - 1 once no O(a, x) row gives it a count: the update gives up after 2^28 attempts."""
    eng = fba.Engine("gridworld", model=FACT, belief=REJ, size=3, particles=8, sims=8, horizon=4, structure_prior=0, slots=2, seed=9)
    assert eng.particle_bytes == _record_bytes(1, 4)
    n, g, A = 3, 3, 4                                  # size 3: goals (1, 2), (2, 1), (2, 2)
    counts = eng.prior()
    trans = A * (2 * n * n * g * n + n * n * g * g)    # the transition nodes come first (per action: x, y, goal)
    for a in range(A):
        x_node = trans + a * (2 * n * n + g * g)       # then per action O(x) [true x][observed x], O(y), O(goal)
        for v in range(n):
            counts[x_node + v * n + n - 1] = 0.0
    eng.set_model_factored(counts)
    eng.belief_init()
    eng.belief_reset_domain_state()
    ob = ((n - 1) * n + 0) * g + 0                     # observed x = N - 1
    with pytest.raises(fba.FbaError, match="accepted fewer than 8 particles"):
        eng.belief_update(0, ob, active=[1, 0])
    assert eng.belief_get(1)[0].shape == (8,)          # the context stays usable


@pytest.mark.parametrize("case", ["ts", "records", "nested", "point"])
def test_what_stays_dense(case, monkeypatch):
    kw = dict(model=FACT, belief=REJ, size=3, particles=16, sims=8, horizon=4, episodes=1, structure_prior=2, slots=1)
    if case == "ts":
        kw["planner"] = "ts"
    elif case == "records":
        monkeypatch.setenv("FBA_HIST_TREE", "records")
    elif case == "nested":
        kw["belief"] = "nested"
    else:
        kw["belief"] = "point_estimate"
    eng = fba.Engine("gridworld", **kw)
    assert eng.particle_bytes > 4096        # the dense count table (4.3 KB at size 3; a history record would be 32 bytes)


def test_reinvigoration_and_cheating_stay_dense():
    # gridworld has no fully connected prior (the reference throws "nyi"): the reinvigoration belief is refused, cheating is a weighted filter
    with pytest.raises(ValueError):
        fba.Engine("gridworld", model=FACT, belief="reinvigoration", size=3, particles=16, sims=8, horizon=4, resample_amount=2, slots=1)
    eng = fba.Engine("gridworld", model=FACT, belief="cheating-reinvigoration", size=3, particles=16, sims=8, horizon=4, resample_amount=2,
                     threshold=-2.0, structure_prior=2, slots=1)
    assert eng.particle_bytes > 4096


def test_scale_sixteen_thousand_particles_in_256_slots():
    """slots=256, particles=16384 at size 7: dense records would need 256 x 16384 x 191 KB (about 800 GB a buffer, two of them);
    history records take 80 bytes.  One tick's trace equals that of a 3-slot engine on the same runs."""
    kw = dict(model=FACT, belief=REJ, size=7, structure_prior=2, particles=16384, sims=256, episodes=2, horizon=9, runs=256, seed=2024, trace=1)
    big = fba.Engine("gridworld", slots=256, **kw)
    assert big.slots == 256 and big.particle_bytes == _record_bytes(2, 9)
    big.run_ticks(1)
    tb = big.trace()
    big.close()
    small = fba.Engine("gridworld", slots=3, **kw)
    small.run_ticks(1)
    ts = small.trace()
    assert len(tb) == 256 and len(ts) == 3
    tb = tb[np.argsort(tb["run"], kind="stable")][:3]
    ts = ts[np.argsort(ts["run"], kind="stable")]
    for name in tb.dtype.names:
        assert np.array_equal(tb[name], ts[name]), name


def _draw(rng):
    kw = dict(size=rng.choice([3, 3, 4, 4, 5]), particles=rng.choice([64, 96, 130]), sims=rng.choice([1, 5, 40, 96]),
              horizon=rng.choice([1, 3, 7, 12]), runs=rng.choice([1, 3, 6]), discount=rng.choice([0.5, 0.95, 1.0]),
              exploration=rng.choice([0.0, 1.0, 100.0]), episodes=rng.choice([1, 2, 3]), counts_total=rng.choice([10.0, 777.0, 10000.0]),
              noise=rng.choice([0.0, 0.1]), structure_prior=rng.choice([0, 2]))
    kw["max_depth"] = rng.choice([-1, 0, 1, 4, kw["horizon"]])
    if rng.random() < 0.15:
        kw["planner"] = "random"
    if rng.random() < 0.5:
        kw["search_budget"] = rng.choice([1, 9, 60, 400])
    if rng.random() < 0.5:
        kw["tree_buckets"] = max(8, kw["sims"] + rng.choice([0, 2, 40]))
    slots = rng.choice([1, 2, kw["runs"]])
    return slots, kw


def test_randomised_configurations_equal_the_oracle():
    """About sixty random gridworld rejection configurations through scripts/fuzz_parity.py's one() (engine against oracle, every trace
    field, statistic and counter); a filter that cannot reproduce an observation is skipped there, as the reference would not return."""
    import fuzz_parity
    rng = random.Random(4242)
    hist = 0
    for i in range(60):
        slots, kw = _draw(rng)
        probe = dict(kw)
        probe.pop("planner", None)
        eng = fba.Engine("gridworld", model=FACT, belief=REJ, planner=kw.get("planner", "po-uct"), slots=slots, **probe)
        hist += eng.particle_bytes < 1024
        eng.close()
        fuzz_parity.one("gridworld", FACT, REJ, slots, kw, seed=7000 + i)
    assert hist >= 40   # (counts_total = 777 with noise is not exact under "+ j": those stay dense)
