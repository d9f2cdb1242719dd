"""History particles for the collision-avoidance FBA-POMDP in the prior's own graph (fbapomdp -D *-collision-avoidance, no structure
prior, -B importance_sampling) where the filter is the multi-launch one (more than 65 536 particles, or from FBA_IS_MULTI_MIN up):
is_multi_ca_step_kernel updates records of 12 + 9n-bit entries over the prior table in LDS and search_ca_hist_kernel searches from them.
Every result must be the dense path's and the oracle's, bit for bit -- also at 7 x 7 with two obstacles, whose prior holds counts c for
which c + j is not the float j additions of 1.0f reach."""
import random

import numpy as np
import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N
from oracle import pyorc as orc

pytestmark = pytest.mark.gpu

FACT = N.MODEL_BA_FACTORED
IS, REJ = "importance_sampling", "rejection_sampling"
RANDOM, CENTERED = "random-collision-avoidance", "centered-collision-avoidance"


@pytest.fixture(autouse=True)
def _small_filters_take_the_large_filter_path(request, monkeypatch):
    """The format's update is the multi-launch filter, so contexts take it where the dense records take that filter too: above 65 536
    particles.  FBA_IS_MULTI_MIN moves that one switch-over, for both formats, so that filters of a few hundred particles, which the oracle
    can follow quickly, run the same kernels.  The tests named in DEFAULTS run without it."""
    if request.function.__name__ not in DEFAULTS:
        monkeypatch.setenv("FBA_IS_MULTI_MIN", "1")


DEFAULTS = {"test_record_size", "test_one_belief_of_200000_particles_equals_the_oracle", "test_scale_256_slots_the_dense_format_cannot_hold",
            "test_one_launch_filters_stay_dense"}


def _record_bytes(episodes, horizon):
    return 4 * ((2 + episodes * horizon + 3) // 4 * 4)   # state, an unused word, one entry per real step


def _dense_bytes(W, H, n):
    return 4 * (3 * (W * W + H * H * (1 + n)) + 3 * n * H * H)   # the count table alone (a dense record also holds the state)


def _pair(domain, seed, belief=IS, slots=None, **kw):
    runs = kw.get("runs", 1)
    eng = fba.Engine(domain, model=FACT, belief=belief, seed=seed, slots=slots or runs, trace=1, **kw)
    okw = dict(kw)
    if domain == CENTERED:
        okw["ca_centered"] = 1
    if isinstance(okw.get("planner"), str):
        okw["planner"] = N.PLANNER_NAMES[okw["planner"]]
    o = orc.Oracle(domain=orc.DOM_COLLISION_AVOID, model=orc.MODEL_BA_FACTORED, belief=N.BELIEF_NAMES[belief], rng_mode=orc.RNG_PHILOX,
                   arith=orc.ARITH_DEV, philox_seed=seed, trace=1, **okw)
    return eng, o


def _assert_same_experiment(eng, o):
    stats = eng.run_bapomdp()
    ostats, res = o.run_bapomdp()
    tr, otr = eng.trace(), o.trace(res.n_trace)
    assert len(tr) == len(otr) > 0
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


def test_record_size(monkeypatch):
    """7 x 7 with two obstacles: a dense particle is 882 floats; a record is 8 bytes + 4 per real step"""
    kw = dict(model=FACT, belief=IS, width=7, height=7, size=2, particles=65537, sims=16, episodes=2, horizon=10, slots=1)
    eng = fba.Engine(RANDOM, **kw)
    assert eng.particle_bytes == 4 * ((2 + 20 + 3) // 4 * 4)
    monkeypatch.setenv("FBA_DENSE_PARTICLES", "1")
    dense = fba.Engine(RANDOM, **kw)
    assert dense.particle_bytes > 3500


SHAPES = [(RANDOM, 7, 7, 2), (CENTERED, 5, 5, 2), (RANDOM, 4, 3, 1)]


@pytest.mark.parametrize("domain,W,H,n", SHAPES)
@pytest.mark.parametrize("planner", ["po-uct", "random"])
def test_history_equals_the_oracle(domain, W, H, n, planner):
    """whole experiments, every trace field (belief_hash and weight_total included), statistics and counters; 130 particles (not a
    multiple of 64), five runs in two slots"""
    eng, o = _pair(domain, 900 + W * 10 + n, slots=2, width=W, height=H, size=n, particles=130, sims=96, runs=5, episodes=2, horizon=6,
                   planner=planner)
    assert eng.particle_bytes == _record_bytes(2, 6)
    _assert_same_experiment(eng, o)


@pytest.mark.parametrize("domain,W,H,n", SHAPES)
@pytest.mark.parametrize("planner", ["po-uct", "random"])
def test_history_equals_dense_particles(domain, W, H, n, planner, monkeypatch):
    kw = dict(model=FACT, belief=IS, seed=371 + W, width=W, height=H, size=n, particles=130, sims=96, runs=3, slots=2, episodes=2, horizon=6,
              planner=planner, trace=1)
    hist = fba.Engine(domain, **kw)
    assert hist.particle_bytes == _record_bytes(2, 6)
    monkeypatch.setenv("FBA_DENSE_PARTICLES", "1")
    dense = fba.Engine(domain, **kw)
    monkeypatch.delenv("FBA_DENSE_PARTICLES")
    assert dense.particle_bytes > _dense_bytes(W, H, n)
    (th, sh, ch), (td, sd, cd) = _run(hist), _run(dense)
    assert len(th) == len(td) > 0
    for name in th.dtype.names:
        assert np.array_equal(th[name], td[name]), name
    assert sh == sd and ch == cd
    for slot in range(2):
        s1, w1, c1 = hist.belief_get(slot)
        s2, w2, c2 = dense.belief_get(slot)
        assert np.array_equal(s1, s2) and np.array_equal(w1, w2) and np.array_equal(c1.view(np.uint32), c2.view(np.uint32))


def _oracle(seed, **kw):
    return orc.Oracle(domain=orc.DOM_COLLISION_AVOID, model=orc.MODEL_BA_FACTORED, belief=orc.BELIEF_IMPORTANCE, rng_mode=orc.RNG_PHILOX,
                      arith=orc.ARITH_DEV, philox_seed=seed, **kw)


def _per_call(seed, steps, select, **kw):
    """init, reset, [select_action,] belief_update, belief_get and belief_get_particle against the oracle's calls after every step"""
    eng = fba.Engine(RANDOM, model=FACT, belief=IS, seed=seed, slots=1, **kw)
    assert eng.particle_bytes == _record_bytes(kw["episodes"], kw["horizon"])
    o = _oracle(seed, **kw)
    L = orc.lib()
    L.orc_rng_episode(o.rng, 0, 0, 0)
    o.belief_initiate()
    eng.belief_init()
    o.belief_reset_domain_state()
    eng.belief_reset_domain_state()
    for t, (a, ob) in enumerate(steps):
        L.orc_rng_episode(o.rng, 0, 0, t)
        eng.set_position(run=0, episode=0, t=t)
        if select:
            a_ref, rec = o.select_action(t)
            assert eng.select_action(hist_len=t)[0] == a_ref
            info = eng.last_step_info()[0]
            assert np.array_equal(info["root_n"], rec["root_n"]) and np.array_equal(info["root_q"], rec["root_q"])
        o.belief_update(a, ob)
        eng.belief_update(a, ob)
        s, w, cnt = eng.belief_get(0)
        os_, ow, ocnt = o.belief_get()
        assert np.array_equal(s, os_) and np.array_equal(w, ow)
        assert np.array_equal(cnt.view(np.uint32), ocnt.view(np.uint32)), f"counts differ after update {t}"
        assert eng.last_step_info()[0]["weight_total"] > 0     # (the filter has not degenerated)
        ps, _, pc = eng.belief_get_particle(kw["particles"] - 1)
        assert ps == os_[-1] and np.array_equal(pc.view(np.uint32), ocnt[-1].view(np.uint32))
    return eng, o


def test_per_call_interface_equals_the_oracle():
    _per_call(515, [(1, 2 * 5 + 2), (0, 2 * 5 + 3), (2, 3 * 5 + 3), (1, 2 * 5 + 2)], True, width=5, height=5, size=2, particles=96, sims=100,
              episodes=1, horizon=6)


def test_updates_on_the_rows_of_inexact_counts_equal_the_oracle():
    """7 x 7 with two obstacles: the tails of the observation rows hold counts c below 0.05 for which c + j is not the float that j
    additions of 1.0f reach (the gridworld formats would refuse this table).  The first obstacle is observed at row 0, then at row 6: six
    cells apart, so most particles weigh at least one of these observations by a tail count, on rows whose other cells the updates raise.
    The tail cells themselves are drawn with a probability of a few in a million, so hardly any is incremented here: this test checks the
    rows that hold them against the oracle (states, weights and counts after every update, the total weight positive: _per_call);
    test_sequence_table_decides_draws_and_weights is the one in which cells read from the sequence table are raised again and again."""
    prior = fba.Engine(RANDOM, model=FACT, belief=IS, width=7, height=7, size=2, particles=4, sims=4, slots=1).prior()
    inexact = set()
    for v in np.unique(prior):
        run = np.float32(v)
        for j in range(1, 128):
            run = np.float32(run + np.float32(1.0))
            if run != np.float32(np.float32(v) + np.float32(j)):
                inexact.add(float(v))
    assert inexact and max(inexact) < 0.05 and min(inexact) > 0
    _per_call(733, [(1, 0 * 7 + 3)] * 3 + [(1, 6 * 7 + 3)] * 3, False, width=7, height=7, size=2, particles=200, sims=8, episodes=1, horizon=12)


def test_multi_launch_filter_forced_at_a_few_hundred_particles(monkeypatch):
    monkeypatch.setenv("FBA_IS_MULTI_MIN", "300")
    eng, o = _pair(RANDOM, 132, width=7, height=7, size=2, particles=333, sims=40, runs=4, episodes=2, horizon=5)
    assert eng.particle_bytes == _record_bytes(2, 5)
    _assert_same_experiment(eng, o)


def test_one_belief_of_200000_particles_equals_the_oracle():
    eng, o = _pair(RANDOM, 1033, width=7, height=7, size=2, particles=200000, sims=8, runs=1, episodes=1, horizon=3)
    assert eng.particle_bytes == _record_bytes(1, 3)
    _assert_same_experiment(eng, o)


def test_full_records_and_belief_set_are_refused():
    eng = fba.Engine(RANDOM, model=FACT, belief=IS, width=5, height=5, size=2, particles=32, sims=16, horizon=2, episodes=1, slots=1, seed=77)
    assert eng.particle_bytes == _record_bytes(1, 2)
    eng.belief_init()
    eng.belief_reset_domain_state()
    for t in range(2):                   # episodes * horizon = 2 entries: full
        eng.set_position(run=0, episode=0, t=t)
        eng.belief_update(1, 2 * 5 + 2)
    eng.set_position(run=0, episode=0, t=2)
    with pytest.raises(fba.FbaError, match="FBA_DENSE_PARTICLES"):
        eng.belief_update(1, 2 * 5 + 2)
    with pytest.raises(ValueError, match="FBA_DENSE_PARTICLES"):
        eng.belief_set(0, state=np.zeros(32, np.int32))


@pytest.mark.parametrize("case", ["structure_prior_1", "structure_prior_2", "rejection", "ts", "three_obstacles", "127_steps"])
def test_what_stays_dense_equals_the_oracle(case):
    belief, W, H, n = IS, 4, 3, 1
    kw = dict(particles=24, sims=24, runs=2, episodes=1, horizon=4)
    if case.startswith("structure_prior"):
        kw["structure_prior"] = int(case[-1])
    elif case == "rejection":
        belief = REJ
    elif case == "ts":
        kw["planner"] = "ts"
    elif case == "three_obstacles":
        W, H, n = 3, 3, 3
    else:
        kw.update(horizon=127, max_depth=10, sims=4, runs=1)   # (a search depth of 127 would not fit the dense search's LDS)
    eng, o = _pair(RANDOM, 31, belief=belief, width=W, height=H, size=n, **kw)
    assert eng.particle_bytes > _dense_bytes(W, H, n)
    _assert_same_experiment(eng, o)


MI355X_HBM_BYTES = 288 * 10 ** 9


def test_scale_256_slots_the_dense_format_cannot_hold(monkeypatch):
    """256 beliefs at 7 x 7 with two obstacles.  fba_create budgets half the card's free memory; by its per-slot formula (two record
    buffers, two weights, a prefix sum and a side row per particle) dense records of a few thousand particles still fit a 288 GB card,
    so the filters are 131 072 particles each: 239 GB dense, 4 GB as records."""
    kw = dict(model=FACT, belief=IS, width=7, height=7, size=2, particles=131072, sims=32, episodes=1, horizon=3)
    monkeypatch.setenv("FBA_DENSE_PARTICLES", "1")
    dense = fba.Engine(RANDOM, slots=1, **{**kw, "particles": 64})
    dense_bytes = dense.particle_bytes
    dense.close()
    monkeypatch.delenv("FBA_DENSE_PARTICLES")
    assert 256 * kw["particles"] * (2 * dense_bytes + 2 * 8 + 8 + 4 * 10) > MI355X_HBM_BYTES // 2
    eng = fba.Engine(RANDOM, runs=256, slots=256, seed=2026, **kw)
    assert eng.slots == 256 and eng.particle_bytes == _record_bytes(1, 3)
    assert 256 * kw["particles"] * (eng.particle_bytes + 2 * 8 + 8 + 4 * 10) < MI355X_HBM_BYTES // 16     # (one record buffer per slot)
    stats = eng.run_bapomdp()
    assert stats[0].count == 256 and np.isfinite(stats[0].mean) and np.isfinite(stats[0].m2)
    c = eng.counters()
    assert c.belief_steps > 0 and c.sim_steps > 0


def _draw(rng):
    W, H, n = rng.choice([(3, 3, 1), (4, 3, 1), (3, 3, 2), (5, 5, 2), (5, 5, 1), (7, 7, 2)])
    kw = dict(width=W, height=H, size=n, particles=rng.choice([16, 64, 96, 130]), sims=rng.choice([1, 5, 40, 96]),
              horizon=rng.choice([1, 3, 7, 12]), runs=rng.choice([1, 3, 6]), discount=rng.choice([0.5, 0.95, 1.0]),
              exploration=rng.choice([0.0, 1.0, 100.0]), episodes=rng.choice([1, 2, 3]), counts_total=rng.choice([10.0, 777.0, 10000.0]),
              noise=rng.choice([0.0, 0.05, 0.1]))
    kw["max_depth"] = rng.choice([-1, 0, 1, 4, kw["horizon"]])
    if rng.random() < 0.2:
        kw["planner"] = "random"
    if rng.random() < 0.25:     # a quarter of the draws are contexts that stay dense
        kw["structure_prior"] = rng.choice([1, 2])
    slots = rng.choice([1, 2, kw["runs"]])
    return rng.choice([RANDOM, CENTERED]), slots, kw


def test_randomised_configurations_equal_the_oracle():
    """Twenty-four random admissible configurations: engine against oracle, every trace field, statistic and counter; at least half of
    them on history records (three quarters are drawn without a structure prior)."""
    rng = random.Random(6161)
    hist = 0
    for i in range(24):
        domain, slots, kw = _draw(rng)
        eng, o = _pair(domain, 9000 + i, slots=slots, **kw)
        hist += eng.particle_bytes == _record_bytes(kw["episodes"], kw["horizon"])
        _assert_same_experiment(eng, o)
        eng.close()
    assert hist >= 12


# counts c for which c + 2.0f is not (c + 1.0f) + 1.0f in fp32: rows of such counts are soon dominated by the increments, so cells raised
# twice or more -- read from the sequence table on the device -- decide every draw and every weight
INEXACT = [0.002, 0.009, 0.011, 0.015]


def _inexact_prior(eng, values):
    for v in values:
        c = np.float32(v)
        assert np.float32(np.float32(c + np.float32(1)) + np.float32(1)) != np.float32(c + np.float32(2))
    prior = eng.prior()
    cells = np.nonzero(prior > 0)[0]
    new = prior.copy()
    new[cells] = np.asarray(values, np.float32)[np.arange(cells.size) % len(values)]
    return new


@pytest.mark.parametrize("W,H,n", [(5, 5, 2), (4, 3, 1)])
def test_sequence_table_decides_draws_and_weights(W, H, n, monkeypatch):
    """A prior set through fba_set_model_factored whose every nonzero count is inexact under c + j from j = 2 on.  The history context
    rebuilds its sequence table; its experiment must equal the dense records' one in every trace field: weight_total is a sum of
    quotients of such counts and the drawn states follow from them, so a count read as prior + (float)j would change both.  The cells
    raised twice or more are there: fba_belief_get shows them."""
    kw = dict(model=FACT, belief=IS, seed=91 + W, width=W, height=H, size=n, particles=130, sims=64, runs=3, slots=3, episodes=2, horizon=8, trace=1)
    hist = fba.Engine(RANDOM, **kw)
    assert hist.particle_bytes == _record_bytes(2, 8)
    new = _inexact_prior(hist, INEXACT)
    hist.set_model_factored(new)
    monkeypatch.setenv("FBA_DENSE_PARTICLES", "1")
    dense = fba.Engine(RANDOM, **kw)
    monkeypatch.delenv("FBA_DENSE_PARTICLES")
    assert dense.particle_bytes > _dense_bytes(W, H, n)
    dense.set_model_factored(new)
    (th, sh, ch), (td, sd, cd) = _run(hist), _run(dense)
    assert len(th) == len(td) > 0 and np.any(th["weight_total"] > 0)
    for name in th.dtype.names:
        assert np.array_equal(th[name], td[name]), name
    assert sh == sd and ch == cd
    raised_twice = 0
    for slot in range(3):
        s1, w1, c1 = hist.belief_get(slot)
        s2, w2, c2 = dense.belief_get(slot)
        assert np.array_equal(s1, s2) and np.array_equal(w1, w2) and np.array_equal(c1.view(np.uint32), c2.view(np.uint32))
        raised_twice += int(np.sum((c1 - new[None, :] >= 2) & (new[None, :] > 0)))
    assert raised_twice > 0


def test_a_prior_of_too_many_inexact_counts_is_refused():
    eng = fba.Engine(RANDOM, model=FACT, belief=IS, width=5, height=5, size=2, particles=16, sims=4, slots=1, episodes=1, horizon=4)
    nine = [0.002, 0.009, 0.011, 0.015, 0.018, 0.022, 0.024, 0.028, 0.031]
    with pytest.raises(ValueError, match="FBA_DENSE_PARTICLES"):
        eng.set_model_factored(_inexact_prior(eng, nine))
    eng.set_model_factored(_inexact_prior(eng, nine[:8]))     # eight distinct values: the table's bound


@pytest.mark.parametrize("particles,history", [(65536, False), (65537, True)])
def test_one_launch_filters_stay_dense(particles, history):
    """no one-launch update exists for these records: without FBA_IS_MULTI_MIN a filter of at most 65 536 particles keeps dense records
    and the one-launch importance_kernel; both sides of the switch-over equal the oracle"""
    eng, o = _pair(RANDOM, 4100, width=5, height=5, size=2, particles=particles, sims=16, runs=1, episodes=1, horizon=3)
    assert (eng.particle_bytes == _record_bytes(1, 3)) == history
    assert history or eng.particle_bytes > _dense_bytes(5, 5, 2)
    _assert_same_experiment(eng, o)
