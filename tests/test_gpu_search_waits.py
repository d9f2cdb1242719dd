"""The episodic-tiger search (search_kernel<..., ETIGER>) where its waits on memory are: simulations that start from a lazily reset
slot (the start state is drawn from the search generator's own registers, lazy_state(P, g, i): no load behind the particle
record's), the child lookup below the LDS-resident levels, and the back-up of levels 4 and deeper -- against the CPU oracle on
identical Philox streams: every trace field, every statistic, every counter, bit for bit (as tests/test_gpu_parity.py).

Every case runs 70 slots: one full wave and a partial one.  Each case first checks on the ORACLE's trace that it reaches that
code, so that none can pass without doing so:
  * deep cases (4096 simulations): tree_depth >= 5 in at least 50 % of the records and >= 6 in at least 15 % (measured on the
    oracle: 69-73 % and 25-33 %) -- the back-up loop over two and three levels in HBM;
  * the 768-simulation case is the one whose trees stop at depth 5 (one deep level: the loop's first trip is also its last);
    its oracle trace has depth 5 in 2.8 % of its records and nothing deeper, so it asserts exactly that: some records at depth
    5, none beyond;
  * lazily reset slots: the records at t = 0 of the episodes after the first.  With 768 simulations they are 39.5 % of those
    records (bound: 30 %).  With 4096 simulations the oracle's episodes last 3.4 steps, so they are 28.5-31.4 % (29.0 % for the
    tabular case with seed 31): the bound for those cases is 25 %, which still means more than a hundred lazy searches each.
"""
import numpy as np
import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N
from oracle import pyorc as orc

pytestmark = pytest.mark.gpu

SLOTS = 70
TIGER = ("episodic-tiger", orc.DOM_TIGER_EPISODIC)
FTIGER = ("episodic-factored-tiger", orc.DOM_FTIGER_EPISODIC)

# name -> (domain, model, Bayes-adaptive?, seed, deep?, lowest share of lazy records, configuration)
CASES = {
    "tabular_ba_tiger": (TIGER, N.MODEL_BA_TABLE, True, 31, True, 0.25, dict(particles=128, sims=4096, runs=70, episodes=2, horizon=10)),
    "tiger_pomdp_planning": (TIGER, N.MODEL_POMDP, False, 32, True, 0.25, dict(particles=64, sims=4096, runs=70)),
    "factored_tiger_fba": (FTIGER, N.MODEL_BA_FACTORED, True, 33, True, 0.25,
                           dict(size=2, structure_prior=2, particles=96, sims=4096, runs=70, episodes=2)),
    "trees_stop_at_depth_5": (TIGER, N.MODEL_BA_TABLE, True, 34, False, 0.30, dict(particles=128, sims=768, runs=70, episodes=3, horizon=10)),
    "slots_reused_after_lazy_reset": (TIGER, N.MODEL_BA_TABLE, True, 35, True, 0.25,
                                      dict(particles=128, sims=4096, runs=140, episodes=2, horizon=10)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_search_equals_oracle(case):
    (domain, odomain), model, ba, seed, deep, lazy_share, kw = CASES[case]
    o = orc.Oracle(domain=odomain, model=model, belief=N.BELIEF_REJECTION, rng_mode=orc.RNG_PHILOX, arith=orc.ARITH_DEV,
                   philox_seed=seed, trace=1, **kw)
    if ba:
        ostats, res = o.run_bapomdp()
    else:
        st, res = o.run_planning()
        ostats = [st]
    otr = o.trace(res.n_trace)

    # the case reaches the changed code (on the oracle's trace, not the engine's)
    depth = otr["tree_depth"]
    if deep:
        assert np.mean(depth >= 5) >= 0.50 and np.mean(depth >= 6) >= 0.15, (np.mean(depth >= 5), np.mean(depth >= 6))
    else:
        assert depth.max() == 5 and np.count_nonzero(depth == 5) >= 10, (depth.max(), np.count_nonzero(depth == 5))
    later = otr[otr["episode"] > 0] if ba else otr     # (a planning run is one episode per run: every run starts from a reset filter)
    assert np.mean(later["t"] == 0) >= lazy_share, np.mean(later["t"] == 0)
    assert kw["runs"] >= SLOTS and (case != "slots_reused_after_lazy_reset" or kw["runs"] > SLOTS)

    eng = fba.Engine(domain, model=model, belief="rejection_sampling", seed=seed, slots=SLOTS, trace=1, **kw)
    stats = eng.run_bapomdp() if ba else [eng.run_planning()]
    tr = eng.trace()
    assert len(tr) == len(otr)
    for name in tr.dtype.names:
        bad = np.nonzero(~np.all((tr[name] == otr[name]).reshape(len(tr), -1), axis=1))[0]
        assert bad.size == 0, f"{name}: first mismatch at record {bad[0]}: {tr[bad[0]]} vs {otr[bad[0]]}"
    for a, b in zip(stats, ostats):
        assert (a.count, a.mean, a.m2) == (b.count, b.mean, b.m2)
    c = eng.counters()
    assert (c.sim_steps, c.belief_steps, c.env_steps) == (res.sim_steps, res.belief_steps, res.env_steps)
