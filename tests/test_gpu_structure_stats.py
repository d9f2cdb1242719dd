"""fba_structure_stats / Engine.structure_stats_enable / Engine.structure_stats: the graph posterior per step of every run, reduced on the
device inside the tick.

The yardstick is existing code (structure_stats_cases.py): a context R with the statistics off, advanced tick by tick, whose filters
fba_belief_structures and numpy describe before every tick and whose last_step_info() names the steps.  The context under test, P, is
created alike, has the statistics on and runs run_ticks(K) in one call; X runs run_bapomdp with runs = slots, where run r is the first run
of slot r (tests/per_call_cases.py, part 2) and the bins are the sums over the keys with run < runs.  Integers are equal; doubles within
2 (8 N + n + 1) 2^-53 max(dev, ref) and 0.0 where the reference is; in a flat filter of 128 particles everything is equal bit for bit."""
import numpy as np
import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N
import structure_cases as SC
import structure_stats_cases as SS

pytestmark = pytest.mark.gpu

FACT = N.MODEL_BA_FACTORED


def _make(name, **kw):
    kw.setdefault("slots", 3)
    kw.setdefault("runs", kw["slots"])
    kw.setdefault("trace", 1)
    return lambda: SC.engine(name, **kw)[0]


def _queries(make, ticks=2):
    """the most frequent graph of slot 0 two ticks into the run, a graph no slot holds then, the graph of all candidates"""
    T = make()
    T.run_ticks(ticks)
    q = SC.standard_queries(T)
    T.close()
    return q


def _legal_structures(make, most=N.STRUCT_STATS_MAX_QUERIES):
    """the first `most` legal word lists, word 0 running fastest"""
    T = make()
    limit = SC.word_limits(T)
    T.close()
    rows = []
    for k in range(min(most, int(np.prod(limit.astype(np.float64))))):
        row, q = [], k
        for m in range(len(limit)):
            row.append(q % int(limit[m]))
            q //= int(limit[m])
        rows.append(row)
    return np.array(rows, np.uint32)


def _check(make, K, Q, what, exact=False, flat_counts=False, experiment=True):
    """P's bins after run_ticks(K), and X's after run_bapomdp, against R's keyed steps; returns (the keyed steps, the reference bins, P's bins)"""
    vals, R = SS.follow(make, K, Q, what, flat_counts)
    nw, ns = R.structure_lens()
    ep, hz, n, E = R.cfg.episodes, R.cfg.horizon, R.cfg.particles, R.slots
    R.close()
    shape = (ep, hz, nw, ns, len(Q))
    P = make()
    P.structure_stats_enable(Q)
    P.run_ticks(K)
    dev = P.structure_stats()
    tr = P.trace()
    assert len(tr) == min(len(vals), E * ep * hz) and all(SS.key_of(r) in vals for r in tr), what      # the yardstick's steps are the run's
    ref = SS.bins_of(vals, *shape)
    assert int(ref[0]["steps"].sum()) == len(vals) == P.counters().env_steps
    SS.compare(dev, ref, n, what + ", run_ticks", exact)
    P.close()
    if experiment:
        assert K >= ep * hz
        X = make()
        X.structure_stats_enable(Q)
        X.run_bapomdp()
        SS.compare(X.structure_stats(), SS.bins_of(vals, *shape, keep=lambda key: key[0] < X.cfg.runs), n, what + ", run_bapomdp", exact)
        X.close()
    return vals, ref, dev


@pytest.mark.parametrize("name", list(SC.FORMATS))
def test_every_record_format(name):
    """130 particles, 3 slots, 2 episodes of 8 steps, 18 ticks: the bins of episode 0 also take the freshly initiated filter of the next run"""
    make = _make(name, particles=130, seed=9700 + len(name))
    vals, ref, dev = _check(make, 2 * 8 + 2, _queries(make), name)
    assert any(key[0] >= 3 for key in vals), name      # a second run has begun
    assert int(ref[3].sum()) > 0 and int(ref[0]["distinct_max"].max()) > 1, name      # a query is held; a filter holds several graphs


@pytest.mark.parametrize("particles", [1, 256, 257])
@pytest.mark.parametrize("name", ["dense_factored_tiger2", "gridworld3_history_importance"])
def test_particle_counts(name, particles):
    """on both sides of the 256 threads of a slot's workgroup, and a filter of one particle (collapsed at every step; importance sampling,
    since a rejection filter of one particle that cannot produce the observation ends the run)"""
    make = _make(name, particles=particles, seed=9720 + particles)
    _, ref, _ = _check(make, 2 * 8 + 2, _queries(make), f"{name}, {particles} particles")
    if particles == 1:
        assert np.array_equal(ref[0]["collapsed"], ref[0]["steps"])


@pytest.mark.parametrize("name", ["packed_factored_tiger2", "gridworld3_history_rejection"])
def test_exact_flat_filter(name):
    """a flat filter of 128 particles: every term is k / 128, every sum exact"""
    make = _make(name, particles=128, seed=9730)
    _check(make, 2 * 8 + 2, _queries(make), name + ", 128 particles", exact=True)


def test_table_overflow():
    """collision avoidance 5 x 5 x 2 under the uniform prior, 4 096 particles: the filter holds more graphs than the table has entries"""
    name = "collision_avoidance_5x5x2_uniform"
    make = _make(name, particles=4096, seed=9740)
    T = make()
    T.run_ticks(0)
    assert max(SC.Reference(T, e).distinct for e in range(T.slots)) > N.STRUCT_TABLE      # the inputs prove the case, in numpy
    q = SC.standard_queries(T)
    T.close()
    _, ref, dev = _check(make, 3, q, name, experiment=False)
    assert int(ref[0]["overflowed"].sum()) > 0 and int(dev.head["overflowed"].sum()) > 0
    assert int(dev.head["distinct_max"].max()) == N.STRUCT_TABLE


def test_equal_hashes(monkeypatch):
    """FBA_STRUCT_HASH_KEEP leaves the table's hash eight bits: graphs of one hash are told apart by their words, in the tick as well"""
    make = _make("collision_avoidance_5x5x1_uniform", particles=130, seed=9750)
    q = _queries(make)
    monkeypatch.setenv("FBA_STRUCT_HASH_KEEP", "0xff")
    _, ref, _ = _check(make, 2 * 8 + 2, q, "equal hashes")
    assert int(ref[0]["distinct_max"].max()) > 2


COMPOSITE = {"reinvigoration": dict(resample_amount=8), "mh-within-gibbs": dict(threshold=-0.5, structure_prior=1)}
COMPOSITE_SEED = 9760
_composite_bins = {}


def _composite(belief):
    args = dict(size=2, structure_prior=2, particles=48, sims=16, horizon=8, episodes=2, slots=3, runs=3, seed=COMPOSITE_SEED, trace=1)
    args.update(COMPOSITE[belief])
    return lambda: fba.Engine("episodic-factored-tiger", model=FACT, belief=belief, **args)


def _falls_and_rises(held):
    """does query_held of some graph, over the bins that took steps in (episode, t) order, fall and later rise again: bins i < j < k with
    held[i] > held[j] < held[k]?"""
    x = held.reshape(-1, held.shape[-1]).astype(np.int64)
    for j in range(1, len(x) - 1):
        if np.any((x[:j].max(axis=0) > x[j]) & (x[j + 1:].max(axis=0) > x[j])):
            return True
    return False


@pytest.mark.parametrize("belief", list(COMPOSITE))
def test_composite_beliefs(belief):
    """the main filter of a belief that changes it inside the update: reinvigoration breeds graphs anew, mh-within-gibbs resamples them"""
    make = _composite(belief)
    vals, ref, dev = _check(make, 2 * 8 + 2, _legal_structures(make), belief)
    _composite_bins[belief] = ref


def test_a_composite_belief_loses_a_graph_and_finds_it_again():
    """on the reference: query_held of some graph falls and rises again across the bins of at least one of the two beliefs"""
    for belief in COMPOSITE:
        if belief not in _composite_bins:
            make = _composite(belief)
            Q = _legal_structures(make)
            vals, R = SS.follow(make, 2 * 8 + 2, Q, belief)
            nw, ns = R.structure_lens()
            _composite_bins[belief] = SS.bins_of(vals, 2, 8, nw, ns, len(Q))
            R.close()
    seen = {belief: _falls_and_rises(ref[3][ref[0]["steps"] > 0]) for belief, ref in _composite_bins.items()}
    print(seen)
    assert any(seen.values())


def test_search_budget():
    """search_budget = 37 iterations of 64 simulations: slots advance on their own, some ticks account only some slots.  Under a budget
    run_ticks(K) launches until K * slots steps are made, so K calls of run_ticks(1) are not its launches; but a step (run, episode, t) and
    the filter it is taken from are those of the run without a budget (tests/test_gpu_per_call_wide.py holds both to the oracle), so R
    runs without one, lock-step, and the bins are the sums over the keys of P's own trace, which has room for every step P makes"""
    args = dict(particles=64, sims=64, seed=9770)
    make, plain = _make("gridworld3_history_importance", search_budget=37, **args), _make("gridworld3_history_importance", **args)
    K = 12
    Q = _queries(plain, ticks=4)
    vals, R = SS.follow(plain, K + 8, Q, "search budget")
    nw, ns = R.structure_lens()
    R.close()
    P = make()
    P.structure_stats_enable(Q)
    P.run_ticks(K)
    dev, tr, made = P.structure_stats(), P.trace(), P.counters().env_steps
    assert 3 * K <= len(tr) == made < 3 * 2 * 8
    keys = {SS.key_of(r) for r in tr}
    assert len(keys) == made and keys <= set(vals)
    SS.compare(dev, SS.bins_of(vals, 2, 8, nw, ns, len(Q), keep=lambda key: key in keys), 64, "search budget")
    per_slot = np.bincount(tr["run"] % 3, minlength=3)
    launches = P.kernel_times()["env_kernel"].launches
    print("steps per slot", per_slot.tolist(), "launches", launches)
    assert launches > per_slot.max()      # in some launch a slot took no step
    P.close()


@pytest.mark.parametrize("name", list(SS.SIZE_CASES))
def test_sizes(name):
    """on both sides of every size at which the reduction takes a second workgroup, window or chunk (structure_stats_cases.SIZE_CASES), on
    the gridworld's history records under rejection sampling; episodes end at different steps, so a launch meets many bins"""
    slots, episodes, horizon, nq, K = SS.SIZE_CASES[name]
    make = _make("gridworld3_history_rejection", particles=32, sims=4 if slots > 1000 else 8, slots=slots, episodes=episodes, horizon=horizon,
                 seed=9780)
    T = make()
    assert T.structure_lens() == (SS.GW_WORDS, SS.GW_SETS)
    assert SS.plan(slots, episodes * horizon, SS.GW_WORDS, SS.GW_SETS, nq) == SS.SIZE_PLANS[name]
    T.run_ticks(1)
    top = SC.Reference(T, 0)
    T.close()
    patterns = [0xff, 0x00, 0x0f, 0xf0, 0x55, 0xaa, 0x33, 0xcc, 0x3c, 0xc3, 0x5a, 0xa5, 0x96, 0x69, 0x11]
    Q = np.array([top.uniq[top.order[0]]] + [[7 if (p >> m) & 1 else 3 for m in range(SS.GW_WORDS)] for p in patterns[:nq - 1]], np.uint32)
    vals, R = SS.follow(make, K, Q, name, flat_counts=True)
    R.close()
    ref = SS.bins_of(vals, episodes, horizon, SS.GW_WORDS, SS.GW_SETS, nq)
    taken = ref[0]["steps"].reshape(-1)
    assert int(np.count_nonzero(taken)) > min(K, horizon) or K < horizon, name      # ragged: more bins than one lock-step run would meet
    if name == "bins_second_window_used":
        c = SS.constants()
        assert int(taken[c["LDS_WORDS"] // c["COLS"]:].sum()) > 0, name
    P = make()
    P.structure_stats_enable(Q)
    P.run_ticks(K)
    SS.compare(P.structure_stats(), ref, P.cfg.particles, name)
    P.close()


def test_adding_up():
    """enable(1) clears; two experiments add; the spans [0, 1) and [1, 2) give the integers of one run_bapomdp and its doubles in the bound"""
    make = _make("gridworld3_history_importance", particles=64, seed=9790)
    Q = _queries(make)
    whole = make()
    whole.structure_stats_enable(Q)
    whole.run_bapomdp()
    one = whole.structure_stats()
    whole.run_bapomdp()
    two = whole.structure_stats()
    assert int(one.head["steps"].sum()) > 0
    for f in SS.INTS[:-1]:
        assert np.array_equal(two.head[f], 2 * one.head[f]), f
    assert np.array_equal(two.head["distinct_max"], one.head["distinct_max"])
    assert np.array_equal(two.query_held, 2 * one.query_held) and np.array_equal(two.query_sole, 2 * one.query_sole)
    assert np.allclose(two.set_frac, 2 * one.set_frac, rtol=1e-12, atol=0) and np.allclose(two.query_frac, 2 * one.query_frac, rtol=1e-12, atol=0)
    whole.structure_stats_enable(Q)
    zero = whole.structure_stats()
    assert not zero.head.tobytes().strip(b"\0") and not np.any(zero.set_frac) and not np.any(zero.query_frac)
    assert not np.any(zero.query_held) and not np.any(zero.query_sole)
    whole.close()
    eng = make()
    eng.structure_stats_enable(Q)
    eng.run_bapomdp(first_episode=0, stop_episode=1)
    first = eng.structure_stats()
    assert not np.any(first.head["steps"][1]) and first.head["steps"][0, 0] == 3      # a span fills only its own episodes
    eng.run_bapomdp(first_episode=1, stop_episode=2, beliefs=eng.belief_export())
    SS.compare(eng.structure_stats(), (one.head, one.set_frac, one.query_frac, one.query_held, one.query_sole), 64, "two spans against one run")
    eng.close()


def _everything(eng, experiment):
    r, ln = eng.returns() if experiment else (np.zeros(0), np.zeros(0))      # (run_ticks keeps no returns)
    return [eng.trace().tobytes(), r.tobytes(), ln.tobytes(), eng.last_step_info().tobytes(), eng.belief_export().tobytes(), eng.probe().tobytes(),
            eng.step_stats().tobytes()]


@pytest.mark.parametrize("name", ["dense_factored_tiger2", "packed_factored_tiger2", "gridworld3_history_importance", "collision_avoidance_5x5x1_uniform"])
def test_read_only(name):
    """with the statistics on and off: every byte of the traces, returns, exported filters, probe records and fba_step_stats bins"""
    make = _make(name, particles=64, seed=9800)      # (one probe workgroup per slot: its records repeat bit for bit from run to run)
    Q = _queries(make)
    seen = []
    for on in (True, False):
        got = []
        for ticks in (None, 2 * 8 + 2):
            eng = make()
            eng.probe_enable()
            eng.step_stats_enable()
            if on:
                eng.structure_stats_enable(Q)
            if ticks is None:
                stats = eng.run_bapomdp()
                got.append(np.array([[s.count, s.mean, s.m2] for s in stats]).tobytes())
            else:
                eng.run_ticks(ticks)
            got += _everything(eng, ticks is None)
            c = eng.counters()
            got.append((c.sim_steps, c.belief_steps, c.env_steps))
            if on:
                assert int(eng.structure_stats().head["steps"].sum()) == c.env_steps
            eng.close()
        seen.append(got)
    assert seen[0] == seen[1]


def test_refusals():
    """every FBA_EINVAL and FBA_ESTATE the public interface can reach (a record layout fba_belief_structures refuses with FBA_ESTATE is one
    no configuration creates), each with its message; after a refused enable the context runs as before"""
    nested = fba.Engine("continuous-tiger", model=N.MODEL_BA_TABLE, belief="nested", particles=12, slots=2, runs=2, sims=16, horizon=8)
    with pytest.raises(ValueError, match="fba_structure_stats_enable: the nested belief's particles are .* fba_belief_get_nested"):
        nested.structure_stats_enable()
    nested.close()
    for model, domain, kw, why in ((N.MODEL_BA_TABLE, "continuous-tiger", {}, "only a factored model under a structure prior learns its graph"),
                                   (FACT, "random-collision-avoidance", dict(width=5, height=5, size=1), "its graph is fixed")):      # (no structure prior)
        eng = fba.Engine(domain, model=model, belief=SC.IS, particles=32, slots=2, runs=2, sims=16, horizon=4, episodes=2, seed=9810, **kw)
        with pytest.raises(ValueError, match=r"fba_structure_stats_enable: the model has no parent-set words \(fba_structure_lens is 0, 0\): " + why):
            eng.structure_stats_enable()
        with pytest.raises(fba.FbaError, match="the structure statistics are off"):
            eng.structure_stats()
        eng.close()
    make = _make("gridworld3_history_importance", particles=32, seed=9811)
    eng, fresh = make(), make()
    nw, ns = eng.structure_lens()
    L, h = eng.L, eng.h
    some = np.full((N.STRUCT_STATS_MAX_QUERIES + 1, nw), 3, np.uint32)
    for nq in (-1, N.STRUCT_STATS_MAX_QUERIES + 1):
        assert L.fba_structure_stats_enable(h, 1, nq, some.ctypes.data) == N.EINVAL
        assert f"fba_structure_stats_enable: {nq} queries (0 to 16 are served)" in L.fba_last_error(h).decode()
    assert L.fba_structure_stats_enable(h, 1, 2, None) == N.EINVAL
    assert "fba_structure_stats_enable: 2 queries and no query array" in L.fba_last_error(h).decode()
    bad = np.full((2, nw), 3, np.uint32)
    bad[1, nw - 1] = int(SC.word_limits(eng)[nw - 1])
    with pytest.raises(ValueError, match=f"fba_structure_stats_enable: query 1, word {nw - 1}: 0x8 names a parent beyond the node's candidates"):
        eng.structure_stats_enable(bad)
    assert L.fba_get_structure_stats(h, 16, None, None, None, None, None) == N.ESTATE      # a refused enable leaves the statistics off
    with pytest.raises(fba.FbaError, match=r"fba_get_structure_stats: the structure statistics are off \(fba_structure_stats_enable\)"):
        eng.structure_stats()
    assert L.fba_structure_stats_enable(None, 1, 0, None) == N.EINVAL and L.fba_get_structure_stats(None, 16, None, None, None, None, None) == N.EINVAL
    # ... and the context runs as one that was never asked
    a, b = eng.run_bapomdp(), fresh.run_bapomdp()
    assert [(s.count, s.mean, s.m2) for s in a] == [(s.count, s.mean, s.m2) for s in b]
    assert eng.trace().tobytes() == fresh.trace().tobytes() and eng.belief_export().tobytes() == fresh.belief_export().tobytes()
    fresh.close()
    eng.structure_stats_enable(bad[:1])
    head = np.zeros(16, N.STRUCTURE_STAT_DTYPE)
    assert L.fba_get_structure_stats(h, 15, head.ctypes.data, None, None, None, None) == N.EINVAL
    assert "fba_get_structure_stats: room for 15 bins where episodes * horizon = 16 are kept" in L.fba_last_error(h).decode()
    assert L.fba_get_structure_stats(h, 16, None, None, None, None, None) == 16      # any pointer may be NULL
    eng.structure_stats_enable(on=False)
    with pytest.raises(fba.FbaError, match="off"):
        eng.structure_stats()
    eng.close()


def test_a_weightless_filter():
    """a step from a filter whose weights are all 0.0 counts in `steps` and `weightless` and in no fraction: the fractions of a bin and
    word sum to the steps that weigh.  An all-zero-weight snapshot block is taken by fba_belief_import and by a span, but the span's first
    step is not weightless (measured: weightless stayed 0 in every bin of the span), so the weights of one slot are set to 0.0 through
    belief_set between run_ticks(0), which initiates the filters, and the run_ticks(1) that takes the step"""
    n = 64
    make = _make("dense_factored_tiger2", particles=n, seed=9820)
    Q = _queries(make)
    eng = make()
    eng.structure_stats_enable(Q)
    eng.run_ticks(0)
    eng.belief_set(1, weight=np.zeros(n))
    assert not np.any(eng.belief_get(1)[1])
    eng.run_ticks(1)
    st = eng.structure_stats()
    print("steps", st.head["steps"].tolist(), "weightless", st.head["weightless"].tolist())
    assert st.head["steps"][0, 0] == 3 == st.head["steps"].sum() and st.head["weightless"][0, 0] == 1 == st.head["weightless"].sum()
    assert np.all(np.isfinite(st.set_frac)) and np.all(np.isfinite(st.query_frac))
    per_word = st.set_frac[0, 0].sum(axis=1)
    assert np.all(np.abs(per_word - 2.0) <= 2 * (8 * n + 3 + 1) * 2.0 ** -53 * 2.0 * st.set_frac.shape[3])
    # ... and they are the fractions of the other two slots alone
    R = make()
    R.run_ticks(0)
    bs = R.belief_structures(0, 3, top_k=0, queries=Q)
    vals = {(e, 0, 0): SS.step_value(bs.weight_total[e], bs.set_mass[e], bs.query_mass[e], bs.distinct[e], bs.overflow[e], SS.counts_of(R, e, Q), n) for e in (0, 2)}
    ref = SS.bins_of(vals, 2, 8, *R.structure_lens(), len(Q))
    for d, r in ((st.set_frac, ref[1]), (st.query_frac, ref[2])):
        assert np.all(np.abs(d - r) <= 2 * (8 * n + 3 + 1) * 2.0 ** -53 * np.maximum(d, r)) and np.all(d[r == 0.0] == 0.0)
    R.close()
    eng.close()
