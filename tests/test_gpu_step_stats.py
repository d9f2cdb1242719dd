"""fba_step_stats / Engine.step_stats_enable / Engine.step_stats: per-(episode, t) statistics of every run, reduced on the device.

The yardstick is the trace: bin (e, t) is defined as a reduction over the trace records of episode e, step t, so every test aggregates
Engine.trace() on the host -- integers exactly, doubles with math.fsum -- and compares.  Integer members and the reward sums (every
built-in reward is a multiple of 0.5 of magnitude <= 1000: every partial sum is exact) compare with ==; a double member summed over n
terms x_i compares within n * 2^-52 * sum |x_i| of the fsum, the bound include/fba_hip.h states.  The probe members are held to
Engine.probe() the same way, with the allowances the header names: one rounding per post_ratio term, and det_log's distance from libm,
3e-16 * max(1, |log x|) per term (tests/test_oracle_golden.py pins it).  For log_evidence_sq_sum a term l^2 computed from a logarithm
that is off by d <= 3e-16 * max(1, |l|) is off by at most 2 |l| d + d^2, plus the rounding of the square, 2^-53 l^2."""
import numpy as np
import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N
from step_stats_size_cases import INTS, Ref as _Ref, check_probe as _check_probe, probe_ref as _probe_ref      # (shared with test_gpu_step_stats_sizes.py)

pytestmark = pytest.mark.gpu

POMDP, TABLE, FACT = N.MODEL_POMDP, N.MODEL_BA_TABLE, N.MODEL_BA_FACTORED

TIGER = dict(domain="episodic-tiger", model=TABLE, belief="rejection_sampling", runs=150, slots=70, episodes=3, horizon=6, sims=32, particles=64, seed=9101)
GRID = dict(domain="gridworld", model=FACT, belief="importance_sampling", size=3, structure_prior=2, runs=40, slots=40, episodes=2, horizon=5, sims=64,
            particles=64, seed=9102, search_budget=37)
COFFEE = dict(domain="coffee", model=POMDP, belief="rejection_sampling", runs=33, slots=33, horizon=8, sims=32, particles=64, seed=9103)
PLAN_TIGER = dict(domain="episodic-tiger", model=POMDP, belief="rejection_sampling", runs=33, slots=20, horizon=8, sims=32, particles=64, seed=9104)
COMPOSITE = dict(domain="episodic-factored-tiger", model=FACT, belief="reinvigoration", size=2, structure_prior=2, resample_amount=8, runs=20, slots=20,
                 episodes=2, horizon=6, sims=32, particles=64, seed=9105)
CASES = {"tiger_rejection": TIGER, "gridworld_budgeted": GRID, "planning_coffee": COFFEE, "planning_tiger": PLAN_TIGER, "reinvigoration": COMPOSITE}


def _engine(cfg, **kw):
    args = dict(cfg, **kw)
    return fba.Engine(args.pop("domain"), **args)


def _run(eng):
    return eng.run_planning() if eng.cfg.model == POMDP else eng.run_bapomdp()


def _exercises(tr, st, what, terminals=True):
    """the inputs exercise what they are there for"""
    steps, term = int(st["steps"].sum()), int(st["terminals"].sum())
    print(f"{what}: {steps} steps, {term} terminal, steps per bin {st['steps'].tolist()}")
    if terminals:
        assert 0 < int(np.sum(tr["terminal"] != 0)) < len(tr), what
        assert len(set(st["steps"].reshape(-1).tolist())) > 1, what


@pytest.mark.parametrize("name", list(CASES))
def test_the_bins_equal_the_trace(name):
    """coffee never ends an episode (its steps per bin are all `runs`): it is there for its rewards of -0.5 and the shape (1, H); the plain
    POMDP path meets terminal steps in planning_tiger"""
    cfg = CASES[name]
    eng = _engine(cfg, trace=1)
    eng.step_stats_enable()
    _run(eng)
    tr, st = eng.trace(), eng.step_stats()
    assert st.shape == (max(eng.cfg.episodes, 1), cfg["horizon"])
    _exercises(tr, st, name, terminals=name != "planning_coffee")
    if name == "planning_coffee":
        assert np.any(tr["reward"] == -0.5) and st.shape == (1, 8)
        assert np.any(st["reward_sum"] % 1.0 != 0.0)
    if name == "gridworld_budgeted":
        assert eng.particle_bytes < 1024      # history records
    assert int(st["steps"].sum()) == len(tr) == eng.counters().env_steps
    _Ref(eng, tr).check(st, name)
    eng.close()


def test_rejection_with_the_trace_off():
    """without the trace nothing resets update_count behind a terminal step: the bins must not read it there"""
    on, off = _engine(TIGER, trace=1), _engine(TIGER, trace=0)
    for eng in (on, off):
        eng.step_stats_enable()
        _run(eng)
    tr = on.trace()
    a, b = on.step_stats(), off.step_stats()
    assert len(off.trace()) == 0
    assert 0 < int(a["terminals"].sum()) < int(a["steps"].sum())
    assert int(a["attempts_steps"].sum()) == int(a["steps"].sum()) - int(a["terminals"].sum()) > 0
    for f in INTS:
        assert np.array_equal(a[f], b[f]), f
    _Ref(on, tr).check(b, "trace off, against the traced run's records")
    assert int(b["steps"].sum()) == off.counters().env_steps
    on.close()
    off.close()


def test_run_ticks():
    eng = _engine(dict(TIGER, runs=70), trace=1)
    eng.step_stats_enable()
    eng.run_ticks(5)
    tr, st = eng.trace(), eng.step_stats()
    assert int(st["steps"].sum()) == 350 == len(tr)
    _Ref(eng, tr).check(st, "run_ticks")
    eng.close()


def _everything(eng):
    r, ln = eng.returns()
    return [eng.trace().tobytes(), r.tobytes(), ln.tobytes(), eng.last_step_info().tobytes(), eng.belief_export().tobytes()]


@pytest.mark.parametrize("particles", [64, 3584])
def test_read_only(particles):
    """3 584 particles: the shape whose slots keep 16-byte filters between updates (test_gpu_tiger_compact.py) -- with the statistics on
    they still do"""
    cfg = dict(TIGER, particles=particles, runs=70, episodes=3, horizon=4, sims=64) if particles > 64 else TIGER
    seen = []
    for on in (True, False):
        eng = _engine(cfg, trace=1)
        if on:
            eng.step_stats_enable()
        stats = _run(eng)
        got = [np.array([[s.count, s.mean, s.m2] for s in stats]).tobytes()] + _everything(eng)
        c = eng.counters()
        got.append((c.sim_steps, c.belief_steps, c.env_steps))
        eng.close()
        eng = _engine(dict(cfg, runs=70), trace=1)
        if on:
            eng.step_stats_enable()
        eng.run_ticks(7)
        if particles > 64:
            assert eng.debug_compact_slots() > 0
        got += [eng.trace().tobytes(), eng.last_step_info().tobytes(), eng.belief_export().tobytes()]
        if on:
            assert int(eng.step_stats()["steps"].sum()) == 7 * 70
        eng.close()
        seen.append(got)
    assert seen[0] == seen[1]


PROBE_TIGER = dict(TIGER, runs=70)
PROBE_GRID = dict(GRID, search_budget=0)


@pytest.mark.parametrize("name", ["tiger", "gridworld"])
def test_the_probe_feeds_the_bins(name):
    cfg = PROBE_TIGER if name == "tiger" else PROBE_GRID
    full = _engine(cfg, trace=1)
    full.probe_enable()
    full.step_stats_enable()
    _run(full)
    recs, tr, st = full.probe(), full.trace(), full.step_stats()
    assert recs.seen == recs.size == int(np.sum(tr["terminal"] == 0)) > 0
    ints, terms = _probe_ref(recs, st.shape)
    assert int(st["probed"].sum()) == recs.size
    _check_probe(st, ints, terms, name + ", full capacity")
    _Ref(full, tr).check(st, name + ", full capacity", probe=False)
    full.close()
    # the bins do not depend on the buffer
    none = _engine(cfg, trace=1)
    none.probe_enable(capacity=0)
    none.step_stats_enable()
    _run(none)
    assert none.probe().size == 0 and none.probe().seen == recs.size
    _check_probe(none.step_stats(), ints, terms, name + ", capacity 0")
    none.close()
    # a range of slots (runs <= slots: run r is executed by slot r)
    part = _engine(cfg, trace=1)
    part.step_stats_enable()
    part.probe_enable(first=5, count=9, capacity=0)
    _run(part)
    tr = part.trace()
    inside = tr[(tr["terminal"] == 0) & (tr["run"] >= 5) & (tr["run"] < 14)]
    want = np.zeros(st.shape, np.uint64)
    for r in inside:
        want[int(r["episode"]), int(r["t"])] += 1
    assert np.array_equal(part.step_stats()["probed"], want) and want.sum() > 0
    part.close()


def test_accumulate_and_clear():
    cfg = dict(TIGER, runs=70)
    whole = _engine(cfg)
    whole.step_stats_enable()
    whole.run_bapomdp()
    ref = whole.step_stats()
    whole.close()
    eng = _engine(cfg)
    eng.step_stats_enable()
    eng.run_bapomdp(first_episode=0, stop_episode=2)
    first = eng.step_stats()
    assert not np.any(first["steps"][2]) and first["steps"][0, 0] == 70 == first["steps"][1, 0]      # a span fills only its own episodes
    blocks = eng.belief_export()
    eng.run_bapomdp(first_episode=2, stop_episode=3, beliefs=blocks)
    st = eng.step_stats()
    for f in INTS:
        assert np.array_equal(st[f], ref[f]), f
    assert np.array_equal(st["reward_sum"], ref["reward_sum"])
    eng.step_stats_enable()
    assert eng.step_stats().tobytes() == np.zeros(ref.shape, N.STEP_STAT_DTYPE).tobytes()
    out = np.zeros(ref.size - 1, N.STEP_STAT_DTYPE)
    assert eng.L.fba_get_step_stats(eng.h, out.ctypes.data, out.size) == N.EINVAL
    assert eng.L.fba_get_step_stats(eng.h, None, ref.size) == N.EINVAL
    assert eng.L.fba_get_step_stats(None, out.ctypes.data, ref.size) == N.EINVAL
    eng.step_stats_enable(False)
    out = np.zeros(ref.size, N.STEP_STAT_DTYPE)
    assert eng.L.fba_get_step_stats(eng.h, out.ctypes.data, out.size) == N.ESTATE
    with pytest.raises(fba.FbaError, match="off"):
        eng.step_stats()
    eng.close()
