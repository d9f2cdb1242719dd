"""fba_belief_summary / Engine.belief_summary: the per-slot posterior reduced on the device from every record format, against numpy
over Engine.belief_get of the same slot.

Bound (derived, not measured): every output is a sum of at most N non-negative terms, each a product rounded once, divided once, so
any fp64 summation order is within (N + 1) * 2^-53 relative of the exact value to first order, on both sides:
|dev - ref| <= 8 * N * 2^-53 * max(dev, ref) per entry, exactly 0.0 wherever the reference is 0.0 (a zero sum of non-negative terms has
only zero terms), and equality for the integer sums of a flat filter.  One lost increment of one particle moves an entry by about 1 / N
of a unit, orders of magnitude above that.  The summary is always taken BEFORE the belief_get it is compared with: belief_get writes a
lazily reset filter's states out, the summary must see them without that."""
import numpy as np
import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

pytestmark = pytest.mark.gpu

POMDP, TABLE, FACT = N.MODEL_POMDP, N.MODEL_BA_TABLE, N.MODEL_BA_FACTORED
IS, REJ = "importance_sampling", "rejection_sampling"
DENSE_ENV = {"FBA_DENSE_PARTICLES": "1"}
MULTI_ENV = {"FBA_IS_MULTI_MIN": "1"}
EPISODES, HORIZON = 2, 8
# the inexact prior of test_gpu_history_ca.py::test_sequence_table_decides_draws_and_weights: c + 2.0f is not (c + 1.0f) + 1.0f in fp32
INEXACT = [0.002, 0.009, 0.011, 0.015]


def _record_bytes():
    return 4 * ((2 + EPISODES * HORIZON + 3) // 4 * 4)


def _dense_bytes(ncnt):
    need, cs = ncnt + 1, 4
    if need <= 64:
        while cs < need:
            cs <<= 1
    else:
        cs = (need + 3) // 4 * 4
    return 4 * cs


def _packed_ftiger_bytes(size):
    fs = size + 1
    nc = 8 * fs + 4 + (2 << fs)
    return 4 * ((nc // 2 + 2 + 3) // 4 * 4)


def _engine(monkeypatch, domain, model, belief, env=None, **kw):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    kw.setdefault("sims", 16)
    if model != POMDP:
        kw.setdefault("episodes", EPISODES)
    kw.setdefault("horizon", HORIZON)
    eng = fba.Engine(domain, model=model, belief=belief, **kw)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return eng


def _layout(eng):
    """(counts, mask words) of a particle's blob"""
    if eng.cfg.model != FACT:
        return eng.ncnt, 0
    lay = eng.factored_layout()
    assert lay.n_counts + lay.n_mask_words == eng.ncnt
    return lay.n_counts, lay.n_mask_words


def _reference(eng, slot):
    """numpy over belief_get: weight totals, state mass, mean counts, edge probabilities, and the particles' mask words"""
    weighted = eng.cfg.belief == N.BELIEF_IMPORTANCE
    s, w, cnt = eng.belief_get(slot, weights=weighted, counts=eng.ncnt > 0)
    if not weighted:
        w = np.ones(len(s), np.float64)
    nc, nm = _layout(eng)
    total = w.sum()
    ref = dict(weight_total=total, weight_sq_total=(w * w).sum(), state_mass=np.bincount(s, weights=w, minlength=eng.S), counts=cnt, masks=None,
               mean_counts=None, edge_prob=None)
    if eng.ncnt:
        mean = (w[:, None] * cnt.astype(np.float64)).sum(axis=0) / total
        mean[nc:] = 0.0
        ref["mean_counts"] = mean
    if nm:
        masks = np.ascontiguousarray(cnt[:, nc:]).view(np.uint32)
        bits = (masks[:, :, None] >> np.arange(N.MAX_FEATURES, dtype=np.uint32)[None, None, :]) & 1
        ref["edge_prob"] = (w[:, None, None] * bits).sum(axis=0) / total
        ref["masks"] = masks
    return ref


def _close(dev, ref, n, what):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    assert dev.shape == ref.shape, what
    scale = np.maximum(dev, ref)
    err = np.abs(dev - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, 0.0)
    print(f"{what}: largest relative difference {rel.max() if rel.size else 0.0:.3e}, bound {8 * n * 2.0 ** -53:.3e}")
    assert np.all(np.isfinite(dev)), what
    assert np.all(dev[ref == 0.0] == 0.0), what
    assert np.all(err <= 8 * n * 2.0 ** -53 * scale), what


def _check(eng, first, count, what, refs=None, **ask):
    """one summary call of slots [first, first + count) against the per-slot references; returns (summary, references by slot)"""
    summ = eng.belief_summary(first, count, **ask)
    n = eng.cfg.particles
    weighted = eng.cfg.belief == N.BELIEF_IMPORTANCE
    refs = {} if refs is None else refs
    for b in range(count):
        e = first + b
        if e not in refs:
            refs[e] = _reference(eng, e)
        ref, w = refs[e], f"{what}, slot {e}"
        assert summ.particles[b] == n and summ.weighted[b] == int(weighted)
        _close(summ.weight_total[b], ref["weight_total"], n, w + ": weight_total")
        _close(summ.weight_sq_total[b], ref["weight_sq_total"], n, w + ": weight_sq_total")
        _close(summ.ess[b], ref["weight_total"] ** 2 / ref["weight_sq_total"], n, w + ": ess")
        if not weighted:
            assert summ.weight_total[b] == n == summ.weight_sq_total[b] and summ.ess[b] == n
        if summ.state_mass is not None:
            _close(summ.state_mass[b], ref["state_mass"], n, w + ": state_mass")
            if not weighted:
                assert np.array_equal(summ.state_mass[b], ref["state_mass"]), w
        if ask.get("mean_counts", True):
            _close(summ.mean_counts[b], ref["mean_counts"], n, w + ": mean_counts")
        if ask.get("edge_prob", True):
            if ref["edge_prob"] is None:
                assert summ.edge_prob is None
            else:
                _close(summ.edge_prob[b], ref["edge_prob"], n, w + ": edge_prob")
    return summ, refs


def _obs_for(eng, kind, e, step):
    """an observation slot e's filter can produce: 0 / 1 for the tigers (every action gives both), else what a particle of the filter
    would see without noise from where it is -- a step that fails leaves it there, and the observation noise allows the exact reading"""
    if kind == "tiger":
        return (e + step) % 2
    s, _, _ = eng.belief_get(e, weights=False, counts=False)
    st = int(s[(7 * e + 3 * step) % len(s)])
    return st if kind == "gridworld" else st % eng.O      # collision avoidance: the state's last digits are the obstacles' rows


def _drive(eng, kind, what, **ask):
    """belief_init, reset, three per-call updates in slots at different (run, episode, t), a check after the reset and after each update"""
    E, ba = eng.slots, eng.cfg.model != POMDP
    run = np.array([5 + 1000 * e for e in range(E)], np.int32)
    episode = np.array([e % 2 for e in range(E)], np.int32) if ba else np.zeros(E, np.int32)
    t = np.array([e % 3 for e in range(E)], np.int32)
    eng.set_position(run=run, episode=0, t=0)
    eng.belief_init()
    eng.set_position(run=run, episode=episode, t=0)
    if ba:
        eng.belief_reset_domain_state()
    out = [_check(eng, 0, E, what + ", after the reset", **ask)]
    for step in range(3):
        eng.set_position(t=t + step)
        action = np.array([(e + step // 2) % eng.A for e in range(E)], np.int32)      # (two steps of one action: cells raised twice)
        obs = np.array([_obs_for(eng, kind, e, step) for e in range(E)], np.int32)
        eng.belief_update(action, obs)
        out.append(_check(eng, 0, E, f"{what}, after update {step}", **ask))
    return out


FORMATS = [
    ("dense_tiger", "tiger", "continuous-tiger", TABLE, IS, DENSE_ENV, {}, lambda e: _dense_bytes(24)),
    ("dense_factored_tiger2", "tiger", "continuous-factored-tiger", FACT, IS, None, dict(size=2, structure_prior=2), lambda e: _dense_bytes(e.ncnt)),
    ("packed_tiger", "tiger", "continuous-tiger", TABLE, REJ, None, {}, lambda e: 64),
    ("packed_factored_tiger2", "tiger", "continuous-factored-tiger", FACT, REJ, None, dict(size=2, structure_prior=2), lambda e: _packed_ftiger_bytes(2)),
    ("gridworld3_history_importance", "gridworld", "gridworld", FACT, IS, None, dict(size=3, structure_prior=2), lambda e: _record_bytes()),
    ("gridworld3_history_rejection", "gridworld", "gridworld", FACT, REJ, None, dict(size=3, structure_prior=2), lambda e: _record_bytes()),
    ("gridworld3_table_history", "gridworld", "gridworld", TABLE, IS, None, dict(size=3), lambda e: _record_bytes()),
    ("collision_avoidance_5x5x2_history", "ca", "random-collision-avoidance", FACT, IS, MULTI_ENV, dict(width=5, height=5, size=2), lambda e: _record_bytes()),
]


@pytest.mark.parametrize("name,kind,domain,model,belief,env,kw,nbytes", FORMATS, ids=[f[0] for f in FORMATS])
def test_every_record_format(name, kind, domain, model, belief, env, kw, nbytes, monkeypatch):
    eng = _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=7100 + len(name), **kw)
    assert eng.particle_bytes == nbytes(eng), name
    out = _drive(eng, kind, name)
    summ, refs = out[-1]
    if name == "dense_factored_tiger2":    # parent sets differ between the particles of a slot
        assert np.any((summ.edge_prob > 0) & (summ.edge_prob < 1))
    if name.startswith("gridworld3_history"):   # both goal-parent forms of an x / y node in one slot
        assert any(np.any(np.any(r["masks"] == 7, axis=0) & np.any(r["masks"] == 3, axis=0)) for r in refs.values())
        assert np.any((summ.edge_prob[:, :, 2] > 0) & (summ.edge_prob[:, :, 2] < 1))
        assert np.all(summ.edge_prob[:, :, 3:] == 0.0)
    if model == TABLE or name.startswith("collision"):
        assert summ.edge_prob is None
    if "history" in name:       # _drive's two steps of one action: some particle holds a cell that two of its entries raised
        prior, (nc, _) = eng.prior(), _layout(eng)
        lo = 0
        if name.startswith("gridworld3_history"):   # the observation nodes' cells, the last ones: their prior is the same under every parent set
            lay = eng.factored_layout()
            lo = nc - eng.A * sum(int(s) ** 2 for s in lay.obs_feature_size[:lay.n_obs_features])
            assert lo == nc - eng.A * (2 * 3 * 3 + 3 * 3)
        raised = max(float(np.max(r["counts"][:, lo:nc] - prior[None, lo:nc])) for r in refs.values())
        print(f"{name}: a cell stands {raised} above the prior")
        assert raised >= 2.0
    eng.close()


def test_collision_avoidance_7x7x2_inexact_prior(monkeypatch):
    """a raised cell's value is the prior after single additions of 1.0f (the sequence table), not prior + multiplicity"""
    eng = _engine(monkeypatch, "random-collision-avoidance", FACT, IS, MULTI_ENV, width=7, height=7, size=2, particles=130, slots=3, runs=3, seed=7191)
    assert eng.particle_bytes == _record_bytes()
    for v in INEXACT:
        c = np.float32(v)
        assert np.float32(np.float32(c + np.float32(1)) + np.float32(1)) != np.float32(c + np.float32(2))
    prior = eng.prior()
    cells = np.nonzero(prior > 0)[0]
    new = prior.copy()
    new[cells] = np.asarray(INEXACT, np.float32)[np.arange(cells.size) % len(INEXACT)]
    eng.set_model_factored(new)
    out = _drive(eng, "ca", "collision avoidance 7 x 7 x 2, inexact prior")
    _, refs = out[-1]
    assert sum(int(np.sum((r["counts"] - new[None, :] >= 2) & (new[None, :] > 0))) for r in refs.values()) > 0   # a cell raised twice
    eng.close()


def test_plain_pomdp_serves_head_and_state_mass(monkeypatch):
    eng = _engine(monkeypatch, "continuous-tiger", POMDP, REJ, particles=130, slots=3, runs=3, seed=7201)
    assert eng.ncnt == 0
    out = _drive(eng, "tiger", "planning tiger", mean_counts=False, edge_prob=False)
    summ, _ = out[-1]
    assert summ.mean_counts is None and summ.edge_prob is None and summ.state_mass.shape == (3, eng.S)
    eng.close()


@pytest.mark.parametrize("particles", [1, 257])
@pytest.mark.parametrize("name", ["dense_tiger", "gridworld3_history_importance"])
def test_other_particle_counts(name, particles, monkeypatch):
    _, kind, domain, model, belief, env, kw, nbytes = next(f for f in FORMATS if f[0] == name)
    eng = _engine(monkeypatch, domain, model, belief, env, particles=particles, slots=3, runs=3, seed=7300 + particles, **kw)
    assert eng.particle_bytes == nbytes(eng)
    _drive(eng, kind, f"{name}, {particles} particles")
    eng.close()


def test_lazy_reset(monkeypatch):
    """the rejection filter's reset is only flagged: the summary right behind it sees the new states, belief_get afterwards agrees"""
    eng = _engine(monkeypatch, "continuous-tiger", TABLE, REJ, DENSE_ENV, particles=130, slots=3, runs=3, seed=7401)
    assert eng.particle_bytes == _dense_bytes(24)
    eng.set_position(run=[3, 40, 500], episode=0, t=0)
    eng.belief_init()
    eng.belief_reset_domain_state()
    eng.belief_update([2, 2, 2], [0, 1, 0])
    before = eng.belief_summary().state_mass
    eng.set_position(episode=1, t=0)
    eng.belief_reset_domain_state()
    summ = eng.belief_summary()
    hist = np.stack([np.bincount(eng.belief_get(e, counts=False)[0], minlength=eng.S) for e in range(3)])
    assert np.array_equal(summ.state_mass, hist.astype(np.float64))
    assert not np.array_equal(before, summ.state_mass)      # (the listen updates had moved the mass to one door)
    eng.close()


def test_unequal_weights(monkeypatch):
    eng = _engine(monkeypatch, "continuous-factored-tiger", FACT, IS, size=2, structure_prior=2, particles=200, slots=2, runs=2, seed=7501)
    eng.set_position(run=[1, 2], episode=0, t=0)
    eng.belief_init()
    eng.belief_reset_domain_state()
    eng.belief_update([2, 0], [1, 0])
    g = np.random.default_rng(7501)
    for e in range(2):
        w = g.random(200) * 10.0 ** g.integers(-6, 3, 200)
        w[g.choice(200, 5, replace=False)] = 0.0
        assert np.all(w >= 0) and np.sum(w == 0) == 5
        eng.belief_set(e, weight=w)
    summ, refs = _check(eng, 0, 2, "random weights")
    for e in range(2):
        assert 1.0 < summ.ess[e] < 200.0
    eng.close()


def test_slot_ranges_in_a_wide_context(monkeypatch):
    eng = _engine(monkeypatch, "gridworld", FACT, IS, size=3, structure_prior=2, particles=64, slots=70, runs=70, horizon=7, sims=32, seed=7601)
    assert eng.particle_bytes == 4 * ((2 + EPISODES * 7 + 3) // 4 * 4)
    eng.run_ticks(1)
    eng.run_ticks(1)
    whole, refs = _check(eng, 0, 70, "slots 0..69")
    tail, _ = _check(eng, 66, 4, "slots 66..69", refs=refs)
    one, _ = _check(eng, 5, 1, "slot 5", refs=refs)
    for name in ("weight_total", "weight_sq_total", "state_mass", "mean_counts", "edge_prob"):
        _close(getattr(tail, name), getattr(whole, name)[66:70], 64, f"{name}: the calls on slots 66..69")
        _close(getattr(one, name), getattr(whole, name)[5:6], 64, f"{name}: the calls on slot 5")
    assert any(not np.array_equal(whole.mean_counts[0], whole.mean_counts[e]) for e in range(1, 70))
    eng.close()


@pytest.mark.parametrize("name,lazy", [("gridworld3_history_importance", False), ("packed_tiger", True), ("dense_factored_tiger2", False)])
def test_read_only(name, lazy, monkeypatch):
    """two contexts of one seed, one takes summaries on the way: every particle, counter, action and step record keeps its bits"""
    _, kind, domain, model, belief, env, kw, _ = next(f for f in FORMATS if f[0] == name)
    seen = []
    for with_summary in (True, False):
        eng = _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=7700, trace=1, **kw)
        got = []
        eng.set_position(run=[11, 12, 13], episode=0, t=0)
        eng.belief_init()
        eng.belief_reset_domain_state()
        if not lazy:      # (belief_get would write a lazily reset filter out in both contexts: there the summary comes first)
            obs = np.array([_obs_for(eng, kind, e, 0) for e in range(3)], np.int32)
            eng.belief_update([0, 1, 2], obs)
        if with_summary:
            eng.belief_summary()
            eng.belief_summary(1, 2, mean_counts=False)
        if not lazy:
            got += [x for e in range(3) for x in eng.belief_get(e)]
        c = eng.counters()
        got.append(np.array([c.sim_steps, c.belief_steps, c.env_steps]))
        eng.set_position(t=1)
        action = eng.select_action(hist_len=1)
        got.append(action)
        if with_summary:
            eng.belief_summary()
        obs = np.array([_obs_for(eng, kind, e, 1) for e in range(3)], np.int32)
        eng.belief_update(action, obs)
        if with_summary:
            eng.belief_summary(0, 1)
        got += [x for e in range(3) for x in eng.belief_get(e)]
        got.append(eng.last_step_info())
        c = eng.counters()
        got.append(np.array([c.sim_steps, c.belief_steps, c.env_steps]))
        seen.append(got)
        eng.close()
    assert len(seen[0]) == len(seen[1])
    for a, b in zip(seen[0], seen[1]):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()


def test_refusals(monkeypatch):
    nested = _engine(monkeypatch, "continuous-tiger", TABLE, "nested", particles=12, slots=2, runs=2)
    with pytest.raises(ValueError, match="fba_belief_get_nested"):
        nested.belief_summary()
    nested.close()
    eng = _engine(monkeypatch, "continuous-tiger", TABLE, IS, particles=32, slots=3, runs=3)
    eng.belief_init()
    with pytest.raises(ValueError, match="slots"):
        eng.belief_summary(0, 4)
    with pytest.raises(ValueError, match="slots"):
        eng.belief_summary(2, 2)
    with pytest.raises(ValueError, match="slots"):
        eng.belief_summary(-1, 2)
    assert eng.L.fba_belief_summary(eng.h, 0, 3, None, None, None, None) == N.OK
    assert eng.belief_summary(1, 2).mean_counts.shape == (2, eng.ncnt)
    eng.close()
    plan = _engine(monkeypatch, "continuous-tiger", POMDP, REJ, particles=32, slots=2, runs=2)
    plan.belief_init()
    with pytest.raises(ValueError, match="POMDP"):
        plan.belief_summary(mean_counts=True, edge_prob=False)
    with pytest.raises(ValueError, match="POMDP"):
        plan.belief_summary(mean_counts=False, edge_prob=True)
    assert plan.belief_summary(mean_counts=False, edge_prob=False).state_mass.sum() == 2 * 32
    plan.close()
