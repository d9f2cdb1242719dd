"""fba_probe / Engine.probe_enable / Engine.probe: the evidence of every real step, recorded from inside the tick.

The yardstick is existing code, never the probe.  Three contexts are created alike, with the same seed and trace = 1:
    P   has the probe on and runs run_ticks(K) in one call;
    T   has no probe and is advanced one run_ticks(1) at a time: its last_step_info() after tick k names the step of every slot in
        tick k -- action, observation, true new state, terminal or not.  (P's own trace says the same for the records it has room for,
        slots * episodes * horizon of them, and is compared with T's record for record; K may be larger than that.)
    R   has no probe and is advanced the same way, but before tick k it is asked for belief_forecast(action_k, obs_k) on all slots --
        fba_belief_forecast, which test_gpu_belief_forecast.py holds to numpy -- and after the tick its last_step_info() must equal
        T's bit for bit: the forecast and the probe disturbed nothing.
Every non-terminal step must then have exactly one probe record whose slot, action, obs and state are the step's and whose evidence,
next_true and post_true are fc.evidence[e], fc.next_mass[e][state] and fc.post_mass[e][state] within the bounds of include/fba_hip.h:
both sides are within the first-order bound of the exact value (the docstring of test_gpu_belief_forecast.py derives it; the probe's
factorised form makes fewer additions than the enumeration, TL + R against S * nodes), and twice that is below the stated 8 * terms *
2^-53.  An entry is exactly 0.0 where the forecast's is.  Terminal steps have no record."""
import numpy as np
import pytest

from test_gpu_belief_forecast import FACT, FORMATS, IS, POMDP, REJ, TABLE, _Slot, _close, _engine, _format

pytestmark = pytest.mark.gpu

KEY = ("run", "episode", "t")


def _key(rec):
    return tuple(int(rec[k]) for k in KEY)


def _terms(eng):
    """(L, FT, FA) of the bounds: the longest row, the transition nodes of an action, all nodes of a step"""
    if eng.cfg.model != FACT:
        return max(eng.S, eng.O), 1, 2
    lay = eng.factored_layout()
    return max(lay.node[k].out for k in range(lay.n_nodes)), lay.n_state_features, lay.n_state_features + lay.n_obs_features


def _factorises(eng):
    """from the layout: does every observation node of every action have at most one parent, whatever a particle's parent-set words
    say?  A node with a parent-set word may have as many parents as it has candidates."""
    lay = eng.factored_layout()
    FS, FO = lay.n_state_features, lay.n_obs_features
    for a in range(eng.A):
        for g in range(FO):
            node = lay.node[eng.A * FS + a * FO + g]
            low = (1 << node.n_candidates) - 1
            parents = node.n_candidates if node.mask_word >= 0 else bin(node.fixed_mask & low).count("1")
            if parents > 1:
                return False
    return True


def _match(pr, step, fc_ev, fc_next, fc_post, eng, what):
    """one probe record against the step it belongs to and the forecast of the slot before the step"""
    n, S = eng.cfg.particles, eng.S
    L, FT, FA = _terms(eng)
    tn, tp = n + FT * (L + 2), n + FA * (L + 2)
    for f in ("action", "obs", "state"):
        assert int(pr[f]) == int(step[f]), f"{what}: {f}"
    _close(pr["evidence"], fc_ev, tp + S, what + ": evidence")
    _close(pr["next_true"], fc_next, tn, what + ": next_true")
    _close(pr["post_true"], fc_post, tp, what + ": post_true")


def _probe_against_forecast(make, K, what, numpy_tick=None, first=0, count=None):
    """P runs K ticks with the probe on [first, first + count); T and R follow tick by tick.  Returns P's records, the steps by key, the
    number of terminal steps and R (open, at the state after the last tick)."""
    P = make()
    E = P.slots
    count = E - first if count is None else count
    P.probe_enable(first=first, count=count, capacity=K * E)
    P.run_ticks(K)
    recs = P.probe()
    ptrace = P.trace()
    assert recs.seen == recs.size
    by_key = {}
    for r in recs:
        assert _key(r) not in by_key, f"{what}: two records of step {_key(r)}"
        by_key[_key(r)] = r
    T, R = make(), make()
    T.run_ticks(0)
    R.run_ticks(0)
    steps, used = {}, set()
    terminal = 0
    for k in range(K):
        T.run_ticks(1)
        info = T.last_step_info().copy()
        fc = R.belief_forecast(info["action"], info["obs"])          # (before any belief_get: a lazily reset filter stays lazy)
        refs = {}
        if k == numpy_tick:
            refs = {e: _Slot(R, e).forecast(int(info["action"][e]), int(info["obs"][e])) for e in range(first, first + count)}
        R.run_ticks(1)
        assert R.last_step_info().tobytes() == info.tobytes(), f"{what}: tick {k}"
        for e in range(E):
            step = info[e]
            steps[_key(step)] = step
            w = f"{what}, tick {k}, slot {e}"
            if step["terminal"] or not first <= e < first + count:
                terminal += int(step["terminal"])
                assert _key(step) not in by_key, w + ": a record of a step without an update, or outside the range"
                continue
            assert _key(step) in by_key, w + ": no record"
            pr = by_key[_key(step)]
            used.add(_key(step))
            assert int(pr["slot"]) == e, w
            s = int(step["state"])
            _match(pr, step, fc.evidence[e], fc.next_mass[e][s], fc.post_mass[e][s], P, w)
            if e in refs:      # an enumeration nobody on the device made
                _match(pr, step, refs[e]["evidence"], refs[e]["next_mass"][s], refs[e]["post_mass"][s], P, w + ", numpy")
    assert used == set(by_key), f"{what}: records of no step"
    # P's trace, as far as it has room, is T's: the probe disturbed nothing
    assert len(ptrace) == min(K * E, E * max(P.cfg.episodes, 1) * P.cfg.horizon)
    for r in ptrace:
        assert r.tobytes() == steps[_key(r)].tobytes(), f"{what}: trace record {_key(r)}"
    for eng in (P, T):
        eng.close()
    return recs, steps, terminal, R


@pytest.mark.parametrize("name,kind,domain,model,belief,env,kw,nbytes", FORMATS, ids=[f[0] for f in FORMATS])
def test_every_record_format(name, kind, domain, model, belief, env, kw, nbytes, monkeypatch):
    """130 particles, 3 slots, 2 episodes of 8 steps, 18 ticks: the first step of episode 1 probes a freshly (under rejection: lazily)
    reset filter, the last two ticks the freshly initiated filter of the next run"""
    make = lambda: _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=7100 + len(name), trace=1, **kw)
    numpy_tick = 5 if name in ("gridworld3_history_importance", "sysadmin3_dense") else None
    recs, steps, _, R = _probe_against_forecast(make, 2 * 8 + 2, name, numpy_tick=numpy_tick)
    assert R.particle_bytes == nbytes(R), name
    if model == FACT:
        expect = kind != "tiger" or domain == "independent-sysadmin"     # gridworld, collision avoidance, sysadmin; not the factored tiger
        assert _factorises(R) == expect, name
        if not expect:      # ... through listen's parent-set word: some particle's observation node has two or more parents
            lay = R.factored_layout()
            FS, FO = lay.n_state_features, lay.n_obs_features
            many = False
            for e in range(R.slots):
                cnt = R.belief_get(e, weights=False)[2]
                words = np.ascontiguousarray(cnt[:, lay.n_counts:]).view(np.uint32)
                for a in range(R.A):
                    for g in range(FO):
                        node = lay.node[R.A * FS + a * FO + g]
                        if node.mask_word >= 0:
                            w = words[:, node.mask_word] & np.uint32((1 << node.n_candidates) - 1)
                            many = many or bool(np.any(np.array([bin(int(x)).count("1") for x in w]) > 1))
            assert many, name + ": no particle enumerates"
    assert np.any((recs["evidence"] > 0) & (recs["evidence"] < 1)), name
    assert any(a["slot"] != b["slot"] and a["evidence"] != b["evidence"] for a in recs for b in recs if _key(a)[1:] == _key(b)[1:]), name + ": two slots differ"
    assert {int(r["episode"]) for r in recs} == {0, 1}, name
    R.close()


@pytest.mark.parametrize("particles", [1, 257])
@pytest.mark.parametrize("name", ["dense_tiger", "packed_factored_tiger2", "gridworld3_history_importance", "gridworld3_table_history"])
def test_other_particle_counts(name, particles, monkeypatch):
    _, kind, domain, model, belief, env, kw, nbytes = _format(name)
    make = lambda: _engine(monkeypatch, domain, model, belief, env, particles=particles, slots=3, runs=3, seed=7300 + particles, trace=1, **kw)
    _, _, _, R = _probe_against_forecast(make, 2 * 8 + 2, f"{name}, {particles} particles")
    assert R.particle_bytes == nbytes(R)
    R.close()


def test_terminal_steps_have_no_record(monkeypatch):
    make = lambda: _engine(monkeypatch, "episodic-tiger", TABLE, REJ, None, particles=64, slots=8, runs=8, seed=7400, trace=1, sims=32)
    recs, steps, terminal, R = _probe_against_forecast(make, 12, "episodic tiger")
    assert terminal > 0
    assert {_key(r) for r in recs} == {k for k, s in steps.items() if not s["terminal"]}
    assert len(steps) == 12 * 8
    R.close()


@pytest.mark.parametrize("name", ["gridworld3_history_importance", "packed_tiger"])
def test_a_range_in_a_wide_context(name, monkeypatch):
    _, kind, domain, model, belief, env, kw, _ = _format(name)
    make = lambda: _engine(monkeypatch, domain, model, belief, env, particles=64, slots=70, runs=70, horizon=7, sims=16, seed=7601, trace=1, **kw)
    part, _, _, R = _probe_against_forecast(make, 3, name + ", slots 37..41", first=37, count=5)
    R.close()
    assert part.size == 3 * 5 and set(part["slot"].tolist()) == {37, 38, 39, 40, 41}
    W = make()
    W.probe_enable(capacity=3 * 70)
    W.run_ticks(3)
    whole = W.probe()
    assert whole.size == 3 * 70
    n, S = 64, W.S
    L, FT, FA = _terms(W)
    by_key = {_key(r): r for r in whole}
    for r in part:
        w = by_key[_key(r)]
        for f in ("slot", "action", "obs", "state"):
            assert r[f] == w[f]
        _close(r["evidence"], w["evidence"], n + S + FA * (L + 2), f"{name}: evidence of {_key(r)}")
        _close(r["next_true"], w["next_true"], n + FT * (L + 2), f"{name}: next_true of {_key(r)}")
        _close(r["post_true"], w["post_true"], n + FA * (L + 2), f"{name}: post_true of {_key(r)}")
    W.close()


def test_a_search_budget(monkeypatch):
    """budgeted launches: a real step takes several launches, and env_kernel flags the update of the slots that stepped in this one only"""
    _, kind, domain, model, belief, env, kw, _ = _format("gridworld3_history_importance")
    got = []
    for budget in (37, 0):
        eng = _engine(monkeypatch, domain, model, belief, env, particles=64, slots=20, runs=20, seed=7700, trace=1, search_budget=budget, **kw)
        eng.probe_enable()
        eng.run_bapomdp()
        recs, tr = eng.probe(), eng.trace()
        assert recs.seen == recs.size
        keys = [_key(r) for r in recs]
        assert len(set(keys)) == len(keys)
        assert set(keys) == {_key(r) for r in tr if not r["terminal"]}
        assert len(tr) > 20 * 2
        by = {_key(r): r for r in tr}
        for r in recs:
            for f in ("action", "obs", "state"):
                assert r[f] == by[_key(r)][f]
            assert r["slot"] == r["run"] % 20
        got.append((recs, tr, eng.S, _terms(eng)))
        eng.close()
    (b, btr, S, (L, FT, FA)), (u, utr, _, _) = got
    assert btr.tobytes() == utr.tobytes()
    assert [_key(r) for r in b] == [_key(r) for r in u]
    _close(b["evidence"], u["evidence"], 64 + S + FA * (L + 2), "budgeted against whole searches: evidence")
    _close(b["next_true"], u["next_true"], 64 + FT * (L + 2), "budgeted against whole searches: next_true")
    _close(b["post_true"], u["post_true"], 64 + FA * (L + 2), "budgeted against whole searches: post_true")


def test_capacity(monkeypatch):
    _, kind, domain, model, belief, env, kw, _ = _format("packed_tiger")
    make = lambda: _engine(monkeypatch, domain, model, belief, env, particles=64, slots=4, runs=4, seed=7800, trace=1, **kw)
    eng, twin = make(), make()
    eng.probe_enable(capacity=5)
    eng.run_ticks(3)
    twin.run_ticks(3)
    recs = eng.probe()
    assert recs.size == 5 and recs.seen == 12
    assert np.all((recs["evidence"] > 0) & (recs["evidence"] <= 1))
    assert eng.trace().tobytes() == twin.trace().tobytes()
    assert eng.last_step_info().tobytes() == twin.last_step_info().tobytes()
    eng.probe_enable(count=0)
    eng.run_ticks(1)
    twin.run_ticks(1)
    off = eng.probe()
    assert off.size == 0 and off.seen == 0
    assert eng.trace().tobytes() == twin.trace().tobytes()
    # enabling again clears the buffer
    eng.probe_enable(capacity=100)
    assert eng.probe().size == 0
    eng.run_ticks(1)
    assert eng.probe().size == 4 and eng.probe().seen == 4
    eng.close()
    twin.close()


def _snapshot(eng):
    return [x for e in range(eng.slots) for x in eng.belief_get(e)] + [eng.last_step_info()]


@pytest.mark.parametrize("name", ["gridworld3_history_importance", "packed_tiger", "dense_factored_tiger2", "gridworld3_history_rejection"])
def test_read_only(name, monkeypatch):
    """two contexts created alike, one with the probe on, over run_ticks and over run_bapomdp: every particle, every field of the step
    records (belief_hash and root_q among them), the trace, the returns and the counters keep their bits"""
    _, kind, domain, model, belief, env, kw, _ = _format(name)
    seen = []
    for probed in (True, False):
        got = []
        eng = _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=7900, trace=1, **kw)
        if probed:
            eng.probe_enable()
        eng.run_ticks(2)
        got += _snapshot(eng)
        eng.run_ticks(9)           # (into the second episode)
        got += _snapshot(eng)
        got.append(eng.trace())
        c = eng.counters()
        got.append(np.array([c.sim_steps, c.belief_steps, c.env_steps]))
        if probed:
            assert eng.probe().size == int(np.sum(got[-2]["terminal"] == 0)) >= 3 * 9
        eng.close()
        eng = _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=6, seed=7901, trace=1, **kw)
        if probed:
            eng.probe_enable(first=1, count=2)
        stats = eng.run_bapomdp()
        got.append(np.array([[s.count, s.mean, s.m2] for s in stats]))
        got += list(eng.returns())
        got.append(eng.trace())
        got += _snapshot(eng)
        c = eng.counters()
        got.append(np.array([c.sim_steps, c.belief_steps, c.env_steps]))
        if probed:
            recs, tr = eng.probe(), eng.trace()
            assert {_key(r) for r in recs} == {_key(r) for r in tr if not r["terminal"] and r["run"] % 3 in (1, 2)}
            assert recs.size > 0 and set(recs["slot"].tolist()) == {1, 2}
        eng.close()
        seen.append(got)
    assert len(seen[0]) == len(seen[1])
    for a, b in zip(seen[0], seen[1]):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()


def test_refusals(monkeypatch):
    nested = _engine(monkeypatch, "continuous-tiger", TABLE, "nested", particles=12, slots=2, runs=2)
    with pytest.raises(ValueError, match="fba_belief_get_nested"):
        nested.probe_enable()
    nested.close()
    plan = _engine(monkeypatch, "continuous-tiger", POMDP, REJ, particles=32, slots=2, runs=2)
    with pytest.raises(ValueError, match="POMDP"):
        plan.probe_enable()
    plan.close()
    eng = _engine(monkeypatch, "continuous-tiger", TABLE, IS, particles=32, slots=3, runs=3)
    for first, count in ((0, 4), (2, 2), (-1, 2), (0, -1)):
        with pytest.raises(ValueError, match="slots"):
            eng.probe_enable(first=first, count=count)
    with pytest.raises(ValueError, match="capacity of -1"):
        eng.probe_enable(capacity=-1)
    assert eng.probe().size == 0 and eng.probe().seen == 0
    eng.close()


def test_a_slot_without_weight_gives_zeros(monkeypatch):
    """the header: a slot whose weights are all 0 gives zeros; the other slots are what they are without it"""
    _, kind, domain, model, belief, env, kw, _ = _format("dense_factored_tiger2")
    make = lambda: _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=7950, trace=1, **kw)
    out = []
    for zero in (True, False):
        eng = make()
        L, FT, FA = _terms(eng)
        eng.run_ticks(1)
        if zero:
            eng.belief_set(1, weight=np.zeros(130))
        eng.probe_enable()
        eng.run_ticks(1)
        out.append(eng.probe())
        eng.close()
    z, ref = out
    assert z.size == 3 and ref.size == 3 and list(z["slot"]) == [0, 1, 2] == list(ref["slot"])
    assert z["evidence"][1] == 0.0 and z["next_true"][1] == 0.0 and z["post_true"][1] == 0.0
    assert ref["evidence"][1] > 0
    for e in (0, 2):
        for f in ("action", "obs", "state"):
            assert z[f][e] == ref[f][e]
        assert z["evidence"][e] > 0
        for f in ("evidence", "next_true", "post_true"):
            _close(z[f][e], ref[f][e], 130 + (eng.S if f == "evidence" else 0) + (FT if f == "next_true" else FA) * (L + 2), f"slot {e}: {f}")
