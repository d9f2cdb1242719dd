"""fba_belief_forecast / Engine.belief_forecast: the filter's one-step predictive evaluated on the device from every record format,
against numpy over Engine.belief_get of the same slot plus factored_layout().  The reference is written from the layout comment of
include/fba_hip.h, as the reference of test_gpu_belief_predict.py is: per particle each node's parent set is the mask word at
n_counts + mask_word (or fixed_mask), the row index is "for j in candidate order, if bit j set: idx = idx * candidate_size[j] +
v[candidate[j]]", rows are normalised in fp64 and a row that sums to 0 gives 0; tabular rows are phi[s*A*S + a*S + s'] and
psi[a*S*O + s'*O + o].  Here the row of a transition node is chosen by each particle's OWN domain state s_i, the row of an observation
node by the next state s', and
    next_mass[s'] = sum_i w_i p_i(s') / W,   post_mass[s'] = sum_i w_i p_i(s') l_i(s') / W,   evidence = sum_s' post_mass[s'].

Bound (derived, not measured): every entry is a sum of at most N non-negative terms, each a weight times at most F quotients, each
quotient's denominator an fp64 sum of at most L fp32 values (on the device, for a history record, the prior row's L values and then at
most L raised cells: 2 L additions).  A sum of L non-negative values is within (L - 1) * 2^-53 relative of the exact one in any order,
the quotient adds one rounding, the product with the weight (or the next factor) one more, the sum over the particles at most N - 1,
the division by the weight total (itself within N * 2^-53, counted in the N of the other side) one: to first order the reference is
within (N + F * (L + 2) + 2) * 2^-53 relative of the exact value and the device within (N + F * (2 L + 2) + 2) * 2^-53, together below
    |dev - ref| <= 8 * (N + F * (L + 2)) * 2^-53 * max(dev, ref)
per entry, with F = the transition nodes of an action for next_mass (1 for a tabular model) and all nodes of a step for post_mass (2
for a tabular model), L the longest row of the case; evidence adds the S - 1 additions over the next states:
8 * (N + S + F * (L + 2)) * 2^-53.  Exactly 0.0 wherever the reference is 0.0 (a zero sum of non-negative terms has only zero terms).
One lost increment of one particle moves an entry by about 1 / (N * R) for a row sum R; at R = 10^4 that is still ten orders of
magnitude above the bound."""
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
# c + 2.0f is not (c + 1.0f) + 1.0f in fp32 for these
INEXACT = [0.002, 0.009, 0.011, 0.015]
U = 2.0 ** -53


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


def _features(index, sizes):
    """the features of an index in mixed radix, last feature fastest: [len(index), len(sizes)]"""
    out = np.zeros((len(index), len(sizes)), np.int64)
    rest = np.asarray(index, np.int64).copy()
    for f in range(len(sizes) - 1, -1, -1):
        out[:, f] = rest % sizes[f]
        rest //= sizes[f]
    return out


def _theta(rows):
    tot = rows.sum(axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tot > 0, rows / tot, 0.0)


def _row_index(node, mask, parents):
    """[particles, len(parents)] or, for parents given per particle ([particles, features], own=True below), [particles]"""
    idx = np.zeros((mask.shape[0], parents.shape[0]), np.int64)
    for j in range(node.n_candidates):
        bit = ((mask >> np.uint32(j)) & 1).astype(bool)
        v = parents[:, node.candidate[j]]
        idx = np.where(bit[:, None], idx * node.candidate_size[j] + v[None, :], idx)
    return idx


def _mask_of(node, words):
    return words[:, node.mask_word] if node.mask_word >= 0 else np.full(words.shape[0], node.fixed_mask, np.uint32)


class _Slot:
    """what belief_get holds of one slot, downloaded once, and the forecast numpy makes of it"""

    def __init__(self, eng, slot):
        self.eng = eng
        weighted = eng.cfg.belief == N.BELIEF_IMPORTANCE
        self.s, w, self.cnt = eng.belief_get(slot, weights=weighted)
        self.w = w if weighted else np.ones(self.cnt.shape[0], np.float64)
        self.c64 = self.cnt.astype(np.float64)
        self.n = self.cnt.shape[0]
        self.differ = self.structures = False
        self.zero_rows = False      # a transition row some particle uses sums to 0
        if eng.cfg.model == FACT:
            self.lay = eng.factored_layout()
            self.words = np.ascontiguousarray(self.cnt[:, self.lay.n_counts:]).view(np.uint32)

    def forecast(self, a, o):
        eng, n, c64, w = self.eng, self.n, self.c64, self.w
        S, A, O = eng.S, eng.A, eng.O
        W = w.sum()
        inside = (self.s >= 0) & (self.s < S)
        si = np.where(inside, self.s, 0)
        we = np.where(inside, w, 0.0)
        me = np.arange(n)
        if eng.cfg.model != FACT:
            phi = c64[:, :S * A * S].reshape(n, S, A, S)
            psi = c64[:, S * A * S:].reshape(n, A, S, O)
            rt = phi[me, si, a, :]                    # [n, S]
            ro = psi[:, a, :, :]                      # [n, S, O]
            for v in np.unique(si):
                grp = rt[si == v]
                self.differ = self.differ or bool(np.any(grp.max(axis=0) != grp.min(axis=0)))
            self.differ = self.differ or bool(np.any(ro.max(axis=0) != ro.min(axis=0)))
            self.zero_rows = self.zero_rows or bool(np.any(rt[inside].sum(axis=1) == 0))
            p = _theta(rt)
            l = _theta(ro)[:, :, o]
            L, FT, FA = max(S, O), 1, 2
        else:
            lay = self.lay
            FS, FO = lay.n_state_features, lay.n_obs_features
            ssz, osz = list(lay.state_feature_size[:FS]), list(lay.obs_feature_size[:FO])
            fs_own = _features(si, ssz)                            # [n, FS]
            fs_all = _features(np.arange(S), ssz)                  # [S, FS]
            fo = _features(np.array([o]), osz)[0]
            p, l, L = np.ones((n, S)), np.ones((n, S)), 1
            for f in range(FS):
                node = lay.node[a * FS + f]
                mask = _mask_of(node, self.words)
                self.structures = self.structures or bool(np.any(mask != mask[0]))
                idx = _row_index(node, mask, fs_own)[me, me]       # each particle's row for its OWN state
                start = node.offset + idx * node.out
                rows = c64[me[:, None], start[:, None] + np.arange(node.out)[None, :]]     # [n, out]
                for v in np.unique(start):
                    grp = rows[start == v]
                    self.differ = self.differ or bool(np.any(grp.max(axis=0) != grp.min(axis=0)))
                self.zero_rows = self.zero_rows or bool(np.any(rows[inside].sum(axis=1) == 0))
                p *= _theta(rows)[:, fs_all[:, f]]
                L = max(L, node.out)
            for g in range(FO):
                node = lay.node[A * FS + a * FO + g]
                mask = _mask_of(node, self.words)
                self.structures = self.structures or bool(np.any(mask != mask[0]))
                start = node.offset + _row_index(node, mask, fs_all) * node.out            # [n, S]
                rows = c64[me[:, None, None], start[:, :, None] + np.arange(node.out)[None, None, :]]
                self.differ = self.differ or bool(np.any(rows.max(axis=0) != rows.min(axis=0)))
                l *= _theta(rows)[:, :, fo[g]]
                L = max(L, node.out)
            FT, FA = FS, FS + FO
        nxt = (we[:, None] * p).sum(axis=0) / W
        post = (we[:, None] * p * l).sum(axis=0) / W
        ev = (we * (p * l).sum(axis=1)).sum() / W
        return dict(next_mass=nxt, post_mass=post, evidence=ev, L=L, FT=FT, FA=FA)


def _close(dev, ref, terms, what):
    dev, ref = np.atleast_1d(np.asarray(dev, np.float64)), np.atleast_1d(np.asarray(ref, np.float64))
    assert dev.shape == ref.shape, what
    scale = np.maximum(dev, ref)
    err = np.abs(dev - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, 0.0)
    print(f"{what}: largest relative difference {rel.max() if rel.size else 0.0:.3e}, bound {8 * terms * U:.3e}")
    assert np.all(np.isfinite(dev)), what
    assert np.all(dev[ref == 0.0] == 0.0), what
    assert np.all(err <= 8 * terms * U * scale), what


def _check(eng, first, count, action, obs, what, slots=None, cache=None):
    """one call on slots [first, first + count) with action / obs per slot of the range, against the references of `slots` (all of the
    range by default; `cache`: the _Slot downloads by slot); the identities between the three outputs; returns (forecast, references)"""
    action = np.broadcast_to(np.asarray(action, np.int32), (count,))
    obs = np.broadcast_to(np.asarray(obs, np.int32), (count,))
    fc = eng.belief_forecast(action, obs, first=first, count=count)       # (before any belief_get: a lazily reset filter stays lazy)
    n, S = eng.cfg.particles, eng.S
    assert fc.next_mass.shape == fc.post_mass.shape == (count, S) and fc.evidence.shape == (count,)
    cache = {} if cache is None else cache
    refs = {}
    for e in (range(first, first + count) if slots is None else slots):
        b = e - first
        if e not in cache:
            cache[e] = _Slot(eng, e)
        ref = refs[e] = cache[e].forecast(int(action[b]), int(obs[b]))
        w = f"{what}, slot {e}, action {action[b]}, obs {obs[b]}"
        tn, tp = n + ref["FT"] * (ref["L"] + 2), n + ref["FA"] * (ref["L"] + 2)
        _close(fc.next_mass[b], ref["next_mass"], tn, w + ": next_mass")
        _close(fc.post_mass[b], ref["post_mass"], tp, w + ": post_mass")
        _close(fc.evidence[b], ref["evidence"], tp + S, w + ": evidence")
        # the identities, within the same bounds
        _close(fc.post_mass[b].sum(), fc.evidence[b], tp + S, w + ": the sum of post_mass against evidence")
        if not cache[e].zero_rows:
            _close(fc.next_mass[b].sum(), 1.0, tn + S, w + ": the sum of next_mass")
        assert np.all(fc.post_mass[b] <= fc.next_mass[b] * (1 + 8 * (tn + tp) * U)), w + ": post_mass <= next_mass"
        assert 0.0 <= fc.evidence[b] <= 1 + 8 * (tp + S) * U, w
    return fc, refs


def _obs_for(eng, kind, e, step):
    """an observation slot e's filter can produce: 0 / 1 for the tigers (every action gives both), else what a particle of the filter
    would see without noise from where it is"""
    if kind == "tiger":
        return (e + step) % 2
    s, _, _ = eng.belief_get(e, weights=False, counts=False)
    st = int(s[(7 * e + 3 * step) % len(s)])
    return st if kind == "gridworld" else st % eng.O      # collision avoidance: the state's last digits are the obstacles' rows


def _start(eng):
    E = eng.slots
    run = np.array([5 + 1000 * e for e in range(E)], np.int32)
    episode = np.array([e % 2 for e in range(E)], np.int32)
    eng.set_position(run=run, episode=0, t=0)
    eng.belief_init()
    eng.set_position(run=run, episode=episode, t=0)
    eng.belief_reset_domain_state()


def _drive(eng, kind, what, twin=None, every_action=True):
    """belief_init, reset, three per-call updates in slots at different (run, episode, t); a check after the reset (rejection contexts are
    lazily reset there: the observations come from `twin`, a context created alike, so that this one is not written out first), after each
    update with action (slot + step) % A, and after the last one with every action in turn.  Returns the _Slot downloads and forecasts."""
    E = eng.slots
    t = np.array([e % 3 for e in range(E)], np.int32)
    _start(eng)
    seen = []
    if twin is not None:
        _start(twin)
    obs = np.array([_obs_for(twin if twin is not None else eng, kind, e, 0) for e in range(E)], np.int32)
    cache = {}
    seen.append((_check(eng, 0, E, np.arange(E) % eng.A, obs, what + ", after the reset", cache=cache), cache))
    for step in range(3):
        eng.set_position(t=t + step)
        action = np.array([(e + step // 2) % eng.A for e in range(E)], np.int32)      # (two steps of one action: cells raised twice)
        obs = np.array([_obs_for(eng, kind, e, step) for e in range(E)], np.int32)
        eng.belief_update(action, obs)
        obs = np.array([_obs_for(eng, kind, e, step + 1) for e in range(E)], np.int32)
        cache = {}
        seen.append((_check(eng, 0, E, (np.arange(E) + step) % eng.A, obs, f"{what}, after update {step}", cache=cache), cache))
    if every_action:
        for a in range(eng.A):
            seen.append((_check(eng, 0, E, a, obs, f"{what}, after the updates, action {a}", cache=cache), cache))
    return seen


FORMATS = [
    ("dense_tiger", "tiger", "continuous-tiger", TABLE, IS, DENSE_ENV, {}, lambda e: _dense_bytes(24)),
    ("dense_factored_tiger2", "tiger", "continuous-factored-tiger", FACT, IS, None, dict(size=2, structure_prior=2), lambda e: _dense_bytes(e.ncnt)),
    ("packed_tiger", "tiger", "continuous-tiger", TABLE, REJ, None, {}, lambda e: 64),
    ("packed_factored_tiger2", "tiger", "continuous-factored-tiger", FACT, REJ, None, dict(size=2, structure_prior=2), lambda e: _packed_ftiger_bytes(2)),
    ("gridworld3_history_importance", "gridworld", "gridworld", FACT, IS, None, dict(size=3, structure_prior=2), lambda e: _record_bytes()),
    ("gridworld3_history_rejection", "gridworld", "gridworld", FACT, REJ, None, dict(size=3, structure_prior=2), lambda e: _record_bytes()),
    ("gridworld3_table_history", "gridworld", "gridworld", TABLE, IS, None, dict(size=3), lambda e: _record_bytes()),
    ("collision_avoidance_5x5x2_history", "ca", "random-collision-avoidance", FACT, IS, MULTI_ENV, dict(width=5, height=5, size=2), lambda e: _record_bytes()),
    # (the two below: any fp32 record, whatever its padding)
    ("sysadmin3_dense", "tiger", "independent-sysadmin", FACT, IS, None, dict(size=3), lambda e: max(e.particle_bytes, 4 * (e.ncnt + 1))),
    ("dense_tiger_regular", "tiger", "continuous-tiger", TABLE, IS, None, dict(dirichlet_regular=1), lambda e: _dense_bytes(24)),
]


def _format(name):
    return next(f for f in FORMATS if f[0] == name)


def _not_trivial(seen, name, structures):
    caches = [c for _, c in seen]
    assert any(np.any(s.s != s.s[0]) for c in caches for s in c.values()), name + ": two particles of a slot differ in their state"
    assert any(s.differ for c in caches for s in c.values()), name + ": two particles differ in a row the forecast reads"
    if structures:
        assert any(s.structures for c in caches for s in c.values()), name + ": parent sets differ"
    assert any(np.any((fc.evidence > 0) & (fc.evidence < 1)) for (fc, _), _ in seen), name + ": an evidence strictly between 0 and 1"


@pytest.mark.parametrize("name,kind,domain,model,belief,env,kw,nbytes", FORMATS, ids=[f[0] for f in FORMATS])
def test_every_record_format(name, kind, domain, model, belief, env, kw, nbytes, monkeypatch):
    make = lambda: _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=9100 + len(name), **kw)
    eng = make()
    assert eng.particle_bytes == nbytes(eng), name
    twin = make() if belief == REJ and kind != "tiger" else None
    seen = _drive(eng, kind, name, twin)
    _not_trivial(seen, name, name in ("dense_factored_tiger2", "gridworld3_history_importance", "gridworld3_history_rejection"))
    if kind == "ca":      # the aircraft always moves on: whole columns of the next state have no mass
        assert any(np.any(r["next_mass"] == 0.0) for (_, refs), _ in seen for r in refs.values()), name
    if twin is not None:
        twin.close()
    eng.close()


def test_collision_avoidance_7x7x2_inexact_prior(monkeypatch):
    """a raised cell's value is the prior after single additions of 1.0f, not prior + multiplicity -- in the cell and in its row's sum"""
    eng = _engine(monkeypatch, "random-collision-avoidance", FACT, IS, MULTI_ENV, width=7, height=7, size=2, particles=130, slots=3, runs=3, seed=8191)
    assert eng.particle_bytes == _record_bytes()
    for v in INEXACT:
        c = np.float32(v)
        assert np.float32(np.float32(c + np.float32(1)) + np.float32(1)) != np.float32(c + np.float32(2))
    prior = eng.prior()
    cells = np.nonzero(prior > 0)[0]
    new = prior.copy()
    new[cells] = np.asarray(INEXACT, np.float32)[np.arange(cells.size) % len(INEXACT)]
    eng.set_model_factored(new)
    seen = _drive(eng, "ca", "collision avoidance 7 x 7 x 2, inexact prior")
    # a cell raised twice lies in a row the forecasts after the last update read (every action in turn): a transition row of some particle's
    # own state, or an observation row (every row of the action's observation nodes is read, one per next state)
    lay = eng.factored_layout()
    FS, FO = lay.n_state_features, lay.n_obs_features
    ssz = list(lay.state_feature_size[:FS])
    assert lay.n_mask_words == 0
    hit = 0
    cache = seen[-1][1]
    for e, a in ((e, a) for e in range(3) for a in range(eng.A)):
        sl = cache[e]
        twice = (sl.cnt[:, :lay.n_counts] - new[None, :lay.n_counts] >= 2) & (new[None, :lay.n_counts] > 0)
        own = _features(sl.s, ssz)
        for f in range(FS):
            node = lay.node[a * FS + f]
            start = node.offset + _row_index(node, _mask_of(node, sl.words), own)[np.arange(sl.n), np.arange(sl.n)] * node.out
            hit += int(np.sum(twice[np.arange(sl.n)[:, None], start[:, None] + np.arange(node.out)[None, :]]))
        for g in range(FO):
            node = lay.node[eng.A * FS + a * FO + g]
            rows = int(np.prod([node.candidate_size[j] for j in range(node.n_candidates) if (node.fixed_mask >> j) & 1]))
            hit += int(np.sum(twice[:, node.offset:node.offset + rows * node.out]))
    print(f"cells raised twice in rows the forecasts read: {hit}; in the tables: {sum(int(np.sum((c.cnt[:, :lay.n_counts] - new[None, :lay.n_counts] >= 2) & (new[None, :lay.n_counts] > 0))) for c in cache.values())}")
    assert hit > 0
    obs = np.array([_obs_for(eng, "ca", e, 5) for e in range(3)], np.int32)
    fc, _ = _check(eng, 0, 3, (np.arange(3) + 1) % eng.A, obs, "collision avoidance 7 x 7 x 2, inexact prior, the updates' action", cache=cache)
    assert np.any((fc.evidence > 0) & (fc.evidence < 1))
    eng.close()


@pytest.mark.parametrize("particles", [1, 257])
@pytest.mark.parametrize("name", ["dense_tiger", "packed_factored_tiger2", "gridworld3_history_importance", "gridworld3_table_history"])
def test_other_particle_counts(name, particles, monkeypatch):
    _, kind, domain, model, belief, env, kw, nbytes = _format(name)
    make = lambda: _engine(monkeypatch, domain, model, belief, env, particles=particles, slots=3, runs=3, seed=9300 + particles, **kw)
    eng = make()
    assert eng.particle_bytes == nbytes(eng)
    twin = make() if belief == REJ and kind != "tiger" else None
    _drive(eng, kind, f"{name}, {particles} particles", twin, every_action=False)
    if twin is not None:
        twin.close()
    eng.close()


def test_unequal_weights(monkeypatch):
    _, kind, domain, model, belief, env, kw, _ = _format("gridworld3_history_importance")
    eng = _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=9501, **kw)
    _drive(eng, kind, "before the weights", every_action=False)
    g = np.random.default_rng(9501)
    for e in range(3):
        w = g.random(130) * 10.0 ** g.integers(-6, 3, 130)
        w[g.choice(130, 5, replace=False)] = 0.0
        eng.belief_set(e, weight=w)
    for e in range(3):
        w = eng.belief_get(e, counts=False)[1]
        assert np.unique(w).size > 100 and np.sum(w == 0) == 5
    obs = np.array([_obs_for(eng, kind, e, 4) for e in range(3)], np.int32)
    cache, seen = {}, []
    for a in range(eng.A):
        seen.append((_check(eng, 0, 3, a, obs, f"random weights, action {a}", cache=cache), cache))
    _not_trivial(seen, "random weights", True)
    eng.close()


@pytest.mark.parametrize("name", ["gridworld3_history_importance", "packed_tiger"])
def test_slot_ranges_in_a_wide_context(name, monkeypatch):
    _, kind, domain, model, belief, env, kw, _ = _format(name)
    eng = _engine(monkeypatch, domain, model, belief, env, particles=64, slots=70, runs=70, horizon=7, sims=32, seed=9601, **kw)
    eng.run_ticks(1)
    eng.run_ticks(1)
    action = (np.arange(70) % eng.A).astype(np.int32)
    obs = np.array([_obs_for(eng, kind, e, 0) for e in range(70)], np.int32)
    cache = {}
    pick = lambda lo, n: [e for e in (0, 37, 41, 69) if lo <= e < lo + n]
    whole, refs = _check(eng, 0, 70, action, obs, "slots 0..69", slots=pick(0, 70), cache=cache)
    part, _ = _check(eng, 37, 5, action[37:42], obs[37:42], "slots 37..41", slots=pick(37, 5), cache=cache)
    one, _ = _check(eng, 69, 1, action[69:], obs[69:], "slot 69", slots=pick(69, 1), cache=cache)
    L, FT, FA = refs[0]["L"], refs[0]["FT"], refs[0]["FA"]
    for field, terms in (("next_mass", 64 + FT * (L + 2)), ("post_mass", 64 + FA * (L + 2)), ("evidence", 64 + eng.S + FA * (L + 2))):
        _close(getattr(part, field), getattr(whole, field)[37:42], terms, f"{field}: the calls on slots 37..41")
        _close(getattr(one, field), getattr(whole, field)[69:70], terms, f"{field}: the calls on slot 69")
    assert any(not np.array_equal(whole.next_mass[0], whole.next_mass[e]) for e in range(1, 70))
    eng.close()


@pytest.mark.parametrize("name", ["gridworld3_history_rejection", "collision_avoidance_5x5x2_history", "dense_tiger"])
def test_identities(name, monkeypatch):
    """the sum of post_mass is the evidence, next_mass sums to 1, post_mass <= next_mass (asserted by _check), and next_mass does not
    depend on the observation"""
    _, kind, domain, model, belief, env, kw, _ = _format(name)
    eng = _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=9650, **kw)
    (fc, refs), cache = _drive(eng, kind, name, every_action=False)[-1]
    assert not any(s.zero_rows for s in cache.values())
    only = eng.belief_forecast((np.arange(3) + 2) % eng.A, post_mass=False, evidence=False)
    assert only.post_mass is None and only.evidence is None
    for e in range(3):
        n = 130 + refs[e]["FT"] * (refs[e]["L"] + 2)
        _close(only.next_mass[e], fc.next_mass[e], n, f"{name}: next_mass without an observation, slot {e}")
        _close(only.next_mass[e].sum(), 1.0, n + eng.S, f"{name}: its sum, slot {e}")
    eng.close()


def _snapshot(eng):
    return [x for e in range(eng.slots) for x in eng.belief_get(e)] + [eng.last_step_info()]


@pytest.mark.parametrize("name", ["gridworld3_history_importance", "packed_tiger", "dense_factored_tiger2"])
def test_read_only(name, monkeypatch):
    """two contexts created alike, one asks for forecasts between every pair of per-call steps: every particle and every field of the
    step records (belief_hash and root_q among them) keeps its bits; the same around run_ticks"""
    _, kind, domain, model, belief, env, kw, _ = _format(name)
    seen = []
    for with_forecast in (True, False):
        got = []
        eng = _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=9800, trace=1, **kw)
        ask = lambda: with_forecast and (eng.belief_forecast(np.arange(3) % eng.A, np.arange(3) % eng.O),
                                         eng.belief_forecast(1, first=1, count=2, post_mass=False, evidence=False))
        eng.set_position(run=[11, 12, 13], episode=0, t=0)
        eng.belief_init()
        ask()
        eng.belief_reset_domain_state()
        ask()                                   # (a lazily reset rejection filter stays lazy)
        for step in range(3):
            eng.set_position(t=step)
            action = eng.select_action(hist_len=step)
            got.append(action)
            ask()
            obs = np.array([_obs_for(eng, kind, e, step) for e in range(3)], np.int32)
            eng.belief_update(action, obs)
            ask()
            got += _snapshot(eng)
            info = eng.last_step_info()
            assert "belief_hash" in info.dtype.names and "root_q" in info.dtype.names
        eng.close()
        eng = _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=9801, trace=1, **kw)
        eng.run_ticks(2)
        ask()
        got += _snapshot(eng)
        eng.run_ticks(1)
        ask()
        got += _snapshot(eng)
        c = eng.counters()
        got.append(np.array([c.sim_steps, c.belief_steps, c.env_steps]))
        eng.close()
        seen.append(got)
    assert len(seen[0]) == len(seen[1])
    for a, b in zip(seen[0], seen[1]):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()


def test_refusals(monkeypatch):
    nested = _engine(monkeypatch, "continuous-tiger", TABLE, "nested", particles=12, slots=2, runs=2)
    with pytest.raises(ValueError, match="fba_belief_get_nested"):
        nested.belief_forecast(0, 0)
    nested.close()
    plan = _engine(monkeypatch, "continuous-tiger", POMDP, REJ, particles=32, slots=2, runs=2)
    plan.belief_init()
    with pytest.raises(ValueError, match="POMDP"):
        plan.belief_forecast(0, 0)
    plan.close()
    eng = _engine(monkeypatch, "continuous-tiger", TABLE, IS, particles=32, slots=3, runs=3)
    eng.belief_init()
    for first, count in ((0, 4), (2, 2), (-1, 2)):
        with pytest.raises(ValueError, match="slots"):
            eng.belief_forecast(0, 0, first=first, count=count)
    with pytest.raises(ValueError, match="slot 1: action"):
        eng.belief_forecast([0, eng.A, 0], 0)
    with pytest.raises(ValueError, match="slot 2: observation"):
        eng.belief_forecast(0, [0, eng.O], first=1, count=2)
    with pytest.raises(ValueError, match="slot 0: action"):
        eng.belief_forecast(-1, 0)
    with pytest.raises(ValueError, match="obs is NULL"):
        eng.belief_forecast(0)
    with pytest.raises(ValueError, match="obs is NULL"):
        eng.belief_forecast(0, next_mass=False, post_mass=False)
    # every output off: nothing is done, whatever the arrays hold; next_mass alone needs no observation
    none = eng.belief_forecast(0, next_mass=False, post_mass=False, evidence=False)
    assert none.next_mass is None and none.post_mass is None and none.evidence is None
    assert eng.L.fba_belief_forecast(eng.h, 0, 3, None, None, None, None, None) == N.OK
    only = eng.belief_forecast(2, first=1, count=2, post_mass=False, evidence=False)
    assert only.next_mass.shape == (2, eng.S) and only.post_mass is None and only.evidence is None
    point = _engine(monkeypatch, "continuous-tiger", TABLE, "point_estimate", slots=2, runs=2)
    point.belief_init()
    assert point.cfg.particles == 1
    for a in range(point.A):
        _check(point, 0, 2, a, [0, 1], f"point estimate, action {a}")
    point.close()
    eng.close()


def test_a_slot_without_weight_gives_zeros(monkeypatch):
    """the header: a slot whose weights are all 0 gives 0.0 in every output; the other slots are what they were"""
    _, kind, domain, model, belief, env, kw, _ = _format("dense_factored_tiger2")
    eng = _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=9900, **kw)
    _start(eng)
    before = eng.belief_forecast(1, 0)
    eng.belief_set(1, weight=np.zeros(130))
    fc = eng.belief_forecast(1, 0)
    assert np.all(fc.next_mass[1] == 0.0) and np.all(fc.post_mass[1] == 0.0) and fc.evidence[1] == 0.0
    lay = eng.factored_layout()
    FT, FA = lay.n_state_features, lay.n_state_features + lay.n_obs_features
    L = max(lay.node[k].out for k in range(lay.n_nodes))
    for e in (0, 2):
        _close(fc.next_mass[e], before.next_mass[e], 130 + FT * (L + 2), f"slot {e}: next_mass")
        _close(fc.evidence[e], before.evidence[e], 130 + eng.S + FA * (L + 2), f"slot {e}: evidence")
        assert fc.evidence[e] > 0
    eng.close()
