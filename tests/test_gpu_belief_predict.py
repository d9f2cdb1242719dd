"""fba_belief_predict / Engine.belief_predict: posterior-predictive model queries evaluated on the device from every record format,
against numpy over Engine.belief_get of the same slot plus factored_layout().  The reference is written from the layout comment of
include/fba_hip.h: per particle each node's parent set is the mask word at n_counts + mask_word (or fixed_mask), the row index is
"for j in candidate order, if bit j set: idx = idx * candidate_size[j] + v[candidate[j]]", rows are normalised in fp64 and a row that
sums to 0 gives 0; tabular rows are phi[s*A*S + a*S + s'] and psi[a*S*O + s'*O + o].

Bound (derived, not measured): every entry is a sum of at most N non-negative terms, each a weight times at most F quotients, each
quotient's denominator an fp64 sum of at most L fp32 values.  A sum of L non-negative values is within (L - 1) * 2^-53 relative of the
exact one in any order, the quotient adds one rounding, the product with the weight (or the next factor) one more, the sum over the
particles at most N - 1, the division by the weight total (itself within N * 2^-53, counted in the N of the other side) one: to first
order both sides are within (N + F * (L + 2) + 2) * 2^-53 relative of the exact value, so
    |dev - ref| <= 8 * (N + F * (L + 2)) * 2^-53 * max(dev, ref)
per entry, with F = 1 for trans and obsp and F = the nodes of one query (at most 16) for joint, L the longest row of the case; and
exactly 0.0 wherever the reference is 0.0 (a zero sum of non-negative terms has only zero terms).  One lost increment of one particle
moves an entry by about 1 / (N * R) for a row sum R; at R = 10^4 that is still ten orders of magnitude above the bound.

Queries: every (s, a) with next_state = s and obs = (7 s + a) % O, which names every transition row and every observation row of the
model, so every cell an update raised lies in some queried row."""
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


def _queries(eng):
    """every (s, a): state, action, next_state, obs"""
    s = np.repeat(np.arange(eng.S, dtype=np.int32), eng.A)
    a = np.tile(np.arange(eng.A, dtype=np.int32), eng.S)
    return s, a, s.copy(), ((7 * s + a) % eng.O).astype(np.int32)


def _likely_queries(eng):
    """every (s, a) once more, with the next state and the observation the PRIOR holds most likely (per node the largest count of the
    row): where the model forbids next_state = s -- the aircraft of collision avoidance always moves on -- the first block's joint
    is 0 throughout, this block's is not"""
    s, a, _, _ = _queries(eng)
    blob = eng.prior()
    if eng.cfg.model != FACT:
        S, A, O = eng.S, eng.A, eng.O
        ns = blob[:S * A * S].reshape(S, A, S)[s, a, :].argmax(axis=1).astype(np.int32)
        o = blob[S * A * S:].reshape(A, S, O)[a, ns, :].argmax(axis=1).astype(np.int32)
        return s, a, ns, o
    lay = eng.factored_layout()
    FS, FO = lay.n_state_features, lay.n_obs_features
    ssz, osz = list(lay.state_feature_size[:FS]), list(lay.obs_feature_size[:FO])
    words = np.ascontiguousarray(blob[None, lay.n_counts:]).view(np.uint32)
    q = np.arange(len(s))

    def pick(first, n, sizes, parents):
        index = np.zeros(len(s), np.int64)
        for f in range(n):
            value = np.zeros(len(s), np.int64)
            for x in range(eng.A):
                node = lay.node[first(x) + f]
                start, _ = _row_starts(lay, node, words, parents)
                value = np.where(a == x, blob[start[0][:, None] + np.arange(node.out)[None, :]].argmax(axis=1), value)
            index = index * sizes[f] + value
        return index.astype(np.int32)

    ns = pick(lambda x: x * FS, FS, ssz, _features(s, ssz))
    o = pick(lambda x: eng.A * FS + x * FO, FO, osz, _features(ns, ssz))
    assert q.size == ns.size == o.size
    return s, a, ns, o


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


def _nodes(eng, Q):
    """the nodes of every query as the layout describes them: a list over (kind, feature) of
    (kind, segment start, out, value per query, per action the node or None, parent values per query)"""
    s, a, ns, o = Q
    if eng.cfg.model != FACT:
        return None
    lay = eng.factored_layout()
    FS, FO = lay.n_state_features, lay.n_obs_features
    ssz, osz = list(lay.state_feature_size[:FS]), list(lay.obs_feature_size[:FO])
    fs, fns, fo = _features(s, ssz), _features(ns, ssz), _features(o, osz)
    out, t_off, o_off = [], 0, 0
    for f in range(FS):
        out.append(("T", t_off, ssz[f], fns[:, f], [lay.node[x * FS + f] for x in range(eng.A)], fs))
        t_off += ssz[f]
    for f in range(FO):
        out.append(("O", o_off, osz[f], fo[:, f], [lay.node[eng.A * FS + x * FO + f] for x in range(eng.A)], fns))
        o_off += osz[f]
    return lay, out


def _row_starts(lay, node, words, parents):
    """[particles, queries]: where the row of each query starts in each particle's blob"""
    mask = words[:, node.mask_word] if node.mask_word >= 0 else np.full(words.shape[0], node.fixed_mask, np.uint32)
    idx = np.zeros((words.shape[0], parents.shape[0]), np.int64)
    for j in range(node.n_candidates):
        bit = ((mask >> np.uint32(j)) & 1).astype(bool)
        v = parents[:, node.candidate[j]]
        idx = np.where(bit[:, None], idx * node.candidate_size[j] + v[None, :], idx)
    return node.offset + idx * node.out, mask


def _reference(eng, slot, Q):
    """numpy over belief_get: trans [nq, TL], obsp [nq, OL], joint [nq]; the longest row, the nodes of a query, whether two particles
    differ in a queried row, whether they differ in a parent set, the particles' tables"""
    s, a, ns, o = Q
    nq = len(s)
    weighted = eng.cfg.belief == N.BELIEF_IMPORTANCE
    _, w, cnt = eng.belief_get(slot, weights=weighted)
    if not weighted:
        w = np.ones(cnt.shape[0], np.float64)
    W = w.sum()
    c64 = cnt.astype(np.float64)
    n = cnt.shape[0]
    differ = structures = False
    if eng.cfg.model != FACT:
        S, A, O = eng.S, eng.A, eng.O
        phi = c64[:, :S * A * S].reshape(n, S, A, S)
        psi = c64[:, S * A * S:].reshape(n, A, S, O)
        rt, ro = phi[:, s, a, :], psi[:, a, ns, :]
        differ = bool(np.any(rt.max(axis=0) != rt.min(axis=0)) or np.any(ro.max(axis=0) != ro.min(axis=0)))
        tt, to = _theta(rt), _theta(ro)
        trans = np.einsum("i,iqk->qk", w, tt) / W
        obsp = np.einsum("i,iqk->qk", w, to) / W
        q = np.arange(nq)
        joint = (w[:, None] * tt[:, q, ns] * to[:, q, o]).sum(axis=0) / W
        return dict(trans=trans, obsp=obsp, joint=joint, L=max(S, O), F=2, differ=differ, structures=False, counts=cnt)
    lay, nodes = _nodes(eng, Q)
    words = np.ascontiguousarray(cnt[:, lay.n_counts:]).view(np.uint32)
    TL, OL = sum(lay.state_feature_size[:lay.n_state_features]), sum(lay.obs_feature_size[:lay.n_obs_features])
    trans, obsp = np.zeros((nq, TL)), np.zeros((nq, OL))
    prod = np.ones((n, nq))
    L = 1
    for kind, seg, out, val, per_action, parents in nodes:
        L = max(L, out)
        for x in range(eng.A):
            sel = np.nonzero(a == x)[0]
            if sel.size == 0:
                continue
            start, mask = _row_starts(lay, per_action[x], words, parents[sel])
            structures = structures or bool(np.any(mask != mask[0]))
            rows = c64[np.arange(n)[:, None, None], start[:, :, None] + np.arange(out)[None, None, :]]
            differ = differ or bool(np.any(rows.max(axis=0) != rows.min(axis=0)))
            th = _theta(rows)
            (trans if kind == "T" else obsp)[sel, seg:seg + out] = np.einsum("i,iqk->qk", w, th) / W
            prod[:, sel] *= th[:, np.arange(sel.size), val[sel]]
    joint = (w[:, None] * prod).sum(axis=0) / W
    return dict(trans=trans, obsp=obsp, joint=joint, L=L, F=len(nodes), differ=differ, structures=structures, counts=cnt)


def _close(dev, ref, terms, what):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    assert dev.shape == ref.shape, what
    scale = np.maximum(dev, ref)
    err = np.abs(dev - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, 0.0)
    print(f"{what}: largest relative difference {rel.max() if rel.size else 0.0:.3e}, bound {8 * terms * 2.0 ** -53:.3e}")
    assert np.all(np.isfinite(dev)), what
    assert np.all(dev[ref == 0.0] == 0.0), what
    assert np.all(err <= 8 * terms * 2.0 ** -53 * scale), what


def _check(eng, first, count, Q, what, refs=None, sub=None):
    """one call on slots [first, first + count) against the per-slot references (taken at the queries Q, compared at Q[sub]);
    returns (prediction, references by slot)"""
    ask = Q if sub is None else tuple(x[sub] for x in Q)
    pred = eng.belief_predict(*ask, first=first, count=count)
    n = eng.cfg.particles
    refs = {} if refs is None else refs
    pick = slice(None) if sub is None else sub
    for b in range(count):
        e = first + b
        if e not in refs:
            refs[e] = _reference(eng, e, Q)
        ref, w = refs[e], f"{what}, slot {e}"
        _close(pred.trans[b], ref["trans"][pick], n + ref["L"] + 2, w + ": trans")
        _close(pred.obsp[b], ref["obsp"][pick], n + ref["L"] + 2, w + ": obsp")
        _close(pred.joint[b], ref["joint"][pick], n + ref["F"] * (ref["L"] + 2), w + ": joint")
    return pred, refs


def _obs_for(eng, kind, e, step):
    """an observation slot e's filter can produce: 0 / 1 for the tigers (every action gives both), else what a particle of the filter
    would see without noise from where it is"""
    if kind == "tiger":
        return (e + step) % 2
    s, _, _ = eng.belief_get(e, weights=False, counts=False)
    st = int(s[(7 * e + 3 * step) % len(s)])
    return st if kind == "gridworld" else st % eng.O      # collision avoidance: the state's last digits are the obstacles' rows


def _drive(eng, kind, what, Q=None, sub=None, check=True):
    """belief_init, reset, three per-call updates in slots at different (run, episode, t), a check after the reset and after each update"""
    E = eng.slots
    Q = _queries(eng) if Q is None else Q
    run = np.array([5 + 1000 * e for e in range(E)], np.int32)
    episode = np.array([e % 2 for e in range(E)], np.int32)
    t = np.array([e % 3 for e in range(E)], np.int32)
    eng.set_position(run=run, episode=0, t=0)
    eng.belief_init()
    eng.set_position(run=run, episode=episode, t=0)
    eng.belief_reset_domain_state()
    out = [_check(eng, 0, E, Q, what + ", after the reset", sub=sub)] if check else []
    for step in range(3):
        eng.set_position(t=t + step)
        action = np.array([(e + step // 2) % eng.A for e in range(E)], np.int32)      # (two steps of one action: cells raised twice)
        obs = np.array([_obs_for(eng, kind, e, step) for e in range(E)], np.int32)
        eng.belief_update(action, obs)
        if check:
            out.append(_check(eng, 0, E, Q, f"{what}, after update {step}", sub=sub))
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
    # (the two below: any fp32 record, whatever its padding)
    ("sysadmin3_dense", "tiger", "independent-sysadmin", FACT, IS, None, dict(size=3), lambda e: max(e.particle_bytes, 4 * (e.ncnt + 1))),
    ("dense_tiger_regular", "tiger", "continuous-tiger", TABLE, IS, None, dict(dirichlet_regular=1), lambda e: _dense_bytes(24)),
]
QUERIES = {"dense_tiger": 6, "gridworld3_history_importance": 108, "collision_avoidance_5x5x2_history": 1875}


@pytest.mark.parametrize("name,kind,domain,model,belief,env,kw,nbytes", FORMATS, ids=[f[0] for f in FORMATS])
def test_every_record_format(name, kind, domain, model, belief, env, kw, nbytes, monkeypatch):
    eng = _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=8100 + len(name), **kw)
    assert eng.particle_bytes == nbytes(eng), name
    Q = _queries(eng)
    assert len(Q[0]) == eng.S * eng.A == QUERIES.get(name, eng.S * eng.A)
    Q = tuple(np.concatenate(pair) for pair in zip(Q, _likely_queries(eng)))      # (and a second block: _likely_queries)
    tl, ol = eng.predict_lens()
    out = _drive(eng, kind, name, Q)
    pred, refs = out[-1]
    assert pred.trans.shape == (3, len(Q[0]), tl) and pred.obsp.shape == (3, len(Q[0]), ol) and pred.joint.shape == (3, len(Q[0]))
    if model == FACT:
        lay = eng.factored_layout()
        assert list(pred.trans_offsets) == list(np.concatenate(([0], np.cumsum(lay.state_feature_size[:lay.n_state_features]))))
        assert pred.trans_offsets[-1] == tl and pred.obs_offsets[-1] == ol
    else:
        assert pred.trans_offsets is None and pred.obs_offsets is None and (tl, ol) == (eng.S, eng.O)
    # not an untouched prior: a queried row differs between two particles of a slot, parent sets do where the prior draws them
    assert any(r["differ"] for r in refs.values()), name
    if name in ("dense_factored_tiger2", "gridworld3_history_importance", "gridworld3_history_rejection"):
        assert any(r["structures"] for r in refs.values()), name
    assert np.any((pred.joint > 0) & (pred.joint < 1)), name
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
    Q = _queries(eng)
    _drive(eng, "ca", "collision avoidance 7 x 7 x 2, inexact prior", Q, check=False)
    # the queries whose rows hold a raised cell (the parent sets are fixed here: particle 0's rows are everyone's), then the first 64
    lay, nodes = _nodes(eng, Q)
    assert lay.n_mask_words == 0
    tables = [eng.belief_get(e)[2] for e in range(3)]
    assert sum(int(np.sum((c - new[None, :] >= 2) & (new[None, :] > 0))) for c in tables) > 0     # a cell raised twice
    raised = np.zeros(eng.ncnt, bool)
    for c in tables:
        raised |= np.any(c != new[None, :], axis=0)
    hit = np.zeros(len(Q[0]), bool)
    for kind, seg, out, val, per_action, parents in nodes:
        for x in range(eng.A):
            sel = np.nonzero(Q[1] == x)[0]
            start, _ = _row_starts(lay, per_action[x], np.zeros((1, 0), np.uint32), parents[sel])
            hit[sel] |= np.any(raised[start[0][:, None] + np.arange(out)[None, :]], axis=1)
    assert hit.sum() >= 8
    rows = np.nonzero(hit)[0]
    rows = rows[np.unique(np.linspace(0, len(rows) - 1, 192).astype(np.int64))]      # (spread over the states: the lowest all have x = 0)
    sub = np.unique(np.concatenate((rows, np.arange(64))))
    sub = np.sort(np.concatenate((sub, np.setdiff1d(np.arange(len(hit)), sub)[:256 - len(sub)])))
    assert len(sub) == 256
    # the reference of the subset alone (the full set is 7 203 queries), compared entry for entry
    Qs = tuple(x[sub] for x in Q)
    _check(eng, 0, 3, Qs, "collision avoidance 7 x 7 x 2, inexact prior, 256 queries")
    # the same rows once more with the prior's likeliest next state and observation: there joint is not 0 (the aircraft moves on)
    Ql = tuple(x[sub] for x in _likely_queries(eng))
    pred, _ = _check(eng, 0, 3, Ql, "collision avoidance 7 x 7 x 2, inexact prior, 256 likely queries")
    assert np.any((pred.joint > 0) & (pred.joint < 1))
    eng.close()


@pytest.mark.parametrize("particles", [1, 257])
@pytest.mark.parametrize("name", ["dense_tiger", "gridworld3_history_importance"])
def test_other_particle_counts(name, particles, monkeypatch):
    _, kind, domain, model, belief, env, kw, nbytes = next(f for f in FORMATS if f[0] == name)
    eng = _engine(monkeypatch, domain, model, belief, env, particles=particles, slots=3, runs=3, seed=8300 + particles, **kw)
    assert eng.particle_bytes == nbytes(eng)
    _drive(eng, kind, f"{name}, {particles} particles")
    eng.close()


def test_unequal_weights(monkeypatch):
    eng = _engine(monkeypatch, "continuous-factored-tiger", FACT, IS, size=2, structure_prior=2, particles=200, slots=2, runs=2, seed=8501)
    eng.set_position(run=[1, 2], episode=0, t=0)
    eng.belief_init()
    eng.belief_reset_domain_state()
    eng.belief_update([2, 0], [1, 0])
    g = np.random.default_rng(8501)
    for e in range(2):
        w = g.random(200) * 10.0 ** g.integers(-6, 3, 200)
        w[g.choice(200, 5, replace=False)] = 0.0
        assert np.all(w >= 0) and np.sum(w == 0) == 5
        eng.belief_set(e, weight=w)
    _check(eng, 0, 2, _queries(eng), "random weights")
    eng.close()


def test_slot_ranges_in_a_wide_context(monkeypatch):
    eng = _engine(monkeypatch, "gridworld", FACT, IS, size=3, structure_prior=2, particles=64, slots=70, runs=70, horizon=7, sims=32, seed=8601)
    assert eng.particle_bytes == 4 * ((2 + EPISODES * 7 + 3) // 4 * 4)
    eng.run_ticks(1)
    eng.run_ticks(1)
    Q = _queries(eng)
    whole, refs = _check(eng, 0, 70, Q, "slots 0..69")
    tail, _ = _check(eng, 66, 4, Q, "slots 66..69", refs=refs)
    one, _ = _check(eng, 5, 1, Q, "slot 5", refs=refs)
    L, F = refs[0]["L"], refs[0]["F"]
    for name, terms in (("trans", 64 + L + 2), ("obsp", 64 + L + 2), ("joint", 64 + F * (L + 2))):
        _close(getattr(tail, name), getattr(whole, name)[66:70], terms, f"{name}: the calls on slots 66..69")
        _close(getattr(one, name), getattr(whole, name)[5:6], terms, f"{name}: the calls on slot 5")
    assert any(not np.array_equal(whole.trans[0], whole.trans[e]) for e in range(1, 70))
    eng.close()


@pytest.mark.parametrize("nq", [1, 300])
@pytest.mark.parametrize("name", ["packed_tiger", "gridworld3_table_history"])
def test_query_counts(name, nq, monkeypatch):
    _, kind, domain, model, belief, env, kw, nbytes = next(f for f in FORMATS if f[0] == name)
    eng = _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=8700 + nq, **kw)
    assert eng.particle_bytes == nbytes(eng)
    full = _queries(eng)
    sub = np.arange(nq) % len(full[0])        # (300: the full set again and again)
    _drive(eng, kind, f"{name}, {nq} queries", full, sub=sub)
    eng.close()


@pytest.mark.parametrize("name,lazy", [("gridworld3_history_importance", False), ("packed_tiger", True), ("dense_factored_tiger2", False)])
def test_read_only(name, lazy, monkeypatch):
    """two contexts of one seed, one asks for predictions on the way: every particle, counter, action and step record keeps its bits"""
    _, kind, domain, model, belief, env, kw, _ = next(f for f in FORMATS if f[0] == name)
    seen = []
    for with_predict in (True, False):
        eng = _engine(monkeypatch, domain, model, belief, env, particles=130, slots=3, runs=3, seed=8800, trace=1, **kw)
        Q = _queries(eng)
        got = []
        eng.set_position(run=[11, 12, 13], episode=0, t=0)
        eng.belief_init()
        eng.belief_reset_domain_state()
        if not lazy:      # (belief_get would write a lazily reset filter out in both contexts: there the prediction comes first)
            obs = np.array([_obs_for(eng, kind, e, 0) for e in range(3)], np.int32)
            eng.belief_update([0, 1, 2], obs)
        if with_predict:
            eng.belief_predict(*Q)
            eng.belief_predict(*Q, first=1, count=2, trans=False)
        if not lazy:
            got += [x for e in range(3) for x in eng.belief_get(e)]
        c = eng.counters()
        got.append(np.array([c.sim_steps, c.belief_steps, c.env_steps]))
        eng.set_position(t=1)
        action = eng.select_action(hist_len=1)
        got.append(action)
        if with_predict:
            eng.belief_predict(*Q)
        obs = np.array([_obs_for(eng, kind, e, 1) for e in range(3)], np.int32)
        eng.belief_update(action, obs)
        if with_predict:
            eng.belief_predict(*Q, first=0, count=1, obsp=False, joint=False)
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
        nested.belief_predict(0, 0, 0, 0)
    nested.close()
    eng = _engine(monkeypatch, "continuous-tiger", TABLE, IS, particles=32, slots=3, runs=3)
    eng.belief_init()
    Q = _queries(eng)
    for first, count in ((0, 4), (2, 2), (-1, 2)):
        with pytest.raises(ValueError, match="slots"):
            eng.belief_predict(*Q, first=first, count=count)
    empty = np.zeros(0, np.int32)
    with pytest.raises(ValueError, match="queries"):
        eng.belief_predict(empty, empty, empty, empty)
    bad = dict(state=(0, eng.S), action=(1, eng.A), next_state=(2, -1), obs=(3, eng.O))
    for pos, (where, value) in enumerate(bad.values()):
        q = [x.copy() for x in Q]
        q[pos][where + 1] = value
        with pytest.raises(ValueError, match=f"query {where + 1} "):
            eng.belief_predict(*q)
    ptr = [x.ctypes.data for x in Q]
    assert eng.L.fba_belief_predict(eng.h, 0, 3, len(Q[0]), *ptr, None, None, None) == N.OK
    pred = eng.belief_predict(*Q, first=1, count=2, obsp=False)
    assert pred.trans.shape == (2, len(Q[0]), eng.S) and pred.obsp is None and pred.joint.shape == (2, len(Q[0]))
    eng.close()
    plan = _engine(monkeypatch, "continuous-tiger", POMDP, REJ, particles=32, slots=2, runs=2)
    plan.belief_init()
    with pytest.raises(ValueError, match="POMDP"):
        plan.belief_predict(0, 0, 0, 0)
    plan.close()
