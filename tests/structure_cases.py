"""Shared by the tests of fba_belief_structures: the contexts, how they are driven, and the numpy reference over Engine.belief_get.

The reference follows the definitions of include/fba_hip.h word for word: the structure of particle i is the n_mask_words uint32 bit
patterns behind the n_counts counts of its blob, w_i its weight (1.0 in a flat filter); the distinct structures are the weighted
np.unique(axis=0) of those rows.

Bound (derived, not measured), as for edge_prob of fba_belief_summary: every mass is a sum of at most N non-negative terms, so any
fp64 summation order is within N * 2^-53 relative of the exact sum to first order, on both sides: |dev - ref| <= 8 * N * 2^-53 *
max(dev, ref), exactly 0.0 where the reference is 0.0.  A flat filter sums 1.0s: integers below 2^53, equality."""
import numpy as np

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

FACT = N.MODEL_BA_FACTORED
IS, REJ = "importance_sampling", "rejection_sampling"
UNIFORM, MATCH_UNIFORM = 1, 2          # FBA_SP_UNIFORM, FBA_SP_MATCH_UNIFORM
WEIGHTED_BELIEFS = (N.BELIEF_IMPORTANCE, N.BELIEF_CHEATING, N.BELIEF_MH_GIBBS, N.BELIEF_MH_NIPS)

# name -> (kind of observation, domain, belief, configuration)
FORMATS = {
    "dense_factored_tiger2": ("tiger", "continuous-factored-tiger", IS, dict(size=2, structure_prior=MATCH_UNIFORM)),
    "packed_factored_tiger2": ("tiger", "continuous-factored-tiger", REJ, dict(size=2, structure_prior=MATCH_UNIFORM)),
    "gridworld3_history_importance": ("gridworld", "gridworld", IS, dict(size=3, structure_prior=MATCH_UNIFORM)),
    "gridworld3_history_rejection": ("gridworld", "gridworld", REJ, dict(size=3, structure_prior=MATCH_UNIFORM)),
    "collision_avoidance_5x5x1_uniform": ("ca", "random-collision-avoidance", IS, dict(width=5, height=5, size=1, structure_prior=UNIFORM)),
}
# 18 bits of legal parent-set choice (three actions, two obstacles, three candidate parents each): more structures than the table holds
MANY_STRUCTURES = {"collision_avoidance_5x5x2_uniform": ("ca", "random-collision-avoidance", IS, dict(width=5, height=5, size=2, structure_prior=UNIFORM))}


def engine(name, **kw):
    kind, domain, belief, cfg = {**FORMATS, **MANY_STRUCTURES}[name]
    args = dict(sims=16, episodes=2, horizon=8)
    args.update(cfg)
    args.update(kw)
    return fba.Engine(domain, model=FACT, belief=belief, **args), kind


def weighted(eng):
    return eng.cfg.belief in WEIGHTED_BELIEFS


def obs_for(eng, kind, e, step):
    """an observation slot e's filter can produce: 0 / 1 for the tigers (every action gives both), else what a particle of the filter
    would see without noise from where it is"""
    if kind == "tiger":
        return (e + step) % 2
    s, _, _ = eng.belief_get(e, weights=False, counts=False)
    st = int(s[(7 * e + 3 * step) % len(s)])
    return st if kind == "gridworld" else st % eng.O      # collision avoidance: the state's last digits are the obstacles' rows


def drive(eng, kind, updates=3):
    """belief_init, reset and `updates` per-call updates in slots at different (run, episode, t): structures have been resampled"""
    E = eng.slots
    run = np.array([5 + 1000 * e for e in range(E)], np.int32)
    t = np.array([e % 3 for e in range(E)], np.int32)
    eng.set_position(run=run, episode=0, t=0)
    eng.belief_init()
    eng.set_position(run=run, episode=np.array([e % 2 for e in range(E)], np.int32), t=0)
    eng.belief_reset_domain_state()
    for step in range(updates):
        eng.set_position(t=t + step)
        action = np.array([(e + step // 2) % eng.A for e in range(E)], np.int32)
        obs = np.array([obs_for(eng, kind, e, step) for e in range(E)], np.int32)
        eng.belief_update(action, obs)


def word_limits(eng):
    """per parent-set word: it is legal below this (1 << n_candidates of every node it serves)"""
    lay = eng.factored_layout()
    limit = np.full(lay.n_mask_words, 2 ** 32, np.int64)
    for k in range(lay.n_nodes):
        nd = lay.node[k]
        if nd.mask_word >= 0:
            limit[nd.mask_word] = min(limit[nd.mask_word], 1 << nd.n_candidates)
    return limit


def lens_from_layout(eng):
    lay = eng.factored_layout()
    most = max([lay.node[k].n_candidates for k in range(lay.n_nodes) if lay.node[k].mask_word >= 0], default=0)
    return lay.n_mask_words, (1 << most) if lay.n_mask_words else 0


def words_of(eng, slot):
    """(weights, uint32[N][n_words]) of a slot's particles, through belief_get"""
    lay = eng.factored_layout()
    _, w, cnt = eng.belief_get(slot, weights=weighted(eng))
    if not weighted(eng):
        w = np.ones(cnt.shape[0], np.float64)
    return w, np.ascontiguousarray(cnt[:, lay.n_counts:]).view(np.uint32)


class Reference:
    """the posterior over structures of one slot, in numpy"""

    def __init__(self, eng, slot, queries=None, w_words=None):
        self.n_words, self.n_sets = lens_from_layout(eng)
        self.w, self.words = words_of(eng, slot) if w_words is None else w_words
        self.weight_total = self.w.sum()
        self.uniq, inv = np.unique(self.words, axis=0, return_inverse=True)      # rows in ascending order, word 0 most significant
        self.mass = np.bincount(inv.reshape(-1), weights=self.w, minlength=len(self.uniq))
        self.order = np.argsort(-self.mass, kind="stable")                       # mass descending, among equal masses rows ascending
        self.distinct = len(self.uniq)
        self.set_mass = np.zeros((self.n_words, self.n_sets), np.float64)
        for m in range(self.n_words):
            ok = self.words[:, m] < self.n_sets
            self.set_mass[m] = np.bincount(self.words[ok, m], weights=self.w[ok], minlength=self.n_sets)
        self.queries = queries
        if queries is not None:
            q = np.asarray(queries, np.uint32).reshape(-1, self.n_words)
            self.query_mass = np.array([self.w[np.all(self.words == row[None, :], axis=1)].sum() for row in q])

    def index_of(self, row):
        hit = np.nonzero(np.all(self.uniq == np.asarray(row, np.uint32)[None, :], axis=1))[0]
        return int(hit[0]) if len(hit) else -1


def absent_structure(eng, refs):
    """a legal word list that no particle of the slots holds: the mixed-radix enumeration of the legal words, first miss"""
    limit = word_limits(eng)
    for k in range(1 << 20):
        row, q = [], k
        for m in range(len(limit)):
            row.append(q % int(limit[m]))
            q //= int(limit[m])
        if all(r.index_of(row) < 0 for r in refs):
            return np.array(row, np.uint32)
    raise AssertionError("every legal structure is in the filter")


def standard_queries(eng):
    """the most frequent structure of slot 0, a structure absent from every slot, the all-candidates structure"""
    refs = [Reference(eng, e) for e in range(eng.slots)]
    top = refs[0].uniq[refs[0].order[0]]
    return np.stack([top, absent_structure(eng, refs), (word_limits(eng) - 1).astype(np.uint32)])


def close(dev, ref, n, what):
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


def compare_slot(res, b, ref, eng, top_k, what, table=N.STRUCT_TABLE):
    """row b of a belief_structures result against the reference of its slot; a reference of more than `table` structures only compares
    what does not depend on the table"""
    n, flat = eng.cfg.particles, not weighted(eng)
    tol = 8 * n * 2.0 ** -53

    def same(dev, expect, w):
        close(dev, expect, n, w)
        if flat:
            np.testing.assert_array_equal(np.asarray(dev, np.float64), np.asarray(expect, np.float64), err_msg=w)

    same(res.weight_total[b], ref.weight_total, what + ": weight_total")
    if flat:
        assert res.weight_total[b] == n
    same(res.set_mass[b], ref.set_mass, what + ": set_mass")
    if ref.queries is not None:
        same(res.query_mass[b], ref.query_mass, what + ": query_mass")
    if ref.distinct > table:
        return
    assert res.overflow[b] == 0 and res.unplaced_mass[b] == 0.0, what
    assert res.distinct[b] == ref.distinct, what
    stored = min(top_k, ref.distinct)
    assert res.stored[b] == stored, what
    if top_k == 0:
        return
    assert np.all(res.top_words[b, stored:] == 0) and np.all(res.top_mass[b, stored:] == 0.0), what
    if flat:
        np.testing.assert_array_equal(res.top_words[b, :stored], ref.uniq[ref.order[:stored]], err_msg=what + ": top_words")
        np.testing.assert_array_equal(res.top_mass[b, :stored], ref.mass[ref.order[:stored]], err_msg=what + ": top_mass")
        return
    # weighted: the reference's order up to swaps among entries whose reference masses lie within the bound of each other
    seen = set()
    for k in range(stored):
        idx = ref.index_of(res.top_words[b, k])
        assert idx >= 0 and idx not in seen, f"{what}: top entry {k} is no structure of the filter, or a repeated one"
        seen.add(idx)
        close(res.top_mass[b, k], ref.mass[idx], n, f"{what}: top_mass[{k}]")
        at_k = ref.mass[ref.order[k]]
        assert abs(ref.mass[idx] - at_k) <= tol * max(ref.mass[idx], at_k), f"{what}: top entry {k} is out of order"


def check(eng, what, top_k=8, queries="standard", first=0, count=None):
    """one call on slots [first, first + count) against the references; returns the result and the references"""
    count = eng.slots - first if count is None else count
    if isinstance(queries, str):
        queries = standard_queries(eng)
    res = eng.belief_structures(first, count, top_k=top_k, queries=queries)
    refs = []
    for b in range(count):
        ref = Reference(eng, first + b, queries)
        compare_slot(res, b, ref, eng, top_k, f"{what}, slot {first + b}")
        refs.append(ref)
    return res, refs
