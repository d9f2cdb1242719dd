"""The packed tiger rejection update of filters of TIGER_ONCE_MIN_N = 3584 particles and more (reject_tiger_once_kernel) reads the filter
once: its sweep parks the four words a step of the slot's action can read and notes whether a record holds anything else; where none does,
the new filter is built from the parked words and the sources are never read again, otherwise the accepted source records are gathered
(reject_tiger_once_gather_kernel's only path, FBA_TIGER_GATHER=1).  Smaller filters stay with reject_tiger_lds_kernel.  Every result
must be that of the generic reject_kernel on dense records (FBA_DENSE_PARTICLES=1) and of the oracle, bit for bit."""
import numpy as np
import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N
from oracle import pyorc as orc

pytestmark = pytest.mark.gpu

DOM = {"episodic-tiger": orc.DOM_TIGER_EPISODIC, "continuous-tiger": orc.DOM_TIGER_CONTINUOUS}
LISTEN = 2
SHAPE = dict(sims=32, horizon=10, episodes=3)
# three slots play nine episodes, and at 32 simulations most episodic ones are "listen, open": seeds whose runs listen twice in a row somewhere
SEEDS = {("episodic-tiger", 257, 3): 10360, ("episodic-tiger", 512, 3): 11615, ("episodic-tiger", 3583, 3): 18686, ("episodic-tiger", 4096, 3): 14199}


def _engine(domain, belief, particles, slots, seed, monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = fba.Engine(domain, model=N.MODEL_BA_TABLE, belief=belief, seed=seed, slots=slots, runs=slots, particles=particles, trace=1, **SHAPE)
    for k in env:
        monkeypatch.delenv(k)
    return eng


def _run(eng):
    stats = eng.run_bapomdp()
    c = eng.counters()
    return eng.trace(), [(s.count, s.mean, s.m2) for s in stats], (c.sim_steps, c.belief_steps, c.env_steps)


def _assert_same_contexts(a, b, ra, rb, slots):
    (ta, sa, ca), (tb, sb, cb) = ra, rb
    assert len(ta) == len(tb) > 0
    for name in ta.dtype.names:     # belief_hash and update_count of every step among them
        bad = np.nonzero(~np.all((ta[name] == tb[name]).reshape(len(ta), -1), axis=1))[0]
        assert bad.size == 0, f"{name}: first mismatch at record {bad[0]}: {ta[bad[0]]} vs {tb[bad[0]]}"
    assert sa == sb and ca == cb
    for slot in range(slots):
        s1, _, c1 = a.belief_get(slot)
        s2, _, c2 = b.belief_get(slot)
        assert np.array_equal(s1, s2), slot
        assert np.array_equal(c1.view(np.uint32), c2.view(np.uint32)), slot


def _assert_equals_oracle(domain, belief, particles, slots, seed, run):
    o = orc.Oracle(domain=DOM[domain], model=orc.MODEL_BA_TABLE, belief=N.BELIEF_NAMES[belief], rng_mode=orc.RNG_PHILOX, arith=orc.ARITH_DEV,
                   philox_seed=seed, trace=1, particles=particles, runs=slots, **SHAPE)
    ostats, res = o.run_bapomdp()
    tr, stats, counters = run
    otr = o.trace(res.n_trace)
    assert len(tr) == len(otr)
    for name in tr.dtype.names:
        bad = np.nonzero(~np.all((tr[name] == otr[name]).reshape(len(tr), -1), axis=1))[0]
        assert bad.size == 0, f"{name}: first mismatch at record {bad[0]}: {tr[bad[0]]} vs {otr[bad[0]]}"
    assert stats == [(s.count, s.mean, s.m2) for s in ostats]
    assert counters == (res.sim_steps, res.belief_steps, res.env_steps)


def _ticks(tr):
    """the launch each record's step belongs to: every slot owns one run (runs = slots) and takes one step per tick"""
    tick = np.zeros(len(tr), np.int64)
    for run in np.unique(tr["run"]):
        idx = np.nonzero(tr["run"] == run)[0]
        idx = idx[np.lexsort((tr["t"][idx], tr["episode"][idx]))]
        tick[idx] = np.arange(len(idx))
    return tick


def _assert_every_kind_of_slot_occurred(tr, domain, slots):
    updated = tr["update_count"] > 0
    assert np.any(updated & (tr["t"] == 0)), "no update behind a lazy reset (the first of an episode)"
    assert np.any(updated & (tr["t"] > 0)), "no update of a filter that carries its states"
    assert np.all(updated == (tr["terminal"] == 0))
    if domain == "episodic-tiger":      # a slot whose step ended its episode sits out an update launch that other slots take part in
        tick = _ticks(tr)                # (the continuous tiger ends no episode early: every slot is in every launch)
        busy = np.unique(tick[updated])
        assert np.any(~updated & np.isin(tick, busy)), "no slot was masked out of an update launch"
    if domain == "continuous-tiger":
        # an update after `open` writes cells outside the listen words: from then on that run's records hold more than any action's
        # parked words and its updates gather; before the first `open` of a run (pristine counts, or listen cells only) they do not
        opened = updated & (tr["action"] != LISTEN)
        assert np.any(opened), "no update after an open action"
        gathered = clean = False
        for run in np.unique(tr["run"]):
            m = tr["run"] == run
            order = np.lexsort((tr["t"][m], tr["episode"][m]))
            acts, upd = tr["action"][m][order], updated[m][order]
            first_open = np.nonzero(upd & (acts != LISTEN))[0]
            k = first_open[0] if first_open.size else len(acts)
            clean = clean or bool(np.any(upd[:k] & (acts[:k] == LISTEN)))
            gathered = gathered or bool(np.any(upd[k + 1:]))
        assert clean and gathered, (clean, gathered)
    else:
        assert np.all(tr["action"][updated] == LISTEN)     # only `listen` continues an episode: every update rebuilds from the parked words


@pytest.mark.parametrize("slots", [3, 130])
@pytest.mark.parametrize("particles", [5, 257, 512, 513, 3583, 3584, 4096])   # 3584: the first filter of reject_tiger_once_kernel
@pytest.mark.parametrize("domain", ["episodic-tiger", "continuous-tiger"])
def test_update_equals_dense_records_and_the_oracle(domain, particles, slots, monkeypatch):
    seed = SEEDS.get((domain, particles, slots), 9100 + particles + slots)
    packed = _engine(domain, "rejection_sampling", particles, slots, seed, monkeypatch)
    dense = _engine(domain, "rejection_sampling", particles, slots, seed, monkeypatch, FBA_DENSE_PARTICLES="1")
    assert packed.particle_bytes == 64 and dense.particle_bytes == 128
    rp, rd = _run(packed), _run(dense)
    _assert_same_contexts(packed, dense, rp, rd, slots)
    _assert_every_kind_of_slot_occurred(rp[0], domain, slots)
    _assert_equals_oracle(domain, "rejection_sampling", particles, slots, seed, rp)


def test_point_estimate_equals_dense_records_and_the_oracle(monkeypatch):
    """one particle per slot (on the episodic tiger a point estimate opens a door at once and is never updated: the continuous one);
    the filter has one record, so this is reject_tiger_lds_kernel"""
    domain, slots, seed = "continuous-tiger", 130, 77
    packed = _engine(domain, "point_estimate", 50, slots, seed, monkeypatch)
    dense = _engine(domain, "point_estimate", 50, slots, seed, monkeypatch, FBA_DENSE_PARTICLES="1")
    assert packed.particle_bytes == 64 and dense.particle_bytes == 128
    rp, rd = _run(packed), _run(dense)
    _assert_same_contexts(packed, dense, rp, rd, slots)
    _assert_every_kind_of_slot_occurred(rp[0], domain, slots)
    _assert_equals_oracle(domain, "point_estimate", 50, slots, seed, rp)


@pytest.mark.parametrize("domain,particles", [("episodic-tiger", 4096), ("continuous-tiger", 3585)])
def test_gather_switch_changes_nothing(domain, particles, monkeypatch):
    """FBA_TIGER_GATHER=1 (read when the context is created) copies every new filter from its source records; unset, the episodic tiger
    never does and the continuous tiger does after an `open` (asserted above): the two contexts must be equal field for field"""
    slots, seed = 130, 4242
    built = _engine(domain, "rejection_sampling", particles, slots, seed, monkeypatch)
    gathered = _engine(domain, "rejection_sampling", particles, slots, seed, monkeypatch, FBA_TIGER_GATHER="1")
    rb, rg = _run(built), _run(gathered)
    _assert_same_contexts(built, gathered, rb, rg, slots)
    _assert_every_kind_of_slot_occurred(rb[0], domain, slots)
