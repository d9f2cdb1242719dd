"""Compact filters: between the belief updates of the experiment loop an episodic-tiger slot keeps its filter as
16-byte records.  A context created under FBA_NO_COMPACT=1 keeps 64-byte records throughout -- the path the oracle-parity tests pin --
and everything a caller can see must be equal in the two, bit for bit: after plain ticks, with readers in the middle, and with the
per-call interface in the middle.  Shapes: 3 584 particles (the smallest filter reject_tiger_once_kernel takes, 7 x 512: the sweep's
last trip is half empty) and 4 096 (the edge of the 12-bit source index), 70 slots (two search waves, the second partial), 30 ticks of
3 episodes x horizon 4 (episode ends: lazy resets; two run ends and more: re-initialisation)."""
import numpy as np
import pytest

import fba_pomdp_amd as fba

pytestmark = pytest.mark.gpu

SLOTS, TICKS, SEED = 70, 30, 20261
KW = dict(sims=64, horizon=4, episodes=3, runs=2)
LISTEN = 2


def _engine(monkeypatch, particles, no_compact=False, domain="episodic-tiger", **kw):
    monkeypatch.delenv("FBA_NO_COMPACT", raising=False)
    if no_compact:
        monkeypatch.setenv("FBA_NO_COMPACT", "1")
    args = dict(KW, particles=particles, slots=SLOTS, seed=SEED)
    args.update(kw)
    eng = fba.Engine(domain, model=fba.MODEL_BA_TABLE, belief="rejection_sampling", **args)
    monkeypatch.delenv("FBA_NO_COMPACT", raising=False)
    assert eng.particle_bytes == 64 and eng.slots == SLOTS
    return eng


def _visible(eng):
    """everything a caller can read of a context: every slot's filter, the counters, the return sums, the last step's records"""
    c = eng.counters()
    out = {"counters": (c.sim_steps, c.belief_steps, c.env_steps), "return_sums": eng.return_sums().tobytes(),
           "last_step_info": eng.last_step_info().tobytes()}
    for slot in range(SLOTS):
        s, _, cnt = eng.belief_get(slot)
        out["states", slot], out["counts", slot] = s.tobytes(), cnt.tobytes()
    return out


def _assert_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], f"{k} differs between the default context and the FBA_NO_COMPACT one"


@pytest.mark.parametrize("particles", [3584, 4096])
def test_ticks_equal_the_64_byte_path(particles, monkeypatch):
    new, old = _engine(monkeypatch, particles), _engine(monkeypatch, particles, no_compact=True)
    for eng in (new, old):
        eng.run_ticks(TICKS)
    assert new.debug_compact_slots() > SLOTS // 2 and old.debug_compact_slots() == 0
    _assert_equal(_visible(new), _visible(old))
    assert new.debug_compact_slots() == 0      # belief_get is a reader


@pytest.mark.parametrize("particles", [3584, 4096])
def test_readers_in_the_middle(particles, monkeypatch):
    new, old = _engine(monkeypatch, particles), _engine(monkeypatch, particles, no_compact=True)
    mid = []
    for eng in (new, old):
        eng.run_ticks(7)
        compact = eng.debug_compact_slots()
        sm = eng.belief_summary()
        assert eng.debug_compact_slots() == 0
        blocks = eng.belief_export(0, 10)
        eng.belief_import(SLOTS - 10, blocks)
        s, _, cnt = eng.belief_get(35)
        mid.append((compact, sm.head.tobytes(), sm.state_mass.tobytes(), sm.mean_counts.tobytes(), blocks.tobytes(), s.tobytes(), cnt.tobytes()))
        eng.run_ticks(TICKS - 7)
    assert mid[0][0] > 0 and mid[1][0] == 0
    assert mid[0][1:] == mid[1][1:], "a reader's output differs between the default context and the FBA_NO_COMPACT one"
    assert new.debug_compact_slots() > 0
    _assert_equal(_visible(new), _visible(old))


@pytest.mark.parametrize("particles", [3584, 4096])
def test_per_call_interface_after_ticks(particles, monkeypatch):
    """a slot goes back to 64-byte records, gains non-zero `open` words and keeps 64-byte records while it has them"""
    new, old = _engine(monkeypatch, particles), _engine(monkeypatch, particles, no_compact=True)
    action = np.where(np.arange(SLOTS) < SLOTS // 2, 0, LISTEN).astype(np.int32)    # `open` for half the slots, `listen` for the rest
    picked = []
    for eng in (new, old):
        eng.run_ticks(TICKS)
        eng.belief_update(action, 0)
        assert eng.debug_compact_slots() == 0      # the per-call entry points never produce a compact filter
        picked.append(eng.select_action(0).tobytes())
        eng.run_ticks(5)
    assert picked[0] == picked[1]
    # the slots whose run has not ended since (a run end re-initialises the filter) still hold their `open` counts: not compact
    assert 0 < new.debug_compact_slots() < SLOTS and old.debug_compact_slots() == 0
    vn, vo = _visible(new), _visible(old)
    _assert_equal(vn, vo)
    dense = [np.frombuffer(vn["counts", slot], np.float32).reshape(particles, -1) for slot in range(SLOTS // 2)]
    prior = new.prior()
    assert any((d[:, [0, 1, 6, 7]] != prior[[0, 1, 6, 7]]).any() for d in dense), "no slot kept counts of its `open` update"


def _expected_compact(rec, flag):
    """one tick of a traced context's last_step_info on the per-slot flags: a belief update (the step was not terminal; in the episodic
    tiger that is a `listen`) leaves the filter compact, the end of a run re-initialises it as 64-byte records"""
    for e in range(SLOTS):
        r = rec[e]
        assert r["run"] % SLOTS == e
        if not r["terminal"]:
            assert r["action"] == LISTEN
            flag[e] = True
        if (r["terminal"] or r["t"] + 1 >= KW["horizon"]) and r["episode"] == KW["episodes"] - 1:
            flag[e] = False


@pytest.mark.parametrize("particles", [3584, 4096])
def test_compact_slots_are_those_last_updated_by_a_listen(particles, monkeypatch):
    plain, traced = _engine(monkeypatch, particles), _engine(monkeypatch, particles, trace=1)
    flag = [False] * SLOTS
    for tick in range(TICKS):
        traced.run_ticks(1)
        _expected_compact(traced.last_step_info(), flag)
        assert traced.debug_compact_slots() == sum(flag), tick
    plain.run_ticks(TICKS)
    assert sum(flag) > SLOTS // 2
    assert plain.debug_compact_slots() == sum(flag)
    plain.belief_summary(state_mass=True, mean_counts=False, edge_prob=False)
    assert plain.debug_compact_slots() == 0


@pytest.mark.parametrize("case", ["3583 particles", "32768 updates per run", "continuous tiger", "FBA_NO_COMPACT"])
def test_contexts_that_never_go_compact(case, monkeypatch):
    kw, domain = dict(particles=3584), "episodic-tiger"
    if case == "3583 particles":
        kw = dict(particles=3583)
    if case == "32768 updates per run":
        kw = dict(particles=3584, episodes=256, horizon=128)
    if case == "continuous tiger":
        domain = "continuous-tiger"
    eng = _engine(monkeypatch, no_compact=case == "FBA_NO_COMPACT", domain=domain, **kw)
    for _ in range(3):
        eng.run_ticks(2)
        assert eng.debug_compact_slots() == 0


def test_traced_context_equals_the_64_byte_path(monkeypatch):
    """the trace readers (belief checksum) see a compact filter through its words view: every record of the trace, belief hashes included"""
    new, old = _engine(monkeypatch, 3584, trace=1), _engine(monkeypatch, 3584, no_compact=True, trace=1)
    seen = 0
    for eng in (new, old):
        for _ in range(3):
            eng.run_ticks(TICKS // 3)
            seen += eng.debug_compact_slots()
    assert seen > 0 and old.debug_compact_slots() == 0
    tn, to = new.trace(), old.trace()
    assert len(tn) == len(to) > 0
    key = lambda t: np.lexsort((t["t"], t["episode"], t["run"]))      # (records of one tick arrive in the order their workgroups finish)
    tn, to = tn[key(tn)], to[key(to)]
    for name in tn.dtype.names:
        assert np.array_equal(tn[name], to[name]), f"trace field {name} differs"
    assert len(np.unique(tn["belief_hash"])) > len(tn) // 2
