"""Belief snapshots (fba_belief_export / _import / _replicate, Engine.belief_export / belief_import / belief_replicate): a filter moved as
the records the context stores must be the filter fba_belief_get shows -- states, weights and fp32 count tables bit for bit -- and must
have the same future: the same actions, root statistics, update counts, weight totals and belief hashes under the same positions.
Every comparison is of bits; there is no tolerance anywhere in this file.  A refused import must leave every slot as it was, and no test
runs a search or an update behind a refused import."""
import numpy as np
import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

pytestmark = pytest.mark.gpu

POMDP, TABLE, FACT = N.MODEL_POMDP, N.MODEL_BA_TABLE, N.MODEL_BA_FACTORED
IS, REJ, POINT = "importance_sampling", "rejection_sampling", "point_estimate"
DENSE_ENV = {"FBA_DENSE_PARTICLES": "1"}
MULTI_ENV = {"FBA_IS_MULTI_MIN": "1"}
EPISODES, HORIZON = 2, 8
HEAD = N.SNAPSHOT_HEAD_DTYPE

# name, kind, domain, model, belief, environment, configuration, record format as the header numbers it
FORMATS = [
    ("dense_tiger", "tiger", "continuous-tiger", TABLE, IS, DENSE_ENV, {}, 0),
    ("dense_factored_tiger2", "tiger", "continuous-factored-tiger", FACT, IS, None, dict(size=2, structure_prior=2), 0),
    ("packed_tiger", "tiger", "continuous-tiger", TABLE, REJ, None, {}, 1),
    ("packed_factored_tiger1", "tiger", "continuous-factored-tiger", FACT, REJ, None, dict(size=1, structure_prior=2), 2),
    ("packed_factored_tiger2", "tiger", "continuous-factored-tiger", FACT, REJ, None, dict(size=2, structure_prior=2), 3),
    ("packed_factored_tiger3", "tiger", "continuous-factored-tiger", FACT, REJ, None, dict(size=3, structure_prior=2), 4),
    ("gridworld3_history_importance", "gridworld", "gridworld", FACT, IS, None, dict(size=3, structure_prior=2), 5),
    ("gridworld3_history_rejection", "gridworld", "gridworld", FACT, REJ, None, dict(size=3, structure_prior=2), 5),
    ("gridworld3_table_history", "gridworld", "gridworld", TABLE, IS, None, dict(size=3), 6),
    ("collision_avoidance_5x5x2_history", "ca", "random-collision-avoidance", FACT, IS, MULTI_ENV, dict(width=5, height=5, size=2), 7),
    ("gridworld3_dense", "gridworld", "gridworld", FACT, IS, DENSE_ENV, dict(size=3, structure_prior=2), 0),
    ("sysadmin3_dense", "tiger", "independent-sysadmin", FACT, IS, None, dict(size=3), 0),
    ("plain_pomdp_tiger", "tiger", "continuous-tiger", POMDP, REJ, None, {}, 0),
    ("point_estimate_tiger", "tiger", "continuous-tiger", TABLE, POINT, None, {}, None),
]
IDS = [f[0] for f in FORMATS]
FUTURE = ["dense_tiger", "packed_tiger", "packed_factored_tiger2", "gridworld3_history_importance", "gridworld3_history_rejection",
          "gridworld3_table_history", "collision_avoidance_5x5x2_history", "dense_factored_tiger2", "plain_pomdp_tiger", "point_estimate_tiger"]
INFO_FIELDS = ("root_n", "root_q", "n_nodes", "tree_depth", "update_count", "weight_total", "belief_hash")


def _format(name):
    return next(f for f in FORMATS if f[0] == name)


def _engine(monkeypatch, fmt, **over):
    name, kind, domain, model, belief, env, kw, _ = fmt
    kw = dict(kw)
    kw.update(over)
    kw.setdefault("particles", 1 if belief == POINT else 130)
    kw.setdefault("slots", 3)
    kw.setdefault("runs", kw["slots"])
    kw.setdefault("seed", 7300 + len(name))
    kw.setdefault("sims", 16)
    kw.setdefault("horizon", HORIZON)
    if model != POMDP:
        kw.setdefault("episodes", EPISODES)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    eng = fba.Engine(domain, model=model, belief=belief, **kw)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return eng


def _runs(eng, offset=0):
    return np.array([5 + offset + 1000 * e for e in range(eng.slots)], np.int32)


def _start(eng, offset=0):
    """belief_init and the reset, every slot at a (run, episode) of its own"""
    episode = np.array([e % 2 for e in range(eng.slots)], np.int32)
    eng.set_position(run=_runs(eng, offset), episode=0, t=0)
    eng.belief_init()
    if eng.cfg.model != POMDP:
        eng.set_position(run=_runs(eng, offset), episode=episode, t=0)
        eng.belief_reset_domain_state()


def _obs_for(eng, kind, e, step):
    """an observation slot e's filter can produce (as tests/test_gpu_belief_forecast.py chooses them)"""
    if kind == "tiger":
        return (e + step) % 2
    s, _, _ = eng.belief_get(e, weights=False, counts=False)
    st = int(s[(7 * e + 3 * step) % len(s)])
    return st if kind == "gridworld" else st % eng.O


def _update(eng, kind, step, shift=0):
    """one per-call update: slot e at t = e % 3 + step, action (e + step // 2 + shift) % A, an observation its filter can produce"""
    E = eng.slots
    eng.set_position(t=np.array([e % 3 + step for e in range(E)], np.int32))
    action = np.array([(e + step // 2 + shift) % eng.A for e in range(E)], np.int32)      # (two steps of one action: cells raised twice)
    obs = np.array([_obs_for(eng, kind, e, step) for e in range(E)], np.int32)
    eng.belief_update(action, obs)


def _drive(eng, kind, steps=3):
    _start(eng)
    for step in range(steps):
        _update(eng, kind, step)


def _other(eng, kind):
    """a twin in another state: other positions, ONE update of another action, so that live buffer, hist_cnt and stride differ"""
    _start(eng, offset=77)
    _update(eng, kind, 0, shift=1)


def _weighted(eng):
    return eng.cfg.belief == N.BELIEF_IMPORTANCE


def _belief(eng, slot):
    s, w, cnt = eng.belief_get(slot, weights=_weighted(eng), counts=eng.ncnt > 0)
    return s.tobytes(), w.tobytes(), b"" if cnt is None else cnt.tobytes()


def _beliefs(eng, slots=None):
    return [_belief(eng, e) for e in (range(eng.slots) if slots is None else slots)]


def _heads(blocks):
    return np.ascontiguousarray(blocks[:, :64]).view(HEAD).reshape(-1)


def _state_offset(eng, record_format):
    """where the state word stands in a record, in bytes (fba_state.h: behind the counts; history records: word 0)"""
    if record_format >= 5:
        return 0
    if record_format == 0:
        return 4 * eng.ncnt
    if record_format == 1:
        return 4 * (eng.ncnt // 2)
    return 4 * (eng.factored_layout().n_counts // 2 + 1)


def _block_bytes(eng):
    n = eng.cfg.particles
    return 64 + (n * 8 if _weighted(eng) else 0) + n * eng.particle_bytes


def _pair(monkeypatch, name, steps=3, **over):
    """A driven for `steps` updates; B created alike, in another state; A's blocks"""
    fmt = _format(name)
    A, B = _engine(monkeypatch, fmt, **over), _engine(monkeypatch, fmt, **over)
    _drive(A, fmt[1], steps)
    _other(B, fmt[1])
    return fmt, A, B, A.belief_export()


# ---- 1. equal to the table form, every format -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_import_equals_the_table_form(name, monkeypatch):
    fmt, A, B, blocks = _pair(monkeypatch, name)
    E = A.slots
    assert A.belief_snapshot_bytes == _block_bytes(A) and blocks.shape == (E, _block_bytes(A)) and blocks.dtype == np.uint8
    heads = _heads(blocks)
    assert np.all(heads["magic"] == N.SNAPSHOT_MAGIC) and np.all(heads["version"] == N.SNAPSHOT_VERSION)
    if fmt[7] is not None:
        assert np.all(heads["record_format"] == fmt[7]), name
    assert np.all(heads["particles"] == A.cfg.particles) and np.all(heads["particle_bytes"] == A.particle_bytes)
    assert np.all(heads["counts_len"] == A.ncnt) and np.all(heads["weighted"] == int(_weighted(A)))
    assert np.all(heads["states"] == A.S) and np.all(heads["actions"] == A.A) and np.all(heads["observations"] == A.O)
    for e in range(E):    # the checksum by the header's formula, recomputed on the host
        assert N.snapshot_checksum(blocks[e, 64:]) == int(heads["checksum"][e]), (name, e)
    hist = heads["record_format"][0] >= 5
    if hist:
        total = sum((heads["hist_cnt"] >> np.uint32(8 * a)) & np.uint32(0xff) for a in range(4))
        assert np.all(total == 3) and np.all(heads["stride"] == 64), name
        before = _heads(B.belief_export())
        assert np.any(before["hist_cnt"] != heads["hist_cnt"]), name + ": the twin's entries per action differ before the import"
    else:
        assert np.all(heads["hist_cnt"] == 0) and np.all(heads["stride"] == A.particle_bytes), name
    want = _beliefs(A)
    assert _beliefs(B) != want, name + ": the twin differs before the import"
    # the payload is what the header says it is: weights, then records at the stride, the state word where the format has it
    n, stride = A.cfg.particles, int(heads["stride"][0])
    rec0, at = 64 + (n * 8 if _weighted(A) else 0), _state_offset(A, int(heads["record_format"][0]))
    for e in range(E):
        recs = blocks[e, rec0:rec0 + n * stride].reshape(n, stride)
        assert np.ascontiguousarray(recs[:, at:at + 4]).tobytes() == want[e][0], (name, e, "states")
        if _weighted(A):
            assert blocks[e, 64:rec0].tobytes() == want[e][1], (name, e, "weights")
        assert not blocks[e, rec0 + n * stride:].any(), (name, e, "zeros behind the last record")
        if not hist:
            assert not recs[:, at + 4:].any(), (name, e, "zeros behind the state word")
        else:
            assert not recs[:, 8 + 4 * 3:].any(), (name, e, "zeros behind the last entry")
    assert np.array_equal(A.belief_export(), blocks), name + ": two exports of one filter"
    B.belief_import(0, blocks)
    assert _beliefs(B) == want, name
    assert np.array_equal(B.belief_export(), blocks), name + ": export(import(x)) == x"
    assert _beliefs(A) == want, name + ": export changes nothing"
    A.close()
    B.close()


# ---- 2. the future is the same -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FUTURE)
def test_the_future_is_the_same(name, monkeypatch):
    fmt, A, B, blocks = _pair(monkeypatch, name)
    kind, E = fmt[1], A.slots
    B.belief_import(0, blocks)
    episode = np.array([e % 2 for e in range(E)], np.int32) if A.cfg.model != POMDP else 0
    for step in (3, 4):
        t = np.array([e % 3 + step for e in range(E)], np.int32)
        for eng in (A, B):
            eng.set_position(run=_runs(A), episode=episode, t=t)
        a_A, a_B = A.select_action(hist_len=t), B.select_action(hist_len=t)
        assert np.array_equal(a_A, a_B), (name, step)
        i_A, i_B = A.last_step_info(), B.last_step_info()
        for f in INFO_FIELDS[:4]:      # (what a search writes; the rest is still each context's own last update, which an import leaves alone)
            assert i_A[f].tobytes() == i_B[f].tobytes(), (name, step, f, "after select_action")
        obs = np.array([_obs_for(A, kind, e, step) for e in range(E)], np.int32)
        A.belief_update(a_A, obs)
        B.belief_update(a_B, obs)
        i_A, i_B = A.last_step_info(), B.last_step_info()
        for f in INFO_FIELDS:
            assert i_A[f].tobytes() == i_B[f].tobytes(), (name, step, f, "after belief_update")
    assert _beliefs(A) == _beliefs(B), name
    assert np.array_equal(A.belief_export(), B.belief_export()), name
    A.close()
    B.close()


# ---- 3. every stride ---------------------------------------------------------------------------------------------------------------
def test_every_stride(monkeypatch):
    fmt = _format("gridworld3_history_importance")
    over = dict(episodes=4, horizon=8)      # room for 32 entries: records of 144 bytes
    A = _engine(monkeypatch, fmt, **over)
    assert A.particle_bytes == 144
    _start(A)
    strides = {}
    for step in range(31):
        _update(A, fmt[1], step)
        if step + 1 not in (14, 15, 30, 31):
            continue
        blocks = A.belief_export()
        heads = _heads(blocks)
        total = sum((heads["hist_cnt"] >> np.uint32(8 * a)) & np.uint32(0xff) for a in range(4))
        assert np.all(total == step + 1)
        assert len(set(heads["stride"].tolist())) == 1
        strides[step + 1] = int(heads["stride"][0])
        B = _engine(monkeypatch, fmt, **over)
        _other(B, fmt[1])
        assert int(_heads(B.belief_export())["stride"][0]) == 64
        B.belief_import(0, blocks)
        assert _beliefs(B) == _beliefs(A), step + 1
        assert np.array_equal(B.belief_export(), blocks), step + 1
        B.close()
    assert strides == {14: 64, 15: 128, 30: 128, 31: 144}
    A.close()


# ---- 4. lazily reset rejection filter ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gridworld3_history_rejection", "packed_tiger", "packed_factored_tiger2"])
def test_export_straight_after_the_reset(name, monkeypatch):
    fmt = _format(name)
    A, B = _engine(monkeypatch, fmt), _engine(monkeypatch, fmt)
    _start(A)
    blocks = A.belief_export()           # (the states of a lazily reset filter exist in no record until now)
    _start(B, offset=4242)
    want = _beliefs(A)
    assert [b[0] for b in _beliefs(B)] != [w[0] for w in want], name + ": the twin's start states differ"
    B.belief_import(0, blocks)
    got = _beliefs(B)
    assert [g[0] for g in got] == [w[0] for w in want], name + ": states"
    assert got == want, name
    assert len(set(w[0] for w in want)) > 1 or name != "gridworld3_history_rejection"
    A.close()
    B.close()


# ---- 5. replicate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gridworld3_history_importance", "packed_tiger", "collision_avoidance_5x5x2_history"])
def test_replicate(name, monkeypatch):
    fmt = _format(name)
    kind = fmt[1]
    eng = _engine(monkeypatch, fmt, slots=70, runs=70)
    E = eng.slots
    assert E == 70
    _drive(eng, kind)
    src = _belief(eng, 0)
    last = _belief(eng, 69)
    assert _belief(eng, 37) != src
    eng.belief_replicate(0, 1, 68)
    for e in (1, 37, 68):
        assert _belief(eng, e) == src, (name, e)
    assert _belief(eng, 69) == last and _belief(eng, 0) == src, name
    eng.belief_replicate(5, 0, 70)       # the source inside the range
    blocks = eng.belief_export()
    assert all(np.array_equal(blocks[e], blocks[5]) for e in range(E)), name
    assert _belief(eng, 69) == src and _belief(eng, 5) == src, name
    # one filter at one position: one search, one update
    episode = 1 if eng.cfg.model != POMDP else 0
    eng.set_position(run=11, episode=episode, t=4)
    act = eng.select_action(hist_len=4)
    info = eng.last_step_info()
    assert len(set(act.tolist())) == 1, name
    for f in ("root_n", "root_q", "n_nodes", "tree_depth"):
        assert all(info[f][e].tobytes() == info[f][0].tobytes() for e in range(E)), (name, f)
    obs = _obs_for(eng, kind, 0, 4)
    eng.belief_update(act, obs)
    info = eng.last_step_info()
    # (belief_hash is filled by traced ticks only and reads 0 behind the per-call interface: the filters themselves are compared, bit for bit)
    assert len(set(info["belief_hash"].tolist())) == 1 and len(set(info["update_count"].tolist())) == 1, name
    assert len(set(info["weight_total"].tobytes()[8 * e:8 * e + 8] for e in range(E))) == 1, name
    blocks = eng.belief_export()
    assert all(np.array_equal(blocks[e], blocks[0]) for e in range(E)), name
    assert _belief(eng, 33) == _belief(eng, 0), name
    # ... and at positions apart the copies go their own ways: they are independent filters
    eng.set_position(run=np.arange(E, dtype=np.int32) * 13 + 1, episode=episode, t=5)
    obs = _obs_for(eng, kind, 0, 5)
    eng.belief_update(int(act[0]), obs)
    blocks = eng.belief_export()
    assert len(set(blocks[e, 64:].tobytes() for e in range(E))) == E, name + ": every copy has gone its own way"
    eng.close()


# ---- 6. ranges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gridworld3_history_importance", "dense_tiger"])
def test_ranges(name, monkeypatch):
    fmt, A, B, _ = _pair(monkeypatch, name, slots=70, runs=70)
    blocks = A.belief_export(17, 40)
    assert blocks.shape[0] == 40
    assert np.array_equal(blocks, A.belief_export()[17:57])
    before = _beliefs(B, (16, 57))
    B.belief_import(17, blocks)
    assert _beliefs(B, range(17, 57)) == _beliefs(A, range(17, 57)), name
    assert _beliefs(B, (16, 57)) == before, name
    assert before != _beliefs(A, (16, 57)), name
    A.close()
    B.close()


def test_ranges_in_several_chunks(monkeypatch):
    """staging memory for two blocks: seven slots leave and arrive in four chunks, and a bad block in the last chunk is met before the
    first chunk is committed"""
    fmt, A, B, whole = _pair(monkeypatch, "gridworld3_history_importance", slots=7, runs=7)
    monkeypatch.setenv("FBA_SNAPSHOT_STAGE_BYTES", str(2 * A.belief_snapshot_bytes + 100))
    blocks = A.belief_export()
    assert np.array_equal(blocks, whole)
    before = _beliefs(B)
    bad = blocks.copy()
    bad[6, 64 + 130 * 8 + 64 * 5] = 0xff        # particle 5 of the last block: a state of 255 + ...
    _resum(bad, 6)
    with pytest.raises(ValueError, match=r"block 6 \(slot 6\), particle 5: a state"):
        B.belief_import(0, bad)
    assert _beliefs(B) == before
    bad = blocks.copy()
    bad[5, -1] ^= 1
    with pytest.raises(ValueError, match=r"block 5 \(slot 5\): checksum"):
        B.belief_import(0, bad)
    assert _beliefs(B) == before
    B.belief_import(0, blocks)
    assert _beliefs(B) == _beliefs(A)
    assert np.array_equal(B.belief_export(), whole)
    A.close()
    B.close()


# ---- 7. after a run ----------------------------------------------------------------------------------------------------------------
def _into_fresh_and_used(monkeypatch, fmt, A, name):
    """A's blocks into a context that was never initiated and into one that holds filters of its own"""
    blocks, want = A.belief_export(), _beliefs(A)
    B = _engine(monkeypatch, fmt, slots=5, runs=5)
    with pytest.raises(fba.FbaError, match="belief not initiated"):
        B.belief_replicate(0, 1, 2)
    B.belief_import(0, blocks)
    assert _beliefs(B) == want, name
    assert np.array_equal(B.belief_export(), blocks), name
    C = _engine(monkeypatch, fmt, slots=5, runs=5)
    C.run_ticks(2)
    assert _beliefs(C) != want, name
    C.belief_import(0, blocks)
    assert _beliefs(C) == want, name
    assert np.array_equal(C.belief_export(), blocks), name
    B.close()
    C.close()
    return blocks


@pytest.mark.parametrize("name", ["gridworld3_history_importance", "packed_tiger"])
def test_after_run_ticks(name, monkeypatch):
    fmt = _format(name)
    A = _engine(monkeypatch, fmt, slots=5, runs=5)
    A.run_ticks(3)                        # (the throughput driver keeps every slot busy, whatever `runs` says: none is inactive here)
    blocks = _into_fresh_and_used(monkeypatch, fmt, A, name)
    assert all(blocks[e, 64:].any() for e in range(5)), name
    A.close()


@pytest.mark.parametrize("name", ["gridworld3_history_importance", "packed_tiger", "dense_tiger"])
def test_after_an_experiment_with_inactive_slots(name, monkeypatch):
    """three runs in five slots: after run_bapomdp slots 0..2 are inactive with the filters their runs ended on, slots 3 and 4 were never
    initiated.  A context created, driven and closed first leaves its records in freed device memory, which the next context's
    allocations may be handed: a never-initiated slot must still export a defined block, all zeros, that an import takes"""
    fmt = _format(name)
    stale = _engine(monkeypatch, fmt, slots=5, runs=5)
    stale.run_ticks(3)
    stale.close()
    A = _engine(monkeypatch, fmt, slots=5, runs=3)
    assert A.slots == 5
    A.run_bapomdp()
    blocks = _into_fresh_and_used(monkeypatch, fmt, A, name)
    heads = _heads(blocks)
    assert all(blocks[e, 64:].any() for e in range(3)), name
    for e in (3, 4):
        assert not blocks[e, 64:].any() and heads["hist_cnt"][e] == 0 and heads["checksum"][e] == 0, (name, e)
    A.close()


# ---- 8. refusals that leave the context untouched ----------------------------------------------------------------------------------
def _import_raw(eng, first, count, arr, nbytes):
    rc = eng.L.fba_belief_import(eng.h, first, count, arr.ctypes.data, nbytes)
    return rc, eng.L.fba_last_error(eng.h).decode()


def _resum(blocks, e):
    """the checksum of block e recomputed from the formula of include/fba_hip.h, for a block patched on purpose"""
    blocks[e, 56:64] = np.frombuffer(np.uint64(N.snapshot_checksum(blocks[e, 64:])).tobytes(), np.uint8)


def _put(blocks, e, offset, value, dtype):
    raw = np.array([value], dtype).tobytes()
    blocks[e, offset:offset + len(raw)] = np.frombuffer(raw, np.uint8)


def test_refused_imports_leave_the_context_untouched(monkeypatch):
    fmt, A, B, good = _pair(monkeypatch, "gridworld3_history_importance")
    n, per = A.cfg.particles, A.belief_snapshot_bytes
    before = _beliefs(B)
    rec0 = 64 + n * 8                      # where the records of a block start; they stand at 64 bytes here
    assert int(_heads(good)["stride"][0]) == 64

    def refused(blocks, match, first=0):
        with pytest.raises(ValueError, match=match):
            B.belief_import(first, blocks)
        assert _beliefs(B) == before, match

    bad = good.copy(); _put(bad, 1, 0, N.SNAPSHOT_MAGIC ^ 1, "<u4")
    refused(bad, r"block 1 \(slot 1\): magic")
    bad = good.copy(); _put(bad, 0, 4, 2, "<u2")
    refused(bad, "layout version 2 / 1")
    rc, msg = _import_raw(B, 0, 3, good, good.nbytes - 1)
    assert rc == N.EINVAL and "bytes %d / %d" % (good.nbytes - 1, good.nbytes) in msg, msg
    assert _beliefs(B) == before
    # an fp32-record block into the history context, and the other way round
    D = _engine(monkeypatch, _format("gridworld3_dense"))
    _drive(D, "gridworld")
    d_before, d_blocks = _beliefs(D), D.belief_export()
    refused(d_blocks, "record format 0 in the block, 5 in this context")
    with pytest.raises(ValueError, match="record format 5 in the block, 0 in this context"):
        D.belief_import(0, good)
    assert _beliefs(D) == d_before
    D.close()
    # 128 particles into 130
    F = _engine(monkeypatch, fmt, particles=128)
    _drive(F, fmt[1])
    refused(F.belief_export(), "particles 128 / 130")
    F.close()
    # the same records over a prior in which one count differs
    G = _engine(monkeypatch, fmt)
    prior = G.prior()
    prior[0] += 1.0
    G.set_model_factored(prior)
    _drive(G, fmt[1])
    g_blocks = G.belief_export()
    assert _heads(g_blocks)["prior_hash"][0] != _heads(good)["prior_hash"][0]
    refused(g_blocks, "prior hash")
    G.close()
    # one payload byte flipped
    bad = good.copy(); bad[2, rec0 + 64 * 9 + 5] ^= 0x10
    refused(bad, r"block 2 \(slot 2\): checksum")
    # the same with the checksum made right: the records themselves are judged
    bad = good.copy(); _put(bad, 1, rec0 + 64 * 7, A.S, "<i4"); _resum(bad, 1)
    refused(bad, r"block 1 \(slot 1\), particle 7: a state outside the domain")
    bad = good.copy(); _put(bad, 1, rec0 + 64 * 129, -1, "<i4"); _resum(bad, 1)
    refused(bad, r"\(slot 1\), particle 129: a state")
    entry = int(np.frombuffer(good[2, rec0 + 64 * 11 + 8:rec0 + 64 * 11 + 12].tobytes(), "<u4")[0])
    bad = good.copy(); _put(bad, 2, rec0 + 64 * 11 + 8, entry | (0x3ff << 20), "<u4"); _resum(bad, 2)     # the observation field: beyond O
    refused(bad, r"\(slot 2\), particle 11: a history entry")
    bad = good.copy(); _put(bad, 0, rec0 + 64 * 3 + 4, 0xffff, "<u2"); _resum(bad, 0)      # structure bits beyond the 2 * A nodes
    refused(bad, r"\(slot 0\), particle 3: an illegal parent-set word")
    bad = good.copy(); _put(bad, 0, 64 + 8 * 100, -0.25, "<f8"); _resum(bad, 0)
    refused(bad, r"\(slot 0\), particle 100: a weight")
    bad = good.copy(); _put(bad, 2, 64 + 8 * 129, np.nan, "<f8"); _resum(bad, 2)
    refused(bad, r"\(slot 2\), particle 129: a weight")
    # the first offender is named where there are several
    bad = good.copy(); _put(bad, 2, rec0 + 64 * 20, A.S + 5, "<i4"); _put(bad, 1, rec0 + 64 * 90, A.S, "<i4"); _resum(bad, 1); _resum(bad, 2)
    refused(bad, r"\(slot 1\), particle 90")
    # hist_cnt that does not go with the stride, or exceeds a record
    bad = good.copy(); _put(bad, 0, 40, 0x0f000000 + 0x01, "<u4")
    refused(bad, r"record stride 64 / \d+ for 16 entries")
    bad = good.copy(); _put(bad, 0, 40, 0x10101010, "<u4")
    refused(bad, "64 entries per record / room for 16")
    # a slot range outside the context
    refused(good, r"slots \[1, 4\) are not within the context's 3", first=1)
    with pytest.raises(ValueError, match="slots"):
        B.belief_export(2, 5)
    with pytest.raises(ValueError, match="slots"):
        B.belief_replicate(0, 2, 2)
    with pytest.raises(ValueError, match="source slot 3"):
        B.belief_replicate(3, 0, 2)
    assert _beliefs(B) == before
    # the good blocks are still taken
    B.belief_import(0, good)
    assert _beliefs(B) == _beliefs(A)
    A.close()
    B.close()


WORD_PATCHES = [
    # format, byte offset inside the record (or None: the state word), value, dtype, message
    ("packed_tiger", None, 2, "<i4", "a state outside the domain"),
    ("dense_factored_tiger2", 0, -1.0, "<f4", "a count that is negative or not finite"),
    ("dense_factored_tiger2", 8, np.inf, "<f4", "a count that is negative or not finite"),
    ("dense_factored_tiger2", "mask", 0xffff, "<u4", "an illegal parent-set word"),
    ("packed_factored_tiger2", "mask", 0x100, "<u4", "an illegal parent-set word"),
    ("gridworld3_table_history", 8, 0x3ff, "<u4", "a history entry"),
    ("collision_avoidance_5x5x2_history", 8, 0x7, "<u4", "a history entry"),
    ("plain_pomdp_tiger", None, 99, "<i4", "a state outside the domain"),
    ("point_estimate_tiger", None, -3, "<i4", "a state outside the domain"),
]


@pytest.mark.parametrize("name,where,value,dtype,message", WORD_PATCHES, ids=["%s-%d" % (w[0], i) for i, w in enumerate(WORD_PATCHES)])
def test_bad_records_are_refused_in_every_format(name, where, value, dtype, message, monkeypatch):
    fmt, A, B, good = _pair(monkeypatch, name)
    before = _beliefs(B)
    n = A.cfg.particles
    head = _heads(good)[1]
    stride, rec0 = int(head["stride"]), 64 + (n * 8 if _weighted(A) else 0)
    p = n - 1
    if where is None:
        where = _state_offset(A, int(head["record_format"]))
    elif where == "mask":
        lay = A.factored_layout()
        where = 4 * lay.n_counts if head["record_format"] == 0 else 4 * (lay.n_counts // 2)
    bad = good.copy()
    _put(bad, 1, rec0 + p * stride + where, value, dtype)
    _resum(bad, 1)
    with pytest.raises(ValueError, match=r"block 1 \(slot 1\), particle %d: %s" % (p, message)):
        B.belief_import(0, bad)
    assert _beliefs(B) == before, name
    B.belief_import(0, good)
    assert _beliefs(B) == _beliefs(A), name
    A.close()
    B.close()


@pytest.mark.parametrize("belief,domain,model,kw,says", [
    ("nested", "episodic-tiger", TABLE, dict(particles=6), "nested"),
    ("reinvigoration", "episodic-factored-tiger", FACT, dict(size=2, particles=16, resample_amount=2), "fully connected"),
    ("mh-within-gibbs", "continuous-factored-tiger", FACT, dict(size=2, particles=16, structure_prior=1, threshold=-1.0), "history"),
])
def test_beliefs_with_more_than_a_main_filter_are_refused(belief, domain, model, kw, says):
    eng = fba.Engine(domain, model=model, belief=belief, slots=2, runs=2, sims=8, horizon=4, episodes=2, **kw)
    eng.set_position(run=np.arange(2, dtype=np.int32), episode=0, t=0)
    eng.belief_init()
    per = eng.belief_snapshot_bytes
    assert per >= 64
    with pytest.raises(ValueError, match=says):
        eng.belief_export()
    with pytest.raises(ValueError, match=says):
        eng.belief_import(0, np.zeros((2, per), np.uint8))
    with pytest.raises(ValueError, match=says):
        eng.belief_replicate(0, 1, 1)
    eng.close()
