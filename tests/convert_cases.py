"""The cases of tests/test_gpu_belief_convert.py (fba_belief_convert: snapshot blocks of one context refitted to another that differs in
its particle count or in the room of a history record) and the host's restatement of which particle becomes which, which needs no GPU
and is checked by tests/test_belief_convert_cpu.py.

Every case is a row of the FORMATS table of tests/test_gpu_belief_snapshot.py at the shapes of tests/resume_cases.py: 130 particles,
16 simulations, horizon 8, 3 to 7 slots, and the seeds found there.  A history record has room for episodes * horizon entries, so a
context of 2 episodes stores records of 80 bytes, one of 4 episodes 144, one of 5 episodes 176; a slot stores its records at 64 bytes up
to 14 entries, at 128 up to 30 and whole beyond.  With the seeds of resume_cases.py some run makes at least 15 updates in a 2-episode
context (records at 80 bytes) and at least 31 in a 4-episode one (at 144): test_belief_convert_cpu.py establishes it on the oracle."""
import ctypes as C
import functools

import numpy as np

import resume_cases as R
import wide_launch_cases as W
from oracle import pyorc as orc
from resume_cases import SEEDS, config, make_engine       # noqa: F401  (the cases' configuration, reused as it stands)
from test_gpu_belief_snapshot import FORMATS              # noqa: F401

PH_CONVERT = 14                 # FBA_PHASE_CONVERT
SHORT, MIDDLE, LONG = 2, 4, R.EPISODES        # episodes of the source contexts and of the destination
ROOM_BYTES = {e: W.record_bytes(e, R.HORIZON) for e in (SHORT, MIDDLE, LONG)}       # 80, 144, 176
IDENTITY = R.SPLIT_FORMATS
HISTORY, GRIDWORLD_HISTORY = R.HISTORY, R.GRIDWORLD_HISTORY
LONGER = GRIDWORLD_HISTORY + ["packed_tiger"]
FLAT = ["packed_tiger", "gridworld3_history_rejection"]
WEIGHTED = ["dense_tiger", "gridworld3_history_importance"]
FLAT_COUNTS = [(130, 37), (130, 300)]
WEIGHTED_COUNTS = [(130, 37), (130, 300), (300, 37), (300, 130), (300, 300)]


def stride_in(room_bytes, entries, full=False):
    """bytes between the records of a slot whose records of room_bytes hold `entries` entries (history_stride_bytes)"""
    need = 8 + 4 * entries
    if full:
        return room_bytes
    return 64 if need <= 64 < room_bytes else (128 if need <= 128 < room_bytes else room_bytes)


@functools.lru_cache(maxsize=None)
def updates_in(name, episodes, seed=None):
    """per run: the belief updates (= entries of a history record) of a whole experiment of `episodes` episodes, on the oracle"""
    over = dict(episodes=episodes)
    if seed is not None:
        over["seed"] = seed
    domain, model, belief, _, kw = R.config(name, **over)
    kw = {k: v for k, v in kw.items() if k != "slots"}
    o = W.make_oracle(dict(domain=domain, model=model, belief=belief, kw=kw))
    _, res = o.run_bapomdp()
    assert not o.L.orc_error(o.h)
    tr = o.trace(res.n_trace)
    upd = np.zeros(R.SLOTS[name], np.int64)
    np.add.at(upd, tr["run"], (tr["terminal"] == 0).astype(np.int64))
    return upd


def weighted_pick(incl, thr):
    """WeightedFilter::sample in device order: the largest i >= 1 whose exclusive prefix sum is below the threshold, else 0"""
    return int(np.searchsorted(incl[:-1], thr, "left"))


def _first_draws(seed, run, n, draw):
    L = orc.lib()
    g = orc.Rng()
    L.orc_rng_init_philox(C.byref(g), seed)
    L.orc_rng_episode(C.byref(g), run, 0, 0)
    out = []
    for j in range(n):
        L.orc_rng_stream(C.byref(g), PH_CONVERT, j)
        out.append(draw(L, g))
    return out


def expected_sources(seed, first_run, b, n_src, n_dst, weights=None):
    """the source particle of every output particle of block b (include/fba_hip.h, fba_belief_convert)"""
    if n_src == n_dst:
        return np.arange(n_dst)
    if weights is None:
        return np.array(_first_draws(seed, first_run + b, n_dst, lambda L, g: L.orc_int(C.byref(g), n_src)))
    _, incl = orc.dev_scan(np.asarray(weights, np.float64))
    total = incl[n_src - 1]
    u = _first_draws(seed, first_run + b, n_dst, lambda L, g: L.orc_u01(C.byref(g)))
    return np.array([weighted_pick(incl, x * total) for x in u])


def set_weights(blocks, weights):
    """a copy of weighted blocks [count, bytes] with the weights [count, n] put in their place and the checksums made right again"""
    from fba_pomdp_amd import _native as N
    out = np.array(blocks, np.uint8, copy=True)
    n = weights.shape[1]
    for b in range(out.shape[0]):
        out[b, 64:64 + 8 * n] = np.frombuffer(np.ascontiguousarray(weights[b], "<f8").tobytes(), np.uint8)
        out[b, 56:64] = np.frombuffer(np.uint64(N.snapshot_checksum(out[b, 64:])).tobytes(), np.uint8)
    return out


def random_weights(rng, count, n, zeros=False):
    """random positive weights of very unequal size; zeros: every third one 0.0"""
    w = rng.random((count, n)) * np.exp(rng.normal(0.0, 2.0, (count, n)))
    w[w <= 0.0] = 1.0
    if zeros:
        w[:, ::3] = 0.0
    return w
