"""Shared by the tests of fba_structure_stats: the host-side yardstick, the comparison and the table of sizes at which the reduction of
fba_structure_stats.hip takes another path.

The yardstick is existing code, never the code under test (the scheme of tests/test_gpu_belief_probe.py): a context R created like the
one under test, statistics off, is advanced one run_ticks(1) at a time.  Before tick k it is asked for belief_structures(0, slots,
top_k=0, queries=Q) -- fba_belief_structures, which test_gpu_belief_structures.py holds to numpy -- and for cnt[q], the particles whose
word list is query q, through structure_cases.words_of in numpy; after the tick its last_step_info() names the step of every slot
(a slot whose record did not change took no step; under a search budget run_ticks(K) is not K calls of run_ticks(1), and
test_search_budget keys a run without a budget instead).  What a step adds to its bin is keyed by (run, episode, t) and summed on the host.

Bound (derived): a term mass / W carries the bound of fba_belief_structures on the mass and on W, 8 N 2^-53 relative each to first order
on either side, and one rounding of the division; the sum of n terms adds n 2^-53.  Device and reference each stay within
(8 N + n + 1) 2^-53 relative of the exact value, so |dev - ref| <= 2 (8 N + n + 1) 2^-53 max(dev, ref), and a member is exactly 0.0
where the reference is.  In a flat filter of N = 2^k particles every term is j / N and every sum exact: equality."""
import os
import re

import numpy as np

from fba_pomdp_amd import _native as N
import structure_cases as SC

INTS = ("steps", "weightless", "overflowed", "collapsed", "distinct_sum", "distinct_max")
KEY = ("run", "episode", "t")
CSRC = os.path.join(N.HERE, "csrc")


def key_of(rec):
    return tuple(int(rec[k]) for k in KEY)


def step_value(weight_total, set_mass, query_mass, distinct, overflow, cnt, particles):
    """what one step adds to its bin, from what fba_belief_structures says of the step's filter and the particle counts per query"""
    W = float(weight_total)
    weighs = bool(np.isfinite(W) and W > 0.0)
    cnt = np.asarray(cnt, np.int64)
    return dict(weightless=int(not weighs), overflowed=int(overflow != 0), collapsed=int(distinct == 1 and overflow == 0), distinct=int(distinct),
                set_frac=np.asarray(set_mass, np.float64) / W if weighs else np.zeros_like(np.asarray(set_mass, np.float64)),
                query_frac=np.asarray(query_mass, np.float64) / W if weighs else np.zeros(len(cnt), np.float64),
                held=(cnt > 0).astype(np.uint64), sole=(cnt == particles).astype(np.uint64))


def counts_of(eng, slot, queries):
    """cnt[q] of a slot, in numpy over belief_get"""
    _, words = SC.words_of(eng, slot)
    q = np.asarray(queries, np.uint32).reshape(-1, words.shape[1])
    return np.array([int(np.sum(np.all(words == row[None, :], axis=1))) for row in q], np.int64)


def follow(make, K, queries, what, flat_counts=False):
    """R, tick by tick: {(run, episode, t): step_value} of the K ticks, and R (open).  flat_counts: cnt[q] of a flat filter is read from
    query_mass -- every weight is 1.0, so the mass IS the count (include/fba_hip.h: an exact integer) -- after the first tick has shown
    that on every slot through words_of; the wide launches use it, where a belief_get per slot and tick would take minutes."""
    R = make()
    R.run_ticks(0)
    E, n = R.slots, R.cfg.particles
    nq = len(queries)
    prev = R.last_step_info().copy()
    vals = {}
    for k in range(K):
        bs = R.belief_structures(0, E, top_k=0, queries=queries)
        if flat_counts:
            assert not SC.weighted(R)
            cnts = np.rint(bs.query_mass).astype(np.int64)
            if k == 0:
                for e in sorted(set(range(min(E, 8))) | set(range(0, E, 509))):      # (a belief_get each: a sample of the slots where they are thousands)
                    assert np.array_equal(counts_of(R, e, queries), cnts[e]), f"{what}: slot {e}"
        else:
            cnts = np.array([counts_of(R, e, queries) for e in range(E)]).reshape(E, nq)
        R.run_ticks(1)
        info = R.last_step_info().copy()
        for e in range(E):
            if info[e].tobytes() == prev[e].tobytes():
                continue      # (a budgeted search that has not finished: the slot took no step in this tick)
            key = key_of(info[e])
            assert key not in vals, f"{what}: tick {k}, slot {e}: step {key} twice"
            vals[key] = step_value(bs.weight_total[e], bs.set_mass[e], bs.query_mass[e], bs.distinct[e], bs.overflow[e], cnts[e], n)
        prev = info
    return vals, R


def bins_of(vals, episodes, horizon, n_words, n_sets, nq, keep=lambda key: True):
    """the bins as the header defines them, summed on the host over the steps `keep` admits"""
    head = np.zeros((episodes, horizon), N.STRUCTURE_STAT_DTYPE)
    sf = np.zeros((episodes, horizon, n_words, n_sets), np.float64)
    qf = np.zeros((episodes, horizon, nq), np.float64)
    qh = np.zeros((episodes, horizon, nq), np.uint64)
    qs = np.zeros((episodes, horizon, nq), np.uint64)
    for key in sorted(vals):
        if not keep(key):
            continue
        v, (_, e, t) = vals[key], key
        h = head[e, t]
        h["steps"] += 1
        h["weightless"] += v["weightless"]
        h["overflowed"] += v["overflowed"]
        h["collapsed"] += v["collapsed"]
        h["distinct_sum"] += v["distinct"]
        h["distinct_max"] = max(int(h["distinct_max"]), v["distinct"])
        sf[e, t] += v["set_frac"]
        qf[e, t] += v["query_frac"]
        qh[e, t] += v["held"]
        qs[e, t] += v["sole"]
    return head, sf, qf, qh, qs


def compare(dev, ref, particles, what, exact=False, table=True):
    """Engine.structure_stats() against bins_of(); table=False leaves out the members that depend on the table of distinct graphs"""
    head, sf, qf, qh, qs = ref
    for f in INTS:
        if not table and f in ("collapsed", "distinct_sum", "distinct_max"):
            continue
        assert np.array_equal(dev.head[f], head[f]), f"{what}: {f}: {dev.head[f].tolist()} != {head[f].tolist()}"
    assert not np.any(dev.head["reserved"])
    assert np.array_equal(dev.query_held, qh), what + ": query_held"
    assert np.array_equal(dev.query_sole, qs), what + ": query_sole"
    n = head["steps"].astype(np.float64)
    for name, d, r in (("set_frac", dev.set_frac, sf), ("query_frac", dev.query_frac, qf)):
        assert d.shape == r.shape, f"{what}: {name}"
        assert np.all(np.isfinite(d)), f"{what}: {name}"
        assert np.all(d[r == 0.0] == 0.0), f"{what}: {name} is not 0.0 where the reference is"
        bound = 2.0 * (8.0 * particles + n + 1.0) * 2.0 ** -53
        bound = bound.reshape(bound.shape + (1,) * (d.ndim - 2))
        scale, err = np.maximum(d, r), np.abs(d - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(scale > 0, err / scale, 0.0)
        print(f"{what}: {name}: largest relative difference {rel.max() if rel.size else 0.0:.3e}, smallest bound {bound.min():.3e}")
        assert np.all(err <= bound * scale), f"{what}: {name}"
        if exact:
            assert np.array_equal(d, r), f"{what}: {name} differs in a flat filter of 2^k particles"


# ---- the sizes at which the reduction changes (fba_kernels.h, fba_structure_stats.hip) ------------------------------------------------
def constants():
    """the constants of the reduction, read out of fba_kernels.h"""
    text = open(os.path.join(CSRC, "fba_kernels.h")).read()
    out = {}
    for name in ("BIN_HEAD", "SLOT_HEAD", "BLOCK", "BINS_BLOCK", "GROUP_SLOTS", "LDS_WORDS", "COLS", "CHUNK_SLOTS"):
        out[name] = int(re.search(r"constexpr int STRUCT_STATS_%s\s*=\s*(\d+);" % name, text).group(1))
    m = re.search(r"constexpr size_t STRUCT_STATS_ROWS_BYTES = \(size_t\)(\d+) << (\d+);", text)
    out["ROWS_BYTES"] = int(m.group(1)) << int(m.group(2))
    return out


def row_words(n_words, n_sets, nq, c=None):
    c = c or constants()
    return c["BIN_HEAD"] + n_words * n_sets + 3 * nq


def plan(slots, bins, n_words, n_sets, nq, c=None):
    """(chunks, workgroups of the first chunk's second stage, column windows, bin windows) of a tick, as fba_kernels.h decides them"""
    c = c or constants()
    rw = row_words(n_words, n_sets, nq, c)
    cap = min(c["CHUNK_SLOTS"], c["ROWS_BYTES"] // ((c["SLOT_HEAD"] + rw - c["BIN_HEAD"]) * 8))
    chunk = max(1, min(slots, cap))
    cols = min(rw, c["COLS"])
    win = min(bins, c["LDS_WORDS"] // cols)
    up = lambda a, b: -(-a // b)
    return up(slots, chunk), up(min(slots, chunk), c["GROUP_SLOTS"]), up(rw, cols), up(bins, win)


# the gridworld's history records: a parent-set word per action for each of the x and y transition nodes, three candidate parents
GW_WORDS, GW_SETS = 8, 8
# name -> (slots, episodes, horizon, nq, ticks): both sides of every size at which plan() changes, at the gridworld's row lengths
#   slots      a second workgroup of stage two behind GROUP_SLOTS slots, a second chunk behind CHUNK_SLOTS
#   row words  6 + 64 + 3 nq: 94 words at 8 queries are one window of COLS = 96 words, 97 at 9 queries are two
#   bins       LDS_WORDS / min(row words, COLS) rows fit a window: 7680 / 96 = 80 bins at 9 queries and up
SIZE_CASES = {
    "ragged_150_slots": (150, 2, 8, 3, 12),
    "slots_one_workgroup": (256, 2, 6, 3, 8),
    "slots_two_workgroups": (257, 2, 6, 3, 8),
    "slots_one_chunk": (32768, 2, 4, 2, 3),
    "slots_two_chunks": (32769, 2, 4, 2, 3),
    "row_one_window": (5, 2, 6, 8, 14),
    "row_two_windows": (5, 2, 6, 9, 14),
    "bins_one_window": (5, 10, 8, 9, 80),
    "bins_two_windows": (5, 9, 9, 9, 81),
    "bins_second_window_used": (5, 10, 9, 9, 90),      # (the last episode's bins stand in the second window: steps are taken there)
}
# what plan() must say of them: (chunks, workgroups, column windows, bin windows)
SIZE_PLANS = {
    "ragged_150_slots": (1, 1, 1, 1),
    "slots_one_workgroup": (1, 1, 1, 1),
    "slots_two_workgroups": (1, 2, 1, 1),
    "slots_one_chunk": (1, 128, 1, 1),
    "slots_two_chunks": (2, 128, 1, 1),
    "row_one_window": (1, 1, 1, 1),
    "row_two_windows": (1, 1, 2, 1),
    "bins_one_window": (1, 1, 2, 1),
    "bins_two_windows": (1, 1, 2, 2),
    "bins_second_window_used": (1, 1, 2, 2),
}
