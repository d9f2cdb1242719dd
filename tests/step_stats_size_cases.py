"""The case table of tests/test_gpu_step_stats_sizes.py and the reference every fba_step_stats test compares with.

step_stats_kernel (fba_pomdp_amd/csrc/fba_step_stats.hip) changes what it does with the number of slots, the number of bins and the number
of actions; tests/test_gpu_step_stats.py runs 20 to 70 slots and at most 18 bins, which is one workgroup, one pass over the slots and one
LDS window.  Here the searches and filters are tiny (4 to 8 simulations, 8 particles) and the slots, the bins and A are the subject:

    switch-over                                      where                           what changes
    STEP_STATS_BLOCK = 1024 slots                    launch_step_stats               a second workgroup: the flush of one LDS table meets another's
                                                                                     in the bins (u64 adds, f64 adds, atomicMax on three maxima)
    STRIDE = BLOCK * STEP_STATS_GROUPS = 131 072     the `el +=` loop                a thread takes a second slot
    FIT = STEP_STATS_LDS / (8 * row_words(A)) bins   the `base` loop                 a second window: `bin - base`, clear / add / flush / barrier
                                                                                     per window, `a.bins + base + rw`, the slots read again, the
                                                                                     probe's mark consumed in the slot's own window only
    TWO_FIT = 2 * FIT                                                                a third window
    A                                                row_word(c, A), T0              the compressed row: A = 2 (coffee), 3, 4 and 16 (sysadmin of 8
                                                                                     computers), the last on both sides of FIT
    adv == 0 beside adv != 0                         the add loop                    budgeted searches in two workgroups

The yardstick is the trace: Ref aggregates Engine.trace() by (episode, t), integers exactly (np.add.at / np.maximum.at), the terms of every
double member sorted by bin and summed with math.fsum.  Integer members and the reward sums compare with ==, value_sum and value_sq_sum
within n * 2^-52 * sum |x_i| of the fsum (include/fba_hip.h), the probe members with Engine.probe() and the allowances derived in
tests/test_gpu_step_stats.py.  Every run stays below the trace's 2^22 records.

Eight particles, not one: a filter of one particle is certain where the tiger is, the first action of every episode opens a door, and no
launch would meet two bins.  Even so an episodic-tiger episode rarely lasts: on the CPU oracle, of 246 400 episodes of horizon 7 at these
sizes six reach t = 6 and 39 t = 5, so the episodic cases cannot put a step into the last row of a window (bin FIT - 1 is (43, 5) of 44 x 7).
They keep what only they have -- slots of one launch in many bins of several windows -- and assert steps in every window; every bin count
is therefore run a second time on the continuous tiger (same A, never terminal), where every row of every window has `runs` steps, the last
row of the last window included, as it has in the sysadmin cases.  (AGR has 23 actions, more than sysadmin, but no case: its rejection update
does not come to an end with a filter this small -- the CPU oracle was stopped after minutes on four runs of five steps -- and a filter that
serves it is not a tiny one.)

Bins no slot addresses.  A slot steps with episode in [first_episode, stop_episode) and t in [0, horizon): init_kernel and advance_kernel
are the only writers of DeviceState::episode and ::t in an experiment, advance_kernel ends an episode when env_kernel saw t + 1 == horizon
and a run when episode + 1 == stop_episode, fba_run_bapomdp_span refuses stop > episodes, and fba_run_ticks restarts a finished run at
first_episode instead of counting on.  (fba_set_position can write anything, but it belongs to the per-call interface, which fills no bin.)
So `episode * horizon + t` is within [0, n_bins) whenever adv != 0, and the `(unsigned)bin >= rows` guard serves only the windows: it has
no case of its own here."""
import math
import os
import re

import numpy as np

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

POMDP, TABLE, FACT = N.MODEL_POMDP, N.MODEL_BA_TABLE, N.MODEL_BA_FACTORED
U = 2.0 ** -53
INTS = ["steps", "terminals", "action", "root_visits", "nodes_sum", "depth_sum", "attempts_steps", "attempts_sum", "nodes_max", "depth_max",
        "attempts_max", "reserved"]
DOUBLES = ["reward_sum", "reward_sq_sum", "value_sum", "value_sq_sum"]
PROBE_INTS = ["probed", "evidence_zero"]
PROBE_DOUBLES = ["evidence_sum", "log_evidence_sum", "log_evidence_sq_sum", "next_true_sum", "post_ratio_sum"]
TRACE_CAP = 1 << 22


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
class Ref:
    """the trace aggregated by (episode, t): the integer members exactly, the terms of every double member kept for fsum and the bound
    (terms[f][e][t]: the terms of bin (e, t) in trace order)"""

    def __init__(self, eng, tr):
        E, H = max(eng.cfg.episodes, 1), eng.cfg.horizon
        nb, n = E * H, len(tr)
        bins = tr["episode"].astype(np.int64) * H + tr["t"].astype(np.int64)
        assert n == 0 or (bins.min() >= 0 and bins.max() < nb and tr["t"].max() < H)
        act = tr["action"].astype(np.int64)
        term = tr["terminal"] != 0
        upd = ~term & (tr["update_count"] >= 0)

        def summed(values, shape=()):
            out = np.zeros((nb,) + shape, np.uint64)
            np.add.at(out, bins, values.astype(np.uint64))
            return out

        def largest(values, where=None):
            out = np.zeros(nb, np.int32)
            np.maximum.at(out, bins if where is None else bins[where], values if where is None else values[where])
            return out

        b = np.zeros(nb, N.STEP_STAT_DTYPE)
        b["steps"] = summed(np.ones(n, np.uint64))
        b["terminals"] = summed(term)
        by_action = np.zeros((nb, N.MAX_ACTIONS), np.uint64)
        np.add.at(by_action, (bins, act), 1)
        b["action"] = by_action
        b["root_visits"] = summed(tr["root_n"], (N.MAX_ACTIONS,))
        b["nodes_sum"] = summed(tr["n_nodes"])
        b["depth_sum"] = summed(tr["tree_depth"])
        b["nodes_max"] = largest(tr["n_nodes"])
        b["depth_max"] = largest(tr["tree_depth"])
        b["attempts_steps"] = summed(upd)
        b["attempts_sum"] = summed(np.where(upd, tr["update_count"], 0))
        b["attempts_max"] = largest(tr["update_count"], upd)
        self.ints = b.reshape(E, H)
        # the doubles: sorted by bin, trace order kept within a bin
        order = np.argsort(bins, kind="stable")
        edge = np.searchsorted(bins[order], np.arange(nb + 1))
        q, rew = tr["root_q"][np.arange(n), act], tr["reward"]
        self.terms, self.sums, self.mags = {}, {}, {}
        self.count = (edge[1:] - edge[:-1]).reshape(E, H)
        for f, v in (("reward_sum", rew), ("reward_sq_sum", rew * rew), ("value_sum", q), ("value_sq_sum", q * q)):
            v = np.ascontiguousarray(v[order], np.float64)
            cut = [v[edge[i]:edge[i + 1]] for i in range(nb)]
            self.terms[f] = [cut[e * H:(e + 1) * H] for e in range(E)]
            self.sums[f] = np.array([math.fsum(x.tolist()) for x in cut]).reshape(E, H)
            self.mags[f] = np.array([math.fsum(np.abs(x).tolist()) for x in cut]).reshape(E, H)

    def bound(self, f):
        """n * 2^-52 * sum |x_i| per bin: what include/fba_hip.h allows a double member summed in any order"""
        return self.count * (2 * U) * self.mags[f]

    def check(self, st, what, probe=True):
        """every bin and every member; returns the largest error / bound of the value sums"""
        assert st.shape == self.ints.shape, what
        for f in INTS:
            assert np.array_equal(st[f], self.ints[f]), f"{what}: {f}\n{st[f]}\n{self.ints[f]}"
        worst = 0.0
        for f in DOUBLES:
            dev, ref = st[f], self.sums[f]
            if f.startswith("reward"):
                bad = np.argwhere(dev != ref)
                assert bad.size == 0, f"{what}: {f}{bad[0].tolist()} {dev[tuple(bad[0])]!r} != {ref[tuple(bad[0])]!r}"
            else:
                bound, err = self.bound(f), np.abs(dev - ref)
                bad = np.argwhere(~(err <= bound))
                assert bad.size == 0, f"{what}: {f}{bad[0].tolist()} {dev[tuple(bad[0])]!r} against {ref[tuple(bad[0])]!r}, bound {bound[tuple(bad[0])]:.3e}"
                if np.any(bound > 0):
                    worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
        print(f"{what}: largest value-sum error / bound {worst:.3e}")
        if probe:
            for f in PROBE_INTS + PROBE_DOUBLES:
                assert not np.any(st[f]), f"{what}: {f} without a probe"
        return worst


def probe_ref(recs, shape):
    terms = {f: [[[] for _ in range(shape[1])] for _ in range(shape[0])] for f in PROBE_DOUBLES + ["log_err", "log_sq_err", "ratio_err"]}
    ints = np.zeros(shape, N.STEP_STAT_DTYPE)
    for r in recs:
        e, t = int(r["episode"]), int(r["t"])
        ev, nt, pt = float(r["evidence"]), float(r["next_true"]), float(r["post_true"])
        ints["probed"][e, t] += 1
        ints["evidence_zero"][e, t] += int(ev == 0.0)
        terms["evidence_sum"][e][t].append(ev)
        terms["next_true_sum"][e][t].append(nt)
        if ev > 0.0:
            l = math.log(ev)
            d = 3e-16 * max(1.0, abs(l))
            terms["post_ratio_sum"][e][t].append(pt / ev)
            terms["ratio_err"][e][t].append(U * pt / ev)
            terms["log_evidence_sum"][e][t].append(l)
            terms["log_err"][e][t].append(d)
            terms["log_evidence_sq_sum"][e][t].append(l * l)
            terms["log_sq_err"][e][t].append(2 * abs(l) * d + d * d + U * l * l)
    return ints, terms


def check_probe(st, ints, terms, what):
    for f in PROBE_INTS:
        assert np.array_equal(st[f], ints[f]), f"{what}: {f}"
    extra = {"evidence_sum": None, "next_true_sum": None, "post_ratio_sum": "ratio_err", "log_evidence_sum": "log_err", "log_evidence_sq_sum": "log_sq_err"}
    for f in PROBE_DOUBLES:
        for e in range(st.shape[0]):
            for t in range(st.shape[1]):
                x = terms[f][e][t]
                mag = math.fsum(abs(v) for v in x)
                bound = len(x) * 2 * U * mag + (math.fsum(terms[extra[f]][e][t]) if extra[f] else U * mag)
                dev, ref = float(st[f][e, t]), math.fsum(x)
                assert abs(dev - ref) <= bound, f"{what}: {f}[{e}][{t}] {dev!r} against {ref!r}, bound {bound:.3e}"
                if not x:
                    assert dev == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# the thresholds, as the sources state them
# ---------------------------------------------------------------------------------------------------------------------------------------
def constants():
    """STEP_STATS_BLOCK, _GROUPS, _LDS, _ROW_TAIL (fba_kernels.h) and FBA_MAX_ACTIONS (include/fba_hip.h); the two formulas they enter are
    checked to read as fit() restates them"""
    with open(os.path.join(N.HERE, "csrc", "fba_kernels.h")) as f:
        header = f.read()
    with open(os.path.join(N.ROOT, "include", "fba_hip.h")) as f:
        api = f.read()
    k = {}
    for name in ("STEP_STATS_BLOCK", "STEP_STATS_GROUPS", "STEP_STATS_LDS", "STEP_STATS_ROW_TAIL"):
        (v,) = re.findall(r"constexpr\s+int\s+%s\s*=\s*([\d\s*]+);" % name, header)
        k[name] = math.prod(int(x) for x in v.split("*"))
    (v,) = re.findall(r"#define\s+FBA_MAX_ACTIONS\s+(\d+)", api)
    k["FBA_MAX_ACTIONS"] = int(v)
    assert re.search(r"int step_stats_row_words\(int A\) \{ return 2 \+ 2 \* \(A < FBA_MAX_ACTIONS \? A : FBA_MAX_ACTIONS\) \+ STEP_STATS_ROW_TAIL; \}", header)
    assert re.search(r"int step_stats_rows\(int n_bins, int A\) \{ const int fit = STEP_STATS_LDS / \(step_stats_row_words\(A\) \* 8\); "
                     r"return n_bins < fit \? n_bins : fit; \}", header)
    return k


K = constants()
BLOCK, GROUPS = K["STEP_STATS_BLOCK"], K["STEP_STATS_GROUPS"]
STRIDE = BLOCK * GROUPS


def row_words(A):
    return 2 + 2 * min(A, K["FBA_MAX_ACTIONS"]) + K["STEP_STATS_ROW_TAIL"]


def fit(A):
    """the rows of a workgroup's LDS table: the bins one window serves (step_stats_rows)"""
    return K["STEP_STATS_LDS"] // (row_words(A) * 8)


def windows(n_bins, A):
    return -(-n_bins // min(n_bins, fit(A)))


def workgroups(slots):
    return min(-(-slots // BLOCK), GROUPS)


def workgroup_of(slot, slots):
    """the workgroup that reduces a slot of a context of `slots` (launch_step_stats, the `el` loop); slot: a number or an array"""
    return (slot // BLOCK) % workgroups(slots)


def threshold(switch, A):
    return {"STEP_STATS_BLOCK": BLOCK, "STRIDE": STRIDE, "FIT": fit(A), "TWO_FIT": 2 * fit(A)}[switch]


def measure(switch, c):
    """what a case holds against a switch-over: its slots or its bins"""
    return c["slots"] if switch in ("STEP_STATS_BLOCK", "STRIDE") else c["n_bins"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------------
# family -> the switch-overs its cases hold both sides of
SWITCHES = {
    "workgroups": ("STEP_STATS_BLOCK",),
    "stride": ("STRIDE",),
    "windows_tiger": ("FIT", "TWO_FIT"),
    "windows_continuous_tiger": ("FIT", "TWO_FIT"),
    "windows_sysadmin": ("FIT",),
    "windows_probe": ("TWO_FIT",),
    # single cases: c["past"] names what each is beyond
    "fewest_actions": (),
    "windows_workgroups": (),
    "windows_probe_range": (),
    "budgeted": (),
}
ACTIONS = {"episodic-tiger": 3, "continuous-tiger": 3, "gridworld": 4, "coffee": 2}     # (sysadmin: 2 * size)
ENDS_EPISODES = ("episodic-tiger", "gridworld")
TIGER_HORIZONS = (6, 7)     # the horizons of the window cases' products
PARTICLES = 8

CASES = []


def add(family, name, domain, model, belief, slots, horizon, episodes=1, probe=None, trace_off=False, past=(), seed=None, **kw):
    """runs = slots: run r is executed by slot r.  probe: None, "full" or (first, count); trace_off: the case is run again with
    trace = 0 and compared with the traced run's bins"""
    kw.setdefault("sims", 4)
    kw.setdefault("particles", PARTICLES)
    A = 2 * kw["size"] if "sysadmin" in domain else ACTIONS[domain]
    cfg = dict(domain=domain, model=model, belief=belief, slots=slots, runs=slots, horizon=horizon, seed=9300 + len(CASES) if seed is None else seed, **kw)
    if model != POMDP:
        cfg["episodes"] = episodes
    else:
        assert episodes == 1
    CASES.append(dict(name=f"{family}_{name}", family=family, cfg=cfg, slots=slots, n_bins=episodes * horizon, A=A, probe=probe,
                      trace_off=trace_off, past=past, ends=domain in ENDS_EPISODES))


def products_around(limit):
    """(episodes, horizon) of the largest product <= limit and of the smallest > limit, horizon in TIGER_HORIZONS"""
    below = max(((limit // h, h) for h in TIGER_HORIZONS), key=lambda p: p[0] * p[1])
    above = min(((limit // h + 1, h) for h in TIGER_HORIZONS), key=lambda p: p[0] * p[1])
    return below, above


TIGER = ("episodic-tiger", TABLE, "rejection_sampling")
# ---- workgroups: episodes end at different steps, so one launch meets several bins
# (BLOCK + 1 slots: under this seed the one slot of the second workgroup holds nodes_max of bin (0, 0), by the CPU oracle's trace)
for n in (BLOCK, BLOCK + 1, 2 * BLOCK + 1):
    add("workgroups", str(n), *TIGER, slots=n, episodes=2, horizon=3, seed=9401 if n == BLOCK + 1 else None)
# ---- stride: a thread's second slot.  2 x 2 bins: at most 4 records a run, 2^19 + 4 in all, 185 MB of trace on the host
for n in (STRIDE, STRIDE + 1):
    add("stride", str(n), *TIGER, slots=n, episodes=2, horizon=2)
# ---- windows, A = 3: FIT (or the largest product below it), the smallest product beyond it, the smallest beyond two windows.  On the
# episodic tiger the rows that these two put into the new window are (43, 6) and (87, 5), (87, 6), which no episode reaches: each is
# followed by the same shape with one episode more, whose new window holds a whole episode
_below, _above = products_around(fit(3))
_third = products_around(2 * fit(3))[1]
_above1, _third1 = (_above[0] + 1, _above[1]), (_third[0] + 1, _third[1])
WINDOW_SHAPES = (_below, _above, _third)
for e, h in (_below, _above, _above1, _third, _third1):
    add("windows_tiger", f"{e}x{h}", *TIGER, slots=70, episodes=e, horizon=h)
for e, h in (_below, _above, _third):
    add("windows_continuous_tiger", f"{e}x{h}", "continuous-tiger", TABLE, "rejection_sampling", slots=70, episodes=e, horizon=h)
# ---- windows, the largest A: planning, one episode, horizon = FIT and FIT + 1.  Sysadmin of 8 computers has 16 actions
for h in (fit(16), fit(16) + 1):
    add("windows_sysadmin", str(h), "linear-sysadmin", POMDP, "rejection_sampling", slots=40, horizon=h, size=8)
# ---- the fewest actions a domain has: coffee's two (horizon <= 255 bins never leave its one window of fit(2) rows)
add("fewest_actions", "coffee", "coffee", POMDP, "rejection_sampling", slots=33, horizon=9)
# ---- windows x workgroups, and the same with the trace off
add("windows_workgroups", f"{BLOCK + 1}_{_above1[0]}x{_above1[1]}", *TIGER, slots=BLOCK + 1, episodes=_above1[0], horizon=_above1[1], trace_off=True,
    past=("STEP_STATS_BLOCK", "FIT"))
# ---- windows x probe: the mark of a slot is consumed in the slot's own window, once
for e, h in (_above, _above1, _third):
    add("windows_probe", f"{e}x{h}", *TIGER, slots=70, episodes=e, horizon=h, probe="full", past=("FIT",))
add("windows_probe_range", f"{BLOCK + 1}_{_third[0]}x{_third[1]}", *TIGER, slots=BLOCK + 1, episodes=_third[0], horizon=_third[1],
    probe=(BLOCK - 5, 6), past=("STEP_STATS_BLOCK", "TWO_FIT"))
# ---- budgeted searches: a launch holds slots that took their step and slots that did not, in both workgroups
add("budgeted", str(BLOCK + 1), "gridworld", FACT, "importance_sampling", slots=BLOCK + 1, episodes=2, horizon=5, size=3, structure_prior=2, sims=8,
    search_budget=7, past=("STEP_STATS_BLOCK",))

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES) and {c["family"] for c in CASES} == set(SWITCHES)


def engine(c, **kw):
    args = dict(c["cfg"], **kw)
    return fba.Engine(args.pop("domain"), **args)


def run(eng):
    return eng.run_planning() if eng.cfg.model == POMDP else eng.run_bapomdp()
