"""Shared by the tests of fba_giveup_policy: the case table and the predictor.

The oracle never gives up, and its trace holds the update_count of every belief update.  A rejection update gives up iff its update_count
would exceed max_attempts, so under FBA_GIVEUP_RETIRE a run is retired at its FIRST record with update_count > max_attempts and nothing
behind that record exists for it.  Runs never couple (their streams are addressed by run), so everything the engine must report follows
from the oracle's trace alone -- predict() below: the retired list, the surviving records, returns and lengths, the per-episode statistics
(fed through orc_stat_add in run order, as the experiment feeds them), the counters and the `steps` of the step-statistics bins.

Every case: Philox streams, device arithmetic, 16 simulations, 48 runs of 2 episodes in 16 slots, so every slot executes three runs and a
slot whose run is retired has another to go on with.  max_attempts is chosen so that some runs are retired and some survive, in either
episode (mix_conditions); tests/test_giveup_cpu.py holds every case to that on the oracle, without a GPU."""
import ctypes as C
import re
import os

import numpy as np

import wide_launch_cases as W
from wide_launch_cases import FACT, REJ, TABLE
from oracle import pyorc as orc

RUNS, SLOTS = 48, 16
COMMON = dict(sims=16, episodes=2)

# name -> the case with max_attempts and the update kernel the launch plan chooses for it (update_plan() below asks the context)
CASES = {}


def add(name, domain, model, fmt, max_attempts, kernel, belief=REJ, **kw):
    CASES[name] = dict(W.case(name, domain, model, belief, fmt, E=SLOTS, runs=RUNS, **dict(COMMON, **kw)), max_attempts=max_attempts, kernel=kernel)


add("tiger_lds", "episodic-tiger", TABLE, "packed_tiger", 1024, "reject_tiger_lds_kernel", particles=512, horizon=4, seed=5)
add("tiger_once", "episodic-tiger", TABLE, "packed_tiger", 8192, "reject_tiger_once_kernel", particles=4096, horizon=4, seed=5)
add("ctiger", "continuous-tiger", TABLE, "packed_tiger", 2048, "reject_tiger_lds_kernel", particles=512, horizon=5, seed=5)
add("ftiger", "episodic-factored-tiger", FACT, "packed_ftiger", 1024, "reject_kernel<packed factored tiger>", size=2, structure_prior=2, particles=512,
    horizon=4, seed=5)
add("gw3_fact", "gridworld", FACT, "history", 2048, "reject_hist_kernel", size=3, structure_prior=2, particles=64, horizon=6, seed=7)
add("gw3_table", "gridworld", TABLE, "history", 2048, "reject_tab_hist_kernel", size=3, particles=64, horizon=6, seed=7)
add("sysadmin", "independent-sysadmin", FACT, "dense", 1024, "reject_kernel<plain>", size=3, particles=128, horizon=5, seed=5)
# the composite case: the fully connected filter of the reinvigoration belief gives up too, and its attempts are not in the trace
COMPOSITE = dict(W.case("ftiger_reinvigoration", "episodic-factored-tiger", FACT, "reinvigoration", "dense", E=SLOTS, runs=RUNS,
                        **dict(COMMON, size=2, structure_prior=2, particles=512, horizon=4, seed=5, resample_amount=4)),
                 max_attempts=1024, kernel=["K_REINVIGORATE", "reject_kernel<factored tiger>", "reject_kernel<factored tiger>"])      # (the fully connected filter, then the main one)

# every kernel of fba_kernels.hip that holds a give-up site (the fully connected launch of reject_kernel: COMPOSITE)
GIVE_UP_KERNELS = {"reject_tiger_lds_kernel", "reject_tiger_once_kernel", "reject_kernel<packed factored tiger>", "reject_hist_kernel",
                   "reject_tab_hist_kernel", "reject_kernel<plain>"}


def kernel_names():
    """enum KernelName of fba_launch_plan.h, by value"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fba_pomdp_amd", "csrc", "fba_launch_plan.h")).read()
    body = re.search(r"enum KernelName : uint32_t \{(.*?)\};", src, re.S).group(1)
    names = [n.strip() for n in body.split(",") if n.strip()]
    assert names[0] == "K_SEARCH = 1"
    return {i + 1: n.split("=")[0].strip() for i, n in enumerate(names)}


PLAIN_NAMES = {"K_REJECT_TIGER_LDS": "reject_tiger_lds_kernel", "K_REJECT_TIGER_ONCE": "reject_tiger_once_kernel",
               "K_REJECT_TIGER_ONCE_GATHER": "reject_tiger_once_gather_kernel", "K_REJECT_HIST": "reject_hist_kernel",
               "K_REJECT_TAB_HIST": "reject_tab_hist_kernel"}


def decode_kernel(key, names):
    """a kernel key of fba_launch_plan.h (kernel_key, reject_key) as the name this table uses"""
    name = names[key >> 24]
    if name != "K_REJECT":
        return PLAIN_NAMES.get(name, name)
    a, tiger_table, ftiger = key >> 18 & 63, key >> 12 & 63, key >> 6 & 63      # reject_key: reg | ftp << 1, TIGER_TABLE, FTIGER, BLK / 64
    if ftiger:
        return "reject_kernel<packed factored tiger>" if a & 2 else "reject_kernel<factored tiger>"
    if tiger_table:
        return "reject_kernel<packed tiger>" if tiger_table == 2 else "reject_kernel<tiger>"
    return "reject_kernel<regular Dirichlet>" if a & 1 else "reject_kernel<plain>"


def update_plan(eng):
    """the kernels launch_belief_update launches for this context, in order: update_plan (fba_launch_plan.h) itself, asked through the
    engine's diagnostic export -- not a restatement of its rules"""
    import ctypes as C_
    keys = (C_.c_uint32 * 16)()
    eng.L.fba_debug_update_plan.argtypes = [C_.c_void_p, C_.c_void_p, C_.c_int32]
    n = eng.L.fba_debug_update_plan(eng.h, keys, 16)
    assert 0 < n <= 16
    names = kernel_names()
    return [decode_kernel(int(k), names) for k in keys[:n]]


_ORACLE = {}


def oracle_run(c):
    """the whole experiment on the oracle, once per process: (trace, the simulated steps of every record's search and update)"""
    if c["name"] not in _ORACLE:
        o = W.make_oracle(c, runs=c["runs"])
        _, res = o.run_bapomdp()
        _ORACLE[c["name"]] = (o.trace(res.n_trace), o.trace_steps(res.n_trace))
    return _ORACLE[c["name"]]


RETIRED_FIELDS = ("run", "episode", "t", "reason", "counted", "max_attempts")


def predict(c, tr, steps, max_attempts=None, runs=None):
    """What the engine must report under FBA_GIVEUP_RETIRE with this limit, from the oracle's trace `tr` (ordered by run, episode, t) and
    trace_steps `steps` alone; runs: the runs that were executed to their end (all)."""
    kw = c["kw"]
    limit = c["max_attempts"] if max_attempts is None else max_attempts
    episodes, horizon = kw["episodes"], kw["horizon"]
    discount = orc.make_config(**{k: v for k, v in kw.items() if k == "discount"}).discount
    keep = np.zeros(len(tr), bool)
    gave = np.zeros(len(tr), bool)
    retired = []
    done = set()
    for i in range(len(tr)):
        r = tr[i]
        run = int(r["run"])
        if run in done or (runs is not None and run not in runs):
            continue
        keep[i] = True
        if r["update_count"] > limit:
            gave[i] = True
            done.add(run)
            counted = int(r["t"] == horizon - 1 and not r["terminal"])
            retired.append((run, int(r["episode"]), int(r["t"]), 1, counted, limit))
    ret, ln = W.returns_of_trace(tr[keep], c["runs"], episodes, discount)
    for run, ep, _, _, counted, _ in retired:      # the episode a run was retired in is void unless it had ended; no later one has a record
        if not counted:
            ret[run, ep], ln[run, ep] = 0.0, 0
    stats = (orc.Stat * episodes)()
    for ep in range(episodes):
        for run in range(c["runs"]):
            if ln[run, ep] > 0:
                orc.lib().orc_stat_add(C.byref(stats[ep]), float(ret[run, ep]))
    bins = np.zeros((episodes, horizon), np.uint64)
    for ep, t in zip(tr["episode"][keep].tolist(), tr["t"][keep].tolist()):
        bins[ep, t] += 1
    return dict(retired=retired, keep=keep, gave=gave, returns=ret, lengths=ln, stats=[(s.count, s.mean, s.m2) for s in stats],
                counters=(int(steps[keep, 0].sum()), int(steps[keep & ~gave, 1].sum()), int(keep.sum())), steps=bins)


def mix_conditions(c, p):
    """the case retires some runs and keeps some, in either episode, and some of the retired runs have a successor in their slot"""
    retired = p["retired"]
    assert len(retired) >= 4 and c["runs"] - len(retired) >= 4, (c["name"], len(retired))
    for ep in range(c["kw"]["episodes"]):
        assert any(r[1] == ep for r in retired), (c["name"], ep)
    assert any(r[0] < c["runs"] - c["E"] for r in retired), c["name"]      # (a run below 32: its slot goes on to another)
    return sum(r[4] for r in retired)


def same_records(got, want, skip=()):
    """every field of the trace records but `skip`, bit for bit"""
    assert len(got) == len(want)
    if len(got) == 0:
        return
    for name in got.dtype.names:
        if name in skip:
            continue
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero(~np.all((a == b).reshape(len(got), -1), axis=1))[0]
        assert bad.size == 0, f"{name}: first mismatch at record {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
