"""The cases of tests/test_gpu_belief_resume.py (fba_run_bapomdp_span: a Bayes-adaptive experiment run in spans, resumed from belief
snapshots) and the oracle's side of them, which needs no GPU and is checked by tests/test_belief_resume_cpu.py.

Every case is one row of the FORMATS table of tests/test_gpu_belief_snapshot.py at the smallest shape at which the restore can still go
wrong: 130 particles (two waves and two lanes), 16 simulations, horizon 8, 5 episodes, 3 to 7 slots.  (A weighted block's record part
stands at 8 bytes in the caller's buffer only where the particle count is odd: the GPU tests run one case at 65 particles for that.)

The seeds of the history formats are chosen, on the oracle alone, so that the three splits meet every stride a block can have: a record of
2 + 5 * 8 words is 176 bytes, and a slot stores its records at 64 bytes up to 14 entries, at 128 up to 30 and whole beyond.  An entry is a
belief update, an update follows every step but a terminal one, so a run must make at least 15 updates in episodes [0, 2) and at least 31
of the 32 possible in episodes [0, 4): a gridworld agent that does not find its goal.  The collision-avoidance plane flies one column per
step from column 4 of 5 to column 0 and its last step is terminal, so an episode makes 3 updates at most and a run holds 12 entries
after four episodes, whatever the seed: its records stay at 64 bytes here (asserted as such), and the whole-record restore of that
format is met under FBA_HIST_STRIDE=full instead (STRIDE_FULL_ENV), which stores every record whole."""
import functools

import numpy as np

import wide_launch_cases as W
from test_gpu_belief_snapshot import FORMATS

PARTICLES, SIMS, HORIZON, EPISODES = 130, 16, 8, 5
SPLITS = (1, 2, 4)
RECORD_BYTES = W.record_bytes(EPISODES, HORIZON)       # 176
STRIDE_FULL_ENV = {"FBA_HIST_STRIDE": "full"}

SPLIT_FORMATS = ["dense_tiger", "packed_tiger", "packed_factored_tiger2", "gridworld3_history_importance", "gridworld3_history_rejection",
                 "gridworld3_table_history", "collision_avoidance_5x5x2_history", "point_estimate_tiger"]
GRIDWORLD_HISTORY = ["gridworld3_history_importance", "gridworld3_history_rejection", "gridworld3_table_history"]
HISTORY = GRIDWORLD_HISTORY + ["collision_avoidance_5x5x2_history"]
ORACLE_FORMATS = ["dense_tiger", "gridworld3_history_importance", "gridworld3_history_rejection", "packed_factored_tiger2"]

# slots (= runs) per case: 3 to 7
SLOTS = {"dense_tiger": 3, "packed_tiger": 7, "packed_factored_tiger2": 4, "gridworld3_history_importance": 5, "gridworld3_history_rejection": 6,
         "gridworld3_table_history": 3, "collision_avoidance_5x5x2_history": 4, "point_estimate_tiger": 5}
# (how each was found: test_belief_resume_cpu.py states the property, `python tests/resume_cases.py` prints the first seeds that have it)
SEEDS = {"dense_tiger": 8101, "packed_tiger": 8102, "packed_factored_tiger2": 8103, "gridworld3_history_importance": 8524,
         "gridworld3_history_rejection": 8335, "gridworld3_table_history": 8316, "collision_avoidance_5x5x2_history": 8107,
         "point_estimate_tiger": 8108}


def fmt_of(name):
    return next(f for f in FORMATS if f[0] == name)


def config(name, **over):
    """(domain, model, belief, environment, keywords) of a case, for fba.Engine"""
    _, _, domain, model, belief, env, kw, _ = fmt_of(name)
    kw = dict(kw)
    kw.update(particles=1 if belief == "point_estimate" else PARTICLES, sims=SIMS, horizon=HORIZON, episodes=EPISODES, slots=SLOTS[name],
              seed=SEEDS[name])
    kw.update(over)
    kw.setdefault("runs", kw["slots"])
    return domain, model, belief, dict(env or {}), kw


def make_engine(monkeypatch, fba, name, env=None, **over):
    domain, model, belief, fenv, kw = config(name, **over)
    fenv.update(env or {})
    for k, v in fenv.items():
        monkeypatch.setenv(k, v)
    eng = fba.Engine(domain, model=model, belief=belief, **kw)
    for k in fenv:
        monkeypatch.delenv(k)
    return eng


def make_oracle(name, **over):
    domain, model, belief, _, kw = config(name)
    kw = {k: v for k, v in kw.items() if k != "slots"}
    kw.update(over)
    return W.make_oracle(dict(domain=domain, model=model, belief=belief, kw=kw))


@functools.lru_cache(maxsize=None)
def oracle_whole(name, seed=None):
    """the whole experiment on the oracle: trace, lengths [run][episode] and updates [run][episode] (the steps that were not terminal)"""
    runs = SLOTS[name]
    over = {} if seed is None else {"seed": seed}
    domain, model, belief, _, kw = config(name, **over)
    kw = {k: v for k, v in kw.items() if k != "slots"}
    o = W.make_oracle(dict(domain=domain, model=model, belief=belief, kw=kw))
    _, res = o.run_bapomdp()
    refused = o.L.orc_error(o.h)
    tr = o.trace(res.n_trace)
    ln = np.zeros((runs, EPISODES), np.int64)
    upd = np.zeros((runs, EPISODES), np.int64)
    np.add.at(ln, (tr["run"], tr["episode"]), 1)
    np.add.at(upd, (tr["run"], tr["episode"]), (tr["terminal"] == 0).astype(np.int64))
    return dict(trace=tr, lengths=ln, updates=upd, refused=refused.decode() if refused else None)


def entries_after(name, k, seed=None):
    """per run: the entries a history record holds when episodes [0, k) are over"""
    return oracle_whole(name, seed)["updates"][:, :k].sum(axis=1)


def stride_of(entries):
    return 64 if entries <= 14 else (128 if entries <= 30 else RECORD_BYTES)


def strides_met(name, seed=None):
    return {stride_of(int(n)) for k in SPLITS for n in entries_after(name, k, seed)}


if __name__ == "__main__":     # the seed search, on the CPU
    for name in SPLIT_FORMATS:
        want = {64, 128, RECORD_BYTES} if name in GRIDWORLD_HISTORY else set()
        for seed in range(SEEDS[name], SEEDS[name] + 4000, 10):
            ref = oracle_whole(name, seed)
            if ref["refused"] is None and (not want or strides_met(name, seed) >= want):
                print(name, seed, [entries_after(name, k, seed).tolist() for k in SPLITS])
                break
        else:
            print(name, "no seed found")
