"""bench.py's result line and --dump-outputs: a plain run prints the headline figures without the CPU baseline (that is --full's),
and the arrays it dumps are what the last timed step computed, identical from run to run with the same arguments."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeEngine:
    """Records shaped like a bench run's: only the fields the timed path writes with tracing off are filled."""
    def __init__(self, slots):
        self.slots = slots

    def last_step_info(self):
        from fba_pomdp_amd import _native as N
        rec = np.zeros(self.slots, N.TRACE_DTYPE)
        rec["n_nodes"] = 3 + np.arange(self.slots) % 50
        rec["tree_depth"] = 1 + np.arange(self.slots) % 7
        rec["update_count"] = 4000 + np.arange(self.slots) % 900
        rec["root_n"][:, :3] = [1000, 2000, 1096]
        rec["root_q"] = np.arange(self.slots)[:, None] * 0.25 + np.arange(N.MAX_ACTIONS)
        rec["weight_total"] = 0.5 + np.arange(self.slots)
        return rec


TRACE_ONLY = ("run", "episode", "t", "action", "state", "obs", "terminal", "reward", "belief_hash", "belief_hash_hi", "belief_hash_lo")


@pytest.mark.parametrize("slots,belief", [(4, "rejection_sampling"), (262144, "rejection_sampling"), (4, "importance_sampling")])
def test_dump_outputs_writes_float64_arrays_of_a_fixed_sample(tmp_path, slots, belief):
    import bench
    c0 = types.SimpleNamespace(sim_steps=10, belief_steps=20, env_steps=3)
    c1 = types.SimpleNamespace(sim_steps=110, belief_steps=220, env_steps=33)
    eng = _FakeEngine(slots)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), eng, c0, c1, np.array([5.0, -1.5, 9.25]), belief)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    fields = set(bench.DUMP_FIELDS) | ({"weight_total"} if belief == "importance_sampling" else set())
    assert set(names) == {"slot_index.npy", "return_sums.npy", "timed_counters.npy"} | {f"last_step_{f}.npy" for f in fields}
    assert not any(f"last_step_{f}.npy" in names for f in TRACE_ONLY)     # a bench run never writes them: they would be zeros
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    load = lambda d, n: np.load(tmp_path / d / (n + ".npy"))
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and np.array_equal(a, b), n
    idx = load("a", "slot_index").astype(np.int64)
    assert len(idx) == min(slots, bench.DUMP_SLOTS) and np.all(np.diff(idx) > 0)
    rec = eng.last_step_info()[idx]
    for f in fields:
        assert np.array_equal(load("a", "last_step_" + f), rec[f]), f
    assert load("a", "timed_counters").tolist() == [100.0, 200.0, 30.0]
    assert load("a", "return_sums").tolist() == [5.0, -1.5, 9.25]


def test_bench_refuses_zero_timed_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_bench_line_and_repeatable_dumps(tmp_path):
    """Two plain runs of a small c2 shape (lock-step ticks: every slot makes one real step per tick) and one with the importance filter:
    the line carries the headline keys and no CPU baseline, the dumps hold what the last step computed, and the two c2 dumps are equal."""
    slots, sims, steps = 256, 128, 3

    def run(d, *extra):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--slots", str(slots),
               "--sims", str(sims), "--particles", "128", "--dump-outputs", str(tmp_path / d)] + list(extra)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0 and "cpu_baseline" not in line
        load = lambda n: np.load(tmp_path / d / (n + ".npy"))
        assert load("slot_index").tolist() == list(range(slots))
        assert np.all(load("last_step_root_n").sum(axis=1) == sims)          # every simulation of the last search visited the root once
        assert np.all(load("last_step_n_nodes") >= 1) and np.all(load("last_step_tree_depth") >= 1)
        sim, belief, env = load("timed_counters")
        assert env == steps * slots and sim >= steps * slots * sims and belief > 0
        return load

    run("a")
    run("b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)), n
    load = run("is", "--belief", "importance_sampling")
    assert np.any(load("last_step_weight_total") > 0)
