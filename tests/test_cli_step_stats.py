"""fba_experiment ... --step-stats-file: one line per (episode, t) at which a step was taken, as Engine.step_stats() holds the bins."""
import math
import subprocess

import numpy as np
import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N
from step_stats_size_cases import WINDOW_SHAPES, Ref as _Ref, fit

pytestmark = pytest.mark.gpu

INT_COLS = ["nodes_sum", "depth_sum", "attempts_steps", "attempts_sum", "probed", "evidence_zero"]
PROBE_COLS = ["evidence_sum", "log_evidence_sum", "log_evidence_sq_sum", "next_true_sum", "post_ratio_sum"]


@pytest.fixture(scope="module")
def cli():
    return fba.build_cli()


def _seed(text):
    h = 1469598103934665603
    for ch in text.encode():
        h = ((h ^ ch) * 1099511628211) % 2 ** 64
    return h


def _rows(path, A):
    text = path.read_text().splitlines()
    assert text[0].startswith("# episode t steps terminals action_0 ")
    names = text[0][2:].split()
    assert names == ["episode", "t", "steps", "terminals"] + [f"action_{a}" for a in range(A)] + ["reward_sum", "reward_sq_sum", "value_sum"] + INT_COLS + PROBE_COLS
    rows = [l.split() for l in text[1:]]
    assert all(not l[0].startswith("#") and len(l) == len(names) for l in rows)
    return [dict(zip(names, l)) for l in rows]


def _compare(rows, st, A, probe, ref):
    bins = [(e, t) for e in range(st.shape[0]) for t in range(st.shape[1]) if st["steps"][e, t] > 0]
    assert [(int(r["episode"]), int(r["t"])) for r in rows] == bins and bins      # one row per non-empty bin, in order
    for r in rows:
        b = st[int(r["episode"]), int(r["t"])]
        assert int(r["steps"]) == b["steps"] and int(r["terminals"]) == b["terminals"]
        assert [int(r[f"action_{a}"]) for a in range(A)] == b["action"][:A].tolist()
        for f in INT_COLS:
            assert int(r[f]) == b[f], f
        assert float(r["reward_sum"]) == b["reward_sum"] and float(r["reward_sq_sum"]) == b["reward_sq_sum"]
        x = ref.terms["value_sum"][int(r["episode"])][int(r["t"])]      # (%.17g round-trips a double; the bound of include/fba_hip.h)
        assert abs(float(r["value_sum"]) - math.fsum(x)) <= len(x) * 2.0 ** -52 * math.fsum(abs(v) for v in x)
        if not probe:
            assert all(float(r[f]) == 0.0 for f in PROBE_COLS)


def test_the_rows_are_the_bins(cli, tmp_path):
    out, stats, probe = tmp_path / "ba.res", tmp_path / "stats.txt", tmp_path / "probe.txt"
    args = [cli, "bapomdp", "-D", "episodic-tiger", "-s", "32", "--particle-amount", "64", "--runs", "6", "--episodes", "3", "-H", "6", "--seed", "steps",
            "-f", str(out), "--step-stats-file", str(stats)]
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    eng = fba.Engine("episodic-tiger", model=N.MODEL_BA_TABLE, sims=32, particles=64, runs=6, episodes=3, horizon=6, seed=_seed("steps"), trace=1)
    eng.step_stats_enable()
    eng.run_bapomdp()
    st = eng.step_stats()
    rows = _rows(stats, eng.A)
    _compare(rows, st, eng.A, False, _Ref(eng, eng.trace()))
    assert sum(int(r["steps"]) for r in rows) == eng.counters().env_steps
    # with --probe-file as well the probe feeds the bins
    r = subprocess.run(args + ["--probe-file", str(probe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    eng.probe_enable()
    eng.step_stats_enable()
    eng.run_bapomdp()
    st = eng.step_stats()
    rows = _rows(stats, eng.A)
    _compare(rows, st, eng.A, True, _Ref(eng, eng.trace()))
    lines = [l for l in probe.read_text().splitlines() if l and not l.startswith("#")]
    assert sum(int(r["probed"]) for r in rows) == len(lines) == int(st["probed"].sum()) > 0
    for r in rows:      # one slot per run and one workgroup per slot: the probe's values repeat, and each bin is one wave's fixed tree
        b = st[int(r["episode"]), int(r["t"])]
        for f in PROBE_COLS:
            assert np.isclose(float(r[f]), b[f], rtol=1e-12, atol=0.0), f
    eng.close()


def test_planning_and_fbapomdp_are_accepted(cli, tmp_path):
    out, stats = tmp_path / "p.res", tmp_path / "stats.txt"
    r = subprocess.run([cli, "planning", "-D", "episodic-tiger", "-s", "32", "--particle-amount", "64", "--runs", "5", "-H", "6", "--seed", "plan", "-f", str(out),
                        "--step-stats-file", str(stats)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    eng = fba.Engine("episodic-tiger", model=N.MODEL_POMDP, sims=32, particles=64, runs=5, horizon=6, seed=_seed("plan"), trace=1)
    eng.step_stats_enable()
    eng.run_planning()
    _compare(_rows(stats, eng.A), eng.step_stats(), eng.A, False, _Ref(eng, eng.trace()))
    eng.close()
    r = subprocess.run([cli, "fbapomdp", "-D", "episodic-factored-tiger", "--size", "2", "-s", "16", "--particle-amount", "32", "--runs", "4", "--episodes", "2",
                        "-H", "4", "--seed", "fact", "-f", str(out), "--step-stats-file", str(stats)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = stats.read_text().splitlines()
    assert len(text) > 1 and sum(int(l.split()[2]) for l in text[1:] if int(l.split()[1]) == 0) == 4 * 2


def test_more_bins_than_one_window(cli, tmp_path):
    """the continuous tiger never ends an episode: every one of the episodes x horizon bins has a row, and they are more than a workgroup's
    LDS table holds (step_stats_size_cases.fit)"""
    e, h = WINDOW_SHAPES[1]
    assert fit(3) < e * h <= 2 * fit(3)
    out, stats = tmp_path / "ba.res", tmp_path / "stats.txt"
    r = subprocess.run([cli, "bapomdp", "-D", "continuous-tiger", "-s", "4", "--particle-amount", "8", "--runs", "5", "--episodes", str(e), "-H", str(h),
                        "--seed", "windows", "-f", str(out), "--step-stats-file", str(stats)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    eng = fba.Engine("continuous-tiger", model=N.MODEL_BA_TABLE, sims=4, particles=8, runs=5, episodes=e, horizon=h, seed=_seed("windows"), trace=1)
    eng.step_stats_enable()
    eng.run_bapomdp()
    st = eng.step_stats()
    rows = _rows(stats, eng.A)
    assert len(rows) == e * h == st.size and np.all(st["steps"] == 5)
    _compare(rows, st, eng.A, False, _Ref(eng, eng.trace()))
    eng.close()
