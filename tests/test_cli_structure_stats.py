"""fba_experiment ... --structure-stats-file / --structure-stats-query: one line per (episode, t) at which a step was taken, as
Engine.structure_stats() holds the bins.  The usage text and the refusals that need no device run without one."""
import subprocess

import numpy as np
import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N


@pytest.fixture(scope="module")
def cli():
    fba.build()
    return fba.build_cli()


def _seed(text):
    h = 1469598103934665603
    for ch in text.encode():
        h = ((h ^ ch) * 1099511628211) % 2 ** 64
    return h


def test_the_usage_names_the_flags(cli):
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    text = r.stdout + r.stderr
    assert "--structure-stats-file FILE" in text and "(fba_structure_stats)" in text
    assert "--structure-stats-query W0:W1:..." in text and "at most 16" in text
    assert "episode t steps weightless overflowed collapsed distinct_sum distinct_max" in text


@pytest.mark.parametrize("mode,domain", [("planning", "episodic-tiger"), ("bapomdp", "episodic-tiger")])
def test_planning_and_bapomdp_are_refused(cli, tmp_path, mode, domain):
    r = subprocess.run([cli, mode, "-D", domain, "-f", str(tmp_path / "x.res"), "--structure-stats-file", str(tmp_path / "s.txt")], capture_output=True, text=True)
    assert r.returncode == 1 and "--structure-stats-file needs a factored Bayes-adaptive experiment (fbapomdp)" in r.stderr
    assert not (tmp_path / "s.txt").exists()


def test_query_lists_are_refused(cli, tmp_path):
    base = [cli, "fbapomdp", "-D", "episodic-factored-tiger", "--size", "2", "-f", str(tmp_path / "x.res")]
    many = [a for k in range(17) for a in ("--structure-stats-query", "%x" % (k % 4))]
    r = subprocess.run(base + ["--structure-stats-file", str(tmp_path / "s.txt")] + many, capture_output=True, text=True)
    assert r.returncode == 1 and "--structure-stats-query: 17 graphs where at most 16 are followed" in r.stderr
    for bad in ("3:g", "3::7", ":3", "3:", "0x3", ""):
        r = subprocess.run(base + ["--structure-stats-file", str(tmp_path / "s.txt"), "--structure-stats-query=" + bad], capture_output=True, text=True)
        assert r.returncode == 1 and f"the argument ('{bad}') for option '--structure-stats-query' is invalid" in r.stderr, bad
    r = subprocess.run(base + ["--structure-stats-query", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "--structure-stats-query names a graph for --structure-stats-file, which is not given" in r.stderr
    assert not (tmp_path / "s.txt").exists()


@pytest.mark.gpu
def test_the_rows_are_the_bins(cli, tmp_path):
    out, stats = tmp_path / "f.res", tmp_path / "stats.txt"
    args = dict(size=2, structure_prior=2, sims=16, particles=32, runs=5, slots=2, episodes=2, horizon=4)
    eng = fba.Engine("episodic-factored-tiger", model=N.MODEL_BA_FACTORED, seed=_seed("graphs"), **args)
    nw, ns = eng.structure_lens()
    assert nw >= 1
    Q = np.zeros((2, nw), np.uint32)
    Q[1, :] = ns - 1
    flags = [a for row in Q for a in ("--structure-stats-query", ":".join("%x" % w for w in row))]
    base = [cli, "fbapomdp", "-D", "episodic-factored-tiger", "--size", "2", "--structure-prior", "match-uniform", "-s", "16", "--particle-amount", "32",
            "--runs", "5", "--slots", "2", "--episodes", "2", "-H", "4", "--seed", "graphs", "-f", str(out)]
    r = subprocess.run(base + ["--structure-stats-file", str(stats)] + flags, capture_output=True, text=True)      # (more runs than slots: no condition)
    assert r.returncode == 0, r.stderr
    eng.structure_stats_enable(Q)
    eng.run_bapomdp()
    st = eng.structure_stats()
    text = stats.read_text().splitlines()
    names = text[0][2:].split()
    assert names == ["episode", "t", "steps", "weightless", "overflowed", "collapsed", "distinct_sum", "distinct_max"] + \
        [f"{k}_{q}" for q in range(2) for k in ("frac", "held", "sole")] + [f"set_frac_{m}[{ns}]" for m in range(nw)]
    rows = [dict(zip(names, l.split())) for l in text[1:]]
    assert all(len(l.split()) == len(names) for l in text[1:])
    bins = [(e, t) for e in range(2) for t in range(4) if st.head["steps"][e, t] > 0]
    assert [(int(r["episode"]), int(r["t"])) for r in rows] == bins and bins      # one row per non-empty bin, in order
    assert sum(int(r["steps"]) for r in rows) == eng.counters().env_steps and int(st.head["steps"][0, 0]) == 5
    for r in rows:
        e, t = int(r["episode"]), int(r["t"])
        for f in ("steps", "weightless", "overflowed", "collapsed", "distinct_sum", "distinct_max"):
            assert int(r[f]) == st.head[f][e, t], f
        for q in range(2):
            assert int(r[f"held_{q}"]) == st.query_held[e, t, q] and int(r[f"sole_{q}"]) == st.query_sole[e, t, q]
            assert float(r[f"frac_{q}"]) == st.query_frac[e, t, q]      # a flat filter of 32 particles: every term is k / 32, %.17g round-trips
        for m in range(nw):
            assert [float(x) for x in r[f"set_frac_{m}[{ns}]"].split(",")] == st.set_frac[e, t, m].tolist()
    # a word list of another length than the model's, and a word beyond the node's candidates
    r = subprocess.run(base + ["--structure-stats-file", str(stats), "--structure-stats-query", ":".join(["1"] * (nw + 1))], capture_output=True, text=True)
    assert r.returncode == 1 and f"{nw + 1} words where the model's particles carry {nw}" in r.stderr
    r = subprocess.run(base + ["--structure-stats-file", str(stats), "--structure-stats-query", ":".join(["ffff"] * nw)], capture_output=True, text=True)
    assert r.returncode == 1 and "fba_structure_stats_enable: query 0, word 0: 0xffff names a parent beyond the node's candidates" in r.stderr
    eng.close()
