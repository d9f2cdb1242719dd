"""search_kernel's root step inside the boundary phase (episodic-tiger instantiations): a waiting lane starts the next simulation's stream
and, from a compact filter, requests its 16-byte record BEFORE the back-up of the finished simulation, then selects at the root from the
registers, steps and resolves the child -- the generic step phase only ever sees nodes below the root.  Same draws, same arithmetic: every
case must give the oracle's experiment on the same Philox streams, every trace field, statistic, counter, return and length, bit for bit.

The cases are the smallest shapes at which that code can go wrong and tests/test_gpu_search_quorum.py does not reach.  70 slots (one full
wave and a wave of six live lanes), 64 particles, and 3 episodes where a model is learnt (searches from lazily reset filters):
  * horizon 1          depth left is 1 everywhere: every simulator step is the boundary phase's; the step phase only ends the simulations
                       that found the node below the root already there (no depth left, no step);
  * horizon 2          slots at t = 1 never leave the boundary phase while their wave neighbours at t = 0 do; the node below the root is
                       created by the root block and its rollout has length 0;
  * two_simulations    the first boundary has nothing to back up, the last a back-up and no next simulation (nothing may be drawn or
                       loaded for simulation `sims`);
  * horizon 10         256 simulations: levels 2, 3 and deeper, with the root no longer in the step phase;
  * compact / full     3584 particles (from where the rejection update leaves 16-byte records behind), 70 runs: a wave whose slots turn
                       compact after the first update (the early load), and under FBA_NO_COMPACT=1 the same wave on full records (the
                       fetch behind the back-up); lazily reset slots in both.  One oracle run serves the two;
  * factored tiger 1, 2 and dense tabular tiger: the instantiations the quorum file does not run;
  * quarter_masked     52 runs in 70 slots: inactive lanes, and a wave whose first lane is live.
Quorums 1 (a boundary on every trip, stragglers mid-tree) and 64 (lanes that finished at the root wait for the deepest) run the horizon 1,
horizon 2 and 3584-particle cases again.  FBA_SEARCH_QUORUM, FBA_NO_COMPACT and FBA_DENSE_PARTICLES are read when a context is created:
each environment runs its cases in one fresh child process, which hands the results back in one file; the oracle's side of a case is
computed once."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import wide_launch_cases as W  # noqa: E402
from wide_launch_cases import FACT, POMDP, REJ, TABLE  # noqa: E402

pytestmark = pytest.mark.gpu

SLOTS = 70
SHAPE = dict(sims=64, particles=64, horizon=4)
NO_COMPACT_ENV = {"FBA_NO_COMPACT": "1"}
SWITCHES = ("FBA_SEARCH_QUORUM", "FBA_NO_ETIGER", "FBA_NO_COMPACT", "FBA_DENSE_PARTICLES")


def _case(name, domain, model, fmt, env=None, runs=2 * SLOTS + 37, **kw):
    kw = dict(SHAPE, **kw)
    if model != POMDP:
        kw.setdefault("episodes", 3)
    return W.case(name, domain, model, REJ, fmt, E=SLOTS, runs=runs, env=env, **kw)


CASES = [
    _case("horizon1_packed_tabular_tiger", "episodic-tiger", TABLE, "packed_tiger", seed=2201, horizon=1),
    _case("horizon1_tiger_pomdp", "episodic-tiger", POMDP, "dense", seed=2202, horizon=1),
    _case("horizon2_packed_tabular_tiger", "episodic-tiger", TABLE, "packed_tiger", seed=2203, horizon=2),
    _case("horizon2_tiger_pomdp", "episodic-tiger", POMDP, "dense", seed=2204, horizon=2),
    _case("two_simulations", "episodic-tiger", TABLE, "packed_tiger", seed=2205, sims=2),
    _case("horizon10_256_simulations", "episodic-tiger", TABLE, "packed_tiger", seed=2206, horizon=10, sims=256),
    _case("compact_filters", "episodic-tiger", TABLE, "packed_tiger", runs=SLOTS, seed=2207, particles=3584),
    _case("full_records_3584", "episodic-tiger", TABLE, "packed_tiger", env=NO_COMPACT_ENV, runs=SLOTS, seed=2207, particles=3584),
    _case("packed_factored_tiger1", "episodic-factored-tiger", FACT, "packed_ftiger", size=1, structure_prior=2, seed=2208),
    _case("packed_factored_tiger2", "episodic-factored-tiger", FACT, "packed_ftiger", size=2, structure_prior=2, seed=2209),
    _case("dense_tabular_tiger", "episodic-tiger", TABLE, "dense", env=W.DENSE_ENV, seed=2210),
    _case("quarter_masked", "episodic-tiger", TABLE, "packed_tiger", runs=52, seed=2211),
]
BY_NAME = {c["name"]: c for c in CASES}
ORACLE_OF = {"full_records_3584": "compact_filters"}   # the same experiment: the switch changes how the engine stores it, not what it is
EVERY_QUORUM = ("horizon1_packed_tabular_tiger", "horizon1_tiger_pomdp", "horizon2_packed_tabular_tiger", "horizon2_tiger_pomdp",
                "compact_filters", "full_records_3584")
PAIRS = [("default", c["name"]) for c in CASES] + [(q, n) for q in ("1", "64") for n in EVERY_QUORUM]
FIELDS = ("trace", "stats", "counters", "returns", "lengths")


def _env_key(name):
    return ",".join(f"{k}={v}" for k, v in sorted(BY_NAME[name]["env"].items()))


def _child(quorum, names, out):
    """(in the child process) the named cases, which share one environment, under the quorum the parent put there"""
    import fba_pomdp_amd as fba

    assert os.environ.get("FBA_SEARCH_QUORUM", "default") == quorum
    res = {}
    for name in names:
        c = BY_NAME[name]
        assert all(os.environ.get(k) == v for k, v in c["env"].items())
        got = W.engine_side(c, fba)
        res.update({name + "." + k: np.asarray(got[k]) for k in FIELDS})
    np.savez(out, **res)


@functools.lru_cache(maxsize=None)
def _engine_results(quorum, env_key, tmp):
    names = [n for q, n in PAIRS if q == quorum and _env_key(n) == env_key]
    out = os.path.join(tmp, f"root_phase_{quorum}_{env_key.replace('=', '-') or 'plain'}.npz")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(BY_NAME[names[0]]["env"])
    if quorum != "default":
        env["FBA_SEARCH_QUORUM"] = quorum
    p = subprocess.run([sys.executable, os.path.abspath(__file__), quorum, ",".join(names), out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (quorum, env_key, p.returncode, p.stderr[-2000:])
    return np.load(out)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    ref = W.oracle_side(BY_NAME[name])
    for k in ("trace", "returns", "lengths"):
        ref[k].setflags(write=False)
    return ref


def min_tree_depths(c):
    """How many distinct tree depths an experiment must show.  Three, as the quorum file asks -- except where the depth cannot vary that
    much: a horizon of 1 or 2 (not asserted), and two simulations, the second of which takes an action the first has not tried and so
    never enters a node below the root (one depth)."""
    if c["kw"]["horizon"] <= 2:
        return 0
    return 1 if c["kw"]["sims"] == 2 else 3


def check_oracle_side(name, ref):
    c = BY_NAME[name]
    if name == "quarter_masked":
        assert c["runs"] < SLOTS and 4 * (SLOTS - c["runs"]) >= SLOTS
    elif c["kw"]["particles"] == SHAPE["particles"]:
        # slots of one wave sit at different t, so their trees have different depths left (a horizon of h allows h lengths)
        assert len(set(ref["lengths"].reshape(-1).tolist())) >= min(W.min_distinct_lengths(c), c["kw"]["horizon"])
        assert len(set(ref["trace"]["tree_depth"].tolist())) >= min_tree_depths(c)


@pytest.fixture(scope="module")
def results_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("search_root_phase"))


@pytest.mark.parametrize("quorum,name", PAIRS)
def test_root_phase_runs_the_oracles_experiment(quorum, name, results_dir):
    c = BY_NAME[name]
    ref = _oracle(ORACLE_OF.get(name, name))
    check_oracle_side(name, ref)
    z = _engine_results(quorum, _env_key(name), results_dir)
    got = {k: z[name + "." + k] for k in FIELDS}
    got["stats"] = [tuple(s) for s in got["stats"].tolist()]
    got["counters"] = tuple(got["counters"].tolist())
    W.assert_same_experiment(c, got, ref)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2].split(","), sys.argv[3])
