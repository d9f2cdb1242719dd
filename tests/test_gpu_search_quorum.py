"""search_kernel under every boundary quorum (fba_launch_plan.h: the share of a wave's live trees that waits at a simulation boundary
before the wave runs the back-up and the next root sample): WHEN a lane runs its simulation i is invisible to it -- the lanes are
independent trees and every draw comes from the counter-based stream of (run, episode, t, phase, simulation) -- so each quorum must give
the oracle's experiment on the same Philox streams, every trace field, statistic, counter, return and length, bit for bit.

FBA_SEARCH_QUORUM is read when a context is created; each value (1: a boundary as soon as one lane waits; 2; 33: just over half; 64:
all lanes together) and the launch plan's default (variable unset) runs in a fresh child process of its own, which runs every case and
hands its results back in one file.  The oracle's side of a case is computed once and shared by the five.

Every case runs in 70 slots (one full wave and a wave of six live lanes), 64 simulations of 64 particles, horizon 4 -- in a slot that is
past the first step of an episode the trees are shallower than in its neighbours, and a wave's lanes stop needing boundaries at
different trips -- and, where the model is learnt, 3 episodes, so that searches start from lazily reset filters.  runs = 2 * 70 + 37: the
slots are used again and the last round leaves 33 of them inactive.  Beside the five kernels:
  * quarter_masked      52 runs in 70 slots: 18 slots never have work, 12 of them the last lanes of the full wave (52-63), the others the
                        whole second wave (the first lane of the full wave is live in every case);
  * one_simulation      sims = 1: every live lane is at a boundary on every trip;
  * compact_filters     3584 particles (TIGER_ONCE_MIN_N, from where the rejection update leaves 16-byte records behind): the search's
                        one-load root sample from a compact filter.  70 runs: the oracle pays for the particles."""
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
QUORUMS = ("1", "2", "33", "64", "default")
SHAPE = dict(sims=64, particles=64, horizon=4)


def _case(name, domain, model, fmt, env=None, runs=2 * SLOTS + 37, **kw):
    kw = dict(SHAPE, **kw)
    if model != POMDP:
        kw.setdefault("episodes", 3)
    return W.case(name, domain, model, REJ, fmt, E=SLOTS, runs=runs, env=env, **kw)


CASES = [
    # the four episodic-tiger kinds (ETIGER) ...
    _case("packed_tabular_tiger", "episodic-tiger", TABLE, "packed_tiger", seed=2101),
    _case("tiger_pomdp", "episodic-tiger", POMDP, "dense", seed=2102),
    _case("dense_tabular_tiger", "episodic-tiger", TABLE, "dense", env=W.DENSE_ENV, seed=2103),
    _case("packed_factored_tiger3", "episodic-factored-tiger", FACT, "packed_ftiger", size=3, structure_prior=2, seed=2104),
    # ... and the general tree layout: the tabular BA-POMDP over continuous tiger, whose episodes all last the horizon
    _case("continuous_tiger", "continuous-tiger", TABLE, "packed_tiger", seed=2105),
    _case("quarter_masked", "episodic-tiger", TABLE, "packed_tiger", runs=52, seed=2106),
    _case("one_simulation", "episodic-tiger", TABLE, "packed_tiger", seed=2107, sims=1),
    _case("compact_filters", "episodic-tiger", TABLE, "packed_tiger", runs=SLOTS, seed=2108, particles=3584),
]
BY_NAME = {c["name"]: c for c in CASES}
FIELDS = ("trace", "stats", "counters", "returns", "lengths")


def _child(quorum, out):
    """(in the child process) every case under the quorum the parent put into the environment"""
    import fba_pomdp_amd as fba

    assert os.environ.get("FBA_SEARCH_QUORUM", "default") == quorum
    res = {}
    for c in CASES:
        for k in W.DENSE_ENV:
            os.environ.pop(k, None)
        os.environ.update(c["env"])
        got = W.engine_side(c, fba)
        res.update({c["name"] + "." + k: np.asarray(got[k]) for k in FIELDS})
    np.savez(out, **res)


@functools.lru_cache(maxsize=None)
def _engine_results(quorum, tmp):
    out = os.path.join(tmp, f"quorum_{quorum}.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("FBA_SEARCH_QUORUM", "FBA_NO_ETIGER", "FBA_NO_COMPACT")}
    if quorum != "default":
        env["FBA_SEARCH_QUORUM"] = quorum
    p = subprocess.run([sys.executable, os.path.abspath(__file__), quorum, out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (quorum, p.returncode, p.stderr[-2000:])
    return np.load(out)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    ref = W.oracle_side(BY_NAME[name])
    for k in ("trace", "returns", "lengths"):
        ref[k].setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def results_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("search_quorum"))


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
@pytest.mark.parametrize("quorum", QUORUMS)
def test_every_quorum_runs_the_oracles_experiment(quorum, name, results_dir):
    c = BY_NAME[name]
    ref = _oracle(name)
    if name == "quarter_masked":
        assert c["runs"] < SLOTS and 4 * (SLOTS - c["runs"]) >= SLOTS
    elif name != "compact_filters":
        # slots of one wave sit at different t, so their trees have different depths left
        assert len(set(ref["lengths"].reshape(-1).tolist())) >= W.min_distinct_lengths(c)
        assert len(set(ref["trace"]["tree_depth"].tolist())) >= (1 if name == "one_simulation" else 3)
    z = _engine_results(quorum, results_dir)
    got = {k: z[name + "." + k] for k in FIELDS}
    got["stats"] = [tuple(s) for s in got["stats"].tolist()]
    got["counters"] = tuple(got["counters"].tolist())
    W.assert_same_experiment(c, got, ref)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
