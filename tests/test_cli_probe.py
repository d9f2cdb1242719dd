"""fba_experiment ... --probe-file: one line per real step that a belief update follows, as Engine.probe() records them."""
import subprocess

import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    return fba.build_cli()


def _lines(path):
    return [l.split() for l in path.read_text().splitlines() if l and not l.startswith("#")]


def test_probe_file_has_one_line_per_updated_step(cli, tmp_path):
    out, probe = tmp_path / "ba.res", tmp_path / "probe.txt"
    r = subprocess.run([cli, "bapomdp", "-D", "episodic-tiger", "-s", "32", "--particle-amount", "64", "--runs", "6", "--episodes", "3",
                        "-H", "6", "--seed", "probe", "-f", str(out), "--probe-file", str(probe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = _lines(probe)
    assert all(len(l) == 9 for l in rows)
    h = 1469598103934665603
    for ch in b"probe":
        h = ((h ^ ch) * 1099511628211) % 2 ** 64
    eng = fba.Engine("episodic-tiger", model=N.MODEL_BA_TABLE, sims=32, particles=64, runs=6, episodes=3, horizon=6, seed=h, trace=1)
    eng.run_bapomdp()
    tr = eng.trace()
    steps = [r for r in tr if not r["terminal"]]
    assert 0 < len(steps) < len(tr)                     # some steps opened a door
    assert len(rows) == len(steps)
    for l, st in zip(rows, steps):                      # both by (run, episode, t)
        assert [int(x) for x in l[:6]] == [st["run"], st["episode"], st["t"], st["action"], st["obs"], st["state"]]
        ev, nt, pt = (float(x) for x in l[6:])
        assert 0.0 < ev <= 1.0 and 0.0 <= pt <= nt <= 1.0
    assert not any(l.startswith("# ") and "kept" in l for l in probe.read_text().splitlines())
    eng.close()
    # a range of slots
    r = subprocess.run([cli, "bapomdp", "-D", "episodic-tiger", "-s", "32", "--particle-amount", "64", "--runs", "6", "--episodes", "3",
                        "-H", "6", "--seed", "probe", "-f", str(out), "--probe-file", str(probe), "--probe-slots", "2:3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    part = _lines(probe)
    assert part == [l for l in rows if int(l[0]) in (2, 3, 4)]
    r = subprocess.run([cli, "planning", "-D", "episodic-tiger", "--probe-file", str(probe)], capture_output=True, text=True)
    assert r.returncode == 1 and "Bayes-adaptive" in r.stderr
