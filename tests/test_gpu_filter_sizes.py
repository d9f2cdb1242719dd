"""Engine == oracle on both sides of every particle count at which the belief filter changes.  The engine chooses a kernel, a branch of a
kernel or a record format from `particles` alone (tests/filter_size_cases.py: the table of switch-overs), and every other oracle comparison
of the suite runs a few hundred particles: a `<` for a `<=` at one of these switches, a 16-bit source index one too narrow, the dropped last
element of a ragged chunk or a carry lost between two tiles would pass them all.  Here a small whole experiment runs at N = c and N = c + 1
of every switch, with at least three belief updates in a row in some slot (the buffer flip; a resampled filter feeding the next update), and
every trace field -- weight_total, update_count and belief_hash after every update among them --, statistic, counter and per-run return
must be the oracle's, bit for bit.  particle_bytes is compared with the format's formula, which says which record format fba_create chose
at that N.  The two tests without a GPU keep the table honest: the thresholds are read out of the sources, so a moved threshold fails the
table instead of leaving it beside the switch."""
import os
import re

import pytest

import filter_size_cases as F
import fba_pomdp_amd as fba
import wide_launch_cases as W

CSRC = os.path.join(os.path.dirname(os.path.abspath(fba.__file__)), "csrc")
MIN_STREAK = 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in F.CASES])
def test_filter_size_equals_the_oracle(name, monkeypatch):
    c = F.BY_NAME[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    ref = W.oracle_side(c)
    streak = F.longest_update_streak(ref["trace"])
    print(f"{name}: {len(ref['trace'])} records, {int((ref['trace']['terminal'] == 0).sum())} updates, {streak} in a row")
    assert streak >= MIN_STREAK
    W.assert_same_experiment(c, W.engine_side(c, fba), ref)   # (engine_side: slots, and particle_bytes against the format's formula)


def _constants():
    """the thresholds as the sources state them"""
    with open(os.path.join(CSRC, "fba_kernels.h")) as f:
        header = f.read()
    with open(os.path.join(CSRC, "fba_kernels.hip")) as f:
        kernels = f.read()
    with open(os.path.join(CSRC, "fba_launch_plan.h")) as f:
        plan = f.read()
    k = {}
    for name in ("IS_LDS_MAX_N", "IS_MAX_CHUNKS", "TIGER_LDS_MAX_N", "PARTICLE_TILE", "CARRY_TILE", "REJECT_BLOCK"):
        (v,) = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, header)
        k[name] = int(v)
    (v,) = re.findall(r"bool\s+hist_all_draws_first\s*\(\s*int\s+N\s*\)\s*\{\s*return\s+N\s*<=\s*(\d+)\s*;", plan)
    k["hist_all_draws_first"] = int(v)
    (v,) = re.findall(r"bool\s+hist_update_multi\s*\([^)]*\)\s*\{[^}]*return\s+P\.N\s*>=\s*(\d+)\s*;", plan)
    k["hist_update_multi"] = int(v) - 1          # (N >= v takes the seven launches: the last one-launch filter is the c of this switch)
    # the packed tiger rejection filter's block, both kernels: the instantiation launched (launch_step) and the block update_plan gives it
    (v,) = set(re.findall(r"reject_tiger_lds_kernel<(\d+)>", kernels))
    assert re.search(r"kernel_key\(K_REJECT_TIGER_LDS\), %s," % v, plan)
    assert re.search(r"reject_key\(false, 2, 0, %s\), %s," % (v, v), plan) and re.search(r"FBA_REJECT\(false, 2, 0, %s\)" % v, kernels)
    k["REJECT_512"] = int(v)
    return k


def test_filter_size_cases_straddle_every_switch_over():
    """every family of cases holds N = c and N = c + 1 of every switch-over that its kernels have, c as the sources state it today"""
    k = _constants()
    assert k["IS_LDS_MAX_N"] < k["IS_MAX_CHUNKS"] * 256 < k["CARRY_TILE"] * 256      # (what the table's comments say of the paths)
    for family, switches in F.SWITCHES.items():
        counts = F.counts_of(family)
        for sw in switches:
            if sw == "power_of_two":        # the root sample of the history search: both kinds of N, next to each other, twice
                pairs = [n for n in counts if n & (n - 1) == 0 and n + 1 in counts]
                assert len(pairs) >= 2, (family, counts)
            elif sw == "ragged_chunks":     # the seven launches: 4 elements per lane, 256 per chunk, 4 chunks per workgroup
                chunks = [(n + 255) // 256 for n in counts]
                assert any(n % 4 for n in counts) and any(n % 256 for n in counts), (family, counts)
                assert any(m % 4 for m in chunks) and any(m > 4 and m % 4 for m in chunks), (family, chunks)
                assert any(n % 256 and (n + 255) // 256 % 4 == 0 for n in counts), (family, counts)     # a ragged last chunk of a full workgroup
            elif sw == "CARRY_TILE":        # in chunks of 256 particles: exactly one tile, and a second tile that only the remainder loop walks
                chunks = [(n + 255) // 256 for n in counts]
                assert k[sw] in chunks, (family, chunks)
                assert any(0 < m - k[sw] < 8 for m in chunks), (family, chunks)
                assert k[sw] * 256 in counts and any(n % 4 for n in counts if n > k[sw] * 256), (family, counts)
            else:
                c = k[sw] * 256 if sw == "IS_MAX_CHUNKS" else k[sw]
                assert c in counts and c + 1 in counts, f"{family}: no case at {c} and {c + 1}, the two sides of {sw}"
    # what fba_create stores on each side of IS_MAX_CHUNKS * 256, as the cases expect it
    top = k["IS_MAX_CHUNKS"] * 256
    fmt = {(c["family"], c["kw"]["particles"]): c["fmt"] for c in F.CASES}
    assert (fmt["is_tiger_packed", top], fmt["is_tiger_packed", top + 1]) == ("packed_tiger", "dense")
    assert (fmt["is_gridworld_history", top], fmt["is_gridworld_history", top + 1]) == ("history", "dense")
    assert (fmt["is_collision_avoidance", top], fmt["is_collision_avoidance", top + 1]) == ("dense", "history")
    # the shape of a case: few slots, one or two of them used again, a search that is not the subject, a run that fits the record
    for c in F.CASES:
        kw = c["kw"]
        assert c["E"] in (2, 3) and c["runs"] in (c["E"] + 1, c["E"] + 2) and kw["sims"] <= 8 and 4 <= kw["horizon"] <= 6
        assert kw.get("episodes", 1) in (1, 2) and kw.get("episodes", 1) * kw["horizon"] <= 126
        assert "episodic" not in c["domain"]


@pytest.mark.parametrize("family", sorted(F.SWITCHES))
def test_filter_size_cases_update_three_times_in_a_row(family):
    """the cheapest case of every family on the oracle alone: some slot makes three belief updates in a row within one run"""
    c = F.cheapest_of(family)
    tr = W.oracle_side(c)["trace"]
    assert len(tr) > 0
    assert F.longest_update_streak(tr) >= MIN_STREAK, (c["name"], tr["terminal"].tolist())
