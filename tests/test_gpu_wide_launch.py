"""Engine == oracle beyond the first 24 slots of a launch.  Every other oracle comparison of the suite runs in at most 24 slots, so for
nearly every kernel family the oracle has only seen lanes 0..23 of workgroup 0.  Here every kernel family that launch_search,
launch_belief_update, launch_init and launch_reset choose between runs a whole experiment in 150 (or 70) ragged slots, reused over
2 E + 37 runs, with episodes that end at different steps (tests/wide_launch_cases.py: the table and its geometry), and every trace field,
statistic, counter and per-run return must be the oracle's, bit for bit.  An LDS access beyond a workgroup's allocation is dropped or reads
zero on this hardware, so a column or a wave's area sized for fewer lanes than a launch has would show here and nowhere else."""
import numpy as np
import pytest

import fba_pomdp_amd as fba
import wide_launch_cases as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c["name"] for c in W.CASES])
def test_wide_launch_equals_the_oracle(name, monkeypatch):
    c = W.BY_NAME[name]
    assert c["E"] % 64 and c["E"] % 16 and c["E"] > 64
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    got = W.engine_side(c, fba)
    distinct = np.unique(got["lengths"])
    print(f"{name}: {len(got['trace'])} records, episode lengths {distinct.tolist()}")
    assert len(distinct) >= W.min_distinct_lengths(c), f"episodes of lengths {distinct.tolist()} only: the slots sit at the same t"
    W.assert_same_experiment(c, got, W.oracle_side(c))


def test_the_case_table_covers_what_it_says():
    """the shapes the table promises: runs = 2 E + 37 everywhere but in one case of fewer runs than slots, a particle count that is no
    power of two, and a horizon at which a history-search workgroup holds two waves, not four (launch_search halves the waves until
    their areas fit 64 KB beside the shared tables, which take under 8 KB at size 3)"""
    fewer = [c for c in W.CASES if c["runs"] < c["E"]]
    assert len(fewer) == 1 and all(c["runs"] == 2 * c["E"] + 37 for c in W.CASES if c not in fewer)
    assert any(c["kw"]["particles"] & (c["kw"]["particles"] - 1) for c in W.CASES)
    deep = W.BY_NAME["fbapomdp_gridworld3_history_importance_two_waves_per_workgroup"]["kw"]
    wave = W.h2_wave_bytes(deep["horizon"], deep["episodes"])
    assert 4 * wave > 64 * 1024 >= 2 * wave + 8 * 1024
    shallow = W.BY_NAME["fbapomdp_gridworld3_history_importance"]["kw"]
    assert 4 * W.h2_wave_bytes(shallow["horizon"], shallow["episodes"]) + 8 * 1024 <= 64 * 1024
