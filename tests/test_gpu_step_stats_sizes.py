"""fba_step_stats == the trace at every size at which step_stats_kernel does something else (tests/step_stats_size_cases.py: the table of
switch-overs, the cases and the reference).  A second workgroup, a thread's second slot, a second and a third LDS window, the compressed
row of the smallest and of the largest A, budgeted searches in two workgroups: a fault in any of them gives statistics that look plausible
and are wrong at exactly the sizes where nobody can hold them against the trace, so every case here stays below the trace's 2^22 records
and compares every member of every bin -- integers and reward sums with ==, the value sums within n * 2^-52 * sum |x_i| of math.fsum, the
probe members with Engine.probe() -- and asserts that its inputs exercise what it is there for."""
import time

import numpy as np
import pytest

import far_slot_cases
import step_stats_size_cases as S

pytestmark = pytest.mark.gpu


def _exercises(c, eng, tr, st):
    """the inputs exercise what the case is there for"""
    name, A, slots, n_bins = c["name"], c["A"], c["slots"], c["n_bins"]
    fit, flat = S.fit(A), st["steps"].reshape(-1)
    nwin, ngroups = S.windows(n_bins, A), S.workgroups(slots)
    assert eng.A == A and eng.slots == slots and st.size == n_bins, name
    assert int(np.count_nonzero(flat)) > 1, name
    if c["ends"]:
        assert 0 < int(st["terminals"].sum()) < int(flat.sum()), name
        assert len(set(flat.tolist())) > 1, name
    for sw in c["past"]:
        assert S.measure(sw, c) > S.threshold(sw, A), (name, sw)
    if nwin > 1:
        per_window = [int(flat[w * fit:(w + 1) * fit].sum()) for w in range(nwin)]
        last_rows = [int(flat[min((w + 1) * fit, n_bins) - 1]) for w in range(nwin)]
        print(f"{name}: steps per window {per_window}, in the last row of each {last_rows}")
        if c["ends"]:           # (an episode of these rarely lasts three steps: a window has steps where it holds the first step of an episode)
            H = eng.cfg.horizon
            assert all(n > 0 for w, n in enumerate(per_window) if any(b % H == 0 for b in range(w * fit, min((w + 1) * fit, n_bins)))), name
        else:
            assert all(per_window) and all(last_rows), name
    if ngroups > 1:
        # in some bin a run that holds nodes_max is reduced by another workgroup than slot 0's (runs = slots: run r is slot r's)
        bins = tr["episode"].astype(np.int64) * eng.cfg.horizon + tr["t"]
        holds = tr["n_nodes"] == st["nodes_max"].reshape(-1)[bins]
        assert np.any(S.workgroup_of(tr["run"][holds], slots) != 0), name
        assert len(set(S.workgroup_of(tr["run"], slots).tolist())) == ngroups, name
    if slots > S.STRIDE:
        assert np.any(tr["run"] >= S.STRIDE), name      # a slot that is some thread's second
    return nwin, ngroups


@pytest.mark.parametrize("name", [c["name"] for c in S.CASES])
def test_the_bins_equal_the_trace_at_this_size(name):
    c = S.BY_NAME[name]
    t0 = time.time()
    eng = S.engine(c, trace=1)
    if c["slots"] >= S.STRIDE:
        total = sum(a.bytes for a in eng.device_arrays().values())
        if total > far_slot_cases.BUDGET:
            pytest.skip(f"{name}: the context takes {total} bytes, more than the {far_slot_cases.BUDGET} a card is asked for")
    if c["probe"] == "full":
        eng.probe_enable()
    elif c["probe"]:
        eng.probe_enable(*c["probe"])
    eng.step_stats_enable()
    S.run(eng)
    tr, st = eng.trace(), eng.step_stats()
    t1 = time.time()
    steps = int(st["steps"].sum())
    assert len(tr) == steps == eng.counters().env_steps and 0 < len(tr) < S.TRACE_CAP, name
    if c["family"] == "budgeted":
        assert eng.particle_bytes < 1024, name      # history records
    nwin, ngroups = _exercises(c, eng, tr, st)
    ref = S.Ref(eng, tr)
    worst = ref.check(st, name, probe=c["probe"] is None)
    if c["probe"]:
        recs = eng.probe()
        first, count = (0, c["slots"]) if c["probe"] == "full" else c["probe"]
        inside = (tr["terminal"] == 0) & (tr["run"] >= first) & (tr["run"] < first + count)
        # a mark consumed in another window than the slot's, or twice, shows here
        assert int(st["probed"].sum()) == recs.size == recs.seen == int(np.sum(inside)) > 0, name
        if c["probe"] != "full":
            assert first < S.BLOCK < first + count and len(set(recs["slot"].tolist())) == count, name
        ints, terms = S.probe_ref(recs, st.shape)
        S.check_probe(st, ints, terms, name)
    eng.close()
    if c["trace_off"]:
        off = S.engine(c, trace=0)
        off.step_stats_enable()
        S.run(off)
        other = off.step_stats()
        assert len(off.trace()) == 0 and int(other["steps"].sum()) == off.counters().env_steps == steps, name
        for f in S.INTS + ["reward_sum", "reward_sq_sum"]:
            assert np.array_equal(other[f], st[f]), f"{name}, trace off: {f}"
        for f in ("value_sum", "value_sq_sum"):     # each within the bound of the exact sum: of each other within twice the bound
            assert np.all(np.abs(other[f] - st[f]) <= 2 * ref.bound(f)), f"{name}, trace off: {f}"
        ref.check(other, name + ", trace off")
        off.close()
    print(f"{name}: {c['slots']} slots, {c['n_bins']} bins, {nwin} windows, {ngroups} workgroups, {steps} steps, "
          f"largest error / bound {worst:.3e}, engine {t1 - t0:.2f} s, reference {time.time() - t1:.2f} s")
