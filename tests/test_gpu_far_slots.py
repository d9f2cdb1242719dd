"""Engine == oracle in slots beyond 4 GiB of a launch's arrays (tests/far_slot_cases.py: the table, what each case crosses and why).

A case runs one short experiment of runs = E in E slots, E so large that the arrays it names pass element 2^32 (or 2^31, or byte 2^32:
asserted from Engine.device_arrays() before anything runs), and
  1. the same experiment in a near context of 150 slots, whose arrays are the few megabytes the wide table pins to the oracle: every
     trace field of every record, every return, length, statistic and counter is equal bit for bit (runs are addressed by run index);
  2. the oracle's single runs at run 0, run E - 1, the slots on both sides of element 2^31 and 2^32 of every named array and four more;
  3. the host getters at the last slot: belief_get and belief_summary of slot E - 1 against a one-slot context that imported
     belief_export(E - 1, 1), or, for the beliefs a snapshot refuses, against the near context's slot that executed run E - 1.
An offset that wraps in 32 bits reads or writes another slot's memory in the far context only; nothing faults, and only this shows it."""
import time

import numpy as np
import pytest

import far_slot_cases as F
import fba_pomdp_amd as fba
import wide_launch_cases as W
from test_gpu_belief_summary import _close as summary_close     # the bound derived there: 8 N 2^-53 relative, zeros exact

gpu = pytest.mark.gpu


def _engine(c, slots, runs, trace):
    return fba.Engine(c["domain"], model=c["model"], belief=c["belief"], slots=slots, runs=runs, trace=trace, **c["kw"])


def _experiment(c, eng):
    stats = eng.run_bapomdp() if c["model"] != W.POMDP else [eng.run_planning()]
    cn = eng.counters()
    ret, ln = eng.returns()
    return dict(trace=eng.trace(), stats=[(s.count, s.mean, s.m2) for s in stats], counters=(cn.sim_steps, cn.belief_steps, cn.env_steps),
                returns=ret, lengths=ln)


def _assert_reaches(c, arrays):
    """the precondition, from the report: every named array is past its line, the context is within the budget, and a line short of
    2^32 elements is the furthest a context of this shape reaches within it; returns the runs to sample"""
    E = c["E"]
    total = sum(a.bytes for a in arrays.values())
    print(f"{c['name']}: E = {E}, {len(arrays)} arrays, {total} bytes")
    assert total <= F.BUDGET, f"the context takes {total} bytes"
    sample = {0, E - 1}
    for name, line in c["lines"].items():
        a = arrays[name]
        print(f"  {name}: {a.bytes} bytes, {a.elems} elements of {a.elem_bytes}, {a.buffers} x {a.slot_elems} per slot: past {line}")
        assert a.slot_elems > 0 and a.elems >= a.buffers * E * a.slot_elems
        assert F.crosses(line, a.elems, a.elem_bytes), f"{name} is not past {line}"
        if F.expected_elems(c, name) is not None:
            assert a.elems == F.expected_elems(c, name) and a.elem_bytes == F.ELEM_BYTES[name]
        if c["slow"]:
            print(f"  (time, not memory, keeps {name} at this line: {c['slow']})")
        elif line != F.ELEMS32:   # the whole context grown until this array reached the next line would not fit
            nxt = 2 ** 32 if line == F.ELEMS31 else 2 ** 31
            assert a.elems <= nxt and total * nxt / a.elems > F.BUDGET, f"{name} could reach {nxt} elements within the budget"
        sample |= F.boundary_slots(E, a.elems, a.slot_elems, a.buffers, a.elem_bytes)
    assert len(sample) > 2, "no slot beside a line was found"
    sample |= set(np.random.default_rng(c["kw"]["seed"]).choice(E, F.RANDOM_RUNS, replace=False).tolist())
    print(f"  runs compared with the oracle: {sorted(sample)}")
    return sorted(sample)


def _first_difference(far, near):
    """the slot (= run) at which the far and the near trace first differ: where to look for the 32-bit product"""
    n = min(len(far), len(near))
    for name in far.dtype.names:
        bad = np.nonzero(~np.all((far[name][:n] == near[name][:n]).reshape(n, -1), axis=1))[0]
        if bad.size:
            return f"field {name} first differs at record {bad[0]}, run (= far slot) {far['run'][bad[0]]}: {far[bad[0]]} vs {near[bad[0]]}"
    return f"{len(far)} records against {len(near)}"


def _getters(c, eng):
    """what the host getters say of a slot: (belief_get arrays [, the second filter's] [, the nested states], summary or None)"""
    nested, second = c["belief"] == "nested", c["belief"] == "reinvigoration"
    plain = c["model"] == W.POMDP

    def of(e, slot):
        summ = None if nested else e.belief_summary(slot, 1, mean_counts=not plain, edge_prob=not plain)      # (before belief_get: a lazy reset stays lazy)
        parts = [x for x in e.belief_get(slot) if x is not None]
        if second:
            parts += list(e.belief_get_fully_connected(slot))
        if nested:
            parts.append(e.belief_get_nested(slot))
        return parts, summ
    return of


def _assert_same_slot(c, got, ref):
    (parts, summ), (rparts, rsumm) = got, ref
    assert len(parts) == len(rparts)
    for a, b in zip(parts, rparts):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), "belief_get of the last slot"
    if summ is not None:
        n = c["kw"]["particles"]
        for name in ("weight_total", "weight_sq_total", "state_mass", "mean_counts", "edge_prob"):
            a, b = getattr(summ, name), getattr(rsumm, name)
            assert (a is None) == (b is None)
            if a is not None:
                summary_close(a, b, n, f"{c['name']}: belief_summary.{name} of the last slot")


@gpu
@pytest.mark.parametrize("name", [c["name"] for c in F.CASES])
def test_far_slots_equal_near_slots_and_the_oracle(name, monkeypatch):
    c = F.BY_NAME[name]
    E = c["E"]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    t0 = time.time()
    # ---- the near context: the same runs, by run index, in arrays of a few megabytes
    near_eng = _engine(c, F.NEAR, E, 1)
    near = _experiment(c, near_eng)
    last = (E - 1) % F.NEAR                       # the near slot whose last run was run E - 1
    assert near["trace"]["run"].max() == E - 1
    read = _getters(c, near_eng)
    near_last = read(near_eng, last)
    near_eng.close()
    t1 = time.time()
    print(f"{name}: the near context took {t1 - t0:.1f} s", flush=True)
    # ---- the far context (an allocation failure is a failure)
    eng = _engine(c, E, E, 1)
    assert eng.slots == E
    assert eng.particle_bytes == W.expected_particle_bytes(c, eng.ncnt), (eng.particle_bytes, eng.ncnt)
    if c["ncnt"]:
        assert eng.ncnt == c["ncnt"]
    sample = _assert_reaches(c, eng.device_arrays())
    far = _experiment(c, eng)
    t2 = time.time()
    total = sum(a.bytes for a in eng.device_arrays().values())     # (now with the per-run returns and the trace)
    print(f"  with returns and trace: {total} bytes")
    assert total <= F.BUDGET
    # 1. every run, engine against engine
    if len(far["trace"]) != len(near["trace"]) or far["trace"].tobytes() != near["trace"].tobytes():
        print("far and near differ: " + _first_difference(far["trace"], near["trace"]))
    W.assert_same_experiment(dict(c, sample=False), far, near)
    # 3. the host getters at the last slot
    far_last = read(eng, E - 1)
    if c["belief"] in ("nested", "reinvigoration"):      # (no snapshot of these beliefs: the near slot that ran run E - 1 holds the same filter)
        _assert_same_slot(c, far_last, near_last)
    else:
        block = eng.belief_export(E - 1, 1)
        one = _engine(c, 1, 1, 0)
        one.belief_import(0, block)
        assert one.belief_export(0, 1).tobytes() == block.tobytes()
        _assert_same_slot(c, far_last, read(one, 0))
        _assert_same_slot(c, far_last, near_last)
        one.close()
    eng.close()
    t3 = time.time()
    # 2. sampled runs, engine against oracle
    cs = dict(c, sample=True, sample_runs=sample)
    W.assert_same_experiment(cs, far, W.oracle_side(cs))
    print(f"{name}: near {t1 - t0:.1f} s, far {t2 - t1:.1f} s, getters {t3 - t2:.1f} s, oracle {time.time() - t3:.1f} s for {len(sample)} runs")


def test_the_far_table_covers_what_it_says():
    """without a GPU: the table's E, particle and simulation counts put every particle array over the line the table claims, by the size
    formulas of the wide table; no E or E + 1 is a multiple of 16; every case names an array; a case is short"""
    for c in F.CASES:
        E, kw = c["E"], c["kw"]
        assert E % 16 and (E + 1) % 16 and c["runs"] == E and E > F.NEAR, c["name"]
        assert c["lines"] and set(c["lines"].values()) <= {F.ELEMS32, F.ELEMS31, F.BYTES32}
        assert kw.get("episodes", 1) <= 2 and kw["horizon"] <= 8
        assert E * kw.get("episodes", 1) * kw["horizon"] <= 1 << 22, "the trace keeps 2^22 records"
        for name, line in c["lines"].items():
            elems = F.expected_elems(c, name)
            if elems is None:
                assert name in ("nodes", "hash", "bkt"), name     # (asserted from the report, on the GPU)
                continue
            assert F.crosses(line, elems, F.ELEM_BYTES[name]), (c["name"], name, line, elems)
            if line == F.ELEMS31:
                assert elems <= 2 ** 32
            if line == F.BYTES32:
                assert elems <= 2 ** 31
    named = {a for c in F.CASES for a in c["lines"]}
    assert {"p_rec", "p_weight", "wscan", "p_side", "nodes", "hash", "bkt", "p_rec_fc", "nest_s"} <= named
    assert F.boundary_slots(32771, 2 * 32771 * 65536, 65536, 2, 4) == {16383, 16384, 16385, 32767, 32768, 32769, 32764, 32765, 32766}
    assert all(set(c["lines"]) == {"p_rec"} for c in F.CASES if c["slow"])
