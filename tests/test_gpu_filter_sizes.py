"""Engine == oracle on both sides of every particle count at which the belief filter changes.  The engine chooses a kernel, a branch of a
kernel or a record format from `particles` alone (tests/filter_size_cases.py: the table of switch-overs), and every other oracle comparison
of the suite runs a few hundred particles: a `<` for a `<=` at one of these switches, a 16-bit source index one too narrow, the dropped last
element of a ragged chunk or a carry lost between two tiles would pass them all.  Here a small whole experiment runs at N = c and N = c + 1
of every switch, with at least three belief updates in a row in some slot (the buffer flip; a resampled filter feeding the next update), and
every trace field -- weight_total, update_count and belief_hash after every update among them --, statistic, counter and per-run return
must be the oracle's, bit for bit.  particle_bytes is compared with the format's formula, which says which record format fba_create chose
at that N.  The composite beliefs (reinvigoration, incubator, cheating-reinvigoration, Metropolis-Hastings, nested) run the same kernels on
further filters that belief_hash does not cover: their cases also compare every filter of one slot, as the experiment left it, with the
oracle's after that slot's last run, and test_composite_belief_caps creates contexts at and beyond their largest filters.  The tests
without a GPU keep the table honest: the thresholds are read out of the sources, so a moved threshold fails the table instead of leaving it
beside the switch; every family's cheapest case makes three updates in a row, re-draws its filter where the belief has a threshold for it,
and makes more rejection attempts than one chunk holds where it has two rejection filters (9 s on the oracle for the composite families)."""
import functools
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
    final = []
    after = (lambda eng: final.append(F.engine_final_filters(c, eng))) if c["family"] in F.FILTERS else None
    W.assert_same_experiment(c, W.engine_side(c, fba, after=after), ref)   # (engine_side: slots, and particle_bytes against the format's formula)
    for run, got in final:      # the composite beliefs: the filters themselves, which the trace's belief_hash covers in part
        F.assert_same_filters(name, run, got, F.oracle_final_filters(c, run))


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
    # the largest filters of the composite beliefs: what map_incubator, plan_filters and map_nested refuse (fba_engine.hip)
    with open(os.path.join(CSRC, "fba_engine.hip")) as f:
        engine = f.read()
    body = lambda fn: re.search(r"\nint %s\([^)]*\)\n\{\n(.*?)\n\}\n" % fn, engine, re.S).group(1)
    (v,) = re.findall(r'if \(cfg\.particles > (\w+)\) return fail\(nullptr, FBA_EINVAL, "incubator belief: at most %d particles per slot", (\w+)\);',
                      body("map_incubator"))
    assert v == ("IS_LDS_MAX_N", "IS_LDS_MAX_N")
    k["INCUBATOR_MAX"] = k["IS_LDS_MAX_N"]
    # (both refusals of plan_filters stand behind D.is_multi: a weighted filter of sw.is_multi_min particles or more)
    refusals = re.findall(r'D\.is_multi\) return fail\(c, FBA_EINVAL, "([\w-]+) belief: at most %d particles per slot", IS_MAX_CHUNKS \* (\d+)\);',
                          body("plan_filters"))
    assert sorted(refusals) == [("cheating-reinvigoration", "256"), ("mh-within-gibbs", "256")]
    assert re.search(r"D\.is_multi\s*=\s*weighted_filters\(P\) && P\.N >= sw\.is_multi_min;", body("plan_filters"))
    assert re.search(r"s\.is_multi_min\s*=\s*multi_min \? [^;]* : IS_MAX_CHUNKS \* 256 \+ 1;", engine)
    k["CHEATING_MAX"] = k["MH_MAX"] = k["IS_MAX_CHUNKS"] * 256
    (v,) = re.findall(r'if \(cfg\.particles > (\d+)\) return fail\(nullptr, FBA_EINVAL, "nested belief: at most (\d+) count particles',
                      body("map_nested"))
    assert v[0] == v[1]
    k["NESTED_MAX"] = int(v[0])
    # (one lane per count particle in one workgroup: that is the limit)
    assert len(re.findall(r"__launch_bounds__\(%s\) nested_(?:fill|update)_kernel\(" % v[0], kernels)) == 2
    k["wave"] = F.WAVE
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
            elif sw in F.CAPS:              # the largest filter of a composite belief: a case at exactly that N, none beyond
                assert max(counts) == k[sw], f"{family}: no case at {k[sw]}, the most particles fba_create takes ({sw})"
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
        assert c["family"] not in F.FILTERS or c["fmt"] == "dense"


@pytest.mark.parametrize("family", sorted(F.SWITCHES))
def test_filter_size_cases_update_three_times_in_a_row(family):
    """the cheapest case of every family on the oracle alone: some slot makes three belief updates in a row within one run"""
    c = F.cheapest_of(family)
    tr = _oracle_trace(c["name"])
    assert len(tr) > 0
    assert F.longest_update_streak(tr) >= MIN_STREAK, (c["name"], tr["terminal"].tolist())


@functools.lru_cache(maxsize=None)
def _oracle_trace(name):
    """the oracle's trace of a case, computed once for the tests without a GPU (read only)"""
    tr = W.oracle_side(F.BY_NAME[name])["trace"]
    tr.setflags(write=False)
    return tr


@pytest.mark.parametrize("family", ["cheating_factored_tiger", "mh_gibbs_messages", "mh_gibbs_rejection", "mh_nips"])
def test_filter_size_cases_trigger_the_redraw(family):
    """the cheapest case of the beliefs that re-draw their filter below a log-likelihood threshold: with a threshold that is never reached
    the oracle leaves other filters behind, so the case runs cheat_kernel or mh_kernel and not the plain importance filter alone"""
    c = F.cheapest_of(family)
    tr = _oracle_trace(c["name"])
    never = W._run(W.make_oracle(c, runs=c["runs"], threshold=-1e9), True)[0]
    assert len(tr) > 0 and len(never) > 0
    n = min(len(tr), len(never))
    differ = int((tr["belief_hash"][:n] != never["belief_hash"][:n]).sum())
    print(f"{c['name']}: belief_hash differs in {differ} of {n} records from the run whose re-draw never triggers")
    assert differ >= 1


@pytest.mark.parametrize("family", ["reinvig_factored_tiger", "reinvig_generic", "incubator_factored_tiger", "incubator_collision_avoidance"])
def test_filter_size_cases_reject_beyond_one_chunk(family):
    """the cheapest case of the beliefs on two rejection filters: some update makes more attempts than the filter has particles (and than
    one chunk of REJECT_BLOCK holds), so a further chunk of attempts has run"""
    c = F.cheapest_of(family)
    most = int(_oracle_trace(c["name"])["update_count"].max())
    print(f"{c['name']}: at most {most} attempts in one update of {c['kw']['particles']} particles")
    assert most > max(c["kw"]["particles"], _constants()["REJECT_BLOCK"])


@pytest.mark.gpu
def test_composite_belief_caps():
    """what fba_create refuses and takes at the largest filters of the composite beliefs (contexts only: nothing runs)"""
    k = _constants()
    ft = dict(model=W.FACT, size=2, sims=8, slots=1)
    with pytest.raises(ValueError, match=f"at most {k['INCUBATOR_MAX']} particles"):
        fba.Engine(F.CFTIGER, belief="incubator", particles=k["INCUBATOR_MAX"] + 1, structure_prior=2, resample_amount=6, threshold=0.5, **ft)
    with pytest.raises(ValueError, match=f"at most {k['CHEATING_MAX']} particles"):
        fba.Engine(F.CFTIGER, belief="cheating-reinvigoration", particles=k["CHEATING_MAX"] + 1, structure_prior=1, threshold=-1.5,
                   resample_amount=7, **ft)
    for belief, option in (("mh-within-gibbs", 0), ("mh-within-gibbs", 1), ("mh-nips", 0)):
        mh = dict(belief=belief, belief_option=option, structure_prior=2, threshold=-1.0, **ft)
        with pytest.raises(ValueError, match=f"at most {k['MH_MAX']} particles"):
            fba.Engine(F.CFTIGER, particles=k["MH_MAX"] + 1, **mh)
        eng = fba.Engine(F.CFTIGER, particles=k["MH_MAX"], **mh)
        assert eng.slots == 1 and eng.particle_bytes == W.dense_bytes(eng.ncnt)
        eng.close()
    with pytest.raises(ValueError, match=f"at most {k['NESTED_MAX']} count particles"):
        fba.Engine(F.CTIGER, model=W.TABLE, belief="nested", particles=k["NESTED_MAX"] + 1, sims=8, slots=1)
