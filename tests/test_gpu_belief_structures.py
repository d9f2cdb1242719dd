"""fba_belief_structures / Engine.belief_structures: the posterior over whole model graphs reduced on the device from every record
format that has parent-set words, against numpy over Engine.belief_get of the same slot (structure_cases.py: the reference, the bound
and where it comes from).  Flat filters compare exactly, the order of the top list included; weighted ones within 8 * N * 2^-53."""
import subprocess

import numpy as np
import pytest

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

import structure_cases as SC

pytestmark = pytest.mark.gpu

TABLE = N.STRUCT_TABLE


@pytest.mark.parametrize("name", list(SC.FORMATS))
def test_every_record_format(name):
    eng, kind = SC.engine(name, particles=257, slots=4, runs=4, seed=9100 + len(name))
    assert eng.structure_lens() == SC.lens_from_layout(eng) and eng.structure_lens()[0] > 0
    SC.drive(eng, kind)
    res, refs = SC.check(eng, name, top_k=8)
    SC.close(res.query_mass[0, 0], res.top_mass[0, 0], 257, name + ": the most frequent structure of slot 0, asked for and listed")
    assert res.query_mass[0, 0] > 0
    assert np.all(res.query_mass[:, 1] == 0.0)                      # the absent one
    assert any(r.distinct > 1 for r in refs), "the particles of a slot differ in structure"
    if "history" in name:                                           # both goal-parent forms of an x / y node in one slot
        assert any(np.any(np.any(r.words == 7, axis=0) & np.any(r.words == 3, axis=0)) for r in refs)
    part, _ = SC.check(eng, name + ", slots 1..2", top_k=3, first=1, count=2)
    if not SC.weighted(eng):
        assert np.array_equal(part.set_mass, res.set_mass[1:3]) and np.array_equal(part.top_words, res.top_words[1:3, :3])
    eng.close()


@pytest.mark.parametrize("belief,domain,kw", [
    ("reinvigoration", "episodic-factored-tiger", dict(size=3, structure_prior=SC.MATCH_UNIFORM, resample_amount=8)),
    ("mh-within-gibbs", "random-collision-avoidance", dict(width=5, height=5, size=1, structure_prior=SC.UNIFORM, threshold=-2.0)),
])
def test_structure_beliefs(belief, domain, kw):
    """the main filter of the beliefs whose graphs move, after two episodes of an experiment"""
    eng = fba.Engine(domain, model=SC.FACT, belief=belief, particles=64, sims=32, horizon=5, episodes=2, runs=3, slots=3, seed=9201, **kw)
    eng.run_bapomdp()
    assert SC.weighted(eng) == (belief == "mh-within-gibbs")
    res, refs = SC.check(eng, belief, top_k=8)
    assert np.all(res.distinct >= 1) and np.all(res.stored == np.minimum(res.distinct, 8))
    eng.close()


def test_more_words_than_one_histogram_pass():
    """linear sysadmin of five computers under reinvigoration: 50 words of 32 parent sets, 1 600 histogram cells where a pass over the
    slot keeps 1 024 (32 words) -- the last 18 words are a second pass"""
    eng = fba.Engine("linear-sysadmin", model=SC.FACT, belief="reinvigoration", size=5, resample_amount=20, particles=50, sims=64, horizon=6,
                     episodes=2, runs=3, slots=3, seed=9251)
    eng.run_bapomdp()
    assert eng.structure_lens() == (50, 32)
    res, refs = SC.check(eng, "linear sysadmin 5", top_k=8)
    assert any(r.distinct > 1 for r in refs) and np.all(res.set_mass.sum(axis=2) == 50)
    eng.close()


def test_more_queries_than_the_kernel_keeps_close():
    """1 031 queries: the masses of the first 1 024 are summed in LDS, the rest directly in the output"""
    eng, kind = SC.engine("dense_factored_tiger2", particles=257, slots=3, runs=3, seed=9261)
    SC.drive(eng, kind)
    limit = int(SC.word_limits(eng)[0])
    assert eng.structure_lens()[0] == 1
    queries = (np.arange(1031, dtype=np.uint32) * 5 % limit).reshape(-1, 1)
    res, refs = SC.check(eng, "1 031 queries", top_k=2, queries=queries)
    assert np.all(res.query_mass[:, 1024:].sum(axis=1) > 0)
    for b in range(3):
        for v in range(limit):
            SC.close(res.query_mass[b][queries[:, 0] == v], np.full(int(np.sum(queries[:, 0] == v)), refs[b].set_mass[0, v]), 257, f"slot {b}, word {v}")
    eng.close()


@pytest.mark.parametrize("name", ["gridworld3_history_importance", "collision_avoidance_5x5x1_uniform", "packed_factored_tiger2"])
def test_consistent_with_the_summary(name):
    """sum of set_mass[m][v] over the v with bit j set = edge_prob[m][j] * weight_total, and set_mass[m] sums to weight_total: each side
    within 8 * N * 2^-53 of the exact sum, the summary's division and the product here one rounding each"""
    eng, kind = SC.engine(name, particles=257, slots=4, runs=4, seed=9300 + len(name))
    SC.drive(eng, kind)
    res = eng.belief_structures(top_k=0)
    summ = eng.belief_summary(state_mass=False, mean_counts=False)
    n, (nw, ns) = eng.cfg.particles, eng.structure_lens()
    tol = (16 * n + 8) * 2.0 ** -53
    v = np.arange(ns)
    for b in range(eng.slots):
        W = res.weight_total[b]
        assert abs(W - summ.weight_total[b]) <= tol * W
        for m in range(nw):
            assert abs(res.set_mass[b, m].sum() - W) <= tol * W, (b, m)
            for j in range(N.MAX_FEATURES):
                mine, theirs = res.set_mass[b, m][(v >> j) & 1 == 1].sum(), summ.edge_prob[b, m, j] * W
                assert abs(mine - theirs) <= tol * max(mine, theirs), (b, m, j, mine, theirs)
                assert (mine == 0.0) == (theirs == 0.0)
    eng.close()


@pytest.mark.parametrize("particles", [1, 64, 257])
@pytest.mark.parametrize("name", ["dense_factored_tiger2", "gridworld3_history_importance"])
def test_particle_counts_and_list_lengths(name, particles):
    eng, kind = SC.engine(name, particles=particles, slots=3, runs=3, seed=9400 + particles)
    SC.drive(eng, kind)
    for top_k in (0, 1, 64):
        res, _ = SC.check(eng, f"{name}, {particles} particles, top_k {top_k}", top_k=top_k, queries=None)
        assert res.query_mass.shape == (3, 0) and res.top_words.shape == (3, top_k, eng.structure_lens()[0])
    SC.check(eng, f"{name}, {particles} particles, queries and no list", top_k=0)
    eng.close()


def _distinct_structures(eng, count):
    """`count` pairwise distinct legal word lists: the mixed-radix enumeration of the legal words"""
    limit = [int(x) for x in SC.word_limits(eng)]
    room = 1
    for x in limit:
        room *= x
    assert room >= 1 << 12 and room >= count, "the layout offers at least 12 bits of legal parent-set choice"
    words = np.zeros((count, len(limit)), np.uint32)
    q = np.arange(count)
    for m, x in enumerate(limit):
        words[:, m] = q % x
        q = q // x
    assert len(np.unique(words, axis=0)) == count
    return words


def _write_structures(eng, words):
    lay = eng.factored_layout()
    _, _, cnt = eng.belief_get(0)
    cnt = cnt.copy()
    cnt[:, lay.n_counts:] = words.view(np.float32)
    eng.belief_set(0, weight=np.ones(len(words)), counts=cnt)
    w, back = SC.words_of(eng, 0)
    assert np.array_equal(back, words) and np.all(w == 1.0)


def test_overflow():
    n = TABLE + 300
    eng, kind = SC.engine("collision_avoidance_5x5x2_uniform", particles=n, slots=1, runs=1, seed=9501)
    SC.drive(eng, kind, updates=1)
    words = _distinct_structures(eng, n)
    queries = np.stack([words[0], words[n - 1], SC.absent_structure(eng, [SC.Reference(eng, 0, w_words=(np.ones(n), words))])])
    # more structures than the table holds
    _write_structures(eng, words)
    res = eng.belief_structures(top_k=64, queries=queries)
    ref = SC.Reference(eng, 0, queries)
    assert ref.distinct == n
    SC.compare_slot(res, 0, ref, eng, 64, "overflow")          # weight_total, set_mass and query_mass: never through the table
    assert res.overflow[0] == 1 and res.distinct[0] <= TABLE and res.stored[0] == 64
    assert res.unplaced_mass[0] + res.distinct[0] == res.weight_total[0] == n      # every placed structure holds one particle of weight 1.0
    assert np.all(res.top_mass[0] == 1.0) and np.array_equal(res.query_mass[0], [1.0, 1.0, 0.0])
    rows = [ref.index_of(r) for r in res.top_words[0]]
    assert min(rows) >= 0 and len(set(rows)) == 64 and rows == sorted(rows)          # placed structures, equal masses: ascending
    # exactly as many as it holds: the last 300 particles repeat the first 300 structures
    words[TABLE:] = words[:300]
    _write_structures(eng, words)
    res, refs = SC.check(eng, "a full table", top_k=64, queries=queries)
    assert refs[0].distinct == TABLE
    assert res.overflow[0] == 0 and res.distinct[0] == TABLE and res.unplaced_mass[0] == 0.0
    assert np.all(res.top_mass[0] == 2.0)
    eng.close()


@pytest.mark.parametrize("keep", ["0", "0x300000"])
def test_equal_hashes(keep, monkeypatch):
    """FBA_STRUCT_HASH_KEEP leaves the table's hash no bit, or two: structures of one hash are told apart by their words"""
    eng, kind = SC.engine("collision_avoidance_5x5x2_uniform", particles=300, slots=2, runs=2, seed=9601)
    SC.drive(eng, kind, updates=1)
    words = np.repeat(_distinct_structures(eng, 1)[:1], 300, axis=0)
    last = int(SC.word_limits(eng)[-1])
    words[:, -1] = np.arange(300) % min(last, 2)              # two structures that differ only in the last word
    assert last >= 2
    _write_structures(eng, words)
    monkeypatch.setenv("FBA_STRUCT_HASH_KEEP", keep)
    res, refs = SC.check(eng, "equal hashes, hash bits kept: " + keep, top_k=8)
    assert res.distinct[0] == 2 and np.array_equal(res.top_mass[0, :3], [150.0, 150.0, 0.0])
    assert np.array_equal(res.top_words[0, 0, :-1], res.top_words[0, 1, :-1]) and list(res.top_words[0, :2, -1]) == [0, 1]
    assert refs[1].distinct > 2                               # slot 1 keeps the structures it drew: many entries of one hash
    eng.close()
    eng, kind = SC.engine("gridworld3_history_rejection", particles=257, slots=2, runs=2, seed=9602)
    SC.drive(eng, kind)
    SC.check(eng, "history records, hash bits kept: " + keep, top_k=64)
    eng.close()


def _state(eng):
    c = eng.counters()
    return [eng.belief_export().tobytes(), eng.last_step_info().tobytes(), bytes(np.array([c.sim_steps, c.belief_steps, c.env_steps])),
            eng.L.fba_trace_count(eng.h)]


def test_read_only():
    """two contexts of one seed, one reads the structures on the way -- first of a lazily reset rejection filter: every particle,
    counter, action and step record keeps its bits; and an experiment that is read between its ticks leaves the trace of one that is not"""
    name = "packed_factored_tiger2"
    queries = np.array([[3], [1]], np.uint32)
    seen = []
    for with_call in (True, False):
        eng, kind = SC.engine(name, particles=130, slots=3, runs=3, seed=9700, trace=1)
        got = []
        eng.set_position(run=[11, 12, 13], episode=0, t=0)
        eng.belief_init()
        eng.belief_reset_domain_state()
        if with_call:                  # the reset is only flagged; belief_get would write it out, the call must not need that
            first = eng.belief_structures(queries=queries)
            assert np.all(first.weight_total == 130) and np.all(first.set_mass.sum(axis=2) == 130)
        eng.set_position(t=1)
        action = eng.select_action(hist_len=1)
        got.append(action)
        eng.belief_update(action, [SC.obs_for(eng, kind, e, 1) for e in range(3)])
        if with_call:
            before = _state(eng)
            eng.belief_structures(queries=queries)
            eng.belief_structures(1, 2, top_k=64)
            assert _state(eng) == before
        got += [x for e in range(3) for x in eng.belief_get(e)]
        got.append(eng.last_step_info())
        c = eng.counters()
        got.append(np.array([c.sim_steps, c.belief_steps, c.env_steps]))
        seen.append(got)
        eng.close()
    assert len(seen[0]) == len(seen[1])
    for a, b in zip(seen[0], seen[1]):
        assert a.tobytes() == b.tobytes()
    traces = []
    for with_call in (True, False):
        eng, _ = SC.engine(name, particles=130, slots=3, runs=6, seed=9701, trace=1, horizon=3, episodes=2)
        for _ in range(4):
            eng.run_ticks(2)
            if with_call:
                eng.belief_structures(queries=queries)
        traces.append(eng.trace())
        eng.close()
    assert len(traces[0]) == len(traces[1]) > 0
    for field in traces[0].dtype.names:
        assert np.array_equal(traces[0][field], traces[1][field]), field


def test_refusals():
    nested = fba.Engine("continuous-tiger", model=N.MODEL_BA_TABLE, belief="nested", particles=12, slots=2, runs=2, sims=16, horizon=8)
    with pytest.raises(ValueError, match="fba_belief_get_nested"):
        nested.belief_structures()
    nested.close()
    for model, domain, kw in ((N.MODEL_POMDP, "continuous-tiger", {}), (N.MODEL_BA_TABLE, "continuous-tiger", {}),
                              (SC.FACT, "random-collision-avoidance", dict(width=5, height=5, size=1))):      # (no structure prior: a fixed graph)
        eng = fba.Engine(domain, model=model, belief=SC.IS, particles=32, slots=2, runs=2, sims=16, horizon=8, **kw)
        eng.belief_init()
        assert eng.structure_lens() == (0, 0)
        with pytest.raises(ValueError, match="no parent-set words"):
            eng.belief_structures()
        assert eng.belief_summary(mean_counts=False, edge_prob=False).weight_total.shape == (2,)      # usable afterwards
        eng.close()
    eng, kind = SC.engine("dense_factored_tiger2", particles=32, slots=3, runs=3, seed=9801)
    SC.drive(eng, kind, updates=1)
    nw, ns = eng.structure_lens()
    for first, count in ((0, 4), (2, 2), (-1, 2)):
        with pytest.raises(ValueError, match="slots"):
            eng.belief_structures(first, count)
    for top_k in (-1, N.STRUCT_MAX_TOP + 1):
        with pytest.raises(ValueError, match="top_k"):
            eng.belief_structures(top_k=top_k)
    head = np.zeros(3, N.STRUCTURE_HEAD_DTYPE)
    ok = np.zeros((1, nw), np.uint32)
    assert eng.L.fba_belief_structures(eng.h, 0, 3, 8, -1, ok.ctypes.data, head.ctypes.data, None, None, None, None) == N.EINVAL
    assert b"queries" in eng.L.fba_last_error(eng.h)
    assert eng.L.fba_belief_structures(eng.h, 0, 3, 8, (1 << 16) + 1, ok.ctypes.data, head.ctypes.data, None, None, None, None) == N.EINVAL
    assert eng.L.fba_belief_structures(eng.h, 0, 3, 8, 1, None, head.ctypes.data, None, None, None, None) == N.EINVAL
    assert b"no query array" in eng.L.fba_last_error(eng.h)
    bad = np.zeros((2, nw), np.uint32)
    bad[1, nw - 1] = int(SC.word_limits(eng)[nw - 1])
    with pytest.raises(ValueError, match=f"query 1, word {nw - 1}"):
        eng.belief_structures(queries=bad)
    assert eng.L.fba_belief_structures(eng.h, 0, 3, 8, 0, None, None, None, None, None, None) == N.OK      # nothing asked for
    SC.check(eng, "after the refusals", top_k=8)
    eng.close()


def test_cli_structure_out(tmp_path):
    cli = fba.build_cli()
    out, path = tmp_path / "res.txt", tmp_path / "structures.txt"
    base = [cli, "fbapomdp", "-D", "episodic-factored-tiger", "--size", "2", "--structure-prior", "match-uniform", "-s", "16",
            "--particle-amount", "64", "--episodes", "2", "-H", "4", "--seed", "graphs", "-f", str(out)]
    r = subprocess.run(base + ["--runs", "3", "--structure-out", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [l.split() for l in path.read_text().splitlines() if l and not l.startswith("#")]
    assert [int(l[0]) for l in rows] == [0, 1, 2]
    for l in rows:
        total, distinct, overflow, stored = float(l[1]), int(l[2]), int(l[3]), int(l[4])
        assert total == 64.0 and overflow == 0 and stored == min(distinct, 8) >= 1 and len(l) == 5 + 2 * stored
        masses = [float(x) for x in l[5::2]]
        assert masses == sorted(masses, reverse=True) and sum(masses) <= 64.0
        assert all(0 <= int(x, 16) < 8 for w in l[6::2] for x in w.split(","))
    r = subprocess.run(base + ["--runs", "5", "--slots", "2", "--structure-out", str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "--structure-out needs runs <= slots" in r.stderr
    r = subprocess.run(base + ["--runs", "2", "-B", "nested", "--structure-out", str(path)], capture_output=True, text=True)
    assert r.returncode == 1
    for mode in ("planning", "bapomdp"):
        r = subprocess.run([cli, mode, "-D", "episodic-tiger", "--structure-out", str(path)], capture_output=True, text=True)
        assert r.returncode == 1 and "fbapomdp" in r.stderr
