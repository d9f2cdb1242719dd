"""fba_run_bapomdp_span (Engine.run_bapomdp(first_episode, stop_episode, beliefs)): a Bayes-adaptive experiment run in spans, each resumed
from the belief snapshots exported after the one before, must be the uninterrupted experiment -- every trace record (belief_hash, root_n
and root_q included), return, length, statistic and final filter, bit for bit.  Engine against itself, against the oracle resumed from the
same filters in table form, across slot counts, under a search budget, with compact tiger filters, and through the command line; a
refused call must leave the context as it was.  There is no tolerance anywhere in this file.  Cases and seeds: tests/resume_cases.py."""
import contextlib
import functools
import os
import subprocess

import numpy as np
import pytest

import fba_pomdp_amd as fba
import resume_cases as R
from fba_pomdp_amd import _native as N
from oracle import pyorc as orc
from per_call_cases import _same_particles

pytestmark = pytest.mark.gpu

HEAD = N.SNAPSHOT_HEAD_DTYPE
EPISODES = R.EPISODES
IS = "importance_sampling"


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(name, env=None, **over):
    domain, model, belief, fenv, kw = R.config(name, **over)
    domain = kw.pop("domain", domain)
    fenv.update(env or {})
    with _environment(fenv):
        return fba.Engine(domain, model=model, belief=belief, **kw)


def _outcome(eng, stats):
    ret, ln = eng.returns()
    return dict(trace=eng.trace(), returns=ret, lengths=ln, stats=[(s.count, s.mean, s.m2) for s in stats])


def _heads(blocks):
    return np.ascontiguousarray(blocks[:, :64]).view(HEAD).reshape(-1)


def _key(env, over):
    return tuple(sorted((env or {}).items())), tuple(sorted(over.items()))


@functools.lru_cache(maxsize=None)
def _whole_cached(name, key):
    env, over = dict(key[0]), dict(key[1])
    eng = _engine(name, env, trace=1, **over)
    out = _outcome(eng, eng.run_bapomdp())
    out["blocks"] = eng.belief_export()
    eng.close()
    return out


def _whole(name, env=None, **over):
    """the uninterrupted experiment of a case: computed once, shared, never changed"""
    return _whole_cached(name, _key(env, over))


@functools.lru_cache(maxsize=None)
def _first_cached(name, k, key):
    env, over = dict(key[0]), dict(key[1])
    eng = _engine(name, env, trace=1, **over)
    out = _outcome(eng, eng.run_bapomdp(0, k))
    out["blocks"] = eng.belief_export()
    eng.close()
    return out


def _first(name, k, env=None, **over):
    """span [0, k) of a case and the blocks exported behind it: computed once, shared, never changed"""
    return _first_cached(name, k, _key(env, over))


def _same_records(got, want, what):
    assert len(got) == len(want) > 0, f"{what}: {len(got)} trace records, {len(want)} in the whole run"
    for field in want.dtype.names:
        a, b = np.ascontiguousarray(got[field]), np.ascontiguousarray(want[field])
        bad = np.nonzero(~np.all((a.view(np.uint8).reshape(len(a), -1) == b.view(np.uint8).reshape(len(b), -1)), axis=1))[0]
        assert bad.size == 0, f"{what}: {field} of record {bad[0]} (run, episode, t = {want[bad[0]]['run']}, {want[bad[0]]['episode']}, {want[bad[0]]['t']}): " \
                              f"{got[bad[0]][field]} / {want[bad[0]][field]}"


def _sorted(tr):
    return tr[np.lexsort((tr["t"], tr["episode"], tr["run"]))]


def _same_span(got, want, first, stop, what):
    """the outcome of span [first, stop) against the whole run's: its records, returns, lengths and statistics there, nothing outside"""
    mine = want["trace"][(want["trace"]["episode"] >= first) & (want["trace"]["episode"] < stop)]
    _same_records(_sorted(got["trace"]), _sorted(mine), what)
    inside = np.zeros(EPISODES, bool)
    inside[first:stop] = True
    assert np.array_equal(got["returns"][:, inside].view(np.uint64), want["returns"][:, inside].view(np.uint64)), what + ": returns"
    assert np.array_equal(got["lengths"][:, inside], want["lengths"][:, inside]), what + ": lengths"
    assert not got["returns"][:, ~inside].any() and not got["lengths"][:, ~inside].any(), what + ": returns and lengths outside the span are 0"
    for e in range(EPISODES):
        assert got["stats"][e] == (want["stats"][e] if inside[e] else (0.0, 0.0, 0.0)), f"{what}: statistic of episode {e}"


def _resume(name, k, blocks, env=None, stop=None, **over):
    eng = _engine(name, env, trace=1, **over)
    out = _outcome(eng, eng.run_bapomdp(k, stop, blocks))
    out["blocks"] = eng.belief_export()
    eng.close()
    return out


# ---- 1. split equals whole ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.SPLITS)
@pytest.mark.parametrize("name", R.SPLIT_FORMATS)
def test_split_equals_whole(name, k):
    whole, a = _whole(name), _first(name, k)
    _same_span(a, whole, 0, k, f"{name}, span [0, {k})")
    b = _resume(name, k, a["blocks"])
    _same_span(b, whole, k, EPISODES, f"{name}, span [{k}, {EPISODES}) from the blocks of [0, {k})")
    _same_records(_sorted(np.concatenate([a["trace"], b["trace"]])), _sorted(whole["trace"]), f"{name}, the two spans' records together")
    assert np.array_equal(a["returns"] + b["returns"], whole["returns"]) and np.array_equal(a["lengths"] + b["lengths"], whole["lengths"])
    assert np.array_equal(b["blocks"], whole["blocks"]), f"{name}, k = {k}: the final filters, as exported"


def test_three_spans_equal_whole():
    """[0, 1), [1, 3), [3, 5): a span in the middle, resumed from and resumed"""
    name = "gridworld3_history_importance"
    whole, a = _whole(name), _first(name, 1)
    b = _resume(name, 1, a["blocks"], stop=3)
    _same_span(b, whole, 1, 3, name + ", span [1, 3)")
    c = _resume(name, 3, b["blocks"])
    _same_span(c, whole, 3, EPISODES, name + ", span [3, 5)")
    assert np.array_equal(c["blocks"], whole["blocks"])


def test_split_equals_whole_at_an_odd_particle_count():
    """65 weighted particles: the record part of a block stands at 8 bytes in the caller's buffer, at 16 in the store"""
    name = "gridworld3_history_importance"
    whole, a = _whole(name, particles=65), _first(name, 2, particles=65)
    assert a["blocks"].shape[1] % 16 == 8
    b = _resume(name, 2, a["blocks"], particles=65)
    _same_span(b, whole, 2, EPISODES, name + ", 65 particles")
    assert np.array_equal(b["blocks"], whole["blocks"])


def test_split_equals_whole_with_whole_record_strides():
    """collision-avoidance records never outgrow 64 bytes at this shape; stored whole, they are restored whole"""
    name = "collision_avoidance_5x5x2_history"
    whole, a = _whole(name, R.STRIDE_FULL_ENV), _first(name, 2, R.STRIDE_FULL_ENV)
    assert np.all(_heads(a["blocks"])["stride"] == R.RECORD_BYTES)
    b = _resume(name, 2, a["blocks"], R.STRIDE_FULL_ENV)
    _same_span(b, whole, 2, EPISODES, name + ", FBA_HIST_STRIDE=full")
    assert np.array_equal(b["blocks"], whole["blocks"])
    assert np.array_equal(whole["trace"], _whole(name)["trace"]), "the stride of the records is storage only"


# ---- 2. the strides are really met -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.HISTORY)
def test_the_blocks_have_every_stride(name):
    seen, entries = set(), {}
    for k in R.SPLITS:
        heads = _heads(_first(name, k)["blocks"])
        total = sum((heads["hist_cnt"] >> np.uint32(8 * a)) & np.uint32(0xff) for a in range(4))
        assert np.array_equal(total, R.entries_after(name, k)), f"{name}, k = {k}: entries per record, the oracle's updates"
        assert [int(s) for s in heads["stride"]] == [R.stride_of(int(n)) for n in total]
        seen |= {int(s) for s in heads["stride"]}
        entries[k] = total.tolist()
    if name in R.GRIDWORLD_HISTORY:
        assert seen == {64, 128, R.RECORD_BYTES}, (name, entries)
    else:       # (resume_cases.py: 12 entries at most, whatever the seed; whole records: test_split_equals_whole_with_whole_record_strides)
        assert seen == {64}, (name, entries)


def test_packed_blocks_count_their_updates():
    """head.updates after a span: the real steps of the slot's run so far, which bound every 16-bit increment of its records"""
    for name in ("packed_tiger", "packed_factored_tiger2"):
        for k in R.SPLITS:
            heads = _heads(_first(name, k)["blocks"])
            assert np.array_equal(heads["updates"], _whole(name)["lengths"][:, :k].sum(axis=1)), (name, k)
        assert np.array_equal(_heads(_whole(name)["blocks"])["updates"], _whole(name)["lengths"].sum(axis=1)), name


# ---- 3. against the oracle, resumed from the same filters in table form ------------------------------------------------------------
@pytest.mark.parametrize("name", R.ORACLE_FORMATS)
def test_resumed_span_equals_the_oracle(name):
    k = 2
    weighted = R.fmt_of(name)[4] == IS
    eng = _engine(name, trace=1)
    eng.run_bapomdp(0, k)
    blocks = eng.belief_export()
    tables = [eng.belief_get(e, weights=weighted, counts=True) for e in range(eng.slots)]
    eng.close()
    eng = _engine(name, trace=1)
    eng.run_bapomdp(k, None, blocks)
    tr = _sorted(eng.trace())
    ret, _ = eng.returns()
    L = orc.lib()
    at = 0
    for run in range(eng.cfg.runs):
        o = R.make_oracle(name, runs=1)
        s, w, cnt = tables[run]
        L.orc_rng_episode(o.rng, run, 0, 0)
        o.belief_initiate()       # (a filter to set; its draws are the run's own INIT streams and move nothing else)
        o.belief_set(s, w if weighted else None, cnt)
        for ep in range(k, EPISODES):
            L.orc_rng_episode(o.rng, run, ep, 0)
            o.belief_reset_domain_state()
            L.orc_rng_stream(o.rng, orc.PH_START, 0)
            hidden = o.env_start()
            total, disc = 0.0, 1.0
            for t in range(R.HORIZON):
                L.orc_rng_episode(o.rng, run, ep, t)
                action, _ = o.select_action(t)
                L.orc_rng_stream(o.rng, orc.PH_ENV, 0)
                hidden, obs, reward, term = o.env_step(hidden, action)
                rec = tr[at]
                at += 1
                what = f"{name}: run {run}, episode {ep}, t {t}"
                assert (rec["run"], rec["episode"], rec["t"]) == (run, ep, t), what
                assert (rec["action"], rec["state"], rec["obs"], rec["terminal"]) == (action, hidden, obs, int(bool(term))), what
                assert np.float64(rec["reward"]).view(np.uint64) == np.float64(reward).view(np.uint64), what
                total += reward * disc
                disc *= eng.cfg.discount
                if term:
                    break
                o.belief_update(action, obs)
                assert not o.L.orc_error(o.h), what + ": the oracle refused the update"
            assert np.float64(ret[run, ep]).view(np.uint64) == np.float64(total).view(np.uint64), f"{name}: return of run {run}, episode {ep}"
        got = eng.belief_get(run, weights=weighted, counts=True)
        os_, ow, ocnt = o.belief_get()
        _same_particles((got[0], got[1] if weighted else None, got[2]), (os_, ow, ocnt), f"{name}: the final filter", run)
    assert at == len(tr)
    eng.close()


# ---- 4. slots do not matter ---------------------------------------------------------------------------------------------------------
def _seven_runs(name, blocks, k=2, env=None, **over):
    return _resume(name, k, blocks, env, runs=7, **over)


def _same_outcome(a, b, what):
    _same_records(_sorted(a["trace"]), _sorted(b["trace"]), what)
    assert np.array_equal(a["returns"].view(np.uint64), b["returns"].view(np.uint64)) and np.array_equal(a["lengths"], b["lengths"]), what
    assert a["stats"] == b["stats"], what


@pytest.mark.parametrize("name", ["gridworld3_history_importance", "packed_tiger", "dense_tiger"])
def test_one_learned_filter_in_three_slots_and_in_seven(name):
    one = _first(name, 2)["blocks"][:1]
    wide = _seven_runs(name, one, slots=7)
    narrow = _seven_runs(name, one, slots=3)      # (slots start their second and third runs in later ticks: restores inside tick())
    _same_outcome(narrow, wide, name + ": 7 runs from one block, 3 slots against 7")
    assert len(np.unique(wide["trace"]["run"])) == 7 and wide["trace"]["episode"].min() == 2


def test_one_learned_filter_under_a_search_budget():
    name = "gridworld3_history_importance"
    one = _first(name, 2)["blocks"][:1]
    wide = _seven_runs(name, one, slots=7)
    parked = _seven_runs(name, one, slots=3, search_budget=37)      # (16 simulations of up to 9 iterations: a search takes several launches)
    _same_outcome(parked, wide, name + ": search_budget 37 in 3 slots against no budget in 7")


def test_one_learned_filter_with_compact_tiger_filters():
    """episodic tiger at 3 584 particles: the experiment loop keeps 16-byte records between updates"""
    name, over = "packed_tiger", dict(domain="episodic-tiger", particles=3584)
    eng = _engine(name, trace=1, **over)
    eng.run_bapomdp(0, 2)
    assert eng.debug_compact_slots() > 0, "the span left no slot compact: the case does not meet the compact path"
    one = eng.belief_export()[:1]
    eng.close()
    compact = _seven_runs(name, one, slots=3, **over)
    plain = _seven_runs(name, one, env={"FBA_NO_COMPACT": "1"}, slots=3, **over)
    _same_outcome(compact, plain, name + ": compact filters against FBA_NO_COMPACT=1")
    assert np.array_equal(compact["blocks"], plain["blocks"])


def test_each_run_takes_its_own_block_in_three_slots():
    name = "packed_tiger"       # (7 slots in resume_cases.py: the blocks are made in a 7-slot context)
    whole, a = _whole(name), _first(name, 2)
    assert a["blocks"].shape[0] == 7
    b = _resume(name, 2, a["blocks"], slots=3, runs=7)
    _same_span(b, whole, 2, EPISODES, name + ": 7 blocks, 7 runs, 3 slots")
    # slot e is left with the filter of the last run it made: runs 6, 4, 5
    assert np.array_equal(b["blocks"], whole["blocks"][[6, 4, 5]])


# ---- 5. refusals leave the context untouched ---------------------------------------------------------------------------------------
def _refused(eng, match, *args):
    before = eng.belief_export()
    with pytest.raises(ValueError, match=match):
        eng.run_bapomdp(*args)
    assert np.array_equal(eng.belief_export(), before), "a refused span changed a filter"


def _then_runs_as_fresh(name, eng, **over):
    _same_outcome(_outcome(eng, eng.run_bapomdp()), _whole(name, **over), name + ": a plain run behind the refusals")
    eng.close()


@pytest.mark.parametrize("name", ["gridworld3_history_importance", "packed_tiger"])
def test_refusals_leave_the_context_untouched(name):
    blocks = _first(name, 2)["blocks"]
    runs, per = blocks.shape
    eng = _engine(name, trace=1)
    eng.run_bapomdp(0, 1)       # (filters to be left alone)
    _refused(eng, "not a span", 3, 3, blocks)
    _refused(eng, "not a span", -1, 2, None)
    _refused(eng, "not a span", 2, EPISODES + 1, blocks)
    _refused(eng, "nblocks 2", 2, None, blocks[:2])
    _refused(eng, "without blocks", 2, None, None)
    before = eng.belief_export()
    with pytest.raises(ValueError, match="bytes"):      # (wrong bytes: the binding would derive them from the array)
        st = (N.Stat * EPISODES)()
        eng._chk(eng.L.fba_run_bapomdp_span(eng.h, 2, EPISODES, blocks.ctypes.data, runs, blocks.nbytes - 8, st))
    assert np.array_equal(eng.belief_export(), before)
    other = blocks.copy()       # a block that stands over another prior: the fingerprint (header bytes 48..55 are the prior's hash)
    other[runs - 2, 48] ^= 1
    _refused(eng, f"block {runs - 2}: prior hash", 2, None, other)
    flipped = blocks.copy()
    flipped[runs - 1, per - 100] ^= 0x10
    _refused(eng, f"block {runs - 1}: checksum", 2, None, flipped)
    bad = blocks.copy()         # a bad record: particle 5 of block 1 in a state outside the domain, the checksum made right again
    heads = _heads(bad)
    at = 64 + (R.PARTICLES * 8 if heads["weighted"][0] else 0) + 5 * int(heads["stride"][1]) + (0 if heads["record_format"][0] >= 5 else 48)
    bad[1, at:at + 4] = np.frombuffer(np.uint32(eng.S + 3).tobytes(), np.uint8)
    bad[1, 56:64] = np.frombuffer(np.uint64(N.snapshot_checksum(bad[1, 64:])).tobytes(), np.uint8)
    _refused(eng, "block 1, particle 5: a state outside the domain", 2, None, bad)
    # the room rule: the blocks of [0, 2) hold up to 16 of a run's 40, episodes [1, 5) would add 32
    hist = name in R.HISTORY
    held = int(R.entries_after(name, 2)[0]) if hist else int(_whole(name)["lengths"][0, :2].sum())
    assert held + 32 > 40, "the case does not meet the room rule"
    what = "history entries per record" if hist else "counted updates"
    _refused(eng, rf"block 0 holds {held} {what}, episodes \[1, 5\) of 8 steps may add 32: {held + 32} / 40", 1, None, blocks)
    _then_runs_as_fresh(name, eng)


def test_a_packed_increment_beyond_the_counted_updates_is_refused():
    name = "packed_tiger"
    blocks = _first(name, 2)["blocks"].copy()
    blocks[2, 64 + 9 * 64 + 2] = 17       # particle 9 of block 2: an increment of 17 + ... where 16 updates were counted
    blocks[2, 56:64] = np.frombuffer(np.uint64(N.snapshot_checksum(blocks[2, 64:])).tobytes(), np.uint8)
    eng = _engine(name, trace=1)
    _refused(eng, "block 2, particle 9: an increment beyond the updates its header counts", 2, None, blocks)
    _then_runs_as_fresh(name, eng)


@pytest.mark.parametrize("belief,kw", [("reinvigoration", dict(resample_amount=8)), ("cheating-reinvigoration", dict(resample_amount=7, threshold=-1.5, structure_prior=1)),
                                       ("incubator", dict(resample_amount=6, threshold=0.5)), ("mh-within-gibbs", dict(threshold=-0.5, structure_prior=1)),
                                       ("mh-nips", dict(threshold=-0.5, structure_prior=1)), ("nested", {})])
def test_beliefs_with_more_than_a_main_filter_are_refused(belief, kw):
    args = dict(size=2, structure_prior=2, particles=12 if belief == "nested" else 48, sims=16, horizon=4, episodes=3, slots=3, runs=3, seed=8201, trace=1)
    args.update(kw)
    model = N.MODEL_BA_TABLE if belief == "nested" else N.MODEL_BA_FACTORED
    if belief == "nested":
        args.pop("size"), args.pop("structure_prior")
    domain = "episodic-tiger" if belief == "nested" else "episodic-factored-tiger"
    eng = fba.Engine(domain, model=model, belief=belief, **args)
    with pytest.raises(ValueError, match="a snapshot holds the main filter of a slot, and the " + belief.split("-")[0]):
        eng.run_bapomdp(0, 2)
    got = _outcome(eng, eng.run_bapomdp())
    fresh = fba.Engine(domain, model=model, belief=belief, **args)
    _same_outcome(got, _outcome(fresh, fresh.run_bapomdp()), belief + ": a plain run behind the refusal")
    eng.close()
    fresh.close()


def test_a_plain_pomdp_context_is_refused():
    eng = fba.Engine("episodic-tiger", model=N.MODEL_POMDP, particles=64, sims=16, horizon=4, slots=3, runs=3, seed=8202)
    st = (N.Stat * 1)()
    with pytest.raises(ValueError, match="needs a Bayes-adaptive model"):
        eng._chk(eng.L.fba_run_bapomdp_span(eng.h, 0, 1, None, 0, 0, st))
    a = eng.run_planning()
    fresh = fba.Engine("episodic-tiger", model=N.MODEL_POMDP, particles=64, sims=16, horizon=4, slots=3, runs=3, seed=8202)
    b = fresh.run_planning()
    assert (a.count, a.mean, a.m2) == (b.count, b.mean, b.m2)
    eng.close()
    fresh.close()


def test_the_restores_are_counted_in_the_kernel_times():
    name = "gridworld3_history_importance"
    blocks = _first(name, 2)["blocks"]
    eng = _engine(name)
    eng.reset_kernel_times()
    eng.run_bapomdp(2, None, blocks)
    kt = eng.kernel_times()["init_kernel"]
    strides = _heads(blocks)["stride"].astype(np.int64)
    assert kt.units == R.PARTICLES * len(blocks) and kt.bytes == 2 * R.PARTICLES * int((strides + 8).sum()) and kt.launches > 0
    eng.close()


# ---- 7. the command line ---------------------------------------------------------------------------------------------------------------
def test_cli_spans_equal_the_whole_run(tmp_path):
    cli = fba.build_cli()
    common = [cli, "fbapomdp", "-D", "gridworld", "--size", "3", "--structure-prior", "match-uniform", "-B", "importance_sampling", "-s", "16",
              "--particle-amount", "130", "-H", "8", "--episodes", "5", "--runs", "4", "--slots", "4", "--seed", "resume"]

    def run(tag, *args):
        out = tmp_path / (tag + ".res")
        r = subprocess.run(common + ["-f", str(out)] + list(args), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = [l for l in out.read_text().splitlines() if l and not l.startswith("#")]
        return [l.split(", ")[:4] for l in lines]       # (the fifth column is a time)

    whole = run("whole")
    f = str(tmp_path / "beliefs.bin")
    a = run("a", "--stop-episode", "2", "--belief-out", f)
    b = run("b", "--first-episode", "2", "--belief-in", f)
    assert len(whole) == 5 and len(a) == 2 and len(b) == 3
    assert a + b == whole
    r = subprocess.run(common + ["--slots", "2", "--belief-out", f, "-f", str(tmp_path / "x.res")], capture_output=True, text=True)
    assert r.returncode == 1 and "--belief-out needs runs <= slots" in r.stderr
