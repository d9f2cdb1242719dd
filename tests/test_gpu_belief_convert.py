"""fba_belief_convert (Engine.belief_convert): snapshot blocks of one context refitted to a context that differs in its particle count
or, for history records, in the room of a record (episodes * horizon), so that the unchanged fba_belief_import and fba_run_bapomdp_span
take them.  What became which particle is stated on the host (tests/convert_cases.py: expected_sources, built on the oracle's Philox and
device-order scan); filters are compared in table form (fba_belief_get) and as bytes, traces field by field.  Every comparison is of
bits; there is no tolerance anywhere in this file.  A refused call must leave the context as it was."""
import functools
import subprocess

import numpy as np
import pytest

import convert_cases as K
import fba_pomdp_amd as fba
import resume_cases as R
from fba_pomdp_amd import _native as N
from test_gpu_belief_resume import _engine, _environment, _heads, _outcome, _same_records, _same_span, _sorted

pytestmark = pytest.mark.gpu

IS = "importance_sampling"
FULL = R.STRIDE_FULL_ENV


def _weighted(name):
    return R.fmt_of(name)[4] == IS


def _tables(eng, name):
    """every slot's filter in table form, as bytes: states, weights (importance filters), counts"""
    out = []
    for e in range(eng.slots):
        s, w, cnt = eng.belief_get(e, weights=_weighted(name), counts=eng.ncnt > 0)
        out.append((s.tobytes(), w.tobytes() if _weighted(name) else b"", b"" if cnt is None else cnt.tobytes()))
    return out


def _key(env, over):
    return tuple(sorted((env or {}).items())), tuple(sorted(over.items()))


@functools.lru_cache(maxsize=None)
def _source_cached(name, stop, key):
    env, over = dict(key[0]), dict(key[1])
    eng = _engine(name, env, trace=1, **over)
    out = _outcome(eng, eng.run_bapomdp() if stop is None else eng.run_bapomdp(0, stop))
    out["blocks"] = eng.belief_export()
    out["tables"] = _tables(eng, name)
    eng.close()
    return out


def _source(name, stop=None, env=None, **over):
    """a context of the case run to its end (or through episodes [0, stop)): outcome, exported blocks and the filters in table form;
    computed once, shared, never changed"""
    return _source_cached(name, stop, _key(env, over))


def _blocks(raw, eng):
    return np.frombuffer(raw, np.uint8).reshape(-1, eng.belief_snapshot_bytes)


def _records(eng, name, blocks):
    """blocks of eng's own fingerprint, imported: the filters in table form, and the export behind the import"""
    eng.belief_import(0, blocks)
    return _tables(eng, name), eng.belief_export(0, len(blocks))


def _entries(heads):
    return sum((heads["hist_cnt"] >> np.uint32(8 * a)) & np.uint32(0xff) for a in range(4)).astype(np.int64)


# ---- 1. identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.IDENTITY)
def test_a_contexts_own_blocks_come_back_as_they_are(name):
    src = _source(name, 2)["blocks"]
    eng = _engine(name)
    for seed, first_run in ((0, 0), (977, 5), (2 ** 63 + 11, 2 ** 32 - 3)):
        assert eng.belief_convert(src, seed=seed, first_run=first_run) == src.tobytes(), (name, seed, first_run)
    assert eng.belief_convert(src.tobytes()) == src.tobytes() and fba.snapshot_block_bytes(src[0, :64]) == src.shape[1] == eng.belief_snapshot_bytes
    eng.close()


# ---- 2. more room, every stride pair ---------------------------------------------------------------------------------------------------
def _more_room(name, env):
    """the blocks of a 2-episode context, a 4-episode context and of a 5-episode context after one episode into the 5-episode context:
    the strides met on both sides"""
    sources = [("2 episodes", _source(name, None, env, episodes=K.SHORT)), ("4 episodes", _source(name, None, env, episodes=K.MIDDLE)),
               ("1 of 5 episodes", _source(name, 1, env))]
    dst = _engine(name, env)
    met_src, met_dst = set(), set()
    for what, src in sources:
        what = f"{name}, {what}"
        sh = _heads(src["blocks"])
        out = _blocks(dst.belief_convert(src["blocks"], seed=31), dst)
        dh = _heads(out)
        assert len(out) == len(src["blocks"]) and np.all(dh["particle_bytes"] == R.RECORD_BYTES) and np.all(dh["particles"] == R.PARTICLES), what
        assert np.array_equal(dh["hist_cnt"], sh["hist_cnt"]) and np.array_equal(dh["updates"], sh["updates"]), what
        full = bool(env)
        assert [int(s) for s in sh["stride"]] == [K.stride_in(int(sh["particle_bytes"][0]), int(n), full) for n in _entries(sh)], what
        assert [int(s) for s in dh["stride"]] == [K.stride_in(R.RECORD_BYTES, int(n), full) for n in _entries(sh)], what
        for b in range(len(out)):
            assert int(dh["checksum"][b]) == N.snapshot_checksum(out[b, 64:]), f"{what}: checksum of block {b}"
        tables, again = _records(dst, name, out)
        assert tables == src["tables"], f"{what}: states, weights and counts behind the import"
        assert np.array_equal(again, out), f"{what}: export(import(convert(x))) == convert(x)"
        met_src |= {int(s) for s in sh["stride"]}
        met_dst |= {int(s) for s in dh["stride"]}
    dst.close()
    return met_src, met_dst


@pytest.mark.parametrize("name", K.HISTORY)
def test_more_room_at_every_stride_pair(name):
    met_src, met_dst = _more_room(name, None)
    if name in K.GRIDWORLD_HISTORY:
        assert met_src >= {64, 80, 144} and met_dst == {64, 128, R.RECORD_BYTES}, (name, met_src, met_dst)
    else:       # (resume_cases.py: the plane makes 3 updates per episode at most, its records stay at 64 bytes)
        assert met_src == {64} and met_dst == {64}, (name, met_src, met_dst)


@pytest.mark.parametrize("name", K.HISTORY)
def test_more_room_with_whole_record_strides(name):
    met_src, met_dst = _more_room(name, FULL)
    assert met_src == {80, 144, R.RECORD_BYTES} and met_dst == {R.RECORD_BYTES}, (name, met_src, met_dst)


# ---- 3. learning longer than planned ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.LONGER)
def test_a_two_episode_experiment_continues_in_a_five_episode_context(name):
    short, whole = _source(name, None, episodes=K.SHORT), _source(name)
    eng = _engine(name, trace=1)
    fitted = _blocks(eng.belief_convert(short["blocks"], seed=5), eng)
    if name == "packed_tiger":
        assert np.array_equal(fitted, short["blocks"]), "packed records have no room to change: the conversion is the identity"
    else:
        assert fitted.shape[1] > short["blocks"].shape[1]
    got = _outcome(eng, eng.run_bapomdp(K.SHORT, None, fitted))
    got["blocks"] = eng.belief_export()
    eng.close()
    _same_span(got, whole, K.SHORT, R.EPISODES, f"{name}: episodes [2, 5) from the fitted blocks of a 2-episode experiment")
    assert np.array_equal(got["blocks"], whole["blocks"]), f"{name}: the final filters, as exported"
    # ... and the short experiment was the long one's first two episodes
    first = whole["trace"][whole["trace"]["episode"] < K.SHORT]
    _same_records(_sorted(short["trace"]), _sorted(first), f"{name}: the 2-episode experiment against episodes [0, 2) of the whole")


# ---- 4. less room ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.GRIDWORLD_HISTORY)
def test_less_room(name):
    one, four = _source(name, 1), _source(name, 4)
    eng = _engine(name, episodes=K.SHORT)
    assert eng.particle_bytes == K.ROOM_BYTES[K.SHORT]
    out = _blocks(eng.belief_convert(one["blocks"]), eng)
    assert [int(s) for s in _heads(out)["stride"]] == [K.stride_in(80, int(n)) for n in _entries(_heads(one["blocks"]))]
    tables, again = _records(eng, name, out)
    assert tables == one["tables"] and np.array_equal(again, out)
    entries = _entries(_heads(four["blocks"]))
    b = int(np.nonzero(entries > 16)[0][0])
    before = eng.belief_export()
    with pytest.raises(ValueError, match=rf"fba_belief_convert: block {b} holds {int(entries[b])} entries per record / room for 16"):
        eng.belief_convert(four["blocks"])
    assert np.array_equal(eng.belief_export(), before)
    eng.close()


# ---- 5. flat resampling --------------------------------------------------------------------------------------------------------------------
def _resampled_equals_the_sources(name, n_src, n_dst, src, seed, first_run, weights=None):
    """convert src (blocks and tables of an n_src-particle context, `weights` put into the blocks where given) into an n_dst-particle
    context: record j of block b, in table form behind an import, is record expected_sources(...)[j] of the source"""
    dst = _engine(name, particles=n_dst)
    blocks = src["blocks"] if weights is None else K.set_weights(src["blocks"], weights)
    out = _blocks(dst.belief_convert(blocks, seed=seed, first_run=first_run), dst)
    dh = _heads(out)
    assert np.all(dh["particles"] == n_dst) and np.array_equal(dh["hist_cnt"], _heads(blocks)["hist_cnt"])
    for b in range(len(out)):
        assert int(dh["checksum"][b]) == N.snapshot_checksum(out[b, 64:]), (name, b)
    tables, again = _records(dst, name, out)
    assert np.array_equal(again, out), f"{name} {n_src} -> {n_dst}: export(import(convert(x))) == convert(x)"
    repeats = missing = 0
    for b in range(len(out)):
        want = K.expected_sources(seed, first_run, b, n_src, n_dst, None if weights is None else weights[b])
        assert want.min() >= 0 and want.max() < n_src
        repeats += len(want) - len(np.unique(want))
        missing += n_src - len(np.unique(want))
        s, w, cnt = (np.frombuffer(x, dt) for x, dt in zip(src["tables"][b], ("<i4", "<u8", "<u4")))
        gs, gw, gcnt = (np.frombuffer(x, dt) for x, dt in zip(tables[b], ("<i4", "<u8", "<u4")))
        what = f"{name} {n_src} -> {n_dst}, block {b}"
        bad = np.nonzero(gs != s[want])[0]
        assert bad.size == 0, f"{what}: state of particle {bad[:1]}: {gs[bad[:1]]}, source {want[bad[:1]]} has {s[want[bad[:1]]]}"
        if cnt.size:
            assert np.array_equal(gcnt.reshape(n_dst, -1), cnt.reshape(n_src, -1)[want]), what + ": counts"
        if _weighted(name):
            if n_src == n_dst:
                assert np.array_equal(gw, np.ascontiguousarray(weights[b], "<f8").view("<u8") if weights is not None else w), what + ": weights kept"
            else:
                assert np.all(gw == np.float64(1.0 / n_dst).view(np.uint64)), what + ": every weight is 1.0 / N"
    dst.close()
    return repeats, missing


@pytest.mark.parametrize("n_src,n_dst", K.FLAT_COUNTS)
@pytest.mark.parametrize("name", K.FLAT)
def test_flat_resampling(name, n_src, n_dst):
    src = _source(name, 2, particles=n_src)
    repeats, missing = _resampled_equals_the_sources(name, n_src, n_dst, src, seed=4242, first_run=3)
    assert repeats > 0 and missing > 0, "the expected indices permute nothing: the case tests nothing"


# ---- 6. weighted resampling ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src,n_dst,zeros", [c + (False,) for c in K.WEIGHTED_COUNTS] + [(300, 37, True)])       # (True: a third of the weights 0.0)
@pytest.mark.parametrize("name", K.WEIGHTED)
def test_weighted_resampling(name, n_src, n_dst, zeros):
    src = _source(name, 2, particles=n_src)
    weights = K.random_weights(np.random.default_rng(1000 + n_src + n_dst), len(src["blocks"]), n_src, zeros)
    repeats, missing = _resampled_equals_the_sources(name, n_src, n_dst, src, seed=99, first_run=0, weights=weights)
    if n_src != n_dst:
        assert repeats > 0 and missing > 0, "the expected indices permute nothing: the case tests nothing"


@pytest.mark.parametrize("name", K.WEIGHTED)
def test_a_block_without_weight_cannot_be_sampled_from(name):
    src = _source(name, 2)
    weights = K.random_weights(np.random.default_rng(7), len(src["blocks"]), R.PARTICLES)
    weights[1] = 0.0
    blocks = K.set_weights(src["blocks"], weights)
    eng = _engine(name, particles=37)
    before = eng.belief_export()
    with pytest.raises(ValueError, match="fba_belief_convert: block 1: weights whose total is zero or not finite"):
        eng.belief_convert(blocks)
    assert np.array_equal(eng.belief_export(), before)
    eng.close()
    eng = _engine(name)      # the same particle count: taken, as an import takes it
    assert eng.belief_convert(blocks) == blocks.tobytes()
    eng.close()


# ---- 7. room and count at once ---------------------------------------------------------------------------------------------------------------
def test_room_and_count_at_once():
    name = "gridworld3_history_importance"
    src = _source(name, None, particles=300, episodes=K.SHORT)
    assert {int(s) for s in _heads(src["blocks"])["stride"]} == {64, 80}
    weights = K.random_weights(np.random.default_rng(12), len(src["blocks"]), 300)
    repeats, missing = _resampled_equals_the_sources(name, 300, R.PARTICLES, src, seed=8, first_run=1, weights=weights)
    assert repeats > 0 and missing > 0


# ---- 8. chunking -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_src", [("packed_tiger", 300), ("gridworld3_history_importance", 300), ("gridworld3_history_importance", 130)])
def test_chunking_changes_nothing(name, n_src):
    over = dict(slots=7, runs=7, particles=n_src) if name != "packed_tiger" else dict(particles=n_src)
    over_src = dict(over, episodes=K.SHORT) if name in K.HISTORY else over
    src = _source(name, None if name in K.HISTORY else 2, **over_src)["blocks"]
    assert len(src) == 7
    if _weighted(name):
        src = K.set_weights(src, K.random_weights(np.random.default_rng(3), 7, n_src))
    eng = _engine(name, slots=7, runs=7)
    whole = eng.belief_convert(src, seed=61)
    per = eng.belief_snapshot_bytes
    assert eng.belief_convert(src[:3], seed=61, first_run=0) + eng.belief_convert(src[3:], seed=61, first_run=3) == whole, "3 + 4 blocks"
    with _environment({"FBA_SNAPSHOT_STAGE_BYTES": str(2 * src.shape[1])}):
        assert eng.belief_convert(src, seed=61) == whole, "staging of two source blocks"
    with _environment({"FBA_SNAPSHOT_STAGE_BYTES": "1"}):
        assert eng.belief_convert(src, seed=61) == whole, "one block of each side at a time"
    assert len(whole) == 7 * per
    if n_src != R.PARTICLES:
        assert eng.belief_convert(src, seed=62) != whole and eng.belief_convert(src, seed=61, first_run=1) != whole
    eng.close()


# ---- 9. refusals and read-only -------------------------------------------------------------------------------------------------------------------
def _raw(eng, count, src, src_bytes, dst, dst_cap, seed=0, first_run=0):
    eng._chk(eng.L.fba_belief_convert(eng.h, count, None if src is None else src.ctypes.data, src_bytes, seed, first_run,
                                      None if dst is None else dst.ctypes.data, dst_cap))


def _resum(blocks, b):
    blocks[b, 56:64] = np.frombuffer(np.uint64(N.snapshot_checksum(blocks[b, 64:])).tobytes(), np.uint8)


def _put(blocks, b, offset, value, dtype):
    blocks[b, offset:offset + np.dtype(dtype).itemsize] = np.frombuffer(np.array(value, dtype).tobytes(), np.uint8)
    _resum(blocks, b)


@pytest.mark.parametrize("n_dst", [R.PARTICLES, 37])
def test_refusals_leave_the_context_untouched(n_dst):
    name = "gridworld3_history_importance"
    src = _source(name, None, episodes=K.SHORT)["blocks"]        # 130 particles, 80-byte records
    count, per_src = src.shape
    eng = _engine(name, trace=1, particles=n_dst)
    eng.run_bapomdp(0, 1)       # (filters to be left alone)
    before = eng.belief_export()
    dst = np.zeros(count * eng.belief_snapshot_bytes, np.uint8)

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            _raw(eng, *args, **kw)
        assert np.array_equal(eng.belief_export(), before), "a refused conversion changed a filter"

    refused("count 0", 0, src, src.nbytes, dst, dst.nbytes)
    refused("count -1", -1, src, src.nbytes, dst, dst.nbytes)
    refused("src null", count, None, src.nbytes, dst, dst.nbytes)
    refused("dst null", count, src, src.nbytes, None, dst.nbytes)
    both = np.zeros(src.nbytes + dst.nbytes, np.uint8)
    both[:src.nbytes] = src.reshape(-1)
    refused("overlap", count, both, src.nbytes, both[src.nbytes - 8:], dst.nbytes)
    refused(rf"bytes {src.nbytes - 8} / {src.nbytes} \({count} blocks of {per_src}\)", count, src, src.nbytes - 8, dst, dst.nbytes)
    refused(rf"bytes {src.nbytes} / {(count - 1) * per_src}", count - 1, src, src.nbytes, dst, dst.nbytes)
    refused(rf"need {dst.nbytes}, the buffer has {dst.nbytes - 1}", count, src, src.nbytes, dst, dst.nbytes - 1)
    # fingerprint: a block over another prior; a block of another room than the first
    other = src.copy()
    other[count - 2, 48] ^= 1
    refused(f"block {count - 2}: prior hash", count, other, other.nbytes, dst, dst.nbytes)
    other = src.copy()
    other[1, 24:28] = np.frombuffer(np.int32(144).tobytes(), np.uint8)
    refused("block 1: particle bytes 144 in the block, 80 in the first block", count, other, other.nbytes, dst, dst.nbytes)
    other = src.copy()
    other[2, 20:24] = np.frombuffer(np.int32(131).tobytes(), np.uint8)
    refused("block 2: particles 131 in the block, 130 in the first block", count, other, other.nbytes, dst, dst.nbytes)
    other = src.copy()
    other[0, 32:36] = np.frombuffer(np.int32(eng.S + 1).tobytes(), np.uint8)
    refused(f"block 0: states {eng.S + 1} in the block, {eng.S} in this context", count, other, other.nbytes, dst, dst.nbytes)
    # the device pass, against the source's own particle count and stride
    heads = _heads(src)
    records = 64 + R.PARTICLES * 8
    flipped = src.copy()
    flipped[count - 1, per_src - 100] ^= 0x10
    refused(f"block {count - 1}: checksum", count, flipped, flipped.nbytes, dst, dst.nbytes)
    bad = src.copy()
    _put(bad, 1, records + 5 * int(heads["stride"][1]), eng.S + 3, "<u4")
    refused("block 1, particle 5: a state outside the domain", count, bad, bad.nbytes, dst, dst.nbytes)
    b = int(np.argmax(_entries(heads)))
    assert int(heads["stride"][b]) == 80 and _entries(heads)[b] >= 15
    bad = src.copy()
    _put(bad, b, records + 129 * 80 + 8 + 4 * 14, 0x3fffffff, "<u4")       # entry 14 of the last particle: beyond 64 bytes, inside the 80
    refused(f"block {b}, particle 129: a history entry outside the domain's tables", count, bad, bad.nbytes, dst, dst.nbytes)
    bad = src.copy()
    _put(bad, 2, 64 + 8 * 77, -0.25, "<f8")
    refused("block 2, particle 77: a weight that is negative or not finite", count, bad, bad.nbytes, dst, dst.nbytes)
    # ---- a successful conversion changes nothing either: the run behind it is the run without it
    eng.belief_convert(src, seed=3)
    assert np.array_equal(eng.belief_export(), before)
    got = _outcome(eng, eng.run_bapomdp())
    eng.close()
    fresh = _engine(name, trace=1, particles=n_dst)
    fresh.run_bapomdp(0, 1)
    want = _outcome(fresh, fresh.run_bapomdp())
    fresh.close()
    _same_records(_sorted(got["trace"]), _sorted(want["trace"]), "a plain run behind the conversions")
    assert np.array_equal(got["returns"].view(np.uint64), want["returns"].view(np.uint64)) and got["stats"] == want["stats"]


@pytest.mark.parametrize("belief,kw,says", [
    ("reinvigoration", dict(resample_amount=8), "fully connected"), ("cheating-reinvigoration", dict(resample_amount=7, threshold=-1.5, structure_prior=1), "cheating"),
    ("incubator", dict(resample_amount=6, threshold=0.5), "incubator"), ("mh-within-gibbs", dict(threshold=-0.5, structure_prior=1), "history"),
    ("mh-nips", dict(threshold=-0.5, structure_prior=1), "history"), ("nested", {}, "nested")])
def test_beliefs_with_more_than_a_main_filter_are_refused(belief, kw, says):
    """(the configurations of the same test of test_gpu_belief_resume.py)"""
    args = dict(size=2, structure_prior=2, particles=12 if belief == "nested" else 48, sims=16, horizon=4, episodes=3, slots=3, runs=3, seed=8201)
    args.update(kw)
    model = N.MODEL_BA_TABLE if belief == "nested" else N.MODEL_BA_FACTORED
    if belief == "nested":
        args.pop("size"), args.pop("structure_prior")
    eng = fba.Engine("episodic-tiger" if belief == "nested" else "episodic-factored-tiger", model=model, belief=belief, **args)
    src, dst = np.zeros(4096, np.uint8), np.zeros(1 << 16, np.uint8)
    with pytest.raises(ValueError, match="fba_belief_convert: a snapshot holds the main filter of a slot, and .*" + says):
        _raw(eng, 1, src, src.nbytes, dst, dst.nbytes)
    eng.close()


# ---- 10. the command line ----------------------------------------------------------------------------------------------------------------------
def test_cli_fits_the_blocks_of_a_shorter_experiment(tmp_path):
    cli = fba.build_cli()
    common = [cli, "fbapomdp", "-D", "gridworld", "--size", "3", "--structure-prior", "match-uniform", "-B", "importance_sampling", "-s", "16",
              "--particle-amount", "130", "-H", "8", "--runs", "4", "--slots", "4", "--seed", "resume"]

    def run(tag, *args, ok=True):
        out = tmp_path / (tag + ".res")
        r = subprocess.run(common + ["-f", str(out)] + list(args), capture_output=True, text=True)
        if not ok:
            return r
        assert r.returncode == 0, r.stderr
        lines = [l for l in out.read_text().splitlines() if l and not l.startswith("#")]
        return [l.split(", ")[:4] for l in lines]       # (the fifth column is a time)

    whole = run("whole", "--episodes", "5")
    f = str(tmp_path / "beliefs.bin")
    a = run("a", "--episodes", "2", "--belief-out", f)
    b = run("b", "--episodes", "5", "--first-episode", "2", "--belief-in", f, "--belief-fit", "5")
    assert len(whole) == 5 and len(a) == 2 and len(b) == 3
    assert a + b == whole
    r = run("c", "--episodes", "5", "--first-episode", "2", "--belief-in", f, ok=False)
    assert r.returncode == 1 and "not a file of snapshot blocks of this configuration" in r.stderr
