"""A resumed span measured: the restore of an experiment start in which every slot takes a snapshot block as its filter
(fba_run_bapomdp_span, restore_kernel), on the shapes profiles/r14_belief_snapshot.jsonl has for fba_belief_replicate and one more:

  history   gridworld --size 7 FBA-POMDP, importance filter, history records, 16 384 particles x 256 slots
  dense     collision avoidance 7 x 7 x 2, importance filter, fp32 records, 4 096 particles x 256 slots
  tiger     episodic tiger BA-POMDP, rejection filter, packed 64-byte records, 4 096 particles x 256 slots

Per shape one JSON line.  A learned filter is made first: one run of the experiment's first span, episodes * horizon = 40 steps of room,
exported from slot 0.  Then a context of `slots` runs whose episodes are ONE step long resumes its last episode from that one block
(nblocks = 1): the call is an experiment start, in which every slot restores, and a single tick.

  restore     the FBA_K_BELIEF_INIT bucket of that call, HIP events around the launches through fba_get_kernel_times: TWO launch
              sequences -- the start's, which moves every slot's filter, and the tick's, which finds no slot starting a run -- so the
              figure holds one idle launch pair and is not corrected for it (`init` below holds the same pair).  bytes = 2 * slots *
              particles * (stride + 8 if weighted), read and written (the library's own count); rates on those bytes and, for
              comparison with replicate's GB/s WRITTEN, on half of them
  init        the same bucket of the same call from the prior (blocks = NULL, span [0, 1)): what Belief::initiate costs there
  replicate   fba_belief_replicate of slot 0 into the others in the same process, host clock around the call as
              scripts/bench_belief_snapshot.py times it: the yardstick on the same bytes, same box, same minute
  `--repeats` contexts are not rebuilt: the resumed call is repeated on one context, after one warm-up call.

`--plain N` instead times N uninterrupted fba_run_bapomdp calls of the shape (wall clock around the call, which ends in a
synchronise) and prints them: run under two builds of the library (FBA_LIB names another), alternating, it says whether a plain
experiment costs what it cost before.

  python3 scripts/bench_belief_resume.py [history|dense|tiger|all] [--slots 256] [--repeats 5] [--plain 0]
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = 40      # episodes * horizon of every context of a shape: the room of its records
SHAPES = {
    "history": dict(domain="gridworld", kw=dict(model=2, belief="importance_sampling", size=7, structure_prior=2, sims=64), particles=16384, learn=20),
    "dense": dict(domain="random-collision-avoidance", kw=dict(model=2, belief="importance_sampling", width=7, height=7, size=2, sims=64),
                  particles=4096, learn=3),
    "tiger": dict(domain="episodic-tiger", kw=dict(model=1, belief="rejection_sampling", sims=64), particles=4096, learn=20),
}
SEED = 20261019


def spread(xs):
    s = sorted(xs)
    return {"all": xs, "min": s[0], "median": s[len(s) // 2], "max": s[-1]}


def learned_block(fba, shape):
    """the filter of one run after an episode of `learn` steps at most, as exported"""
    eng = fba.Engine(shape["domain"], particles=shape["particles"], slots=1, runs=1, seed=SEED, horizon=shape["learn"], episodes=STEPS // shape["learn"],
                     **shape["kw"])
    eng.run_bapomdp(0, 1)
    block = eng.belief_export(0, 1)
    eng.close()
    return block


def bucket(eng, call):
    eng.reset_kernel_times()
    t0 = time.perf_counter()
    call()
    wall = time.perf_counter() - t0
    kt = eng.kernel_times()["init_kernel"]
    return dict(ms=kt.ms, launches=int(kt.launches), units=int(kt.units), bytes=int(kt.bytes), wall_ms=1e3 * wall)


def run(fba, name, slots, repeats):
    shape = SHAPES[name]
    block = learned_block(fba, shape)
    head = np.ascontiguousarray(block[:, :64]).view(fba._native.SNAPSHOT_HEAD_DTYPE).reshape(-1)[0]
    eng = fba.Engine(shape["domain"], particles=shape["particles"], slots=slots, runs=slots, seed=SEED, horizon=1, episodes=STEPS, **shape["kw"])
    n, weighted, stride = eng.cfg.particles, int(head["weighted"]), int(head["stride"])
    out = {"metric": "resumed span: the restore of an experiment start in which every slot takes a snapshot block", "shape": name,
           "domain": shape["domain"], "particles": n, "slots": eng.slots, "particle_bytes": eng.particle_bytes, "record_format": int(head["record_format"]),
           "block_stride": stride, "weighted": weighted, "entries_or_updates_in_the_block": int(head["updates"]) if head["record_format"] < 5 else
           int(sum((int(head["hist_cnt"]) >> (8 * a)) & 0xff for a in range(4)))}
    resume = lambda: eng.run_bapomdp(STEPS - 1, STEPS, block)
    prior = lambda: eng.run_bapomdp(0, 1)
    resume(), prior()       # warm-up of both paths
    r = [bucket(eng, resume) for _ in range(repeats)]
    p = [bucket(eng, prior) for _ in range(repeats)]
    nbytes = r[0]["bytes"]
    assert nbytes == 2 * eng.slots * n * (stride + 8 * weighted) and r[0]["units"] == eng.slots * n, (nbytes, r[0])
    ms = spread([x["ms"] for x in r])
    out["restore"] = dict(bucket_ms=ms, launches_in_the_bucket=r[0]["launches"], bytes_read_and_written=nbytes,
                          bytes_basis="2 * slots * N * (stride + 8 if weighted)", GBps_at_median=nbytes / ms["median"] / 1e6,
                          GBps_written_at_median=nbytes / 2 / ms["median"] / 1e6, call_wall_ms=spread([x["wall_ms"] for x in r]))
    out["init_from_the_prior"] = dict(bucket_ms=spread([x["ms"] for x in p]), launches_in_the_bucket=p[0]["launches"],
                                      call_wall_ms=spread([x["wall_ms"] for x in p]))
    # the yardstick: slot 0 into the others, timed as scripts/bench_belief_snapshot.py times it
    eng.belief_import(0, block)
    for _ in range(2):
        eng.belief_replicate(0, 0, eng.slots)
    t = []
    for _ in range(max(repeats, 5)):
        t0 = time.perf_counter()
        eng.belief_replicate(0, 0, eng.slots)
        t.append(1e3 * (time.perf_counter() - t0))
    wrote = (eng.slots - 1) * n * (stride + 8 * weighted)
    tt = spread(t)
    out["replicate_yardstick"] = dict(wall_ms=tt, bytes_written=wrote, GBps_written_at_median=wrote / tt["median"] / 1e6,
                                      timing="host clock around the call, which ends in a stream synchronise and holds three small flag downloads")
    out["restore_over_replicate_written_rate"] = out["restore"]["GBps_written_at_median"] / out["replicate_yardstick"]["GBps_written_at_median"]
    eng.close()
    print(json.dumps(out), flush=True)


def plain(fba, name, slots, times):
    shape = SHAPES[name]
    eng = fba.Engine(shape["domain"], particles=shape["particles"], slots=slots, runs=slots, seed=SEED, horizon=10, episodes=2, **shape["kw"])
    eng.run_bapomdp()       # warm-up
    t = []
    for _ in range(times):
        t0 = time.perf_counter()
        eng.run_bapomdp()
        t.append(1e3 * (time.perf_counter() - t0))
    ret, _ = eng.returns()
    print(json.dumps({"metric": "plain fba_run_bapomdp, wall ms per call (2 episodes x horizon 10)", "shape": name, "library": fba._native.LIB_PATH,
                      "particles": eng.cfg.particles, "slots": eng.slots, "wall_ms": spread(t), "returns_crc32": zlib.crc32(ret.tobytes())}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("shape", nargs="?", default="all", choices=list(SHAPES) + ["all"])
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--plain", type=int, default=0)
    args = ap.parse_args()
    import fba_pomdp_amd as fba
    for name in (tuple(SHAPES) if args.shape == "all" else (args.shape,)):
        if args.plain:
            plain(fba, name, args.slots, args.plain)
        else:
            run(fba, name, args.slots, args.repeats)


if __name__ == "__main__":
    main()
