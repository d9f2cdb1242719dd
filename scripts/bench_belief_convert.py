"""fba_belief_convert measured: 256 snapshot blocks refitted to another context, on the shapes of scripts/bench_belief_resume.py:

  history   gridworld --size 7 FBA-POMDP, importance filter, history records; source records with room for 20 entries (96 bytes),
            destination with room for 40 (176 bytes): 16 384 particles re-roomed only, 16 384 -> 4 096, 4 096 -> 16 384
  dense     collision avoidance 7 x 7 x 2, importance filter, fp32 records: 4 096 -> 1 024 particles
  tiger     episodic tiger BA-POMDP, rejection filter, packed 64-byte records, 4 096 particles: the identity

Per conversion one JSON line.  A learned filter is made first (one run of one episode in a one-slot source context) and its block is
repeated 256 times on the host; weighted blocks get unequal weights, so that the pick is not the trivial one.  Then, after one warm-up,
five timed calls:

  call        host clock around fba_belief_convert: upload of the source blocks from pageable memory, the kernels, download of the
              destination blocks, a chunk of both sides at a time under the staging bound
  kernels     HIP events around the launches of every chunk (validation of the source, prefix sums, the convert kernel), summed over
              the chunks: fba_debug_convert_kernel_ms; the validation's part of it (fba_debug_convert_validate_ms, which reads every
              source block whole) and the rest, scan and convert kernel, apart
  written     bytes = blocks * destination particles * (stride + 8 if weighted); rate on the kernels' time
  replicate   fba_belief_replicate of slot 0 into the 255 others of a 256-slot destination context that has imported the converted
              blocks, host clock around the call as scripts/bench_belief_snapshot.py times it: bytes written and rate, for comparison

  python3 scripts/bench_belief_convert.py [history|dense|tiger|all] [--blocks 256] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 20261020
HIST = dict(domain="gridworld", kw=dict(model=2, belief="importance_sampling", size=7, structure_prior=2, sims=64, horizon=20))
DENSE = dict(domain="random-collision-avoidance", kw=dict(model=2, belief="importance_sampling", width=7, height=7, size=2, sims=64, horizon=20, episodes=2))
TIGER = dict(domain="episodic-tiger", kw=dict(model=1, belief="rejection_sampling", sims=64, horizon=20, episodes=2))
# name: (shape, source particles and overrides, destination particles and overrides)
CASES = {
    "history": [("re-room only", HIST, 16384, dict(episodes=1), 16384, dict(episodes=2)),
                ("16384 -> 4096", HIST, 16384, dict(episodes=1), 4096, dict(episodes=2)),
                ("4096 -> 16384", HIST, 4096, dict(episodes=1), 16384, dict(episodes=2))],
    "dense": [("4096 -> 1024", DENSE, 4096, {}, 1024, {})],
    "tiger": [("identity", TIGER, 4096, {}, 4096, {})],
}


def spread(xs):
    s = sorted(xs)
    return {"all": xs, "min": s[0], "median": s[len(s) // 2], "max": s[-1]}


def learned_blocks(fba, shape, particles, over, count):
    """one run's filter after its first episode, as exported, `count` times; weighted blocks with unequal weights"""
    N = fba._native
    kw = dict(shape["kw"], **over)
    eng = fba.Engine(shape["domain"], particles=particles, slots=1, runs=1, seed=SEED, **kw)
    eng.run_bapomdp(0, 1)
    block = eng.belief_export(0, 1)
    eng.close()
    head = np.ascontiguousarray(block[:, :64]).view(N.SNAPSHOT_HEAD_DTYPE).reshape(-1)[0]
    if head["weighted"]:
        w = np.random.default_rng(SEED).random(particles) + 0.05
        block[0, 64:64 + 8 * particles] = np.frombuffer(w.astype("<f8").tobytes(), np.uint8)
        block[0, 56:64] = np.frombuffer(np.uint64(N.snapshot_checksum(block[0, 64:])).tobytes(), np.uint8)
    return np.ascontiguousarray(np.repeat(block, count, axis=0)), head


def run(fba, name, what, shape, n_src, over_src, n_dst, over_dst, count, repeats):
    N = fba._native
    src, shead = learned_blocks(fba, shape, n_src, over_src, count)
    eng = fba.Engine(shape["domain"], particles=n_dst, slots=count, runs=count, seed=SEED, **dict(shape["kw"], **over_dst))
    per = eng.belief_snapshot_bytes
    dst = np.zeros(count * per, np.uint8)
    L = eng.L
    call = lambda: eng._chk(L.fba_belief_convert(eng.h, count, src.ctypes.data, src.nbytes, SEED, 0, dst.ctypes.data, dst.nbytes))
    call()      # warm-up
    t_call, t_kern, t_val = [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        t_call.append(1e3 * (time.perf_counter() - t0))
        t_kern.append(L.fba_debug_convert_kernel_ms())
        t_val.append(L.fba_debug_convert_validate_ms())
    out_blocks = dst.reshape(count, per)
    dhead = np.ascontiguousarray(out_blocks[:, :64]).view(N.SNAPSHOT_HEAD_DTYPE).reshape(-1)[0]
    weighted, stride = int(dhead["weighted"]), int(dhead["stride"])
    wrote = count * n_dst * (stride + 8 * weighted)
    kern, wall = spread(t_kern), spread(t_call)
    conv = spread([k - v for k, v in zip(t_kern, t_val)])
    src_payload = count * (int(src.shape[1]) - 64)
    stage = int(os.environ.get("FBA_SNAPSHOT_STAGE_BYTES", 256 << 20))
    out = {"metric": "fba_belief_convert: snapshot blocks refitted to another context", "shape": name, "conversion": what, "domain": shape["domain"],
           "blocks": count, "record_format": int(dhead["record_format"]), "weighted": weighted,
           "source": {"particles": n_src, "particle_bytes": int(shead["particle_bytes"]), "stride": int(shead["stride"]), "block_bytes": int(src.shape[1])},
           "destination": {"particles": n_dst, "particle_bytes": int(dhead["particle_bytes"]), "stride": stride, "block_bytes": per},
           "entries_or_updates_in_a_block": int(shead["updates"]) if shead["record_format"] < 5 else int(sum((int(shead["hist_cnt"]) >> (8 * a)) & 0xff for a in range(4))),
           "staging_bound_bytes": stage, "call_wall_ms": wall, "kernels_ms": kern, "validate_ms": spread(t_val), "scan_and_convert_ms": conv,
           "validate_bytes_read": src_payload, "validate_GBps_read_at_median": src_payload / max(spread(t_val)["median"], 1e-9) / 1e6,
           "GBps_written_on_scan_and_convert_at_median": wrote / conv["median"] / 1e6,
           "kernels": "validation of the source blocks, prefix sums (weighted, another particle count), convert: HIP events around the launches, summed over the chunks",
           "bytes_written": wrote, "bytes_basis": "blocks * destination particles * (stride + 8 if weighted)",
           "GBps_written_on_the_kernels_at_median": wrote / kern["median"] / 1e6, "GBps_written_on_the_call_at_median": wrote / wall["median"] / 1e6,
           "bytes_uploaded_and_downloaded": int(src.nbytes + dst.nbytes)}
    # the blocks are ones the unchanged import takes; then the yardstick: slot 0 into the others, timed as scripts/bench_belief_snapshot.py times it
    eng.belief_import(0, out_blocks)
    out["import_takes_the_blocks_and_exports_them_again"] = bool(np.array_equal(eng.belief_export(), out_blocks))
    for _ in range(2):
        eng.belief_replicate(0, 0, count)
    t = []
    for _ in range(max(repeats, 5)):
        t0 = time.perf_counter()
        eng.belief_replicate(0, 0, count)
        t.append(1e3 * (time.perf_counter() - t0))
    rep = spread(t)
    rep_wrote = (count - 1) * n_dst * (stride + 8 * weighted)
    out["replicate_yardstick"] = dict(wall_ms=rep, bytes_written=rep_wrote, GBps_written_at_median=rep_wrote / rep["median"] / 1e6,
                                      timing="host clock around the call, which ends in a stream synchronise and holds three small flag downloads")
    out["convert_kernels_over_replicate_written_rate"] = out["GBps_written_on_the_kernels_at_median"] / out["replicate_yardstick"]["GBps_written_at_median"]
    out["scan_and_convert_over_replicate_written_rate"] = out["GBps_written_on_scan_and_convert_at_median"] / out["replicate_yardstick"]["GBps_written_at_median"]
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("shape", nargs="?", default="all", choices=list(CASES) + ["all"])
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import fba_pomdp_amd as fba
    for name in (tuple(CASES) if args.shape == "all" else (args.shape,)):
        for what, shape, n_src, over_src, n_dst, over_dst in CASES[name]:
            run(fba, name, what, shape, n_src, over_src, n_dst, over_dst, args.blocks, args.repeats)


if __name__ == "__main__":
    main()
