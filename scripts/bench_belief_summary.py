"""One fba_belief_summary over every slot of a context, all outputs, against what a host had before it: fba_belief_get of a slot
reduced in numpy.  Two shapes:

  history   gridworld --size 7 FBA-POMDP, importance filter, history records, 16 384 particles x 256 slots, 20 ticks run first
  dense     collision avoidance 7 x 7 x 2, importance filter, fp32 records, 4 096 particles x 256 slots, 3 ticks run first

Prints one JSON line per shape: wall time of the call (host clock around it; the call synchronises), the bytes it moved by the
stated formula and their share of the 8 TB/s peak OVER THE WALL TIME OF THE CALL -- which also holds two device allocations and the
copy of the results to the host; kernel times come from running this script under `rocprofv3 --kernel-trace --stats` --, and the
host path's time for one slot of 256 particles SCALED linearly to the shape (stated as scaled: nobody would wait for it).

  python3 scripts/bench_belief_summary.py [history|dense|both] [--slots 256] [--repeats 5] [--no-host-path]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12
SHAPES = {
    "history": dict(domain="gridworld", kw=dict(model=2, belief="importance_sampling", size=7, structure_prior=2, sims=64, horizon=20, episodes=2),
                    particles=16384, ticks=20),
    "dense": dict(domain="random-collision-avoidance", kw=dict(model=2, belief="importance_sampling", width=7, height=7, size=2, sims=64, horizon=20,
                                                               episodes=2), particles=4096, ticks=3),
}


def formula_bytes(eng, fba, entries):
    """bytes one call moves per the formulas of DESIGN.md section 5a"""
    n, slots, c, s = eng.cfg.particles, eng.slots, eng.ncnt, eng.S
    nm = eng.factored_layout().n_mask_words
    out = (c + s + 8 * nm + 3) * 8                        # results written once
    if eng.particle_bytes >= 4 * c:                         # fp32 records: every record once, every weight once
        return slots * (n * (eng.particle_bytes + 8) + out), "slots * (N * (Cs * 4 + 8) + results)"
    words = 2 + entries
    stride = 64 if words <= 16 else (128 if words <= 32 else eng.particle_bytes)
    # records and weights read by the head pass and by the scatter pass; the fp64 table zeroed, raised by 6 atomics of 8 B per entry
    # and particle, and read and written once more by the prior pass
    return slots * (2 * n * (stride + 8) + 3 * c * 8 + n * entries * 6 * 8 + out), \
        "slots * (2 * N * (stride + 8) + 3 * C * 8 + N * entries * 6 * 8 + results)"


def host_path_seconds(fba, shape, ticks):
    """fba_belief_get of one slot of 256 particles reduced in numpy: seconds per particle"""
    eng = fba.Engine(shape["domain"], particles=256, slots=1, runs=1 << 20, seed=20261018, **shape["kw"])
    eng.run_ticks(ticks)
    eng.belief_get(0)
    t0 = time.perf_counter()
    s, w, cnt = eng.belief_get(0)
    total = w.sum()
    mean = (w[:, None] * cnt.astype(np.float64)).sum(axis=0) / total
    mass = np.bincount(s, weights=w, minlength=eng.S)
    dt = time.perf_counter() - t0
    eng.close()
    return dt / 256, float(mean.sum() + mass.sum())


def run(fba, name, slots, repeats, host_path):
    shape = SHAPES[name]
    eng = fba.Engine(shape["domain"], particles=shape["particles"], slots=slots, runs=1 << 20, seed=20261018, **shape["kw"])
    eng.run_ticks(shape["ticks"])
    eng.belief_summary()                                   # warm-up: code objects, allocator
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        summ = eng.belief_summary()
        times.append(time.perf_counter() - t0)
    entries = shape["ticks"] if name == "history" else 0   # (every slot has taken that many updates unless an episode ended on the way)
    nbytes, basis = formula_bytes(eng, fba, entries)
    best = min(times)
    out = {
        "metric": "one fba_belief_summary over all slots, all outputs",
        "shape": name, "domain": shape["domain"], "particles": shape["particles"], "slots": eng.slots, "ticks_before": shape["ticks"],
        "particle_bytes": eng.particle_bytes, "counts_len": eng.ncnt,
        "call_ms": [1e3 * t for t in times], "call_ms_best": 1e3 * best,
        "bytes": nbytes, "bytes_basis": basis, "result_bytes_to_host": eng.slots * (eng.ncnt + eng.S) * 8,
        "fraction_of_8TBps_over_call_wall_time": nbytes / best / PEAK,
        "ess_mean": float(np.mean(summ.ess)), "weight_total_mean": float(np.mean(summ.weight_total)),
    }
    if host_path:
        per_particle, _ = host_path_seconds(fba, shape, shape["ticks"])
        out["host_path"] = {"what": "fba_belief_get of one slot of 256 particles + numpy, SCALED linearly (not measured at this size)",
                            "seconds_per_particle": per_particle,
                            "scaled_seconds": per_particle * shape["particles"] * eng.slots}
    print(json.dumps(out), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("shape", nargs="?", default="both", choices=["history", "dense", "both"])
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host-path", action="store_true")
    args = ap.parse_args()
    import fba_pomdp_amd as fba
    for name in (("history", "dense") if args.shape == "both" else (args.shape,)):
        run(fba, name, args.slots, args.repeats, not args.no_host_path)


if __name__ == "__main__":
    main()
