"""What fba_probe costs a tick, on the two shapes of scripts/bench_belief_forecast.py:

  history   gridworld --size 7 FBA-POMDP, importance filter, history records, 16 384 particles x 256 slots, 20 warm-up ticks
  dense     collision avoidance 7 x 7 x 2, importance filter, fp32 records, 4 096 particles x 256 slots, 3 warm-up ticks

Per shape two contexts are created alike, one with the probe on all slots, and driven alike: the warm-up ticks, then the timed ticks (host
clock around fba_run_ticks, which ends in a synchronise).  The probe reads only, so both contexts hold the same filters tick for tick and
their times compare like for like; the pair is run twice, alternating, and every time is printed.  Prints one JSON line per shape: the
tick times, the bytes the probe's kernels have to move by the stated formula, and the records' evidence -- kernel times come from
running this script under `rocprofv3 --kernel-trace --stats`.

  python3 scripts/bench_belief_probe.py [history|dense|both] [--slots 256] [--ticks 10] [--rounds 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_belief_forecast import SHAPES, layout_sizes   # noqa: E402  (the same shapes, by construction)


def probe_bytes(eng, entries):
    """bytes every record and weight once (the weights twice: the finish kernel's total), the accumulators and the record"""
    n, slots = eng.cfg.particles, eng.slots
    fixed = 3 * 8 * 3 + 56          # three fp64 accumulators raised, read, zeroed; one record
    if eng.particle_bytes >= 4 * eng.ncnt:
        return slots * (n * (eng.particle_bytes + 16) + fixed), "slots * (N * (Cs * 4 + 16) + 3 * 3 * 8 + 56)"
    words = 2 + entries
    stride = 64 if words <= 16 else (128 if words <= 32 else eng.particle_bytes)
    return slots * (n * (stride + 16) + fixed), "slots * (N * (stride + 16) + 3 * 3 * 8 + 56)"


def timed_ticks(fba, shape, slots, ticks, probed):
    eng = fba.Engine(shape["domain"], particles=shape["particles"], slots=slots, runs=1 << 20, seed=20261018, **shape["kw"])
    if probed:
        eng.probe_enable(capacity=(shape["ticks"] + ticks) * slots)
    eng.run_ticks(shape["ticks"])
    t0 = time.perf_counter()
    eng.run_ticks(ticks)
    dt = time.perf_counter() - t0
    recs = eng.probe() if probed else None
    sizes = (eng.particle_bytes, eng.S, layout_sizes(eng), probe_bytes(eng, shape["ticks"] + ticks // 2 if eng.particle_bytes < 4 * eng.ncnt else 0))
    steps = eng.counters().env_steps
    eng.close()
    return dt / ticks, recs, sizes, steps


def run(fba, name, slots, ticks, rounds):
    shape = SHAPES[name]
    off, on, recs, sizes, steps = [], [], None, None, []
    for _ in range(rounds):
        t, _, sizes, s0 = timed_ticks(fba, shape, slots, ticks, False)
        off.append(1e3 * t)
        t, recs, _, s1 = timed_ticks(fba, shape, slots, ticks, True)
        on.append(1e3 * t)
        steps.append((s0, s1))
    particle_bytes, S, (tl, rl, _), (nbytes, basis) = sizes
    timed = recs[recs["t"] >= 0]
    out = {
        "metric": "one tick with fba_probe off / on all slots",
        "shape": name, "domain": shape["domain"], "particles": shape["particles"], "slots": slots, "warmup_ticks": shape["ticks"], "timed_ticks": ticks,
        "particle_bytes": particle_bytes, "S": S, "TL": tl, "observation_rows": rl,
        "tick_ms_probe_off": off, "tick_ms_probe_on": on, "tick_ms_probe_off_best": min(off), "tick_ms_probe_on_best": min(on),
        "env_steps_off_on": steps,
        "probe_bytes_per_tick": nbytes, "probe_bytes_basis": basis,
        "records": int(timed.size), "seen": int(recs.seen),
        "evidence_mean": float(timed["evidence"].mean()), "evidence_min": float(timed["evidence"].min()),
        "log_evidence_per_step": float(np.log(timed["evidence"][timed["evidence"] > 0]).mean()),
        "posterior_of_the_true_state_mean": float(np.mean(timed["post_true"][timed["evidence"] > 0] / timed["evidence"][timed["evidence"] > 0])),
    }
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("shape", nargs="?", default="both", choices=["history", "dense", "both"])
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    import fba_pomdp_amd as fba
    for name in (("history", "dense") if args.shape == "both" else (args.shape,)):
        run(fba, name, args.slots, args.ticks, args.rounds)


if __name__ == "__main__":
    main()
