"""What fba_structure_stats costs a tick, on two shapes:

  gridworld  the shape of scripts/bench_gridworld_rejection.py: gridworld --size 7 FBA-POMDP, rejection filter, history records, 16 384
             particles, 49 152 slots under a search budget: the slots of one launch step at different (episode, t)
  ftiger     episodic-factored-tiger --size 3 FBA-POMDP, rejection filter, packed records, 4 096 particles, at the 163 840 slots of
             bench.py --workload c3: lock-step, nearly every slot of a launch lands in one bin

--sims shortens the searches (the statistics read filters, not trees: their cost does not depend on it), --slots the launch.

One process, one context per shape.  After the warm-up ticks, windows of `--ticks` run_ticks each alternate between the statistics off and
on, `--windows` of each, timed with a host clock around fba_run_ticks (which ends in a synchronise).  The statistics read only, so the
context runs the same experiment whichever windows are on.  Then `--windows` more windows with FBA_STRUCT_STATS_TIME=1, in which the engine
puts a HIP-event pair on its stream around the launches of a tick's struct_stats_slot_kernel and struct_stats_bins_kernel and waits for it:
the kernels' own time, kept out of the windows above because the wait serialises the tick.  Last, the same context's
fba_belief_structures(0, slots, top_k=0) with the same queries, `--windows` times by the host clock: it reads the same words and builds
the same table for every slot, and copies its answer to the host.  Prints one JSON line per shape: every window, the per-tick difference
of the means, the spread (largest minus smallest) among the windows of a kind, and the kernels' time per tick.

--off-only times the stats-off windows alone (a library named by FBA_LIB that predates the call: the control against the parent commit).

  python3 scripts/bench_structure_stats.py [gridworld|ftiger|both] [--slots N] [--sims N] [--ticks 3] [--windows 5] [--warmup 2] [--off-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "gridworld": dict(domain="gridworld", slots=49152, seed=20261003,
                      kw=dict(model=2, belief="rejection_sampling", size=7, structure_prior=2, sims=65536, particles=16384, horizon=20, episodes=2,
                              search_budget=16384, tree_buckets=32768)),
    "ftiger": dict(domain="episodic-factored-tiger", slots=163840,
                   kw=dict(model=2, belief="rejection_sampling", size=3, structure_prior=2, sims=16384, particles=4096, horizon=10, episodes=64)),
}


def window(eng, ticks):
    t0 = time.perf_counter()
    eng.run_ticks(ticks)
    return 1e3 * (time.perf_counter() - t0) / ticks


def queries(eng):
    """three legal graphs: no parent beyond the node itself ... every candidate (history records hold the words 3 and 7 only)"""
    import numpy as np
    nw, ns = eng.structure_lens()
    if eng.particle_bytes < 1024 and nw == 2 * eng.A:
        return np.array([[3] * nw, [7] * nw, [3, 7] * (nw // 2)], np.uint32)
    return np.array([[0] * nw, [ns - 1] * nw, [1] * nw], np.uint32)


def run(fba, name, slots, sims, ticks, windows, warmup, off_only, belief=None):
    import ctypes as C
    shape = SHAPES[name]
    slots = slots or shape["slots"]
    kw = dict(shape["kw"])
    if belief:
        kw["belief"] = belief
    if sims:
        kw["sims"] = sims
        if "search_budget" in kw:
            kw["search_budget"] = min(kw["search_budget"], max(sims // 4, 1))
            kw["tree_buckets"] = 0
    os.environ.pop("FBA_STRUCT_STATS_TIME", None)
    eng = fba.Engine(shape["domain"], slots=slots, runs=1 << 30, seed=shape.get("seed", 20261021), **kw)
    eng.run_ticks(warmup)
    off, on = [], []
    Q = None if off_only else queries(eng)
    for _ in range(windows):
        off.append(window(eng, ticks))
        if off_only:
            continue
        eng.structure_stats_enable(Q)
        on.append(window(eng, ticks))
        st = eng.structure_stats()
        eng.structure_stats_enable(on=False)
    out = {"metric": "one tick with fba_structure_stats off / on", "shape": name, "domain": shape["domain"], "slots": eng.slots, **kw,
           "warmup_ticks": warmup, "ticks_per_window": ticks, "tick_ms_off": off, "tick_ms_off_mean": statistics.mean(off), "tick_ms_off_spread": max(off) - min(off)}
    if not off_only:
        os.environ["FBA_STRUCT_STATS_TIME"] = "1"
        eng.structure_stats_enable(Q)
        timed = [window(eng, ticks) for _ in range(windows)]
        ms, launches = C.c_double(), C.c_uint64()
        eng._chk(eng.L.fba_debug_structure_stats_ms(eng.h, C.byref(ms), C.byref(launches)))
        os.environ.pop("FBA_STRUCT_STATS_TIME", None)
        bins = int((eng.structure_stats().head["steps"] > 0).sum())
        eng.structure_stats_enable(on=False)
        call = []
        for _ in range(windows + 1):      # (the first call allocates: dropped)
            t0 = time.perf_counter()
            eng.belief_structures(0, eng.slots, top_k=0, queries=Q)
            call.append(1e3 * (time.perf_counter() - t0))
        call = call[1:]
        diff = statistics.mean(on) - statistics.mean(off)
        out.update({"queries": len(Q), "structure_lens": list(eng.structure_lens()),
                    "tick_ms_on": on, "tick_ms_on_mean": statistics.mean(on), "tick_ms_on_spread": max(on) - min(on), "tick_ms_difference": diff,
                    "steps_in_the_last_on_window": int(st.head["steps"].sum()), "bins_met_in_the_timed_windows": bins,
                    "tick_ms_event_timed_windows": timed, "timed_ticks": launches.value, "kernels_ms_per_tick": ms.value / max(launches.value, 1),
                    "belief_structures_call_ms": call, "belief_structures_call_ms_mean": statistics.mean(call),
                    "belief_structures_call_ms_spread": max(call) - min(call)})
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("shape", nargs="?", default="both", choices=["gridworld", "ftiger", "both"])
    ap.add_argument("--slots", type=int, default=0)
    ap.add_argument("--sims", type=int, default=0)
    ap.add_argument("--belief", default=None, help="the filter, where not the shape's own (a rejection filter ends the run where shortened searches walk it "
                                                   "to an observation no particle can produce)")
    ap.add_argument("--ticks", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--off-only", action="store_true")
    args = ap.parse_args()
    import fba_pomdp_amd as fba
    for name in (("gridworld", "ftiger") if args.shape == "both" else (args.shape,)):
        run(fba, name, args.slots, args.sims, args.ticks, args.windows, args.warmup, args.off_only, args.belief)


if __name__ == "__main__":
    main()
