"""What fba_step_stats costs a tick, on two shapes:

  headline   episodic-tiger BA-table, rejection filter, 4 096 simulations x 4 096 particles, 262 144 slots in lock-step: nearly every slot
             of a launch lands in one bin
  budgeted   gridworld --size 3 FBA-POMDP, importance filter, history records, 256 simulations x 256 particles, 4 096 slots under a search
             budget: the slots of one launch step at different (episode, t)

One process, one context per shape.  After the warm-up ticks, windows of `--ticks` run_ticks each alternate between the statistics off and
on, `--windows` of each, timed with a host clock around fba_run_ticks (which ends in a synchronise).  The statistics read only, so the
context runs the same experiment whichever windows are on.  Then `--windows` more windows with FBA_STEP_STATS_TIME=1, in which the engine
puts a HIP-event pair around every launch of step_stats_kernel and waits for it: the kernel's own time, kept out of the windows above
because the wait serialises the tick.  Prints one JSON line per shape: every window, the per-tick difference of the means, the spread
(largest minus smallest) among the windows of a kind, and the kernel's time per launch.  Budget: 1 % of the stats-off tick.

--off-only times the stats-off windows alone (a library named by FBA_LIB that predates the call: the control against the parent commit).

  python3 scripts/bench_step_stats.py [headline|budgeted|both] [--slots N] [--ticks 3] [--windows 5] [--warmup 2] [--off-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "headline": dict(domain="episodic-tiger", slots=262144,
                     kw=dict(model=1, belief="rejection_sampling", sims=4096, particles=4096, horizon=10, episodes=20)),
    "budgeted": dict(domain="gridworld", slots=4096,
                     kw=dict(model=2, belief="importance_sampling", size=3, structure_prior=2, sims=256, particles=256, horizon=10, episodes=4,
                             search_budget=256)),
}


def window(eng, ticks):
    t0 = time.perf_counter()
    eng.run_ticks(ticks)
    return 1e3 * (time.perf_counter() - t0) / ticks


def run(fba, name, slots, ticks, windows, warmup, off_only):
    import ctypes as C
    shape = SHAPES[name]
    slots = slots or shape["slots"]
    os.environ.pop("FBA_STEP_STATS_TIME", None)
    eng = fba.Engine(shape["domain"], slots=slots, runs=1 << 30, seed=20261021, **shape["kw"])
    eng.run_ticks(warmup)
    off, on = [], []
    for _ in range(windows):
        off.append(window(eng, ticks))
        if off_only:
            continue
        eng.step_stats_enable()
        on.append(window(eng, ticks))
        st = eng.step_stats()
        eng.step_stats_enable(False)
    out = {"metric": "one tick with fba_step_stats off / on", "shape": name, "domain": shape["domain"], "slots": eng.slots, **shape["kw"],
           "warmup_ticks": warmup, "ticks_per_window": ticks, "tick_ms_off": off, "tick_ms_off_mean": statistics.mean(off), "tick_ms_off_spread": max(off) - min(off)}
    if not off_only:
        os.environ["FBA_STEP_STATS_TIME"] = "1"
        eng.step_stats_enable()
        timed = [window(eng, ticks) for _ in range(windows)]
        ms, launches = C.c_double(), C.c_uint64()
        eng._chk(eng.L.fba_debug_step_stats_ms(eng.h, C.byref(ms), C.byref(launches)))
        os.environ.pop("FBA_STEP_STATS_TIME", None)
        bins = int((eng.step_stats()["steps"] > 0).sum())
        diff = statistics.mean(on) - statistics.mean(off)
        out.update({"tick_ms_on": on, "tick_ms_on_mean": statistics.mean(on), "tick_ms_on_spread": max(on) - min(on),
                    "tick_ms_difference": diff, "budget_ms": 0.01 * statistics.mean(off), "within_budget": diff <= 0.01 * statistics.mean(off),
                    "steps_in_the_last_on_window": int(st["steps"].sum()), "bins_met_in_the_timed_windows": bins,
                    "tick_ms_event_timed_windows": timed, "kernel_launches": launches.value,
                    "kernel_ms_per_launch": ms.value / max(launches.value, 1),
                    "kernel_share_of_budget": (ms.value / max(launches.value, 1)) / (0.01 * statistics.mean(off))})
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("shape", nargs="?", default="both", choices=["headline", "budgeted", "both"])
    ap.add_argument("--slots", type=int, default=0)
    ap.add_argument("--ticks", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--off-only", action="store_true")
    args = ap.parse_args()
    import fba_pomdp_amd as fba
    for name in (("headline", "budgeted") if args.shape == "both" else (args.shape,)):
        run(fba, name, args.slots, args.ticks, args.windows, args.warmup, args.off_only)


if __name__ == "__main__":
    main()
