"""What fba_giveup_policy costs where nothing gives up.

  builds   the rejection kernels read their attempt limit from Problem where a constant stood.  `bench.py` (the default workload) and
           `bench.py --workload c3` as child processes, `--windows` of each per build, alternating between this build and the library
           named by --parent-lib (the parent commit's, built from its sources; bench.py loads it through FBA_LIB).  The difference of the
           means has to lie inside the spread between repeated windows of the parent itself.
  policy   one context per shape (the two workloads' own), windows of `--ticks` run_ticks alternating between FBA_GIVEUP_STOP and
           FBA_GIVEUP_RETIRE at the default limit, at which no update of these shapes gives up: the cost of retire_kernel, one launch of
           one thread per slot in every tick.

Prints one JSON line per workload and part.

  python3 scripts/bench_giveup.py [builds|policy|both] [--parent-lib FILE] [--windows 3] [--steps 8] [--warmup 2] [--ticks 3] [--slots N]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ("c2", "c3")      # c2 is what `python bench.py` runs


def bench_window(workload, steps, warmup, lib):
    env = dict(os.environ)
    env.pop("FBA_LIB", None)
    if lib:
        env["FBA_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--workload", workload],
                         env=env, stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode()
    line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    return line["ms_per_step"], line["value"], line["config"]["slots_per_gpu"]


def builds(args):
    for wl in WORKLOADS:
        ms = {"this": [], "parent": []}
        value = {"this": [], "parent": []}
        slots = None
        for _ in range(args.windows):
            for which, lib in (("parent", args.parent_lib), ("this", None)):
                m, v, slots = bench_window(wl, args.steps, args.warmup, lib)
                ms[which].append(m)
                value[which].append(v)
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        diff = statistics.mean(ms["this"]) - statistics.mean(ms["parent"])
        print(json.dumps({"metric": "bench.py ms_per_step, this build against the parent commit's", "workload": wl, "slots": slots, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step_parent": ms["parent"], "ms_per_step_this": ms["this"],
                          "mean_parent": statistics.mean(ms["parent"]), "mean_this": statistics.mean(ms["this"]),
                          "spread_parent": spread["parent"], "spread_this": spread["this"], "difference": diff,
                          "inside_the_parents_spread": abs(diff) <= spread["parent"],
                          "steps_per_s_parent": value["parent"], "steps_per_s_this": value["this"]}), flush=True)


def policy(args):
    import bench
    import fba_pomdp_amd as fba
    for wl in WORKLOADS:
        w = dict(bench.WORKLOADS[wl])
        slots = args.slots or w.get("slots") or 262144      # (c2: what bench.py makes of 256 CUs)
        eng = fba.Engine(w["domain"], slots=slots, runs=1 << 30, seed=20261021, **{k: w[k] for k in bench.ENGINE_KEYS if k in w})
        eng.run_ticks(args.warmup)
        ms = {"stop": [], "retire": []}
        for _ in range(args.windows):
            for pol in ("stop", "retire"):
                eng.giveup_policy(pol, 0)
                t0 = time.perf_counter()
                eng.run_ticks(args.ticks)
                ms[pol].append(1e3 * (time.perf_counter() - t0) / args.ticks)
        retired = eng.retired().seen
        diff = statistics.mean(ms["retire"]) - statistics.mean(ms["stop"])
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        print(json.dumps({"metric": "one tick under FBA_GIVEUP_STOP / FBA_GIVEUP_RETIRE with no retirement", "workload": wl, "slots": eng.slots,
                          "ticks_per_window": args.ticks, "warmup_ticks": args.warmup, "tick_ms_stop": ms["stop"], "tick_ms_retire": ms["retire"],
                          "mean_stop": statistics.mean(ms["stop"]), "mean_retire": statistics.mean(ms["retire"]), "spread_stop": spread["stop"],
                          "spread_retire": spread["retire"], "difference": diff, "inside_the_spread_of_stop": abs(diff) <= spread["stop"],
                          "retired": int(retired)}), flush=True)
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("part", nargs="?", default="both", choices=["builds", "policy", "both"])
    ap.add_argument("--parent-lib", default=None, help="libfba_hip.so built from the parent commit (builds)")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ticks", type=int, default=3)
    ap.add_argument("--slots", type=int, default=0)
    args = ap.parse_args()
    if args.part in ("builds", "both"):
        if not args.parent_lib or not os.path.exists(args.parent_lib):
            ap.error("builds needs --parent-lib FILE")
        builds(args)
    if args.part in ("policy", "both"):
        policy(args)


if __name__ == "__main__":
    main()
