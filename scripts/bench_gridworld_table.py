"""C4's shape (gridworld --size 7, 65536 sims/step, H = 20, two episodes, budgeted searches on the bucket tree) on the TABULAR BA-POMDP
(bapomdp -D gridworld, model = BA_TABLE), run the way `bench.py --workload c4` runs C4: history particles of state-index entries over the
prior's sparse rows, updated by is_multi_tab_step_kernel (importance) or reject_tab_hist_kernel (rejection), the search in search_tabhist_kernel.
Steady-state protocol of DESIGN.md section 5a: warm-up ticks, then timed ticks.  Prints one JSON line.

  python3 scripts/bench_gridworld_table.py --belief importance_sampling [--particles 16384] [--slots 49152] [--warmup 20] [--steps 10]
  python3 scripts/bench_gridworld_table.py --belief rejection_sampling  [--particles 1024]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C4 = dict(model=1, size=7, sims=65536, horizon=20, episodes=2, search_budget=16384, tree_buckets=32768)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--belief", choices=["importance_sampling", "rejection_sampling"], default="importance_sampling")
    ap.add_argument("--slots", type=int, default=49152, help="concurrent runs (C4's); 0 = the engine's default")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--particles", type=int, default=None, help="default: 16384 (importance), 1024 (rejection)")
    ap.add_argument("--sims", type=int, default=None)
    args = ap.parse_args()

    import fba_pomdp_amd as fba
    w = dict(C4)
    w["particles"] = args.particles or (16384 if args.belief == "importance_sampling" else 1024)
    if args.sims is not None:
        w["sims"] = args.sims
    slots = args.slots
    while True:   # as bench.py: step down while this GPU cannot give the memory
        try:
            t_create = time.perf_counter()
            eng = fba.Engine("gridworld", belief=args.belief, runs=1 << 30, slots=slots, seed=20261016, **w)
            t_create = time.perf_counter() - t_create
            break
        except fba.FbaError as e:
            if "out of memory" not in str(e) or slots <= 1024:
                raise
            print(f"[bench] {slots} slots do not fit ({e}); retrying with {slots // 2}", file=sys.stderr)
            slots //= 2

    eng.run_ticks(args.warmup)
    c0 = eng.counters()
    eng.reset_kernel_times()
    t0 = time.perf_counter()
    eng.run_ticks(args.steps)   # synchronises its HIP stream before returning
    dt = time.perf_counter() - t0
    c1 = eng.counters()
    kt = eng.kernel_times()
    steps = (c1.sim_steps - c0.sim_steps) + (c1.belief_steps - c0.belief_steps)
    rej = args.belief == "rejection_sampling"
    upd, search = kt["reject_kernel" if rej else "importance_kernel"], kt["search_kernel"]
    out = {
        "metric": "simulated env steps/sec (belief+rollout)",
        "value": steps / dt,
        "unit": "steps/s",
        "workload": "C4 shape, tabular BA-POMDP, %s: gridworld --size 7, %d sims/step, %d particles, H=%d, %d episodes"
                    % (args.belief, w["sims"], w["particles"], w["horizon"], w["episodes"]),
        "protocol": f"{args.warmup} warm-up ticks, {args.steps} timed",
        "slots": eng.slots,
        "particle_bytes": eng.particle_bytes,
        "ms_per_tick": 1e3 * dt / args.steps,
        "search_ms_per_tick": search.ms / args.steps,
        "update_ms_per_tick": upd.ms / args.steps,
        "sim_steps": c1.sim_steps - c0.sim_steps,
        "belief_steps": c1.belief_steps - c0.belief_steps,
        "update": {
            "kernel": "reject_tab_hist_kernel" if rej else "is_multi_tab_step_kernel + the multi-launch resample",
            "launches": int(upd.launches),
            "particles": int(upd.units),
            "bytes": int(upd.bytes),
            "bytes_basis": "fba_kernel_times (DESIGN.md section 5a); the prior's sparse rows are L2-resident and not counted",
            "GB_per_s": (upd.bytes / 1e9) / (upd.ms / 1e3) if upd.ms > 0 else 0.0,
        },
        "search_steps_per_s": search.units / (search.ms / 1e3) if search.ms > 0 else 0.0,
        "create_s": t_create,
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
