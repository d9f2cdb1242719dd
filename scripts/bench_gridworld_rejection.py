"""BASELINE configs[3]'s shape (gridworld --size 7 FBA-POMDP, match-uniform structure prior, 65536 sims/step, 16384 particles, H = 20,
two episodes, budgeted searches on the bucket tree) with the reference's default belief, rejection sampling, run the way
`bench.py --workload c4` runs C4 -- history particles updated by reject_hist_kernel, the search in hist2_flat_search.  Steady-state
protocol of DESIGN.md section 5a: warm-up ticks, then timed ticks.  Prints one JSON line.

  python3 scripts/bench_gridworld_rejection.py [--slots 49152] [--warmup 20] [--steps 10]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C4 = dict(model=2, size=7, structure_prior=2, sims=65536, particles=16384, horizon=20, episodes=2, search_budget=16384, tree_buckets=32768)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slots", type=int, default=49152, help="concurrent runs (C4's: three search waves of 16 trees per SIMD); 0 = the engine's default")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--particles", type=int, default=None)
    ap.add_argument("--sims", type=int, default=None)
    args = ap.parse_args()

    import fba_pomdp_amd as fba
    w = dict(C4)
    for k in ("particles", "sims"):
        if getattr(args, k) is not None:
            w[k] = getattr(args, k)
    slots = args.slots
    while True:   # as bench.py: step down while this GPU cannot give the memory
        try:
            t_create = time.perf_counter()
            eng = fba.Engine("gridworld", belief="rejection_sampling", runs=1 << 30, slots=slots, seed=20261003, **w)
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
    upd, search = kt["reject_kernel"], kt["search_kernel"]
    out = {
        "metric": "simulated env steps/sec (belief+rollout)",
        "value": steps / dt,
        "unit": "steps/s",
        "workload": "configs[3] shape, rejection_sampling: gridworld --size 7, match-uniform, %d sims/step, %d particles, H=%d, %d episodes"
                    % (w["sims"], w["particles"], w["horizon"], w["episodes"]),
        "protocol": f"{args.warmup} warm-up ticks, {args.steps} timed",
        "slots": eng.slots,
        "particle_bytes": eng.particle_bytes,
        "ms_per_tick": 1e3 * dt / args.steps,
        "search_ms_per_tick": search.ms / args.steps,
        "update_ms_per_tick": upd.ms / args.steps,
        "sim_steps": c1.sim_steps - c0.sim_steps,
        "belief_steps": c1.belief_steps - c0.belief_steps,
        "update": {
            "kernel": "reject_hist_kernel",
            "launches": int(upd.launches),
            "particles": int(upd.units),
            "attempts_per_particle": (c1.belief_steps - c0.belief_steps) / max(int(upd.units), 1),
            "bytes": int(upd.bytes),
            "bytes_basis": "fba_kernel_times: attempts x 8 + particles x 20 + 4 x entries (DESIGN.md section 5a); rows from LDS",
            "GB_per_s": (upd.bytes / 1e9) / (upd.ms / 1e3) if upd.ms > 0 else 0.0,
        },
        "search_steps_per_s": search.units / (search.ms / 1e3) if search.ms > 0 else 0.0,
        "create_s": t_create,
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
