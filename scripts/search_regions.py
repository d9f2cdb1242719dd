"""Where a wave of search_kernel spends its cycles: an instrumented build of the same sources (-DFBA_PROFILE_SEARCH:
clock64() marks between the regions of the search loop, summed per wave) run on the bench workload.
python scripts/search_regions.py build   (here: hipcc, no GPU needed)  ->  fba_pomdp_amd/libfba_hip_prof.so
python scripts/search_regions.py [slots] (on the GPU box)              ->  one JSON line
search_kernel also counts, per wave, its loop trips, the lanes that step in each and the boundary phases (back-up + next root sample) it
runs: lane-steps per wave-trip and boundary phases per simulation, under FBA_SEARCH_QUORUM=1..64 or the launch plan's default."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF = os.environ.get("FBA_PROF_LIB") or os.path.join(ROOT, "fba_pomdp_amd", "libfba_hip_prof.so")   # (FBA_PROF_LIB: another instrumented build, for A/B runs)
sys.path.insert(0, ROOT)

if len(sys.argv) > 1 and sys.argv[1] == "build":
    from fba_pomdp_amd import _native as N
    N.build(extra_flags=["-DFBA_PROFILE_SEARCH"], lib_path=PROF, obj_tag="_prof")
    print("built", PROF)
    sys.exit(0)

os.environ["FBA_LIB"] = PROF
import fba_pomdp_amd as fba  # noqa: E402
from fba_pomdp_amd import _native as N  # noqa: E402

cfg = os.environ.get("FBA_CFG", "c2")
slots = int(sys.argv[1]) if len(sys.argv) > 1 else (81920 if cfg == "c3" else 262144)
if cfg == "c4":      # BASELINE configs[3]: gridworld N = 7, history particles, four lanes per tree (search_hist_kernel)
    slots = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    kw = dict(size=7, sims=int(os.environ.get("FBA_SIMS", "65536")), particles=16384, structure_prior=2, horizon=20, episodes=2,
              search_budget=int(os.environ.get("FBA_BUDGET", "16384")), tree_buckets=int(os.environ.get("FBA_BUCKETS", "32768")))   # (bench.py's c4 shape)
    eng = fba.Engine("gridworld", model=fba.MODEL_BA_FACTORED, belief="importance_sampling", runs=1 << 30, slots=slots, seed=20261003, **kw)
elif cfg == "c3":      # BASELINE configs[2]: factored tiger, 16384 simulations, packed records
    kw = dict(size=3, sims=16384, particles=4096, structure_prior=2, horizon=10, episodes=64)
    eng = fba.Engine("episodic-factored-tiger", model=fba.MODEL_BA_FACTORED, belief="rejection_sampling", runs=1 << 30, slots=slots, seed=20261003, **kw)
else:
    kw = dict(sims=4096, particles=4096, horizon=10, episodes=64) if cfg == "c2" else dict(sims=1024, particles=1024, horizon=10, episodes=64)
    eng = fba.Engine("episodic-tiger", model=fba.MODEL_BA_TABLE, belief="rejection_sampling", runs=1 << 30, slots=slots, seed=20261003, **kw)
L = N.load()
out = (C.c_ulonglong * 12)()
eng.run_ticks(int(os.environ.get("FBA_WARM", "1")) if cfg in ("c3", "c4") else 2)
L.fba_debug_search_profile(out, 1)
c0 = eng.counters()
ticks = 2 if cfg in ("c3", "c4") else 3   # the measured ticks
eng.run_ticks(ticks)
L.fba_debug_search_profile(out, 0)
c1 = eng.counters()
names = ["root sample + particle fetch", "action (UCB / rollout draw)", "simulator step", "child lookup / expand / rollout sums", "back-up", "iterations", "loop head",
         "root block (selection, step, child)"]
v = list(out)
regions = (0, 1, 2, 3, 4, 6) + ((7,) if v[7] else ())   # (the root block: search_kernel's episodic-tiger instantiations only)
total = sum(v[i] for i in regions)
steps = c1.sim_steps - c0.sim_steps
line = {"slots": slots, "config": kw, "waves": slots // (16 if cfg == "c4" else 64), "sim_steps": steps, "wave_iterations": v[5],
        "steps_per_wave_iteration": steps / max(v[5], 1),
        "cycles_per_wave_iteration": total / max(v[5], 1),
        "share": {names[i]: round(v[i] / total, 4) for i in regions}}
if v[8]:   # search_kernel: what its waves executed.  A trip is charged once per wave, by the first active lane of a ballot, and the lanes that
    # step in it are counted by another, so lane_steps_per_wave_trip is the step's lane utilisation x 64 whatever the schedule is
    # (steps_per_wave_iteration above is that only while a wave's first lane runs as many trips as the wave)
    launches = ticks * line["waves"] * kw["sims"]   # simulations of a wave's trees, as the wave sees them: one per tree and simulation index
    line.update({"quorum": os.environ.get("FBA_SEARCH_QUORUM", "default"), "lane_steps": v[8], "lane_steps_per_wave_trip": v[8] / max(v[5], 1),
                 "boundary_phases": v[9], "boundary_phases_per_simulation": v[9] / launches, "lanes_per_boundary_phase": v[10] / max(v[9], 1),
                 # the steps made by the boundary phase's root block are counted apart (no part of lane_steps); a trip whose step phase had
                 # no lane to serve still counts as a trip
                 "root_lane_steps": v[11], "trips_per_simulation": v[5] / launches})
print(json.dumps(line))
