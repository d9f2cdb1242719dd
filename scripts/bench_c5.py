"""BASELINE configs[4] shape: collision avoidance (largest factored domain, W = H = 7, 2 obstacles,
correct-graph prior, Pb = 3532 B), 10^6 particles per belief, importance-weighted update + resample.
Prints the achieved algorithmic HBM rate of the update (all launches of the multi-workgroup filter).
usage: bench_c5.py [particles] [beliefs] [updates] [--dense]
The context stores history records (8 B + 4 B per real step) unless --dense is given; its horizon is sized to hold the warm-up and
every timed update (a record refuses more updates than episodes * horizon, at most 126)."""
import json
import sys
import time

import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

args = [a for a in sys.argv[1:] if a != "--dense"]
if "--dense" in sys.argv[1:]:
    os.environ["FBA_DENSE_PARTICLES"] = "1"     # read by fba_create
Np = int(args[0]) if len(args) > 0 else 1_000_000
slots = int(args[1]) if len(args) > 1 else 1
reps = int(args[2]) if len(args) > 2 else 10
eng = fba.Engine("random-collision-avoidance", model=N.MODEL_BA_FACTORED, belief="importance_sampling", size=2,
                 width=7, height=7, particles=Np, sims=4, slots=slots, seed=5, episodes=1, horizon=reps + 1)
eng.belief_init()
eng.belief_reset_domain_state()
obs = 3 * 7 + 3
eng.belief_update(1, obs)           # warm-up
eng.reset_kernel_times()
t0 = time.perf_counter()
for k in range(reps):
    eng.set_position(t=(k + 1) % 200)
    eng.belief_update(1 + (k % 2), obs)
dt = time.perf_counter() - t0
kt = eng.kernel_times()["importance_kernel"]
gbs = kt.bytes / 1e9 / (kt.ms / 1e3)
print(json.dumps({"particle_bytes": eng.particle_bytes, "workload": f"collision-avoidance 7x7x2, {Np} particles x {slots} beliefs, importance update+resample",
                  "updates": reps, "ms_per_update": kt.ms / reps, "wall_ms_per_update": 1e3 * dt / reps,
                  "algorithmic_GB_per_update": kt.bytes / reps / 1e9, "achieved_GBs": gbs, "frac_of_8TBs": gbs / 8000.0,
                  "particles_per_s": kt.units / (kt.ms / 1e3)}))
