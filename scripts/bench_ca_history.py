"""Collision avoidance 7 x 7 with two obstacles under the importance filter: history records against dense records.
usage: bench_ca_history.py update [particles] [updates] [--dense]     ms per importance update + resample of one belief (default 10^6, 10)
       bench_ca_history.py slots PARTICLES [--dense]                  the slot count fba_create chooses by itself (4 096 simulations, 2 x 20 steps)
       bench_ca_history.py search PARTICLES SLOTS [--dense]           steps/s of whole experiments: 4 096 simulations, horizon 20, 2 episodes
--dense sets FBA_DENSE_PARTICLES=1 (fp32 count tables, the format of every filter of at most 65 536 particles).  Prints one JSON line.
To compare two builds, run the same command in a checkout of each, alternating them in one session (profiles/README.md)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = [a for a in sys.argv[1:] if a != "--dense"]
if "--dense" in sys.argv[1:]:
    os.environ["FBA_DENSE_PARTICLES"] = "1"     # read by fba_create

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

DOM = "random-collision-avoidance"
SHAPE = dict(model=N.MODEL_BA_FACTORED, belief="importance_sampling", size=2, width=7, height=7, seed=5)
mode = args[0] if args else "update"
out = {"mode": mode, "dense": "--dense" in sys.argv[1:]}
if mode == "update":
    Np = int(args[1]) if len(args) > 1 else 1_000_000
    reps = int(args[2]) if len(args) > 2 else 10
    eng = fba.Engine(DOM, particles=Np, sims=4, slots=1, episodes=1, horizon=reps + 2, **SHAPE)   # (a record holds episodes * horizon updates)
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
    out.update(particles=Np, particle_bytes=eng.particle_bytes, updates=reps, ms_per_update=kt.ms / reps, wall_ms_per_update=1e3 * dt / reps,
               algorithmic_GB_per_update=kt.bytes / reps / 1e9)
elif mode == "slots":
    eng = fba.Engine(DOM, particles=int(args[1]), sims=4096, runs=32768, slots=0, episodes=2, horizon=20, **SHAPE)
    out.update(particles=int(args[1]), particle_bytes=eng.particle_bytes, slots=eng.slots)
elif mode == "search":
    eng = fba.Engine(DOM, particles=int(args[1]), sims=4096, runs=int(args[2]), slots=int(args[2]), episodes=2, horizon=20, **SHAPE)
    t0 = time.perf_counter()
    eng.run_bapomdp()
    dt = time.perf_counter() - t0
    c = eng.counters()
    out.update(particles=int(args[1]), particle_bytes=eng.particle_bytes, slots=eng.slots, seconds=dt, sim_steps=int(c.sim_steps),
               belief_steps=int(c.belief_steps), env_steps=int(c.env_steps), steps_per_s=(c.sim_steps + c.belief_steps) / dt)
else:
    sys.exit(__doc__)
eng.close()
print(json.dumps(out))
