"""Where a workgroup of the packed tiger rejection update spends its cycles: an instrumented build of the same sources
(-DFBA_PROFILE_REJECT: clock64() marks behind the sweep, the attempts and the pass that writes the new filter, each behind a barrier and
a wait for the workgroup's outstanding loads and stores) run on the bench workload.  reject_tiger_once_kernel stores the new filter
inside its attempt loop where it need not gather: there the second region is the attempts with their stores, drained, and the third
(the gather behind the loop) is all but empty.  The names of the regions are those of the three marks in every build, so that a
library of an older commit (FBA_LIB) prints the same line.
python scripts/reject_regions.py build      (hipcc, no GPU needed)  ->  fba_pomdp_amd/libfba_hip_rprof.so
python scripts/reject_regions.py [slots]    (on the GPU box)        ->  one JSON line
FBA_LIB names another instrumented library (an older build of the kernel, for the before / after pair); FBA_PARTICLES another filter size."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF = os.path.join(ROOT, "fba_pomdp_amd", "libfba_hip_rprof.so")
sys.path.insert(0, ROOT)

if len(sys.argv) > 1 and sys.argv[1] == "build":
    from fba_pomdp_amd import _native as N
    N.build(extra_flags=["-DFBA_PROFILE_REJECT"], lib_path=PROF, obj_tag="_rprof")
    print("built", PROF)
    sys.exit(0)

os.environ.setdefault("FBA_LIB", PROF)
import fba_pomdp_amd as fba  # noqa: E402
from fba_pomdp_amd import _native as N  # noqa: E402

slots = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
particles = int(os.environ.get("FBA_PARTICLES", "4096"))
kw = dict(sims=4096, particles=particles, horizon=10, episodes=64)      # bench.py's default workload (c2)
eng = fba.Engine("episodic-tiger", model=fba.MODEL_BA_TABLE, belief="rejection_sampling", runs=1 << 30, slots=slots, seed=20261003, **kw)
L = N.load()
out = (C.c_ulonglong * 4)()
eng.run_ticks(2)
L.fba_debug_reject_profile(out, 1)
eng.run_ticks(8)
L.fba_debug_reject_profile(out, 0)
names = ["sweep", "attempts", "new filter"]     # reject_tiger_once_kernel: sweep | attempts with the stores | gather behind the loop
v = list(out)
total = sum(v[:3])
print(json.dumps({"lib": os.path.basename(os.environ["FBA_LIB"]), "slots": slots, "config": kw, "workgroups": v[3],
                  "cycles_per_workgroup": round(total / max(v[3], 1), 1),
                  "cycles": {names[i]: round(v[i] / max(v[3], 1), 1) for i in range(3)},
                  "share": {names[i]: round(v[i] / max(total, 1), 4) for i in range(3)}}))
