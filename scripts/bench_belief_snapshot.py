"""Belief snapshots measured: fba_belief_replicate, fba_belief_export and fba_belief_import against plain copies of the same bytes, on the
two shapes of the other posterior benchmarks (scripts/bench_belief_forecast.py):

  history   gridworld --size 7 FBA-POMDP, importance filter, history records, 16 384 particles x 256 slots, 20 ticks run first
  dense     collision avoidance 7 x 7 x 2, importance filter, fp32 records, 4 096 particles x 256 slots, 3 ticks run first

Per shape one JSON line:
  replicate   slot 0 into the 255 others: wall time of each of `--repeats` calls after two warm-ups (host clock around the call, which ends
              in a stream synchronise and holds its three small flag downloads), bytes written = 255 * N * (stride + 8), GB/s written; the
              yardstick is ONE hipMemcpyAsync device-to-device of that byte count between two plain buffers plus a synchronise, timed the
              same way in the same process, the calls of the two alternating
  export      all slots into a pinned host buffer (and once more into pageable memory, which is what Engine.belief_export returns), bytes =
              slots * fba_belief_snapshot_bytes; yardstick: one hipMemcpy device-to-host of those bytes into the same pinned buffer
  import      the same blocks back (host pass, upload, device pass, commit); yardstick: one hipMemcpy host-to-device from that buffer
  parent      what the parent commit offers for moving a filter: fba_belief_get + fba_belief_set of one slot through fp32 tables on the host,
              timed at 256 particles and SCALED linearly to the shape (stated as scaled).  History-record contexts refuse fba_belief_set of
              states or counts: no route exists there, and the line says so.

  python3 scripts/bench_belief_snapshot.py [history|dense|both] [--slots 256] [--repeats 7]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "history": dict(domain="gridworld", kw=dict(model=2, belief="importance_sampling", size=7, structure_prior=2, sims=64, horizon=20, episodes=2),
                    particles=16384, ticks=20),
    "dense": dict(domain="random-collision-avoidance", kw=dict(model=2, belief="importance_sampling", width=7, height=7, size=2, sims=64, horizon=20,
                                                               episodes=2), particles=4096, ticks=3),
}
H2D, D2H, D2D = 1, 2, 3


class Hip:
    """the few runtime calls the yardsticks need, straight from libamdhip64"""

    def __init__(self):
        self.L = C.CDLL("libamdhip64.so")
        vp, sz = C.c_void_p, C.c_size_t
        self.L.hipMalloc.argtypes = [C.POINTER(vp), sz]
        self.L.hipFree.argtypes = [vp]
        self.L.hipHostMalloc.argtypes = [C.POINTER(vp), sz, C.c_uint]
        self.L.hipHostFree.argtypes = [vp]
        self.L.hipMemcpy.argtypes = [vp, vp, sz, C.c_int]
        self.L.hipMemcpyAsync.argtypes = [vp, vp, sz, C.c_int, vp]

    def chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: hipError %d" % (what, rc))

    def malloc(self, n):
        p = C.c_void_p()
        self.chk(self.L.hipMalloc(C.byref(p), n), "hipMalloc")
        return p

    def host_malloc(self, n):
        p = C.c_void_p()
        self.chk(self.L.hipHostMalloc(C.byref(p), n, 0), "hipHostMalloc")
        return p

    def copy(self, dst, src, n, kind):
        self.chk(self.L.hipMemcpy(dst, src, n, kind), "hipMemcpy")

    def copy_async_sync(self, dst, src, n, kind):
        self.chk(self.L.hipMemcpyAsync(dst, src, n, kind, None), "hipMemcpyAsync")
        self.chk(self.L.hipDeviceSynchronize(), "hipDeviceSynchronize")


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def spread(times, nbytes):
    t = sorted(times)
    return {"ms": [1e3 * x for x in times], "ms_min": 1e3 * t[0], "ms_median": 1e3 * t[len(t) // 2], "ms_max": 1e3 * t[-1],
            "GBps_at_median": nbytes / t[len(t) // 2] / 1e9, "GBps_at_min": nbytes / t[0] / 1e9}


def parent_route(fba, shape):
    """fba_belief_get + fba_belief_set of one slot of 256 particles through the host: seconds per particle, or why there is none"""
    eng = fba.Engine(shape["domain"], particles=256, slots=2, runs=1 << 20, seed=20261019, **shape["kw"])
    eng.run_ticks(shape["ticks"])
    try:
        s, w, cnt = eng.belief_get(0)
        eng.belief_set(1, state=s, weight=w, counts=cnt)
        t0 = time.perf_counter()
        s, w, cnt = eng.belief_get(0)
        eng.belief_set(1, state=s, weight=w, counts=cnt)
        dt = time.perf_counter() - t0
        same = all(np.array_equal(a, b) for a, b in zip(eng.belief_get(0), eng.belief_get(1)))
        out = {"what": "fba_belief_get + fba_belief_set of one slot of 256 particles through fp32 tables on the host",
               "seconds_per_particle": dt / 256, "table_bytes_per_particle": 4 * eng.ncnt, "copy_equals_source": bool(same)}
    except ValueError as e:
        out = {"what": "none: fba_belief_set refuses this context", "message": str(e)}
    eng.close()
    return out


def run(fba, hip, name, slots, repeats):
    shape = SHAPES[name]
    eng = fba.Engine(shape["domain"], particles=shape["particles"], slots=slots, runs=1 << 20, seed=20261019, **shape["kw"])
    eng.run_ticks(shape["ticks"])
    n, E, per = eng.cfg.particles, eng.slots, eng.belief_snapshot_bytes
    head = np.ascontiguousarray(eng.belief_export(0, 1)[:, :64]).view(fba._native.SNAPSHOT_HEAD_DTYPE).reshape(-1)[0]
    stride = int(head["stride"])
    out = {"metric": "belief snapshots: replicate, export and import against plain copies of the same bytes", "shape": name,
           "domain": shape["domain"], "particles": n, "slots": E, "ticks_before": shape["ticks"], "particle_bytes": eng.particle_bytes,
           "record_format": int(head["record_format"]), "stride_of_slot_0": stride, "snapshot_bytes_per_slot": per,
           "table_form_bytes_per_slot": n * (4 * eng.ncnt + 12)}

    # ---- replicate: slot 0 into the others, against one device-to-device copy of the bytes it writes
    wrote = (E - 1) * n * (stride + 8)
    a, b = hip.malloc(wrote), hip.malloc(wrote)
    for _ in range(2):
        eng.belief_replicate(0, 0, E)
        hip.copy_async_sync(b, a, wrote, D2D)
    t_rep, t_cpy = [], []
    for _ in range(repeats):
        t_rep.append(timed(lambda: eng.belief_replicate(0, 0, E)))
        t_cpy.append(timed(lambda: hip.copy_async_sync(b, a, wrote, D2D)))
    hip.L.hipFree(a)
    hip.L.hipFree(b)
    out["replicate"] = dict(spread(t_rep, wrote), bytes_written=wrote, bytes_basis="(slots - 1) * N * (stride + 8)",
                            source_bytes=n * (stride + 8))
    out["replicate_yardstick_hipMemcpyAsync_d2d"] = spread(t_cpy, wrote)
    out["replicate_over_yardstick_at_median"] = out["replicate"]["ms_median"] / out["replicate_yardstick_hipMemcpyAsync_d2d"]["ms_median"]

    # ---- export and import through a pinned host buffer, against plain copies of the same bytes in the same direction
    total = E * per
    pinned, dev = hip.host_malloc(total), hip.malloc(total)
    L, h = eng.L, eng.h
    for _ in range(2):
        eng._chk(L.fba_belief_export(h, 0, E, pinned, total))
        hip.copy(pinned, dev, total, D2H)
    t_exp, t_d2h = [], []
    for _ in range(repeats):
        t_d2h.append(timed(lambda: hip.copy(pinned, dev, total, D2H)))
        t_exp.append(timed(lambda: eng._chk(L.fba_belief_export(h, 0, E, pinned, total))))      # (last: the buffer ends up holding the blocks)
    for _ in range(2):
        eng._chk(L.fba_belief_import(h, 0, E, pinned, total))
        hip.copy(dev, pinned, total, H2D)
    t_imp, t_h2d = [], []
    for _ in range(repeats):
        t_imp.append(timed(lambda: eng._chk(L.fba_belief_import(h, 0, E, pinned, total))))
        t_h2d.append(timed(lambda: hip.copy(dev, pinned, total, H2D)))
    t_page = [timed(lambda: eng.belief_export()) for _ in range(3)]
    again = eng.belief_export()
    back = np.ctypeslib.as_array(C.cast(pinned, C.POINTER(C.c_uint8)), shape=(E, per))
    out["export_pinned"] = dict(spread(t_exp, total), bytes=total, staging_chunks=-(-total // (256 << 20)))
    out["export_yardstick_hipMemcpy_d2h_pinned"] = spread(t_d2h, total)
    out["export_pageable_numpy"] = spread(t_page, total)
    out["import_pinned"] = dict(spread(t_imp, total), bytes=total, uploads="twice where the range takes several chunks (validate all, then commit)")
    out["import_yardstick_hipMemcpy_h2d_pinned"] = spread(t_h2d, total)
    out["export_after_import_equals_the_blocks"] = bool(np.array_equal(again, back))
    hip.L.hipHostFree(pinned)
    hip.L.hipFree(dev)
    eng.close()

    route = parent_route(fba, shape)
    if "seconds_per_particle" in route:
        route["scaled_seconds_one_slot_into_the_others"] = route["seconds_per_particle"] * n * (E - 1)
        route["scaled"] = "linearly from 256 particles and one slot: not measured at this size"
    out["parent_commit_route"] = route
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("shape", nargs="?", default="both", choices=["history", "dense", "both"])
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import fba_pomdp_amd as fba
    hip = Hip()
    for name in (("history", "dense") if args.shape == "both" else (args.shape,)):
        run(fba, hip, name, args.slots, args.repeats)


if __name__ == "__main__":
    main()
