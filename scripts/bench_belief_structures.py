"""One fba_belief_structures over every slot of a context (top 8, three queries, all outputs) against what a host had before it:
fba_belief_get of one slot and numpy's weighted unique over the word rows.  Three shapes:

  history   gridworld --size 7 FBA-POMDP, importance filter, history records, 16 384 particles x 256 slots, 20 ticks run first
  dense     collision avoidance 7 x 7 x 2 under the uniform structure prior, importance filter, fp32 records, 4 096 particles x 256 slots
            (or as many slots, halved from there, as the device has room for), 3 ticks run first
  large     10^6 particles in one slot (the multi-launch importance filter), 2 ticks run first: ONE workgroup walks the slot.  The dense
            model above where it fits, else the gridworld history records, else the continuous factored tiger of size 3 (fp32 records)

Prints one JSON line per shape: device-event time and wall time of the call, one warm-up call and `--repeats` timed ones with their
spread (the events are recorded on the null stream, which the engine's blocking stream orders itself with, so they bracket the
kernel, the call's device allocations and the copies of the results), the bytes the call must read by the stated formula, and the
host route measured on ONE slot at the largest size it runs at (stated per slot: nobody would wait for 256 of them).

  python3 scripts/bench_belief_structures.py [history|dense|large|all] [--slots 256] [--repeats 5] [--no-host-path]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRID = dict(model=2, belief="importance_sampling", size=7, structure_prior=2, sims=64, horizon=20, episodes=2)
FTIGER = dict(model=2, belief="importance_sampling", size=3, structure_prior=2, sims=64, horizon=20, episodes=2)
CA = dict(model=2, belief="importance_sampling", width=7, height=7, size=2, structure_prior=1, sims=64, horizon=20, episodes=2)
SHAPES = {
    "history": [dict(domain="gridworld", kw=GRID, particles=16384, ticks=20, host_particles=16384)],
    "dense": [dict(domain="random-collision-avoidance", kw=CA, particles=4096, ticks=3, host_particles=4096)],
    "large": [dict(domain="random-collision-avoidance", kw=CA, particles=1000000, ticks=2, slots=1, host_particles=65536),
              dict(domain="gridworld", kw=GRID, particles=1000000, ticks=2, slots=1, host_particles=16384),
              dict(domain="continuous-factored-tiger", kw=FTIGER, particles=1000000, ticks=2, slots=1, host_particles=65536)],
}


def create(fba, name, slots):
    """the first candidate of the shape the engine makes, at the most slots it has room for: (engine, candidate, what was refused)"""
    refused = []
    for shape in SHAPES[name]:
        n = shape.get("slots", slots)
        while n >= 1:
            try:
                return fba.Engine(shape["domain"], particles=shape["particles"], slots=n, runs=1 << 20, seed=20261020, **shape["kw"]), shape, refused
            except (ValueError, fba.FbaError) as e:
                refused.append(f"{shape['domain']}, {shape['particles']} particles x {n} slots: {e}")
                n //= 2
    return None, None, refused


class Events:
    """HIP events on the null stream through the runtime the engine itself has loaded; `ok` is False where that cannot be had"""

    def __init__(self):
        try:
            self.hip = C.CDLL("libamdhip64.so")
            self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
            self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
            self.ok = True
        except (OSError, AttributeError):
            self.ok = False

    def mark(self):
        ev = C.c_void_p()
        if not self.ok or self.hip.hipEventCreate(C.byref(ev)) != 0 or self.hip.hipEventRecord(ev, None) != 0:
            self.ok = False
            return None
        return ev

    def ms(self, a, b):
        out = C.c_float()
        if not self.ok or self.hip.hipEventSynchronize(b) != 0 or self.hip.hipEventElapsedTime(C.byref(out), a, b) != 0:
            return None
        return float(out.value)


def timed(call, repeats):
    """(result, event ms or None, wall ms) of `repeats` calls after one warm-up call"""
    events = Events()
    call()
    wall, marks = [], []
    for _ in range(repeats):
        a = events.mark()
        t0 = time.perf_counter()
        out = call()
        wall.append(1e3 * (time.perf_counter() - t0))
        marks.append((a, events.mark()))
    dev = [events.ms(a, b) for a, b in marks] if events.ok else None
    return out, dev if dev and all(d is not None for d in dev) else None, wall


def host_route(fba, shape):
    """fba_belief_get of one slot and the weighted np.unique of its word rows, at `host_particles`: (ms, table bytes brought to the host)"""
    eng = fba.Engine(shape["domain"], particles=shape["host_particles"], slots=1, runs=1 << 20, seed=20261020, **shape["kw"])
    eng.run_ticks(min(shape["ticks"], 3))
    lay = eng.factored_layout()
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        _, w, cnt = eng.belief_get(0)
        words = np.ascontiguousarray(cnt[:, lay.n_counts:]).view(np.uint32)
        uniq, inv = np.unique(words, axis=0, return_inverse=True)
        mass = np.bincount(inv.reshape(-1), weights=w, minlength=len(uniq))
        order = np.argsort(-mass, kind="stable")[:8]
        times.append(1e3 * (time.perf_counter() - t0))
    nbytes = cnt.nbytes
    eng.close()
    return times, nbytes, int(len(uniq)), float(mass[order[0]])


def run(fba, name, slots, repeats, host_path):
    eng, shape, refused = create(fba, name, slots)
    if eng is None:
        print(json.dumps({"shape": name, "refused": refused}), flush=True)
        return
    eng.run_ticks(shape["ticks"])
    nw, ns = eng.structure_lens()
    first = eng.belief_structures(0, 1, top_k=1)
    queries = np.stack([first.top_words[0, 0], np.zeros(nw, np.uint32), first.top_words[0, 0]])
    queries[2, nw - 1] ^= 1                               # the most frequent structure of slot 0, the empty graph, a neighbour of the first
    res, dev, wall = timed(lambda: eng.belief_structures(top_k=8, queries=queries), repeats)
    n, weighted = eng.cfg.particles, True
    key_words = 1 if eng.particle_bytes < 4 * eng.ncnt else nw      # history records: the bits of one word
    out = {
        "metric": "one fba_belief_structures over all slots: head, set_mass, top 8, 3 queries",
        "shape": name, "domain": shape["domain"], "particles": n, "slots": eng.slots, "ticks_before": shape["ticks"],
        "particle_bytes": eng.particle_bytes, "n_words": nw, "n_sets": ns, "refused_before": refused,
        "event_ms": dev, "event_ms_best": min(dev) if dev else None, "event_ms_spread": (max(dev) - min(dev)) if dev else None,
        "wall_ms": wall, "wall_ms_best": min(wall), "wall_ms_spread": max(wall) - min(wall),
        "ms_per_slot_best": (min(dev) if dev else min(wall)) / eng.slots,
        "bytes_words": eng.slots * n * (4 * key_words + (8 if weighted else 0)),
        "bytes_words_basis": "slots * particles * (4 * words read per record + 8 per weight)",
        "bytes_at_record_stride": eng.slots * n * (min(eng.particle_bytes, max(64, 4 * key_words)) + (8 if weighted else 0)),
        "bytes_at_record_stride_basis": "slots * particles * (the 64-byte pieces of a record that hold its words + 8 per weight)",
        "distinct_mean": float(np.mean(res.distinct)), "distinct_max": int(np.max(res.distinct)), "overflow_slots": int(np.sum(res.overflow)),
        "top_share_mean": float(np.mean(res.top_mass[:, 0] / res.weight_total)),
    }
    eng.close()
    if host_path:
        times, nbytes, distinct, _ = host_route(fba, shape)
        out["host_route"] = {"what": "fba_belief_get of ONE slot + weighted np.unique over its word rows, measured at this particle count",
                             "particles": shape["host_particles"], "ms_per_slot": times, "ms_per_slot_best": min(times),
                             "table_bytes_to_host_per_slot": nbytes, "distinct": distinct}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("shape", nargs="?", default="all", choices=["history", "dense", "large", "all"])
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host-path", action="store_true")
    args = ap.parse_args()
    import fba_pomdp_amd as fba
    for name in (("history", "dense", "large") if args.shape == "all" else (args.shape,)):
        try:
            run(fba, name, args.slots, args.repeats, not args.no_host_path)
        except (ValueError, fba.FbaError, MemoryError) as e:      # (a shape the device or the engine has no room for: say so, go on)
            print(json.dumps({"shape": name, "refused": str(e)}), flush=True)


if __name__ == "__main__":
    main()
