"""One fba_belief_predict over every slot of a context, all three outputs, at 64 and at 1 024 queries, against what a host had before
it: fba_belief_get of a slot normalised row by row in numpy.  Two shapes:

  history   gridworld --size 7 FBA-POMDP, importance filter, history records, 16 384 particles x 256 slots, 20 ticks run first
  dense     collision avoidance 7 x 7 x 2, importance filter, fp32 records, 4 096 particles x 256 slots, 3 ticks run first

Prints one JSON line per shape and query count: wall time of the call (host clock around it; the call synchronises, and holds the
device allocations, the upload of the queries and the copy of the results), the bytes by the stated formulas and their share of the
8 TB/s peak over the call's wall time -- kernel times come from running this script under `rocprofv3 --kernel-trace --stats` --, and
the host path's time for one slot of 256 particles SCALED linearly to the shape (stated as scaled: nobody would wait for it).

  python3 scripts/bench_belief_predict.py [history|dense|both] [--slots 256] [--repeats 5] [--queries 64 1024] [--no-host-path]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12
SHAPES = {
    "history": dict(domain="gridworld", kw=dict(model=2, belief="importance_sampling", size=7, structure_prior=2, sims=64, horizon=20, episodes=2),
                    particles=16384, ticks=20),
    "dense": dict(domain="random-collision-avoidance", kw=dict(model=2, belief="importance_sampling", width=7, height=7, size=2, sims=64, horizon=20,
                                                               episodes=2), particles=4096, ticks=3),
}


def queries(eng, nq):
    g = np.random.default_rng(20261018 + nq)
    return (g.integers(0, eng.S, nq).astype(np.int32), g.integers(0, eng.A, nq).astype(np.int32),
            g.integers(0, eng.S, nq).astype(np.int32), g.integers(0, eng.O, nq).astype(np.int32))


def formula_bytes(eng, nq, entries):
    """(bytes every record, weight and result once = what HBM has to deliver; bytes the kernels ask the memory system for)"""
    n, slots = eng.cfg.particles, eng.slots
    tl, ol = eng.predict_lens()
    lay = eng.factored_layout()
    nn = lay.n_state_features + lay.n_obs_features
    results = nq * (tl + ol + 1) * 8
    if eng.particle_bytes >= 4 * eng.ncnt:      # fp32 records: a wave per (query, node) and per (query, joint), each reads its rows of every particle
        once = slots * (n * (eng.particle_bytes + 8) + results)
        asked = slots * (nq * n * (2 * (tl + ol) * 4 + (nn + 1) * 8) + results)
        return once, asked, "slots * (N * (Cs * 4 + 8) + results)", "slots * (nq * N * (2 * (TL + OL) * 4 + (nodes + 1) * 8) + results)"
    words = 2 + entries
    stride = 64 if words <= 16 else (128 if words <= 32 else eng.particle_bytes)
    hw = tl + ol + 13
    once = slots * (n * (stride + 8) + 3 * nq * hw * 8 + results)      # the fp64 accumulators zeroed, raised, read
    asked = slots * (nq * n * 4 * (entries / eng.A) + n * (stride + 8) + 3 * nq * hw * 8 + results)     # the entries of the query's action, per query
    return once, asked, "slots * (N * (stride + 8) + 3 * nq * (TL + OL + 13) * 8 + results)", \
        "slots * (nq * N * 4 * entries / A + N * (stride + 8) + 3 * nq * (TL + OL + 13) * 8 + results)"


def host_predict(eng, Q):
    """what the parent commit offers: fba_belief_get of slot 0, every queried row of every particle normalised in numpy"""
    s, a, ns, o = Q
    _, w, cnt = eng.belief_get(0)
    lay = eng.factored_layout()
    FS, FO, n = lay.n_state_features, lay.n_obs_features, cnt.shape[0]
    ssz, osz = list(lay.state_feature_size[:FS]), list(lay.obs_feature_size[:FO])
    words = np.ascontiguousarray(cnt[:, lay.n_counts:]).view(np.uint32)

    def features(index, sizes):
        out, rest = np.zeros((len(index), len(sizes)), np.int64), np.asarray(index, np.int64).copy()
        for f in range(len(sizes) - 1, -1, -1):
            out[:, f] = rest % sizes[f]
            rest //= sizes[f]
        return out

    fs, fns, fo = features(s, ssz), features(ns, ssz), features(o, osz)
    total, prod, out = w.sum(), np.ones((n, len(s))), []
    for f in range(FS + FO):
        T = f < FS
        parents, value, length = (fs, fns[:, f], ssz[f]) if T else (fns, fo[:, f - FS], osz[f - FS])
        seg = np.zeros((len(s), length))
        for x in range(eng.A):
            sel = np.nonzero(a == x)[0]
            node = lay.node[x * FS + f if T else eng.A * FS + x * FO + f - FS]
            mask = words[:, node.mask_word] if node.mask_word >= 0 else np.full(n, node.fixed_mask, np.uint32)
            idx = np.zeros((n, sel.size), np.int64)
            for j in range(node.n_candidates):
                bit = ((mask >> np.uint32(j)) & 1).astype(bool)
                idx = np.where(bit[:, None], idx * node.candidate_size[j] + parents[sel, node.candidate[j]][None, :], idx)
            rows = cnt[np.arange(n)[:, None, None], (node.offset + idx * node.out)[:, :, None] + np.arange(length)[None, None, :]].astype(np.float64)
            tot = rows.sum(axis=2, keepdims=True)
            with np.errstate(divide="ignore", invalid="ignore"):
                th = np.where(tot > 0, rows / tot, 0.0)
            seg[sel] = np.einsum("i,iqk->qk", w, th) / total
            prod[:, sel] *= th[:, np.arange(sel.size), value[sel]]
        out.append(seg)
    return np.concatenate(out[:FS], axis=1), np.concatenate(out[FS:], axis=1), (w[:, None] * prod).sum(axis=0) / total


def host_path_seconds(fba, shape, nq):
    eng = fba.Engine(shape["domain"], particles=256, slots=1, runs=1 << 20, seed=20261018, **shape["kw"])
    eng.run_ticks(shape["ticks"])
    Q = queries(eng, nq)
    host_predict(eng, Q)
    t0 = time.perf_counter()
    trans, obsp, joint = host_predict(eng, Q)
    dt = time.perf_counter() - t0
    dev = eng.belief_predict(*Q)
    agree = float(max(np.abs(dev.trans[0] - trans).max(), np.abs(dev.obsp[0] - obsp).max(), np.abs(dev.joint[0] - joint).max()))
    eng.close()
    return dt / 256, agree


def run(fba, name, slots, repeats, counts, host_path):
    shape = SHAPES[name]
    eng = fba.Engine(shape["domain"], particles=shape["particles"], slots=slots, runs=1 << 20, seed=20261018, **shape["kw"])
    eng.run_ticks(shape["ticks"])
    entries = shape["ticks"] if name == "history" else 0   # (every slot has taken that many updates unless an episode ended on the way)
    for nq in counts:
        Q = queries(eng, nq)
        eng.belief_predict(*Q)                              # warm-up: code objects, allocator
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            pred = eng.belief_predict(*Q)
            times.append(time.perf_counter() - t0)
        once, asked, once_basis, asked_basis = formula_bytes(eng, nq, entries)
        best = min(times)
        tl, ol = eng.predict_lens()
        out = {
            "metric": "one fba_belief_predict over all slots, all outputs",
            "shape": name, "domain": shape["domain"], "particles": shape["particles"], "slots": eng.slots, "ticks_before": shape["ticks"],
            "queries": nq, "particle_bytes": eng.particle_bytes, "TL": tl, "OL": ol,
            "call_ms": [1e3 * t for t in times], "call_ms_best": 1e3 * best,
            "bytes_once": once, "bytes_once_basis": once_basis, "bytes_asked": asked, "bytes_asked_basis": asked_basis,
            "result_bytes_to_host": eng.slots * nq * (tl + ol + 1) * 8,
            "fraction_of_8TBps_over_call_wall_time": once / best / PEAK,
            "joint_mean": float(pred.joint.mean()), "trans_sum_mean": float(pred.trans.sum(axis=2).mean()),
        }
        if host_path:
            per_particle, agree = host_path_seconds(fba, shape, nq)
            out["host_path"] = {"what": "fba_belief_get of one slot of 256 particles + numpy, SCALED linearly (not measured at this size)",
                                "seconds_per_particle": per_particle, "scaled_seconds": per_particle * shape["particles"] * eng.slots,
                                "largest_difference_from_the_device_at_256_particles": agree}
        print(json.dumps(out), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("shape", nargs="?", default="both", choices=["history", "dense", "both"])
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--no-host-path", action="store_true")
    args = ap.parse_args()
    import fba_pomdp_amd as fba
    for name in (("history", "dense") if args.shape == "both" else (args.shape,)):
        run(fba, name, args.slots, args.repeats, args.queries, not args.no_host_path)


if __name__ == "__main__":
    main()
