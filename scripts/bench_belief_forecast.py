"""One fba_belief_forecast over every slot of a context, all three outputs, against what a host had before it: fba_belief_get of a slot
and the same sums in numpy.  The two shapes of scripts/bench_belief_predict.py, so that the three posterior-reading calls can be read
side by side:

  history   gridworld --size 7 FBA-POMDP, importance filter, history records, 16 384 particles x 256 slots, 20 ticks run first
  dense     collision avoidance 7 x 7 x 2, importance filter, fp32 records, 4 096 particles x 256 slots, 3 ticks run first

Prints one JSON line per shape: wall time of five calls after one warm-up (host clock around the call; the call synchronises, and holds
the device allocations, the upload of actions and observations and the copy of the results), the bytes by the stated formulas and their
share of the 8 TB/s peak over the call's wall time -- kernel times come from running this script under `rocprofv3 --kernel-trace
--stats` --, and the host path's time for one slot of 256 particles in seconds per particle, SCALED linearly to the shape (stated as
scaled: nobody would wait for it).

  python3 scripts/bench_belief_forecast.py [history|dense|both] [--slots 256] [--repeats 5] [--no-host-path]
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


def step(eng):
    """an action per slot and an observation per slot that its filter can produce: what particle 0 would see without noise"""
    g = np.random.default_rng(20261019)
    action = g.integers(0, eng.A, eng.slots).astype(np.int32)
    obs = np.array([int(eng.belief_get_particle(0, slot=e)[0]) % eng.O for e in range(eng.slots)], np.int32)
    return action, obs


def layout_sizes(eng):
    """(TL, rows of the observation nodes, cells of the observation nodes' tables of one action)"""
    lay = eng.factored_layout()
    FS, FO = lay.n_state_features, lay.n_obs_features
    tl = int(sum(lay.state_feature_size[:FS]))
    rl = cells = 0
    for g in range(FO):
        node = lay.node[eng.A * FS + g]
        rows = 1
        for j in range(node.n_candidates):
            if node.mask_word >= 0 or (node.fixed_mask >> j) & 1:
                rows *= node.candidate_size[j]
        rl += rows
        cells += rows * node.out
    return tl, rl, cells


def formula_bytes(eng, entries):
    """(bytes every record, weight, accumulator and result once = what HBM has to deliver; bytes the kernels ask the memory system for)"""
    n, slots, S = eng.cfg.particles, eng.slots, eng.S
    tl, rl, cells = layout_sizes(eng)
    results = (2 * S + 1) * 8
    acc = 3 * 2 * S * 8           # the fp64 accumulators zeroed, raised, read
    if eng.particle_bytes >= 4 * eng.ncnt:      # fp32 records: the transition rows twice (sum, quotient), every observation row and its cell at o
        once = slots * (n * (eng.particle_bytes + 16) + acc + results)
        asked = slots * (n * ((2 * tl + cells + rl) * 4 + 16) + acc + results)
        return once, asked, "slots * (N * (Cs * 4 + 16) + 3 * 2 * S * 8 + results)", \
            "slots * (N * ((2 * TL + observation cells + observation rows) * 4 + 16) + 3 * 2 * S * 8 + results)"
    words = 2 + entries
    stride = 64 if words <= 16 else (128 if words <= 32 else eng.particle_bytes)
    once = slots * (n * (stride + 16) + acc + results)
    asked = slots * (n * (8 + 4 * entries / eng.A + 16) + acc + results)     # state and parent-set word, the entries of the action, the weight twice
    return once, asked, "slots * (N * (stride + 16) + 3 * 2 * S * 8 + results)", "slots * (N * (8 + 4 * entries / A + 16) + 3 * 2 * S * 8 + results)"


def host_forecast(eng, a, o):
    """what the parent commit offers: fba_belief_get of slot 0, every particle's rows normalised and multiplied out in numpy"""
    s, w, cnt = eng.belief_get(0)
    lay = eng.factored_layout()
    FS, FO, n, S = lay.n_state_features, lay.n_obs_features, cnt.shape[0], eng.S
    ssz, osz = list(lay.state_feature_size[:FS]), list(lay.obs_feature_size[:FO])
    words = np.ascontiguousarray(cnt[:, lay.n_counts:]).view(np.uint32)
    c64 = cnt.astype(np.float64)

    def features(index, sizes):
        out, rest = np.zeros((len(index), len(sizes)), np.int64), np.asarray(index, np.int64).copy()
        for f in range(len(sizes) - 1, -1, -1):
            out[:, f] = rest % sizes[f]
            rest //= sizes[f]
        return out

    def theta(rows):
        tot = rows.sum(axis=-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(tot > 0, rows / tot, 0.0)

    own, every, fo = features(s, ssz), features(np.arange(S), ssz), features(np.array([o]), osz)[0]
    me = np.arange(n)
    p, l = np.ones((n, S)), np.ones((n, S))
    for f in range(FS + FO):
        T = f < FS
        node = lay.node[a * FS + f if T else eng.A * FS + a * FO + f - FS]
        mask = words[:, node.mask_word] if node.mask_word >= 0 else np.full(n, node.fixed_mask, np.uint32)
        if T:
            idx = np.zeros(n, np.int64)
            for j in range(node.n_candidates):
                bit = ((mask >> np.uint32(j)) & 1).astype(bool)
                idx = np.where(bit, idx * node.candidate_size[j] + own[:, node.candidate[j]], idx)
            rows = c64[me[:, None], (node.offset + idx * node.out)[:, None] + np.arange(node.out)[None, :]]
            p *= theta(rows)[:, every[:, f]]
        else:
            idx = np.zeros((n, S), np.int64)
            for j in range(node.n_candidates):
                bit = ((mask >> np.uint32(j)) & 1).astype(bool)
                idx = np.where(bit[:, None], idx * node.candidate_size[j] + every[:, node.candidate[j]][None, :], idx)
            rows = c64[me[:, None, None], (node.offset + idx * node.out)[:, :, None] + np.arange(node.out)[None, None, :]]
            l *= theta(rows)[:, :, fo[f - FS]]
    W = w.sum()
    post = (w[:, None] * p * l).sum(axis=0) / W
    return (w[:, None] * p).sum(axis=0) / W, post, post.sum()


def host_path_seconds(fba, shape):
    eng = fba.Engine(shape["domain"], particles=256, slots=1, runs=1 << 20, seed=20261018, **shape["kw"])
    eng.run_ticks(shape["ticks"])
    action, obs = step(eng)
    host_forecast(eng, int(action[0]), int(obs[0]))
    t0 = time.perf_counter()
    nxt, post, ev = host_forecast(eng, int(action[0]), int(obs[0]))
    dt = time.perf_counter() - t0
    dev = eng.belief_forecast(action, obs)
    agree = float(max(np.abs(dev.next_mass[0] - nxt).max(), np.abs(dev.post_mass[0] - post).max(), abs(dev.evidence[0] - ev)))
    eng.close()
    return dt / 256, agree


def run(fba, name, slots, repeats, host_path):
    shape = SHAPES[name]
    eng = fba.Engine(shape["domain"], particles=shape["particles"], slots=slots, runs=1 << 20, seed=20261018, **shape["kw"])
    eng.run_ticks(shape["ticks"])
    entries = shape["ticks"] if name == "history" else 0   # (every slot has taken that many updates unless an episode ended on the way)
    action, obs = step(eng)
    eng.belief_forecast(action, obs)                        # warm-up: code objects, allocator
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fc = eng.belief_forecast(action, obs)
        times.append(time.perf_counter() - t0)
    once, asked, once_basis, asked_basis = formula_bytes(eng, entries)
    best = min(times)
    tl, rl, cells = layout_sizes(eng)
    out = {
        "metric": "one fba_belief_forecast over all slots, all outputs",
        "shape": name, "domain": shape["domain"], "particles": shape["particles"], "slots": eng.slots, "ticks_before": shape["ticks"],
        "particle_bytes": eng.particle_bytes, "S": eng.S, "TL": tl, "observation_rows": rl,
        "call_ms": [1e3 * t for t in times], "call_ms_best": 1e3 * best,
        "bytes_once": once, "bytes_once_basis": once_basis, "bytes_asked": asked, "bytes_asked_basis": asked_basis,
        "result_bytes_to_host": eng.slots * (2 * eng.S + 1) * 8,
        "fraction_of_8TBps_over_call_wall_time": once / best / PEAK,
        "evidence_mean": float(fc.evidence.mean()), "evidence_min": float(fc.evidence.min()), "next_mass_sum_mean": float(fc.next_mass.sum(axis=1).mean()),
    }
    if host_path:
        per_particle, agree = host_path_seconds(fba, shape)
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
    ap.add_argument("--no-host-path", action="store_true")
    args = ap.parse_args()
    import fba_pomdp_amd as fba
    for name in (("history", "dense") if args.shape == "both" else (args.shape,)):
        run(fba, name, args.slots, args.repeats, not args.no_host_path)


if __name__ == "__main__":
    main()
