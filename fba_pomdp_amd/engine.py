"""Host-side mirror of the reference's experiment / planner / belief interface over the C-ABI.

Method names follow the reference: `select_action` = Planner::selectAction (Planner.hpp:23-24),
`belief_*` = Belief::initiate / updateEstimation / sample (Belief.hpp:25-40) and
BABelief::resetDomainStateDistribution (BABelief.hpp:34), `run_planning` / `run_bapomdp` =
experiment::planning::run / experiment::bapomdp::run.  Errors the reference throws as strings
surface as ValueError with the same wording.
"""
import collections
import ctypes as C

import numpy as np

from . import _native as N


class FbaError(RuntimeError):
    pass


def _enum(value, table, what):
    if isinstance(value, str):
        if value not in table:
            raise ValueError(f"{what} '{value}' is not supported")
        return table[value]
    return int(value)


def snapshot_block_bytes(head_bytes):
    """Bytes of the snapshot block a 64-byte header starts (fba_snapshot_block_bytes): 64 + [particles * 8] + particles * particle_bytes.
    Host arithmetic, no context: how a file of blocks of another context is cut into blocks before Engine.belief_convert."""
    h = np.ascontiguousarray(np.frombuffer(head_bytes, np.uint8) if isinstance(head_bytes, (bytes, bytearray, memoryview)) else head_bytes, np.uint8).reshape(-1)
    if h.size < N.SNAPSHOT_HEAD_DTYPE.itemsize:
        raise ValueError(f"a snapshot header has {N.SNAPSHOT_HEAD_DTYPE.itemsize} bytes, not {h.size}")
    h = np.ascontiguousarray(h[:N.SNAPSHOT_HEAD_DTYPE.itemsize])
    return int(N.load().fba_snapshot_block_bytes(h.ctypes.data))


class BeliefPrediction:
    """What Engine.belief_predict returns: numpy arrays [slot, query, ...] (None where not asked for) and, for a factored model, where
    each feature's segment starts: feature f of `trans` is trans[..., trans_offsets[f]:trans_offsets[f + 1]], likewise `obsp`."""

    def __init__(self, trans, obsp, joint, trans_offsets, obs_offsets):
        self.trans = trans
        self.obsp = obsp
        self.joint = joint
        self.trans_offsets = trans_offsets   # None for a tabular model
        self.obs_offsets = obs_offsets


class BeliefForecast:
    """What Engine.belief_forecast returns: numpy arrays with one row per slot of the range (None where not asked for)."""

    def __init__(self, next_mass, post_mass, evidence):
        self.next_mass = next_mass   # [slots][S] predictive next-state marginal
        self.post_mass = post_mass   # [slots][S] Rao-Blackwellised posterior, unnormalised: its sum over the states is the evidence
        self.evidence = evidence     # [slots]    P(obs | belief, action)


class ProbeRecords(np.ndarray):
    """What Engine.probe returns: the fba_probe_rec records stored, sorted by (run, episode, t); `.seen` counts every step probed, so
    seen > len(records) says the buffer was too small."""
    seen = 0


class RetiredRecords(np.ndarray):
    """What Engine.retired returns: the fba_retired_rec records stored, ordered by run; `.seen` counts every retirement since
    Engine.giveup_policy, so seen > len(records) says the list was too small (endless run_ticks only)."""
    seen = 0


class BeliefSummary:
    """What Engine.belief_summary returns: numpy arrays with one row per slot of the range (None where not asked for)."""

    def __init__(self, head, state_mass, mean_counts, edge_prob):
        self.head = head                                  # fba_belief_summary_head per slot
        self.weight_total = head["weight_total"]
        self.weight_sq_total = head["weight_sq_total"]
        self.particles = head["particles"]
        self.weighted = head["weighted"]
        with np.errstate(divide="ignore", invalid="ignore"):
            self.ess = self.weight_total ** 2 / self.weight_sq_total   # effective sample size
        self.state_mass = state_mass                      # [slots][S]
        self.mean_counts = mean_counts                    # [slots][fba_counts_len]
        self.edge_prob = edge_prob                        # [slots][n_mask_words][FBA_MAX_FEATURES]


class BeliefStructures:
    """What Engine.belief_structures returns: numpy arrays with one row per slot of the range.  All masses are unnormalised: divide by
    `weight_total`."""

    def __init__(self, head, set_mass, top_words, top_mass, query_mass):
        self.head = head                                  # fba_structure_head per slot
        self.weight_total = head["weight_total"]
        self.unplaced_mass = head["unplaced_mass"]
        self.distinct = head["distinct"]
        self.overflow = head["overflow"]
        self.stored = head["stored"]
        self.set_mass = set_mass                          # [slots][n_words][n_sets]
        self.top_words = top_words                        # [slots][top_k][n_words], uint32
        self.top_mass = top_mass                          # [slots][top_k]
        self.query_mass = query_mass                      # [slots][nq]


class StructureStats(collections.namedtuple("StructureStats", "head set_frac query_frac query_held query_sole")):
    """What Engine.structure_stats returns: the fba_structure_stat heads [episodes][horizon] and, with the same two leading axes, the
    sums of set_mass / W [n_words][n_sets] and query_mass / W [nq] over the bin's steps and the steps that held / held only query q."""
    __slots__ = ()


class DeviceArray(collections.namedtuple("DeviceArray", "name elem_bytes elems slot_elems buffers")):
    """One entry of Engine.device_arrays()."""
    __slots__ = ()

    @property
    def bytes(self):
        return self.elem_bytes * self.elems


class Engine:
    """One fba_ctx: `slots` independent (planner, belief) pairs resident on one MI355X."""

    def __init__(self, domain="episodic-tiger", model=N.MODEL_POMDP, belief="rejection_sampling",
                 planner="po-uct", **kw):
        self.L = N.load()
        cfg = N.Config()
        self.L.fba_default_config(C.byref(cfg))
        cfg.domain = _enum(domain, N.DOMAIN_NAMES, "domain")
        cfg.model = int(model)
        cfg.belief = _enum(belief, N.BELIEF_NAMES, "belief")
        cfg.planner = _enum(planner, N.PLANNER_NAMES, "planner")
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise AttributeError(f"fba_config has no field '{k}'")
            setattr(cfg, k, v)
        if cfg.belief == N.BELIEF_POINT:
            cfg.particles = 1   # what fba_create does with it; keeps the array sizes of this wrapper right
        self.cfg = cfg
        h = C.c_void_p()
        rc = self.L.fba_create(C.byref(cfg), C.byref(h))
        if rc != N.OK:
            msg = self.L.fba_last_error(None).decode()
            raise (ValueError if rc == N.EINVAL else FbaError)(msg)
        self.h = h
        S, A, O = C.c_int32(), C.c_int32(), C.c_int32()
        self.L.fba_domain_sizes(h, C.byref(S), C.byref(A), C.byref(O))
        self.S, self.A, self.O = S.value, A.value, O.value
        self.ncnt = self.L.fba_counts_len(h)
        self.slots = self.L.fba_slots(h)
        self.particle_bytes = self.L.fba_particle_bytes(h)

    def close(self):
        if getattr(self, "h", None):
            self.L.fba_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc != N.OK:
            msg = self.L.fba_last_error(self.h).decode()
            raise (ValueError if rc == N.EINVAL else FbaError)(msg)

    def device_arrays(self):
        """What the context holds on the device (fba_device_arrays): {name: DeviceArray}, in allocation order.  A per-slot array is
        `buffers` buffers of `slots` slots of `slot_elems` elements; the sum of `bytes` is what a context of this configuration takes."""
        n = self._count(self.L.fba_device_arrays(self.h, None, 0))
        out = (N.ArrayInfo * n)()
        n = min(n, self._count(self.L.fba_device_arrays(self.h, out, n)))
        return {a.name.decode(): DeviceArray(a.name.decode(), a.elem_bytes, a.elems, a.slot_elems, a.buffers) for a in out[:n]}

    def _count(self, n):
        if n < 0:
            self._chk(n)
        return n

    # ---- experiments
    def run_planning(self):
        st = N.Stat()
        self._chk(self.L.fba_run_planning(self.h, C.byref(st)))
        return st

    def run_bapomdp(self, first_episode=0, stop_episode=None, beliefs=None):
        """experiment::bapomdp::run.  With arguments, episodes [first_episode, stop_episode) of every run only (fba_run_bapomdp_span):
        `beliefs` -- uint8[nblocks, belief_snapshot_bytes] as belief_export returns, one block for every run or one per run -- are the
        filters the runs continue from, at the stream positions of the uninterrupted experiment; statistics outside the span have count 0."""
        st = (N.Stat * self.cfg.episodes)()
        if first_episode == 0 and stop_episode is None and beliefs is None:
            self._chk(self.L.fba_run_bapomdp(self.h, st))
            return list(st)
        stop = self.cfg.episodes if stop_episode is None else stop_episode
        if beliefs is None:
            self._chk(self.L.fba_run_bapomdp_span(self.h, first_episode, stop, None, 0, 0, st))
            return list(st)
        b = np.ascontiguousarray(beliefs, np.uint8)
        nblocks = b.shape[0] if b.ndim == 2 else b.size // self.belief_snapshot_bytes
        self._chk(self.L.fba_run_bapomdp_span(self.h, first_episode, stop, b.ctypes.data, nblocks, b.nbytes, st))
        return list(st)

    def run_ticks(self, ticks):
        self._chk(self.L.fba_run_ticks(self.h, ticks))

    def returns(self):
        n = self.cfg.runs * self.cfg.episodes
        r = np.zeros(n, np.float64)
        ln = np.zeros(n, np.int32)
        self._chk(self.L.fba_get_returns(self.h, r.ctypes.data, ln.ctypes.data))
        return r.reshape(self.cfg.runs, self.cfg.episodes), ln.reshape(self.cfg.runs, self.cfg.episodes)

    def counters(self):
        c = N.Counters()
        self._chk(self.L.fba_get_counters(self.h, C.byref(c)))
        return c

    def return_sums(self):
        out = np.zeros(3, np.float64)
        self._chk(self.L.fba_get_return_sums(self.h, out.ctypes.data))
        return out

    def kernel_times(self):
        kt = (N.KernelTime * N.K_COUNT)()
        self._chk(self.L.fba_get_kernel_times(self.h, kt))
        return {N.KERNEL_NAMES[i]: kt[i] for i in range(N.K_COUNT)}

    def debug_compact_slots(self):
        """Diagnostic: how many slots hold their filter as 16-byte records right now."""
        n = C.c_int32(0)
        self._chk(self.L.fba_debug_compact_slots(self.h, C.byref(n)))
        return n.value

    def reset_kernel_times(self):
        self._chk(self.L.fba_reset_kernel_times(self.h))

    def trace(self):
        n = self.L.fba_trace_count(self.h)
        out = np.zeros(max(n, 1), N.TRACE_DTYPE)
        n = self.L.fba_get_trace(self.h, out.ctypes.data, len(out))
        if n < 0:
            self._chk(n)
        return out[:n]

    def trace_hist(self):
        """trace = 2: the filter's state histogram after the belief update of every trace record, in the order of trace()."""
        n = self.L.fba_trace_count(self.h)
        out = np.zeros((max(n, 1), N.TRACE_HIST_BINS), np.uint32)
        n = self.L.fba_get_trace_hist(self.h, out.ctypes.data, len(out))
        if n < 0:
            self._chk(n)
        return out[:n]

    def probe_enable(self, first=0, count=None, capacity=None):
        """Record, for every real step of slots [first, first + count) that run_bapomdp / run_ticks make from now on and that a belief
        update follows, what the filter said about it (fba_probe_enable): the evidence P(obs | belief, action) and the predictive and
        posterior mass at the true new state.  `capacity` records are kept (default: runs * episodes * horizon), later ones are only
        counted; count=0 turns the probe off and frees the buffer.  Read-only on everything else."""
        count = self.slots - first if count is None else count
        if capacity is None:
            capacity = max(self.cfg.runs, 1) * max(self.cfg.episodes, 1) * self.cfg.horizon
        self._chk(self.L.fba_probe_enable(self.h, first, count, capacity))

    def step_stats_enable(self, on=True):
        """Accumulate, for every real step run_planning / run_bapomdp / run_ticks make from now on, the per-(episode, t) statistics of
        fba_step_stat on the device (fba_step_stats_enable); on=True allocates and clears the bins, on=False frees them.  A probe that
        is enabled as well feeds the probe members, whatever its capacity.  Read-only on everything else."""
        self._chk(self.L.fba_step_stats_enable(self.h, 1 if on else 0))

    def step_stats(self):
        """The bins as a structured array (N.STEP_STAT_DTYPE) of shape (episodes, horizon); raises FbaError while the statistics are off."""
        out = np.zeros((max(self.cfg.episodes, 1), self.cfg.horizon), N.STEP_STAT_DTYPE)
        n = self.L.fba_get_step_stats(self.h, out.ctypes.data, out.size)
        if n < 0:
            self._chk(n)
        return out

    def structure_stats_enable(self, queries=None, on=True):
        """Accumulate, for every real step run_bapomdp / run_bapomdp_span / run_ticks make from now on, the graph posterior of the
        step's main filter into per-(episode, t) bins on the device (fba_structure_stats_enable): how many graphs the filter holds,
        the mass per (word, parent set) and, for each of `queries` (uint32[nq][n_words] word lists as belief_get shows them, at most
        N.STRUCT_STATS_MAX_QUERIES), its mass and whether the filter still holds it.  on=True allocates and clears the bins, on=False
        frees them.  Read-only on everything else."""
        nw, _ = self.structure_lens()
        q = None if queries is None or not on else np.ascontiguousarray(queries, np.uint32).reshape(-1, max(nw, 1))
        nq = 0 if q is None else q.shape[0]
        self._chk(self.L.fba_structure_stats_enable(self.h, 1 if on else 0, nq, q.ctypes.data if nq else None))
        self._structure_stats_nq = nq if on else 0

    def structure_stats(self):
        """The bins (fba_get_structure_stats): a StructureStats of `head` (N.STRUCTURE_STAT_DTYPE, shape (episodes, horizon)),
        `set_frac` (episodes, horizon, n_words, n_sets), `query_frac`, `query_held` and `query_sole` (episodes, horizon, nq); raises
        FbaError while the statistics are off."""
        ep, hz = max(self.cfg.episodes, 1), self.cfg.horizon
        nw, ns = self.structure_lens()
        nq = getattr(self, "_structure_stats_nq", 0)
        head = np.zeros((ep, hz), N.STRUCTURE_STAT_DTYPE)
        sf = np.zeros((ep, hz, nw, ns), np.float64)
        qf = np.zeros((ep, hz, nq), np.float64)
        qh = np.zeros((ep, hz, nq), np.uint64)
        qs = np.zeros((ep, hz, nq), np.uint64)
        n = self.L.fba_get_structure_stats(self.h, head.size, head.ctypes.data, sf.ctypes.data, qf.ctypes.data, qh.ctypes.data, qs.ctypes.data)
        if n < 0:
            self._chk(n)
        return StructureStats(head, sf, qf, qh, qs)

    def probe(self):
        """The probe's records as a structured array (N.PROBE_DTYPE) sorted by (run, episode, t), with `.seen`."""
        seen = C.c_int64()
        n = self.L.fba_probe_count(self.h, C.byref(seen))
        if n < 0:
            self._chk(n)
        out = np.zeros(max(n, 1), N.PROBE_DTYPE)
        n = self.L.fba_get_probe(self.h, out.ctypes.data, len(out)) if n else 0
        if n < 0:
            self._chk(n)
        out = out[:n]
        out = out[np.lexsort((out["t"], out["episode"], out["run"]))].view(ProbeRecords)
        out.seen = seen.value
        return out

    def giveup_policy(self, policy="stop", max_attempts=0):
        """What becomes of a run whose rejection update gives up (fba_giveup_policy): "stop" fails the whole experiment, as ever; "retire"
        takes that run out, reports it in retired() and lets the slot go on with its next run.  `max_attempts` is the limit after which an
        update gives up, a positive multiple of N.REJECT_QUANTUM (0: 2^28); it holds for belief_update too.  Clears the list."""
        self._chk(self.L.fba_giveup_policy(self.h, _enum(policy, N.GIVEUP_NAMES, "giveup policy"), max_attempts))

    def retired(self):
        """The runs retired since giveup_policy as a structured array (N.RETIRED_DTYPE) ordered by run, with `.seen` as probe() has it."""
        seen = C.c_int64()
        n = self.L.fba_retired_count(self.h, C.byref(seen))
        if n < 0:
            self._chk(n)
        out = np.zeros(max(n, 1), N.RETIRED_DTYPE)
        n = self.L.fba_get_retired(self.h, out.ctypes.data, len(out)) if n else 0
        if n < 0:
            self._chk(n)
        out = out[:n].view(RetiredRecords)
        out.seen = seen.value
        return out

    def belief_get_particle(self, index, slot=0, weight=False):
        """One particle of the filter (Belief::sample() for a host planner that has drawn the index): state, weight, counts."""
        s = np.zeros(1, np.int32)
        w = np.zeros(1, np.float64)
        cnt = np.zeros(max(self.ncnt, 1), np.float32)
        self._chk(self.L.fba_belief_get_particle(self.h, slot, index, s.ctypes.data, w.ctypes.data if weight else None,
                                                 cnt.ctypes.data if self.ncnt else None))
        return int(s[0]), float(w[0]), cnt[:self.ncnt]

    # ---- per-step interface
    def prior(self):
        out = np.zeros(self.ncnt, np.float32)
        self._chk(self.L.fba_get_prior(self.h, out.ctypes.data))
        return out

    def factored_layout(self):
        """How a factored particle's count blob is laid out (include/fba_hip.h, fba_factored_layout)."""
        out = N.FactoredLayout()
        self._chk(self.L.fba_get_factored_layout(self.h, C.byref(out)))
        return out

    def set_model_tabular(self, phi, psi):
        phi = np.ascontiguousarray(phi, np.float32)
        psi = np.ascontiguousarray(psi, np.float32)
        self._chk(self.L.fba_set_model_tabular(self.h, phi.ctypes.data, psi.ctypes.data))

    def set_model_factored(self, counts, layout=None):
        """Replace the factored base prior: `counts` = a particle's whole blob (CPT counts, then the parent-set words) in
        the engine's layout (factored_layout())."""
        layout = layout or self.factored_layout()
        c = np.ascontiguousarray(counts, np.float32)
        assert c.size == self.ncnt
        self._chk(self.L.fba_set_model_factored(self.h, C.byref(layout), c.ctypes.data))

    def set_position(self, run=None, episode=None, t=None):
        def arr(x):
            if x is None:
                return None, None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.int32), (self.slots,)))
            return a, a.ctypes.data
        r, rp = arr(run)
        e, ep = arr(episode)
        tt, tp = arr(t)
        self._chk(self.L.fba_set_position(self.h, rp, ep, tp))

    def belief_init(self):
        self._chk(self.L.fba_belief_init(self.h))

    def belief_reset_domain_state(self):
        self._chk(self.L.fba_belief_reset_domain_state(self.h))

    def select_action(self, hist_len=0, active=None):
        hl = np.ascontiguousarray(np.broadcast_to(np.asarray(hist_len, np.int32), (self.slots,)))
        act = None if active is None else np.ascontiguousarray(active, np.uint8)
        out = np.zeros(self.slots, np.int32)
        self._chk(self.L.fba_select_action(self.h, hl.ctypes.data, None if act is None else act.ctypes.data, out.ctypes.data))
        return out

    def belief_update(self, action, obs, active=None):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(action, np.int32), (self.slots,)))
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(obs, np.int32), (self.slots,)))
        act = None if active is None else np.ascontiguousarray(active, np.uint8)
        self._chk(self.L.fba_belief_update(self.h, a.ctypes.data, o.ctypes.data, None if act is None else act.ctypes.data))

    def belief_get(self, slot=0, weights=None, counts=True):
        """States, weights and (counts=True) every particle's count table -- N x fba_counts_len floats, whatever the
        storage on the device; ask for counts=False where that is gigabytes."""
        n = self.cfg.particles
        s = np.zeros(n, np.int32)
        want_w = self.cfg.belief in (N.BELIEF_IMPORTANCE, N.BELIEF_CHEATING, N.BELIEF_MH_GIBBS, N.BELIEF_MH_NIPS, N.BELIEF_NESTED) if weights is None else weights
        w = np.zeros(n, np.float64)
        cnt = np.zeros((n, self.ncnt), np.float32) if counts else None
        self._chk(self.L.fba_belief_get(self.h, slot, s.ctypes.data, w.ctypes.data if want_w else None,
                                        cnt.ctypes.data if counts and self.ncnt else None))
        return s, w, cnt

    def belief_summary(self, first=0, count=None, state_mass=True, mean_counts=True, edge_prob=True):
        """The posterior of slots [first, first + count) reduced on the device (fba_belief_summary): per slot the weight totals,
        `ess`, the mass per domain state, the weighted mean of the count tables belief_get would return and, per parent-set word
        of a factored model, the weighted fraction of particles that use each candidate parent.  No table is built anywhere, so
        this is the way to read a filter of history records.  `edge_prob` of a model without parent-set words is None; a plain
        POMDP context serves `state_mass` only (ask with mean_counts=False, edge_prob=False); cells of a factored node compare across particles only where `edge_prob` of
        that node's word is 0 or 1.  Outside the parity contract: the last bits may differ from call to call."""
        count = self.slots - first if count is None else count
        n = max(count, 0)
        if not hasattr(self, "_n_mask_words"):
            self._n_mask_words = self.factored_layout().n_mask_words if self.cfg.model == N.MODEL_BA_FACTORED else 0
        head = np.zeros(n, N.SUMMARY_HEAD_DTYPE)
        sm = np.zeros((n, self.S), np.float64) if state_mass else None
        mc = np.zeros((n, self.ncnt), np.float64) if mean_counts and self.ncnt else None
        ep = np.zeros((n, self._n_mask_words, N.MAX_FEATURES), np.float64) if edge_prob and self._n_mask_words else None
        if self.cfg.model == N.MODEL_POMDP and (mean_counts or edge_prob):   # (the library says what a plain POMDP context serves)
            mc = np.zeros((n, 1), np.float64)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._chk(self.L.fba_belief_summary(self.h, first, count, ptr(head), ptr(sm), ptr(mc), ptr(ep)))
        return BeliefSummary(head, sm, mc, ep)

    def structure_lens(self):
        """(n_words, n_sets): parent-set words of a particle and parent sets a word can name (fba_structure_lens); (0, 0) where the
        model has no parent-set words."""
        nw, ns = C.c_int32(), C.c_int32()
        self._chk(self.L.fba_structure_lens(self.h, C.byref(nw), C.byref(ns)))
        return nw.value, ns.value

    def belief_structures(self, first=0, count=None, top_k=8, queries=None):
        """The posterior over whole model graphs of slots [first, first + count) reduced on the device (fba_belief_structures): per slot
        the mass of every parent set of every word (`set_mass`), the `top_k` distinct structures of largest mass (`top_words`,
        `top_mass`, `stored` of them), how many distinct structures the filter holds (`distinct`) and the mass on each of `queries`,
        uint32[nq][n_words] word lists as belief_get shows them (`query_mass`).  No table is built anywhere.  Outside the parity
        contract; exact and repeatable in a flat filter."""
        count = self.slots - first if count is None else count
        n = max(count, 0)
        nw, ns = self.structure_lens()
        q = None if queries is None else np.ascontiguousarray(queries, np.uint32).reshape(-1, max(nw, 1))
        nq = 0 if q is None else q.shape[0]
        head = np.zeros(n, N.STRUCTURE_HEAD_DTYPE)
        sm = np.zeros((n, nw, ns), np.float64)
        tw = np.zeros((n, max(top_k, 0), nw), np.uint32)
        tm = np.zeros((n, max(top_k, 0)), np.float64)
        qm = np.zeros((n, nq), np.float64)
        self._chk(self.L.fba_belief_structures(self.h, first, count, top_k, nq, None if q is None else q.ctypes.data, head.ctypes.data, sm.ctypes.data,
                                               tw.ctypes.data, tm.ctypes.data, qm.ctypes.data))
        return BeliefStructures(head, sm, tw, tm, qm)

    def predict_lens(self):
        """(TL, OL): entries of one query's `trans` and `obsp` answer (fba_predict_lens)."""
        tl, ol = C.c_int32(), C.c_int32()
        self._chk(self.L.fba_predict_lens(self.h, C.byref(tl), C.byref(ol)))
        return tl.value, ol.value

    def belief_predict(self, state, action, next_state, obs, first=0, count=None, trans=True, obsp=True, joint=True):
        """The posterior-predictive model of slots [first, first + count) at the queries (state, action, next_state, obs), evaluated
        on the device (fba_belief_predict): `trans[slot, q]` = the filter's mean of each particle's expected Dirichlet row of (state, action)
        under that particle's own parent sets, `obsp[slot, q]` the same for the observation row of (action, next_state), `joint[slot, q]`
        the mean probability of the whole transition.  For a factored model trans / obsp hold one segment per feature -- marginals of a
        mixture, which is not their product; `joint` is the structure-aware quantity.  Returns a BeliefPrediction; outputs not asked for
        are None.  Outside the parity contract: the last bits may differ from call to call."""
        count = self.slots - first if count is None else count
        n = max(count, 0)
        q = [np.ascontiguousarray(np.atleast_1d(x), np.int32) for x in (state, action, next_state, obs)]
        nq = len(q[0])
        if any(x.ndim != 1 or len(x) != nq for x in q):
            raise ValueError("belief_predict: state, action, next_state and obs are one-dimensional arrays of one length")
        tl, ol = self.predict_lens()
        tr = np.zeros((n, nq, tl), np.float64) if trans else None
        ob = np.zeros((n, nq, ol), np.float64) if obsp else None
        jt = np.zeros((n, nq), np.float64) if joint else None
        ptr = lambda a: None if a is None else a.ctypes.data
        self._chk(self.L.fba_belief_predict(self.h, first, count, nq, q[0].ctypes.data, q[1].ctypes.data, q[2].ctypes.data, q[3].ctypes.data,
                                            ptr(tr), ptr(ob), ptr(jt)))
        t_off = o_off = None
        if self.cfg.model == N.MODEL_BA_FACTORED:
            lay = self.factored_layout()
            t_off = np.concatenate(([0], np.cumsum(lay.state_feature_size[:lay.n_state_features]))).astype(np.int64)
            o_off = np.concatenate(([0], np.cumsum(lay.obs_feature_size[:lay.n_obs_features]))).astype(np.int64)
        return BeliefPrediction(tr, ob, jt, t_off, o_off)

    def belief_forecast(self, action, obs=None, first=0, count=None, next_mass=True, post_mass=True, evidence=True):
        """The one-step predictive of slots [first, first + count) on the device (fba_belief_forecast): every particle's own domain state
        propagated through its own model by `action` (a scalar, or one per slot of the range).  `next_mass[slot, s']` is the predictive
        next-state marginal, `post_mass[slot, s']` the exact (Rao-Blackwellised) domain-state marginal after observing `obs`, unnormalised,
        and `evidence[slot]` its sum: P(obs | belief, action), the acceptance rate the rejection update is to expect.  `obs` may be None
        where only `next_mass` is asked for.  Returns a BeliefForecast; outputs not asked for are None.  Read-only and outside the parity
        contract: the last bits may differ from call to call."""
        count = self.slots - first if count is None else count
        n = max(count, 0)
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(action, np.int32), (n,)))
        o = None if obs is None else np.ascontiguousarray(np.broadcast_to(np.asarray(obs, np.int32), (n,)))
        nm = np.zeros((n, self.S), np.float64) if next_mass else None
        pm = np.zeros((n, self.S), np.float64) if post_mass else None
        ev = np.zeros(n, np.float64) if evidence else None
        ptr = lambda x: None if x is None else x.ctypes.data
        self._chk(self.L.fba_belief_forecast(self.h, first, count, ptr(a), ptr(o), ptr(nm), ptr(pm), ptr(ev)))
        return BeliefForecast(nm, pm, ev)

    def belief_get_fully_connected(self, slot=0):
        """The second filter of the reinvigoration (fully connected) / cheating (correct graph) belief."""
        n = self.cfg.particles
        s = np.zeros(n, np.int32)
        cnt = np.zeros((n, self.ncnt), np.float32)
        self._chk(self.L.fba_belief_get_fully_connected(self.h, slot, s.ctypes.data, cnt.ctypes.data))
        return s, cnt

    def belief_get_shadow(self, slot=0):
        """The incubator belief's weighted shadow filter: states, weights, counts."""
        n = self.cfg.particles
        s = np.zeros(n, np.int32)
        w = np.zeros(n, np.float64)
        cnt = np.zeros((n, self.ncnt), np.float32)
        self._chk(self.L.fba_belief_get_shadow(self.h, slot, s.ctypes.data, w.ctypes.data, cnt.ctypes.data))
        return s, w, cnt

    def belief_get_nested(self, slot=0):
        """The nested belief's flat filters of domain states, [particles][particles^2] (belief_get returns the count particles)."""
        n = self.cfg.particles
        st = np.zeros((n, n * n), np.int32)
        self._chk(self.L.fba_belief_get_nested(self.h, slot, st.ctypes.data))
        return st

    def belief_set(self, slot, state=None, weight=None, counts=None):
        s = None if state is None else np.ascontiguousarray(state, np.int32)
        w = None if weight is None else np.ascontiguousarray(weight, np.float64)
        c = None if counts is None else np.ascontiguousarray(counts, np.float32)
        self._chk(self.L.fba_belief_set(self.h, slot, None if s is None else s.ctypes.data,
                                        None if w is None else w.ctypes.data, None if c is None else c.ctypes.data))

    # ---- belief snapshots
    @property
    def belief_snapshot_bytes(self):
        """Bytes of one slot's snapshot block (fba_belief_snapshot_bytes): 64 + [particles * 8] + particles * particle_bytes."""
        n = C.c_int64()
        self._chk(self.L.fba_belief_snapshot_bytes(self.h, C.byref(n)))
        return n.value

    def belief_export(self, first=0, count=None):
        """The main filters of slots [first, first + count) as stored (fba_belief_export): np.uint8[count, belief_snapshot_bytes], one
        self-describing block per slot -- header (N.SNAPSHOT_HEAD_DTYPE), weights, records.  No count table is built."""
        count = self.slots - first if count is None else count
        out = np.zeros((max(count, 0), self.belief_snapshot_bytes), np.uint8)
        self._chk(self.L.fba_belief_export(self.h, first, count, out.ctypes.data, out.nbytes))
        return out

    def belief_import(self, first, blocks):
        """Blocks of belief_export (of this or another context of the same configuration and prior) into slots first, first + 1, ...
        (fba_belief_import).  Every block is checked before any is taken: a ValueError leaves the context as it was."""
        b = np.ascontiguousarray(blocks, np.uint8)
        per = self.belief_snapshot_bytes
        count = b.size // per if b.ndim != 2 else b.shape[0]
        self._chk(self.L.fba_belief_import(self.h, first, count, b.ctypes.data, b.nbytes))

    def belief_replicate(self, src, first, count):
        """The filter of slot `src` into every slot of [first, first + count) on the device (fba_belief_replicate); `src` is skipped."""
        self._chk(self.L.fba_belief_replicate(self.h, src, first, count))

    def belief_convert(self, blocks, seed=0, first_run=0):
        """Blocks of a context that differs from this one in its particle count or, for history records, in the room of a record
        (episodes * horizon), refitted to this context (fba_belief_convert): the bytes of as many blocks of belief_snapshot_bytes, which
        belief_import and run_bapomdp(beliefs=...) then take.  Block b draws from the Philox streams of run first_run + b under `seed` where
        the particle count changes.  Nothing of the context changes."""
        b = np.ascontiguousarray(np.frombuffer(blocks, np.uint8) if isinstance(blocks, (bytes, bytearray, memoryview)) else blocks, np.uint8).reshape(-1)
        per = snapshot_block_bytes(b[:64]) if b.size >= 64 else 0
        count = b.size // per if per > 0 else 0
        out = np.zeros(max(count, 1) * self.belief_snapshot_bytes, np.uint8)
        self._chk(self.L.fba_belief_convert(self.h, count, b.ctypes.data if b.size else None, b.nbytes, seed, first_run, out.ctypes.data, out.nbytes))
        return out.tobytes()

    def last_step_info(self):
        out = np.zeros(self.slots, N.TRACE_DTYPE)
        self._chk(self.L.fba_last_step_info(self.h, out.ctypes.data))
        return out
