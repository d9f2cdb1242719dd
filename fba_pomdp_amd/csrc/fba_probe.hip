// fba_probe.hip -- fba_probe: the evidence of the step that actually happens, recorded from inside the tick, between the environment step and
// the belief update.  For every slot of the probed range with an update pending, from the action, observation and true new state s* the
// device holds (DeviceState::action / obs / env_state), in the notation of fba_belief_forecast (include/fba_hip.h):
//     evidence = sum_i w_i sum_s' p_i(s') l_i(s') / W     next_true = sum_i w_i p_i(s*) / W     post_true = sum_i w_i p_i(s*) l_i(s*) / W
//
//   probe_chunk_kernel   a workgroup takes a chunk of a slot's particles:
//                          factors    each particle's normalised transition rows (TL entries) and, per observation node and row,
//                                     theta[row][o_g], as fp64 tables in LDS: belief_factors (fba_belief_factors.h), the phase that
//                                     forecast_chunk_kernel runs as well -- the only one that knows the record format
//                          evidence   one thread per particle.  Where every observation node of the action has at most one parent under the
//                                     particle's OWN parent set, the sum over s' factorises:
//                                         prod_{g without parent} l_g(row 0) * prod_f sum_v p_f(v) * prod_{g whose parent is f} l_g(row v)
//                                     TL + RL operations; no next state is enumerated.  A particle with an observation node of two or more
//                                     parents (the factored tiger's listen) enumerates S as the forecast does; a tabular model's evidence is
//                                     the dot product of its two rows over S.
//                          combine    lanes, then waves, in a fixed order; one global fp64 atomic per workgroup and output
//   probe_finish_kernel  weight total in a fixed tree order, / W, the record at an index taken with atomicAdd       one workgroup per slot
//
// Workgroups of slots that are inactive or have no update pending return at once.  A translation unit of its own, outside the parity path;
// read-only on the context: it writes the accumulators and records of BeliefProbeArgs only.
#include "fba_belief_factors.h"

namespace fba {

// does slot e get a record in this launch?  A step that is followed by a belief update: the slot is live, env_kernel has just flagged the
// update, and a history record has room for the step's entry (the update of a full record stops the run instead)
__device__ __forceinline__ bool probe_slot_pending(const Problem& P, const DeviceState& D, int e)
{
    if (!D.active[e] || !D.need_update[e]) return false;
    return !P.hist || hist_total(D.hist_cnt[e]) < P.hist_cap;
}

// FMT: the record format (with_record_format).  Dynamic LDS: forecast_lds_bytes (fba_kernels.h).
template <int FMT>
__global__ void __launch_bounds__(256) probe_chunk_kernel(Problem P, DeviceState D, BeliefProbeArgs a)
{
    __shared__ double s_red[3][4];   // the waves' partial sums per output
    static_assert(FACTORS_STATIC_LDS + sizeof(s_red) + FORECAST_LDS <= 64 * 1024, "probe_chunk_kernel: static + dynamic LDS exceed 64 KB");
    const int tid = threadIdx.x, lane = tid & 63;
    const int b = blockIdx.y, e = a.first + b;
    if (!probe_slot_pending(P, D, e)) return;   // (the whole workgroup: nothing of the slot is read)
    const int nT = a.lay.nT, nO = a.lay.nO, nn = nT + nO, TL = a.lay.TL, RL = a.lay.RL, S = P.S;
    const int star = D.env_state[e];
    // (probe_slot_pending has seen that the record has room: the phase need not check)
    const auto [s_P, s_L, s_w, s_mask, s_nd, s_seg, s_out, nloc] = belief_factors<FMT>(P, D, a.lay, e, D.action[e], D.obs[e], true, false);

    // ---- evidence: thread i owns particle i and, from here on, its rows of s_P ----
    double ve = 0.0, vn = 0.0, vp = 0.0;
    const bool star_in = (unsigned)star < (unsigned)S;
    if (tid < nloc && s_w[tid] != 0.0) {
        const int i = tid;
        double* Pi = s_P + (size_t)i * TL;
        const double* Li = s_L + (size_t)i * RL;
        double pt = star_in ? 1.0 : 0.0, lt = 1.0, ev;
        if (!P.fd) {
            pt = star_in ? Pi[star] : 0.0;
            lt = star_in ? Li[star] : 0.0;
            ev = 0.0;
            for (int sp = 0; sp < S; ++sp) ev += Pi[sp] * Li[sp];
        } else {
            const uint32_t* Mi = s_mask + i * nn;
            const uint64_t fstar = pack_features(star_in ? star : 0, P.fd->Sstep, nT);
            bool single = true;
#pragma unroll
            for (int g = 0; g < MAXF; ++g)
                if (g < nO) {
                    const NodeRegs nd = s_nd[nT + g];
                    single = single && __popc(Mi[nT + g] & ((1u << nd.nmax) - 1u)) <= 1;
                    lt *= Li[s_seg[nT + g] + node_row(nullptr, nd, Mi[nT + g], fstar)];
                }
#pragma unroll
            for (int f = 0; f < MAXF; ++f)
                if (f < nT) pt *= Pi[s_seg[f] + feat(fstar, f)];
            ev = 1.0;
            if (single) {
                // fold every observation node into the transition row of its one parent (row v of the node = value v of that feature)
                for (int g = 0; g < nO; ++g) {
                    const NodeRegs nd = s_nd[nT + g];
                    const uint32_t m = Mi[nT + g] & ((1u << nd.nmax) - 1u);
                    const double* Lg = Li + s_seg[nT + g];
                    if (!m) { ev *= Lg[0]; continue; }
                    const int jp = __ffs(m) - 1, f = nd.parent(jp);
                    if (f >= nT) { ev = 0.0; continue; }   // (no layout has such a parent: node_row would read a feature the state lacks)
                    double* Pf = Pi + s_seg[f];
                    const int nv = min(nd.psize(jp), s_out[f]);
                    for (int v = 0; v < nv; ++v) Pf[v] *= Lg[v];
                }
                for (int f = 0; f < nT; ++f) {
                    const double* Pf = Pi + s_seg[f];
                    double sum = 0.0;
                    for (int v = 0; v < s_out[f]; ++v) sum += Pf[v];
                    ev *= sum;
                }
            } else {
                ev = 0.0;
                for (int sp = 0; sp < S; ++sp) {
                    const uint64_t fv = pack_features(sp, P.fd->Sstep, nT);
                    double p = 1.0;
#pragma unroll
                    for (int f = 0; f < MAXF; ++f)
                        if (f < nT) p *= Pi[s_seg[f] + feat(fv, f)];
#pragma unroll
                    for (int g = 0; g < MAXF; ++g)
                        if (g < nO) p *= Li[s_seg[nT + g] + node_row(nullptr, s_nd[nT + g], Mi[nT + g], fv)];
                    ev += p;
                }
            }
        }
        const double w = s_w[i];
        ve = w * ev;
        vn = w * pt;
        vp = vn * lt;
    }
    // ---- combine: no atomics inside the workgroup ----
    ve = lanes_sum(ve, 64);
    vn = lanes_sum(vn, 64);
    vp = lanes_sum(vp, 64);
    if (lane == 0) { s_red[0][tid >> 6] = ve; s_red[1][tid >> 6] = vn; s_red[2][tid >> 6] = vp; }
    __syncthreads();
    if (tid < 3) {
        const double v = ((s_red[tid][0] + s_red[tid][1]) + s_red[tid][2]) + s_red[tid][3];
        if (v != 0.0) unsafeAtomicAdd(&a.acc[(size_t)b * 3 + tid], v);
    }
}

__global__ void __launch_bounds__(256) probe_finish_kernel(Problem P, DeviceState D, BeliefProbeArgs a)
{
    __shared__ double s_part[256];
    const int b = blockIdx.x, e = a.first + b, tid = threadIdx.x;
    if (!probe_slot_pending(P, D, e)) return;
    const double W = slot_weight_total(P, D, slot_recs(P, D, e), s_part);
    if (tid != 0) return;
    double* acc = a.acc + (size_t)b * 3;
    fba_probe_rec rec;
    rec.run = D.run[e]; rec.episode = D.episode[e]; rec.t = D.t[e];   // (the position moves in advance_kernel, after the update)
    rec.slot = e;
    rec.action = D.action[e]; rec.obs = D.obs[e]; rec.state = D.env_state[e];
    rec.reserved = 0;
    // (a filter whose weights are all 0 has no predictive: every output is 0.0, as every term is)
    rec.evidence  = W > 0.0 ? acc[0] / W : 0.0;
    rec.next_true = W > 0.0 ? acc[1] / W : 0.0;
    rec.post_true = W > 0.0 ? acc[2] / W : 0.0;
    acc[0] = acc[1] = acc[2] = 0.0;   // zeroed for the slot's next step
    double* step = a.step + (size_t)b * PROBE_STEP_WORDS;   // for fba_step_stats: every evaluated step, whatever the buffer holds
    step[0] = rec.evidence; step[1] = rec.next_true; step[2] = rec.post_true; step[3] = 1.0;
    const unsigned long long idx = atomicAdd(a.seen, 1ull);   // every record is counted, those below the capacity are kept
    if (idx < (unsigned long long)a.capacity) a.recs[idx] = rec;
}

void launch_belief_probe(const Problem& P, const DeviceState& D, const BeliefProbeArgs& a, hipStream_t st)
{
    const size_t lds = forecast_lds_bytes(a.lay.TL, a.lay.RL, a.lay.nT + a.lay.nO, a.lay.chunk, P.hist != 0);
    const dim3 grid(ceil_div(P.N, a.lay.chunk), a.count), block(256);
    with_record_format(P, a.lay.ft_FS, [&](auto fmt) { hipLaunchKernelGGL(probe_chunk_kernel<decltype(fmt)::value>, grid, block, lds, st, P, D, a); });
    hipLaunchKernelGGL(probe_finish_kernel, dim3(a.count), block, 0, st, P, D, a);
}

}  // namespace fba
