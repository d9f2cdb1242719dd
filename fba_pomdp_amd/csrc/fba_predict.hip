// fba_predict.hip -- fba_belief_predict: the posterior-predictive model of a range of slots, evaluated on the device for a list of
// queries (s, a, s', o) from whatever record format the context stores, without building a particle's table.  Per particle the
// expected Dirichlet row c / sum(c) of each node of the query, under the particle's own parent set, averaged over the filter.
//
//   predict_total_kernel        weight total of each slot                                  one workgroup per slot
//   predict_rows_kernel         dense / packed records: one wave per (query, node) and one per (query, joint); the lanes of a group own the
//                               entries of the row, the groups of a wave take the particles in index order, registers only
//   predict_hist_kernel         history records: one thread per particle, queries in a loop; per node sum w / R per prior form, the raised
//                               cells' w * delta / R and the joint product, combined per workgroup in LDS, then fp64 atomics
//   predict_hist_finish_kernel  history records: prior row * that sum + the raised terms, / weight total   one thread per output entry
//
// A translation unit of its own, outside the parity path: the order of the fp64 additions is the engine's.  Read-only on the context.
#include "fba_belief_factors.h"   // lanes_sum, raised, slot_weight_total

namespace fba {

__device__ __forceinline__ double groups_sum(double v, int width)   // over the groups of a wave, lane by lane
{
    for (int off = width; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void __launch_bounds__(256) predict_total_kernel(Problem P, DeviceState D, BeliefPredictArgs a)
{
    __shared__ double s_part[256];
    const int b = blockIdx.x, e = a.first + b, tid = threadIdx.x;
    const double W = slot_weight_total(P, D, slot_recs(P, D, e), s_part);
    if (tid == 0) a.wtot[b] = W;
}

// ---------------------------------------------------------------------------------------------
// dense and packed records
// ---------------------------------------------------------------------------------------------
// node j of query q: T(a, j) for j < nT (parents: the features of s, value: that feature of s'), then O(a, j - nT) (parents: the features
// of s', value: that feature of o).  A tabular model is two nodes without parents whose `off` is the row itself.
struct QueryNode {
    NodeRegs nd;
    uint64_t fv;   // the parent values
    int val;       // the query's own value of the node
};
__device__ __forceinline__ QueryNode predict_query_node(const Problem& P, const BeliefPredictArgs& a, int q, int j)
{
    const int s = a.state[q], act = a.action[q], ns = a.next_state[q], ob = a.obs[q];
    QueryNode n;
    if (!P.fd) {
        n.nd.off  = j == 0 ? (s * P.A + act) * P.S : P.phi_len + (act * P.S + ns) * P.O;
        n.nd.out  = j == 0 ? P.S : P.O;
        n.nd.nmax = 0; n.nd.var = -1; n.nd.fixed_mask = 0;
        n.nd.maxp_lo = n.nd.maxp_hi = n.nd.psz_lo = n.nd.psz_hi = 0;
        n.fv  = 0;
        n.val = j == 0 ? ns : ob;
        return n;
    }
    const FDesc* fd = P.fd;
    const int FS = fd->FS, FO = fd->FO;
    const bool T = j < FS;
    const int f  = T ? j : j - FS;
    n.nd  = load_node(&fd->nodes[T ? act * FS + f : P.A * FS + act * FO + f]);
    n.fv  = pack_features(T ? s : ns, fd->Sstep, FS);
    n.val = T ? feat(pack_features(ns, fd->Sstep, FS), f) : feat(pack_features(ob, fd->Ostep, FO), f);
    return n;
}
template <int FMT>
__device__ __forceinline__ int predict_row(const Problem& P, const DeviceState& D, const BeliefPredictArgs& a, const NodeRegs& nd, uint64_t fv, const float* rec)
{
    const uint32_t mask = nd.var >= 0 ? __float_as_uint(record_count<FMT>(P, D, rec, a.ncounts + nd.var)) : nd.fixed_mask;
    return node_row(nullptr, nd, mask, fv);
}

constexpr int PREDICT_WAVES = 4;   // waves (items) per workgroup
constexpr int PREDICT_TILES = 8;   // row entries one lane accumulates side by side
template <int FMT>
__global__ void __launch_bounds__(64 * PREDICT_WAVES) predict_rows_kernel(Problem P, DeviceState D, BeliefPredictArgs a)
{
    __shared__ NodeRegs s_nd[PREDICT_WAVES][PREDICT_MAXQN];
    __shared__ uint64_t s_fv[PREDICT_WAVES][PREDICT_MAXQN];
    __shared__ int s_val[PREDICT_WAVES][PREDICT_MAXQN];
    __shared__ int s_row[PREDICT_WAVES][PREDICT_MAXQN];   // the row of a node without a parent-set word: the same in every particle
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.y, e = a.first + b;
    const int per = a.nn + 1;
    const long long item = (long long)blockIdx.x * PREDICT_WAVES + wave;
    const bool live = item < (long long)a.nq * per;
    const int q = live ? (int)(item / per) : 0, j = live ? (int)(item % per) : 0;
    const bool is_joint = j == a.nn;
    if (live && is_joint && a.joint && lane < a.nn) {
        const QueryNode n = predict_query_node(P, a, q, lane);
        s_nd[wave][lane] = n.nd; s_fv[wave][lane] = n.fv; s_val[wave][lane] = n.val;
        s_row[wave][lane] = node_row(nullptr, n.nd, n.nd.fixed_mask, n.fv);
    }
    __syncthreads();
    if (!live) return;
    const SlotRecs r = slot_recs(P, D, e);
    const size_t oq = (size_t)b * a.nq + q;
    const double W  = a.wtot[b];
    if (is_joint) {
        if (!a.joint) return;
        const int Wd = a.jw, kl = lane & (Wd - 1), g = lane / Wd, G = 64 / Wd;
        double acc = 0.0;
        for (int i0 = 0; i0 < P.N; i0 += G) {
            const bool valid = i0 + g < P.N;
            const int i      = valid ? i0 + g : 0;
            const float* rec = r.rec + (size_t)i * r.stride;
            double prod      = 1.0;
            for (int n = 0; n < a.nn; ++n) {
                const int len = s_nd[wave][n].out;
                int row       = s_row[wave][n];
                if (s_nd[wave][n].var >= 0) row = predict_row<FMT>(P, D, a, s_nd[wave][n], s_fv[wave][n], rec);
                double sum = 0.0;
                for (int k = kl; k < len; k += Wd) sum += (double)record_count<FMT>(P, D, rec, row + k);
                sum = lanes_sum(sum, Wd);
                const double cv = (double)record_count<FMT>(P, D, rec, row + s_val[wave][n]);
                prod *= sum > 0.0 ? cv / sum : 0.0;
            }
            acc += valid ? particle_weight(P, D, r, i) * prod : 0.0;
        }
        acc = groups_sum(acc, Wd);
        if (lane == 0) a.joint[oq] = acc / W;
        return;
    }
    const bool isT = j < a.nT;
    double* out    = isT ? a.trans : a.obsp;
    if (!out) return;
    out += oq * (size_t)(isT ? a.TL : a.OL) + a.seg[j];
    const QueryNode n = predict_query_node(P, a, q, j);
    const int len = n.nd.out;
    int Wd = 1;
    while (Wd < len && Wd < 64) Wd <<= 1;
    const int kl = lane & (Wd - 1), g = lane / Wd, G = 64 / Wd;
    const int row0 = node_row(nullptr, n.nd, n.nd.fixed_mask, n.fv);
    for (int c0 = 0; c0 < len; c0 += PREDICT_TILES * Wd) {   // (more than one round only for rows beyond 512 entries)
        double acc[PREDICT_TILES];
#pragma unroll
        for (int t = 0; t < PREDICT_TILES; ++t) acc[t] = 0.0;
        for (int i0 = 0; i0 < P.N; i0 += G) {
            const bool valid = i0 + g < P.N;
            const int i      = valid ? i0 + g : 0;
            const float* rec = r.rec + (size_t)i * r.stride;
            const int row    = n.nd.var >= 0 ? predict_row<FMT>(P, D, a, n.nd, n.fv, rec) : row0;
            double sum = 0.0;
            for (int k = kl; k < len; k += Wd) sum += (double)record_count<FMT>(P, D, rec, row + k);
            sum = lanes_sum(sum, Wd);
            const double w = valid ? particle_weight(P, D, r, i) : 0.0;
#pragma unroll
            for (int t = 0; t < PREDICT_TILES; ++t) {
                const int k = c0 + t * Wd + kl;
                if (k < len && sum > 0.0) acc[t] += w * (double)record_count<FMT>(P, D, rec, row + k) / sum;
            }
        }
#pragma unroll
        for (int t = 0; t < PREDICT_TILES; ++t) {
            const double tot = groups_sum(acc[t], Wd);
            const int k      = c0 + t * Wd + kl;
            if (g == 0 && k < len) out[k] = tot / W;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// history records.  A particle's row = the prior row of its own parent set (two forms at most: a gridworld x / y node with and without the
// goal parent) + what its entries of the query's action added to it, so per (particle, query, node) one walk over those entries gives the
// row sum R and the few raised cells; trans / obsp = (prior row * sum_i w_i / R_i + sum_i w_i delta_i / R_i) / W.  The host hands over, per
// query and entry-cell slot, where the row starts per form, its prior sum and the prior rows themselves (PredictSlotNode, qprior).
// ---------------------------------------------------------------------------------------------
template <int HIST>
__global__ void __launch_bounds__(256) predict_hist_kernel(Problem P, DeviceState D, BeliefPredictArgs a)
{
    constexpr int NC = HIST == 2 ? 2 : PREDICT_SLOTS;
    extern __shared__ double s_acc[];   // [hw]: the raised terms of the TL + OL entries, sum w / R per (slot, form), the joint sum
    const int b = blockIdx.y, e = a.first + b, tid = threadIdx.x, lane = tid & 63, i = blockIdx.x * 256 + tid;
    const int TLOL = a.TL + a.OL, hw = TLOL + 2 * PREDICT_SLOTS + 1;
    for (int k = tid; k < hw; k += 256) s_acc[k] = 0.0;
    __syncthreads();
    const SlotRecs r = slot_recs(P, D, e);
    // (more entries than a record has room for: the update kernels report that)
    const bool ok       = i < P.N && hist_total(r.cnt) <= P.hist_cap;
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(r.rec + (size_t)(ok ? i : 0) * r.stride);
    const double w      = ok ? particle_weight(P, D, r, i) : 0.0;
    const uint32_t mask = rec[1];
    const HistDims dims = hist_dims<HIST>(P, P.ca);
    const bool rows     = a.trans || a.obsp;
    double* gacc        = a.hacc + (size_t)b * a.nq * hw;
    for (int q = 0; q < a.nq; ++q) {
        const int act = a.action[q];
        const int j0  = act < 4 ? hist_offset(r.cnt, act) : 0, na = ok && act < 4 ? hist_count(r.cnt, act) : 0;
        int rb[NC], len[NC], seg[NC], form[NC], val[NC];
        double R[NC], hit[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const PredictSlotNode& n = a.qn[(size_t)q * PREDICT_SLOTS + k];
            form[k] = n.var >= 0 ? (int)((mask >> n.var) & 1u) : 0;
            rb[k]   = form[k] ? n.rb1 : n.rb0;
            R[k]    = form[k] ? n.prs1 : n.prs0;
            len[k]  = n.out; seg[k] = n.seg; val[k] = n.val;
            hit[k]  = 0.0;
        }
        const float* qp = a.qprior + (size_t)q * 2 * TLOL;
        auto delta_of = [&](int k, int rel, int mult) -> double {
            if (HIST != 3) return (double)mult;
            // the prior's count after `mult` single additions of 1.0f, which need not be prior + mult
            const float p0 = qp[form[k] * TLOL + seg[k] + rel];
            return (double)raised(p0, mult) - (double)p0;
        };
        if (HIST == 3) {
            hist_distinct_cells<HIST, NC>(dims, rec, mask, act, j0, na, rb, len, [&](int k, int rel, int mult) {
                const double d = delta_of(k, rel, mult);
                R[k] += d;
                if (rel == val[k]) hit[k] = d;
            });
            if (rows)
                hist_distinct_cells<HIST, NC>(dims, rec, mask, act, j0, na, rb, len, [&](int k, int rel, int mult) {
                    unsafeAtomicAdd(&s_acc[seg[k] + rel], w * delta_of(k, rel, mult) / R[k]);
                });
        } else {
            // prior + j is exact in these formats: an entry adds 1 to its cell and to its row, whatever the other entries name
            for (int j = j0; j < j0 + na; ++j) {
                int c[HIST_ENTRY_CELLS];
                hist_entry_cells<HIST>(dims, mask, act, rec[2 + j], c);
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const int rel = c[k] - rb[k];
                    const bool in = (unsigned)rel < (unsigned)len[k];
                    R[k] += in ? 1.0 : 0.0;
                    hit[k] += in && rel == val[k] ? 1.0 : 0.0;
                }
            }
            if (rows)
                for (int j = j0; j < j0 + na; ++j) {
                    int c[HIST_ENTRY_CELLS];
                    hist_entry_cells<HIST>(dims, mask, act, rec[2 + j], c);
#pragma unroll
                    for (int k = 0; k < NC; ++k) {
                        const int rel = c[k] - rb[k];
                        if ((unsigned)rel < (unsigned)len[k]) unsafeAtomicAdd(&s_acc[seg[k] + rel], w / R[k]);
                    }
                }
        }
        double prod = 1.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const PredictSlotNode& n = a.qn[(size_t)q * PREDICT_SLOTS + k];
            if (n.out > 0) {   // (the same for every thread)
                const double p0 = (double)qp[form[k] * TLOL + n.seg + n.val];
                prod *= R[k] > 0.0 ? (p0 + hit[k]) / R[k] : 0.0;
                const double inv = R[k] > 0.0 ? w / R[k] : 0.0;
                const double v0  = lanes_sum(form[k] ? 0.0 : inv, 64);
                if (lane == 0 && v0 != 0.0) unsafeAtomicAdd(&s_acc[TLOL + 2 * k], v0);
                if (n.var >= 0) {
                    const double v1 = lanes_sum(form[k] ? inv : 0.0, 64);
                    if (lane == 0 && v1 != 0.0) unsafeAtomicAdd(&s_acc[TLOL + 2 * k + 1], v1);
                }
            }
        }
        const double js = lanes_sum(w * prod, 64);
        if (lane == 0 && js != 0.0) unsafeAtomicAdd(&s_acc[TLOL + 2 * PREDICT_SLOTS], js);
        __syncthreads();
        for (int k = tid; k < hw; k += 256) {
            const double v = s_acc[k];
            if (v != 0.0) {
                unsafeAtomicAdd(&gacc[(size_t)q * hw + k], v);
                s_acc[k] = 0.0;
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) predict_hist_finish_kernel(Problem P, BeliefPredictArgs a)
{
    const int b = blockIdx.y, TLOL = a.TL + a.OL, per = TLOL + 1, hw = TLOL + 2 * PREDICT_SLOTS + 1;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.nq * per) return;
    const int q = (int)(idx / per), en = (int)(idx % per);
    const size_t oq   = (size_t)b * a.nq + q;
    const double* row = a.hacc + oq * hw;
    const double W    = a.wtot[b];
    if (en == TLOL) {
        if (a.joint) a.joint[oq] = row[TLOL + 2 * PREDICT_SLOTS] / W;
        return;
    }
    const int k     = a.ent_slot[en];
    const float* qp = a.qprior + (size_t)q * 2 * TLOL;
    const double v  = (row[en] + (double)qp[en] * row[TLOL + 2 * k] + (double)qp[TLOL + en] * row[TLOL + 2 * k + 1]) / W;
    if (en < a.TL) {
        if (a.trans) a.trans[oq * a.TL + en] = v;
    } else if (a.obsp) a.obsp[oq * a.OL + (en - a.TL)] = v;
}

void launch_belief_predict(const Problem& P, const DeviceState& D, const BeliefPredictArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(predict_total_kernel, dim3(a.count), dim3(256), 0, st, P, D, a);
    if (P.hist) {
        const int TLOL = a.TL + a.OL;
        const size_t lds = (size_t)(TLOL + 2 * PREDICT_SLOTS + 1) * sizeof(double);
        const dim3 grid(ceil_div(P.N, 256), a.count);
        if (P.hist == 3) hipLaunchKernelGGL(predict_hist_kernel<3>, grid, dim3(256), lds, st, P, D, a);
        else if (P.hist == 2) hipLaunchKernelGGL(predict_hist_kernel<2>, grid, dim3(256), lds, st, P, D, a);
        else hipLaunchKernelGGL(predict_hist_kernel<1>, grid, dim3(256), lds, st, P, D, a);
        const long long n = (long long)a.nq * (TLOL + 1);
        hipLaunchKernelGGL(predict_hist_finish_kernel, dim3((unsigned)((n + 255) / 256), a.count), dim3(256), 0, st, P, a);
        return;
    }
    const long long items = (long long)a.nq * (a.nn + 1);
    const dim3 grid((unsigned)((items + PREDICT_WAVES - 1) / PREDICT_WAVES), a.count), block(64 * PREDICT_WAVES);
    if (P.ft_packed) {
        if (a.ft_FS == 2) hipLaunchKernelGGL(predict_rows_kernel<2>, grid, block, 0, st, P, D, a);
        else if (a.ft_FS == 3) hipLaunchKernelGGL(predict_rows_kernel<3>, grid, block, 0, st, P, D, a);
        else hipLaunchKernelGGL(predict_rows_kernel<4>, grid, block, 0, st, P, D, a);
    } else if (P.packed) hipLaunchKernelGGL(predict_rows_kernel<1>, grid, block, 0, st, P, D, a);
    else hipLaunchKernelGGL(predict_rows_kernel<0>, grid, block, 0, st, P, D, a);
}

}  // namespace fba
