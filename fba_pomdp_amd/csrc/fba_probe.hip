// fba_probe.hip -- fba_probe: the evidence of the step that actually happens, recorded from inside the tick, between the environment step and
// the belief update.  For every slot of the probed range with an update pending, from the action, observation and true new state s* the
// device holds (DeviceState::action / obs / env_state), in the notation of fba_belief_forecast (include/fba_hip.h):
//     evidence = sum_i w_i sum_s' p_i(s') l_i(s') / W     next_true = sum_i w_i p_i(s*) / W     post_true = sum_i w_i p_i(s*) l_i(s*) / W
//
//   probe_chunk_kernel   a workgroup takes a chunk of a slot's particles:
//                          factors    each particle's normalised transition rows (TL entries) and, per observation node and row,
//                                     theta[row][o_g], as fp64 tables in LDS -- forecast_chunk_kernel's first phase, copied: folding the two
//                                     into one header is a follow-up (the forecast's kernels are pinned register for register)
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
#include "fba_kernels_common.h"

namespace fba {

__device__ __forceinline__ double probe_lanes_sum(double v, int width)   // over aligned groups of `width` lanes (a power of two)
{
    for (int off = 1; off < width; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

// the count after `mult` single additions of 1.0f (prior + mult where that is exact, which the history formats of the gridworld require)
__device__ __forceinline__ float probe_raised(float p0, int mult)
{
    float v = p0;
    for (int m = 0; m < mult; ++m) v += 1.0f;
    return v;
}

// the node whose cell an entry holds in cell slot k (hist_entry_cells), or -1
template <int HIST>
__device__ __forceinline__ int probe_slot_node(int k, int nT, int nO)
{
    if (HIST == 3) return k < 4 ? (k < nT ? k : -1) : (k - 4 < nO ? nT + k - 4 : -1);
    return k < nT + nO ? k : -1;
}

// gridworld records: the prior row `idx` of node j (0..2 T(x), T(y), T(goal); 3..5 the observation nodes) in the padded tables
__device__ __forceinline__ const float* probe_gw_prior_row(const Problem& P, const HistLayout& L, int act, int j, bool with_goal, int idx)
{
    if (j >= 3) return P.hist_base + L.o_row(act, j - 3, idx);
    if (j == 2) return P.hist_base + act * L.tstride + 2 * L.XY + idx * L.GS;
    return with_goal ? P.hist_alt + (act * 2 + j) * L.XY + idx * L.NS : P.hist_base + act * L.tstride + j * L.XY + idx * L.NS;
}

// does slot e get a record in this launch?  A step that is followed by a belief update: the slot is live, env_kernel has just flagged the
// update, and a history record has room for the step's entry (the update of a full record stops the run instead)
__device__ __forceinline__ bool probe_slot_pending(const Problem& P, const DeviceState& D, int e)
{
    if (!D.active[e] || !D.need_update[e]) return false;
    return !P.hist || hist_total(D.hist_cnt[e]) < P.hist_cap;
}

// the node descriptions, per-node integers and wave partials probe_chunk_kernel keeps in static LDS, beside the FORECAST_LDS bytes of dynamic LDS
static_assert((sizeof(NodeRegs) + 5 * sizeof(int)) * PREDICT_MAXQN + 12 * sizeof(double) + FORECAST_LDS <= 64 * 1024,
              "probe_chunk_kernel: static + dynamic LDS exceed 64 KB");

// FMT: 0 fp32 counts, 1 packed tiger, 2..4 packed factored tiger of that many state features (record_count), 5..7 history records of
// Problem::hist = FMT - 4.  Dynamic LDS: forecast_lds_bytes (fba_kernels.h).
template <int FMT>
__global__ void __launch_bounds__(256) probe_chunk_kernel(Problem P, DeviceState D, BeliefProbeArgs a)
{
    constexpr int HIST = FMT > 4 ? FMT - 4 : 0;
    constexpr int RF   = HIST ? 0 : FMT;   // the record_count of the dense and packed formats
    extern __shared__ double s_dyn[];
    // node j: the transition nodes of the action, then its observation nodes.  s_nd holds the description with off = 0, out = 1, so that
    // node_row returns the row's INDEX; the row starts at s_off + index * s_out
    __shared__ NodeRegs s_nd[PREDICT_MAXQN];
    __shared__ int s_off[PREDICT_MAXQN], s_out[PREDICT_MAXQN], s_var[PREDICT_MAXQN];
    __shared__ int s_seg[PREDICT_MAXQN];   // where the node's entries start in a particle's transition table / its rows in the observation table
    __shared__ int s_val[PREDICT_MAXQN];   // observation nodes: the observation's value of the node
    __shared__ double s_red[3][4];         // the waves' partial sums per output
    const int tid = threadIdx.x, lane = tid & 63;
    const int b = blockIdx.y, e = a.first + b;
    if (!probe_slot_pending(P, D, e)) return;   // (the whole workgroup: nothing of the slot is read)
    const int nT = a.nT, nO = a.nO, nn = nT + nO, TL = a.TL, RL = a.RL, S = P.S;
    const int i0 = blockIdx.x * a.chunk, nloc = min(a.chunk, P.N - i0);
    const int act = D.action[e], ob = D.obs[e], star = D.env_state[e];
    double* s_P   = s_dyn;                                  // [chunk][TL] p_i's factor rows
    double* s_L   = s_P + (size_t)a.chunk * TL;             // [chunk][RL] theta[row][o_g] per observation node and row
    double* s_num = s_L + (size_t)a.chunk * RL;             // history records: [chunk][RL] the count at o_g while s_L holds the row's sum
    double* s_ps  = s_num + (HIST ? (size_t)a.chunk * RL : 0);   // history records: [RL] the prior's row sums, [RL] its counts at o_g
    double* s_pn  = s_ps + (HIST ? RL : 0);
    double* s_w   = s_pn + (HIST ? RL : 0);                 // [chunk]
    int* s_st     = reinterpret_cast<int*>(s_w + a.chunk);  // [chunk]
    uint32_t* s_mask = reinterpret_cast<uint32_t*>(s_st + a.chunk);   // [chunk][nn] the parent set of node j in particle i

    if (tid < nn) {
        const int j = tid;
        NodeRegs nd;
        if (!P.fd) {   // a tabular model: phi row (s, a) = index s * A + a of S entries; psi row (a, s') = index s' behind action a's block
            nd.off  = j == 0 ? 0 : P.phi_len + act * S * P.O;
            nd.out  = j == 0 ? S : P.O;
            nd.nmax = 0; nd.var = -1; nd.fixed_mask = 0;
            nd.maxp_lo = nd.maxp_hi = nd.psz_lo = nd.psz_hi = 0;
            s_val[j] = ob;
        } else {
            const FDesc* fd = P.fd;
            nd = load_node(&fd->nodes[j < nT ? act * nT + j : P.A * nT + act * nO + (j - nT)]);
            s_val[j] = j < nT ? 0 : feat(pack_features(ob, fd->Ostep, nO), j - nT);
        }
        s_off[j] = nd.off; s_out[j] = nd.out; s_var[j] = nd.var;
        s_seg[j] = a.seg[j];
        nd.off = 0; nd.out = 1;
        s_nd[j] = nd;
    }
    const SlotRecs r = slot_recs(P, D, e);
    const bool lazy  = slot_lazy(D, e);
    for (int i = tid; i < nloc; i += 256) {
        const float* rec = r.rec + (size_t)(i0 + i) * r.stride;
        const int st     = lazy ? lazy_state(P, D, e, i0 + i) : rec_state(rec, P.C);
        const bool in    = (unsigned)st < (unsigned)S;
        s_w[i]  = in ? particle_weight(P, D, r, i0 + i) : 0.0;
        s_st[i] = in ? st : 0;
    }
    __syncthreads();
    BeliefSummaryArgs sa{};
    sa.ncounts = a.ncounts;
    for (int x = tid; x < nloc * nn; x += 256) {
        const int i = x / nn, j = x - i * nn;
        const float* rec = r.rec + (size_t)(i0 + i) * r.stride;
        uint32_t mask = s_nd[j].fixed_mask;
        if (s_var[j] >= 0) mask = HIST ? record_mask_word(P, sa, rec, s_var[j]) : __float_as_uint(record_count<RF>(P, D, rec, a.ncounts + s_var[j]));
        s_mask[x] = mask;
    }
    __syncthreads();
    // index of the row of node j that state s chooses under parent set `mask`
    auto row_index = [&](int j, int s, uint32_t mask) -> int {
        if (!P.fd) return j == 0 ? s * P.A + act : s;
        return node_row(nullptr, s_nd[j], mask, pack_features(s, P.fd->Sstep, nT));
    };
    // the observation node and its row that entry rr of a particle's observation table stands for
    auto obs_place = [&](int rr, int& j, int& idx) {
        j = nT;
        for (int g = 1; g < nO; ++g)
            if (rr >= s_seg[nT + g]) j = nT + g;
        idx = rr - s_seg[j];
    };

    // ---- factors ----
    if (!HIST) {
        // a group of Wd lanes per row, the lanes along the row; the groups take (particle, transition node) and (particle, observation row)
        const int Wd = a.jw, kl = lane & (Wd - 1), gid = tid / Wd, ngroups = 256 / Wd;
        const int per = nT + RL, items = nloc * per;
        for (int it0 = 0; it0 < items; it0 += ngroups) {
            const bool valid = it0 + gid < items;
            const int it = valid ? it0 + gid : 0, i = it / per, x = it - i * per;
            const float* rec = r.rec + (size_t)(i0 + i) * r.stride;
            int j, idx;
            if (x < nT) { j = x; idx = row_index(j, s_st[i], s_mask[i * nn + j]); }
            else obs_place(x - nT, j, idx);
            const int len = s_out[j], row = s_off[j] + idx * len;
            double sum = 0.0;
            for (int k = kl; k < len; k += Wd) sum += valid ? (double)record_count<RF>(P, D, rec, row + k) : 0.0;
            sum = probe_lanes_sum(sum, Wd);
            if (!valid) continue;
            if (x < nT) {
                for (int k = kl; k < len; k += Wd) s_P[(size_t)i * TL + s_seg[j] + k] = sum > 0.0 ? (double)record_count<RF>(P, D, rec, row + k) / sum : 0.0;
            } else if (kl == 0)
                s_L[(size_t)i * RL + (x - nT)] = sum > 0.0 ? (double)record_count<RF>(P, D, rec, row + s_val[j]) / sum : 0.0;
        }
    } else {
        // a particle's row = the prior row of its own parent set + what its entries of the action added.  The prior's observation rows are
        // the same for every particle: their sums and counts at o_g once per workgroup, then a copy per particle that its entries raise
        const HistLayout GL(P.gw_N, P.gw_G, P.A);
        for (int rr = tid; rr < RL; rr += 256) {
            int j, idx;
            obs_place(rr, j, idx);
            double sum = 0.0, at = 0.0;
            if (HIST == 2) {
                const TabRows T(P);
                const int trow = P.A * S + act * S + idx;
                for (int ip = (int)T.ptr[trow]; ip < (int)T.ptr[trow + 1]; ++ip) {
                    const uint2 pc = T.col[ip];
                    sum += (double)__uint_as_float(pc.y);
                    if ((int)pc.x == s_val[j]) at = (double)__uint_as_float(pc.y);
                }
            } else {
                const float* pr = HIST == 1 ? probe_gw_prior_row(P, GL, act, j, false, idx) : D.prior_dense + s_off[j] + idx * s_out[j];
                for (int k = 0; k < s_out[j]; ++k) sum += (double)pr[k];
                at = (double)pr[s_val[j]];
            }
            s_ps[rr] = sum; s_pn[rr] = at;
        }
        if (HIST == 2)
            for (int x = tid; x < nloc * TL; x += 256) s_P[x] = 0.0;
        __syncthreads();
        if (HIST == 2) {
            const TabRows T(P);
            for (int i = tid; i < nloc; i += 256) {
                const int trow = s_st[i] * P.A + act;
                for (int ip = (int)T.ptr[trow]; ip < (int)T.ptr[trow + 1]; ++ip) {
                    const uint2 pc = T.col[ip];
                    if (pc.x < (uint32_t)TL) s_P[(size_t)i * TL + pc.x] = (double)__uint_as_float(pc.y);
                }
            }
        } else
            for (int x = tid; x < nloc * nT; x += 256) {
                const int i = x / nT, j = x - i * nT;
                const uint32_t mask = s_mask[i * nn + j];
                const int idx = row_index(j, s_st[i], mask);
                const float* pr = HIST == 1 ? probe_gw_prior_row(P, GL, act, j, s_var[j] >= 0 && ((mask >> 2) & 1u), idx) : D.prior_dense + s_off[j] + idx * s_out[j];
                for (int k = 0; k < s_out[j]; ++k) s_P[(size_t)i * TL + s_seg[j] + k] = (double)pr[k];
            }
        for (int x = tid; x < nloc * RL; x += 256) {
            const int rr = x % RL;
            s_L[x] = s_ps[rr]; s_num[x] = s_pn[rr];
        }
        __syncthreads();
        // one thread per particle walks its entries of the action: every distinct cell once, with its multiplicity
        const HistDims dims = hist_dims<(HIST ? HIST : 1)>(P, P.ca);
        const int j0 = act < 4 ? hist_offset(r.cnt, act) : 0, na = act < 4 ? hist_count(r.cnt, act) : 0;
        for (int i = tid; i < nloc; i += 256) {
            const uint32_t* rec = reinterpret_cast<const uint32_t*>(r.rec + (size_t)(i0 + i) * r.stride);
            int rb[HIST_ENTRY_CELLS], len[HIST_ENTRY_CELLS];
#pragma unroll
            for (int k = 0; k < HIST_ENTRY_CELLS; ++k) {
                const int j = probe_slot_node<HIST>(k, nT, nO);
                rb[k] = 0; len[k] = 0;
                if (j >= 0 && j < nT) {
                    rb[k]  = s_off[j] + row_index(j, s_st[i], s_mask[i * nn + j]) * s_out[j];
                    len[k] = s_out[j];
                } else if (j >= nT) {
                    rb[k]  = s_off[j];
                    len[k] = a.rows[j] * s_out[j];
                }
            }
            hist_distinct_cells<(HIST ? HIST : 1), HIST_ENTRY_CELLS>(dims, rec, rec[1], act, j0, na, rb, len, [&](int k, int rel, int mult) {
                const int j = probe_slot_node<HIST>(k, nT, nO);
                if (j < nT) {
                    double* cell = &s_P[(size_t)i * TL + s_seg[j] + rel];
                    *cell = (double)probe_raised((float)*cell, mult);
                    return;
                }
                const int out = s_out[j], rr = rel / out, v = rel - rr * out;
                const size_t x = (size_t)i * RL + s_seg[j] + rr;
                if (HIST == 3) {   // the prior's count after `mult` single additions of 1.0f, which need not be prior + mult
                    const float p0 = D.prior_dense[rb[k] + rel], pv = probe_raised(p0, mult);
                    s_L[x] += (double)pv - (double)p0;
                    if (v == s_val[j]) s_num[x] = (double)pv;
                } else {
                    s_L[x] += (double)mult;
                    if (v == s_val[j]) s_num[x] += (double)mult;
                }
            });
        }
        __syncthreads();
        for (int x = tid; x < nloc * nT; x += 256) {
            const int i = x / nT, j = x - i * nT;
            double* row = &s_P[(size_t)i * TL + s_seg[j]];
            double sum = 0.0;
            for (int k = 0; k < s_out[j]; ++k) sum += row[k];
            for (int k = 0; k < s_out[j]; ++k) row[k] = sum > 0.0 ? row[k] / sum : 0.0;
        }
        for (int x = tid; x < nloc * RL; x += 256) s_L[x] = s_L[x] > 0.0 ? s_num[x] / s_L[x] : 0.0;
    }
    __syncthreads();

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
    ve = probe_lanes_sum(ve, 64);
    vn = probe_lanes_sum(vn, 64);
    vp = probe_lanes_sum(vp, 64);
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
    const SlotRecs r = slot_recs(P, D, e);
    double lw = 0.0;
    for (int i = tid; i < P.N; i += 256) lw += particle_weight(P, D, r, i);
    s_part[tid] = lw;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) s_part[tid] += s_part[tid + st];
        __syncthreads();
    }
    if (tid != 0) return;
    const double W = s_part[0];
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
    const unsigned long long idx = atomicAdd(a.seen, 1ull);   // every record is counted, those below the capacity are kept
    if (idx < (unsigned long long)a.capacity) a.recs[idx] = rec;
}

void launch_belief_probe(const Problem& P, const DeviceState& D, const BeliefProbeArgs& a, hipStream_t st)
{
    const size_t lds = forecast_lds_bytes(a.TL, a.RL, a.nT + a.nO, a.chunk, P.hist != 0);
    const dim3 grid(ceil_div(P.N, a.chunk), a.count), block(256);
    if (P.hist == 3) hipLaunchKernelGGL(probe_chunk_kernel<7>, grid, block, lds, st, P, D, a);
    else if (P.hist == 2) hipLaunchKernelGGL(probe_chunk_kernel<6>, grid, block, lds, st, P, D, a);
    else if (P.hist) hipLaunchKernelGGL(probe_chunk_kernel<5>, grid, block, lds, st, P, D, a);
    else if (P.ft_packed) {
        if (a.ft_FS == 2) hipLaunchKernelGGL(probe_chunk_kernel<2>, grid, block, lds, st, P, D, a);
        else if (a.ft_FS == 3) hipLaunchKernelGGL(probe_chunk_kernel<3>, grid, block, lds, st, P, D, a);
        else hipLaunchKernelGGL(probe_chunk_kernel<4>, grid, block, lds, st, P, D, a);
    } else if (P.packed) hipLaunchKernelGGL(probe_chunk_kernel<1>, grid, block, lds, st, P, D, a);
    else hipLaunchKernelGGL(probe_chunk_kernel<0>, grid, block, lds, st, P, D, a);
    hipLaunchKernelGGL(probe_finish_kernel, dim3(a.count), block, 0, st, P, D, a);
}

}  // namespace fba
