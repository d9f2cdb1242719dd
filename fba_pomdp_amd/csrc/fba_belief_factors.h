// fba_belief_factors.h -- what fba_belief_forecast (fba_forecast.hip) and fba_probe (fba_probe.hip) share on the device: the phase that
// turns a chunk of a slot's particles, in whatever record format the context stores, into fp64 factor tables in LDS -- the only code of
// either kernel that knows the record formats -- with its helpers, the launch ladder over the formats, and the weight total of a slot
// (fba_predict.hip's as well).  The layout both kernels are told is BeliefFactorLayout (fba_kernels.h, filled by factor_layout in
// fba_engine.hip).
#pragma once

#include <type_traits>

#include "fba_kernels_common.h"

namespace fba {

__device__ __forceinline__ double lanes_sum(double v, int width)   // over aligned groups of `width` lanes (a power of two)
{
    for (int off = 1; off < width; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

// the count after `mult` single additions of 1.0f (prior + mult where that is exact, which the history formats of the gridworld require)
__device__ __forceinline__ float raised(float p0, int mult)
{
    float v = p0;
    for (int m = 0; m < mult; ++m) v += 1.0f;
    return v;
}

// the node whose cell an entry holds in cell slot k (hist_entry_cells), or -1
template <int HIST>
__device__ __forceinline__ int slot_node(int k, int nT, int nO)
{
    if (HIST == 3) return k < 4 ? (k < nT ? k : -1) : (k - 4 < nO ? nT + k - 4 : -1);
    return k < nT + nO ? k : -1;
}

// gridworld records: the prior row `idx` of node j (0..2 T(x), T(y), T(goal); 3..5 the observation nodes) in the padded tables
__device__ __forceinline__ const float* gw_prior_row(const Problem& P, const HistLayout& L, int act, int j, bool with_goal, int idx)
{
    if (j >= 3) return P.hist_base + L.o_row(act, j - 3, idx);
    if (j == 2) return P.hist_base + act * L.tstride + 2 * L.XY + idx * L.GS;
    return with_goal ? P.hist_alt + (act * 2 + j) * L.XY + idx * L.NS : P.hist_base + act * L.tstride + j * L.XY + idx * L.NS;
}

// the weights of slot r's N particles, summed by a workgroup of 256 threads in a fixed tree order.  s_part: 256 doubles of LDS, which
// hold the partial sums until the caller's next barrier
__device__ __forceinline__ double slot_weight_total(const Problem& P, const DeviceState& D, const SlotRecs& r, double* s_part)
{
    const int tid = threadIdx.x;
    double lw = 0.0;
    for (int i = tid; i < P.N; i += 256) lw += particle_weight(P, D, r, i);
    s_part[tid] = lw;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) s_part[tid] += s_part[tid + st];
        __syncthreads();
    }
    return s_part[0];
}

// the record format of a context, FMT: 0 fp32 counts, 1 packed tiger, 2..4 packed factored tiger of that many state features (ft_FS;
// record_count), 5..7 history records of Problem::hist = FMT - 4.  The one numbering: the kernels' FMT and the snapshot header's record_format
inline int record_format(const Problem& P, int ft_FS)
{
    if (P.hist) return 4 + P.hist;
    if (P.ft_packed) return ft_FS == 2 ? 2 : (ft_FS == 3 ? 3 : 4);
    return P.packed ? 1 : 0;
}

// calls f(std::integral_constant<int, FMT>) with the record format of the context
template <class F>
void with_record_format(const Problem& P, int ft_FS, F&& f)
{
    switch (record_format(P, ft_FS)) {
        case 7: return f(std::integral_constant<int, 7>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 1: return f(std::integral_constant<int, 1>{});
        default: return f(std::integral_constant<int, 0>{});
    }
}

// what belief_factors leaves in LDS for the caller's own phases
struct FactorViews {
    double* s_P;              // [chunk][TL] p_i's normalised factor rows (the caller's to overwrite)
    const double* s_L;        // [chunk][RL] theta[row][o_g] per observation node and row (written where want_l)
    const double* s_w;        // [chunk] the particle's weight; 0 where its state is outside the model
    const uint32_t* s_mask;   // [chunk][nT + nO] the parent set of node j in particle i
    const NodeRegs* s_nd;     // [nT + nO] node j: the transition nodes of the action, then its observation nodes; off = 0, out = 1
    const int *s_seg, *s_out; // [nT + nO] BeliefFactorLayout::seg; the node's row length
    int nloc;                 // particles of this workgroup's chunk
};

// the static LDS of belief_factors (the node descriptions and five integers per node), beside the FORECAST_LDS bytes of dynamic LDS: a
// caller that declares static LDS of its own asserts that the three still fit
constexpr size_t FACTORS_STATIC_LDS = (sizeof(NodeRegs) + 5 * sizeof(int)) * PREDICT_MAXQN;
static_assert(FACTORS_STATIC_LDS + FORECAST_LDS <= 64 * 1024, "belief_factors: static + dynamic LDS exceed 64 KB");

// The factor tables of the chunk blockIdx.x of slot e's particles, for action `act` and observation `ob`: every thread of a workgroup of
// 256 calls it; it ends with a barrier.  want_l: the observation tables are wanted.  check_room: a history record with more entries than
// it has room for counts as empty (a caller that has not established hist_total < hist_cap itself).  Dynamic LDS: forecast_lds_bytes
// (fba_kernels.h).
template <int FMT>
__device__ __forceinline__ FactorViews belief_factors(const Problem& P, const DeviceState& D, const BeliefFactorLayout& a, int e, int act, int ob,
                                                      bool want_l, bool check_room)
{
    constexpr int HIST = FMT > 4 ? FMT - 4 : 0;
    constexpr int RF   = HIST ? 0 : FMT;   // the record_count of the dense and packed formats
    extern __shared__ double s_dyn[];
    // s_nd holds the description with off = 0, out = 1, so that node_row returns the row's INDEX; the row starts at s_off + index * s_out
    __shared__ NodeRegs s_nd[PREDICT_MAXQN];
    __shared__ int s_off[PREDICT_MAXQN], s_out[PREDICT_MAXQN];
    __shared__ int s_seg[PREDICT_MAXQN];   // where the node's entries start in a particle's transition table / its rows in the observation table
    __shared__ int s_rows[PREDICT_MAXQN];  // rows of the node in the max layout
    __shared__ int s_val[PREDICT_MAXQN];   // observation nodes: the observation's value of the node
    const int tid = threadIdx.x, lane = tid & 63;
    const int nT = a.nT, nO = a.nO, nn = nT + nO, TL = a.TL, RL = a.RL, S = P.S;
    const int i0 = blockIdx.x * a.chunk, nloc = min(a.chunk, P.N - i0);
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
        s_off[j] = nd.off; s_out[j] = nd.out;
        s_seg[j] = a.seg[j]; s_rows[j] = a.rows[j];
        nd.off = 0; nd.out = 1;
        s_nd[j] = nd;
    }
    const SlotRecs r = slot_recs(P, D, e);
    const bool lazy  = slot_lazy(D, e);
    const bool rec_ok = !HIST || !check_room || hist_total(r.cnt) <= P.hist_cap;
    for (int i = tid; i < nloc; i += 256) {
        const float* rec = r.rec + (size_t)(i0 + i) * r.stride;
        const int st     = lazy ? lazy_state(P, D, e, i0 + i) : rec_state(rec, P.C);
        const bool in    = rec_ok && (unsigned)st < (unsigned)S;
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
        if (s_nd[j].var >= 0) mask = HIST ? record_mask_word(P, sa, rec, s_nd[j].var) : __float_as_uint(record_count<RF>(P, D, rec, a.ncounts + s_nd[j].var));
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

    if (!HIST) {
        // a group of Wd lanes per row, the lanes along the row; the groups take (particle, transition node) and (particle, observation row)
        const int Wd = a.jw, kl = lane & (Wd - 1), gid = tid / Wd, ngroups = 256 / Wd;
        const int per = nT + (want_l ? RL : 0), items = nloc * per;
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
            sum = lanes_sum(sum, Wd);
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
        if (want_l)
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
                    const float* pr = HIST == 1 ? gw_prior_row(P, GL, act, j, false, idx) : D.prior_dense + s_off[j] + idx * s_out[j];
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
                const float* pr = HIST == 1 ? gw_prior_row(P, GL, act, j, s_nd[j].var >= 0 && ((mask >> 2) & 1u), idx) : D.prior_dense + s_off[j] + idx * s_out[j];
                for (int k = 0; k < s_out[j]; ++k) s_P[(size_t)i * TL + s_seg[j] + k] = (double)pr[k];
            }
        if (want_l)
            for (int x = tid; x < nloc * RL; x += 256) {
                const int rr = x % RL;
                s_L[x] = s_ps[rr]; s_num[x] = s_pn[rr];
            }
        __syncthreads();
        // one thread per particle walks its entries of the action: every distinct cell once, with its multiplicity
        const HistDims dims = hist_dims<(HIST ? HIST : 1)>(P, P.ca);
        const int j0 = act < 4 ? hist_offset(r.cnt, act) : 0, na = rec_ok && act < 4 ? hist_count(r.cnt, act) : 0;
        for (int i = tid; i < nloc; i += 256) {
            const uint32_t* rec = reinterpret_cast<const uint32_t*>(r.rec + (size_t)(i0 + i) * r.stride);
            int rb[HIST_ENTRY_CELLS], len[HIST_ENTRY_CELLS];
#pragma unroll
            for (int k = 0; k < HIST_ENTRY_CELLS; ++k) {
                const int j = slot_node<HIST>(k, nT, nO);
                rb[k] = 0; len[k] = 0;
                if (j >= 0 && j < nT) {
                    rb[k]  = s_off[j] + row_index(j, s_st[i], s_mask[i * nn + j]) * s_out[j];
                    len[k] = s_out[j];
                } else if (j >= nT && want_l) {
                    rb[k]  = s_off[j];
                    len[k] = s_rows[j] * s_out[j];
                }
            }
            hist_distinct_cells<(HIST ? HIST : 1), HIST_ENTRY_CELLS>(dims, rec, rec[1], act, j0, na, rb, len, [&](int k, int rel, int mult) {
                const int j = slot_node<HIST>(k, nT, nO);
                if (j < nT) {
                    double* cell = &s_P[(size_t)i * TL + s_seg[j] + rel];
                    *cell = (double)raised((float)*cell, mult);
                    return;
                }
                const int out = s_out[j], rr = rel / out, v = rel - rr * out;
                const size_t x = (size_t)i * RL + s_seg[j] + rr;
                if (HIST == 3) {   // the prior's count after `mult` single additions of 1.0f, which need not be prior + mult
                    const float p0 = D.prior_dense[rb[k] + rel], pv = raised(p0, mult);
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
        if (want_l)
            for (int x = tid; x < nloc * RL; x += 256) s_L[x] = s_L[x] > 0.0 ? s_num[x] / s_L[x] : 0.0;
    }
    __syncthreads();
    return {s_P, s_L, s_w, s_mask, s_nd, s_seg, s_out, nloc};
}

}  // namespace fba
