// fba_summary.hip -- fba_belief_summary: the posterior of a range of slots reduced on the device from whatever record format
// the context stores (dense fp32, packed tiger, packed factored tiger, history records), without building a particle's table.
//
//   summary_head_kernel     weight totals, state mass, parent-set masses           one workgroup per slot
//   summary_cols_kernel     weighted column sum of dense / packed records          one thread per cell, particles in index order
//   summary_scatter_kernel  history records: w * (what a particle added to a cell)  one thread per particle, fp64 atomics (LDS table, then global)
//   summary_prior_kernel    history records: + the prior part, / weight total      one thread per cell
//
// A translation unit of its own: nothing here is on the parity path (the order of the fp64 additions is the hardware's), and the
// code generation of the search and belief kernels stays what it was.  Read-only on every buffer of the context.
#include "fba_kernels_common.h"

namespace fba {

// ---------------------------------------------------------------------------------------------
// head: sum w, sum w^2, state mass, mass per (mask word, bit) -- and, for the gridworld records, the mass of the particles whose
// x / y node has NO goal parent (the prior part of such a node is a split of the weight mass, summary_prior_kernel).
// Dynamic LDS: [S] doubles where a.lds_states, then [nvar * 9].
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) summary_head_kernel(Problem P, DeviceState D, BeliefSummaryArgs a)
{
    extern __shared__ double s_dyn[];
    __shared__ double s_tot[2];
    const int b = blockIdx.x, e = a.first + b, tid = threadIdx.x;
    double* s_state = s_dyn;
    double* s_edge  = s_dyn + (a.lds_states ? P.S : 0);
    const int n_edge = a.edge_mass ? a.nvar * 9 : 0;
    if (tid < 2) s_tot[tid] = 0.0;
    if (a.lds_states)
        for (int k = tid; k < P.S; k += 256) s_state[k] = 0.0;
    for (int k = tid; k < n_edge; k += 256) s_edge[k] = 0.0;
    __syncthreads();
    const SlotRecs r = slot_recs(P, D, e);
    const bool lazy  = slot_lazy(D, e);
    double lw = 0.0, lw2 = 0.0;
    for (int i = tid; i < P.N; i += 256) {
        const float* rec = r.rec + (size_t)i * r.stride;
        const double w   = particle_weight(P, D, r, i);
        lw += w;
        lw2 += w * w;
        if (a.state_mass) {
            const int st = lazy ? lazy_state(P, D, e, i) : rec_state(rec, P.C);
            if ((unsigned)st < (unsigned)P.S) {
                if (a.lds_states) unsafeAtomicAdd(&s_state[st], w);
                else unsafeAtomicAdd(&a.state_mass[(size_t)b * P.S + st], w);
            }
        }
        if (n_edge)
            for (int m = 0; m < a.nvar; ++m) {
                const uint32_t mask = record_mask_word(P, a, rec, m);
#pragma unroll
                for (int j = 0; j < MAXF; ++j)
                    if ((mask >> j) & 1u) unsafeAtomicAdd(&s_edge[m * MAXF + j], w);
                if (P.hist && !((mask >> 2) & 1u)) unsafeAtomicAdd(&s_edge[a.nvar * MAXF + m], w);
            }
    }
    unsafeAtomicAdd(&s_tot[0], lw);
    unsafeAtomicAdd(&s_tot[1], lw2);
    __syncthreads();
    if (tid < 2) a.head[(size_t)b * 2 + tid] = s_tot[tid];
    if (a.state_mass && a.lds_states)
        for (int k = tid; k < P.S; k += 256) a.state_mass[(size_t)b * P.S + k] = s_state[k];
    const double total = s_tot[0];
    for (int k = tid; k < n_edge; k += 256) {
        a.edge_mass[(size_t)b * a.nvar * 9 + k] = s_edge[k];
        if (a.edge_prob && k < a.nvar * MAXF) a.edge_prob[(size_t)b * a.nvar * MAXF + k] = s_edge[k] / total;
    }
}

// ---------------------------------------------------------------------------------------------
// dense and packed records: a weighted column sum of the slot's N x C matrix.  A workgroup owns a.cb consecutive cells (a power
// of two, 256 where the table has that many); its 256 / a.cb thread groups take the particles g, g + groups, ... in index order,
// so a wave reads whole consecutive records, and their partial sums are combined in LDS in group order.
// FMT: 0 fp32 counts, 1 packed tiger (PackedView), 2..4 packed factored tiger of that many state features (PackedFtigerView).
// ---------------------------------------------------------------------------------------------
template <int FMT>
__global__ void __launch_bounds__(256) summary_cols_kernel(Problem P, DeviceState D, BeliefSummaryArgs a)
{
    __shared__ double s_part[256];
    const int b = blockIdx.y, e = a.first + b, tid = threadIdx.x;
    const int cl = tid & (a.cb - 1), g = tid / a.cb, groups = 256 / a.cb;
    const int k  = blockIdx.x * a.cb + cl;
    const SlotRecs r = slot_recs(P, D, e);
    double sum = 0.0;
    if (k < a.ncounts) {
#pragma unroll 4
        for (int i = g; i < P.N; i += groups) {
            const float v = record_count<FMT>(P, D, r.rec + (size_t)i * r.stride, k);
            sum += particle_weight(P, D, r, i) * (double)v;
        }
    }
    s_part[tid] = sum;
    __syncthreads();
    if (g == 0 && k < a.dense_C) {
        double tot = 0.0;
        for (int q = 0; q < groups; ++q) tot += s_part[q * a.cb + cl];
        a.mean_counts[(size_t)b * a.dense_C + k] = k < a.ncounts ? tot / a.head[(size_t)b * 2] : 0.0;   // (mask-word positions: 0.0)
    }
}

// ---------------------------------------------------------------------------------------------
// history records: mean = (sum_i w_i prior_i[k] + sum_i w_i delta_i[k]) / W.  delta is non-zero only at the cells a particle's
// entries name, so a thread walks one particle's entries and adds w * delta to the slot's zeroed table with fp64 atomics --
// once per distinct cell, with the cell's multiplicity (hist_distinct_cells, fba_device.h).
// ---------------------------------------------------------------------------------------------
// A workgroup's 256 particles mostly name the same few cells (a filter is resampled after every update, and the slot's particles have
// taken the same actions), so their terms meet in a small LDS table first -- open addressing, a bounded probe, straight to the global
// table where that finds no place -- and a workgroup sends one global atomic per distinct cell.  (Measured without the table: 20 entries
// x 16 384 particles x 256 slots = 5 * 10^8 global fp64 atomics on a few hundred addresses per slot, 25.8 ms)
constexpr int SUMMARY_HASH = 1024, SUMMARY_PROBES = 8;
struct SummaryCellTable {
    int* key;      // [SUMMARY_HASH] cell, -1 = free
    double* val;   // [SUMMARY_HASH]
    double* acc;   // the slot's global table
    __device__ __forceinline__ void add(int c, double v) const
    {
        uint32_t h = ((uint32_t)c * 2654435761u) >> 22;
#pragma unroll 1
        for (int probe = 0; probe < SUMMARY_PROBES; ++probe) {
            const int k = atomicCAS(&key[h], -1, c);
            if (k == -1 || k == c) { unsafeAtomicAdd(&val[h], v); return; }
            h = (h + 1) & (SUMMARY_HASH - 1);
        }
        unsafeAtomicAdd(&acc[c], v);
    }
};
template <int HIST>
__global__ void __launch_bounds__(256) summary_scatter_kernel(Problem P, DeviceState D, BeliefSummaryArgs a)
{
    constexpr int NC = HIST == 2 ? 2 : HIST_ENTRY_CELLS;
    __shared__ int s_key[SUMMARY_HASH];
    __shared__ double s_val[SUMMARY_HASH];
    const int b = blockIdx.y, e = a.first + b, tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    for (int h = tid; h < SUMMARY_HASH; h += 256) { s_key[h] = -1; s_val[h] = 0.0; }
    __syncthreads();
    const SlotRecs r = slot_recs(P, D, e);
    double* acc = a.mean_counts + (size_t)b * a.dense_C;
    const SummaryCellTable tab{s_key, s_val, acc};
    // (more entries than a record has room for: the update kernels report that)
    if (i < P.N && hist_total(r.cnt) <= P.hist_cap) {
        const uint32_t* rec = reinterpret_cast<const uint32_t*>(r.rec + (size_t)i * r.stride);
        const double w      = particle_weight(P, D, r, i);
        const uint32_t mask = rec[1];
        const HistDims dims = hist_dims<HIST>(P, P.ca);
        int rb[NC], len[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) { rb[k] = 0; len[k] = a.ncounts; }   // every cell of the table
        int j0 = 0;
        for (int act = 0; act < P.A && act < 4; ++act) {
            const int na = hist_count(r.cnt, act);
            hist_distinct_cells<HIST, NC>(dims, rec, mask, act, j0, na, rb, len, [&](int, int c, int mult) {
                double delta = (double)mult;
                if (HIST == 3) {   // the prior's count after `mult` single additions of 1.0f, which need not be prior + mult
                    const float p0 = D.prior_dense[c];
                    float v = p0;
                    for (int q = 0; q < mult; ++q) v += 1.0f;
                    delta = (double)v - (double)p0;
                }
                tab.add(c, w * delta);
            });
            j0 += na;
        }
    }
    __syncthreads();
    for (int h = tid; h < SUMMARY_HASH; h += 256) {
        const int c = s_key[h];
        if ((unsigned)c < (unsigned)a.ncounts) unsafeAtomicAdd(&acc[c], s_val[h]);
    }
}

// the prior part of cell k: the weight total times the prior's count -- for the x / y nodes of a gridworld record the prior is the
// particle's own (hist_alt rows with the goal parent, hist_base rows and zero rows beyond N * N without), so the two masses apart
__device__ __forceinline__ double summary_prior_part(const Problem& P, const DeviceState& D, const BeliefSummaryArgs& a, int b, long long k, double W)
{
    if (P.hist != 1) return W * (double)D.prior_dense[k];
    const HistLayout L(P.gw_N, P.gw_G, P.A);
    const int N = L.N, G = L.G, A = L.A;
    const int XY = N * N * G * N, GG = N * N * G * G, NN = N * N, tsz = 2 * XY + GG, osz = 2 * NN + G * G;
    int q = (int)k;
    if (q < A * tsz) {
        const int act = q / tsz;
        q -= act * tsz;
        if (q < 2 * XY) {
            const int f = q / XY, row = (q - f * XY) / N, i = (q - f * XY) % N, m = 2 * act + f;
            const double* em = a.edge_mass + (size_t)b * a.nvar * 9;
            double v = em[m * MAXF + 2] * (double)P.hist_alt[(size_t)(act * 2 + f) * L.XY + row * L.NS + i];
            if (row < NN) v += em[a.nvar * MAXF + m] * (double)P.hist_base[act * L.tstride + f * L.XY + row * L.NS + i];
            return v;
        }
        q -= 2 * XY;
        return W * (double)P.hist_base[act * L.tstride + 2 * L.XY + (q / G) * L.GS + q % G];
    }
    q -= A * tsz;
    const int act = q / osz;
    q -= act * osz;
    const int f = q < NN ? 0 : (q < 2 * NN ? 1 : 2);
    q -= f * NN;
    const int n = f == 2 ? G : N;
    return W * (double)P.hist_base[L.o_row(act, f, q / n) + q % n];
}
__global__ void __launch_bounds__(256) summary_prior_kernel(Problem P, DeviceState D, BeliefSummaryArgs a)
{
    const int b = blockIdx.y;
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.dense_C) return;
    double* cell = a.mean_counts + (size_t)b * a.dense_C + k;
    if (k >= a.ncounts) { *cell = 0.0; return; }   // (mask-word positions)
    const double W = a.head[(size_t)b * 2];
    *cell = (*cell + summary_prior_part(P, D, a, b, k, W)) / W;
}

void launch_belief_summary(const Problem& P, const DeviceState& D, const BeliefSummaryArgs& a, hipStream_t st)
{
    const size_t lds = ((a.lds_states ? (size_t)P.S : 0) + (a.edge_mass ? (size_t)a.nvar * 9 : 0)) * sizeof(double);
    hipLaunchKernelGGL(summary_head_kernel, dim3(a.count), dim3(256), lds, st, P, D, a);
    if (!a.mean_counts) return;
    if (P.hist) {
        const dim3 grid(ceil_div(P.N, 256), a.count);
        if (P.hist == 3) hipLaunchKernelGGL(summary_scatter_kernel<3>, grid, dim3(256), 0, st, P, D, a);
        else if (P.hist == 2) hipLaunchKernelGGL(summary_scatter_kernel<2>, grid, dim3(256), 0, st, P, D, a);
        else hipLaunchKernelGGL(summary_scatter_kernel<1>, grid, dim3(256), 0, st, P, D, a);
        hipLaunchKernelGGL(summary_prior_kernel, dim3((a.dense_C + 255) / 256, a.count), dim3(256), 0, st, P, D, a);
        return;
    }
    const dim3 grid(ceil_div(a.dense_C, a.cb), a.count);
    if (P.ft_packed) {
        if (a.ft_FS == 2) hipLaunchKernelGGL(summary_cols_kernel<2>, grid, dim3(256), 0, st, P, D, a);
        else if (a.ft_FS == 3) hipLaunchKernelGGL(summary_cols_kernel<3>, grid, dim3(256), 0, st, P, D, a);
        else hipLaunchKernelGGL(summary_cols_kernel<4>, grid, dim3(256), 0, st, P, D, a);
    } else if (P.packed) hipLaunchKernelGGL(summary_cols_kernel<1>, grid, dim3(256), 0, st, P, D, a);
    else hipLaunchKernelGGL(summary_cols_kernel<0>, grid, dim3(256), 0, st, P, D, a);
}

}  // namespace fba
