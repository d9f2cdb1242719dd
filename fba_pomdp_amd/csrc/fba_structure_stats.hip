// fba_structure_stats.hip -- fba_structure_stats: the graph posterior per step of every run, reduced on the device inside the tick into one
// bin per (episode, t) (include/fba_hip.h).  Launched by tick() between env_kernel and the belief update, beside the probe: the one place
// where adv, episode and t address the step and the main filter has not yet seen it.  Only while the statistics are on.
//
//   struct_stats_slot_kernel   one workgroup per slot, gone at once where the slot took no step (adv == 0).  Otherwise the slot's main
//                              filter reduced in LDS as structures_kernel reduces it (fba_structures.hip; the key word of a record and
//                              the table's claim-or-find rounds are those of fba_structures_table.h): weight total, the histograms per
//                              (word, parent set), mass and particle count per query, the table for `distinct`.  One row per slot goes
//                              to StructStatsArgs::rows -- every mass already divided by W, so that a row is what the step adds to its bin.
//                              LDS: the table's hashes and representatives (24 KB; no masses: no top list is kept), STRUCT_HIST_CELLS
//                              histogram cells (8 KB) and the queries -- 32 KB and a little, four workgroups to a CU.
//   struct_stats_bins_kernel   the rows into the bins the way step_stats_kernel does it (fba_step_stats.hip): a workgroup takes
//                              STRUCT_STATS_GROUP_SLOTS slots and keeps a partial row for every bin of a window in LDS --
//                                clear     the window
//                                add       consecutive lanes add consecutive words of a slot's row to the row of its bin with LDS atomics
//                                          (u64 adds, f64 adds, a max): slots that advance in lock-step share a bin
//                                flush     consecutive lanes add consecutive non-zero words of the window to the bins: at most one global
//                                          atomic per workgroup, bin and word
//                              A window is win_rows bins by cols words (StructStatsArgs); where the bins or a row exceed it, the rows are
//                              read again per window.
//
// A translation unit of its own, outside the parity path: the order of the fp64 additions is the hardware's.  Read-only on the context: it
// writes the rows and bins of StructStatsArgs only.
#include "fba_structures_table.h"

namespace fba {

static_assert(sizeof(fba_structure_stat) == STRUCT_STATS_BIN_HEAD * 8, "fba_structure_stat is the head of a bin");
static_assert(offsetof(fba_structure_stat, distinct_sum) == 4 * 8 && offsetof(fba_structure_stat, distinct_max) == 5 * 8, "the words of a bin's head");
constexpr int W_STEPS = 0, W_WEIGHTLESS = 1, W_OVERFLOWED = 2, W_COLLAPSED = 3, W_DISTINCT_SUM = 4, W_DISTINCT_MAX = 5;
constexpr unsigned long long ROW_WEIGHTLESS = 1ull << 32, ROW_OVERFLOWED = 1ull << 33;

__global__ void __launch_bounds__(STRUCT_STATS_BLOCK) struct_stats_slot_kernel(Problem P, DeviceState D, StructStatsArgs a)
{
    __shared__ unsigned long long s_hash[STRUCT_TABLE];
    __shared__ int s_rep[STRUCT_TABLE];
    __shared__ double s_hist[STRUCT_HIST_CELLS];
    __shared__ double s_qm[FBA_STRUCT_STATS_MAX_QUERIES];
    __shared__ int s_qc[FBA_STRUCT_STATS_MAX_QUERIES];
    __shared__ double s_tot;
    __shared__ int s_flag[2];   // overflow, distinct

    const int b = blockIdx.x, e = a.first + b, tid = threadIdx.x;
    const int nw = a.n_words, ns = a.n_sets, nk = a.n_keys, nq = a.nq;
    unsigned long long* row = a.rows + (size_t)b * (size_t)(STRUCT_STATS_SLOT_HEAD + a.row_words - STRUCT_STATS_BIN_HEAD);
    // the step: taken in this tick (budgeted searches: by the slots whose search finished), at a position that has a bin
    const int bin = D.adv[e] != 0 ? D.episode[e] * P.horizon + D.t[e] : -1;
    if ((unsigned)bin >= (unsigned)a.n_bins) {   // (the whole workgroup: nothing of the slot is read, nothing of the row but this word is)
        if (tid == 0) row[0] = 0ull;
        return;
    }
    const int tile = min(nw, STRUCT_HIST_CELLS / ns);   // words whose histograms one pass keeps (n_sets <= 256: four at least)
    for (int k = tid; k < STRUCT_TABLE; k += STRUCT_STATS_BLOCK) { s_hash[k] = STRUCT_HASH_FREE; s_rep[k] = -1; }
    for (int k = tid; k < STRUCT_HIST_CELLS; k += STRUCT_STATS_BLOCK) s_hist[k] = 0.0;
    if (tid < FBA_STRUCT_STATS_MAX_QUERIES) { s_qm[tid] = 0.0; s_qc[tid] = 0; }
    if (tid == 0) { s_tot = 0.0; s_flag[0] = 0; s_flag[1] = 0; }
    __syncthreads();

    const SlotRecs r = slot_recs(P, D, e);
    BeliefSummaryArgs sa{};   // (record_mask_word asks it where the words stand)
    sa.ncounts = a.ncounts;

    // ---- first pass over the slot: weight total, the histograms of the first `tile` words, the queries, the table
    double lw = 0.0;
    for (int base = 0; base < P.N; base += STRUCT_STATS_BLOCK) {   // (every thread makes every trip: the table's rounds hold barriers)
        const int i     = base + tid;
        const bool live = i < P.N;
        const float* rec = r.rec + (size_t)(live ? i : 0) * r.stride;
        const double w   = live ? particle_weight(P, D, r, i) : 0.0;
        const auto key   = [&](int m) { return record_key_word(P, nw, a.ncounts, rec, m); };
        lw += w;
        if (live) {
            for (int m = 0; m < tile; ++m) {
                const uint32_t v = record_mask_word(P, sa, rec, m);
                if (v < (uint32_t)ns) unsafeAtomicAdd(&s_hist[m * ns + (int)v], w);
            }
            for (int q = 0; q < nq; ++q) {
                const uint32_t* qw = a.query + (size_t)q * nk;
                bool same = true;
                for (int m = 0; m < nk && same; ++m) same = key(m) == qw[m];
                if (same) {
                    unsafeAtomicAdd(&s_qm[q], w);
                    atomicAdd(&s_qc[q], 1);
                }
            }
        }
        const unsigned long long h = live ? struct_hash(key, nk, a.hash_keep) : 0ull;
        struct_table_rounds<STRUCT_TABLE>(s_hash, nullptr, s_rep, nullptr, &s_flag[0], live, i, w, h, key,
                                          [&](int rp, int m) { return record_key_word(P, nw, a.ncounts, r.rec + (size_t)rp * r.stride, m); }, nk);
    }
    unsafeAtomicAdd(&s_tot, lw);
    __syncthreads();
    const double W = s_tot;
    const bool weighs = W > 0.0 && W <= DBL_MAX;   // (finite and positive: neither NaN nor an infinity passes)

    // ---- the queries: mass / W, held, sole
    unsigned long long* payload = row + STRUCT_STATS_SLOT_HEAD;
    const size_t cells = (size_t)nw * ns;
    if (tid < nq) {
        payload[cells + tid]          = (unsigned long long)__double_as_longlong(weighs ? s_qm[tid] / W : 0.0);
        payload[cells + nq + tid]     = s_qc[tid] > 0 ? 1ull : 0ull;
        payload[cells + 2 * nq + tid] = s_qc[tid] == P.N ? 1ull : 0ull;
    }
    // ---- the histograms: the first tile is there, each further one is a pass of its own
    for (int m0 = 0; m0 < nw; m0 += tile) {
        const int mw = min(tile, nw - m0);
        if (m0 > 0) {
            __syncthreads();
            for (int k = tid; k < mw * ns; k += STRUCT_STATS_BLOCK) s_hist[k] = 0.0;
            __syncthreads();
            for (int i = tid; i < P.N; i += STRUCT_STATS_BLOCK) {
                const float* rec = r.rec + (size_t)i * r.stride;
                const double w   = particle_weight(P, D, r, i);
                for (int m = 0; m < mw; ++m) {
                    const uint32_t v = record_mask_word(P, sa, rec, m0 + m);
                    if (v < (uint32_t)ns) unsafeAtomicAdd(&s_hist[m * ns + (int)v], w);
                }
            }
            __syncthreads();
        }
        for (int k = tid; k < mw * ns; k += STRUCT_STATS_BLOCK)
            payload[(size_t)m0 * ns + k] = (unsigned long long)__double_as_longlong(weighs ? s_hist[k] / W : 0.0);
    }
    // ---- the table: how many structures
    int mine = 0;
    for (int k = tid; k < STRUCT_TABLE; k += STRUCT_STATS_BLOCK) mine += s_hash[k] != STRUCT_HASH_FREE ? 1 : 0;
    if (mine) atomicAdd(&s_flag[1], mine);
    __syncthreads();
    if (tid == 0) {
        row[0] = (unsigned long long)(uint32_t)(bin + 1) | (weighs ? 0ull : ROW_WEIGHTLESS) | (s_flag[0] ? ROW_OVERFLOWED : 0ull);
        row[1] = (unsigned long long)(uint32_t)s_flag[1];
    }
}

// word c of a bin, by what is added to it
__device__ __forceinline__ bool bin_word_is_f64(int c, int f64_end) { return c >= STRUCT_STATS_BIN_HEAD && c < f64_end; }

__global__ void __launch_bounds__(STRUCT_STATS_BINS_BLOCK) struct_stats_bins_kernel(StructStatsArgs a)
{
    extern __shared__ unsigned long long s_tab[];   // [a.win_rows][a.cols]
    const int tid = threadIdx.x;
    const int RW = a.row_words, SW = STRUCT_STATS_SLOT_HEAD + RW - STRUCT_STATS_BIN_HEAD;
    const int f64_end = STRUCT_STATS_BIN_HEAD + a.n_words * a.n_sets + a.nq;   // the set and query fractions; counts behind them
    const int s0 = blockIdx.x * STRUCT_STATS_GROUP_SLOTS, n_slots = min(STRUCT_STATS_GROUP_SLOTS, a.count - s0);
    for (int c0 = 0; c0 < RW; c0 += a.cols) {
        const int cw = min(a.cols, RW - c0);
        for (int base = 0; base < a.n_bins; base += a.win_rows) {
            const int rows = min(a.win_rows, a.n_bins - base), words = rows * cw;
            // ---- clear ----
            for (int i = tid; i < words; i += STRUCT_STATS_BINS_BLOCK) s_tab[i] = 0;
            __syncthreads();
            // ---- add: word c of slot s's row ----
            for (int k = tid; k < n_slots * cw; k += STRUCT_STATS_BINS_BLOCK) {
                const int s = k / cw, c = c0 + (k - s * cw);
                const unsigned long long* sr = a.rows + (size_t)(s0 + s) * SW;
                const unsigned long long hd = sr[0];
                const int bin = (int)(uint32_t)hd - 1 - base;
                if ((unsigned)bin >= (unsigned)rows) continue;   // (no step, or another window's)
                unsigned long long* cell = s_tab + bin * cw + (c - c0);
                if (c >= STRUCT_STATS_BIN_HEAD) {
                    const unsigned long long v = sr[STRUCT_STATS_SLOT_HEAD + c - STRUCT_STATS_BIN_HEAD];
                    if (c < f64_end) {
                        const double x = __longlong_as_double((long long)v);
                        if (x != 0.0) unsafeAtomicAdd(reinterpret_cast<double*>(cell), x);
                    } else if (v) atomicAdd(cell, v);
                    continue;
                }
                const int distinct  = (int)(uint32_t)sr[1];
                const bool overflow = (hd & ROW_OVERFLOWED) != 0;
                unsigned long long v = 0;
                if (c == W_STEPS) v = 1;
                else if (c == W_WEIGHTLESS) v = (hd & ROW_WEIGHTLESS) ? 1 : 0;
                else if (c == W_OVERFLOWED) v = overflow ? 1 : 0;
                else if (c == W_COLLAPSED) v = distinct == 1 && !overflow ? 1 : 0;
                else if (c == W_DISTINCT_SUM) v = (unsigned long long)distinct;
                else { if (distinct > 0) atomicMax(reinterpret_cast<int*>(cell), distinct); continue; }
                if (v) atomicAdd(cell, v);
            }
            __syncthreads();
            // ---- flush ----
            for (int i = tid; i < words; i += STRUCT_STATS_BINS_BLOCK) {
                const unsigned long long v = s_tab[i];
                if (!v) continue;
                const int rw = i / cw, c = c0 + (i - rw * cw);
                unsigned long long* g = a.bins + (size_t)(base + rw) * RW + c;
                if (c == W_DISTINCT_MAX) atomicMax(reinterpret_cast<int*>(g), (int)(uint32_t)v);
                else if (bin_word_is_f64(c, f64_end)) unsafeAtomicAdd(reinterpret_cast<double*>(g), __longlong_as_double((long long)v));
                else atomicAdd(g, v);
            }
            __syncthreads();   // (the next window clears the table)
        }
    }
}

void launch_structure_stats(const Problem& P, const DeviceState& D, const StructStatsArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(struct_stats_slot_kernel, dim3(a.count), dim3(STRUCT_STATS_BLOCK), 0, st, P, D, a);
    const size_t lds = (size_t)a.win_rows * a.cols * 8;
    hipLaunchKernelGGL(struct_stats_bins_kernel, dim3(ceil_div(a.count, STRUCT_STATS_GROUP_SLOTS)), dim3(STRUCT_STATS_BINS_BLOCK), lds, st, a);
}

}  // namespace fba
