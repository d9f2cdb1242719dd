// fba_step_stats.hip -- fba_step_stats: what the runs do step by step, reduced on the device inside the tick into one fba_step_stat per
// (episode, t) (include/fba_hip.h).  Launched by tick() behind the belief update (update_count is written by the update kernels) and in
// front of advance_kernel (DeviceState::t / episode still address the step), only while the statistics are on.
//
//   step_stats_kernel   few, large workgroups stride over the slots, one slot per thread and pass.  A slot took its step in this tick iff
//                       adv != 0 (budgeted searches: only the slots whose search finished).  Nothing is added to a bin per slot: a
//                       workgroup keeps a partial row for EVERY bin in LDS -- rows of the words a model of A actions can touch, 19 + 2 A
//                       of the 67, so the 200 bins of 20 episodes x 10 steps of the tiger are 40 KB --
//                         clear     the table
//                         add       each thread adds its slot's step to the row of its bin with LDS atomics (u64 adds, f64 adds, max):
//                                   slots of one workgroup differ in (episode, t) as soon as episodes end at different steps -- the
//                                   headline shape meets over a hundred bins in a launch -- and where they do not, a wave's adds to one
//                                   LDS word cost it tens of cycles, not a trip to L2
//                         flush     consecutive lanes add consecutive non-zero words of the table to the bins: u64 adds, f64 adds and an
//                                   atomicMax on the three maxima -- at most one add per workgroup, bin and word
//                       Where the bins do not fit STEP_STATS_LDS they are served a window of rows at a time, the slots read again per
//                       window (adv, episode and t only for the slots of another window).
//
// From DeviceState::cur the kernel reads what every search and update kernel writes whatever the trace (n_nodes, tree_depth, root_n,
// root_q, update_count); the reward and the terminal flag come from DeviceState::step_scratch, which env_kernel fills, the action from
// DeviceState::action.  update_count of a terminal step is stale while the trace is off, and is not read.  The probe's per-slot values of
// this tick come from BeliefProbeArgs::step, whose mark is cleared here.  A translation unit of its own, outside the parity path;
// read-only on the context but for that mark: it writes the bins of StepStatsArgs only.
#include <stddef.h>

#include "fba_kernels_common.h"

namespace fba {

constexpr int ROW_WORDS = (int)(sizeof(fba_step_stat) / 8);   // a bin as 8-byte words
// the words of a row by what is added to them: the maxima stand as pairs of int32, the double sums behind them and behind the probe's counts
constexpr int W_ACTION = 2, W_VISITS = W_ACTION + FBA_MAX_ACTIONS, W_NODES = W_VISITS + FBA_MAX_ACTIONS, W_DEPTH = W_NODES + 1,
              W_ATT_STEPS = W_DEPTH + 1, W_ATT_SUM = W_ATT_STEPS + 1, W_MAX = W_ATT_SUM + 1, W_REWARD = W_MAX + 2, W_VALUE = W_REWARD + 2,
              W_PROBED = W_VALUE + 2, W_EVIDENCE = W_PROBED + 2;
static_assert(sizeof(fba_step_stat) == 536 && ROW_WORDS == 67, "fba_step_stat is 67 words of 8 bytes");
static_assert(offsetof(fba_step_stat, action) == W_ACTION * 8 && offsetof(fba_step_stat, root_visits) == W_VISITS * 8 &&
              offsetof(fba_step_stat, nodes_sum) == W_NODES * 8 && offsetof(fba_step_stat, attempts_steps) == W_ATT_STEPS * 8 &&
              offsetof(fba_step_stat, nodes_max) == W_MAX * 8 && offsetof(fba_step_stat, reward_sum) == W_REWARD * 8 &&
              offsetof(fba_step_stat, value_sum) == W_VALUE * 8 && offsetof(fba_step_stat, probed) == W_PROBED * 8 &&
              offsetof(fba_step_stat, evidence_sum) == W_EVIDENCE * 8 && offsetof(fba_step_stat, post_ratio_sum) == (ROW_WORDS - 1) * 8,
              "the words of a row follow the members of fba_step_stat");
__device__ __forceinline__ bool word_is_max(int w) { return w == W_MAX || w == W_MAX + 1; }
__device__ __forceinline__ bool word_is_f64(int w) { return (w >= W_REWARD && w < W_PROBED) || w >= W_EVIDENCE; }

// a row of the LDS table holds the words a model of A actions can touch: {steps, terminals}, action[A], root_visits[A], then the TAIL words
// from nodes_sum on.  Word c of such a row is word row_word(c, A) of the bin
constexpr int TAIL = ROW_WORDS - W_NODES;
static_assert(TAIL == STEP_STATS_ROW_TAIL, "step_stats_row_words counts the words behind root_visits");
__device__ __forceinline__ int row_word(int c, int A)
{
    if (c < 2 + A) return c;
    if (c < 2 + 2 * A) return W_VISITS + (c - 2 - A);
    return W_NODES + (c - 2 - 2 * A);
}

__device__ __forceinline__ void row_add(unsigned long long* row, int c, unsigned long long v) { if (v) atomicAdd(&row[c], v); }
__device__ __forceinline__ void row_add(unsigned long long* row, int c, double v) { if (v != 0.0) unsafeAtomicAdd(reinterpret_cast<double*>(&row[c]), v); }
__device__ __forceinline__ void row_max(unsigned long long* row, int c, int half, int v) { if (v > 0) atomicMax(reinterpret_cast<int*>(&row[c]) + half, v); }

__global__ void __launch_bounds__(STEP_STATS_BLOCK) step_stats_kernel(Problem P, DeviceState D, StepStatsArgs a)
{
    extern __shared__ unsigned long long s_tab[];   // [a.rows][RW]
    const int tid = threadIdx.x;
    const int A = min(P.A, FBA_MAX_ACTIONS), RW = step_stats_row_words(P.A), T0 = 2 + 2 * A;   // T0: where the tail of a row starts
    for (int base = 0; base < a.n_bins; base += a.rows) {
        const int rows = min(a.rows, a.n_bins - base), words = rows * RW;
        // ---- clear ----
        for (int i = tid; i < words; i += STEP_STATS_BLOCK) s_tab[i] = 0;
        __syncthreads();
        // ---- add: the slot's step, as its trace record has it ----
        for (long long el = (long long)blockIdx.x * STEP_STATS_BLOCK + tid; el < P.E; el += (long long)gridDim.x * STEP_STATS_BLOCK) {
            const int e = (int)el;
            if (D.adv[e] == 0) continue;
            const int bin = D.episode[e] * P.horizon + D.t[e] - base;
            if ((unsigned)bin >= (unsigned)rows) continue;   // (another window's, or no bin at all)
            unsigned long long* row = s_tab + bin * RW;
            const fba_trace_rec& c = D.cur[e];
            const StepScratch sc  = D.step_scratch[e];
            const int act = D.action[e], nodes = c.n_nodes, depth = c.tree_depth;
            const int upd = sc.terminal ? -1 : c.update_count;   // (stale behind a terminal step while the trace is off; the trace record holds -1 there)
            const double r = sc.reward, q = (unsigned)act < (unsigned)FBA_MAX_ACTIONS ? c.root_q[act] : 0.0;
            row_add(row, 0, 1ull);
            row_add(row, 1, sc.terminal ? 1ull : 0ull);
            if ((unsigned)act < (unsigned)A) row_add(row, 2 + act, 1ull);
            for (int k = 0; k < A; ++k) row_add(row, 2 + A + k, (unsigned long long)(long long)c.root_n[k]);
            row_add(row, T0 + 0, (unsigned long long)(long long)nodes);
            row_add(row, T0 + 1, (unsigned long long)(long long)depth);
            if (upd >= 0) { row_add(row, T0 + 2, 1ull); row_add(row, T0 + 3, (unsigned long long)upd); }
            row_max(row, T0 + 4, 0, nodes); row_max(row, T0 + 4, 1, depth); row_max(row, T0 + 5, 0, upd);
            row_add(row, T0 + 6, r); row_add(row, T0 + 7, r * r);
            row_add(row, T0 + 8, q); row_add(row, T0 + 9, q * q);
            const long long pe = el - a.probe_first;
            if (pe >= 0 && pe < a.probe_count) {
                double* ps = a.probe_step + (size_t)pe * PROBE_STEP_WORDS;
                if (ps[3] != 0.0) {
                    ps[3] = 0.0;   // the mark: consumed
                    const double ev = ps[0];
                    row_add(row, T0 + 10, 1ull);
                    row_add(row, T0 + 11, ev == 0.0 ? 1ull : 0ull);
                    row_add(row, T0 + 12, ev);
                    if (ev > 0.0) {
                        const double lev = det_log(ev);
                        row_add(row, T0 + 13, lev); row_add(row, T0 + 14, lev * lev);
                        row_add(row, T0 + 16, ps[2] / ev);
                    }
                    row_add(row, T0 + 15, ps[1]);
                }
            }
        }
        __syncthreads();
        // ---- flush ----
        for (int i = tid; i < words; i += STEP_STATS_BLOCK) {
            const unsigned long long v = s_tab[i];
            if (!v) continue;
            const int rw = i / RW, w = row_word(i - rw * RW, A);
            unsigned long long* g = reinterpret_cast<unsigned long long*>(a.bins + base + rw) + w;
            if (word_is_max(w)) {
                const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
                if (lo > 0) atomicMax(reinterpret_cast<int*>(g), lo);
                if (hi > 0) atomicMax(reinterpret_cast<int*>(g) + 1, hi);
            } else if (word_is_f64(w)) unsafeAtomicAdd(reinterpret_cast<double*>(g), __longlong_as_double((long long)v));
            else atomicAdd(g, v);
        }
        __syncthreads();   // (the next window clears the table)
    }
}

void launch_step_stats(const Problem& P, const DeviceState& D, const StepStatsArgs& a, hipStream_t st)
{
    const int groups = ceil_div(P.E, STEP_STATS_BLOCK) < STEP_STATS_GROUPS ? ceil_div(P.E, STEP_STATS_BLOCK) : STEP_STATS_GROUPS;
    const size_t lds = (size_t)a.rows * step_stats_row_words(P.A) * 8;
    hipLaunchKernelGGL(step_stats_kernel, dim3(groups), dim3(STEP_STATS_BLOCK), lds, st, P, D, a);
}

}  // namespace fba
