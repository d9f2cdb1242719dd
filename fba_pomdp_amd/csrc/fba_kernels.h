// fba_kernels.h -- launch interface between the host engine and the HIP kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "fba_state.h"

namespace fba {

constexpr int SEARCH_BLOCK  = 64;    // one wave per workgroup, one tree per lane
constexpr int SEARCH_STAGE_WORDS = 128; // particle records up to this many words are staged in LDS by the search
constexpr int ROOT_CHILDREN = 8;        // root child pointers are kept in LDS when A*O is at most this
constexpr int REJECT_BLOCK  = 256;   // attempts per chunk of the rejection filter
// (which kernel a tick launch runs under these limits: search_plan / update_plan / reset_plan, fba_launch_plan.h)
constexpr int TIGER_LDS_MAX_N = 4096;  // reject_tiger_lds_kernel: filters up to this many packed tiger particles are parked in LDS
constexpr int TIGER_ONCE_MIN_N = 3584;  // reject_tiger_once_kernel from here up: 13 N + 8.3 KB of reject_tiger_lds_kernel no longer fit three times into a CU's 160 KB
constexpr int REJECT_MAX_ATTEMPTS = 1 << 28;  // per update: beyond this the observation is taken to be impossible under the filter -- the default of
                                              // Problem::reject_max, which is what the kernels test (fba_giveup_policy sets another)
static_assert(REJECT_MAX_ATTEMPTS % FBA_REJECT_QUANTUM == 0, "the default limit is a multiple of the quantum, like every other");
constexpr int IS_BLOCK      = 512;   // one workgroup per slot in the importance filter (same-box A/B on the bench shape: 1024 -> 37.3 ms, 512 -> 31.1, 256 -> 32.3: three workgroups per CU overlap their barrier-separated phases)
constexpr int PARTICLE_TILE = 4096;  // particles one workgroup initialises / resets
constexpr int CARRY_TILE    = 2048;  // chunk totals staged in LDS per step of the carry chain
constexpr int IS_MAX_CHUNKS = 256;   // 256-element scan chunks per slot => N <= 65536
constexpr int MH_MAXVAR = 128;  // structure words of one particle the MH beliefs' chains handle
constexpr int MH_TERMS  = 1024; // doubles: LogBDScore terms one chain evaluates side by side
constexpr int MH_LDS_HEAD = MH_TERMS * 8 + 2 * MH_MAXVAR * 4 + 64 * 4;  // those terms, two structures, terms per lane
inline bool mh_scratch_in_lds(int scratch_words) { return MH_LDS_HEAD + (size_t)scratch_words * 4 <= 64 * 1024; }  // else [E][words] in HBM
constexpr int IS_LDS_MAX_N  = 8192;  // importance filters up to this many particles keep their weights and prefix sums in LDS (64 KB)

// dynamic LDS of one search_ca_hist_kernel workgroup: the prior and sequence tables, then per lane the path and one staged record
inline size_t ca_hist_search_lds(const Problem& P)
{
    const int depth_cap = P.max_depth > 0 ? P.max_depth : 1;
    return ca_hist_table_bytes(P.hist_row, P.hist_rid_bytes, P.hist_distinct, P.hist_cap) + ((size_t)2 * depth_cap + P.Cs) * SEARCH_BLOCK * sizeof(uint32_t);
}

void launch_search(const Problem& P, const DeviceState& D, hipStream_t st);
void launch_start(const Problem& P, const DeviceState& D, hipStream_t st);
void launch_env(const Problem& P, const DeviceState& D, int32_t* n_active, hipStream_t st);
void launch_advance(const Problem& P, const DeviceState& D, int32_t* n_active, hipStream_t st);
void launch_belief_update(const Problem& P, const DeviceState& D, hipStream_t st);
void launch_init(const Problem& P, const DeviceState& D, hipStream_t st);
void launch_reset(const Problem& P, const DeviceState& D, hipStream_t st);
void launch_materialize_reset(const Problem& P, const DeviceState& D, hipStream_t st);
void launch_materialize_records(const Problem& P, const DeviceState& D, hipStream_t st);   // ... behind the compact filters' expansion (fba_state.h)
void launch_flush(const Problem& P, const DeviceState& D, hipStream_t st);
void launch_selftest_lgamma(const double* x, int count, double* out, hipStream_t st);
void launch_selftest_bd(const Problem& P, const float* cnt, const float* prior, double* out, hipStream_t st);
void launch_selftest_ucb(const double* L, const int32_t* n, int count, double u, double* out, hipStream_t st);
hipError_t launch_take_error();   // a HIP error a launch_* function met on its way (and clears it); hipSuccess if none
// fba_belief_summary (fba_summary.hip): slots [first, first + count) reduced into device buffers of the caller's; a null pointer = that
// output is not wanted.  The caller zeroes the two the kernels accumulate into: state_mass where !lds_states, mean_counts of history records
struct BeliefSummaryArgs {
    int32_t first, count;
    double* head;         // [count][2] sum of weights, sum of squared weights
    double* state_mass;   // [count][S]
    double* mean_counts;  // [count][dense_C]
    double* edge_mass;    // [count][nvar * 9]: mass per (mask word, bit), then per word the mass of the gridworld records without the goal parent
    double* edge_prob;    // [count][nvar][MAXF]
    int32_t dense_C, ncounts, nvar;   // floats of a particle's table as the API speaks of it; the counts among them; the mask words behind those
    int32_t cb;           // dense / packed records: cells per workgroup (a power of two, at most 256)
    int32_t lds_states;   // the state histogram fits LDS
    int32_t ft_FS;        // packed factored tiger: state features
};
void launch_belief_summary(const Problem& P, const DeviceState& D, const BeliefSummaryArgs& a, hipStream_t st);
// fba_belief_predict (fba_predict.hip): nq queries (s, a, s', o) answered for slots [first, first + count) into device buffers of the caller's;
// a null output = not wanted.  History records: the caller zeroes hacc and supplies what the prior contributes (qn, qprior, ent_slot)
constexpr int PREDICT_MAXQN = 16;   // nodes of one query: FS + FO
constexpr int PREDICT_SLOTS = HIST_ENTRY_CELLS;   // entry-cell slots of a history record (hist_entry_cells, fba_device.h)
struct PredictSlotNode {            // the node whose cell an entry holds in slot k, for one query; out = 0: the slot is unused
    int32_t rb0, rb1;               // dense index where the queried row starts, per prior form (form 1: the parent-set bit `var` of the record is set)
    int32_t out, seg, val, var;     // row length; where the row's entries start in [trans | obsp]; the query's own value; parent-set bit or -1
    double prs0, prs1;              // fp64 sum of the prior row, per form
};
struct BeliefPredictArgs {
    int32_t first, count, nq;
    const int32_t *state, *action, *next_state, *obs;   // [nq]
    double *trans, *obsp, *joint;                       // [count][nq][TL], [count][nq][OL], [count][nq]
    double* wtot;                                       // [count] weight totals (written first)
    int32_t TL, OL, nn, nT;     // entries of a query's answer; nodes of a query, the transition nodes among them
    int32_t ncounts, jw, ft_FS; // counts of a particle's table; lanes that share one particle in a joint item (a power of two); packed factored tiger: state features
    const int32_t* seg;         // [nn] where node j's entries start in trans (j < nT) or obsp
    const PredictSlotNode* qn;  // history records: [nq][PREDICT_SLOTS]
    const float* qprior;        // history records: [nq][2][TL + OL] the prior rows of the query per form
    const int32_t* ent_slot;    // history records: [TL + OL] slot of the node an entry belongs to
    double* hacc;               // history records: [count][nq][TL + OL + 2 * PREDICT_SLOTS + 1] raised terms, sum w / R per (slot, form), joint sum
};
void launch_belief_predict(const Problem& P, const DeviceState& D, const BeliefPredictArgs& a, hipStream_t st);
// what the kernels of fba_belief_forecast and fba_probe are told of a model's layout (factor_layout in fba_engine.hip fills it,
// belief_factors in fba_belief_factors.h reads it)
struct BeliefFactorLayout {
    int32_t nT, nO;             // transition / observation nodes of an action (1 / 1 for a tabular model)
    int32_t TL, RL;             // entries of a particle's transition rows; rows of its observation nodes in the max layout
    int32_t chunk;              // particles per workgroup (at most 256)
    int32_t ncounts, jw, ft_FS; // counts of a particle's table; lanes that share one row (a power of two); packed factored tiger: state features
    const int32_t* seg;         // [nT + nO] where node j's entries start among the TL (j < nT), its rows among the RL
    const int32_t* rows;        // [nT + nO] rows of node j in the max layout
};
// fba_belief_forecast (fba_forecast.hip): the one-step predictive of slots [first, first + count) after action[slot] (and under obs[slot])
// into device buffers of the caller's; a null output = not wanted, obs may be null where only next_mass is.  The caller zeroes acc
struct BeliefForecastArgs {
    int32_t first, count;
    const int32_t *action, *obs;                 // [count]
    double *next_mass, *post_mass, *evidence;    // [count][S], [count][S], [count]
    double* acc;                                 // [count][2][S]: sum_i w_i p_i(s'), sum_i w_i p_i(s') l_i(s')
    BeliefFactorLayout lay;
};
constexpr int FORECAST_LDS = 63 * 1024;   // dynamic LDS a forecast workgroup may use (the node descriptions take the rest of 64 KB)
// dynamic LDS of one forecast_chunk_kernel or probe_chunk_kernel workgroup (belief_factors carves it): per particle the fp64 factor tables
// (history records: the observation rows' sums and counts apart), weight, state and a parent-set word per node; history records: the
// prior's observation row sums and counts once
inline size_t forecast_lds_bytes(int TL, int RL, int nn, int chunk, bool hist)
{
    return ((size_t)chunk * ((size_t)TL + (size_t)RL * (hist ? 2 : 1) + 1) + (hist ? (size_t)2 * RL : 0)) * sizeof(double) + (size_t)chunk * (1 + nn) * 4;
}
void launch_belief_forecast(const Problem& P, const DeviceState& D, const BeliefForecastArgs& a, hipStream_t st);
// fba_probe (fba_probe.hip): inside a tick, between the environment step and the belief update -- the evidence of the step that is about to
// be filtered in, for the slots [first, first + count) that have an update pending, from DeviceState::action / obs / env_state.  All state
// of the feature is here: buffers of the context's that fba_probe_enable allocates.  acc is zero between launches (the finish kernel
// leaves it so)
struct BeliefProbeArgs {
    int32_t first, count;
    double* acc;                // [count][3]: sum_i w_i sum_s' p_i(s') l_i(s'), sum_i w_i p_i(s*), sum_i w_i p_i(s*) l_i(s*)
    fba_probe_rec* recs;        // [capacity]
    unsigned long long* seen;   // [1] records written or counted since fba_probe_enable
    int32_t capacity;
    BeliefFactorLayout lay;     // chunk: PROBE_CHUNK, or what the LDS holds if that is fewer: one thread per particle in the evidence phase
    double* step;               // [count][PROBE_STEP_WORDS]: the slot's evidence, next_true, post_true of this tick and a mark (1.0: probed this
                                // tick) for fba_step_stats, whose kernel clears the mark; written whether or not the record fitted the buffer
};
constexpr int PROBE_STEP_WORDS = 4;
// particles per probe workgroup, where the LDS holds more: one wave's worth for the one-thread-per-particle phases, and three to four
// workgroups on a CU instead of the two that a full LDS leaves (same-box A/B on the shapes of scripts/bench_belief_probe.py, cost per
// tick: gridworld 7 history records 104 -> 3.68 ms, 64 -> 2.73, 48 -> 2.91, 32 -> 4.05, 16 -> 7.79; collision avoidance fp32 173 -> 1.83,
// 64 -> 0.75, 32 -> 0.80, 16 -> 0.95)
constexpr int PROBE_CHUNK = 64;
void launch_belief_probe(const Problem& P, const DeviceState& D, const BeliefProbeArgs& a, hipStream_t st);
// fba_step_stats (fba_step_stats.hip): inside a tick, between the belief update and advance_kernel -- the slots that took their step in this
// tick (DeviceState::adv != 0) reduced into the bins (episode, t) their steps belong to.  All state of the feature is here and in
// DeviceState::step_scratch: buffers of the context's that fba_step_stats_enable allocates.  The probe members mirror the BeliefProbeArgs of
// the tick (probe_count = 0: no probe)
struct StepStatsArgs {
    fba_step_stat* bins;        // [n_bins]
    int32_t n_bins;             // episodes * horizon
    int32_t rows;               // rows of a workgroup's LDS table: step_stats_rows bins are served per window
    int32_t probe_first, probe_count;
    double* probe_step;         // BeliefProbeArgs::step
};
constexpr int STEP_STATS_BLOCK  = 1024;  // slots one workgroup reduces per pass: few, large workgroups, so that few rows are added to a bin
constexpr int STEP_STATS_GROUPS = 128;   // workgroups of a launch at most; beyond BLOCK * GROUPS slots they stride
constexpr int STEP_STATS_LDS    = 60 * 1024;   // bytes of a workgroup's table of partial rows
constexpr int STEP_STATS_ROW_TAIL = 17;  // words of fba_step_stat behind root_visits
// 8-byte words of a partial row: {steps, terminals}, action and root_visits of the model's A actions, the tail
__host__ __device__ inline int step_stats_row_words(int A) { return 2 + 2 * (A < FBA_MAX_ACTIONS ? A : FBA_MAX_ACTIONS) + STEP_STATS_ROW_TAIL; }
inline int step_stats_rows(int n_bins, int A) { const int fit = STEP_STATS_LDS / (step_stats_row_words(A) * 8); return n_bins < fit ? n_bins : fit; }
void launch_step_stats(const Problem& P, const DeviceState& D, const StepStatsArgs& a, hipStream_t st);
// fba_giveup_policy, FBA_GIVEUP_RETIRE (fba_retire.hip): inside a tick, between the belief update and flush_kernel -- the slots whose
// rejection update has just given up (DeviceState::gave_up) are reported and their runs ended.  The list is the context's
// (fba_giveup_policy allocates and clears it); everything else the kernel touches is the slot's own state in DeviceState
struct RetireArgs {
    fba_retired_rec* recs;      // [capacity]
    unsigned long long* seen;   // [1] retirements since fba_giveup_policy
    int32_t capacity;
};
void launch_retire(const Problem& P, const DeviceState& D, const RetireArgs& a, hipStream_t st);
// fba_belief_structures (fba_structures.hip): the parent-set word lists of slots [first, first + count) reduced into device buffers of the
// caller's; a null output = not wanted (head is always).  The caller zeroes query_mass where nq > STRUCT_QUERY_LDS
constexpr int STRUCT_TABLE      = FBA_STRUCT_TABLE;   // entries of a slot's table of distinct structures (open addressing, in LDS)
constexpr int STRUCT_HIST_CELLS = 1024;   // fp64 cells of the per-word histogram one pass over the slot keeps in LDS: whole words of n_sets cells
constexpr int STRUCT_QUERY_LDS  = 1024;   // query masses kept in LDS; queries beyond them add to the output directly
struct BeliefStructuresArgs {
    int32_t first, count;
    int32_t top_k, nq;
    int32_t n_words, n_sets;        // as fba_structure_lens gives them
    int32_t n_keys;                 // words that identify a structure in the record: 1 for history records (the bits of rec[1]), else n_words
    int32_t ncounts;                // counts of a particle's table: where the words stand (record_mask_word)
    uint64_t hash_keep;             // struct_hash's `keep`
    const uint32_t* query;          // [nq][n_keys] in key form; a first word of 0xffffffff: no record can hold this query
    fba_structure_head* head;       // [count]
    double* set_mass;               // [count][n_words][n_sets]
    uint32_t* top_words;            // [count][top_k][n_words]
    double* top_mass;               // [count][top_k]
    double* query_mass;             // [count][nq]
};
void launch_belief_structures(const Problem& P, const DeviceState& D, const BeliefStructuresArgs& a, hipStream_t st);
// fba_structure_stats (fba_structure_stats.hip): inside a tick, between the environment step and the belief update -- the main filters of
// the slots that took their step in this tick (DeviceState::adv != 0) reduced as fba_belief_structures reduces them, and those per-slot
// rows into the bins (episode, t) their steps belong to.  All state of the feature is here: buffers of the context's that
// fba_structure_stats_enable allocates.  A bin, and a row of the reduction, is a list of 8-byte words:
//   the fba_structure_stat head (STRUCT_STATS_BIN_HEAD words) | set_frac [n_words][n_sets] | query_frac [nq] | query_held [nq] | query_sole [nq]
// and the row a slot's workgroup leaves in `rows` the same behind a head of its own (STRUCT_STATS_SLOT_HEAD words: bin + 1 in the low half
// of the first -- 0: the slot took no step -- with the flags weightless (bit 32) and overflowed (bit 33); `distinct` in the second)
constexpr int STRUCT_STATS_BIN_HEAD    = 6;      // 8-byte words of fba_structure_stat
constexpr int STRUCT_STATS_SLOT_HEAD   = 2;
constexpr int STRUCT_STATS_BLOCK       = 256;    // stage one: threads of a slot's workgroup
constexpr int STRUCT_STATS_BINS_BLOCK  = 1024;   // stage two: threads of a workgroup
constexpr int STRUCT_STATS_GROUP_SLOTS = 256;    // stage two: slots one workgroup reduces
constexpr int STRUCT_STATS_LDS_WORDS   = 7680;   // stage two: 8-byte words of a workgroup's window of partial rows (60 KB) ...
constexpr int STRUCT_STATS_COLS        = 96;     // ... of which a bin takes this many at most: a longer row is reduced a window of words at a time
constexpr int STRUCT_STATS_CHUNK_SLOTS = 32768;  // slots of one pair of launches at most, as fba_belief_structures has it ...
constexpr size_t STRUCT_STATS_ROWS_BYTES = (size_t)64 << 20;   // ... and what their rows may take
struct StructStatsArgs {
    unsigned long long* bins;   // [n_bins][row_words]
    unsigned long long* rows;   // [chunk][STRUCT_STATS_SLOT_HEAD + row_words - STRUCT_STATS_BIN_HEAD]
    uint32_t* query;            // [nq][n_keys] in key form (BeliefStructuresArgs::query)
    int32_t n_bins;             // episodes * horizon
    int32_t nq, n_words, n_sets, n_keys, ncounts;   // as in BeliefStructuresArgs
    int32_t row_words;          // struct_stats_row_words
    int32_t chunk;              // struct_stats_chunk: slots per pair of launches
    int32_t cols, win_rows;     // stage two's LDS window: words of a row, bins (struct_stats_cols, struct_stats_win_rows)
    int32_t first, count;       // the slots of this pair of launches
    uint64_t hash_keep;         // struct_hash's `keep`
};
inline int struct_stats_row_words(int n_words, int n_sets, int nq) { return STRUCT_STATS_BIN_HEAD + n_words * n_sets + 3 * nq; }
inline int struct_stats_cols(int row_words) { return row_words < STRUCT_STATS_COLS ? row_words : STRUCT_STATS_COLS; }
inline int struct_stats_win_rows(int n_bins, int cols) { const int fit = STRUCT_STATS_LDS_WORDS / cols; return n_bins < fit ? n_bins : fit; }
inline int struct_stats_chunk(int slots, int row_words)
{
    const size_t fit = STRUCT_STATS_ROWS_BYTES / ((size_t)(STRUCT_STATS_SLOT_HEAD + row_words - STRUCT_STATS_BIN_HEAD) * 8);
    const int cap = fit < (size_t)STRUCT_STATS_CHUNK_SLOTS ? (int)fit : STRUCT_STATS_CHUNK_SLOTS;
    return slots < cap ? (slots > 0 ? slots : 1) : (cap > 0 ? cap : 1);
}
void launch_structure_stats(const Problem& P, const DeviceState& D, const StructStatsArgs& a, hipStream_t st);   // one chunk: [a.first, a.first + a.count)
// belief snapshots (fba_snapshot.hip): the blocks of `count` slots stand in `stage` at per_slot bytes each, laid out as include/fba_hip.h
// states it (fba_snapshot_head, weights, records); slot first + b owns block b.  All state of the feature is in these arguments
constexpr int SNAPSHOT_MAX_SLOTS = 32768;            // slots of one launch (a grid row each)
constexpr size_t SNAPSHOT_STAGE_BYTES = (size_t)256 << 20;   // staging memory of one export / import chunk (one block at least)
enum { SNAP_BAD_WEIGHT = 1, SNAP_BAD_STATE = 2, SNAP_BAD_STRUCTURE = 3, SNAP_BAD_ENTRY = 4, SNAP_BAD_COUNT = 5, SNAP_BAD_INCREMENT = 6 };
struct BeliefSnapshotArgs {
    int32_t first, count;
    uint8_t* stage;                 // [count][per_slot]
    int64_t per_slot;               // bytes of a block
    unsigned long long* check;      // [count] the payload checksums (the caller zeroes them)
    unsigned long long* bad;        // [1] validation: the smallest (block << 40 | particle << 8 | SNAP_BAD_*) met; the caller sets ~0
    int32_t weighted;               // the blocks hold weights
    int32_t ncounts;                // fp32 records: the words of a record that are counts
    int32_t nvar, mask_at;          // parent-set words of a record (0: none) and the word the first stands at
    int32_t ncells;                 // history records: cells of the dense table an entry may name
    const uint32_t* mask_limit;     // [nvar] parent-set word m is legal below this
};
void launch_snapshot_pack(const Problem& P, const DeviceState& D, const BeliefSnapshotArgs& a, hipStream_t st);      // export: gather + checksum
void launch_snapshot_validate(const Problem& P, const DeviceState& D, const BeliefSnapshotArgs& a, hipStream_t st);  // import, first pass
void launch_snapshot_commit(const Problem& P, const DeviceState& D, const BeliefSnapshotArgs& a, hipStream_t st);    // import, second pass
void launch_snapshot_replicate(const Problem& P, const DeviceState& D, int src, int first, int count, hipStream_t st);
// where block b of a snapshot store stands (DeviceState::restore_store): b * pitch + pad, so that the record part of every block starts at a
// multiple of 16 bytes -- the weights of an odd particle count would leave it at 8
__host__ __device__ inline int64_t snapshot_store_pad(int weighted, int64_t particles) { return weighted && (particles & 1) ? 8 : 0; }
inline int64_t snapshot_store_pitch(int64_t per_slot, int weighted, int64_t particles) { return (per_slot + snapshot_store_pad(weighted, particles) + 15) & ~(int64_t)15; }
// fba_restore.hip: the experiment loop's Belief::initiate of a resumed span, launched in launch_init's place while DeviceState::restore_store is set
void launch_restore(const Problem& P, const DeviceState& D, hipStream_t st);
// ... and the one thing a resumed span asks of a packed block beyond what an import judges: none of the 16-bit increments in the first
// inc_words words of a record exceeds head.updates.  Over the `count` blocks validated last (a.stage, a.per_slot, a.bad as for
// launch_snapshot_validate: the smallest block << 40 | particle << 8 | SNAP_BAD_INCREMENT met)
void launch_span_increments(const Problem& P, const BeliefSnapshotArgs& a, int inc_words, hipStream_t st);
// fba_belief_convert (fba_convert.hip): `count` staged source blocks (n_src particles, records of src_cs words) refitted into `count` staged
// destination blocks of the Problem the launch is given; both sides stand as a span's store does, block b at b * pitch behind the pad, so
// that record parts start at multiples of 16 bytes.  The headers of the destination are the host's.  All state of the feature is here
enum { CONVERT_SAME = 0, CONVERT_FLAT = 1, CONVERT_WEIGHTED = 2 };   // the source of output particle j: j, uniform_int(n_src), the pick on incl
constexpr int SNAP_BAD_TOTAL = 7;   // (beside SNAP_BAD_*: a weight total that is zero or not finite; particle 0)
struct BeliefConvertArgs {
    int32_t count;
    uint32_t first_run;             // block b draws from the streams of run first_run + b
    const uint8_t* src;             // [count] blocks at src_pitch, validated headers
    uint8_t* dst;                   // [count] blocks at dst_pitch
    int64_t src_pitch, dst_pitch;
    int32_t n_src, src_cs;          // particles of a source block, words a source record has room for
    int32_t weighted, mode;         // the blocks hold weights; CONVERT_*
    uint32_t seed_lo, seed_hi;
    double* incl;                   // CONVERT_WEIGHTED: [count][n_src] inclusive prefix sums of the source weights (launch_convert_scan writes them)
    unsigned long long* check;      // [count] the destination payloads' checksums (the caller zeroes them)
    unsigned long long* bad;        // [1] as BeliefSnapshotArgs::bad: block << 40 | SNAP_BAD_TOTAL
};
void launch_convert_scan(const BeliefConvertArgs& a, hipStream_t st);
void launch_snapshot_convert(const Problem& P, const BeliefConvertArgs& a, hipStream_t st);
void launch_uniform_scan(int n, double* w_tmp, double* out, double* total, double* ctot, hipStream_t st);

}  // namespace fba
