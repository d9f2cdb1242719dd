// fba_launch_plan.h -- THE place where a tick launch's kernel is chosen.
//
// search_plan, update_plan and reset_plan say, from Problem and DeviceState alone, which instantiation launch_search, launch_belief_update
// and launch_reset launch, with what block, grid (per slot count of the launch), dynamic LDS and LDS limit, and in what order.  The
// launchers (fba_search.hip, fba_kernels.hip) ask and launch; fba_create and fba_get_kernel_times (fba_engine.hip) ask the same functions
// where they need to know which kernel will run.  A new variant is added here and at one launch site.  Pure host code: no HIP call, no
// environment read.  tests/test_launch_plan_cpu.py pins every decision to a recording.
#pragma once

#include <cstdlib>

#include "fba_kernels.h"

namespace fba {

// ---- what the kernels and the decisions both compute: LDS sizes, and the predicates behind the tiger instantiations
__host__ __device__ __forceinline__ bool root_children_in_lds(const Problem& P, const DeviceState& D)
{
    return P.A * P.O <= ROOT_CHILDREN && D.max_nodes <= 32767;
}
constexpr int ET_NODE_WORDS = 9;   // an LDS node of the ETIGER tree layout (fba_search.hip): n0 | n1 << 16, n2, child0 | child1 << 16, q0, q1, q2 (two words each)
// 32-bit words of the dynamic LDS allocation of one search workgroup in front of the staged model description
__host__ __device__ __forceinline__ size_t search_lds_words(const Problem& P, const DeviceState& D, bool stage, bool etiger)
{
    const int depth_cap = P.max_depth > 0 ? P.max_depth : 1;
    if (etiger)
        return (size_t)((depth_cap + 1) / 2) * SEARCH_BLOCK + (stage ? (size_t)P.Cs * SEARCH_BLOCK : 0) + (size_t)2 * ET_NODE_WORDS * SEARCH_BLOCK;
    return (size_t)depth_cap * SEARCH_BLOCK * 2 + (stage ? (size_t)P.Cs * SEARCH_BLOCK : 0) +
           (root_children_in_lds(P, D) ? (size_t)P.A * P.O * SEARCH_BLOCK / 2 : 0);
}
constexpr int HIST_TREES = SEARCH_BLOCK / HIST_QUAD;   // trees of one wave of the history-record searches
constexpr int H2_WAVES = 4;                            // waves per workgroup of the bucket-tree searches, at most
__host__ __device__ __forceinline__ size_t h2_shared_bytes(const Problem& P, bool lrows)
{
    const int K = hist_row_width(P.hist_row);
    return lrows ? (size_t)P.hist_rid_bytes + (size_t)P.hist_distinct * K * sizeof(float) : (size_t)4 * HistLayout(P.gw_N, P.gw_G, 4).ostride * sizeof(float);
}
__host__ __device__ __forceinline__ size_t h2_wave_bytes(const Problem& P)
{
    const int depth_cap = P.max_depth > 0 ? P.max_depth : 1;
    return (size_t)depth_cap * HIST_TREES * (sizeof(double) + sizeof(int32_t) + sizeof(float) + sizeof(int32_t)) +
           (size_t)(P.Cs > 2 * depth_cap ? P.Cs : 2 * depth_cap) * HIST_TREES * sizeof(float) + (size_t)14 * HIST_TREES * sizeof(float);   // (+ the root's statistics, the record geometry)
}
__host__ __device__ __forceinline__ bool hist_all_draws_first(int N) { return N <= 16384; }   // importance_kernel on history records: the drawn sources fit LDS

// the tabular BA-POMDP over (episodic or continuous) tiger on the expected Dirichlet: what the TIGER_TABLE instantiations are written for
inline bool tiger_table_model(const Problem& P) { return P.model == FBA_MODEL_BA_TABLE && dom_is_tiger(P.domain) && !P.dirichlet_regular; }
// the factored BA-POMDP over factored tiger on the expected Dirichlet: its state features (S = 2^FS), else 0
inline int ftiger_features(const Problem& P)
{
    return P.model == FBA_MODEL_BA_FACTORED && dom_is_ftiger(P.domain) && !P.dirichlet_regular && P.S > 0 ? 31 - __builtin_clz((unsigned)P.S) : 0;
}
// the ETIGER tree layout (fba_search.hip) can hold this context's trees
inline bool etiger_ok(const Problem& P, const DeviceState& D)
{
    return dom_is_episodic(P.domain) && P.A == 3 && P.O == 2 && P.sims <= 65535 && D.max_nodes <= 4093 && !D.hash && P.planner != FBA_PLANNER_RANDOM;
}
// history records: the belief updates read the prior's deduplicated rows from LDS (rows wider than 12 floats stay in L2; FBA_HIST_ROWS=hbm: all do)
inline bool update_rows_in_lds(const Problem& P, const DeviceState& D) { return P.hist_lds && P.hist_row <= 10 && !D.ab_rows_hbm; }
// history particles: several workgroups per slot from this many particles up (FBA_HIST_MULTI=1 / 0 forces / forbids it: tests, A/B runs)
inline bool hist_update_multi(const Problem& P, const DeviceState& D)
{
    if (D.ab_hist_multi) return D.ab_hist_multi == 2;
    return P.N >= 4096;
}

// ---- a kernel instantiation as a value: the kernel and its template arguments.  The launchers switch over these, so every instantiation
// is spelled once where it is launched and once, as its key, where it is chosen
enum KernelName : uint32_t {
    K_SEARCH = 1, K_SEARCH_CA_HIST, K_SEARCH_HIST, K_SEARCH_HIST2, K_HIST2_FLAT_SEARCH, K_SEARCH_TABHIST,
    K_NESTED_UPDATE, K_REINVIGORATE, K_COPY_FLAGS, K_IMPORTANCE, K_REJECT_TAB_HIST, K_REJECT_HIST, K_REJECT, K_REJECT_TIGER_ONCE_GATHER,
    K_REJECT_TIGER_ONCE, K_REJECT_TIGER_LDS, K_CHEAT, K_MH, K_IS_MULTI_TAB_STEP, K_IS_MULTI_CA_STEP, K_IS_MULTI_STEP, K_SCAN_CARRY,
    K_IS_MULTI_NORM, K_IS_MULTI_SCAN, K_IS_MULTI_RESAMPLE, K_IS_MULTI_FINISH,
    K_RESET_HIST_FLAT, K_POST_RESET, K_LAZY_RESET, K_NESTED_FILL, K_RESET,
};
constexpr uint32_t kernel_key(KernelName k, int a = 0, int b = 0, int c = 0, int d = 0) { return k << 24 | a << 18 | b << 12 | c << 6 | d; }
constexpr KernelName kernel_name(uint32_t key) { return (KernelName)(key >> 24); }
// search_kernel<STAGE, AMAX, REG, TIGER_TABLE, MODEL, FTIGER, TIGER_POMDP, FTP, ETIGER>
constexpr uint32_t search_key(bool stage, int amax, bool reg, int tiger_table, int model, int ftiger = 0, bool tiger_pomdp = false, bool ftp = false, bool etiger = false)
{
    return kernel_key(K_SEARCH, stage | reg << 1 | tiger_pomdp << 2 | ftp << 3 | etiger << 4, amax, tiger_table | model << 2, ftiger);
}
constexpr uint32_t SEARCH_READS_COMPACT = search_key(true, 4, false, 2, FBA_MODEL_BA_TABLE, 0, false, false, true);   // the one search that reads compact filters (fba_state.h)
// reject_kernel<REG, TIGER_TABLE, FTIGER, BLK, FTP>
constexpr uint32_t reject_key(bool reg, int tiger_table, int ftiger = 0, int blk = REJECT_BLOCK, bool ftp = false)
{
    return kernel_key(K_REJECT, reg | ftp << 1, tiger_table, ftiger, blk / 64);
}
// importance_kernel<REG, TIGER_TABLE, HIST, WLDS>
constexpr uint32_t importance_key(bool reg, int tiger_table, bool hist, bool wlds) { return kernel_key(K_IMPORTANCE, reg, tiger_table, hist, wlds); }
// what fba_create's checks and the byte formulas of fba_get_kernel_times ask of a chosen kernel
constexpr bool tiger_filter_in_lds(uint32_t key)   // the packed tiger rejection updates whose attempts run from LDS
{
    return kernel_name(key) == K_REJECT_TIGER_LDS || kernel_name(key) == K_REJECT_TIGER_ONCE || kernel_name(key) == K_REJECT_TIGER_ONCE_GATHER;
}
constexpr bool reads_packed_tiger(uint32_t key)
{
    return key == search_key(true, 4, false, 2, FBA_MODEL_BA_TABLE) || key == SEARCH_READS_COMPACT || key == reject_key(false, 2, 0, 512) ||
           tiger_filter_in_lds(key) || key == importance_key(false, 2, false, false) || key == importance_key(false, 2, false, true);
}
constexpr bool reads_packed_ftiger(uint32_t key, int fs = 4)   // (FS = 2..4)
{
    return key == reject_key(false, 0, fs, REJECT_BLOCK, true) || key == search_key(true, 4, false, 0, FBA_MODEL_BA_FACTORED, fs, false, true, false) ||
           key == search_key(true, 4, false, 0, FBA_MODEL_BA_FACTORED, fs, false, true, true) || (fs > 2 && reads_packed_ftiger(key, fs - 1));
}
constexpr bool updates_history_records(uint32_t key)
{
    return kernel_name(key) == K_REJECT_HIST || kernel_name(key) == K_REJECT_TAB_HIST || kernel_name(key) == K_IS_MULTI_TAB_STEP ||
           kernel_name(key) == K_IS_MULTI_CA_STEP || key == importance_key(false, 0, true, false) || key == importance_key(false, 0, true, true) ||
           (kernel_name(key) == K_IS_MULTI_STEP && (key >> 12 & 63));   // (is_multi_step_kernel<REG, HIST, K>)
}

// ---- launch_search
// The share of a wave's live trees, in 64ths, that has to wait at a simulation boundary before search_kernel runs the boundary phase for
// them (back-up, then the next root sample) -- 64: when all of them wait, so the wave's trees run simulation i together (what every
// instantiation executed before the schedule was explicit); 1: as soon as one waits.  A value below 64 stands here only where a same-box
// A/B run against 64 found it faster (profiles/r21_search_quorum.txt): 60 -- the wave goes on when at most four of 64 trees are still in
// their simulation -- for the two instantiations the benchmarks run, 2 to 8 % of their ticks; 56 and 62 gain less, 48 and below lose.
constexpr int SEARCH_QUORUM_LOCKSTEP = 64;
constexpr uint32_t SEARCH_C3 = search_key(true, 4, false, 0, FBA_MODEL_BA_FACTORED, 3, false, true, true);   // packed factored tiger of size 3 on the ETIGER layout
constexpr int search_quorum_default(uint32_t kernel)
{
    return kernel == SEARCH_READS_COMPACT /* packed tabular tiger: C1, C2 */ || kernel == SEARCH_C3 ? 60 : SEARCH_QUORUM_LOCKSTEP;
}
// FBA_SEARCH_QUORUM as fba_create reads it: 1..64, or 0 (search_plan's default) when unset, not a number or out of range
inline int search_quorum_switch(const char* text)
{
    const int v = text ? std::atoi(text) : 0;
    return v >= 1 && v <= SEARCH_QUORUM_LOCKSTEP ? v : 0;
}
struct SearchPlan {
    uint32_t kernel;
    int block, slots_per_block;
    size_t lds;            // dynamic LDS bytes (search_kernel: the launcher adds FBA_SEARCH_LDS_PAD)
    int raise_lds;         // > 0: the kernel's limit of dynamic LDS has to be raised to this first
    bool order_first;      // search_order_kernel goes first (DeviceState::search_order)
    int quorum;            // search_kernel: DeviceState::search_quorum of the launch (search_quorum_default, or the context's override)
    int grid(int slots) const { return (slots + slots_per_block - 1) / slots_per_block; }
};
inline SearchPlan search_plan(const Problem& P, const DeviceState& D)
{
    SearchPlan pl{0, SEARCH_BLOCK, SEARCH_BLOCK, 0, 0, false, SEARCH_QUORUM_LOCKSTEP};
    const int depth_cap = P.max_depth > 0 ? P.max_depth : 1;
    if (P.hist == 3) {  // history particles of the collision-avoidance FBA-POMDP: one lane per tree, node records (A = 3)
        pl.kernel = kernel_key(K_SEARCH_CA_HIST, 4);
        pl.lds    = ca_hist_search_lds(P);   // (at most 64 KB: fba_create keeps other contexts dense)
        return pl;
    }
    if (P.hist) {  // history particles (gridworld): four lanes per tree
        const int K = hist_row_width(P.hist_row);
        pl.slots_per_block = HIST_TREES;
        if (!D.bkt) {   // node records
            pl.kernel = kernel_key(K_SEARCH_HIST, K);
            pl.lds = (size_t)depth_cap * HIST_TREES * (sizeof(double) + sizeof(int32_t) + sizeof(float) + sizeof(int32_t)) + (size_t)P.Cs * HIST_TREES * sizeof(float);
            return pl;
        }
        // the tree as one table of buckets.  Tabular records (fba_create gives them the bucket tree only) share no tables; the others
        // every Dirichlet row (LROWS; FBA_HIST_ROWS=hbm: the transition rows from the padded tables)
        const bool tab = P.hist == 2, flat = P.belief == FBA_BELIEF_REJECTION;   // (a flat filter's root sample)
        const bool lrows = !tab && P.hist_lds != nullptr && !D.ab_rows_hbm;
        const size_t shared = tab ? 0 : h2_shared_bytes(P, lrows);
        int nw = H2_WAVES;   // waves per workgroup: as many as 64 KB of LDS hold beside the shared tables (deep horizons have long paths)
        while (nw > 1 && shared + (size_t)nw * h2_wave_bytes(P) > 64 * 1024) nw >>= 1;
        pl.lds = shared + (size_t)nw * h2_wave_bytes(P);
        pl.block = 64 * nw;
        pl.slots_per_block = HIST_TREES * nw;
        pl.raise_lds = pl.lds > 64 * 1024 ? (int)pl.lds : 0;   // (one wave of a very deep horizon: past the default limit of a workgroup's dynamic LDS)
        pl.order_first = D.ab_lockstep != 0;
        pl.kernel = tab ? kernel_key(K_SEARCH_TABHIST, flat) : kernel_key(flat ? K_HIST2_FLAT_SEARCH : K_SEARCH_HIST2, K, lrows);
        return pl;
    }
    const bool stage = P.model != FBA_MODEL_POMDP && P.Cs <= SEARCH_STAGE_WORDS;
    // the tiger instantiations: their model's predicate, and po-uct on a tree of node records without a hash table
    const bool plain_tree  = P.planner == FBA_PLANNER_POUCT && !D.hash;
    const bool tiger_table = tiger_table_model(P) && stage && plain_tree;
    const bool tiger_pomdp = P.model == FBA_MODEL_POMDP && dom_is_tiger(P.domain) && plain_tree;
    const int fs           = ftiger_features(P);
    const bool ftiger      = fs >= 2 && fs <= 4 && plain_tree;
    // the episodic tiger family on its own tree layout (ETIGER); FBA_NO_ETIGER=1 keeps the general layout, for A/B runs
    // (the instantiations that exist on that layout: the tabular tiger BA-POMDP, planning on tiger itself, packed factored tiger)
    const bool et = !D.ab_no_etiger && etiger_ok(P, D) && (tiger_table || tiger_pomdp || (ftiger && P.ft_packed));
    pl.lds = search_lds_words(P, D, stage, et) * sizeof(uint32_t);
    if (P.model == FBA_MODEL_BA_FACTORED && !ftiger)
        pl.lds = ((pl.lds + 15) & ~(size_t)15) + (((size_t)P.fd_bytes + 15) & ~(size_t)15);  // + the model description (not the factored-tiger instantiations: 0.9 KB
                                                                                              //   that kept C3 at nine waves per CU where ten fit)
    if (tiger_table) pl.kernel = search_key(true, 4, false, P.packed ? 2 : 1, FBA_MODEL_BA_TABLE, 0, false, false, et);
    else if (tiger_pomdp) pl.kernel = search_key(false, 4, false, 0, FBA_MODEL_POMDP, 0, true, false, et);
    else if (ftiger) pl.kernel = search_key(stage || P.ft_packed, 4, false, 0, FBA_MODEL_BA_FACTORED, fs, false, P.ft_packed != 0, et);
    else {
        const int amax  = P.A <= 4 ? 4 : (P.A <= 8 ? 8 : (P.A <= 16 ? 16 : 24));   // (24: agr, 23 actions, is a POMDP-only domain)
        const int model = amax < 24 && (P.model == FBA_MODEL_BA_FACTORED || P.model == FBA_MODEL_BA_TABLE) ? P.model : FBA_MODEL_POMDP;
        pl.kernel = search_key(stage && model != FBA_MODEL_POMDP, amax, P.dirichlet_regular && model != FBA_MODEL_POMDP, 0, model);
    }
    pl.quorum = D.search_quorum >= 1 && D.search_quorum <= SEARCH_QUORUM_LOCKSTEP ? D.search_quorum : search_quorum_default(pl.kernel);
    return pl;
}

// ---- launch_belief_update and launch_reset: the launches that make one up, in order
struct LaunchStep {
    uint32_t kernel;
    int block;
    int rows;          // 0: a workgroup per `per_group` slots; else a grid of rows x slots
    int per_group;
    size_t lds;
    int raise_lds;     // > 0: raise the kernel's limit of dynamic LDS to this (once per device) in front of the launch
    int arg;           // the kernel's last argument where it has one: which filter, which pass
    bool chunked;      // DeviceState::single_rec: per chunk of as many slots as the scratch pool holds (for_each_chunk), with the chunked steps next to it
    bool shadow;       // on the incubator's shadow filter
    dim3 grid(int slots) const { return rows ? dim3(rows, slots) : dim3((slots + per_group - 1) / per_group); }
};
struct LaunchPlan {
    LaunchStep step[12];
    int n = 0;
    uint32_t filter = 0;   // the kernel that updates the main filter (what fba_get_kernel_times counts the bytes of)
    LaunchStep& add(uint32_t kernel, int block = 256, int rows = 0, int per_group = 1, size_t lds = 0, int arg = 0)
    {
        step[n] = LaunchStep{kernel, block, rows, per_group, lds, 0, arg, false, false};
        return step[n++];
    }
};
// importance_kernel of one slot per workgroup
inline void plan_importance_single(LaunchPlan& pl, const Problem& P, bool chunked, bool shadow)
{
    const bool packed_tiger = tiger_table_model(P) && P.packed;
    // weights and prefix sums of a slot in LDS while its workgroup works on them (8 bytes per particle)
    const bool wlds = P.N <= IS_LDS_MAX_N && !P.dirichlet_regular;
    const size_t lds = (wlds ? (size_t)P.N * (sizeof(double) + (packed_tiger ? 4 : 0)) : 0) +   // (packed tiger: + pending updates and sources, 16 bits each)
                       ((P.hist && hist_all_draws_first(P.N)) ? (size_t)P.N * 2 : 0);            // (history particles: the drawn sources)
    const uint32_t k = P.hist ? importance_key(false, 0, true, wlds)
                              : (P.dirichlet_regular ? importance_key(true, 0, false, false)
                                                     : importance_key(false, tiger_table_model(P) ? (P.packed ? 2 : 1) : 0, false, wlds));
    LaunchStep& s = pl.add(k, IS_BLOCK, 0, 1, lds);
    s.raise_lds = lds > 16384 ? IS_LDS_MAX_N * 12 : 0;
    s.chunked = chunked; s.shadow = shadow;
    if (!shadow) pl.filter = k;
}
// the importance update as seven launches, so that a slot's particles spread over many workgroups
inline void plan_importance_multi(LaunchPlan& pl, const Problem& P, const DeviceState& D, bool chunked)
{
    const int first = pl.n, nchunks = (P.N + 255) / 256, rows = (nchunks + 3) / 4;
    if (P.hist == 2) pl.add(kernel_key(K_IS_MULTI_TAB_STEP), 256, rows);   // (tabular records: sparse prior rows from L2)
    else if (P.hist == 3)   // (collision-avoidance records: the whole prior and its sequence table in LDS)
        pl.add(kernel_key(K_IS_MULTI_CA_STEP), 256, rows, 1, ca_hist_table_bytes(P.hist_row, P.hist_rid_bytes, P.hist_distinct, P.hist_cap));
    else if (P.hist) {   // is_multi_step_kernel<REG, HIST, K>: the prior's rows from LDS where the deduplicated blob exists, K floats each
        const int K = update_rows_in_lds(P, D) ? hist_row_width(P.hist_row) : 0;
        pl.add(kernel_key(K_IS_MULTI_STEP, false, true, K), 256, rows, 1, K ? (size_t)P.hist_rid_bytes + (size_t)P.hist_distinct * K * sizeof(float) : 0);
    }
    else pl.add(kernel_key(K_IS_MULTI_STEP, P.dirichlet_regular != 0, false, 0), 256, rows);
    pl.filter = pl.step[first].kernel;
    pl.add(kernel_key(K_SCAN_CARRY), 256, 0, 1, 0, 0);
    pl.add(kernel_key(K_IS_MULTI_NORM), 256, rows);
    pl.add(kernel_key(K_SCAN_CARRY), 256, 0, 1, 0, 1);
    pl.add(kernel_key(K_IS_MULTI_SCAN), 256, rows);
    pl.add(kernel_key(K_IS_MULTI_RESAMPLE), 256, (P.N + 255) / 256);
    pl.add(kernel_key(K_IS_MULTI_FINISH), 64, 0, 64);
    for (int i = first; i < pl.n; ++i) pl.step[i].chunked = chunked;
}
inline LaunchPlan update_plan(const Problem& P, const DeviceState& D)
{
    LaunchPlan pl;
    const bool chunked = D.single_rec != 0;
    if (P.nested) {
        pl.filter = pl.add(kernel_key(K_NESTED_UPDATE, P.dirichlet_regular != 0)).kernel;
        return pl;
    }
    if (P.belief == FBA_BELIEF_REJECTION) {
        if (P.reinvig) pl.add(kernel_key(K_REINVIGORATE));
        if (P.incub) {
            // StructureIncubatorSampling::updateEstimation (:105-131): breed the least likely shadow particles from the two
            // rejection filters as they are now, importance-sample the shadow filter (it has its own copy of the request
            // flags: its kernel clears them), then the two rejection updates below
            pl.add(kernel_key(K_COPY_FLAGS), 256, 0, 256);
            pl.add(kernel_key(K_REINVIGORATE), 256, 0, 1, 0, 1);
            plan_importance_single(pl, P, false, true);
        }
        if (P.hist == 2) {   // tabular history particles (fba_create: the plain filter, expected Dirichlet)
            LaunchStep& s = pl.add(kernel_key(K_REJECT_TAB_HIST), REJECT_BLOCK);
            s.chunked = chunked;
            pl.filter = s.kernel;
            return pl;
        }
        if (P.hist) {   // (fba_create: the plain filter, expected Dirichlet)
            const int K = update_rows_in_lds(P, D) ? hist_row_width(P.hist_row) : 0;
            LaunchStep& s = pl.add(kernel_key(K_REJECT_HIST, K), REJECT_BLOCK, 0, 1, K ? (size_t)P.hist_rid_bytes + (size_t)P.hist_distinct * K * sizeof(float) : 0);
            s.chunked = chunked;
            pl.filter = s.kernel;
            return pl;
        }
        const int fs = ftiger_features(P);
        const bool lds_n = P.N <= TIGER_LDS_MAX_N, once_n = lds_n && P.N >= TIGER_ONCE_MIN_N;
        for (int fc = (P.reinvig || P.incub) ? 1 : 0; fc >= 0; --fc) {  // the main filter's launch clears the request flag: last
            if (fs >= 2 && fs <= 4) pl.add(reject_key(false, 0, fs, REJECT_BLOCK, P.ft_packed != 0), REJECT_BLOCK, 0, 1, 0, fc);
            else if (P.dirichlet_regular) pl.add(reject_key(true, 0), REJECT_BLOCK, 0, 1, 0, fc);
            else if (tiger_table_model(P) && P.packed && once_n)
                pl.add(kernel_key(D.ab_tiger_gather ? K_REJECT_TIGER_ONCE_GATHER : K_REJECT_TIGER_ONCE), 512, 0, 1, (size_t)P.N * 17 + 16);
            else if (tiger_table_model(P) && P.packed && lds_n) pl.add(kernel_key(K_REJECT_TIGER_LDS), 512, 0, 1, (size_t)P.N * 13 + 16);
            else if (tiger_table_model(P) && P.packed) pl.add(reject_key(false, 2, 0, 512), 512, 0, 1, 0, fc);  // (chunks of 512 are 4 % faster than 256 / 1024 on packed records)
            else pl.add(reject_key(false, tiger_table_model(P) ? 1 : 0), REJECT_BLOCK, 0, 1, 0, fc);
        }
        pl.filter = pl.step[pl.n - 1].kernel;
        return pl;
    }
    if (P.cheat) pl.add(reject_key(P.dirichlet_regular != 0, 0), REJECT_BLOCK, 0, 1, 0, 1);  // rejectSample on the correct-graph filter first (CheatingReinvigoration.cpp:111)
    // tabular / collision-avoidance history particles: the update is always the multi-launch one, one slot or many, 65 536 particles or a million
    if (P.hist >= 2) plan_importance_multi(pl, P, D, chunked);
    else if (D.is_multi) plan_importance_multi(pl, P, D, false);
    else {
        if (chunked && P.hist && hist_update_multi(P, D)) plan_importance_multi(pl, P, D, true);
        else plan_importance_single(pl, P, chunked, false);
        if (P.cheat) pl.add(kernel_key(K_CHEAT));
        if (P.mh) {  // a wave per slot; the chain's scratch in LDS when it fits (the kernel is told)
            const int in_lds = mh_scratch_in_lds(D.mh_scratch_words);
            pl.add(kernel_key(K_MH), 64, 0, 1, MH_LDS_HEAD + (in_lds ? (size_t)D.mh_scratch_words * 4 : 0), in_lds);
        }
    }
    return pl;
}
inline LaunchPlan reset_plan(const Problem& P, const DeviceState& D)
{
    LaunchPlan pl;
    const int tiles = (P.N + PARTICLE_TILE - 1) / PARTICLE_TILE;
    const bool second = P.reinvig || P.cheat || P.incub;
    if (P.belief == FBA_BELIEF_REJECTION && !second) {  // the plain rejection filter resets lazily
        if (!P.hist) pl.add(kernel_key(K_LAZY_RESET), 256, 0, 256);
        else {   // ... except on history particles, which keep a second copy of the state (reset_hist_flat_kernel)
            pl.add(kernel_key(K_RESET_HIST_FLAT), 256, tiles);
            pl.add(kernel_key(K_POST_RESET), 256, 0, 256);
        }
        return pl;
    }
    if (P.nested) pl.add(kernel_key(K_NESTED_FILL), 256, 0, 1, 0, 1);
    else {
        pl.add(kernel_key(K_RESET), 256, tiles).chunked = D.single_rec != 0;
        if (second) pl.add(kernel_key(K_RESET), 256, tiles, 1, 0, 1);
        if (P.incub) pl.add(kernel_key(K_RESET), 256, tiles).shadow = true;  // StructureIncubatorSampling::resetDomainStateDistribution (:46-61): the shadow filter too, in place
    }
    pl.add(kernel_key(K_POST_RESET), 256, 0, 256);
    return pl;
}

}  // namespace fba
