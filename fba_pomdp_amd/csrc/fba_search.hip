// fba_search.hip -- the tree-search kernels of the BA-POMCP engine (gfx950 / CDNA4, wave64).
//
//   search_kernel        POUCT / RBAPOUCT tree search, one lane per tree          (P1-P8)
//   search_hist_kernel   the same search on history particles, four lanes per tree (BASELINE configs[3])
//
// The search is latency bound and gets its throughput from running one independent tree per lane (or quad), all
// lanes executing the common "simulate one step" body together.  No dense contraction, no MFMA.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fba_kernels_common.h"

namespace fba {

// ---------------------------------------------------------------------------------------------
// search_kernel: one lane = one slot = one tree; `sims` simulations, sequential semantics.
// POUCT::selectAction POUCT.cpp:63-129, RBAPOUCT::selectAction RBAPOUCT.cpp:67-153 (the root
// particle's counts are read and never written: StepType::KeepCounts).
// The recursion traverseActionNode / traverseChanceNode / rollout (POUCT.cpp:183-303) is unrolled
// into a state machine: a lane is in the tree, in a rollout, or AT A BOUNDARY -- its simulation has
// finished, the back-up is pending and the next simulation not yet started.  Every trip of the loop
// performs at most one simulator.step per lane, for the lanes that are in a simulation; which of
// its two phases a trip runs is decided for the whole wave, from two ballots:
//   boundary phase   back-up of the finished simulation, ++sim, root sample + particle fetch of the
//                    next -- run when waiting lanes x 64 >= quorum x live lanes (or nobody steps);
//   step phase       select, step, resolve the child -- for every lane in a simulation.
// In the episodic-tiger instantiations (ETIGER, below) the boundary phase also makes the new
// simulation's first step, which is the same work for every lane it serves: at the root, statistics
// in registers, the child one bit of l1_exists.  Its order for a waiting lane:
//   1. start stream(sim + 1), draw the root particle; from a compact filter, request its 16-byte
//      record (the back-up draws nothing, and the record is not needed before step 4);
//   2. the back-up, ++sim;
//   3. select at the root, from the registers as the back-up left them;
//   4. wait for the record (the wider formats are fetched here), stage it for the deeper steps;
//   5. the root's simulator.step -- a compact record's words straight from the load's registers;
//   6. path entry 0, then the child: terminal or no depth left -> back to the boundary; the node
//      after (listen, o) exists -> into the tree; else create it in LDS and start the rollout.
// So the step phase of these instantiations never sees the root: no gather from registers, no root
// case in the child lookup or the expansion, one trip fewer per simulation.
// DeviceState::search_quorum = 64 is the wave whose trees run simulation i together (a lane that has
// finished idles until the longest of the 64 ends); 1 pays the boundary phase on nearly every trip for
// the third of the lanes that need it.  The value is the launch plan's (fba_launch_plan.h), measured
// per instantiation.  When a lane runs its simulation i is invisible to it: the lanes are independent
// trees and every draw comes from the stream of (run, episode, t, phase, simulation).
// (Before the schedule was explicit the source read as "a boundary as soon as any lane waits"; the
// compiler had split its single loop into a loop per simulation around a loop per step, which is
// quorum 64.  The conditions are scalar now, so there is no divergent exit to nest.)
// LDS per lane: the path needed for the bottom-up back-up, [depth][lane], and -- when a particle
// record fits SEARCH_STAGE_WORDS (STAGE) -- the root particle's whole count blob, [word][lane], fetched with
// one burst of 16-byte loads per simulation so that no step waits on HBM for its Dirichlet rows.
// ---------------------------------------------------------------------------------------------
// FTIGER > 0: the simulator is the factored-tiger FBA-POMDP with FTIGER binary state features (expected
// Dirichlet mode); its step is ftiger_step<FTIGER>, the layout restated as literals.
// TIGER_POMDP: planning on the tiger POMDP itself (BASELINE configs[0]); the sizes and the domain are literals.
// FTP: the factored-tiger records are packed (PackedFtigerView).
//
// ETIGER: the episodic tiger family (tiger and factored tiger, POMDP or Bayes-adaptive simulator): A = 3, O = 2, and only
// `listen` (action 2) continues -- opening a door ends the episode in the domain and in the BA extensions alike
// (Tiger.cpp:75-79, TigerBAExtension.cpp:32-36, FactoredTigerBAExtension.cpp) -- so a node has at most two children and the
// tree is a binary tree over the observations heard.  What a simulation costs this kernel is the 64-byte sectors it has
// the memory system fetch (one more random sector per simulation is +45 ms on the bench), and the two
// nodes below the root are on nearly every path; they live in LDS beside the path (18 words per lane: counts as uint16,
// child indices as uint16, Q as fp64), never in HBM.  The path itself shrinks to 16 bits per level -- node index (12 bits:
// the host bounds the tree at 2^(depth+1) + 1 nodes), action (2), and the reward as a code (-1 / 10 / -100: the only
// rewards of these domains) -- which is what pays for the room.  Same draws, same arithmetic, same results.
// (ET_NODE_WORDS, etiger_ok and the LDS sizes of this file's kernels: fba_launch_plan.h)
__device__ __forceinline__ int et_reward_code(double r) { return r == -1.0 ? 0 : (r == 10.0 ? 1 : 2); }
__device__ __forceinline__ double et_reward(int code) { return code == 0 ? -1.0 : (code == 1 ? 10.0 : -100.0); }
#ifdef FBA_PROFILE_SEARCH
// profiling build only (scripts/search_regions.py): shader-clock cycles a wave spends in each region of the search loop [0..4, 6], and --
// search_kernel -- what its waves executed: loop trips [5], lanes that stepped summed over the trips [8], boundary phases run [9] and the
// lanes that were waiting for them [10]; the root block of the episodic-tiger boundary phase (selection, step, child) has its cycles in [7]
// and the steps its lanes made in [11] (they are no part of [8])
__device__ unsigned long long g_search_prof[12];
#define PROF_MARK(r) { const long long now_ = clock64(); prof_[r] += now_ - prev_; prev_ = now_; }
#else
#define PROF_MARK(r)
#endif
template <bool STAGE, int AMAX, bool REG, int TIGER_TABLE, int MODEL, int FTIGER = 0, bool TIGER_POMDP = false, bool FTP = false, bool ETIGER = false>
__global__ void __launch_bounds__(SEARCH_BLOCK) search_kernel(Problem P, DeviceState D)
{
    if (TIGER_POMDP) {
        P.S = 2; P.A = 3; P.O = 2; P.C = 0; P.Cs = 4; P.planner = FBA_PLANNER_POUCT;
        if (P.domain != FBA_DOM_TIGER_CONTINUOUS) P.domain = FBA_DOM_TIGER_EPISODIC;
        P.belief = P.belief == FBA_BELIEF_IMPORTANCE ? FBA_BELIEF_IMPORTANCE : FBA_BELIEF_REJECTION;
        D.cn_off = 1; D.cq_off = 4; D.child_off = 10; D.node_words = 16; D.hash = nullptr;  // node layout of A = 3, O = 2 (fba_engine.hip)
    }
    // one instantiation per simulator: the launcher passes the model it read from P, so restating it
    // here drops the other simulators' code (a plain-POMDP search carries every domain's step(),
    // the Bayes-adaptive ones none of them) from this instantiation
    P.model = MODEL;
    if (FTIGER > 0) {  // sizes of factored tiger with FTIGER - 1 irrelevant features
        P.S = 1 << FTIGER; P.A = 3; P.O = 2;
        if (P.domain != FBA_DOM_FTIGER_CONTINUOUS) P.domain = FBA_DOM_FTIGER_EPISODIC;
        if (ETIGER) P.domain = FBA_DOM_FTIGER_EPISODIC;
    }
    if (ETIGER) { P.A = 3; P.O = 2; }
    // TIGER_TABLE: the launcher has checked that this is the tabular BA-POMDP over (episodic or
    // continuous) tiger; restating its sizes as literals lets the compiler unroll the two-entry
    // Dirichlet rows and fold every model / domain branch.  Same code, same results.
    if (TIGER_TABLE) {
        P.model = FBA_MODEL_BA_TABLE; P.planner = FBA_PLANNER_POUCT;
        P.S = 2; P.A = 3; P.O = 2; P.phi_len = 12; P.C = 24; P.Cs = 32;
        if (P.domain != FBA_DOM_TIGER_CONTINUOUS) P.domain = FBA_DOM_TIGER_EPISODIC;
        P.belief = P.belief == FBA_BELIEF_IMPORTANCE ? FBA_BELIEF_IMPORTANCE : FBA_BELIEF_REJECTION;
        D.cn_off = 1; D.cq_off = 4; D.child_off = 10; D.node_words = 16; D.hash = nullptr;  // node layout of A = 3, O = 2 (fba_engine.hip)
        if (TIGER_TABLE == 2) { P.C = 12; P.Cs = 16; }  // packed particles (PackedView): 24 uint16 + state in 64 bytes
    }
    if (ETIGER && (TIGER_TABLE || TIGER_POMDP)) P.domain = FBA_DOM_TIGER_EPISODIC;
    extern __shared__ double lds[];
    __shared__ __attribute__((aligned(8))) float s_prior[TIGER_TABLE == 2 ? 24 : 2];
    const int lane = threadIdx.x;
    const int e    = blockIdx.x * SEARCH_BLOCK + lane;
    if (TIGER_TABLE == 2) {
        if (lane < 24) s_prior[lane] = D.prior_dense[lane];
        __syncthreads();
    }
    if (MODEL == FBA_MODEL_BA_FACTORED && FTIGER == 0) {  // (the factored-tiger instantiations carry their layout as constants)
        // the factored model's description (which parents, how many values, where the rows start) is
        // consulted several times per sampled feature: keep the part in use in LDS, at the end of
        // this workgroup's allocation, instead of chasing it through global memory
        size_t words = search_lds_words(P, D, STAGE, ETIGER);
        words = (words + 3) & ~(size_t)3;  // 16-byte aligned
        uint4* dst       = reinterpret_cast<uint4*>(reinterpret_cast<uint32_t*>(lds) + words);
        const uint4* src = reinterpret_cast<const uint4*>(P.fd);
        for (int k = lane; k < (P.fd_bytes + 15) / 16; k += SEARCH_BLOCK) dst[k] = src[k];
        __syncthreads();
        P.fd = reinterpret_cast<const FDesc*>(dst);
    }
    if (e >= P.E || !D.active[e]) return;

    const int depth_cap = P.max_depth > 0 ? P.max_depth : 1;
    // Rewards on the path are kept as fp32: every reward of every domain here (and of the BA extensions) is a
    // small integer or a multiple of 1/2, so the round trip through float is exact and the back-up still
    // computes in fp64 -- and 4 bytes x depth x 64 lanes of LDS per wave buy one more resident wave per CU.
    float* path_r       = reinterpret_cast<float*>(lds) + lane;                         // [depth][block]
    int32_t* path_na    = reinterpret_cast<int32_t*>(path_r - lane + (size_t)depth_cap * SEARCH_BLOCK) + lane;
    // ETIGER: the path is [depth][block] of uint16 {node (12 bits; at level 1: which of the two LDS nodes), action << 12, reward code << 14}
    uint16_t* path16    = reinterpret_cast<uint16_t*>(lds) + lane;
    float* stage        = ETIGER ? reinterpret_cast<float*>(lds) + (size_t)((depth_cap + 1) / 2) * SEARCH_BLOCK + lane
                                 : reinterpret_cast<float*>(path_na - lane + (size_t)depth_cap * SEARCH_BLOCK) + lane;  // [Cs][block]
    // children of the root, [a*O + o][block], when there are at most ROOT_CHILDREN of them
    // (node indices fit 16 bits up to 32 766 simulations; beyond that the root's children stay in its record)
    const bool root_lds = !ETIGER && root_children_in_lds(P, D);
    int16_t* rootch     = reinterpret_cast<int16_t*>(stage - lane + (STAGE ? (size_t)P.Cs * SEARCH_BLOCK : 0)) + lane;
    // ETIGER: the two nodes below the root, [2][ET_NODE_WORDS][block]
    uint32_t* l1        = reinterpret_cast<uint32_t*>(stage - lane + (STAGE ? (size_t)P.Cs * SEARCH_BLOCK : 0)) + lane;

    Rng g               = slot_rng(P, D, e);
    const int hist_len  = D.t[e];
    const int max_tree_depth = min(P.horizon - hist_len, P.max_depth);
    const int W         = D.node_words;
    int32_t* tree       = D.nodes + (size_t)e * D.max_nodes * W;
    const float* prec   = D.p_rec + pbase(P, e, D.bufsel[e]) * (size_t)P.Cs;

    // (the nested belief stores dense records only: never with the packed instantiations)
    const bool nested = TIGER_TABLE != 2 && !TIGER_POMDP && !FTP && MODEL != FBA_MODEL_POMDP && P.nested != 0;
    if (P.planner == FBA_PLANNER_RANDOM) {  // RandomPlanner::selectAction RandomPlanner.cpp:14-24
        g.stream(FBA_PHASE_SEARCH, (uint32_t)P.sims);
        int ns = 0;
        const int src = nested ? nested_sample(P, D, e, g, ns) : belief_sample_uniform(P, D, g);
        D.action[e]   = domain_random_action(P, g, nested ? ns : slot_lazy(D, e) ? lazy_state(P, D, e, src) : rec_state(prec + (size_t)src * P.Cs, P.C));
        return;
    }

    // addLegalActions(belief.sample(), ...): the probe draw lives in its own stream (unit = sims)
    // and its result is not needed -- legal actions do not depend on the state in these domains.
    node_init(D, tree, P.A, P.O);
    int n_nodes = 1, tree_depth = 0;
    unsigned long long steps = 0;
    // The root is on the path of every simulation: its visit counts and Q values live in registers
    // for the whole search and its child pointers sit in LDS.
    int r_vis = 0, r_cn[AMAX];
    double r_cq[AMAX];
#pragma unroll
    for (int a = 0; a < AMAX; ++a) { r_cn[a] = 0; r_cq[a] = 0.0; }
    if (root_lds)
        for (int k = 0; k < P.A * P.O; ++k) rootch[k * SEARCH_BLOCK] = -1;
    uint32_t l1_exists = 0;   // ETIGER: bit o = the root's child after (listen, o) has been created
    // ETIGER: header and chosen Q of the path's nodes at levels 2 and 3 as this simulation's descent loaded them -- nothing
    // else writes this tree, so the back-up need not fetch their sectors again (by then they have left the L2)
    int4 cy_h2 = make_int4(0, 0, 0, 0), cy_h3 = make_int4(0, 0, 0, 0);
    double cy_q2 = 0, cy_q3 = 0;
    int4* tab      = hash_table(D, e);
    const uint32_t epoch = D.hash ? hash_begin_search(D, e, tab, 0, 1) : 0;

    // bit 0: particle states are still the episode's start-state draws (lazy_state); bit 1 (packed episodic tiger only): the slot's
    // filter is compact (fba_state.h) -- a root sample is ONE 16-byte load, its four `listen` words staged where tiger_step_packed reads
    // them.  The other count words of such a record are zero by construction: staged once, here
    constexpr bool COMPACT = TIGER_TABLE == 2 && ETIGER;
    const int lazy_c = (slot_lazy(D, e) ? 1 : 0) | (COMPACT && D.compact[e] ? 2 : 0);
    if (COMPACT && (lazy_c & 2)) {
#pragma unroll
        for (int w = 0; w < 10; ++w)
            if (w != 2 && w != 5) stage[w * SEARCH_BLOCK] = 0.f;
    }
    // -P ts: TSPlanner / BATSPlanner (src/planners/ts/TSPlanner.cpp:16-29, bayes-adaptive/BATSPlanner.cpp:19-34) sample
    // the belief once and plan on that point estimate, whose sample() draws nothing: every simulation starts
    // from the same particle and its stream begins with the UCB tie-break.
    int ts_src = -1, ts_state = 0;
    if (P.planner == FBA_PLANNER_TS) {
        g.stream(FBA_PHASE_SEARCH, (uint32_t)P.sims + 2u);
        ts_src = nested ? nested_sample(P, D, e, g, ts_state) : belief_sample_uniform(P, D, g);
    }
    // mode: 0 = at a boundary (simulation `sim` has finished: its back-up is pending -- `plen` path entries and the rollout's return in
    // `rret` -- and the next one is to start; sim = -1: nothing to back up yet), 1 = in the tree, 2 = rollout.  A lane whose sim has
    // reached P.sims is done and only waits for the wave.
    int sim = -1, mode = 0;
    int s = 0, node = 0, dtg = 0, plen = 0, rdepth = 0;
    const float* cnt = prec;
    double rret = 0, rdisc = 1;
    const int quorum = D.search_quorum;   // (a kernel argument: scalar)
#ifdef FBA_PROFILE_SEARCH
    long long prof_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, prev_ = clock64();
#endif
    while (true) {
        PROF_MARK(6)
        // which phases this trip runs is decided for the wave, from two ballots: every branch on it is scalar
        const bool waiting = mode == 0 && sim < P.sims;
        const int n_wait = __popcll(__ballot(waiting)), n_act = __popcll(__ballot(mode != 0));
        if (n_wait + n_act == 0) break;
        const bool boundary = n_act == 0 || n_wait * 64 >= quorum * (n_wait + n_act);
#ifdef FBA_PROFILE_SEARCH
        const bool lead_ = lane == __ffsll((unsigned long long)__ballot(true)) - 1;   // the trip is charged once per wave
        if (lead_) { prof_[5] += 1; if (boundary) { prof_[9] += 1; prof_[10] += n_wait; } }
#endif
        int src = 0, nest_state = ts_state;
        uint4 cv = make_uint4(0, 0, 0, 0);   // COMPACT: the next root particle's record, on its way while the back-up runs
        if (ETIGER && boundary && waiting && sim + 1 < P.sims) {
            // the next simulation's stream and its root sample first: the back-up draws nothing, and a compact record (one 16-byte
            // load) is not needed before the back-up and the root's selection are done.  (The wider records keep their fetch behind
            // the back-up: a burst of 4 to 12 float4 must not live across it.)
            g.stream(FBA_PHASE_SEARCH, (uint32_t)(sim + 1));
            src = ts_src >= 0 ? ts_src : (nested ? nested_sample(P, D, e, g, nest_state) : belief_sample_uniform(P, D, g));
            if (COMPACT && (lazy_c & 2)) cv = reinterpret_cast<const uint4*>(prec)[src];
        }
        if (boundary && waiting) {
            // back-up, leaf to root: ret = r + gamma * delayed; ChanceNode::addVisit(ret)
            // (MCTSTreeNodes.cpp:8-12); ActionNode::addVisit() (:59-62)
            // (the root is entry 0 of every path and no other entry: the loop runs over the nodes below it, the root's
            // register copy is updated once behind it -- one code path per level instead of two)
            double del = rret;
            for (int k = plen - 1; k >= (ETIGER ? 4 : 1); --k) {
                const int na     = ETIGER ? (int)path16[(size_t)k * SEARCH_BLOCK] : path_na[(size_t)k * SEARCH_BLOCK];
                const double ret = (ETIGER ? et_reward(na >> 14) : (double)path_r[(size_t)k * SEARCH_BLOCK]) + P.gamma * del;
                const int act    = ETIGER ? ((na >> 12) & 3) : (na & 31);
                int32_t* rec = tree + (size_t)(ETIGER ? (na & 0xfff) : (na >> 5)) * W;
                double* q    = reinterpret_cast<double*>(rec + D.cq_off) + act;
                int n;
                if (P.A == 3) {  // {visits, n0, n1, n2} is one 16-byte word: one load, one store
                    int4* hp = reinterpret_cast<int4*>(rec);
                    int4 h   = *hp;
                    n = act == 0 ? ++h.y : (act == 1 ? ++h.z : ++h.w);
                    ++h.x;
                    *hp = h;
                } else {
                    n = ++rec[D.cn_off + act];
                    if (D.cn_off) ++rec[0];
                }
                *q += (ret - *q) / (double)n;
                del = ret;
            }
            if (ETIGER) {   // levels 3 and 2: header and Q from the descent, two stores each, no load
#pragma unroll
                for (int lv = 3; lv >= 2; --lv)
                    if (plen > lv) {
                        const int na     = (int)path16[(size_t)lv * SEARCH_BLOCK];
                        const double ret = et_reward(na >> 14) + P.gamma * del;
                        const int act    = (na >> 12) & 3;
                        int32_t* rec     = tree + (size_t)(na & 0xfff) * W;
                        int4 h           = lv == 3 ? cy_h3 : cy_h2;
                        const double q0  = lv == 3 ? cy_q3 : cy_q2;
                        const int n      = act == 0 ? ++h.y : (act == 1 ? ++h.z : ++h.w);
                        ++h.x;
                        *reinterpret_cast<int4*>(rec) = h;
                        reinterpret_cast<double*>(rec + D.cq_off)[act] = q0 + (ret - q0) / (double)n;
                        del = ret;
                    }
            }
            if (ETIGER && plen > 1) {   // the node below the root: in LDS
                const int na     = (int)path16[1 * SEARCH_BLOCK];
                const double ret = et_reward(na >> 14) + P.gamma * del;
                const int act    = (na >> 12) & 3;
                uint32_t* nd     = l1 + (size_t)(na & 0xfff) * ET_NODE_WORDS * SEARCH_BLOCK;
                uint32_t* cw     = nd + (act >> 1) * SEARCH_BLOCK;   // n0 | n1 << 16, n2
                const uint32_t w = *cw;
                const int n      = (int)((act & 1) ? (w >> 16) : (w & 0xffffu)) + 1;
                *cw              = (act & 1) ? ((w & 0xffffu) | ((uint32_t)n << 16)) : ((w & 0xffff0000u) | (uint32_t)n);
                uint32_t* qw     = nd + (size_t)(3 + 2 * act) * SEARCH_BLOCK;
                double q         = __hiloint2double((int)qw[SEARCH_BLOCK], (int)qw[0]);
                q += (ret - q) / (double)n;
                qw[0]            = (uint32_t)__double2loint(q);
                qw[SEARCH_BLOCK] = (uint32_t)__double2hiint(q);
                del = ret;
            }
            if (plen > 0) {
                const double ret = (ETIGER ? et_reward((int)path16[0] >> 14) : (double)path_r[0]) + P.gamma * del;
                const int act    = ETIGER ? (((int)path16[0] >> 12) & 3) : (path_na[0] & 31);
                // register-array element `act`: select, ONE division, write back
                int n = 0;
                double q = 0.0;
#pragma unroll
                for (int a2 = 0; a2 < AMAX; ++a2)
                    if (a2 == act) { n = r_cn[a2]; q = r_cq[a2]; }
                ++n;
                q += (ret - q) / (double)n;
#pragma unroll
                for (int a2 = 0; a2 < AMAX; ++a2)
                    if (a2 == act) { r_cn[a2] = n; r_cq[a2] = q; }
                ++r_vis;
            }
            ++sim;
            plen = 0;
        }
        PROF_MARK(4)
        const bool start = boundary && waiting && sim < P.sims;   // (ETIGER: the lanes that drew `src` above)
        int a = 0;
        if (ETIGER && start && max_tree_depth != 0)   // the root's selection, from the registers as the back-up left them
            a = ucb_pick<AMAX>(P, g, D.log1p_tab, r_vis, r_cn, r_cq, true);
        PROF_MARK(7)
        if (start) {
            if (!ETIGER) {
                g.stream(FBA_PHASE_SEARCH, (uint32_t)sim);
                src = ts_src >= 0 ? ts_src : (nested ? nested_sample(P, D, e, g, nest_state) : belief_sample_uniform(P, D, g));
            }
            cnt = prec + (size_t)src * P.Cs;
            if (COMPACT && (lazy_c & 2)) {
                const uint4 v = cv;
                stage[2 * SEARCH_BLOCK]  = __uint_as_float(v.x);
                stage[5 * SEARCH_BLOCK]  = __uint_as_float(v.y);
                stage[10 * SEARCH_BLOCK] = __uint_as_float(v.z);
                stage[11 * SEARCH_BLOCK] = __uint_as_float(v.w & 0x7fffffffu);
                s = (int)(v.w >> 31);
                stage[12 * SEARCH_BLOCK] = __int_as_float(s);
            } else if (STAGE) {
                const float4* rp = reinterpret_cast<const float4*>(cnt);
                const int n4 = (P.C + 4) >> 2;  // counts and the state word; the padding behind them is not needed
                // up to twelve 16-byte loads in flight before the first of them is waited for: with a trip count the compiler does
                // not know, a load-then-store loop is one trip to memory per 16 bytes (C3: nine in a row, 42 % of the kernel)
                constexpr int NB = TIGER_TABLE == 2 ? 4 : 12;   // (same-box A/B on C3, nine 16-byte pieces: 4 -> 385.9 ms per tick, 8 -> 374, 12 -> 365.5)
                for (int k0 = 0; k0 < n4; k0 += NB) {
                    float4 v[NB];
#pragma unroll
                    for (int q = 0; q < NB; ++q) v[q] = rp[min(k0 + q, n4 - 1)];
#pragma unroll
                    for (int q = 0; q < NB; ++q) {
                        const int k = k0 + q;
                        if (k < n4) {
                            stage[(4 * k + 0) * SEARCH_BLOCK] = v[q].x;
                            stage[(4 * k + 1) * SEARCH_BLOCK] = v[q].y;
                            stage[(4 * k + 2) * SEARCH_BLOCK] = v[q].z;
                            stage[(4 * k + 3) * SEARCH_BLOCK] = v[q].w;
                        }
                    }
                }
                s = __float_as_int(stage[P.C * SEARCH_BLOCK]);
            } else {
                s = rec_state(cnt, P.C);
            }
            if (lazy_c & 1) s = lazy_state(P, g, src);   // (from g's own registers: no load behind the record's)
            if (nested) s = nest_state;
            node = 0; dtg = max_tree_depth; plen = 0; mode = 1;
        }
        PROF_MARK(0)
        if (ETIGER && start) {
            // the root's step and its child, here and not in the step phase: every lane of the phase is at node 0, its statistics are
            // in registers, its child is one bit of l1_exists -- none of what the deeper nodes need (below) is paid for
            if (dtg == 0) { mode = 0; rret = 0; }   // no depth left: the simulation ends without a step
            else {
                int o;
                double r;
                bool term;
                if (FTIGER > 0 && STAGE && FTP)
                    term = ftiger_step_packed<(FTIGER > 0 ? FTIGER : 1)>(P, g, LdsView<SEARCH_BLOCK>{stage}, s, a, o, r, NoInc{});
                else if (FTIGER > 0 && STAGE) term = ftiger_step<(FTIGER > 0 ? FTIGER : 1)>(P, g, LdsView<SEARCH_BLOCK>{stage}, s, a, o, r, NoInc{});
                else if (FTIGER > 0) term = ftiger_step<(FTIGER > 0 ? FTIGER : 1)>(P, g, GlobalSearchView{cnt}, s, a, o, r, NoInc{});
                else if (TIGER_TABLE == 2)   // (a compact record's words from the registers its load filled, not back from the stage)
                    term = tiger_step_packed(P, g, [&](int w) {
                        if (lazy_c & 2) return w == 2 ? cv.x : (w == 5 ? cv.y : (w == 10 ? cv.z : (w == 11 ? cv.w & 0x7fffffffu : 0u)));
                        return __float_as_uint(stage[w * SEARCH_BLOCK]);
                    }, s_prior, s, a, o, r, NoInc{});
                else if (STAGE) term = sim_step<REG>(P, g, LdsView<SEARCH_BLOCK>{stage}, s, a, o, r, NoInc{});
                else term = sim_step<REG>(P, g, GlobalSearchView{cnt}, s, a, o, r, NoInc{});
                ++steps;
#ifdef FBA_PROFILE_SEARCH
                prof_[11] += 1;
#endif
                path16[0] = (uint16_t)((a << 12) | (et_reward_code(r) << 14));
                plen = 1;
                if (term) { mode = 0; rret = 0; }
                else if ((l1_exists >> o) & 1u) { node = -1 - o; --dtg; }   // (a continuing step is a `listen`: the child after observation o)
                else {  // expand: the node below the root lives in LDS; then rollout(depth_to_go - 1)
                    ++n_nodes;
                    uint32_t* nd = l1 + (size_t)o * ET_NODE_WORDS * SEARCH_BLOCK;
#pragma unroll
                    for (int k = 0; k < ET_NODE_WORDS; ++k) nd[k * SEARCH_BLOCK] = 0;
                    l1_exists |= 1u << o;
                    mode = 2; rdepth = dtg - 1; rret = 0; rdisc = 1;
                    if (rdepth == 0) mode = 0;
                }
            }
        }
        PROF_MARK(7)
        bool finish = false, do_step = mode != 0;   // (lanes at a boundary sit the rest of the trip out)
        double delayed = 0;
        if (mode == 1) {  // traverseActionNode
            tree_depth = max(tree_depth, max_tree_depth - dtg);
            if (dtg == 0) { finish = true; do_step = false; }
            else if (ETIGER) {
                // the node's statistics from where they live -- LDS (the two nodes below the root, node = -1 - o), HBM (the rest) --
                // then ONE selection for all lanes.  (The root's step is the boundary phase's: node != 0 here.)
                int cn[AMAX], vis;
                double cq[AMAX];
#pragma unroll
                for (int a2 = 3; a2 < AMAX; ++a2) { cn[a2] = 0; cq[a2] = 0.0; }   // (A = 3: never looked at)
                if (node < 0) {
                    const uint32_t* nd = l1 + (size_t)(-1 - node) * ET_NODE_WORDS * SEARCH_BLOCK;
                    const uint32_t w0 = nd[0], w1 = nd[1 * SEARCH_BLOCK];
                    cn[0] = (int)(w0 & 0xffffu); cn[1] = (int)(w0 >> 16); cn[2] = (int)(w1 & 0xffffu);
#pragma unroll
                    for (int a2 = 0; a2 < 3; ++a2)
                        cq[a2] = __hiloint2double((int)nd[(4 + 2 * a2) * SEARCH_BLOCK], (int)nd[(3 + 2 * a2) * SEARCH_BLOCK]);
                    vis = (cn[0] + cn[1]) + cn[2];
                } else {
                    const int32_t* rec = tree + (size_t)node * W;
                    const int4 h      = *reinterpret_cast<const int4*>(rec);
                    const double2 q01 = *reinterpret_cast<const double2*>(rec + 4);
                    const double q2   = *reinterpret_cast<const double*>(rec + 8);
                    vis = h.x; cn[0] = h.y; cn[1] = h.z; cn[2] = h.w;
                    cq[0] = q01.x; cq[1] = q01.y; cq[2] = q2;
                }
                a = ucb_pick<AMAX>(P, g, D.log1p_tab, vis, cn, cq, true);
                if (plen == 2) { cy_h2 = make_int4(vis, cn[0], cn[1], cn[2]); cy_q2 = a == 0 ? cq[0] : (a == 1 ? cq[1] : cq[2]); }
                if (plen == 3) { cy_h3 = make_int4(vis, cn[0], cn[1], cn[2]); cy_q3 = a == 0 ? cq[0] : (a == 1 ? cq[1] : cq[2]); }
            }
            else if (node == 0) a = ucb_pick<AMAX>(P, g, D.log1p_tab, r_vis, r_cn, r_cq, true);
            else a = ucb_select<AMAX>(P, D, g, tree + (size_t)node * W, true);
        } else if (mode == 2) {  // rollout: uniformly random action
            a = domain_random_action(P, g, s);
        }
        PROF_MARK(1)
        int o;
        double r;
        bool term;
        if (do_step) {
            if (FTIGER > 0 && STAGE && FTP)
                term = ftiger_step_packed<(FTIGER > 0 ? FTIGER : 1)>(P, g, LdsView<SEARCH_BLOCK>{stage}, s, a, o, r, NoInc{});
            else if (FTIGER > 0 && STAGE) term = ftiger_step<(FTIGER > 0 ? FTIGER : 1)>(P, g, LdsView<SEARCH_BLOCK>{stage}, s, a, o, r, NoInc{});
            else if (FTIGER > 0) term = ftiger_step<(FTIGER > 0 ? FTIGER : 1)>(P, g, GlobalSearchView{cnt}, s, a, o, r, NoInc{});
            else if (TIGER_TABLE == 2)
                term = tiger_step_packed(P, g, [&](int w) { return __float_as_uint(stage[w * SEARCH_BLOCK]); }, s_prior, s, a, o, r, NoInc{});
            else if (STAGE) term = sim_step<REG>(P, g, LdsView<SEARCH_BLOCK>{stage}, s, a, o, r, NoInc{});
            else term = sim_step<REG>(P, g, GlobalSearchView{cnt}, s, a, o, r, NoInc{});
            ++steps;
#ifdef FBA_PROFILE_SEARCH
        }
        PROF_MARK(2)
        if (do_step) {
#endif
            if (ETIGER && mode == 1) {  // traverseChanceNode on the episodic tiger tree
                path16[(size_t)plen * SEARCH_BLOCK] = (uint16_t)((node < 0 ? -1 - node : node) | (a << 12) | (et_reward_code(r) << 14));
                ++plen;
                if (term) finish = true;
                else {   // (a continuing step is a `listen`: the child after observation o)
                    int c = 0;   // 0 = none yet (the root is nobody's child)
                    if (node < 0) {
                        const uint32_t w2 = l1[((size_t)(-1 - node) * ET_NODE_WORDS + 2) * SEARCH_BLOCK];
                        c = (int)(o ? (w2 >> 16) : (w2 & 0xffffu));
                    } else {
                        c = tree[(size_t)node * W + D.child_off + 2 * 2 + o];
                        c = c < 0 ? 0 : c;
                    }
                    if (c != 0) { node = c; --dtg; }
                    else {  // expand: new leaf, then rollout(depth_to_go - 1)
                        const int nn = min(n_nodes, D.max_nodes - 1);
                        ++n_nodes;
                        node_init(D, tree + (size_t)nn * W, P.A, P.O);
                        if (node < 0) {
                            uint32_t* w2 = l1 + ((size_t)(-1 - node) * ET_NODE_WORDS + 2) * SEARCH_BLOCK;
                            *w2 = o ? ((*w2 & 0xffffu) | ((uint32_t)nn << 16)) : ((*w2 & 0xffff0000u) | (uint32_t)nn);
                        } else tree[(size_t)node * W + D.child_off + 2 * 2 + o] = nn;
                        mode = 2; rdepth = dtg - 1; rret = 0; rdisc = 1;
                        if (rdepth == 0) finish = true;
                    }
                }
            } else if (mode == 1) {  // traverseChanceNode
                path_r[(size_t)plen * SEARCH_BLOCK]  = (float)r;
                path_na[(size_t)plen * SEARCH_BLOCK] = (node << 5) | a  /* a < FBA_MAX_ACTIONS <= 32 */;
                ++plen;
                if (term) finish = true;
                else {
                    const bool at_root_lds = root_lds && node == 0;
                    const int c = at_root_lds ? rootch[(a * P.O + o) * SEARCH_BLOCK] : child_get(P, D, tree, tab, epoch, node, a, o);
                    if (c >= 0) { node = c; --dtg; }
                    else {  // expand: new leaf, then rollout(depth_to_go - 1)
                        // never write past the slot's records: beyond the host's node bound (fba_engine.hip; cannot happen
                        // while that bound holds) the last record is reused and the overflow reported after the loop.  (A
                        // `break` here instead cost the whole kernel 45 %: the loop lost its shape.)
                        const int nn = min(n_nodes, D.max_nodes - 1);
                        ++n_nodes;
                        node_init(D, tree + (size_t)nn * W, P.A, P.O);
                        if (at_root_lds) rootch[(a * P.O + o) * SEARCH_BLOCK] = (int16_t)nn;
                        else child_set(P, D, tree, tab, epoch, node, a, o, nn);
                        mode = 2; rdepth = dtg - 1; rret = 0; rdisc = 1;
                        if (rdepth == 0) finish = true;
                    }
                }
            } else {
                rret += r * rdisc;
                rdisc *= P.gamma;
                --rdepth;
                if (rdepth == 0 || term) { delayed = rret; finish = true; }
            }
        }
        PROF_MARK(3)
        if (finish) { rret = delayed; mode = 0; }   // (to the boundary: what the back-up needs beside the path is the rollout's return)
#ifdef FBA_PROFILE_SEARCH
        {
            const int n_step_ = __popcll(__ballot(do_step));
            if (lead_) prof_[8] += n_step_;
        }
#endif
    }
#ifdef FBA_PROFILE_SEARCH
    // cycles: lane 0's clock, as ever; trips [5], stepping lanes [8], boundary phases [9] and the lanes they served [10]: from whichever
    // lane led its wave (the first active lane of a ballot -- lane 0 may belong to an inactive slot); root steps [11]: every lane's own
    for (int r = 0; r < 12; ++r)
        if (r == 5 || r >= 8 ? prof_[r] != 0 : lane == 0) atomicAdd(&g_search_prof[r], (unsigned long long)prof_[r]);
#endif
    g.stream(FBA_PHASE_SEARCH, (uint32_t)P.sims + 1u);
    if (n_nodes > D.max_nodes) atomicCAS(D.fault, 0, -(1 + e));  // -> FBA_ESTATE on the host
    const int best = ucb_pick<AMAX>(P, g, D.log1p_tab, 0, r_cn, r_cq, false);
    D.action[e]    = best;
    D.sim_steps[e] += steps;
    fba_trace_rec& rec = D.cur[e];
    rec.n_nodes    = n_nodes;
    rec.tree_depth = tree_depth;
#pragma unroll
    for (int a = 0; a < FBA_MAX_ACTIONS; ++a) {
        rec.root_n[a] = a < AMAX && a < P.A ? r_cn[a < AMAX ? a : 0] : 0;
        rec.root_q[a] = a < AMAX && a < P.A ? r_cq[a < AMAX ? a : 0] : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------
// search_hist_kernel: the same search (POUCT / RBAPOUCT::selectAction, state machine of search_kernel) for
// history particles (fba_device.h) -- the gridworld FBA-POMDP of BASELINE configs[3].  A tree of 65 536
// simulations costs megabytes of HBM, so a GPU holds tens of thousands of them, not the hundreds of thousands that
// "one lane = one tree" needs to keep its SIMDs busy.  Here FOUR lanes share a tree: every lane carries the whole
// search state and executes the tree logic redundantly (same addresses, same values: loads coalesce, stores
// agree), and the simulator step -- where the time goes -- is split: lane q generates Philox block q of the
// quad's eight draws, lane f < 3 scans the history for, fetches and samples the Dirichlet row of state /
// observation feature f (gridworld_hist_step_quad).  Sixteen trees per wave, four times the waves per tree count;
// same draws, same order, same results as search_kernel on dense records.
// LDS per wave: path [depth][16], the root particle's record [2 + entries][16].
// ---------------------------------------------------------------------------------------------
template <int K>
__global__ void __launch_bounds__(SEARCH_BLOCK) search_hist_kernel(Problem P, DeviceState D)
{
    constexpr int AMAX = 4;
    P.model = FBA_MODEL_BA_FACTORED; P.domain = FBA_DOM_GRIDWORLD; P.A = 4; P.belief = FBA_BELIEF_IMPORTANCE;
    extern __shared__ double lds[];
    const int lane = threadIdx.x, tl = lane >> 2;
    const int e    = blockIdx.x * HIST_TREES + tl;
    if (e >= P.E || !D.active[e]) return;  // (a quad leaves together)

    const int depth_cap = P.max_depth > 0 ? P.max_depth : 1;
    // the chosen action's count and Q of every node on the path as the descent loaded them: the back-up needs no load (a trip to
    // memory per level, twenty in a row at t = 0), only its two stores -- nothing else writes this tree
    double* path_q   = lds + tl;                                                                                  // [depth][trees]
    int32_t* path_n  = reinterpret_cast<int32_t*>(path_q - tl + (size_t)depth_cap * HIST_TREES) + tl;
    float* path_r    = reinterpret_cast<float*>(path_n - tl + (size_t)depth_cap * HIST_TREES) + tl;
    int32_t* path_na = reinterpret_cast<int32_t*>(path_r - tl + (size_t)depth_cap * HIST_TREES) + tl;
    uint32_t* stage  = reinterpret_cast<uint32_t*>(path_na - tl + (size_t)depth_cap * HIST_TREES) + tl;           // [Cs][trees]
    const bool carry = D.cn_off == 0;   // (the 48-byte record of hashed trees with four actions: {n0..n3}, {q0..q3}; others reload)
    // Child speculation.  A tree level costs two dependent trips to memory: the node's statistics, then -- once the step has produced
    // the observation -- the hash probe for the child.  The upper 16 bits of a node's count words (a node below the root has fewer than
    // 65 536 visits) remember the child each action led to last time; its statistics are requested right after the action is chosen,
    // so they are on their way while the step is computed and the probe answers.  The probe still decides: a wrong guess costs a
    // wasted request, never a result.  (child index = hint + 2; hint + 2 == the node itself = none; the root's hints live in registers.)
    const bool spec = carry && D.max_nodes <= 65538 && P.sims <= 65536;
    int pf_node = -1;
    int4 pf_h = make_int4(0, 0, 0, 0);
    double2 pf_q01 = make_double2(0, 0), pf_q23 = make_double2(0, 0);
    int r_hint[AMAX] = {0, 0, 0, 0};   // the root's: child index, 0 = none

    QuadRng g;
    g.init(P.seed_lo, P.seed_hi, (uint32_t)D.run[e], (uint32_t)D.episode[e], (uint32_t)D.t[e], lane);
    const int hist_len  = D.t[e];
    const int max_tree_depth = min(P.horizon - hist_len, P.max_depth);
    const int W         = D.node_words;
    int32_t* tree       = D.nodes + (size_t)e * D.max_nodes * W;
    const float* prec   = D.p_rec + rec_base(P, D, e, D.bufsel[e]) * (size_t)P.Cs;
    const uint32_t hist_cnt = D.hist_cnt[e];  // entries of each action in every record of this slot, and where each group starts
    const int hist_n        = hist_total(hist_cnt);
    const uint32_t hist_off = (uint32_t)hist_offset(hist_cnt, 1) << 8 | (uint32_t)hist_offset(hist_cnt, 2) << 16 | (uint32_t)hist_offset(hist_cnt, 3) << 24;

    if (P.planner == FBA_PLANNER_RANDOM) {  // RandomPlanner::selectAction RandomPlanner.cpp:14-24
        g.stream(FBA_PHASE_SEARCH, (uint32_t)P.sims);
        g.ensure(2);
        (void)g.u01();                      // the belief sample: GridWorld::generateRandomAction does not look at the state
        D.action[e] = g.slow_int(0, 4);
        if (P.search_budget > 0) D.search_done[e] = 1;
        return;
    }
    // budgeted launches (Problem::search_budget): a search parked by an earlier launch is taken up where it stopped -- its tree and
    // hash table are where it left them, the root's statistics come back from the root's record
    const int budget  = P.search_budget;
    int sim           = budget > 0 ? D.s_sim[e] : 0;
    const bool resume = sim > 0;
    int n_nodes = 1, tree_depth = 0;
    unsigned long long steps = 0;
    int r_vis = 0, r_cn[AMAX];
    double r_cq[AMAX];
#pragma unroll
    for (int a = 0; a < AMAX; ++a) { r_cn[a] = 0; r_cq[a] = 0.0; }
    int4* tab = hash_table(D, e);
    uint32_t epoch;
    if (!resume) {
        node_init(D, tree, P.A, P.O);
        epoch = hash_begin_search(D, e, tab, g.q, HIST_QUAD);
    } else {
        n_nodes    = D.s_nodes[e];
        tree_depth = D.s_depth[e];
        epoch      = D.epoch[e];
        const double* rq = reinterpret_cast<const double*>(tree + D.cq_off);
#pragma unroll
        for (int a = 0; a < AMAX; ++a) { r_cn[a] = tree[D.cn_off + a]; r_cq[a] = rq[a]; r_vis += r_cn[a]; }
    }
    int ts_src = -1;
    if (P.planner == FBA_PLANNER_TS) {  // TSPlanner / BATSPlanner: one belief sample, then the search from that particle
        g.stream(FBA_PHASE_SEARCH, (uint32_t)P.sims + 2u);
        g.ensure(1);
        ts_src = uniform_weight_pick(D.uni_scan, P.N, g.u01() * D.uni_total, D.uni_total);
    }
    int mode = 0, iter = 0;  // 0 = start a simulation, 1 = in the tree, 2 = rollout
    int node = 0, dtg = 0, plen = 0, rdepth = 0;
    uint32_t sp = 0, hist_mask = 0;
    double rret = 0, rdisc = 1;
#ifdef FBA_PROFILE_SEARCH
    long long prof_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, prev_ = clock64();
#endif
    while (true) {
        PROF_MARK(6)
        if (mode == 0) {
            if (sim >= P.sims) break;
            if (budget > 0 && iter >= budget) break;   // out of iterations at a simulation boundary: park the search (below)
            g.stream(FBA_PHASE_SEARCH, (uint32_t)sim);
            g.ensure(8);  // the root sample, the first action, six rows
            const int src = ts_src >= 0 ? ts_src : uniform_weight_pick(D.uni_scan, P.N, g.u01() * D.uni_total, D.uni_total);
            const uint4* rp = reinterpret_cast<const uint4*>(prec + (size_t)src * hist_stride(P, hist_n));
            const int n4 = (hist_n + 5) >> 2;  // state, structure bits, entries
            for (int k0 = g.q; k0 < n4; k0 += 4 * HIST_QUAD) {   // (four loads in flight per lane, as in search_kernel)
                uint4 v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = rp[min(k0 + q * HIST_QUAD, n4 - 1)];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = k0 + q * HIST_QUAD;
                    if (k < n4) {
                        stage[(4 * k + 0) * HIST_TREES] = v[q].x;
                        stage[(4 * k + 1) * HIST_TREES] = v[q].y;
                        stage[(4 * k + 2) * HIST_TREES] = v[q].z;
                        stage[(4 * k + 3) * HIST_TREES] = v[q].w;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the other lanes' pieces (LDS operations of one wave complete in order)
            hist_mask = stage[1 * HIST_TREES];
            sp        = (hist_mask >> 16) & 0x3ffu;
            node = 0; dtg = max_tree_depth; plen = 0; mode = 1;
        }
        PROF_MARK(0)
        bool finish = false, do_step = true;
        double delayed = 0;
        int a = 0;
        if (mode == 1 && dtg == 0) { finish = true; do_step = false; }
        if (mode == 1) tree_depth = max(tree_depth, max_tree_depth - dtg);
        int o = 0;
        double r = 0;
        bool term = false;
        if (do_step) {
            g.ensure(7);  // the action, six rows
            if (mode == 1) {  // traverseActionNode
                int guess = 0;   // spec: the child this (node, action) led to last time, 0 = none
                if (node == 0) {
                    a = ucb_pick<AMAX>(P, g, D.log1p_tab, r_vis, r_cn, r_cq, true);
                    if (spec) {
                        guess = a == 0 ? r_hint[0] : (a == 1 ? r_hint[1] : (a == 2 ? r_hint[2] : r_hint[3]));
                        if (guess >= min(n_nodes, D.max_nodes)) guess = 0;
                    }
                } else if (carry) {
                    const int32_t* rec = tree + (size_t)node * W;
                    int4 h;
                    double2 q01, q23;
                    if (spec && node == pf_node) { h = pf_h; q01 = pf_q01; q23 = pf_q23; }   // requested a level ago
                    else {
                        h   = *reinterpret_cast<const int4*>(rec);
                        q01 = *reinterpret_cast<const double2*>(rec + 4);
                        q23 = *reinterpret_cast<const double2*>(rec + 8);
                    }
                    const int m = spec ? 0xffff : -1;
                    const int cn[AMAX]    = {h.x & m, h.y & m, h.z & m, h.w & m};
                    const double cq[AMAX] = {q01.x, q01.y, q23.x, q23.y};
                    a = ucb_pick<AMAX>(P, g, D.log1p_tab, ((cn[0] + cn[1]) + cn[2]) + cn[3], cn, cq, true);
                    const int word = a == 0 ? h.x : (a == 1 ? h.y : (a == 2 ? h.z : h.w));
                    path_n[(size_t)plen * HIST_TREES] = word;   // (spec: count | hint << 16)
                    path_q[(size_t)plen * HIST_TREES] = a == 0 ? q01.x : (a == 1 ? q01.y : (a == 2 ? q23.x : q23.y));
                    if (spec) {
                        guess = (int)((uint32_t)word >> 16) + 2;
                        if (guess == node || guess >= min(n_nodes, D.max_nodes)) guess = 0;   // none (node 1's "itself" does not fit the encoding), or not a node
                    }
                } else a = ucb_select<AMAX>(P, D, g, tree + (size_t)node * W, true);
                if (spec && guess > 0) {   // the likely child's statistics, on their way while the step is computed
                    const int32_t* crec = tree + (size_t)guess * W;
                    pf_h    = *reinterpret_cast<const int4*>(crec);
                    pf_q01  = *reinterpret_cast<const double2*>(crec + 4);
                    pf_q23  = *reinterpret_cast<const double2*>(crec + 8);
                    pf_node = guess;
                } else pf_node = -1;
            } else {
                a = g.slow_int(0, 4);  // GridWorld::generateRandomAction :220-226
            }
#ifdef FBA_PROFILE_SEARCH
        }
        PROF_MARK(1)
        if (do_step) {
#endif
            term = gridworld_hist_step_quad<K, HIST_TREES>(P, g, stage + (size_t)(2 + ((hist_off >> (8 * a)) & 0xffu)) * HIST_TREES,
                                                           hist_count(hist_cnt, a), hist_mask, sp, a, o, r,
                                                           HistRowsGlobal{P.hist_base, P.hist_alt, P.hist_base + HistLayout(P.gw_N, P.gw_G, 4).obase0, HistLayout(P.gw_N, P.gw_G, 4)});
            ++steps;
#ifdef FBA_PROFILE_SEARCH
        }
        PROF_MARK(2)
        if (do_step) {
#endif
            if (mode == 1) {  // traverseChanceNode
                path_r[(size_t)plen * HIST_TREES]  = (float)r;
                path_na[(size_t)plen * HIST_TREES] = (node << 5) | a;
                ++plen;
                if (term) finish = true;
                else {
                    const int c = child_get(P, D, tree, tab, epoch, node, a, o);
                    const int nn = min(n_nodes, D.max_nodes - 1);   // (the node an expansion creates)
                    if (spec) {   // remember where (node, a) led: the root's hint in its register, a node's in the word the back-up stores
                        const int to = c >= 0 ? c : nn;
                        if (node == 0) {
#pragma unroll
                            for (int a2 = 0; a2 < AMAX; ++a2)
                                if (a2 == a) r_hint[a2] = to;
                        } else {
                            int32_t* pw = path_n + (size_t)(plen - 1) * HIST_TREES;
                            *pw = (*pw & 0xffff) | (int)((uint32_t)((to - 2) & 0xffff) << 16);
                        }
                    }
                    if (c >= 0) { node = c; --dtg; }
                    else {  // expand: new leaf, then rollout(depth_to_go - 1)
                        ++n_nodes;
                        if (spec) {   // counts 0, no child remembered (hint + 2 == the node itself), Q 0
                            int32_t* nrec = tree + (size_t)nn * W;
                            const int none = (int)((uint32_t)((nn - 2) & 0xffff) << 16);
                            *reinterpret_cast<int4*>(nrec)        = make_int4(none, none, none, none);
                            *reinterpret_cast<double2*>(nrec + 4) = make_double2(0.0, 0.0);
                            *reinterpret_cast<double2*>(nrec + 8) = make_double2(0.0, 0.0);
                        } else node_init(D, tree + (size_t)nn * W, P.A, P.O);
                        child_set(P, D, tree, tab, epoch, node, a, o, nn);
                        mode = 2; rdepth = dtg - 1; rret = 0; rdisc = 1;
                        if (rdepth == 0) finish = true;
                    }
                }
            } else {
                rret += r * rdisc;
                rdisc *= P.gamma;
                --rdepth;
                if (rdepth == 0 || term) { delayed = rret; finish = true; }
            }
        }
        PROF_MARK(3)
        if (finish) {  // back-up, leaf to root (MCTSTreeNodes.cpp:8-12, 59-62)
            double del = delayed;
            for (int k = plen - 1; k >= 0; --k) {
                const int na     = path_na[(size_t)k * HIST_TREES];
                const double ret = (double)path_r[(size_t)k * HIST_TREES] + P.gamma * del;
                const int act    = na & 31;
                if ((na >> 5) == 0) {
                    int n = 0;
                    double q = 0.0;
#pragma unroll
                    for (int a2 = 0; a2 < AMAX; ++a2)
                        if (a2 == act) { n = r_cn[a2]; q = r_cq[a2]; }
                    ++n;
                    q += (ret - q) / (double)n;
#pragma unroll
                    for (int a2 = 0; a2 < AMAX; ++a2)
                        if (a2 == act) { r_cn[a2] = n; r_cq[a2] = q; }
                    ++r_vis;
                } else if (carry) {
                    int32_t* rec    = tree + (size_t)(na >> 5) * W;
                    const int word  = path_n[(size_t)k * HIST_TREES];
                    const int n     = (spec ? (word & 0xffff) : word) + 1;
                    const double q0 = path_q[(size_t)k * HIST_TREES];
                    rec[act] = spec ? ((word & (int)0xffff0000) | n) : n;
                    reinterpret_cast<double*>(rec + D.cq_off)[act] = q0 + (ret - q0) / (double)n;
                } else {
                    int32_t* rec = tree + (size_t)(na >> 5) * W;
                    double* q    = reinterpret_cast<double*>(rec + D.cq_off) + act;
                    const int n  = ++rec[D.cn_off + act];
                    if (D.cn_off) ++rec[0];
                    *q += (ret - *q) / (double)n;
                }
                del = ret;
            }
            ++sim;
            mode = 0;
        }
        PROF_MARK(4)
        ++iter;
#ifdef FBA_PROFILE_SEARCH
        prof_[5] += 1;
#endif
    }
#ifdef FBA_PROFILE_SEARCH
    if (lane == 0)
        for (int r2 = 0; r2 < 8; ++r2) atomicAdd(&g_search_prof[r2], (unsigned long long)prof_[r2]);
#endif
    if (sim < P.sims) {   // parked: the four lanes of the quad hold the same values and store them to the same places
        double* rq = reinterpret_cast<double*>(tree + D.cq_off);
#pragma unroll
        for (int a = 0; a < AMAX; ++a) { tree[D.cn_off + a] = r_cn[a]; rq[a] = r_cq[a]; }
        if (D.cn_off) tree[0] = r_vis;
        D.s_sim[e]   = sim;
        D.s_nodes[e] = n_nodes;
        D.s_depth[e] = tree_depth;
        if (g.q == 0) D.sim_steps[e] += steps;
        return;   // (search_done[e] stays 0: env_kernel leaves the slot alone)
    }
    if (D.s_sim) D.s_sim[e] = 0;   // (also after a whole search run on a budgeted context, fba_select_action: what was parked for this slot is stale)
    if (budget > 0) D.search_done[e] = 1;
    g.stream(FBA_PHASE_SEARCH, (uint32_t)P.sims + 1u);
    g.ensure(1);
    if (n_nodes > D.max_nodes) atomicCAS(D.fault, 0, -(1 + e));
    const int best = ucb_pick<AMAX>(P, g, D.log1p_tab, 0, r_cn, r_cq, false);
    D.action[e]    = best;
    if (g.q == 0) D.sim_steps[e] += steps;
    fba_trace_rec& rec = D.cur[e];
    rec.n_nodes    = n_nodes;
    rec.tree_depth = tree_depth;
#pragma unroll
    for (int a = 0; a < FBA_MAX_ACTIONS; ++a) {
        rec.root_n[a] = a < AMAX ? r_cn[a < AMAX ? a : 0] : 0;
        rec.root_q[a] = a < AMAX ? r_cq[a < AMAX ? a : 0] : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------
// search_hist2_kernel: the history-particle search on a tree whose node IS its hash bucket, with every trip to HBM asked for one
// loop iteration before it is needed.
//
// What bounded search_hist_kernel was the chain of dependent trips a tree level makes -- the node's
// statistics, the two Dirichlet-row fetches of the step, then the hash probe for the child -- at two waves per SIMD, with the sixteen
// trees of a wave in different phases, so that nearly every iteration of the wave waited for all of them.  Here:
//   * DeviceState::bkt: one open-addressing table per slot, 64-byte buckets, two to a 128-byte line (the unit the memory side moves:
//     profiles/r04_randline_counters.json).  A bucket is a node -- key = (parent bucket, action, observation) | epoch << 28, the four
//     action counts as uint16, the four Q values -- so the probe for the child of (node, a, o) returns the child's statistics: one trip
//     per level where there were two.  Three quarters of a gridworld tree's nodes are created and never reached again (measured on the
//     CPU restatement: 48 000 of 65 537 at the BASELINE size); they have no statistics to keep and live as 4-byte keys in the last 16 bytes
//     of the buckets (eight per line), found by the same one-line probe.  A node gets a bucket when it is reached a second time.
//     Probing is linear over lines; a probe ends at the first line with a free bucket (nodes) / a free key slot (keys), nothing is ever
//     deleted, the epoch in the key makes the table empty for the next search.
//   * The line of the child is requested right after the step that produced the observation and consumed at the top of the NEXT
//     iteration: the wave executes a whole iteration of the other trees' work in between.  The four lanes of a quad each load a quarter
//     of the line (lane q: piece q of both buckets; lane 3 the eight keys) and exchange what is needed by DPP.  The next simulation's
//     root particle is requested when the current one finishes, the same way.
//   * The observation tables of the prior (3.7 KB) sit in LDS: the second of a step's two dependent row fetches never leaves the CU.
//   * A filter of 2^k uniformly weighted particles is sampled in closed form (its prefix sums are exact multiples of 2^-k).
// Same streams, same draws, same arithmetic as search_hist_kernel: every trace field is bit-equal.
// ---------------------------------------------------------------------------------------------
constexpr int H2_PF = 3;   // 16-byte pieces per lane the prefetch registers hold (a root particle of up to 12 pieces = 46 entries; more are fetched in place)

template <int LANE>
__device__ __forceinline__ uint32_t quad_get(uint32_t v)   // the value lane LANE of this quad holds (all four lanes of a quad are always active together)
{
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, LANE * 0x55, 0xf, 0xf, true);
}
template <int LANE>
__device__ __forceinline__ double quad_get_f64(uint32_t lo, uint32_t hi)
{
    return __hiloint2double((int)quad_get<LANE>(hi), (int)quad_get<LANE>(lo));
}
__device__ __forceinline__ uint32_t h2_home_line(uint32_t code, uint32_t nlines) { return __umulhi(child_hash((uint64_t)code), nlines); }
// (24-bit multiplies for the row numbers and a cheaper 32-bit mix here were each about 1 % SLOWER on C4, same box: profiles/r04_search_experiments.txt 11)

#ifndef FBA_HIST2_WAVES
#define FBA_HIST2_WAVES 3   // waves per SIMD the register allocation aims at: 3 = at most 168 VGPRs, which the kernel meets with two spilled registers since
                            // the root's statistics moved to LDS (with them in registers the cap spilled 14-17 and cost 24 %); 2 = 175, for A/B builds
#endif
// LROWS: every Dirichlet row of the prior comes from LDS (Problem::hist_lds: row ids + the distinct rows, shared by the H2_WAVES waves of a
// workgroup); otherwise the transition rows come from the padded tables in HBM and only the observation tables sit in LDS.
constexpr int H2_BLOCK = H2_WAVES * 64;   // (H2_WAVES, h2_shared_bytes, h2_wave_bytes: fba_launch_plan.h)
// search_order (fba_state.h): a counting sort of the slots by the depth their searches have left (inactive slots first).  One workgroup; which of two
// slots of equal depth comes first is left to the atomics -- every tree is independent, so no result can depend on it.
__global__ void __launch_bounds__(1024) search_order_kernel(Problem P, DeviceState D)
{
    __shared__ int32_t s_cnt[258];
    const int tid = threadIdx.x;
    for (int k = tid; k < 258; k += 1024) s_cnt[k] = 0;
    __syncthreads();
    auto key_of = [&](int e) { return D.active[e] ? 1 + min(max(min(P.horizon - D.t[e], P.max_depth), 0), 255) : 0; };
    for (int e = tid; e < P.E; e += 1024) atomicAdd(&s_cnt[key_of(e) + 1], 1);
    __syncthreads();
    if (tid == 0)
        for (int k = 1; k < 258; ++k) s_cnt[k] += s_cnt[k - 1];   // s_cnt[key] = first place of the key
    __syncthreads();
    for (int e = tid; e < P.E; e += 1024) D.search_order[atomicAdd(&s_cnt[key_of(e)], 1)] = e;
}

// The kernel's body is fba_search_hist2.inc, stamped into two kernels by FLAT:
//   search_hist2_kernel  FLAT = false: an importance filter -- the root particle is the weighted pick on the prefix sums of N weights 1/N
//                        (WeightedFilter::sample), in closed form for N = 2^k;
//   hist2_flat_search    FLAT = true: the plain rejection filter -- the root particle is uniform_int(N) (FlatFilter::sample, FlatFilter.cpp:97-102).
// One draw either way, so the eight draws ensured per root stay.  (Textual inclusion, not an inlined template function: inlining the body
// into the kernel changed the importance kernel's register allocation; included, its code is the instruction stream it was.)
template <int K, bool LROWS>
__global__ void __launch_bounds__(H2_BLOCK) __attribute__((amdgpu_waves_per_eu(FBA_HIST2_WAVES, FBA_HIST2_WAVES))) search_hist2_kernel(Problem P, DeviceState D)
{
    constexpr bool FLAT = false, TAB = false;
#include "fba_search_hist2.inc"
}
template <int K, bool LROWS>
__global__ void __launch_bounds__(H2_BLOCK) __attribute__((amdgpu_waves_per_eu(FBA_HIST2_WAVES, FBA_HIST2_WAVES))) hist2_flat_search(Problem P, DeviceState D)
{
    constexpr bool FLAT = true, TAB = false;
#include "fba_search_hist2.inc"
}
// The same search on the records of the tabular gridworld BA-POMDP (Problem::hist == 2), for the two root samples.  K and LROWS name no rows
// here: the step reads the prior's sparse rows (TabRows) from L2, and the workgroup stages no shared tables.
template <bool FLATV>
__global__ void __launch_bounds__(H2_BLOCK) __attribute__((amdgpu_waves_per_eu(FBA_HIST2_WAVES, FBA_HIST2_WAVES))) search_tabhist_kernel(Problem P, DeviceState D)
{
    constexpr bool FLAT = FLATV, TAB = true, LROWS = false;
    constexpr int K = 8;
#include "fba_search_hist2.inc"
}

// ---------------------------------------------------------------------------------------------
// search_ca_hist_kernel: search_kernel's search -- one lane = one slot = one tree, the same state machine, node records and
// child table, the same streams and draws -- on history particles of the collision-avoidance FBA-POMDP (Problem::hist == 3).
// The workgroup keeps the whole prior table and its sequence table in LDS (ca_hist_stage_tables); a simulation root-samples
// through the weighted filter (uniform weights: the filter was resampled by its last update), stages the chosen record --
// 8 + 4 * entries bytes instead of the dense 3.5 KB -- as [word][lane] and steps with ca_hist_step over it.
// LDS: the tables, then per lane the path [depth] {reward, node << 5 | action} and the record [Cs].
// ---------------------------------------------------------------------------------------------
template <int AMAX>
__global__ void __launch_bounds__(SEARCH_BLOCK) search_ca_hist_kernel(Problem P, DeviceState D)
{
    extern __shared__ uint4 lds4[];
    const int lane = threadIdx.x;
    const int e    = blockIdx.x * SEARCH_BLOCK + lane;
    CaTables T;
    const int tbytes = ca_hist_stage_tables(P, P.hist_row, lds4, lane, SEARCH_BLOCK, T);
    __syncthreads();
    if (e >= P.E || !D.active[e]) return;

    const int depth_cap = P.max_depth > 0 ? P.max_depth : 1;
    float* path_r    = reinterpret_cast<float*>(reinterpret_cast<char*>(lds4) + tbytes) + lane;                      // [depth][block]
    int32_t* path_na = reinterpret_cast<int32_t*>(path_r - lane + (size_t)depth_cap * SEARCH_BLOCK) + lane;          // [depth][block]
    uint32_t* stage  = reinterpret_cast<uint32_t*>(path_na - lane + (size_t)depth_cap * SEARCH_BLOCK) + lane;        // [Cs][block]

    Rng g               = slot_rng(P, D, e);
    const int hist_len  = D.t[e];
    const int max_tree_depth = min(P.horizon - hist_len, P.max_depth);
    const int W         = D.node_words;
    int32_t* tree       = D.nodes + (size_t)e * D.max_nodes * W;
    const uint32_t hist_cnt = D.hist_cnt[e];
    const int total     = hist_total(hist_cnt), rs = hist_stride(P, total);
    const uint32_t* prec = reinterpret_cast<const uint32_t*>(D.p_rec + rec_base(P, D, e, D.bufsel[e]) * (size_t)P.Cs);

    if (P.planner == FBA_PLANNER_RANDOM) {  // RandomPlanner::selectAction RandomPlanner.cpp:14-24
        g.stream(FBA_PHASE_SEARCH, (uint32_t)P.sims);
        const int src = belief_sample_uniform(P, D, g);
        D.action[e]   = domain_random_action(P, g, (int)prec[(size_t)src * rs]);
        return;
    }
    node_init(D, tree, P.A, P.O);
    int n_nodes = 1, tree_depth = 0;
    unsigned long long steps = 0;
    // the root's visit counts and Q values live in registers for the whole search (search_kernel)
    int r_vis = 0, r_cn[AMAX];
    double r_cq[AMAX];
#pragma unroll
    for (int a = 0; a < AMAX; ++a) { r_cn[a] = 0; r_cq[a] = 0.0; }
    int4* tab            = hash_table(D, e);
    const uint32_t epoch = D.hash ? hash_begin_search(D, e, tab, 0, 1) : 0;
    const int n4         = (2 + total + 3) >> 2;   // 16-byte pieces of a record that are alive

    int sim = 0, mode = 0;  // 0 = start a simulation, 1 = in the tree, 2 = rollout
    int s = 0, node = 0, dtg = 0, plen = 0, rdepth = 0;
    double rret = 0, rdisc = 1;
    while (true) {
        if (mode == 0) {
            if (sim >= P.sims) break;
            g.stream(FBA_PHASE_SEARCH, (uint32_t)sim);
            const int src   = belief_sample_uniform(P, D, g);
            const uint4* rp = reinterpret_cast<const uint4*>(prec + (size_t)src * rs);
            constexpr int NB = 8;   // 16-byte loads in flight before the first is waited for
            for (int k0 = 0; k0 < n4; k0 += NB) {
                uint4 v[NB];
#pragma unroll
                for (int q = 0; q < NB; ++q) v[q] = rp[min(k0 + q, n4 - 1)];
#pragma unroll
                for (int q = 0; q < NB; ++q) {
                    const int k = k0 + q;
                    if (k < n4) {
                        stage[(4 * k + 0) * SEARCH_BLOCK] = v[q].x;
                        stage[(4 * k + 1) * SEARCH_BLOCK] = v[q].y;
                        stage[(4 * k + 2) * SEARCH_BLOCK] = v[q].z;
                        stage[(4 * k + 3) * SEARCH_BLOCK] = v[q].w;
                    }
                }
            }
            s = (int)stage[0];
            node = 0; dtg = max_tree_depth; plen = 0; mode = 1;
        }
        bool finish = false, do_step = true;
        double delayed = 0;
        int a = 0;
        if (mode == 1) {  // traverseActionNode
            tree_depth = max(tree_depth, max_tree_depth - dtg);
            if (dtg == 0) { finish = true; do_step = false; }
            else if (node == 0) a = ucb_pick<AMAX>(P, g, D.log1p_tab, r_vis, r_cn, r_cq, true);
            else a = ucb_select<AMAX>(P, D, g, tree + (size_t)node * W, true);
        } else {          // rollout: uniformly random action
            a = domain_random_action(P, g, s);
        }
        if (do_step) {
            int o;
            double r, unused_prob;
            uint32_t unused_entry;
            const bool term = ca_hist_step<false>(P, g, T, StridedEntries<SEARCH_BLOCK>{stage + (size_t)(2 + hist_offset(hist_cnt, a)) * SEARCH_BLOCK},
                                                  hist_count(hist_cnt, a), s, a, o, r, unused_entry, 0, unused_prob);
            ++steps;
            if (mode == 1) {  // traverseChanceNode
                path_r[(size_t)plen * SEARCH_BLOCK]  = (float)r;
                path_na[(size_t)plen * SEARCH_BLOCK] = (node << 5) | a;
                ++plen;
                if (term) finish = true;
                else {
                    const int c = child_get(P, D, tree, tab, epoch, node, a, o);
                    if (c >= 0) { node = c; --dtg; }
                    else {  // expand: new leaf, then rollout(depth_to_go - 1); never past the slot's records (search_kernel)
                        const int nn = min(n_nodes, D.max_nodes - 1);
                        ++n_nodes;
                        node_init(D, tree + (size_t)nn * W, P.A, P.O);
                        child_set(P, D, tree, tab, epoch, node, a, o, nn);
                        mode = 2; rdepth = dtg - 1; rret = 0; rdisc = 1;
                        if (rdepth == 0) finish = true;
                    }
                }
            } else {
                rret += r * rdisc;
                rdisc *= P.gamma;
                --rdepth;
                if (rdepth == 0 || term) { delayed = rret; finish = true; }
            }
        }
        if (finish) {
            // back-up, leaf to root: ret = r + gamma * delayed; ChanceNode::addVisit(ret), ActionNode::addVisit() (search_kernel)
            double del = delayed;
            for (int k = plen - 1; k >= 1; --k) {
                const int na     = path_na[(size_t)k * SEARCH_BLOCK];
                const double ret = (double)path_r[(size_t)k * SEARCH_BLOCK] + P.gamma * del;
                const int act    = na & 31;
                int32_t* rec = tree + (size_t)(na >> 5) * W;
                double* q    = reinterpret_cast<double*>(rec + D.cq_off) + act;
                const int nv = ++rec[D.cn_off + act];
                if (D.cn_off) ++rec[0];
                *q += (ret - *q) / (double)nv;
                del = ret;
            }
            if (plen > 0) {
                const double ret = (double)path_r[0] + P.gamma * del;
                const int act    = path_na[0] & 31;
                int nv = 0;
                double q = 0.0;
#pragma unroll
                for (int a2 = 0; a2 < AMAX; ++a2)
                    if (a2 == act) { nv = r_cn[a2]; q = r_cq[a2]; }
                ++nv;
                q += (ret - q) / (double)nv;
#pragma unroll
                for (int a2 = 0; a2 < AMAX; ++a2)
                    if (a2 == act) { r_cn[a2] = nv; r_cq[a2] = q; }
                ++r_vis;
            }
            ++sim;
            mode = 0;
        }
    }
    g.stream(FBA_PHASE_SEARCH, (uint32_t)P.sims + 1u);
    if (n_nodes > D.max_nodes) atomicCAS(D.fault, 0, -(1 + e));  // -> FBA_ESTATE on the host
    const int best = ucb_pick<AMAX>(P, g, D.log1p_tab, 0, r_cn, r_cq, false);
    D.action[e]    = best;
    D.sim_steps[e] += steps;
    fba_trace_rec& rec = D.cur[e];
    rec.n_nodes    = n_nodes;
    rec.tree_depth = tree_depth;
#pragma unroll
    for (int a = 0; a < FBA_MAX_ACTIONS; ++a) {
        rec.root_n[a] = a < AMAX && a < P.A ? r_cn[a < AMAX ? a : 0] : 0;
        rec.root_q[a] = a < AMAX && a < P.A ? r_cq[a < AMAX ? a : 0] : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------
// host launcher
// ---------------------------------------------------------------------------------------------
// Which instantiation, with what block, grid and LDS, is search_plan's decision (fba_launch_plan.h); here every instantiation stands once, behind
// its key -- spelled from the same template arguments -- and is launched the same way
void launch_search(const Problem& P, const DeviceState& D0, hipStream_t st)
{
    const SearchPlan pl = search_plan(P, D0);
    DeviceState D = D0;
    D.search_quorum = (int8_t)pl.quorum;   // (the kernel's copy names the value itself, never "the default")
    static const size_t lds_pad = std::getenv("FBA_SEARCH_LDS_PAD") ? (size_t)std::atoi(std::getenv("FBA_SEARCH_LDS_PAD")) : 0;  // occupancy experiments
    const size_t lds = pl.lds + (kernel_name(pl.kernel) == K_SEARCH ? lds_pad : 0);
    const dim3 grid(pl.grid(P.E)), block(pl.block);
    if (pl.order_first) hipLaunchKernelGGL(search_order_kernel, dim3(1), dim3(1024), 0, st, P, D);
#define FBA_LAUNCH(...)                                                                                                                     \
    {                                                                                                                                       \
        if (pl.raise_lds) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&__VA_ARGS__), hipFuncAttributeMaxDynamicSharedMemorySize, pl.raise_lds); \
        hipLaunchKernelGGL((__VA_ARGS__), grid, block, lds, st, P, D);                                                                      \
        return;                                                                                                                             \
    }
#define FBA_SEARCH(...) case search_key(__VA_ARGS__): FBA_LAUNCH(search_kernel<__VA_ARGS__>)
#define FBA_HIST_SEARCH(NAME, KERNEL, ...) case kernel_key(NAME, __VA_ARGS__): FBA_LAUNCH(KERNEL<__VA_ARGS__>)
    switch (pl.kernel) {
        FBA_HIST_SEARCH(K_SEARCH_CA_HIST, search_ca_hist_kernel, 4)
        FBA_HIST_SEARCH(K_SEARCH_TABHIST, search_tabhist_kernel, true)
        FBA_HIST_SEARCH(K_SEARCH_TABHIST, search_tabhist_kernel, false)
        FBA_HIST_SEARCH(K_HIST2_FLAT_SEARCH, hist2_flat_search, 8, true)
        FBA_HIST_SEARCH(K_HIST2_FLAT_SEARCH, hist2_flat_search, 8, false)
        FBA_HIST_SEARCH(K_HIST2_FLAT_SEARCH, hist2_flat_search, 12, true)
        FBA_HIST_SEARCH(K_HIST2_FLAT_SEARCH, hist2_flat_search, 12, false)
        FBA_HIST_SEARCH(K_HIST2_FLAT_SEARCH, hist2_flat_search, 16, true)
        FBA_HIST_SEARCH(K_HIST2_FLAT_SEARCH, hist2_flat_search, 16, false)
        FBA_HIST_SEARCH(K_SEARCH_HIST2, search_hist2_kernel, 8, true)
        FBA_HIST_SEARCH(K_SEARCH_HIST2, search_hist2_kernel, 8, false)
        FBA_HIST_SEARCH(K_SEARCH_HIST2, search_hist2_kernel, 12, true)
        FBA_HIST_SEARCH(K_SEARCH_HIST2, search_hist2_kernel, 12, false)
        FBA_HIST_SEARCH(K_SEARCH_HIST2, search_hist2_kernel, 16, true)
        FBA_HIST_SEARCH(K_SEARCH_HIST2, search_hist2_kernel, 16, false)
        FBA_HIST_SEARCH(K_SEARCH_HIST, search_hist_kernel, 8)
        FBA_HIST_SEARCH(K_SEARCH_HIST, search_hist_kernel, 12)
        FBA_HIST_SEARCH(K_SEARCH_HIST, search_hist_kernel, 16)
        // the tabular tiger BA-POMDP: dense / packed records, general / ETIGER tree layout; planning on tiger itself
        FBA_SEARCH(true, 4, false, 2, FBA_MODEL_BA_TABLE, 0, false, false, true)
        FBA_SEARCH(true, 4, false, 2, FBA_MODEL_BA_TABLE, 0, false, false, false)
        FBA_SEARCH(true, 4, false, 1, FBA_MODEL_BA_TABLE, 0, false, false, true)
        FBA_SEARCH(true, 4, false, 1, FBA_MODEL_BA_TABLE, 0, false, false, false)
        FBA_SEARCH(false, 4, false, 0, FBA_MODEL_POMDP, 0, true, false, true)
        FBA_SEARCH(false, 4, false, 0, FBA_MODEL_POMDP, 0, true, false, false)
        // factored tiger with FS state features: packed on the ETIGER / the general layout, dense staged / unstaged
        FBA_SEARCH(true, 4, false, 0, FBA_MODEL_BA_FACTORED, 2, false, true, true)
        FBA_SEARCH(true, 4, false, 0, FBA_MODEL_BA_FACTORED, 2, false, true, false)
        FBA_SEARCH(true, 4, false, 0, FBA_MODEL_BA_FACTORED, 2)
        FBA_SEARCH(false, 4, false, 0, FBA_MODEL_BA_FACTORED, 2)
        FBA_SEARCH(true, 4, false, 0, FBA_MODEL_BA_FACTORED, 3, false, true, true)
        FBA_SEARCH(true, 4, false, 0, FBA_MODEL_BA_FACTORED, 3, false, true, false)
        FBA_SEARCH(true, 4, false, 0, FBA_MODEL_BA_FACTORED, 3)
        FBA_SEARCH(false, 4, false, 0, FBA_MODEL_BA_FACTORED, 3)
        FBA_SEARCH(true, 4, false, 0, FBA_MODEL_BA_FACTORED, 4, false, true, true)
        FBA_SEARCH(true, 4, false, 0, FBA_MODEL_BA_FACTORED, 4, false, true, false)
        FBA_SEARCH(true, 4, false, 0, FBA_MODEL_BA_FACTORED, 4)
        FBA_SEARCH(false, 4, false, 0, FBA_MODEL_BA_FACTORED, 4)
        // every other model, by action count: staged or not, regular or expected Dirichlet
        FBA_SEARCH(true, 4, true, 0, FBA_MODEL_BA_FACTORED)
        FBA_SEARCH(true, 4, false, 0, FBA_MODEL_BA_FACTORED)
        FBA_SEARCH(true, 4, true, 0, FBA_MODEL_BA_TABLE)
        FBA_SEARCH(true, 4, false, 0, FBA_MODEL_BA_TABLE)
        FBA_SEARCH(false, 4, true, 0, FBA_MODEL_BA_FACTORED)
        FBA_SEARCH(false, 4, false, 0, FBA_MODEL_BA_FACTORED)
        FBA_SEARCH(false, 4, true, 0, FBA_MODEL_BA_TABLE)
        FBA_SEARCH(false, 4, false, 0, FBA_MODEL_BA_TABLE)
        FBA_SEARCH(false, 4, false, 0, FBA_MODEL_POMDP)
        FBA_SEARCH(true, 8, true, 0, FBA_MODEL_BA_FACTORED)
        FBA_SEARCH(true, 8, false, 0, FBA_MODEL_BA_FACTORED)
        FBA_SEARCH(true, 8, true, 0, FBA_MODEL_BA_TABLE)
        FBA_SEARCH(true, 8, false, 0, FBA_MODEL_BA_TABLE)
        FBA_SEARCH(false, 8, true, 0, FBA_MODEL_BA_FACTORED)
        FBA_SEARCH(false, 8, false, 0, FBA_MODEL_BA_FACTORED)
        FBA_SEARCH(false, 8, true, 0, FBA_MODEL_BA_TABLE)
        FBA_SEARCH(false, 8, false, 0, FBA_MODEL_BA_TABLE)
        FBA_SEARCH(false, 8, false, 0, FBA_MODEL_POMDP)
        FBA_SEARCH(true, 16, true, 0, FBA_MODEL_BA_FACTORED)
        FBA_SEARCH(true, 16, false, 0, FBA_MODEL_BA_FACTORED)
        FBA_SEARCH(true, 16, true, 0, FBA_MODEL_BA_TABLE)
        FBA_SEARCH(true, 16, false, 0, FBA_MODEL_BA_TABLE)
        FBA_SEARCH(false, 16, true, 0, FBA_MODEL_BA_FACTORED)
        FBA_SEARCH(false, 16, false, 0, FBA_MODEL_BA_FACTORED)
        FBA_SEARCH(false, 16, true, 0, FBA_MODEL_BA_TABLE)
        FBA_SEARCH(false, 16, false, 0, FBA_MODEL_BA_TABLE)
        FBA_SEARCH(false, 16, false, 0, FBA_MODEL_POMDP)
        FBA_SEARCH(false, 24, false, 0, FBA_MODEL_POMDP)
    }
#undef FBA_HIST_SEARCH
#undef FBA_SEARCH
#undef FBA_LAUNCH
    std::fprintf(stderr, "launch_search: no instantiation behind kernel key %#x\n", pl.kernel);   // (search_plan names one this switch lacks)
    std::abort();
}
#ifdef FBA_PROFILE_SEARCH
extern "C" int fba_debug_search_profile(unsigned long long* out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_search_prof), sizeof(unsigned long long) * 12) != hipSuccess) return -1;   // (out: 12 entries)
    if (reset) {
        const unsigned long long z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_search_prof), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#endif

}  // namespace fba
