/*
 * include/fba_hip.h -- C-ABI of libfba_hip.so, the MI355X-native BA-POMCP engine.
 *
 * This is the drop-in boundary for the reference's hot path.  samkatt/fba-pomdp has no FFI of
 * its own: its boundary is a set of C++ abstract classes + string-keyed factories
 * (SURVEY.md section 8b).  Each entry point below names the reference interface it replaces;
 * INTEGRATION.md shows the C++ adapter classes (fba_pomdp_amd/csrc/host/adapters.hpp) a
 * maintainer registers in those factories.
 *
 * Conventions: every function returns 0 on success or a negative FBA_E* code;
 * fba_last_error() gives the message (the adapters re-throw it as std::string, which the
 * reference's main()s already catch: src/planning.cpp:46-54).  The caller owns every host
 * buffer; the ctx owns all device memory.  One ctx <-> one host thread <-> one HIP stream.
 *
 * A ctx holds `slots` independent (planner, belief) pairs that advance in lock-step on the
 * device; slots = 1 is exactly one reference Planner + Belief.  All per-slot array arguments
 * have length `slots`.
 */
#ifndef FBA_HIP_H
#define FBA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FBA_ABI_VERSION 3   /* 3: fba_config.tree_buckets; 2: fba_config.belief_option and .search_budget, fba_belief_get_particle, fba_get_trace_hist; hosts check fba_abi_version() == FBA_ABI_VERSION before fba_create */
#define FBA_MAX_ACTIONS 24

/* domains: reference src/domains, selected by -D (DomainConf.hpp) */
enum {
    FBA_DOM_TIGER_EPISODIC    = 0, /* episodic-tiger             src/domains/tiger/Tiger.cpp          */
    FBA_DOM_TIGER_CONTINUOUS  = 1, /* continuous-tiger                                                */
    FBA_DOM_FTIGER_EPISODIC   = 2, /* episodic-factored-tiger    src/domains/tiger/FactoredTiger.cpp  */
    FBA_DOM_FTIGER_CONTINUOUS = 3, /* continuous-factored-tiger                                       */
    FBA_DOM_GRIDWORLD         = 4, /* gridworld                  src/domains/gridworld/GridWorld.cpp  */
    FBA_DOM_COLLISION_AVOID   = 5, /* random-collision-avoidance src/domains/collision-avoidance/CollisionAvoidance.cpp */
    FBA_DOM_COLLISION_AVOID_CENTERED = 6, /* centered-collision-avoidance (VERSION INITIALIZE_CENTRE) */
    FBA_DOM_SYSADMIN_INDEPENDENT = 7, /* independent-sysadmin --size N  src/domains/sysadmin/SysAdmin.cpp */
    FBA_DOM_SYSADMIN_LINEAR      = 8, /* linear-sysadmin --size N                                         */
    FBA_DOM_COFFEE               = 9, /* coffee            src/domains/coffee/CoffeeProblem.cpp (planning only) */
    FBA_DOM_COFFEE_BOUTILIER     = 10, /* boutilier-coffee  (the version with acquiring / losing coffee switched off) */
    FBA_DOM_AGR                  = 11  /* agr               src/domains/agr/AGR.cpp, AGR(10): planning with rejection sampling only */
};
/* simulator: plain POMDP (planning), tabular BA-POMDP (bapomdp), factored (fbapomdp) */
enum { FBA_MODEL_POMDP = 0, FBA_MODEL_BA_TABLE = 1, FBA_MODEL_BA_FACTORED = 2 };
/* -B rejection_sampling | importance_sampling (BeliefConf.hpp, Belief.cpp:13-24) | reinvigoration
 * (BABelief.cpp:28-31: ReinvigoratingRejectionSampling, factored models only) */
enum { FBA_BELIEF_REJECTION = 0, FBA_BELIEF_IMPORTANCE = 1, FBA_BELIEF_REINVIGORATION = 2,
       FBA_BELIEF_CHEATING = 3, /* cheating-reinvigoration (BABelief.cpp:60-65: prototypes::CheatingReinvigoration) */
       FBA_BELIEF_POINT = 4, /* point_estimate (Belief.cpp:13-14 PointEstimation, BABelief.cpp:19-20 BAPointEstimation): one state,
                             * updated by rejection; `particles` is ignored (1) and sample() draws nothing */
       FBA_BELIEF_MH_GIBBS = 5, /* mh-within-gibbs (BABelief.cpp:37-47: factored::MHwithinGibbs; `belief_option` 1 = "rs"): importance
                                 * filter whose particles are re-drawn by a Metropolis-Hastings chain over structures when the log
                                 * likelihood falls below `threshold`; factored tiger, collision avoidance, gridworld, sysadmin */
       FBA_BELIEF_MH_NIPS = 6,  /* mh-nips (BABelief.cpp:33-36: factored::MHNIPS2018): the same filter and trigger; the re-draw makes
                                 * independent proposals (a particle's structure or a mutation, updated along a simulated history) */
       FBA_BELIEF_INCUBATOR = 8, /* incubator (BABelief.cpp:53-58: factored::StructureIncubatorSampling(particles, resample_amount, threshold)): the
                                  * reinvigoration belief's two rejection filters + a weighted shadow filter of bred particles
                                  * (fba_belief_get_shadow), importance-sampled; factored tiger, collision avoidance, sysadmin */
       FBA_BELIEF_NESTED = 7    /* nested (BABelief.cpp:67-70: NestedBelief(particles, particles^2)): a weighted filter of count particles,
                                 * each with its own flat filter of particles^2 domain states (fba_belief_get_nested); bapomdp / fbapomdp */ };
/* -P po-uct | random | ts (Planner.cpp:12-19, BAPlanner.cpp:13-20; ts = Thompson sampling: TSPlanner / BATSPlanner) */
enum { FBA_PLANNER_POUCT = 0, FBA_PLANNER_RANDOM = 1, FBA_PLANNER_TS = 2 };
/* --structure-prior (FBAConf.hpp) */
enum { FBA_SP_NONE = 0, FBA_SP_UNIFORM = 1, FBA_SP_MATCH_UNIFORM = 2, FBA_SP_FULLY_CONNECTED = 3 };

/* Philox stream phases: a draw is addressed by (seed, run, episode, t, phase, unit, draw#) */
enum {
    FBA_PHASE_INIT      = 0,
    FBA_PHASE_RESET     = 1,
    FBA_PHASE_START     = 2,
    FBA_PHASE_SEARCH    = 3,
    FBA_PHASE_ENV       = 4,
    FBA_PHASE_REJECT    = 5,
    FBA_PHASE_IS_UPDATE = 6,
    FBA_PHASE_RESAMPLE  = 7,
    FBA_PHASE_REINVIG   = 8,  /* reinvigoration: unit = index of the bred particle            */
    FBA_PHASE_INIT_FC   = 9,  /* fully connected filter of the reinvigoration belief: initiate */
    FBA_PHASE_RESET_FC  = 10, /*   ... resetDomainStateDistribution                            */
    FBA_PHASE_REJECT_FC = 11, /*   ... rejection sampling, unit = attempt index                */
    FBA_PHASE_RESET_SH  = 12, /* incubator belief, shadow filter: resetDomainStateDistribution     */
    FBA_PHASE_INIT_SH   = 13, /*   ... initiate, unit = index of the bred particle                 */
    FBA_PHASE_CONVERT   = 14  /* fba_belief_convert: run = first_run + block, episode 0, t 0, unit = index of the particle written */
};

enum {
    FBA_OK        = 0,
    FBA_EINVAL    = -1, /* bad argument / unsupported configuration (reference: throw "...") */
    FBA_EHIP      = -2, /* HIP runtime error                                                  */
    FBA_ENODEVICE = -3, /* no gfx950 device visible: the engine never falls back to the CPU   */
    FBA_ESTATE    = -4  /* call order violated (e.g. select_action before belief_init)        */
};

/* Flag names and defaults follow the reference CLI (Conf.hpp:14-45, PlannerConf.hpp:16-18,
 * BeliefConf.hpp:16-21, BAConf.hpp:17-22, FBAConf.hpp).  fba_default_config() fills them. */
typedef struct fba_config {
    int32_t domain;          /* -D                                  */
    int32_t size;            /* --size                              */
    int32_t width;           /* --width                             */
    int32_t height;          /* --height                            */
    int32_t model;           /* which executable: planning / bapomdp / fbapomdp */
    int32_t belief;          /* -B                                  */
    int32_t planner;         /* -P                                  */
    int32_t particles;       /* --particle-amount        (100)      */
    int32_t sims;            /* -s / --num-sims          (1000)     */
    int32_t max_depth;       /* --mcts-max-depth   (-1 => horizon)  */
    int32_t horizon;         /* -H                       (10)       */
    double exploration;      /* -u                       (100)      */
    double discount;         /* -d                       (0.95)     */
    int32_t runs;            /* --runs                   (1)        */
    int32_t episodes;        /* --episodes               (1)        */
    float noise;             /* --noise                  (0)        */
    float counts_total;      /* -C                       (10000)    */
    int32_t structure_prior; /* --structure-prior                   */
    uint64_t seed;           /* --seed (Philox key)                 */
    int32_t run_offset;      /* global index of this ctx's first run (episode sharding)      */
    int32_t slots;           /* concurrent runs on the device; 0 => min(runs, auto)          */
    int32_t device;          /* HIP device ordinal                                           */
    int32_t trace;           /* 1 => record one fba_trace_rec per real time-step; 2 => also the filter's state histogram
                              * after every belief update (domains of at most FBA_TRACE_HIST_BINS states): fba_get_trace_hist */
    int32_t dirichlet_regular; /* --dirichlet_sampling_method regular (0 = expected, default);
                                * bug-compatible with the reference's biased sampler (BAConf.hpp:22,
                                * random.cpp:146-242) */
    int32_t resample_amount; /* --resample-amount: particles bred per update by the reinvigoration
                              * belief / copied per cheat by the cheating belief (BeliefConf.cpp:17-21) */
    double threshold;        /* --threshold: log likelihood below which the cheating belief cheats (< 0) */
    int32_t belief_option;   /* --belief-option: mh-within-gibbs 0 = state histories by message passing (default), 1 = "rs" */
    int32_t search_budget;   /* history-particle searches (gridworld FBA-POMDP, fba_particle_bytes): iterations of the search loop per launch.
                              * 0 = a launch runs every slot's whole search (lock-step ticks: a tick lasts as long as its deepest tree);
                              * > 0 = a launch stops at the first simulation boundary behind that many iterations, unfinished searches
                              * are parked in their trees and resumed by the next launch, and slots whose search is done take their
                              * real step and belief update meanwhile -- slots advance on their own, results are the same
                              * (Episode.cpp:39-55 and BAPOMDPExperiment.cpp:44-75 never couple two runs) */
    int32_t tree_buckets;    /* history-particle searches: 64-byte node buckets per slot's tree (the reference's tree is heap-allocated and
                              * unbounded: MCTSTreeNodes.hpp:39-108).  0 = 2 * (sims + 2), which no search can fill -- 8.4 MB per slot at 65 536
                              * simulations.  A gridworld tree gives a bucket only to the nodes it reaches a second time (a quarter of them at
                              * the BASELINE size), so a throughput run that wants more slots per GB passes less here; a search that does outgrow
                              * its table stops with FBA_ESTATE and a message, never with a wrong result */
} fba_config;

/* One record per real time-step: the information the reference prints at -v 2 / -v 3
 * (Episode.cpp:44-45, POUCT.cpp:93-101, RejectionSampling.hpp:68) plus a belief checksum. */
typedef struct fba_trace_rec {
    int32_t run, episode, t;
    int32_t action, state, obs;
    int32_t terminal;
    int32_t n_nodes, tree_depth;
    int32_t update_count;    /* attempts of the step's rejection update; -1: none (terminal step); FBA_UPDATE_GAVE_UP: see fba_giveup_policy */
    int32_t root_n[FBA_MAX_ACTIONS];
    double root_q[FBA_MAX_ACTIONS];
    double reward;
    double weight_total;
    uint64_t belief_hash;
} fba_trace_rec;
#define FBA_UPDATE_GAVE_UP (-2)   /* fba_trace_rec.update_count of the step at which a run was retired (fba_giveup_policy) */

/* utils::Statistic (src/utils/Statistic.cpp:5-46) */
typedef struct fba_stat {
    double count, mean, m2;
} fba_stat;

typedef struct fba_counters {
    uint64_t sim_steps;    /* simulator.step calls made by the planner (tree + rollout) */
    uint64_t belief_steps; /* simulator.step calls made by the belief update            */
    uint64_t env_steps;    /* true-environment steps                                     */
} fba_counters;

/* kernels the engine times with HIP events on its own stream (bench.py roofline) */
enum {
    FBA_K_SEARCH       = 0,
    FBA_K_ENV          = 1,
    FBA_K_BELIEF_RS    = 2, /* rejection update: sample, step, compact, gather */
    FBA_K_BELIEF_IS    = 3, /* importance update + scan + resample gather      */
    FBA_K_BELIEF_RESET = 4,
    FBA_K_BELIEF_INIT  = 5,
    FBA_K_COUNT        = 6
};
typedef struct fba_kernel_time {
    double ms;          /* sum of HIP-event durations */
    uint64_t launches;
    uint64_t units;     /* particles written (belief kernels) / simulated steps (search) */
    uint64_t bytes;     /* algorithmic bytes, SURVEY.md section 8(d) formulas.  History records have formulas of their own
                         * (DESIGN.md section 5a); collision-avoidance records under the importance filter:
                         * particles * 100 + entries * 12 (weights, prefix sums and side rows 72, the record's 8-byte header
                         * read twice and written once with the new entry 28, every older 4-byte entry moved three times) */
} fba_kernel_time;

typedef struct fba_ctx fba_ctx;

int fba_abi_version(void);
void fba_default_config(fba_config* cfg);

/* Construction.  Replaces the factory calls of experiment::planning::run /
 * experiment::bapomdp::run (PlanningExperiment.cpp:31-36, BAPOMDPExperiment.cpp:36-42):
 * makePlanner / makeBAPlanner, makeBelief / makeBABelief, makePOMDP / makeTBAPOMDP / makeFBAPOMDP. */
int fba_create(const fba_config* cfg, fba_ctx** out);
void fba_destroy(fba_ctx* ctx);
const char* fba_last_error(const fba_ctx* ctx); /* ctx may be NULL: last create error */

int fba_domain_sizes(const fba_ctx* ctx, int32_t* S, int32_t* A, int32_t* O);
int fba_counts_len(const fba_ctx* ctx); /* floats per particle count blob (0 for plain POMDP) */
int fba_particle_bytes(const fba_ctx* ctx); /* HBM bytes of one particle record.  Tabular tiger particles are stored packed
                                             * (uint16 increment counts over the shared prior, 64 B instead of 128 B) when the
                                             * prior allows it exactly.  Gridworld FBA-POMDP particles are stored as histories of
                                             * their own steps over the shared prior (8 B + 4 B per real step instead of 191 KB at
                                             * --size 7) under the importance filter, and under the plain rejection filter where
                                             * the planner is po-uct or random with at most 65 536 simulations.  The tabular gridworld
                                             * BA-POMDP stores them the same way (8 B + 4 B per real step instead of 7.68 MB at
                                             * --size 7) under both filters where the planner is po-uct or random with at most 65 536
                                             * simulations.  The collision-avoidance FBA-POMDP without a structure prior stores them too
                                             * under the plain importance filter above 65 536 particles, where the filter is the multi-launch one (smaller filters stay dense; 8 B + 4 B per real step instead of
                                             * 3.5 KB at 7 x 7 with two obstacles), for po-uct or random, width and height <= 8, at most
                                             * two obstacles, episodes * horizon <= 126, a search whose LDS (prior tables, 512 B per level of
                                             * max_depth, 256 B per record word) fits 64 KB, and a prior with at most 8 distinct counts c for
                                             * which c + j is inexact in fp32.  Such contexts refuse fba_belief_set of states or counts.  FBA_DENSE_PARTICLES=1 in the environment forces
                                             * fp32 counts.  fba_belief_get / fba_belief_set always speak fp32 counts. */
int fba_slots(const fba_ctx* ctx);      /* slots actually resident (cfg.slots, or the library's choice) */

/* The device arrays the context holds for its slots, filters, composite beliefs, search trees and -- once an experiment has been
 * started -- its per-run returns and trace, and from fba_giveup_policy on the list of retired runs ("retired"), in allocation order: what a context of this configuration takes in HBM (the sum of
 * elems * elem_bytes; the prior's tables and the probe, a few kilobytes to megabytes, are not listed) and where one slot's part of an
 * array stands.  A per-slot array is `buffers` buffers of fba_slots slots of slot_elems
 * elements each: the part of slot e in buffer b starts at element (b * fba_slots + e) * slot_elems.  History records keep one buffer
 * (buffers = 1) with the scratch places' records behind the slots', so elems exceeds buffers * fba_slots * slot_elems there; which
 * record buffer is whose changes while the context runs.  Arrays a configuration does not use are absent or one element long.  Host
 * bookkeeping only: nothing is launched or copied.  Writes min(cap, n) entries to out (NULL with cap = 0) and returns n, the number of
 * arrays, which grows when an experiment allocates its returns and trace. */
typedef struct fba_array_info {
    char     name[32];     /* the member of the engine's device state that holds the array: "p_rec", "nodes", "bkt", ... */
    uint64_t elem_bytes;   /* bytes of one element                                                                       */
    uint64_t elems;        /* elements allocated                                                                         */
    uint64_t slot_elems;   /* elements one slot takes in one buffer; 0: the array is not laid out by slot                */
    int32_t  buffers;      /* buffers of fba_slots slots each                                                            */
    int32_t  reserved;
} fba_array_info;
int fba_device_arrays(const fba_ctx* ctx, fba_array_info* out, int32_t cap);

/* Prior count tables.  fba_create builds the domain's own prior (TigerPriors.cpp:14-43,
 * FactoredTigerPriors.cpp:18-88); this call overrides it with tables built by the caller
 * (BAFlatModel layout: phi[s*A*S + a*S + s'], psi[a*S*O + s'*O + o]).  Takes effect at the next
 * fba_belief_init (the prior is what initiate copies into the particles); where particles are stored packed
 * (fba_particle_bytes) that call is required before the belief is used again. */
int fba_set_model_tabular(fba_ctx* ctx, const float* phi, const float* psi);
int fba_get_prior(const fba_ctx* ctx, float* counts);

/* Layout of a factored particle's count blob (model = FBA_MODEL_BA_FACTORED), for hosts that read or
 * write particles with fba_belief_get / fba_belief_set -- what BABNModel + DBNNode hold per state
 * (BABNModel.hpp:30-200, DBNNode.hpp:20-120), flattened:
 *   blob = n_counts floats of CPTs, then n_mask_words words (uint32 bit patterns stored in float slots).
 *   node k: T(a, f) = node[a * n_state_features + f], O(a, f) = node[A * n_state_features + a * n_obs_features + f].
 *   A node owns room for EVERY candidate parent set ("max layout"); the parents in use are the candidates j
 *   whose bit j is set in the particle's mask word `mask_word` (or in `fixed_mask` when mask_word < 0).
 *   Row of parent values v: idx = 0; for j in candidate order, if bit j set: idx = idx * candidate_size[j] + v[candidate[j]];
 *   the row starts at blob[offset + idx * out] and has `out` counts (DBNNode::cptIndex, last parent fastest).
 *   Parent values are features of the PREVIOUS state for T nodes and of the NEW state for O nodes; a state index
 *   is its features in mixed radix, last feature fastest (indexing::project, utils/index.cpp:51-83). */
#define FBA_MAX_FEATURES 8
#define FBA_MAX_NODES 160
typedef struct fba_factored_node {
    int32_t offset, out, n_candidates, mask_word;
    uint32_t fixed_mask;
    uint8_t candidate[FBA_MAX_FEATURES];      /* state-feature ids, in order */
    uint8_t candidate_size[FBA_MAX_FEATURES]; /* number of values of each candidate */
} fba_factored_node;
typedef struct fba_factored_layout {
    int32_t n_state_features, n_obs_features, n_nodes, n_counts, n_mask_words;
    int32_t state_feature_size[FBA_MAX_FEATURES], obs_feature_size[FBA_MAX_FEATURES];
    fba_factored_node node[FBA_MAX_NODES];
} fba_factored_layout;
int fba_get_factored_layout(const fba_ctx* ctx, fba_factored_layout* out);
/* The factored counterpart of fba_set_model_tabular: replaces the base prior every particle starts from with CPTs built
 * by the caller -- what FBAPOMDPPrior::sample copies into a new FBAPOMDPState (FBAPOMDPPrior.cpp:27-37: the prior's
 * BABNModel, node by node, DBNNode::count order).  `layout` must be the engine's own (fba_get_factored_layout: the host
 * walks it to know where node (a, f)'s rows go); `counts` = n_counts floats followed by n_mask_words parent-set words,
 * exactly a particle's blob.  Per-particle structure draws of the configured structure prior still apply on top.  Takes
 * effect at the next fba_belief_init, which is required before the belief is used again. */
int fba_set_model_factored(fba_ctx* ctx, const fba_factored_layout* layout, const float* counts);

/* ---- per-step interface: one call per reference virtual call -------------------------- */

/* Where each slot is in its experiment; addresses the Philox streams of the calls below. */
int fba_set_position(fba_ctx* ctx, const int32_t* run, const int32_t* episode, const int32_t* t);

/* Belief::initiate(POMDP const&)                       src/beliefs/Belief.hpp:25          */
int fba_belief_init(fba_ctx* ctx);
/* BABelief::resetDomainStateDistribution(BAPOMDP const&) src/beliefs/bayes-adaptive/BABelief.hpp:34 */
int fba_belief_reset_domain_state(fba_ctx* ctx);
/* Planner::selectAction(POMDP const&, Belief const&, History const&)  src/planners/Planner.hpp:23-24
 * hist_len[slot] = History::length(); action[slot] <- chosen action index.
 * active may be NULL (all slots) */
int fba_select_action(fba_ctx* ctx, const int32_t* hist_len, const uint8_t* active, int32_t* action);
/* Belief::updateEstimation(Action const*, Observation const*, POMDP const&)  Belief.hpp:40 */
int fba_belief_update(fba_ctx* ctx, const int32_t* action, const int32_t* obs, const uint8_t* active);
/* Belief::sample() for a host-side planner, and bulk download for tests:
 * state[particles], weight[particles] (may be NULL), counts[particles * counts_len] (may be NULL) */
int fba_belief_get(fba_ctx* ctx, int32_t slot, int32_t* state, double* weight, float* counts);
int fba_belief_set(fba_ctx* ctx, int32_t slot, const int32_t* state, const double* weight, const float* counts);
/* One particle of the filter -- what Belief::sample() (Belief.hpp:33) hands a HOST-side planner once the host has drawn the
 * index (FlatFilter::sample FlatFilter.cpp:97-102: uniform; WeightedFilter::sample WeightedFilter.cpp:163-191: by weight):
 * state[1], weight[1] (may be NULL; importance filters only), counts[counts_len] (may be NULL).  The adapters build the
 * BAPOMDPState / FBAPOMDPState a reference planner borrows from it (RBAPOUCT.cpp:89-107). */
int fba_belief_get_particle(fba_ctx* ctx, int32_t slot, int32_t index, int32_t* state, double* weight, float* counts);
/* the second filter of the reinvigoration belief (ReinvigoratingRejectionSampling.hpp:
 * _fully_connected_belief) or of the cheating belief (CheatingReinvigoration.hpp:
 * _correct_structured_belief), for tests */
int fba_belief_get_fully_connected(fba_ctx* ctx, int32_t slot, int32_t* state, float* counts);
/* the nested belief's flat filters of domain states (NestedBelief.hpp: the FlatFilter<State const*> of every top
 * particle): states[particles][particles^2]; fba_belief_get returns the count particles and their weights */
int fba_belief_get_nested(fba_ctx* ctx, int32_t slot, int32_t* states);
/* the incubator belief's shadow filter (StructureIncubatorSampling.hpp: _shadow_belief), for tests */
int fba_belief_get_shadow(fba_ctx* ctx, int32_t slot, int32_t* state, double* weight, float* counts);
/* Posterior summary of slots [first, first + count), reduced on the device from whatever record format the context stores
 * (fba_particle_bytes) -- no particle's count table is built, on the device or on the host.  Any output pointer may be NULL.
 *   head       [count]
 *   state_mass [count][S]              sum of w_i over the particles whose domain state is s
 *   mean_counts[count][fba_counts_len] sum_i w_i * c_i[k] / weight_total, where c_i is the fp32 table fba_belief_get returns
 *                                      for particle i.  Entries at the mask-word positions of a factored blob (k >= n_counts) are 0.0.
 *   edge_prob  [count][n_mask_words][FBA_MAX_FEATURES]
 *                                      weighted fraction of particles whose mask word m has bit j set; 0.0 for j >= 32 or unused.
 * Serves the main filter of every belief but the nested one (FBA_EINVAL there: its particles are pairs, fba_belief_get_nested), not
 * the second or shadow filters; a plain POMDP context has head and state_mass only.  Read-only: no buffer, flag, counter or Philox
 * position of the context changes, so the call may stand between any two others, after fba_run_*, and on inactive slots.
 * The call is OUTSIDE the parity contract: the order of its fp64 additions is the engine's choice and need not repeat bit for bit
 * from call to call; nothing of it enters the trace or belief_hash.  Every entry is within 8 * particles * 2^-53 relative of the
 * exact sum, and exactly 0.0 where every term is.  Cells of a factored node compare across particles only where the particles share
 * that node's parent set: edge_prob of 0 or 1 says where that is so. */
typedef struct fba_belief_summary_head {
    double  weight_total;     /* sum of w_i; a flat (rejection) filter counts every particle with w_i = 1.0, so this is N exactly */
    double  weight_sq_total;  /* sum of w_i^2 (effective sample size = weight_total^2 / weight_sq_total)                           */
    int32_t particles;        /* N                                                                                                */
    int32_t weighted;         /* 1: importance filter, 0: flat filter                                                             */
} fba_belief_summary_head;
int fba_belief_summary(fba_ctx* ctx, int32_t first, int32_t count, fba_belief_summary_head* head,
                       double* state_mass, double* mean_counts, double* edge_prob);
/* Posterior-predictive model queries on the device: under the posterior of each slot in [first, first + count), what happens when action[q]
 * is taken in state[q], and how probable is the transition to next_state[q] under observation obs[q]?  The nq queries (1 to 2^24) are shared
 * by the slots.  With c_i the fp32 table fba_belief_get returns for particle i, w_i its weight (1.0 in a flat filter), W = sum w_i and
 * theta_i(row)[k] = c_i[row + k] / sum_k c_i[row + k] in fp64 (a row whose counts sum to 0 contributes 0 to every entry):
 *   tabular   trans[slot][q][s'] = sum_i w_i theta_i(phi row (s_q, a_q))[s'] / W                       TL = S
 *             obsp [slot][q][o]  = sum_i w_i theta_i(psi row (a_q, s'_q))[o] / W                       OL = O
 *             joint[slot][q]     = sum_i w_i theta_i(phi)[s'_q] * theta_i(psi)[o_q] / W
 *   factored  segment f of trans (TL = sum of state_feature_size) is the same mean for node T(a_q, f), the row chosen by particle i's OWN
 *             parent set from the features of s_q exactly as the layout comment above states it (DBNNode::cptIndex); segment f of obsp
 *             (OL = sum of obs_feature_size) the same for node O(a_q, f), the row chosen from the features of s'_q;
 *             joint = sum_i w_i prod_f theta_i,T(a,f)[s'_q,f] * prod_g theta_i,O(a,g)[o_q,g] / W.
 *             trans and obsp hold PER-FEATURE MARGINALS OF A MIXTURE over particles and structures: the mixture itself is not the product of
 *             them; joint is the structure-aware quantity.
 * Any output pointer may be NULL (all three: FBA_OK, nothing is done).  Evaluated from whatever record format the context stores, without
 * building a particle's table anywhere.  Serves the main filter of every belief but the nested one (FBA_EINVAL there: its particles are
 * pairs, fba_belief_get_nested), in either Dirichlet mode (the Dirichlet's expectation is the same row); FBA_EINVAL for a plain POMDP
 * context (no counts), a slot range outside the context, nq < 1 and any query index out of range (the message names the query).
 * Read-only: no buffer, flag, counter or Philox position of the context changes, so the call may stand between any two others, after
 * fba_run_*, and on inactive slots.  It does not depend on the particles' domain states, so a lazily reset filter needs no special case.
 * The call is OUTSIDE the parity contract: it is not the simulator's float sum and float division (expected_mult_at, fact_obs_prob), the
 * order of its fp64 additions is the engine's choice and need not repeat bit for bit from call to call, and nothing of it enters the
 * trace or belief_hash.  Every entry is within 8 * (particles + F * (L + 2)) * 2^-53 relative of the exact value (L the longest row, F = 1
 * for trans / obsp and the number of nodes for joint), and exactly 0.0 where every term is. */
int fba_predict_lens(const fba_ctx* ctx, int32_t* TL, int32_t* OL); /* lengths of one query's answer (0, 0 for a plain POMDP) */
int fba_belief_predict(fba_ctx* ctx, int32_t first, int32_t count, int32_t nq,
                       const int32_t* state, const int32_t* action, const int32_t* next_state, const int32_t* obs, /* [nq] each */
                       double* trans,  /* [count][nq][TL] */
                       double* obsp,   /* [count][nq][OL] */
                       double* joint); /* [count][nq]     */
/* The filter's one-step predictive on the device: what the posterior of each slot in [first, first + count) says about the step that takes
 * action[slot - first] and observes obs[slot - first] -- each particle's OWN domain state s_i propagated through its OWN model c_i.  With
 * s_i the state fba_belief_get returns for particle i (a lazily reset rejection filter included), c_i its fp32 table, w_i its weight (1.0 in
 * a flat filter), W = sum w_i and theta_i(row)[k] = c_i[row + k] / sum_k c_i[row + k] in fp64 (a row whose counts sum to 0 gives 0), as for
 * fba_belief_predict:
 *   tabular   p_i(s') = theta_i(phi row (s_i, a))[s']        l_i(s') = theta_i(psi row (a, s'))[o]
 *   factored  p_i(s') = prod_f theta_i,T(a,f)(row chosen by particle i's OWN parent set from the features of s_i)[s'_f]
 *             l_i(s') = prod_g theta_i,O(a,g)(row chosen from the features of s')[o_g]
 *             rows and features exactly as the layout comment above states them (DBNNode::cptIndex): the observation row is chosen by the
 *             NEW state.
 *   next_mass[slot][s'] = sum_i w_i p_i(s') / W              the predictive next-state marginal
 *   post_mass[slot][s'] = sum_i w_i p_i(s') l_i(s') / W      the Rao-Blackwellised posterior, UNNORMALISED: its sum over s' is the evidence
 *   evidence [slot]     = sum_i w_i sum_s' p_i(s') l_i(s') / W   P(o | b, a): the expected acceptance rate of the rejection update, the
 *                                                            expected ratio of the importance filter's weight totals
 * A particle whose state is outside [0, S) contributes nothing, as in state_mass of fba_belief_summary.  Any output pointer may be NULL (all
 * three: FBA_OK, nothing is done); obs may be NULL iff post_mass and evidence are.  Evaluated from whatever record format the context stores,
 * without building a particle's table anywhere.  Serves the main filter of every belief but the nested one, in either Dirichlet mode, the
 * point-estimate belief's one particle included; FBA_EINVAL for the nested belief, a plain POMDP context, a slot range outside the context,
 * an action or observation index out of range (the message names the slot) and obs == NULL while post_mass or evidence is asked for.
 * FBA_ESTATE where the model does not fit the kernels: one particle's fp64 factor tables -- (TL + R + 1) * 8 + (1 + nodes) * 4 bytes, TL the
 * entries of the transition rows (S for a tabular model) and R the rows of an action's observation nodes (S for a tabular model); history
 * records: R counted twice, plus R * 16 once -- must fit 63 KB of LDS, so a tabular model of fp32 records is served up to S = 4 030; more than
 * FBA_MAX_FEATURES transition or observation nodes, a layout whose nodes differ in size between actions, and a slot whose history records
 * hold more entries than they have room for are refused the same way.  A slot whose weights are all 0 gives 0.0 in every output.
 * Read-only: no buffer, flag, counter, Philox position, trace record or belief_hash changes, so the call may stand between any two others,
 * after fba_run_*, and on inactive slots.  The call is OUTSIDE the parity contract: it is not the simulator's float arithmetic
 * (expected_mult_at, fact_obs_prob), the order of its fp64 additions is the engine's choice and need not repeat bit for bit from call to
 * call.  Every entry of next_mass and post_mass is within 8 * (particles + F * (L + 2)) * 2^-53 relative of the exact value (L the longest
 * row; F the transition nodes of an action for next_mass, 1 for a tabular model, and all nodes of a step for post_mass, 2 for a tabular
 * model), evidence within 8 * (particles + S + F * (L + 2)) * 2^-53, and exactly 0.0 where every term is. */
int fba_belief_forecast(fba_ctx* ctx, int32_t first, int32_t count,
                        const int32_t* action,   /* [count], one per slot of the range                  */
                        const int32_t* obs,      /* [count]; may be NULL iff post_mass and evidence are */
                        double* next_mass,       /* [count][S] */
                        double* post_mass,       /* [count][S] */
                        double* evidence);       /* [count]    */
/* The posterior over whole model graphs on the device: what edge_prob of fba_belief_summary, a marginal per (word, candidate), cannot
 * say.  Everything is defined through what fba_belief_get returns: the STRUCTURE of particle i is the list of n_words = n_mask_words
 * uint32 bit patterns at positions n_counts + m of its blob, w_i its weight (1.0 in a flat filter).  n_sets = 1 << the largest
 * n_candidates over the nodes with mask_word >= 0 (at most 256); fba_structure_lens gives (0, 0) where the model has no parent-set words.
 * All masses are UNNORMALISED: the caller divides by weight_total.
 *   head      [count]
 *   set_mass  [count][n_words][n_sets]  sum of w_i over the particles whose word m equals v; 0.0 for a v that never occurs (a value
 *                                       >= n_sets cannot occur in a legal record and is counted nowhere)
 *   top_words [count][top_k][n_words]   the `stored` distinct structures of largest mass, by mass descending and among equal masses by
 *   top_mass  [count][top_k]            word list ascending (word 0 most significant); rows behind `stored` are zero
 *   query_mass[count][nq]               sum of w_i over the particles whose whole word list equals query[q]
 * Distinct structures are found in a per-slot table of FBA_STRUCT_TABLE entries.  Up to that many distinct structures everything is
 * exact; beyond it overflow = 1, `distinct` counts the structures that found a place, the top list is taken among those, and
 * unplaced_mass is the weight that found none.  set_mass and query_mass never depend on the table.  A particle of weight 0.0 still
 * counts as a structure.
 * Any output pointer may be NULL (all of them: FBA_OK, nothing is done).  top_k is 0..FBA_STRUCT_MAX_TOP (0: top_words and top_mass are
 * ignored), nq is 0..65536 (query may be NULL iff nq is 0).  Serves what fba_belief_summary serves: the main filter of every belief but
 * the nested one, in every record format, a lazily reset rejection filter included (words do not depend on states).  FBA_EINVAL for the
 * nested belief, a context whose model has no parent-set words (a plain POMDP, a tabular model, a factored model of a fixed graph), a
 * slot range outside the context, top_k or nq out of range, query == NULL with nq > 0, and a query word that is illegal for its node
 * by the rule of fba_belief_import (word m < 1 << n_candidates of every node it serves; the message names the query and the word).
 * Read-only: no buffer, flag, counter or Philox position of the context changes, so the call may stand between any two others, after
 * fba_run_*, and on inactive slots.
 * The call is OUTSIDE the parity contract: the order of its fp64 additions is the engine's choice and need not repeat bit for bit from
 * call to call; nothing of it enters the trace or belief_hash.  Every mass is within 8 * particles * 2^-53 relative of the exact sum,
 * and exactly 0.0 where every term is.  In a flat filter every mass is an integer below 2^53, hence exact, and the whole answer --
 * the order of the top list included -- repeats bit for bit. */
#define FBA_STRUCT_MAX_TOP 64
#define FBA_STRUCT_TABLE 2048
typedef struct fba_structure_head {
    double  weight_total;   /* sum of w_i (N exactly in a flat filter), as in fba_belief_summary            */
    double  unplaced_mass;  /* weight of the particles whose structure found no place in the table          */
    int32_t distinct;       /* distinct structures found; exact when overflow == 0, a lower bound otherwise */
    int32_t overflow;       /* 1: more than FBA_STRUCT_TABLE distinct structures in this slot               */
    int32_t stored;         /* entries written to top_words / top_mass for this slot: min(top_k, distinct)  */
    int32_t reserved;
} fba_structure_head;
int fba_structure_lens(const fba_ctx* ctx, int32_t* n_words, int32_t* n_sets);
int fba_belief_structures(fba_ctx* ctx, int32_t first, int32_t count,
                          int32_t top_k, int32_t nq,
                          const uint32_t* query,    /* [nq][n_words], may be NULL iff nq == 0 */
                          fba_structure_head* head, /* [count]                                */
                          double*   set_mass,       /* [count][n_words][n_sets]               */
                          uint32_t* top_words,      /* [count][top_k][n_words]                */
                          double*   top_mass,       /* [count][top_k]                         */
                          double*   query_mass);    /* [count][nq]                            */
/* per-slot record of the last select_action / belief_update (root statistics, rejection count,
 * belief checksum) */
int fba_last_step_info(fba_ctx* ctx, fba_trace_rec* recs /* [slots] */);

/* ---- whole-experiment interface ------------------------------------------------------- */

/* experiment::planning::run(conf)            src/experiments/PlanningExperiment.cpp:27-55
 * stats[1]; all `runs` runs execute concurrently, `slots` at a time. */
int fba_run_planning(fba_ctx* ctx, fba_stat* stats);
/* experiment::bapomdp::run(bapomdp, conf)    src/experiments/BAPOMDPExperiment.cpp:32-78
 * stats[episodes]: statistic e accumulates the return of episode e over runs, in run order. */
int fba_run_bapomdp(fba_ctx* ctx, fba_stat* stats);
/* throughput driver used by bench.py: advance every slot by `ticks` real time-steps
 * (search + env step + belief update), restarting episodes/runs as they finish. */
int fba_run_ticks(fba_ctx* ctx, int32_t ticks);

/* What becomes of a run whose rejection update gives up.  The reference's rejectSample (RejectionSampling.hpp:26-72) loops until it has
 * accepted `particles` attempts; the engine cannot loop forever, so an update GIVES UP iff its particles-th acceptance is not among its
 * first max_attempts attempts, i.e. iff its update_count would exceed max_attempts.  That holds exactly for every rejection kernel -- the
 * plain, fully connected, packed tiger (LDS / once / compact), packed factored-tiger and history-record ones: they test the limit where a
 * round of attempts starts, every round size divides FBA_REJECT_QUANTUM, and max_attempts must be a positive multiple of it (0: 2^28, the
 * limit of a context that never made this call); anything else is FBA_EINVAL and leaves policy and limit as they were.  The limit also
 * holds for fba_belief_update, which otherwise behaves as ever: it returns FBA_ESTATE with a message that names the slot and the limit in
 * force, and the context stays usable.  (The nested belief counts its own attempts and the Metropolis-Hastings beliefs have limits of
 * their own: neither is touched.)
 *   FBA_GIVEUP_STOP    (default) the first such slot stops the whole fba_run_* with FBA_ESTATE, as that message says.
 *   FBA_GIVEUP_RETIRE  in fba_run_planning, fba_run_bapomdp, fba_run_bapomdp_span and fba_run_ticks a slot whose update gives up, in any of
 *                      its rejection filters (the main one, or the fully connected / correct-graph filter of the reinvigoration,
 *                      incubator and cheating beliefs), RETIRES its run.  Runs never couple -- their streams are addressed by run -- so
 *                      nothing else changes by a bit:
 *     - the real step has been taken and is accounted like any other (trace record, fba_step_stats, fba_structure_stats, probe); its
 *       trace record carries update_count = FBA_UPDATE_GAVE_UP, and its weight_total and belief_hash are unspecified;
 *     - if that step was the last of the horizon its episode's return is recorded and stays counted (counted = 1); else the episode is
 *       void, and so is every later episode of the run.  A void episode has lengths == 0 and returns == 0.0 in fba_get_returns and enters
 *       neither the per-episode statistics, whose `count` drops, nor fba_get_return_sums;
 *     - a given-up update adds nothing to fba_counters.belief_steps, as under STOP;
 *     - the slot goes on with its next run (run + slots) exactly as behind a run's last episode, or becomes inactive if there is none;
 *     - one fba_retired_rec is appended to the list.
 *     Every run that is not retired keeps every bit it has under STOP: trace records, returns, lengths, its contributions to counters,
 *     probe records and statistics bins, Philox positions, final filter.  A retired run keeps every bit up to and including the step that
 *     gave up, but for the three record members named above.  The filter a retired run leaves in a slot whose last run it was is
 *     unspecified in content but valid: fba_belief_export / fba_belief_import take it, fba_belief_init and every later call work.
 *     Retiring conditions every statistic on survival; the list is there so that the caller can judge what was taken out.
 * The list has room for max(runs, slots) records (at most max(slots, 2^22), the trace's own limit: only a context made for endless
 * fba_run_ticks names more runs than that); this call allocates and clears it (under either policy), a new fba_run_* does not, as
 * with the probe.  fba_retired_count returns the records stored and *seen (may be NULL) every retirement since this call: seen > stored
 * can happen only under endless fba_run_ticks.  fba_get_retired copies up to `cap` of them ordered by run.  Retirement is per call: a later
 * span (fba_run_bapomdp_span) starts every run it is given, so dropping retired runs between spans is the caller's job, from this list.
 * The other faults keep stopping the context under either policy: search-tree tables, the room of history records, and a Metropolis-
 * Hastings belief that cannot reproduce the run's history.  With FBA_GIVEUP_STOP and max_attempts = 0 a tick launches exactly what it
 * launched before this call existed. */
#define FBA_REJECT_QUANTUM 1024            /* max_attempts is a multiple of this; every rejection kernel's round of attempts divides it */
enum { FBA_GIVEUP_STOP = 0, FBA_GIVEUP_RETIRE = 1 };
int fba_giveup_policy(fba_ctx* ctx, int32_t policy, int32_t max_attempts /* 0 = 2^28, today's limit */);
#define FBA_RETIRED_REJECTION 1
typedef struct fba_retired_rec {           /* 32 bytes */
    int32_t run, episode, t, slot;         /* the real step whose belief update gave up, addressed as in fba_trace_rec */
    int32_t reason;                        /* FBA_RETIRED_REJECTION (1): rejection sampling accepted fewer than `particles` in max_attempts attempts */
    int32_t counted;                       /* 1: the episode had already ended with this step and its return is counted; 0: the episode is void */
    int32_t max_attempts, reserved;
} fba_retired_rec;
int fba_retired_count(const fba_ctx* ctx, int64_t* seen);   /* records stored; *seen (may be NULL) every retirement, as fba_probe_count */
int fba_get_retired(const fba_ctx* ctx, fba_retired_rec* out, int32_t cap);   /* ordered by (run) */

/* per-(run, episode) discounted returns of the last fba_run_*: returns[runs * episodes] */
int fba_get_returns(const fba_ctx* ctx, double* returns, int32_t* lengths);
int fba_get_counters(fba_ctx* ctx, fba_counters* out);
/* {episodes finished, sum of returns, sum of squared returns} over all slots since fba_create:
 * what a multi-GPU job all-reduces (the pooled merge of analysis/preprocess/merge_result_files.py:60-78) */
int fba_get_return_sums(fba_ctx* ctx, double* out /* [3] */);
int fba_get_kernel_times(fba_ctx* ctx, fba_kernel_time* out /* [FBA_K_COUNT] */);
int fba_reset_kernel_times(fba_ctx* ctx);
/* The records kept: min(records written, capacity).  The trace holds at most 2^22 records (2^18 with cfg.trace = 2, whose histograms take
 * 256 bytes more per record), and never more than the experiment asked room for; records beyond the capacity are dropped silently.  With
 * fba_step_stats on, the sum of `steps` over all bins exceeding fba_trace_count says the trace was truncated. */
int fba_trace_count(const fba_ctx* ctx);
int fba_get_trace(const fba_ctx* ctx, fba_trace_rec* out, int32_t cap);
/* cfg.trace = 2: hist[i][s] = how many particles of the filter held domain state s after the belief update of trace record i
 * (the order of fba_get_trace) -- what FlatFilter::toString (src/beliefs/particle_filters/FlatFilter.cpp:70-94) prints at -v 3
 * ("Status of rejection sampling filter after update", RejectionSampling.cpp:39, BARejectionSampling.cpp:46); all zero for a
 * record without an update (terminal step).  out[cap][FBA_TRACE_HIST_BINS]. */
#define FBA_TRACE_HIST_BINS 64
int fba_get_trace_hist(const fba_ctx* ctx, uint32_t* out, int32_t cap);
/* Per-step evidence recorded while experiments run: what the filter of a slot said about the step that actually happened, evaluated on
 * the device inside the tick, between the environment step and the belief update -- the one place where the action, the observation and
 * the true new state s* of a real step exist beside the belief that has not seen them yet.  In the notation of fba_belief_forecast, with
 * a and o the step's action and observation:
 *   evidence  = sum_i w_i sum_s' p_i(s') l_i(s') / W   P(o | b, a): its logarithm summed over the steps is the prequential likelihood
 *   next_true = sum_i w_i p_i(s*) / W                  the predictive probability of the true new state
 *   post_true = sum_i w_i p_i(s*) l_i(s*) / W          UNNORMALISED: post_true / evidence is the Rao-Blackwellised posterior of s*
 * fba_probe_enable(first, count, capacity) turns the probe on for slots [first, first + count) with room for `capacity` records and
 * clears the buffer; count = 0 turns it off and frees the buffer.  Records are written by fba_run_bapomdp and fba_run_ticks, one for every
 * real step of a slot of the range that is followed by a belief update: a terminal step has no update and no record, and the per-call
 * interface writes none (its host has the action and the observation: fba_belief_forecast).  A new fba_run_bapomdp does not clear the
 * buffer.  fba_probe_count returns the records stored; *seen (may be NULL) counts every step probed, so seen > stored says the buffer was
 * too small.  fba_get_probe copies up to `cap` of the stored records, ordered by (run, episode, t) as fba_get_trace orders its own; which
 * records of one launch are kept when the buffer runs full is unspecified.  (run, episode, t) identifies a record.
 * Same coverage as fba_belief_forecast: every record format, either Dirichlet mode, a lazily reset rejection filter, each particle under
 * its OWN parent sets; a particle whose state is outside [0, S) has weight 0.  Where every observation node of the action has at most one
 * parent under a particle's parent set (gridworld, collision avoidance, sysadmin) the sum over s' is evaluated in its factorised form,
 * TL + R operations per particle instead of S * nodes; other particles (the factored tiger's listen) and tabular models enumerate S.
 * FBA_EINVAL for the nested belief, a plain POMDP context, a slot range outside the context and a negative capacity; FBA_ESTATE where
 * the model does not fit the kernel's LDS or node limits, under the rule fba_belief_forecast documents.  A slot whose history records
 * have no room for the step's entry writes no record: the update that follows stops the run as it does without a probe.
 * Read-only on everything else: with a probe on, every particle, every trace record (belief_hash included), every return and counter
 * and every Philox position keep their bits; with no probe enabled a tick launches exactly what it launched before.
 * The values are OUTSIDE the parity contract, as fba_belief_forecast's are: evidence is within 8 * (particles + S + F * (L + 2)) * 2^-53
 * relative of the exact value, next_true and post_true within the bounds of next_mass and post_mass, an output is exactly 0.0 where
 * every term is, and a slot whose weights are all 0 gives zeros. */
typedef struct fba_probe_rec {
    int32_t run, episode, t;      /* the step's position, as in fba_trace_rec */
    int32_t slot;
    int32_t action, obs, state;   /* state: the true environment state after the step */
    int32_t reserved;
    double  evidence, next_true, post_true;
} fba_probe_rec;
int fba_probe_enable(fba_ctx* ctx, int32_t first, int32_t count, int32_t capacity); /* count = 0: off, the buffer is freed */
int fba_probe_count(const fba_ctx* ctx, int64_t* seen);  /* returns the records stored; *seen (may be NULL) counts every step probed, so seen > stored says the buffer was too small */
int fba_get_probe(const fba_ctx* ctx, fba_probe_rec* out, int32_t cap);
/* Per-step statistics of every run, reduced on the device inside the tick: episodes * horizon bins of 536 bytes whatever the number of runs,
 * where the trace (capped, above) and the probe (a buffer with a capacity) cannot follow.  Bin (e, t) is a reduction over the trace records
 * that fba_run_planning, fba_run_bapomdp, fba_run_bapomdp_span and fba_run_ticks would write for episode e, step t with cfg.trace = 1 and
 * unlimited capacity, each member from the record's own fields (action, terminal, reward, n_nodes, tree_depth, root_n, root_q,
 * update_count) -- filled whether or not cfg.trace is set.  Episodes are counted from 0 of the run; a span fills only its own episodes; the
 * per-call interface writes nothing (its host holds every value).  A new fba_run_* does not clear the bins, as with the probe: runs
 * executed one after the other by one slot, experiments run one after the other and spans add up; fba_step_stats_enable(1) clears them.
 * Budgeted searches (search_budget > 0) are covered: a tick accounts only the slots that took their step in it.
 * The probe members are filled for the steps a probe evaluates -- fba_probe_enable is on and covers the slot -- whether or not the step's
 * record fitted the probe's buffer, so fba_probe_enable(first, count, 0) feeds the bins without keeping a record; without a probe they
 * stay 0.  The logarithm is the engine's deterministic one (det_log), within 3e-16 * max(1, |log x|) of libm's.
 * Every model (a plain POMDP included), belief, planner and record format is served.  FBA_EINVAL: a null ctx, out == NULL, cap < episodes *
 * horizon; FBA_ESTATE: fba_get_step_stats while the statistics are off.  fba_get_step_stats synchronises the stream, like fba_get_probe.
 * Read-only on everything else: with the statistics on, every trace record (belief_hash included), return, statistic, counter, probe
 * record, fba_last_step_info, Philox position and particle keeps its bits; with them off a tick launches exactly what it launched before.
 * The values are OUTSIDE the parity contract for their double sums only: the integer members are exact; a double member summed over n
 * terms x_i is within n * 2^-52 * sum |x_i| of the exact sum, and exact where every term is (the built-in domains' rewards are multiples
 * of 0.5 of magnitude <= 1000, so reward_sum and reward_sq_sum are exact below 2^53); each post_ratio term carries the one rounding of
 * its division, each log term det_log's distance from libm. */
typedef struct fba_step_stat {              /* one per (episode, t); every member 8-byte aligned, 536 bytes */
    uint64_t steps;                         /* real steps taken at this (episode, t), over all runs            */
    uint64_t terminals;                     /* of them terminal (no belief update follows)                     */
    uint64_t action[FBA_MAX_ACTIONS];       /* steps by the action taken                                       */
    uint64_t root_visits[FBA_MAX_ACTIONS];  /* sum of root_n[a] of the step's search                           */
    uint64_t nodes_sum, depth_sum;          /* sum of n_nodes, tree_depth                                      */
    uint64_t attempts_steps, attempts_sum;  /* non-terminal steps whose update reports update_count >= 0, and the sum of those counts */
    int32_t  nodes_max, depth_max, attempts_max, reserved;
    double   reward_sum, reward_sq_sum;     /* r, r*r                                                          */
    double   value_sum, value_sq_sum;       /* q = root_q[action taken], q*q                                   */
    uint64_t probed, evidence_zero;         /* steps the probe evaluated; of them with evidence == 0.0         */
    double   evidence_sum, log_evidence_sum, log_evidence_sq_sum;   /* logs over the probed steps with evidence > 0 */
    double   next_true_sum, post_ratio_sum; /* next_true; post_true / evidence (evidence > 0)                  */
} fba_step_stat;
int fba_step_stats_enable(fba_ctx* ctx, int32_t on);   /* 1: allocate (episodes * horizon bins) and clear; 0: free */
int fba_get_step_stats(fba_ctx* ctx, fba_step_stat* out, int32_t cap);   /* out[episodes][horizon]; returns episodes * horizon */
/* The graph posterior per step of every run, reduced on the device inside the tick: episodes * horizon bins whatever the number of runs,
 * where fba_belief_structures answers only for the filters as they stand between two calls and, after an experiment, for the last run
 * of each slot.  Built like fba_step_stats; neither it nor the probe looks at a parent-set word.
 * A STEP of a slot is a real step that fba_run_bapomdp, fba_run_bapomdp_span or fba_run_ticks takes, terminal steps included; with a
 * search budget only the slots that take their step in a tick are accounted in it.  The step's FILTER is the main filter as it stands
 * when the step is taken, before the belief update that may follow: the filter the step was planned from, the one fba_probe reads.  For
 * that filter, in the notation of fba_belief_structures: W the weight total, set_mass[m][v] and query_mass[q] the unnormalised masses,
 * `distinct` and `overflow` those of the FBA_STRUCT_TABLE table, and cnt[q] the number of particles, whatever their weight, whose whole
 * word list equals query[q].  Bin (episode, t), the episode counted from 0 of the run as in fba_step_stats, accumulates over all steps of
 * all runs the head below and, beside the heads, as arrays of their own because their lengths follow the model (fba_structure_lens) and nq:
 *   set_frac  [bins][n_words][n_sets]  double    sum over the steps with finite W > 0 of set_mass[m][v] / W
 *   query_frac[bins][nq]               double    sum over the same steps of query_mass[q] / W
 *   query_held[bins][nq]               uint64_t  steps with cnt[q] > 0: the filter still holds graph q
 *   query_sole[bins][nq]               uint64_t  steps with cnt[q] == particles: the filter holds nothing else
 * fba_structure_stats_enable(on = 1, nq, query) allocates the bins, clears them and stores the queries (uint32[nq][n_words] word lists as
 * fba_belief_get shows them, nq at most FBA_STRUCT_STATS_MAX_QUERIES); on = 0 frees them (nq and query are ignored).  A new fba_run_* does
 * not clear the bins: runs, experiments and spans add up, as with fba_step_stats and the probe; a span fills only its own episodes.  The
 * per-call interface writes nothing.  fba_get_structure_stats synchronises the stream; any of its pointers may be NULL; it returns
 * episodes * horizon.
 * Every context fba_belief_structures serves is served: every record format with parent-set words, flat and weighted filters, the main
 * filter of the reinvigoration, cheating, incubator and both Metropolis-Hastings beliefs, either Dirichlet mode.  FBA_EINVAL for the
 * nested belief, a model without parent-set words (with the message of fba_belief_structures), nq outside 0..16, query == NULL with
 * nq > 0, a query word that is illegal for its node (the rule and message of fba_belief_structures) and cap_bins < episodes * horizon;
 * FBA_ESTATE for fba_get_structure_stats while the statistics are off and for a record layout fba_belief_structures refuses with
 * FBA_ESTATE.  A refused enable leaves the context as it was, its statistics off.
 * Read-only on everything else: with the statistics on, every particle, trace record (belief_hash included), return, statistic, counter,
 * probe record, fba_step_stats bin, fba_last_step_info and Philox position keeps its bits; with them off a tick launches exactly what
 * it launched before.
 * The integer members are exact.  The double members are OUTSIDE the parity contract: each term carries the bound of
 * fba_belief_structures on its mass and on W (8 * particles * 2^-53 relative each) plus the one rounding of its division, and the sum
 * over n steps adds n * 2^-53 relative; a member is exactly 0.0 where every term is.  In a flat filter every term is k / N: with N a power
 * of two all terms and their sums are exact, and the bins repeat bit for bit. */
#define FBA_STRUCT_STATS_MAX_QUERIES 16
typedef struct fba_structure_stat {   /* one per (episode, t); 48 bytes, every member 8-byte aligned */
    uint64_t steps;          /* steps taken at this (episode, t), over all runs                                        */
    uint64_t weightless;     /* of them from a filter with W == 0 or not finite: they enter no fraction                */
    uint64_t overflowed;     /* of them whose filter held more than FBA_STRUCT_TABLE distinct graphs                   */
    uint64_t collapsed;      /* of them whose filter held exactly one graph (distinct == 1, overflow == 0)             */
    uint64_t distinct_sum;   /* sum of `distinct` as fba_belief_structures reports it (a lower bound where overflowed) */
    int32_t  distinct_max, reserved;
} fba_structure_stat;
int fba_structure_stats_enable(fba_ctx* ctx, int32_t on, int32_t nq, const uint32_t* query /* [nq][n_words]; NULL iff nq == 0 */);
int fba_get_structure_stats(fba_ctx* ctx, int32_t cap_bins, fba_structure_stat* head, double* set_frac, double* query_frac,
                            uint64_t* query_held, uint64_t* query_sole);   /* any pointer may be NULL; returns episodes * horizon */

/* Belief snapshots: keeping, moving and copying the main filter of a slot in the record format the context stores (fba_particle_bytes) --
 * no count table is built anywhere, so a 16 384-particle gridworld filter is 3.0 MB, not the 3.1 GB fba_belief_get would hand out, and the
 * history-record contexts that refuse fba_belief_set are served like every other.
 * A snapshot is one opaque, self-describing block per slot, of fba_belief_snapshot_bytes bytes, constant for a context:
 *   the header fba_snapshot_head, 64 bytes | weights, particles * 8 bytes (importance filters only) | records, particles * fba_particle_bytes bytes
 * The header carries a fingerprint of what a block must match to be taken: the record format (0 fp32 counts, a plain POMDP's states included,
 * 1 packed tiger, 2..4 packed factored tiger of that many state features, 5 gridworld FBA-POMDP history records, 6 tabular gridworld
 * history records, 7 collision-avoidance history records), model, domain and its size arguments, particles, fba_particle_bytes,
 * fba_counts_len, S / A / O, weighted or flat, and a 64-bit hash of the prior the records stand over (FNV-1a over the 32-bit words of
 * what fba_get_prior returns, then of the gridworld's alternative x / y rows where history records use them, then of the structure prior
 * and, for packed factored-tiger records, the three counts of the listen node).  Records stand from the start of their part at the slot's
 * CURRENT stride, head.stride bytes: 64, 128 or fba_particle_bytes for history records of up to 14, up to 30 or more entries,
 * fba_particle_bytes otherwise; the bytes behind the last record, behind a history record's last entry and behind a record's state word
 * are zero, so two exports of one filter are equal byte for byte and export(import(x)) == x.
 *   checksum = sum over the 32-bit words w[i] of the payload (all that follows the header, i from 0) of w[i] * ((i + 1) * FBA_SNAPSHOT_CHECK_MUL)
 *              modulo 2^64 -- a sum, so no order of additions can change it; a host recomputes it from this line.
 * fba_belief_export writes the blocks of slots [first, first + count) to buf (cap >= count * fba_belief_snapshot_bytes).  Like fba_belief_get
 *   it first writes out the states of a lazily reset rejection filter (results keep their bits); nothing else of the context changes, so
 *   it may stand between any two calls, after fba_run_*, and on inactive slots.  Slots are packed on the device and copied a chunk at a
 *   time, through at most 256 MB of staging memory (FBA_SNAPSHOT_STAGE_BYTES in the environment, read at every export and import, sets
 *   another bound in bytes; one block is staged at least).  Export does not ask whether a belief was ever initiated: a slot that never
 *   was -- a slot of fba_run_planning / fba_run_bapomdp beyond the configured runs (fba_run_ticks keeps every slot busy), any slot before fba_belief_init -- holds all-zero records and weights
 *   since fba_create, and its block says so: state 0 in every particle, no history entries, counts 0.0, weights 0.0.  Such a block is
 *   well-formed, an import takes it, and the slot it lands in is as uninitiated as its source.  Export does not look at pending updates or
 *   parked searches of its slots either: it writes the filter as it stands.
 * fba_belief_import takes `count` blocks (bytes == count * fba_belief_snapshot_bytes) into slots [first, first + count), in two passes, so
 *   that a refused block leaves the context untouched.  Host pass: magic, layout version, every fingerprint field, hist_cnt against the
 *   stride and the room of a record, the stride against the format -- FBA_EINVAL, the message names the block, the field and both values.
 *   Device pass: the checksum, then EVERY record before anything is committed -- weights finite and >= 0, state in [0, S), parent-set words
 *   legal for their nodes, fp32 counts finite and >= 0, every history entry decoding to fields of the domain and cells inside the table --
 *   FBA_EINVAL, the message names the slot, the particle and what was wrong with it (the first such particle).  Commit: records into the
 *   slot's live buffer at the block's stride, weights into the live weight buffer, the slot's entries per action set, a pending lazy reset
 *   dropped.  Nothing else of the slot is touched: position, environment state, returns, counters, trace and fba_last_step_info stay.  A
 *   destination slot with a belief update pending, a parked search or a pending buffer swap (inside fba_run_* with a search budget) gives
 *   FBA_ESTATE.  Like fba_belief_set, a successful import makes the belief usable without fba_belief_init.  The caller's buffer must not
 *   change during the call: a range beyond the staging bound is read twice (every chunk validated, then every chunk committed), and the
 *   second reading is not judged again.  The weights are judged one by one, as stated: a block whose weights are all 0.0 (what a
 *   never-initiated slot exports) or whose weights sum beyond the fp64 range is taken, and the slot then behaves as a filter of that
 *   weight total does everywhere else in the engine -- the readers above give zeros for it; it is the host's to import filters it means to run.
 * fba_belief_replicate copies the filter of slot src into every slot of [first, first + count) on the device, with no host round trip
 *   and no validation (the source is the engine's own); src itself is skipped where it lies inside the range.  Same commit, same FBA_ESTATE,
 *   and FBA_ESTATE too on a context whose belief was never made usable (fba_belief_init, fba_belief_set, fba_belief_import or fba_run_*).
 *   The copies are independent filters: they run on at their own slots' Philox positions.
 * Serves the rejection, importance and point-estimate beliefs in every record format, fp32 records under FBA_DENSE_PARTICLES=1 and the
 * plain POMDP filter (states only) included.  FBA_EINVAL for the beliefs whose state is more than the main filter -- reinvigoration and
 * cheating (a second filter), incubator (second and shadow filters), mh-within-gibbs and mh-nips (the run's action-observation history and
 * log likelihood), nested (a filter of domain states per particle) -- for a slot range outside the context and for a buffer too small.
 * fba_run_planning and fba_run_bapomdp initiate a slot's belief at the start of every run, and so does fba_run_ticks when it first
 * sets the slots up and whenever a slot starts a run: an imported belief lives until its slot's run ends.  fba_run_bapomdp_span (below)
 * is the driver that starts its runs from snapshots; fba_run_ticks cannot be warm-started. */
#define FBA_SNAPSHOT_MAGIC     0x53414246u              /* "FBAS" */
#define FBA_SNAPSHOT_VERSION   1
#define FBA_SNAPSHOT_CHECK_MUL 0x9E3779B97F4A7C15ull
#define FBA_SNAPSHOT_HASH_SEED 0xcbf29ce484222325ull
typedef struct fba_snapshot_head {
    uint32_t magic;           /* FBA_SNAPSHOT_MAGIC                                                                            */
    uint16_t version;         /* FBA_SNAPSHOT_VERSION                                                                          */
    uint8_t  record_format;   /* 0..7, above                                                                                   */
    uint8_t  weighted;        /* 1: importance filter, the block holds weights; 0: flat filter                                 */
    uint8_t  model, domain;   /* FBA_MODEL_*, FBA_DOM_*                                                                        */
    uint16_t actions;         /* A                                                                                             */
    int16_t  size, width, height;   /* fba_config's domain size arguments                                                      */
    uint16_t updates;         /* packed records: belief updates the slot has counted since fba_belief_init (what fba_belief_update
                               * guards the 16-bit increments with); 0 otherwise                                              */
    int32_t  particles;       /* N                                                                                             */
    int32_t  particle_bytes;  /* fba_particle_bytes                                                                            */
    int32_t  counts_len;      /* fba_counts_len                                                                                */
    int32_t  states;          /* S                                                                                             */
    int32_t  observations;    /* O                                                                                             */
    uint32_t hist_cnt;        /* history records: entries per record of action a in bits 8a..8a+7; 0 otherwise                 */
    uint32_t stride;          /* bytes between the records of this block                                                       */
    uint64_t prior_hash;
    uint64_t checksum;
} fba_snapshot_head;
int fba_belief_snapshot_bytes(const fba_ctx* ctx, int64_t* per_slot);
int fba_belief_export   (fba_ctx* ctx, int32_t first, int32_t count, void* buf, int64_t cap);
int fba_belief_import   (fba_ctx* ctx, int32_t first, int32_t count, const void* buf, int64_t bytes);
int fba_belief_replicate(fba_ctx* ctx, int32_t src, int32_t first, int32_t count);

/* Fitting snapshot blocks to another context.  fba_belief_import and fba_run_bapomdp_span take blocks of the context's own fingerprint only;
 * fba_belief_convert makes such blocks out of the blocks of a context that differs from `ctx`, the DESTINATION, in two fields only:
 *   particles       (N' in the blocks, N in the context) may differ in every record format;
 *   particle_bytes  may differ in the history formats 5..7, where it is the room of a record: particle_bytes / 4 - 2 entries.  It follows
 *                   episodes * horizon, so this is what lets a filter learned in a 20-episode context continue in a 40-episode one.
 * Every other fingerprint field -- magic, layout version, record format, weighted, model, domain, size, width, height, counts length, S, A,
 * O, prior hash -- and, in the formats 0..4, particle_bytes too must equal the context's: FBA_EINVAL names block, field and both values, as
 * an import does.  A block's hist_cnt and stride are judged against the room of the block's OWN records, by the rule an import applies to a
 * context's.  `src` holds `count` blocks of one size, fba_snapshot_block_bytes of block 0 (src_bytes == count * that); a block of another
 * particle count or room than block 0 is refused by name.  `dst` takes count blocks of fba_belief_snapshot_bytes (dst_cap says how much
 * room it has) and must not overlap src.  fba_snapshot_block_bytes is host arithmetic on a header, 64 + (weighted ? particles * 8 : 0) +
 * particles * particle_bytes, and needs no context.
 * An output block carries the context's own header with hist_cnt and updates copied, the stride the context stores records of that many
 * entries at, and the checksum of the new payload.  It is canonical -- every byte behind a record's last entry, behind the last record and
 * behind a state word is zero -- so export(import(convert(x))) == convert(x) byte for byte.  Output particle j of block b is
 *   N == N':            particle j, its weight bits unchanged: a change of room and stride only, and the input itself where particle_bytes
 *                       is equal as well;
 *   N != N', flat:      particle uniform_int(N'), the first draw of the Philox stream keyed by `seed` at position (run first_run + b,
 *                       episode 0, t 0), phase FBA_PHASE_CONVERT, unit j;
 *   N != N', weighted:  the particle WeightedFilter::sample picks for the threshold u01 * total, u01 the first draw of the same stream, over
 *                       the device-order inclusive prefix sums of the N' source weights, total = the last of them; every output weight is
 *                       1.0 / N, what a resampling leaves.  A block whose total is 0 or not finite cannot be sampled from: FBA_EINVAL names
 *                       it (with N == N' it is taken, as an import takes it).
 * first_run makes blocks [0, k) and [k, n) converted in two calls (first_run 0 and k) the bytes of one call.  Records are copied whole in the
 * formats 0..4; history records move as words [0, 2 + entries), read at the source's stride, written at the destination's.
 * FBA_EINVAL, all with the context untouched (the content of dst is then unspecified): count < 1, a null or overlapping buffer, src_bytes
 * other than count blocks, dst_cap too small, a belief that snapshots refuse, a fingerprint mismatch, more entries per record than the
 * destination has room for ("block b holds t entries per record / room for r"), and a source block that fails the device pass of an import
 * -- the checksum and every weight, state, parent-set word, count and history entry, judged against the source's own particle count and
 * stride; the message names block, particle and what was wrong.  FBA_EHIP where the staging memory cannot be had, with the bytes asked for.
 * The call reads nothing of the context but its configuration and writes nothing: no slot, flag, counter, Philox position or trace record
 * changes, so it may stand between any two calls.  Source and destination blocks are staged a chunk at a time, both sides together under
 * the bound of fba_belief_import (FBA_SNAPSHOT_STAGE_BYTES), one block of each at least; results do not depend on the chunking. */
int64_t fba_snapshot_block_bytes(const fba_snapshot_head* head);
int fba_belief_convert(fba_ctx* ctx, int32_t count, const void* src, int64_t src_bytes, uint64_t seed, uint32_t first_run, void* dst, int64_t dst_cap);

/* A Bayes-adaptive experiment in spans, resumed from belief snapshots bit for bit.  The call runs episodes [first_episode, stop_episode)
 * of every run of the experiment (0 <= first < stop <= episodes) at the stream positions of the uninterrupted experiment -- (run, episode, t)
 * with the episode counted from 0 of the run -- so spans run one after the other, each from the blocks exported after the one before,
 * give the trace records, returns, lengths, statistics and final filters of one fba_run_bapomdp, every bit of them.
 *   blocks == NULL: first_episode and nblocks must be 0; every run starts from the prior, as in fba_run_bapomdp (which is unchanged).
 *   blocks given:   Belief::initiate of a run is replaced by taking block (run - run_offset) % nblocks as that run's filter; nblocks is 1
 *                   (one learned filter for every run) or `runs` (each run's own checkpoint), bytes == nblocks * fba_belief_snapshot_bytes.
 *                   resetDomainStateDistribution at the start of episode first_episode follows as at every episode, so a block is the
 *                   filter as it stood when the episode before ended -- what fba_belief_export gives after a span.
 * After a span with runs <= slots, slot run - run_offset holds that run's filter as its last update left it (nothing touches a slot once
 * it is inactive): fba_belief_export of those slots is the checkpoint for first_episode = this call's stop_episode.  With runs > slots a
 * slot is left with the filter of the LAST run it executed only; checkpoints of more runs than slots are made by sharding with run_offset.
 * stats[e] has count 0 outside the span, fba_get_returns gives 0 there, the trace holds the span's records only; counters, return sums,
 * the probe and the kernel times behave as in fba_run_bapomdp (FBA_K_BELIEF_INIT: the restores, units = particles taken from blocks,
 * bytes = particles * (block stride + 8 if weighted), read and written).
 * Every block passes the two passes of fba_belief_import before anything runs -- host: every header field; device: checksum and every
 * record -- and two rules of this call's: (host) what a block holds plus (stop - first) * horizon may not exceed episodes * horizon, where
 * "holds" is the entries per record of a history format and head.updates of a packed one, so that a resumed run never holds more than an
 * uninterrupted run of this context could and every bound fba_create derived from episodes * horizon keeps holding; (device) no 16-bit
 * increment of a packed record exceeds head.updates.  After fba_run_bapomdp and after a span, head.updates of an exported packed filter
 * is the real steps of the slot's run so far (an update follows every step but a terminal one), on top of its block's.  The blocks stand
 * in device memory for the duration of the call, uploaded and judged a chunk at a time under the staging bound of fba_belief_import.
 * FBA_EINVAL, with the context left as it was: a plain POMDP context, a belief that snapshots refuse, a span outside [0, episodes], blocks
 * == NULL with first_episode or nblocks != 0, nblocks other than 1 or runs, wrong bytes, any block refused by a pass (the message names
 * the block and what was wrong).  FBA_EHIP where the store does not fit (the message says how many bytes were asked for). */
int fba_run_bapomdp_span(fba_ctx* ctx, int32_t first_episode, int32_t stop_episode, const void* blocks, int32_t nblocks, int64_t bytes,
                         fba_stat* stats /* [episodes] */);

/* diagnostic: out[i] = u * sqrt(L[i] / n[i]) evaluated on the device, to check that the
 * engine's fp64 divide and square root round like the host's (they must, for UCB parity) */
int fba_selftest_ucb(fba_ctx* ctx, const double* L, const int32_t* n, int32_t count, double u, double* out);

/* BABNModel::LogBDScore(prior) (src/bayes-adaptive/states/factored/BABNModel.cpp:451-478 over DBNNode::LogBDScore,
 * DBNNode.cpp:82-117): the log Bayesian-Dirichlet score of one particle's counts against a prior blob of the same
 * structure -- what the structure-learning beliefs (MHwithinGibbs.cpp:334-395, MHNIPS2018.cpp) accept and reject models by.
 * Evaluated on the device with the engine's deterministic lgamma; fba_selftest_lgamma exposes that function. */
int fba_log_bd_score(fba_ctx* ctx, const float* counts, const float* prior, double* out);
int fba_selftest_lgamma(fba_ctx* ctx, const double* x, int32_t count, double* out);

/* utils::Statistic::add / var / stder, exported so hosts merge returns exactly as the
 * reference does */
void fba_stat_add(fba_stat* s, double v);
double fba_stat_var(const fba_stat* s);
double fba_stat_stder(const fba_stat* s);

#ifdef __cplusplus
}
#endif
#endif
