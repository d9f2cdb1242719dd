// fba_search_hist2.inc -- the body of search_hist2_kernel and hist2_flat_search (fba_search.hip), which include it inside their braces
// with `constexpr bool FLAT` set (true: the root particle of a plain rejection filter), and of search_tabhist_kernel / tabhist_flat_search
// with `constexpr bool TAB` set (the tabular model's records, Problem::hist == 2: one step per iteration, gridworld_tab_hist_step, on
// every lane of the quad; no shared tables).  Not a header: it is only valid there.
    constexpr int AMAX = 4;
    P.model = TAB ? FBA_MODEL_BA_TABLE : FBA_MODEL_BA_FACTORED; P.domain = FBA_DOM_GRIDWORLD; P.A = 4; P.belief = FLAT ? FBA_BELIEF_REJECTION : FBA_BELIEF_IMPORTANCE;
    extern __shared__ double lds_all[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tl = lane >> 2;
    const int depth_cap = P.max_depth > 0 ? P.max_depth : 1;
    const size_t shared_bytes = TAB ? 0 : h2_shared_bytes(P, LROWS);
    double* lds = reinterpret_cast<double*>(reinterpret_cast<char*>(lds_all) + shared_bytes + (size_t)wave * h2_wave_bytes(P));   // this wave's paths and staging area
    double* path_q   = lds + tl;                                                                                  // [depth][trees]: the chosen action's Q as the descent saw it
    int32_t* path_n  = reinterpret_cast<int32_t*>(path_q - tl + (size_t)depth_cap * HIST_TREES) + tl;            // ... and its count
    float* path_r    = reinterpret_cast<float*>(path_n - tl + (size_t)depth_cap * HIST_TREES) + tl;
    int32_t* path_na = reinterpret_cast<int32_t*>(path_r - tl + (size_t)depth_cap * HIST_TREES) + tl;            // bucket << 5 | action
    uint32_t* stage  = reinterpret_cast<uint32_t*>(path_na - tl + (size_t)depth_cap * HIST_TREES) + tl;           // [Cs][trees]
                                                                                                                  // (stage also holds the back-up's returns: two words per level)
    // the root's statistics, [4 counts, 4 Q's][trees]: read where the root is selected at and where it is backed up, i.e. twice per simulation -- in
    // registers they were thirteen of the kernel's live values for the whole search
    double* root_q  = reinterpret_cast<double*>(stage - tl + (size_t)max(P.Cs, 2 * depth_cap) * HIST_TREES) + tl;      // [4][trees]
    int32_t* root_n = reinterpret_cast<int32_t*>(root_q - tl + (size_t)4 * HIST_TREES) + tl;                           // [4][trees]
    int32_t* rec_geo = root_n - tl + (size_t)4 * HIST_TREES + tl;   // [trees]: pieces of a record | pieces between records << 8 (read twice per simulation)
    const HistLayout HL(P.gw_N, P.gw_G, 4);
    {   // the workgroup's shared tables: every thread, before any quad leaves
        const uint4* src = LROWS ? reinterpret_cast<const uint4*>(P.hist_lds) : reinterpret_cast<const uint4*>(P.hist_base + HL.obase0);
        uint4* dst       = reinterpret_cast<uint4*>(lds_all);
        for (int i = threadIdx.x; i < (int)(shared_bytes / 16); i += (int)blockDim.x) dst[i] = src[i];
        __syncthreads();
    }
    const uint8_t* s_rid = reinterpret_cast<const uint8_t*>(lds_all);
    const float* s_rows  = reinterpret_cast<const float*>(reinterpret_cast<const char*>(lds_all) + (LROWS ? P.hist_rid_bytes : 0));
    const int tree_k = (blockIdx.x * (int)(blockDim.x >> 6) + wave) * HIST_TREES + tl;   // (the launcher picks 4, 2 or 1 waves per workgroup: what 64 KB of LDS hold)
    if (tree_k >= P.E) return;
    const int e = D.ab_lockstep ? D.search_order[tree_k] : tree_k;   // (lock-step waves: slots dealt to waves by the depth their searches have left)
    if (!D.active[e]) return;  // (a quad leaves together)

    QuadRng g;
    g.init(P.seed_lo, P.seed_hi, (uint32_t)D.run[e], (uint32_t)D.episode[e], (uint32_t)D.t[e], lane);
    const int hist_len  = D.t[e];
    const int max_tree_depth = min(P.horizon - hist_len, P.max_depth);
    const float* prec   = D.p_rec + rec_base(P, D, e, D.bufsel[e]) * (size_t)P.Cs;
    const uint32_t hist_cnt = D.hist_cnt[e];
    // 16-byte pieces of a record (state, structure bits, entries) and, above them, the 16-byte pieces between this slot's records (hist_stride)
    *rec_geo = ((hist_total(hist_cnt) + 5) >> 2) | (hist_stride(P, hist_total(hist_cnt)) >> 2) << 8;
    const bool uni_exact    = !FLAT && (P.N & (P.N - 1)) == 0 && D.uni_total == 1.0;   // N = 2^k: the prefix sums of the weights 1/N are the exact values (i + 1) / N

    if (P.planner == FBA_PLANNER_RANDOM) {  // RandomPlanner::selectAction RandomPlanner.cpp:14-24
        g.stream(FBA_PHASE_SEARCH, (uint32_t)P.sims);
        g.ensure(2);
        (void)g.u01();                      // the belief sample: GridWorld::generateRandomAction does not look at the state
        D.action[e] = g.slow_int(0, 4);
        if (P.search_budget > 0) D.search_done[e] = 1;
        return;
    }
    const uint32_t nlines = (uint32_t)D.bkt_lines;
    uint4* tab            = D.bkt + (size_t)e * nlines * 8;
    uint32_t* tabw        = reinterpret_cast<uint32_t*>(tab);
    const int ROOT        = (int)(nlines * 2u);   // the root has no bucket: its statistics live in registers
    const int budget      = P.search_budget;
    int sim               = budget > 0 ? D.s_sim[e] : 0;
    const bool resume     = sim > 0;
    int n_nodes = 1, tree_depth = 0;
    uint32_t steps = 0;   // (of this launch: at most sims x horizon)
#pragma unroll
    for (int a = 0; a < AMAX; ++a) { root_n[a * HIST_TREES] = 0; root_q[a * HIST_TREES] = 0.0; }
    uint32_t epoch;
    if (!resume) {
        epoch = D.epoch[e] + 1;
        if (epoch > 15u) {   // the four bits of the key are used up: empty the table (once in fifteen searches)
            for (uint32_t k = (uint32_t)g.q; k < nlines * 8u; k += HIST_QUAD) tab[k] = make_uint4(0, 0, 0, 0);
            epoch = 1;
        }
        D.epoch[e] = epoch;
    } else {
        n_nodes    = D.s_nodes[e];
        tree_depth = D.s_depth[e];
        epoch      = D.epoch[e];
        const int32_t* rn = reinterpret_cast<const int32_t*>(D.s_root + (size_t)e * 6);
        const double* rq  = D.s_root + (size_t)e * 6 + 2;
#pragma unroll
        for (int a = 0; a < AMAX; ++a) { root_n[a * HIST_TREES] = rn[a]; root_q[a * HIST_TREES] = rq[a]; }
    }
    const uint32_t ekey = epoch << 28;
    int ts_src = -1;
    if (!FLAT && P.planner == FBA_PLANNER_TS) {  // TSPlanner / BATSPlanner: one belief sample, then the search from that particle (flat filters: dense contexts)
        g.stream(FBA_PHASE_SEARCH, (uint32_t)P.sims + 2u);
        g.ensure(1);
        ts_src = uniform_weight_pick(D.uni_scan, P.N, g.u01() * D.uni_total, D.uni_total);
    }
    int mode = 0, iter = 0;  // 0 = start a simulation, 1 = in the tree, 2 = rollout
    int node = ROOT, dtg = 0, plen = 0, rdepth = 0, cur_src = 0;
    uint32_t sp = 0, hist_mask = 0;
    double rret = 0, rdisc = 1;
    bool have_particle = false, pend = false, broken = false;
    uint32_t pk = 0, pline = 0;          // the child being looked up: its key, its home line
    uint4 pf[H2_PF];                     // this lane's share of what was requested an iteration ago: a line of the table, or a root particle
#pragma unroll
    for (int j = 0; j < H2_PF; ++j) pf[j] = make_uint4(0, 0, 0, 0);

    // the root particle of simulation `sim`: Belief::sample() on its stream, and this lane's pieces of the record on their way
    // (its stream is set and eight draws -- the root sample, the first action, six rows -- are ensured by the caller)
    auto request_particle = [&]() {
        if (ts_src >= 0) cur_src = ts_src;
        else if (FLAT) cur_src = (int)__umul64hi(g.next64(), (uint64_t)(uint32_t)P.N);   // uniform_int(N) (Rng::uniform_int, fba_device.h)
        else {
            const double u = g.u01();
            if (uni_exact) cur_src = max((int)ceil(u * (double)P.N) - 1, 0);   // the largest i with i / N < u (WeightedFilter.cpp:163-191 on exact prefix sums)
            else cur_src = uniform_weight_pick(D.uni_scan, P.N, u * D.uni_total, D.uni_total);
        }
        const int n4s = *rec_geo;
        const uint4* rp = reinterpret_cast<const uint4*>(prec) + __umul24((uint32_t)cur_src, (uint32_t)n4s >> 8);   // (N * Cs / 4 < 2^24)
#pragma unroll
        for (int j = 0; j < H2_PF; ++j) pf[j] = rp[min(g.q + HIST_QUAD * j, (n4s & 0xff) - 1)];
    };

#ifdef FBA_PROFILE_SEARCH
    long long prof_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, prev_ = clock64();
#endif
    while (true) {
        PROF_MARK(6)
        int cn[AMAX] = {0, 0, 0, 0};          // the current node's statistics (below the root), set where the node is entered
        double cq[AMAX] = {0.0, 0.0, 0.0, 0.0};
        bool finish = false, do_step = true;
        double delayed = 0;
        if (D.ab_lockstep) {
            // Lock-step waves (FBA_HIST_LOCKSTEP=0 turns them off): the wave's trees start their simulations together -- a tree whose simulation is over
            // waits in mode 3 until every tree of the wave that is still searching is there too.  Sixteen trees in sixteen phases made the wave
            // execute the selection, the particle's consumption and the back-up in nearly every iteration for one or two trees each; in step, the
            // selection runs in the iterations of the descent only, the other two once per simulation.  What the waiting costs is small because the
            // wave's slots have the same depth left (search_order: a rollout runs to the horizon), so their simulations have nearly the same length.
            // Every tree still runs the same simulations in the same order: no result changes.
            const bool waiting = mode == 3;
            if (__builtin_amdgcn_ballot_w64(waiting) == __builtin_amdgcn_ballot_w64(true)) mode = 0;
            else if (waiting) do_step = false;
        }
        if (mode == 0) {
            if (sim >= P.sims) break;
            if (budget > 0 && iter >= budget) break;   // out of iterations at a simulation boundary: park the search (below)
            if (!have_particle) {   // the launch's first simulation (later ones are asked for when their predecessor finishes)
                g.stream(FBA_PHASE_SEARCH, (uint32_t)sim);
                g.ensure(8);
                request_particle();
            }
            have_particle = false;
            const int n4s = *rec_geo;
#pragma unroll
            for (int j = 0; j < H2_PF; ++j) {
                const int k = g.q + HIST_QUAD * j;
                if (k < (n4s & 0xff)) {
                    stage[(4 * k + 0) * HIST_TREES] = pf[j].x;
                    stage[(4 * k + 1) * HIST_TREES] = pf[j].y;
                    stage[(4 * k + 2) * HIST_TREES] = pf[j].z;
                    stage[(4 * k + 3) * HIST_TREES] = pf[j].w;
                }
            }
            if ((n4s & 0xff) > HIST_QUAD * H2_PF) {   // (records of more than 46 entries: the rest in place)
                const uint4* rp = reinterpret_cast<const uint4*>(prec) + __umul24((uint32_t)cur_src, (uint32_t)n4s >> 8);   // (N * Cs / 4 < 2^24)
                for (int k = g.q + HIST_QUAD * H2_PF; k < (n4s & 0xff); k += HIST_QUAD) {
                    const uint4 v = rp[k];
                    stage[(4 * k + 0) * HIST_TREES] = v.x;
                    stage[(4 * k + 1) * HIST_TREES] = v.y;
                    stage[(4 * k + 2) * HIST_TREES] = v.z;
                    stage[(4 * k + 3) * HIST_TREES] = v.w;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the other lanes' pieces (LDS operations of one wave complete in order)
            hist_mask = stage[1 * HIST_TREES];
            sp        = TAB ? stage[0] : (hist_mask >> 16) & 0x3ffu;   // (tabular records: the state index of word 0)
            node = ROOT; dtg = max_tree_depth; plen = 0; mode = 1; pend = false;
        } else if (mode == 1 && pend) {
            // traverseChanceNode's child lookup (POUCT.cpp:224-246), answered by the line requested an iteration ago
            pend = false;
            const uint32_t k0 = quad_get<0>(pf[0].x), k1 = quad_get<0>(pf[1].x);
            const bool v0 = (k0 >> 28) == epoch, v1 = (k1 >> 28) == epoch;
            uint32_t lm = 0, lf = 8;   // lane 3 holds the line's eight keys: is pk among them, and the first free place
            {
                const uint32_t w[8] = {pf[0].x, pf[0].y, pf[0].z, pf[0].w, pf[1].x, pf[1].y, pf[1].z, pf[1].w};
#pragma unroll
                for (int j = 7; j >= 0; --j) {
                    lm |= (w[j] == pk) ? 1u : 0u;
                    lf = ((w[j] >> 28) != epoch) ? (uint32_t)j : lf;
                }
            }
            lm = quad_get<3>(lm);
            lf = quad_get<3>(lf);
            int hit = (k0 == pk) ? 0 : ((k1 == pk) ? 1 : -1);          // the child has a bucket in its home line
            int bucket = (int)(pline * 2u) + max(hit, 0);
            bool is_leaf = false, have_stats = hit >= 0;
            int free_bucket = (!v0) ? (int)(pline * 2u) : ((!v1) ? (int)(pline * 2u) + 1 : -1);
            int free_key    = lf < 8u ? (int)((pline * 2u + (lf >> 2)) * 16u + 12u + (lf & 3u)) : -1;   // word index in the table
            if (hit < 0) {
                const bool nodes_done = free_bucket >= 0;              // a free bucket ends the probe for a node
                const bool keys_done  = lm != 0u || free_key >= 0;     // a match or a free place ends the probe for a key
                is_leaf = lm != 0u;
                if (!(nodes_done && keys_done)) {
                    // the home line is full of other nodes or other keys: walk on, line by line (a few per cent of the lookups at load 1/2)
                    bool need_n = !nodes_done, need_k = !keys_done;
                    uint32_t line = pline;
                    for (uint32_t n = 1; n < nlines && (need_n || need_k); ++n) {
                        line = line + 1u == nlines ? 0u : line + 1u;
                        const uint4* lp = tab + (size_t)line * 8;
                        const uint32_t c0 = lp[0].x, c1 = lp[4].x;
                        const uint4 ka = lp[3], kb = lp[7];
                        if (need_n) {
                            if (c0 == pk || c1 == pk) { hit = c0 == pk ? 0 : 1; bucket = (int)(line * 2u) + hit; need_n = false; need_k = false; is_leaf = false; }
                            else if ((c0 >> 28) != epoch || (c1 >> 28) != epoch) { free_bucket = (int)(line * 2u) + ((c0 >> 28) != epoch ? 0 : 1); need_n = false; }
                        }
                        if (need_k) {
                            const uint32_t w[8] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w};
                            int fj = 8;
                            bool m = false;
#pragma unroll
                            for (int j = 7; j >= 0; --j) {
                                m  = m || w[j] == pk;
                                fj = ((w[j] >> 28) != epoch) ? j : fj;
                            }
                            if (m) { is_leaf = true; need_k = false; }
                            else if (fj < 8) { free_key = (int)((line * 2u + ((uint32_t)fj >> 2)) * 16u + 12u + ((uint32_t)fj & 3u)); need_k = false; }
                        }
                    }
                    if (need_n || need_k) { atomicCAS(D.fault, 0, -(1 + e)); broken = true; }   // the table is full (DeviceState::bkt_lines too small for this tree)
                }
            }
            if (hit >= 0) {          // traverseActionNode of an existing node with statistics
                if (have_stats) {
                    const uint4 mine = hit ? pf[1] : pf[0];   // this lane's piece of the bucket
                    const uint32_t c01 = quad_get<0>(mine.y), c23 = quad_get<0>(mine.z);
                    cn[0] = (int)(c01 & 0xffffu); cn[1] = (int)(c01 >> 16); cn[2] = (int)(c23 & 0xffffu); cn[3] = (int)(c23 >> 16);
                    cq[0] = quad_get_f64<1>(mine.x, mine.y); cq[1] = quad_get_f64<1>(mine.z, mine.w);
                    cq[2] = quad_get_f64<2>(mine.x, mine.y); cq[3] = quad_get_f64<2>(mine.z, mine.w);
                } else {             // found further down the probe sequence: fetch it now
                    const uint4* bp   = tab + (size_t)bucket * 4;
                    const uint4 h     = bp[0];
                    const double2 q01 = *reinterpret_cast<const double2*>(bp + 1);
                    const double2 q23 = *reinterpret_cast<const double2*>(bp + 2);
                    cn[0] = (int)(h.y & 0xffffu); cn[1] = (int)(h.y >> 16); cn[2] = (int)(h.z & 0xffffu); cn[3] = (int)(h.z >> 16);
                    cq[0] = q01.x; cq[1] = q01.y; cq[2] = q23.x; cq[3] = q23.y;
                }
                node = bucket; --dtg;
            } else if (broken) {
                finish = true; do_step = false; plen = 0; sim = P.sims;   // (the host reports the fault; leave the loop)
            } else if (is_leaf) {    // a node that exists and was never reached again: all its statistics are zero; it gets a bucket now
                if (free_bucket < 0) { atomicCAS(D.fault, 0, -(1 + e)); broken = true; finish = true; do_step = false; plen = 0; sim = P.sims; }
                else {
                    uint4* bp = tab + (size_t)free_bucket * 4;
                    if (g.q < 3) bp[g.q] = make_uint4(g.q == 0 ? pk : 0u, 0u, 0u, 0u);   // key + counts, Q's; the bucket's four keys stay
                    node = free_bucket; --dtg;
                }
            } else {                 // no such child: create it, then rollout(depth_to_go - 1)  (POUCT.cpp:236-244)
                if (free_key < 0) { atomicCAS(D.fault, 0, -(1 + e)); broken = true; finish = true; do_step = false; plen = 0; sim = P.sims; }
                else {
                    tabw[free_key] = pk;
                    ++n_nodes;
                    mode = 2; rdepth = dtg - 1; rret = 0; rdisc = 1;
                    if (rdepth == 0) { finish = true; do_step = false; }
                }
            }
        }
        PROF_MARK(0)
        if (mode == 1 && dtg == 0 && !finish) { finish = true; do_step = false; }
        if (mode == 1) tree_depth = max(tree_depth, max_tree_depth - dtg);
        int a = 0, o = 0;
        double r = 0;
        bool term = false;
        if (do_step) {
            // (the action's draw and the six rows': ensured at the end of the previous iteration)
            if (mode == 1) {  // traverseActionNode
                // one selectChanceNodeUCB for the wave, on the root's registers or the bucket's values (two inlined copies would run one after the other)
                const bool at_root = node == ROOT;
                int vis = 0;
#pragma unroll
                for (int a2 = 0; a2 < AMAX; ++a2) {
                    const int rn2 = root_n[a2 * HIST_TREES];
                    const double rq2 = root_q[a2 * HIST_TREES];
                    cn[a2] = at_root ? rn2 : cn[a2];
                    cq[a2] = at_root ? rq2 : cq[a2];
                    vis += cn[a2];    // (ActionNode::_visit_count is the sum of its chance nodes' counts: every back-up through the node adds one to exactly one of them)
                }
                a = ucb_pick<AMAX>(P, g, D.log1p_tab, vis, cn, cq, true);   // (the root's visits are the sum of its counts too: MCTSTreeNodes.cpp:59-62)
                path_n[(size_t)plen * HIST_TREES] = a == 0 ? cn[0] : (a == 1 ? cn[1] : (a == 2 ? cn[2] : cn[3]));   // (unused at the root: its back-up works on the registers)
                path_q[(size_t)plen * HIST_TREES] = a == 0 ? cq[0] : (a == 1 ? cq[1] : (a == 2 ? cq[2] : cq[3]));
            } else {
                a = g.slow_int4();  // GridWorld::generateRandomAction :220-226 (slowRandomInt(0, 4))
            }
#ifdef FBA_PROFILE_SEARCH
        }
        PROF_MARK(1)
        if (do_step) {
#endif
          if constexpr (TAB) {
            // BAPOMDP::step over BAFlatModel (sim_step's tabular branch) on the staged record, the same on the four lanes: T(s, a, .) with the
            // step's first draw, O(a, s', .) with its second.  A rollout never looks at an observation (POUCT.cpp:273-303): its row is not walked,
            // its draw is skipped.
            const uint32_t* listA = stage + (size_t)(2 + hist_offset(hist_cnt, a)) * HIST_TREES;
            const int nA = hist_count(hist_cnt, a), NW = P.gw_N, GW = P.gw_G, s = (int)sp;
            const TabRows T(P);
            const int ns = tab_row_sample<HIST_TREES>(T, s * 4 + a, listA, nA, (uint32_t)s, 0, 10, u01_of(g.at(g.draw)), P.S);
            const bool found = gridworld_on_goal(P, (s / (NW * GW)) * NW + (s / GW) % NW, s % GW);  // terminal and reward from the OLD state
            if (mode == 1) {  // traverseChanceNode
                o    = tab_row_sample<HIST_TREES>(T, 4 * P.S + a * P.S + ns, listA, nA, (uint32_t)ns, 10, 20, u01_of(g.at(g.draw + 1u)), P.O);
                r    = found ? 1 : 0;
                term = found;
                g.draw += 2;
                ++steps;
                sp = (uint32_t)ns;
                path_r[(size_t)plen * HIST_TREES]  = (float)r;
                path_na[(size_t)plen * HIST_TREES] = (node << 5) | a;
                ++plen;
                if (term) finish = true;
                else {   // ask for the child's line; it is looked at when this loop comes round again
                    const uint32_t code = ((uint32_t)node * 4u + (uint32_t)a) * (uint32_t)P.O + (uint32_t)o;
                    pk    = ekey | code;
                    pline = h2_home_line(code, nlines);
                    const uint4* lp = tab + (size_t)pline * 8;
                    pf[0] = lp[g.q];
                    pf[1] = lp[4 + g.q];
                    pend  = true;
                }
            } else {          // a rollout step
                rret += (found ? 1.0 : 0.0) * rdisc;
                rdisc *= P.gamma;
                --rdepth;
                ++steps;
                g.draw += 2;
                sp = (uint32_t)ns;
                if (rdepth == 0 || found) { delayed = rret; finish = true; }
            }
          } else {
            // BAPOMDP::step over BABNModel (BAPOMDP.cpp:111-143, BABNModel.cpp:292-325) as two passes of hist_row_pass.  Pass A: the transition rows
            // of (state, a) for every lane.  Pass B: the observation rows of (a, s') for the trees that are in their tree -- and, for the trees that are
            // in a rollout, the transition rows of the NEXT step: a rollout never looks at an observation (POUCT.cpp:273-303 uses reward and terminal
            // only), so its three observation draws are skipped and the pass the wave executes anyway carries a second simulated step.
            const int f = min(g.q, 2), NW = P.gw_N, GW = P.gw_G, nrow = f == 2 ? GW : NW;
            const HistRowsLds<K> rl{s_rid, s_rows, HistRowIds(P.gw_N, P.gw_G, 4)};
            const HistRowsGlobal rg{P.hist_base, P.hist_alt, s_rows, HL};
            int x = hist_x(sp), y = hist_y(sp), gl = hist_g(sp), cell = x * NW + y;
            const uint32_t* listA = stage + (size_t)(2 + hist_offset(hist_cnt, a)) * HIST_TREES;
            const int nA = hist_count(hist_cnt, a);
            int nv;
            {
                const bool mx = (hist_mask >> (2 * a)) & 1u, my = (hist_mask >> (2 * a + 1)) & 1u;
                const bool with_goal = f == 2 || ((hist_mask >> (2 * a + f)) & 1u);
                const float* rowp = LROWS ? rl.t(a, f, with_goal, cell, gl) : rg.t(a, f, with_goal, cell, gl);
                nv = hist_row_pass<K, HIST_TREES, LROWS>(P, g, listA, nA, sp, false, mx, my, rowp, nrow, f, u01_of(g.at(g.draw + (uint32_t)f)));
            }
            const int nx = quad_bcast(g.addr0, 0, nv), ny = quad_bcast(g.addr0, 1, nv), ng = quad_bcast(g.addr0, 2, nv);
            const bool found = gridworld_on_goal(P, cell, gl);  // GridWorldBAExtension.cpp:74-99: terminal and reward from the OLD state
            const uint32_t spN = hist_pack(nx, ny, ng);
            // what pass B is for this tree
            bool second = false;
            int aB = a, nB = nA;   // (pass B walks the entries of this action: the step's own, or the rollout's next)
            const uint32_t* listB = listA;
            const float* rowB;
            double uB;
            if (mode == 1) {
                const int nvf = f == 0 ? nx : (f == 1 ? ny : ng);
                rowB = LROWS ? rl.o(a, f, nvf) : rg.o(a, f, nvf);
                uB   = u01_of(g.at(g.draw + 3u + (uint32_t)f));
            } else {
                // the rollout's step ends here (its observation would be sampled from draws 3..5 of the step: skipped, never used)
                rret += (found ? 1.0 : 0.0) * rdisc;
                rdisc *= P.gamma;
                --rdepth;
                ++steps;
                g.draw += 6;
                sp = spN;
                rowB = LROWS ? rl.o(a, f, 0) : rg.o(a, f, 0);   // (any row: nothing is counted into it and its draw is dropped)
                uB   = 0.0;
                nB   = 0;
                if (rdepth == 0 || found) { delayed = rret; finish = true; }
                else {   // the next step of the rollout, in this iteration's second pass
                    second = true;
                    g.ensure(4);   // its action and its three transition rows
                    aB = g.slow_int4();
                    x = nx; y = ny; gl = ng; cell = x * NW + y;
                    const bool with_goal = f == 2 || ((hist_mask >> (2 * aB + f)) & 1u);
                    listB = stage + (size_t)(2 + hist_offset(hist_cnt, aB)) * HIST_TREES;
                    nB    = hist_count(hist_cnt, aB);
                    rowB = LROWS ? rl.t(aB, f, with_goal, cell, gl) : rg.t(aB, f, with_goal, cell, gl);
                    uB   = u01_of(g.at(g.draw + (uint32_t)f));
                }
            }
            const int nvB = hist_row_pass<K, HIST_TREES, LROWS>(P, g, listB, nB, spN, mode == 1, (hist_mask >> (2 * aB)) & 1u, (hist_mask >> (2 * aB + 1)) & 1u, rowB, nrow, f, uB);
            const int v0 = quad_bcast(g.addr0, 0, nvB), v1 = quad_bcast(g.addr0, 1, nvB), v2 = quad_bcast(g.addr0, 2, nvB);
            if (mode == 1) {  // traverseChanceNode
                o = (v0 * NW + v1) * GW + v2;
                r = found ? 1 : 0;
                term = found;
                g.draw += 6;
                ++steps;
                sp = spN;
                path_r[(size_t)plen * HIST_TREES]  = (float)r;
                path_na[(size_t)plen * HIST_TREES] = (node << 5) | a;
                ++plen;
                if (term) finish = true;
                else {   // ask for the child's line; it is looked at when this loop comes round again
                    const uint32_t code = ((uint32_t)node * 4u + (uint32_t)a) * (uint32_t)P.O + (uint32_t)o;
                    pk    = ekey | code;
                    pline = h2_home_line(code, nlines);
                    const uint4* lp = tab + (size_t)pline * 8;
                    pf[0] = lp[g.q];
                    pf[1] = lp[4 + g.q];
                    pend  = true;
                }
            } else if (second) {
                const bool found2 = gridworld_on_goal(P, cell, gl);
                rret += (found2 ? 1.0 : 0.0) * rdisc;
                rdisc *= P.gamma;
                --rdepth;
                ++steps;
                g.draw += 6;
                sp = hist_pack(v0, v1, v2);
                if (rdepth == 0 || found2) { delayed = rret; finish = true; }
            }
          }
        }
        PROF_MARK(2)
        PROF_MARK(3)
        if (finish) {
            // back-up, leaf to root (MCTSTreeNodes.cpp:8-12, 59-62).  The returns chain down the path (ret = r + gamma * delayed: two operations
            // per level, every lane); the Q updates -- a division each -- do not depend on one another, so lane j of the quad takes level j
            // (4 + j, ...) and the quad does four at a time.  Count and Q of the chosen action are the descent's (path_n, path_q: nothing else
            // writes this tree), the root's included; level 0 is the root, lane 0 hands its new statistics to the quad's registers.
            double del = delayed;
            for (int k = plen - 1; k >= 0; --k) {
                const double ret = (double)path_r[(size_t)k * HIST_TREES] + P.gamma * del;
                stage[(size_t)(2 * k) * HIST_TREES]     = (uint32_t)__double2loint(ret);   // (the simulation is over: its staged particle is no longer read)
                stage[(size_t)(2 * k + 1) * HIST_TREES] = (uint32_t)__double2hiint(ret);
                del = ret;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int k0 = 0; k0 < plen; k0 += HIST_QUAD) {
                const int k      = min(k0 + g.q, plen - 1);
                const int na     = path_na[(size_t)k * HIST_TREES];
                const double ret = __hiloint2double((int)stage[(size_t)(2 * k + 1) * HIST_TREES], (int)stage[(size_t)(2 * k) * HIST_TREES]);
                const int act    = na & 31;
                const int n      = path_n[(size_t)k * HIST_TREES] + 1;
                const double q0  = path_q[(size_t)k * HIST_TREES];
                const double qn  = q0 + (ret - q0) / (double)n;
                if (k0 + g.q < plen && (na >> 5) != ROOT) {
                    uint32_t* bw = tabw + (size_t)(na >> 5) * 16;
                    reinterpret_cast<uint16_t*>(bw + 1)[act] = (uint16_t)n;
                    reinterpret_cast<double*>(bw + 4)[act]   = qn;
                }
                if (k0 == 0) {   // the root's level is lane 0's
                    const int ract   = (int)quad_get<0>((uint32_t)act), rn = (int)quad_get<0>((uint32_t)n);
                    const double rq  = quad_get_f64<0>((uint32_t)__double2loint(qn), (uint32_t)__double2hiint(qn));
                    root_n[ract * HIST_TREES] = rn;   // (the quad's four lanes store the same values)
                    root_q[ract * HIST_TREES] = rq;
                }
            }
            if (!broken) ++sim;
            mode = D.ab_lockstep ? 3 : 0; pend = false;
        }
        {
            // The one place of the loop where Philox blocks are made: what the next iteration draws -- a step's seven (the action, six rows), or
            // a new simulation's eight on its own stream (the root sample first).  ensure() only prepares blocks: the draws are the same ones.
            const bool new_sim = finish && sim < P.sims;
            if (new_sim) g.stream(FBA_PHASE_SEARCH, (uint32_t)sim);
            g.ensure(new_sim ? 8 : 7);
            if (new_sim) { request_particle(); have_particle = true; }
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
        int32_t* rn = reinterpret_cast<int32_t*>(D.s_root + (size_t)e * 6);
        double* rq  = D.s_root + (size_t)e * 6 + 2;
#pragma unroll
        for (int a = 0; a < AMAX; ++a) { rn[a] = root_n[a * HIST_TREES]; rq[a] = root_q[a * HIST_TREES]; }
        D.s_sim[e]   = sim;
        D.s_nodes[e] = n_nodes;
        D.s_depth[e] = tree_depth;
        if (g.q == 0) D.sim_steps[e] += steps;
        return;   // (search_done[e] stays 0: env_kernel leaves the slot alone)
    }
    if (D.s_sim) D.s_sim[e] = 0;
    if (budget > 0) D.search_done[e] = 1;
    g.stream(FBA_PHASE_SEARCH, (uint32_t)P.sims + 1u);
    g.ensure(1);
    int r_cn[AMAX];
    double r_cq[AMAX];
#pragma unroll
    for (int a = 0; a < AMAX; ++a) { r_cn[a] = root_n[a * HIST_TREES]; r_cq[a] = root_q[a * HIST_TREES]; }
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
