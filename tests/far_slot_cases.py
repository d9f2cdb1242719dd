"""The case table of tests/test_gpu_far_slots.py: one short experiment per way the engine lays out its slots, in so many slots that the
arrays the case names reach past 4 GiB -- past element 2^32 where a context of at most BUDGET bytes can hold that, else past element 2^31,
else past byte 2^32 -- with the oracle's side of it.

Every other oracle comparison of the suite stays within a few megabytes of every array (tests/wide_launch_cases.py: 150 slots), while the
headline context is tens of gigabytes long.  A slot offset computed in 32 bits does not fault there: it wraps into another slot's memory,
and the launch stays fast.  Here runs = E, so slot e executes run e; everything but the slot count is as small as still selects the
family's kernels (fba_launch_plan.h), since neither the search's nor the oracle's cost matters to an offset.  E and E + 1 are no multiples
of 16, as in the wide table.

What a case reaches (`lines`) is asserted twice: without a GPU from the size formulas of the wide table for the particle arrays
(expected_elems: test_the_far_table_covers_what_it_says), and on the GPU from Engine.device_arrays() for every array, tree arrays -- whose
strides only that report shows -- included, together with the reason for settling for less than 2^32 elements: the context scaled to the next
line would not fit BUDGET.

What no context within BUDGET reaches, and where a case therefore settles for less or names less:
  ctot    N / 256 + 2 doubles per slot beside at least 64 bytes per particle: 2^32 bytes of it would stand beside terabytes of particles.
          No case names it.
  p_side  of the tiger importance filter: 4 bytes per particle (planning) beside 56 more -- 2^32 bytes need 64 GB; the BA table model's
          filter (164 bytes per particle with packed records) brings none of p_weight (44 GB), wscan (88 GB), p_side (58 GB) that far.
          So the tiger importance case is the planning one, whose p_weight, wscan and p_rec do cross; p_side crosses on history records.
  hash    reaches 2^32 bytes, not 2^31 elements (16-byte elements: 2^31 of them are 34 GB beside 103 GB of node records).
  mh_scratch, p_rec_sh  no case: the table has one case per slot layout, and these are laid out as p_rec_fc and p_side are.
History records under the plain rejection filter stand at 2^32 bytes for their run time, not for memory: see REJECTION_TAIL below.

Seconds per case, measured: see SECONDS below (oracle: the sampled single runs on one CPU core; GPU: near and far context together)."""
import wide_launch_cases as W
from wide_launch_cases import FACT, IS, POMDP, REJ, TABLE

BUDGET = 40 * 10 ** 9          # bytes of one context, summed from Engine.device_arrays()
NEAR = 150                     # slots of the context whose arrays stay in the region the wide table pins to the oracle
ELEMS32, ELEMS31, BYTES32 = "2^32 elements", "2^31 elements", "2^32 bytes"
RANDOM_RUNS = 4                # runs drawn with the case's seed beside the boundary slots

CASES = []


def far(name, domain, model, belief, fmt, E, lines, env=None, ncnt=0, slow="", **kw):
    """lines: {array: the line it crosses}; ncnt: fba_counts_len where the record is dense (the size formulas need it without a GPU);
    slow: why a case stands at a line that memory would let it pass (the test then does not assert that the budget holds no more)"""
    c = W.case("far_" + name, domain, model, belief, fmt, E=E, runs=E, env=env, **kw)
    c.update(lines=lines, ncnt=ncnt, slow=slow)
    CASES.append(c)


NO_COMPACT_ENV = {"FBA_NO_COMPACT": "1"}

# C2: packed 64-byte records, 16-byte compact records between updates (reject_tiger_once_kernel).  2 * E * 4096 * 16 words: 2^32 words
# at E = 32768, 17.2 GB
far("bapomdp_tiger_compact", "episodic-tiger", TABLE, REJ, "packed_tiger", 32771, {"p_rec": ELEMS32}, particles=4096, horizon=6, seed=5101)
# the same records below TIGER_ONCE_MIN_N = 3584 particles: reject_tiger_lds_kernel, never compact.  2 * E * 3072 * 16 words, 17.2 GB
far("bapomdp_tiger_lds", "episodic-tiger", TABLE, REJ, "packed_tiger", 43691, {"p_rec": ELEMS32}, env=NO_COMPACT_ENV, particles=3072,
    horizon=6, seed=5102)
# the tiger importance filter with weights and prefix sums in HBM (N > IS_LDS_MAX_N): 60 bytes per particle, 32.2 GB.  wscan is E * N
# doubles: 2^32 bytes; 2^31 of them would take 129 GB.  p_weight is twice that: 2^30 doubles.  p_rec: 2 * E * N * 4 words
far("planning_tiger_importance", "episodic-tiger", POMDP, IS, "dense", 32771, {"p_weight": BYTES32, "wscan": BYTES32, "p_rec": ELEMS32},
    particles=16384, horizon=6, seed=5103)
# the BA table model's importance filter on packed 64-byte records (importance_kernel<false, 2, false, true>): of its arrays only p_rec
# crosses (above), 2 * E * 4096 * 16 words in a context of 22 GB
far("bapomdp_tiger_packed_importance", "episodic-tiger", TABLE, IS, "packed_tiger", 32771, {"p_rec": ELEMS32}, particles=4096, horizon=6,
    seed=5115)
# search_kernel's node records without the episodic node cap: 16 386 records of 16 words per slot.  (One step per run: the near context
# runs E / 150 = 110 rounds of 16 384 simulations per lane, 10.8 s at two steps)
far("planning_continuous_tiger_nodes", "continuous-tiger", POMDP, REJ, "dense", 16387, {"nodes": ELEMS32}, particles=64, sims=16384,
    horizon=1, seed=5104)
# the hashed child table: E * 4098 node records of 12 words, E * 8192 entries of 8 bytes.  FBA_NODE_BOUND, not sims, sets the 4098 records
# and with them the table's capacity: 4096 simulations of depth 1 took the near context 12 s and built trees of one level, 64 of depth 6
# probe and fill the table through six levels
far("planning_gridworld5_hashed_children", "gridworld", POMDP, IS, "dense", 87339, {"nodes": ELEMS32, "hash": BYTES32},
    env={"FBA_NODE_BOUND": "4098"}, size=5, particles=64, horizon=6, seed=5105)
# C3: packed factored-tiger records of 36 words (reject_kernel): 2 * E * 4096 * 36 words, 17.2 GB
far("fbapomdp_factored_tiger3_packed", "episodic-factored-tiger", FACT, REJ, "packed_ftiger", 14565, {"p_rec": ELEMS32}, size=3,
    structure_prior=2, particles=4096, horizon=6, seed=5106)
# the same domain under -B reinvigoration: dense records of 72 words (69 counts and parent-set words, the state) in two filters,
# 2 * E * 4096 * 72 words each, 34.4 GB together
far("fbapomdp_factored_tiger3_reinvigoration", "episodic-factored-tiger", FACT, "reinvigoration", "dense", 7283,
    {"p_rec_fc": ELEMS32, "p_rec": ELEMS32}, ncnt=69, size=3, structure_prior=2, resample_amount=8, particles=4096, horizon=6, seed=5107)
# the bucket tree in lock-step order over all E slots.  tree_buckets, not sims, makes the table long (8192 buckets = 4096 lines of 128
# bytes = 32 768 16-byte elements per slot): keys are hashed over the whole table, so 64 simulations reach every part of a slot's block.
# 2^31 elements at 34.4 GB; 2^32 would take 69 GB
far("fbapomdp_gridworld3_bucket_tree", "gridworld", FACT, IS, "history", 65539, {"bkt": ELEMS31}, size=3, particles=64, structure_prior=2,
    horizon=7, episodes=1, tree_buckets=8192, seed=5108)
# history records behind rec_buf, the scratch pool, for_each_chunk over 33 chunks of 1024 slots, the seven launches per update.  One
# episode of three steps, the fewest that keep the record at 8 words (at 4 words the context would take 51 GB); two episodes took 30 s.
# 64 bytes per particle: E * N * 8 words of p_rec, E * N * 2 of p_side (2^32 bytes; 2^31 elements: 69 GB), E * N doubles of wscan
far("fbapomdp_gridworld3_history_importance", "gridworld", FACT, IS, "history", 32771, {"p_rec": ELEMS32, "p_side": BYTES32, "wscan": BYTES32},
    size=3, particles=16384, structure_prior=2, sims=8, horizon=3, episodes=1, seed=5109)
# tabular history records under the same filter (search_tabhist_kernel, is_multi_tab_step_kernel).  8192 particles in twice the slots: the
# oracle needs half a second per run of this filter at 8192.  The tabular step reads the prior's sparse rows from L2 and is the slowest
# of the importance steps: the near context takes 30 s, and no shorter experiment keeps the record at 8 words (above)
far("bapomdp_gridworld3_table_history_importance", "gridworld", TABLE, IS, "history", 65539, {"p_rec": ELEMS32, "p_side": BYTES32, "wscan": BYTES32},
    size=3, particles=8192, sims=8, horizon=3, episodes=1, seed=5111)
# The same records under plain rejection: hist2_flat_search and reject_hist_kernel; search_tabhist_kernel's flat root sample and
# reject_tab_hist_kernel.  TIME, not memory, sets their line.  An update needs N / P(observation | filter) attempts, 256 at a time by one
# workgroup, and in gridworld that probability has three levels even at the first step of a run (both coordinates read right, one wrong,
# both wrong): of 300 oracle runs half need 4 attempts per particle, a tenth 65, one in a hundred about 1000; the prior's noise and
# total do not move it.  A tick of the near context waits for the slowest of its 150 slots -- 1000 N attempts two ticks out of
# three -- E / 150 ticks in a row, and a far tick for the slowest of every chunk of 1024: the cost is that of E * N, whatever the split.
# At 2^32 elements (E * N = 2^30: 131 075 slots of 8192 particles, one step per run) both contexts ran past 150 s.  So these two stand
# below it, at one step per run.  At 2^32 bytes of four-word records (E * N = 2^28) the factored case took 20 s and the tabular one,
# whose step reads sparse rows from L2, 42 s, of which the near context took 16 and 33.  The tabular case stays there; the factored one
# stands at 2^31 elements (E * N = 2^29) for about the same time.  `slow` says so where the other cases show that memory holds no more
REJECTION_TAIL = "the attempts of a rejection update on gridworld have a tail of 1000 per particle: 2^32 elements ran past 150 s"
far("fbapomdp_gridworld3_history_rejection", "gridworld", FACT, REJ, "history", 131075, {"p_rec": ELEMS31}, slow=REJECTION_TAIL, size=3,
    particles=4096, structure_prior=2, sims=8, horizon=1, episodes=1, seed=5110)
far("bapomdp_gridworld3_table_history_rejection", "gridworld", TABLE, REJ, "history", 131075, {"p_rec": BYTES32}, slow=REJECTION_TAIL, size=3,
    particles=2048, sims=8, horizon=1, episodes=1, seed=5114)
# collision-avoidance history records, the multi-launch filter walking chunks of slots: 64 bytes per particle, 34.9 GB.  p_weight is
# 2 * E * N doubles: 2^33 bytes, 2^30 elements (2^31: 69 GB)
far("fbapomdp_collision_avoidance_history", "random-collision-avoidance", FACT, IS, "history", 32771, {"p_rec": ELEMS32, "p_weight": BYTES32},
    env=W.MULTI_ENV, particles=16384, sims=8, episodes=1, **W.CA431, seed=5112)
# the nested belief: 2 * E * 32 * 32^2 states
far("bapomdp_nested", "episodic-tiger", TABLE, "nested", "dense", 65539, {"nest_s": ELEMS32}, ncnt=24, particles=32, sims=16, horizon=4,
    episodes=1, seed=5113)

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# measured seconds per case: (the oracle's twelve single runs, on a CPU without a GPU; the whole test on the GPU, of which the near
# context is the larger part: E / 150 rounds of lock-step ticks against one)
SECONDS = {
    "far_bapomdp_tiger_compact": (0.05, 1.4), "far_bapomdp_tiger_lds": (0.03, 1.5), "far_planning_tiger_importance": (0.06, 1.1),
    "far_planning_continuous_tiger_nodes": (0.02, 4.1), "far_planning_gridworld5_hashed_children": (0.01, 5.4),
    "far_fbapomdp_factored_tiger3_packed": (0.12, 1.4), "far_fbapomdp_factored_tiger3_reinvigoration": (0.18, 1.8),
    "far_fbapomdp_gridworld3_bucket_tree": (0.03, 4.4), "far_fbapomdp_gridworld3_history_importance": (5.5, 12.8),
    "far_fbapomdp_collision_avoidance_history": (0.87, 3.2), "far_bapomdp_nested": (0.05, 4.9),
    "far_bapomdp_tiger_packed_importance": (0.08, 3.7), "far_bapomdp_gridworld3_table_history_importance": (12.6, 44.0),
    "far_fbapomdp_gridworld3_history_rejection": (1.9, 38.2), "far_bapomdp_gridworld3_table_history_rejection": (1.66, 41.7),
}
assert set(SECONDS) == set(BY_NAME)


def record_words(c):
    """32-bit words of one particle record, from the wide table's formulas"""
    return W.expected_particle_bytes(c, c["ncnt"]) // 4


def expected_elems(c, array):
    """Elements of a particle array as fba_create allocates it, or None for an array whose stride only Engine.device_arrays() shows"""
    E, N, cs = c["E"], c["kw"]["particles"], record_words(c)
    hist = c["fmt"] == "history"
    side_w = 2 if hist else 1 + {POMDP: 0, TABLE: 2}.get(c["model"], 0)
    return {"p_rec": (E + min(E, 1024) if hist else 2 * E) * N * cs, "p_rec_fc": 2 * E * N * cs, "p_weight": 2 * E * N, "wscan": E * N,
            "p_side": E * N * side_w if c["model"] != FACT or hist else None, "nest_s": 2 * E * N * N * N}.get(array)


ELEM_BYTES = {"p_rec": 4, "p_rec_fc": 4, "p_weight": 8, "wscan": 8, "p_side": 4, "nest_s": 4}


def crosses(line, elems, elem_bytes):
    return elems * elem_bytes > 2 ** 32 and (line == BYTES32 or elems > (2 ** 32 if line == ELEMS32 else 2 ** 31))


def boundary_slots(E, elems, slot_elems, buffers, elem_bytes):
    """the slots whose block holds element 2^31, element 2^32 and byte 2^32 of an array, and their neighbours: within the first buffer the
    block number is the slot, behind it the buf * E term comes off"""
    out = set()
    for B in (2 ** 31, 2 ** 32, 2 ** 32 // elem_bytes):
        if B < elems and slot_elems and B // slot_elems < buffers * E:
            slot = (B // slot_elems) % E
            out.update(s for s in (slot - 1, slot, slot + 1) if 0 <= s < E)
    return out
