"""The case table of tests/test_launch_plan_cpu.py: which kernels the tick launchers (launch_search, launch_belief_update, launch_reset) launch
for a Problem / DeviceState, with what grid, block and dynamic LDS, and which LDS limits they raise first.

A case is a set of field values -- synthetic ones, not necessarily a context fba_create can make -- and the launchers it is handed to;
tests/launch_capture.cpp calls the real launchers on them with the launch macros redirected, so nothing needs a GPU.  There is a case on
each side of every condition the launchers test, at the smallest values that reach it.

The expected side, tests/golden/launch_plan_expected.jsonl, was recorded by scripts/record_launch_plan.py from the launchers of the commit
before the launch decisions were gathered in fba_launch_plan.h (b672baa) and is compared without tolerance.  As for
tests/create_plan_cases.py, a record comes from a commit whose launchers are trusted, never from the code under test: a change that means
to move some configurations to another kernel re-records those cases only, and its diff of the golden file shows which they are."""
import json
import os
import subprocess

import fba_pomdp_amd._native as N

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "launch_plan_expected.jsonl")
POMDP, TABLE, FACT = N.MODEL_POMDP, N.MODEL_BA_TABLE, N.MODEL_BA_FACTORED
REJ, IS = N.BELIEF_REJECTION, N.BELIEF_IMPORTANCE
POUCT, RANDOM, TS = N.PLANNER_POUCT, N.PLANNER_RANDOM, N.PLANNER_TS
TIGER, CTIGER, FTIGER, CFTIGER = N.DOM_TIGER_EPISODIC, N.DOM_TIGER_CONTINUOUS, N.DOM_FTIGER_EPISODIC, N.DOM_FTIGER_CONTINUOUS
GRID, CA, SYS, AGR = N.DOM_GRIDWORLD, N.DOM_COLLISION_AVOID, N.DOM_SYSADMIN_INDEPENDENT, N.DOM_AGR
# fba_kernels.h
TIGER_ONCE_MIN_N, TIGER_LDS_MAX_N, IS_LDS_MAX_N, SEARCH_STAGE_WORDS, MH_LDS_HEAD = 3584, 4096, 8192, 128, 1024 * 8 + 2 * 128 * 4 + 64 * 4

CASES = []


def add(name, launchers, *parts, **fields):
    """launchers: a string of s (launch_search), u (launch_belief_update), r (launch_reset); parts: dicts of fields, later ones win;
    a field is written P_x or D_x"""
    merged = {}
    for p in parts:
        merged.update(p)
    merged.update(fields)
    assert all(k[:2] in ("P_", "D_") for k in merged), merged
    CASES.append(dict(name=name, launchers=launchers, fields=merged))


tiger = dict(P_model=TABLE, P_domain=TIGER, P_planner=POUCT, P_belief=REJ, P_S=2, P_A=3, P_O=2, P_C=24, P_Cs=32, P_N=64, P_E=100, P_sims=64,
             P_max_depth=10, P_horizon=10, D_max_nodes=66)
packed = dict(P_packed=1, P_C=12, P_Cs=16)
tiger_pomdp = dict(tiger, P_model=POMDP, P_C=0, P_Cs=4)
ftiger = dict(tiger, P_model=FACT, P_domain=FTIGER, P_S=8, P_C=70, P_Cs=72, P_fd_bytes=904)
ft_packed = dict(P_ft_packed=1, P_C=35, P_Cs=36)
sysadmin = dict(P_model=FACT, P_domain=SYS, P_planner=POUCT, P_belief=REJ, P_S=8, P_A=4, P_O=8, P_C=100, P_Cs=104, P_N=64, P_E=100, P_sims=64,
                P_max_depth=10, P_horizon=10, P_fd_bytes=904, D_max_nodes=66)
grid_hist = dict(P_model=FACT, P_domain=GRID, P_planner=POUCT, P_belief=IS, P_S=27, P_A=4, P_O=27, P_C=0, P_Cs=12, P_N=64, P_E=100, P_sims=64,
                 P_max_depth=10, P_horizon=10, P_hist=1, P_hist_cap=10, P_hist_row=3, P_hist_rid_bytes=1024, P_hist_distinct=32, P_gw_N=3,
                 P_gw_G=1, D_max_nodes=66)
grid_tab = dict(grid_hist, P_model=TABLE, P_hist=2, P_hist_lds=0)
ca_hist = dict(grid_hist, P_domain=CA, P_hist=3, P_hist_row=200, P_hist_rid_bytes=208, P_hist_distinct=16, P_A=3, P_hist_lds=1, D_is_multi=1)
chunks = dict(D_single_rec=1, D_scratch_slots=3, P_E=8)       # 3 + 3 + 2 slots
one_chunk = dict(D_single_rec=1, D_scratch_slots=8, P_E=8)
wide_pool = dict(D_single_rec=1, D_scratch_slots=16, P_E=8)

# ---- tiger rejection filters
for form, rec in (("dense", {}), ("packed", packed)):
    for n in (TIGER_ONCE_MIN_N - 1, TIGER_ONCE_MIN_N, TIGER_LDS_MAX_N, TIGER_LDS_MAX_N + 1):
        for gather in (0, 1):
            add(f"reject_tiger_{form}_{n}" + ("_gather" if gather else ""), "ur", tiger, rec, P_N=n, D_ab_tiger_gather=gather)
add("reject_tiger_regular", "ur", tiger, P_N=TIGER_ONCE_MIN_N, P_dirichlet_regular=1)
add("reject_tiger_packed_regular", "u", tiger, packed, P_N=TIGER_ONCE_MIN_N, P_dirichlet_regular=1)
add("reject_ctiger_packed", "u", tiger, packed, P_N=TIGER_ONCE_MIN_N, P_domain=CTIGER)
add("reject_tiger_packed_random_planner", "u", tiger, packed, P_N=TIGER_ONCE_MIN_N, P_planner=RANDOM)
add("reject_tiger_pomdp", "ur", tiger_pomdp)
add("reject_sysadmin", "ur", sysadmin)
add("reject_sysadmin_regular", "u", sysadmin, P_dirichlet_regular=1)
add("reject_sysadmin_table", "u", sysadmin, P_model=TABLE)

# ---- importance filters
for form, rec in (("dense", {}), ("packed", packed)):
    for n in (IS_LDS_MAX_N, IS_LDS_MAX_N + 1):
        for multi in (0, 1):
            add(f"importance_tiger_{form}_{n}_multi{multi}", "ur", tiger, rec, P_belief=IS, P_N=n, D_is_multi=multi)
add("importance_tiger_small", "u", tiger, P_belief=IS, P_N=2048)           # at most 16 KB of LDS: no limit to raise
add("importance_tiger_2049", "u", tiger, P_belief=IS, P_N=2049)
add("importance_tiger_regular", "u", tiger, P_belief=IS, P_N=IS_LDS_MAX_N, P_dirichlet_regular=1)
add("importance_tiger_regular_multi", "u", tiger, P_belief=IS, P_N=IS_LDS_MAX_N, P_dirichlet_regular=1, D_is_multi=1)
add("importance_sysadmin", "u", sysadmin, P_belief=IS, P_N=IS_LDS_MAX_N)
add("importance_sysadmin_above_lds", "u", sysadmin, P_belief=IS, P_N=IS_LDS_MAX_N + 1)
add("importance_ftiger", "u", ftiger, P_belief=IS)
for multi in (0, 1):
    for n in (IS_LDS_MAX_N, IS_LDS_MAX_N + 1, 16384, 16385):
        add(f"importance_grid_hist_{n}_multi{multi}", "ur", grid_hist, P_N=n, D_is_multi=multi)
    for row in (8, 9, 10, 11):
        for lds in (0, 1):
            add(f"importance_grid_hist_row{row}_lds{lds}_multi{multi}", "u", grid_hist, P_hist_row=row, P_hist_lds=lds, D_is_multi=multi)
    add(f"importance_grid_hist_rows_hbm_multi{multi}", "u", grid_hist, P_hist_lds=1, D_ab_rows_hbm=1, D_is_multi=multi)
    add(f"importance_grid_tab_multi{multi}", "ur", grid_tab, D_is_multi=multi)
    add(f"importance_ca_hist_multi{multi}", "ur", ca_hist, D_is_multi=multi)

# ---- chunked launches (DeviceState::single_rec)
for pool_name, pool in (("chunks", chunks), ("one_chunk", one_chunk), ("wide_pool", wide_pool)):
    add(f"importance_grid_hist_{pool_name}", "ur", grid_hist, pool)
    add(f"importance_grid_tab_{pool_name}", "ur", grid_tab, pool)
    add(f"importance_ca_hist_{pool_name}", "ur", ca_hist, pool)
    add(f"reject_grid_hist_{pool_name}", "ur", grid_hist, pool, P_belief=REJ)
    add(f"reject_grid_tab_{pool_name}", "ur", grid_tab, pool, P_belief=REJ)
for n in (4095, 4096):
    for forced in (0, 1, 2):     # FBA_HIST_MULTI: by the particle count, never, always
        add(f"importance_grid_hist_chunks_{n}_hist_multi{forced}", "u", grid_hist, chunks, P_N=n, D_ab_hist_multi=forced)
add("importance_grid_hist_4096_unchunked", "u", grid_hist, P_N=4096)
add("importance_grid_hist_chunks_is_multi", "u", grid_hist, chunks, D_is_multi=1)
for row in (8, 9, 10, 11):
    for lds in (0, 1):
        add(f"reject_grid_hist_row{row}_lds{lds}", "u", grid_hist, P_belief=REJ, P_hist_row=row, P_hist_lds=lds)
add("reject_grid_hist_rows_hbm", "u", grid_hist, P_belief=REJ, P_hist_lds=1, D_ab_rows_hbm=1)
add("reject_grid_tab", "ur", grid_tab, P_belief=REJ)

# ---- composite beliefs
for reg in (0, 1):
    tag = "_regular" if reg else ""
    add("reinvigoration" + tag, "ur", ftiger, P_reinvig=2, P_dirichlet_regular=reg)
    add("incubator" + tag, "ur", ftiger, P_incub=2, P_dirichlet_regular=reg)
    add("cheating" + tag, "ur", ftiger, P_belief=IS, P_cheat=2, P_dirichlet_regular=reg)
    add("nested" + tag, "ur", tiger, P_belief=IS, P_nested=16, P_N=4, P_dirichlet_regular=reg)
add("incubator_8192", "u", ftiger, P_incub=2, P_N=IS_LDS_MAX_N)
add("reinvigoration_packed_tiger", "u", tiger, packed, P_reinvig=2, P_N=TIGER_LDS_MAX_N)
add("mh_scratch_in_lds", "ur", ftiger, P_belief=IS, P_mh=1, D_mh_scratch_words=(64 * 1024 - MH_LDS_HEAD) // 4)
add("mh_scratch_in_hbm", "u", ftiger, P_belief=IS, P_mh=1, D_mh_scratch_words=(64 * 1024 - MH_LDS_HEAD) // 4 + 1)
add("mh_multi", "u", ftiger, P_belief=IS, P_mh=1, D_is_multi=1)
add("cheating_multi", "u", ftiger, P_belief=IS, P_cheat=2, D_is_multi=1)

# ---- factored tiger
for s in (2, 4, 8, 16, 32, 64):
    add(f"ftiger_dense_S{s}", "su", ftiger, P_S=s)
    add(f"ftiger_packed_S{s}", "su", ftiger, ft_packed, P_S=s)
add("ftiger_dense_regular", "su", ftiger, P_dirichlet_regular=1)
add("ftiger_continuous_packed", "su", ftiger, ft_packed, P_domain=CFTIGER)
add("ftiger_table", "su", ftiger, P_model=TABLE)
add("ftiger_dense_unstaged", "s", ftiger, P_Cs=SEARCH_STAGE_WORDS + 4)
add("ftiger_random_planner", "s", ftiger, ft_packed, P_planner=RANDOM)
add("ftiger_hash", "s", ftiger, ft_packed, D_hash=1)

# ---- search: the tiger variants and the ETIGER tree layout, through every term of etiger_ok
for fam_name, fam in (("tiger_dense", tiger), ("tiger_packed", dict(tiger, **packed)), ("tiger_pomdp", tiger_pomdp),
                      ("ftiger_packed", dict(ftiger, **ft_packed))):
    add(f"search_{fam_name}", "s", fam)
    add(f"search_{fam_name}_no_etiger", "s", fam, D_ab_no_etiger=1)
    add(f"search_{fam_name}_continuous", "s", fam, P_domain=CFTIGER if fam["P_domain"] == FTIGER else CTIGER)
    add(f"search_{fam_name}_A4", "s", fam, P_A=4)
    add(f"search_{fam_name}_O3", "s", fam, P_O=3)
    add(f"search_{fam_name}_65535_sims", "s", fam, P_sims=65535)
    add(f"search_{fam_name}_65536_sims", "s", fam, P_sims=65536)
    add(f"search_{fam_name}_4093_nodes", "s", fam, D_max_nodes=4093)
    add(f"search_{fam_name}_4094_nodes", "s", fam, D_max_nodes=4094)
    add(f"search_{fam_name}_hash", "s", fam, D_hash=1)
    add(f"search_{fam_name}_random_planner", "s", fam, P_planner=RANDOM)
    add(f"search_{fam_name}_ts_planner", "s", fam, P_planner=TS)
    add(f"search_{fam_name}_regular", "s", fam, P_dirichlet_regular=1)
    add(f"search_{fam_name}_no_depth", "s", fam, P_max_depth=0)
    add(f"search_{fam_name}_odd_depth", "s", fam, P_max_depth=7)
add("search_tiger_dense_stage_words", "s", tiger, P_Cs=SEARCH_STAGE_WORDS)
add("search_tiger_dense_above_stage_words", "s", tiger, P_Cs=SEARCH_STAGE_WORDS + 4)
add("search_tiger_root_children_32768_nodes", "s", tiger, D_ab_no_etiger=1, D_max_nodes=32768)

# ---- search: the general instantiations by action count, model, staging and Dirichlet form
for a in (4, 5, 8, 9, 16):
    for model_name, model in (("table", TABLE), ("fact", FACT)):
        for reg in (0, 1):
            for cs in (SEARCH_STAGE_WORDS, SEARCH_STAGE_WORDS + 4):
                add(f"search_sysadmin_{model_name}_A{a}_Cs{cs}" + ("_regular" if reg else ""), "s", sysadmin, P_model=model, P_A=a, P_Cs=cs,
                    P_dirichlet_regular=reg)
    add(f"search_pomdp_A{a}", "s", sysadmin, P_model=POMDP, P_A=a, P_Cs=4)
    add(f"search_pomdp_A{a}_regular", "s", sysadmin, P_model=POMDP, P_A=a, P_Cs=4, P_dirichlet_regular=1)
add("search_pomdp_A17", "s", sysadmin, P_model=POMDP, P_domain=AGR, P_A=17, P_Cs=4)
add("search_pomdp_A23_hash", "s", sysadmin, P_model=POMDP, P_domain=AGR, P_A=23, P_O=441, P_Cs=4, D_hash=1)
add("search_sysadmin_root_children", "s", sysadmin, P_A=4, P_O=2)
add("search_sysadmin_65_slots", "s", sysadmin, P_E=65)
add("search_sysadmin_64_slots", "s", sysadmin, P_E=64)

# ---- search: history records
bucket = dict(D_bkt=1, D_ab_lockstep=1)
add("search_ca_hist", "s", ca_hist)
add("search_ca_hist_deep", "s", ca_hist, P_max_depth=40, P_Cs=84)
for row in (8, 9, 10, 11):
    add(f"search_grid_hist_records_row{row}", "s", grid_hist, P_hist_row=row)
    for belief_name, belief in (("importance", IS), ("rejection", REJ)):
        for lds in (0, 1):
            add(f"search_grid_hist_bucket_{belief_name}_row{row}_lds{lds}", "s", grid_hist, bucket, P_belief=belief, P_hist_row=row, P_hist_lds=lds)
add("search_grid_hist_bucket_rows_hbm", "s", grid_hist, bucket, P_hist_lds=1, D_ab_rows_hbm=1)
add("search_grid_hist_bucket_no_lockstep", "s", grid_hist, bucket, D_ab_lockstep=0)
add("search_grid_hist_records_budget", "s", grid_hist, P_search_budget=16)
add("search_grid_hist_records_17_slots", "s", grid_hist, P_E=17)
add("search_grid_tab_records", "s", grid_tab)
for belief_name, belief in (("importance", IS), ("rejection", REJ)):
    add(f"search_grid_tab_bucket_{belief_name}", "s", grid_tab, bucket, P_belief=belief)
    add(f"search_grid_tab_bucket_{belief_name}_no_lockstep", "s", grid_tab, bucket, P_belief=belief, D_ab_lockstep=0)
    for depth in (36, 37, 72, 73, 144, 145):     # 4 -> 2 -> 1 waves per workgroup, then one wave past 64 KB: 448 bytes per level + 896 per wave
        add(f"search_grid_tab_bucket_{belief_name}_depth{depth}", "s", grid_tab, bucket, P_belief=belief, P_max_depth=depth)
for belief_name, belief in (("importance", IS), ("rejection", REJ)):
    # (the halvings themselves: 4 * (448 * 34 + 896) = 64512 <= 64 KB < 4 * (448 * 35 + 896), 2 * (448 * 71 + 896) = 65408 <= 64 KB < 2 * (448 * 72 + 896);
    #  36 | 37 and 72 | 73 above stand on one side each)
    for depth in (34, 35, 71):
        add(f"search_grid_tab_bucket_{belief_name}_depth{depth}", "s", grid_tab, bucket, P_belief=belief, P_max_depth=depth)
for lds in (0, 1):
    for depth in (30, 40, 70, 80, 140, 150):
        add(f"search_grid_hist_bucket_lds{lds}_depth{depth}", "s", grid_hist, bucket, P_hist_lds=lds, P_max_depth=depth)
add("search_grid_hist_bucket_long_record", "s", grid_hist, bucket, P_Cs=64)
add("search_grid_hist_bucket_65_slots", "s", grid_hist, bucket, P_E=65)

# ---- launch_reset beyond the cases above
add("reset_nested_chunked", "r", tiger, chunks, P_belief=IS, P_nested=16, P_N=4)
add("reset_importance_4097", "r", sysadmin, P_belief=IS, P_N=4097)
add("reset_reject_grid_hist_4097", "r", grid_hist, P_belief=REJ, P_N=4097)
add("reset_cheating_chunked", "r", grid_hist, chunks, P_cheat=2)

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def build_capture(exe, csrc=None, include=None):
    """tests/launch_capture.cpp against the launchers under csrc (this tree's unless told otherwise).  The launchers' translation units come
    with their kernels, which are compiled and never run; -O0 keeps that short."""
    csrc = csrc or os.path.join(N.HERE, "csrc")
    include = include or os.path.join(N.ROOT, "include")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O0", "-std=c++17", "-w", "-I" + include, "-I" + csrc,
                           os.path.join(HERE, "launch_capture.cpp"), "-o", str(exe)])


def capture(exe, cases=None):
    """name -> what the launchers did for the case"""
    text = "".join("%s %s %s\n" % (c["name"], c["launchers"], " ".join(f"{k[0]}.{k[2:]}={v}" for k, v in c["fields"].items()))
                   for c in (CASES if cases is None else cases))
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return read_records(r.stdout.splitlines())


def read_records(lines):
    table = {}
    for line in lines:
        rec = json.loads(line)
        table[rec.pop("name")] = rec
    return table


def expected():
    with open(GOLDEN) as f:
        return read_records(f)
