// search_quorum_plan.cpp -- which boundary quorum search_plan gives a launch, and how FBA_SEARCH_QUORUM is read, without a GPU
// (tests/test_search_quorum_plan_cpu.py).  fba_launch_plan.h is pure host code; nothing is launched.
//
// stdin: one line per case.  "plan name field=value ...": fields as in tests/launch_capture.cpp (P.x / D.x; a pointer field takes 0 or 1;
// unnamed fields are zero, but S = E = 1), and D.search_quorum.  "switch name [text]": the value of the environment variable, absent = unset.
// stdout: "plan name <kernel as search_plan names it, the template arguments of search_kernel or 'other'> <quorum>" / "switch name <value>".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fba_launch_plan.h"

#define FIELDS(X)                                                                                                                          \
    X(P, model) X(P, domain) X(P, planner) X(P, belief) X(P, dirichlet_regular) X(P, N) X(P, E) X(P, S) X(P, A) X(P, O) X(P, C) X(P, Cs)     \
    X(P, packed) X(P, ft_packed) X(P, hist) X(P, hist_row) X(P, hist_rid_bytes) X(P, hist_distinct) X(P, hist_cap) X(P, nested)            \
    X(P, reinvig) X(P, incub) X(P, cheat) X(P, mh) X(P, point) X(P, max_depth) X(P, sims) X(P, horizon) X(P, fd_bytes) X(P, gw_N)           \
    X(P, gw_G) X(P, search_budget) X(D, single_rec) X(D, scratch_slots) X(D, is_multi) X(D, ab_rows_hbm) X(D, ab_hist_multi)              \
    X(D, ab_no_etiger) X(D, ab_tiger_gather) X(D, ab_lockstep) X(D, max_nodes) X(D, mh_scratch_words) X(D, hmask) X(D, search_quorum)
#define POINTERS(X) X(P, hist_lds) X(D, hash) X(D, bkt)

static bool set_field(fba::Problem& P, fba::DeviceState& D, const char* key, long v)
{
    static uint4 dummy[8];   // (what a set pointer points at; never read)
#define X(S, F) if (!strcmp(key, #S "." #F)) { S.F = (decltype(S.F))v; return true; }
    FIELDS(X)
#undef X
#define X(S, F) if (!strcmp(key, #S "." #F)) { S.F = v ? reinterpret_cast<decltype(S.F)>(dummy) : nullptr; return true; }
    POINTERS(X)
#undef X
    return false;
}

int main()
{
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        char* save = nullptr;
        const char* what = strtok_r(line, " \n", &save);
        const char* name = strtok_r(nullptr, " \n", &save);
        if (!what || !name) continue;
        if (!strcmp(what, "switch")) {
            printf("switch %s %d\n", name, fba::search_quorum_switch(strtok_r(nullptr, "\n", &save)));
            continue;
        }
        fba::Problem P{};
        fba::DeviceState D{};
        P.S = P.E = 1;
        for (char* tok; (tok = strtok_r(nullptr, " \n", &save));) {
            char* eq = strchr(tok, '=');
            if (!eq) return 2;
            *eq = 0;
            if (!set_field(P, D, tok, strtol(eq + 1, nullptr, 0))) { fprintf(stderr, "%s: unknown field %s\n", name, tok); return 2; }
        }
        const fba::SearchPlan pl = fba::search_plan(P, D);
        // search_key's packing (fba_launch_plan.h): flags, AMAX, tiger_table | model << 2, FTIGER
        const unsigned k = pl.kernel, f = k >> 18 & 63;
        if (fba::kernel_name(k) == fba::K_SEARCH)
            printf("plan %s search_kernel<%s,%u,%s,%u,%u,%u,%s,%s,%s> %d\n", name, f & 1 ? "true" : "false", k >> 12 & 63, f & 2 ? "true" : "false",
                   k >> 6 & 3, k >> 8 & 15, k & 63, f & 4 ? "true" : "false", f & 8 ? "true" : "false", f & 16 ? "true" : "false", pl.quorum);
        else printf("plan %s other %d\n", name, pl.quorum);
    }
    return 0;
}
