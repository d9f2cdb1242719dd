// fba_cli.cpp -- `fba_experiment planning|bapomdp|fbapomdp <flags>`: the reference's three
// executables (src/planning.cpp, src/bapomdp.cpp, src/fbapomdp.cpp) over libfba_hip.so.
//
// Flag names and defaults are the reference's (src/configurations/Conf.cpp:7-60, PlannerConf.cpp:5-26,
// BeliefConf.cpp:5-35, DomainConf.cpp:5-31, BAConf.cpp:42-68, FBAConf.cpp:5-25); the result file has
// the reference's format (PlannerExperiment.cpp:19-25: one "mean, var, count, stder, step duration"
// line; BAPOMDPExperiment.cpp:20-30: one such line per episode index), so
// analysis/preprocess/merge_result_files.py and the plotting scripts read it unchanged.
// -v 2 prints one "T=.. a=.. s'=.. o=.. r=.." line per real step (Episode.cpp:44-45), -v 3 adds the
// root statistics of every search (POUCT.cpp:93-101) and the rejection-loop count
// (RejectionSampling.hpp:68).
//
// All --runs execute concurrently on the GPU (--slots at a time); --seed is hashed into the Philox
// key, so results for a seed differ from the reference's mt19937 stream but not in distribution.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <chrono>
#include <fstream>
#include <iostream>
#include <iterator>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "fba_hip.h"
#include "conf_bridge.hpp"

namespace {

struct Options {
    std::string mode;
    std::string domain, planner = "po-uct", belief = "rejection_sampling", seed, output_file = "results.txt", structure_prior,
                                dirichlet = "expected", id, belief_option, probe_file, probe_slots, step_stats_file, belief_in, belief_out, structure_out, structure_stats_file, on_giveup, retired_file;
    std::vector<std::string> structure_stats_queries;   // --structure-stats-query, as given
    int verbose = 0, runs = 1, horizon = 10, sims = 1000, max_depth = -1, particles = 100, size = 0, height = 0, width = 0,
        episodes = 1, slots = 0, device = 0, resample_amount = 0, first_episode = 0, stop_episode = -1, reject_attempts = 0;
    double discount = .95, exploration = 100, threshold = 0;
    float noise = 0, counts_total = 10000;
    bool help = false, belief_fit = false;
    unsigned long long belief_fit_seed = 0;
};

void usage()
{
    std::puts(
        "usage: fba_experiment planning|bapomdp|fbapomdp [options]\n"
        "  -h, --help                     Print help options\n"
        "  -v, --verbose N                1: track episodes, 2: environment interactions, 3: algorithm summaries\n"
        "  -f, --output-file FILE         result file (results.txt)\n"
        "      --runs N                   Number of runs (1)\n"
        "  -H, --horizon N                Horizon, number of steps per episode (10)\n"
        "  -d, --discount X               Discount for future rewards (0.95)\n"
        "  -P, --planner NAME             random, ts (Thompson sampling) or po-uct (po-uct)\n"
        "  -B, --belief NAME              point_estimate, rejection_sampling, importance_sampling or (fbapomdp) reinvigoration,\n"
        "                                 cheating-reinvigoration, mh-within-gibbs\n"
        "      --seed STR                 Global seed for all random samples\n"
        "      --id STR                   The id to give this process\n"
        "  -s, --simulation-amount N      simulations per search (1000)\n"
        "      --mcts-max-depth N         max search depth, horizon if negative (-1)\n"
        "  -u, --exploration-constant X   UCB exploration constant (100)\n"
        "      --particle-amount N        particles in the filter (100)\n"
        "      --resample-amount N        particles reinvigorated per belief update (reinvigoration beliefs)\n"
        "      --threshold X              cheating-reinvigoration / mh-within-gibbs / mh-nips: log likelihood below which the belief is repaired (< 0);\n"
        "                                 incubator: normalised weight above which a shadow particle is promoted (0 < X <= 1)\n"
        "      --belief-option rs         mh-within-gibbs: state histories by rejection sampling instead of message passing\n"
        "  -D, --domain NAME              episodic-tiger, continuous-tiger, episodic-factored-tiger,\n"
        "                                 continuous-factored-tiger, gridworld, random-collision-avoidance,\n"
        "                                 centered-collision-avoidance, independent-sysadmin, linear-sysadmin,\n"
        "                                 coffee, boutilier-coffee, agr (planning only)\n"
        "      --size N  --height N  --width N\n"
        "      --episodes N               (bapomdp, fbapomdp) episodes per run (1)\n"
        "      --dirichlet_sampling_method regular|expected (expected)\n"
        "      --noise X                  prior noise (0)\n"
        "  -C, --counts-total X           prior counts (10000)\n"
        "      --structure-prior NAME     (fbapomdp) '', uniform, match-counts, match-uniform, fully-connected\n"
        "      --slots N  --device N      runs resident at once on the GPU (auto), HIP device (0)\n"
        "      --probe-file FILE          (bapomdp, fbapomdp) one line per real step that a belief update follows:\n"
        "                                 run episode t action obs state evidence next_true post_true (fba_probe)\n"
        "      --probe-slots FIRST:COUNT  the slots whose steps are probed (all)\n"
        "      --step-stats-file FILE     (every mode) one line per (episode, t) at which a step was taken, summed over all runs on the device:\n"
        "                                 episode t steps terminals, the steps by action, reward_sum reward_sq_sum value_sum nodes_sum depth_sum\n"
        "                                 attempts_steps attempts_sum, and -- fed by --probe-file's probe, else 0 -- probed evidence_zero\n"
        "                                 evidence_sum log_evidence_sum log_evidence_sq_sum next_true_sum post_ratio_sum (fba_step_stats)\n"
        "      --on-giveup stop|retire    a run whose rejection update gives up: stop fails the experiment (default); retire takes the run out,\n"
        "                                 voids its unfinished episodes and lets the slot go on with its next run (fba_giveup_policy)\n"
        "      --reject-attempts N        attempts after which a rejection update gives up: a multiple of 1024 (0: 2^28)\n"
        "      --retired-file FILE        one line per retired run: run episode t slot reason counted max_attempts\n"
        "      --first-episode K          (bapomdp, fbapomdp) run episodes [K, M) of every run only (0, --episodes): the result file\n"
        "      --stop-episode M           has one line per episode of the span\n"
        "      --belief-in FILE           the filters the runs continue from at episode K: one snapshot block for every run, or one\n"
        "                                 per run, concatenated (what --belief-out of the span that ended at K wrote)\n"
        "      --belief-fit SEED          with --belief-in: the file's blocks may be of another particle count or, for history records, of\n"
        "                                 another episodes * horizon; they are refitted to this configuration first (fba_belief_convert:\n"
        "                                 block b draws from the streams of run b under SEED where the particle count changes)\n"
        "      --belief-out FILE          every run's filter when the span is over (needs runs <= slots)\n"
        "      --structure-out FILE       (fbapomdp) one line per run when the experiment or span is over (needs runs <= slots):\n"
        "                                 run weight_total distinct overflow stored, then per stored structure of the top 8\n"
        "                                 its mass and its parent-set words, hexadecimal, joined by commas (fba_belief_structures)\n"
        "      --structure-stats-file FILE  (fbapomdp) one line per (episode, t) at which a step was taken, summed over all runs on the device,\n"
        "                                 whatever runs and slots: episode t steps weightless overflowed collapsed distinct_sum distinct_max,\n"
        "                                 per query frac held sole, then per parent-set word the sums of set_mass / W joined by commas\n"
        "                                 (fba_structure_stats)\n"
        "      --structure-stats-query W0:W1:...  a graph the statistics follow: its parent-set words, hexadecimal (repeatable, at most 16)");
}

bool parse(int argc, char** argv, Options& o, std::string& err)
{
    if (argc < 2) { err = "missing mode (planning, bapomdp or fbapomdp)"; return false; }
    o.mode = argv[1];
    if (o.mode == "-h" || o.mode == "--help") { o.help = true; return true; }
    if (o.mode != "planning" && o.mode != "bapomdp" && o.mode != "fbapomdp") { err = "unknown mode '" + o.mode + "'"; return false; }
    o.id = std::to_string(std::time(nullptr));
    static const std::map<std::string, std::string> shorts = {
        {"-h", "--help"}, {"-v", "--verbose"}, {"-f", "--output-file"}, {"-H", "--horizon"}, {"-d", "--discount"},
        {"-P", "--planner"}, {"-B", "--belief"}, {"-s", "--simulation-amount"}, {"-u", "--exploration-constant"},
        {"-D", "--domain"}, {"-C", "--counts-total"}};
    for (int i = 2; i < argc; ++i) {
        std::string k = argv[i], v;
        const size_t eq = k.find('=');
        bool has_v = false;
        if (k.rfind("--", 0) == 0 && eq != std::string::npos) { v = k.substr(eq + 1); k = k.substr(0, eq); has_v = true; }
        if (shorts.count(k)) k = shorts.at(k);
        if (k == "--help") { o.help = true; continue; }
        if (!has_v) {
            if (i + 1 >= argc) { err = "the required argument for option '" + k + "' is missing"; return false; }
            v = argv[++i];
        }
        try {
            if (k == "--verbose") o.verbose = std::stoi(v);
            else if (k == "--output-file") o.output_file = v;
            else if (k == "--runs") o.runs = std::stoi(v);
            else if (k == "--horizon") o.horizon = std::stoi(v);
            else if (k == "--discount") o.discount = std::stod(v);
            else if (k == "--planner") o.planner = v;
            else if (k == "--belief") o.belief = v;
            else if (k == "--seed") o.seed = v;
            else if (k == "--id") o.id = v;
            else if (k == "--simulation-amount") o.sims = std::stoi(v);
            else if (k == "--mcts-max-depth") o.max_depth = std::stoi(v);
            else if (k == "--exploration-constant") o.exploration = std::stod(v);
            else if (k == "--particle-amount") o.particles = std::stoi(v);
            else if (k == "--resample-amount") o.resample_amount = std::stoi(v);
            else if (k == "--threshold") o.threshold = std::stod(v);
            else if (k == "--belief-option") o.belief_option = v;
            else if (k == "--domain") o.domain = v;
            else if (k == "--size") o.size = std::stoi(v);
            else if (k == "--height") o.height = std::stoi(v);
            else if (k == "--width") o.width = std::stoi(v);
            else if (k == "--episodes") o.episodes = std::stoi(v);
            else if (k == "--dirichlet_sampling_method") o.dirichlet = v;
            else if (k == "--noise") o.noise = std::stof(v);
            else if (k == "--counts-total") o.counts_total = std::stof(v);
            else if (k == "--structure-prior") o.structure_prior = v;
            else if (k == "--slots") o.slots = std::stoi(v);
            else if (k == "--device") o.device = std::stoi(v);
            else if (k == "--probe-file") o.probe_file = v;
            else if (k == "--step-stats-file") o.step_stats_file = v;
            else if (k == "--on-giveup") {
                if (v != "stop" && v != "retire") throw std::invalid_argument(v);
                o.on_giveup = v;
            }
            else if (k == "--reject-attempts") o.reject_attempts = std::stoi(v);
            else if (k == "--retired-file") o.retired_file = v;
            else if (k == "--first-episode") o.first_episode = std::stoi(v);
            else if (k == "--stop-episode") o.stop_episode = std::stoi(v);
            else if (k == "--belief-in") o.belief_in = v;
            else if (k == "--belief-out") o.belief_out = v;
            else if (k == "--belief-fit") { o.belief_fit = true; o.belief_fit_seed = std::stoull(v); }
            else if (k == "--structure-out") o.structure_out = v;
            else if (k == "--structure-stats-file") o.structure_stats_file = v;
            else if (k == "--structure-stats-query") {
                if (v.empty() || v.find_first_not_of("0123456789abcdefABCDEF:") != std::string::npos || v.front() == ':' || v.back() == ':' ||
                    v.find("::") != std::string::npos)
                    throw std::invalid_argument(v);
                o.structure_stats_queries.push_back(v);
            }
            else if (k == "--probe-slots") {
                const size_t colon = v.find(':');
                if (colon == std::string::npos || std::stoi(v.substr(0, colon)) < 0 || std::stoi(v.substr(colon + 1)) < 1) throw std::invalid_argument(v);
                o.probe_slots = v;
            }
            else { err = "unrecognised option '" + k + "'"; return false; }
        } catch (std::exception const&) {
            err = "the argument ('" + v + "') for option '" + k + "' is invalid";
            return false;
        }
    }
    return true;
}

// The reference seeds mt19937 from the characters of --seed; here they key Philox (FNV-1a: conf_bridge.hpp, the function the
// factory patch of INTEGRATION.md uses too).
uint64_t seed_from(std::string const& s) { return fba::seed_from_string(s); }

bool to_config(Options const& o, fba_config& c, std::string& err)
{
    fba_default_config(&c);
    static const std::map<std::string, int> domains = {
        {"episodic-tiger", FBA_DOM_TIGER_EPISODIC}, {"continuous-tiger", FBA_DOM_TIGER_CONTINUOUS},
        {"episodic-factored-tiger", FBA_DOM_FTIGER_EPISODIC}, {"continuous-factored-tiger", FBA_DOM_FTIGER_CONTINUOUS},
        {"gridworld", FBA_DOM_GRIDWORLD}, {"random-collision-avoidance", FBA_DOM_COLLISION_AVOID},
        {"centered-collision-avoidance", FBA_DOM_COLLISION_AVOID_CENTERED},
        {"independent-sysadmin", FBA_DOM_SYSADMIN_INDEPENDENT}, {"linear-sysadmin", FBA_DOM_SYSADMIN_LINEAR},
        {"coffee", FBA_DOM_COFFEE}, {"boutilier-coffee", FBA_DOM_COFFEE_BOUTILIER}, {"agr", FBA_DOM_AGR}};
    if (!domains.count(o.domain)) { err = "please enter a legit domain, provided: " + o.domain; return false; }  // DomainConf.cpp:52-58
    c.domain = domains.at(o.domain);
    if (o.planner == "po-uct" || o.planner == "hip-po-uct") c.planner = FBA_PLANNER_POUCT;
    else if (o.planner == "random") c.planner = FBA_PLANNER_RANDOM;
    else if (o.planner == "ts") c.planner = FBA_PLANNER_TS;
    else { err = "please enter a legit planner: random, ts or po-uct, provided: " + o.planner; return false; }
    if (o.belief == "rejection_sampling" || o.belief == "hip-rejection_sampling") c.belief = FBA_BELIEF_REJECTION;
    else if (o.belief == "importance_sampling" || o.belief == "hip-importance_sampling") c.belief = FBA_BELIEF_IMPORTANCE;
    else if (o.belief == "point_estimate") c.belief = FBA_BELIEF_POINT;  // Belief.cpp:13-14, BABelief.cpp:19-20
    else if (o.belief == "reinvigoration" && o.mode == "fbapomdp") c.belief = FBA_BELIEF_REINVIGORATION;  // BABelief.cpp:28-31
    else if (o.belief == "cheating-reinvigoration" && o.mode == "fbapomdp") c.belief = FBA_BELIEF_CHEATING;  // BABelief.cpp:60-65
    else if (o.belief == "mh-within-gibbs" && o.mode == "fbapomdp") {  // BABelief.cpp:33-47: "" = MSG, "rs" = RS
        c.belief = FBA_BELIEF_MH_GIBBS;
        if (!o.belief_option.empty() && o.belief_option != "rs") {  // BeliefConf.cpp:51-56
            err = "You have set the illegal belief_option '" + o.belief_option + "' with belief " + o.belief + ".";
            return false;
        }
        c.belief_option = o.belief_option == "rs" ? 1 : 0;
    }
    else if (o.belief == "mh-nips" && o.mode == "fbapomdp") c.belief = FBA_BELIEF_MH_NIPS;  // BABelief.cpp:33-36
    else if (o.belief == "nested" && o.mode != "planning") c.belief = FBA_BELIEF_NESTED;   // BABelief.cpp:67-70
    else if (o.belief == "incubator" && o.mode == "fbapomdp") c.belief = FBA_BELIEF_INCUBATOR;   // BABelief.cpp:53-58
    else { err = "please enter a legit state stimator: point_estimate, rejection_sampling, importance_sampling or (fbapomdp) reinvigoration, provided: " + o.belief; return false; }
    if ((o.resample_amount == 0) ^ (o.belief != "reinvigoration" && o.belief != "cheating-reinvigoration" && o.belief != "incubator")) {  // BeliefConf.cpp:40-49
        err = "You have set the resample amount (" + std::to_string(o.resample_amount) + "), but are not using one of the beliefs (" + o.belief +
              ") that use it: reinvigoration, cheating-reinvigoration and incubator";
        return false;
    }
    if (!o.belief_option.empty() && o.belief != "mh-within-gibbs") {  // BeliefConf.cpp:51-56
        err = "You have set the illegal belief_option '" + o.belief_option + "' with belief " + o.belief + ".";
        return false;
    }
    c.resample_amount = o.resample_amount;
    c.threshold = o.threshold;
    if (o.dirichlet == "expected" || o.dirichlet == "1") c.dirichlet_regular = 0;
    else if (o.dirichlet == "regular" || o.dirichlet == "0") c.dirichlet_regular = 1;
    else { err = "please enter either 'regular' or 'expected' for dirichlet_sampling_method, given: " + o.dirichlet; return false; }
    if (o.structure_prior.empty() || o.structure_prior == "match-counts") c.structure_prior = FBA_SP_NONE;
    else if (o.structure_prior == "uniform") c.structure_prior = FBA_SP_UNIFORM;
    else if (o.structure_prior == "match-uniform") c.structure_prior = FBA_SP_MATCH_UNIFORM;
    else if (o.structure_prior == "fully-connected") c.structure_prior = FBA_SP_FULLY_CONNECTED;
    else { err = "unknown structure prior '" + o.structure_prior + "'"; return false; }
    c.model = o.mode == "planning" ? FBA_MODEL_POMDP : (o.mode == "bapomdp" ? FBA_MODEL_BA_TABLE : FBA_MODEL_BA_FACTORED);
    if (o.mode != "planning" && o.episodes < 1) { err = "episodes must be >= 1"; return false; }
    if (o.mode == "planning" && c.dirichlet_regular) c.dirichlet_regular = 0;
    c.size = o.size; c.width = o.width; c.height = o.height;
    c.particles = o.particles; c.sims = o.sims; c.max_depth = o.max_depth; c.horizon = o.horizon;
    c.exploration = o.exploration; c.discount = o.discount;
    c.runs = o.runs; c.episodes = o.mode == "planning" ? 1 : o.episodes;
    c.noise = o.noise; c.counts_total = o.counts_total;
    c.seed = seed_from(o.seed);
    c.slots = o.slots; c.device = o.device;
    c.trace = o.verbose >= 3 ? 2 : (o.verbose >= 2 ? 1 : 0);   // (2: with the filter's state histogram after every update)
    return true;
}

// --probe-file: the probe's records, run by run, episode by episode; a final comment line when the buffer was too small for all of them
bool write_probe(fba_ctx* ctx, const std::string& path)
{
    int64_t seen = 0;
    const int n = fba_probe_count(ctx, &seen);
    if (n < 0) return false;
    std::vector<fba_probe_rec> pr((size_t)std::max(n, 1));
    const int got = n ? fba_get_probe(ctx, pr.data(), n) : 0;
    if (got < 0) return false;
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    std::fprintf(f, "# run episode t action obs state evidence next_true post_true\n");
    for (int i = 0; i < got; ++i) {
        const fba_probe_rec& r = pr[(size_t)i];
        std::fprintf(f, "%d %d %d %d %d %d %.17g %.17g %.17g\n", r.run, r.episode, r.t, r.action, r.obs, r.state, r.evidence, r.next_true, r.post_true);
    }
    if (seen > got) std::fprintf(f, "# %lld steps were probed, %d records were kept\n", (long long)seen, got);
    return std::fclose(f) == 0;
}

// --retired-file: the runs retired under --on-giveup retire, by run; a leading comment line names the columns
bool write_retired(fba_ctx* ctx, const std::string& path, int& got)
{
    const int n = fba_retired_count(ctx, nullptr);
    if (n < 0) return false;
    std::vector<fba_retired_rec> rr((size_t)std::max(n, 1));
    got = n ? fba_get_retired(ctx, rr.data(), n) : 0;
    if (got < 0) return false;
    if (path.empty()) return true;
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    std::fprintf(f, "# run episode t slot reason counted max_attempts\n");
    for (int i = 0; i < got; ++i) {
        const fba_retired_rec& r = rr[(size_t)i];
        std::fprintf(f, "%d %d %d %d %d %d %d\n", r.run, r.episode, r.t, r.slot, r.reason, r.counted, r.max_attempts);
    }
    return std::fclose(f) == 0;
}

// --step-stats-file: one line per bin (episode, t) in which a step was taken; a leading comment line names the columns
bool write_step_stats(fba_ctx* ctx, const fba_config& cfg, int A, const std::string& path)
{
    std::vector<fba_step_stat> bins((size_t)cfg.episodes * (size_t)cfg.horizon);
    if (fba_get_step_stats(ctx, bins.data(), (int32_t)bins.size()) != (int)bins.size()) return false;
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    std::fprintf(f, "# episode t steps terminals");
    for (int a = 0; a < A; ++a) std::fprintf(f, " action_%d", a);
    std::fprintf(f, " reward_sum reward_sq_sum value_sum nodes_sum depth_sum attempts_steps attempts_sum probed evidence_zero evidence_sum log_evidence_sum "
                    "log_evidence_sq_sum next_true_sum post_ratio_sum\n");
    for (int e = 0; e < cfg.episodes; ++e)
        for (int t = 0; t < cfg.horizon; ++t) {
            const fba_step_stat& b = bins[(size_t)e * (size_t)cfg.horizon + (size_t)t];
            if (!b.steps) continue;
            std::fprintf(f, "%d %d %llu %llu", e, t, (unsigned long long)b.steps, (unsigned long long)b.terminals);
            for (int a = 0; a < A; ++a) std::fprintf(f, " %llu", (unsigned long long)b.action[a]);
            std::fprintf(f, " %.17g %.17g %.17g %llu %llu %llu %llu %llu %llu %.17g %.17g %.17g %.17g %.17g\n", b.reward_sum, b.reward_sq_sum, b.value_sum,
                         (unsigned long long)b.nodes_sum, (unsigned long long)b.depth_sum, (unsigned long long)b.attempts_steps,
                         (unsigned long long)b.attempts_sum, (unsigned long long)b.probed, (unsigned long long)b.evidence_zero, b.evidence_sum,
                         b.log_evidence_sum, b.log_evidence_sq_sum, b.next_true_sum, b.post_ratio_sum);
        }
    return std::fclose(f) == 0;
}

// --structure-stats-query: the words of one query, hexadecimal and joined by colons (parse has seen that nothing else stands there)
std::vector<uint32_t> query_words(const std::string& v)
{
    std::vector<uint32_t> w;
    for (size_t at = 0; at <= v.size();) {
        const size_t colon = std::min(v.find(':', at), v.size());
        w.push_back((uint32_t)std::stoul(v.substr(at, colon - at), nullptr, 16));
        at = colon + 1;
    }
    return w;
}

// --structure-stats-file: one line per bin (episode, t) in which a step was taken; a leading comment line names the columns
bool write_structure_stats(fba_ctx* ctx, const fba_config& cfg, int nq, const std::string& path)
{
    int32_t nw = 0, ns = 0;
    fba_structure_lens(ctx, &nw, &ns);
    const size_t bins = (size_t)cfg.episodes * (size_t)cfg.horizon, cells = (size_t)nw * ns;
    std::vector<fba_structure_stat> head(bins);
    std::vector<double> set_frac(bins * cells), query_frac(bins * nq);
    std::vector<uint64_t> held(bins * nq), sole(bins * nq);
    if (fba_get_structure_stats(ctx, (int32_t)bins, head.data(), set_frac.data(), query_frac.data(), held.data(), sole.data()) != (int)bins) return false;
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    std::fprintf(f, "# episode t steps weightless overflowed collapsed distinct_sum distinct_max");
    for (int q = 0; q < nq; ++q) std::fprintf(f, " frac_%d held_%d sole_%d", q, q, q);
    for (int m = 0; m < nw; ++m) std::fprintf(f, " set_frac_%d[%d]", m, ns);
    std::fprintf(f, "\n");
    for (size_t b = 0; b < bins; ++b) {
        const fba_structure_stat& h = head[b];
        if (!h.steps) continue;
        std::fprintf(f, "%d %d %llu %llu %llu %llu %llu %d", (int)(b / (size_t)cfg.horizon), (int)(b % (size_t)cfg.horizon), (unsigned long long)h.steps,
                     (unsigned long long)h.weightless, (unsigned long long)h.overflowed, (unsigned long long)h.collapsed,
                     (unsigned long long)h.distinct_sum, h.distinct_max);
        for (int q = 0; q < nq; ++q)
            std::fprintf(f, " %.17g %llu %llu", query_frac[b * nq + q], (unsigned long long)held[b * nq + q], (unsigned long long)sole[b * nq + q]);
        for (int m = 0; m < nw; ++m)
            for (int v = 0; v < ns; ++v) std::fprintf(f, "%s%.17g", v ? "," : " ", set_frac[b * cells + (size_t)m * ns + v]);
        std::fprintf(f, "\n");
    }
    return std::fclose(f) == 0;
}

// -v 1 / 2 / 3 in the reference's own format, "V%vlevel: %fbase\t%msg" (ArgumentParser.cpp:16-20), from the trace the engine kept:
//   V1  run / episode                                       BAPOMDPExperiment.cpp:56, PlanningExperiment.cpp:41
//   V2  the real step, the end of an episode                 Episode.cpp:44, :58
//   V3  po-uct's pick and root statistics                    POUCT.cpp:94-100, RBAPOUCT.cpp:118-124 (ChanceNode::toString, MCTSTreeNodes.cpp:24-28)
//       the rejection update's loops, the filter behind it   RejectionSampling.hpp:68; (BA)RejectionSampling.cpp:39 / :46 + FlatFilter::toString (FlatFilter.cpp:70-94)
//       the importance update's total weight                 ImportanceSampler.hpp:56
// States, actions and observations are printed as the index elements they are here, "(i)" (IndexedElements.hpp:25) -- the reference's
// gridworld / collision-avoidance types describe themselves in words.  The runs of an experiment execute side by side; their records
// are printed run by run, episode by episode.
void print_trace(fba_ctx* ctx, const Options& o, const fba_config& cfg, int A)
{
    const int n = fba_trace_count(ctx);
    if (n <= 0) return;
    std::vector<fba_trace_rec> tr((size_t)n);
    const int got = fba_get_trace(ctx, tr.data(), n);
    const int verbose = o.verbose;
    const bool planning = o.mode == "planning", pouct = cfg.planner == FBA_PLANNER_POUCT;
    const int particles = cfg.belief == FBA_BELIEF_POINT ? 1 : cfg.particles;
    const char* planner_file = planning ? "POUCT.cpp" : "RBAPOUCT.cpp";
    std::vector<uint32_t> hist;   // the filter's state histogram after every update (domains of at most FBA_TRACE_HIST_BINS states)
    if (verbose >= 3) {
        hist.resize((size_t)n * FBA_TRACE_HIST_BINS);
        if (fba_get_trace_hist(ctx, hist.data(), n) != got) hist.clear();
    }
    double ret = 0, disc = 1;
    for (int i = 0; i < got; ++i) {
        const fba_trace_rec& r = tr[(size_t)i];
        if (r.t == 0) {
            if (planning) std::printf("V1: PlanningExperiment.cpp\trun %d/%d\n", r.run + 1, cfg.runs);
            else std::printf("V1: BAPOMDPExperiment.cpp\trun %d/%d, episode %d/%d\n", r.run + 1, cfg.runs, r.episode + 1, cfg.episodes);
            ret = 0; disc = 1;
        }
        if (verbose >= 3 && pouct) {
            const int a = r.action;
            std::printf("V3: %s\tpo-uct picked node (a=(%d), q=%f, n=%d) at tree of depth=%d and %d action nodes\n", planner_file, a,
                        r.root_q[a], r.root_n[a], r.tree_depth, r.n_nodes);
            std::printf("V3: %s\tAction stats:\n", planner_file);
            for (int k = 0; k < A; ++k) std::printf("V3: %s\t\t(a=(%d), q=%f, n=%d)\n", planner_file, k, r.root_q[k], r.root_n[k]);
        }
        std::printf("V2: Episode.cpp\tT=%d\ta=(%d)\ts'=(%d)\to=(%d)\tr=%g\n", r.t, r.action, r.state, r.obs, r.reward);
        ret += r.reward * disc;
        disc *= cfg.discount;
        if (verbose >= 3 && !r.terminal) {
            if (r.update_count >= 0) {
                std::printf("V3: RejectionSampling.hpp\tperformed %d loops for rejection sampling for %d samples\n", r.update_count, particles);
                if (!hist.empty()) {   // one message of several lines, as the reference's
                    std::printf("V3: %s\tStatus of rejection sampling filter after update:Particle filter contains:\n",
                                planning ? "RejectionSampling.cpp" : "BARejectionSampling.cpp");
                    for (int st = 0; st < FBA_TRACE_HIST_BINS; ++st) {
                        const uint32_t k = hist[(size_t)i * FBA_TRACE_HIST_BINS + st];
                        if (k) std::printf("\t((%d): %f(%u))\n", st, k / static_cast<double>(particles), k);
                    }
                }
            } else if (cfg.belief == FBA_BELIEF_IMPORTANCE) {
                std::printf("V3: ImportanceSampler.hpp\tacquired total weight of %g after updating %d particles\n", r.weight_total, particles);
            }
        }
        const bool last = i + 1 == got || tr[(size_t)i + 1].t == 0;
        if (last) std::printf("V2: Episode.cpp\tEnd of episode at s=(%d) with return=%g\n", r.state, ret);
    }
}

// --structure-out: run r's filter stands in slot r (runs <= slots); the top 8 graphs of each, one line per run
bool write_structures(fba_ctx* ctx, int runs, const std::string& path)
{
    constexpr int top = 8;
    int32_t nw = 0, ns = 0;
    if (fba_structure_lens(ctx, &nw, &ns) != FBA_OK) return false;
    std::vector<fba_structure_head> head((size_t)runs);
    std::vector<uint32_t> words((size_t)runs * top * (size_t)nw);
    std::vector<double> mass((size_t)runs * top);
    if (fba_belief_structures(ctx, 0, runs, top, 0, nullptr, head.data(), nullptr, words.data(), mass.data(), nullptr) != FBA_OK) return false;
    std::ofstream f(path);
    f << "# run weight_total distinct overflow stored, then per stored structure: mass words (hexadecimal, word 0 first)\n";
    char buf[64];
    for (int r = 0; r < runs; ++r) {
        const fba_structure_head& h = head[(size_t)r];
        std::snprintf(buf, sizeof buf, "%.17g", h.weight_total);
        f << r << ' ' << buf << ' ' << h.distinct << ' ' << h.overflow << ' ' << h.stored;
        for (int k = 0; k < h.stored; ++k) {
            std::snprintf(buf, sizeof buf, "%.17g", mass[(size_t)r * top + k]);
            f << ' ' << buf << ' ';
            for (int m = 0; m < nw; ++m) {
                std::snprintf(buf, sizeof buf, "%x", words[((size_t)r * top + k) * (size_t)nw + m]);
                f << (m ? "," : "") << buf;
            }
        }
        f << '\n';
    }
    return (bool)f.flush();
}

}  // namespace

int main(int argc, char** argv)
{
    Options o;
    std::string err;
    if (!parse(argc, argv, o, err)) {
        std::fprintf(stderr, "ERROR: %s\n", err.c_str());
        return 1;
    }
    if (o.help) {
        usage();
        return 0;
    }
    fba_config cfg;
    if (!to_config(o, cfg, err)) {
        std::fprintf(stderr, "ERROR: %s\n", err.c_str());
        return 1;
    }
    {   // --structure-stats-file, --structure-stats-query: what is refused before a device is asked for
        std::string what;
        if (!o.structure_stats_file.empty() && o.mode != "fbapomdp")
            what = "--structure-stats-file needs a factored Bayes-adaptive experiment (fbapomdp): only its particles carry a graph";
        else if (o.structure_stats_queries.size() > FBA_STRUCT_STATS_MAX_QUERIES)
            what = "--structure-stats-query: " + std::to_string(o.structure_stats_queries.size()) + " graphs where at most 16 are followed";
        else if (o.structure_stats_file.empty() && !o.structure_stats_queries.empty())
            what = "--structure-stats-query names a graph for --structure-stats-file, which is not given";
        if (!what.empty()) {
            std::fprintf(stderr, "ERROR: %s\n", what.c_str());
            return 1;
        }
    }
    fba_ctx* ctx = nullptr;
    if (fba_create(&cfg, &ctx) != FBA_OK) {
        std::fprintf(stderr, "ERROR: %s\n", fba_last_error(nullptr));
        return 1;
    }
    if (!o.probe_file.empty()) {
        if (o.mode == "planning") {
            std::fprintf(stderr, "ERROR: --probe-file needs a Bayes-adaptive experiment (bapomdp or fbapomdp)\n");
            fba_destroy(ctx);
            return 1;
        }
        int first = 0, count = fba_slots(ctx);
        if (!o.probe_slots.empty()) {
            const size_t colon = o.probe_slots.find(':');
            first = std::stoi(o.probe_slots.substr(0, colon));
            count = std::stoi(o.probe_slots.substr(colon + 1));
        }
        const long long want = (long long)cfg.runs * cfg.episodes * cfg.horizon;
        if (fba_probe_enable(ctx, first, count, (int32_t)std::min<long long>(want, 1ll << 26)) != FBA_OK) {
            std::fprintf(stderr, "ERROR: %s\n", fba_last_error(ctx));
            fba_destroy(ctx);
            return 1;
        }
    }
    const bool giveup = !o.on_giveup.empty() || o.reject_attempts != 0 || !o.retired_file.empty();
    if (giveup && fba_giveup_policy(ctx, o.on_giveup == "retire" ? FBA_GIVEUP_RETIRE : FBA_GIVEUP_STOP, o.reject_attempts) != FBA_OK) {
        std::fprintf(stderr, "ERROR: %s\n", fba_last_error(ctx));
        fba_destroy(ctx);
        return 1;
    }
    if (!o.step_stats_file.empty() && fba_step_stats_enable(ctx, 1) != FBA_OK) {
        std::fprintf(stderr, "ERROR: %s\n", fba_last_error(ctx));
        fba_destroy(ctx);
        return 1;
    }
    if (!o.structure_stats_file.empty()) {
        std::string what;
        int32_t nw = 0, ns = 0;
        fba_structure_lens(ctx, &nw, &ns);
        std::vector<uint32_t> query;
        for (const std::string& v : o.structure_stats_queries) {
            const std::vector<uint32_t> w = query_words(v);
            if (nw > 0 && (int)w.size() != nw) {
                what = "--structure-stats-query " + v + ": " + std::to_string(w.size()) + " words where the model's particles carry " + std::to_string(nw);
                break;
            }
            query.insert(query.end(), w.begin(), w.end());
        }
        if (what.empty() && fba_structure_stats_enable(ctx, 1, (int32_t)o.structure_stats_queries.size(), query.empty() ? nullptr : query.data()) != FBA_OK)
            what = fba_last_error(ctx);
        if (!what.empty()) {
            std::fprintf(stderr, "ERROR: %s\n", what.c_str());
            fba_destroy(ctx);
            return 1;
        }
    }
    if (!o.structure_out.empty()) {
        const char* what = nullptr;
        if (o.mode != "fbapomdp") what = "--structure-out needs a factored Bayes-adaptive experiment (fbapomdp): only its particles carry a graph";
        else if (fba_belief_structures(ctx, 0, 0, 8, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != FBA_OK) what = fba_last_error(ctx);
        else if (cfg.runs > fba_slots(ctx))
            what = "--structure-out needs runs <= slots: a slot keeps the filter of the last run it executed only (shard the runs over processes instead)";
        if (what) {
            std::fprintf(stderr, "ERROR: %s\n", what);
            fba_destroy(ctx);
            return 1;
        }
    }
    // a span of the experiment (--first-episode, --stop-episode, --belief-in, --belief-out: fba_run_bapomdp_span)
    const bool span = o.first_episode != 0 || o.stop_episode >= 0 || !o.belief_in.empty() || !o.belief_out.empty();
    const int first_episode = o.first_episode, stop_episode = o.stop_episode < 0 ? cfg.episodes : o.stop_episode;
    std::vector<char> blocks;
    int64_t per_block = 0;
    if (span) {
        const char* what = nullptr;
        if (o.mode == "planning") what = "--first-episode, --stop-episode, --belief-in and --belief-out need a Bayes-adaptive experiment (bapomdp or fbapomdp)";
        else if (fba_belief_snapshot_bytes(ctx, &per_block) != FBA_OK) what = fba_last_error(ctx);
        else if (!o.belief_out.empty() && cfg.runs > fba_slots(ctx))
            what = "--belief-out needs runs <= slots: a slot keeps the filter of the last run it executed only (shard the runs over processes instead)";
        if (!what && !o.belief_in.empty()) {
            std::ifstream in(o.belief_in, std::ios::binary);
            if (in) blocks.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
            if (in && !blocks.empty() && o.belief_fit) {   // blocks of another particle count or record room: refitted, then taken as any
                const int64_t src_block = blocks.size() >= sizeof(fba_snapshot_head) ? fba_snapshot_block_bytes(reinterpret_cast<const fba_snapshot_head*>(blocks.data())) : 0;
                if (src_block < (int64_t)sizeof(fba_snapshot_head) || blocks.size() % (size_t)src_block) {
                    err = "--belief-in " + o.belief_in + ": not a file of snapshot blocks (" + std::to_string(blocks.size()) + " bytes, " + std::to_string(src_block) +
                          " per block by its first header)";
                    what = err.c_str();
                } else {
                    const size_t n = blocks.size() / (size_t)src_block;
                    std::vector<char> fitted(n * (size_t)per_block);
                    if (fba_belief_convert(ctx, (int32_t)n, blocks.data(), (int64_t)blocks.size(), o.belief_fit_seed, 0, fitted.data(), (int64_t)fitted.size()) != FBA_OK) {
                        err = "--belief-in " + o.belief_in + " --belief-fit: " + fba_last_error(ctx);
                        what = err.c_str();
                    } else blocks.swap(fitted);
                }
            } else if (!in || blocks.empty() || blocks.size() % (size_t)per_block) {
                err = "--belief-in " + o.belief_in + ": not a file of snapshot blocks of this configuration (" + std::to_string(blocks.size()) + " bytes, " +
                      std::to_string(per_block) + " per block)";
                what = err.c_str();
            }
        }
        if (what) {
            std::fprintf(stderr, "ERROR: %s\n", what);
            fba_destroy(ctx);
            return 1;
        }
    }
    std::fprintf(stderr, "INFO: (%s): Starting %s experiment\n", o.id.c_str(), o.mode == "planning" ? "planning" : "BAPOMDP");
    std::vector<fba_stat> stats((size_t)cfg.episodes);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc  = o.mode == "planning" ? fba_run_planning(ctx, stats.data())
                    : !span             ? fba_run_bapomdp(ctx, stats.data())
                                        : fba_run_bapomdp_span(ctx, first_episode, stop_episode, blocks.empty() ? nullptr : blocks.data(),
                                                               blocks.empty() ? 0 : (int32_t)(blocks.size() / (size_t)per_block), (int64_t)blocks.size(), stats.data());
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc != FBA_OK) {
        std::fprintf(stderr, "ERROR: %s\n", fba_last_error(ctx));
        fba_destroy(ctx);
        return 1;
    }
    fba_counters cnt;
    fba_get_counters(ctx, &cnt);
    // "step duration mean": every run advances one real step per tick, so the time one run's step
    // takes is the wall time over the ticks = real steps of the longest chain of runs on one slot
    const int slots = fba_slots(ctx);
    const double chains = std::ceil((double)cfg.runs / slots);
    const double step_duration = cnt.env_steps ? wall / ((double)cnt.env_steps / ((double)cfg.runs / chains)) : 0.0;
    if (o.verbose >= 2) {
        int32_t S, A, O;
        fba_domain_sizes(ctx, &S, &A, &O);
        print_trace(ctx, o, cfg, A);
    }
    if (!o.probe_file.empty() && !write_probe(ctx, o.probe_file)) {
        std::fprintf(stderr, "ERROR: the probe's records could not be written to %s: %s\n", o.probe_file.c_str(), fba_last_error(ctx));
        fba_destroy(ctx);
        return 1;
    }
    if (giveup) {
        int retired = 0;
        if (!write_retired(ctx, o.retired_file, retired)) {
            std::fprintf(stderr, "ERROR: the retired runs could not be written to %s: %s\n", o.retired_file.c_str(), fba_last_error(ctx));
            fba_destroy(ctx);
            return 1;
        }
        if (o.on_giveup == "retire")
            std::fprintf(stderr, "NOTICE: (%s): %d of %d runs were retired: their rejection updates gave up; the statistics are over the others\n", o.id.c_str(),
                         retired, cfg.runs);
    }
    if (!o.step_stats_file.empty()) {
        int32_t S, A, O;
        fba_domain_sizes(ctx, &S, &A, &O);
        if (!write_step_stats(ctx, cfg, A, o.step_stats_file)) {
            std::fprintf(stderr, "ERROR: the step statistics could not be written to %s: %s\n", o.step_stats_file.c_str(), fba_last_error(ctx));
            fba_destroy(ctx);
            return 1;
        }
    }
    if (!o.belief_out.empty()) {   // run r's filter stands in slot r (runs <= slots)
        std::vector<char> out((size_t)cfg.runs * (size_t)per_block);
        bool ok = fba_belief_export(ctx, 0, cfg.runs, out.data(), (int64_t)out.size()) == FBA_OK;
        if (ok) {
            std::ofstream f(o.belief_out, std::ios::binary);
            f.write(out.data(), (std::streamsize)out.size());
            ok = (bool)f.flush();
        }
        if (!ok) {
            std::fprintf(stderr, "ERROR: the filters could not be written to %s: %s\n", o.belief_out.c_str(), fba_last_error(ctx));
            fba_destroy(ctx);
            return 1;
        }
    }
    if (!o.structure_stats_file.empty() && !write_structure_stats(ctx, cfg, (int)o.structure_stats_queries.size(), o.structure_stats_file)) {
        std::fprintf(stderr, "ERROR: the structure statistics could not be written to %s: %s\n", o.structure_stats_file.c_str(), fba_last_error(ctx));
        fba_destroy(ctx);
        return 1;
    }
    if (!o.structure_out.empty() && !write_structures(ctx, cfg.runs, o.structure_out)) {
        std::fprintf(stderr, "ERROR: the structures could not be written to %s: %s\n", o.structure_out.c_str(), fba_last_error(ctx));
        fba_destroy(ctx);
        return 1;
    }
    {
        std::ofstream f(o.output_file);
        f << "# version 1:\n# return mean, return var, return count, return stder, step duration mean\n";
        if (o.mode == "planning") {
            f << stats[0].mean << ", " << fba_stat_var(&stats[0]) << ", " << stats[0].count << ", " << fba_stat_stder(&stats[0]) << ", "
              << step_duration;
        } else {
            for (int e = span ? first_episode : 0; e < (span ? stop_episode : cfg.episodes); ++e) {
                auto const& s = stats[(size_t)e];
                f << s.mean << ", " << fba_stat_var(&s) << ", " << s.count << ", " << fba_stat_stder(&s) << ", " << step_duration << "\n";
            }
        }
        f << std::endl;
    }
    std::fprintf(stderr, "INFO: (%s): Succesfully ran experiment: %llu simulated steps in %.3f s\n", o.id.c_str(),
                 (unsigned long long)(cnt.sim_steps + cnt.belief_steps), wall);
    fba_destroy(ctx);
    return 0;
}
