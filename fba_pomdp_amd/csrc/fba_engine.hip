// fba_engine.hip -- host side of libfba_hip.so: context, HBM allocation, prior tables,
// kernel orchestration (one HIP stream per ctx), HIP-event timing, and the C-ABI of
// include/fba_hip.h.  There is no CPU fallback anywhere in this file: without a gfx950 device
// fba_create fails with FBA_ENODEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <map>
#include <memory>
#include <vector>

#include "fba_belief_factors.h"   // record_format
#include "fba_launch_plan.h"
#include "fba_snapshot_format.h"

using namespace fba;

namespace {

thread_local std::string g_create_error;

struct EventPair {
    hipEvent_t a, b;
    int kind;
};

}  // namespace

struct fba_ctx {
    fba_config cfg{};
    Problem P{};
    DeviceState D{};
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<void*> allocs;
    struct ArrayEntry { const void* p; fba_array_info info; };
    std::vector<ArrayEntry> arrays;   // fba_device_arrays: one entry per named dev_alloc, in allocation order
    std::vector<float> prior;  // host copy, dense_C floats
    int dense_C          = 0;   // length of a particle's count table as the API sees it (= P.C unless P.packed)
    float* d_prior       = nullptr;
    float* d_prior_dense = nullptr;  // packed / history particles: the dense prior table on the device
    std::vector<float> prior_alt;    // history particles: the x / y transition nodes with the goal as third parent, [A][2][N*N*G*N]
    float* d_hist_base   = nullptr;  // ... and both tables on the device, rows padded to 16 bytes (HistLayout)
    float* d_hist_alt    = nullptr;
    uint8_t* d_hist_lds  = nullptr;  // ... and deduplicated: row ids + distinct rows (Problem::hist_lds)
    uint32_t* d_tab_rows = nullptr;  // tabular history particles (Problem::hist == 2): the prior's sparse rows (TabRows, fba_device.h)
    FDesc fdesc{};          // host copy of the factored model description
    FDesc* d_fdesc       = nullptr;
    GridDesc gdesc{};
    GridDesc* d_gdesc    = nullptr;
    CADesc cadesc{};
    CADesc* d_cadesc     = nullptr;
    SysDesc sysdesc{};
    SysDesc* d_sysdesc   = nullptr;
    ZigDesc* d_zig       = nullptr;
    double* d_uni_scan   = nullptr;
    double* d_log1p      = nullptr;
    int32_t* d_n_active  = nullptr;
    size_t returns_cap   = 0;
    bool started         = false;  // fba_run_ticks has set the slots up
    bool belief_ready    = false;
    std::vector<uint32_t> packed_updates;  // per slot: fba_belief_update calls since fba_belief_init (packed records hold uint16 increments)
    // timing
    bool timing = true;
    std::vector<EventPair> pending;
    std::vector<EventPair> free_events;
    double k_ms[FBA_K_COUNT]          = {0};
    uint64_t k_launches[FBA_K_COUNT]  = {0};
    uint64_t base_sim = 0, base_attempts = 0, base_particles = 0, base_entries = 0, base_compact_full = 0, base_compact = 0;
    uint64_t restored_particles = 0, restored_bytes = 0;   // resumed spans since fba_reset_kernel_times: particles taken from blocks, bytes read and written
    std::vector<fba_trace_rec> trace_host;
    // compact filters (fba_state.h): the experiment loop of this context may keep them (plan_filters), and a tick has run that way since
    // the last materialize_records
    bool compact_ok = false, compact_dirty = false;
    // fba_probe: on while probe.count > 0; the buffers probe points into are the context's (fba_probe_enable)
    BeliefProbeArgs probe{};
    int32_t* d_probe_meta = nullptr;   // [2][nodes] seg, rows
    // fba_step_stats: on while step_stats.bins is set (with D.step_scratch); the buffers are the context's (fba_step_stats_enable)
    StepStatsArgs step_stats{};
    double step_stats_ms = 0;          // diagnostic (FBA_STEP_STATS_TIME=1 in the environment, scripts/bench_step_stats.py): the kernel's own time
    uint64_t step_stats_launches = 0;  // ... by a HIP-event pair around each launch, and the launches
    bool step_stats_timed = false;
    // fba_structure_stats: on while struct_stats.bins is set; the buffers are the context's (fba_structure_stats_enable)
    StructStatsArgs struct_stats{};
    double struct_stats_ms = 0;          // diagnostic (FBA_STRUCT_STATS_TIME=1 in the environment, scripts/bench_structure_stats.py): the
    uint64_t struct_stats_launches = 0;  // kernels' own time by a HIP-event pair around the launches of a tick, and those ticks
    bool struct_stats_timed = false;
    // fba_giveup_policy: the policy of the experiment loops (the limit itself is P.reject_max) and the list of retired runs, whose buffers
    // are the context's (fba_giveup_policy allocates them; retired.recs is null in a context that never made the call)
    int32_t giveup_policy = FBA_GIVEUP_STOP;
    RetireArgs retired{};
};

namespace {

int fail(fba_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(c, call)                                                                             \
    do {                                                                                            \
        hipError_t _e = (call);                                                                     \
        if (_e != hipSuccess)                                                                       \
            return fail((c), FBA_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

#define TRY(x) do { if (const int _rc = (x)) return _rc; } while (0)   // passes a refusal on to the caller

template <typename T>
int dev_alloc(fba_ctx* c, T** p, size_t n, bool zero = true)
{
    if (n == 0) n = 1;
    void* q = nullptr;
    {
        const hipError_t e = hipMalloc(&q, n * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();  // the error is reported here; it must not stay behind for a later context's hipGetLastError()
            return fail(c, FBA_EHIP, "hipMalloc(&q, n * sizeof(T)) failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
        }
    }
    c->allocs.push_back(q);
    if (zero) HIPCHK(c, hipMemsetAsync(q, 0, n * sizeof(T), c->stream));
    *p = static_cast<T*>(q);
    return FBA_OK;
}

// dev_alloc of an array that fba_device_arrays reports, under the name of the member that holds it: `buffers` buffers in which every
// slot takes `slot_elems` elements (0: the array is not laid out by slot).  The entry is written here and nowhere else, from the very
// numbers the allocation used
template <typename T>
int dev_alloc(fba_ctx* c, const char* name, T** p, size_t n, size_t slot_elems = 0, int buffers = 1, bool zero = true)
{
    TRY(dev_alloc(c, p, n, zero));
    fba_array_info a{};
    std::snprintf(a.name, sizeof a.name, "%s", name);
    a.elem_bytes = sizeof(T);
    a.elems      = n ? n : 1;
    a.slot_elems = slot_elems;
    a.buffers    = buffers;
    c->arrays.push_back({*p, a});
    return FBA_OK;
}
#define ARR(m) #m, &D.m   // a DeviceState member as (name, pointer)

// ... of `buffers` buffers of E slots of slot_elems elements each
template <typename T>
int slot_alloc(fba_ctx* c, const char* name, T** p, size_t slot_elems, int buffers = 1, bool zero = true)
{
    return dev_alloc(c, name, p, (size_t)buffers * c->P.E * slot_elems, slot_elems, buffers, zero);
}

// gives a dev_alloc'ed buffer back before the ctx goes (buffers that are re-grown: the trace)
template <typename T>
void dev_free(fba_ctx* c, T*& p)
{
    if (!p) return;
    auto it = std::find(c->allocs.begin(), c->allocs.end(), static_cast<void*>(p));
    if (it != c->allocs.end()) c->allocs.erase(it);
    c->arrays.erase(std::remove_if(c->arrays.begin(), c->arrays.end(), [&](const fba_ctx::ArrayEntry& a) { return a.p == p; }), c->arrays.end());
    (void)hipFree(p);
    p = nullptr;
}

// room for `want` trace records (and, with trace = 2, their histograms: FBA_TRACE_HIST_BINS words each, so the cap is lower there --
// 2^18 records = 64 MB of histograms instead of 1 GiB; later records are counted, not kept)
int ensure_trace(fba_ctx* c, size_t want)
{
    const bool hist = c->cfg.trace >= 2 && c->P.S <= FBA_TRACE_HIST_BINS && !c->P.nested;
    const size_t cap = std::min<size_t>(want, hist ? (size_t)1 << 18 : (size_t)1 << 22);
    if ((size_t)c->D.trace_cap < cap) {
        int rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (nothing in flight reads the old buffers)
        dev_free(c, c->D.trace);
        dev_free(c, c->D.trace_hist);
        DeviceState& D = c->D;
        if ((rc = dev_alloc(c, ARR(trace), cap))) return rc;
        if (hist)
            if ((rc = dev_alloc(c, ARR(trace_hist), cap * FBA_TRACE_HIST_BINS))) return rc;
        c->D.trace_cap = (int32_t)cap;
    }
    HIPCHK(c, hipMemsetAsync(c->D.trace_count, 0, sizeof(int32_t), c->stream));
    return FBA_OK;
}

// a device buffer that is freed on every way out of the function (the selftests return early through HIPCHK)
template <typename T>
struct ScratchBuf {
    T* p = nullptr;
    ~ScratchBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n * sizeof(T)); }
};

bool is_ca(int d) { return d == FBA_DOM_COLLISION_AVOID || d == FBA_DOM_COLLISION_AVOID_CENTERED; }
bool is_sys(int d) { return d == FBA_DOM_SYSADMIN_INDEPENDENT || d == FBA_DOM_SYSADMIN_LINEAR; }

// SysAdmin (reference src/domains/sysadmin/SysAdmin.cpp:12: parameters .025f, .95f, .95f, 1.0f, .075f).
// keep[n] = (1 - fail_prob) * pow(1 - fail_neighbour_factor, n) as SysAdmin::step (:116-118)
// evaluates it: float factor times a double pow, libm on the host so the device only looks it up.
constexpr float SYS_FAIL = .025f, SYS_OBSERVE = .95f, SYS_REBOOT = .95f, SYS_NEIGHBOUR = .075f;
void build_sysadmin(SysDesc& d, int n)
{
    d.N = n; d.pad = 0;
    for (int k = 0; k < 3; ++k) d.keep[k] = (double)(1 - SYS_FAIL) * std::pow((double)(1 - SYS_NEIGHBOUR), (double)k);
}
int sys_failing_neighbours(const SysDesc& d, bool linear, int comp, int s)  // SysAdmin::numFailingNeighbours :221-246
{
    if (!linear) return 0;
    int n = 0;
    if (comp > 0 && !((s >> (comp - 1)) & 1)) n++;
    if (comp < d.N - 1 && !((s >> (comp + 1)) & 1)) n++;
    return n;
}

// SysAdminFlatPrior::precomputeFlatPrior (SysAdminFlatPrior.cpp:38-247): every transition
// probability times 10000, enumerated by a recursion over the computers N-1 .. 0 that multiplies
// the per-computer outcomes in double and writes float counts at its leaves.  The order of the
// leaves is the reference's, because reboot-branch leaves overwrite counts written earlier; so is
// the quirk that setTrueTCounts (:168-172) hands numFailingNeighbours the ACTION index.
struct SysFlat {
    const Problem& P;
    const SysDesc& d;
    float* phi;
    double keep(int comp, int s) const { return d.keep[sys_failing_neighbours(d, P.domain == FBA_DOM_SYSADMIN_LINEAR, comp, s)]; }
    void leaf_reboot(int s, int ns, double prob, int reb) { phi[(s * P.A + d.N + reb) * P.S + ns] = (float)prob * 10000.f; }
    void recur_reboot(int s, int ns, int comp, double acc, int reb)  // :188-234
    {
        if (comp < 0) return leaf_reboot(s, ns, acc, reb);
        const int ns_fail = ns & ~(1 << comp);
        if (!((s >> comp) & 1)) return recur_reboot(s, ns_fail, comp - 1, acc, reb);
        const double fail = 1 - keep(comp, s);
        recur_reboot(s, ns, comp - 1, acc * (1 - fail), reb);
        recur_reboot(s, ns_fail, comp - 1, acc * fail, reb);
    }
    void leaf(int s, int ns, double prob)  // setTrueTCounts :150-186
    {
        const int N = d.N;
        for (int a = 0; a < N; ++a) phi[(s * P.A + a) * P.S + ns] = (float)prob * 10000.f;
        for (int a = N; a < 2 * N; ++a) {
            if ((ns >> (a - N)) & 1) {
                const double fail = 1 - keep(a, s);
                phi[(s * P.A + a) * P.S + ns] = 10000.f * (float)(prob + (prob * fail / (1 - fail) * SYS_REBOOT));
            } else {
                phi[(s * P.A + a) * P.S + ns] = 10000.f * (float)(prob * (1 - SYS_REBOOT));
            }
        }
    }
    void recur(int s, int ns, int comp, double acc)  // :93-148
    {
        if (comp < 0) return leaf(s, ns, acc);
        const int ns_fail = ns & ~(1 << comp);
        if (!((s >> comp) & 1)) {
            recur(s, ns_fail, comp - 1, acc);
            recur_reboot(s, ns_fail, comp - 1, acc * (1 - SYS_REBOOT), comp);
            recur_reboot(s, ns, comp - 1, acc * SYS_REBOOT, comp);
        } else {
            const double fail = 1 - keep(comp, s);
            recur(s, ns, comp - 1, acc * (1 - fail));
            recur(s, ns_fail, comp - 1, acc * fail);
        }
    }
};
double normal_cdf(double x) { return .5 + .5 * std::erf(x / (1 * std::sqrt(2.0))); }  // rnd::normal::cdf random.cpp:119-124

// Collision avoidance tables (reference CollisionAvoidance.cpp ctor :100-142)
void build_collision_avoidance(CADesc& c, int W, int H, int n, bool random_start)
{
    std::memset(&c, 0, sizeof c);
    c.W = W; c.H = H; c.n = n; c.Hn = 1;
    for (int k = 0; k < n; ++k) c.Hn *= H;
    for (int d = 0; d < H; ++d) c.err[d] = normal_cdf(d + .5) - normal_cdf(d - .5);
    for (int k = 0; k < 19; ++k) c.phi[k] = normal_cdf((k - 9) + .5);
    if (random_start) {  // every state with x = W-1, probability 1.f / pow(H, n + 1) each
        c.start_v   = (float)(1.f / std::pow(H, n + 1));
        c.start_i0  = (W - 1) * H * c.Hn;
        c.start_cnt = H * c.Hn;
        c.start_total = 0;
        for (int k = 0; k < c.start_cnt; ++k) c.start_total += c.start_v;  // categoricalDistr::setRawValue
    } else {             // agent and obstacles in the middle row
        int obs = 0;
        for (int k = 0; k < n; ++k) obs = obs * H + H / 2;
        c.start_v = 1; c.start_total = 1; c.start_cnt = 1;
        c.start_i0 = ((W - 1) * H + H / 2) * c.Hn + obs;
    }
}

// ziggurat tables of rnd::initiate() (reference src/utils/random.cpp:47-74), libm on the host
void build_ziggurat(ZigDesc& z)
{
    double tn = 3.442619855899;
    const double m1 = 2147483648.0, vn = 9.91256303526217e-3, q = vn / std::exp(-.5 * tn * tn);
    z.ul[0]   = (uint32_t)(unsigned long)((tn / q) * m1);
    z.ul[1]   = 0;
    z.wn[0]   = q / m1;
    z.wn[127] = tn / m1;
    z.fn[0]   = 1.;
    z.fn[127] = std::exp(-.5 * tn * tn);
    for (int i = 126; i > 0; --i) {
        const double dn = std::sqrt(-2 * std::log(vn / tn + std::exp(-.5 * tn * tn)));
        z.ul[i + 1]     = (uint32_t)(unsigned long)((dn / tn) * m1);
        z.fn[i]         = std::exp(-.5 * dn * dn);
        z.wn[i]         = dn / m1;
        tn              = dn;
    }
}

// GridWorld geometry (reference src/domains/gridworld/GridWorld.cpp)
void build_gridworld(GridDesc& g, int N)
{
    std::memset(&g, 0, sizeof g);
    const int edge = N - 1;
    g.N = N;
    int G = 0;
    // goalLocations :124-152
    const int start = (N < 5) ? N - 2 : (N < 7) ? N - 3 : N - 4;
    for (int i = start; i < N - 1; ++i) {
        g.goal[G][0] = i; g.goal[G][1] = edge; ++G;
        g.goal[G][0] = edge; g.goal[G][1] = i; ++G;
    }
    g.goal[G][0] = edge; g.goal[G][1] = edge; ++G;
    if (N > 3) { g.goal[G][0] = edge - 1; g.goal[G][1] = edge - 1; ++G; }
    if (N > 6) {
        g.goal[G][0] = edge - 2; g.goal[G][1] = edge - 1; ++G;
        g.goal[G][0] = edge - 1; g.goal[G][1] = edge - 2; ++G;
    }
    g.G = G;
    // generateSlowLocations :78-103
    int ns = 0;
    if (N > 5) { g.slow[ns][0] = 1; g.slow[ns][1] = 1; ++ns; }
    if (N == 3) { g.slow[ns][0] = 1; g.slow[ns][1] = 1; ++ns; }
    else if (N < 7) {
        g.slow[ns][0] = edge - 1; g.slow[ns][1] = edge - 2; ++ns;
        g.slow[ns][0] = edge - 2; g.slow[ns][1] = edge - 1; ++ns;
    } else {
        g.slow[ns][0] = edge - 1; g.slow[ns][1] = edge - 3; ++ns;
        g.slow[ns][0] = edge - 3; g.slow[ns][1] = edge - 1; ++ns;
        g.slow[ns][0] = edge - 2; g.slow[ns][1] = edge - 2; ++ns;
    }
    g.nslow = ns;
    // _obs_displacement_probs (ctor :60-70): {.8, .1, .05, ..., last one repeated}
    g.disp[0] = (float)(1 - .2);
    double prob = .2;
    for (int i = 1; i < N - 1; ++i) { prob *= .5; g.disp[i] = (float)prob; }
    g.disp[N - 1] = (float)prob;
}
bool gw_slow_at_h(const GridDesc& g, int x, int y)
{
    for (int i = 0; i < g.nslow; ++i)
        if (g.slow[i][0] == x && g.slow[i][1] == y) return true;
    return false;
}
void gw_move_h(const GridDesc& g, int a, int& x, int& y)
{
    const int N = g.N;
    if (a == 0) { if (y != N - 1) ++y; }
    else if (a == 2) { if (y != 0) --y; }
    else if (a == 1) { if (x != N - 1) ++x; }
    else { if (x != 0) --x; }
}
float gw_obs_displ_prob_h(const GridDesc& g, int loc, int observed)
{
    const int disp = std::abs(loc - observed);
    float res = (disp == 0) ? (float)(1 - .2) : (float)((double)g.disp[disp] * .5);
    if (observed == g.N - 1 || observed == 0)
        for (int i = disp + 1; i < g.N; ++i) res = (float)((double)res + (double)g.disp[i] * .5);
    return res;
}

// Tabular prior count tables, built on the host once per ctx (cold path).
// TigerBAPrior (reference src/domains/tiger/TigerPriors.cpp:14-43): every count 5000 except
// listen: T off-diagonal 0, O = (.85 - noise) * C / (.15 + noise) * C.
// FactoredTigerFlatPrior (src/domains/tiger/FactoredTigerPriors.cpp:18-88): same over S = 2^(K+1)
// states, tiger location = (s < S/2 ? LEFT : RIGHT).
int build_tabular_prior(fba_ctx* c)
{
    const Problem& P = c->P;
    const int S = P.S, A = P.A, O = P.O;
    const float noise = c->cfg.noise, total = c->cfg.counts_total;
    if (is_sys(P.domain)) {  // SysAdminFlatPrior: zero-initialised BAFlatModel, --noise / -C unused
        c->prior.assign((size_t)c->dense_C, 0.f);
        SysFlat flat{P, c->sysdesc, c->prior.data()};
        for (int s = 0; s < S; ++s) flat.recur(s, S - 1, c->sysdesc.N - 1, 1);
        float* psi = c->prior.data() + P.phi_len;  // :60-90: the observation tells the operated computer's bit
        const float high = 10000.f * SYS_OBSERVE, low = 10000.f * (1 - SYS_OBSERVE);
        for (int a = 0; a < A; ++a)
            for (int ns = 0; ns < S; ++ns) {
                const int up = (ns >> (a % c->sysdesc.N)) & 1;
                psi[(a * S + ns) * O + up]     = high;
                psi[(a * S + ns) * O + 1 - up] = low;
            }
        return FBA_OK;
    }
    if (is_ca(P.domain)) {
        // CollisionAvoidanceTablePrior (CollisionAvoidancePriors.cpp:65-208).  For state (x, y, b) and every
        // obstacle configuration b': transition count to (x-1, y', b') = prod_i obstacleTransProb(b_i, b'_i) * -C
        // (none from x = 0; the product stops at its first zero), observation count of b' in that state =
        // prod_i observationDistr(H, b_i)[b'_i] * 10000.
        const CADesc& ca = c->cadesc;
        const int W = ca.W, H = ca.H, n = ca.n, Hn = ca.Hn;
        if (!(noise < .5 && noise > -.5)) return fail(c, FBA_EINVAL, "CollisionAvoidanceTablePrior needs -.5 < noise < .5 (is: %f)", noise);
        c->prior.assign((size_t)c->dense_C, 0.f);
        float* phi = c->prior.data();
        float* psi = c->prior.data() + P.phi_len;
        auto trans = [&](int y, int ny) -> double {  // obstacleTransProb :136-170
            const int dist = std::abs(y - ny);
            if (dist > 1) return 0;
            if (y == 0 || y == H - 1) return dist == 0 ? .75 + .5 * noise : .25 - .5 * noise;
            return dist == 0 ? .5 + noise : .25 - .5 * noise;
        };
        auto seen = [&](int pos, int oy) -> float {  // observationDistr(height, obstacle_pos) :46-63
            if (oy == 0) return (float)normal_cdf(-pos + .5);
            if (oy == H - 1) return (float)normal_cdf(-(H - 1 - pos) + .5);
            const int dist = std::abs(oy - pos);
            return (float)(normal_cdf(dist + .5) - normal_cdf(dist - .5));
        };
        for (int ob = 0; ob < Hn; ++ob)
            for (int nob = 0; nob < Hn; ++nob) {
                int b[MAXF], nb[MAXF], r1 = ob, r2 = nob;
                for (int i = n - 1; i >= 0; --i) { b[i] = r1 % H; r1 /= H; nb[i] = r2 % H; r2 /= H; }
                double tprob = 1, oprob = 1;
                for (int i = 0; i < n && tprob != 0; ++i) tprob *= trans(b[i], nb[i]);
                for (int i = 0; i < n; ++i) oprob *= seen(b[i], nb[i]);
                for (int x = 0; x < W; ++x)
                    for (int y = 0; y < H; ++y) {
                        const int s = (x * H + y) * Hn + ob;
                        for (int a = 0; a < A; ++a) {
                            psi[((size_t)a * S + s) * O + nob] = (float)(oprob * 10000);
                            if (x == 0 || tprob == 0) continue;
                            int ny = y + a - 1;
                            if (ny == -1 || ny == H) ny = y;
                            phi[((size_t)s * A + a) * S + ((x - 1) * H + ny) * Hn + nob] = (float)(tprob * total);
                        }
                    }
            }
        return FBA_OK;
    }
    if (P.domain == FBA_DOM_GRIDWORLD) {
        // GridWorldFlatBAPrior (GridWorldBAPriors.cpp:21-156).  Transition counts accumulate (a move
        // into a wall and a failed move are the same cell; on a goal the next goal is uniform);
        // observation counts = P(o | s') * 100000 for the observations that carry s' own goal.
        const GridDesc& g = c->gdesc;
        const int N = g.N, G = g.G;
        if (noise < 0 || noise > (1 - .15))
            return fail(c, FBA_EINVAL, "Gridworld expects noise in between 0 and %f (received %f)", 1 - .15, noise);
        c->prior.assign((size_t)c->dense_C, 0.f);
        float* phi = c->prior.data();
        float* psi = c->prior.data() + P.phi_len;
        for (int a = 0; a < A; ++a)
            for (int s = 0; s < S; ++s) {
                const int ax = s / (N * G), ay = (s / G) % N, gl = s % G;
                const bool on_goal = g.goal[gl][0] == ax && g.goal[gl][1] == ay;
                const float success = gw_slow_at_h(g, ax, ay) ? (float)(.15 + noise) : (float).95;
                const float goal_prob = (float)1 / (float)G;
                float* row = phi + ((size_t)s * A + a) * S;
                int nx = ax, ny = ay;
                gw_move_h(g, a, nx, ny);
                if (on_goal) {  // the move fails / succeeds, then the goal is re-drawn uniformly (:76-88, :104-117)
                    const float stay = (1 - success) * goal_prob, go = success * goal_prob;
                    for (int g2 = 0; g2 < G; ++g2) row[(ax * N + ay) * G + g2] += stay * total;
                    for (int g2 = 0; g2 < G; ++g2) row[(nx * N + ny) * G + g2] += go * total;
                } else {
                    const float stay = 1 - success;
                    row[s] += stay * total;
                    row[(nx * N + ny) * G + gl] += success * total;
                }
                for (int x = 0; x < N; ++x)
                    for (int y = 0; y < N; ++y) {
                        const double prob = (double)(gw_obs_displ_prob_h(g, ax, x) * gw_obs_displ_prob_h(g, ay, y));
                        psi[((size_t)a * S + s) * O + (x * N + y) * G + gl] = (float)(prob * 100000.0f);
                    }
            }
        return FBA_OK;
    }
    if (noise <= -.15 || noise > .3) return fail(c, FBA_EINVAL, "noise has to be between -.15 and .3");
    const float acc = (.85f - noise) * total, inacc = (.15f + noise) * total;
    c->prior.assign((size_t)c->dense_C, 5000.f);
    float* phi = c->prior.data();
    float* psi = c->prior.data() + P.phi_len;
    const int listen = 2;
    if (dom_is_tiger(P.domain)) {
        phi[1 * A * S + listen * S + 0] = 0;
        phi[0 * A * S + listen * S + 1] = 0;
        psi[listen * S * O + 1 * O + 1] = acc;
        psi[listen * S * O + 1 * O + 0] = inacc;
        psi[listen * S * O + 0 * O + 1] = inacc;
        psi[listen * S * O + 0 * O + 0] = acc;
    } else if (dom_is_ftiger(P.domain)) {
        for (int s = 0; s < S; ++s)
            for (int ns = 0; ns < S; ++ns)
                if (s != ns) phi[s * A * S + listen * S + ns] = 0;
        for (int s = 0; s < S; ++s) {
            const bool left = s < S / 2;
            psi[listen * S * O + s * O + (left ? 0 : 1)] = acc;
            psi[listen * S * O + s * O + (left ? 1 : 0)] = inacc;
        }
    } else {
        return fail(c, FBA_EINVAL, "domain %d has no built-in tabular prior; use fba_set_model_tabular", P.domain);
    }
    return FBA_OK;
}

void fdesc_steps(const int32_t* size, int n, int32_t* step)
{
    step[n - 1] = 1;
    for (int i = n - 2; i >= 0; --i) step[i] = step[i + 1] * size[i + 1];
}

// Factored model description + base prior record for episodic/continuous factored tiger.
// FactoredTigerFactoredPrior ctor (reference src/domains/tiger/FactoredTigerPriors.cpp:95-195):
//   T listen (a = 2): feature f depends on feature f only, count 5000 on "keeps its value";
//   T open: no parents, {5000, 5000};  O open: no parents, {5000, 5000};
//   O listen: parents are per particle (structure prior), filled on the device by
//   ftiger_set_observation_model; the base record carries the correct structure {tiger location}.
// GridWorldFactBAPrior ctor + preComputePrior (reference
// src/domains/gridworld/GridWorldBAPriors.cpp:158-198, 316-413): correct-structure prior.
// Features {x, y, goal}; T parents x:{x,y}, y:{x,y}, goal:{x,y,goal}; O parents x_obs:{x},
// y_obs:{y}, goal_obs:{goal}.  The x / y transition nodes own room for the goal as a third parent
// (structure prior match-uniform, filled per particle on the device).
int build_gridworld_factored_prior(fba_ctx* c)
{
    Problem& P = c->P;
    const GridDesc& g = c->gdesc;
    const int N = g.N, G = g.G, A = P.A;
    const float noise = c->cfg.noise, total = c->cfg.counts_total, static_total = 100000;
    if (noise < 0 || noise > (1 - .15)) return fail(c, FBA_EINVAL, "Gridworld expects noise in between 0 and %f (received %f)", 1 - .15, noise);
    if (c->cfg.structure_prior != FBA_SP_NONE && c->cfg.structure_prior != FBA_SP_MATCH_UNIFORM)
        return fail(c, FBA_EINVAL, "Please enter a valid structure noise option for the GridWorld problem ('match-uniform' or 'match-counts')");
    FDesc& d = c->fdesc;
    std::memset(&d, 0, sizeof d);
    d.FS = d.FO = 3;
    d.Ssz[0] = d.Ssz[1] = d.Osz[0] = d.Osz[1] = N;
    d.Ssz[2] = d.Osz[2] = G;
    fdesc_steps(d.Ssz, 3, d.Sstep);
    fdesc_steps(d.Osz, 3, d.Ostep);
    int off = 0, nvar = 0;
    for (int a = 0; a < A; ++a)
        for (int f = 0; f < 3; ++f) {
            FNode& nd = d.nodes[a * 3 + f];
            nd.off = off; nd.nmax = 3; nd.maxp[0] = 0; nd.maxp[1] = 1; nd.maxp[2] = 2;
            if (f < 2) { nd.out = N; nd.var = nvar++; nd.fixed_mask = 3; off += N * N * G * N; }
            else { nd.out = G; nd.var = -1; nd.fixed_mask = 7; off += N * N * G * G; }
        }
    for (int a = 0; a < A; ++a)
        for (int f = 0; f < 3; ++f) {
            FNode& nd = d.nodes[A * 3 + a * 3 + f];
            nd.off = off; nd.nmax = 1; nd.maxp[0] = (uint8_t)f; nd.var = -1; nd.fixed_mask = 1;
            nd.out = d.Osz[f];
            off += d.Ssz[f] * d.Osz[f];
        }
    d.ncounts = off;
    d.nvar    = nvar;
    c->prior.assign((size_t)off + nvar, 0.f);
    float* pr = c->prior.data();
    for (int a = 0; a < A; ++a) {
        for (int f = 0; f < 2; ++f)
            for (int v = 0; v < N; ++v)
                for (int x = 0; x < N; ++x) pr[d.nodes[A * 3 + a * 3 + f].off + v * N + x] = gw_obs_displ_prob_h(g, v, x) * static_total;
        for (int v = 0; v < G; ++v) pr[d.nodes[A * 3 + a * 3 + 2].off + v * G + v] = static_total;
        for (int x = 0; x < N; ++x)
            for (int y = 0; y < N; ++y) {
                int nx = x, ny = y;
                const float trans_prob = gw_slow_at_h(g, x, y) ? (float)(.15 + (double)noise) : (float).95;
                gw_move_h(g, a, nx, ny);
                float* rx = pr + d.nodes[a * 3 + 0].off + (x * N + y) * N;
                float* ry = pr + d.nodes[a * 3 + 1].off + (x * N + y) * N;
                rx[x] += (1 - trans_prob) * total;
                ry[y] += (1 - trans_prob) * total;
                rx[nx] += (trans_prob)*total;
                ry[ny] += (trans_prob)*total;
                for (int gl = 0; gl < G; ++gl) {
                    float* row = pr + d.nodes[a * 3 + 2].off + ((x * N + y) * G + gl) * G;
                    if (g.goal[gl][0] != x || g.goal[gl][1] != y) row[gl] = static_total;
                    else for (int ng = 0; ng < G; ++ng) row[ng] = static_total;
                }
            }
        const uint32_t m3 = 3u;
        std::memcpy(&pr[off + d.nodes[a * 3 + 0].var], &m3, 4);
        std::memcpy(&pr[off + d.nodes[a * 3 + 1].var], &m3, 4);
    }
    return FBA_OK;
}

// CollisionAvoidanceFactoredPrior ctor (reference
// src/domains/collision-avoidance/CollisionAvoidancePriors.cpp:210-347, obstacleTransition :385-404,
// observationDistr :46-63) for the fixed structures: "" / match-counts (every obstacle depends on
// itself) and fully-connected (every obstacle depends on all features).  Features
// {x, y, obstacle_1..n}; observation features = the n observed obstacle rows.
int build_ca_factored_prior(fba_ctx* c)
{
    Problem& P = c->P;
    const CADesc& ca = c->cadesc;
    const int A = P.A, W = ca.W, H = ca.H, n = ca.n, FS = 2 + n;
    const float noise = c->cfg.noise, total = c->cfg.counts_total;
    const bool full = c->cfg.structure_prior == FBA_SP_FULLY_CONNECTED;
    if (noise > .5 || noise < -.5) return fail(c, FBA_EINVAL, "CollisionAvoidanceFactoredPrior must be intiiated with -.5 < noise < .5 (is: %f)", noise);
    // edge noise "uniform" / "match-uniform" (:349-383): every obstacle node's parents are drawn per particle
    // (on the device, factored_prior_sample); the node owns room for every state feature as a parent
    // (the reinvigoration belief breeds particles with structures of their own: same layout)
    const bool noisy = c->cfg.structure_prior == FBA_SP_UNIFORM || c->cfg.structure_prior == FBA_SP_MATCH_UNIFORM ||
                       ((c->cfg.belief == FBA_BELIEF_REINVIGORATION || c->cfg.belief == FBA_BELIEF_INCUBATOR || c->cfg.belief == FBA_BELIEF_MH_GIBBS ||
                         c->cfg.belief == FBA_BELIEF_MH_NIPS) && !full);
    if (FS > MAXF || A * (FS + n) > MAXNODES) return fail(c, FBA_EINVAL, "too many state features");
    FDesc& d = c->fdesc;
    std::memset(&d, 0, sizeof d);
    d.FS = FS; d.FO = n;
    d.Ssz[0] = W; d.Ssz[1] = H;
    for (int f = 0; f < n; ++f) { d.Ssz[2 + f] = H; d.Osz[f] = H; }
    fdesc_steps(d.Ssz, FS, d.Sstep);
    fdesc_steps(d.Osz, n, d.Ostep);
    int off = 0;
    for (int a = 0; a < A; ++a)
        for (int f = 0; f < FS; ++f) {
            FNode& nd = d.nodes[a * FS + f];
            nd.off = off; nd.out = d.Ssz[f]; nd.var = -1;
            if (f >= 2 && (full || noisy)) {
                int rows = 1;
                nd.nmax = FS;
                for (int k = 0; k < FS; ++k) { nd.maxp[k] = (uint8_t)k; rows *= d.Ssz[k]; }
                nd.fixed_mask = (1u << FS) - 1u;
                if (noisy) nd.var = a * n + (f - 2);
                off += rows * H;
            } else {
                nd.nmax = 1; nd.maxp[0] = (uint8_t)f; nd.fixed_mask = 1;
                off += d.Ssz[f] * d.Ssz[f];
            }
        }
    for (int a = 0; a < A; ++a)
        for (int f = 0; f < n; ++f) {
            FNode& nd = d.nodes[A * FS + a * n + f];
            nd.off = off; nd.out = H; nd.var = -1; nd.nmax = 1; nd.maxp[0] = (uint8_t)(2 + f); nd.fixed_mask = 1;
            off += H * H;
        }
    d.ncounts = off;
    d.nvar    = noisy ? A * n : 0;
    c->prior.assign((size_t)off + d.nvar, 0.f);
    float* pr = c->prior.data();
    auto obstacle_transition = [&](int y, float* out) {
        const float move_prob = (float)(.25 - .5 * noise);
        const float stay_prob = (y == 0 || y == H - 1) ? (float)(3 * .25 + .5 * noise) : (float)(2 * .25 + noise);
        for (int k = 0; k < H; ++k) out[k] = 0;
        if (y != 0) out[y - 1] = move_prob * total;
        if (y != H - 1) out[y + 1] = move_prob * total;
        out[y] = stay_prob * total;
    };
    for (int a = 0; a < A; ++a) {
        for (int x = 1; x < W; ++x) pr[d.nodes[a * FS + 0].off + x * W + (x - 1)] = 1;
        for (int y = 0; y < H; ++y) pr[d.nodes[a * FS + 1].off + y * H + std::max(0, std::min(H - 1, y + a - 1))] += 1;
        for (int f = 2; f < FS; ++f) {
            const FNode& nd = d.nodes[a * FS + f];
            if (noisy) {  // the base record carries the correct graph {f}; every particle overwrites it
                for (int y = 0; y < H; ++y) obstacle_transition(y, pr + nd.off + y * H);
                const uint32_t own = 1u << f;
                std::memcpy(&pr[off + nd.var], &own, 4);
            } else if (!full) {
                for (int y = 0; y < H; ++y) obstacle_transition(y, pr + nd.off + y * H);
            } else {
                int rows = 1;
                for (int k = 0; k < FS; ++k) rows *= d.Ssz[k];
                for (int r = 0; r < rows; ++r) obstacle_transition((r / d.Sstep[f]) % d.Ssz[f], pr + nd.off + r * H);
            }
        }
        for (int f = 0; f < n; ++f)
            for (int y = 0; y < H; ++y) {
                float* row = pr + d.nodes[A * FS + a * n + f].off + y * H;
                row[0] = (float)normal_cdf(-y + .5);
                for (int oy = 1; oy < H - 1; ++oy) {
                    const int dist = std::abs(oy - y);
                    row[oy] = (float)(normal_cdf(dist + .5) - normal_cdf(dist - .5));
                }
                row[H - 1] = (float)normal_cdf(-(H - 1 - y) + .5);
                for (int oy = 0; oy < H; ++oy) row[oy] *= 10000;
            }
    }
    return FBA_OK;
}

int build_ftiger_factored_prior(fba_ctx* c);

// SysAdminFactoredPrior (SysAdminFactoredPrior.cpp:17-45, 129-257, 279-333).  One binary feature per
// computer; transition node (a, c): parents {c} (independent) or {c-1, c, c+1} (linear), counts
// {p, 1-p} * 10000 with p = computeFailureProbability; observation node (a): parent {a mod N}.
// "Structure noise is not enabled for the Sysadmin problem": nothing is drawn per particle.
int build_sysadmin_factored_prior(fba_ctx* c)
{
    Problem& P = c->P;
    const int A = P.A, N = c->sysdesc.N;
    const bool linear = P.domain == FBA_DOM_SYSADMIN_LINEAR;
    const bool reinvig = c->cfg.belief == FBA_BELIEF_REINVIGORATION || c->cfg.belief == FBA_BELIEF_INCUBATOR ||
                         c->cfg.belief == FBA_BELIEF_MH_GIBBS || c->cfg.belief == FBA_BELIEF_MH_NIPS;   // particles with structures of their own
    if (c->cfg.structure_prior != FBA_SP_NONE) return fail(c, FBA_EINVAL, "Structure noise is not enabled for the Sysadmin problem");
    if (N > MAXF || A * (N + 1) > MAXNODES) return fail(c, FBA_EINVAL, "too many state features");
    FDesc& d = c->fdesc;
    std::memset(&d, 0, sizeof d);
    d.FS = N; d.FO = 1;
    for (int f = 0; f < N; ++f) d.Ssz[f] = 2;
    d.Osz[0] = 2;
    fdesc_steps(d.Ssz, N, d.Sstep);
    fdesc_steps(d.Osz, 1, d.Ostep);
    int off = 0;
    for (int a = 0; a < A; ++a)
        for (int f = 0; f < N; ++f) {
            FNode& nd = d.nodes[a * N + f];
            nd.off = off; nd.out = 2; nd.var = -1; nd.nmax = 0;
            if (reinvig) {  // bred particles choose any parent set: room for all N, the prior's set as the base mask
                uint32_t m = 1u << f;
                if (linear && f > 0) m |= 1u << (f - 1);
                if (linear && f < N - 1) m |= 1u << (f + 1);
                for (int k = 0; k < N; ++k) nd.maxp[k] = (uint8_t)k;
                nd.nmax = N; nd.var = a * N + f; nd.fixed_mask = m;
                off += 2 << N;
                continue;
            }
            if (linear && f > 0) nd.maxp[nd.nmax++] = (uint8_t)(f - 1);
            nd.maxp[nd.nmax++] = (uint8_t)f;
            if (linear && f < N - 1) nd.maxp[nd.nmax++] = (uint8_t)(f + 1);
            nd.fixed_mask = (1u << nd.nmax) - 1u;
            off += 2 << nd.nmax;
        }
    for (int a = 0; a < A; ++a) {
        FNode& nd = d.nodes[A * N + a];
        nd.off = off; nd.out = 2; nd.var = -1; nd.nmax = 1; nd.maxp[0] = (uint8_t)(a % N); nd.fixed_mask = 1;
        off += 4;
    }
    d.ncounts = off;
    d.nvar    = reinvig ? A * N : 0;
    c->prior.assign((size_t)off + d.nvar, 0.f);
    float* pr = c->prior.data();
    for (int a = 0; a < A; ++a)
        for (int f = 0; f < N; ++f) {
            const FNode& nd = d.nodes[a * N + f];
            const bool rebooting = a == N + f;
            int parents[MAXF], np = 0;
            for (int k = 0; k < nd.nmax; ++k)
                if ((nd.fixed_mask >> k) & 1u) parents[np++] = nd.maxp[k];
            if (reinvig) std::memcpy(&pr[off + nd.var], &nd.fixed_mask, 4);
            for (int r = 0; r < (1 << np); ++r) {  // row r: parent values, last parent the fastest digit
                int failing = 0;
                bool own_up = true;
                for (int k = 0; k < np; ++k) {
                    const int v = (r >> (np - 1 - k)) & 1;
                    if (parents[k] == f) own_up = v != 0;
                    else if (!v) failing++;              // parents other than f are its linear neighbours
                }
                float p;
                if (!own_up) p = rebooting ? 1 - SYS_REBOOT : 1;   // :295-298
                else {
                    double fail = 1 - c->sysdesc.keep[failing];          // :313-315
                    if (rebooting) fail *= (1 - SYS_REBOOT);
                    p = (float)fail;
                }
                pr[nd.off + 2 * r + 0] = p * 10000.f;
                pr[nd.off + 2 * r + 1] = (1 - p) * 10000.f;
            }
        }
    for (int a = 0; a < A; ++a) {  // precomputeFactoredPrior :148-183: output 0 = FAILING
        float* o = pr + d.nodes[A * N + a].off;
        o[0] = 10000.f * SYS_OBSERVE; o[1] = 10000.f * (1 - SYS_OBSERVE);   // operated computer failing
        o[2] = 10000.f * (1 - SYS_OBSERVE); o[3] = 10000.f * SYS_OBSERVE;   // operated computer working
    }
    return FBA_OK;
}

int build_factored_prior(fba_ctx* c)
{
    if (is_sys(c->P.domain)) return build_sysadmin_factored_prior(c);
    if (is_ca(c->P.domain)) return build_ca_factored_prior(c);
    if (c->P.domain == FBA_DOM_GRIDWORLD) return build_gridworld_factored_prior(c);
    return build_ftiger_factored_prior(c);
}

int build_ftiger_factored_prior(fba_ctx* c)
{
    Problem& P = c->P;
    if (!dom_is_ftiger(P.domain)) return fail(c, FBA_EINVAL, "domain %d has no built-in factored prior", P.domain);
    const float noise = c->cfg.noise, total = c->cfg.counts_total;
    if (noise <= -.15 || noise > .3) return fail(c, FBA_EINVAL, "noise must be between -.15 and .3");
    FDesc& d = c->fdesc;
    std::memset(&d, 0, sizeof d);
    d.FS = c->cfg.size + 1;
    d.FO = 1;
    if (d.FS > MAXF) return fail(c, FBA_EINVAL, "factored tiger supports at most %d irrelevant features", MAXF - 1);
    if (P.A * (d.FS + d.FO) > MAXNODES) return fail(c, FBA_EINVAL, "too many DBN nodes");
    for (int f = 0; f < d.FS; ++f) d.Ssz[f] = 2;
    d.Osz[0] = 2;
    fdesc_steps(d.Ssz, d.FS, d.Sstep);
    fdesc_steps(d.Osz, d.FO, d.Ostep);
    int off = 0;
    for (int a = 0; a < P.A; ++a)
        for (int f = 0; f < d.FS; ++f) {
            FNode& nd = d.nodes[a * d.FS + f];
            nd.off = off; nd.out = 2; nd.var = -1;
            if (a == 2) { nd.nmax = 1; nd.maxp[0] = (uint8_t)f; nd.fixed_mask = 1; off += 4; }
            else { nd.nmax = 0; nd.fixed_mask = 0; off += 2; }
        }
    for (int a = 0; a < P.A; ++a) {
        FNode& nd = d.nodes[P.A * d.FS + a * d.FO];
        nd.off = off; nd.out = 2; nd.var = -1;
        if (a == 2) {
            nd.nmax = d.FS; nd.var = 0;
            for (int f = 0; f < d.FS; ++f) nd.maxp[f] = (uint8_t)f;
            off += 2 << d.FS;
        } else { nd.nmax = 0; off += 2; }
    }
    d.ncounts = off;
    d.nvar    = 1;
    c->prior.assign((size_t)off + d.nvar, 0.f);
    for (int a = 0; a < P.A; ++a)
        for (int f = 0; f < d.FS; ++f) {
            const FNode& nd = d.nodes[a * d.FS + f];
            if (a == 2) { c->prior[nd.off + 0] = 5000; c->prior[nd.off + 3] = 5000; }
            else { c->prior[nd.off] = 5000; c->prior[nd.off + 1] = 5000; }
        }
    for (int a = 0; a < 2; ++a) {
        const FNode& nd = d.nodes[P.A * d.FS + a * d.FO];
        c->prior[nd.off] = 5000; c->prior[nd.off + 1] = 5000;
    }
    {   // correct structure {0}: rows (LEFT, RIGHT) = (acc, inacc), (inacc, acc)
        const FNode& nd = d.nodes[P.A * d.FS + 2 * d.FO];
        const float acc = (.85f - noise) * total, inacc = (.15f + noise) * total;
        c->prior[nd.off + 0] = acc; c->prior[nd.off + 1] = inacc;
        c->prior[nd.off + 2] = inacc; c->prior[nd.off + 3] = acc;
        const uint32_t mask = 1u;
        std::memcpy(&c->prior[off + 0], &mask, 4);
    }
    return FBA_OK;
}

// PackedFtigerView::prior on the host (fba_device.h): the prior count of cell k of the factored-tiger model under the
// listen observation node's parent set `mask`
float ftiger_prior_host(int FS, int k, uint32_t mask, float acc, float inacc, float unif)
{
    if (k < 4 * FS) return 5000.f;
    if (k < 8 * FS) { const int j = k - 4 * FS; return (((j >> 1) ^ j) & 1) ? 0.f : 5000.f; }
    if (k < 8 * FS + 4) return 5000.f;
    const int j = k - (8 * FS + 4), row = j >> 1, np = __builtin_popcount(mask);
    if (row >= (1 << np)) return 0.f;
    if (!(mask & 1u)) return unif;
    return ((row >> (np - 1)) == (j & 1)) ? acc : inacc;
}

// prior[k] + j is the float the reference reaches by j additions of 1.0f for every j a uint16 holds
bool packable_prior(const std::vector<float>& prior)
{
    for (float p : prior) {
        const double top = (double)p + 65535.0;
        if (!(p >= 0.f) || (double)(float)top != top) return false;
    }
    return true;
}

// History particles (fba_device.h): GridWorldFactBAPrior::setNoisyTransitionNode (GridWorldBAPriors.cpp:255-295) for
// every action and the x / y node -- what gw_fill_xy_node_with_goal writes into a dense record on the device.
void build_gridworld_alt_prior(fba_ctx* c)
{
    const GridDesc& g = c->gdesc;
    const int N = g.N, G = g.G, A = c->P.A, XY = N * N * G * N;
    const float noise = c->cfg.noise, total = c->cfg.counts_total;
    c->prior_alt.assign((size_t)A * 2 * XY, 0.f);
    for (int a = 0; a < A; ++a)
        for (int f = 0; f < 2; ++f) {
            float* base = c->prior_alt.data() + (size_t)(a * 2 + f) * XY;
            for (int x = 0; x < N; ++x)
                for (int y = 0; y < N; ++y) {
                    int nx = x, ny = y;
                    const float trans_prob = gw_slow_at_h(g, x, y) ? (float)(.15 + (double)noise) : (float).95;
                    gw_move_h(g, a, nx, ny);
                    const int loc = f == 0 ? x : y, new_loc = f == 0 ? nx : ny;
                    for (int gl = 0; gl < G; ++gl) {
                        float* row = base + ((x * N + y) * G + gl) * N;
                        row[loc] += (1 - trans_prob) * total;
                        row[new_loc] += (trans_prob)*total;
                    }
                }
        }
}
// v + (float)j is the float that j additions of 1.0f to v reach, for every j up to `most`
bool increments_exact(const std::vector<float>& table, int most)
{
    for (float v : table) {
        if (!(v >= 0.f)) return false;
        float seq = v;
        for (int j = 1; j <= most; ++j) {
            seq += 1.0f;
            if (seq != v + (float)j) return false;
        }
    }
    return true;
}

// Collision-avoidance history particles (CaTables, fba_device.h): which cells of the prior are not exact under prior + (float)j, j <= most,
// and for every distinct value among them the floats that j additions of 1.0f reach.  sid[k] = 0 (exact) or 1 + the row of `seq`
// ([rows][most + 1]).  False when a count is negative or more than CA_HIST_MAX_SEQ distinct values need a row.
bool ca_hist_sequences(const std::vector<float>& table, int ncounts, int most, std::vector<uint8_t>& sid, std::vector<float>& seq)
{
    sid.assign((size_t)ncounts, 0);
    seq.clear();
    std::vector<float> values;
    for (int k = 0; k < ncounts; ++k) {
        const float v = table[(size_t)k];
        if (!(v >= 0.f)) return false;
        if (increments_exact(std::vector<float>{v}, most)) continue;
        size_t id = 0;
        while (id < values.size() && std::memcmp(&values[id], &v, 4) != 0) ++id;
        if (id == values.size()) {
            if (values.size() >= (size_t)CA_HIST_MAX_SEQ) return false;
            values.push_back(v);
            float run = v;
            for (int j = 0; j <= most; ++j) { seq.push_back(run); run += 1.0f; }
        }
        sid[(size_t)k] = (uint8_t)(id + 1);
    }
    return true;
}

// The sparse rows of a tabular prior (TabRows, fba_device.h): row offsets, then {column, fp32 count} pairs of the nonzero columns, ascending
std::vector<uint32_t> tab_sparse_rows(const Problem& P, const std::vector<float>& prior)
{
    const int S = P.S, A = P.A, O = P.O, R = 2 * A * S;
    std::vector<uint32_t> ptr((size_t)tab_cols_word(A, S), 0u), cols;
    for (int r = 0; r < R; ++r) {
        ptr[(size_t)r] = (uint32_t)(cols.size() / 2);
        const size_t off = r < A * S ? (size_t)r * S : (size_t)P.phi_len + (size_t)(r - A * S) * O;
        const int n = r < A * S ? S : O;
        for (int i = 0; i < n; ++i)
            if (prior[off + i] != 0.f) {
                uint32_t bits;
                std::memcpy(&bits, &prior[off + i], 4);
                cols.push_back((uint32_t)i);
                cols.push_back(bits);
            }
    }
    ptr[(size_t)R] = (uint32_t)(cols.size() / 2);
    ptr.insert(ptr.end(), cols.begin(), cols.end());
    return ptr;
}

int upload_prior(fba_ctx* c)
{
    std::vector<float> padded((size_t)c->P.Cs, 0.f);
    if (c->P.ft_packed) {  // the prior record in packed form: no increments, the correct structure's bits
        const uint32_t m = 1u;
        std::memcpy(&padded[(size_t)c->fdesc.ncounts / 2], &m, 4);
    } else if (c->P.hist == 2) {
        // tabular records: the prior's nonzero columns per row (TabRows, fba_device.h), and the dense table for the belief checksum
        // (flush_kernel) and fba_belief_get
        if (!increments_exact(c->prior, c->P.hist_cap + 1))
            return fail(c, FBA_EINVAL, "this context stores particles as histories over the prior table, which needs prior counts c with c + j exact "
                                       "in fp32 for j <= %d; create it with FBA_DENSE_PARTICLES=1 in the environment for other tables", c->P.hist_cap + 1);
        const std::vector<uint32_t> rows = tab_sparse_rows(c->P, c->prior);
        dev_free(c, c->d_tab_rows);
        if (const int rc = dev_alloc(c, &c->d_tab_rows, rows.size(), false)) return rc;
        HIPCHK(c, hipMemcpyAsync(c->d_tab_rows, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_prior_dense, c->prior.data(), c->prior.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (rows is a local)
        c->P.hist_base = reinterpret_cast<const float*>(c->d_tab_rows);
    } else if (c->P.hist == 3) {
        // collision-avoidance records: the dense prior table (staged in LDS by every kernel that steps; fba_belief_get and the belief
        // checksum read it too) and, beside it, which of its cells are inexact under prior + j and their sequences (CaTables)
        std::vector<uint8_t> sid;
        std::vector<float> seq;
        const int nc = c->fdesc.ncounts;
        if (!ca_hist_sequences(c->prior, nc, c->P.hist_cap + 1, sid, seq))
            return fail(c, FBA_EINVAL, "this context stores particles as histories over the prior table, which holds at most %d distinct counts c for which "
                                       "c + j is not exact in fp32; create it with FBA_DENSE_PARTICLES=1 in the environment for other tables", CA_HIST_MAX_SEQ);
        const int rid_bytes = (nc + 15) & ~15;
        std::vector<uint8_t> blob((size_t)rid_bytes + (size_t)CA_HIST_MAX_SEQ * (c->P.hist_cap + 2) * sizeof(float) + 16, 0);
        std::copy(sid.begin(), sid.end(), blob.begin());
        if (!seq.empty()) std::memcpy(blob.data() + rid_bytes, seq.data(), seq.size() * sizeof(float));
        HIPCHK(c, hipMemcpyAsync(c->d_hist_lds, blob.data(), blob.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_prior_dense, c->prior.data(), (size_t)nc * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (blob is a local)
        c->P.hist_base      = c->d_prior_dense;
        c->P.hist_lds       = c->d_hist_lds;
        c->P.hist_rid_bytes = rid_bytes;
        c->P.hist_distinct  = (int)(seq.size() / (size_t)(c->P.hist_cap + 2));
    } else if (c->P.hist) {  // records carry no counts: the tables sit beside them, rows padded to 16 bytes (HistLayout, fba_device.h)
        const HistLayout L(c->gdesc.N, c->gdesc.G, c->P.A);
        const int N = L.N, G = L.G, A = L.A, XYd = N * N * G * N, GGd = N * N * G * G, NNd = N * N;
        std::vector<float> base((size_t)L.total + 16, 0.f), alt((size_t)L.alt_total + 16, 0.f);
        const float* pr = c->prior.data();
        for (int a = 0; a < A; ++a) {
            const int td = a * (2 * XYd + GGd), od = A * (2 * XYd + GGd) + a * (2 * NNd + G * G);
            for (int f = 0; f < 2; ++f)
                for (int row = 0; row < N * N * G; ++row)
                    for (int i = 0; i < N; ++i) {
                        if (row < N * N) base[(size_t)a * L.tstride + f * L.XY + row * L.NS + i] = pr[td + f * XYd + row * N + i];
                        alt[(size_t)(a * 2 + f) * L.XY + row * L.NS + i] = c->prior_alt[(size_t)(a * 2 + f) * XYd + row * N + i];
                    }
            for (int row = 0; row < N * N * G; ++row)
                for (int i = 0; i < G; ++i) base[(size_t)a * L.tstride + 2 * L.XY + row * L.GS + i] = pr[td + 2 * XYd + row * G + i];
            for (int f = 0; f < 3; ++f) {
                const int n = f == 2 ? G : N;
                for (int v = 0; v < n; ++v)
                    for (int i = 0; i < n; ++i) base[(size_t)L.o_row(a, f, v) + i] = pr[od + (f == 2 ? 2 * NNd : f * NNd) + v * n + i];
            }
        }
        HIPCHK(c, hipMemcpyAsync(c->d_hist_base, base.data(), base.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_hist_alt, alt.data(), alt.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        {
            // the same rows deduplicated (Problem::hist_lds): a row slot -> one byte, the distinct rows K floats each
            const HistRowIds I(N, G, A);
            const int K = hist_row_width(c->P.hist_row);   // (a 12-float row is walked to 10: HistRow::KL)
            const int rid_bytes = (I.total + 15) & ~15;
            std::vector<uint8_t> blob((size_t)rid_bytes, 0);
            std::vector<float> rows;
            std::map<std::vector<uint32_t>, int> ids;
            bool fits = true;
            auto put = [&](int slot, const float* src, int n) {
                std::vector<uint32_t> key((size_t)K, 0u);
                for (int i = 0; i < n; ++i) std::memcpy(&key[i], &src[i], 4);
                auto it = ids.find(key);
                if (it == ids.end()) {
                    if (ids.size() >= 256) { fits = false; return; }
                    it = ids.emplace(key, (int)ids.size()).first;
                    for (int i = 0; i < K; ++i) { float f; std::memcpy(&f, &key[i], 4); rows.push_back(f); }
                }
                blob[(size_t)slot] = (uint8_t)it->second;
            };
            for (int a = 0; a < A && fits; ++a) {
                for (int f = 0; f < 2; ++f)
                    for (int cell = 0; cell < N * N; ++cell) put(I.t(a, f, false, cell, 0), &base[(size_t)L.t_row(a, f, false, cell, 0)], N);
                for (int cell = 0; cell < N * N; ++cell)
                    for (int gl = 0; gl < G; ++gl) {
                        put(I.t(a, 2, true, cell, gl), &base[(size_t)L.t_row(a, 2, true, cell, gl)], G);
                        for (int f = 0; f < 2; ++f) put(I.t(a, f, true, cell, gl), &alt[(size_t)L.alt_row(a, f, cell, gl)], N);
                    }
                for (int f = 0; f < 3; ++f)
                    for (int v = 0; v < (f == 2 ? G : N); ++v) put(I.o(a, f, v), &base[(size_t)L.o_row(a, f, v)], f == 2 ? G : N);
            }
            if (fits) {
                const size_t nb = blob.size();
                blob.resize(nb + rows.size() * sizeof(float));
                std::memcpy(blob.data() + nb, rows.data(), rows.size() * sizeof(float));
                HIPCHK(c, hipMemcpyAsync(c->d_hist_lds, blob.data(), blob.size(), hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));   // (blob is a local)
                c->P.hist_lds       = c->d_hist_lds;
                c->P.hist_rid_bytes = rid_bytes;
                c->P.hist_distinct  = (int)ids.size();
            } else {
                c->P.hist_lds = nullptr; c->P.hist_rid_bytes = 0; c->P.hist_distinct = 0;
            }
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else if (c->P.packed) {  // records start as "no increments yet"; the table itself goes beside them
        if (!packable_prior(c->prior))
            return fail(c, FBA_EINVAL, "this context stores particles packed (uint16 increments over the prior), which needs prior counts c with "
                                       "c + 65535 exact in fp32; create it with FBA_DENSE_PARTICLES=1 in the environment for other tables");
        HIPCHK(c, hipMemcpyAsync(c->d_prior_dense, c->prior.data(), c->prior.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    } else if (!c->P.ft_packed)
        std::copy(c->prior.begin(), c->prior.end(), padded.begin());
    HIPCHK(c, hipMemcpyAsync(c->d_prior, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FBA_OK;
}

// ---- timed launches ---------------------------------------------------------------------------
int flush_events(fba_ctx* c)
{
    if (c->pending.empty()) return FBA_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto& p : c->pending) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, p.a, p.b));
        c->k_ms[p.kind] += ms;
        c->k_launches[p.kind] += 1;
        c->free_events.push_back(p);
    }
    c->pending.clear();
    return FBA_OK;
}

template <typename F>
int timed(fba_ctx* c, int kind, F&& launch)
{
    if (!c->timing) {
        launch();
        if (const hipError_t le = launch_take_error(); le != hipSuccess) return fail(c, FBA_EHIP, "inside a kernel launch sequence: %s", hipGetErrorString(le));
        return FBA_OK;
    }
    if (c->pending.size() >= 2048) {
        int rc = flush_events(c);
        if (rc) return rc;
    }
    EventPair p;
    if (!c->free_events.empty()) {
        p = c->free_events.back();
        c->free_events.pop_back();
    } else {
        HIPCHK(c, hipEventCreate(&p.a));
        HIPCHK(c, hipEventCreate(&p.b));
    }
    p.kind = kind;
    HIPCHK(c, hipEventRecord(p.a, c->stream));
    launch();
    HIPCHK(c, hipEventRecord(p.b, c->stream));
    c->pending.push_back(p);
    if (const hipError_t le = launch_take_error(); le != hipSuccess) return fail(c, FBA_EHIP, "inside a kernel launch sequence: %s", hipGetErrorString(le));
    return FBA_OK;
}

int k_update_kind(const fba_ctx* c) { return c->P.belief == FBA_BELIEF_REJECTION ? FBA_K_BELIEF_RS : FBA_K_BELIEF_IS; }

// Every slot in 64-byte records: in front of everything outside tick() that reads or writes p_rec.  Where no tick has run compact since
// the last call (fba_state.h) nothing is launched -- but for the callers that want pending lazy resets written out whatever the
// format (`reset`: where launch_materialize_reset stood before compact filters existed)
void materialize_records(fba_ctx* c, bool reset = false)
{
    if (c->compact_dirty) launch_materialize_records(c->P, c->D, c->stream);
    else if (reset) launch_materialize_reset(c->P, c->D, c->stream);
    c->compact_dirty = false;
    c->D.compact_on  = 0;   // the per-call launches never leave a slot compact
    c->D.retire_on   = 0;   // ... and never retire a run: a per-call update that gives up is an error of its call (check_fault)
}

// Belief::initiate of the slots that start a run: drawn from the prior, or -- in a resumed span -- taken from the snapshot store
void launch_initiate(fba_ctx* c)
{
    if (c->D.restore_store) launch_restore(c->P, c->D, c->stream);
    else launch_init(c->P, c->D, c->stream);
}

// fba_step_stats: the slots that took their step in this tick, reduced into their bins (fba_step_stats.hip; in no time bucket)
int launch_tick_step_stats(fba_ctx* c)
{
    StepStatsArgs a = c->step_stats;
    a.probe_first = c->probe.first; a.probe_count = c->probe.count; a.probe_step = c->probe.step;
    if (!c->step_stats_timed) {
        launch_step_stats(c->P, c->D, a, c->stream);
        return FBA_OK;
    }
    hipEvent_t ev[2];
    HIPCHK(c, hipEventCreate(&ev[0]));
    HIPCHK(c, hipEventCreate(&ev[1]));
    HIPCHK(c, hipEventRecord(ev[0], c->stream));
    launch_step_stats(c->P, c->D, a, c->stream);
    HIPCHK(c, hipEventRecord(ev[1], c->stream));
    HIPCHK(c, hipEventSynchronize(ev[1]));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    c->step_stats_ms += ms;
    c->step_stats_launches += 1;
    return FBA_OK;
}

// fba_structure_stats: the main filters of the slots that took their step in this tick, a chunk of slots at a time, reduced into their
// bins (fba_structure_stats.hip; in no time bucket)
int launch_tick_structure_stats(fba_ctx* c)
{
    StructStatsArgs a = c->struct_stats;
    hipEvent_t ev[2];
    if (c->struct_stats_timed) {
        HIPCHK(c, hipEventCreate(&ev[0]));
        HIPCHK(c, hipEventCreate(&ev[1]));
        HIPCHK(c, hipEventRecord(ev[0], c->stream));
    }
    for (int done = 0; done < c->P.E; done += a.chunk) {
        a.first = done;
        a.count = std::min(a.chunk, c->P.E - done);
        launch_structure_stats(c->P, c->D, a, c->stream);
    }
    if (!c->struct_stats_timed) return FBA_OK;
    HIPCHK(c, hipEventRecord(ev[1], c->stream));
    HIPCHK(c, hipEventSynchronize(ev[1]));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    c->struct_stats_ms += ms;
    c->struct_stats_launches += 1;
    return FBA_OK;
}

// one real time-step of every active slot
int tick(fba_ctx* c)
{
    int rc;
    c->D.compact_on = c->compact_ok && c->probe.count == 0 ? 1 : 0;   // (the probe reads records)
    if (c->D.compact_on) c->compact_dirty = true;
    c->D.retire_on = c->giveup_policy == FBA_GIVEUP_RETIRE && c->retired.recs ? 1 : 0;
    if ((rc = timed(c, FBA_K_SEARCH, [&] { launch_search(c->P, c->D, c->stream); }))) return rc;
    if ((rc = timed(c, FBA_K_ENV, [&] { launch_env(c->P, c->D, c->d_n_active, c->stream); }))) return rc;
    if (c->probe.count > 0) launch_belief_probe(c->P, c->D, c->probe, c->stream);   // (the slots env_kernel has just flagged for an update; in no time bucket)
    if (c->struct_stats.bins)
        if ((rc = launch_tick_structure_stats(c))) return rc;   // (adv, episode and t address the step; the filter has not seen it)
    if ((rc = timed(c, k_update_kind(c), [&] { launch_belief_update(c->P, c->D, c->stream); }))) return rc;
    if (c->D.retire_on) launch_retire(c->P, c->D, c->retired, c->stream);   // (the slots whose update has just given up; in no time bucket)
    if (c->D.trace_on) launch_flush(c->P, c->D, c->stream);
    if (c->step_stats.bins)
        if ((rc = launch_tick_step_stats(c))) return rc;   // (update_count is written; t and episode still address the step)
    launch_advance(c->P, c->D, c->d_n_active, c->stream);
    if ((rc = timed(c, FBA_K_BELIEF_INIT, [&] { launch_initiate(c); }))) return rc;
    if (c->P.model != FBA_MODEL_POMDP)
        if ((rc = timed(c, FBA_K_BELIEF_RESET, [&] { launch_reset(c->P, c->D, c->stream); }))) return rc;
    HIPCHK(c, hipGetLastError());
    return FBA_OK;
}

// after a synchronisation point: did a rejection update give up (Problem::reject_max; under FBA_GIVEUP_RETIRE a tick raises no fault for that)?
int check_fault(fba_ctx* c)
{
    int32_t f = 0;
    HIPCHK(c, hipMemcpy(&f, c->D.fault, sizeof f, hipMemcpyDeviceToHost));
    if (!f) return FBA_OK;
    HIPCHK(c, hipMemset(c->D.fault, 0, sizeof f));
    if (f >= 0x20000000 && f < 0x40000000)
        return fail(c, FBA_ESTATE, "%s in slot %d: the sampled model cannot reproduce the run's history (the reference would never "
                    "return from %s)", c->P.mh == 3 ? "mh-nips" : "mh-within-gibbs", f - 0x20000000,
                    c->P.mh == 3 ? "computePosterior, MHNIPS2018.cpp:39-105" : "rejectionSampleStateHistory, MHwithinGibbs.cpp:38-94");
    if (f >= 0x40000000)
        return fail(c, FBA_ESTATE, "slot %d: more belief updates in one run than the %d (episodes * horizon) a history particle was "
                    "sized for; create the context with FBA_DENSE_PARTICLES=1 in the environment to drive it beyond that", f - 0x40000000, c->P.hist_cap);
    if (f < 0 && c->D.bkt)
        return fail(c, FBA_ESTATE, "the search tree of slot %d outgrew its table of %d buckets (fba_config.tree_buckets; 0 = 2 * (sims + 2), which no search can fill)",
                    -f - 1, 2 * c->D.bkt_lines);
    if (f < 0) return fail(c, FBA_ESTATE, "the search tree of slot %d needed more than the %d node records it has", -f - 1, c->D.max_nodes);
    HIPCHK(c, hipMemset(c->D.gave_up, 0, (size_t)c->P.E));   // (the flags of the slots that gave up go with the fault that reports them)
    return fail(c, FBA_ESTATE, "rejection sampling in slot %d accepted fewer than %d particles in %d attempts: no particle of the filter "
                "can produce the observation (the reference loops forever in RejectionSampling.hpp:26-72 here)", f - 1, c->P.N,
                c->P.reject_max);
}

int set_flags(fba_ctx* c, uint8_t* dev, const uint8_t* mask, uint8_t value)
{
    std::vector<uint8_t> h((size_t)c->P.E, value);
    if (mask)
        for (int e = 0; e < c->P.E; ++e) h[e] = mask[e] ? value : 0;
    HIPCHK(c, hipMemcpyAsync(dev, h.data(), h.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FBA_OK;
}

int ensure_outputs(fba_ctx* c, int runs)
{
    const size_t need = (size_t)std::max(runs, 1) * c->P.episodes;
    if (need > c->returns_cap) {
        int rc;
        DeviceState& D = c->D;   // (re-grown like the trace: the old buffers go, and their entries of the report with them)
        dev_free(c, D.returns);
        dev_free(c, D.lengths);
        if ((rc = dev_alloc(c, ARR(returns), need))) return rc;
        if ((rc = dev_alloc(c, ARR(lengths), need))) return rc;
        c->returns_cap = need;
    } else {
        HIPCHK(c, hipMemsetAsync(c->D.returns, 0, need * sizeof(double), c->stream));
        HIPCHK(c, hipMemsetAsync(c->D.lengths, 0, need * sizeof(int32_t), c->stream));
    }
    if (c->cfg.trace) return ensure_trace(c, (size_t)std::max(runs, 1) * c->P.episodes * c->P.horizon);
    return FBA_OK;
}

// Budgeted searches park their state per slot (s_sim / s_nodes / s_depth, fba_state.h).  Whatever re-positions the slots -- a new
// experiment, fba_belief_init, fba_set_position -- makes a parked search stale: the next launch must start a search, not resume one.
int clear_parked_searches(fba_ctx* c)
{
    if (!c->D.s_sim) return FBA_OK;
    const size_t E = (size_t)c->P.E;
    HIPCHK(c, hipMemsetAsync(c->D.s_sim, 0, E * sizeof *c->D.s_sim, c->stream));
    HIPCHK(c, hipMemsetAsync(c->D.s_nodes, 0, E * sizeof *c->D.s_nodes, c->stream));
    HIPCHK(c, hipMemsetAsync(c->D.s_depth, 0, E * sizeof *c->D.s_depth, c->stream));
    HIPCHK(c, hipMemsetAsync(c->D.search_done, 0, E * sizeof *c->D.search_done, c->stream));
    return FBA_OK;
}

// first_episode, stop_episode: the span of every run (stop_episode < 0: to the last episode)
int start_experiment(fba_ctx* c, int runs_total, int first_episode = 0, int stop_episode = -1)
{
    int rc;
    if ((rc = clear_parked_searches(c))) return rc;
    materialize_records(c);   // (bufsel is rewritten below)
    c->D.runs_total = runs_total;
    c->D.run_offset = c->cfg.run_offset;
    c->D.first_episode = first_episode;
    c->D.stop_episode  = stop_episode < 0 ? c->P.episodes : stop_episode;
    const int32_t n_active = runs_total < 0 ? c->P.E : std::min(c->P.E, runs_total);
    HIPCHK(c, hipMemcpyAsync(c->d_n_active, &n_active, sizeof n_active, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->D.bufsel, 0, (size_t)c->P.E, c->stream));
    HIPCHK(c, hipMemsetAsync(c->D.lazy_reset, 0, (size_t)c->P.E, c->stream));
    HIPCHK(c, hipMemsetAsync(c->D.gave_up, 0, (size_t)c->P.E, c->stream));
    if (c->D.bufsel_fc) HIPCHK(c, hipMemsetAsync(c->D.bufsel_fc, 0, (size_t)c->P.E, c->stream));
    if (c->D.bufsel_sh) HIPCHK(c, hipMemsetAsync(c->D.bufsel_sh, 0, (size_t)c->P.E, c->stream));
    launch_start(c->P, c->D, c->stream);
    if ((rc = timed(c, FBA_K_BELIEF_INIT, [&] { launch_initiate(c); }))) return rc;
    if (c->P.model != FBA_MODEL_POMDP)
        if ((rc = timed(c, FBA_K_BELIEF_RESET, [&] { launch_reset(c->P, c->D, c->stream); }))) return rc;
    HIPCHK(c, hipGetLastError());
    c->belief_ready = true;
    return FBA_OK;
}

// Episodes [first, stop) of every run (stop < 0: all of them).  block_updates: what the blocks of a resumed span had counted (SpanStore), or null
int run_experiment(fba_ctx* c, fba_stat* stats, int first = 0, int stop = -1, const std::vector<uint32_t>* block_updates = nullptr)
{
    int rc;
    const int runs = c->cfg.runs, E = c->P.E, eps = c->P.episodes;
    if (stop < 0) stop = eps;
    const int retired0 = std::max(fba_retired_count(c, nullptr), 0);   // (the list is not cleared here: what it holds of earlier experiments)
    if ((rc = ensure_outputs(c, runs))) return rc;
    if ((rc = start_experiment(c, runs, first, stop))) return rc;
    long long max_ticks = (long long)((runs + E - 1) / E) * (stop - first) * c->P.horizon + 2;
    if (c->P.search_budget > 0)   // budgeted launches: a real step takes as many launches as its search needs (<= horizon + 1 iterations per simulation)
        max_ticks *= ((long long)c->P.sims * (c->P.horizon + 1)) / c->P.search_budget + 2;
    for (long long k = 0; k < max_ticks; ++k) {
        if ((rc = tick(c))) return rc;
        int32_t n_active = 0;
        HIPCHK(c, hipMemcpyAsync(&n_active, c->d_n_active, sizeof n_active, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if ((rc = check_fault(c))) return rc;
        if (n_active <= 0) break;
    }
    std::vector<double> ret((size_t)runs * eps);
    HIPCHK(c, hipMemcpy(ret.data(), c->D.returns, ret.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<int32_t> len((size_t)runs * eps);
    HIPCHK(c, hipMemcpy(len.data(), c->D.lengths, len.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::memset(stats, 0, sizeof(fba_stat) * (size_t)eps);
    for (int r = 0; r < runs; ++r)
        for (int ep = first; ep < stop; ++ep)
            if (len[(size_t)r * eps + ep] > 0) fba_stat_add(&stats[ep], ret[(size_t)r * eps + ep]);   // (length 0: a void episode of a retired run, fba_giveup_policy)
    if (c->P.packed || c->P.ft_packed) {
        // what a snapshot header says of a slot's uint16 increments (fba_snapshot_head::updates): the filter a slot is left with is that of
        // its last run, which has made one update per real step at most, on top of what its block had counted.  The void episodes of a
        // retired run count nothing (length 0) but the one it was retired in: t updates had succeeded before the step that gave up
        if (c->packed_updates.size() != (size_t)E) c->packed_updates.assign((size_t)E, 0);
        const int gone1 = std::max(fba_retired_count(c, nullptr), retired0);   // the records [retired0, gone1) are this experiment's
        std::vector<fba_retired_rec> gone((size_t)(gone1 - retired0));
        if (!gone.empty())
            HIPCHK(c, hipMemcpy(gone.data(), c->retired.recs + retired0, gone.size() * sizeof(fba_retired_rec), hipMemcpyDeviceToHost));
        for (int e = 0; e < E && e < runs; ++e) {
            const int r = e + E * ((runs - 1 - e) / E);
            uint32_t n = block_updates ? (*block_updates)[(size_t)r % block_updates->size()] : 0u;
            for (int ep = first; ep < stop; ++ep) n += (uint32_t)len[(size_t)r * eps + ep];
            for (const fba_retired_rec& g : gone)
                if (g.run == r + c->cfg.run_offset && !g.counted) n += (uint32_t)g.t;
            c->packed_updates[(size_t)e] = n;
        }
    }
    c->started = false;
    return FBA_OK;
}

template <typename T>
uint64_t sum_counter(fba_ctx* c, const T* dev, int n, int* rc)
{
    std::vector<unsigned long long> h((size_t)n);
    hipError_t e = hipMemcpy(h.data(), dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        *rc = fail(c, FBA_EHIP, "counter download failed: %s", hipGetErrorString(e));
        return 0;
    }
    uint64_t s = 0;
    for (auto v : h) s += v;
    return s;
}

// ==== The stages of fba_create, in the order it calls them ("How a context is made").  A stage returns FBA_OK or the
// code of a refusal whose message fail() has stored: in g_create_error while no context exists, in the context from then on.

// ---- stage 1: the environment switches, read once per fba_create (not cached: tests change them between contexts of one process)
struct CreateSwitches {
    bool double_buffer, node_visits, wide_hash, dense_particles;   // set at all
    bool no_etiger, tiger_gather, no_compact;                      // set to a number other than 0
    int hist_multi;                                                // 0 unset, 1 set to 0, 2 set to another number
    bool hist_lockstep;                                            // on unless set to 0
    bool tree_records, rows_hbm, stride_full;                      // FBA_HIST_TREE=records, FBA_HIST_ROWS=hbm, FBA_HIST_STRIDE=full
    bool is_multi_min_set;                                         // FBA_IS_MULTI_MIN is set (tests: exercise the large-filter path), and
    int is_multi_min;                                              // ... the particle count from which the importance filter takes several launches
    int scratch_slots, node_bound;                                 // 0 unset, else at least 1 / 2
    int node_words;                                                // 0 unset
    int search_quorum;                                             // 0 unset or out of 1..64
};
CreateSwitches read_create_switches()
{
    const auto number = [](const char* v, int unset) { return v ? std::atoi(v) : unset; };
    const auto says   = [](const char* v, const char* word) { return v && !std::strcmp(v, word); };
    const auto at_least = [](const char* v, int least) { return v ? std::max(least, std::atoi(v)) : 0; };
    CreateSwitches s{};
    s.double_buffer   = std::getenv("FBA_DOUBLE_BUFFER") != nullptr;
    s.node_visits     = std::getenv("FBA_NODE_VISITS") != nullptr;
    s.wide_hash       = std::getenv("FBA_WIDE_HASH") != nullptr;
    s.dense_particles = std::getenv("FBA_DENSE_PARTICLES") != nullptr;
    s.no_etiger       = number(std::getenv("FBA_NO_ETIGER"), 0) != 0;
    s.tiger_gather    = number(std::getenv("FBA_TIGER_GATHER"), 0) != 0;
    s.no_compact      = number(std::getenv("FBA_NO_COMPACT"), 0) != 0;
    const char* multi = std::getenv("FBA_HIST_MULTI");
    s.hist_multi      = multi ? (std::atoi(multi) != 0 ? 2 : 1) : 0;
    s.hist_lockstep   = number(std::getenv("FBA_HIST_LOCKSTEP"), 1) != 0;
    s.tree_records    = says(std::getenv("FBA_HIST_TREE"), "records");
    s.rows_hbm        = says(std::getenv("FBA_HIST_ROWS"), "hbm");
    s.stride_full     = says(std::getenv("FBA_HIST_STRIDE"), "full");
    // one workgroup per slot up to IS_MAX_CHUNKS * 256 particles, several launches beyond; the switch lowers the switch-over
    const char* multi_min = std::getenv("FBA_IS_MULTI_MIN");
    s.is_multi_min_set = multi_min != nullptr;
    s.is_multi_min     = multi_min ? std::max(1, std::atoi(multi_min)) : IS_MAX_CHUNKS * 256 + 1;
    s.scratch_slots   = at_least(std::getenv("FBA_SCRATCH_SLOTS"), 1);   // (tests: several chunks with a few slots)
    s.node_bound      = at_least(std::getenv("FBA_NODE_BOUND"), 2);      // (tests: exercise the overflow guard)
    s.node_words      = number(std::getenv("FBA_NODE_WORDS"), 0);        // (layout experiments: padded records)
    s.search_quorum   = search_quorum_switch(std::getenv("FBA_SEARCH_QUORUM"));   // (A/B runs, tests: search_kernel's boundary quorum, fba_launch_plan.h)
    return s;
}

// ---- stage 2: what needs no context -- the argument checks, the composite beliefs mapped onto the two filters, the domain
// the reference's constructor / validate() errors (POUCT.cpp:34-50, RejectionSampling.cpp:7-13, FactoredTiger.cpp:13-17, TigerPriors.cpp:22-25)
int check_arguments(const fba_config& cfg)
{
    if (cfg.sims < 1 && cfg.planner == FBA_PLANNER_POUCT) return fail(nullptr, FBA_EINVAL, "cannot initiate POUCT with %d simulations, must be greater than 0", cfg.sims);
    if (cfg.horizon <= 0) return fail(nullptr, FBA_EINVAL, "cannot initiate POUCT with %d horizon, must be greater than 0", cfg.horizon);
    if (cfg.horizon > 255) return fail(nullptr, FBA_EINVAL, "horizon %d exceeds the 255 steps a stream address holds", cfg.horizon);
    if (cfg.particles < 1) return fail(nullptr, FBA_EINVAL, "cannot initiate belief with n = %d", cfg.particles);
    if (cfg.discount <= 0 || cfg.discount > 1) return fail(nullptr, FBA_EINVAL, "discount must be in (0, 1]");
    if (cfg.runs < 1 || cfg.episodes < 1) return fail(nullptr, FBA_EINVAL, "runs and episodes must be >= 1");
    if (cfg.episodes > 65535) return fail(nullptr, FBA_EINVAL, "episodes %d exceeds the 65535 a stream address holds", cfg.episodes);
    if (cfg.model == FBA_MODEL_POMDP && cfg.episodes != 1) return fail(nullptr, FBA_EINVAL, "planning runs have exactly one episode per run");
    int ndev = 0;   // (behind the checks above: they answer on a machine without a device too)
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, FBA_ENODEVICE, "no HIP device visible: libfba_hip has no CPU path");
    if (cfg.device < 0 || cfg.device >= ndev) return fail(nullptr, FBA_EINVAL, "device %d out of range (%d visible)", cfg.device, ndev);
    return FBA_OK;
}

// the reference has fully connected priors for factored tiger, collision avoidance and sysadmin
// (GridWorldFactBAPrior::sampleFullyConnectedState throws "nyi"): all three are built
bool has_fully_connected_prior(const fba_config& cfg)
{
    return cfg.model == FBA_MODEL_BA_FACTORED && (dom_is_ftiger(cfg.domain) || is_ca(cfg.domain) || is_sys(cfg.domain)) &&
           !(is_ca(cfg.domain) && cfg.structure_prior == FBA_SP_FULLY_CONNECTED);
}

// a weighted (importance) filter + a rejection filter of correct-graph particles it copies from when
// its log likelihood drops below --threshold (prototypes/CheatingReinvigoration.cpp)
int map_cheating(const fba_config& cfg, Problem& P)
{
    if (cfg.model != FBA_MODEL_BA_FACTORED) return fail(nullptr, FBA_EINVAL, "cheating-reinvigoration belief: needs a factored model (fbapomdp)");
    if (cfg.particles < 1 || cfg.resample_amount < 1)  // CheatingReinvigoration.cpp:30-34; :36-40 below
        return fail(nullptr, FBA_EINVAL, "CheatingReinvigoration::cannot initiate belief of size < 1 (%d), or resample size of < 1 (%d)", cfg.particles, cfg.resample_amount);
    if (cfg.threshold >= 0) return fail(nullptr, FBA_EINVAL, "CheatingReinvigoration::cannot initiate with resample_threshold >= 0 (is:%f)", cfg.threshold);
    P.belief = FBA_BELIEF_IMPORTANCE;
    P.cheat  = cfg.resample_amount;
    return FBA_OK;
}

// an importance filter + the run's (a, o) history + a Metropolis-Hastings re-draw of the filter when the log
// likelihood drops below --threshold (MHwithinGibbs.cpp, MHNIPS2018.cpp); built for the priors that have
// computePriorModel and mutate and a fully enumerable state space: factored tiger, collision avoidance
int map_mh(const fba_config& cfg, Problem& P)
{
    const bool nips  = cfg.belief == FBA_BELIEF_MH_NIPS;
    const char* name = nips ? "MHNIPS2018" : "MHwithinGibbs";
    if (cfg.model != FBA_MODEL_BA_FACTORED || cfg.dirichlet_regular ||
        !(dom_is_ftiger(cfg.domain) || is_ca(cfg.domain) || cfg.domain == FBA_DOM_GRIDWORLD || is_sys(cfg.domain)) ||
        (is_ca(cfg.domain) && cfg.structure_prior == FBA_SP_FULLY_CONNECTED))
        return fail(nullptr, FBA_EINVAL, "%s belief: needs a factored model (fbapomdp) in the expected Dirichlet mode, at most %d structure words per particle",
                    nips ? "mh-nips" : "mh-within-gibbs", MH_MAXVAR);
    if (nips && is_sys(cfg.domain))
        return fail(nullptr, FBA_EINVAL, "mh-nips belief on sysadmin: MHNIPS2018::MH scores a particle's counts (grown from the domain's prior, 10000 per row) "
                    "against computePriorModel(structure) (rows {total * p, total - p}, SysAdminFactoredPrior.cpp:98-127): a different prior, "
                    "whose score difference admits no proposal -- the reference does not return from it");
    if (cfg.particles < 1) return fail(nullptr, FBA_EINVAL, "%s::cannot initiate MH with size 0", name);  // MHwithinGibbs.cpp:243-246, MHNIPS2018.cpp:116-119
    if (cfg.threshold >= 0) return fail(nullptr, FBA_EINVAL, "%s::cannot initiate with threshold >= 0 (is:%f)", name, cfg.threshold);  // :248-252, MHNIPS2018.cpp:121-126
    P.belief = FBA_BELIEF_IMPORTANCE;
    P.mh     = nips ? 3 : cfg.belief_option == 1 ? 2 : 1;
    return FBA_OK;
}

// StructureIncubatorSampling(size, reinvigor_amount, threshold) (BABelief.cpp:53-58): the reinvigoration belief's two
// rejection filters + a weighted shadow filter of bred particles; same domains (a fully connected prior is needed)
int map_incubator(const fba_config& cfg, Problem& P)
{
    if (!has_fully_connected_prior(cfg))
        return fail(nullptr, FBA_EINVAL, "incubator belief: needs a factored model (fbapomdp) of factored tiger, collision avoidance or sysadmin");
    if (cfg.particles < 1 || cfg.resample_amount < 1)  // StructureIncubatorSampling.cpp:28-33; :35-39 below
        return fail(nullptr, FBA_EINVAL, "StructureIncubatorSampling::Cannot initiate Incubator belief update with size < 1 (%d) or resample size < 1 (%d)",
                    cfg.particles, cfg.resample_amount);
    if (cfg.threshold <= 0 || cfg.threshold > 1) return fail(nullptr, FBA_EINVAL, "StructureIncubatorSampling::must initiate with 1 < threshold <= 0 (is:%f)", cfg.threshold);
    if (cfg.resample_amount >= cfg.particles || cfg.resample_amount > 1024)  // WeightedFilter::leastLikely asserts n < size() (WeightedFilter.cpp:207)
        return fail(nullptr, FBA_EINVAL, "incubator belief: the resample amount (%d) must be below the number of particles (%d): WeightedFilter::leastLikely",
                    cfg.resample_amount, cfg.particles);
    if (cfg.particles > IS_LDS_MAX_N) return fail(nullptr, FBA_EINVAL, "incubator belief: at most %d particles per slot", IS_LDS_MAX_N);
    P.belief = FBA_BELIEF_REJECTION;
    P.incub  = cfg.resample_amount;
    return FBA_OK;
}

// NestedBelief(particle_amount, particle_amount^2) (BABelief.cpp:67-70): a weighted filter of count particles, each
// with its own flat filter of domain states; the BABelief factory only, i.e. bapomdp / fbapomdp
int map_nested(const fba_config& cfg, Problem& P)
{
    if (cfg.model == FBA_MODEL_POMDP) return fail(nullptr, FBA_EINVAL, "nested belief: needs a Bayes-adaptive model (bapomdp / fbapomdp)");
    if (cfg.particles < 1)  // NestedBelief.cpp:22-27
        return fail(nullptr, FBA_EINVAL, "NestedBelief: cannot initiate with filter size < 1 (top: %d, bottom: %d)", cfg.particles, cfg.particles * cfg.particles);
    if (cfg.particles > 256) return fail(nullptr, FBA_EINVAL, "nested belief: at most 256 count particles (each carries particles^2 domain states)");
    P.belief = FBA_BELIEF_IMPORTANCE;
    P.nested = cfg.particles * cfg.particles;
    return FBA_OK;
}

// two rejection filters + breeding (ReinvigoratingRejectionSampling.hpp)
int map_reinvigoration(const fba_config& cfg, Problem& P)
{
    if (!has_fully_connected_prior(cfg))
        return fail(nullptr, FBA_EINVAL, "reinvigoration belief: needs a factored model (fbapomdp) of factored tiger, collision avoidance or sysadmin");
    if (cfg.particles < 1 || cfg.resample_amount < 1)  // ReinvigoratingRejectionSampling.cpp:43-49
        return fail(nullptr, FBA_EINVAL, "ReinvigoratingRejectionSampling::cannot initiate belief of size < 1 (%d), or resample size of < 1 (%d)",
                    cfg.particles, cfg.resample_amount);
    P.belief  = FBA_BELIEF_REJECTION;
    P.reinvig = cfg.resample_amount;
    return FBA_OK;
}

// cfg.belief onto the filter that carries it (P.belief) and what it keeps beside that filter.  A point estimate is the rejection update of
// a single state (PointEstimation.cpp:36-76 / BAPointEstimation.cpp): the configuration itself changes.
int map_belief(fba_config& cfg, Problem& P)
{
    if (cfg.belief == FBA_BELIEF_POINT) { cfg.belief = FBA_BELIEF_REJECTION; cfg.particles = 1; P.point = 1; }
    P.belief = cfg.belief;
    switch (cfg.belief) {
        case FBA_BELIEF_CHEATING: return map_cheating(cfg, P);
        case FBA_BELIEF_MH_GIBBS:
        case FBA_BELIEF_MH_NIPS: return map_mh(cfg, P);
        case FBA_BELIEF_INCUBATOR: return map_incubator(cfg, P);
        case FBA_BELIEF_NESTED: return map_nested(cfg, P);
        case FBA_BELIEF_REINVIGORATION: return map_reinvigoration(cfg, P);
        default: return FBA_OK;
    }
}

// the domain's tables as the context keeps them on the host
struct DomainTables { SysDesc sys{}; CADesc ca{}; GridDesc grid{}; };

// the domain's sizes and tables, or the error of its constructor in the reference
int map_domain(const fba_config& cfg, Problem& P, DomainTables& t)
{
    switch (cfg.domain) {
        case FBA_DOM_TIGER_EPISODIC:
        case FBA_DOM_TIGER_CONTINUOUS: P.S = 2; P.A = 3; P.O = 2; break;
        case FBA_DOM_FTIGER_EPISODIC:
        case FBA_DOM_FTIGER_CONTINUOUS:
            if (cfg.size < 1 || cfg.size > 12) return fail(nullptr, FBA_EINVAL, "cannot initiate FactoredTiger with %d irrelevant features", cfg.size);
            P.S = 2 << cfg.size; P.A = 3; P.O = 2;
            break;
        case FBA_DOM_AGR:  // AGR(10): 21 x 21 (goal, position) states, 21 help actions + work + observe, 21 positions + "none"
            if (cfg.model != FBA_MODEL_POMDP || cfg.belief != FBA_BELIEF_REJECTION)  // AGR.cpp:307-310 (thrown by the first weighted update)
                return fail(nullptr, FBA_EINVAL, "AGR::computeObservationProbability nyi");
            P.S = 21 * 21; P.A = 23; P.O = 22;
            break;
        case FBA_DOM_COFFEE:
        case FBA_DOM_COFFEE_BOUTILIER:  // CoffeeProblem.hpp: 5 binary features, {GetCoffee, CheckCoffee}, {Want, NotWant}
            if (cfg.model != FBA_MODEL_POMDP)  // factory::makeBADomainExtension has no coffee entry
                return fail(nullptr, FBA_EINVAL, "the coffee problem has no Bayes-adaptive extension: planning only");
            P.S = 32; P.A = 2; P.O = 2;
            break;
        case FBA_DOM_SYSADMIN_INDEPENDENT:
        case FBA_DOM_SYSADMIN_LINEAR:
            if (cfg.size < 1 || cfg.size > 8)  // SysAdmin.cpp:17-21; 2N actions <= FBA_MAX_ACTIONS
                return fail(nullptr, FBA_EINVAL, cfg.size < 1 ? "Cannot initiate Sysadmin with n %d" : "sysadmin: at most 8 computers (n = %d)", cfg.size);
            build_sysadmin(t.sys, cfg.size);
            P.S = 1 << cfg.size; P.A = 2 * cfg.size; P.O = 2;
            break;
        case FBA_DOM_COLLISION_AVOID:
        case FBA_DOM_COLLISION_AVOID_CENTERED: {
            const int W = cfg.width, H = cfg.height, n = cfg.size;
            if (W < 1) return fail(nullptr, FBA_EINVAL, "Cannot initiate CollisionAvoidance with width %d", W);
            if (H < 1 || H % 2 != 1 || H > 15) return fail(nullptr, FBA_EINVAL, "Cannot initiate CollisionAvoidance with height %d, must be uneven", H);
            if (n > W || n < 1 || n > MAXF - 2)
                return fail(nullptr, FBA_EINVAL, "cannot initiate collision avoidance with more obstacles (%d ) than columns (%d)!", n, W);
            build_collision_avoidance(t.ca, W, H, n, cfg.domain == FBA_DOM_COLLISION_AVOID);
            P.S = W * H * t.ca.Hn; P.A = 3; P.O = t.ca.Hn;
            break;
        }
        case FBA_DOM_GRIDWORLD:
            if (cfg.size < 3 || cfg.size > 15)
                return fail(nullptr, FBA_EINVAL, "please enter a size larger than 3 to be able to run gridworld (you entered %d)", cfg.size);
            build_gridworld(t.grid, cfg.size);
            P.S = P.O = cfg.size * cfg.size * t.grid.G; P.A = 4;
            break;
        default: return fail(nullptr, FBA_EINVAL, "domain %d is not supported by this build", cfg.domain);
    }
    return FBA_OK;
}

// what the configuration says of the problem in so many words
void set_problem_parameters(const fba_config& cfg, Problem& P)
{
    P.domain = cfg.domain; P.model = cfg.model; P.planner = cfg.planner;
    P.N = cfg.particles; P.sims = cfg.sims; P.horizon = cfg.horizon; P.episodes = cfg.episodes;
    P.max_depth = cfg.max_depth < 0 ? cfg.horizon : cfg.max_depth;  // ArgumentParser.cpp:37-40
    P.exploration = cfg.exploration; P.gamma = cfg.discount;
    P.seed_lo = (uint32_t)cfg.seed; P.seed_hi = (uint32_t)(cfg.seed >> 32);
    P.noise = cfg.noise; P.counts_total = cfg.counts_total; P.structure_prior = cfg.structure_prior;
    P.dirichlet_regular = cfg.dirichlet_regular ? 1 : 0;
}

// ---- the context exists from here on
// the length of a particle's count table and, for a factored model, its built-in prior and description; then the two limits of every model
int build_model(fba_ctx* c)
{
    const fba_config& cfg = c->cfg;
    Problem& P = c->P;
    if (cfg.model == FBA_MODEL_BA_TABLE) {
        P.phi_len = P.S * P.A * P.S;
        P.C       = P.phi_len + P.A * P.S * P.O;
    } else if (cfg.model == FBA_MODEL_BA_FACTORED) {
        TRY(build_factored_prior(c));
        P.C = c->fdesc.ncounts + c->fdesc.nvar;
    } else if (cfg.model != FBA_MODEL_POMDP) return fail(c, FBA_EINVAL, "model %d is not supported by this build", cfg.model);
    c->dense_C = P.C;
    if (P.A > FBA_MAX_ACTIONS) return fail(c, FBA_EINVAL, "more than %d actions", FBA_MAX_ACTIONS);
    if (cfg.belief == FBA_BELIEF_IMPORTANCE && P.N > (1 << 26)) return fail(c, FBA_EINVAL, "importance sampling supports at most %d particles per slot", 1 << 26);
    return FBA_OK;
}

// ---- stage 3: the particle record format (fba_state.h): dense fp32 counts unless one of the four below applies
long long run_steps(const fba_config& cfg) { return (long long)cfg.episodes * cfg.horizon; }   // the most belief updates of one run

// the most 64-byte buckets whose keys fit 28 bits: (buckets * 4 + 3) * O + O - 1 < 2^28 (the root's "bucket" is index `buckets`)
long long tree_bucket_fit(const Problem& P) { return (1ll << 28) / (4ll * P.O) - 2; }

// the search of a history-particle context is the bucket-tree one (search_hist2_kernel, search_tabhist_kernel) and its keys fit: po-uct or
// random, at most 65536 simulations, no records tree, a table of the default size or an explicit one within the fit
bool bucket_tree_search(const fba_config& cfg, const CreateSwitches& sw, const Problem& P)
{
    return (cfg.planner == FBA_PLANNER_POUCT || cfg.planner == FBA_PLANNER_RANDOM) && cfg.sims <= 65536 && !sw.tree_records &&
           (cfg.tree_buckets <= 0 || (long long)cfg.tree_buckets <= tree_bucket_fit(P));
}

// Packed particles (PackedView, fba_device.h): the tabular tiger particle as 24 uint16 increment counts over
// the shared prior -- 64 bytes instead of 128 in every belief update and every root sample.  Only where every
// kernel that touches the records is a tiger-table instantiation (check_packed_kernels below holds the launch
// decisions to that), the prior is exact under "+ 65535" (TigerBAPrior: 5000, 0 and the two listen counts below)
// and one run cannot add more than 65535 to a cell (one T and one O increment per real step).
void try_packed_tiger(fba_ctx* c, const CreateSwitches& sw)
{
    const fba_config& cfg = c->cfg;
    if (!(tiger_table_model(c->P) && cfg.planner == FBA_PLANNER_POUCT &&
          (cfg.belief == FBA_BELIEF_REJECTION || cfg.belief == FBA_BELIEF_IMPORTANCE) && cfg.particles <= IS_MAX_CHUNKS * 256 &&
          !sw.is_multi_min_set && !sw.dense_particles && run_steps(cfg) <= 65535 && cfg.noise > -.15 && cfg.noise <= .3))
        return;
    if (!packable_prior({(.85f - cfg.noise) * cfg.counts_total, (.15f + cfg.noise) * cfg.counts_total, 5000.f, 0.f})) return;
    c->P.packed = 1;
    c->P.C      = (c->dense_C + 1) / 2;  // words holding the uint16 pairs; the state word follows
}

// Packed factored-tiger particles (PackedFtigerView, fba_device.h): uint16 increments over a prior that is a function of
// the cell and the particle's structure bits -- 144 B instead of 288 B at --size 3, so twice the beliefs per gigabyte and
// per kilobyte of LDS.  Only where every kernel that touches the records is a factored-tiger instantiation (po-uct,
// plain rejection filter, expected Dirichlet, --size 1..3: check_packed_kernels below) and the prior's five values
// are exact under "+ 65535".
void try_packed_ftiger(fba_ctx* c, const CreateSwitches& sw)
{
    const fba_config& cfg = c->cfg;
    Problem& P = c->P;
    if (!(ftiger_features(P) && cfg.belief == FBA_BELIEF_REJECTION && !P.point &&
          cfg.planner == FBA_PLANNER_POUCT && cfg.size >= 1 && cfg.size <= 3 && !sw.dense_particles &&
          run_steps(cfg) <= 65535))
        return;
    const float acc = (.85f - cfg.noise) * cfg.counts_total, inacc = (.15f + cfg.noise) * cfg.counts_total, unif = .5f * cfg.counts_total;
    if (!packable_prior({acc, inacc, unif, 5000.f, 0.f})) return;
    P.ft_packed = 1;
    P.ft_acc = acc; P.ft_inacc = inacc; P.ft_unif = unif;
    P.C = c->fdesc.ncounts / 2 + 1;   // words of uint16 pairs, the structure word; the state word follows
}

// History particles (fba_device.h): the gridworld FBA-POMDP particle as one 4-byte entry per real step over the
// shared prior tables -- 100-500 bytes instead of 191 KB (N = 7) -- where the importance filter is the plain one,
// the run fits the record (one entry per belief update), the grid fits 3-bit coordinates and prior + j is exact in
// fp32 for every count a run can reach (so a row read through the entries is bit for bit the dense row).
// The plain rejection filter (reject_hist_kernel) stores them too where its search is the bucket-tree one (hist2_flat_search,
// bucket_tree_search above -- the flat root sample exists there only); ts and the rest stay dense.
// The tabular gridworld BA-POMDP stores them too (P.hist = 2: entries of state indices over the prior's sparse rows, 176 B instead of
// 7.68 MB at N = 7) under the same filters, where its search is the bucket-tree one (search_tabhist_kernel); ts and the rest stay dense.
void try_gridworld_history(fba_ctx* c, const CreateSwitches& sw)
{
    const fba_config& cfg = c->cfg;
    Problem& P = c->P;
    const bool bucket_tree = bucket_tree_search(cfg, sw, P);
    const bool flat     = cfg.belief == FBA_BELIEF_REJECTION && !P.point && bucket_tree;
    const bool weighted = cfg.belief == FBA_BELIEF_IMPORTANCE && cfg.particles <= IS_MAX_CHUNKS * 256 && !sw.is_multi_min_set;
    const bool tabular  = cfg.model == FBA_MODEL_BA_TABLE && bucket_tree;
    if (!((cfg.model == FBA_MODEL_BA_FACTORED || tabular) && cfg.domain == FBA_DOM_GRIDWORLD && (weighted || flat) && !cfg.dirichlet_regular &&
          !sw.dense_particles && run_steps(cfg) <= HIST_MAX_CAP && cfg.size <= HIST_MAX_N))
        return;
    const int cap = cfg.episodes * cfg.horizon;
    if (tabular) {
        if (build_tabular_prior(c) != FBA_OK || !increments_exact(c->prior, cap + 1)) return;   // (built again by make_context, as for every tabular context)
    } else {
        build_gridworld_alt_prior(c);
        const std::vector<float> counts(c->prior.begin(), c->prior.begin() + c->fdesc.ncounts);
        if (!increments_exact(counts, cap + 1) || !increments_exact(c->prior_alt, cap + 1)) return;
    }
    P.hist     = tabular ? 2 : 1;
    P.hist_cap = cap;
    P.hist_row = std::max(c->gdesc.N, c->gdesc.G);
    P.gw_N = c->gdesc.N; P.gw_G = c->gdesc.G;
    uint32_t cells[4] = {0, 0, 0, 0};
    for (int gq = 0; gq < c->gdesc.G; ++gq)
        cells[gq >> 2] |= (uint32_t)(c->gdesc.goal[gq][0] * c->gdesc.N + c->gdesc.goal[gq][1]) << (8 * (gq & 3));
    P.gw_goalcell0 = cells[0]; P.gw_goalcell1 = cells[1]; P.gw_goalcell2 = cells[2]; P.gw_goalcell3 = cells[3];
    P.C        = 0;  // word 0 = state, word 1 = structure bits, words 2.. = entries
}

// The collision-avoidance FBA-POMDP in the prior's own graph (no structure prior: ca_fact_step's contexts) stores them too under the plain
// importance filter where that filter is the multi-launch one (P.hist = 3: entries of 12 + 9n bits, the whole prior in LDS -- 328 B instead of
// 3.5 KB at 7 x 7 with two obstacles and 80 steps), where the planner is po-uct or random, the grid fits 3-bit fields (W, H <= 8, n <= 2), the
// run fits the record and the search's LDS (tables, path, one staged record per lane) fits a workgroup.  The prior need not be exact under
// "+ j": cells that are not read their count from a table of sequential sums (ca_hist_sequences), at most CA_HIST_MAX_SEQ distinct values;
// other priors stay dense.  Their update exists as the multi-launch filter only (is_multi_ca_step_kernel and the launches behind it), so the
// format is used exactly where the dense records take that filter too (D.is_multi, plan_filters: from CreateSwitches::is_multi_min particles
// up).  Up to 65 536 particles the records stay dense on the one-launch importance_kernel, as before.
void try_collision_avoidance_history(fba_ctx* c, const CreateSwitches& sw)
{
    const fba_config& cfg = c->cfg;
    Problem& P = c->P;
    if (!(cfg.model == FBA_MODEL_BA_FACTORED && is_ca(cfg.domain) && cfg.belief == FBA_BELIEF_IMPORTANCE && !P.point && cfg.particles >= sw.is_multi_min &&
          (cfg.planner == FBA_PLANNER_POUCT || cfg.planner == FBA_PLANNER_RANDOM) && !cfg.dirichlet_regular && !sw.dense_particles &&
          c->fdesc.nvar == 0 && c->fdesc.nodes[2].nmax == 1 && !P.nested && !P.mh && !P.cheat && !P.incub && !P.reinvig &&
          run_steps(cfg) <= HIST_MAX_CAP && run_steps(cfg) >= 1 &&
          c->cadesc.W <= 8 && c->cadesc.H <= 8 && c->cadesc.n >= 1 && c->cadesc.n <= 2 && P.A == 3))
        return;
    const int cap = cfg.episodes * cfg.horizon, nc = c->fdesc.ncounts;
    std::vector<uint8_t> sid;
    std::vector<float> seq;
    Problem Q = P;
    Q.hist_row = nc; Q.hist_rid_bytes = (nc + 15) & ~15; Q.hist_distinct = CA_HIST_MAX_SEQ; Q.hist_cap = cap; Q.Cs = (2 + cap + 3) & ~3;
    if (!(nc == ca_hist_ncounts(P.A, c->cadesc.W, c->cadesc.H, c->cadesc.n) && ca_hist_sequences(c->prior, nc, cap + 1, sid, seq) &&
          ca_hist_search_lds(Q) <= 64 * 1024))
        return;
    P.hist     = 3;
    P.hist_cap = cap;
    P.hist_row = nc;   // (for these records: the cells of the prior table)
    P.gw_N = 1; P.gw_G = 1;   // (init_kernel / reset_kernel pack the state into word 1 with these; nothing reads that word here)
    P.C        = 0;    // word 0 = state, word 1 unused, words 2.. = entries
}

// the record format and, with it, the words of a record and its stride
void choose_record_format(fba_ctx* c, const CreateSwitches& sw)
{
    Problem& P = c->P;
    try_packed_tiger(c, sw);
    try_packed_ftiger(c, sw);
    try_gridworld_history(c, sw);
    try_collision_avoidance_history(c, sw);
    P.hist_compact = P.hist && !sw.stride_full ? 1 : 0;   // (A/B switch: every record at the full stride)
    // record stride (fba_state.h): counts + state word, padded to a power of two up to 64 words
    // (so small particles are whole cache lines), to a multiple of 4 words beyond that
    if (P.hist) P.Cs = (2 + P.hist_cap + 3) & ~3;
    else if (P.ft_packed) P.Cs = (P.C + 1 + 3) & ~3;   // 36 words at --size 3: the point is the bytes, not a power of two
    else {
        int need = P.C + 1, cs = 4;
        if (need <= 64) { while (cs < need) cs <<= 1; }
        else cs = (need + 3) & ~3;
        P.Cs = cs;
    }
}

// ---- stage 4: the search tree's layout and what one slot takes
struct TreePlan {
    bool hashed = false;                   // children through a hash table, not a dense child array per node
    uint32_t hcap = 0;                     // ... of this many entries of hash_entry bytes (0: none)
    size_t hash_entry = 16, bkt_lines = 0; // bkt_lines: the bucket tree's 128-byte lines (0: node records)
    size_t per_slot = 0;                   // bytes of one slot, for the slot count of slots = 0
};

int plan_tree(fba_ctx* c, const CreateSwitches& sw, TreePlan& t)
{
    const fba_config& cfg = c->cfg;
    Problem& P = c->P;
    DeviceState& D = c->D;
    // node record layout (fba_state.h)
    t.hashed = P.A * P.O > 64;
    // a hashed tree with an even number of actions drops the visits word (it is the sum of the action counts) and the
    // padding word with it: 56 -> 48 bytes per node for the four actions of gridworld
    D.cn_off     = (t.hashed && P.A % 2 == 0 && !sw.node_visits) ? 0 : 1;
    D.cq_off     = (D.cn_off + P.A + 1) & ~1;
    D.child_off  = D.cq_off + 2 * P.A;
    D.node_words = std::max(t.hashed ? D.child_off : ((D.child_off + P.A * P.O + 1) & ~1), sw.node_words);
    D.max_nodes  = P.sims + 2;  // one new node per simulation at most
    // Episodic (factored) tiger: only `listen` continues an episode and it has two observations, so a node has at most
    // two children and the tree of a search of depth D is at most the complete binary tree with levels 0..D:
    // 2^(D+1) - 1 nodes, whatever the number of simulations (2047 at the default depth 10 against 4098 / 16386
    // records for 4096 / 16384 simulations).  search_kernel refuses to go past max_nodes (fault -> FBA_ESTATE).
    if (dom_is_episodic(cfg.domain) && P.max_depth >= 0 && P.max_depth < 24)
        D.max_nodes = std::min(D.max_nodes, (1 << (P.max_depth + 1)) + 1);  // (+1: odd, so that the slots' trees are not a power of two
                                                                             // of bytes apart -- at exactly 128 KB the search ran 45 % slower)
    if (sw.node_bound) D.max_nodes = sw.node_bound;
    if (t.hashed) {
        t.hcap = 64;
        while (t.hcap < 2u * (uint32_t)(D.max_nodes - 2)) t.hcap <<= 1;  // at most max_nodes - 2 children (one per simulation): load <= 1/2
        D.hmask = t.hcap - 1;
        if ((unsigned long long)D.max_nodes * P.A * P.O < (1ull << 27) && !sw.wide_hash) {
            D.hash_compact = 1;
            t.hash_entry   = 8;
        }
    }
    // History-particle searches keep their tree in one table of 64-byte buckets (search_hist2_kernel, fba_state.h) where its keys fit:
    // (parent bucket, action, observation) in 28 bits, counts below the root in 16.  FBA_HIST_TREE=records keeps node records + hash table
    // (search_hist_kernel), for A/B runs and for what does not fit.
    const bool bucket_records = P.hist && P.hist != 3 && !sw.tree_records;   // (collision-avoidance records: search_kernel's node records)
    if (bucket_records && P.sims <= 65536) {
        const long long buckets = std::max(cfg.tree_buckets > 0 ? (long long)cfg.tree_buckets : 2ll * (P.sims + 2), 8ll);
        const long long fit     = tree_bucket_fit(P);
        if (cfg.tree_buckets <= 0 || buckets <= fit) t.bkt_lines = (size_t)((std::min(buckets, fit) + 1) / 2);
    }
    if (cfg.tree_buckets < 0 || (cfg.tree_buckets > 0 && !t.bkt_lines && bucket_records))
        return fail(c, FBA_EINVAL, "tree_buckets = %d: not a size this context's search can use (history-particle searches of at most 65536 "
                    "simulations, keys of 28 bits)", cfg.tree_buckets);
    if (t.bkt_lines) {   // no node records, no separate hash table
        D.max_nodes = P.sims + 2;
        t.hcap = 0;
    }
    P.search_budget = (P.hist && P.hist != 3 && cfg.search_budget > 0) ? cfg.search_budget : 0;   // (only search_hist_kernel parks and resumes)
    // (per particle: two weights, a prefix sum and a side row, which a plain rejection filter of history records does not have, + its records)
    const size_t per_particle_aux = (P.hist && P.belief == FBA_BELIEF_REJECTION) ? 0 : (size_t)(2 * 8 + 8 + 4 * (MAXINC + 1));
    t.per_slot = (size_t)P.N * (per_particle_aux + ((P.reinvig || P.cheat) ? 4 : (P.incub ? 6 : (P.hist ? 1 : 2))) * (size_t)P.Cs * 4) +
                 (t.bkt_lines ? t.bkt_lines * 128 : (size_t)D.max_nodes * D.node_words * 4 + (size_t)t.hcap * t.hash_entry) + 1024;
    return FBA_OK;
}

// slots = 0: as many slots as half the free device memory holds (`budget` bytes), at most 32768 and no more than there are runs
int slot_count(const fba_config& cfg, const TreePlan& t, size_t budget)
{
    if (cfg.slots > 0) return cfg.slots;
    return std::min((int)std::min<size_t>(std::max<size_t>(budget / t.per_slot, 1), 32768), cfg.runs);
}

bool weighted_filters(const Problem& P) { return P.belief == FBA_BELIEF_IMPORTANCE || P.incub; }   // (the incubator's shadow filter is importance-sampled)

// how the filters are kept and updated, and the limits of the composite beliefs that follow from it
int plan_filters(fba_ctx* c, const CreateSwitches& sw)
{
    const Problem& P = c->P;
    DeviceState& D = c->D;
    // history particles keep ONE record buffer per slot; a resample / reset builds the new filter in a scratch pool shared by a
    // chunk of slots (launch_belief_update / launch_reset: for_each_chunk) -- the second buffer was a quarter of a slot's memory
    D.single_rec      = P.hist && !sw.double_buffer ? 1 : 0;
    D.ab_rows_hbm = sw.rows_hbm ? 1 : 0; D.ab_hist_multi = sw.hist_multi; D.ab_no_etiger = sw.no_etiger ? 1 : 0; D.ab_tiger_gather = sw.tiger_gather ? 1 : 0;
    D.ab_lockstep = sw.hist_lockstep ? 1 : 0;   // (on; only the bucket tree has it: alloc_tree)
    D.search_quorum = (int8_t)sw.search_quorum;   // (0: search_plan's default for the kernel it chooses)
    D.side_w = 1 + (P.model == FBA_MODEL_BA_FACTORED ? c->fdesc.FS + c->fdesc.FO : (P.model == FBA_MODEL_BA_TABLE ? 2 : 0));
    if (P.hist) D.side_w = 2;  // {new state, the step's entry}
    D.is_multi    = weighted_filters(P) && P.N >= sw.is_multi_min;
    D.ctot_stride = (P.N + 255) / 256 + 2;
    if (P.mh) {
        if (D.is_multi) return fail(c, FBA_EINVAL, "mh-within-gibbs belief: at most %d particles per slot", IS_MAX_CHUNKS * 256);
        if (c->fdesc.nvar > MH_MAXVAR) return fail(c, FBA_EINVAL, "mh beliefs: at most %d structure words per particle", MH_MAXVAR);
        size_t words = (size_t)3 * P.Cs + (size_t)P.S * P.A * P.S + (size_t)P.A * P.S * P.O + 2;
        words += 2 * ((size_t)(P.horizon + 1) * P.S + P.S) + (size_t)P.episodes * (P.horizon + 1) + 2 * (size_t)P.horizon + 2;
        D.mh_scratch_words = (int32_t)((words + 3) & ~(size_t)3);
    }
    if (P.cheat && D.is_multi) return fail(c, FBA_EINVAL, "cheating-reinvigoration belief: at most %d particles per slot", IS_MAX_CHUNKS * 256);
    return FBA_OK;
}

// Compact filters between the updates of the experiment loop (fba_state.h; FBA_NO_COMPACT=1 keeps 64-byte records, for A/B runs and
// tests): where the launch decisions (fba_launch_plan.h) name the one update that writes them and the one search that reads them, on the
// episodic tiger's plain rejection filter without a search budget, and a run cannot carry a count into bit 15 of its half.  Asked once
// the tree is allocated
bool compact_filters_ok(const fba_ctx* c, const CreateSwitches& sw)
{
    const Problem& P = c->P;
    return c->cfg.domain == FBA_DOM_TIGER_EPISODIC && P.belief == FBA_BELIEF_REJECTION && !P.reinvig && !P.incub && !P.cheat && !P.nested &&
           !P.point && run_steps(c->cfg) <= 32767 && !sw.dense_particles && !sw.no_compact && P.search_budget <= 0 &&
           kernel_name(update_plan(P, c->D).filter) == K_REJECT_TIGER_ONCE && search_plan(P, c->D).kernel == SEARCH_READS_COMPACT;
}

// What try_packed_tiger and try_packed_ftiger promise: every tick kernel that touches packed records is one of the format's instantiations
int check_packed_kernels(fba_ctx* c)
{
    const Problem& P = c->P;
    const uint32_t search = search_plan(P, c->D).kernel, update = update_plan(P, c->D).filter;
    if (P.packed && !(reads_packed_tiger(search) && reads_packed_tiger(update)))
        return fail(c, FBA_ESTATE, "packed tiger records met a kernel that does not read them (search %#x, update %#x)", search, update);
    if (P.ft_packed && !(reads_packed_ftiger(search) && reads_packed_ftiger(update)))
        return fail(c, FBA_ESTATE, "packed factored-tiger records met a kernel that does not read them (search %#x, update %#x)", search, update);
    return FBA_OK;
}

// ---- stage 5: the device buffers, grouped as the data is, and the uploads
inline int alloc_each(fba_ctx*, size_t, size_t) { return FBA_OK; }
template <typename T, typename... R>
int alloc_each(fba_ctx* c, size_t n, size_t slot_elems, const char* name, T** p, R... rest)   // n zeroed elements for every one of the ARR()s
{
    TRY(dev_alloc(c, name, p, n, slot_elems));
    return alloc_each(c, n, slot_elems, rest...);
}

// per slot: where its run stands and what its last step was (slot bookkeeping), then its counters; the context's single words
int alloc_slot_state(fba_ctx* c)
{
    DeviceState& D = c->D;
    const size_t E = (size_t)c->P.E;
    TRY(alloc_each(c, E, 1, ARR(run), ARR(episode), ARR(t), ARR(active), ARR(need_update), ARR(need_reset), ARR(need_init), ARR(adv), ARR(env_state),
                   ARR(ret), ARR(disc), ARR(action), ARR(obs), ARR(bufsel), ARR(cur), ARR(lazy_reset), ARR(compact)));
    TRY(alloc_each(c, E, 1, ARR(sim_steps), ARR(belief_steps), ARR(env_steps), ARR(upd_particles), ARR(upd_attempts), ARR(upd_entries),
                   ARR(upd_compact_full), ARR(upd_compact)));
    TRY(slot_alloc(c, ARR(ep_sums), 3));
    TRY(alloc_each(c, 1, 0, ARR(trace_count), "n_active", &c->d_n_active, ARR(fault)));
    TRY(dev_alloc(c, ARR(gave_up), E, 1));
    D.trace_on   = c->cfg.trace ? 1 : 0;
    D.runs_total = c->cfg.runs;
    D.run_offset = c->cfg.run_offset;
    return FBA_OK;
}

int alloc_filters(fba_ctx* c, const CreateSwitches& sw)
{
    const Problem& P = c->P;
    DeviceState& D = c->D;
    const int E = P.E;
    const bool is = weighted_filters(P);
    const size_t rec = (size_t)P.N * P.Cs;
    TRY(is ? slot_alloc(c, ARR(p_weight), P.N, 2) : dev_alloc(c, ARR(p_weight), 1));
    if (D.single_rec) D.scratch_slots = sw.scratch_slots ? std::min(E, sw.scratch_slots) : std::min(E, 1024);
    // (zeroed: a slot whose belief was never initiated -- a slot of fba_run_bapomdp beyond the configured runs -- then holds all-zero records and weights, which is
    // what fba_belief_export writes for it and a block fba_belief_import takes in every record format; nothing else reads such a slot)
    // (single_rec: reported as ONE buffer, the scratch places' records behind the E slots')
    TRY(D.single_rec ? dev_alloc(c, ARR(p_rec), ((size_t)E + D.scratch_slots) * rec, rec) : slot_alloc(c, ARR(p_rec), rec, 2));
    if (D.single_rec) {   // E + scratch_slots buffers; a slot's filter and a scratch place's buffer change places after a resample / reset (swap_buffers_kernel)
        TRY(dev_alloc(c, ARR(rec_buf), (size_t)E + D.scratch_slots, 1));
        std::vector<int32_t> ids((size_t)E + D.scratch_slots);
        for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int32_t)i;
        HIPCHK(c, hipMemcpy(D.rec_buf, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        TRY(slot_alloc(c, ARR(copy_pending), 1));
    }
    TRY(is ? slot_alloc(c, ARR(wscan), P.N, 1, false) : dev_alloc(c, ARR(wscan), 1, 0, 1, false));
    TRY(slot_alloc(c, ARR(hist_cnt), 1));
    TRY(is ? slot_alloc(c, ARR(p_side), (size_t)P.N * D.side_w, 1, false) : dev_alloc(c, ARR(p_side), 1, 0, 1, false));
    TRY(is ? slot_alloc(c, ARR(ctot), D.ctot_stride) : dev_alloc(c, ARR(ctot), 1));
    TRY(slot_alloc(c, ARR(is_tot), 2));
    return FBA_OK;
}

// Which shadow particles the incubator breeds anew: the reference asks its weighted filter for the `n` least likely particles
// (WeightedFilter.cpp:193-238) at a moment when all N weights are equal, so no particle ever displaces one of the first `n`
// and the answer is those indices in the order a binary max-heap of equal keys releases them.  That order is libstdc++'s
// (std::push_heap / std::pop_heap, which its priority_queue is made of); it is computed here once, with a comparison that
// finds no key smaller than another.
std::vector<int32_t> incubator_breeding_order(int n)
{
    std::vector<int32_t> heap, order;
    const auto equal_keys = [](int32_t, int32_t) { return false; };
    for (int i = 0; i < n; ++i) { heap.push_back(i); std::push_heap(heap.begin(), heap.end(), equal_keys); }
    for (; !heap.empty(); heap.pop_back()) { std::pop_heap(heap.begin(), heap.end(), equal_keys); order.push_back(heap.back()); }
    return order;
}

// what the composite beliefs keep beside the main filter: fully connected and shadow filters, nested states, the MH chains, the likelihood
int alloc_composite(fba_ctx* c)
{
    const Problem& P = c->P;
    DeviceState& D = c->D;
    const int E = P.E;
    if (P.reinvig || P.cheat || P.incub) {
        TRY(slot_alloc(c, ARR(p_rec_fc), (size_t)P.N * P.Cs, 2, false));
        TRY(slot_alloc(c, ARR(bufsel_fc), 1));
    }
    if (P.incub) {
        TRY(slot_alloc(c, ARR(p_rec_sh), (size_t)P.N * P.Cs, 2, false));
        TRY(slot_alloc(c, ARR(p_weight_sh), P.N, 2));
        TRY(alloc_each(c, E, 1, ARR(bufsel_sh), ARR(need_update_sh)));
        const std::vector<int32_t> order = incubator_breeding_order(P.incub);
        int32_t* d_order = nullptr;
        TRY(dev_alloc(c, "inc_order", &d_order, order.size()));
        HIPCHK(c, hipMemcpy(d_order, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        D.inc_order = d_order;
    }
    if (P.nested) {
        TRY(slot_alloc(c, ARR(nest_s), (size_t)P.N * P.nested, 2));
        TRY(slot_alloc(c, ARR(nest_scan), P.N));
        TRY(alloc_each(c, E, 1, ARR(nest_sel), ARR(nest_total)));
    }
    if (P.mh || P.cheat) {   // the log likelihood per slot, and the threshold behind them
        TRY(dev_alloc(c, ARR(lik), (size_t)E + 1, 1));
        TRY(slot_alloc(c, ARR(cheat_pending), 1));
        const double thr = c->cfg.threshold;
        HIPCHK(c, hipMemcpy(D.lik + E, &thr, sizeof thr, hipMemcpyHostToDevice));
    }
    if (P.mh) {
        const size_t cap = (size_t)P.episodes * P.horizon;
        TRY(alloc_each(c, (size_t)E * cap, cap, ARR(mh_a), ARR(mh_o)));
        TRY(slot_alloc(c, ARR(mh_ep_len), P.episodes + 1));
        TRY(slot_alloc(c, ARR(mh_n_ep), 1));
        if (!mh_scratch_in_lds(D.mh_scratch_words)) TRY(slot_alloc(c, ARR(mh_scratch), D.mh_scratch_words));  // (else the chain's scratch is LDS)
    }
    return FBA_OK;
}

// the search's memory: the tree, the launch order of lock-step waves, the lists of budgeted searches (search_budget > 0)
int alloc_tree(fba_ctx* c, const TreePlan& t)
{
    DeviceState& D = c->D;
    const size_t E = (size_t)c->P.E;
    if (t.bkt_lines) {
        D.bkt_lines = (int32_t)t.bkt_lines;
        TRY(slot_alloc(c, ARR(bkt), t.bkt_lines * 8));   // (zeroed: key 0 carries epoch 0, which no search uses)
        TRY(slot_alloc(c, ARR(epoch), 1));
        TRY(dev_alloc(c, ARR(nodes), 16));
    } else {
        TRY(slot_alloc(c, ARR(nodes), (size_t)D.max_nodes * D.node_words, 1, false));
        if (t.hashed) {
            TRY(slot_alloc(c, ARR(hash), t.hcap * t.hash_entry / 16));
            TRY(slot_alloc(c, ARR(epoch), 1));
        }
    }
    if (D.bkt && D.ab_lockstep) TRY(slot_alloc(c, ARR(search_order), 1));
    if (!D.search_order) D.ab_lockstep = 0;   // (lock-step waves exist on the bucket tree only: search_hist2_kernel)
    if (c->P.search_budget <= 0) return FBA_OK;
    // budgeted searches: where a parked search stands
    TRY(alloc_each(c, E, 1, ARR(s_sim), ARR(s_nodes), ARR(s_depth), ARR(search_done)));
    if (D.bkt) TRY(slot_alloc(c, ARR(s_root), 6));
    if (D.single_rec) {   // the chunked belief launches run over compacted lists of the slots that have work (fba_state.h)
        TRY(alloc_each(c, E, 1, ARR(slot_list), ARR(scratch_idx)));
        TRY(dev_alloc(c, ARR(list_count), 1));
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&D.list_count_host), sizeof(int32_t), hipHostMallocDefault));
    }
    return FBA_OK;
}

// log1p(m) table: UCB(m, n) = u * sqrt(log1p(m) / n)  (POUCT.cpp:330-338, factorised so the
// n x n table -- 134 MB at 4096 simulations, int overflow at 65536 -- never exists)
std::vector<double> log1p_table(int sims)
{
    std::vector<double> t((size_t)sims + 2);
    for (size_t m = 0; m < t.size(); ++m) t[m] = std::log1p((double)m);
    return t;
}

// the prior buffers, the tables every search and filter reads, and the uniform weights' prefix sums (D.uni_total)
int alloc_tables(fba_ctx* c)
{
    Problem& P = c->P;
    DeviceState& D = c->D;
    TRY(dev_alloc(c, &c->d_prior, P.Cs));
    TRY(dev_alloc(c, &c->d_prior_dense, std::max(c->dense_C, 1) + 4));   // (+4: staged in 16-byte pieces)
    if (P.hist == 1) {
        const HistLayout L(c->gdesc.N, c->gdesc.G, P.A);
        TRY(dev_alloc(c, &c->d_hist_base, (size_t)L.total + 16));   // (+16: a row fetch may run up to a row width past the last row)
        TRY(dev_alloc(c, &c->d_hist_alt, (size_t)L.alt_total + 16));
        TRY(dev_alloc(c, &c->d_hist_lds, (size_t)HistRowIds(c->gdesc.N, c->gdesc.G, P.A).total + 16 + 256 * 16 * sizeof(float)));
        P.hist_base = c->d_hist_base; P.hist_alt = c->d_hist_alt;
    }
    if (P.hist == 3) TRY(dev_alloc(c, &c->d_hist_lds, (size_t)((P.hist_row + 15) & ~15) + (size_t)CA_HIST_MAX_SEQ * (P.hist_cap + 2) * sizeof(float) + 16));
    TRY(dev_alloc(c, &c->d_uni_scan, (size_t)P.N + 1));
    TRY(dev_alloc(c, &c->d_log1p, (size_t)P.sims + 2));
    D.prior = c->d_prior; D.prior_dense = c->d_prior_dense;
    D.uni_scan = c->d_uni_scan; D.log1p_tab = c->d_log1p;
    const std::vector<double> t = log1p_table(P.sims);
    HIPCHK(c, hipMemcpyAsync(c->d_log1p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (weighted_filters(P)) {
        double* tmp = nullptr;
        TRY(dev_alloc(c, &tmp, (size_t)P.N + 1));
        launch_uniform_scan(P.N, tmp, c->d_uni_scan, c->d_uni_scan + P.N, D.ctot, c->stream);
        HIPCHK(c, hipMemcpyAsync(&D.uni_total, c->d_uni_scan + P.N, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return FBA_OK;
}

// reinvigorateBelief (StructureIncubatorSampling.cpp:155-188) tests normalised shadow weights that are uniform
// whenever it runs (every update ends in a resample): none is promoted, or all of them -- and then every
// shadow weight is zero and normalize() divides by their sum.  (D.uni_total is the device's sum: alloc_tables)
int check_incubator_threshold(fba_ctx* c)
{
    const Problem& P = c->P;
    if (P.incub && (1.0 / (double)P.N) / c->D.uni_total > c->cfg.threshold)
        return fail(c, FBA_EINVAL, "incubator belief: with threshold %g every one of the %d shadow particles (normalised weight %g) is promoted at "
                    "once; the shadow filter's total weight is then zero and StructureIncubatorSampling.cpp:160-188 divides by it",
                    c->cfg.threshold, P.N, (1.0 / (double)P.N) / c->D.uni_total);
    return FBA_OK;
}

// the regular Dirichlet mode: its two refusals, and the ziggurat tables of its normal draws
int upload_regular_dirichlet(fba_ctx* c)
{
    Problem& P = c->P;
    if (!P.dirichlet_regular) return FBA_OK;
    if (P.model == FBA_MODEL_POMDP) return fail(c, FBA_EINVAL, "the Dirichlet sampling method only exists for Bayes-adaptive models");
    int longest = std::max(P.S, P.O);
    if (P.model == FBA_MODEL_BA_FACTORED) {
        longest = 0;
        for (int f = 0; f < c->fdesc.FS; ++f) longest = std::max(longest, c->fdesc.Ssz[f]);
        for (int f = 0; f < c->fdesc.FO; ++f) longest = std::max(longest, c->fdesc.Osz[f]);
    }
    if (longest > MAXROW) return fail(c, FBA_EINVAL, "regular Dirichlet mode samples rows of at most %d counts (this model has %d)", MAXROW, longest);
    ZigDesc z; build_ziggurat(z);
    TRY(dev_alloc(c, &c->d_zig, 1));
    HIPCHK(c, hipMemcpyAsync(c->d_zig, &z, sizeof z, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    P.zig = c->d_zig;
    return FBA_OK;
}

template <typename T>
int upload_desc(fba_ctx* c, T** dev, const T& host)   // (the host copy lives in the context: the copy may complete later)
{
    TRY(dev_alloc(c, dev, 1));
    HIPCHK(c, hipMemcpyAsync(*dev, &host, sizeof(T), hipMemcpyHostToDevice, c->stream));
    return FBA_OK;
}

// the descriptions of the domain and the factored model, the prior, and the default positions of the per-step interface
int upload_model(fba_ctx* c)
{
    const fba_config& cfg = c->cfg;
    Problem& P = c->P;
    if (is_ca(cfg.domain)) { TRY(upload_desc(c, &c->d_cadesc, c->cadesc)); P.ca = c->d_cadesc; }
    if (is_sys(cfg.domain)) { TRY(upload_desc(c, &c->d_sysdesc, c->sysdesc)); P.sys = c->d_sysdesc; }
    if (cfg.domain == FBA_DOM_GRIDWORLD) { TRY(upload_desc(c, &c->d_gdesc, c->gdesc)); P.gw = c->d_gdesc; }
    if (cfg.model == FBA_MODEL_BA_FACTORED) {
        FDesc& fdh = c->fdesc;
        const int nnodes = P.A * (fdh.FS + fdh.FO);
        for (int k = 0; k < nnodes; ++k)
            for (int j = 0; j < fdh.nodes[k].nmax; ++j) fdh.nodes[k].psz[j] = (uint8_t)fdh.Ssz[fdh.nodes[k].maxp[j]];
        P.fd_bytes = (int32_t)(offsetof(FDesc, nodes) + (size_t)nnodes * sizeof(FNode));
        P.ca_plain = (is_ca(cfg.domain) && fdh.nvar == 0 && fdh.nodes[2].nmax == 1) ||  // correct graph, no masks (not fully-connected)
                     (is_sys(cfg.domain) && fdh.nvar == 0);
        TRY(upload_desc(c, &c->d_fdesc, c->fdesc));
        P.fd = c->d_fdesc;
    }
    TRY(upload_prior(c));
    // default positions for the per-step interface: slot e is run run_offset + e
    std::vector<int32_t> run((size_t)P.E);
    for (int e = 0; e < P.E; ++e) run[e] = cfg.run_offset + e;
    HIPCHK(c, hipMemcpyAsync(c->D.run, run.data(), run.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->D.active, 1, (size_t)P.E, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FBA_OK;
}

// everything fba_create does once the context exists; on a refusal the context holds the message and the caller destroys it
int make_context(fba_ctx* c, const CreateSwitches& sw)
{
    TreePlan tree;
    TRY(build_model(c));
    choose_record_format(c, sw);
    TRY(plan_tree(c, sw, tree));
    TRY(plan_filters(c, sw));
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamCreate(&c->stream));
    size_t free_b = 0, total_b = 0;
    if (c->cfg.slots <= 0) HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    c->P.E = slot_count(c->cfg, tree, free_b / 2);
    TRY(alloc_slot_state(c));
    TRY(alloc_filters(c, sw));
    TRY(alloc_composite(c));
    TRY(alloc_tree(c, tree));
    TRY(alloc_tables(c));
    TRY(check_incubator_threshold(c));
    if (c->cfg.model == FBA_MODEL_BA_TABLE) TRY(build_tabular_prior(c));
    TRY(upload_regular_dirichlet(c));
    TRY(upload_model(c));
    c->compact_ok = compact_filters_ok(c, sw);
    return check_packed_kernels(c);
}

struct CtxDestroy { void operator()(fba_ctx* c) const { fba_destroy(c); } };

}  // namespace

// =============================================================================================
// C-ABI
// =============================================================================================
extern "C" {

int fba_abi_version(void) { return FBA_ABI_VERSION; }

void fba_default_config(fba_config* cfg)
{
    std::memset(cfg, 0, sizeof *cfg);
    cfg->domain       = FBA_DOM_TIGER_EPISODIC;
    cfg->model        = FBA_MODEL_POMDP;
    cfg->belief       = FBA_BELIEF_REJECTION;
    cfg->planner      = FBA_PLANNER_POUCT;
    cfg->particles    = 100;
    cfg->sims         = 1000;
    cfg->max_depth    = -1;
    cfg->horizon      = 10;
    cfg->exploration  = 100;
    cfg->discount     = .95;
    cfg->runs         = 1;
    cfg->episodes     = 1;
    cfg->noise        = 0;
    cfg->counts_total = 10000;
    cfg->slots        = 0;
}

const char* fba_last_error(const fba_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

void fba_destroy(fba_ctx* c)
{
    if (!c) return;
    const std::unique_ptr<fba_ctx> freed_on_return(c);   // (the only place a context is freed: fba_create hands every one it abandons here)
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& p : c->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto& p : c->free_events) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (void* p : c->allocs) (void)hipFree(p);
    if (c->D.list_count_host) (void)hipHostFree(c->D.list_count_host);
    if (c->stream) (void)hipStreamDestroy(c->stream);
}

int fba_create(const fba_config* cfg_in, fba_ctx** out)
{
    if (!cfg_in || !out) return fail(nullptr, FBA_EINVAL, "fba_create: null argument");
    *out = nullptr;
    (void)hipGetLastError();  // a new context starts from a clean error state
    const CreateSwitches sw = read_create_switches();
    TRY(check_arguments(*cfg_in));
    fba_config cfg = *cfg_in;
    Problem P{};
    DomainTables tables;
    TRY(map_belief(cfg, P));
    TRY(map_domain(cfg, P, tables));
    set_problem_parameters(cfg, P);
    std::unique_ptr<fba_ctx, CtxDestroy> c(new fba_ctx());   // destroyed on every way out but the last
    c->cfg = cfg; c->P = P; c->sysdesc = tables.sys; c->cadesc = tables.ca; c->gdesc = tables.grid;
    if (const int rc = make_context(c.get(), sw)) {
        g_create_error = c->err;   // (the context, which held the message, goes)
        return rc;
    }
    *out = c.release();
    return FBA_OK;
}

int fba_domain_sizes(const fba_ctx* c, int32_t* S, int32_t* A, int32_t* O)
{
    if (!c) return FBA_EINVAL;
    *S = c->P.S; *A = c->P.A; *O = c->P.O;
    return FBA_OK;
}
int fba_counts_len(const fba_ctx* c) { return c ? c->dense_C : FBA_EINVAL; }
int fba_slots(const fba_ctx* c) { return c ? c->P.E : FBA_EINVAL; }
int fba_particle_bytes(const fba_ctx* c) { return c ? c->P.Cs * 4 : FBA_EINVAL; }

int fba_device_arrays(const fba_ctx* c, fba_array_info* out, int32_t cap)
{
    if (!c || cap < 0 || (cap > 0 && !out)) return FBA_EINVAL;
    const int32_t n = (int32_t)c->arrays.size();
    for (int32_t i = 0; i < std::min(n, cap); ++i) out[i] = c->arrays[(size_t)i].info;
    return n;
}

int fba_set_model_tabular(fba_ctx* c, const float* phi, const float* psi)
{
    if (!c || !phi || !psi) return FBA_EINVAL;
    if (c->P.model != FBA_MODEL_BA_TABLE) return fail(c, FBA_EINVAL, "fba_set_model_tabular needs model = BA_TABLE");
    std::vector<float> keep = c->prior;
    c->prior.assign((size_t)c->dense_C, 0.f);
    std::copy(phi, phi + c->P.phi_len, c->prior.begin());
    std::copy(psi, psi + (c->dense_C - c->P.phi_len), c->prior.begin() + c->P.phi_len);
    const int rc = upload_prior(c);
    if (rc) c->prior = keep;
    // The prior is what Belief::initiate copies into every particle (BAPOMDPPrior::sample).  Packed particles hold
    // increments over the table, so live particles would silently move to the new table: require a new initiate.
    else if (c->P.packed || c->P.hist == 2) c->belief_ready = false;
    return rc;
}

int fba_get_factored_layout(const fba_ctx* c, fba_factored_layout* out)
{
    if (!c || !out) return FBA_EINVAL;
    if (c->P.model != FBA_MODEL_BA_FACTORED) return fail(const_cast<fba_ctx*>(c), FBA_EINVAL, "fba_get_factored_layout: not a factored model");
    static_assert(FBA_MAX_FEATURES == MAXF && FBA_MAX_NODES == MAXNODES, "public layout struct mirrors FDesc");
    const FDesc& d = c->fdesc;
    memset(out, 0, sizeof *out);
    out->n_state_features = d.FS;
    out->n_obs_features   = d.FO;
    out->n_nodes          = c->P.A * (d.FS + d.FO);
    out->n_counts         = d.ncounts;
    out->n_mask_words     = d.nvar;
    for (int f = 0; f < d.FS; ++f) out->state_feature_size[f] = d.Ssz[f];
    for (int f = 0; f < d.FO; ++f) out->obs_feature_size[f] = d.Osz[f];
    for (int k = 0; k < out->n_nodes; ++k) {
        const FNode& nd       = d.nodes[k];
        fba_factored_node& o  = out->node[k];
        o.offset = nd.off; o.out = nd.out; o.n_candidates = nd.nmax; o.mask_word = nd.var; o.fixed_mask = nd.fixed_mask;
        for (int j = 0; j < nd.nmax; ++j) { o.candidate[j] = nd.maxp[j]; o.candidate_size[j] = (uint8_t)d.Ssz[nd.maxp[j]]; }
    }
    return FBA_OK;
}

int fba_set_model_factored(fba_ctx* c, const fba_factored_layout* layout, const float* counts)
{
    if (!c || !layout || !counts) return FBA_EINVAL;
    if (c->P.model != FBA_MODEL_BA_FACTORED) return fail(c, FBA_EINVAL, "fba_set_model_factored needs model = BA_FACTORED");
    fba_factored_layout mine;
    int rc = fba_get_factored_layout(c, &mine);
    if (rc) return rc;
    bool same = layout->n_state_features == mine.n_state_features && layout->n_obs_features == mine.n_obs_features &&
                layout->n_nodes == mine.n_nodes && layout->n_counts == mine.n_counts && layout->n_mask_words == mine.n_mask_words;
    for (int k = 0; same && k < mine.n_nodes; ++k) {
        const fba_factored_node &a = layout->node[k], &b = mine.node[k];
        same = a.offset == b.offset && a.out == b.out && a.n_candidates == b.n_candidates && a.mask_word == b.mask_word &&
               std::memcmp(a.candidate, b.candidate, (size_t)b.n_candidates) == 0;
    }
    if (!same)
        return fail(c, FBA_EINVAL, "fba_set_model_factored: the layout is not this context's (obtain it with fba_get_factored_layout and fill "
                                   "the counts where it says each node's rows are)");
    for (int k = 0; k < mine.n_counts; ++k)
        if (!(counts[k] >= 0.f)) return fail(c, FBA_EINVAL, "fba_set_model_factored: count %d is %g: Dirichlet counts cannot be negative", k, (double)counts[k]);
    std::vector<float> keep = c->prior;
    c->prior.assign(counts, counts + mine.n_counts + mine.n_mask_words);
    if (c->P.ft_packed) {
        c->prior = keep;
        return fail(c, FBA_EINVAL, "this context stores factored-tiger particles packed over the built-in prior; create it with "
                                   "FBA_DENSE_PARTICLES=1 in the environment to replace the prior");
    }
    if (c->P.hist && c->P.hist != 3) {  // history particles read rows as prior + j: the new table must keep that exact (fba_create checked the built-in one;
                                        // collision-avoidance records: upload_prior rebuilds their sequence table or refuses)
        std::vector<float> only(c->prior.begin(), c->prior.begin() + mine.n_counts);
        if (!increments_exact(only, c->P.hist_cap + 1)) {
            c->prior = keep;
            return fail(c, FBA_EINVAL, "this context stores particles as histories over the prior table, which needs prior counts c with c + j exact "
                                       "in fp32 for every j up to episodes * horizon; create it with FBA_DENSE_PARTICLES=1 in the environment for this table");
        }
    }
    rc = upload_prior(c);
    if (rc) c->prior = keep;
    else c->belief_ready = false;
    return rc;
}

int fba_get_prior(const fba_ctx* c, float* counts)
{
    if (!c || !counts) return FBA_EINVAL;
    std::copy(c->prior.begin(), c->prior.end(), counts);
    return FBA_OK;
}

int fba_set_position(fba_ctx* c, const int32_t* run, const int32_t* episode, const int32_t* t)
{
    if (!c) return FBA_EINVAL;
    const size_t n = (size_t)c->P.E * 4;
    int rc;
    if ((rc = clear_parked_searches(c))) return rc;
    if (run || episode) materialize_records(c, true);  // a pending lazy reset belongs to the old (run, episode)
    if (run) HIPCHK(c, hipMemcpyAsync(c->D.run, run, n, hipMemcpyHostToDevice, c->stream));
    if (episode) HIPCHK(c, hipMemcpyAsync(c->D.episode, episode, n, hipMemcpyHostToDevice, c->stream));
    if (t) HIPCHK(c, hipMemcpyAsync(c->D.t, t, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FBA_OK;
}

int fba_belief_init(fba_ctx* c)
{
    if (!c) return FBA_EINVAL;
    int rc;
    if ((rc = clear_parked_searches(c))) return rc;
    materialize_records(c);   // (init_kernel writes 64-byte records)
    if ((rc = set_flags(c, c->D.need_init, nullptr, 1))) return rc;
    if ((rc = timed(c, FBA_K_BELIEF_INIT, [&] { launch_init(c->P, c->D, c->stream); }))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->belief_ready = true;
    c->packed_updates.assign((size_t)c->P.E, 0);
    return FBA_OK;
}

int fba_belief_reset_domain_state(fba_ctx* c)
{
    if (!c) return FBA_EINVAL;
    if (c->P.model == FBA_MODEL_POMDP) return fail(c, FBA_EINVAL, "resetDomainStateDistribution exists for Bayes-adaptive beliefs only");
    if (!c->belief_ready) return fail(c, FBA_ESTATE, "belief not initiated");
    int rc;
    materialize_records(c);
    if ((rc = set_flags(c, c->D.need_reset, nullptr, 1))) return rc;
    if ((rc = timed(c, FBA_K_BELIEF_RESET, [&] { launch_reset(c->P, c->D, c->stream); }))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FBA_OK;
}

int fba_select_action(fba_ctx* c, const int32_t* hist_len, const uint8_t* active, int32_t* action)
{
    if (!c || !action) return FBA_EINVAL;
    if (!c->belief_ready) return fail(c, FBA_ESTATE, "belief not initiated");
    int rc;
    materialize_records(c);   // the per-call interface works on 64-byte records
    if (hist_len) HIPCHK(c, hipMemcpyAsync(c->D.t, hist_len, (size_t)c->P.E * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = set_flags(c, c->D.active, active, 1))) return rc;
    {   // Planner::selectAction returns a finished search: whole searches in one launch, whatever the context's search_budget
        Problem Pw = c->P;
        DeviceState Dw = c->D;
        Pw.search_budget = 0;
        Dw.search_done   = nullptr;
        if ((rc = timed(c, FBA_K_SEARCH, [&] { launch_search(Pw, Dw, c->stream); }))) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(action, c->D.action, (size_t)c->P.E * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return check_fault(c);
}

int fba_belief_update(fba_ctx* c, const int32_t* action, const int32_t* obs, const uint8_t* active)
{
    if (!c || !action || !obs) return FBA_EINVAL;
    if (!c->belief_ready) return fail(c, FBA_ESTATE, "belief not initiated");
    for (int e = 0; e < c->P.E; ++e) {
        if (active && !active[e]) continue;
        if (action[e] < 0 || action[e] >= c->P.A) return fail(c, FBA_EINVAL, "action %d out of range", action[e]);
        if (obs[e] < 0 || obs[e] >= c->P.O) return fail(c, FBA_EINVAL, "observation %d out of range", obs[e]);
    }
    if (c->P.packed || c->P.ft_packed) {
        // a packed record counts a cell's "+1"s in 16 bits: the experiment loops cannot exceed that (episodes * horizon <= 65535 is
        // part of the packing condition), a host driving the per-step interface can -- refuse instead of wrapping into the next cell
        if (c->packed_updates.size() != (size_t)c->P.E) c->packed_updates.assign((size_t)c->P.E, 0);
        for (int e = 0; e < c->P.E; ++e) {
            if (active && !active[e]) continue;
            if (c->packed_updates[e] >= 65535u)
                return fail(c, FBA_ESTATE, "slot %d: more than 65535 belief updates since fba_belief_init, which packed particle records cannot count; "
                            "create the context with FBA_DENSE_PARTICLES=1 in the environment to drive it beyond that", e);
        }
        for (int e = 0; e < c->P.E; ++e)
            if (!active || active[e]) ++c->packed_updates[e];
    }
    int rc;
    materialize_records(c);   // the per-call interface works on 64-byte records
    HIPCHK(c, hipMemcpyAsync(c->D.action, action, (size_t)c->P.E * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->D.obs, obs, (size_t)c->P.E * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = set_flags(c, c->D.need_update, active, 1))) return rc;
    if ((rc = timed(c, k_update_kind(c), [&] { launch_belief_update(c->P, c->D, c->stream); }))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return check_fault(c);
}

// History particles: the dense count table of one record, as the API speaks of particles -- the prior (the goal-parent
// form of the x / y nodes the structure bits name) plus 1.0f per entry and incremented cell, one addition at a time
// (BABNModel::incrementCountsOf BABNModel.cpp:354-382, BAFlatModel.cpp:126-139 replayed; `cnt` = the slot's entries per action).
static void hist_add_entries(const fba_ctx* c, const uint32_t* rec, uint32_t cnt, float* counts)
{
    const int hist = c->P.hist;
    const HistDims dims = hist == 3 ? hist_dims<3>(c->P, &c->cadesc) : (hist == 2 ? hist_dims<2>(c->P, nullptr) : hist_dims<1>(c->P, nullptr));
    int j = 0;
    for (int a = 0; a < c->P.A; ++a)
        for (int q = 0; q < hist_count(cnt, a); ++q, ++j) {
            int cells[HIST_ENTRY_CELLS];
            if (hist == 3) hist_entry_cells<3>(dims, rec[1], a, rec[2 + j], cells);
            else if (hist == 2) hist_entry_cells<2>(dims, rec[1], a, rec[2 + j], cells);
            else hist_entry_cells<1>(dims, rec[1], a, rec[2 + j], cells);
            for (int k = 0; k < HIST_ENTRY_CELLS; ++k)
                if (cells[k] >= 0) counts[cells[k]] += 1.0f;
        }
}
static void hist_materialize(const fba_ctx* c, const uint32_t* rec, uint32_t cnt, float* counts)
{
    if (c->P.hist == 2) {   // tabular records
        std::copy(c->prior.begin(), c->prior.end(), counts);
        hist_add_entries(c, rec, cnt, counts);
        return;
    }
    const int ncounts = c->fdesc.ncounts;
    std::copy(c->prior.begin(), c->prior.begin() + ncounts, counts);
    if (c->P.hist == 3) {   // collision-avoidance records
        hist_add_entries(c, rec, cnt, counts);
        return;
    }
    const GridDesc& g = c->gdesc;
    const int N = g.N, G = g.G, A = c->P.A;
    const int XY = N * N * G * N, GG = N * N * G * G;
    const uint32_t mask = rec[1];
    for (int a = 0; a < A; ++a)
        for (int f = 0; f < 2; ++f) {
            const bool with_goal = (mask >> (2 * a + f)) & 1u;
            if (with_goal) std::copy(c->prior_alt.begin() + (size_t)(a * 2 + f) * XY, c->prior_alt.begin() + (size_t)(a * 2 + f + 1) * XY,
                                     counts + a * (2 * XY + GG) + f * XY);
            const uint32_t m = with_goal ? 7u : 3u;
            std::memcpy(&counts[ncounts + 2 * a + f], &m, 4);
        }
    hist_add_entries(c, rec, cnt, counts);
}

// particles [first, first + n) of slot `slot`'s filter, as the API speaks of particles (fp32 count tables whatever the record format)
static int belief_get_range(fba_ctx* c, int32_t slot, int32_t first, int32_t n, int32_t* state, double* weight, float* counts)
{
    const Problem& P = c->P;
    materialize_records(c, true);  // a lazily reset rejection filter: write the states out first
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint8_t sel = 0;
    HIPCHK(c, hipMemcpy(&sel, c->D.bufsel + slot, 1, hipMemcpyDeviceToHost));
    const size_t pb = ((size_t)sel * P.E + slot) * (size_t)P.N;
    if (weight) {
        if (P.belief != FBA_BELIEF_IMPORTANCE) return fail(c, FBA_EINVAL, "the rejection filter is unweighted");
        HIPCHK(c, hipMemcpy(weight, c->D.p_weight + pb + first, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    if (state || (counts && (P.C || P.hist))) {
        std::vector<float> tmp((size_t)n * P.Cs);
        size_t rb = pb;
        if (c->D.single_rec) {   // (history particles: one record buffer per slot, whichever of the pool it currently is)
            int32_t buf = 0;
            HIPCHK(c, hipMemcpy(&buf, c->D.rec_buf + slot, 4, hipMemcpyDeviceToHost));
            rb = (size_t)buf * (size_t)P.N;
        }
        uint32_t hist_cnt = 0;
        if (P.hist) HIPCHK(c, hipMemcpy(&hist_cnt, c->D.hist_cnt + slot, 4, hipMemcpyDeviceToHost));
        const size_t rs = P.hist ? (size_t)hist_stride(P, hist_total(hist_cnt)) : (size_t)P.Cs;   // words between this slot's records
        HIPCHK(c, hipMemcpy(tmp.data(), c->D.p_rec + rb * P.Cs + (size_t)first * rs, (size_t)n * rs * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) {
            const float* rec = tmp.data() + (size_t)i * rs;
            if (state) std::memcpy(&state[i], &rec[P.C], 4);
            if (counts && P.ft_packed) {  // count = prior(cell, structure) + increments, then the structure word (PackedFtigerView)
                const uint32_t* w = reinterpret_cast<const uint32_t*>(rec);
                const int nc = c->fdesc.ncounts;
                const uint32_t mask = w[nc / 2];
                float* out = counts + (size_t)i * c->dense_C;
                for (int k = 0; k < nc; ++k)
                    out[k] = ftiger_prior_host(c->fdesc.FS, k, mask, P.ft_acc, P.ft_inacc, P.ft_unif) + (float)((k & 1) ? (w[k >> 1] >> 16) : (w[k >> 1] & 0xffffu));
                std::memcpy(&out[nc], &mask, 4);
            } else if (counts && P.hist) hist_materialize(c, reinterpret_cast<const uint32_t*>(rec), hist_cnt, counts + (size_t)i * c->dense_C);
            else if (counts && P.packed) {  // count = prior + number of increments (PackedView)
                const uint32_t* w = reinterpret_cast<const uint32_t*>(rec);
                for (int k = 0; k < c->dense_C; ++k)
                    counts[(size_t)i * c->dense_C + k] = c->prior[k] + (float)((k & 1) ? (w[k >> 1] >> 16) : (w[k >> 1] & 0xffffu));
            } else if (counts && P.C) std::copy(rec, rec + P.C, counts + (size_t)i * P.C);
        }
    }
    return FBA_OK;
}

int fba_belief_get(fba_ctx* c, int32_t slot, int32_t* state, double* weight, float* counts)
{
    if (!c || slot < 0 || slot >= c->P.E) return FBA_EINVAL;
    return belief_get_range(c, slot, 0, c->P.N, state, weight, counts);
}

int fba_belief_get_particle(fba_ctx* c, int32_t slot, int32_t index, int32_t* state, double* weight, float* counts)
{
    if (!c || slot < 0 || slot >= c->P.E) return FBA_EINVAL;
    if (index < 0 || index >= c->P.N) return fail(c, FBA_EINVAL, "particle %d out of range (the filter holds %d)", index, c->P.N);
    if (c->P.nested) return fail(c, FBA_EINVAL, "the nested belief's particles are (model, state filter) pairs: fba_belief_get / fba_belief_get_nested");
    return belief_get_range(c, slot, index, 1, state, weight, counts);
}

int fba_belief_get_fully_connected(fba_ctx* c, int32_t slot, int32_t* state, float* counts)
{
    if (!c || slot < 0 || slot >= c->P.E) return FBA_EINVAL;
    const Problem& P = c->P;
    if (!P.reinvig && !P.cheat && !P.incub) return fail(c, FBA_EINVAL, "only the reinvigoration, incubator and cheating beliefs have a second filter");
    uint8_t sel = 0;
    HIPCHK(c, hipMemcpy(&sel, c->D.bufsel_fc + slot, 1, hipMemcpyDeviceToHost));
    const size_t pb = ((size_t)sel * P.E + slot) * (size_t)P.N;
    std::vector<float> tmp((size_t)P.N * P.Cs);
    HIPCHK(c, hipMemcpy(tmp.data(), c->D.p_rec_fc + pb * P.Cs, tmp.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < P.N; ++i) {
        const float* rec = tmp.data() + (size_t)i * P.Cs;
        if (state) std::memcpy(&state[i], &rec[P.C], 4);
        if (counts) std::copy(rec, rec + P.C, counts + (size_t)i * P.C);
    }
    return FBA_OK;
}

int fba_belief_get_shadow(fba_ctx* c, int32_t slot, int32_t* state, double* weight, float* counts)
{
    if (!c || slot < 0 || slot >= c->P.E) return FBA_EINVAL;
    const Problem& P = c->P;
    if (!P.incub) return fail(c, FBA_EINVAL, "only the incubator belief has a shadow filter");
    uint8_t sel = 0;
    HIPCHK(c, hipMemcpy(&sel, c->D.bufsel_sh + slot, 1, hipMemcpyDeviceToHost));
    const size_t pb = ((size_t)sel * P.E + slot) * (size_t)P.N;
    if (weight) HIPCHK(c, hipMemcpy(weight, c->D.p_weight_sh + pb, (size_t)P.N * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<float> tmp((size_t)P.N * P.Cs);
    HIPCHK(c, hipMemcpy(tmp.data(), c->D.p_rec_sh + pb * P.Cs, tmp.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < P.N; ++i) {
        const float* rec = tmp.data() + (size_t)i * P.Cs;
        if (state) std::memcpy(&state[i], &rec[P.C], 4);
        if (counts) std::copy(rec, rec + P.C, counts + (size_t)i * P.C);
    }
    return FBA_OK;
}

int fba_belief_get_nested(fba_ctx* c, int32_t slot, int32_t* states)
{
    if (!c || slot < 0 || slot >= c->P.E || !states) return FBA_EINVAL;
    const Problem& P = c->P;
    if (!P.nested) return fail(c, FBA_EINVAL, "only the nested belief has flat filters of domain states");
    int32_t sel = 0;
    HIPCHK(c, hipMemcpy(&sel, c->D.nest_sel + slot, sizeof sel, hipMemcpyDeviceToHost));
    const size_t per = (size_t)P.N * P.nested, off = ((size_t)sel * P.E + slot) * per;
    HIPCHK(c, hipMemcpy(states, c->D.nest_s + off, per * sizeof(int32_t), hipMemcpyDeviceToHost));
    return FBA_OK;
}

// The posterior of slots [first, first + count) reduced on the device (fba_summary.hip), a chunk of slots at a time so that the
// fp64 tables of a chunk stay below 256 MB.  Reads the context only: no flag, buffer index, counter or stream position moves,
// and a lazily reset filter stays lazy (the kernel derives the states as every other reader does).
int fba_belief_summary(fba_ctx* c, int32_t first, int32_t count, fba_belief_summary_head* head, double* state_mass, double* mean_counts,
                       double* edge_prob)
{
    if (!c) return FBA_EINVAL;
    const Problem& P = c->P;
    if (first < 0 || count < 0 || (long long)first + count > P.E)
        return fail(c, FBA_EINVAL, "fba_belief_summary: slots [%d, %lld) are not within the context's %d", first, (long long)first + count, P.E);
    if (P.nested)
        return fail(c, FBA_EINVAL, "fba_belief_summary: the nested belief's particles are (model, state filter) pairs; read them with "
                                   "fba_belief_get and fba_belief_get_nested");
    if (P.model == FBA_MODEL_POMDP && (mean_counts || edge_prob))
        return fail(c, FBA_EINVAL, "fba_belief_summary: a plain POMDP belief has no counts (fba_counts_len is 0); only head and state_mass are served");
    if (count == 0 || (!head && !state_mass && !mean_counts && !edge_prob)) return FBA_OK;
    const bool factored = P.model == FBA_MODEL_BA_FACTORED;
    const int S = P.S, dense_C = c->dense_C, ncounts = factored ? c->fdesc.ncounts : dense_C, nvar = factored ? c->fdesc.nvar : 0;
    if (P.hist == 1 && nvar != 2 * P.A) return fail(c, FBA_ESTATE, "fba_belief_summary: gridworld records without their %d parent-set words", 2 * P.A);
    const bool want_edge = nvar > 0 && (edge_prob || (P.hist == 1 && mean_counts));
    size_t per_slot = 2 + (size_t)S + (mean_counts ? (size_t)dense_C : 0) + (size_t)nvar * 17;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)count, (size_t)32768, ((size_t)256 << 20) / (per_slot * 8)}));
    ScratchBuf<double> d_head, d_state, d_mean, d_emass, d_eprob;
    materialize_records(c);   // the kernels below read 64-byte records
    HIPCHK(c, d_head.alloc((size_t)chunk * 2));
    if (state_mass) HIPCHK(c, d_state.alloc((size_t)chunk * S));
    if (mean_counts) HIPCHK(c, d_mean.alloc((size_t)chunk * dense_C));
    if (want_edge) {
        HIPCHK(c, d_emass.alloc((size_t)chunk * nvar * 9));
        if (edge_prob) HIPCHK(c, d_eprob.alloc((size_t)chunk * nvar * MAXF));
    }
    std::vector<double> h_head((size_t)chunk * 2);
    for (int done = 0; done < count; done += chunk) {
        const int n = std::min(chunk, count - done);
        BeliefSummaryArgs a{};
        a.first = first + done; a.count = n;
        a.head = d_head.p; a.state_mass = d_state.p; a.mean_counts = d_mean.p; a.edge_mass = d_emass.p; a.edge_prob = d_eprob.p;
        a.dense_C = dense_C; a.ncounts = ncounts; a.nvar = nvar;
        a.cb = 256;
        if (dense_C < 256) { a.cb = 1; while (a.cb < dense_C) a.cb <<= 1; }
        a.lds_states = S <= 4096 ? 1 : 0;
        a.ft_FS = factored ? c->fdesc.FS : 0;
        if (state_mass && !a.lds_states) HIPCHK(c, hipMemsetAsync(d_state.p, 0, (size_t)n * S * 8, c->stream));
        if (mean_counts && P.hist) HIPCHK(c, hipMemsetAsync(d_mean.p, 0, (size_t)n * dense_C * 8, c->stream));
        launch_belief_summary(P, c->D, a, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h_head.data(), d_head.p, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
        if (state_mass) HIPCHK(c, hipMemcpyAsync(state_mass + (size_t)done * S, d_state.p, (size_t)n * S * 8, hipMemcpyDeviceToHost, c->stream));
        if (mean_counts) HIPCHK(c, hipMemcpyAsync(mean_counts + (size_t)done * dense_C, d_mean.p, (size_t)n * dense_C * 8, hipMemcpyDeviceToHost, c->stream));
        if (edge_prob && nvar) HIPCHK(c, hipMemcpyAsync(edge_prob + (size_t)done * nvar * MAXF, d_eprob.p, (size_t)n * nvar * MAXF * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (head)
            for (int i = 0; i < n; ++i) {
                fba_belief_summary_head& h = head[done + i];
                h.weight_total = h_head[(size_t)i * 2]; h.weight_sq_total = h_head[(size_t)i * 2 + 1];
                h.particles = P.N; h.weighted = P.belief == FBA_BELIEF_IMPORTANCE ? 1 : 0;
            }
    }
    return check_fault(c);
}

// per parent-set word of a factored model: the word is legal below this (1 << n_candidates of every node it serves, the rule of
// fba_belief_import); empty where the model has no words
static void structure_limits(const fba_ctx* c, std::vector<uint32_t>& limit)
{
    limit.clear();
    if (c->P.model != FBA_MODEL_BA_FACTORED || c->fdesc.nvar <= 0) return;
    limit.assign((size_t)c->fdesc.nvar, 0xffffffffu);
    const int nodes = c->P.A * (c->fdesc.FS + c->fdesc.FO);
    for (int k = 0; k < nodes && k < MAXNODES; ++k) {
        const FNode& nd = c->fdesc.nodes[k];
        if (nd.var >= 0 && nd.var < c->fdesc.nvar && nd.nmax >= 0 && nd.nmax < 32) limit[(size_t)nd.var] = std::min(limit[(size_t)nd.var], 1u << nd.nmax);
    }
}

int fba_structure_lens(const fba_ctx* c, int32_t* n_words, int32_t* n_sets)
{
    if (!c) return FBA_EINVAL;
    int nw = 0, ns = 0;
    if (c->P.model == FBA_MODEL_BA_FACTORED && c->fdesc.nvar > 0) {
        nw = c->fdesc.nvar;
        int most = 0;
        const int nodes = c->P.A * (c->fdesc.FS + c->fdesc.FO);
        for (int k = 0; k < nodes && k < MAXNODES; ++k)
            if (c->fdesc.nodes[k].var >= 0) most = std::max(most, (int)c->fdesc.nodes[k].nmax);
        ns = 1 << std::min(most, MAXF);
    }
    if (n_words) *n_words = nw;
    if (n_sets) *n_sets = ns;
    return FBA_OK;
}

// What fba_belief_structures and fba_structure_stats_enable (`who`) refuse alike, each with one text: the context ...
static int structures_check_context(fba_ctx* c, const char* who, int32_t* n_words, int32_t* n_sets)
{
    const Problem& P = c->P;
    if (P.nested)
        return fail(c, FBA_EINVAL, "%s: the nested belief's particles are (model, state filter) pairs; read them with "
                                   "fba_belief_get and fba_belief_get_nested", who);
    fba_structure_lens(c, n_words, n_sets);
    if (*n_words == 0)
        return fail(c, FBA_EINVAL, "%s: the model has no parent-set words (fba_structure_lens is 0, 0): %s", who,
                    P.model == FBA_MODEL_BA_FACTORED ? "its graph is fixed" : "only a factored model under a structure prior learns its graph");
    return FBA_OK;
}
// ... the queries ...
static int structures_check_queries(fba_ctx* c, const char* who, int32_t nq, int32_t nq_max, const char* nq_max_text, const uint32_t* query, int nw)
{
    if (nq < 0 || nq > nq_max) return fail(c, FBA_EINVAL, "%s: %d queries (0 to %s are served)", who, nq, nq_max_text);
    if (nq > 0 && !query) return fail(c, FBA_EINVAL, "%s: %d queries and no query array", who, nq);
    std::vector<uint32_t> limit;
    structure_limits(c, limit);
    for (int q = 0; q < nq; ++q)
        for (int m = 0; m < nw; ++m)
            if (query[(size_t)q * nw + m] >= limit[(size_t)m])
                return fail(c, FBA_EINVAL, "%s: query %d, word %d: 0x%x names a parent beyond the node's candidates (legal below 0x%x)", who, q, m,
                            query[(size_t)q * nw + m], limit[(size_t)m]);
    return FBA_OK;
}
// ... and a record layout whose words the kernels cannot find
static int structures_check_layout(fba_ctx* c, const char* who, int nw)
{
    const Problem& P = c->P;
    if (P.hist && (P.hist != 1 || nw != 2 * P.A || nw >= 32)) return fail(c, FBA_ESTATE, "%s: history records without their %d parent-set words", who, 2 * P.A);
    if (P.ft_packed && nw != 1) return fail(c, FBA_ESTATE, "%s: packed factored-tiger records of %d parent-set words", who, nw);
    return FBA_OK;
}
// the queries as the records hold a structure ([nq][n_keys]): history records keep one bit per word (the word is 3 or 7, fba_belief_get
// expands it), one key word in all
static void structure_query_keys(const Problem& P, int nq, int nw, const uint32_t* query, std::vector<uint32_t>& keys)
{
    const int nk = P.hist ? 1 : nw;
    keys.assign((size_t)nq * nk, 0u);
    for (int q = 0; q < nq; ++q) {
        const uint32_t* qw = query + (size_t)q * nw;
        if (!P.hist) { std::copy(qw, qw + nw, keys.begin() + (size_t)q * nk); continue; }
        uint32_t bits = 0;
        for (int m = 0; m < nw; ++m) {
            if (qw[m] == 7u) bits |= 1u << m;
            else if (qw[m] != 3u) { bits = 0xffffffffu; break; }   // (legal for the node, but no record holds it: mass 0)
        }
        keys[(size_t)q] = bits;
    }
}

// The parent-set word lists of slots [first, first + count) reduced on the device (fba_structures.hip), a chunk of slots at a time so that
// the buffers of a chunk stay below 256 MB.  Reads the context only, as fba_belief_summary does.
int fba_belief_structures(fba_ctx* c, int32_t first, int32_t count, int32_t top_k, int32_t nq, const uint32_t* query, fba_structure_head* head,
                          double* set_mass, uint32_t* top_words, double* top_mass, double* query_mass)
{
    if (!c) return FBA_EINVAL;
    const Problem& P = c->P;
    int32_t nw = 0, ns = 0;
    TRY(structures_check_context(c, "fba_belief_structures", &nw, &ns));
    if (first < 0 || count < 0 || (long long)first + count > P.E)
        return fail(c, FBA_EINVAL, "fba_belief_structures: slots [%d, %lld) are not within the context's %d", first, (long long)first + count, P.E);
    if (top_k < 0 || top_k > FBA_STRUCT_MAX_TOP) return fail(c, FBA_EINVAL, "fba_belief_structures: top_k %d (0 to %d are served)", top_k, FBA_STRUCT_MAX_TOP);
    TRY(structures_check_queries(c, "fba_belief_structures", nq, 1 << 16, "65 536", query, nw));
    if (top_k == 0) { top_words = nullptr; top_mass = nullptr; }
    if (nq == 0) query_mass = nullptr;
    if (count == 0 || (!head && !set_mass && !top_words && !top_mass && !query_mass)) return FBA_OK;
    TRY(structures_check_layout(c, "fba_belief_structures", nw));
    const int nk = P.hist ? 1 : nw;
    std::vector<uint32_t> keys;
    if (query_mass) structure_query_keys(P, nq, nw, query, keys);
    uint64_t keep = ~0ull;   // (FBA_STRUCT_HASH_KEEP in the environment: the bits of the table's hash that count, read at every call -- the tests' way to equal hashes)
    if (const char* ev = std::getenv("FBA_STRUCT_HASH_KEEP")) keep = std::strtoull(ev, nullptr, 0);
    const size_t per_slot = sizeof(fba_structure_head) + (set_mass ? (size_t)nw * ns * 8 : 0) + (top_words ? (size_t)top_k * nw * 4 : 0) +
                            (top_mass ? (size_t)top_k * 8 : 0) + (query_mass ? (size_t)nq * 8 : 0);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)count, (size_t)32768, ((size_t)256 << 20) / per_slot}));
    ScratchBuf<fba_structure_head> d_head;
    ScratchBuf<double> d_set, d_tmass, d_qmass;
    ScratchBuf<uint32_t> d_twords, d_query;
    materialize_records(c);   // the kernel below reads 64-byte records
    HIPCHK(c, d_head.alloc((size_t)chunk));
    if (set_mass) HIPCHK(c, d_set.alloc((size_t)chunk * nw * ns));
    if (top_words) HIPCHK(c, d_twords.alloc((size_t)chunk * top_k * nw));
    if (top_mass) HIPCHK(c, d_tmass.alloc((size_t)chunk * top_k));
    if (query_mass) {
        HIPCHK(c, d_qmass.alloc((size_t)chunk * nq));
        HIPCHK(c, d_query.alloc(keys.size()));
        HIPCHK(c, hipMemcpyAsync(d_query.p, keys.data(), keys.size() * 4, hipMemcpyHostToDevice, c->stream));
    }
    for (int done = 0; done < count; done += chunk) {
        const int n = std::min(chunk, count - done);
        BeliefStructuresArgs a{};
        a.first = first + done; a.count = n; a.top_k = top_k; a.nq = query_mass ? nq : 0;
        a.n_words = nw; a.n_sets = ns; a.n_keys = nk; a.ncounts = c->fdesc.ncounts; a.hash_keep = keep;
        a.query = d_query.p; a.head = d_head.p; a.set_mass = d_set.p; a.top_words = d_twords.p; a.top_mass = d_tmass.p; a.query_mass = d_qmass.p;
        if (query_mass && nq > STRUCT_QUERY_LDS) HIPCHK(c, hipMemsetAsync(d_qmass.p, 0, (size_t)n * nq * 8, c->stream));   // (those add to the output directly)
        launch_belief_structures(P, c->D, a, c->stream);
        HIPCHK(c, hipGetLastError());
        if (head) HIPCHK(c, hipMemcpyAsync(head + done, d_head.p, (size_t)n * sizeof(fba_structure_head), hipMemcpyDeviceToHost, c->stream));
        if (set_mass) HIPCHK(c, hipMemcpyAsync(set_mass + (size_t)done * nw * ns, d_set.p, (size_t)n * nw * ns * 8, hipMemcpyDeviceToHost, c->stream));
        if (top_words) HIPCHK(c, hipMemcpyAsync(top_words + (size_t)done * top_k * nw, d_twords.p, (size_t)n * top_k * nw * 4, hipMemcpyDeviceToHost, c->stream));
        if (top_mass) HIPCHK(c, hipMemcpyAsync(top_mass + (size_t)done * top_k, d_tmass.p, (size_t)n * top_k * 8, hipMemcpyDeviceToHost, c->stream));
        if (query_mass) HIPCHK(c, hipMemcpyAsync(query_mass + (size_t)done * nq, d_qmass.p, (size_t)n * nq * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return check_fault(c);
}

int fba_predict_lens(const fba_ctx* c, int32_t* TL, int32_t* OL)
{
    if (!c) return FBA_EINVAL;
    int tl = 0, ol = 0;
    if (c->P.model == FBA_MODEL_BA_FACTORED) {
        for (int f = 0; f < c->fdesc.FS; ++f) tl += c->fdesc.Ssz[f];
        for (int f = 0; f < c->fdesc.FO; ++f) ol += c->fdesc.Osz[f];
    } else if (c->P.model == FBA_MODEL_BA_TABLE) {
        tl = c->P.S; ol = c->P.O;
    }
    if (TL) *TL = tl;
    if (OL) *OL = ol;
    return FBA_OK;
}

namespace {
// pack_features and node_row of fba_device.h on the host: the features of an index, 8 bits each, and DBNNode::cptIndex
uint64_t predict_features(int v, const int32_t* step, int n)
{
    if (n == 1) return (uint64_t)v;
    uint64_t p = 0;
    for (int i = 0; i < n; ++i) { p |= (uint64_t)(v / step[i]) << (8 * i); v = v % step[i]; }
    return p;
}
int predict_node_row(const FNode& nd, uint32_t mask, uint64_t fv)
{
    int idx = 0;
    for (int j = 0; j < nd.nmax; ++j)
        if ((mask >> j) & 1u) idx = idx * nd.psz[j] + (int)((fv >> (8 * nd.maxp[j])) & 0xffu);
    return nd.off + idx * nd.out;
}
}  // namespace

// The posterior-predictive model of slots [first, first + count) at nq queries, reduced on the device (fba_predict.hip), a chunk of slots at
// a time so that the fp64 buffers of a chunk stay below 256 MB.  Reads the context only, as fba_belief_summary does.
int fba_belief_predict(fba_ctx* c, int32_t first, int32_t count, int32_t nq, const int32_t* state, const int32_t* action, const int32_t* next_state,
                       const int32_t* obs, double* trans, double* obsp, double* joint)
{
    if (!c) return FBA_EINVAL;
    const Problem& P = c->P;
    if (P.nested)
        return fail(c, FBA_EINVAL, "fba_belief_predict: the nested belief's particles are (model, state filter) pairs; read them with "
                                   "fba_belief_get and fba_belief_get_nested");
    if (P.model == FBA_MODEL_POMDP) return fail(c, FBA_EINVAL, "fba_belief_predict: a plain POMDP belief has no counts (fba_counts_len is 0)");
    if (first < 0 || count < 0 || (long long)first + count > P.E)
        return fail(c, FBA_EINVAL, "fba_belief_predict: slots [%d, %lld) are not within the context's %d", first, (long long)first + count, P.E);
    if (nq < 1 || nq > (1 << 24)) return fail(c, FBA_EINVAL, "fba_belief_predict: %d queries (1 to 16 777 216 are served)", nq);
    if (!state || !action || !next_state || !obs) return fail(c, FBA_EINVAL, "fba_belief_predict: a query array is missing");
    for (int q = 0; q < nq; ++q)
        if (state[q] < 0 || state[q] >= P.S || action[q] < 0 || action[q] >= P.A || next_state[q] < 0 || next_state[q] >= P.S || obs[q] < 0 || obs[q] >= P.O)
            return fail(c, FBA_EINVAL, "fba_belief_predict: query %d (state %d, action %d, next_state %d, obs %d) is outside the model's %d states, %d actions, "
                                       "%d observations", q, state[q], action[q], next_state[q], obs[q], P.S, P.A, P.O);
    if (count == 0 || (!trans && !obsp && !joint)) return FBA_OK;
    const bool factored = P.model == FBA_MODEL_BA_FACTORED;
    const FDesc& fd = c->fdesc;
    const int S = P.S, A = P.A, O = P.O, FS = factored ? fd.FS : 1, FO = factored ? fd.FO : 1, nn = FS + FO;
    int32_t TL = 0, OL = 0;
    fba_predict_lens(c, &TL, &OL);
    const int TLOL = TL + OL, hw = TLOL + 2 * PREDICT_SLOTS + 1;
    if (nn > PREDICT_MAXQN) return fail(c, FBA_ESTATE, "fba_belief_predict: %d nodes per action (at most %d are served)", nn, PREDICT_MAXQN);
    std::vector<int32_t> seg((size_t)nn, 0);
    int longest = 1;
    for (int j = 0, t = 0, o = 0; j < nn; ++j) {
        const int len = !factored ? (j == 0 ? S : O) : (j < FS ? fd.Ssz[j] : fd.Osz[j - FS]);
        seg[(size_t)j] = j < FS ? t : o;
        (j < FS ? t : o) += len;
        longest = std::max(longest, len);
    }
    ScratchBuf<int32_t> d_query, d_seg, d_slot;
    ScratchBuf<PredictSlotNode> d_qn;
    ScratchBuf<float> d_qprior;
    HIPCHK(c, d_query.alloc((size_t)nq * 4));
    HIPCHK(c, d_seg.alloc((size_t)nn));
    HIPCHK(c, hipMemcpyAsync(d_query.p, state, (size_t)nq * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_query.p + nq, action, (size_t)nq * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_query.p + (size_t)2 * nq, next_state, (size_t)nq * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_query.p + (size_t)3 * nq, obs, (size_t)nq * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_seg.p, seg.data(), (size_t)nn * 4, hipMemcpyHostToDevice, c->stream));
    // history records: what the shared prior contributes to each query -- per entry-cell slot the queried row per prior form
    std::vector<PredictSlotNode> qn;
    std::vector<float> qprior;
    std::vector<int32_t> ent_slot;
    if (P.hist) {
        if (hw * (int)sizeof(double) > 64 * 1024) return fail(c, FBA_ESTATE, "fba_belief_predict: an answer of %d entries does not fit the kernel's LDS", TLOL);
        if (P.hist == 1 && (FS != 3 || FO != 3 || fd.nvar != 2 * A))
            return fail(c, FBA_ESTATE, "fba_belief_predict: gridworld records without their %d parent-set words", 2 * A);
        if (P.hist == 3 && (FS > 4 || FO > 2)) return fail(c, FBA_ESTATE, "fba_belief_predict: collision-avoidance records of %d + %d nodes", FS, FO);
        const int XYd = P.hist == 1 ? c->gdesc.N * c->gdesc.N * c->gdesc.G * c->gdesc.N : 0;
        auto slot_node = [&](int k) { return P.hist == 3 ? (k < 4 ? (k < FS ? k : -1) : (k - 4 < FO ? FS + k - 4 : -1)) : (k < nn ? k : -1); };
        qn.assign((size_t)nq * PREDICT_SLOTS, PredictSlotNode{});
        qprior.assign((size_t)nq * 2 * TLOL, 0.f);
        ent_slot.assign((size_t)TLOL, 0);
        for (int k = 0; k < PREDICT_SLOTS; ++k) {
            const int j = slot_node(k);
            if (j < 0) continue;
            const int len = !factored ? (j == 0 ? S : O) : (j < FS ? fd.Ssz[j] : fd.Osz[j - FS]);
            for (int i = 0; i < len; ++i) ent_slot[(size_t)(j < FS ? 0 : TL) + seg[(size_t)j] + i] = k;
        }
        for (int q = 0; q < nq; ++q) {
            const int s = state[q], a = action[q], ns = next_state[q], ob = obs[q];
            for (int k = 0; k < PREDICT_SLOTS; ++k) {
                PredictSlotNode& n = qn[(size_t)q * PREDICT_SLOTS + k];
                n.var = -1;
                const int j = slot_node(k);
                if (j < 0) continue;
                const bool T = j < FS;
                const int f  = T ? j : j - FS;
                n.seg = (T ? 0 : TL) + seg[(size_t)j];
                const float* alt = nullptr;   // the row of form 1 where there is one
                if (!factored) {
                    n.rb0 = n.rb1 = T ? (s * A + a) * S : P.phi_len + (a * S + ns) * O;
                    n.out = T ? S : O;
                    n.val = T ? ns : ob;
                } else {
                    const FNode& nd   = fd.nodes[T ? a * FS + f : A * FS + a * FO + f];
                    const uint64_t fv = predict_features(T ? s : ns, fd.Sstep, FS);
                    n.out = nd.out;
                    n.val = T ? (int)((predict_features(ns, fd.Sstep, FS) >> (8 * f)) & 0xffu) : (int)((predict_features(ob, fd.Ostep, FO) >> (8 * f)) & 0xffu);
                    if (P.hist == 1 && nd.var >= 0) {   // an x / y node: with (7) or without (3) the goal parent, as fba_belief_get writes the word
                        if (nd.var != 2 * a + f || f > 1) return fail(c, FBA_ESTATE, "fba_belief_predict: parent-set word %d at node T(%d, %d)", nd.var, a, f);
                        n.var = nd.var;
                        n.rb0 = predict_node_row(nd, 3u, fv);
                        n.rb1 = predict_node_row(nd, 7u, fv);
                        alt   = c->prior_alt.data() + (size_t)(a * 2 + f) * XYd + (n.rb1 - nd.off);
                    } else
                        n.rb0 = n.rb1 = predict_node_row(nd, nd.fixed_mask, fv);
                }
                if (n.val < 0 || n.val >= n.out || (size_t)n.seg + n.out > (size_t)TLOL || n.rb0 < 0 || (size_t)n.rb0 + n.out > c->prior.size())
                    return fail(c, FBA_ESTATE, "fba_belief_predict: query %d does not fit the layout at slot %d", q, k);
                float* p0 = &qprior[((size_t)q * 2) * TLOL + n.seg];
                float* p1 = p0 + TLOL;
                for (int i = 0; i < n.out; ++i) {
                    p0[i] = c->prior[(size_t)n.rb0 + i];
                    p1[i] = alt ? alt[i] : 0.f;
                    n.prs0 += (double)p0[i];
                    n.prs1 += (double)p1[i];
                }
            }
        }
        HIPCHK(c, d_qn.alloc(qn.size()));
        HIPCHK(c, d_qprior.alloc(qprior.size()));
        HIPCHK(c, d_slot.alloc(ent_slot.size()));
        HIPCHK(c, hipMemcpyAsync(d_qn.p, qn.data(), qn.size() * sizeof(PredictSlotNode), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_qprior.p, qprior.data(), qprior.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_slot.p, ent_slot.data(), ent_slot.size() * 4, hipMemcpyHostToDevice, c->stream));
    }
    const size_t per_slot = (size_t)nq * ((trans ? (size_t)TL : 0) + (obsp ? (size_t)OL : 0) + 1 + (P.hist ? (size_t)hw : 0)) + 1;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)count, (size_t)32768, ((size_t)256 << 20) / (per_slot * 8)}));
    ScratchBuf<double> d_trans, d_obsp, d_joint, d_wtot, d_hacc;
    materialize_records(c);   // the kernels below read 64-byte records
    HIPCHK(c, d_wtot.alloc((size_t)chunk));
    if (trans) HIPCHK(c, d_trans.alloc((size_t)chunk * nq * TL));
    if (obsp) HIPCHK(c, d_obsp.alloc((size_t)chunk * nq * OL));
    if (joint) HIPCHK(c, d_joint.alloc((size_t)chunk * nq));
    if (P.hist) HIPCHK(c, d_hacc.alloc((size_t)chunk * nq * hw));
    for (int done = 0; done < count; done += chunk) {
        const int n = std::min(chunk, count - done);
        BeliefPredictArgs a{};
        a.first = first + done; a.count = n; a.nq = nq;
        a.state = d_query.p; a.action = d_query.p + nq; a.next_state = d_query.p + (size_t)2 * nq; a.obs = d_query.p + (size_t)3 * nq;
        a.trans = d_trans.p; a.obsp = d_obsp.p; a.joint = d_joint.p; a.wtot = d_wtot.p;
        a.TL = TL; a.OL = OL; a.nn = nn; a.nT = FS;
        a.ncounts = factored ? fd.ncounts : c->dense_C;
        a.jw = 1;
        while (a.jw < longest && a.jw < 64) a.jw <<= 1;
        a.ft_FS = factored ? fd.FS : 0;
        a.seg = d_seg.p; a.qn = d_qn.p; a.qprior = d_qprior.p; a.ent_slot = d_slot.p; a.hacc = d_hacc.p;
        if (P.hist) HIPCHK(c, hipMemsetAsync(d_hacc.p, 0, (size_t)n * nq * hw * 8, c->stream));
        launch_belief_predict(P, c->D, a, c->stream);
        HIPCHK(c, hipGetLastError());
        if (trans) HIPCHK(c, hipMemcpyAsync(trans + (size_t)done * nq * TL, d_trans.p, (size_t)n * nq * TL * 8, hipMemcpyDeviceToHost, c->stream));
        if (obsp) HIPCHK(c, hipMemcpyAsync(obsp + (size_t)done * nq * OL, d_obsp.p, (size_t)n * nq * OL * 8, hipMemcpyDeviceToHost, c->stream));
        if (joint) HIPCHK(c, hipMemcpyAsync(joint + (size_t)done * nq, d_joint.p, (size_t)n * nq * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return check_fault(c);
}

// What the forecast's and the probe's kernels need to know of a model's layout: where node j's entries start in a particle's transition
// table (TL entries), its rows in the observation table (RL rows), the rows of the max layout, the lanes that share one row and the
// particles of one workgroup (what the LDS holds); FBA_ESTATE (named after `who`) where the model does not fit the kernels
namespace {

struct FactorLayout {
    BeliefFactorLayout lay{};         // for the kernels: everything but seg and rows, which point to the device copy the caller makes ...
    std::vector<int32_t> seg, rows;   // ... of these ([nn] each)
    int nn = 2;
};
int factor_layout(fba_ctx* c, const char* who, FactorLayout& fl)
{
    const Problem& P = c->P;
    int FS, FO, TL, RL, longest;
    int& nn = fl.nn;
    std::vector<int32_t>&seg = fl.seg, &rows = fl.rows;
    const bool factored = P.model == FBA_MODEL_BA_FACTORED;
    const FDesc& fd = c->fdesc;
    const int S = P.S, A = P.A;
    FS = factored ? fd.FS : 1; FO = factored ? fd.FO : 1; nn = FS + FO;
    if (FS > MAXF || FO > MAXF || nn > PREDICT_MAXQN) return fail(c, FBA_ESTATE, "%s: %d + %d nodes per action (at most %d each are served)", who, FS, FO, MAXF);
    if (P.hist == 1 && (FS != 3 || FO != 3 || fd.nvar != 2 * A))
        return fail(c, FBA_ESTATE, "%s: gridworld records without their %d parent-set words", who, 2 * A);
    if (P.hist == 3 && (FS > 4 || FO > 2)) return fail(c, FBA_ESTATE, "%s: collision-avoidance records of %d + %d nodes", who, FS, FO);
    // where node j's entries start in a particle's transition table, its rows in the observation table; the rows of the max layout.  The
    // sizes are those of action 0's nodes: every action's nodes have them (checked)
    seg.assign((size_t)nn, 0); rows.assign((size_t)nn, 1);
    TL = 0; RL = 0; longest = 1;
    for (int j = 0; j < nn; ++j) {
        int len, nrows;
        if (!factored) { len = j == 0 ? S : P.O; nrows = j == 0 ? S * A : S; }
        else {
            const bool T = j < FS;
            const FNode& n0 = fd.nodes[T ? j : A * FS + (j - FS)];
            len = n0.out;
            nrows = 1;
            for (int p = 0; p < n0.nmax; ++p)
                if (n0.var >= 0 || ((n0.fixed_mask >> p) & 1u)) nrows *= n0.psz[p];
            for (int a = 0; a < A; ++a) {
                const FNode& nd = fd.nodes[T ? a * FS + j : A * FS + a * FO + (j - FS)];
                int r = 1;
                for (int p = 0; p < nd.nmax; ++p)
                    if (nd.var >= 0 || ((nd.fixed_mask >> p) & 1u)) r *= nd.psz[p];
                if (nd.out != len || nd.out != (T ? fd.Ssz[j] : fd.Osz[j - FS]) || nd.nmax > MAXF) return fail(c, FBA_ESTATE, "%s: node %d of action %d does not fit the layout", who, j, a);
                if (P.hist == 1 && nd.var >= 0 && (nd.var != 2 * a + j || j > 1)) return fail(c, FBA_ESTATE, "%s: parent-set word %d at node T(%d, %d)", who, nd.var, a, j);
                nrows = std::max(nrows, r);
            }
        }
        rows[(size_t)j] = nrows;
        if (j < FS) { seg[(size_t)j] = TL; TL += len; }
        else { seg[(size_t)j] = RL; RL += nrows; }
        longest = std::max(longest, len);
    }
    // particles per workgroup: what fits the LDS
    const size_t fixed = forecast_lds_bytes(TL, RL, nn, 0, P.hist != 0), per = forecast_lds_bytes(TL, RL, nn, 1, P.hist != 0) - fixed;
    if (fixed + per > (size_t)FORECAST_LDS)
        return fail(c, FBA_ESTATE, "%s: one particle's factor tables (%d transition entries, %d observation rows) do not fit the kernel's LDS", who, TL, RL);
    BeliefFactorLayout& lay = fl.lay;
    lay.nT = FS; lay.nO = FO; lay.TL = TL; lay.RL = RL;
    lay.chunk = (int)std::min<size_t>({(size_t)256, (size_t)P.N, ((size_t)FORECAST_LDS - fixed) / per});
    lay.ncounts = factored ? fd.ncounts : c->dense_C;
    lay.jw = 1;
    while (lay.jw < longest && lay.jw < 64) lay.jw <<= 1;
    lay.ft_FS = factored ? fd.FS : 0;
    return FBA_OK;
}

}  // namespace

// The one-step predictive of slots [first, first + count) after action[slot] and under obs[slot], reduced on the device (fba_forecast.hip),
// a chunk of slots at a time so that the fp64 buffers of a chunk stay below 256 MB.  Reads the context only, as fba_belief_summary does.
int fba_belief_forecast(fba_ctx* c, int32_t first, int32_t count, const int32_t* action, const int32_t* obs, double* next_mass, double* post_mass,
                        double* evidence)
{
    if (!c) return FBA_EINVAL;
    const Problem& P = c->P;
    if (P.nested)
        return fail(c, FBA_EINVAL, "fba_belief_forecast: the nested belief's particles are (model, state filter) pairs; read them with "
                                   "fba_belief_get and fba_belief_get_nested");
    if (P.model == FBA_MODEL_POMDP) return fail(c, FBA_EINVAL, "fba_belief_forecast: a plain POMDP belief has no counts (fba_counts_len is 0)");
    if (first < 0 || count < 0 || (long long)first + count > P.E)
        return fail(c, FBA_EINVAL, "fba_belief_forecast: slots [%d, %lld) are not within the context's %d", first, (long long)first + count, P.E);
    if (!next_mass && !post_mass && !evidence) return FBA_OK;
    if (!obs && (post_mass || evidence)) return fail(c, FBA_EINVAL, "fba_belief_forecast: post_mass and evidence need the observations (obs is NULL)");
    if (count == 0) return FBA_OK;
    if (!action) return fail(c, FBA_EINVAL, "fba_belief_forecast: the action array is missing");
    for (int b = 0; b < count; ++b) {
        if (action[b] < 0 || action[b] >= P.A)
            return fail(c, FBA_EINVAL, "fba_belief_forecast: slot %d: action %d is outside the model's %d actions", first + b, action[b], P.A);
        if (obs && (obs[b] < 0 || obs[b] >= P.O))
            return fail(c, FBA_EINVAL, "fba_belief_forecast: slot %d: observation %d is outside the model's %d observations", first + b, obs[b], P.O);
    }
    FactorLayout fl;
    if (const int rc = factor_layout(c, "fba_belief_forecast", fl)) return rc;
    const int S = P.S, nn = fl.nn;
    if (P.hist) {   // a slot whose records hold more entries than they have room for has no readable filter (the update kernels report it)
        std::vector<uint32_t> cnt((size_t)count);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(cnt.data(), c->D.hist_cnt + first, (size_t)count * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < count; ++b)
            if (hist_total(cnt[(size_t)b]) > P.hist_cap)
                return fail(c, FBA_ESTATE, "fba_belief_forecast: slot %d: the history records hold %d entries, more than their %d", first + b, hist_total(cnt[(size_t)b]), P.hist_cap);
    }
    ScratchBuf<int32_t> d_in, d_meta;
    HIPCHK(c, d_in.alloc((size_t)count * 2));
    HIPCHK(c, d_meta.alloc((size_t)nn * 2));
    HIPCHK(c, hipMemcpyAsync(d_in.p, action, (size_t)count * 4, hipMemcpyHostToDevice, c->stream));
    if (obs) HIPCHK(c, hipMemcpyAsync(d_in.p + count, obs, (size_t)count * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_meta.p, fl.seg.data(), (size_t)nn * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_meta.p + nn, fl.rows.data(), (size_t)nn * 4, hipMemcpyHostToDevice, c->stream));
    fl.lay.seg = d_meta.p; fl.lay.rows = d_meta.p + nn;
    const size_t per_slot = (size_t)S * 4 + 1;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)count, (size_t)32768, ((size_t)256 << 20) / (per_slot * 8)}));
    ScratchBuf<double> d_acc, d_next, d_post, d_ev;
    materialize_records(c);   // the kernels below read 64-byte records
    HIPCHK(c, d_acc.alloc((size_t)chunk * 2 * S));
    if (next_mass) HIPCHK(c, d_next.alloc((size_t)chunk * S));
    if (post_mass) HIPCHK(c, d_post.alloc((size_t)chunk * S));
    if (evidence) HIPCHK(c, d_ev.alloc((size_t)chunk));
    for (int done = 0; done < count; done += chunk) {
        const int n = std::min(chunk, count - done);
        BeliefForecastArgs a{};
        a.first = first + done; a.count = n;
        a.action = d_in.p + done; a.obs = obs ? d_in.p + count + done : nullptr;
        a.next_mass = d_next.p; a.post_mass = d_post.p; a.evidence = d_ev.p; a.acc = d_acc.p;
        a.lay = fl.lay;
        HIPCHK(c, hipMemsetAsync(d_acc.p, 0, (size_t)n * 2 * S * 8, c->stream));
        launch_belief_forecast(P, c->D, a, c->stream);
        HIPCHK(c, hipGetLastError());
        if (next_mass) HIPCHK(c, hipMemcpyAsync(next_mass + (size_t)done * S, d_next.p, (size_t)n * S * 8, hipMemcpyDeviceToHost, c->stream));
        if (post_mass) HIPCHK(c, hipMemcpyAsync(post_mass + (size_t)done * S, d_post.p, (size_t)n * S * 8, hipMemcpyDeviceToHost, c->stream));
        if (evidence) HIPCHK(c, hipMemcpyAsync(evidence + (size_t)done, d_ev.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return check_fault(c);
}

// fba_probe: the buffers and the layout go into c->probe, which tick() hands to launch_belief_probe (fba_probe.hip) while count > 0
int fba_probe_enable(fba_ctx* c, int32_t first, int32_t count, int32_t capacity)
{
    if (!c) return FBA_EINVAL;
    const Problem& P = c->P;
    if (P.nested)
        return fail(c, FBA_EINVAL, "fba_probe_enable: the nested belief's particles are (model, state filter) pairs; read them with "
                                   "fba_belief_get and fba_belief_get_nested");
    if (P.model == FBA_MODEL_POMDP) return fail(c, FBA_EINVAL, "fba_probe_enable: a plain POMDP belief has no counts (fba_counts_len is 0)");
    if (first < 0 || count < 0 || (long long)first + count > P.E)
        return fail(c, FBA_EINVAL, "fba_probe_enable: slots [%d, %lld) are not within the context's %d", first, (long long)first + count, P.E);
    if (capacity < 0) return fail(c, FBA_EINVAL, "fba_probe_enable: a capacity of %d records", capacity);
    FactorLayout fl;
    if (count > 0)
        if (const int rc = factor_layout(c, "fba_probe_enable", fl)) return rc;
    materialize_records(c);   // (the probe reads 64-byte records: while it is on, tick() keeps them)
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (nothing in flight writes the old buffers)
    dev_free(c, c->probe.acc);
    dev_free(c, c->probe.recs);
    dev_free(c, c->probe.seen);
    dev_free(c, c->probe.step);
    dev_free(c, c->d_probe_meta);
    c->probe = BeliefProbeArgs{};
    if (count == 0) return FBA_OK;
    int rc;
    BeliefProbeArgs a{};
    if ((rc = dev_alloc(c, &a.acc, (size_t)count * 3))) return rc;
    if ((rc = dev_alloc(c, &a.recs, (size_t)capacity))) return rc;
    if ((rc = dev_alloc(c, &a.seen, 1))) return rc;
    if ((rc = dev_alloc(c, &a.step, (size_t)count * PROBE_STEP_WORDS))) return rc;
    if ((rc = dev_alloc(c, &c->d_probe_meta, (size_t)fl.nn * 2))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_probe_meta, fl.seg.data(), (size_t)fl.nn * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_probe_meta + fl.nn, fl.rows.data(), (size_t)fl.nn * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (fl is a local)
    a.first = first; a.count = count; a.capacity = capacity;
    a.lay = fl.lay;
    a.lay.chunk = std::min(fl.lay.chunk, PROBE_CHUNK);
    if (const char* env = std::getenv("FBA_PROBE_CHUNK"))   // A/B: another number of particles per workgroup, up to what the LDS holds
        a.lay.chunk = std::max(1, std::min(fl.lay.chunk, std::atoi(env)));
    a.lay.seg = c->d_probe_meta; a.lay.rows = c->d_probe_meta + fl.nn;
    c->probe = a;
    return FBA_OK;
}

int fba_probe_count(const fba_ctx* cc, int64_t* seen)
{
    fba_ctx* c = const_cast<fba_ctx*>(cc);
    if (!c) return FBA_EINVAL;
    if (seen) *seen = 0;
    if (c->probe.count <= 0) return 0;
    unsigned long long n = 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&n, c->probe.seen, sizeof n, hipMemcpyDeviceToHost) != hipSuccess) return FBA_EHIP;
    if (seen) *seen = (int64_t)n;
    return (int)std::min<unsigned long long>(n, (unsigned long long)c->probe.capacity);
}

int fba_get_probe(const fba_ctx* cc, fba_probe_rec* out, int32_t cap)
{
    fba_ctx* c = const_cast<fba_ctx*>(cc);
    if (!c || !out) return FBA_EINVAL;
    const int n = std::min(fba_probe_count(c, nullptr), cap);
    if (n <= 0) return n;
    HIPCHK(c, hipMemcpy(out, c->probe.recs, (size_t)n * sizeof(fba_probe_rec), hipMemcpyDeviceToHost));
    std::sort(out, out + n, [](const fba_probe_rec& a, const fba_probe_rec& b) {   // the order of fba_get_trace
        if (a.run != b.run) return a.run < b.run;
        if (a.episode != b.episode) return a.episode < b.episode;
        return a.t < b.t;
    });
    return n;
}

// fba_giveup_policy: the limit goes into P.reject_max, which every rejection kernel tests; the policy and the list into the context, from
// where tick() sets DeviceState::retire_on and launches retire_kernel (fba_retire.hip)
int fba_giveup_policy(fba_ctx* c, int32_t policy, int32_t max_attempts)
{
    if (!c) return FBA_EINVAL;
    if (policy != FBA_GIVEUP_STOP && policy != FBA_GIVEUP_RETIRE)
        return fail(c, FBA_EINVAL, "fba_giveup_policy: policy %d (FBA_GIVEUP_STOP = 0, FBA_GIVEUP_RETIRE = 1)", policy);
    if (max_attempts < 0 || max_attempts % FBA_REJECT_QUANTUM != 0)
        return fail(c, FBA_EINVAL, "fba_giveup_policy: max_attempts %d is not a positive multiple of FBA_REJECT_QUANTUM (%d), nor 0 for the default of %d",
                    max_attempts, FBA_REJECT_QUANTUM, REJECT_MAX_ATTEMPTS);
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (nothing in flight writes the old list)
    // max(runs, slots) records: a run is retired once.  (A context made for endless fba_run_ticks names 2^30 runs it never ends: beyond 2^22
    // records, the trace's own limit, the list keeps room for the slots and counts the rest in `seen`)
    const int32_t capacity = std::min(std::max(c->cfg.runs, c->P.E), std::max(c->P.E, 1 << 22));
    if (!c->retired.recs) {
        int rc;
        RetireArgs a{};
        if ((rc = dev_alloc(c, "retired", &a.recs, (size_t)capacity))) return rc;   // (in the report of fba_device_arrays from this call on)
        if ((rc = dev_alloc(c, "retired_seen", &a.seen, 1))) return rc;
        a.capacity = capacity;
        c->retired = a;
    } else {
        HIPCHK(c, hipMemset(c->retired.recs, 0, (size_t)capacity * sizeof(fba_retired_rec)));
        HIPCHK(c, hipMemset(c->retired.seen, 0, sizeof(unsigned long long)));
    }
    HIPCHK(c, hipMemset(c->D.gave_up, 0, (size_t)c->P.E));
    c->giveup_policy = policy;
    c->P.reject_max  = max_attempts ? max_attempts : REJECT_MAX_ATTEMPTS;
    return FBA_OK;
}

int fba_retired_count(const fba_ctx* cc, int64_t* seen)
{
    fba_ctx* c = const_cast<fba_ctx*>(cc);
    if (!c) return FBA_EINVAL;
    if (seen) *seen = 0;
    if (!c->retired.recs) return 0;
    unsigned long long n = 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&n, c->retired.seen, sizeof n, hipMemcpyDeviceToHost) != hipSuccess) return FBA_EHIP;
    if (seen) *seen = (int64_t)n;
    return (int)std::min<unsigned long long>(n, (unsigned long long)c->retired.capacity);
}

int fba_get_retired(const fba_ctx* cc, fba_retired_rec* out, int32_t cap)
{
    fba_ctx* c = const_cast<fba_ctx*>(cc);
    if (!c || !out) return FBA_EINVAL;
    const int stored = fba_retired_count(c, nullptr);
    if (stored <= 0 || cap <= 0) return std::min(stored, 0);
    // every stored record is sorted, then the first `cap` are handed over: the records of one launch are appended in no fixed order, so a
    // short buffer gets the retirements of the lowest runs, not whichever were appended first.  By run; a run that stands in the list more
    // than once (experiments repeated on one context) in the order of its retirements, which are launches apart
    std::vector<fba_retired_rec> all((size_t)stored);
    HIPCHK(c, hipMemcpy(all.data(), c->retired.recs, all.size() * sizeof(fba_retired_rec), hipMemcpyDeviceToHost));
    std::stable_sort(all.begin(), all.end(), [](const fba_retired_rec& a, const fba_retired_rec& b) { return a.run < b.run; });
    const int n = std::min(stored, cap);
    std::memcpy(out, all.data(), (size_t)n * sizeof(fba_retired_rec));
    return n;
}

// fba_step_stats: the bins go into c->step_stats and the per-slot scratch of env_kernel into D.step_scratch; tick() launches
// step_stats_kernel (fba_step_stats.hip) while they are set
int fba_step_stats_enable(fba_ctx* c, int32_t on)
{
    if (!c) return FBA_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (nothing in flight writes the old buffers)
    dev_free(c, c->step_stats.bins);
    dev_free(c, c->D.step_scratch);
    c->step_stats = StepStatsArgs{};
    if (!on) return FBA_OK;
    int rc;
    const size_t n_bins = (size_t)c->P.episodes * (size_t)c->P.horizon;
    StepStatsArgs a{};
    if ((rc = dev_alloc(c, &a.bins, n_bins))) return rc;
    if ((rc = dev_alloc(c, &c->D.step_scratch, (size_t)c->P.E))) { dev_free(c, a.bins); return rc; }
    // (a mark the probe left while the statistics were off belongs to a step that no bin accounts)
    if (c->probe.count > 0) HIPCHK(c, hipMemsetAsync(c->probe.step, 0, (size_t)c->probe.count * PROBE_STEP_WORDS * sizeof(double), c->stream));
    a.n_bins = (int32_t)n_bins;
    a.rows   = step_stats_rows(a.n_bins, c->P.A);
    c->step_stats = a;
    const char* env = std::getenv("FBA_STEP_STATS_TIME");
    c->step_stats_timed = env && std::atoi(env) != 0;
    c->step_stats_ms = 0; c->step_stats_launches = 0;
    return FBA_OK;
}

int fba_get_step_stats(fba_ctx* c, fba_step_stat* out, int32_t cap)
{
    if (!c) return FBA_EINVAL;
    if (!c->step_stats.bins) return fail(c, FBA_ESTATE, "fba_get_step_stats: the step statistics are off (fba_step_stats_enable)");
    if (!out || cap < c->step_stats.n_bins)
        return fail(c, FBA_EINVAL, "fba_get_step_stats: room for %d bins where episodes * horizon = %d are kept", out ? cap : 0, c->step_stats.n_bins);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->step_stats.bins, (size_t)c->step_stats.n_bins * sizeof(fba_step_stat), hipMemcpyDeviceToHost));
    return c->step_stats.n_bins;
}

// diagnostic (scripts/bench_step_stats.py; not part of include/fba_hip.h): step_stats_kernel's own time since fba_step_stats_enable(1),
// measured while FBA_STEP_STATS_TIME=1 stood in the environment of that call, and its launches
int fba_debug_step_stats_ms(fba_ctx* c, double* ms, uint64_t* launches)
{
    if (!c) return FBA_EINVAL;
    if (ms) *ms = c->step_stats_ms;
    if (launches) *launches = c->step_stats_launches;
    return FBA_OK;
}

// fba_structure_stats: bins, per-slot rows and the queries go into c->struct_stats; tick() launches the kernels of fba_structure_stats.hip
// while they are set
int fba_structure_stats_enable(fba_ctx* c, int32_t on, int32_t nq, const uint32_t* query)
{
    if (!c) return FBA_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (nothing in flight writes the old buffers)
    dev_free(c, c->struct_stats.bins);
    dev_free(c, c->struct_stats.rows);
    dev_free(c, c->struct_stats.query);
    c->struct_stats = StructStatsArgs{};
    if (!on) return FBA_OK;
    int32_t nw = 0, ns = 0;
    TRY(structures_check_context(c, "fba_structure_stats_enable", &nw, &ns));
    TRY(structures_check_queries(c, "fba_structure_stats_enable", nq, FBA_STRUCT_STATS_MAX_QUERIES, "16", query, nw));
    TRY(structures_check_layout(c, "fba_structure_stats_enable", nw));
    std::vector<uint32_t> keys;
    structure_query_keys(c->P, nq, nw, query, keys);
    StructStatsArgs a{};
    a.n_bins = (int32_t)((size_t)c->P.episodes * (size_t)c->P.horizon);
    a.nq = nq; a.n_words = nw; a.n_sets = ns; a.n_keys = c->P.hist ? 1 : nw; a.ncounts = c->fdesc.ncounts;
    a.row_words = struct_stats_row_words(nw, ns, nq);
    a.chunk     = struct_stats_chunk(c->P.E, a.row_words);
    a.cols      = struct_stats_cols(a.row_words);
    a.win_rows  = struct_stats_win_rows(a.n_bins, a.cols);
    a.hash_keep = ~0ull;   // (FBA_STRUCT_HASH_KEEP in the environment, as fba_belief_structures reads it: here once, at enable)
    if (const char* ev = std::getenv("FBA_STRUCT_HASH_KEEP")) a.hash_keep = std::strtoull(ev, nullptr, 0);
    uint32_t* d_query = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &a.bins, (size_t)a.n_bins * a.row_words))) return rc;
    if ((rc = dev_alloc(c, &a.rows, (size_t)a.chunk * (STRUCT_STATS_SLOT_HEAD + a.row_words - STRUCT_STATS_BIN_HEAD)))) { dev_free(c, a.bins); return rc; }
    if ((rc = dev_alloc(c, &d_query, keys.size()))) { dev_free(c, a.bins); dev_free(c, a.rows); return rc; }
    a.query = d_query;
    c->struct_stats = a;   // (from here on a failure leaves buffers the next enable or fba_destroy frees)
    if (!keys.empty()) HIPCHK(c, hipMemcpyAsync(d_query, keys.data(), keys.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (keys is the host's)
    const char* env = std::getenv("FBA_STRUCT_STATS_TIME");
    c->struct_stats_timed = env && std::atoi(env) != 0;
    c->struct_stats_ms = 0; c->struct_stats_launches = 0;
    return FBA_OK;
}

int fba_get_structure_stats(fba_ctx* c, int32_t cap_bins, fba_structure_stat* head, double* set_frac, double* query_frac, uint64_t* query_held,
                            uint64_t* query_sole)
{
    if (!c) return FBA_EINVAL;
    const StructStatsArgs& a = c->struct_stats;
    if (!a.bins) return fail(c, FBA_ESTATE, "fba_get_structure_stats: the structure statistics are off (fba_structure_stats_enable)");
    if (cap_bins < a.n_bins)
        return fail(c, FBA_EINVAL, "fba_get_structure_stats: room for %d bins where episodes * horizon = %d are kept", cap_bins, a.n_bins);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<uint64_t> h((size_t)a.n_bins * a.row_words);
    HIPCHK(c, hipMemcpy(h.data(), a.bins, h.size() * 8, hipMemcpyDeviceToHost));
    const size_t cells = (size_t)a.n_words * a.n_sets, nq = (size_t)a.nq;
    for (size_t b = 0; b < (size_t)a.n_bins; ++b) {   // a bin's words: head | set_frac | query_frac | query_held | query_sole (fba_kernels.h)
        const uint64_t* w = h.data() + b * a.row_words;
        if (head) std::memcpy(head + b, w, sizeof(fba_structure_stat));
        w += STRUCT_STATS_BIN_HEAD;
        if (set_frac) std::memcpy(set_frac + b * cells, w, cells * 8);
        if (query_frac && nq) std::memcpy(query_frac + b * nq, w + cells, nq * 8);
        if (query_held && nq) std::memcpy(query_held + b * nq, w + cells + nq, nq * 8);
        if (query_sole && nq) std::memcpy(query_sole + b * nq, w + cells + 2 * nq, nq * 8);
    }
    return a.n_bins;
}

// diagnostic (scripts/bench_structure_stats.py; not part of include/fba_hip.h): the time of the kernels of fba_structure_stats.hip since
// fba_structure_stats_enable(1), measured while FBA_STRUCT_STATS_TIME=1 stood in the environment of that call, and the ticks that launched them
int fba_debug_structure_stats_ms(fba_ctx* c, double* ms, uint64_t* launches)
{
    if (!c) return FBA_EINVAL;
    if (ms) *ms = c->struct_stats_ms;
    if (launches) *launches = c->struct_stats_launches;
    return FBA_OK;
}

int fba_belief_set(fba_ctx* c, int32_t slot, const int32_t* state, const double* weight, const float* counts)
{
    if (!c || slot < 0 || slot >= c->P.E) return FBA_EINVAL;
    const Problem& P = c->P;
    if (P.nested) return fail(c, FBA_EINVAL, "the nested belief cannot be set from the host (its weights' prefix sums and flat filters live on the device)");
    materialize_records(c, true);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint8_t sel = 0;
    HIPCHK(c, hipMemcpy(&sel, c->D.bufsel + slot, 1, hipMemcpyDeviceToHost));
    const size_t pb = ((size_t)sel * P.E + slot) * (size_t)P.N;
    if (P.hist && (state || counts))
        return fail(c, FBA_EINVAL, "this context stores particles as histories of their own steps over the shared prior (gridworld BA-POMDP), which "
                                   "cannot take on arbitrary states or counts; create it with FBA_DENSE_PARTICLES=1 in the environment to set them");
    if (state)
        for (int i = 0; i < P.N; ++i)
            if (state[i] < 0 || state[i] >= P.S) return fail(c, FBA_EINVAL, "state %d out of range", state[i]);
    if (weight && P.belief == FBA_BELIEF_IMPORTANCE) HIPCHK(c, hipMemcpy(c->D.p_weight + pb, weight, (size_t)P.N * 8, hipMemcpyHostToDevice));
    if (state || (counts && P.C)) {
        std::vector<float> tmp((size_t)P.N * P.Cs);
        HIPCHK(c, hipMemcpy(tmp.data(), c->D.p_rec + pb * P.Cs, tmp.size() * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < P.N; ++i) {
            float* rec = tmp.data() + (size_t)i * P.Cs;
            if (state) std::memcpy(&rec[P.C], &state[i], 4);
            if (counts && P.ft_packed) {
                uint32_t* w = reinterpret_cast<uint32_t*>(rec);
                const int nc = c->fdesc.ncounts;
                const float* in = counts + (size_t)i * c->dense_C;
                uint32_t mask;
                std::memcpy(&mask, &in[nc], 4);
                for (int k = 0; k < P.C; ++k) w[k] = 0;
                w[nc / 2] = mask;
                for (int k = 0; k < nc; ++k) {
                    const double inc = (double)in[k] - (double)ftiger_prior_host(c->fdesc.FS, k, mask, P.ft_acc, P.ft_inacc, P.ft_unif);
                    if (inc < 0 || inc > 65535 || inc != std::floor(inc))
                        return fail(c, FBA_EINVAL, "particle %d, count %d: %g is not the prior of its structure plus 0..65535 increments, which packed "
                                                   "particles need; create the context with FBA_DENSE_PARTICLES=1 in the environment for arbitrary counts",
                                    i, k, (double)in[k]);
                    w[k >> 1] |= (uint32_t)inc << (16 * (k & 1));
                }
            } else if (counts && P.packed) {
                uint32_t* w = reinterpret_cast<uint32_t*>(rec);
                for (int k = 0; k < P.C; ++k) w[k] = 0;
                for (int k = 0; k < c->dense_C; ++k) {
                    const double inc = (double)counts[(size_t)i * c->dense_C + k] - (double)c->prior[k];
                    if (inc < 0 || inc > 65535 || inc != std::floor(inc))
                        return fail(c, FBA_EINVAL, "particle %d, count %d: %g is not the prior (%g) plus 0..65535 increments, which packed particles "
                                                   "need; create the context with FBA_DENSE_PARTICLES=1 in the environment for arbitrary counts",
                                    i, k, (double)counts[(size_t)i * c->dense_C + k], (double)c->prior[k]);
                    w[k >> 1] |= (uint32_t)inc << (16 * (k & 1));
                }
            } else if (counts && P.C) std::copy(counts + (size_t)i * P.C, counts + (size_t)(i + 1) * P.C, rec);
        }
        HIPCHK(c, hipMemcpy(c->D.p_rec + pb * P.Cs, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
    }
    c->belief_ready = true;
    return FBA_OK;
}

// ---- belief snapshots (include/fba_hip.h; format and host pass: fba_snapshot_format.h; kernels: fba_snapshot.hip) ----

// the state a belief keeps beside its main filter, which a snapshot would not carry; null = the belief is the main filter alone
static const char* snapshot_extra_state(const fba_ctx* c)
{
    switch (c->cfg.belief) {
        case FBA_BELIEF_REJECTION: case FBA_BELIEF_IMPORTANCE: case FBA_BELIEF_POINT: return nullptr;
        case FBA_BELIEF_REINVIGORATION: return "the reinvigoration belief also keeps a fully connected filter (fba_belief_get_fully_connected)";
        case FBA_BELIEF_CHEATING: return "the cheating belief also keeps a correct-graph filter and a likelihood";
        case FBA_BELIEF_INCUBATOR: return "the incubator belief also keeps a fully connected filter and a weighted shadow filter";
        case FBA_BELIEF_MH_GIBBS: return "the mh-within-gibbs belief also keeps the run's action-observation history and log likelihood";
        case FBA_BELIEF_MH_NIPS: return "the mh-nips belief also keeps the run's action-observation history and log likelihood";
        case FBA_BELIEF_NESTED: return "the nested belief also keeps a flat filter of domain states per particle (fba_belief_get_nested)";
        default: return "this belief keeps state beside its main filter";
    }
}
static bool snapshot_weighted(const fba_ctx* c) { return c->P.belief == FBA_BELIEF_IMPORTANCE; }
// what a block must match to be taken by this context
static fba_snapshot::Accepts snapshot_accepts(const fba_ctx* c)
{
    const Problem& P = c->P;
    fba_snapshot::Accepts acc{};
    fba_snapshot_head& h = acc.want;
    h.magic = FBA_SNAPSHOT_MAGIC; h.version = FBA_SNAPSHOT_VERSION;
    h.record_format = (uint8_t)record_format(P, c->fdesc.FS);
    h.weighted = snapshot_weighted(c) ? 1 : 0;
    h.model = (uint8_t)P.model; h.domain = (uint8_t)P.domain; h.actions = (uint16_t)P.A;
    h.size = (int16_t)c->cfg.size; h.width = (int16_t)c->cfg.width; h.height = (int16_t)c->cfg.height;
    h.particles = P.N; h.particle_bytes = P.Cs * 4; h.counts_len = c->dense_C;
    h.states = P.S; h.observations = P.O;
    uint64_t ph = fba_snapshot::hash_words(FBA_SNAPSHOT_HASH_SEED, c->prior.data(), c->prior.size());
    ph = fba_snapshot::hash_words(ph, c->prior_alt.data(), c->prior_alt.size());
    ph = fba_snapshot::hash_words(ph, &P.structure_prior, 1);
    if (P.ft_packed) {
        const float listen[3] = {P.ft_acc, P.ft_inacc, P.ft_unif};
        ph = fba_snapshot::hash_words(ph, listen, 3);
    }
    h.prior_hash = ph;
    acc.hist_cap = P.hist_cap;
    acc.compact  = P.hist_compact;
    return acc;
}
// range and belief checks shared by the three calls
static int snapshot_range(fba_ctx* c, const char* call, int32_t first, int32_t count)
{
    if (first < 0 || count < 0 || (long long)first + count > c->P.E)
        return fail(c, FBA_EINVAL, "%s: slots [%d, %lld) are not within the context's %d", call, first, (long long)first + count, c->P.E);
    if (const char* extra = snapshot_extra_state(c))
        return fail(c, FBA_EINVAL, "%s: a snapshot holds the main filter of a slot, and %s", call, extra);
    return FBA_OK;
}
// a destination slot must be between steps: no update pending, no parked search, no buffer swap pending (src >= 0: skipped, but its own
// filter must be in its live buffer)
static int snapshot_quiet(fba_ctx* c, const char* call, int32_t first, int32_t count, int32_t src)
{
    if (count <= 0) return FBA_OK;
    const DeviceState& D = c->D;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<uint8_t> upd((size_t)count), swp((size_t)count, 0);
    std::vector<int32_t> sim((size_t)count, 0);
    HIPCHK(c, hipMemcpy(upd.data(), D.need_update + first, (size_t)count, hipMemcpyDeviceToHost));
    if (D.copy_pending) HIPCHK(c, hipMemcpy(swp.data(), D.copy_pending + first, (size_t)count, hipMemcpyDeviceToHost));
    if (D.s_sim) HIPCHK(c, hipMemcpy(sim.data(), D.s_sim + first, (size_t)count * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < count; ++b) {
        if (first + b == src) continue;
        if (upd[(size_t)b]) return fail(c, FBA_ESTATE, "%s: slot %d has a belief update pending", call, first + b);
        if (sim[(size_t)b]) return fail(c, FBA_ESTATE, "%s: slot %d has a parked search", call, first + b);
        if (swp[(size_t)b]) return fail(c, FBA_ESTATE, "%s: slot %d has a buffer swap pending", call, first + b);
    }
    if (src >= 0 && D.copy_pending) {
        uint8_t s = 0;
        HIPCHK(c, hipMemcpy(&s, D.copy_pending + src, 1, hipMemcpyDeviceToHost));
        if (s) return fail(c, FBA_ESTATE, "%s: slot %d has a buffer swap pending", call, src);
    }
    return FBA_OK;
}
// the kernels' arguments but for the range; d_limit: the limits of the parent-set words, uploaded here
static int snapshot_args(fba_ctx* c, BeliefSnapshotArgs& a, ScratchBuf<uint32_t>& d_limit)
{
    const Problem& P = c->P;
    const bool factored = P.model == FBA_MODEL_BA_FACTORED;
    a = BeliefSnapshotArgs{};
    a.per_slot = fba_snapshot::block_bytes(snapshot_weighted(c), P.N, (int64_t)P.Cs * 4);
    a.weighted = snapshot_weighted(c) ? 1 : 0;
    a.ncounts  = factored ? c->fdesc.ncounts : P.C;
    a.ncells   = P.hist ? (factored ? c->fdesc.ncounts : c->dense_C) : 0;
    if (factored && !P.hist && c->fdesc.nvar > 0) {
        a.nvar    = P.ft_packed ? 1 : c->fdesc.nvar;
        a.mask_at = P.ft_packed ? c->fdesc.ncounts / 2 : c->fdesc.ncounts;
        std::vector<uint32_t> limit((size_t)a.nvar, 0xffffffffu);   // word m names parents among the candidates of every node it serves
        const int nodes = P.A * (c->fdesc.FS + c->fdesc.FO);
        for (int k = 0; k < nodes && k < MAXNODES; ++k) {
            const FNode& nd = c->fdesc.nodes[k];
            if (nd.var >= 0 && nd.var < a.nvar && nd.nmax >= 0 && nd.nmax < 32) limit[(size_t)nd.var] = std::min(limit[(size_t)nd.var], 1u << nd.nmax);
        }
        HIPCHK(c, d_limit.alloc(limit.size()));
        HIPCHK(c, hipMemcpy(d_limit.p, limit.data(), limit.size() * 4, hipMemcpyHostToDevice));
        a.mask_limit = d_limit.p;
    }
    return FBA_OK;
}
// slots of one chunk: what SNAPSHOT_STAGE_BYTES of staging memory hold (one block at least), a grid's rows at most
// (FBA_SNAPSHOT_STAGE_BYTES in the environment: another bound, read at every call -- include/fba_hip.h and INTEGRATION.md section 4a state it;
// the tests use it for several chunks of a few small slots, a host short of device memory for less staging)
static int snapshot_chunk(int64_t per_slot, int32_t count)
{
    int64_t stage = (int64_t)SNAPSHOT_STAGE_BYTES;
    if (const char* ev = std::getenv("FBA_SNAPSHOT_STAGE_BYTES")) stage = std::max<int64_t>(1, std::atoll(ev));
    return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)count, (int64_t)SNAPSHOT_MAX_SLOTS, stage / per_slot}));
}

int fba_belief_snapshot_bytes(const fba_ctx* c, int64_t* per_slot)
{
    if (!c || !per_slot) return FBA_EINVAL;
    *per_slot = fba_snapshot::block_bytes(snapshot_weighted(c), c->P.N, (int64_t)c->P.Cs * 4);
    return FBA_OK;
}

int fba_belief_export(fba_ctx* c, int32_t first, int32_t count, void* buf, int64_t cap)
{
    if (!c) return FBA_EINVAL;
    int rc;
    if ((rc = snapshot_range(c, "fba_belief_export", first, count))) return rc;
    const Problem& P = c->P;
    BeliefSnapshotArgs a;
    ScratchBuf<uint32_t> d_limit;
    if ((rc = snapshot_args(c, a, d_limit))) return rc;
    const int64_t per = a.per_slot;
    if (count > 0 && (!buf || cap < (int64_t)count * per))
        return fail(c, FBA_EINVAL, "fba_belief_export: %d blocks of %lld bytes need %lld, the buffer has %lld", count, (long long)per,
                    (long long)count * per, (long long)(buf ? cap : 0));
    if (count == 0) return FBA_OK;
    materialize_records(c, true);   // a lazily reset rejection filter: write the states out first, as fba_belief_get does
    const int chunk = snapshot_chunk(per, count);
    ScratchBuf<uint8_t> d_stage;
    ScratchBuf<unsigned long long> d_check;
    HIPCHK(c, d_stage.alloc((size_t)chunk * (size_t)per));
    HIPCHK(c, d_check.alloc((size_t)chunk));
    std::vector<unsigned long long> h_check((size_t)chunk);
    std::vector<uint32_t> h_cnt((size_t)chunk, 0);
    const fba_snapshot_head want = snapshot_accepts(c).want;
    uint8_t* out = static_cast<uint8_t*>(buf);
    for (int done = 0; done < count; done += chunk) {
        const int n = std::min(chunk, count - done);
        a.first = first + done; a.count = n; a.stage = d_stage.p; a.check = d_check.p;
        HIPCHK(c, hipMemsetAsync(d_check.p, 0, (size_t)n * 8, c->stream));
        launch_snapshot_pack(P, c->D, a, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(out + (size_t)done * (size_t)per, d_stage.p, (size_t)n * (size_t)per, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(h_check.data(), d_check.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        if (P.hist) HIPCHK(c, hipMemcpyAsync(h_cnt.data(), c->D.hist_cnt + first + done, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int b = 0; b < n; ++b) {
            const int e = first + done + b;
            fba_snapshot_head h = want;
            h.hist_cnt = h_cnt[(size_t)b];
            h.stride   = (uint32_t)(P.hist ? hist_stride(P, hist_total(h.hist_cnt)) : P.Cs) * 4u;
            h.updates  = (P.packed || P.ft_packed) && (size_t)e < c->packed_updates.size() ? (uint16_t)std::min<uint32_t>(c->packed_updates[(size_t)e], 65535u) : 0;
            h.checksum = h_check[(size_t)b];
            std::memcpy(out + (size_t)(done + b) * (size_t)per, &h, sizeof h);
        }
    }
    return FBA_OK;
}

int fba_belief_import(fba_ctx* c, int32_t first, int32_t count, const void* buf, int64_t bytes)
{
    if (!c) return FBA_EINVAL;
    int rc;
    if ((rc = snapshot_range(c, "fba_belief_import", first, count))) return rc;
    const Problem& P = c->P;
    BeliefSnapshotArgs a;
    ScratchBuf<uint32_t> d_limit;
    if ((rc = snapshot_args(c, a, d_limit))) return rc;
    const int64_t per = a.per_slot;
    const uint8_t* in = static_cast<const uint8_t*>(buf);
    const fba_snapshot::Accepts acc = snapshot_accepts(c);
    if (bytes != (int64_t)count * per || (count > 0 && !buf)) {
        // (blocks of another configuration have another size: where the first header says which field differs, that is the better message)
        char msg[256];
        if (buf && count > 0 && bytes >= (int64_t)sizeof(fba_snapshot_head) && fba_snapshot::check_head(in, per, acc, msg, sizeof msg))
            return fail(c, FBA_EINVAL, "fba_belief_import: block 0 (slot %d): %s", first, msg);
        return fail(c, FBA_EINVAL, "fba_belief_import: bytes %lld / %lld (%d blocks of %lld)", (long long)(buf ? bytes : 0), (long long)count * per, count, (long long)per);
    }
    if (count == 0) return FBA_OK;
    // ---- host pass: every header, before anything reaches the device ----
    std::vector<fba_snapshot_head> heads((size_t)count);
    for (int b = 0; b < count; ++b) {
        char msg[256];
        if (fba_snapshot::check_head(in + (size_t)b * (size_t)per, per, acc, msg, sizeof msg))
            return fail(c, FBA_EINVAL, "fba_belief_import: block %d (slot %d): %s", b, first + b, msg);
        std::memcpy(&heads[(size_t)b], in + (size_t)b * (size_t)per, sizeof(fba_snapshot_head));
    }
    if ((rc = snapshot_quiet(c, "fba_belief_import", first, count, -1))) return rc;
    materialize_records(c);   // (the commit writes 64-byte records into the live buffer)
    // ---- device pass: checksum and every record of every block, then (and only then) the commit ----
    const int chunk = snapshot_chunk(per, count);
    const bool one = chunk >= count;   // the whole range is staged at once: it is uploaded once
    ScratchBuf<uint8_t> d_stage;
    ScratchBuf<unsigned long long> d_check;   // [chunk] checksums, then the error word
    HIPCHK(c, d_stage.alloc((size_t)chunk * (size_t)per));
    HIPCHK(c, d_check.alloc((size_t)chunk + 1));
    std::vector<unsigned long long> h_check((size_t)chunk + 1);
    static const char* const what_names[] = {"", "a weight that is negative or not finite", "a state outside the domain", "an illegal parent-set word",
                                             "a history entry outside the domain's tables", "a count that is negative or not finite"};
    for (int pass = 0; pass < 2; ++pass)
        for (int done = 0; done < count; done += chunk) {
            const int n = std::min(chunk, count - done);
            a.first = first + done; a.count = n; a.stage = d_stage.p; a.check = d_check.p; a.bad = d_check.p + chunk;
            if (pass == 0 || !one)
                HIPCHK(c, hipMemcpyAsync(d_stage.p, in + (size_t)done * (size_t)per, (size_t)n * (size_t)per, hipMemcpyHostToDevice, c->stream));
            if (pass == 1) {
                launch_snapshot_commit(P, c->D, a, c->stream);
                HIPCHK(c, hipGetLastError());
                HIPCHK(c, hipStreamSynchronize(c->stream));   // (the staging buffer is reused by the next chunk, the caller's by the caller)
                continue;
            }
            HIPCHK(c, hipMemsetAsync(d_check.p, 0, (size_t)chunk * 8, c->stream));
            HIPCHK(c, hipMemsetAsync(a.bad, 0xff, 8, c->stream));
            launch_snapshot_validate(P, c->D, a, c->stream);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(h_check.data(), d_check.p, ((size_t)chunk + 1) * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (int b = 0; b < n; ++b)
                if (h_check[(size_t)b] != heads[(size_t)(done + b)].checksum)
                    return fail(c, FBA_EINVAL, "fba_belief_import: block %d (slot %d): checksum %016llx in the header, %016llx over the payload", done + b,
                                first + done + b, (unsigned long long)heads[(size_t)(done + b)].checksum, h_check[(size_t)b]);
            const unsigned long long bad = h_check[(size_t)chunk];
            if (bad != ~0ull) {
                const int b = done + (int)(bad >> 40), what = (int)(bad & 0xffu);
                return fail(c, FBA_EINVAL, "fba_belief_import: block %d (slot %d), particle %lld: %s", b, first + b, (long long)((bad >> 8) & 0xffffffffull),
                            what >= 1 && what <= 5 ? what_names[what] : "an invalid record");
            }
        }
    if (P.packed || P.ft_packed) {
        if (c->packed_updates.size() != (size_t)P.E) c->packed_updates.assign((size_t)P.E, 0);
        for (int b = 0; b < count; ++b) c->packed_updates[(size_t)(first + b)] = heads[(size_t)b].updates;
    }
    c->belief_ready = true;
    return FBA_OK;
}

int fba_belief_replicate(fba_ctx* c, int32_t src, int32_t first, int32_t count)
{
    if (!c) return FBA_EINVAL;
    int rc;
    if ((rc = snapshot_range(c, "fba_belief_replicate", first, count))) return rc;
    if (src < 0 || src >= c->P.E) return fail(c, FBA_EINVAL, "fba_belief_replicate: source slot %d is not within the context's %d", src, c->P.E);
    if (count == 0) return FBA_OK;
    if (!c->belief_ready) return fail(c, FBA_ESTATE, "fba_belief_replicate: belief not initiated");
    if ((rc = snapshot_quiet(c, "fba_belief_replicate", first, count, src))) return rc;
    materialize_records(c, true);   // (a lazily reset source: its states are written out, results keep their bits)
    launch_snapshot_replicate(c->P, c->D, src, first, count, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((c->P.packed || c->P.ft_packed) && c->packed_updates.size() == (size_t)c->P.E)
        for (int b = 0; b < count; ++b) c->packed_updates[(size_t)(first + b)] = c->packed_updates[(size_t)src];
    return FBA_OK;
}

// what the kernels of the last fba_belief_convert of this thread took (HIP events around the launches of every chunk); kept outside the
// context, which the call leaves untouched.  fba_debug_convert_kernel_ms: diagnostic, not in include/fba_hip.h (scripts/bench_belief_convert.py)
// fba_debug_convert_validate_ms: the part of it that judged the source blocks (snapshot_validate_kernel)
static thread_local double g_convert_kernel_ms = 0.0, g_convert_validate_ms = 0.0;
extern "C" double fba_debug_convert_kernel_ms(void) { return g_convert_kernel_ms; }
extern "C" double fba_debug_convert_validate_ms(void) { return g_convert_validate_ms; }
namespace {
struct ConvertEvents {
    hipEvent_t a = nullptr, m = nullptr, b = nullptr;
    ~ConvertEvents() { if (a) (void)hipEventDestroy(a); if (m) (void)hipEventDestroy(m); if (b) (void)hipEventDestroy(b); }
};
}  // namespace

int64_t fba_snapshot_block_bytes(const fba_snapshot_head* head)
{
    if (!head) return 0;
    fba_snapshot_head h;
    std::memcpy(&h, head, sizeof h);   // (a header inside a caller's byte buffer may stand anywhere)
    return fba_snapshot::block_bytes(h.weighted, h.particles, h.particle_bytes);
}

int fba_belief_convert(fba_ctx* c, int32_t count, const void* src, int64_t src_bytes, uint64_t seed, uint32_t first_run, void* dst, int64_t dst_cap)
{
    static const char* const call = "fba_belief_convert";
    if (!c) return FBA_EINVAL;
    if (const char* extra = snapshot_extra_state(c))
        return fail(c, FBA_EINVAL, "%s: a snapshot holds the main filter of a slot, and %s", call, extra);
    if (count < 1 || !src || !dst)
        return fail(c, FBA_EINVAL, "%s: count %d, src %s, dst %s: one block at least, from a buffer into a buffer", call, count, src ? "set" : "null", dst ? "set" : "null");
    const Problem& P = c->P;
    const uint8_t* in = static_cast<const uint8_t*>(src);
    uint8_t* out      = static_cast<uint8_t*>(dst);
    const fba_snapshot::Accepts acc = snapshot_accepts(c);
    const int weighted = snapshot_weighted(c) ? 1 : 0;
    const int64_t dper = fba_snapshot::block_bytes(weighted, P.N, (int64_t)P.Cs * 4);
    // ---- host pass: the first header says what the blocks of the call are, then every header against it and the context ----
    if (src_bytes < (int64_t)sizeof(fba_snapshot_head))
        return fail(c, FBA_EINVAL, "%s: bytes %lld: not even one header of %d", call, (long long)src_bytes, (int)sizeof(fba_snapshot_head));
    fba_snapshot_head h0;
    std::memcpy(&h0, in, sizeof h0);
    char msg[256];
    {
        const int rc = fba_snapshot::check_convert_head(in, std::max<int64_t>(src_bytes, 0), acc, h0.particles, h0.particle_bytes, msg, sizeof msg);
        // (a first block cut short: the size of the whole buffer is the better message, below)
        if (rc && std::strncmp(msg, "bytes ", 6) != 0) return fail(c, FBA_EINVAL, rc == -2 ? "%s: block 0 %s" : "%s: block 0: %s", call, msg);
    }
    const int32_t n_src = h0.particles, src_cs = h0.particle_bytes / 4;
    const int64_t sper = fba_snapshot::block_bytes(weighted, n_src, h0.particle_bytes);
    if (src_bytes != (int64_t)count * sper)
        return fail(c, FBA_EINVAL, "%s: bytes %lld / %lld (%d blocks of %lld)", call, (long long)src_bytes, (long long)count * sper, count, (long long)sper);
    if (dst_cap < (int64_t)count * dper)
        return fail(c, FBA_EINVAL, "%s: %d blocks of %lld bytes need %lld, the buffer has %lld", call, count, (long long)dper, (long long)count * dper, (long long)dst_cap);
    if (in < out + dst_cap && out < in + src_bytes) return fail(c, FBA_EINVAL, "%s: src and dst overlap", call);
    std::vector<fba_snapshot_head> heads((size_t)count);
    std::vector<int64_t> strides((size_t)count);
    for (int b = 0; b < count; ++b) {
        const int rc = fba_snapshot::check_convert_head(in + (size_t)b * (size_t)sper, sper, acc, n_src, h0.particle_bytes, msg, sizeof msg, &strides[(size_t)b]);
        if (rc) return fail(c, FBA_EINVAL, rc == -2 ? "%s: block %d %s" : "%s: block %d: %s", call, b, msg);
        std::memcpy(&heads[(size_t)b], in + (size_t)b * (size_t)sper, sizeof(fba_snapshot_head));
    }
    const int mode = n_src == P.N ? CONVERT_SAME : (weighted ? CONVERT_WEIGHTED : CONVERT_FLAT);
    if (mode == CONVERT_WEIGHTED && n_src > 256 * IS_MAX_CHUNKS)
        return fail(c, FBA_EINVAL, "%s: %d weighted particles in a block / %d a weighted filter of this engine holds", call, n_src, 256 * IS_MAX_CHUNKS);
    // ---- the kernels' arguments: the validation sees a Problem shaped like the source ----
    BeliefSnapshotArgs va;
    ScratchBuf<uint32_t> d_limit;
    int rc;
    if ((rc = snapshot_args(c, va, d_limit))) return rc;
    Problem S = P;
    S.N = n_src; S.Cs = src_cs;
    if (P.hist) S.hist_cap = src_cs - 2;
    const int64_t spad = snapshot_store_pad(weighted, n_src), spitch = snapshot_store_pitch(sper, weighted, n_src);
    const int64_t dpad = snapshot_store_pad(weighted, P.N), dpitch = snapshot_store_pitch(dper, weighted, P.N);
    const int chunk = snapshot_chunk(spitch + dpitch, count);   // both sides of a chunk within the staging bound, one block of each at least
    ScratchBuf<uint8_t> d_src, d_dst;
    ScratchBuf<double> d_incl;
    ScratchBuf<unsigned long long> d_check;   // [chunk] source checksums, [chunk] destination checksums, then the error word
    const size_t want[3] = {(size_t)chunk * (size_t)spitch, (size_t)chunk * (size_t)dpitch, mode == CONVERT_WEIGHTED ? (size_t)chunk * (size_t)n_src * 8 : 0};
    if (d_src.alloc(want[0]) != hipSuccess || d_dst.alloc(want[1]) != hipSuccess || (want[2] && d_incl.alloc(want[2] / 8) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(c, FBA_EHIP, "%s: no device memory for staging: %lld bytes (%d blocks: %lld of the source, %lld of the destination, %lld of prefix sums)", call,
                    (long long)(want[0] + want[1] + want[2]), chunk, (long long)want[0], (long long)want[1], (long long)want[2]);
    }
    HIPCHK(c, d_check.alloc((size_t)2 * chunk + 1));
    std::vector<unsigned long long> h_check((size_t)2 * chunk + 1);
    ConvertEvents ev;
    HIPCHK(c, hipEventCreate(&ev.a));
    HIPCHK(c, hipEventCreate(&ev.m));
    HIPCHK(c, hipEventCreate(&ev.b));
    g_convert_kernel_ms = g_convert_validate_ms = 0.0;
    static const char* const what_names[] = {"", "a weight that is negative or not finite", "a state outside the domain", "an illegal parent-set word",
                                             "a history entry outside the domain's tables", "a count that is negative or not finite", "",
                                             "weights whose total is zero or not finite: nothing to sample from"};
    BeliefConvertArgs a{};
    a.first_run = first_run; a.src_pitch = spitch; a.dst_pitch = dpitch; a.n_src = n_src; a.src_cs = src_cs; a.weighted = weighted; a.mode = mode;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    for (int done = 0; done < count; done += chunk) {
        const int n = std::min(chunk, count - done);
        va.first = 0; va.count = n; va.stage = d_src.p + (size_t)spad; va.per_slot = spitch; va.check = d_check.p; va.bad = d_check.p + 2 * chunk;
        a.count = n; a.first_run = first_run + (uint32_t)done; a.src = va.stage; a.dst = d_dst.p + (size_t)dpad; a.incl = d_incl.p;
        a.check = d_check.p + chunk; a.bad = va.bad;
        HIPCHK(c, hipMemcpy2DAsync(va.stage, (size_t)spitch, in + (size_t)done * (size_t)sper, (size_t)sper, (size_t)sper, (size_t)n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(d_check.p, 0, (size_t)2 * chunk * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(va.bad, 0xff, 8, c->stream));
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        launch_snapshot_validate(S, c->D, va, c->stream);
        HIPCHK(c, hipEventRecord(ev.m, c->stream));
        if (mode == CONVERT_WEIGHTED) launch_convert_scan(a, c->stream);
        launch_snapshot_convert(P, a, c->stream);   // (in bounds whatever the payload holds: the headers are the host's, a source index is below n_src by construction)
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h_check.data(), d_check.p, ((size_t)2 * chunk + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) g_convert_kernel_ms += (double)ms;
            if (hipEventElapsedTime(&ms, ev.a, ev.m) == hipSuccess) g_convert_validate_ms += (double)ms;
        }
        for (int b = 0; b < n; ++b)
            if (h_check[(size_t)b] != heads[(size_t)(done + b)].checksum)
                return fail(c, FBA_EINVAL, "%s: block %d: checksum %016llx in the header, %016llx over the payload", call, done + b,
                            (unsigned long long)heads[(size_t)(done + b)].checksum, h_check[(size_t)b]);
        const unsigned long long bad = h_check[(size_t)2 * chunk];
        if (bad != ~0ull) {
            const int b = done + (int)(bad >> 40), what = (int)(bad & 0xffu);
            if (what == SNAP_BAD_TOTAL) return fail(c, FBA_EINVAL, "%s: block %d: %s", call, b, what_names[what]);
            return fail(c, FBA_EINVAL, "%s: block %d, particle %lld: %s", call, b, (long long)((bad >> 8) & 0xffffffffull),
                        what >= 1 && what <= 5 ? what_names[what] : "an invalid record");
        }
        HIPCHK(c, hipMemcpy2D(out + (size_t)done * (size_t)dper, (size_t)dper, a.dst, (size_t)dpitch, (size_t)dper, (size_t)n, hipMemcpyDeviceToHost));
        for (int b = 0; b < n; ++b) {
            const fba_snapshot_head& s = heads[(size_t)(done + b)];
            fba_snapshot_head h = acc.want;
            h.hist_cnt = s.hist_cnt; h.updates = s.updates;
            h.stride   = (uint32_t)strides[(size_t)(done + b)];
            h.checksum = h_check[(size_t)chunk + (size_t)b];
            std::memcpy(out + (size_t)(done + b) * (size_t)dper, &h, sizeof h);
        }
    }
    return FBA_OK;
}

int fba_last_step_info(fba_ctx* c, fba_trace_rec* recs)
{
    if (!c || !recs) return FBA_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(recs, c->D.cur, (size_t)c->P.E * sizeof(fba_trace_rec), hipMemcpyDeviceToHost));
    return FBA_OK;
}

int fba_run_planning(fba_ctx* c, fba_stat* stats)
{
    if (!c || !stats) return FBA_EINVAL;
    if (c->P.model != FBA_MODEL_POMDP) return fail(c, FBA_EINVAL, "planning::run needs model = POMDP");
    return run_experiment(c, stats);
}

int fba_run_bapomdp(fba_ctx* c, fba_stat* stats)
{
    if (!c || !stats) return FBA_EINVAL;
    if (c->P.model == FBA_MODEL_POMDP) return fail(c, FBA_EINVAL, "bapomdp::run needs a Bayes-adaptive model");
    return run_experiment(c, stats);
}

namespace {
// the device-resident blocks of a resumed span: the context's DeviceState points into them while the call runs, and on no way out beyond it
struct SpanStore {
    fba_ctx* c;
    uint8_t* p = nullptr;
    explicit SpanStore(fba_ctx* ctx) : c(ctx) {}
    ~SpanStore()
    {
        c->D.restore_store = nullptr; c->D.restore_pitch = 0; c->D.restore_nblocks = 0;
        if (p) { (void)hipStreamSynchronize(c->stream); (void)hipFree(p); }
    }
};
}  // namespace

int fba_run_bapomdp_span(fba_ctx* c, int32_t first, int32_t stop, const void* blocks, int32_t nblocks, int64_t bytes, fba_stat* stats)
{
    static const char* const call = "fba_run_bapomdp_span";
    if (!c || !stats) return FBA_EINVAL;
    if (c->P.model == FBA_MODEL_POMDP) return fail(c, FBA_EINVAL, "%s: bapomdp::run needs a Bayes-adaptive model", call);
    if (const char* extra = snapshot_extra_state(c))
        return fail(c, FBA_EINVAL, "%s: a span is continued from snapshots, a snapshot holds the main filter of a slot, and %s", call, extra);
    const Problem& P = c->P;
    if (first < 0 || stop <= first || stop > P.episodes)
        return fail(c, FBA_EINVAL, "%s: episodes [%d, %d) are not a span within the context's %d", call, first, stop, P.episodes);
    if (!blocks) {
        if (first != 0 || nblocks != 0)
            return fail(c, FBA_EINVAL, "%s: without blocks a run starts from the prior, at episode 0 (first_episode %d, nblocks %d)", call, first, nblocks);
        return run_experiment(c, stats, 0, stop);
    }
    if (nblocks != 1 && nblocks != c->cfg.runs)
        return fail(c, FBA_EINVAL, "%s: nblocks %d: one block for every run (1) or one per run (%d)", call, nblocks, c->cfg.runs);
    int rc;
    BeliefSnapshotArgs a;
    ScratchBuf<uint32_t> d_limit;
    if ((rc = snapshot_args(c, a, d_limit))) return rc;
    const int64_t per = a.per_slot;
    const uint8_t* in = static_cast<const uint8_t*>(blocks);
    const fba_snapshot::Accepts acc = snapshot_accepts(c);
    if (bytes != (int64_t)nblocks * per) {
        char msg[256];
        if (bytes >= (int64_t)sizeof(fba_snapshot_head) && fba_snapshot::check_head(in, per, acc, msg, sizeof msg))
            return fail(c, FBA_EINVAL, "%s: block 0: %s", call, msg);
        return fail(c, FBA_EINVAL, "%s: bytes %lld / %lld (%d blocks of %lld)", call, (long long)bytes, (long long)nblocks * per, nblocks, (long long)per);
    }
    // ---- host pass: every header, and the room the span needs in every block ----
    std::vector<fba_snapshot_head> heads((size_t)nblocks);
    for (int b = 0; b < nblocks; ++b) {
        char msg[320];
        if (fba_snapshot::check_head(in + (size_t)b * (size_t)per, per, acc, msg, sizeof msg)) return fail(c, FBA_EINVAL, "%s: block %d: %s", call, b, msg);
        if (fba_snapshot::check_span_room(in + (size_t)b * (size_t)per, b, first, stop, P.episodes, P.horizon, msg, sizeof msg))
            return fail(c, FBA_EINVAL, "%s: %s", call, msg);
        std::memcpy(&heads[(size_t)b], in + (size_t)b * (size_t)per, sizeof(fba_snapshot_head));
    }
    // ---- the store, and the device pass over it a chunk at a time: checksum and every record of every block ----
    const int64_t pad = snapshot_store_pad(a.weighted, P.N), pitch = snapshot_store_pitch(per, a.weighted, P.N);
    SpanStore store(c);
    if (hipMalloc(reinterpret_cast<void**>(&store.p), (size_t)nblocks * (size_t)pitch) != hipSuccess) {
        (void)hipGetLastError();
        store.p = nullptr;
        return fail(c, FBA_EHIP, "%s: no device memory for a store of %lld bytes (%d blocks of %lld)", call, (long long)nblocks * (long long)pitch, nblocks,
                    (long long)pitch);
    }
    const int chunk = snapshot_chunk(per, nblocks);
    ScratchBuf<unsigned long long> d_check;   // [chunk] checksums, then the error word
    HIPCHK(c, d_check.alloc((size_t)chunk + 1));
    std::vector<unsigned long long> h_check((size_t)chunk + 1);
    const int inc_words = P.packed ? P.C : (P.ft_packed ? c->fdesc.ncounts / 2 : 0);   // the words of a packed record that hold two uint16 increments
    for (int done = 0; done < nblocks; done += chunk) {
        const int n = std::min(chunk, nblocks - done);
        a.first = 0; a.count = n; a.stage = store.p + (size_t)done * (size_t)pitch + (size_t)pad; a.per_slot = pitch;
        a.check = d_check.p; a.bad = d_check.p + chunk;
        HIPCHK(c, hipMemcpy2DAsync(a.stage, (size_t)pitch, in + (size_t)done * (size_t)per, (size_t)per, (size_t)per, (size_t)n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(d_check.p, 0, (size_t)chunk * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(a.bad, 0xff, 8, c->stream));
        launch_snapshot_validate(P, c->D, a, c->stream);
        launch_span_increments(P, a, inc_words, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h_check.data(), d_check.p, ((size_t)chunk + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int b = 0; b < n; ++b)
            if (h_check[(size_t)b] != heads[(size_t)(done + b)].checksum)
                return fail(c, FBA_EINVAL, "%s: block %d: checksum %016llx in the header, %016llx over the payload", call, done + b,
                            (unsigned long long)heads[(size_t)(done + b)].checksum, h_check[(size_t)b]);
        const unsigned long long bad = h_check[(size_t)chunk];
        if (bad != ~0ull) {
            static const char* const what_names[] = {"", "a weight that is negative or not finite", "a state outside the domain", "an illegal parent-set word",
                                                     "a history entry outside the domain's tables", "a count that is negative or not finite",
                                                     "an increment beyond the updates its header counts"};
            const int b = done + (int)(bad >> 40), what = (int)(bad & 0xffu);
            return fail(c, FBA_EINVAL, "%s: block %d, particle %lld: %s", call, b, (long long)((bad >> 8) & 0xffffffffull),
                        what >= 1 && what <= 6 ? what_names[what] : "an invalid record");
        }
    }
    // ---- every block is one this context can run from: the experiment, with the store in Belief::initiate's place ----
    c->D.restore_store = store.p; c->D.restore_pitch = pitch; c->D.restore_nblocks = nblocks;
    std::vector<uint32_t> updates((size_t)nblocks);
    for (int b = 0; b < nblocks; ++b) updates[(size_t)b] = heads[(size_t)b].updates;
    if ((rc = run_experiment(c, stats, first, stop, &updates))) return rc;
    for (int r = 0; r < c->cfg.runs; ++r) {   // every run has taken its block once
        c->restored_particles += (uint64_t)P.N;
        c->restored_bytes += 2 * (uint64_t)P.N * ((uint64_t)heads[(size_t)(r % nblocks)].stride + (a.weighted ? 8u : 0u));
    }
    return FBA_OK;
}

int fba_run_ticks(fba_ctx* c, int32_t ticks)
{
    if (!c || ticks < 0) return FBA_EINVAL;
    int rc;
    if (!c->started) {
        if (c->cfg.trace)   // room for one run's worth of records per slot (later ones are counted, not kept)
            if ((rc = ensure_trace(c, (size_t)c->P.E * c->P.episodes * c->P.horizon))) return rc;
        if ((rc = start_experiment(c, -1))) return rc;
        c->started = true;
    }
    if (c->P.search_budget > 0) {
        // slots advance on their own: "ticks" real steps per slot on average = launches until the slots have together made
        // ticks x slots of them (a launch = one budget of search iterations + the step and belief update of the slots that finished)
        int rc2 = FBA_OK;
        const uint64_t base   = sum_counter(c, c->D.env_steps, c->P.E, &rc2);
        const uint64_t target = (uint64_t)ticks * (uint64_t)c->P.E;
        // (a simulation takes at most horizon + 1 loop iterations: the last one finishes it when depth-to-go is 0)
        const long long bound = ((long long)ticks + 2) * (((long long)c->P.sims * (c->P.horizon + 1)) / c->P.search_budget + 2);
        uint64_t made = 0;
        for (long long k = 0; k < bound && !rc2; ++k) {
            made = sum_counter(c, c->D.env_steps, c->P.E, &rc2) - base;   // (synchronises: the launches of the last round are done)
            if (made >= target) break;
            if ((rc = tick(c))) return rc;
        }
        if (rc2) return rc2;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if ((rc = check_fault(c))) return rc;
        if (made < target) {
            made = sum_counter(c, c->D.env_steps, c->P.E, &rc2) - base;
            if (rc2) return rc2;
            if (made < target)
                return fail(c, FBA_ESTATE, "budgeted run_ticks: %llu of %llu real steps made after %lld launches", (unsigned long long)made,
                            (unsigned long long)target, bound);
        }
        return FBA_OK;
    }
    for (int k = 0; k < ticks; ++k)
        if ((rc = tick(c))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return check_fault(c);
}

int fba_get_returns(const fba_ctx* cc, double* returns, int32_t* lengths)
{
    fba_ctx* c = const_cast<fba_ctx*>(cc);
    if (!c) return FBA_EINVAL;
    const size_t n = (size_t)c->cfg.runs * c->P.episodes;
    if (n > c->returns_cap) return fail(c, FBA_ESTATE, "no experiment has been run on this ctx");
    if (returns) HIPCHK(c, hipMemcpy(returns, c->D.returns, n * sizeof(double), hipMemcpyDeviceToHost));
    if (lengths) HIPCHK(c, hipMemcpy(lengths, c->D.lengths, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return FBA_OK;
}

int fba_get_return_sums(fba_ctx* c, double* out)
{
    if (!c || !out) return FBA_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<double> h((size_t)3 * c->P.E);
    HIPCHK(c, hipMemcpy(h.data(), c->D.ep_sums, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    out[0] = out[1] = out[2] = 0;
    for (int e = 0; e < c->P.E; ++e)
        for (int k = 0; k < 3; ++k) out[k] += h[(size_t)3 * e + k];
    return FBA_OK;
}

int fba_get_counters(fba_ctx* c, fba_counters* out)
{
    if (!c || !out) return FBA_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc = FBA_OK;
    out->sim_steps    = sum_counter(c, c->D.sim_steps, c->P.E, &rc);
    out->belief_steps = sum_counter(c, c->D.belief_steps, c->P.E, &rc);
    out->env_steps    = sum_counter(c, c->D.env_steps, c->P.E, &rc);
    return rc;
}

int fba_get_kernel_times(fba_ctx* c, fba_kernel_time* out)
{
    if (!c || !out) return FBA_EINVAL;
    int rc = flush_events(c);
    if (rc) return rc;
    const Problem& P = c->P;
    const uint32_t update    = update_plan(P, c->D).filter;   // the kernel that ran picks each alternative byte formula below
    const uint64_t sim       = sum_counter(c, c->D.sim_steps, P.E, &rc) - c->base_sim;
    const uint64_t attempts  = sum_counter(c, c->D.upd_attempts, P.E, &rc) - c->base_attempts;
    const uint64_t particles = sum_counter(c, c->D.upd_particles, P.E, &rc) - c->base_particles;
    const uint64_t entries   = sum_counter(c, c->D.upd_entries, P.E, &rc) - c->base_entries;
    const uint64_t compact_full = sum_counter(c, c->D.upd_compact_full, P.E, &rc) - c->base_compact_full;
    const uint64_t compact      = sum_counter(c, c->D.upd_compact, P.E, &rc) - c->base_compact;
    if (rc) return rc;
    // algorithmic bytes, SURVEY.md section 8(d): Pb = particle payload, Rt / Ro = bytes of the
    // transition / observation rows one step consults
    // (SURVEY's dense figure, 4 bytes per count, unless one of the packed / history formulas below applies: DESIGN.md section 5)
    const uint64_t cell = 4;
    const uint64_t Pb = 4 + cell * (uint64_t)c->dense_C;
    uint64_t Rt = 0, Ro = 0;
    if (P.model == FBA_MODEL_BA_TABLE) { Rt = cell * (uint64_t)P.S; Ro = cell * (uint64_t)P.O; }
    if (P.model == FBA_MODEL_BA_FACTORED) {
        for (int f = 0; f < c->fdesc.FS; ++f) Rt += 4 * (uint64_t)c->fdesc.Ssz[f];
        for (int f = 0; f < c->fdesc.FO; ++f) Ro += 4 * (uint64_t)c->fdesc.Osz[f];
    }
    for (int k = 0; k < FBA_K_COUNT; ++k) {
        out[k].ms = c->k_ms[k];
        out[k].launches = c->k_launches[k];
        out[k].units = 0;
        out[k].bytes = 0;
    }
    out[FBA_K_SEARCH].units = sim;
    // restore_kernel (resumed spans): a particle's record at the block's stride and its weight, read from the store and written to the slot
    out[FBA_K_BELIEF_INIT].units = c->restored_particles;
    out[FBA_K_BELIEF_INIT].bytes = c->restored_bytes;
    if (P.belief == FBA_BELIEF_REJECTION) {
        out[FBA_K_BELIEF_RS].units = particles;
        out[FBA_K_BELIEF_RS].bytes = attempts * (Pb + Rt + Ro) + particles * Pb;
        // reject_tiger_lds_kernel (packed particles, N <= TIGER_LDS_MAX_N): the alternative formula SURVEY 8(d) asks to be
        // stated when the build does not move dense particles -- the attempts run from LDS, so an update reads the
        // filter once to park it, reads the N accepted sources and writes N records, 64 bytes each
        // ... and where the experiment loop keeps compact filters (fba_state.h), what those launches moved: a particle written compact
        // was read as 64 or as 16 bytes and written as 16 -- 80 or 32 bytes
        if (tiger_filter_in_lds(update))
            out[FBA_K_BELIEF_RS].bytes = (particles - compact_full - compact) * 3 * (uint64_t)(P.Cs * 4) + compact_full * 80 + compact * 32;
        // packed factored-tiger records (reject_kernel on 144-byte records at --size 3): SURVEY's formula on the bytes a packed particle has --
        // an attempt reads its source record and one 4-byte word per two-cell Dirichlet row it samples, an accepted one writes a record
        if (reads_packed_ftiger(update)) {
            const uint64_t rec = (uint64_t)P.Cs * 4, rows = 4 * (uint64_t)(c->fdesc.FS + c->fdesc.FO);
            out[FBA_K_BELIEF_RS].bytes = attempts * (rec + rows) + particles * rec;
        }
        // history particles (reject_hist_kernel): an attempt reads its source's two header words (8) and the entries
        // of the real action, an accepted one is gathered -- its source record read (8 + 4 per entry) and written with the new entry
        // (8 + 4 per entry + 4); `entries` counts the 4-byte entries of both (fba_state.h upd_entries); the Dirichlet rows come from LDS
        // (tabular records, reject_tab_hist_kernel: the same formula; their sparse prior rows are L2-resident, 380 KB at N = 7, and not counted)
        if (updates_history_records(update)) out[FBA_K_BELIEF_RS].bytes = attempts * 8 + particles * 20 + entries * 4;
    } else {
        out[FBA_K_BELIEF_IS].units = particles;
        out[FBA_K_BELIEF_IS].bytes = particles * (32 + Rt + Ro) + particles * (8 + 2 * Pb);
        // history particles (alternative formula, stated in DESIGN.md section 5 before it was measured): per particle the
        // weight read and written (16), the record -- 8 bytes + 4 per entry -- read once by the update, once as a
        // resample source, written once with its new entry (+4); the Dirichlet rows come from the shared tables
        // (tabular records, is_multi_tab_step_kernel: the same formula; their sparse prior rows are L2-resident and not counted)
        if (updates_history_records(update)) out[FBA_K_BELIEF_IS].bytes = particles * 44 + entries * 12;
        // collision-avoidance records (is_multi_ca_step_kernel and the launches behind it, at every filter size): per particle the weight read
        // and written by the step (16), read by the normalisation (8), read again and its prefix sum written by the scan (16), one prefix sum
        // read per draw at least and the new weight written (16), the side row {state, entry} written and read (16) = 72; the record -- 8
        // bytes + 4 per entry -- read by the step, read as a resample source, written with its new entry (3 * 8 + 4 = 28 + 12 per entry).
        // The prior and its sequence table sit in LDS and are not counted.
        if (kernel_name(update) == K_IS_MULTI_CA_STEP) out[FBA_K_BELIEF_IS].bytes = particles * 100 + entries * 12;
        // packed tiger particles (64-byte records): the same formula on the bytes a packed particle has -- the update reads
        // state + weight + its two rows and writes state + weight + two counts (32 + Rt + Ro = 48), the resample reads the
        // weight and moves a record in and out (8 + 2 * 64)
        if (reads_packed_tiger(update)) out[FBA_K_BELIEF_IS].bytes = particles * (32 + Rt + Ro) + particles * (8 + 2 * (uint64_t)(P.Cs * 4));
    }
    return FBA_OK;
}

// diagnostic (scripts/tick_probe.py; not part of include/fba_hip.h): every slot's simulated-step counter and time-step
int fba_debug_slot_counters(fba_ctx* c, unsigned long long* sim_steps, int32_t* t)
{
    if (!c) return FBA_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sim_steps) HIPCHK(c, hipMemcpy(sim_steps, c->D.sim_steps, (size_t)c->P.E * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (t) HIPCHK(c, hipMemcpy(t, c->D.t, (size_t)c->P.E * sizeof(int32_t), hipMemcpyDeviceToHost));
    return FBA_OK;
}

// diagnostic (tests; not part of include/fba_hip.h): the slots whose filter is compact right now (fba_state.h)
int fba_debug_compact_slots(fba_ctx* c, int32_t* n)
{
    if (!c || !n) return FBA_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<uint8_t> h((size_t)c->P.E);
    HIPCHK(c, hipMemcpy(h.data(), c->D.compact, h.size(), hipMemcpyDeviceToHost));
    *n = 0;
    for (uint8_t v : h) *n += v != 0;
    return FBA_OK;
}

// diagnostic, not in include/fba_hip.h: the kernels launch_belief_update launches for this context, in order, as update_plan
// (fba_launch_plan.h) names them -- what a test asks that wants to know which kernel its case runs.  Returns the number of steps
int fba_debug_update_plan(fba_ctx* c, uint32_t* keys, int32_t cap)
{
    if (!c || (!keys && cap > 0)) return FBA_EINVAL;
    const LaunchPlan pl = update_plan(c->P, c->D);
    for (int i = 0; i < pl.n && i < cap; ++i) keys[i] = pl.step[i].kernel;
    return pl.n;
}

int fba_reset_kernel_times(fba_ctx* c)
{
    if (!c) return FBA_EINVAL;
    int rc = flush_events(c);
    if (rc) return rc;
    for (int k = 0; k < FBA_K_COUNT; ++k) { c->k_ms[k] = 0; c->k_launches[k] = 0; }
    c->restored_particles = c->restored_bytes = 0;
    c->base_sim       = sum_counter(c, c->D.sim_steps, c->P.E, &rc);
    c->base_attempts  = sum_counter(c, c->D.upd_attempts, c->P.E, &rc);
    c->base_particles = sum_counter(c, c->D.upd_particles, c->P.E, &rc);
    c->base_entries   = sum_counter(c, c->D.upd_entries, c->P.E, &rc);
    c->base_compact_full = sum_counter(c, c->D.upd_compact_full, c->P.E, &rc);
    c->base_compact      = sum_counter(c, c->D.upd_compact, c->P.E, &rc);
    return rc;
}

int fba_trace_count(const fba_ctx* cc)
{
    fba_ctx* c = const_cast<fba_ctx*>(cc);
    if (!c) return FBA_EINVAL;
    int32_t n = 0;
    if (hipMemcpy(&n, c->D.trace_count, sizeof n, hipMemcpyDeviceToHost) != hipSuccess) return FBA_EHIP;
    return std::min(n, c->D.trace_cap);
}

int fba_get_trace(const fba_ctx* cc, fba_trace_rec* out, int32_t cap)
{
    fba_ctx* c = const_cast<fba_ctx*>(cc);
    if (!c || !out) return FBA_EINVAL;
    const int n = std::min(fba_trace_count(c), cap);
    if (n <= 0) return n;
    HIPCHK(c, hipMemcpy(out, c->D.trace, (size_t)n * sizeof(fba_trace_rec), hipMemcpyDeviceToHost));
    // slots finish their ticks in arbitrary order: present the records as the reference would
    // print them, by (run, episode, t)
    std::sort(out, out + n, [](const fba_trace_rec& a, const fba_trace_rec& b) {
        if (a.run != b.run) return a.run < b.run;
        if (a.episode != b.episode) return a.episode < b.episode;
        return a.t < b.t;
    });
    return n;
}

int fba_get_trace_hist(const fba_ctx* cc, uint32_t* out, int32_t cap)
{
    fba_ctx* c = const_cast<fba_ctx*>(cc);
    if (!c || !out) return FBA_EINVAL;
    if (!c->D.trace_hist) return fail(c, FBA_EINVAL, "no histograms were recorded: create the context with trace = 2 (domains of at most %d states)", FBA_TRACE_HIST_BINS);
    const int n = std::min(fba_trace_count(c), cap);
    if (n <= 0) return n;
    std::vector<fba_trace_rec> tr((size_t)n);
    std::vector<uint32_t> h((size_t)n * FBA_TRACE_HIST_BINS);
    HIPCHK(c, hipMemcpy(tr.data(), c->D.trace, (size_t)n * sizeof(fba_trace_rec), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(h.data(), c->D.trace_hist, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) {   // the order of fba_get_trace
        if (tr[a].run != tr[b].run) return tr[a].run < tr[b].run;
        if (tr[a].episode != tr[b].episode) return tr[a].episode < tr[b].episode;
        return tr[a].t < tr[b].t;
    });
    for (int i = 0; i < n; ++i)
        std::copy(h.begin() + (size_t)order[(size_t)i] * FBA_TRACE_HIST_BINS, h.begin() + (size_t)(order[(size_t)i] + 1) * FBA_TRACE_HIST_BINS,
                  out + (size_t)i * FBA_TRACE_HIST_BINS);
    return n;
}

int fba_selftest_ucb(fba_ctx* c, const double* L, const int32_t* n, int32_t count, double u, double* out)
{
    if (!c || !L || !n || !out || count <= 0) return FBA_EINVAL;
    ScratchBuf<double> dL, dout;
    ScratchBuf<int32_t> dn;
    HIPCHK(c, dL.alloc((size_t)count));
    HIPCHK(c, dout.alloc((size_t)count));
    HIPCHK(c, dn.alloc((size_t)count));
    HIPCHK(c, hipMemcpy(dL.p, L, (size_t)count * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dn.p, n, (size_t)count * 4, hipMemcpyHostToDevice));
    launch_selftest_ucb(dL.p, dn.p, count, u, dout.p, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, dout.p, (size_t)count * 8, hipMemcpyDeviceToHost));
    return FBA_OK;
}

int fba_selftest_lgamma(fba_ctx* c, const double* x, int32_t count, double* out)
{
    if (!c || !x || !out || count <= 0) return FBA_EINVAL;
    ScratchBuf<double> dx, dout;
    HIPCHK(c, dx.alloc((size_t)count));
    HIPCHK(c, dout.alloc((size_t)count));
    HIPCHK(c, hipMemcpy(dx.p, x, (size_t)count * 8, hipMemcpyHostToDevice));
    launch_selftest_lgamma(dx.p, count, dout.p, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, dout.p, (size_t)count * 8, hipMemcpyDeviceToHost));
    return FBA_OK;
}

int fba_log_bd_score(fba_ctx* c, const float* counts, const float* prior, double* out)
{
    if (!c || !counts || !prior || !out) return FBA_EINVAL;
    if (c->P.model != FBA_MODEL_BA_FACTORED) return fail(c, FBA_EINVAL, "fba_log_bd_score: not a factored model");
    ScratchBuf<float> dc, dp;
    ScratchBuf<double> dout;
    const size_t n = (size_t)c->dense_C;
    HIPCHK(c, dc.alloc(n));
    HIPCHK(c, dp.alloc(n));
    HIPCHK(c, dout.alloc(1));
    HIPCHK(c, hipMemcpy(dc.p, counts, n * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dp.p, prior, n * 4, hipMemcpyHostToDevice));
    launch_selftest_bd(c->P, dc.p, dp.p, dout.p, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, dout.p, 8, hipMemcpyDeviceToHost));
    return FBA_OK;
}

// utils::Statistic (reference src/utils/Statistic.cpp:5-46)
void fba_stat_add(fba_stat* s, double v)
{
    s->count += 1;
    const double delta = v - s->mean;
    s->mean += delta / s->count;
    const double delta2 = v - s->mean;
    s->m2 += delta * delta2;
}
double fba_stat_var(const fba_stat* s) { return s->count < 2 ? 0 : s->m2 / (s->count - 1); }
double fba_stat_stder(const fba_stat* s) { return s->count < 2 ? 0 : std::sqrt(fba_stat_var(s) / s->count); }

}  // extern "C"
