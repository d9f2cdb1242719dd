// launch_capture.cpp -- what the tick launchers would launch, recorded on a machine without a GPU (tests/test_launch_plan_cpu.py).
//
// hipLaunchKernelGGL and hipFuncSetAttribute are redefined to write down their arguments, then the launchers' own translation units are
// included and the real launch_search / launch_belief_update / launch_reset are called on hand-filled Problem / DeviceState values.  No
// kernel runs and no pointer is dereferenced on the host; the HIP calls that remain (hipGetDevice, hipMemsetAsync) fail and are ignored
// by the launchers as they always were.
//
// stdin: one case per line, "name launchers field=value ...": launchers is a string of s (search), u (belief update), r (reset); a field is
// one of FIELDS below, P.x or D.x; a pointer field takes 0 (null) or 1 (set).  Unnamed fields are zero, but S = E = 1.
// stdout: one JSON line per case, {"name": ..., "s": [call...], ...}; a call is
//     ["L", kernel, gx, gy, gz, bx, by, bz, dynamic LDS bytes]                 a launch
//     ["A", the function is the one launched next (1 / 0), attribute, value]    hipFuncSetAttribute
// `kernel` is the instantiation as the compiler names it, every template argument filled in, so how a launch line spells it does not matter.
// Every case runs in a child process of its own: the launchers raise a kernel's LDS limit once per process and device, and a case's record
// must not depend on the cases in front of it.
#include <hip/hip_runtime.h>

#include <cxxabi.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <typeinfo>

namespace capture {
static std::string out;
static const void* attr_fn = nullptr;
template <auto K>
struct Tag {};
// the instantiation behind a kernel's name, from the mangled name of Tag<&kernel> (which spells every template argument out)
template <auto K>
static std::string kernel_name()
{
    int status = 0;
    char* d = abi::__cxa_demangle(typeid(Tag<K>).name(), nullptr, nullptr, &status);
    std::string f = status == 0 && d ? d : typeid(Tag<K>).name();
    free(d);
    size_t a = f.find("fba::"), b = a, depth = 0;
    if (a == std::string::npos) return f;
    for (; b < f.size(); ++b) {   // up to the parameter list, or to the end of Tag's argument
        if (f[b] == '<') ++depth;
        else if ((f[b] == '(' || f[b] == '>') && depth == 0) break;
        else if (f[b] == '>') --depth;
    }
    f = f.substr(a + 5, b - a - 5);
    const size_t stub = f.find("__device_stub__");
    if (stub != std::string::npos) f.erase(stub, 15);
    return f;
}
static void launch(const std::string& name, const void* fn, dim3 g, dim3 b, size_t lds)
{
    // (an attribute call that was recorded in front of this launch: was it for this kernel?)
    const size_t mark = out.rfind("\"A\", ?");
    if (mark != std::string::npos) out[mark + 5] = attr_fn == fn ? '1' : '0';
    char buf[160];
    snprintf(buf, sizeof buf, "\", %u, %u, %u, %u, %u, %u, %zu], ", g.x, g.y, g.z, b.x, b.y, b.z, lds);
    out += "[\"L\", \"" + name + buf;
}
static void attribute(const void* fn, int attr, int value)
{
    attr_fn = fn;
    out += "[\"A\", ?, " + std::to_string(attr) + ", " + std::to_string(value) + "], ";
}
}  // namespace capture

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, lds, st, ...) capture::launch(capture::kernel_name<k>(), reinterpret_cast<const void*>(k), g, b, lds)
#define hipFuncSetAttribute(f, a, v) (capture::attribute(f, (int)(a), (int)(v)), hipSuccess)

#include "fba_kernels.hip"
#include "fba_search.hip"

#define FIELDS(X)                                                                                                                          \
    X(P, model) X(P, domain) X(P, planner) X(P, belief) X(P, dirichlet_regular) X(P, N) X(P, E) X(P, S) X(P, A) X(P, O) X(P, C) X(P, Cs)     \
    X(P, packed) X(P, ft_packed) X(P, hist) X(P, hist_row) X(P, hist_rid_bytes) X(P, hist_distinct) X(P, hist_cap) X(P, nested)            \
    X(P, reinvig) X(P, incub) X(P, cheat) X(P, mh) X(P, point) X(P, max_depth) X(P, sims) X(P, horizon) X(P, fd_bytes) X(P, gw_N)           \
    X(P, gw_G) X(P, search_budget) X(D, single_rec) X(D, scratch_slots) X(D, is_multi) X(D, ab_rows_hbm) X(D, ab_hist_multi)              \
    X(D, ab_no_etiger) X(D, ab_tiger_gather) X(D, ab_lockstep) X(D, max_nodes) X(D, mh_scratch_words) X(D, hmask)
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

static int run_case(char* line)
{
    fba::Problem P{};
    fba::DeviceState D{};
    P.S = P.E = 1;
    char* save = nullptr;
    const char* name = strtok_r(line, " \n", &save);
    const char* what = strtok_r(nullptr, " \n", &save);
    if (!name || !what) return 2;
    for (char* tok; (tok = strtok_r(nullptr, " \n", &save));) {
        char* eq = strchr(tok, '=');
        if (!eq) return 2;
        *eq = 0;
        if (!set_field(P, D, tok, strtol(eq + 1, nullptr, 0))) { fprintf(stderr, "%s: unknown field %s\n", name, tok); return 2; }
    }
    std::string json = std::string("{\"name\": \"") + name + "\"";
    for (const char* w = what; *w; ++w) {
        capture::out.clear();
        if (*w == 's') fba::launch_search(P, D, nullptr);
        else if (*w == 'u') fba::launch_belief_update(P, D, nullptr);
        else if (*w == 'r') fba::launch_reset(P, D, nullptr);
        else return 2;
        std::string calls = capture::out;
        if (!calls.empty()) calls.resize(calls.size() - 2);
        json += std::string(", \"") + *w + "\": [" + calls + "]";
    }
    puts((json + "}").c_str());
    return fflush(stdout) ? 2 : 0;
}

int main()
{
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == '\n' || line[0] == '#') continue;
        fflush(stdout);
        const pid_t pid = fork();
        if (pid < 0) return 3;
        if (pid == 0) _exit(run_case(line));
        int status = 0;
        if (waitpid(pid, &status, 0) != pid || !WIFEXITED(status) || WEXITSTATUS(status) != 0) {
            fprintf(stderr, "launch_capture: a case failed: %s\n", line);
            return 1;
        }
    }
    return 0;
}
