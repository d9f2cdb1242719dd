"""fba_giveup_policy without a GPU: the cases of tests/giveup_cases.py do on the oracle what they are there for, the header declares the
new interface under the ABI version it had, and the Python binding knows the symbols."""
import os
import re

import numpy as np
import pytest

import giveup_cases as G
from fba_pomdp_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(G.CASES, **{G.COMPOSITE["name"]: G.COMPOSITE})


@pytest.mark.parametrize("name", list(ALL))
def test_the_case_retires_some_runs_and_keeps_some(name):
    """at least 4 runs retired and 4 surviving, a retirement in each episode, a retired run whose slot has another to go on with.  (The
    composite case is held to its main filter's counts: the fully connected filter can only retire more, and earlier.)"""
    c = ALL[name]
    tr, steps = G.oracle_run(c)
    assert np.all(np.diff(tr["run"]) >= 0)                      # ordered by run: predict() walks a run's records in their order
    p = G.predict(c, tr, steps)
    counted = G.mix_conditions(c, p)
    eps = [sum(1 for r in p["retired"] if r[1] == ep) for ep in range(c["kw"]["episodes"])]
    print(f"{name}: max_attempts {c['max_attempts']}: {len(p['retired'])} / {c['runs']} retired, by episode {eps}, {counted} at an episode's last step; "
          f"{int(p['keep'].sum())} of {len(tr)} records kept")
    # the predictor against itself: a limit nobody exceeds retires nobody and leaves the oracle's experiment
    q = G.predict(c, tr, steps, max_attempts=1 << 28)
    assert not q["retired"] and q["keep"].all() and q["counters"][2] == len(tr)
    assert all(s[0] == c["runs"] for s in q["stats"])
    # a retired run's records end with the one that gave up; void episodes have no length
    for run, ep, t, _, is_counted, _ in p["retired"]:
        mine = tr[p["keep"] & (tr["run"] == run)]
        assert (mine["episode"][-1], mine["t"][-1]) == (ep, t) and mine["update_count"][-1] > c["max_attempts"]
        assert np.all(mine["update_count"][:-1] <= c["max_attempts"])
        assert (p["lengths"][run, ep] > 0) == bool(is_counted) and not np.any(p["lengths"][run, ep + 1:])
    assert [s[0] for s in p["stats"]] == [float(np.sum(p["lengths"][:, ep] > 0)) for ep in range(c["kw"]["episodes"])]


def test_some_retirement_is_at_an_episodes_last_step():
    """counted = 1: the step that gave up had ended its episode, whose return stays"""
    total = 0
    for c in G.CASES.values():
        total += sum(r[4] for r in G.predict(c, *G.oracle_run(c))["retired"])
    assert total >= 1


def test_every_kernel_with_a_give_up_site_has_a_case():
    """the table names a case for each; tests/test_gpu_giveup.py asks every case's context for its real launch plan and holds it to the
    name (that a kernel's round divides the quantum is a static_assert of the kernel's own)"""
    assert {c["kernel"] for c in G.CASES.values()} == G.GIVE_UP_KERNELS
    assert G.COMPOSITE["kernel"].count("reject_kernel<factored tiger>") == 2      # the fully connected launch, then the main filter's
    for c in list(G.CASES.values()) + [G.COMPOSITE]:
        assert c["max_attempts"] % N.REJECT_QUANTUM == 0 and c["max_attempts"] > 0


def test_kernel_keys_decode_to_the_names_of_the_table():
    """decode_kernel against the key layout of fba_launch_plan.h (kernel_key: name << 24 | a << 18 | b << 12 | c << 6 | d)"""
    names = G.kernel_names()
    num = {v: k for k, v in names.items()}
    assert names[1] == "K_SEARCH" and "K_REJECT" in num and "K_REINVIGORATE" in num
    key = lambda k, a=0, b=0, c=0, d=0: num[k] << 24 | a << 18 | b << 12 | c << 6 | d
    assert G.decode_kernel(key("K_REJECT_TIGER_LDS"), names) == "reject_tiger_lds_kernel"
    assert G.decode_kernel(key("K_REJECT_HIST", 8), names) == "reject_hist_kernel"
    assert G.decode_kernel(key("K_REJECT", 2, 0, 3, 4), names) == "reject_kernel<packed factored tiger>"
    assert G.decode_kernel(key("K_REJECT", 0, 0, 3, 4), names) == "reject_kernel<factored tiger>"
    assert G.decode_kernel(key("K_REJECT", 0, 2, 0, 8), names) == "reject_kernel<packed tiger>"
    assert G.decode_kernel(key("K_REJECT", 0, 0, 0, 4), names) == "reject_kernel<plain>"
    assert G.decode_kernel(key("K_REINVIGORATE"), names) == "K_REINVIGORATE"


def test_header_declares_the_interface():
    h = open(os.path.join(ROOT, "include", "fba_hip.h")).read()
    assert re.search(r"#define FBA_ABI_VERSION 3\b", h)
    assert re.search(r"#define FBA_REJECT_QUANTUM 1024\b", h) and N.REJECT_QUANTUM == 1024
    assert re.search(r"#define FBA_UPDATE_GAVE_UP \(-2\)", h) and N.UPDATE_GAVE_UP == -2
    assert re.search(r"enum \{ FBA_GIVEUP_STOP = 0, FBA_GIVEUP_RETIRE = 1 \};", h) and (N.GIVEUP_STOP, N.GIVEUP_RETIRE) == (0, 1)
    assert re.search(r"int fba_giveup_policy\(fba_ctx\* ctx, int32_t policy, int32_t max_attempts", h)
    assert re.search(r"int fba_retired_count\(const fba_ctx\* ctx, int64_t\* seen\);", h)
    assert re.search(r"int fba_get_retired\(const fba_ctx\* ctx, fba_retired_rec\* out, int32_t cap\);", h)
    body = re.search(r"typedef struct fba_retired_rec \{(.*?)\} fba_retired_rec;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.strip() for decl in re.findall(r"int32_t ([^;]+);", body) for m in decl.split(",")]
    assert members == list(N.RETIRED_DTYPE.names) and N.RETIRED_DTYPE.itemsize == 32
    assert all(N.RETIRED_DTYPE.fields[m][0] == np.dtype("<i4") for m in members)


def test_the_binding_knows_the_symbols():
    for name in ("fba_giveup_policy", "fba_retired_count", "fba_get_retired"):
        assert name in N.EXPORTS
    assert os.path.join(N.HERE, "csrc", "fba_retire.hip") in N.SOURCES
    lib = N.load()
    assert len(lib.fba_giveup_policy.argtypes) == 3 and len(lib.fba_retired_count.argtypes) == 2 and len(lib.fba_get_retired.argtypes) == 3
    import fba_pomdp_amd as fba
    assert callable(fba.Engine.giveup_policy) and callable(fba.Engine.retired)
    assert N.GIVEUP_NAMES == {"stop": 0, "retire": 1}
