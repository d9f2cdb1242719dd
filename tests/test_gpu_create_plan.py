"""fba_create decides what it decided before it was split into stages: tests/create_plan_cases.py lists configurations on both sides of
every choice of record format, of every tree_buckets rule, one good context of each composite belief, one case for every refusal with its
message, and six with two faults at once that pin which refusal wins.  Each is created (nothing runs) and what the context answers --
return code, message, sizes, record bytes, slots, snapshot bytes and the header of an exported slot -- is compared with the recording of
the earlier fba_create, field by field and without tolerance.  The layout fields no getter shows (node words, node bound, hash capacity,
bucket lines, scratch slots, side row width) are pinned by the suite's bit-exact oracle experiments instead."""
import ctypes as C

import pytest

import create_plan_cases as T
import fba_pomdp_amd as fba

DEVICE_CASES = ("device_out_of_range", "device_negative")


@pytest.fixture(scope="module")
def expected():
    return T.expected()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in T.CASES])
def test_fba_create_plans_as_recorded(name, expected):
    L = fba.load()
    want = dict(expected[name])
    if name in DEVICE_CASES:     # (the recording machine showed one device)
        ndev = C.c_int()
        assert C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(ndev)) == 0
        assert "(1 visible)" in want["error"]
        want["error"] = want["error"].replace("(1 visible)", f"({ndev.value} visible)")
    seen = T.observe(L, T.BY_NAME[name])
    print(name, seen)
    assert seen == want


def test_every_case_has_a_recording():
    """the table and the recording list the same cases; every refusal's message is there in full"""
    want = T.expected()
    assert sorted(want) == sorted(T.BY_NAME)
    for name, rec in want.items():
        assert (rec["rc"] == 0) == ("sizes" in rec) and (rec["rc"] != 0) == bool(rec.get("error")), name
