"""fba_belief_convert without a GPU: the built library exports the two calls and the header declares them, the kernels of
fba_convert.hip cross-compile for gfx950 without scratch or spills (read from the code-object metadata hipcc emits, as
test_structures_abi.py reads it), the host pass -- check_convert_head of fba_snapshot_format.h, header-only and free of HIP -- judges
headers as stated when a stand-alone host program feeds them to it under the address and undefined-behaviour sanitizers (the sanitizers
see that program alone, never code loaded into Python), the host restatement of tests/convert_cases.py picks what its definition says,
and the seeds of tests/resume_cases.py have the property tests/test_gpu_belief_convert.py relies on, established on the oracle."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import convert_cases as K
import fba_pomdp_amd as fba
import resume_cases as R
from fba_pomdp_amd import _native as N

CSRC = os.path.join(N.HERE, "csrc")
KERNELS = ("_ZN3fba28snapshot_convert_scan_kernelENS_17BeliefConvertArgsE",
           "_ZN3fba23snapshot_convert_kernelILb1EEEvNS_7ProblemENS_17BeliefConvertArgsE",
           "_ZN3fba23snapshot_convert_kernelILb0EEEvNS_7ProblemENS_17BeliefConvertArgsE")


def _header():
    return open(os.path.join(N.ROOT, "include", "fba_hip.h")).read()


def test_the_library_exports_the_calls():
    fba.build()
    lib = fba.load()
    for name in ("fba_belief_convert", "fba_snapshot_block_bytes"):
        assert name in N.EXPORTS and hasattr(lib, name), name
    assert os.path.join(CSRC, "fba_convert.hip") in N.SOURCES
    assert list(inspect.signature(fba.Engine.belief_convert).parameters) == ["self", "blocks", "seed", "first_run"]
    sig = inspect.signature(fba.Engine.belief_convert).parameters
    assert (sig["seed"].default, sig["first_run"].default) == (0, 0)
    assert callable(fba.snapshot_block_bytes)


def test_the_header_declares_the_calls():
    h = _header()
    assert re.search(r"FBA_PHASE_CONVERT\s*=\s*14\b", h)
    assert re.search(r"int64_t fba_snapshot_block_bytes\(const fba_snapshot_head\* head\);", h)
    decl = re.search(r"int fba_belief_convert\((.*?)\);", h, re.S).group(1)
    args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert args == ["fba_ctx* ctx", "int32_t count", "const void* src", "int64_t src_bytes", "uint64_t seed", "uint32_t first_run", "void* dst", "int64_t dst_cap"]
    assert len(fba.load().fba_belief_convert.argtypes) == len(args)
    assert "#define FBA_ABI_VERSION 3 " in h and "#define FBA_SNAPSHOT_VERSION   1" in h
    assert K.PH_CONVERT == 14


def test_block_bytes_is_host_arithmetic():
    """64 + (weighted ? particles * 8 : 0) + particles * particle_bytes, from a header alone: no context, no GPU"""
    fba.build()
    head = np.zeros(1, N.SNAPSHOT_HEAD_DTYPE)
    head["particles"], head["particle_bytes"], head["weighted"] = 300, 80, 1
    assert fba.snapshot_block_bytes(head.tobytes()) == 64 + 300 * 8 + 300 * 80
    head["weighted"] = 0
    assert fba.snapshot_block_bytes(head.tobytes() + b"payload") == 64 + 300 * 80
    head["particles"], head["particle_bytes"] = 2 ** 31 - 1, 2 ** 31 - 4      # (no overflow in the product)
    assert fba.snapshot_block_bytes(head.view(np.uint8)) == 64 + (2 ** 31 - 1) * (2 ** 31 - 4)
    with pytest.raises(ValueError):
        fba.snapshot_block_bytes(b"short")


def test_convert_kernels_use_no_scratch(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "fba_convert.s"
    subprocess.check_call(["hipcc"] + flags + ["-I" + os.path.join(N.ROOT, "include"), "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(CSRC, "fba_convert.hip")], stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        seen[name] = (get("private_segment_fixed_size"), get("vgpr_spill_count"), get("sgpr_spill_count"), get("vgpr_count"))
    assert set(seen) == set(KERNELS)
    for name, (scratch, spills, sspills, vgprs) in seen.items():
        assert (scratch, spills, sspills) == (0, 0, 0) and vgprs <= 64, (name, scratch, spills, sspills, vgprs)
    # the record mover of the 16-byte form loads and stores whole pieces
    body = text[text.index(KERNELS[1] + ":"):text.index(KERNELS[2] + ":")]
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body


def test_the_scan_has_one_definition():
    """block_device_scan and wave_inclusive_scan: moved to fba_kernels_common.h, not copied"""
    defs = {}
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h", ".inc")):
            src = open(os.path.join(CSRC, f)).read()
            for fn in ("block_device_scan", "wave_inclusive_scan", "block_check_add", "check_term"):
                if re.search(r"__device__ __forceinline__ [a-z ]+ %s\(" % fn, src):
                    defs.setdefault(fn, []).append(f)
    assert defs == {fn: ["fba_kernels_common.h"] for fn in ("block_device_scan", "wave_inclusive_scan", "block_check_add", "check_term")}
    assert "snapshot_validate_kernel" not in open(os.path.join(CSRC, "fba_convert.hip")).read().replace("judged by snapshot_validate_kernel", "")


def test_the_host_pass_under_sanitizers(tmp_path):
    exe = tmp_path / "convert_head_check"
    src = os.path.join(N.ROOT, "tests", "convert_head_check.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-I" + os.path.join(N.ROOT, "include"), "-I" + CSRC, src, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "convert_head_check: ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_host_restatement_of_the_pick():
    """weighted_pick is WeightedFilter::sample in device order: the largest i >= 1 whose exclusive prefix sum is below the threshold"""
    rng = np.random.default_rng(41)
    for n in (1, 2, 37, 300):
        w = K.random_weights(rng, 1, n, zeros=n > 2)[0]
        _, incl = K.orc.dev_scan(w)
        for thr in list(rng.random(50) * incl[-1]) + [0.0, incl[-1], incl[0], incl[n // 2]]:
            by_hand = max([i for i in range(1, n) if incl[i - 1] < thr], default=0)
            assert K.weighted_pick(incl, thr) == by_hand, (n, thr)
    # the draws are addressed by (seed, run, particle): another block is another run, and first_run shifts them
    a = K.expected_sources(5, 0, 3, 130, 300)
    assert np.array_equal(a, K.expected_sources(5, 3, 0, 130, 300)) and not np.array_equal(a, K.expected_sources(5, 0, 2, 130, 300))
    assert not np.array_equal(a, K.expected_sources(6, 0, 3, 130, 300)) and a.min() >= 0 and a.max() < 130
    assert np.array_equal(K.expected_sources(5, 0, 0, 130, 130, np.ones(130)), np.arange(130))
    w = K.random_weights(rng, 1, 300, zeros=True)[0]
    picked = K.expected_sources(9, 0, 1, 300, 130, w)
    assert np.all(w[picked] > 0.0), "a particle of weight 0.0 was picked"


@pytest.mark.parametrize("name", R.GRIDWORLD_HISTORY)
def test_the_seeds_reach_the_whole_record_strides_of_the_short_contexts(name):
    """with the seed of resume_cases.SEEDS, some run makes at least 15 updates in a 2-episode context (its 80-byte records then stand at
    80, not 64) and at least 31 in a 4-episode one (144, not 128); other runs stay at the short strides.  No other seed was needed."""
    short, middle = K.updates_in(name, K.SHORT), K.updates_in(name, K.MIDDLE)
    assert short.max() >= 15 and middle.max() >= 31, (short, middle)
    assert {K.stride_in(K.ROOM_BYTES[K.SHORT], int(n)) for n in short} == {64, 80}, short
    assert 144 in {K.stride_in(K.ROOM_BYTES[K.MIDDLE], int(n)) for n in middle}, middle
    # what the issue's premise says: the short experiments are the first episodes of the long one
    assert np.array_equal(short, R.entries_after(name, K.SHORT)) and np.array_equal(middle, R.entries_after(name, K.MIDDLE))
    assert K.ROOM_BYTES == {2: 80, 4: 144, 5: 176}
