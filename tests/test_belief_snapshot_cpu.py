"""Belief snapshots without a GPU: the built library exports the four calls, the header declares them under the unchanged ABI version,
the kernels of fba_snapshot.hip cross-compile for gfx950 without scratch or spills, their VGPR counts pinned (read from the code-object
metadata hipcc emits, as test_belief_probe_cpu.py does), and the host pass of an import -- fba_snapshot_format.h, header-only and free of
HIP -- refuses truncated, zeroed and bit-flipped headers when a stand-alone host program feeds them to it under the address and
undefined-behaviour sanitizers.  The sanitizers see that program alone, never code loaded into Python."""
import os
import re
import subprocess

import numpy as np

import fba_pomdp_amd as fba
from fba_pomdp_amd import _native as N

ARGS = "ENS_7ProblemENS_11DeviceStateENS_18BeliefSnapshotArgsE"
# (scratch bytes, VGPRs, spilled VGPRs)
PINNED = {
    "_ZN3fba20snapshot_pack_kernel" + ARGS: (0, 22, 0),
    "_ZN3fba22snapshot_commit_kernel" + ARGS: (0, 8, 0),
    "_ZN3fba25snapshot_replicate_kernelENS_7ProblemENS_11DeviceStateEii": (0, 48, 0),     # sixteen 16-byte pieces in flight per lane
    "_ZN3fba24snapshot_validate_kernelILi0EEEv" + ARGS[1:]: (0, 28, 0),    # fp32 counts
    "_ZN3fba24snapshot_validate_kernelILi1EEEv" + ARGS[1:]: (0, 26, 0),    # the packed formats
    "_ZN3fba24snapshot_validate_kernelILi5EEEv" + ARGS[1:]: (0, 37, 0),    # gridworld FBA-POMDP records
    "_ZN3fba24snapshot_validate_kernelILi6EEEv" + ARGS[1:]: (0, 28, 0),    # tabular gridworld records
    "_ZN3fba24snapshot_validate_kernelILi7EEEv" + ARGS[1:]: (0, 28, 0),    # collision-avoidance records
}
CALLS = ("fba_belief_snapshot_bytes", "fba_belief_export", "fba_belief_import", "fba_belief_replicate")
CSRC = os.path.join(N.HERE, "csrc")


def test_the_library_exports_the_snapshot_calls():
    fba.build()
    lib = fba.load()
    for name in CALLS:
        assert name in N.EXPORTS and hasattr(lib, name), name
    assert os.path.join(CSRC, "fba_snapshot.hip") in N.SOURCES
    assert os.path.join(CSRC, "fba_snapshot_format.h") in N.HEADERS
    for name in ("belief_snapshot_bytes", "belief_export", "belief_import", "belief_replicate"):
        assert hasattr(fba.Engine, name), name


def test_the_header_declares_the_calls():
    header = open(os.path.join(N.ROOT, "include", "fba_hip.h")).read()
    assert re.search(r"int fba_belief_snapshot_bytes\(const fba_ctx\* ctx, int64_t\* per_slot\);", header)
    assert re.search(r"int fba_belief_export\s*\(fba_ctx\* ctx, int32_t first, int32_t count, void\* buf, int64_t cap\);", header)
    assert re.search(r"int fba_belief_import\s*\(fba_ctx\* ctx, int32_t first, int32_t count, const void\* buf, int64_t bytes\);", header)
    assert re.search(r"int fba_belief_replicate\(fba_ctx\* ctx, int32_t src, int32_t first, int32_t count\);", header)
    assert "#define FBA_ABI_VERSION 3 " in header
    assert "typedef struct fba_snapshot_head {" in header
    # the header as the C struct lays it out: 64 bytes, the two 64-bit fields last
    assert N.SNAPSHOT_HEAD_DTYPE.itemsize == 64
    assert N.SNAPSHOT_HEAD_DTYPE.names == ("magic", "version", "record_format", "weighted", "model", "domain", "actions", "size", "width", "height",
                                           "updates", "particles", "particle_bytes", "counts_len", "states", "observations", "hist_cnt", "stride",
                                           "prior_hash", "checksum")
    assert [N.SNAPSHOT_HEAD_DTYPE.fields[k][1] for k in ("particles", "hist_cnt", "stride", "prior_hash", "checksum")] == [20, 40, 44, 48, 56]
    assert "#define FBA_SNAPSHOT_MAGIC     0x%08xu" % N.SNAPSHOT_MAGIC in header
    assert "#define FBA_SNAPSHOT_CHECK_MUL 0x%016Xull" % N.SNAPSHOT_CHECK_MUL in header


def test_the_checksum_formula_in_numpy():
    words = np.array([7, 0, 0xffffffff, 12345, 1], "<u4")
    by_hand = sum(int(w) * ((i + 1) * N.SNAPSHOT_CHECK_MUL) for i, w in enumerate(words)) % 2 ** 64
    assert N.snapshot_checksum(words) == by_hand
    assert N.snapshot_checksum(words.view(np.uint8)) == by_hand
    assert N.snapshot_checksum(words[::-1].copy()) != by_hand


def test_snapshot_kernels_use_no_scratch(tmp_path):
    flags = [f for f in N.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "fba_snapshot.s"
    src = os.path.join(CSRC, "fba_snapshot.hip")
    subprocess.check_call(["hipcc"] + flags + ["-I" + os.path.join(N.ROOT, "include"), "-S", "--cuda-device-only", "-o", str(out), src],
                          stderr=subprocess.DEVNULL)
    meta = out.read_text()
    meta = meta[meta.index("amdhsa.kernels:"):]
    seen = {}
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        seen[name] = (get("private_segment_fixed_size"), get("vgpr_count"), get("vgpr_spill_count"))
    assert seen == PINNED


def test_the_host_pass_refuses_bad_headers_under_sanitizers(tmp_path):
    exe = tmp_path / "snapshot_format_check"
    src = os.path.join(N.ROOT, "tests", "snapshot_format_check.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-I" + os.path.join(N.ROOT, "include"), "-I" + CSRC, src, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "snapshot_format_check: ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
