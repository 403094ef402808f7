"""The counted waits of the three-step fp64 block strip's edge values (crd_fused_impl.h: kEdgeLadder; crd_edge_waits.h), without a device:

lint        tools/kernel_regs.py async_lds_read_hazards on synthetic assembly: a read's register touched behind a counted wait that covers
            it is no finding, behind one that is one too lax it is, and so is a covering wait with a scalar memory load between read and
            wait; the `lgkmcnt(0)` cases are what they were.
table       the three-step fp64 rows of the build's kernel table: no hazard, no vector memory skipped on the execution mask, no scratch,
            registers and the loop's vector instructions at the parent's figures, no wait of the compiler's in the edge window.
others      every other kernel's row of the table as profiles/r10/kernel_table.txt has it, to the character.
constants   tests/native/edge_ladder_selftest.cpp: the header's constants against a written-out list of an iteration's LDS operations."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_regs  # noqa: E402

CSRC = os.path.join(ROOT, "crdmodel_amd", "csrc")

EXCHANGE = """
\t;;#ASMSTART
\ts_waitcnt lgkmcnt(0)
\ts_barrier
\ts_mov_b64 exec, s[30:31]
\tds_read_b128 v[22:25], v239 offset:0
\tds_read_b128 v[18:21], v239 offset:16
\tds_read_b128 v[14:17], v239 offset:32
\ts_mov_b64 exec, -1
\t;;#ASMEND
"""
PUBLISH = """
\t;;#ASMSTART
\tds_write_b64 v238, v[52:53] offset:0
\t;;#ASMEND
"""


def _wait(n):
    return "\t;;#ASMSTART\n\ts_waitcnt lgkmcnt(%d)\n\t;;#ASMEND\n" % n


def _hazards(text):
    return kernel_regs.async_lds_read_hazards(("kernel:\n" + text + "\ts_endpgm\n").splitlines())


USE_FIRST = "\tv_add_f64 v[46:47], v[42:43], -v[22:23]\n"   # reads the first read's register
USE_LAST = "\tv_add_f64 v[46:47], v[42:43], -v[14:15]\n"    # ... the last read's
LANDED = _wait(0) + USE_FIRST + USE_LAST


def test_a_counted_wait_that_covers_the_read_retires_it():
    # behind the first read: two reads and one publish = 3 operations; lgkmcnt(3) leaves exactly those outstanding
    assert _hazards(EXCHANGE + PUBLISH + _wait(3) + USE_FIRST + LANDED) == []
    # ... stricter waits too
    assert _hazards(EXCHANGE + PUBLISH + _wait(2) + USE_FIRST + LANDED) == []
    # the last read: one publish behind it
    assert _hazards(EXCHANGE + PUBLISH + _wait(1) + USE_FIRST + USE_LAST) == []
    # a ladder: publishes between the waits count for the later reads
    assert _hazards(EXCHANGE + PUBLISH + _wait(3) + USE_FIRST + PUBLISH + PUBLISH + _wait(3) + USE_LAST) == []


def test_a_counted_wait_one_too_lax_is_a_finding():
    found = _hazards(EXCHANGE + PUBLISH + _wait(4) + USE_FIRST + LANDED)
    assert len(found) == 1 and found[0][1] == 22 and "v[22:23]" in found[0][2], found
    found = _hazards(EXCHANGE + PUBLISH + _wait(2) + USE_LAST + LANDED)
    assert len(found) == 1 and found[0][1] == 14, found
    # only asm blocks' LDS instructions count: the wait's number comes from the source's own operations
    found = _hazards(EXCHANGE + "\tds_write_b64 v238, v[52:53] offset:0\n" + _wait(3) + USE_FIRST + LANDED)
    assert len(found) == 1 and found[0][1] == 22, found
    # every path keeps its own count: a branch around the publish reaches the wait with one operation fewer
    found = _hazards(EXCHANGE + "\ts_cbranch_scc1 .LBB0_1\n" + PUBLISH + ".LBB0_1:\n" + _wait(3) + USE_FIRST + LANDED)
    assert len(found) == 1 and found[0][1] == 22, found


def test_a_scalar_load_in_flight_leaves_only_lgkmcnt_zero():
    for load in ("\ts_load_dwordx2 s[34:35], s[48:49], s1 offset:0x0\n", "\ts_buffer_load_dword s3, s[4:7], 0x0\n"):
        found = _hazards(EXCHANGE + load + PUBLISH + _wait(3) + USE_FIRST + LANDED)
        assert len(found) == 1 and found[0][1] == 22, found
        found = _hazards(EXCHANGE + PUBLISH + load + _wait(3) + USE_FIRST + LANDED)
        assert len(found) == 1 and found[0][1] == 22, found
        # ... which retires whatever is in flight
        assert _hazards(EXCHANGE + load + PUBLISH + _wait(0) + USE_FIRST + USE_LAST) == []
        # a load BEHIND the wait is nobody's business
        assert _hazards(EXCHANGE + PUBLISH + _wait(3) + load + USE_FIRST + LANDED) == []
        # the compiler's own lgkmcnt(0) in front of the loaded value's first use: nothing scalar is in flight behind it -- and it lands no read
        assert _hazards(EXCHANGE + load + "\ts_waitcnt lgkmcnt(0)\n" + PUBLISH + _wait(3) + USE_FIRST + LANDED) == []
        assert len(_hazards(EXCHANGE + load + "\ts_waitcnt lgkmcnt(0)\n" + USE_FIRST + LANDED)) == 1


def test_lgkmcnt_zero_cases_are_what_they_were():
    assert _hazards(EXCHANGE + PUBLISH + _wait(0) + USE_FIRST + USE_LAST) == []
    found = _hazards(EXCHANGE + PUBLISH + USE_FIRST + _wait(0) + USE_LAST)
    assert len(found) == 1 and found[0][1] == 22, found
    # a wait of the compiler's (outside asm blocks) lands nothing
    found = _hazards(EXCHANGE + "\ts_waitcnt lgkmcnt(0)\n" + USE_LAST + _wait(0))
    assert len(found) == 1 and found[0][1] == 14, found
    # a copy at the loop's back edge, the case the check was written for
    found = _hazards(".LBB0_1:\n" + _wait(0) + USE_FIRST + EXCHANGE + "\tv_mov_b32_e32 v100, v18\n\ts_cbranch_scc1 .LBB0_1\n" + _wait(0))
    assert len(found) == 1 and found[0][1] == 18, found
    # a block that waits for its own reads is no asynchronous read
    own = "\t;;#ASMSTART\n\tds_read_b64 v[2:3], v9 offset:0\n\ts_waitcnt lgkmcnt(0)\n\t;;#ASMEND\n\tv_mov_b32_e32 v4, v2\n"
    assert _hazards(own) == []


def test_the_edge_window_counts_the_compilers_waits_between_the_reads_and_the_last_wait():
    two_reads = EXCHANGE
    loop = (".LBB0_1:\n" + "\ts_waitcnt lgkmcnt(0)\n" + PUBLISH + _wait(3) + USE_FIRST + "\ts_waitcnt vmcnt(0) lgkmcnt(0)\n" + _wait(1) + "\ts_waitcnt lgkmcnt(0)\n" + USE_LAST + two_reads
            + "\ts_cbranch_scc1 .LBB0_1\n")
    # around the back edge: the wait at the loop's top and the one between the two counted waits; the one behind the last counted wait is outside
    assert kernel_regs.lgkm_waits_in_edge_window(loop.splitlines()) == 2
    assert kernel_regs.lgkm_waits_in_edge_window((".LBB0_1:\n" + PUBLISH + _wait(3) + USE_FIRST + _wait(1) + "\ts_waitcnt lgkmcnt(0)\n" + two_reads).splitlines()) == 0
    # no stand-alone wait, no window
    assert kernel_regs.lgkm_waits_in_edge_window((".LBB0_1:\n" + PUBLISH + two_reads).splitlines()) is None


def _table():
    path = os.path.join(CSRC, "build", "kernel_table.json")
    if not os.path.exists(path):
        pytest.skip("no kernel table beside the library (a build with KERNEL_TABLE=0)")
    return json.load(open(path))["kernels"]


# The parent's figures (profiles/r10/kernel_table.txt): registers and the vector instructions of one trip of the steady-state loop
PARENT = {0: {"vgprs": 243, "valu": 842}, 1: {"vgprs": 246, "valu": 1165}}  # by `absorb`


def test_three_step_fp64_rows_of_this_build():
    rows = [r for r in _table() if r["precision"] == "f64" and r["steps"] == 3]
    assert sorted((r["absorb"], r["nt"], r.get("waves", 4)) for r in rows) == [(0, 0, 4), (0, 0, 8), (0, 1, 4), (0, 1, 8), (1, 0, 4), (1, 1, 4)]
    for r in rows:
        assert r["model"] == 0 and r["cols"] == 1
        assert r["async_lds_read_hazards"] == 0, r
        assert r["exec_skipped_vmem"] == 0, r
        assert r["scratch_bytes"] == 0, r
        assert r["vgprs"] <= PARENT[r["absorb"]]["vgprs"], r
        assert r["loop"]["valu"] == PARENT[r["absorb"]]["valu"], r
        assert r["lgkm_waits_in_edge_window"] == 0, r


THREE_STEP_F64 = re.compile(r"crd_rk4_fused_step_kernel<double, 0, (true|false), 0, 1, (true|false), 3, [48]>")


def test_every_other_kernels_row_is_the_parents():
    path = os.path.join(CSRC, "build", "kernel_table.txt")
    if not os.path.exists(path):
        pytest.skip("no kernel table beside the library (a build with KERNEL_TABLE=0)")
    mine = [ln.rstrip("\n") for ln in open(path)]
    parent = [ln.rstrip("\n") for ln in open(os.path.join(ROOT, "profiles", "r10", "kernel_table.txt"))]
    assert sum(1 for ln in parent if THREE_STEP_F64.search(ln)) == 6 and sum(1 for ln in mine if THREE_STEP_F64.search(ln)) == 6
    assert [ln for ln in mine if not THREE_STEP_F64.search(ln)] == [ln for ln in parent if not THREE_STEP_F64.search(ln)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_wait_constants_against_a_written_out_iteration(tmp_path):
    exe = tmp_path / "edge_ladder_selftest"
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "native", "edge_ladder_selftest.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "edge ladder selftest ok" in run.stdout
