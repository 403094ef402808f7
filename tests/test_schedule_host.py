"""The launch schedule of the fixed-step calls -- crd_schedule.h: how many steps each launch takes (the plan's pairs and triples, the
recorder's sample limits, the exchange cycle, the absorbing rows' decisions) and which launches a timed call times -- checked by a
stand-alone C++ program (tests/native/schedule_selftest.cpp) that walks whole calls with the rule, against sequences written out there
and the rule's properties over small ranges.  Plain g++, no device; once more under AddressSanitizer + UndefinedBehaviorSanitizer, as
that stand-alone program."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "crdmodel_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "native", "schedule_selftest.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("sanitizers", [None, "address,undefined"])
def test_schedule_selftest(tmp_path, sanitizers):
    exe = tmp_path / "schedule_selftest"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC, SOURCE, "-o", str(exe)]
    if sanitizers:
        cmd[4:4] = ["-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizers, "-fno-sanitize-recover=all"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if sanitizers and build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "schedule selftest ok" in run.stdout

