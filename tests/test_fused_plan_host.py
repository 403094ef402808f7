"""The launch-plan arithmetic of the one-launch step -- crd_fused_plan.h: steps per launch, strip count, chunk rows, XCD mapping, band cut,
candidate liveness, ghost-row reach -- checked by a stand-alone C++ program (tests/native/fused_plan_selftest.cpp) against expectations
written out there: the project's recorded plans, the four statements the one steps rule replaced, the recorded ghost-row fault.  Plain
g++, no device and nothing of HIP; once more under AddressSanitizer + UndefinedBehaviorSanitizer, as that stand-alone program."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "crdmodel_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "native", "fused_plan_selftest.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("sanitizers", [None, "address,undefined"])
def test_fused_plan_selftest(tmp_path, sanitizers):
    exe = tmp_path / "fused_plan_selftest"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC, SOURCE, "-o", str(exe)]
    if sanitizers:
        cmd[4:4] = ["-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizers, "-fno-sanitize-recover=all"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if sanitizers and build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "fused plan selftest ok" in run.stdout


def test_the_plan_header_includes_nothing_of_hip():
    text = open(os.path.join(CSRC, "crd_fused_plan.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<algorithm>", "<cstdlib>", '"crd_internal.h"', '"crd_tuning.h"']
    assert not [word for word in ("hip/", "hipError_t", "hipStream_t", "__global__", "__device__") if word in text]
