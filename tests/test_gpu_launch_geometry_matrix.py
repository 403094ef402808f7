"""What the fused step launcher would launch -- strips, rows per item, items, workgroups, block width, XCD mapping's workgroup count,
valid lanes, the kernel the launch resolves to (by its row of the build's kernel table) and the plan as resolved -- over a matrix of
shapes and pinned plans, against tests/golden/fused_launch_geometry.json.gz: every plan candidate x fp64 / fp32 x FHN / Goldbeter x
nx in {40, 57, 232, 233, 489, 2048, 8192} x ny in {24, 64, 1024}, plus 8192 x 8192 and 4096 x 4096 fp64 FHN.  Plans are pinned
(crd_set_launch_plan) and read back (crd_get_launch_plan, crd_get_launch_geometry); nothing is launched.

The fixture was written by tools/dump_launch_geometry.py on an MI355X before the launcher was split into crd_fused_plan.h and
crd_fused_launch.h: the split must not move a number.  It depends on the device's CU count and on the kernels' occupancy (resident
wavefront slots enter the chunk rule and the XCD mapping), so a later change of occupancy regenerates it with that tool; on a device
with another CU count the test skips."""
import os
import sys

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def test_every_launch_of_the_matrix_has_the_recorded_geometry(gpu_device):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import dump_launch_geometry as tool
    finally:
        sys.path.pop(0)
    want = tool.load(os.path.join(GOLDEN, "fused_launch_geometry.json.gz"))
    got = tool.dump()
    if got["simds"] != want["simds"]:
        pytest.skip("the fixture is an MI355X's (%d SIMDs); this device has %d" % (want["simds"], got["simds"]))
    assert got["plans"] == want["plans"] and len(got["plans"]) == 60
    assert got["fields"] == want["fields"]
    assert len(got["cases"]) == len(want["cases"]) == 2 * 2 * 7 * 3 + 2
    fields = want["fields"]
    for g, w in zip(got["cases"], want["cases"]):
        head = {f: w[f] for f in ("precision", "model", "nx", "ny")}
        assert {f: g[f] for f in head} == head
        assert len(g["rows"]) == len(w["rows"]) == len(want["plans"])
        for plan, grow, wrow in zip(want["plans"], g["rows"], w["rows"]):
            if grow != wrow:
                diff = {f: (a, b) for f, a, b in zip(fields, grow, wrow) if a != b}
                assert not diff, (head, plan, diff)
