#!/usr/bin/env python3
"""What the fused step launcher WOULD launch over a fixed matrix of shapes and pinned plans, as JSON: every plan candidate
(crd_launch_plan_candidate) x fp64 / fp32 x FHN / Goldbeter x nx in NX x ny in NY, plus 8192 x 8192 fp64 FHN and 4096 x 4096 fp64 FHN.
Plans are pinned with crd_set_launch_plan and read back with crd_get_launch_plan / crd_get_launch_geometry: nothing is launched.

    python tools/dump_launch_geometry.py tests/golden/fused_launch_geometry.json.gz      # (without a path: the JSON itself, to stdout)

tests/test_gpu_launch_geometry_matrix.py holds the tree to the committed file.  The numbers depend on the device's CU count and on the
kernels' occupancy (resident wavefront slots enter the chunk rule and the XCD mapping): a change of either regenerates the file with this
tool.  CRD_LIBRARY selects another build of the library (crdmodel_amd/_capi.py)."""
import ctypes as C
import gzip
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crdmodel_amd as crd  # noqa: E402
from crdmodel_amd import _capi as capi  # noqa: E402

NX = (40, 57, 232, 233, 489, 2048, 8192)
NY = (24, 64, 1024)
EXTRA = (("f64", "fhn", 8192, 8192), ("f64", "fhn", 4096, 4096))
# every integer crd_get_launch_geometry reports but the clock, which is the device's and not the launch's; then the plan as resolved
GEOMETRY_FIELDS = tuple(f for f, _ in capi.LaunchGeometry._fields_ if f not in ("simds", "clock_khz"))
PLAN_FIELDS = ("one_round", "xcd_mapping", "columns_per_lane", "nontemporal_stores", "steps_per_launch")
FIELDS = GEOMETRY_FIELDS + PLAN_FIELDS


def candidates():
    out = []
    while True:
        lp = capi.LaunchPlan()
        if capi.lib().crd_launch_plan_candidate(len(out), C.byref(lp)) != 0:
            return out
        out.append([lp.one_round, lp.xcd_mapping, lp.columns_per_lane, lp.nontemporal_stores, lp.steps_per_launch])


def shapes():
    for precision in ("f64", "f32"):
        for model in ("fhn", "goldbeter"):
            for nx in NX:
                for ny in NY:
                    yield precision, model, nx, ny
    yield from EXTRA


def dump():
    plans = candidates()
    simds, cases = None, []
    for precision, model, nx, ny in shapes():
        p = crd.make_params(model, "torus", nx, 80.0, 20.0, 0.12, 1.25 if model == "fhn" else 0.4, ny=ny, precision=precision)
        rows = []
        with crd.Slab(p) as s:
            for plan in plans:
                s.set_launch_plan(*plan)
                g, lp = s.launch_geometry(), s.launch_plan()
                simds = g["simds"] if simds is None else simds
                assert g["simds"] == simds
                rows.append([int(g[f]) for f in GEOMETRY_FIELDS] + [int(lp[f]) for f in PLAN_FIELDS])
        cases.append({"precision": precision, "model": model, "nx": nx, "ny": ny, "rows": rows})
    return {"simds": simds, "plans": plans, "fields": list(FIELDS), "cases": cases}


def write(doc, out):
    # one line per case and candidate row kept short: the file is read by people too
    out.write('{"simds": %d,\n "plans": %s,\n "fields": %s,\n "cases": [\n' % (doc["simds"], json.dumps(doc["plans"]), json.dumps(doc["fields"])))
    for k, c in enumerate(doc["cases"]):
        head = {f: c[f] for f in ("precision", "model", "nx", "ny")}
        out.write("  " + json.dumps(head)[:-1] + ', "rows": ' + json.dumps(c["rows"], separators=(",", ":")) + "}" + (",\n" if k + 1 < len(doc["cases"]) else "\n"))
    out.write(" ]}\n")


def load(path):
    with gzip.open(path, "rt") as f:
        return json.load(f)


if __name__ == "__main__":
    if len(sys.argv) > 1:  # compressed (437 KB of digits otherwise), with no time stamp in it: the same numbers give the same file
        text = io.StringIO()
        write(dump(), text)
        with open(sys.argv[1], "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(text.getvalue().encode())
    else:
        write(dump(), sys.stdout)
