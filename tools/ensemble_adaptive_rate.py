"""Error-controlled ensembles against the same members integrated one after another as lone contexts ("Ensembles").

The shipped FHN 400 x 1600 and Goldbeter 100 x 400 grids in fp64, B in {1, 4, 16, 64} members that differ in beta, each integrated
from its initial state to a fixed tout with the reference's integrator (CRD_ADAPT_ARKODE, rtol 1e-5, atol 1e-10, capped at the
stability bound): (a) one Ensemble.integrate_adaptive call; (b) B Slabs, one integrate_adaptive call each, one after another.  Wall
time of the call(s) after one warm-up run of each; attempts per second (accepted + rejected, summed over the members); the
ensemble's rounds (attempt launches: the largest member's attempt count) and its mean active fraction (attempts / (rounds x B)).
The lone contexts run their default launch plan (no plan measurement inside the timed calls).

    python tools/ensemble_adaptive_rate.py [--members 1,4,16,64] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import crdmodel_amd as crd  # noqa: E402

INI = os.path.join(ROOT, "tests", "golden", "ini")
TOUT = {"fhn": 2.0, "goldbeter": 1.0}


def members_of(case, n):
    model = "fhn" if case == "fhn" else "goldbeter"
    cfg = crd.load_ini(os.path.join(INI, "%s_shipped.ini" % case), model, "torus")
    lo, hi = (0.9, 1.3) if case == "fhn" else (0.3, 0.75)
    out = []
    for b in np.linspace(lo, hi, n):
        q = crd._capi.Params.from_buffer_copy(cfg.params)
        q.beta = float(b)
        out.append(q)
    return cfg, out


def ensemble_run(members, ys, tout):
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        t0 = time.perf_counter()
        sts = e.integrate_adaptive(0.0, tout)
        wall = time.perf_counter() - t0
    assert all(st["status"] == crd._capi.OK for st in sts)
    return wall, [st["accepted"] + st["rejected"] for st in sts]


def lone_run(members, ys, tout):
    slabs = []
    for p, y in zip(members, ys):
        s = crd.Slab(p)
        s.set_autotune(0)  # (the default plan: a lone run's one-time plan measurement is not part of its stepping)
        s.upload(y)
        slabs.append(s)
    t0 = time.perf_counter()
    sts = [s.integrate_adaptive(0.0, tout) for s in slabs]
    wall = time.perf_counter() - t0
    for s in slabs:
        s.close()
    return wall, [st["accepted"] + st["rejected"] for st in sts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="1,4,16,64")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for case in ("fhn", "goldbeter"):
        for n in [int(x) for x in a.members.split(",")]:
            cfg, members = members_of(case, n)
            cfgs = [crd.run_config(p, wave_length=cfg.wave_length, wave_width=cfg.wave_width, wave_inside=cfg.wave_inside) for p in members]
            ys = [crd.initial_conditions(c) for c in cfgs]
            tout = TOUT[case]
            ensemble_run(members, ys, tout)  # warm-up (allocations, code objects)
            lone_run(members, ys, tout)
            ew, ea = ensemble_run(members, ys, tout)
            lw, la = lone_run(members, ys, tout)
            rounds = max(ea)
            row = dict(case=case, nx=members[0].nx, ny=crd.grid_of(members[0]).ny, members=n, tout=tout, ensemble_s=ew, lone_s=lw,
                       attempts=sum(ea), lone_attempts=sum(la), rounds=rounds, active_fraction=sum(ea) / (rounds * n), speedup=lw / ew)
            rows.append(row)
            print("%-10s %dx%d B=%2d tout %g  ensemble %.4f s (%.0f attempts/s, %d rounds, active %.2f)  lone %.4f s (%.0f attempts/s)  x%.2f" %
                  (case, row["nx"], row["ny"], n, tout, ew, sum(ea) / ew, rounds, row["active_fraction"], lw, sum(la) / lw, row["speedup"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
