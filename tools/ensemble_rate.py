"""Aggregate rate of an ensemble against the same members stepped one after another as single contexts ("Ensembles").

The shipped FHN 400 x 1600 and Goldbeter 100 x 400 grids in fp64, B in {1, 4, 16, 64} members that differ in beta: (a) one Ensemble,
one launch per step for all members; (b) B Slabs, each with its measured launch plan, stepped one after another (each call
asynchronous, one synchronisation at the end).  Both device-synchronised, warmed up, with enough steps for a window of at least
--window seconds.  Reports grid-point-steps/s and the fraction of the 8 TB/s roof at 32 B per grid-point-step (one read and one write
of the fp64 state); `in_infinity_cache` says whether the members' two state buffers (2 x 16 B per point each) fit the 256 MiB cache.

    python tools/ensemble_rate.py [--members 1,4,16,64] [--window 1.0] [--json OUT]

--steps-per-launch 1,2 measures the ENSEMBLE alone under each setting (Ensemble.set_steps_per_launch: single steps, pairs) in one
process: after a warm-up of --window seconds, --batches batches (at least 9) per setting, the settings interleaved batch by batch, each
batch timed by events on the ensemble's stream; reports the median per-step time, the batches' spread (min .. max) and the ratio of
the medians.  --precision 64|32.

    python tools/ensemble_rate.py --steps-per-launch 1,2 [--precision 32] [--batches 11] [--cases fhn] [--members 16]

--mixed measures a mixed-geometry ensemble (Ensemble(..., mixed=True)): 8 members of the shipped FHN 400 x 1600 grid plus 8 of
400 x 800 (surfaceLength 40), fp64, ONE launch per step (or pair) for all sixteen, against the same members as TWO uniform ensembles
stepped one after the other (each batch timed by events and waited for before the other starts; the sum of the two).  One process:
after a warm-up, --batches batches (at least 9) per arrangement and setting, interleaved batch by batch; median, spread and the ratio
two-uniform / mixed per --steps-per-launch setting (default 1,2).  --root DIR imports crdmodel_amd from another checkout: with a build
of the parent commit (no mixed entry point) only the two uniform ensembles are timed -- the same-visit check that nothing existing moved.

    python tools/ensemble_rate.py --mixed [--batches 11] [--root ../parent-build] [--json OUT]

--own-dt measures every member at its own step size (Ensemble.step_rk4_own) against the common step, all to one fixed t1, in fp64:
16 members of the shipped FHN grid with diffusion 0.06 / 0.12 / 0.24, the --mixed members (torus 80/20 against 40/20), and 16 members
of the shipped Goldbeter grid with the ini's diffusion times 0.5 / 1 / 2.  t1 is --own-steps (default 100) steps of the member with
the largest bound.  (a) step_rk4 at the smallest member's step, t1 / max_k n_k; (b) step_rk4_own with the counts of the driver's rule,
n_k = ceil(t1 / (0.8 stable_dt_k) - 1e-12).  One process: after a warm-up, --batches batches (at least 9) of each, interleaved, every
batch from the same uploaded states and timed by events on the ensemble's stream (step_rk4_timed, step_rk4_own_timed: (b)'s time holds
its table copies between the rounds).  Reports the counts, the ratio of grid-point-steps (the arithmetic expectation) and the ratio of
the medians.  --root DIR: with a build of the parent commit only (a) is timed; --common-only times only (a) on this build too, so that
two builds run the same sequence of work when they are compared.

    python tools/ensemble_rate.py --own-dt [--batches 9] [--own-steps 100] [--common-only] [--root ../parent-build] [--json OUT]
"""
import math
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv[1:-1]:  # (before the import below: the package of another checkout)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
import crdmodel_amd as crd  # noqa: E402

INI = os.path.join(ROOT, "tests", "golden", "ini")
ROOF_BYTES_PER_S = 8.0e12
INFINITY_CACHE = 256 * 2**20


def members_of(case, n):
    model = "fhn" if case == "fhn" else "goldbeter"
    p = crd.load_ini(os.path.join(INI, "%s_shipped.ini" % case), model, "torus").params
    lo, hi = (0.9, 1.3) if case == "fhn" else (0.3, 0.75)
    out = []
    for b in np.linspace(lo, hi, n):
        q = crd._capi.Params.from_buffer_copy(p)
        q.beta, q.t_boundary = float(b), 0.0
        out.append(q)
    return out


def timed(fn, steps):
    fn(steps)  # (the caller synchronises inside fn)
    t = time.perf_counter()
    fn(steps)
    return time.perf_counter() - t


def calibrate(fn, window):
    steps = 16
    while True:
        s = timed(fn, steps)
        if s >= window or steps >= 1 << 22:
            return steps, s
        steps = int(steps * max(2.0, 1.2 * window / max(s, 1e-6)))


def measure(case, n, window, dt):
    members = members_of(case, n)
    g = crd.grid_of(members[0])
    points = g.nx * g.ny
    y0 = [crd.initial_conditions(crd.run_config(m)) for m in members]

    with crd.Ensemble(members) as e:
        for k, y in enumerate(y0):
            e.upload(k, y)

        def ens(steps):
            e.step_rk4(0.0, dt, steps, sync=True)

        ens(8)  # warm-up
        steps_e, s_e = calibrate(ens, window)

    slabs = [crd.Slab(m) for m in members]
    try:
        for s, y in zip(slabs, y0):
            s.set_stepper("fused")
            s.upload(y)
            s.plan_launches()

        def seq(steps):
            for s in slabs:
                s.step_rk4(0.0, dt, steps, sync=False)
            for s in slabs:
                s.synchronize()

        seq(8)
        steps_s, s_s = calibrate(seq, window)
        plan = slabs[0].launch_plan()
    finally:
        for s in slabs:
            s.close()
    rate_e = n * points * steps_e / s_e
    rate_s = n * points * steps_s / s_s
    return {
        "case": case, "grid": [g.nx, g.ny], "members": n, "ensemble_gpss": rate_e, "sequential_gpss": rate_s, "speedup": rate_e / rate_s,
        "ensemble_us_per_step": 1e6 * s_e / steps_e, "sequential_us_per_member_step": 1e6 * s_s / steps_s / n,
        "ensemble_roof_frac": rate_e * 32.0 / ROOF_BYTES_PER_S, "sequential_roof_frac": rate_s * 32.0 / ROOF_BYTES_PER_S,
        "in_infinity_cache": n * 2 * 16 * points <= INFINITY_CACHE, "window_s": [s_e, s_s], "steps": [steps_e, steps_s],
        "single_plan": {k: plan[k] for k in ("one_round", "xcd_mapping", "columns_per_lane", "nontemporal_stores", "steps_per_launch")},
    }


def measure_settings(case, n, precision, settings, window, batches, dt):
    members = members_of(case, n)
    for m in members:
        m.precision = crd._capi.PRECISION_F64 if precision == 64 else crd._capi.PRECISION_F32
    g = crd.grid_of(members[0])
    points = g.nx * g.ny
    real = 8 if precision == 64 else 4
    with crd.Ensemble(members) as e:
        for k, m in enumerate(members):
            e.upload(k, crd.initial_conditions(crd.run_config(m)))
        # steps per batch: an even count that fills about a tenth of the window under single steps; the warm-up fills the window
        ms = e.step_rk4_timed(0.0, dt, 16)
        ms = e.step_rk4_timed(0.0, dt, 16)
        steps = max(16, 2 * int(0.05 * window * 1e3 / max(ms / 16, 1e-6)))
        t_end = time.perf_counter() + window
        while time.perf_counter() < t_end:
            for k in settings:
                e.set_steps_per_launch(k)
                e.step_rk4_timed(0.0, dt, steps)
        us = {k: [] for k in settings}
        for _ in range(batches):
            for k in settings:
                e.set_steps_per_launch(k)
                us[k].append(1e3 * e.step_rk4_timed(0.0, dt, steps) / steps)
    row = {"case": case, "grid": [g.nx, g.ny], "precision": precision, "members": n, "steps_per_batch": steps, "batches": batches,
           "in_infinity_cache": n * 2 * 2 * real * points <= INFINITY_CACHE, "settings": {}}
    for k in settings:
        med = float(np.median(us[k]))
        row["settings"][str(k)] = {"us_per_step_median": med, "us_per_step_min": min(us[k]), "us_per_step_max": max(us[k]), "gpss": n * points / (med * 1e-6),
                                   "roof_frac_one_pass_per_step": n * points * 4 * real / (med * 1e-6) / ROOF_BYTES_PER_S}
    return row


def main_settings(a):
    settings = [int(x) for x in a.steps_per_launch.split(",")]
    if a.batches < 9:
        sys.exit("--batches: at least 9")
    rows = []
    for case in a.cases.split(","):
        dt = 0.004 if case == "fhn" else 0.002
        for n in [int(x) for x in a.members.split(",")]:
            r = measure_settings(case, n, a.precision, settings, a.window, a.batches, dt)
            rows.append(r)
            base = r["settings"][str(settings[0])]["us_per_step_median"]
            print("%-9s fp%d %4dx%-4d B=%2d  " % (case, a.precision, r["grid"][0], r["grid"][1], n) + "  ".join(
                "steps/launch %d: %8.2f us/step (%.2f .. %.2f) %.3e gpss x%.3f" % (k, q["us_per_step_median"], q["us_per_step_min"], q["us_per_step_max"], q["gpss"],
                                                                                     base / q["us_per_step_median"])
                for k, q in ((k, r["settings"][str(k)]) for k in settings)) + "  [%d batches of %d steps, %s]" % (
                    a.batches, r["steps_per_batch"], "in Infinity Cache" if r["in_infinity_cache"] else "beyond Infinity Cache"), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"device": "MI355X", "rows": rows}, f, indent=1)


def mixed_members():
    """8 members of the shipped FHN grid (400 x 1600) and 8 at surfaceLength 40 (400 x 800), one beta each."""
    p = crd.load_ini(os.path.join(INI, "fhn_shipped.ini"), "fhn", "torus").params
    out = []
    for k, b in enumerate(np.linspace(0.9, 1.3, 16)):
        q = crd._capi.Params.from_buffer_copy(p)
        q.beta, q.t_boundary = float(b), 0.0
        if k >= 8:
            q.surface_length = 40.0
        out.append(q)
    return out


def main_mixed(a):
    settings = [int(x) for x in (a.steps_per_launch or "1,2").split(",")]
    if a.batches < 9:
        sys.exit("--batches: at least 9")
    members = mixed_members()
    grids = [crd.grid_of(m) for m in members]
    assert (grids[0].nx, grids[0].ny, grids[8].nx, grids[8].ny) == (400, 1600, 400, 800), [(g.nx, g.ny) for g in grids]
    points = sum(g.nx * g.ny for g in grids)
    dt = 0.8 * min(crd.stable_dt(m) for m in members)
    y0 = [crd.initial_conditions(crd.run_config(m)) for m in members]
    has_mixed = hasattr(crd._capi.lib(), "crd_ensemble_create_mixed")
    arrangements = {"two_uniform": [crd.Ensemble(members[:8]), crd.Ensemble(members[8:])]}
    if has_mixed:
        arrangements["mixed"] = [crd.Ensemble(members, mixed=True)]
    try:
        for name, ens in arrangements.items():
            first = 0
            for e in ens:
                for k in range(len(e)):
                    e.upload(k, y0[first + k])
                first += len(e)

        def batch(name, k, steps):  # ms of `steps` steps: the ensembles of the arrangement one after the other
            ms = 0.0
            for e in arrangements[name]:
                e.set_steps_per_launch(k)
                ms += e.step_rk4_timed(0.0, dt, steps)
            return ms

        ms = batch("two_uniform", 1, 16)
        ms = batch("two_uniform", 1, 16)
        steps = max(16, 2 * int(0.05 * a.window * 1e3 / max(ms / 16, 1e-6)))
        t_end = time.perf_counter() + a.window
        while time.perf_counter() < t_end:
            for name in arrangements:
                for k in settings:
                    batch(name, k, steps)
        us = {(name, k): [] for name in arrangements for k in settings}
        for _ in range(a.batches):
            for k in settings:
                for name in arrangements:
                    us[(name, k)].append(1e3 * batch(name, k, steps) / steps)
    finally:
        for ens in arrangements.values():
            for e in ens:
                e.close()
    row = {"case": "fhn 8 x 400x1600 + 8 x 400x800", "precision": 64, "steps_per_batch": steps, "batches": a.batches, "dt": dt, "root": ROOT, "mixed_entry_point": has_mixed,
           "settings": {}}
    for k in settings:
        row["settings"][str(k)] = {}
        for name in arrangements:
            v = us[(name, k)]
            med = float(np.median(v))
            row["settings"][str(k)][name] = {"us_per_step_median": med, "us_per_step_min": min(v), "us_per_step_max": max(v), "gpss": points / (med * 1e-6)}
        q = row["settings"][str(k)]
        print("steps/launch %d:  " % k + "  ".join("%s %8.2f us/step (%.2f .. %.2f) %.3e gpss" % (name, r["us_per_step_median"], r["us_per_step_min"], r["us_per_step_max"], r["gpss"])
                                                  for name, r in q.items())
              + ("  two_uniform / mixed x%.3f" % (q["two_uniform"]["us_per_step_median"] / q["mixed"]["us_per_step_median"]) if has_mixed else "  (no mixed entry point in this build)")
              + "  [%d batches of %d steps]" % (a.batches, steps), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"device": "MI355X", "rows": [row]}, f, indent=1)


def own_dt_cases():
    """name -> (members, mixed)."""
    def scan(case, model, scale):
        p = crd.load_ini(os.path.join(INI, "%s_shipped.ini" % case), model, "torus").params
        out = []
        for k in range(16):
            q = crd._capi.Params.from_buffer_copy(p)
            q.diffusion, q.t_boundary = scale[k % 3] * (1.0 if case == "fhn" else p.diffusion), 0.0
            out.append(q)
        return out
    return {"fhn 16 x 400x1600, diffusion 0.06 / 0.12 / 0.24": (scan("fhn", "fhn", (0.06, 0.12, 0.24)), False),
            "fhn 8 x 400x1600 (torus 80/20) + 8 x 400x800 (torus 40/20)": (mixed_members(), True),
            "goldbeter 16 x 100x400, diffusion x 0.5 / 1 / 2": (scan("goldbeter", "goldbeter", (0.5, 1.0, 2.0)), False)}


def main_own_dt(a):
    if a.batches < 9:
        sys.exit("--batches: at least 9")
    has_own = hasattr(crd.Ensemble, "step_rk4_own_timed") and not a.common_only
    rows = []
    for name, (members, mixed) in own_dt_cases().items():
        bound = [0.8 * crd.stable_dt(m) for m in members]
        t1 = a.own_steps * max(bound)
        counts = [max(1, math.ceil(t1 / b - 1e-12)) for b in bound]
        points = [crd.grid_of(m).nx * crd.grid_of(m).ny for m in members]
        n_max = max(counts)
        with (crd.Ensemble(members, mixed=True) if mixed else crd.Ensemble(members)) as e:
            if hasattr(crd.Ensemble, "own_steps"):
                assert e.own_steps(0.0, t1) == counts, (e.own_steps(0.0, t1), counts)
            y0 = [crd.initial_conditions(crd.run_config(m)) for m in members]

            def reset():  # every batch from the same states: the work does not depend on the batch
                for k, y in enumerate(y0):
                    e.upload(k, y)

            arrangements = {"common": lambda: e.step_rk4_timed(0.0, t1 / n_max, n_max)}
            if has_own:
                arrangements["own"] = lambda: e.step_rk4_own_timed(0.0, t1, counts)
            t_end = time.perf_counter() + a.window
            while time.perf_counter() < t_end:
                for fn in arrangements.values():
                    reset()
                    fn()
            ms = {k: [] for k in arrangements}
            for _ in range(a.batches):
                for k, fn in arrangements.items():
                    reset()
                    ms[k].append(fn())
            finite = all(np.isfinite(v) for v in e.max_abs())
        work_common, work_own = n_max * sum(points), sum(p * n for p, n in zip(points, counts))
        row = {"case": name, "precision": 64, "t1": t1, "counts": counts, "rounds": n_max, "point_steps_common": work_common, "point_steps_own": work_own,
               "point_step_ratio": work_common / work_own, "batches": a.batches, "root": ROOT, "own_entry_point": has_own, "finite": finite, "ms": {}}
        for k, v in ms.items():
            row["ms"][k] = {"median": float(np.median(v)), "min": min(v), "max": max(v)}
        rows.append(row)
        print("%s\n   t1 = %.6g, counts %s\n   grid-point-steps: common %d, own %d, ratio x%.3f" % (name, t1, counts, work_common, work_own, row["point_step_ratio"]))
        print("   " + "  ".join("%s %.3f ms (%.3f .. %.3f)" % (k, q["median"], q["min"], q["max"]) for k, q in row["ms"].items())
              + ("  common / own x%.3f" % (row["ms"]["common"]["median"] / row["ms"]["own"]["median"]) if has_own else "  (own steps not timed)")
              + "  [%d batches, event-timed]%s" % (a.batches, "" if finite else "  NON-FINITE STATE"), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"device": "MI355X", "rows": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--members", default="1,4,16,64")
    ap.add_argument("--cases", default="fhn,goldbeter")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps-per-launch", default=None, help="e.g. 1,2: the ensemble alone under each setting, interleaved batches")
    ap.add_argument("--precision", type=int, choices=(64, 32), default=64)
    ap.add_argument("--batches", type=int, default=11)
    ap.add_argument("--mixed", action="store_true", help="a mixed-geometry ensemble against the same members as two uniform ensembles in sequence")
    ap.add_argument("--own-dt", action="store_true", help="every member at its own step size against the common step, to one fixed t1")
    ap.add_argument("--common-only", action="store_true", help="--own-dt: time the common step alone (what a build without the entry point times)")
    ap.add_argument("--own-steps", type=int, default=100, help="--own-dt: steps of the member with the largest bound to t1")
    ap.add_argument("--root", default=None, help="import crdmodel_amd from this checkout (a build of another commit)")
    a = ap.parse_args()
    if a.own_dt:
        return main_own_dt(a)
    if a.mixed:
        return main_mixed(a)
    if a.steps_per_launch:
        return main_settings(a)
    rows = []
    for case in a.cases.split(","):
        dt = 0.004 if case == "fhn" else 0.002  # (under both grids' RK4 stability bounds: 0.0052, 0.0069)
        for n in [int(x) for x in a.members.split(",")]:
            r = measure(case, n, a.window, dt)
            rows.append(r)
            print("%-9s %4dx%-4d B=%2d  ensemble %.3e gpss (%.1f us/step, %.3f of roof)  sequential %.3e gpss (%.1f us/member-step)  x%.2f  %s" % (
                case, r["grid"][0], r["grid"][1], n, r["ensemble_gpss"], r["ensemble_us_per_step"], r["ensemble_roof_frac"], r["sequential_gpss"],
                r["sequential_us_per_member_step"], r["speedup"], "in Infinity Cache" if r["in_infinity_cache"] else "beyond Infinity Cache"), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"device": "MI355X", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
