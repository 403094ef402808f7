#!/usr/bin/env python3
"""Interleaved A/B of several builds of libcrd on one box with PINNED launch plans: one worker process per library holds the state
(CRD_LIBRARY selects the build), and per round every plan is pinned in turn, the workers taking turns plan by plan -- 9 untimed steps,
AB_STEPS (198) timed ones (crd_step_rk4_timed).  AB_PREHEAT (2) rounds are thrown away, AB_ROUNDS (7) counted.  The first two
libraries are the SAME build twice (the parent's): what they differ by is the session's noise.  spread = the largest
|parentA - parentB| of medians over the plans of a size; the bar for every other library: faster than the mean of the two parents by
more than 3 x the mean |parentA - parentB| of the rounds, and below BOTH parents in every round.  After the rounds every worker steps
19 times from the initial state under the first plan and prints the digest of the result: builds that compute the same bits print the
same digest.  The A/B records of profiles/r11 are runs of this script.

    AB_LIBS="parentA=tools/_variants/libcrd_parent.so;parentB=tools/_variants/libcrd_parent.so;tree=crdmodel_amd/libcrd.so" \\
    AB_CASES="8192:8192:3,1,1,1,3+1,1,1,1,3;4096:4096:1,1,1,1,3" python3 tools/ab_workers.py

A worker that dies ends the run at once (exit status 1): nothing more is started on the device."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = r'''
import hashlib, os, sys
sys.path.insert(0, %r)
import numpy as np
import crdmodel_amd as crd
slab = None
for line in sys.stdin:
    cmd = line.split()
    if cmd[0] == "case":
        if slab is not None:
            slab.close()
        p = crd.make_params("fhn", "torus", int(cmd[1]), 80.0, 20.0, 0.12, 1.25, ny=int(cmd[2]), precision="f64")
        dt = 0.8 * crd.stable_dt(p)
        y0 = crd.initial_conditions(crd.run_config(p, wave_length=0.1, wave_width=0.5))
        slab = crd.Slab(p)
        slab.set_stepper("fused")
        slab.upload(y0)
        print("ok", flush=True)
    elif cmd[0] == "time":
        slab.set_launch_plan(*[int(v) for v in cmd[1].split(",")])
        slab.step_rk4(0.0, dt, 9)
        ms, _, _ = slab.step_rk4_timed(0.0, dt, int(cmd[2]))
        print("%%.6f" %% (ms / int(cmd[2])), flush=True)
    elif cmd[0] == "sha":
        slab.upload(y0)
        slab.set_launch_plan(*[int(v) for v in cmd[1].split(",")])
        slab.step_rk4(0.0, dt, 19)
        print(hashlib.sha256(np.ascontiguousarray(slab.download()).tobytes()).hexdigest()[:16], flush=True)
''' % ROOT


def main():
    libs = [kv.split("=", 1) for kv in os.environ["AB_LIBS"].split(";") if kv]
    cases = [c.split(":") for c in os.environ.get("AB_CASES", "8192:8192:3,1,1,1,3+1,1,1,1,3").split(";") if c]
    rounds, preheat, steps = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_PREHEAT", "2")), int(os.environ.get("AB_STEPS", "198"))
    assert len(libs) >= 3 and len(libs) <= 12, "parentA, parentB and at least one build to judge"
    workers = {}
    for name, path in libs:
        workers[name] = subprocess.Popen([sys.executable, "-c", WORKER], env=dict(os.environ, CRD_LIBRARY=os.path.join(ROOT, path)), stdin=subprocess.PIPE,
                                         stdout=subprocess.PIPE, text=True)

    def ask(name, line):
        w = workers[name]
        w.stdin.write(line + "\n")
        w.stdin.flush()
        answer = w.stdout.readline().strip()
        if not answer:  # the worker died: stop everything, start nothing more
            print("worker %s ended (exit status %r) at %r" % (name, w.poll(), line), flush=True)
            for v in workers.values():
                v.stdin.close()
            for v in workers.values():
                try:
                    v.wait(timeout=30)
                except subprocess.TimeoutExpired:
                    v.kill()
            sys.exit(1)
        return answer

    pa, pb = libs[0][0], libs[1][0]
    raw = []
    for nx, ny, plans in cases:
        plans = plans.split("+")
        for name, _ in libs:
            ask(name, "case %s %s" % (nx, ny))
        res = {(name, pl): [] for name, _ in libs for pl in plans}
        for r in range(-preheat, rounds):
            for pl in plans:
                for name, _ in libs:
                    t = float(ask(name, "time %s %d" % (pl, steps)))
                    if r >= 0:
                        res[(name, pl)].append(t)
                        raw.append("%sx%s round %d %-8s %s %.4f" % (nx, ny, r, name, pl, t))
        med = {k: statistics.median(v) for k, v in res.items()}
        spread = max(abs(med[(pa, pl)] - med[(pb, pl)]) for pl in plans)
        print("--- %sx%s fp64 FHN, ms per step, %d rounds of %d steps, interleaved; spread (largest |%s - %s| of medians) %.4f ---" % (nx, ny, rounds, steps, pa, pb, spread))
        for pl in plans:
            for name in (pa, pb):
                print("  %-8s %s median %.4f  min %.4f  max %.4f" % (name, pl, med[(name, pl)], min(res[(name, pl)]), max(res[(name, pl)])))
            a, b = res[(pa, pl)], res[(pb, pl)]
            noise = statistics.mean(abs(x - y) for x, y in zip(a, b))
            for name, _ in libs[2:]:
                t = res[(name, pl)]
                gain = statistics.mean((x + y) / 2 - z for x, y, z in zip(a, b, t))
                below = all(z < min(x, y) for x, y, z in zip(a, b, t))
                above = all(z > max(x, y) for x, y, z in zip(a, b, t))
                parent = (med[(pa, pl)] + med[(pb, pl)]) / 2
                print("  %-8s %s median %.4f  parent %.4f  diff %+.4f (%+.2f %%)  mean gain %.4f  3 x mean |%s - %s| %.4f  below BOTH parents every round: %s  above both every round: %s  "
                      "faster beyond the bar: %s" % (name, pl, med[(name, pl)], parent, med[(name, pl)] - parent, 100 * (med[(name, pl)] - parent) / parent, gain, pa, pb, 3 * noise, below,
                                                     above, below and gain >= 3 * noise))
        for name, _ in libs:
            print("%sx%s sha after 19 steps under %s: %-8s %s" % (nx, ny, plans[0], name, ask(name, "sha %s" % plans[0])))
        print(flush=True)
    for w in workers.values():
        w.stdin.close()
    for w in workers.values():
        w.wait(timeout=60)
    print("raw rounds")
    print("\n".join(raw))


if __name__ == "__main__":
    main()
