#!/usr/bin/env python3
"""What error-controlled IMEX integration (crd_integrate_imex) costs on one MI355X: the estimating last close against its bytes, and a run
at rtol = 1e-4 against RK4 at its stable step.  A sibling of tools/imex_rate.py, whose problem and yardsticks it uses.

    tools/imex_adaptive_rate.py measure > measure.txt                                        (one MI355X; host clock around calls that wait)
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/imex_adaptive_rate.py workload   (a run of its own)
    tools/imex_adaptive_rate.py report DIR >> measure.txt                                    (no GPU: reads the trace)
    -> appended to profiles/imex/rate.txt, with a reading written under it

measure: FHN torus N x N fp64 (N = 8192; env N), the reference's initial wave.  RK4 as tools/imex_rate.py measures it; then one
  crd_integrate_imex call from 0 to T (env T, default 1) at rtol = 1e-4, atol = 1e-6 with the BiCGStab solve, h0 = 0 (crd_stable_dt), its
  attempts recorded: accepted and rejected counts, the step sizes as multiples of crd_stable_dt, seconds per unit of simulated time.
workload / report: crd_integrate_imex over ATTEMPTS attempts (max_steps; the call's CRD_ESTATE is expected) under a kernel trace.  Every
  launch of crd_imex_estimate_kernel is priced at its 11 crossings (crd_imex.hip) at the copy rate (profiles/hbm_streams.json:
  copy_16B_per_lane_gbs), beside the other closes of the same trace at the crossings tools/imex_rate.py counts for ars443."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import imex_rate as base  # noqa: E402

N = base.N
T = float(os.environ.get("T", "1.0"))
ATTEMPTS = int(os.environ.get("ATTEMPTS", "4"))
RTOL, ATOL, SOLVER = 1e-4, 1e-6, "bicgstab"
ESTIMATE_CROSSINGS = 11  # R_s, k_s, y_n and seven stored vectors in; Y_s out


def measure():
    import torch

    crd, p, y0 = base.problem()
    sd = crd.stable_dt(p)
    print("# tools/imex_adaptive_rate.py measure: FHN torus %d x %d fp64, %s; crd_stable_dt = %.6g; rtol %g, atol %g, solver %s, T = %g" % (
        N, N, torch.cuda.get_device_name(0), sd, RTOL, ATOL, SOLVER, T))
    with crd.Slab(p) as s:
        s.upload(y0)
        s.plan_launches()
        s.step_rk4(0.0, sd, 30)
        s.synchronize()
        t0 = time.perf_counter()
        s.step_rk4(30 * sd, sd, base.STEPS)
        s.synchronize()
        rk4_ms = (time.perf_counter() - t0) * 1e3 / base.STEPS
        print("rk4: %.4f ms per step of crd_stable_dt: %.4g s per unit of simulated time" % (rk4_ms, rk4_ms / sd / 1e3), flush=True)
        s.upload(y0)
        t0 = time.perf_counter()
        st, hist = s.integrate_imex(0.0, T, rtol=RTOL, atol=ATOL, solver=SOLVER, history=True)
        seconds = time.perf_counter() - t0
        taken = [a.h / sd for a in hist if a.accepted]
        print("integrate_imex 0 -> %g: %d accepted, %d rejected, %.2f s: %.4g s per unit of simulated time = %.2f x RK4's" % (
            T, st.accepted, st.rejected, seconds, seconds / T, (seconds / T) / (rk4_ms / sd / 1e3)))
        print("steps as multiples of crd_stable_dt: first %.3g, smallest %.3g, largest %.3g, last full %.3g; h_next %.3g x; %.1f iterations per solve, worst residual %.2g ||r||, max |u| %.3f" % (
            taken[0], min(taken), max(taken), st.h_next / sd, st.h_next / sd, st.imex.iterations / st.imex.solves, st.imex.worst_residual, st.imex.max_abs_u))
        print("attempts (multiple of crd_stable_dt, bias x norm, accepted): " + " ".join("%.3g/%.2g/%d" % (a.h / sd, a.err, a.accepted) for a in hist), flush=True)


def workload():
    crd, p, y0 = base.problem()
    with crd.Slab(p) as s:
        s.upload(y0)
        try:
            s.integrate_imex(0.0, T, rtol=RTOL, atol=ATOL, solver=SOLVER, max_steps=ATTEMPTS)
        except crd.CrdError as e:  # max_steps attempts short of T: what this workload asks for
            print("workload: %d attempts, %d accepted" % (e.stats.attempts, e.stats.accepted), flush=True)


def report(directory):
    vector = 2.0 * N * N * 8
    copy_gbs = json.load(open(os.path.join(ROOT, "profiles", "hbm_streams.json")))["copy_16B_per_lane_gbs"]
    traces = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not traces:
        sys.exit("no *kernel_trace.csv under %s" % directory)
    rows = list(csv.DictReader(open(traces[-1])))
    key = lambda want: next(k for k in rows[0] if k.lower() == want)
    name, start, end = key("kernel_name"), key("start_timestamp"), key("end_timestamp")
    rows.sort(key=lambda r: int(r[start]))
    print("# tools/imex_adaptive_rate.py report: the closes of %d attempts of crd_integrate_imex, %d x %d fp64, from a kernel trace (rocprofv3 --kernel-trace);" % (ATTEMPTS, N, N))
    print("# crossings counted from crd_imex.hip, priced at the copy rate of %d GB/s (profiles/hbm_streams.json: copy_16B_per_lane_gbs); the first attempt is the warm-up and left out" % copy_gbs)
    table, stage, attempt = {}, 0, 0
    for r in rows:
        ms = (int(r[end]) - int(r[start])) / 1e6
        if "crd_imex_estimate_kernel" in r[name]:
            if attempt > 0:
                table.setdefault(("estimating close (stage 4)", ESTIMATE_CROSSINGS), []).append(ms)
            stage, attempt = 0, attempt + 1
        elif "crd_imex_close_kernel" in r[name]:
            if attempt > 0:
                table.setdefault(("close stage %d" % stage, base.crossings("ars443", stage)), []).append(ms)
            stage += 1
    for (label, cr), times in sorted(table.items()):
        ms = sum(times) / len(times)
        at_copy = cr * vector / (copy_gbs * 1e9) * 1e3
        print("%s: %d crossings = %.2f GB, %.3f ms (%d launches: %s): %.0f GB/s, %.2f x its time at the copy rate" % (
            label, cr, cr * vector / 1e9, ms, len(times), " ".join("%.3f" % t for t in times), cr * vector / (ms * 1e-3) / 1e9, ms / at_copy))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "measure":
        measure()
    elif len(sys.argv) == 2 and sys.argv[1] == "workload":
        workload()
    elif len(sys.argv) == 3 and sys.argv[1] == "report":
        report(sys.argv[2])
    else:
        sys.exit(__doc__)
