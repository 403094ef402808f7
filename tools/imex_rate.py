#!/usr/bin/env python3
"""What an IMEX step (crd_step_imex) costs on one MI355X, and where it starts to pay against the fixed-step RK4 kernel.

    tools/imex_rate.py measure [--solver gmres|bicgstab|bicgstab-warm] > measure.txt      (one MI355X; host clock around calls that wait)
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/imex_rate.py workload DIR/closes.json [SOLVER]    (a run of its own)
    tools/imex_rate.py report DIR >> measure.txt                                          (no GPU: reads the trace)
    -> profiles/imex/rate.txt, with a reading written under it

measure: FHN torus N x N fp64 (N = 8192; env N), the reference's initial wave.
  * RK4: crd_step_rk4 under the plan the context measures for itself, STEPS steps of crd_stable_dt after a warm-up, host clock + synchronise.
  * f_D: crd_rhs_part_device(CRD_PART_DIFFUSION), BATCH calls back to back + synchronise, best of REPEATS.
  * IMEX: for each multiple m of crd_stable_dt, the state uploaded again, one warm step, then IMEX_STEPS steps of ars222 (and, at one multiple,
    of euler and ars443) under the host clock (the call waits); iterations from the call's stats.  The time to a fixed T is what T / dt steps
    of that cost take -- extrapolated from IMEX_STEPS steps, not run: at the small multiples it would be minutes.
    Break-even: the multiple at which an IMEX step costs what the RK4 steps covering the same time cost.
workload / report: two steps of ars222 and of ars443 at 1000 x crd_stable_dt under a kernel trace; the stage-close launches are matched, in
  order, with the vector crossings counted from crd_imex.hip for their stage, and priced at the device's copy rate
  (profiles/hbm_streams.json: copy_16B_per_lane_gbs, the yardstick of profiles/krylov/rate.txt).  With SOLVER bicgstab or bicgstab-warm
  the same trace holds the fused kernels of crd_bicgstab.hip: the report prices each at its counted crossings beside the closes."""
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = int(os.environ.get("N", "8192"))
STEPS, BATCH, REPEATS, IMEX_STEPS = int(os.environ.get("STEPS", "600")), int(os.environ.get("BATCH", "20")), int(os.environ.get("REPEATS", "3")), int(os.environ.get("IMEX_STEPS", "3"))
MULTIPLES = [float(x) for x in os.environ.get("MULTIPLES", "50,200,500,1000,2000,4000").split(",")]
TRACE_MULTIPLE = 1000.0
STAGES = {"euler": 1, "ars222": 2, "ars443": 4}
# coefficients that are not zero, from the tableaux (crd_imex_tables.h): stored vectors the close at stage i reads besides R_i, k_i and y_n
STORED = {"euler": {}, "ars222": {1: 1}, "ars443": {1: 1, 2: 3, 3: 5}}


def crossings(scheme, stage):
    """Vector crossings of the close at `stage`, counted from the loop of crd_imex_close_kernel: reads + writes."""
    s = STAGES[scheme]
    if stage == 0:
        return 1 + 2  # y_n in; FR_0 and R_1 out
    if stage == s:
        return 2 + 1  # R_s and k_s in; Y_s out
    return 3 + STORED[scheme][stage] + 2  # R_i, k_i, y_n and the row's stored vectors in; FR_i and R_{i+1} out


def problem():
    import crdmodel_amd as crd

    p = crd.make_params("fhn", "torus", N, 80.0, 20.0, 0.12, 1.25, ny=N, precision="f64")
    y0 = crd.initial_conditions(crd.run_config(p, wave_length=0.1, wave_width=0.5, wave_inside=0))
    return crd, p, y0


def measure(solver="gmres"):
    import torch

    crd, p, y0 = problem()
    from crdmodel_amd import _capi

    L = _capi.lib()
    sd = crd.stable_dt(p)
    vector = 2.0 * N * N * 8
    copy_gbs = json.load(open(os.path.join(ROOT, "profiles", "hbm_streams.json")))["copy_16B_per_lane_gbs"]
    print("# tools/imex_rate.py measure --solver %s: FHN torus %d x %d fp64, %s, kernel table %s; crd_stable_dt = %.6g; vector %.0f MB" % (solver, N, N, torch.cuda.get_device_name(0), crd.kernel_table_digest(), sd, vector / 2 ** 20))
    with crd.Slab(p) as s:
        s.upload(y0)
        s.plan_launches()
        s.step_rk4(0.0, sd, 30)
        s.synchronize()
        t0 = time.perf_counter()
        s.step_rk4(30 * sd, sd, STEPS)
        s.synchronize()
        rk4_ms = (time.perf_counter() - t0) * 1e3 / STEPS
        plan = s.launch_plan()
        print("rk4: %.4f ms per step of crd_stable_dt (%d steps, %d steps per launch): %.4g ms per unit of simulated time" % (rk4_ms, STEPS, plan["steps_per_launch"], rk4_ms / sd), flush=True)
        print("imex workspace: ars222 %.0f MB, ars443 %.0f MB (the solve's %.0f MB included)" % (s.imex_info("ars222", solver=solver) / 2 ** 20, s.imex_info("ars443", solver=solver) / 2 ** 20, (s.lsolve_info() if solver == "gmres" else s.lsolve_bicgstab_info()) / 2 ** 20))
        r = torch.randn((N, N, 2), dtype=torch.float64, device="cuda")
        out = torch.empty_like(r)
        best = []
        for _ in range(REPEATS):
            s.synchronize()
            t0 = time.perf_counter()
            for _ in range(BATCH):
                assert L.crd_rhs_part_device(s.handle, 1.0, _capi.PART_DIFFUSION, C.c_void_p(r.data_ptr()), C.c_void_p(out.data_ptr())) == 0
            s.synchronize()
            best.append((time.perf_counter() - t0) * 1e3 / BATCH)
        fd_ms = min(best)
        del r, out
        torch.cuda.empty_cache()
        print("f_D: %.4f ms per call (2 crossings = %.2f GB: %.2f x their time at the copy rate of %d GB/s)" % (fd_ms, 2 * vector / 1e9, fd_ms / (2 * vector / (copy_gbs * 1e9) * 1e3), copy_gbs), flush=True)
        rows = []
        for scheme, multiples in (("ars222", MULTIPLES), ("euler", [TRACE_MULTIPLE]), ("ars443", [TRACE_MULTIPLE])):
            for m in multiples:
                dt = m * sd
                s.upload(y0)
                s.step_imex(0.0, dt, 1, scheme, solver=solver)
                t0 = time.perf_counter()
                st = s.step_imex(dt, dt, IMEX_STEPS, scheme, solver=solver)
                ms = (time.perf_counter() - t0) * 1e3 / IMEX_STEPS
                per_time = ms / dt
                rows.append((scheme, m, ms, per_time))
                print("imex %s (%s) at %g x crd_stable_dt (dt = %.4g): %.1f ms per step, %.1f iterations per solve (most %d), worst residual %.2g ||r||, max |u| %.3f; f_D %.1f ms of it; "
                      "%.4g ms per unit of simulated time = %.2f x RK4's" % (scheme, solver, m, dt, ms, st.iterations / st.solves, st.max_iterations, st.worst_residual, st.max_abs_u, STAGES[scheme] * fd_ms,
                                                                             per_time, per_time / (rk4_ms / sd)), flush=True)
        T = 4000 * sd
        print("time to T = 4000 x crd_stable_dt = %.4g (IMEX: T / dt steps at the measured cost of a step, extrapolated): RK4 %.1f ms; ars222 %s" % (
            T, 4000 * rk4_ms, ", ".join("%g x: %.1f ms" % (m, T / (m * sd) * ms) for sch, m, ms, _ in rows if sch == "ars222")))
        even = None
        ars = [(m, ms) for sch, m, ms, _ in rows if sch == "ars222"]
        for (m0, a0), (m1, a1) in zip(ars, ars[1:]):
            # cost ratio against RK4 over the same time: ms / (m rk4_ms); linear in between
            q0, q1 = a0 / (m0 * rk4_ms), a1 / (m1 * rk4_ms)
            if q0 > 1 >= q1:
                even = m0 + (m1 - m0) * (q0 - 1) / (q0 - q1)
        print("break-even (ars222, %s, against RK4 at crd_stable_dt): %s" % (solver, "%.0f x crd_stable_dt (interpolated between the two multiples around it)" % even if even else
                                                                        ("below %g x" % ars[0][0] if ars[0][1] / (ars[0][0] * rk4_ms) <= 1 else "not reached up to %g x" % ars[-1][0])))


# vector crossings of the kernels of crd_bicgstab.hip, counted from their loops: reads + writes (start: r in, res, rhat, p out -- or r, x,
# J x in and one out with a guess and for the true residual: 4 either way)
BCG_CROSSINGS = {"crd_bcg_apply_dot_kernel": 4, "crd_bcg_s_update_kernel": 3, "crd_bcg_xr_update_kernel": 8, "crd_bcg_p_update_kernel": 4, "crd_bcg_x_half_kernel": 3,
                 "crd_bcg_start_kernel": 4}


def workload(sidecar, solver="gmres"):
    crd, p, y0 = problem()
    sd = crd.stable_dt(p)
    closes = []
    with crd.Slab(p) as s:
        for scheme in ("ars222", "ars443"):
            dt = TRACE_MULTIPLE * sd
            s.upload(y0)
            for call, steps in ((0, 1), (1, 2)):  # a warm step, then the two that count
                st = s.step_imex(call * dt, dt, steps, scheme, solver=solver)
                for _ in range(steps):
                    closes += [dict(scheme=scheme, stage=i, crossings=crossings(scheme, i), warm=call == 0) for i in range(STAGES[scheme] + 1)]
            print("workload %s: %d iterations in %d solves" % (scheme, st.iterations, st.solves), flush=True)
    json.dump(dict(n=N, solver=solver, closes=closes), open(sidecar, "w"))


def report(directory):
    side = json.load(open(os.path.join(directory, "closes.json")))
    n, closes = side["n"], side["closes"]
    vector = 2.0 * n * n * 8
    copy_gbs = json.load(open(os.path.join(ROOT, "profiles", "hbm_streams.json")))["copy_16B_per_lane_gbs"]
    traces = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not traces:
        sys.exit("no *kernel_trace.csv under %s" % directory)
    rows = list(csv.DictReader(open(traces[-1])))
    key = lambda want: next(k for k in rows[0] if k.lower() == want)
    name, start, end = key("kernel_name"), key("start_timestamp"), key("end_timestamp")
    rows.sort(key=lambda r: int(r[start]))
    got = [(r[name], (int(r[end]) - int(r[start])) / 1e6) for r in rows if "crd_imex_close_kernel" in r[name]]
    if len(got) != len(closes):
        sys.exit("%d stage-close launches in the trace, %d expected" % (len(got), len(closes)))
    print("# tools/imex_rate.py report: the stage-close launches of two steps of ars222 and of ars443 at %g x crd_stable_dt, %d x %d fp64, from a kernel trace (rocprofv3 --kernel-trace);" % (TRACE_MULTIPLE, n, n))
    print("# crossings counted from crd_imex.hip, priced at the copy rate of %d GB/s (profiles/hbm_streams.json: copy_16B_per_lane_gbs)" % copy_gbs)
    table = {}
    for (kernel, ms), c in zip(got, closes):
        assert ("true>" in kernel or "Lb1" in kernel) == (c["stage"] == STAGES[c["scheme"]]), (kernel, c)  # the LAST instantiation closes the last stage
        if not c["warm"]:
            table.setdefault((c["scheme"], c["stage"], c["crossings"]), []).append(ms)
    total = {}
    for (scheme, stage, cr), times in sorted(table.items()):
        ms = sum(times) / len(times)
        at_copy = cr * vector / (copy_gbs * 1e9) * 1e3
        total[scheme] = total.get(scheme, 0.0) + ms
        print("close %s stage %d: %d crossings = %.2f GB, %.3f ms (%d launches: %s): %.0f GB/s, %.2f x its time at the copy rate" % (
            scheme, stage, cr, cr * vector / 1e9, ms, len(times), " ".join("%.3f" % t for t in times), cr * vector / (ms * 1e-3) / 1e9, ms / at_copy))
    for scheme, ms in sorted(total.items()):
        print("closes of one %s step: %.3f ms" % (scheme, ms))
    # the kernels of crd_bicgstab.hip, each launch attributed to the stage whose close follows it (the sidecar's list, in order): the
    # launches of the warm-up steps are left out exactly as their closes are
    import re

    bcg, at = {}, 0
    for r in rows:
        if "crd_imex_close_kernel" in r[name]:
            at += 1
            continue
        kernel = next((k for k in BCG_CROSSINGS if k in r[name]), None)
        if kernel is None or at >= len(closes) or closes[at]["warm"]:
            continue
        label, cr = kernel, BCG_CROSSINGS[kernel]
        if kernel == "crd_bcg_apply_dot_kernel":
            m = re.search(r"crd_bcg_apply_dot_kernel<\w+, *(true|false)>|crd_bcg_apply_dot_kernelI[df]Lb([01])E", r[name])
            if not m:
                sys.exit("cannot tell the one-dot from the two-dot apply kernel in %r" % r[name])
            label += " (two dots)" if (m.group(1) == "true" or m.group(2) == "1") else " (one dot)"
        if kernel == "crd_bcg_start_kernel" and side.get("solver") != "bicgstab":
            cr = 0  # with a guess the first start of a solve reads three vectors, not one: not priced here
        bcg.setdefault((label, cr), []).append((int(r[end]) - int(r[start])) / 1e6)
    for (kernel, cr), times in sorted(bcg.items()):
        ms = sum(times) / len(times)
        if cr == 0:
            print("bicgstab %s: %.3f ms (mean of %d launches), not priced" % (kernel, ms, len(times)))
            continue
        at_copy = cr * vector / (copy_gbs * 1e9) * 1e3
        print("bicgstab %s: %d crossings = %.2f GB, %.3f ms (mean of %d launches, %.3f .. %.3f): %.0f GB/s, %.2f x its time at the copy rate" % (
            kernel, cr, cr * vector / 1e9, ms, len(times), min(times), max(times), cr * vector / (ms * 1e-3) / 1e9, ms / at_copy))
    timed = [r for r in rows if "crd_imex" not in r[name]]
    print("# the other %d launches of the trace (f_D, and the solves' J_D v, cycles and vector kernels) took %.1f ms in all, warm steps included" % (len(timed), sum((int(r[end]) - int(r[start])) / 1e6 for r in timed)))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "measure" and sys.argv[2] == "--solver" and sys.argv[3] in ("gmres", "bicgstab", "bicgstab-warm"):
        measure(sys.argv[3])
    elif len(sys.argv) == 2 and sys.argv[1] == "measure":
        measure()
    elif len(sys.argv) in (3, 4) and sys.argv[1] == "workload":
        workload(sys.argv[2], *sys.argv[3:])
    elif len(sys.argv) == 3 and sys.argv[1] == "report":
        report(sys.argv[2])
    else:
        sys.exit(__doc__)
