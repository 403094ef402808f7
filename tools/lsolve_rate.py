#!/usr/bin/env python3
"""Time of one inner iteration of the linear solve (crd_lsolve_device: restarted GMRES on the device) at three depths of the basis, beside
J_D v and one V-cycle measured in the same process, and the same system solved the only way the tree could before: scipy's gmres with
the matvec and the cycle on the device and every vector through the host.

    tools/lsolve_rate.py > profiles/krylov/rate.txt        (one MI355X)
    tools/lsolve_rate.py --solver both >> profiles/krylov/rate.txt     (the same, and BiCGStab on the same system in the same process)

--solver gmres (the default) | bicgstab | both.  BiCGStab (crd_bicgstab_device) is timed the same way: one iteration -- two J_D v, two
cycles, the five fused kernels and four reads of the host -- as T(k + 1) - T(k) at rtol = 0, and a whole solve at rtol 1e-8 (fp32: 1e-5).
Its fused kernels move 23 vector crossings per iteration (crd_bicgstab.hip).

FHN torus 8192^2 fp64 and fp32 and 4096^2 fp64 (CASES overrides: "8192:f64,8192:f32,4096:f64"), gamma = 2000 x crd_stable_dt, rows free,
restart 30.  Inner iteration j (the basis holds j + 1 vectors) is timed as T(j + 1) - T(j), T(k) the host's clock around one
crd_lsolve_device call with rtol = 0 and max_iters = k (the call waits for the stream): the call's fixed part -- ||r||, the first
vector, the cycle's closing M -- cancels, one vector more in the closing combine does not (one crossing).  Best of REPEATS calls.  The
iteration is split into J_D v and the cycle, each timed through its own entry point as tools/multigrid_rate.py does, and the rest: the four
orthogonalisation launches with their two partial sums, apply and scale, and the host's read of the column -- not separated further here
(that takes a kernel trace).

Bytes of that rest, in vector crossings counted from crd_krylov.hip, c = j + 1: multi-dot c + ceil(c / 8), update c + 2, both twice; apply
3; scale 2:  2 (2 c + ceil(c / 8) + 2) + 5.  Priced at the device's copy rate (profiles/hbm_streams.json: copy_16B_per_lane_gbs, the rate
profiles/multigrid/rate.txt quotes)."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (device memory for the caller's vectors)

import crdmodel_amd as crd  # noqa: E402
from crdmodel_amd import _capi  # noqa: E402

BATCH, REPEATS = int(os.environ.get("BATCH", "20")), int(os.environ.get("REPEATS", "3"))
DEPTHS = (1, 10, 29)
L = _capi.lib()


def ptr(x):
    return C.c_void_p(x.data_ptr())


def crossings(j):
    c = j + 1
    return 2 * (2 * c + -(-c // 8) + 2) + 5


def scipy_solve(s, t, gamma, r, rtol):
    """(seconds, iterations) of scipy gmres(restart 30) on the same system: matvec and cycle on the device, vectors through the host."""
    import numpy as np
    from scipy.sparse.linalg import LinearOperator, gmres

    shape, n, count = r.shape, r.size, [0]
    A = LinearOperator((n, n), matvec=lambda x: x - gamma * s.jtimes(t, x.reshape(shape), x.reshape(shape), "diffusion").ravel(), dtype=r.dtype)
    M = LinearOperator((n, n), matvec=lambda x: s.psolve(t, gamma, x.reshape(shape)).ravel(), dtype=r.dtype)

    def tick(_):
        count[0] += 1
        print("# scipy iteration %d" % count[0], flush=True)

    t0 = time.perf_counter()
    x, info = gmres(A, r.ravel(), M=M, rtol=rtol, atol=0.0, restart=30, maxiter=4, callback=tick, callback_type="pr_norm")
    dt = time.perf_counter() - t0
    res = float(np.linalg.norm(A.matvec(x) - r.ravel()) / np.linalg.norm(r))
    return dt, count[0], info, res


def bicgstab_rate(s, n, precision, t, gamma, r, z, parts, vector, copy_gbs):
    """One BiCGStab iteration at three depths (they cost the same: there is no basis) and a whole solve, on the system GMRES was given."""
    h = s.handle
    opt, st = crd.Slab._bicgstab_options(rtol=0.0, max_iters=1), _capi.BicgstabStats()

    def solve(k, rtol=0.0):
        opt.max_iters, opt.rtol = k, rtol
        t0 = time.perf_counter()
        assert L.crd_bicgstab_device(h, t, gamma, C.byref(opt), None, ptr(r), ptr(z), C.byref(st)) == 0
        return (time.perf_counter() - t0) * 1e3

    solve(2)
    print("fhn %dx%d %s bicgstab workspace %.0f MB (lsolve: %.0f MB)" % (n, n, precision, s.lsolve_bicgstab_info() / 2 ** 20, s.lsolve_info() / 2 ** 20), flush=True)
    for k in (1, 5, 10):
        lo, hi = min(solve(k) for _ in range(REPEATS)), min(solve(k + 1) for _ in range(REPEATS))
        assert st.iterations == k + 1 and st.breakdown == 0
        it = hi - lo
        rest = it - 2 * parts["J_D v"] - 2 * parts["V-cycle"]
        nbytes = 23 * vector
        print("fhn %dx%d %s bicgstab iteration %2d: %.3f ms = 2 J_D v %.3f + 2 V-cycles %.3f + the fused kernels and the host's four reads %.3f ms; those move 23 vectors = %.2f GB: %.0f GB/s, "
              "%.2f x their time at the copy rate" % (n, n, precision, k + 1, it, 2 * parts["J_D v"], 2 * parts["V-cycle"], rest, nbytes / 1e9, nbytes / (rest * 1e-3) / 1e9,
                                                 rest / (nbytes / (copy_gbs * 1e9) * 1e3)), flush=True)
    rtol = 1e-8 if precision == "f64" else 1e-5
    ms = min(solve(200, rtol) for _ in range(REPEATS))
    halves = 2 * st.iterations - st.half_exit
    print("fhn %dx%d %s bicgstab solve to rtol %g: %d iterations (%d half-steps, %d matvecs, %d cycles), %.1f ms on the device = %.2f ms per iteration (converged %d, breakdown %d, "
          "recurrence residual %.3g ||r||, true residual %.3g ||r||)" % (n, n, precision, rtol, st.iterations, halves, st.matvecs, st.psolves, ms, ms / max(st.iterations, 1), st.converged,
                                                                         st.breakdown, st.res_norm / st.r_norm, st.true_res_norm / st.r_norm), flush=True)


def main():
    solver = sys.argv[sys.argv.index("--solver") + 1] if "--solver" in sys.argv else "gmres"
    if solver not in ("gmres", "bicgstab", "both"):
        sys.exit("--solver takes gmres, bicgstab or both")
    copy_gbs = json.load(open(os.path.join(ROOT, "profiles", "hbm_streams.json")))["copy_16B_per_lane_gbs"]
    print("# tools/lsolve_rate.py: inner iteration j = T(j + 1) - T(j), T(k) the host clock around crd_lsolve_device(rtol 0, max_iters k), best of %d; J_D v and the cycle:" % REPEATS)
    print("# %d calls back to back + synchronise, best of %d batches.  %s, kernel table %s" % (BATCH, REPEATS, torch.cuda.get_device_name(0), crd.kernel_table_digest()))
    print("# FHN torus, gamma = 2000 x crd_stable_dt, rows free, restart 30, default cycle; copy rate %d GB/s (profiles/hbm_streams.json: copy_16B_per_lane_gbs)" % copy_gbs)
    scipy_cases = os.environ.get("SCIPY_CASES", "4096:f64").split(",")
    for spec in os.environ.get("CASES", "8192:f64,8192:f32,4096:f64").split(","):
        n, precision = int(spec.split(":")[0]), spec.split(":")[1]
        real = 8 if precision == "f64" else 4
        p = crd.make_params("fhn", "torus", n, 80.0, 20.0, 0.12, 1.25, ny=n, precision=precision)
        gamma_f = 2000.0 * crd.stable_dt(p)
        gamma, t = C.c_double(gamma_f), C.c_double(1.0)
        dtype = torch.float64 if precision == "f64" else torch.float32
        torch.manual_seed(5)
        r = torch.randn((n, n, 2), dtype=dtype, device="cuda")
        z, jv = torch.empty_like(r), torch.empty_like(r)
        torch.cuda.synchronize()
        vector = 2.0 * n * n * real
        with crd.Slab(p) as s:
            h = s.handle
            opt, st = crd.Slab._lsolve_options(rtol=0.0, max_iters=1), _capi.LsolveStats()
            print("fhn %dx%d %s: vector %.0f MB, lsolve workspace %.0f MB, psolve workspace %.0f MB" % (n, n, precision, vector / 2 ** 20, s.lsolve_info() / 2 ** 20, s.psolve_info()[2] / 2 ** 20), flush=True)

            def solve(k, rtol=0.0):
                opt.max_iters, opt.rtol = k, rtol
                t0 = time.perf_counter()
                assert L.crd_lsolve_device(h, t, gamma, C.byref(opt), None, ptr(r), ptr(z), C.byref(st)) == 0
                return (time.perf_counter() - t0) * 1e3

            solve(2)  # allocate, warm every kernel up
            parts = {}
            for name, fn in (("J_D v", lambda: L.crd_jtimes_device(h, t, _capi.PART_DIFFUSION, ptr(r), ptr(r), ptr(jv))), ("V-cycle", lambda: L.crd_psolve_device(h, t, gamma, None, ptr(r), ptr(jv)))):
                best = []
                for _ in range(REPEATS):
                    s.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(BATCH):
                        fn()
                    s.synchronize()
                    best.append((time.perf_counter() - t0) * 1e3 / BATCH)
                parts[name] = min(best)
            print("fhn %dx%d %s J_D v %.4f ms, V-cycle %.4f ms" % (n, n, precision, parts["J_D v"], parts["V-cycle"]), flush=True)
            for j in DEPTHS if solver != "bicgstab" else ():
                lo, hi = min(solve(j) for _ in range(REPEATS)), min(solve(j + 1) for _ in range(REPEATS))
                assert st.iterations == j + 1 and st.restarts == 0
                it = hi - lo
                rest = it - parts["J_D v"] - parts["V-cycle"]
                nbytes = crossings(j) * vector
                print("fhn %dx%d %s j = %2d: iteration %.3f ms = J_D v %.3f + V-cycle %.3f + orthogonalisation, apply, scale and the host's read %.3f ms; those move %d vectors = %.2f GB: %.0f GB/s, "
                      "%.2f x their time at the copy rate" % (n, n, precision, j, it, parts["J_D v"], parts["V-cycle"], rest, crossings(j), nbytes / 1e9, nbytes / (rest * 1e-3) / 1e9,
                                                         rest / (nbytes / (copy_gbs * 1e9) * 1e3)), flush=True)
            # a whole solve at rtol 1e-8 (fp32: 1e-5), on the device and (where asked) through scipy
            rtol = 1e-8 if precision == "f64" else 1e-5
            ms = min(solve(200, rtol) for _ in range(REPEATS))
            print("fhn %dx%d %s solve to rtol %g: %d iterations, %.1f ms on the device = %.2f ms per iteration (converged %d, residual %.3g ||r||)" % (n, n, precision, rtol, st.iterations, ms, ms / max(st.iterations, 1), st.converged, st.res_norm / st.r_norm), flush=True)
            if solver != "gmres":
                bicgstab_rate(s, n, precision, t, gamma, r, z, parts, vector, copy_gbs)
            if spec in scipy_cases:
                sec, its, info, res = scipy_solve(s, 1.0, gamma_f, r.cpu().numpy(), rtol)
                print("fhn %dx%d %s the same system through scipy gmres (matvec and cycle on the device, vectors through the host): %d iterations, %.1f ms (info %d, residual %.3g ||r||): "
                      "%.0f x the device solve" % (n, n, precision, its, sec * 1e3, info, res, sec * 1e3 / ms), flush=True)
        del r, z, jv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
