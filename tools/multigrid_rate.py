#!/usr/bin/env python3
"""Time of one default V-cycle of the preconditioner solve (crd_psolve_device) on device-resident AoS vectors, beside J_D v
(crd_jtimes_device, CRD_PART_DIFFUSION) measured in the same process.

    tools/multigrid_rate.py > profiles/multigrid/rate.txt        (one MI355X)

FHN torus 4096^2 and 8192^2 fp64 and 8192^2 fp32 (CASES overrides: "4096:f64,8192:f64,8192:f32").  The method is
tools/jacobian_rate.py's: a batch is BATCH calls issued back to back and ended by a synchronise of the context, the clock the host's
around it; REPEATS batches per call, the two calls in alternation; the figure is the best batch, spread = (worst - best) / best.

The cycle's compulsory traffic, counted from crd_multigrid.hip and crd_multigrid.cpp with the default options, in reals per point of the
level (an AoS vector costs 2 per point whichever field is wanted: the pairs share their cache lines):
    level 0      first sweep 2 (AoS r) + 1 (z out) + 1 (r plane out); second sweep 3 (z, r in; z out); residual + restriction 2 + 1/4
                 (the coarse right-hand side out); prolongation + correction 2 + 1/4 (the coarse correction in); third sweep 3; last sweep
                 1 (z) + 2 (AoS r) + 2 (AoS z out): 19.5
    level l > 0  first sweep 2 (its right-hand side and z are planes), second 3, residual + restriction 2 + 1/4, prolongation 2 + 1/4, two
                 sweeps 6: 15.5, on 1/4, 1/16, ... of the points: 15.5 / 3 per fine point (the coarsest level's 8 sweeps on 16 - 64 points
                 are nothing)
    together     19.5 + 15.5 / 3 = 24.67 reals per fine point: 197 B in fp64, 99 B in fp32.
That is priced at the device's measured copy rate (profiles/hbm_streams.json: copy_16B_per_lane_gbs), and the measured time is reported
as a fraction of it."""
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

BATCH, REPEATS = int(os.environ.get("BATCH", "40")), int(os.environ.get("REPEATS", "7"))
REALS_PER_POINT = 19.5 + 15.5 / 3
L = _capi.lib()


def ptr(x):
    return C.c_void_p(x.data_ptr())


def main():
    streams = json.load(open(os.path.join(ROOT, "profiles", "hbm_streams.json")))
    copy_gbs = streams["copy_16B_per_lane_gbs"]
    print("# tools/multigrid_rate.py: host clock around %d calls back to back + synchronise, best of %d alternating batches; spread = (worst - best) / best" % (BATCH, REPEATS))
    print("# %s, kernel table %s; default options (pre = post = 2, coarse = 8, omega = 0.8), gamma = 2000 x crd_stable_dt, rows free (t >= tBoundary)" % (
        torch.cuda.get_device_name(0), crd.kernel_table_digest()))
    print("# compulsory traffic of a cycle, counted from the code: %.2f reals per fine point; streaming rate: %d GB/s (profiles/hbm_streams.json: copy_16B_per_lane_gbs)" % (REALS_PER_POINT, copy_gbs))
    for spec in os.environ.get("CASES", "4096:f64,8192:f64,8192:f32").split(","):
        n, precision = int(spec.split(":")[0]), spec.split(":")[1]
        real = 8 if precision == "f64" else 4
        p = crd.make_params("fhn", "torus", n, 80.0, 20.0, 0.12, 1.25, ny=n, precision=precision)
        gamma = C.c_double(2000.0 * crd.stable_dt(p))
        dtype = torch.float64 if precision == "f64" else torch.float32
        r = torch.randn((n, n, 2), dtype=dtype, device="cuda")
        z, jv = torch.empty_like(r), torch.empty_like(r)
        torch.cuda.synchronize()
        t = C.c_double(1.0)
        with crd.Slab(p) as s:
            h = s.handle
            levels, shapes, nbytes = s.psolve_info()
            calls = [("crd_jtimes_device diffusion", lambda: L.crd_jtimes_device(h, t, _capi.PART_DIFFUSION, ptr(r), ptr(r), ptr(jv))),
                     ("crd_psolve_device", lambda: L.crd_psolve_device(h, t, gamma, None, ptr(r), ptr(z)))]
            for name, fn in calls:  # warm up every kernel, allocate the workspace
                for _ in range(5):
                    assert fn() == 0, name
            s.synchronize()
            ms = {name: [] for name, _ in calls}
            for _ in range(REPEATS):
                for name, fn in calls:
                    t0 = time.perf_counter()
                    for _ in range(BATCH):
                        fn()
                    s.synchronize()
                    ms[name].append((time.perf_counter() - t0) * 1e3 / BATCH)
            jd, cyc = min(ms["crd_jtimes_device diffusion"]), min(ms["crd_psolve_device"])
            nbytes_cycle = REALS_PER_POINT * real * n * n
            at_stream = nbytes_cycle / (copy_gbs * 1e9) * 1e3
            print("fhn %dx%d %s: %d levels (coarsest %dx%d), workspace %.0f MB" % (n, n, precision, levels, shapes[-1][0], shapes[-1][1], nbytes / 2 ** 20))
            for name in ms:
                print("fhn %dx%d %s %-28s %.4f ms per call, spread %.3f" % (n, n, precision, name, min(ms[name]), (max(ms[name]) - min(ms[name])) / min(ms[name])), flush=True)
            print("fhn %dx%d %s one V-cycle = %.2f J_D v; %.0f B per fine point -> %.3f ms at the streaming rate; measured / streaming = %.2f (%.0f GB/s on the compulsory bytes)" % (
                n, n, precision, cyc / jd, REALS_PER_POINT * real, at_stream, cyc / at_stream, nbytes_cycle / (cyc * 1e-3) / 1e9), flush=True)


if __name__ == "__main__":
    main()
