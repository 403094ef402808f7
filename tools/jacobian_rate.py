#!/usr/bin/env python3
"""Rates of the split right-hand side and of J v on device-resident AoS vectors, beside crd_rhs_device's measured in the same process.

    tools/jacobian_rate.py > profiles/jacobian/rate.txt        (one MI355X)

FHN 8192^2 fp64 and Goldbeter 4096^2 fp64 (CASES overrides: "fhn:8192,goldbeter:4096").  A batch is BATCH calls issued back to back
and ended by a synchronise of the context; the clock is the host's around it (the calls run on the context's own stream, whose handle
the ABI does not export, so a device event pair cannot be put around them from outside; at 0.2 - 0.6 ms per call a batch is tens to
hundreds of milliseconds against a few microseconds of synchronise).  REPEATS batches per call, the calls in alternation so that
drift hits each alike; the figure is the best batch, and spread = (worst - best) / best of a call's batches is printed beside it.
Each call is priced by its own compulsory bytes per point in fp64 -- 32 B where one vector is read and one written (crd_rhs_device,
the parts, and J_D v, which does not read y), 48 B where y, v and Jv all move -- and reported as a fraction of 8 TB/s beside
crd_rhs_device's fraction of the same run."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device memory for the caller's vectors)

import crdmodel_amd as crd  # noqa: E402
from crdmodel_amd import _capi  # noqa: E402

PEAK = 8e12
BATCH, REPEATS = int(os.environ.get("BATCH", "200")), int(os.environ.get("REPEATS", "7"))
L = _capi.lib()


def ptr(x):
    return C.c_void_p(x.data_ptr())


def main():
    print("# tools/jacobian_rate.py: host clock around %d calls back to back + synchronise, best of %d alternating batches; spread = (worst - best) / best" % (BATCH, REPEATS))
    print("# %s, kernel table %s" % (torch.cuda.get_device_name(0), crd.kernel_table_digest()))
    for spec in os.environ.get("CASES", "fhn:8192,goldbeter:4096").split(","):
        model, n = spec.split(":")[0], int(spec.split(":")[1])
        p = crd.make_params(model, "torus", n, 80.0, 20.0, 0.12, 1.25 if model == "fhn" else 0.4, ny=n)
        y = torch.from_numpy(crd.initial_conditions(crd.run_config(p))).cuda()
        v, out = torch.randn_like(y), torch.empty_like(y)
        torch.cuda.synchronize()
        t = C.c_double(1.0)
        with crd.Slab(p) as s:
            h = s.handle
            calls = [("crd_rhs_device", 32, lambda: L.crd_rhs_device(h, t, ptr(y), ptr(out)))]
            for name, part in (("diffusion", 1), ("reaction", 2)):
                calls.append(("crd_rhs_part_device " + name, 32, lambda part=part: L.crd_rhs_part_device(h, t, part, ptr(y), ptr(out))))
            for name, part, nbytes in (("full", 0, 48), ("diffusion", 1, 32), ("reaction", 2, 48)):
                calls.append(("crd_jtimes_device " + name, nbytes, lambda part=part: L.crd_jtimes_device(h, t, part, ptr(y), ptr(v), ptr(out))))
            for name, _, fn in calls:  # warm up every kernel
                for _ in range(10):
                    assert fn() == 0, name
            s.synchronize()
            ms = {name: [] for name, _, _ in calls}
            for _ in range(REPEATS):
                for name, _, fn in calls:
                    t0 = time.perf_counter()
                    for _ in range(BATCH):
                        fn()
                    s.synchronize()
                    ms[name].append((time.perf_counter() - t0) * 1e3 / BATCH)
            cached = 16 * n * n <= 2 * (256 << 20)
            if cached:
                print("# %dx%d: a vector is %d MB; unchanged inputs stay in the 256 MB memory-side cache between calls -- rates here are not HBM figures" % (n, n, 16 * n * n >> 20))
            base = None
            for name, nbytes, _ in calls:
                best, worst = min(ms[name]), max(ms[name])
                frac = nbytes * n * n / (best * 1e-3) / PEAK
                base = frac if base is None else base
                print("%s %dx%d fp64 %-30s %.4f ms per call, spread %.3f, %5.0f GB/s on %d B per point = %.3f of 8 TB/s (crd_rhs_device in this run: %.3f)" % (
                    model, n, n, name, best, (worst - best) / best, nbytes * n * n / (best * 1e-3) / 1e9, nbytes, frac, base), flush=True)


if __name__ == "__main__":
    main()
