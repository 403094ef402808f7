"""CPU-side checks of ensembles with every member at its own step size: the entry points in the header and the ctypes table, compiled
and linked from plain C; what crd_run --ensemble-own-dt refuses before any device is asked for; the new kernels' registers against the
step kernels' in profiles/ensemble/kernel_resources.txt.  No kernel is launched.  (crd_ensemble_own_steps needs an ensemble, and an
ensemble a device: its rule is checked in tests/test_gpu_ensemble_own.py against crd.stable_dt.)"""
import ctypes as C
import os
import re
import subprocess

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
SMALL_INI = os.path.join(GOLDEN, "ini", "small_run.ini")
HEADER = os.path.join(ROOT, "include", "crd.h")


def test_entry_points_in_header_and_ctypes_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+crd_ensemble_step_rk4_own\s*\(\s*crd_ensemble\s*\*\s*e\s*,\s*double\s+t0\s*,\s*double\s+t1\s*,\s*const\s+int64_t\s*\*\s*nsteps\s*\)\s*;", text)
    assert re.search(r"\bint\s+crd_ensemble_own_steps\s*\(\s*const\s+crd_ensemble\s*\*\s*e\s*,\s*double\s+t0\s*,\s*double\s+t1\s*,\s*double\s+dt_safety\s*,\s*int64_t\s*\*\s*nsteps\s*\)\s*;", text)
    assert re.search(r"\bint\s+crd_ensemble_step_rk4_own_dt\s*\(\s*crd_ensemble\s*\*\s*e\s*,\s*double\s+t0\s*,\s*double\s+t1\s*,\s*const\s+double\s*\*\s*dt\s*,\s*const\s+int64_t\s*\*\s*nsteps\s*\)\s*;", text)
    assert re.search(r"\bint\s+crd_ensemble_step_rk4_own_timed\s*\(\s*crd_ensemble\s*\*\s*e\s*,\s*double\s+t0\s*,\s*double\s+t1\s*,\s*const\s+int64_t\s*\*\s*nsteps\s*,\s*double\s*\*\s*ms_total\s*\)\s*;", text)
    sig = crd._capi._SIGNATURES
    assert sig["crd_ensemble_step_rk4_own_timed"] == (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_double)])
    assert sig["crd_ensemble_step_rk4_own"] == (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_int64)])
    assert sig["crd_ensemble_own_steps"] == (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int64)])
    assert sig["crd_ensemble_step_rk4_own_dt"] == (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int64)])
    assert "#define CRD_ABI_VERSION 8" in open(HEADER).read() and crd._capi.ABI_VERSION == 8 and crd._capi.lib().crd_abi_version() == 8
    L = crd._capi.lib()
    n = (C.c_int64 * 2)(1, 2)
    dt = (C.c_double * 2)(0.1, 0.05)
    assert L.crd_ensemble_step_rk4_own(None, 0.0, 0.1, n) == crd._capi.EINVAL
    assert L.crd_ensemble_step_rk4_own_dt(None, 0.0, 0.1, dt, n) == crd._capi.EINVAL
    assert L.crd_ensemble_step_rk4_own_timed(None, 0.0, 0.1, n, None) == crd._capi.EINVAL
    assert L.crd_ensemble_own_steps(None, 0.0, 0.1, 0.8, n) == crd._capi.EINVAL and list(n) == [1, 2]
    assert hasattr(crd.Ensemble, "step_rk4_own") and hasattr(crd.Ensemble, "own_steps")


def test_entry_points_compile_and_link_from_c(tmp_path):
    src = tmp_path / "own.c"
    src.write_text(r'''
#include <stdio.h>
#include "crd.h"
int main(void) {
	crd_ensemble *e = (crd_ensemble *)0;
	int64_t n[2] = {1, 2};
	double dt[2] = {0.1, 0.05};
	int (*step)(crd_ensemble *, double, double, const int64_t *) = crd_ensemble_step_rk4_own;
	int (*step_dt)(crd_ensemble *, double, double, const double *, const int64_t *) = crd_ensemble_step_rk4_own_dt;
	int (*rule)(const crd_ensemble *, double, double, double, int64_t *) = crd_ensemble_own_steps;
	int (*timed)(crd_ensemble *, double, double, const int64_t *, double *) = crd_ensemble_step_rk4_own_timed;
	if (CRD_ABI_VERSION != 8 || crd_abi_version() != CRD_ABI_VERSION) return 1;
	if (step(e, 0.0, 0.1, n) != CRD_EINVAL || step_dt(e, 0.0, 0.1, dt, n) != CRD_EINVAL || rule(e, 0.0, 0.1, 0.8, n) != CRD_EINVAL ||
	    timed(e, 0.0, 0.1, n, dt) != CRD_EINVAL) return 2;
	if (n[0] != 1 || n[1] != 2) return 3;
	printf("ok\n");
	return 0;
}
''')
    exe = tmp_path / "own"
    libdir = os.path.join(ROOT, "crdmodel_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lcrd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout, r.stderr)


def crd_run(*args, ini=SMALL_INI):
    return subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus"] + list(args) + [ini], capture_output=True, text=True, timeout=120)


def ini_with(tmp_path, name, **solver):
    """small_run.ini with [Solver] keys replaced or added."""
    lines = [ln for ln in open(SMALL_INI).read().splitlines() if ln.split("=")[0].strip() not in solver]
    at = lines.index("[Solver]") + 1
    lines[at:at] = ["%s = %s" % kv for kv in solver.items()]
    path = tmp_path / name
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_driver_refuses_own_dt_without_an_ensemble(tmp_path):
    r = crd_run("--ensemble-own-dt", "--outdir", str(tmp_path), ini=ini_with(tmp_path, "free.ini", dt="0"))
    assert r.returncode != 0 and "--ensemble-own-dt" in r.stderr and "needs --ensemble" in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert not [f for f in os.listdir(tmp_path) if not f.endswith(".ini")]


def test_driver_refuses_own_dt_with_adaptive(tmp_path):
    r = crd_run("--ensemble", "diffusion=0.12,0.24", "--ensemble-own-dt", "--outdir", str(tmp_path), ini=ini_with(tmp_path, "adaptive.ini", dt="0", adaptive="1"))
    assert r.returncode != 0 and "--ensemble-own-dt" in r.stderr and "adaptive = 1" in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("member_")]  # refused before anything was created


def test_driver_refuses_own_dt_with_a_pinned_step(tmp_path):
    r = crd_run("--ensemble", "diffusion=0.12,0.24", "--ensemble-own-dt", "--outdir", str(tmp_path))  # small_run.ini: [Solver] dt = 0.02
    assert r.returncode != 0 and "--ensemble-own-dt" in r.stderr and "dt" in r.stderr and "no HIP device" not in r.stderr, r.stderr
    r = crd_run("--ensemble", "diffusion=0.12,0.24", "--ensemble-own-dt", "--dt", "0.01", "--outdir", str(tmp_path), ini=ini_with(tmp_path, "free.ini", dt="0"))
    assert r.returncode != 0 and "--ensemble-own-dt" in r.stderr and "--dt" in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("member_")]


def test_driver_refuses_own_dt_with_pairs(tmp_path):
    r = crd_run("--ensemble", "diffusion=0.12,0.24", "--ensemble-own-dt", "--ensemble-steps", "2", "--outdir", str(tmp_path), ini=ini_with(tmp_path, "free.ini", dt="0"))
    assert r.returncode != 0 and "--ensemble-own-dt" in r.stderr and "--ensemble-steps 2" in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("member_")]


def test_own_kernels_are_listed_at_the_step_kernels_resources():
    """profiles/ensemble/kernel_resources.txt lists every instantiation of the own-steps kernel against its step-kernel counterpart: no
    scratch, the same wavefronts per SIMD."""
    text = open(os.path.join(ROOT, "profiles", "ensemble", "kernel_resources.txt")).read()
    rows = re.findall(r"^crd_ensemble_own_kernel<(double|float), (\d), (true|false), (\d), (true|false)>\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+\|\s+"
                      r"(crd_ensemble_step(?:_mixed)?_kernel)<(double|float), (\d), (true|false), (\d)>\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", text, flags=re.M)
    want = sorted([("double", m, a, 1) for m in (0, 1) for a in (False, True)] + [("double", 2, False, 1)] +
                  [("float", m, a, c) for m in (0, 1) for a in (False, True) for c in (1, 2)] + [("float", 2, False, c) for c in (1, 2)])
    for mixed in (False, True):
        got = sorted((r[0], int(r[1]), r[2] == "true", int(r[3])) for r in rows if (r[4] == "true") == mixed)
        assert got == want, (mixed, got)
    for r in rows:
        assert r[9] == ("crd_ensemble_step_mixed_kernel" if r[4] == "true" else "crd_ensemble_step_kernel") and r[0:4] == r[10:14], r
        assert int(r[6]) == 0 and int(r[15]) == 0 and r[7] == r[16], r  # no scratch; the same wavefronts per SIMD
