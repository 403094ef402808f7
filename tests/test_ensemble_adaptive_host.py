"""CPU-side checks of error-controlled ensembles (crd_ensemble_integrate_adaptive, crd_run --ensemble with [Solver] adaptive = 1):
the declaration compiled from plain C, refusals that need no device, the ABI version, and what the driver refuses before the device."""
import ctypes as C
import os
import re
import subprocess

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
SMALL_INI = os.path.join(GOLDEN, "ini", "small_run.ini")


def test_abi_version_is_8():
    header = int(re.search(r"#define CRD_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "crd.h")).read()).group(1))
    assert header == crd._capi.ABI_VERSION == crd._capi.lib().crd_abi_version() == 8


def test_null_ensemble_is_refused():
    L = crd._capi.lib()
    opt, st = crd._capi.AdaptiveOptions(), (crd._capi.AdaptiveStats * 2)()
    status = (C.c_int32 * 2)()
    assert L.crd_adaptive_defaults(C.byref(opt)) == crd._capi.OK
    assert L.crd_ensemble_integrate_adaptive(None, 0.0, 1.0, C.byref(opt), st, status) == crd._capi.EINVAL
    assert L.crd_ensemble_integrate_adaptive(None, 0.0, 1.0, None, None, None) == crd._capi.EINVAL
    opt.method = crd._capi.ADAPT_RK43
    assert L.crd_ensemble_integrate_adaptive(None, 0.0, 1.0, C.byref(opt), None, None) == crd._capi.EINVAL


def test_adaptive_declaration_links_from_c(tmp_path):
    src = tmp_path / "ens_adapt.c"
    src.write_text(r'''
#include <stdio.h>
#include "crd.h"
int main(void) {
	crd_ensemble *e = (crd_ensemble *)0; crd_adaptive_options o; crd_adaptive_stats st[2]; int32_t status[2];
	int (*fn)(crd_ensemble *, double, double, const crd_adaptive_options *, crd_adaptive_stats *, int32_t *) = crd_ensemble_integrate_adaptive;
	if (CRD_ABI_VERSION < 8 || crd_abi_version() != CRD_ABI_VERSION) return 1;
	if (crd_adaptive_defaults(&o) != CRD_OK) return 2;
	if (fn(e, 0.0, 1.0, &o, st, status) != CRD_EINVAL) return 3;
	o.method = CRD_ADAPT_RK43;
	if (crd_ensemble_integrate_adaptive(e, 0.0, 1.0, &o, NULL, NULL) != CRD_EINVAL) return 4;
	printf("ok\n");
	return 0;
}
''')
    exe = tmp_path / "ens_adapt"
    libdir = os.path.join(ROOT, "crdmodel_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lcrd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout, r.stderr)


def ini_with_adaptive(tmp_path, value):
    text = open(SMALL_INI).read().replace("[Solver]\n", "[Solver]\nadaptive = %d\n" % value)
    assert "adaptive = %d" % value in text
    path = tmp_path / ("adaptive_%d.ini" % value)
    path.write_text(text)
    return str(path)


def test_driver_takes_adaptive_ensembles_from_the_ini(tmp_path):
    """adaptive = 1 in the ini: the ensemble integrates error-controlled.  Without a device the run fails for lack of one, not with
    the old fixed-step-only refusal (on a machine with a device it runs: tests/test_gpu_ensemble_adaptive.py)."""
    r = subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus", "--ensemble", "beta=1,2", "--outdir", str(tmp_path),
                        ini_with_adaptive(tmp_path, 1)], capture_output=True, text=True, timeout=120)
    assert "fixed-step RK4 only" not in r.stderr and "adaptive" not in r.stderr, r.stderr
    if r.returncode != 0:
        assert "no HIP device available" in r.stderr, r.stderr


def test_driver_still_refuses_rk43_ensembles(tmp_path):
    r = subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus", "--ensemble", "beta=1,2", "--outdir", str(tmp_path),
                        ini_with_adaptive(tmp_path, 2)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "adaptive = 2" in r.stderr and "RK4(3)" in r.stderr, r.stderr
    assert not (tmp_path / "member_0").exists()  # refused before the device and before any file
