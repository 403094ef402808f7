"""CPU-side checks of ensembles (crd_ensemble_*, crd_run --ensemble): what is refused before any device is touched, and the header's
ensemble declarations compiled from plain C.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import pytest

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
SMALL_INI = os.path.join(GOLDEN, "ini", "small_run.ini")


def base(**kw):
    p = crd.make_params("fhn", "torus", 32, 80.0, 20.0, 0.12, 1.25)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def create(members):
    L = crd._capi.lib()
    h = C.c_void_p()
    arr = (crd._capi.Params * max(len(members), 1))(*members)
    rc = L.crd_ensemble_create(arr, len(members), 0, C.byref(h))
    msg = L.crd_ensemble_last_error(None).decode()
    if rc == crd._capi.OK:
        L.crd_ensemble_destroy(h)
    return rc, msg


@pytest.mark.parametrize("field,value", [("model", 1), ("surface", 1), ("nx", 34), ("ny", 200), ("surface_length", 90.0), ("surface_width", 19.0),
                                         ("precision", 1), ("just_diffusion", 1)])
def test_members_must_agree(field, value):
    other = base()
    setattr(other, field, value)
    rc, msg = create([base(), base(beta=0.9), other])
    assert rc == crd._capi.EINVAL, (rc, msg)
    assert "member 2" in msg and field in msg, msg


def test_members_may_differ_in_their_parameters():
    """Differences in diffusion, beta, betaMin, betaMax, varyBeta and tBoundary pass validation: without a device the refusal is EHIP."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    members = [base(), base(diffusion=0.3), base(beta=0.9), base(beta_min=0.1, beta_max=2.0, vary_beta=1), base(t_boundary=5.0)]
    rc, msg = create(members)
    assert rc == crd._capi.EHIP and "no CPU fallback" in msg, (rc, msg)
    with pytest.raises(crd.CrdError) as e:
        crd.Ensemble(members)
    assert e.value.status == crd._capi.EHIP


def test_empty_and_invalid_members_are_refused():
    rc, msg = create([])
    assert rc == crd._capi.EINVAL and "at least one member" in msg, msg
    rc, msg = create([base(), base(diffusion=float("nan"))])
    assert rc == crd._capi.EINVAL and "member 1" in msg, msg
    with pytest.raises(crd.CrdError) as e:
        crd.Ensemble([base(), base(surface_width=10.0)])
    assert e.value.status == crd._capi.EINVAL and "surface_width" in str(e.value)
    L = crd._capi.lib()
    assert L.crd_ensemble_info(None, None, None) == crd._capi.EINVAL
    assert L.crd_ensemble_last_error(None) is not None


def crd_run(*args):
    return subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus"] + list(args) + [SMALL_INI], capture_output=True, text=True,
                          timeout=120)


def test_driver_refuses_unequal_lists():
    r = crd_run("--ensemble", "beta=1,2", "--ensemble", "tBoundary=5")
    assert r.returncode != 0 and "beta has 2" in r.stderr and "tBoundary has 1" in r.stderr, r.stderr


@pytest.mark.parametrize("extra,needle", [(["--adaptive"], "--adaptive"), (["--gpus", "2"], "--gpus"), (["--decomp", "2x2"], "--decomp"),
                                          (["--ensemble", "gamma=1,2"], "gamma"), (["--ensemble", "beta=1,x"], "'x' is not a number")])
def test_driver_refuses_conflicts(extra, needle):
    r = crd_run("--ensemble", "diffusion=0.1,0.2", *extra)
    assert r.returncode != 0 and needle in r.stderr, r.stderr


def test_ensemble_declarations_link_from_c(tmp_path):
    src = tmp_path / "ens.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "crd.h"
int main(void) {
	crd_params p[2]; crd_ensemble *e = (crd_ensemble *)0; int n = 0; crd_grid g; double m[2]; int rc;
	memset(p, 0, sizeof p);
	p[0].model = CRD_MODEL_FHN; p[0].surface = CRD_SURFACE_TORUS; p[0].nx = 32; p[0].surface_length = 80.0; p[0].surface_width = 20.0;
	p[0].diffusion = 0.12; p[0].beta = 1.25; p[0].precision = CRD_PRECISION_F64;
	p[1] = p[0];
	p[1].nx = 34;
	if (CRD_ABI_VERSION < 7 || crd_abi_version() != CRD_ABI_VERSION) return 1;
	rc = crd_ensemble_create(p, 2, 0, &e);
	if (rc != CRD_EINVAL || e || !strstr(crd_ensemble_last_error(NULL), "nx")) return 2;
	if (crd_ensemble_info(e, &n, &g) != CRD_EINVAL || crd_ensemble_max_abs(e, m) != CRD_EINVAL || crd_ensemble_synchronize(e) != CRD_EINVAL) return 3;
	if (crd_ensemble_step_rk4(e, 0.0, 0.1, 1) != CRD_EINVAL || crd_ensemble_step_rk4_timed(e, 0.0, 0.1, 1, m) != CRD_EINVAL) return 4;
	if (crd_ensemble_upload(e, 0, m, 1) != CRD_EINVAL || crd_ensemble_download(e, 0, m, 1) != CRD_EINVAL) return 5;
	crd_ensemble_destroy(e);
	printf("ok %s\n", crd_ensemble_last_error(NULL));
	return 0;
}
''')
    exe = tmp_path / "ens"
    libdir = os.path.join(ROOT, "crdmodel_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lcrd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stdout.startswith("ok member 1 differs from member 0 in nx"), r.stdout
