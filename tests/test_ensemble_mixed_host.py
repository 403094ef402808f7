"""CPU-side checks of mixed-geometry ensembles (crd_ensemble_create_mixed): what is refused before any device is touched, what passes
through to the device, and the new declarations compiled from plain C.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import pytest

import crdmodel_amd as crd
from conftest import ROOT


def base(**kw):
    p = crd.make_params("fhn", "torus", 32, 80.0, 20.0, 0.12, 1.25)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def create_mixed(members):
    L = crd._capi.lib()
    h = C.c_void_p()
    arr = (crd._capi.Params * max(len(members), 1))(*members)
    rc = L.crd_ensemble_create_mixed(arr, len(members), 0, C.byref(h))
    msg = L.crd_ensemble_last_error(None).decode()
    if rc == crd._capi.OK:
        L.crd_ensemble_destroy(h)
    return rc, msg


@pytest.mark.parametrize("field,value", [("model", 1), ("precision", 1), ("just_diffusion", 1)])
def test_members_must_agree_on_model_precision_and_just_diffusion(field, value):
    other = base(surface_length=40.0)
    setattr(other, field, value)
    rc, msg = create_mixed([base(), base(nx=40), other])
    assert rc == crd._capi.EINVAL, (rc, msg)
    assert "member 2" in msg and field in msg, msg


def test_a_seven_row_member_is_refused():
    rc, msg = create_mixed([base(), base(nx=40, ny=7), base(ny=12)])
    assert rc == crd._capi.EINVAL, (rc, msg)
    assert "member 1" in msg and "ny = 7" in msg and "8 rows" in msg, msg


def test_block_ids_of_all_members_together_are_32_bit():
    big = base(nx=48000, ny=40000)  # 1000 strips x 10000 chunks = 10^7 blocks per member at the most
    rc, msg = create_mixed([base()] + [big] * 250)
    assert rc == crd._capi.EINVAL, (rc, msg)
    assert "member 215" in msg and "32 bits" in msg and "nx" in msg, msg  # 32 + 214 x 10^7 <= 2^31 - 1 < 32 + 215 x 10^7


def test_empty_and_invalid_members_are_refused():
    rc, msg = create_mixed([])
    assert rc == crd._capi.EINVAL and "at least one member" in msg, msg
    rc, msg = create_mixed([base(), base(diffusion=float("nan"))])
    assert rc == crd._capi.EINVAL and "member 1" in msg, msg
    assert crd._capi.lib().crd_ensemble_member_grid(None, 0, None) == crd._capi.EINVAL


def test_shape_differences_reach_the_device():
    """Differences in surface, nx, ny and the surface's length and width pass validation: without a device the refusal is EHIP."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    members = [base(), base(surface=1), base(nx=40), base(ny=24), base(surface_length=40.0), base(surface_width=10.0), base(beta=0.9, t_boundary=5.0)]
    rc, msg = create_mixed(members)
    assert rc == crd._capi.EHIP and "no CPU fallback" in msg, (rc, msg)
    with pytest.raises(crd.CrdError) as e:
        crd.Ensemble(members, mixed=True)
    assert e.value.status == crd._capi.EHIP
    with pytest.raises(crd.CrdError) as e:  # the default constructor still refuses them
        crd.Ensemble(members)
    assert e.value.status == crd._capi.EINVAL and "surface" in str(e.value)


def test_new_declarations_compile_and_link_from_c99(tmp_path):
    src = tmp_path / "mixed.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "crd.h"
int main(void)
{
	crd_params p[2];
	crd_ensemble *e = NULL;
	crd_grid g;
	int rc;
	memset(p, 0, sizeof p);
	p[0].model = p[1].model = CRD_MODEL_FHN;
	p[0].surface = CRD_SURFACE_TORUS;
	p[1].surface = CRD_SURFACE_FLAT;
	p[0].nx = 32;
	p[1].nx = 40;
	p[0].surface_length = 80.0;
	p[1].surface_length = 40.0;
	p[0].surface_width = p[1].surface_width = 20.0;
	p[0].diffusion = p[1].diffusion = 0.12;
	p[0].beta = p[1].beta = 1.25;
	p[1].precision = CRD_PRECISION_F32;
	if (CRD_ABI_VERSION != 8 || crd_abi_version() != CRD_ABI_VERSION) return 1;
	rc = crd_ensemble_create_mixed(p, 2, 0, &e);
	if (rc != CRD_EINVAL || e || !strstr(crd_ensemble_last_error(NULL), "precision")) return 2;
	if (crd_ensemble_member_grid(e, 0, &g) != CRD_EINVAL) return 3;
	printf("ok %s\n", crd_ensemble_last_error(NULL));
	return 0;
}
''')
    exe = tmp_path / "mixed"
    libdir = os.path.join(ROOT, "crdmodel_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lcrd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stdout.startswith("ok member 1 differs from member 0 in precision"), r.stdout


BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
SMALL_INI = os.path.join(ROOT, "tests", "golden", "ini", "small_run.ini")


def crd_run(*args, ini=SMALL_INI):
    return subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus"] + list(args) + [ini], capture_output=True, text=True, timeout=120)


def test_driver_refuses_a_bad_surface_value():
    r = crd_run("--ensemble", "surface=torus,sphere")
    assert r.returncode != 0 and "'sphere'" in r.stderr and "torus" in r.stderr and "flat" in r.stderr, r.stderr


def test_driver_refuses_geometry_lists_of_unequal_length():
    r = crd_run("--ensemble", "surfaceLength=80,40", "--ensemble", "surface=torus")
    assert r.returncode != 0 and "surfaceLength has 2" in r.stderr and "surface has 1" in r.stderr, r.stderr


def test_driver_unknown_key_lists_the_geometry_keys():
    r = crd_run("--ensemble", "gamma=1,2")
    assert r.returncode != 0 and "gamma" in r.stderr, r.stderr
    for key in ("surfaceLength", "surfaceWidth", "xMesh", "surface"):
        assert key in r.stderr, (key, r.stderr)
    r = crd_run("--ensemble", "xMesh=16,2.5")
    assert r.returncode != 0 and "'2.5'" in r.stderr, r.stderr


def test_driver_refuses_what_mixed_shapes_cannot_do(tmp_path):
    """Members of different nx (xMesh; small_run.ini pins ny by phiMesh): [Solver] adaptive = 1, --section and --observe-cycles are
    refused up front, by name, and so is a probe outside the smaller member."""
    ini = tmp_path / "adaptive.ini"
    ini.write_text(open(SMALL_INI).read() + "adaptive = 1\n")
    r = crd_run("--ensemble", "xMesh=16,24", ini=str(ini))
    assert r.returncode != 0 and "adaptive = 1" in r.stderr and "members of different shape" in r.stderr, r.stderr
    r = crd_run("--ensemble", "xMesh=16,24", "--observe", "1", "--section", "row:3")
    assert r.returncode != 0 and "--section" in r.stderr and "members of different shape" in r.stderr, r.stderr
    r = crd_run("--ensemble", "xMesh=16,24", "--observe", "1", "--observe-cycles", "0.5")
    assert r.returncode != 0 and "--observe-cycles" in r.stderr and "members of different shape" in r.stderr, r.stderr
    r = crd_run("--ensemble", "xMesh=24,16", "--observe", "1", "--probe", "20,3")
    assert r.returncode != 0 and "--probe 20,3" in r.stderr and "member 1" in r.stderr, r.stderr
