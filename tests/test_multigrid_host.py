"""The preconditioner solve's reference on the host (tests/multigrid_reference.py): the level rule, the kernel-order restatement inside
the per-point bound in both precisions, mutants outside it, the cycle as a GMRES preconditioner against the issue's table, its
symmetry on the flat surface, and the C ABI's new entries.  No GPU: what the device computes is held to the same reference and bound
in tests/test_gpu_multigrid.py.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
import jacobian_reference as jr
import multigrid_reference as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("crd_psolve_defaults", "crd_psolve_info", "crd_psolve_device", "crd_psolve_host")
DTYPES = {"f64": np.float64, "f32": np.float32}


def worst_ratio(got, ref, bound):
    """Largest err / bound over var0 (inf where a zero bound is missed); var1 must be r's bits."""
    err = np.abs(np.asarray(got)[..., 0].astype(ref.dtype) - ref[..., 0]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / bound)
    return float(np.nan_to_num(q, nan=np.inf, posinf=np.inf).max())


def problem(config, nx, ny):
    _, model, surface, beta, kw = config
    return jr.problem_of(model, surface, nx, ny, beta, t_boundary=jr.T_BOUNDARY, **kw)


def right_hand_side(nx, ny, R, seed=3):
    return np.random.default_rng(seed).standard_normal((ny, nx, 2)).astype(R)


# ---- the level rule ---------------------------------------------------------------------------------------------------------------
def test_level_rule():
    for (nx, ny), levels in mg.LEVEL_CASES:
        shapes = mg.level_shapes(nx, ny)
        assert len(shapes) == levels, ((nx, ny), shapes)
        assert all(shapes[k + 1] == (shapes[k][0] // 2, shapes[k][1] // 2) for k in range(levels - 1))
    assert [s[0] for s in mg.level_shapes(136, 72)] == [136, 68, 34, 17]
    assert mg.level_shapes(48, 40)[-1] == (6, 5)
    assert mg.level_shapes(32, 128)[-1] == (4, 16)
    assert len(mg.level_shapes(96, 384)) == 5 and len(mg.level_shapes(96, 384, max_levels=2)) == 2
    assert len(mg.level_shapes(8192, 8192)) == 12 and len(mg.level_shapes(1 << 20, 1 << 20)) == 16  # the cap


# ---- the restatement is inside the bound, mutants are not -------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config", jr.CONFIGS, ids=[c[0] for c in jr.CONFIGS])
def test_kernel_order_within_the_bound(config, precision):
    R, worst = DTYPES[precision], 0.0
    for nx, ny in mg.GRIDS:
        op, r = problem(config, nx, ny), right_hand_side(nx, ny, R)
        for t in jr.TIMES:
            for multiple in mg.GAMMAS:
                gamma = multiple * mg.explicit_bound(op)
                for opts in mg.OPTION_SETS:
                    ref, bound, bound_v = mg.vcycle_bound(op, t, gamma, r, precision, **opts)
                    got = mg.kernel_order_vcycle(op, t, gamma, r, R, **opts)
                    assert np.array_equal(got[..., 1], r[..., 1]) and not bound_v.any()
                    q = worst_ratio(got, ref, bound)
                    assert q <= 1.0, (config[0], precision, nx, ny, t, multiple, opts, q)
                    worst = max(worst, q)
    print("BOUND WORST kernel order %s %s: %.3g" % (precision, config[0], worst))


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("mutant", mg.MUTANTS)
def test_mutants_exceed_the_bound(mutant, precision):
    """On the torus with held rows (what every mutant needs to show) each mutant is outside the bound on every grid with a coarse level."""
    R = DTYPES[precision]
    for nx, ny in [(32, 128), (136, 72), (48, 40), (64, 16)]:
        op, r = problem(jr.CONFIGS[0], nx, ny), right_hand_side(nx, ny, R)
        for multiple in mg.GAMMAS:
            gamma = multiple * mg.explicit_bound(op)
            ref, bound, _ = mg.vcycle_bound(op, jr.TIMES[0], gamma, r, precision)
            assert worst_ratio(mg.kernel_order_vcycle(op, jr.TIMES[0], gamma, r, R), ref, bound) <= 1.0
            q = worst_ratio(mg.kernel_order_vcycle(op, jr.TIMES[0], gamma, r, R, mutant=mutant), ref, bound)
            assert q > 1.0, (mutant, precision, nx, ny, multiple, q)


def test_gamma_zero_and_var1():
    op, r = problem(jr.CONFIGS[0], 48, 40), right_hand_side(48, 40, np.float64)
    ref, bound, _ = mg.vcycle_bound(op, 0.25, 0.0, r, "f64")
    assert np.array_equal(ref.astype(np.float64), r) and not bound.any()
    assert np.array_equal(mg.kernel_order_vcycle(op, 0.25, 0.0, r, np.float64), r)


# ---- what it is for ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", mg.GMRES_TABLE[:5], ids=["%dx%d-%s-%s-%gx" % (r[0], r[1], r[2], "held" if r[3] else "free", r[4]) for r in mg.GMRES_TABLE[:5]])
def test_cycle_as_gmres_preconditioner(row):
    """The reference cycle as M in scipy gmres (rtol 1e-10, no restart) on (I - gamma J_D) z = r: at most a quarter of the
    unpreconditioned iteration count, and at most 25 -- caps that keep a broken cycle from passing (the prototype's counts are in
    multigrid_reference.GMRES_TABLE; its worst ratio is 19 / 432)."""
    nx, ny, surface, held, multiple, plain_proto, pre_proto = row
    op = jr.problem_of("fhn", surface, nx, ny, 1.25, t_boundary=jr.T_BOUNDARY)
    t = jr.TIMES[0] if held else jr.TIMES[2]
    gamma = multiple * mg.explicit_bound(op)
    b = np.random.default_rng(5).standard_normal(nx * ny)
    A = lambda x: mg.operator(op, t, gamma, x.reshape(ny, nx)).ravel()
    M = lambda x: mg.reference_vcycle(op, t, gamma, x.reshape(ny, nx)).ravel()
    x_plain, plain = mg.gmres_iterations(A, b)
    x_pre, pre = mg.gmres_iterations(A, b, M)
    print("GMRES %dx%d %s %s %gx: %d iterations without, %d with the cycle (prototype: %d, %d)" % (nx, ny, surface, "held" if held else "free", multiple, plain, pre, plain_proto, pre_proto))
    assert 4 * pre <= plain and pre <= 25, (plain, pre)
    for x in (x_plain, x_pre):
        assert np.linalg.norm(A(x) - b) <= 1e-9 * np.linalg.norm(b)


def test_cycle_is_symmetric_on_the_flat_surface():
    """Flat surface, pre = post, no held rows: <x, M y> = <M x, y> on the long-double reference.  Tolerance: the per-point bound of the
    module with u = 2^-64 bounds each product's rounding, sum |x| B(M y) + sum |y| B(M x), and each inner product adds n 2^-64 of
    its terms' magnitudes."""
    L, u = np.longdouble, 2.0 ** -64
    for nx, ny in [(48, 40), (64, 16)]:
        op = jr.problem_of("fhn", "flat", nx, ny, 1.25, t_boundary=jr.T_BOUNDARY)
        rng = np.random.default_rng(11)
        x, y = rng.standard_normal((ny, nx, 2)), rng.standard_normal((ny, nx, 2))
        for multiple in mg.GAMMAS:
            gamma = multiple * mg.explicit_bound(op)
            for opts in (dict(), dict(pre=1, post=1, coarse=3)):
                mx, bx, _ = mg.vcycle_bound(op, jr.TIMES[2], gamma, x, "f64", unit=u, **opts)
                my, by, _ = mg.vcycle_bound(op, jr.TIMES[2], gamma, y, "f64", unit=u, **opts)
                x0, y0, mx, my = x[..., 0].astype(L), y[..., 0].astype(L), mx[..., 0], my[..., 0]
                lhs, rhs = np.sum(x0 * my), np.sum(mx * y0)
                tol = np.sum(np.abs(x[..., 0]) * by) + np.sum(np.abs(y[..., 0]) * bx) + nx * ny * u * float(np.sum(np.abs(x0 * my)) + np.sum(np.abs(mx * y0)))
                assert abs(float(lhs - rhs)) <= tol, (nx, ny, multiple, opts, float(lhs - rhs), tol)
                assert abs(float(lhs)) > 1e3 * tol  # the tolerance means something
    # ... and the torus is not: the first-order term makes A, hence M, unsymmetric
    op = jr.problem_of("fhn", "torus", 48, 40, 1.25, t_boundary=jr.T_BOUNDARY)
    gamma = 2000.0 * mg.explicit_bound(op)
    x, y = rng.standard_normal((40, 48, 2)), rng.standard_normal((40, 48, 2))
    mx, my =(mg.vcycle_bound(op, jr.TIMES[2], gamma, v, "f64")[0][..., 0] for v in (x, y))
    assert abs(float(np.sum(x[..., 0] * my) - np.sum(mx * y[..., 0]))) > 1e-6


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_agree():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crd.h")).read(), flags=re.S)
    L = C.CDLL(crd._capi.LIB_PATH)
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name
        assert hasattr(L, name), name
        res, args = crd._capi._SIGNATURES[name]
        assert res is C.c_int and len(args) == len(m.group(1).split(",")), (name, m.group(1))
    assert re.search(r"typedef struct crd_psolve_options\s*\{\s*int32_t pre, post, coarse, max_levels;\s*double omega;\s*\}\s*crd_psolve_options;", header)
    assert [f for f, _ in crd._capi.PsolveOptions._fields_] == ["pre", "post", "coarse", "max_levels", "omega"] and C.sizeof(crd._capi.PsolveOptions) == 24
    assert int(re.search(r"#define CRD_ABI_VERSION (\d+)", header).group(1)) == 8  # additions only
    assert hasattr(crd.Slab, "psolve") and hasattr(crd.Slab, "psolve_info")


def test_defaults_and_null_arguments():
    L = crd._capi.lib()
    opt = crd._capi.PsolveOptions()
    assert L.crd_psolve_defaults(C.byref(opt)) == crd._capi.OK
    assert (opt.pre, opt.post, opt.coarse, opt.max_levels, opt.omega) == (2, 2, 8, 16, 0.8)
    assert {k: getattr(opt, k) for k in mg.DEFAULTS} == mg.DEFAULTS
    assert L.crd_psolve_defaults(None) == crd._capi.EINVAL
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    assert L.crd_psolve_device(None, 0.0, 1.0, None, p, p) == crd._capi.EINVAL
    assert L.crd_psolve_host(None, 0.0, 1.0, None, p, p) == crd._capi.EINVAL
    assert L.crd_psolve_info(None, None, None, None, None, None) == crd._capi.EINVAL


def test_header_compiles_as_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "psolve.c"
    src.write_text(r'''
#include <stddef.h>
#include "crd.h"
int main(void) {
	double r[4] = {0, 0, 0, 0}, z[4];
	int32_t levels, nx[16], ny[16]; int64_t bytes;
	crd_psolve_options o;
	if (crd_psolve_defaults(&o) != CRD_OK || o.pre != 2 || o.post != 2 || o.coarse != 8 || o.max_levels != 16 || o.omega != 0.8) return 1;
	if (crd_psolve_defaults(NULL) != CRD_EINVAL) return 2;
	if (crd_psolve_info(NULL, &o, &levels, nx, ny, &bytes) != CRD_EINVAL) return 3;
	if (crd_psolve_device(NULL, 0.0, 1.0, &o, r, z) != CRD_EINVAL) return 4;
	if (crd_psolve_host(NULL, 0.0, 1.0, NULL, r, z) != CRD_EINVAL) return 5;
	if (crd_abi_version() != 8) return 6;
	return 0;
}
''')
    exe = tmp_path / "psolve"
    libdir = os.path.dirname(crd._capi.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lcrd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_psolve_shim_compiles_as_c(tmp_path):
    """integration/crd_arkode_shim.c with crd_arkode_psolve and tests/native/shim_psolve_selftest.c compile as C against the test double
    and link against libcrd; running them needs a GPU (tests/test_gpu_multigrid.py)."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    r = subprocess.run(mg.shim_build_command(tmp_path / "shim_psolve"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
