"""CPU-side checks of the split right-hand side and of J v (crd_rhs_part_* / crd_jtimes_*): the ABI's new entries, that the
reference of tests/jacobian_reference.py is right (Goldbeter partials against sympy.diff, the FHN block against a central difference
of the numpy right-hand side), and that its per-point bound is honest (the kernels' own order, restated in the working precision,
stays inside it on every shape tests/test_gpu_jacobian.py uses) and sharp (four planted mistakes miss it by more than 10x).
No kernel is launched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
import jacobian_reference as jr
from conftest import ROOT
from oracle import crd_oracle_np as cn
from oracle import error_bounds as eb

ENTRIES = ["crd_rhs_part_device", "crd_rhs_part_host", "crd_jtimes_device", "crd_jtimes_host", "crd_group_rhs_part_device", "crd_group_rhs_part_host",
           "crd_group_jtimes_device", "crd_group_jtimes_host"]
DTYPE = {"f64": np.float64, "f32": np.float32}


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_capi_and_library_agree():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crd.h")).read(), flags=re.S)
    L = C.CDLL(crd._capi.LIB_PATH)
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name
        assert hasattr(L, name), name
        res, args = crd._capi._SIGNATURES[name]
        assert res is C.c_int and len(args) == len(m.group(1).split(",")), (name, m.group(1))
        assert "int part" in m.group(1) and "double t" in m.group(1)
    assert re.search(r"enum\s*\{\s*CRD_PART_FULL = 0, CRD_PART_DIFFUSION = 1, CRD_PART_REACTION = 2\s*\}", header)
    k = crd._capi
    assert (k.PART_FULL, k.PART_DIFFUSION, k.PART_REACTION) == (0, 1, 2) and k.PARTS == {"full": 0, "diffusion": 1, "reaction": 2}
    assert int(re.search(r"#define CRD_ABI_VERSION (\d+)", header).group(1)) == 8  # additions only


def test_null_arguments_are_einval():
    L = crd._capi.lib()
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    ptrs = (C.c_void_p * 1)(p)
    for part in (0, 1, 2, 7):
        assert L.crd_rhs_part_device(None, 0.0, part, p, p) == crd._capi.EINVAL
        assert L.crd_rhs_part_host(None, 0.0, part, p, p) == crd._capi.EINVAL
        assert L.crd_jtimes_device(None, 0.0, part, p, p, p) == crd._capi.EINVAL
        assert L.crd_jtimes_host(None, 0.0, part, p, p, p) == crd._capi.EINVAL
        assert L.crd_group_rhs_part_device(None, 1, 0.0, part, ptrs, ptrs) == crd._capi.EINVAL
        assert L.crd_group_rhs_part_host(None, 1, 0.0, part, ptrs, ptrs) == crd._capi.EINVAL
        assert L.crd_group_jtimes_device(None, 1, 0.0, part, ptrs, ptrs, ptrs) == crd._capi.EINVAL
        assert L.crd_group_jtimes_host(None, 1, 0.0, part, ptrs, ptrs, ptrs) == crd._capi.EINVAL
        null_ctx = (C.c_void_p * 1)(None)
        assert L.crd_group_jtimes_host(null_ctx, 1, 0.0, part, ptrs, ptrs, ptrs) == crd._capi.EINVAL


def test_entries_link_from_c(tmp_path):
    """A C99 program links every new entry point, calls each with a NULL context and gets CRD_EINVAL."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "parts.c"
    src.write_text(r'''
#include <stddef.h>
#include "crd.h"
int main(void) {
	double y[4] = {0, 0, 0, 0};
	const void *in[1]; void *out[1];
	in[0] = y; out[0] = y;
	if (CRD_PART_FULL != 0 || CRD_PART_DIFFUSION != 1 || CRD_PART_REACTION != 2) return 1;
	if (crd_rhs_part_device(NULL, 0.0, CRD_PART_DIFFUSION, y, y) != CRD_EINVAL) return 2;
	if (crd_rhs_part_host(NULL, 0.0, CRD_PART_REACTION, y, y) != CRD_EINVAL) return 3;
	if (crd_jtimes_device(NULL, 0.0, CRD_PART_FULL, y, y, y) != CRD_EINVAL) return 4;
	if (crd_jtimes_host(NULL, 0.0, CRD_PART_FULL, y, y, y) != CRD_EINVAL) return 5;
	if (crd_group_rhs_part_device(NULL, 1, 0.0, CRD_PART_DIFFUSION, in, out) != CRD_EINVAL) return 6;
	if (crd_group_rhs_part_host(NULL, 1, 0.0, CRD_PART_DIFFUSION, in, out) != CRD_EINVAL) return 7;
	if (crd_group_jtimes_device(NULL, 1, 0.0, CRD_PART_FULL, in, in, out) != CRD_EINVAL) return 8;
	if (crd_group_jtimes_host(NULL, 1, 0.0, CRD_PART_FULL, in, in, out) != CRD_EINVAL) return 9;
	return 0;
}
''')
    exe = tmp_path / "parts"
    libdir = os.path.join(ROOT, "crdmodel_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lcrd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_imex_shim_compiles_as_c(tmp_path):
    """integration/crd_arkode_shim.c with its IMEX callbacks and tests/native/shim_imex_selftest.c compile as C against the test double
    and link against libcrd; running them needs a GPU (tests/test_gpu_jacobian.py)."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    r = subprocess.run(jr.shim_build_command(tmp_path / "shim_imex"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the reference is right ------------------------------------------------------------------------------------------------------
def test_goldbeter_partials_equal_sympy_diff():
    """w_z = wz2 - wz3 and w_y of the reference equal sympy.diff of w = v2(z) - v3(z, y) at sampled points, to long-double rounding:
    sympy evaluates the derivative at 40 digits; the long-double formula has a dozen roundings of 2^-64 on terms that cancel in
    w_z, so it is held to 32 x 2^-64 of the terms' magnitudes."""
    import sympy

    z, y = sympy.symbols("z y", positive=True)
    q = sympy.Rational
    ka4 = q(9, 10) ** 4
    w = 65 * z ** 2 / (1 + z ** 2) - 500 * y ** 2 * z ** 4 / ((4 + y ** 2) * (ka4 + z ** 4))
    w_z, w_y = sympy.diff(w, z), sympy.diff(w, y)
    rng = np.random.default_rng(5)
    zs = np.concatenate([rng.uniform(1e-3, 1.6, 40), [0.39, 0.2, 1.0]])
    ys = np.concatenate([rng.uniform(1e-3, 3.2, 40), [1.66, 0.5, 3.0]])
    for zv, yv in zip(zs, ys):
        zl, yl = np.longdouble(zv), np.longdouble(yv)
        exact_ka4 = (np.longdouble(9) / np.longdouble(10)) ** 4
        wz2, wz3, wy = jr.goldbeter_partials(np.array([zl]), np.array([yl]), ka4=exact_ka4)
        at = {z: q(*float(zv).as_integer_ratio()), y: q(*float(yv).as_integer_ratio())}
        want_z, want_y = sympy.N(w_z.subs(at), 40), sympy.N(w_y.subs(at), 40)
        tol = 32 * 2.0 ** -64
        # (compare in long double: the residual against sympy's value rounded to long double)
        res_z = abs(float((wz2[0] - wz3[0]) - _longdouble(want_z)))
        res_y = abs(float(wy[0] - _longdouble(want_y)))
        assert res_z <= tol * float(abs(wz2[0]) + abs(wz3[0])), (zv, yv, res_z, want_z)
        assert res_y <= tol * float(abs(wy[0])), (zv, yv, res_y, want_y)


def _longdouble(x):
    """A 40-digit sympy Float as np.longdouble: its double head plus the remainder."""
    import sympy

    head = float(x)
    return np.longdouble(head) + np.longdouble(float(x - sympy.Float(head, 40)))


def test_fhn_block_equals_central_difference():
    """FHN is cubic: (f(y + h d) - f(y - h d)) / 2h = J d - h^2 du^3 exactly (u field), so the central difference of the numpy
    right-hand side in long double, h = 2^-10, pins the reference's J d to long-double rounding: each f rounds a few times relative to
    the sum S of its terms' magnitudes (error_bounds: S_u, S_v), the subtraction divides by 2h, so 16 x 2^-64 S / h per point."""
    h = np.longdouble(2.0) ** -10
    for config in jr.CONFIGS[:2]:
        for nx, ny in jr.GRIDS:
            p, op = jr.case(config, nx, ny)
            y, d = jr.start_state(p, 3), jr.direction(p, 4)
            P = eb._Problem(op)
            for t in jr.TIMES:
                yl, dl = y.astype(np.longdouble), d.astype(np.longdouble)
                fp = P.rhs(t, yl[..., 0] + h * dl[..., 0], yl[..., 1] + h * dl[..., 1], np.longdouble, 0)
                fm = P.rhs(t, yl[..., 0] - h * dl[..., 0], yl[..., 1] - h * dl[..., 1], np.longdouble, 0)
                ref, _, _ = jr.jtimes_bound(op, t, y, d, "f64", jr.FULL)
                cubic = h * h * dl[..., 0] ** 3
                cubic[P.zero_rows(t, ny, 0)] = 0
                S_u, S_v = P.terms(y[..., 0], y[..., 1], 0)[:2]
                tol = 16 * 2.0 ** -64 / float(h)
                res_u = np.abs(((fp[0] - fm[0]) / (2 * h) - (ref[..., 0] - cubic)).astype(np.float64))
                res_v = np.abs(((fp[1] - fm[1]) / (2 * h) - ref[..., 1]).astype(np.float64))
                assert np.all(res_u <= tol * (S_u + 1.0)) and np.all(res_v <= tol * (S_v + 1.0)), (config[0], nx, ny, t, (res_u / (S_u + 1)).max() / tol)


def test_parts_of_the_reference_add_up_to_the_oracle():
    """diffusion + reaction of the reference is crd_oracle_np's f, to long-double rounding of the terms."""
    for config in jr.CONFIGS:
        p, op = jr.case(config, 130, 33)
        y = jr.start_state(p, 6)
        for t in jr.TIMES:
            full, bu, bv = eb.rhs_bound(op, t, y, "f64")
            parts = [jr.part_bound(op, t, y, "f64", part)[0] for part in (jr.DIFFUSION, jr.REACTION)]
            both = jr.part_bound(op, t, y, "f64", jr.FULL)[0]
            assert np.array_equal(both, parts[0] + parts[1])
            err = np.abs((both - full).astype(np.float64))
            assert np.all(err[..., 0] <= bu / 256) and np.all(err[..., 1] <= bv / 256), config[0]  # 2^-64 against 2^-53 of the same terms


# ---- the bound is neither vacuous nor slack ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config", jr.CONFIGS, ids=[c[0] for c in jr.CONFIGS])
def test_kernel_order_stays_inside_the_bound(config, precision):
    """The kernels' operation order in the working precision stays at or below 1.0 of the bound: every grid, time, part and J v form
    of the GPU test."""
    R = DTYPE[precision]
    worst = 0.0
    for nx, ny in jr.GRIDS:
        p, op = jr.case(config, nx, ny, precision)
        y, d = jr.start_state(p, 1), jr.direction(p, 2)
        for t in jr.TIMES:
            for part in jr.PARTS:
                w = eb.check("kernel-order Jv %s %s %dx%d t=%g %s" % (precision, config[0], nx, ny, t, part), jr.kernel_order_jtimes(op, t, y, d, R, part),
                             jr.jtimes_bound(op, t, y, d, precision, part))
                worst = max(worst, w["u"][0], w["v"][0])
                if part != jr.FULL:
                    w = eb.check("kernel-order part %s %s %dx%d t=%g %s" % (precision, config[0], nx, ny, t, part), jr.kernel_order_part(op, t, y, R, part),
                                 jr.part_bound(op, t, y, precision, part))
                    worst = max(worst, w["u"][0], w["v"][0])
    print("BOUND kernel order %s %s: worst err/bound %.3g" % (precision, config[0], worst))
    assert worst > 0.01 or config[0] == "goldbeter-just-diffusion" and worst > 0.0, "a bound a hundred times the error gates nothing"


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("mutant", ["seam", "a11", "transpose", "nowrap"])
def test_mutants_miss_the_bound(mutant, precision):
    """A theta-seam neighbour one column off, 3 - u^2 for 3 - 3 u^2, the off-diagonal entries transposed, a phi neighbour not wrapped:
    each exceeds the bound on J v by more than 10x, on every grid."""
    R = DTYPE[precision]
    for nx, ny in jr.GRIDS:
        p, op = jr.case(jr.CONFIGS[0], nx, ny, precision)
        y, d = jr.start_state(p, 1), jr.direction(p, 2)
        bounded = jr.jtimes_bound(op, 0.75, y, d, precision, jr.FULL)
        w = eb.worst(jr.kernel_order_jtimes(op, 0.75, y, d, R, jr.FULL, mutant), *bounded)
        assert max(w["u"][0], w["v"][0]) > 10.0, (mutant, nx, ny, w)
        w = eb.worst(jr.kernel_order_jtimes(op, 0.75, y, d, R, jr.FULL), *bounded)
        assert max(w["u"][0], w["v"][0]) <= 1.0
    if mutant == "transpose":  # ... and in the Goldbeter block, whose entries are not constants
        p, op = jr.case(jr.CONFIGS[2], 130, 33, precision)
        y, d = jr.start_state(p, 1), jr.direction(p, 2)
        w = eb.worst(jr.kernel_order_jtimes(op, 0.75, y, d, R, jr.REACTION, mutant), *jr.jtimes_bound(op, 0.75, y, d, precision, jr.REACTION))
        assert max(w["u"][0], w["v"][0]) > 10.0


def test_reference_diffusion_is_the_oracles():
    """J_D v of the reference IS crd_oracle_np.diffusion on v's activator (the operator is linear), zero rows apart."""
    p, op = jr.case(jr.CONFIGS[0], 61, 9)
    y, d = jr.start_state(p, 1), jr.direction(p, 2)
    P = eb._Problem(op)
    ref, _, _ = jr.jtimes_bound(op, 0.75, y, d, "f64", jr.DIFFUSION)
    assert np.array_equal(ref[..., 0], cn.diffusion(P.surface, P.g, P.D, d[..., 0].astype(np.longdouble), np.longdouble))
    assert not ref[..., 1].any()
