"""The linear solve's reference on the host (tests/krylov_reference.py): the kernel-order restatement passes every gate the device is
held to in tests/test_gpu_krylov.py -- the multi-dot's bound, the orthogonality of the basis, the iteration count and the residual's
allowance -- and each mutant is rejected by the gate that claims it; crd_krylov_host.h's Givens / least-squares code runs its selftest as
a stand-alone program, once more under AddressSanitizer + UndefinedBehaviorSanitizer; the C ABI's new entries agree with the header.
No GPU.
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
import krylov_reference as kr
import multigrid_reference as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("crd_lsolve_defaults", "crd_lsolve_info", "crd_lsolve_device", "crd_lsolve_host", "crd_krylov_probe_dots")
T_ON, T_AT, T_OFF = jr.TIMES


# ---- gate 1: the multi-dot --------------------------------------------------------------------------------------------------------
def dots_gate(got, V, w):
    """Largest |h_i - ref| / bound."""
    ref, bound, _ = kr.dots_bound(V, w)
    return float((np.abs(np.asarray(got).astype(np.longdouble) - ref).astype(np.float64) / bound).max())


def test_the_summation_tree_is_counted():
    assert kr.grid(1026) == 5 and kr.dot_roundings(1026) == 17  # 19 x 27
    assert kr.grid(132000) == 512 and kr.dot_roundings(132000) == 25  # 264 x 250: a second grid-stride trip
    assert kr.grid(131072) == 512 and kr.dot_roundings(131072) == 24  # the cap exactly: one trip
    assert kr.dot_roundings(2 * 8192 * 8192) == 1024 + 23
    assert kr.plant_positions(1026) == [0, 63, 64, 255, 256, 1025]
    assert kr.plant_positions(132000) == [0, 63, 64, 255, 256, 131071, 131072, 131999]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("n", [1026, 132000], ids=["19x27", "264x250"])
def test_kernel_order_dots_within_the_bound_and_mutants_outside(n, precision):
    R = kr.DTYPES[precision]
    positions = kr.plant_positions(n)
    for count in (1, kr.GROUP, kr.GROUP + 1, 31):
        for shift in range(len(positions) if count == 1 else 1):
            V, w, where = kr.planted(n, count, positions[shift:] + positions[:shift], R)
            _, _, sizes = kr.dots_bound(V, w)
            for i, q in enumerate(where):
                assert abs(float(V[i, q]) * float(w[q])) >= 0.5 * sizes[i]  # the planted element carries the sum
            assert dots_gate(kr.kernel_order_dots(V, w), V, w) <= 1.0, (n, count, shift)
            # every mutant that changes anything here is outside (even the noise it drops is far above the bound): all but the slot
            # shift of a single vector and the second trip of a vector that has none
            for mutant in kr.DOT_MUTANTS:
                changes = count > 1 if mutant == "slot_shift" else (n > kr.grid(n) * kr.THREADS if mutant == "first_trip" else True)
                q = dots_gate(kr.kernel_order_dots(V, w, mutant), V, w)
                assert (q > 1.0) == changes, (mutant, n, count, shift, q)


# ---- gates 2 and 3: the solve -----------------------------------------------------------------------------------------------------
def problem(nx, ny, surface="torus"):
    return jr.problem_of("fhn", surface, nx, ny, 1.25, t_boundary=jr.T_BOUNDARY)


def rhs(nx, ny, R, seed=5):
    return np.random.default_rng(seed).standard_normal((ny, nx, 2)).astype(R)


def solve_gate(op, t, gamma, r, precision, got, reference, rtol, count_slack=0):
    """The gate of tests/test_gpu_krylov.py on a Result-like (z, iterations, res_norm): the count, and both residuals inside the allowance."""
    res, allowed = kr.residual_allowance(op, t, gamma, None, got.z, r, precision, jr.DIFFUSION, rtol)
    return abs(got.iterations - reference.iterations) <= count_slack and got.res_norm <= allowed and res <= allowed, (got.iterations, reference.iterations, res, allowed)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_kernel_order_solve_passes_every_gate_and_mutants_do_not(precision):
    R = kr.DTYPES[precision]
    nx, ny, t = 32, 128, T_OFF
    op = problem(nx, ny)
    gamma = 20.0 * mg.explicit_bound(op)
    r = rhs(nx, ny, R)
    full = kr.reference_solve(op, t, gamma, r, precision, rtol=0.0, max_iters=20)
    floor = 0.0 if precision == "f64" else 100 * kr.UNIT["f32"]
    pick = kr.tolerance_between(full.history, full.r_norm, floor)
    assert pick is not None, full.history
    rtol, iterations = pick
    reference = kr.reference_solve(op, t, gamma, r, precision, rtol=rtol)
    assert reference.converged and reference.iterations == iterations
    got = kr.kernel_order_solve(op, t, gamma, r, R, rtol=rtol)
    ok, detail = solve_gate(op, t, gamma, r, precision, got, reference, rtol, 0 if precision == "f64" else 1)
    assert ok and got.converged, detail
    assert np.array_equal(got.z[..., 1], r[..., 1])
    assert kr.orthogonality(got.basis) <= kr.orthogonality_allowance(len(got.basis), r.size, precision)
    for mutant in ("no_final_m", "givens_sign"):
        bad = kr.kernel_order_solve(op, t, gamma, r, R, rtol=rtol, mutant=mutant)
        ok, detail = solve_gate(op, t, gamma, r, precision, bad, reference, rtol, 0 if precision == "f64" else 1)
        assert not ok, (mutant, detail)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_one_gram_schmidt_pass_loses_the_basis(precision):
    """Iterated until the residual has fallen by more than 1 / sqrt(u) (but not to the rounding floor), one pass of classical Gram-Schmidt
    has lost the basis; two passes keep it inside the allowance."""
    R = kr.DTYPES[precision]
    nx, ny = 32, 128
    op = problem(nx, ny)
    gamma = 20.0 * mg.explicit_bound(op)
    r = rhs(nx, ny, R)
    columns = 10 if precision == "f64" else 4
    kw = dict(restart=30, max_iters=columns, rtol=0.0)
    good = kr.kernel_order_solve(op, T_OFF, gamma, r, R, **kw)
    bad = kr.kernel_order_solve(op, T_OFF, gamma, r, R, mutant="one_pass", **kw)
    allowed = kr.orthogonality_allowance(columns, r.size, precision)
    assert len(good.basis) == len(bad.basis) == columns and 10 * kr.UNIT[precision] < good.res_norm / good.r_norm < np.sqrt(kr.UNIT[precision])
    assert kr.orthogonality(good.basis) <= allowed < kr.orthogonality(bad.basis), (kr.orthogonality(good.basis), allowed, kr.orthogonality(bad.basis))


def test_restart_exhaustion_and_breakdown_in_the_restatement():
    nx, ny = 64, 16
    op = jr.problem_of("goldbeter", "torus", nx, ny, 0.4, t_boundary=jr.T_BOUNDARY)
    gamma = 20.0 * mg.explicit_bound(op)
    r = rhs(nx, ny, np.float64)
    for solve in (lambda **kw: kr.reference_solve(op, T_ON, gamma, r, "f64", **kw), lambda **kw: kr.kernel_order_solve(op, T_ON, gamma, r, np.float64, **kw)):
        a = solve(restart=10)
        assert a.converged and a.restarts >= 2, (a.restarts, a.iterations)
        res, allowed = kr.residual_allowance(op, T_ON, gamma, None, a.z, r, "f64", jr.DIFFUSION, 1e-8)
        assert res <= allowed
        b = solve(max_iters=7)
        assert not b.converged and b.iterations == 7 and np.isfinite(b.z.astype(np.float64)).all()
        assert kr.residual_allowance(op, T_ON, gamma, None, b.z, r, "f64", jr.DIFFUSION, 0.0)[0] < b.r_norm
    # a uniform field diffuses to exactly zero: A v_0 = v_0, the first column is a breakdown
    u = np.full((ny, nx, 2), 0.75)
    for res in (kr.reference_solve(op, T_OFF, gamma, u, "f64", precondition=False), kr.kernel_order_solve(op, T_OFF, gamma, u, np.float64, precondition=False)):
        assert res.converged and res.breakdown and res.iterations == 1
        assert np.all(np.abs(res.z.astype(np.float64) - u) <= 4 * kr.UNIT["f64"] * np.abs(u))
    for g, rr in ((0.0, r), (gamma, np.zeros_like(r))):
        res = kr.kernel_order_solve(op, T_OFF, g, rr, np.float64)
        assert res.iterations == 0 and np.array_equal(res.z, rr)


# ---- crd_krylov_host.h ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("sanitizers", [None, "address,undefined"])
def test_krylov_host_selftest(tmp_path, sanitizers):
    exe = tmp_path / "krylov_host_selftest"
    build = subprocess.run(kr.selftest_build_command(exe, sanitizers), capture_output=True, text=True)
    if sanitizers and build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "krylov host selftest ok" in run.stdout


def test_the_host_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "crdmodel_amd", "csrc", "crd_krylov_host.h")).read()
    assert [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")] == ["<cmath>", "<vector>"]
    assert not [word for word in ("hip/", "hipError_t", "hipStream_t", "__global__", "__device__") if word in text]


def test_python_least_squares_is_the_headers():
    """The restatement's LeastSquares on the selftest's cases: the two stay one algorithm."""
    ls = kr.LeastSquares(3, 3.0)
    for col in ([2.0, 1.0], [1.0, 3.0, 2.0], [0.5, 1.0, 1.0, 0.5]):
        ls.push(col, kr.U64)
    H = np.array([[2, 1, 0.5], [1, 3, 1], [0, 2, 1], [0, 0, 0.5]])
    y, *_ = np.linalg.lstsq(H, np.array([3.0, 0, 0, 0]), rcond=None)
    assert np.allclose(ls.solve(), y, rtol=0, atol=1e-14) and abs(ls.residual() - np.linalg.norm(H @ y - [3.0, 0, 0, 0])) <= 1e-14
    ls = kr.LeastSquares(30, 7.0)
    ls.push([2.0, 0.0], kr.U64)
    assert ls.breakdown and ls.full() and ls.residual() == 0 and ls.solve()[0] == 3.5


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
    K = crd._capi
    assert [f for f, _ in K.LsolveOptions._fields_] == ["part", "precondition", "restart", "max_iters", "rtol", "atol", "psolve"] and C.sizeof(K.LsolveOptions) == 56
    assert [f for f, _ in K.LsolveStats._fields_] == ["converged", "iterations", "restarts", "matvecs", "psolves", "breakdown", "r_norm", "res_norm"]
    assert C.sizeof(K.LsolveStats) == 40
    assert int(re.search(r"#define CRD_ABI_VERSION (\d+)", header).group(1)) == 8  # additions only
    assert hasattr(crd.Slab, "lsolve") and hasattr(crd.Slab, "lsolve_info")


def test_defaults_and_null_arguments():
    K = crd._capi
    L = K.lib()
    opt = K.LsolveOptions()
    assert L.crd_lsolve_defaults(C.byref(opt)) == K.OK
    assert (opt.part, opt.precondition, opt.restart, opt.max_iters, opt.rtol, opt.atol) == (K.PART_DIFFUSION, 1, 30, 200, 1e-8, 0.0)
    assert {k: getattr(opt.psolve, k) for k in mg.DEFAULTS} == mg.DEFAULTS
    assert L.crd_lsolve_defaults(None) == K.EINVAL
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    assert L.crd_lsolve_device(None, 0.0, 1.0, None, p, p, p, None) == K.EINVAL
    assert L.crd_lsolve_host(None, 0.0, 1.0, None, p, p, p, None) == K.EINVAL
    assert L.crd_lsolve_info(None, None, None) == K.EINVAL
    assert L.crd_krylov_probe_dots(None, p, 1, p, buf) == K.EINVAL


def test_header_compiles_as_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "lsolve.c"
    src.write_text(r'''
#include <stddef.h>
#include "crd.h"
int main(void) {
	double r[4] = {0, 0, 0, 0}, z[4];
	int64_t bytes;
	crd_lsolve_options o;
	crd_lsolve_stats st;
	if (crd_lsolve_defaults(&o) != CRD_OK || o.part != CRD_PART_DIFFUSION || o.precondition != 1 || o.restart != 30 || o.max_iters != 200) return 1;
	if (o.rtol != 1e-8 || o.atol != 0.0 || o.psolve.pre != 2 || o.psolve.omega != 0.8) return 2;
	if (crd_lsolve_info(NULL, &o, &bytes) != CRD_EINVAL) return 3;
	if (crd_lsolve_device(NULL, 0.0, 1.0, &o, NULL, r, z, &st) != CRD_EINVAL) return 4;
	if (crd_lsolve_host(NULL, 0.0, 1.0, NULL, NULL, r, z, NULL) != CRD_EINVAL) return 5;
	if (crd_abi_version() != 8) return 6;
	return 0;
}
''')
    exe = tmp_path / "lsolve"
    libdir = os.path.dirname(crd._capi.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lcrd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
