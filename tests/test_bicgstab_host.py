"""CPU-side checks of the BiCGStab solve (crd_bicgstab_*): the long-double reference against a dense solve, the kernel-order restatement
against every gate the device is held to in tests/test_gpu_bicgstab.py, mutants against the gate that claims each, crd_bicgstab_host.h
through its stand-alone selftest and against the Python restatement bit for bit, and the ABI mirrors.  No kernel is launched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bicgstab_reference as br
import crdmodel_amd as crd
import imex_reference as ir
import jacobian_reference as jr
import krylov_reference as kr
import multigrid_reference as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("crd_bicgstab_defaults", "crd_bicgstab_info", "crd_bicgstab_device", "crd_bicgstab_host", "crd_bicgstab_probe")
T_ON, T_AT, T_OFF = jr.TIMES


def problem(nx, ny, surface="torus", model="fhn", beta=1.25, **kw):
    return jr.problem_of(model, surface, nx, ny, beta, t_boundary=jr.T_BOUNDARY, **kw)


def rhs(nx, ny, R, seed=5):
    return np.random.default_rng(seed).standard_normal((ny, nx, 2)).astype(R)


# ---- 1. the reference against a dense solve ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [T_ON, T_OFF], ids=["held", "free"])
def test_reference_solves_the_dense_system(t):
    nx, ny = 12, 16
    op = problem(nx, ny)
    D = ir.Dense(op)
    gamma, rtol = 20.0 * mg.explicit_bound(op), 1e-10
    r = rhs(nx, ny, np.float64)
    A = np.eye(nx * ny) - gamma * D.L(t)
    exact = np.linalg.solve(A, r[..., 0].ravel())
    ref = br.reference_solve(op, t, gamma, r, "f64", rtol=rtol)
    assert ref.converged and ref.breakdown == 0 and len(ref.history) == 1 + br.half_steps(ref)
    tol = rtol * ref.r_norm
    kappa = D.norms(t, gamma)[0]
    assert np.linalg.norm(ref.z[..., 0].ravel().astype(np.float64) - exact) <= kappa * tol + 1e-13 * np.linalg.norm(exact)
    assert np.array_equal(ref.z[..., 1], r[..., 1])
    assert ref.true_res_norm <= 1.01 * tol and (ref.matvecs, ref.psolves) == br.implied_counts(ref.iterations, ref.half_exit)


# ---- 2. the sums' tree ------------------------------------------------------------------------------------------------------------
def test_the_summation_tree_is_counted():
    assert (br.grid(1026, "f64"), br.sum_roundings(1026, "f64")) == (3, 18) and (br.grid(1026, "f32"), br.sum_roundings(1026, "f32")) == (2, 20)
    for precision in ("f64", "f32"):
        nx, ny = br.smallest_grid_above_one_trip(precision)
        n = 2 * nx * ny
        assert br.trips(n, precision) == 2 and br.trips(2 * nx * (ny - 1), precision) == 1 and br.grid(n, precision) == br.BLOCKS
        assert br.sum_roundings(n, precision) == 2 * br.REALS[precision] + 15 + 32
        first = br.BLOCKS * br.THREADS * br.REALS[precision]
        assert br.plant_positions(n, precision)[-3:] == [first - 1, first, n - 1]
    assert br.plant_positions(1026, "f64") == [0, 127, 128, 511, 512, 1025] and br.plant_positions(1026, "f32") == [0, 255, 256, 1023, 1024, 1025]
    assert br.sum_roundings(2 * 8192 * 8192, "f64") == 2 * 128 + 15 + 32


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("big", [False, True], ids=["19x27", "two-trips"])
def test_kernel_order_sums_within_the_bound_and_mutants_outside(big, precision):
    nx, ny = br.smallest_grid_above_one_trip(precision) if big else (19, 27)
    n = 2 * nx * ny
    positions = br.plant_positions(n, precision)
    for kernel in ("apply_dot2", "xr_update") if big else [k for k in br.KERNELS if br.KERNELS[k][3]]:
        for i, q1 in enumerate(positions if not big else positions[-3:]):
            q2 = positions[(positions.index(q1) + 1) % len(positions)]
            ins = br.planted_case(kernel, n, precision, q1, q2)
            outs, pairs = br.kernel_reference(kernel, ins, br.SCALARS[kernel], precision)
            for (a, b), q in zip(pairs, br.carriers(kernel, q1, q2)):
                assert abs(float(a[q]) * float(b[q])) >= 0.5 * br.sum_bound(a, b, precision)[2]  # the planted element carries the sum
            assert br.sums_gate([br.kernel_order_sum(a, b, precision) for a, b in pairs], pairs, precision) <= 1.0, (kernel, q1)
            for mutant in br.SUM_MUTANTS:
                changes = br.trips(n, precision) > 1 if mutant == "first_trip" else True
                q = br.sums_gate([br.kernel_order_sum(a, b, precision, mutant) for a, b in pairs], pairs, precision)
                assert (q > 1.0) == changes, (kernel, mutant, q1, q)


# ---- 3. the solve in the kernels' order, and the mutants --------------------------------------------------------------------------
def gates(op, t, gamma, r, precision, got, reference, rtol):
    """The gates of tests/test_gpu_bicgstab.py on a Result: {gate: passed}."""
    res, allowed = kr.residual_allowance(op, t, gamma, None, got.z, r, precision, jr.DIFFUSION, rtol)
    slack = 0 if precision == "f64" else 1
    return {"count": bool(got.converged) and abs(br.half_steps(got) - br.half_steps(reference)) <= slack,
            "true_residual": res <= allowed and got.true_res_norm <= allowed,
            "var1": np.array_equal(got.z[..., 1], r[..., 1])}


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_kernel_order_solve_passes_every_gate_and_mutants_do_not(precision):
    nx, ny, t = 32, 128, T_ON
    op = problem(nx, ny)
    gamma = 500.0 * mg.explicit_bound(op)
    r = rhs(nx, ny, kr.DTYPES[precision])
    full = br.reference_solve(op, t, gamma, r, precision, rtol=0.0, max_iters=12)
    pick = kr.tolerance_between(full.history, full.r_norm, 0.0 if precision == "f64" else 100 * kr.UNIT["f32"], near=1e-8 if precision == "f64" else 1e-5)
    assert pick is not None, full.history
    rtol = pick[0]
    reference = br.reference_solve(op, t, gamma, r, precision, rtol=rtol)
    assert reference.converged and br.half_steps(reference) == pick[1] and br.half_steps(reference) >= 4
    got = br.kernel_order_solve(op, t, gamma, r, precision, rtol=rtol)
    assert all(gates(op, t, gamma, r, precision, got, reference, rtol).values()), gates(op, t, gamma, r, precision, got, reference, rtol)
    assert (got.matvecs, got.psolves) == br.implied_counts(got.iterations, got.half_exit) and got.breakdown == 0
    # (the count gate's mutants in fp64, where the gate has no slack: in fp32 it allows a half-step either way, and at a tolerance near
    # 1e-5 the solve is over before beta or the direction's v term has entered more than once)
    for mutant in ("x_without_omega", "var1_unmasked") + (("beta_without_ratio", "p_without_v", "omega_over_ss") if precision == "f64" else ()):
        bad = br.kernel_order_solve(op, t, gamma, r, precision, rtol=rtol, mutant=mutant)
        assert not gates(op, t, gamma, r, precision, bad, reference, rtol)[br.MUTANT_GATES[mutant]], mutant


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_half_exit_and_its_mutant(precision):
    """A uniform field diffuses to exactly zero, so A p = p: alpha = 1, s = 0, the half exit.  Without x += alpha phat, z stays 0."""
    nx, ny = 48, 40
    op = problem(nx, ny)
    u = np.full((ny, nx, 2), 0.75, dtype=kr.DTYPES[precision])
    gamma = 20.0 * mg.explicit_bound(op)
    for solve in (br.reference_solve, br.kernel_order_solve):
        res = solve(op, T_OFF, gamma, u, precision, precondition=False)
        assert (res.converged, res.iterations, res.half_exit, res.breakdown) == (1, 1, 1, 0)
        assert np.all(np.abs(res.z.astype(np.float64) - u.astype(np.float64)) <= 4 * kr.UNIT[precision] * np.abs(u.astype(np.float64)))
        assert (res.matvecs, res.psolves) == br.implied_counts(1, 1, precondition=False)
    bad = br.kernel_order_solve(op, T_OFF, gamma, u, precision, precondition=False, mutant="half_exit_without_x")
    res, allowed = kr.residual_allowance(op, T_OFF, gamma, None, bad.z, u, precision, jr.DIFFUSION, 1e-8)
    assert res > allowed and bad.true_res_norm > allowed


def test_exhaustion_guess_and_trivial_exits_in_the_restatement():
    nx, ny = 64, 16
    op = problem(nx, ny, model="goldbeter", beta=0.4)
    gamma = 20.0 * mg.explicit_bound(op)
    r = rhs(nx, ny, np.float64)
    full = br.reference_solve(op, T_ON, gamma, r, "f64")
    assert full.converged and full.iterations > 4
    for solve in (br.reference_solve, br.kernel_order_solve):
        b = solve(op, T_ON, gamma, r, "f64", max_iters=4)
        assert (b.converged, b.iterations) == (0, 4) and np.isfinite(b.z.astype(np.float64)).all()
        assert kr.residual_allowance(op, T_ON, gamma, None, b.z, r, "f64", jr.DIFFUSION, 0.0)[0] < b.r_norm
        # a converged z as the guess: no iteration; 1.01 x the solution: fewer than cold
        warm = solve(op, T_ON, gamma, r, "f64", guess=full.z.astype(np.float64), rtol=1e-6)
        assert (warm.converged, warm.iterations, warm.matvecs) == (1, 0, 2)
        near = solve(op, T_ON, gamma, r, "f64", guess=1.01 * full.z.astype(np.float64))
        assert near.converged and br.half_steps(near) < br.half_steps(full)
    cold = br.kernel_order_solve(op, T_ON, gamma, r, "f64")
    zero = br.kernel_order_solve(op, T_ON, gamma, r, "f64", guess=np.zeros_like(r))
    assert np.array_equal(cold.z, zero.z) and zero.matvecs == cold.matvecs + 1
    for g, rr in ((0.0, r), (gamma, np.zeros_like(r))):
        res = br.kernel_order_solve(op, T_OFF, g, rr, "f64")
        assert res.iterations == 0 and res.converged and np.array_equal(res.z, rr)
    bad = r.copy()
    bad[3, 5, 0] = np.nan
    res = br.kernel_order_solve(op, T_OFF, gamma, bad, "f64")
    assert (res.converged, res.iterations, res.breakdown) == (0, 0, 0)


# ---- 3b. the IMEX step with the BiCGStab solve, against the dense restatement ------------------------------------------------------
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("scheme", ir.SCHEMES)
def test_imex_allowance_holds_for_the_restatement(scheme, warm):
    """The case of tests/test_gpu_imex_bicgstab.py: test_against_the_dense_restatement (16 x 24 points of a 1 x 2 torus, three steps from
    tBoundary - 1.4 dt at 5 x crd_stable_dt, the solves at rtol = 1e-10), composed on the CPU from the kernel-order solve.  The allowance
    of imex_reference is given the solves' OWN largest true_res_norm / r_norm as the bound on a solve's residual -- the recurrence's
    residual is what met rtol, and the true one may sit a rounding above it -- and the step must be inside it; that figure itself may
    not exceed 2 rtol."""
    geometry = dict(L=2.0, W=1.0, D=0.12)
    dt = 5.0 * crd.stable_dt(crd.make_params("fhn", "torus", 16, 2.0, 1.0, 0.12, 1.25, ny=24))
    kw = dict(vary_beta=1, beta_min=0.3, beta_max=1.4)
    assert jr.CONFIGS[0][1:] == ("fhn", "torus", 1.25, kw)
    p = crd.make_params("fhn", "torus", 16, 2.0, 1.0, 0.12, 1.25, ny=24, t_boundary=10.0 * dt, **kw)
    op = jr.problem_of("fhn", "torus", 16, 24, 1.25, t_boundary=10.0 * dt, **geometry, **kw)
    y0, rtol = jr.start_state(p, 2), 1e-10
    got, solves = br.kernel_order_imex_steps(op, scheme, 8.6 * dt, dt, 3, y0, "f64", warm=warm, rtol=rtol)
    worst = max(r.true_res_norm / r.r_norm for r in solves)
    assert len(solves) == 3 * ir.tableau(scheme)[0] and all(r.res_norm <= rtol * r.r_norm for r in solves) and rtol / 1e3 < worst <= 2 * rtol, worst
    allowed, expected = ir.steps_allowance(ir.Dense(op), scheme, 8.6 * dt, dt, 3, y0, worst)
    err = float(np.linalg.norm(got - expected))
    assert np.isfinite(expected).all() and err <= allowed, (err, allowed, worst)
    if warm:  # the chain of guesses is used: the solves after the first start below ||r||
        assert all(r.matvecs == br.implied_counts(r.iterations, r.half_exit, guess=True)[0] for r in solves[1:]) and solves[0].matvecs == br.implied_counts(solves[0].iterations, solves[0].half_exit)[0]


# ---- 4. crd_bicgstab_host.h -------------------------------------------------------------------------------------------------------
def _run_selftest(tmp_path, sanitizers):
    exe = tmp_path / "bicgstab_host_selftest"
    build = subprocess.run(br.selftest_build_command(exe, sanitizers), capture_output=True, text=True)
    if sanitizers and build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "bicgstab host selftest ok" in run.stdout
    return run.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("sanitizers", [None, "address,undefined"])
def test_bicgstab_host_selftest(tmp_path, sanitizers):
    _run_selftest(tmp_path, sanitizers)


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or (a == b and np.signbit(a) == np.signbit(b))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_python_recurrence_is_the_headers(tmp_path):
    """Every scripted sequence of the selftest replayed through bicgstab_reference.Recurrence: the same decision after every reduction
    and the same rho, alpha, omega, beta and residual norm, bit for bit."""
    k, scripts, steps = None, 0, 0
    for line in _run_selftest(tmp_path, None).splitlines():
        w = line.split()
        if w and w[0] == "script":
            k = br.Recurrence(float.fromhex(w[3]), int(w[4]), f32=w[2] == "1")
            scripts += 1
        elif w and w[0] == "op":
            a, b = float.fromhex(w[2]), float.fromhex(w[3])
            go = {"s": lambda: k.start(a), "d": lambda: k.take_d(a), "n": lambda: k.take_s(a), "t": lambda: k.take_t(a, b), "r": lambda: k.take_res(a, b)}[w[1]]()
            want = w[5:]
            assert int(go) == int(want[0]), line
            for got, text in zip((k.rho, k.alpha, k.omega, k.beta, k.res_norm), want[1:6]):
                assert _same(float(got), float.fromhex(text)), (line, float(got))
            assert [k.iterations, k.half_exit, k.breakdown, k.converged] == [int(v) for v in want[6:10]], line
            steps += 1
    assert scripts >= 20 and steps >= 60


def test_the_host_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "crdmodel_amd", "csrc", "crd_bicgstab_host.h")).read()
    assert [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")] == ["<cmath>"]
    assert not [word for word in ("hip/", "hipError_t", "hipStream_t", "__global__", "__device__") if word in text]


# ---- 5. the ABI -------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_agree():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crd.h")).read(), flags=re.S)
    L = C.CDLL(crd._capi.LIB_PATH)
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m and hasattr(L, name), name
        res, args = crd._capi._SIGNATURES[name]
        assert res is C.c_int and len(args) == len(m.group(1).split(",")), (name, m.group(1))
    K = crd._capi
    assert [f for f, _ in K.BicgstabOptions._fields_] == ["part", "precondition", "max_iters", "guess", "rtol", "atol", "psolve"]
    assert [f for f, _ in K.BicgstabStats._fields_] == ["converged", "iterations", "half_exit", "matvecs", "psolves", "breakdown", "r_norm", "res_norm", "true_res_norm"]
    assert int(re.search(r"#define CRD_ABI_VERSION (\d+)", header).group(1)) == 8 == K.ABI_VERSION  # additions only
    assert C.sizeof(K.LsolveOptions) == 56 and K.ImexOptions.solver.offset == 4 and K.ImexOptions.solver.size == 4 and C.sizeof(K.ImexOptions) == 64
    for name, value in list(K.BICGSTAB_BREAKDOWNS.items()) + [("kernel_" + k, v) for k, v in K.BICGSTAB_KERNELS.items()]:
        assert re.search(r"\bCRD_BICGSTAB_(BREAKDOWN_)?%s = %d\b" % (name.upper(), value), header), name
    for name, value in K.IMEX_SOLVERS.items():
        assert re.search(r"\bCRD_IMEX_SOLVER_%s = %d\b" % (name.upper().replace("-", "_"), value), header), name
    assert all(hasattr(crd.Slab, m) for m in ("lsolve_bicgstab", "lsolve_bicgstab_info"))


def test_defaults_and_null_arguments():
    K = crd._capi
    L = K.lib()
    opt = K.BicgstabOptions()
    assert L.crd_bicgstab_defaults(C.byref(opt)) == K.OK
    assert (opt.part, opt.precondition, opt.max_iters, opt.guess, opt.rtol, opt.atol) == (K.PART_DIFFUSION, 1, 200, 0, 1e-8, 0.0)
    assert {k: getattr(opt.psolve, k) for k in mg.DEFAULTS} == mg.DEFAULTS
    assert L.crd_bicgstab_defaults(None) == K.EINVAL
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    assert L.crd_bicgstab_device(None, 0.0, 1.0, None, p, p, p, None) == K.EINVAL
    assert L.crd_bicgstab_host(None, 0.0, 1.0, None, p, p, p, None) == K.EINVAL
    assert L.crd_bicgstab_info(None, None, None) == K.EINVAL
    assert L.crd_bicgstab_probe(None, 0, 0, buf, p, p, buf) == K.EINVAL
    io = K.ImexOptions()
    assert L.crd_imex_defaults(C.byref(io)) == K.OK and io.solver == K.IMEX_SOLVERS["gmres"] == 0


def test_struct_layouts_match_a_c_compiler(tmp_path):
    """A C99 program prints sizeof / offsetof of the two new structures and of crd_imex_options.solver: they are _capi's."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    K = crd._capi
    fields = [("crd_bicgstab_options", K.BicgstabOptions, [f for f, _ in K.BicgstabOptions._fields_]),
              ("crd_bicgstab_stats", K.BicgstabStats, [f for f, _ in K.BicgstabStats._fields_]), ("crd_imex_options", K.ImexOptions, ["scheme", "solver", "lsolve"]),
              ("crd_lsolve_options", K.LsolveOptions, ["psolve"])]
    prints = "".join('\tprintf("%%ld", (long)sizeof(%s));%s\n\tprintf("\\n");\n' % (s, "".join(' printf(" %%ld", (long)offsetof(%s, %s));' % (s, f) for f in fs))
                     for s, _, fs in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crd.h"\nint main(void) {\n%s\tif (crd_abi_version() != 8 || CRD_ABI_VERSION != 8) return 1;\n\treturn 0;\n}\n' % prints)
    exe = tmp_path / "layout"
    libdir = os.path.dirname(K.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lcrd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    for line, (_, T, fs) in zip(run.stdout.splitlines(), fields):
        assert [int(v) for v in line.split()] == [C.sizeof(T)] + [getattr(T, f).offset for f in fs], (line, T)
    assert C.sizeof(K.BicgstabOptions) == 56 and C.sizeof(K.BicgstabStats) == 48
