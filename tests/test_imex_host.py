"""The IMEX stepper's host side, without a GPU: the three tableaux against their order conditions, crd_imex_tables.h's own self-test
(plain, and under ASan + UBSan), the Python restatement's coefficients against the header's bit for bit, and the dense restatement of
the step (tests/imex_reference.py): its observed order on a smooth FHN problem against a small-step RK4 solution of the oracle's f, a
step that straddles tBoundary against a hand-written Euler step, and mutants that must each fail one of those assertions.
"""
import functools
import os
import subprocess
from fractions import Fraction as Fr

import numpy as np
import pytest

import crdmodel_amd as crd
import imex_reference as ir
import jacobian_reference as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The observed slope log2(err(dt) / err(dt / 2)) of an order-p scheme tends to p; p - 1 and p + 1 are the neighbours it has to be told
# from, so the bracket is the open interval between the midpoints, (p - 1/2, p + 1/2).
HALF = 0.5


# ---- the tableaux -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ir.SCHEMES)
def test_order_conditions(scheme):
    """Exactly, in Fractions, for euler and ars443; to 4 ulps of 1 for ars222, whose gamma is irrational.  The conditions of the next
    order do NOT all hold: the schemes have the orders they claim and no more."""
    p = ir.ORDER[scheme]
    res = ir.order_residuals(scheme)
    tol = 0 if scheme != "ars222" else 4 * 2.0 ** -52
    for name, r in res.items():
        if ir.condition_order(name) <= p:
            assert abs(r) <= tol, (scheme, name, r)
            if scheme != "ars222":
                assert isinstance(r, Fr) and r == 0
    if p < 3:
        assert any(abs(r) > 1e-3 for name, r in res.items() if ir.condition_order(name) == p + 1), scheme


@pytest.mark.parametrize("scheme", ir.SCHEMES)
def test_structure(scheme):
    s, c, AE, AI, g = ir.exact(scheme)
    assert c[0] == 0 and c[s] == 1
    for i in range(s + 1):
        assert AI[i][0] == 0 and all(AE[i][j] == 0 for j in range(i, s + 1)) and all(AI[i][j] == 0 for j in range(i + 1, s + 1))
        if i >= 1:
            assert AI[i][i] == g


@pytest.mark.parametrize("sanitizers", [None, "address,undefined"])
def test_tables_selftest_and_its_coefficients(tmp_path, sanitizers):
    exe = tmp_path / "imex_tables_selftest"
    build = subprocess.run(ir.selftest_build_command(exe, sanitizers), capture_output=True, text=True)
    if sanitizers and build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "imex tables selftest ok" in run.stdout
    # the header's doubles are the restatement's, bit for bit
    seen, scheme = set(), None
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] in ir.SCHEMES:
            scheme = w[0]
            s, c, AE, AI, g = ir.tableau(scheme)
            assert (int(w[1]), int(w[2]), float.fromhex(w[3])) == (s, ir.ORDER[scheme], g)
            seen.add(scheme)
        elif w[0] == "c":
            assert float.fromhex(w[2]) == c[int(w[1])], line
        elif w[0] == "A":
            i, j = int(w[1]), int(w[2])
            assert (float.fromhex(w[3]), float.fromhex(w[4])) == (AE[i][j], AI[i][j + 1]), (scheme, line)
    assert seen == set(ir.SCHEMES)


def test_the_tables_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "crdmodel_amd", "csrc", "crd_imex_tables.h")).read()
    assert [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")] == ["<cmath>"]
    assert not [word for word in ("hip/", "hipError_t", "hipStream_t", "__global__", "__device__") if word in text]


def test_python_mirrors_the_header():
    K = crd._capi
    header = open(os.path.join(ROOT, "include", "crd.h")).read()
    for name, value in K.IMEX_SCHEMES.items():
        assert "CRD_IMEX_%s = %d" % (name.upper(), value) in header
    assert C_sizeof(K.ImexOptions) == 8 + C_sizeof(K.LsolveOptions) and C_sizeof(K.ImexStats) == 4 * 8 + 2 * 4 + 3 * 8


def C_sizeof(t):
    import ctypes

    return ctypes.sizeof(t)


# ---- the dense restatement --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def smooth_problem(surface):
    """FHN on a 12 x 16 grid of a 1 x 2 domain (D = 0.12: crd_stable_dt is 0.029 flat, 0.015 torus -- the diffusion bound), no
    absorbing rows, a smooth state, and the oracle's RK4 at T / 4096 as the solution at T = 0.4 (halving its step moves it by 1e-14)."""
    op = jr.problem_of("fhn", surface, 12, 16, 1.25, L=2.0, W=1.0, D=0.12, t_boundary=0.0)
    D = ir.Dense(op)
    y0 = ir.smooth_state(op)
    T = 0.4
    ref = ir.rk4_steps(D, 0.0, T / 4096, 4096, y0)
    assert np.abs(ref - ir.rk4_steps(D, 0.0, T / 2048, 2048, y0)).max() < 1e-12
    return D, y0, T, ref


def slopes(D, y0, T, ref, scheme, mutant=None):
    errs = [float(np.linalg.norm(ir.dense_steps(D, scheme, 0.0, T / n, n, y0, mutant) - ref)) for n in (4, 8, 16)]  # dt, dt / 2, dt / 4
    return [float(np.log2(errs[k] / errs[k + 1])) for k in range(2)], errs


def test_dense_operator_is_the_oracles():
    D, y0, _, _ = smooth_problem("torus")
    from oracle import crd_oracle_np as cn

    du, dv = cn.rhs(D.P.model, D.P.surface, D.P.g, D.P.D, 0.0, y0[..., 0], y0[..., 1], **D.P.kw)
    f = D.f(0.0, y0)
    assert np.abs(f[..., 0] - du).max() <= 1e-12 * np.abs(du).max() and np.abs(f[..., 1] - dv).max() <= 1e-13


@pytest.mark.parametrize("surface", ["flat", "torus"])
@pytest.mark.parametrize("scheme", ir.SCHEMES)
def test_observed_order(scheme, surface):
    D, y0, T, ref = smooth_problem(surface)
    got, errs = slopes(D, y0, T, ref, scheme)
    print("ORDER %s %s: errors %s, slopes %s" % (scheme, surface, ["%.3g" % e for e in errs], ["%.2f" % s for s in got]))
    p = ir.ORDER[scheme]
    assert all(p - HALF < s < p + HALF for s in got), (scheme, got)
    assert errs[-1] > 1e3 * 1e-12  # far above the solution's own error


def straddling_euler(D, mutant=None):
    """One Euler step from t < tBoundary whose only implicit stage lies behind it, against the step written out by hand: the kinetics
    at t_n hold the boundary rows, the operator at t_n + dt does not."""
    y0 = ir.smooth_state(D.op)
    tb = D.P.kw["t_boundary"]
    dt = 0.05
    t = tb - 0.5 * dt
    assert D.held(t) and not D.held(t + dt)
    n = D.ny * D.nx
    R = y0 + dt * D.f_R(t, y0)
    expected = R.copy()
    expected[..., 0] = np.linalg.solve(np.eye(n) - dt * D.L_free, R[..., 0].ravel()).reshape(D.ny, D.nx)
    got = ir.dense_step(D, "euler", t, dt, y0, mutant)
    return float(np.abs(got - expected).max()), float(np.abs(expected[0] - y0[0]).max())


@functools.lru_cache(maxsize=None)
def held_problem():
    return ir.Dense(jr.problem_of("fhn", "torus", 12, 16, 1.25, L=2.0, W=1.0, D=0.12, t_boundary=0.5))


def test_a_step_that_straddles_tboundary():
    err, moved = straddling_euler(held_problem())
    assert err <= 1e-12 and moved > 1e-4  # the boundary rows, free at the stage's time, have moved


@pytest.mark.parametrize("scheme", ["ars222", "ars443"])
@pytest.mark.parametrize("mutant", ir.MUTANTS)
def test_mutants_fail(mutant, scheme):
    """swapped_coefficient, rows_exchanged and dropped_term lose the order (test_observed_order's assertion); stage_time -- every stage
    at t_n -- leaves a smooth autonomous problem alone and fails test_a_step_that_straddles_tboundary's."""
    if mutant == "stage_time":
        err, _ = straddling_euler(held_problem(), mutant)
        assert err > 1e-6
        return
    D, y0, T, ref = smooth_problem("flat")
    got, _ = slopes(D, y0, T, ref, scheme, mutant)
    p = ir.ORDER[scheme]
    assert not all(p - HALF < s < p + HALF for s in got), (scheme, mutant, got)


def test_the_allowance_is_of_the_size_of_the_solves_tolerance():
    """step_allowance on the CPU: above what one solve's residual alone may leave (0.1 rtol dt ||f_D||), and not orders above it."""
    D, y0, _, _ = smooth_problem("torus")
    dt, rtol = 0.2, 1e-8
    for scheme in ir.SCHEMES:
        bound, y1 = ir.step_allowance(D, scheme, 0.0, dt, y0, 0.0, rtol)
        scale = float(np.linalg.norm(D.L_free @ y0[..., 0].ravel()))
        assert 0.1 * rtol * scale * dt < bound < 1e4 * rtol * scale * dt, (scheme, bound, rtol * scale * dt)
        assert np.isfinite(y1).all()


# ---- the fused multiply-add of the composition ------------------------------------------------------------------------------------
def test_fma_exact_is_correctly_rounded():
    """imex_reference.fma_exact against exact rational arithmetic on 20000 random triples and on planted ties, both precisions; and
    jacobian_reference._fma, which rounds twice, agrees with it except on a few float64 results in ten thousand -- which is why the
    bit-for-bit composition of tests/test_gpu_imex.py is written with fma_exact."""
    rng = np.random.default_rng(3)
    n = 20000
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    c = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 3, n)
    exact = lambda x, y, z: Fr(float(x)) * Fr(float(y)) + Fr(float(z))
    got = ir.fma_exact(np.float64)(a, b, c)
    ref = np.array([float(exact(x, y, z)) for x, y, z in zip(a, b, c)])  # float(Fraction) is correctly rounded
    assert np.array_equal(got, ref)
    twice = jr._fma(np.float64)(a, b, c)
    assert 0 <= int((twice != ref).sum()) <= 40 and np.abs(twice - ref).max() <= 2.0 ** -52 * np.abs(ref).max()
    # ties of the float64 result, decided by the part of the product a second rounding loses
    a = np.full(4, 1 + 2.0 ** -30)
    c = np.array([2.0 ** -53, -2.0 ** -53, 2.0 ** -53 - 2.0 ** -60, 0.0])
    assert np.array_equal(ir.fma_exact(np.float64)(a, a, c), np.array([float(exact(x, x, z)) for x, z in zip(a, c)]))
    # float32: the nearest float32 of the exact value, ties to even
    a32, b32, c32 = (x[:4000].astype(np.float32) for x in (rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)))
    c32[:8] = np.float32(1.0)
    a32[:8] = np.float32(2.0 ** -12)
    b32[:8] = np.array([2.0 ** -12, -2.0 ** -12, 3 * 2.0 ** -13, 2.0 ** -12 + 2.0 ** -30, 2.0 ** -13, 2.0 ** -11, 5 * 2.0 ** -14, 2.0 ** -12 - 2.0 ** -30], dtype=np.float32)
    got = ir.fma_exact(np.float32)(a32, b32, c32)

    def nearest32(fr):
        lo = np.float32(float(fr))
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        return min(cands, key=lambda x: (abs(Fr(float(x)) - fr), int(np.float32(x).view(np.int32)) & 1))

    assert np.array_equal(got, np.array([nearest32(exact(x, y, z)) for x, y, z in zip(a32, b32, c32)], dtype=np.float32))


# ---- the driver's refusals --------------------------------------------------------------------------------------------------------
INI = os.path.join(ROOT, "tests", "golden", "ini", "small_run.ini")
DRIVER_REFUSALS = [
    (["--imex", "rk4"], "--imex takes euler, ars222 or ars443 (got 'rk4')"),
    (["--imex", "ars222", "--gpus", "2"], "--imex steps a lone single-slab run: not with --gpus 2"),
    (["--imex", "ars222", "--decomp", "2x1"], "--imex steps a lone single-slab run: not with --decomp / --block-contexts"),
    (["--imex", "ars222", "--decomp", "mpi"], "--imex steps a lone single-slab run: not with --decomp / --block-contexts"),
    (["--imex", "euler", "--ensemble", "beta=1.0,1.5"], "--imex steps a lone single-slab run: not with --ensemble"),
    (["--imex", "ars443", "--observe", "2", "--probe", "1,1"], "--imex takes no recorder samples: not with --observe"),
    (["--imex", "ars443", "--adaptive"], "--imex steps at the run's fixed dt: not with --adaptive / --adaptive-rk43"),
    (["--imex", "ars443", "--adaptive-rk43"], "--imex steps at the run's fixed dt: not with --adaptive / --adaptive-rk43"),
]


def run_driver(args, ini, cwd):
    exe = os.path.join(ROOT, "crdmodel_amd", "bin", "crd_run")
    return subprocess.run([exe, "--model", "fhn", "--surface", "torus"] + args + [str(ini)], cwd=cwd, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,message", DRIVER_REFUSALS, ids=[" ".join(a) for a, _ in DRIVER_REFUSALS])
def test_driver_refuses_with_a_message(args, message, tmp_path):
    r = run_driver(args, INI, tmp_path)
    assert r.returncode == 1 and r.stdout == "" and r.stderr == "\nCRD_ERROR: " + message + "\n\n", (r.stdout, r.stderr)
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("line,args,needle", [("dt = 0", [], "--imex needs the run's fixed step"), ("dt = 0", ["--dt", "0"], "--imex needs the run's fixed step"),
                                               ("dt = 0.02\ngpus = 2", [], "[Solver] gpus = 2 (pass --gpus 1)"), ("dt = 0.02\nadaptive = 1", [], "[Solver] adaptive = 1 (pass --fixed)")],
                         ids=["dt-0", "--dt-0", "ini-gpus", "ini-adaptive"])
def test_driver_refuses_what_the_ini_asks(line, args, needle, tmp_path):
    """The fixed step must be given and positive -- dt = 0, the stable step of RK4, is meaningless for an IMEX run -- and what the
    command line refuses the ini may not ask for either; refused before any device is touched (this test runs without one)."""
    text = open(INI).read()
    assert "dt = 0.02\ngpus = 1" in text
    ini = tmp_path / "run.ini"
    ini.write_text(text.replace("dt = 0.02\ngpus = 1", line if "gpus" in line else line + "\ngpus = 1"))
    out = tmp_path / "out"
    out.mkdir()
    r = run_driver(["--imex", "ars222"] + args, ini, out)
    assert r.returncode == 1 and needle in r.stderr and r.stderr.startswith("\nCRD_ERROR: --imex"), r.stderr
    assert not os.listdir(out)
