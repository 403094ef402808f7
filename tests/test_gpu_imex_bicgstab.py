"""IMEX steps with the BiCGStab solve (crd_step_imex with CRD_IMEX_SOLVER_BICGSTAB / _BICGSTAB_WARM; Slab.step_imex(solver=...)).

The step is, bit for bit, the composition of Slab.rhs_part, Slab.lsolve_bicgstab (with the chain of guesses for "bicgstab-warm") and
imex_reference.fma_exact (tests/bicgstab_reference.composed_steps), and its stats are the sums over the composition's solves; against the
dense restatement it is inside imex_reference's allowance; crd_imex_info counts the chosen solver's workspace alone; the default is
GMRES, unchanged; and the driver's --imex-solver reaches it.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bicgstab_reference as br
import crdmodel_amd as crd
import imex_reference as ir
import jacobian_reference as jr
from test_gpu_imex import CONFIGS, CONFIG_IDS, RTOL, dense_of, same_bits, stats_of, timed_case

pytestmark = pytest.mark.gpu

K = crd._capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVERS = ("bicgstab", "bicgstab-warm")


def check_stats(st, composed, nsteps, t0, dt, scheme):
    s = ir.tableau(scheme)[0]
    assert (st.steps, st.solves, st.failed_step, st.failed_stage) == (nsteps, nsteps * s, -1, -1), stats_of(st)
    assert st.solves == len(composed) and st.iterations == sum(c.iterations for c in composed)
    assert st.max_iterations == max(c.iterations for c in composed)
    assert st.worst_residual == max(c.true_res_norm / c.r_norm for c in composed if c.r_norm > 0)
    assert st.t == t0 + float(nsteps) * dt


# ---- 1. the composition, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config_index", range(len(CONFIGS)), ids=CONFIG_IDS)
def test_step_is_the_composition(gpu_device, config_index, precision):
    """61 x 9, two steps of each scheme before, from and across tBoundary, as tests/test_gpu_imex.py: test_step_is_the_composition."""
    nx, ny = 61, 9
    p, op, dt = timed_case(CONFIGS[config_index], nx, ny, precision, 2.0)
    tb = 10 * dt
    y0 = jr.start_state(p, 1)
    kw = dict(rtol=RTOL[precision])
    with crd.Slab(p) as slab:
        for solver in SOLVERS:
            for scheme in ir.SCHEMES:
                for t0 in (0.0, tb, tb - 0.6 * dt):
                    expected, composed = br.composed_steps(slab, scheme, t0, dt, 2, y0, warm=solver == "bicgstab-warm", **kw)
                    assert expected is not None and np.isfinite(expected).all() and np.abs(expected - y0).max() > 1e-4
                    slab.upload(y0)
                    st = slab.step_imex(t0, dt, 2, scheme, solver=solver, **kw)
                    got = slab.download(dtype=slab.dtype)
                    assert same_bits(got, expected), (solver, scheme, t0, np.abs(got.astype(np.float64) - expected).max())
                    check_stats(st, composed, 2, t0, dt, scheme)
                    assert st.max_abs_u == np.abs(expected[..., 0]).max()


def test_warm_starts_save_iterations_and_restart_ignored(gpu_device):
    """On a grid where the solve takes several iterations a warm chain takes fewer in total than cold solves; `restart` is not read."""
    p0 = crd.make_params("fhn", "torus", 64, 2.0, 1.0, 0.12, 1.25, ny=96)  # a 1 x 2 domain: crd_stable_dt is the diffusion bound, far below the kinetics'
    dt = 200.0 * crd.stable_dt(p0)
    p = crd.make_params("fhn", "torus", 64, 2.0, 1.0, 0.12, 1.25, ny=96, t_boundary=1.5 * dt)
    y0 = jr.start_state(p, 1)
    with crd.Slab(p) as slab:
        out = {}
        for solver in SOLVERS:
            slab.upload(y0)
            st = slab.step_imex(0.0, dt, 3, "ars443", solver=solver, restart=1)
            out[solver] = (slab.download(), st.iterations, st.worst_residual)
            assert st.steps == 3 and st.worst_residual <= 1e-7
    print("IMEX bicgstab 64x96 ars443 200x: %d iterations cold, %d warm" % (out["bicgstab"][1], out["bicgstab-warm"][1]))
    assert out["bicgstab-warm"][1] < out["bicgstab"][1]
    assert np.abs(out["bicgstab"][0] - out["bicgstab-warm"][0]).max() <= 1e-5 * np.abs(out["bicgstab"][0]).max()


# ---- 2. against the dense restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("scheme", ir.SCHEMES)
def test_against_the_dense_restatement(gpu_device, scheme, solver):
    """Three steps from tBoundary - 1.4 dt on the FHN torus of tests/test_gpu_imex.py's dense cases, the solves at rtol = 1e-10.  The
    allowance takes a bound on every solve's residual: the device's own worst_residual, the largest true_res_norm / r_norm of a solve
    (the recurrence's residual is what met rtol; the true one may sit a rounding above it), which itself may not exceed 2 rtol.  That
    the allowance holds for a step solved this way is shown without a device in tests/test_bicgstab_host.py:
    test_imex_allowance_holds_for_the_restatement, on this very case."""
    p, D, dt = dense_of(0, 10.0, 5.0)
    y0 = jr.start_state(p, 2)
    rtol = 1e-10
    expected = ir.dense_steps(D, scheme, 8.6 * dt, dt, 3, y0)
    assert np.isfinite(expected).all()  # on the reference, before the device is read
    with crd.Slab(p) as slab:
        slab.upload(y0)
        st = slab.step_imex(8.6 * dt, dt, 3, scheme, solver=solver, rtol=rtol)
        err = float(np.linalg.norm(slab.download() - expected))
    assert 0.0 < st.worst_residual <= 2 * rtol, st.worst_residual
    allowed = ir.steps_allowance(D, scheme, 8.6 * dt, dt, 3, y0, st.worst_residual)[0]
    print("BOUND imex %s %s: |device - dense| = %.3g, allowed %.3g, worst true residual %.3g (%d iterations)" % (solver, scheme, err, allowed, st.worst_residual, st.iterations))
    assert np.isfinite(allowed) and err <= allowed, (solver, scheme, err, allowed)


# ---- 3. workspace, defaults, refusals ---------------------------------------------------------------------------------------------
def test_info_defaults_and_refusals(gpu_device):
    p, op, dt = timed_case(CONFIGS[0], 61, 9, "f64", 2.0)
    y0 = jr.start_state(p, 1)
    vec = -(-y0.nbytes // 256) * 256
    with crd.Slab(p) as slab:
        for scheme, s in (("euler", 1), ("ars222", 2), ("ars443", 4)):
            own = (2 * s + 3) * vec + 2048 * 8
            assert slab.imex_info(scheme) == own + slab.lsolve_info()
            for solver in SOLVERS:
                assert slab.imex_info(scheme, solver=solver) == own + slab.lsolve_bicgstab_info() < slab.imex_info(scheme)
        # the default is GMRES, and solver="gmres" is the call without it
        slab.upload(y0)
        a = slab.step_imex(0.0, dt, 2)
        ya = slab.download()
        slab.upload(y0)
        b = slab.step_imex(0.0, dt, 2, solver="gmres")
        assert same_bits(slab.download(), ya) and stats_of(a) == stats_of(b)
        for solver in (3, -1):
            with pytest.raises(K.CrdError) as e:
                slab.step_imex(0.0, dt, 1, solver=solver)
            assert e.value.status == K.EINVAL and "solver must be" in str(e.value)
            with pytest.raises(K.CrdError):
                slab.imex_info(solver=solver)
        with pytest.raises(K.CrdError) as e:
            slab.step_imex(0.0, dt, 1, solver="bicgstab", max_iters=0)
        assert e.value.status == K.EINVAL and "bicgstab: max_iters" in str(e.value)
        # a solve that runs out of iterations stops the call as with GMRES
        slab.upload(y0)
        with pytest.raises(K.CrdError) as e:
            slab.step_imex(0.0, 50 * dt, 2, "ars222", solver="bicgstab", max_iters=1, rtol=1e-14)
        assert e.value.status == K.ESTATE and "did not converge" in str(e.value) and (e.value.stats.failed_step, e.value.stats.failed_stage) == (0, 1)
        assert same_bits(slab.download(), y0)


# ---- 4. the driver ----------------------------------------------------------------------------------------------------------------
def test_driver_runs_imex_with_bicgstab(gpu_device, tmp_path):
    """crd_run --imex ars222 --imex-solver bicgstab on tests/golden/ini/small_run.ini, as tests/test_gpu_imex.py: test_driver_runs_imex:
    the frames are the states Slab.step_imex(solver="bicgstab") reaches in the same calls."""
    ini = os.path.join(ROOT, "tests", "golden", "ini", "small_run.ini")
    cfg = crd.load_ini(ini, "fhn", "torus")
    exe = os.path.join(ROOT, "crdmodel_amd", "bin", "crd_run")
    r = subprocess.run([exe, "--model", "fhn", "--surface", "torus", "--imex", "ars222", "--imex-solver", "bicgstab", "--dt", "0.25", "--binary", ini], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "rate: 6 IMEX steps in" in r.stdout and "12 linear solves" in r.stdout and "BiCGStab iterations" in r.stdout
    d_tout = cfg.t_final / cfg.output_timestep
    u, v = (np.load(tmp_path / ("FHNmodel_torus_%s.000.npy" % name)) for name in "uv")
    with crd.Slab(cfg.params) as slab:
        slab.upload(crd.initial_conditions(cfg))
        for k in range(cfg.output_timestep):
            slab.step_imex(k * d_tout, d_tout / 2, 2, "ars222", solver="bicgstab")
            y = slab.download()
            assert same_bits(u[k + 1], y[..., 0]) and same_bits(v[k + 1], y[..., 1]), k
    assert np.abs(u[-1] - u[0]).max() > 0.1
    # --imex-solver without --imex, and a solver it does not know, are usage errors
    for args in (["--imex-solver", "bicgstab"], ["--imex", "ars222", "--imex-solver", "cg"]):
        bad = subprocess.run([exe, "--model", "fhn", "--surface", "torus"] + args + ["--dt", "0.25", ini], cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert bad.returncode != 0 and "--imex-solver" in bad.stderr
