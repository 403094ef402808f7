"""The IMEX stepper on the device (crd_step_imex / Slab.step_imex): additive Runge-Kutta steps with the diffusion part implicit.

1. Slab.step_imex equals, bit for bit, the step of include/crd.h composed in Python from Slab.rhs_part, Slab.lsolve and an exactly rounded
   fused multiply-add (tests/imex_reference.py: composed_step) -- each scheme, FHN and Goldbeter, torus and flat, fp64 and fp32, before,
   after and across tBoundary, on vectors that end in a ragged block (and, in fp32, in a lone point), and once beyond a grid-stride trip.
2. Against the dense restatement in float64 at rtol = 1e-12, inside imex_reference.steps_allowance.
3. At 30 x crd_stable_dt, where the oracle's RK4 overflows within a few steps, the device stays inside that allowance.
4. nsteps = 0, n + m steps, repeat runs, exhaustion, every refusal of the header, the stats against the composition's.
5. One crd_run --imex ars222 run whose final frame is Slab.step_imex's.

Worst observed / allowed on MI355X (printed with -s as "BOUND ..."): see DESIGN.md section 2.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
import imex_reference as ir
import jacobian_reference as jr

pytestmark = pytest.mark.gpu

K = crd._capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = list(jr.CONFIGS) + [("goldbeter-flat", "goldbeter", "flat", 0.4, {})]
CONFIG_IDS = [c[0] for c in CONFIGS]
RTOL = {"f64": 1e-8, "f32": 1e-5}  # the solve's default, and one above 100 u for fp32 (tests/test_gpu_krylov.py)
STATS = ("steps", "solves", "iterations", "failed_step", "max_iterations", "failed_stage", "t", "worst_residual", "max_abs_u")
THREADS, BLOCKS = 256, 2048  # kImexThreads, kImexBlocks of crd_imex.h


def stats_of(st):
    return tuple(getattr(st, f) for f in STATS)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    kind = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(kind), b.view(kind))


def units(nx, ny, precision):
    """16-byte units of a vector: one fp64 point, two fp32 points."""
    return nx * ny if precision == "f64" else (nx * ny + 1) // 2


def timed_case(config, nx, ny, precision, multiple):
    """(p, op, dt) with dt = multiple x crd_stable_dt and tBoundary = 10 dt."""
    p0, _ = jr.case(config, nx, ny, precision)
    dt = multiple * crd.stable_dt(p0)
    p, op = jr.case(config, nx, ny, precision, t_boundary=10 * dt)
    return p, op, dt


def check_stats(st, composed, nsteps, t0, dt, scheme):
    s = ir.tableau(scheme)[0]
    assert (st.steps, st.solves, st.failed_step, st.failed_stage) == (nsteps, nsteps * s, -1, -1), stats_of(st)
    assert st.solves == len(composed) and st.iterations == sum(c.iterations for c in composed)
    assert st.max_iterations == max(c.iterations for c in composed)
    assert st.worst_residual == max(c.res_norm / c.r_norm for c in composed if c.r_norm > 0)
    assert st.t == t0 + float(nsteps) * dt


# ---- 1. the composition, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config_index", range(len(CONFIGS)), ids=CONFIG_IDS)
def test_step_is_the_composition(gpu_device, config_index, precision):
    """61 x 9 = 549 points: two blocks and a ragged third in fp64, one ragged block in fp32 whose last thread takes a lone point; one
    multigrid level.  Two steps of each scheme from t = 0 (rows held throughout), from tBoundary (free: the comparison is strict) and
    from tBoundary - 0.6 dt, where stage 0 and, for ars222, stage 1 are held and every later stage is free.  dt = 2 x crd_stable_dt: on
    this coarse grid of the 80 x 20 domain that bound is the kinetics' own, which no IMEX step may exceed by much (at 20 x the dense
    restatement overflows within two steps)."""
    nx, ny = 61, 9
    assert units(nx, ny, precision) % THREADS != 0 and (precision == "f64" or (nx * ny) % 2 == 1)
    p, op, dt = timed_case(CONFIGS[config_index], nx, ny, precision, 2.0)
    tb = 10 * dt
    y0 = jr.start_state(p, 1)
    kw = dict(rtol=RTOL[precision])
    with crd.Slab(p) as slab:
        for scheme in ir.SCHEMES:
            for t0 in (0.0, tb, tb - 0.6 * dt):
                expected, composed = ir.composed_steps(slab, scheme, t0, dt, 2, y0, **kw)
                assert expected is not None and np.isfinite(expected).all() and np.abs(expected - y0).max() > 1e-4
                slab.upload(y0)
                st = slab.step_imex(t0, dt, 2, scheme, **kw)
                got = slab.download(dtype=slab.dtype)
                assert same_bits(got, expected), (scheme, t0, np.abs(got.astype(np.float64) - expected).max())
                check_stats(st, composed, 2, t0, dt, scheme)
                assert st.max_abs_u == np.abs(expected[..., 0]).max() == slab.max_abs()
        if not CONFIGS[config_index][4].get("just_diffusion"):
            # the rows held at stage 0 and free behind it received no kinetics at stage 0: across tBoundary differs from after it
            slab.upload(y0)
            slab.step_imex(tb, dt, 1, "euler", **kw)
            after = slab.download()
            slab.upload(y0)
            slab.step_imex(tb - 0.6 * dt, dt, 1, "euler", **kw)
            assert np.abs(slab.download()[0] - after[0]).max() > 0


def test_beyond_one_grid_stride_trip(gpu_device):
    """1030 x 510 = 525300 fp64 points: more than 2048 x 256 units, so 1012 threads take a second trip, and a ragged last block.  On this
    grid crd_stable_dt is the diffusion bound, and the step is 20 x that."""
    nx, ny = 1030, 510
    assert BLOCKS * THREADS < units(nx, ny, "f64") < 2 * BLOCKS * THREADS and units(nx, ny, "f64") % THREADS != 0
    p, op, dt = timed_case(CONFIGS[0], nx, ny, "f64", 20.0)
    y0 = jr.start_state(p, 1)
    with crd.Slab(p) as slab:
        expected, composed = ir.composed_steps(slab, "ars222", 9.5 * dt, dt, 1, y0)
        slab.upload(y0)
        st = slab.step_imex(9.5 * dt, dt, 1, "ars222")
        assert same_bits(slab.download(), expected)
        check_stats(st, composed, 1, 9.5 * dt, dt, "ars222")
        assert st.max_abs_u == np.abs(expected[..., 0]).max()


# ---- 2. and 3. against the dense restatement --------------------------------------------------------------------------------------
def small_case(config, t_boundary, multiple):
    """16 x 24 points of a 1 x 2 domain, D = 0.12: crd_stable_dt is the diffusion bound (0.0073 on the torus), and a dense matrix of the
    operator has 384 rows."""
    _, model, surface, beta, kw = config
    geometry = dict(L=2.0, W=1.0, D=0.12)
    p0 = crd.make_params(model, surface, 16, 2.0, 1.0, 0.12, beta, ny=24, **kw)
    dt = multiple * crd.stable_dt(p0)
    tb = t_boundary * dt
    p = crd.make_params(model, surface, 16, 2.0, 1.0, 0.12, beta, ny=24, t_boundary=tb, **kw)
    return p, jr.problem_of(model, surface, 16, 24, beta, t_boundary=tb, **geometry, **kw), dt


@functools.lru_cache(maxsize=None)
def dense_of(config_index, t_boundary, multiple):
    p, op, dt = small_case(CONFIGS[config_index], t_boundary, multiple)
    return p, ir.Dense(op), dt


def inside(case, slab, D, scheme, t0, dt, nsteps, y0, rtol):
    allowed, expected = ir.steps_allowance(D, scheme, t0, dt, nsteps, y0, rtol)
    assert np.isfinite(expected).all() and np.isfinite(allowed)  # on the reference, before the device is read
    slab.upload(y0)
    st = slab.step_imex(t0, dt, nsteps, scheme, rtol=rtol)
    err = float(np.linalg.norm(slab.download() - expected))
    print("BOUND imex %s: |device - dense| = %.3g, allowed %.3g (||y|| = %.3g, %d iterations)" % (case, err, allowed, np.linalg.norm(expected), st.iterations))
    assert err <= allowed, (case, err, allowed)
    return expected


@pytest.mark.parametrize("scheme", ir.SCHEMES)
@pytest.mark.parametrize("config_index", [0, 2, 4], ids=[CONFIG_IDS[k] for k in (0, 2, 4)])
def test_against_the_dense_restatement(gpu_device, config_index, scheme):
    """Three steps from tBoundary - 1.4 dt at rtol = 1e-12: held, across and free.  FHN at 5 x crd_stable_dt; Goldbeter at 2 x, inside
    the explicit limit of its kinetics (2 / 176, the block's norm on this state, against dt = 0.0072 and 0.0097)."""
    p, D, dt = dense_of(config_index, 10.0, 5.0 if config_index == 0 else 2.0)
    y0 = jr.start_state(p, 2)
    with crd.Slab(p) as slab:
        y = inside("%s %s" % (CONFIG_IDS[config_index], scheme), slab, D, scheme, 8.6 * dt, dt, 3, y0, 1e-12)
    assert np.abs(y - y0).max() > 1e-3


@pytest.mark.parametrize("scheme", ir.SCHEMES)
def test_a_step_size_rk4_cannot_take(gpu_device, scheme):
    """FHN on the torus at 30 x crd_stable_dt: the oracle's RK4 is not finite after 6 steps (after 2, in fact), the dense IMEX stays
    where the solution lives, and the device follows it inside the allowance.  The factor was chosen on the CPU, on the oracle alone."""
    p, D, dt = dense_of(0, 0.0, 30.0)
    y0 = jr.start_state(p, 1)
    with np.errstate(all="ignore"):
        assert not np.isfinite(ir.rk4_steps(D, 0.0, dt, 6, y0)).all()
    with crd.Slab(p) as slab:
        y = inside("30 x stable dt, %s" % scheme, slab, D, scheme, 0.0, dt, 6, y0, 1e-12)
    assert np.abs(y[..., 0]).max() < 3.0 and np.abs(y - y0).max() > 1e-2


# ---- 4. other checks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_zero_steps_splitting_and_repeats(gpu_device, precision):
    p, op, dt = timed_case(CONFIGS[0], 48, 40, precision, 1.0)
    y0 = jr.start_state(p, 1)
    kw = dict(rtol=RTOL[precision])
    with crd.Slab(p) as slab:
        slab.upload(y0)
        st = slab.step_imex(0.0, dt, 0, "ars443", **kw)
        assert same_bits(slab.download(dtype=slab.dtype), y0) and stats_of(st)[:7] == (0, 0, 0, -1, 0, -1, 0.0) and st.max_abs_u == np.abs(y0[..., 0]).max()
        whole = slab.step_imex(8.0 * dt, dt, 5, "ars443", **kw)
        y5 = slab.download(dtype=slab.dtype)
        slab.upload(y0)
        first = slab.step_imex(8.0 * dt, dt, 2, "ars443", **kw)
        second = slab.step_imex(8.0 * dt + 2.0 * dt, dt, 3, "ars443", **kw)
        assert 8.0 * dt + 2.0 * dt == 10.0 * dt and same_bits(slab.download(dtype=slab.dtype), y5)  # n then m steps are n + m steps
        assert (first.solves + second.solves, first.iterations + second.iterations) == (whole.solves, whole.iterations) and second.max_abs_u == whole.max_abs_u
        slab.upload(y0)
        again = slab.step_imex(8.0 * dt, dt, 5, "ars443", **kw)
        assert same_bits(slab.download(dtype=slab.dtype), y5) and stats_of(again) == stats_of(whole)  # the same bits from run to run
    with crd.Slab(p) as other:  # ... and from context to context, whatever ran before
        other.upload(y0)
        other.step_rk4(0.0, 0.5 * crd.stable_dt(p), 2)
        other.upload(y0)
        assert stats_of(other.step_imex(8.0 * dt, dt, 5, "ars443", **kw)) == stats_of(whole) and same_bits(other.download(dtype=other.dtype), y5)
        # fixed steps carry on from an IMEX state as from any other
        other.step_rk4(13.0 * dt, 0.5 * crd.stable_dt(p), 3)
        assert np.isfinite(other.download()).all()


def test_exhaustion(gpu_device):
    """max_iters = 1 at 20 x crd_stable_dt on the 16 x 24 grid of the small domain, where that is 20 x the diffusion bound: no solve
    converges.  From the start: nothing has been stepped.  With a first call that completes two steps: the state is theirs, and the
    failing call says which stage of which step stopped it."""
    p, _, dt = small_case(CONFIGS[0], 10.0, 20.0)
    y0 = jr.start_state(p, 1)
    with crd.Slab(p) as slab:
        slab.upload(y0)
        with pytest.raises(K.CrdError) as e:
            slab.step_imex(0.0, dt, 3, "ars222", max_iters=1)
        st = e.value.stats
        assert e.value.status == K.ESTATE and "did not converge" in str(e.value)
        assert (st.steps, st.failed_step, st.failed_stage, st.solves, st.iterations, st.t) == (0, 0, 1, 1, 1, 0.0), stats_of(st)
        assert same_bits(slab.download(), y0)
        slab.step_imex(0.0, dt, 2, "ars222")
        y2 = slab.download()
        with pytest.raises(K.CrdError) as e:
            slab.step_imex(2 * dt, dt, 3, "ars222", max_iters=1)
        assert e.value.status == K.ESTATE and (e.value.stats.steps, e.value.stats.failed_step, e.value.stats.failed_stage) == (0, 0, 1)
        assert same_bits(slab.download(), y2)


def test_a_state_that_is_not_finite(gpu_device):
    p, op, dt = timed_case(CONFIGS[1], 48, 40, "f64", 1.0)
    y0 = jr.start_state(p, 1)
    y0[7, 5, 0] = np.inf
    with crd.Slab(p) as slab:
        slab.upload(y0)
        with pytest.raises(K.CrdError) as e:
            slab.step_imex(0.0, dt, 2, "euler")
        st = e.value.stats
        assert e.value.status == K.ESTATE and st.steps == 0 and st.failed_step == 0 and st.failed_stage >= 1, stats_of(st)
        assert same_bits(slab.download(), y0)


def test_refusals(gpu_device):
    """Each refusal of the header, before any device work: the state is untouched and crd_imex_info reports no allocation made."""
    p, op, dt = timed_case(CONFIGS[0], 48, 40, "f64", 1.0)
    y0 = jr.start_state(p, 1)
    L = K.lib()

    def refused(call, status, word="imex"):
        with pytest.raises(K.CrdError) as e:
            call()
        assert e.value.status == status and word in str(e.value), e.value
        return str(e.value)

    with crd.Slab(p) as slab:
        slab.upload(y0)
        for kw in (dict(scheme=3), dict(scheme=-1), dict(part="full"), dict(part="reaction"), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("inf")), dict(dt=float("nan")),
                   dict(nsteps=-1), dict(t0=float("nan")), dict(restart=0), dict(restart=65), dict(max_iters=0), dict(rtol=-1.0), dict(atol=float("nan")),
                   dict(precondition=2), dict(pre=0, post=0), dict(omega=0.0)):
            kw = dict(kw)
            t0, h, n, scheme = kw.pop("t0", 0.0), kw.pop("dt", dt), kw.pop("nsteps", 1), kw.pop("scheme", "ars222")
            refused(lambda: slab.step_imex(t0, h, n, scheme, **kw), K.EINVAL)
        refused(lambda: slab.imex_info(scheme=5), K.EINVAL)
        refused(lambda: slab.imex_info(part="full"), K.EINVAL)
        assert L.crd_step_imex(None, 0.0, dt, 1, None, None) == K.EINVAL and L.crd_imex_defaults(None) == K.EINVAL
        assert same_bits(slab.download(), y0)
        # the workspace: y_n, R, s vectors k, s + 1 vectors FR, each padded to 256 bytes, 2048 partials; and the solve's own
        vec = -(-y0.nbytes // 256) * 256
        for scheme, s in (("euler", 1), ("ars222", 2), ("ars443", 4)):
            assert slab.imex_info(scheme) == (2 * s + 3) * vec + BLOCKS * 8 + slab.lsolve_info()
            assert slab.imex_info(scheme, restart=7) == (2 * s + 3) * vec + BLOCKS * 8 + slab.lsolve_info(restart=7)
        # opt == NULL: the defaults, ars222
        import ctypes as C

        st = K.ImexStats()
        slab._check(L.crd_step_imex(slab.handle, 0.0, dt, 1, None, C.byref(st)), "crd_step_imex")
        y1 = slab.download()
        slab.upload(y0)
        assert stats_of(slab.step_imex(0.0, dt, 1)) == stats_of(st) and st.solves == 2 and same_bits(slab.download(), y1)
        opt = K.ImexOptions()
        assert L.crd_imex_defaults(C.byref(opt)) == K.OK and (opt.scheme, opt.lsolve.part, opt.lsolve.restart, opt.lsolve.rtol) == (K.IMEX_ARS222, K.PART_DIFFUSION, 30, 1e-8)
        # a run recorder on the context
        with crd.Recorder(slab, stride=1, capacity=4):
            msg = refused(lambda: slab.step_imex(0.0, dt, 1), K.ESTATE)
            assert "recorder" in msg
    with crd.LocalGroup(p, 2) as group:
        s = group.slabs[1]
        assert "whole grid" in refused(lambda: s.step_imex(0.0, dt, 1), K.ESTATE)
        refused(lambda: s.imex_info(), K.ESTATE)
    with crd.LocalGroup(p, 4, blocks=(2, 2)) as blocks:
        assert "theta-blocks" in refused(lambda: blocks.slabs[0].step_imex(0.0, dt, 1), K.ESTATE)


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------------
def test_driver_runs_imex(gpu_device, tmp_path):
    """crd_run --imex ars222 --dt 0.25 on the 16 x 40 FHN torus of tests/golden/ini/small_run.ini (three outputs 0.4 apart: two steps of 0.2
    each, the first interval ending at tBoundary): the frames it writes -- the .npy side channel holds the state's own bits -- are the
    states Slab.step_imex reaches in the same calls, and the text files hold the same numbers."""
    ini = os.path.join(ROOT, "tests", "golden", "ini", "small_run.ini")
    cfg = crd.load_ini(ini, "fhn", "torus")
    exe = os.path.join(ROOT, "crdmodel_amd", "bin", "crd_run")
    r = subprocess.run([exe, "--model", "fhn", "--surface", "torus", "--imex", "ars222", "--dt", "0.25", "--binary", ini], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "integrator = IMEX ARS(2,2,2) on GPU (diffusion implicit), dt = 0.2 (2 steps per output)" in r.stdout
    assert "rate: 6 IMEX steps in" in r.stdout and "12 linear solves" in r.stdout
    d_tout = cfg.t_final / cfg.output_timestep
    steps = int(np.ceil(d_tout / 0.25 - 1e-12))
    u, v = (np.load(tmp_path / ("FHNmodel_torus_%s.000.npy" % name)) for name in "uv")
    assert u.shape == (cfg.output_timestep + 1, 40, 16) and steps == 2
    with crd.Slab(cfg.params) as slab:
        slab.upload(crd.initial_conditions(cfg))
        for k in range(cfg.output_timestep):
            slab.step_imex(k * d_tout, d_tout / steps, steps, "ars222")
            y = slab.download()
            assert same_bits(u[k + 1], y[..., 0]) and same_bits(v[k + 1], y[..., 1]), k
    rows = np.loadtxt(tmp_path / "FHNmodel_torus_u.000.txt", ndmin=2)
    assert np.array_equal(rows, u.reshape(u.shape[0], -1)) and np.abs(u[-1] - u[0]).max() > 0.1
