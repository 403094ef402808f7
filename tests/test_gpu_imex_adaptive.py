"""Error-controlled IMEX integration on the device (crd_integrate_imex / Slab.integrate_imex, crd_imex_estimate_probe).

1. The estimating last close alone, through the probe: out and e bit for bit, the sum of the weighted squares inside gamma_K sum q of
   the long-double sum of the bit-exact q, one planted element carrying the sum at every seam of the reduction, max |var0| exactly.
2. One accepted attempt: the state is crd_step_imex's of the same step bit for bit, err_last the norm of the composed step's stages.
3. One rejected attempt: CRD_ESTATE with max_steps = 1, the state untouched, h_next the restated controller's.
4. A run with rejections: the recorded attempts replayed by crd_step_imex and by the restated controller; across tBoundary; a second call.
5. crd_run --imex ars443 --imex-adaptive against Slab.integrate_imex, interval by interval.
6. Every refusal of the header.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import bicgstab_reference as br
import crdmodel_amd as crd
import imex_adaptive_reference as ar
import imex_reference as ir
import jacobian_reference as jr
from test_gpu_imex import CONFIGS, RTOL, same_bits, timed_case, units

pytestmark = pytest.mark.gpu

K = crd._capi
ROOT = ar.ROOT
SOLVERS = ("gmres", "bicgstab", "bicgstab-warm")
BIAS = 1.5
# FHN torus and flat, Goldbeter, diffusion only (tests/jacobian_reference.py: CONFIGS)
ATTEMPT_CONFIGS = [CONFIGS[0], CONFIGS[1], CONFIGS[2], CONFIGS[3]]
SHAPES = [(61, 9), (1030, 510)]  # a ragged last block (in fp32 a lone last point); a second grid-stride trip


def shape_is_what_it_is_for(nx, ny, precision):
    u = units(nx, ny, precision)
    if (nx, ny) == (61, 9):
        return u % 256 != 0 and (precision == "f64" or (nx * ny) % 2 == 1)
    return (u > 2048 * 256) == (precision == "f64") and u % 256 != 0


# ---- 1. the close alone -----------------------------------------------------------------------------------------------------------
def probe_vectors(nx, ny, precision, seed):
    R_ = br.DTYPES[precision]
    rng = np.random.default_rng(seed)
    vec = lambda scale: (scale * rng.standard_normal((ny, nx, 2))).astype(R_)
    return vec(1.0), vec(0.5), vec(1.0), [vec(0.7) for _ in range(7)]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_close_alone(gpu_device, nx, ny, precision):
    assert shape_is_what_it_is_for(nx, ny, precision)
    p, _ = jr.case(CONFIGS[1], nx, ny, precision)
    R, k, yn, stored = probe_vectors(nx, ny, precision, 11)
    hg, dt, rtol, atol = 0.11, 0.22, 1e-3, 1e-5
    want_out, want_e, q = ar.close_reference(R, k, yn, stored, hg, dt, rtol, atol, precision)
    ref, bound = ar.sum_bound(q, precision)
    with crd.Slab(p) as slab:
        out, e, total, biggest = slab.imex_estimate_probe(R, k, yn, stored, hg, dt, rtol, atol)
        assert same_bits(out, want_out), np.abs(out.astype(np.float64) - want_out).max()
        assert same_bits(e, want_e), np.abs(e.astype(np.float64) - want_e).max()
        print("SUM %dx%d %s: |device - long double| = %.3g, allowed %.3g (K = %d)" % (nx, ny, precision, abs(float(total - ref)), bound, br.sum_roundings(q.size, precision)))
        assert abs(float(np.longdouble(total) - ref)) <= bound, (total, float(ref), bound)
        assert biggest == np.max(np.abs(want_out[..., 0]).astype(np.float64))
        # the same bits again
        again = slab.imex_estimate_probe(R, k, yn, stored, hg, dt, rtol, atol)
        assert again[2] == total and again[3] == biggest and same_bits(again[1], e)
        # one planted element carries the sum: everything but FR_0 at one real is zero, so every other q is +0 and every addition exact
        zero = np.zeros_like(R)
        positions = br.plant_positions(q.size, precision)
        assert {x % 2 for x in positions} == {0, 1} and (len(positions) == 8) == (units(nx, ny, precision) > 2048 * 256)
        for pos in positions:
            fr0 = zero.copy()
            fr0.reshape(-1)[pos] = 0.75
            _, _, q1 = ar.close_reference(zero, zero, yn, [fr0] + [zero] * 6, hg, dt, rtol, atol, precision)
            assert np.count_nonzero(q1) == 1 and q1.reshape(-1)[pos] > 0
            _, e1, total1, _ = slab.imex_estimate_probe(zero, zero, yn, [fr0] + [zero] * 6, hg, dt, rtol, atol)
            assert total1 == q1.reshape(-1)[pos], (pos, total1, q1.reshape(-1)[pos])
            assert np.count_nonzero(e1) == 1
        # a NaN in var0 of the new state propagates into max |u|, wherever it lies; one in var1 alone does not reach it
        for pos in (0, q.size - 2):
            bad = R.copy()
            bad.reshape(-1)[pos] = np.nan
            assert math.isnan(slab.imex_estimate_probe(bad, k, yn, stored, hg, dt, rtol, atol)[3])
        bad = R.copy()
        bad.reshape(-1)[1] = np.nan
        assert slab.imex_estimate_probe(bad, k, yn, stored, hg, dt, rtol, atol)[3] == np.max(np.abs(want_out[..., 0]).astype(np.float64))


# ---- the attempt composed from the public pieces ----------------------------------------------------------------------------------
def composed_attempt(slab, t, h, y, solver="gmres", **solve_options):
    """(Y_s, R_s, k_s, stored, iterations) of one ARS(4,4,3) step from (t, y) as imex_reference.composed_step / bicgstab_reference.
    composed_steps compose it, with the vectors the estimate reads; `stored` in imex_adaptive_reference.STORED's order."""
    R_ = slab.dtype
    fma = ir.fma_exact(R_)
    s, c, AE, AI, g = ir.tableau("ars443")
    hg = R_(h * g)
    y = np.ascontiguousarray(y, dtype=R_)
    FR, k, iterations, last_k = [slab.rhs_part(t, y, "reaction")], [None], 0, None
    R = fma(R_(h * AE[1][0]), FR[0], y)
    for i in range(1, s + 1):
        ti = t + c[i] * h
        r = slab.rhs_part(ti, R, "diffusion")
        if solver == "gmres":
            ki, st = slab.lsolve(ti, float(hg), r, **solve_options)
        else:
            ki, st = slab.lsolve_bicgstab(ti, float(hg), r, guess=last_k if solver == "bicgstab-warm" else None, **solve_options)
        assert st.converged
        iterations += st.iterations
        k.append(ki)
        last_k = ki
        Y = fma(hg, ki, R)
        if i == s:
            stored = [FR[j] if which == "E" else k[j] for j, which in ar.STORED]
            return np.ascontiguousarray(Y, dtype=R_), R, ki, stored, iterations
        FR.append(slab.rhs_part(ti, Y, "reaction"))
        R = y
        for j, which, coef in ir.row_terms("ars443", i + 1, h, R_):
            R = fma(coef, FR[j] if which == "E" else k[j], R)


def reference_sum(slab, precision, t, h, y, rtol, atol, solver, solve_options={}):
    """(Y_s, long-double sum of the bit-exact q, its allowance, iterations) of the composed attempt."""
    Y, R, ks, stored, iterations = composed_attempt(slab, t, h, y, solver, **solve_options)  # (the solve's own rtol, not the integrator's)
    hg = float(slab.dtype(h * ir.tableau("ars443")[4]))
    out, _, q = ar.close_reference(R, ks, y, stored, hg, h, rtol, atol, precision)
    assert same_bits(out, Y)
    ref, bound = ar.sum_bound(q, precision)
    return Y, ref, bound, iterations


def scaled_tolerances(slab, precision, t, h, y, solver, target, solve_options={}):
    """(rtol, atol) = s (1e-3, 1e-5) with s such that bias x the reference norm is `target`: the norm is inversely proportional to s."""
    _, ref, _, _ = reference_sum(slab, precision, t, h, y, 1e-3, 1e-5, solver, solve_options)
    norm = math.sqrt(float(ref) / y.size)
    assert norm > 0
    s = BIAS * norm / target
    return 1e-3 * s, 1e-5 * s


def check_err_last(err_last, ref, bound, n):
    """bias x sqrt(sum / n) with the device's sum inside ref +- bound; the square root, the quotient and the product add three roundings."""
    lo, hi = (BIAS * math.sqrt(max(float(ref) - bound, 0.0) / n), BIAS * math.sqrt((float(ref) + bound) / n))
    assert lo * (1 - 4 * 2.0 ** -52) <= err_last <= hi * (1 + 4 * 2.0 ** -52), (lo, err_last, hi)


# ---- 2. one accepted attempt ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config_index", range(len(ATTEMPT_CONFIGS)), ids=[c[0] for c in ATTEMPT_CONFIGS])
def test_one_accepted_attempt(gpu_device, config_index, precision):
    """61 x 9, one attempt of 2 x crd_stable_dt before, from and across tBoundary with each solver: tout - t0 is h0 exactly, the
    tolerances scaled on the reference so that bias x norm is 0.1."""
    nx, ny = 61, 9
    p, op, dt = timed_case(ATTEMPT_CONFIGS[config_index], nx, ny, precision, 2.0)
    tb = 10 * dt
    y0 = jr.start_state(p, 1)
    kw = dict(rtol=RTOL[precision])
    with crd.Slab(p) as slab, crd.Slab(p) as second:
        for solver in SOLVERS:
            for t0 in (0.0, tb, tb - 0.6 * dt):
                tout = t0 + dt
                h = tout - t0
                rtol, atol = scaled_tolerances(slab, precision, t0, h, y0, solver, 0.1, kw)
                Y, ref, bound, iterations = reference_sum(slab, precision, t0, h, y0, rtol, atol, solver, kw)
                assert 0.09 < BIAS * math.sqrt(float(ref) / y0.size) < 0.11
                slab.upload(y0)
                st, hist = slab.integrate_imex(t0, tout, rtol=rtol, atol=atol, h0=h, solver=solver, history=True, lsolve_rtol=kw["rtol"])
                got = slab.download(dtype=slab.dtype)
                second.upload(y0)
                fixed = second.step_imex(t0, h, 1, "ars443", solver=solver, **kw)
                assert same_bits(got, second.download(dtype=second.dtype)) and same_bits(got, Y), (solver, t0)
                assert (st.accepted, st.rejected, st.attempts, st.recorded, st.t) == (1, 0, 1, 1, tout)
                assert (st.h_first, st.h_last, st.h_min, st.h_max) == (h, h, h, h) and st.h_next >= h
                check_err_last(st.err_last, ref, bound, y0.size)
                assert (st.imex.steps, st.imex.solves, st.imex.iterations, st.imex.failed_step) == (1, 4, fixed.iterations, -1) and fixed.iterations == iterations
                assert st.imex.max_abs_u == fixed.max_abs_u == np.abs(Y[..., 0]).max() and st.imex.worst_residual == fixed.worst_residual
                assert (hist[0].t, hist[0].h, hist[0].err, hist[0].accepted, hist[0].iterations) == (t0, h, st.err_last, 1, iterations)


def test_one_accepted_attempt_beyond_one_trip(gpu_device):
    """1030 x 510 fp64: a second grid-stride trip and a ragged last block, 20 x crd_stable_dt across tBoundary, BiCGStab."""
    nx, ny = 1030, 510
    p, op, dt = timed_case(CONFIGS[0], nx, ny, "f64", 20.0)
    y0 = jr.start_state(p, 1)
    t0 = 9.5 * dt
    tout = t0 + dt
    h = tout - t0
    with crd.Slab(p) as slab:
        rtol, atol = scaled_tolerances(slab, "f64", t0, h, y0, "bicgstab", 0.1)
        Y, ref, bound, iterations = reference_sum(slab, "f64", t0, h, y0, rtol, atol, "bicgstab")
        slab.upload(y0)
        st = slab.integrate_imex(t0, tout, rtol=rtol, atol=atol, h0=h, solver="bicgstab")
        assert same_bits(slab.download(), Y) and (st.accepted, st.rejected, st.t, st.imex.iterations) == (1, 0, tout, iterations)
        check_err_last(st.err_last, ref, bound, y0.size)
        slab.upload(y0)
        slab.step_imex(t0, h, 1, "ars443", solver="bicgstab")
        assert same_bits(slab.download(), Y)


# ---- 3. one rejected attempt ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_one_rejected_attempt(gpu_device, precision):
    nx, ny = 61, 9
    p, op, dt = timed_case(CONFIGS[0], nx, ny, precision, 2.0)
    y0 = jr.start_state(p, 1)
    kw = dict(rtol=RTOL[precision])
    t0, tout = 9.4 * dt, 30 * dt
    with crd.Slab(p) as slab:
        rtol, atol = scaled_tolerances(slab, precision, t0, dt, y0, "gmres", BIAS * 3.0, kw)
        _, ref, bound, iterations = reference_sum(slab, precision, t0, dt, y0, rtol, atol, "gmres", kw)
        assert math.sqrt(float(ref) / y0.size) > 1.5  # the reference norm, before the device is asked
        slab.upload(y0)
        with pytest.raises(K.CrdError) as e:
            slab.integrate_imex(t0, tout, rtol=rtol, atol=atol, h0=dt, max_steps=1, history=True, lsolve_rtol=kw["rtol"])
        st = e.value.stats
        assert e.value.status == K.ESTATE and "max_steps" in str(e.value)
        assert (st.accepted, st.rejected, st.attempts, st.recorded, st.t, st.imex.steps) == (0, 1, 1, 1, t0, 0)
        assert same_bits(slab.download(dtype=slab.dtype), np.ascontiguousarray(y0, dtype=slab.dtype))
        check_err_last(st.err_last, ref, bound, y0.size)
        assert (e.value.history[0].accepted, e.value.history[0].h, e.value.history[0].iterations) == (0, dt, iterations)
        P = ar.Control(t0, tout, dt, max_steps=1)
        assert P.next() == (t0, dt) and P.verdict(st.err_last / BIAS) == 0
        assert ar.ulps(P.h_next(), st.h_next) <= 4 and st.h_next < dt, (P.h_next(), st.h_next)
        # the context steps on as if nothing had been attempted
        st2 = slab.integrate_imex(t0, t0 + st.h_next, rtol=rtol, atol=atol, h0=st.h_next, lsolve_rtol=kw["rtol"])
        assert st2.attempts >= 1 and st2.t == t0 + st.h_next


# ---- 4. a run ---------------------------------------------------------------------------------------------------------------------
def run_case(t_boundary):
    p = crd.make_params("fhn", "torus", 12, 2.0, 1.0, 0.12, 1.25, ny=16, t_boundary=t_boundary)
    op = jr.problem_of("fhn", "torus", 12, 16, 1.25, L=2.0, W=1.0, D=0.12, t_boundary=t_boundary)
    return p, op, ir.smooth_state(op)


@pytest.mark.parametrize("t_boundary", [0.0, 0.7], ids=["free", "across-tBoundary"])
def test_a_run_with_rejections(gpu_device, t_boundary):
    """FHN 12 x 16 on the 1 x 2 torus of tests/test_imex_host.py: smooth_problem, rtol = 1e-4, T = 2 from h0 = 1: the dense restatement
    rejects the first attempt at least (asserted on it first).  The device's recorded attempts are then replayed twice."""
    p, op, y0 = run_case(t_boundary)
    rtol, atol, h0, T = 1e-4, 1e-6, 1.0, 2.0
    ref_state, ref_control, ref_record = ar.integrate_dense(ir.Dense(op), 0.0, T, y0, rtol, atol, h0)
    assert ref_control.rejected >= 1 and ref_control.t == T
    with crd.Slab(p) as slab, crd.Slab(p) as second:
        slab.upload(y0)
        st, hist = slab.integrate_imex(0.0, T, rtol=rtol, atol=atol, h0=h0, history=True)
        got = slab.download()
        assert st.t == T and st.rejected >= 1 and st.attempts == st.accepted + st.rejected == st.recorded == len(hist)
        print("RUN tBoundary %.1f: device %d + %d rejected, reference %d + %d" % (t_boundary, st.accepted, st.rejected, ref_control.accepted, ref_control.rejected))
        assert abs(st.accepted - ref_control.accepted) <= 2
        # the accepted attempts, replayed by the fixed stepper
        second.upload(y0)
        for a in hist:
            if a.accepted:
                second.step_imex(a.t, a.h, 1, "ars443")
        assert same_bits(second.download(), got)
        assert hist[-1].accepted and hist[-1].t + hist[-1].h == pytest.approx(T, abs=1e-12)
        # the recorded norms, replayed through the restated controller
        P = ar.Control(0.0, T, h0)
        for a in hist:
            t, h = P.next()
            assert ar.ulps(t, a.t) <= 4 and ar.ulps(h, a.h) <= 4, (t, a.t, h, a.h)
            assert P.verdict(a.err / BIAS) == a.accepted
        assert P.done() and P.t == T and ar.ulps(P.h_next(), st.h_next) <= 4
        assert (st.h_first, st.h_last) == (hist[0].h, hist[-1].h) and st.h_min == min(a.h for a in hist if a.accepted) and st.h_max == max(a.h for a in hist if a.accepted)
        assert st.imex.iterations == sum(a.iterations for a in hist) and st.imex.solves == 4 * len(hist)
        # against the dense restatement's own run: two runs at this tolerance, each within 10 rtol of the solution
        # (tests/test_imex_adaptive_host.py: test_runs_follow_the_tolerance), are within 20 rtol of each other
        assert float(np.linalg.norm(got - ref_state)) <= 20 * rtol
        # a second call from h_next
        st2 = slab.integrate_imex(T, T + 0.5, rtol=rtol, atol=atol, h0=st.h_next)
        assert st2.t == T + 0.5 and st2.h_first == min(st.h_next, 0.5) and st2.accepted >= 1


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------------
def test_driver_runs_imex_adaptive(gpu_device, tmp_path):
    ini = os.path.join(ROOT, "tests", "golden", "ini", "small_run.ini")
    cfg = crd.load_ini(ini, "fhn", "torus")
    exe = os.path.join(ROOT, "crdmodel_amd", "bin", "crd_run")
    r = subprocess.run([exe, "--model", "fhn", "--surface", "torus", "--imex", "ars443", "--imex-adaptive", "--imex-solver", "bicgstab", "--dt", "0.25", "--binary", ini],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "embedded order 2" in r.stdout and "steps = " in r.stdout and "BiCGStab iterations" in r.stdout
    d_tout = cfg.t_final / cfg.output_timestep
    u, v = (np.load(tmp_path / ("FHNmodel_torus_%s.000.npy" % name)) for name in "uv")
    accepted = rejected = 0
    with crd.Slab(cfg.params) as slab:
        slab.upload(crd.initial_conditions(cfg))
        h = 0.25
        for k in range(cfg.output_timestep):
            tout = cfg.t_final if k + 1 == cfg.output_timestep else (k + 1) * d_tout
            st = slab.integrate_imex(k * d_tout, tout, rtol=cfg.rtol, atol=cfg.atol, h0=h, solver="bicgstab")
            h = st.h_next
            accepted, rejected = accepted + st.accepted, rejected + st.rejected
            y = slab.download()
            assert same_bits(u[k + 1], y[..., 0]) and same_bits(v[k + 1], y[..., 1]), k
    assert "steps = %d (+%d rejected)" % (accepted, rejected) in r.stdout
    assert np.abs(u[-1] - u[0]).max() > 0.1
    # without a fixed step: h0 = 0 starts from crd_stable_dt
    auto = tmp_path / "auto"
    auto.mkdir()
    r0 = subprocess.run([exe, "--model", "fhn", "--surface", "torus", "--imex", "ars443", "--imex-adaptive", "--dt", "0", "--binary", ini], cwd=auto, capture_output=True,
                        text=True, timeout=300)
    assert r0.returncode == 0 and "steps = " in r0.stdout, r0.stderr


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_interval(gpu_device):
    p, op, dt = timed_case(CONFIGS[0], 61, 9, "f64", 2.0)
    y0 = jr.start_state(p, 1)
    with crd.Slab(p) as slab:
        slab.upload(y0)
        ok = dict(rtol=1e-4, atol=1e-6, h0=dt)
        bad = [dict(scheme="euler"), dict(scheme="ars222"), dict(scheme=7), dict(solver=3), dict(part="full"), dict(max_iters=0), dict(rtol=-1e-4), dict(atol=-1.0),
               dict(rtol=0.0, atol=0.0), dict(rtol=math.nan), dict(atol=math.inf), dict(h0=-dt), dict(h0=math.inf), dict(h_max=math.nan), dict(safety=0.0), dict(bias=0.0),
               dict(growth=0.5), dict(shrink=0.0), dict(shrink=1.0), dict(max_steps=0)]
        for change in bad:
            with pytest.raises(K.CrdError) as e:
                slab.integrate_imex(0.0, 4 * dt, **dict(ok, **change))
            assert e.value.status == K.EINVAL and "imex" in str(e.value), (change, str(e.value))
        for t0, tout in ((1.0, 0.5), (math.nan, 1.0), (0.0, math.inf)):
            with pytest.raises(K.CrdError) as e:
                slab.integrate_imex(t0, tout, **ok)
            assert e.value.status == K.EINVAL
        with pytest.raises(K.CrdError) as e:
            slab.integrate_imex(0.0, 4 * dt, scheme="ars222", **ok)
        assert "embedded" in str(e.value)
        # the history's arguments, through the ABI itself
        opt, st = K.ImexAdaptiveOptions(), K.ImexAdaptiveStats()
        assert K.lib().crd_imex_adaptive_defaults(C.byref(opt)) == K.OK
        assert K.lib().crd_integrate_imex(slab._h, 0.0, dt, C.byref(opt), C.byref(st), None, 3) == K.EINVAL
        assert K.lib().crd_integrate_imex(slab._h, 0.0, dt, C.byref(opt), C.byref(st), None, -1) == K.EINVAL
        for args in ((None, y0.ctypes.data, y0.ctypes.data, (C.c_double * 2)()), ((C.c_double * 4)(), None, y0.ctypes.data, (C.c_double * 2)())):
            assert K.lib().crd_imex_estimate_probe(slab._h, *args) == K.EINVAL
        # nothing was touched; an empty interval takes no step and reports the state's max |u|; opt == NULL runs the defaults
        assert same_bits(slab.download(), y0)
        st = slab.integrate_imex(0.3, 0.3, **ok)
        assert (st.accepted, st.attempts, st.t, st.h_next, st.imex.max_abs_u) == (0, 0, 0.3, dt, np.abs(y0[..., 0]).max()) and same_bits(slab.download(), y0)
        st = K.ImexAdaptiveStats()
        assert K.lib().crd_integrate_imex(slab._h, 0.0, dt, None, C.byref(st), None, 0) == K.OK and st.t == dt and st.h_first == min(crd.stable_dt(p), dt)
        # the workspace is the fixed stepper's
        assert slab.imex_info("ars443") == 11 * (-(-y0.nbytes // 256) * 256) + 2048 * 8 + slab.lsolve_info()
    # a recorder on the context, several slabs: crd_step_imex's own refusals reach this entry point (tests/test_gpu_imex.py holds them there)
