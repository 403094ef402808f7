"""The linear solve on the device (crd_lsolve_* / Slab.lsolve): restarted, right-preconditioned GMRES for (I - gamma J_part(t, y)) z = r.

The multi-dot alone is held entry by entry to the bound counted from its summation tree (tests/krylov_reference.py); the solve to the
iteration count of the long-double reference (fp32: float64 on the widened vectors, +- 1) at a tolerance placed between two of the
reference's residuals, and its residual under the reference operator to the allowance of
test_gpu_multigrid.test_gmres_with_the_device_preconditioner; restart, exhaustion, one-level grids of odd width, the full Jacobian, the
solve without the cycle and a breakdown each take their own path; the identities the header promises are held bit for bit; and what the
entry points refuse, they refuse with a message.

Worst observed / allowed on MI355X (printed with -s as "BOUND ..."): see DESIGN.md section 2.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import crdmodel_amd as crd
import jacobian_reference as jr
import krylov_reference as kr
import multigrid_reference as mg
from oracle import error_bounds as eb

pytestmark = pytest.mark.gpu

CONFIG_IDS = [c[0] for c in jr.CONFIGS]
T_ON, T_AT, T_OFF = jr.TIMES  # rows held; at tBoundary (strict <: free); free
K = crd._capi
STATS = ("converged", "iterations", "restarts", "matvecs", "psolves", "breakdown", "r_norm", "res_norm")


def right_hand_side(p, seed=5):
    g = crd.grid_of(p)
    r = np.random.default_rng(seed).standard_normal((g.ny, g.nx, 2))
    return r.astype(np.float32) if p.precision == K.PRECISION_F32 else r


def stats_of(st):
    return tuple(getattr(st, f) for f in STATS)


def inside(case, op, t, gamma, y, z, r, precision, part, rtol, st=None, atol=0.0):
    """The residual of z under the reference operator, and the solver's own, against the allowance; returns observed / allowed."""
    res, allowed = kr.residual_allowance(op, t, gamma, y, z, r, precision, part, rtol, atol)
    print("BOUND lsolve %s: residual %.3g, allowed %.3g%s" % (case, res, allowed, "" if st is None else ", solver's own %.3g after %d iterations" % (st.res_norm, st.iterations)))
    assert np.isfinite(np.asarray(z, dtype=np.float64)).all(), case
    assert res <= allowed, (case, res, allowed)
    if st is not None:
        assert st.res_norm <= allowed, (case, st.res_norm, allowed)
    return res / allowed


# ---- 1. the reductions alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny", [(19, 27), (264, 250)], ids=["19x27", "264x250"])
def test_multi_dot_within_the_bound(gpu_device, nx, ny, precision):
    """crd_krylov_probe_dots on planted vectors: one element carries each sum, at index 0, 63 | 64, 255 | 256, the last index of the first
    grid-stride trip and the first of the second (264 x 250: n = 132000 > 512 x 256), and n - 1 -- var0 and var1 -- for 1, 8, 9 and 31
    basis vectors.  19 x 27: n = 1026 = 4 x 256 + 2, a tail of two in the fifth block."""
    p, _ = jr.case(jr.CONFIGS[0], nx, ny, precision)
    R, n, L, worst = kr.DTYPES[precision], 2 * nx * ny, K.lib(), 0.0
    positions = kr.plant_positions(n)
    assert (n > kr.BLOCKS * kr.THREADS) == (nx == 264) and n % kr.THREADS != 0
    with crd.Slab(p) as slab:
        for count in (1, kr.GROUP, kr.GROUP + 1, 31):
            for shift in range(len(positions) if count == 1 else 1):
                V, w, where = kr.planted(n, count, positions[shift:] + positions[:shift], R)
                ref, bound, sizes = kr.dots_bound(V, w)
                for i, q in enumerate(where):
                    assert abs(float(V[i, q]) * float(w[q])) >= 0.5 * sizes[i]  # on the reference, before the device is read
                out = np.full(count, np.nan)
                slab._check(L.crd_krylov_probe_dots(slab.handle, V.ctypes.data, count, w.ctypes.data, out.ctypes.data_as(C.POINTER(C.c_double))), "crd_krylov_probe_dots")
                err = np.abs(out.astype(np.longdouble) - ref).astype(np.float64)
                worst = max(worst, float((err / bound).max()))
                assert np.all(err <= bound), (count, shift, where, (err / bound).max())
    print("BOUND WORST multi-dot %s %dx%d: %.3g of the bound (K = %d)" % (precision, nx, ny, worst, kr.dot_roundings(n)))


# ---- 2. iteration counts ----------------------------------------------------------------------------------------------------------
COUNT_CASES = [(32, 128, "torus", False, 20.0), (32, 128, "torus", True, 500.0), (48, 192, "torus", False, 2000.0), (48, 192, "flat", True, 2000.0)]
assert all(c in [row[:5] for row in mg.GMRES_TABLE] for c in COUNT_CASES)


@functools.lru_cache(maxsize=None)
def counted_case(nx, ny, surface, held, multiple, precision):
    """(p, op, t, gamma, r, rtol, the reference's iteration count) of one row: rtol the geometric mean of two successive reference
    residuals whose ratio is at least 4 (fp32: both at least 100 u ||r||), the pair nearest 1e-8."""
    p, op = jr.case(jr.CONFIGS[0 if surface == "torus" else 1], nx, ny, precision)
    t, gamma, r = (T_ON if held else T_OFF), multiple * crd.stable_dt(p), right_hand_side(p)
    full = kr.reference_solve(op, t, gamma, r, precision, rtol=0.0, max_iters=30)
    pick = kr.tolerance_between(full.history, full.r_norm, 0.0 if precision == "f64" else 100 * eb.UNIT["f32"])
    assert pick is not None, full.history  # the condition holds on the reference
    return p, op, t, gamma, r, pick[0], pick[1]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny,surface,held,multiple", COUNT_CASES, ids=["%dx%d-%s-%s-%gx" % (c[0], c[1], c[2], "held" if c[3] else "free", c[4]) for c in COUNT_CASES])
def test_iteration_counts(gpu_device, nx, ny, surface, held, multiple, precision):
    p, op, t, gamma, r, rtol, expected = counted_case(nx, ny, surface, held, multiple, precision)
    with crd.Slab(p) as slab:
        z, st = slab.lsolve(t, gamma, r, rtol=rtol)
    print("COUNT %s %dx%d %s %s %gx: rtol %.3g, %d iterations on the device, %d in the reference" % (precision, nx, ny, surface, "held" if held else "free", multiple, rtol, st.iterations, expected))
    assert st.converged == 1 and st.restarts == 0 and st.breakdown == 0
    assert abs(st.iterations - expected) <= (0 if precision == "f64" else 1), (st.iterations, expected)
    assert st.matvecs == st.iterations and st.psolves == st.iterations + 1
    inside("%s %dx%d %s %gx" % (precision, nx, ny, surface, multiple), op, t, gamma, None, z, r, precision, jr.DIFFUSION, rtol, st)
    assert np.array_equal(z[..., 1], r[..., 1])


# ---- 3. restart and exhaustion ----------------------------------------------------------------------------------------------------
def test_restart_and_exhaustion(gpu_device):
    """Goldbeter torus 64 x 16 with held rows at 20 x the diffusion operator's explicit bound (multigrid_reference.explicit_bound: for
    Goldbeter crd_stable_dt is set by the kinetics and is 84 times smaller, and at 20 x THAT the solve takes four iterations): the coarse
    levels hold a row shifted by one fine row, one cycle is a poor inverse, and the reference gains about a factor 2 per iteration."""
    p, op = jr.case(jr.CONFIGS[2], 64, 16, "f64")
    gamma, r = 20.0 * mg.explicit_bound(op), right_hand_side(p)
    slow = kr.reference_solve(op, T_ON, gamma, r, "f64", restart=10)
    assert slow.converged and slow.restarts >= 2, (slow.restarts, slow.iterations)  # on the reference, before the device is read
    with crd.Slab(p) as slab:
        z, st = slab.lsolve(T_ON, gamma, r, restart=10)
        assert st.converged == 1 and st.restarts >= 2 and st.iterations > 20, stats_of(st)
        assert st.matvecs == st.iterations + st.restarts
        inside("restart 10", op, T_ON, gamma, None, z, r, "f64", jr.DIFFUSION, 1e-8, st)
        z, st = slab.lsolve(T_ON, gamma, r, max_iters=7)
        assert (st.converged, st.iterations, st.restarts) == (0, 7, 0), stats_of(st)
        assert np.isfinite(z).all()
        res, _ = kr.residual_allowance(op, T_ON, gamma, None, z, r, "f64", jr.DIFFUSION, 0.0)
        assert res < st.r_norm and abs(st.r_norm - np.linalg.norm(r)) <= 1e-12 * st.r_norm, (res, st.r_norm)
        # restart = 1: every cycle is one column
        z, st = slab.lsolve(T_ON, gamma, r, restart=1, max_iters=5)
        assert (st.converged, st.iterations, st.restarts) == (0, 5, 4) and np.isfinite(z).all()


# ---- 4. one level, odd widths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config_index", range(len(jr.CONFIGS)), ids=CONFIG_IDS)
def test_one_level_grids(gpu_device, config_index, precision):
    """61 x 9 and 130 x 33 have a single multigrid level and ragged tiles.  rtol: the default 1e-8 in fp64, 1e-5 in fp32 (above 100 u)."""
    rtol, u, worst = (1e-8 if precision == "f64" else 1e-5), eb.UNIT[precision], 0.0
    for nx, ny in [(61, 9), (130, 33)]:
        p, op = jr.case(jr.CONFIGS[config_index], nx, ny, precision)
        gamma, r = 20.0 * crd.stable_dt(p), right_hand_side(p)
        with crd.Slab(p) as slab:
            assert slab.psolve_info()[0] == 1
            for t in (T_ON, T_AT, T_OFF):
                z, st = slab.lsolve(t, gamma, r, rtol=rtol)
                assert st.converged == 1, (nx, ny, t, stats_of(st))
                worst = max(worst, inside("%s %s %dx%d t=%g" % (precision, CONFIG_IDS[config_index], nx, ny, t), op, t, gamma, None, z, r, precision, jr.DIFFUSION, rtol, st))
                assert np.all(np.abs(z[..., 1].astype(np.float64) - r[..., 1].astype(np.float64)) <= 2 * u * np.abs(r[..., 1].astype(np.float64)))
    print("BOUND WORST lsolve one level %s %s: %.3g of the allowance" % (precision, CONFIG_IDS[config_index], worst))


# ---- 5. the full Jacobian ---------------------------------------------------------------------------------------------------------
def test_full_jacobian_and_a_linearly_implicit_euler_step(gpu_device):
    """FHN flat 64 x 16 at h = 20 x crd_stable_dt around a non-uniform y0: (I - h J(y0)) z = f(y0) and y1 = y0 + h z, the Rosenbrock-Euler
    step; and the system of test_gpu_jacobian.test_linearly_implicit_euler_step, (I - h J_D) z = f(y0) (J_D y0 = f_D(y0): y0 + h z is that
    test's y1), against scipy's gmres on the same device matvec: the two y1 differ, under the long-double operator, by no more than the
    two solves' allowances.  With the kinetics in J the system is indefinite at this h (h (3 - 3 u^2) reaches 11) and the cycle for
    I - h J_D is a poor inverse of it: the long-double reference needs 255 iterations at restart 64 and stalls at restart 30, so the full
    part is solved with restart 64."""
    p, op = jr.case(jr.CONFIGS[1], 64, 16, "f64", t_boundary=0.0)
    y0 = jr.start_state(p, 1)
    h, rtol, shape = 20.0 * crd.stable_dt(p), 1e-10, y0.shape
    L = np.longdouble
    with crd.Slab(p) as slab:
        f0 = slab.rhs_part(0.0, y0, "full")
        for part, code in (("full", jr.FULL), ("diffusion", jr.DIFFUSION)):
            z, st = slab.lsolve(0.0, h, f0, y=y0, part=part, rtol=rtol, **(dict(restart=64, max_iters=1000) if part == "full" else {}))
            assert st.converged == 1, stats_of(st)
            _, allowed = kr.residual_allowance(op, 0.0, h, y0, z, f0, "f64", code, rtol)
            inside("implicit Euler, %s" % part, op, 0.0, h, y0, z, f0, "f64", code, rtol, st)
            x, _ = mg.gmres_iterations(lambda v: v - h * slab.jtimes(0.0, y0, v.reshape(shape), part).ravel(), f0.ravel(), rtol=rtol)
            x = x.reshape(shape)
            _, allowed_x = kr.residual_allowance(op, 0.0, h, y0, x, f0, "f64", code, rtol)
            inside("implicit Euler, %s, scipy" % part, op, 0.0, h, y0, x, f0, "f64", code, rtol)
            y1, y1_x = y0 + h * z, y0 + h * x
            d = y1.astype(L) - y1_x.astype(L)
            ad = d - L(h) * jr.jtimes_bound(op, 0.0, y0, d, "f64", code)[0]
            # forming y0 + h z on the host rounds twice per point, and A carries that on with ||A|| <= 1 + h (8 D / min(dx, dy)^2 + 3)
            forming = 2 * eb.UNIT["f64"] * (np.linalg.norm(y1) + np.linalg.norm(y1_x)) * (1 + h * (8 * np.abs(op.diff) / min(op.dx, op.dy) ** 2 + 3))
            assert float(np.linalg.norm(ad.astype(np.float64))) <= h * (allowed + allowed_x) + forming, part
            assert np.isfinite(y1).all() and np.abs(y1 - y0).max() > 1e-3  # the step went somewhere
    # y is read: another y gives another z
    with crd.Slab(p) as slab:
        z2, _ = slab.lsolve(0.0, h, f0, y=y0 + 0.5, part="full", rtol=rtol, restart=64, max_iters=1000)
        assert np.abs(z2 - z).max() > 1e-6


# ---- 6. without the preconditioner ------------------------------------------------------------------------------------------------
def test_without_preconditioner(gpu_device):
    p, op, t, gamma, r, _, _ = counted_case(32, 128, "torus", False, 20.0, "f64")
    with crd.Slab(p) as slab:
        z, st = slab.lsolve(t, gamma, r)
        zp, plain = slab.lsolve(t, gamma, r, precondition=False, restart=64, max_iters=2000)
    print("COUNT 32x128 free 20x: %d iterations with the cycle, %d without" % (st.iterations, plain.iterations))
    assert st.converged == 1 and plain.converged == 1 and plain.psolves == 0 and st.psolves == st.iterations + 1
    assert plain.iterations >= 4 * st.iterations, (plain.iterations, st.iterations)
    inside("no preconditioner", op, t, gamma, None, zp, r, "f64", jr.DIFFUSION, 1e-8, plain)


# ---- 7. breakdown -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_breakdown(gpu_device, precision):
    """A uniform field diffuses to exactly zero, so A v_0 = v_0: the first column is final."""
    p, op = jr.case(jr.CONFIGS[0], 48, 40, precision)
    r = np.full((40, 48, 2), 0.75, dtype=kr.DTYPES[precision])
    with crd.Slab(p) as slab:
        z, st = slab.lsolve(T_OFF, 20.0 * crd.stable_dt(p), r, precondition=False)
    assert (st.converged, st.iterations, st.breakdown, st.restarts) == (1, 1, 1, 0), stats_of(st)
    assert np.isfinite(z).all() and np.isfinite(st.res_norm)
    err = np.abs(z.astype(np.float64) - r.astype(np.float64)).max() / 0.75 / eb.UNIT[precision]
    print("BOUND breakdown %s: |z - r| = %.3g u |r| (allowed 4)" % (precision, err))
    assert err <= 4.0


# ---- 8. bit identities ------------------------------------------------------------------------------------------------------------
class Vectors:
    """Three device vectors of a slab's size in the process's own HIP runtime (test_gpu_multigrid.Device says why not torch)."""

    H2D, D2H = 1, 2

    def __init__(self, slab):
        self.slab, self.hip = slab, C.CDLL(None)
        self.hip.hipMalloc.argtypes, self.hip.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
        self.hip.hipFree.argtypes, self.hip.hipFree.restype = [C.c_void_p], C.c_int
        self.hip.hipMemcpy.argtypes, self.hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
        self.shape = (slab.nyl, slab.nx, 2)
        self.nbytes = int(np.prod(self.shape)) * np.dtype(slab.dtype).itemsize
        self.v = [C.c_void_p() for _ in range(3)]
        for v in self.v:
            assert self.hip.hipMalloc(C.byref(v), self.nbytes) == 0 and v.value

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.slab.synchronize()
        for v in self.v:
            assert self.hip.hipFree(v) == 0

    def up(self, k, x):
        x = np.ascontiguousarray(x, dtype=self.slab.dtype)
        assert x.shape == self.shape and self.hip.hipMemcpy(self.v[k], x.ctypes.data, self.nbytes, self.H2D) == 0
        return self.v[k]

    def down(self, k):
        out = np.empty(self.shape, dtype=self.slab.dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, self.v[k], self.nbytes, self.D2H) == 0
        return out


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("part", ["diffusion", "full"])
def test_bit_identities(gpu_device, part, precision):
    R = kr.DTYPES[precision]
    rtol = 1e-8 if precision == "f64" else 1e-5
    for nx, ny in [(48, 40), (130, 33)]:
        p, op = jr.case(jr.CONFIGS[0], nx, ny, precision)
        r, y0 = right_hand_side(p), jr.start_state(p, 1)
        gamma = 20.0 * crd.stable_dt(p)
        kw = dict(y=y0, part=part, rtol=rtol, restart=5)
        with crd.Slab(p) as slab, Vectors(slab) as dev:
            for t in (T_ON, T_OFF):
                z, st = slab.lsolve(t, gamma, r, **kw)
                assert st.converged == 1 and st.iterations > 0
                z2, st2 = slab.lsolve(t, gamma, r, **kw)
                assert np.array_equal(z, z2) and stats_of(st) == stats_of(st2)  # the same bits from run to run
                opt, std = crd.Slab._lsolve_options(part, True, 5, 200, rtol, 0.0), K.LsolveStats()
                slab._check(K.lib().crd_lsolve_device(slab.handle, t, gamma, C.byref(opt), dev.up(0, y0), dev.up(1, r), dev.v[2], C.byref(std)), "crd_lsolve_device")
                assert np.array_equal(dev.down(2), z) and stats_of(std) == stats_of(st)  # _host is _device
                z4, st4 = slab.lsolve(t, gamma, R(4.0) * r, **kw)
                assert np.array_equal(z4, R(4.0) * z) and st4.iterations == st.iterations  # powers of two commute with every rounding
                z0, st0 = slab.lsolve(t, 0.0, r, **kw)
                assert np.array_equal(z0, r) and (st0.iterations, st0.converged, st0.matvecs) == (0, 1, 0)  # gamma = 0: A = I
                zz, stz = slab.lsolve(t, gamma, np.zeros_like(r), **kw)
                assert not zz.any() and (stz.iterations, stz.converged, stz.r_norm) == (0, 1, 0.0)
                if part == "diffusion":
                    assert np.array_equal(z[..., 1], r[..., 1])
                    zn, _ = slab.lsolve(t, gamma, r, y=None, part=part, rtol=rtol, restart=5)  # y is not read
                    assert np.array_equal(zn, z)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_solve_leaves_the_state_alone(gpu_device, precision):
    p, op = jr.case(jr.CONFIGS[0], 48, 40, precision)
    y0, r = jr.start_state(p, 1), right_hand_side(p)
    dt = 0.5 * crd.stable_dt(p)
    with crd.Slab(p) as plain:
        plain.upload(y0)
        plain.step_rk4(0.0, dt, 3)
        plain.step_rk4(3 * dt, dt, 3)
        expected = plain.download()
    with crd.Slab(p) as slab:
        slab.upload(y0)
        slab.step_rk4(0.0, dt, 3)
        z, st = slab.lsolve(3 * dt, 20.0 * crd.stable_dt(p), r, y=y0, part="full", rtol=1e-5)
        assert st.iterations > 0
        slab.step_rk4(3 * dt, dt, 3)
        assert np.array_equal(slab.download(), expected)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_device):
    """Each CRD_EINVAL of the header, a member of a two-slab LOCAL group and a theta-block context (CRD_ESTATE), each with a message;
    crd_lsolve_info is the size of what the first call allocates."""
    p, op = jr.case(jr.CONFIGS[0], 48, 40, "f64")
    r = right_hand_side(p)
    L = K.lib()

    def refused(call, status):
        with pytest.raises(K.CrdError) as e:
            call()
        assert e.value.status == status, e.value
        return str(e.value)

    with crd.Slab(p) as slab:
        bad = [dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(part="reaction"), dict(part=7), dict(restart=0), dict(restart=65),
               dict(max_iters=0), dict(max_iters=-3), dict(rtol=-1e-3), dict(rtol=float("nan")), dict(atol=-1.0), dict(atol=float("inf")), dict(part="full"),
               dict(pre=0, post=0), dict(coarse=0), dict(max_levels=17), dict(omega=0.0), dict(precondition=2)]
        for kw in bad:
            gamma = kw.pop("gamma", 1.0)
            refused(lambda: slab.lsolve(0.0, gamma, r, **kw), K.EINVAL)
            assert "lsolve" in L.crd_last_error(slab.handle).decode(), kw
            if gamma == 1.0 and kw != dict(part="full"):  # (the options alone: crd_lsolve_info refuses them too)
                refused(lambda: slab.lsolve_info(**kw), K.EINVAL)
        refused(lambda: slab.lsolve(0.0, 1.0, r, part="full"), K.EINVAL)
        assert "needs y" in L.crd_last_error(slab.handle).decode()
        same, other = np.ascontiguousarray(r), np.ascontiguousarray(r.copy())
        st = K.LsolveStats()
        for y, rr, z in ((None, same, same), (same, other, same)):  # z == r; z == y
            for entry in (L.crd_lsolve_host, L.crd_lsolve_device):
                rc = entry(slab.handle, 0.0, 1.0, None, None if y is None else y.ctypes.data, rr.ctypes.data, z.ctypes.data, C.byref(st))
                assert rc == K.EINVAL and "z must not be" in L.crd_last_error(slab.handle).decode()
        assert L.crd_lsolve_host(slab.handle, 0.0, 1.0, None, None, None, same.ctypes.data, None) == K.EINVAL
        # nothing was allocated by any of that; the size reported is (restart + 3) vectors, each padded to 256 bytes, and the scalars:
        # 65 x 512 + 512 partials and three blocks of 128 doubles
        vec = -(-r.nbytes // 256) * 256
        for restart in (30, 7, 64):
            assert slab.lsolve_info(restart=restart) == (restart + 3) * vec + (65 * 512 + 512 + 3 * 128) * 8
        z, st = slab.lsolve(0.0, 1.0, r, restart=64, max_iters=1, rtol=0.0, atol=0.0)  # the ends of the ranges are inside
        assert st.iterations == 1 and np.isfinite(z).all()
    with crd.LocalGroup(p, 2) as group:
        s = group.slabs[1]
        msg = refused(lambda: s.lsolve(0.0, 1.0, r[s.js:s.je + 1]), K.ESTATE)
        assert "whole grid" in msg
        refused(lambda: s.lsolve(0.0, 1.0, r[s.js:s.je + 1], precondition=False), K.ESTATE)
        refused(lambda: s.lsolve_info(), K.ESTATE)
    with crd.LocalGroup(p, 4, blocks=(2, 2)) as blocks:
        s = blocks.slabs[0]
        msg = refused(lambda: s.lsolve(0.0, 1.0, r[s.js:s.je + 1, s.is_:s.ie + 1]), K.ESTATE)
        assert "theta-blocks" in msg
