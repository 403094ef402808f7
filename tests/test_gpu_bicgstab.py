"""The BiCGStab solve on the device (crd_bicgstab_* / Slab.lsolve_bicgstab): right-preconditioned BiCGStab for (I - gamma J_part) z = r.

Each fused kernel alone, through crd_bicgstab_probe: its output vectors bit for bit the fma_exact composition, its sums within the bound
counted from the summation tree (tests/bicgstab_reference.py), one planted element carrying each.  The solve: the half-step at which the
long-double reference stops (fp32: float64 on the widened vectors, +- 1 half-step) at a tolerance placed between two of the reference's
residuals, both residuals inside the allowance of tests/krylov_reference.py, the launch counts the algorithm implies; one-level grids,
exhaustion, the half exit, a NaN, warm starts, the full Jacobian where the system is definite, GMRES's solution of the same system; the
identities the header promises bit for bit; and every refusal with its message.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bicgstab_reference as br
import crdmodel_amd as crd
import jacobian_reference as jr
import krylov_reference as kr
import multigrid_reference as mg
from oracle import error_bounds as eb
from test_gpu_krylov import COUNT_CASES, Vectors, right_hand_side

pytestmark = pytest.mark.gpu

CONFIG_IDS = [c[0] for c in jr.CONFIGS]
T_ON, T_AT, T_OFF = jr.TIMES
K = crd._capi
STATS = ("converged", "iterations", "half_exit", "matvecs", "psolves", "breakdown", "r_norm", "res_norm", "true_res_norm")
RTOL = {"f64": 1e-8, "f32": 1e-5}


def stats_of(st):
    return tuple(getattr(st, f) for f in STATS)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    kind = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(kind), b.view(kind))


def inside(case, op, t, gamma, y, z, r, precision, part, rtol, st, atol=0.0):
    """The residual of z under the reference operator and the device's own true residual against the allowance; observed / allowed."""
    res, allowed = kr.residual_allowance(op, t, gamma, y, z, r, precision, part, rtol, atol)
    print("BOUND bicgstab %s: residual %.3g, true_res_norm %.3g, recurrence %.3g, allowed %.3g after %d iterations" % (case, res, st.true_res_norm, st.res_norm, allowed, st.iterations))
    assert np.isfinite(np.asarray(z, dtype=np.float64)).all(), case
    assert res <= allowed and st.true_res_norm <= allowed, (case, res, st.true_res_norm, allowed)
    return res / allowed


# ---- 1. each fused kernel alone ---------------------------------------------------------------------------------------------------
def probe(slab, kernel, ins, scalars, var0_only=False):
    n_in, _, n_out, n_sums = br.KERNELS[kernel]
    packed = np.ascontiguousarray(np.stack(ins))
    out = np.full((n_out,) + ins[0].shape, np.nan, dtype=ins[0].dtype)
    sums, sc = np.full(2, np.nan), np.array(list(scalars) + [0.0], dtype=np.float64)
    slab._check(K.lib().crd_bicgstab_probe(slab.handle, K.BICGSTAB_KERNELS[kernel], int(var0_only), sc.ctypes.data_as(C.POINTER(C.c_double)), packed.ctypes.data,
                                           out.ctypes.data, sums.ctypes.data_as(C.POINTER(C.c_double))), "crd_bicgstab_probe")
    return list(out), list(sums[:n_sums])


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("big", [False, True], ids=["19x27", "two-trips"])
def test_each_kernel_alone(gpu_device, big, precision):
    """19 x 27: 513 points -- a ragged last block, and in fp32 a lone last point (two reals of a unit).  two-trips: the smallest grid 1030
    wide above one grid-stride trip of kBcgBlocks x kBcgThreads units.  Every plant position for every kernel that leaves sums (on
    the large grid index 0, those around the trip's boundary and the last: its vectors are 8 MB, and the restatement is numpy); the two
    kernels without sums once per grid; the var1 mask of the apply kernels once per grid."""
    nx, ny = br.smallest_grid_above_one_trip(precision) if big else (19, 27)
    n = 2 * nx * ny
    assert br.trips(n, precision) == (2 if big else 1) and br.units(n, precision) % br.THREADS != 0 and (big or precision == "f64" or n % 4 == 2)
    p, _ = jr.case(jr.CONFIGS[0], nx, ny, precision)
    positions = br.plant_positions(n, precision)
    assert {q % 2 for q in positions} == {0, 1}
    worst = 0.0
    with crd.Slab(p) as slab:
        for kernel in br.KERNELS:
            # (two-trips: index 0 and the positions only that grid has -- either side of the trip's boundary, and n - 1; the wavefront's
            # and the block's boundaries are 19 x 27's, and an error there in a second trip's indexing would move output bits, which
            # are compared over the whole vector)
            for q1 in (positions[:1] + positions[-3:] if big else positions) if br.KERNELS[kernel][3] else positions[:1]:
                q2 = positions[(positions.index(q1) + 1) % len(positions)]
                for var0_only in (False, True) if kernel.startswith("apply") and q1 == positions[0] else (False,):
                    if var0_only:  # (a plant in var1 would be masked)
                        q2 = [q for q in positions if q % 2 == 0 and q != q1][0]
                    ins = br.planted_case(kernel, n, precision, q1, q2)
                    outs, pairs = br.kernel_reference(kernel, ins, br.SCALARS[kernel], precision, var0_only)
                    for (a, b), q in zip(pairs, br.carriers(kernel, q1, q2)):
                        assert abs(float(a[q]) * float(b[q])) >= 0.5 * br.sum_bound(a, b, precision)[2]  # on the reference, before the device is read
                    got, sums = probe(slab, kernel, ins, br.SCALARS[kernel], var0_only)
                    for g, o in zip(got, outs):
                        assert same_bits(g, o), (kernel, q1, var0_only, np.abs(g.astype(np.float64) - o).max())
                    q = br.sums_gate(sums, br.sum_pairs(kernel, ins, got), precision)  # the sums over the device's own stored vectors
                    worst = max(worst, q)
                    assert q <= 1.0, (kernel, q1, var0_only, q)
    print("BOUND WORST bicgstab sums %s %dx%d: %.3g of the bound (K = %d)" % (precision, nx, ny, worst, br.sum_roundings(n, precision)))


# ---- 2. iteration counts ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counted_case(nx, ny, surface, held, multiple, precision):
    """(p, op, t, gamma, r, rtol, the reference's half-steps): rtol the geometric mean of two successive entries of the reference's
    interleaved history whose ratio is at least 4 (fp32: both at least 100 u ||r||), the pair nearest 1e-8 (fp32: 1e-5).  BiCGStab's
    residuals do not fall monotonically (48 x 192 flat: 2.5e-8, 8.0e-9, 9.7e-8, 2.0e-8 in a row), so the half-step expected is the FIRST
    entry at or below the tolerance, not the pair's own, and no entry up to it may lie within a factor 1.5 of the tolerance."""
    p, op = jr.case(jr.CONFIGS[0 if surface == "torus" else 1], nx, ny, precision)
    t, gamma, r = (T_ON if held else T_OFF), multiple * crd.stable_dt(p), right_hand_side(p)
    full = br.reference_solve(op, t, gamma, r, precision, rtol=0.0, max_iters=20)
    pick = kr.tolerance_between(full.history, full.r_norm, 0.0 if precision == "f64" else 100 * eb.UNIT["f32"], near=RTOL[precision])
    assert pick is not None, full.history  # the condition holds on the reference
    rel = np.asarray(full.history) / full.r_norm
    first = int(np.argmax(rel <= pick[0]))
    assert rel[first] <= pick[0] and first <= pick[1] and np.all(np.abs(np.log(rel[:first + 1] / pick[0])) >= np.log(1.5)), (rel, pick)
    return p, op, t, gamma, r, pick[0], first


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny,surface,held,multiple", COUNT_CASES, ids=["%dx%d-%s-%s-%gx" % (c[0], c[1], c[2], "held" if c[3] else "free", c[4]) for c in COUNT_CASES])
def test_iteration_counts(gpu_device, nx, ny, surface, held, multiple, precision):
    p, op, t, gamma, r, rtol, expected = counted_case(nx, ny, surface, held, multiple, precision)
    with crd.Slab(p) as slab:
        z, st = slab.lsolve_bicgstab(t, gamma, r, rtol=rtol)
    halves = 2 * st.iterations - st.half_exit
    print("COUNT bicgstab %s %dx%d %s %s %gx: rtol %.3g, %d half-steps on the device, %d in the reference" % (precision, nx, ny, surface, "held" if held else "free", multiple, rtol, halves, expected))
    assert st.converged == 1 and st.breakdown == 0, stats_of(st)
    assert abs(halves - expected) <= (0 if precision == "f64" else 1), (halves, expected)
    assert (st.matvecs, st.psolves) == br.implied_counts(st.iterations, st.half_exit), stats_of(st)
    inside("%s %dx%d %s %gx" % (precision, nx, ny, surface, multiple), op, t, gamma, None, z, r, precision, jr.DIFFUSION, rtol, st)
    assert np.array_equal(z[..., 1], r[..., 1])


# ---- 3. one level, odd widths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config_index", range(len(jr.CONFIGS)), ids=CONFIG_IDS)
def test_one_level_grids(gpu_device, config_index, precision):
    rtol, worst = RTOL[precision], 0.0
    for nx, ny in [(61, 9), (130, 33)]:
        p, op = jr.case(jr.CONFIGS[config_index], nx, ny, precision)
        gamma, r = 20.0 * crd.stable_dt(p), right_hand_side(p)
        with crd.Slab(p) as slab:
            assert slab.psolve_info()[0] == 1
            for t in (T_ON, T_AT, T_OFF):
                z, st = slab.lsolve_bicgstab(t, gamma, r, rtol=rtol)
                assert st.converged == 1 and st.breakdown == 0, (nx, ny, t, stats_of(st))
                worst = max(worst, inside("%s %s %dx%d t=%g" % (precision, CONFIG_IDS[config_index], nx, ny, t), op, t, gamma, None, z, r, precision, jr.DIFFUSION, rtol, st))
                assert np.array_equal(z[..., 1], r[..., 1])
    print("BOUND WORST bicgstab one level %s %s: %.3g of the allowance" % (precision, CONFIG_IDS[config_index], worst))


# ---- 4. - 6. exhaustion, the half exit, a NaN -------------------------------------------------------------------------------------
def test_exhaustion(gpu_device):
    p, op = jr.case(jr.CONFIGS[2], 64, 16, "f64")
    gamma, r = 20.0 * mg.explicit_bound(op), right_hand_side(p)
    full = br.reference_solve(op, T_ON, gamma, r, "f64")
    assert full.converged and full.iterations > 8, full.iterations  # on the reference, before the device is read
    with crd.Slab(p) as slab:
        z, st = slab.lsolve_bicgstab(T_ON, gamma, r, max_iters=4)
        assert (st.converged, st.iterations, st.half_exit, st.breakdown) == (0, 4, 0, 0), stats_of(st)
        assert (st.matvecs, st.psolves) == br.implied_counts(4, 0)
        assert np.isfinite(z).all()
        res, _ = kr.residual_allowance(op, T_ON, gamma, None, z, r, "f64", jr.DIFFUSION, 0.0)
        assert res < st.r_norm and st.true_res_norm < st.r_norm and abs(st.r_norm - np.linalg.norm(r)) <= 1e-12 * st.r_norm


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_half_exit(gpu_device, precision):
    """A uniform field diffuses to exactly zero, so A p = p: alpha = 1 and s = 0."""
    p, op = jr.case(jr.CONFIGS[0], 48, 40, precision)
    r = np.full((40, 48, 2), 0.75, dtype=kr.DTYPES[precision])
    with crd.Slab(p) as slab:
        z, st = slab.lsolve_bicgstab(T_OFF, 20.0 * crd.stable_dt(p), r, precondition=False)
    assert (st.converged, st.iterations, st.half_exit, st.breakdown) == (1, 1, 1, 0), stats_of(st)
    assert (st.matvecs, st.psolves) == br.implied_counts(1, 1, precondition=False)
    err = np.abs(z.astype(np.float64) - r.astype(np.float64)).max() / 0.75 / eb.UNIT[precision]
    print("BOUND bicgstab half exit %s: |z - r| = %.3g u |r| (allowed 4)" % (precision, err))
    assert err <= 4.0


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_right_hand_side_that_is_not_finite(gpu_device, precision):
    p, op = jr.case(jr.CONFIGS[0], 48, 40, precision)
    r = right_hand_side(p)
    r[7, 11, 0] = np.nan
    with crd.Slab(p) as slab:
        z, st = slab.lsolve_bicgstab(T_OFF, 20.0 * crd.stable_dt(p), r)
        assert (st.converged, st.iterations, st.breakdown, st.psolves) == (0, 0, 0, 0) and np.isnan(st.r_norm), stats_of(st)
        good = right_hand_side(p)
        z, st = slab.lsolve_bicgstab(T_OFF, 20.0 * crd.stable_dt(p), good, rtol=RTOL[precision])  # the context is none the worse
        assert st.converged == 1 and np.isfinite(z).all()


# ---- 7. warm starts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_warm_starts(gpu_device, precision):
    nx, ny, surface, held, multiple = COUNT_CASES[1]
    p, op = jr.case(jr.CONFIGS[0], nx, ny, precision)
    t, gamma, r, rtol = T_ON, multiple * crd.stable_dt(p), right_hand_side(p), RTOL[precision]
    ref = br.reference_solve(op, t, gamma, r, precision, rtol=rtol)
    near = br.reference_solve(op, t, gamma, r, precision, rtol=rtol, guess=1.01 * ref.z)
    assert near.converged and br.half_steps(near) < br.half_steps(ref) - 1  # on the reference first
    with crd.Slab(p) as slab:
        cold, sc = slab.lsolve_bicgstab(t, gamma, r, rtol=rtol)
        # (at 10 rtol: cold was converged on the recurrence's residual, and the residual r - A z the warm start forms may sit a rounding
        # above that -- asserted next, on the device's own true residual)
        assert sc.res_norm <= rtol * sc.r_norm and sc.true_res_norm <= 10 * rtol * sc.r_norm
        again, sa = slab.lsolve_bicgstab(t, gamma, r, rtol=10 * rtol, guess=cold)
        assert (sa.converged, sa.iterations, sa.matvecs, sa.psolves) == (1, 0, 2, 0), stats_of(sa)
        assert same_bits(again[..., 0], cold[..., 0]) and same_bits(again[..., 1], r[..., 1])
        zero, sz = slab.lsolve_bicgstab(t, gamma, r, rtol=rtol, guess=np.zeros_like(r))
        assert same_bits(zero, cold) and sz.iterations == sc.iterations and sz.matvecs == sc.matvecs + 1
        R = kr.DTYPES[precision]
        warm, sw = slab.lsolve_bicgstab(t, gamma, r, rtol=rtol, guess=(R(1.01) * cold).astype(R))
        assert sw.converged == 1 and 2 * sw.iterations - sw.half_exit < 2 * sc.iterations - sc.half_exit, (stats_of(sw), stats_of(sc))
        assert (sw.matvecs, sw.psolves) == br.implied_counts(sw.iterations, sw.half_exit, guess=True)
        inside("warm %s" % precision, op, t, gamma, None, warm, r, precision, jr.DIFFUSION, rtol, sw)
        # var1 of the guess is not read
        junk = (R(1.01) * cold).astype(R)
        junk[..., 1] = np.nan
        warm2, sw2 = slab.lsolve_bicgstab(t, gamma, r, rtol=rtol, guess=junk)
        assert same_bits(warm2, warm) and stats_of(sw2) == stats_of(sw)


# the seven systems of the issue's table: (configuration, nx, ny, rows held, multiple, its unit)
WARM_CASES = [(0 if c[2] == "torus" else 1, c[0], c[1], c[3], c[4], "stable_dt") for c in COUNT_CASES] + [
    (2, 64, 16, True, 20.0, "explicit_bound"), (0, 61, 9, True, 20.0, "explicit_bound"), (3, 130, 33, True, 20.0, "explicit_bound")]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config,nx,ny,held,multiple,unit", WARM_CASES, ids=["%s-%dx%d-%gx" % (CONFIG_IDS[c[0]], c[1], c[2], c[4]) for c in WARM_CASES])
def test_a_guess_near_the_solution_takes_fewer_iterations(gpu_device, config, nx, ny, held, multiple, unit, precision):
    """guess = 1.01 x the solution against a cold start.  On the reference first: the warm solve stops strictly earlier in every case
    (fp64 5 - 22 half-steps against 7 - 30, fp32 3 - 11 against 4 - 19).  The device is held to "strictly fewer" where the reference's gap
    exceeds what the two counts may differ from the reference's by themselves (fp64: these tolerances are not placed between two
    residuals, so one half-step each; fp32: the count gate's own half-step each), and to "no more" otherwise."""
    p, op = jr.case(jr.CONFIGS[config], nx, ny, precision)
    t, r, rtol = (T_ON if held else T_OFF), right_hand_side(p), RTOL[precision]
    gamma = multiple * (crd.stable_dt(p) if unit == "stable_dt" else mg.explicit_bound(op))
    ref = br.reference_solve(op, t, gamma, r, precision, rtol=rtol)
    near = br.reference_solve(op, t, gamma, r, precision, rtol=rtol, guess=1.01 * ref.z)
    assert ref.converged and near.converged and br.half_steps(near) < br.half_steps(ref)  # on the reference first
    R = kr.DTYPES[precision]
    with crd.Slab(p) as slab:
        cold, sc = slab.lsolve_bicgstab(t, gamma, r, rtol=rtol)
        warm, sw = slab.lsolve_bicgstab(t, gamma, r, rtol=rtol, guess=(R(1.01) * cold).astype(R))
    hc, hw = 2 * sc.iterations - sc.half_exit, 2 * sw.iterations - sw.half_exit
    print("COUNT bicgstab warm %s %s %dx%d %gx: %d half-steps cold, %d warm (reference %d, %d)" % (precision, CONFIG_IDS[config], nx, ny, multiple, hc, hw, br.half_steps(ref), br.half_steps(near)))
    assert sc.converged == 1 and sw.converged == 1 and sw.breakdown == 0
    assert hw <= hc and (hw < hc or br.half_steps(ref) - br.half_steps(near) <= 2), (hc, hw)
    inside("warm %s %s %dx%d" % (precision, CONFIG_IDS[config], nx, ny), op, t, gamma, None, warm, r, precision, jr.DIFFUSION, rtol, sw)


# ---- 8. bit identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("part", ["diffusion", "full"])
def test_bit_identities(gpu_device, part, precision):
    R, rtol = kr.DTYPES[precision], RTOL[precision]
    for nx, ny in [(48, 40), (130, 33)]:
        p, op = jr.case(jr.CONFIGS[0], nx, ny, precision)
        r, y0 = right_hand_side(p), jr.start_state(p, 1)
        # (the full part where I - gamma J is definite: gamma max |3 - 3 u^2| = 1 / 2)
        gamma = 20.0 * crd.stable_dt(p) if part == "diffusion" else 0.5 / float(np.abs(3.0 - 3.0 * y0[..., 0].astype(np.float64) ** 2).max())
        kw = dict(y=y0, part=part, rtol=rtol)
        with crd.Slab(p) as slab, Vectors(slab) as dev:
            for t in (T_ON, T_OFF):
                zg, sg = slab.lsolve(t, gamma, r, **kw)
                z, st = slab.lsolve_bicgstab(t, gamma, r, **kw)
                assert st.converged == 1 and st.iterations > 0, stats_of(st)
                z2, st2 = slab.lsolve_bicgstab(t, gamma, r, **kw)
                assert same_bits(z, z2) and stats_of(st) == stats_of(st2)  # the same bits from run to run
                zg2, sg2 = slab.lsolve(t, gamma, r, **kw)
                assert same_bits(zg, zg2) and sg.iterations == sg2.iterations  # GMRES before and after: its workspace is its own
                opt, std = crd.Slab._bicgstab_options(part, True, 200, False, rtol, 0.0), K.BicgstabStats()
                slab._check(K.lib().crd_bicgstab_device(slab.handle, t, gamma, C.byref(opt), dev.up(0, y0), dev.up(1, r), dev.v[2], C.byref(std)), "crd_bicgstab_device")
                assert same_bits(dev.down(2), z) and stats_of(std) == stats_of(st)  # _host is _device
                z4, st4 = slab.lsolve_bicgstab(t, gamma, R(4.0) * r, **kw)
                assert same_bits(z4, R(4.0) * z) and st4.iterations == st.iterations  # powers of two commute with every rounding
                z0, st0 = slab.lsolve_bicgstab(t, 0.0, r, **kw)
                assert same_bits(z0, r) and (st0.iterations, st0.converged, st0.matvecs) == (0, 1, 0)  # gamma = 0: A = I
                zz, stz = slab.lsolve_bicgstab(t, gamma, np.zeros_like(r), **kw)
                assert not zz.any() and (stz.iterations, stz.converged, stz.r_norm) == (0, 1, 0.0)
                if part == "diffusion":
                    assert np.array_equal(z[..., 1], r[..., 1])
                    zn, _ = slab.lsolve_bicgstab(t, gamma, r, part=part, rtol=rtol)  # y is not read
                    assert same_bits(zn, z)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_solve_leaves_the_state_alone(gpu_device, precision):
    p, op = jr.case(jr.CONFIGS[0], 48, 40, precision)
    y0, r = jr.start_state(p, 1), right_hand_side(p)
    dt = 0.5 * crd.stable_dt(p)
    with crd.Slab(p) as plain:
        plain.upload(y0)
        plain.step_rk4(0.0, dt, 6)
        expected = plain.download()
    with crd.Slab(p) as slab:
        slab.upload(y0)
        slab.step_rk4(0.0, dt, 3)
        z, st = slab.lsolve_bicgstab(3 * dt, 20.0 * crd.stable_dt(p), r, rtol=1e-5)
        assert st.iterations > 0
        slab.step_rk4(3 * dt, dt, 3)
        assert np.array_equal(slab.download(), expected)


# ---- 9. the full Jacobian where the system is definite ----------------------------------------------------------------------------
def test_full_jacobian_where_the_system_is_definite(gpu_device):
    p, op = jr.case(jr.CONFIGS[1], 64, 16, "f64", t_boundary=0.0)
    y0 = jr.start_state(p, 1)
    peak = float(np.abs(3.0 - 3.0 * y0[..., 0] ** 2).max())
    gamma = 0.9 / peak
    assert gamma * peak < 1.0  # on the reference: the kinetics cannot make I - gamma J indefinite
    rtol = 1e-10
    with crd.Slab(p) as slab:
        f0 = slab.rhs_part(0.0, y0, "full")
        z, st = slab.lsolve_bicgstab(0.0, gamma, f0, y=y0, part="full", rtol=rtol)
        assert st.converged == 1 and st.breakdown == 0, stats_of(st)
        inside("full Jacobian", op, 0.0, gamma, y0, z, f0, "f64", jr.FULL, rtol, st)
        z2, st2 = slab.lsolve_bicgstab(0.0, gamma, f0, y=y0 + 0.5, part="full", rtol=rtol)  # y is read: another y gives another z
        assert st2.converged == 1 and np.abs(z2 - z).max() > 1e-6


# ---- 10. against GMRES ------------------------------------------------------------------------------------------------------------
def test_against_gmres(gpu_device):
    p, op, t, gamma, r, _, _ = counted_case(48, 192, "flat", True, 2000.0, "f64")
    L = np.longdouble
    with crd.Slab(p) as slab:
        zb, sb = slab.lsolve_bicgstab(t, gamma, r)
        zg, sg = slab.lsolve(t, gamma, r)
    assert sb.converged == 1 and sg.converged == 1
    _, allowed_b = kr.residual_allowance(op, t, gamma, None, zb, r, "f64", jr.DIFFUSION, 1e-8)
    _, allowed_g = kr.residual_allowance(op, t, gamma, None, zg, r, "f64", jr.DIFFUSION, 1e-8)
    d = zb.astype(L) - zg.astype(L)
    ad = d - L(gamma) * jr.jtimes_bound(op, t, np.zeros(d.shape), d, "f64", jr.DIFFUSION)[0]
    gap = float(np.linalg.norm(ad.astype(np.float64)))
    print("BOUND bicgstab against GMRES: ||A (z_b - z_g)|| = %.3g, allowed %.3g; %d BiCGStab iterations, %d GMRES" % (gap, allowed_b + allowed_g, sb.iterations, sg.iterations))
    assert gap <= allowed_b + allowed_g


# ---- 11. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_device):
    p, op = jr.case(jr.CONFIGS[0], 48, 40, "f64")
    r = right_hand_side(p)
    L = K.lib()

    def refused(call, status):
        with pytest.raises(K.CrdError) as e:
            call()
        assert e.value.status == status, e.value
        return str(e.value)

    with crd.Slab(p) as slab:
        bad = [dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(part="reaction"), dict(part=7), dict(max_iters=0), dict(max_iters=-3),
               dict(rtol=-1e-3), dict(rtol=float("nan")), dict(atol=-1.0), dict(atol=float("inf")), dict(part="full"), dict(pre=0, post=0), dict(coarse=0),
               dict(max_levels=17), dict(omega=0.0), dict(precondition=2)]
        for kw in bad:
            gamma = kw.pop("gamma", 1.0)
            refused(lambda: slab.lsolve_bicgstab(0.0, gamma, r, **kw), K.EINVAL)
            assert "bicgstab" in L.crd_last_error(slab.handle).decode(), kw
            if gamma == 1.0 and kw != dict(part="full"):
                refused(lambda: slab.lsolve_bicgstab_info(**kw), K.EINVAL)
        refused(lambda: slab.lsolve_bicgstab(0.0, 1.0, r, part="full"), K.EINVAL)
        assert "needs y" in L.crd_last_error(slab.handle).decode()
        same, other = np.ascontiguousarray(r), np.ascontiguousarray(r.copy())
        st = K.BicgstabStats()
        for y, rr, z in ((None, same, same), (same, other, same)):  # z == r; z == y
            for entry in (L.crd_bicgstab_host, L.crd_bicgstab_device):
                rc = entry(slab.handle, 0.0, 1.0, None, None if y is None else y.ctypes.data, rr.ctypes.data, z.ctypes.data, C.byref(st))
                assert rc == K.EINVAL and "z must not be" in L.crd_last_error(slab.handle).decode()
        assert L.crd_bicgstab_host(slab.handle, 0.0, 1.0, None, None, None, same.ctypes.data, None) == K.EINVAL
        for guess in (2, -1):
            opt = crd.Slab._bicgstab_options()
            opt.guess = guess
            assert L.crd_bicgstab_host(slab.handle, 0.0, 1.0, C.byref(opt), None, same.ctypes.data, other.ctypes.data, None) == K.EINVAL
            assert "guess must be 0 or 1" in L.crd_last_error(slab.handle).decode()
        sc = (C.c_double * 2)(0.5, 0.5)
        assert L.crd_bicgstab_probe(slab.handle, 6, 0, sc, same.ctypes.data, other.ctypes.data, None) == K.EINVAL
        assert L.crd_bicgstab_probe(slab.handle, 0, 2, sc, same.ctypes.data, other.ctypes.data, None) == K.EINVAL
        # eight vectors, each padded to 256 bytes, and two slots of 2048 partials -- whatever the options, and less than GMRES(30)'s 33
        vec = -(-r.nbytes // 256) * 256
        assert slab.lsolve_bicgstab_info() == slab.lsolve_bicgstab_info(max_iters=7, precondition=False) == 8 * vec + 2 * 2048 * 8
        z, st = slab.lsolve_bicgstab(0.0, 1.0, r, max_iters=1, rtol=0.0, atol=0.0)  # the ends of the ranges are inside
        assert st.iterations == 1 and np.isfinite(z).all()
    with crd.LocalGroup(p, 2) as group:
        s = group.slabs[1]
        msg = refused(lambda: s.lsolve_bicgstab(0.0, 1.0, r[s.js:s.je + 1]), K.ESTATE)
        assert "whole grid" in msg
        refused(lambda: s.lsolve_bicgstab_info(), K.ESTATE)
    with crd.LocalGroup(p, 4, blocks=(2, 2)) as blocks:
        s = blocks.slabs[0]
        msg = refused(lambda: s.lsolve_bicgstab(0.0, 1.0, r[s.js:s.je + 1, s.is_:s.ie + 1]), K.ESTATE)
        assert "theta-blocks" in msg
