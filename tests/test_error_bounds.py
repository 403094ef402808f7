"""The per-point rounding-error bound of oracle/error_bounds.py on the host: honest (correct restatements stay inside it), sharp
(the kernel-order fp32 restatement comes within a small factor of it) and powerful (mistakes that pass the joint max-norm gate
of conftest.rel_err fail it, with the point named)."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import crd_oracle as co
from oracle import crd_oracle_np as cn
from oracle import error_bounds as eb

L, W, D = 80.0, 20.0, 0.12

# (label, model, surface, beta, keyword arguments of co.make_problem)
CASES = [
    ("fhn-torus-varybeta", co.FHN, co.TORUS, 1.25, dict(vary_beta=1, beta_min=0.3, beta_max=1.4)),
    ("fhn-flat", co.FHN, co.FLAT, 1.25, {}),
    ("goldbeter-torus", co.GOLDBETER, co.TORUS, 0.4, {}),
    ("goldbeter-flat-varybeta", co.GOLDBETER, co.FLAT, 0.4, dict(vary_beta=1, beta_min=0.0, beta_max=1.0)),
    ("diffusion-only-torus", co.GOLDBETER, co.TORUS, 0.4, dict(just_diffusion=1)),
    ("diffusion-only-flat", co.GOLDBETER, co.FLAT, 0.4, dict(just_diffusion=1)),
]


def problem(case, n, t_boundary=0.0):
    _, model, surface, beta, kw = case
    return co.make_problem(model, surface, n, L, W, D, beta, ny=n, t_boundary=t_boundary, **kw)


def state(op, seed=1):
    """The reference's front-style initial state (built with vary_beta off, so the front exists), a smooth perturbation, a little
    noise, and for Goldbeter a patch of small z."""
    q = co.Problem.from_buffer_copy(op)
    q.vary_beta = 0
    y = co.initial_conditions(q, 0.1, 0.5, 0)
    ny, nx = y.shape[:2]
    th, ph = np.arange(nx) * op.dx, np.arange(ny) * op.dy
    y[..., 0] += 0.05 * np.sin(th)[None, :] * np.cos(ph)[:, None]
    y[..., 1] += 0.05 * np.cos(th)[None, :] * np.sin(2 * ph)[:, None]
    rng = np.random.default_rng(seed)
    y += 1e-5 * rng.standard_normal(y.shape)
    if op.model == co.GOLDBETER:
        r0, r1, c1 = ny // 2, ny // 2 + ny // 4, nx // 3
        y[r0:r1, :c1, 0] = rng.uniform(1e-3, 0.2, (r1 - r0, c1))
    return y


# ---- restatements ----------------------------------------------------------------------------------------------------------------
def _fma(R):
    """Fused multiply-add of the precision R, emulated one size up (exact product for float32; 64-bit significand for float64)."""
    wide = np.float64 if R == np.float32 else np.longdouble
    return lambda a, b, c: (np.asarray(a, wide) * np.asarray(b, wide) + np.asarray(c, wide)).astype(R)


def _reciprocal(x):
    """The device's 1/x: an estimate (here the correctly rounded value) refined by one Newton step."""
    fma = _fma(x.dtype.type)
    r = (1 / x.astype(np.longdouble)).astype(x.dtype)
    return fma(r, fma(-x, r, x.dtype.type(1)), r)


def kernel_order_rhs(op, t, y, R, plant=None, eps=cn.EPSILON, j0=0):
    """crd_device.h's point function in precision R, in its order: theta first differences, explicit fused multiply-adds, the host's
    fp64 tables rounded to R.  plant: "seam" (column 0 takes its west neighbour from column nx-2), "brow" (the row parameter read
    one row below), "row_n" (the absorbing rule forgets row ny-1)."""
    fma = _fma(R)
    P = eb._Problem(op)
    cE, cWn, cP = (c.astype(R)[None, :] for c in (P.cE, P.cWn, P.cP))
    b = cn.beta_rows(P.g, op.beta, op.vary_beta, op.beta_min, op.beta_max, np.float64, j0 - 1, y.shape[0] + 1)
    rowp = cn.EPSILON * b if op.model == co.FHN else (np.longdouble(7.3) * b.astype(np.longdouble) + 1).astype(np.float64)  # host: fma(v1, b, v0)
    rowp = (rowp[:-1] if plant == "brow" else rowp[1:]).astype(R)[:, None]
    u, v = y[..., 0].astype(R), y[..., 1].astype(R)
    uW, uE = np.roll(u, 1, axis=1), np.roll(u, -1, axis=1)
    if plant == "seam":
        uW[:, 0] = u[:, -2]
    uS, uN = np.roll(u, 1, axis=0), np.roll(u, -1, axis=0)
    gE, gW = uE - u, u - uW
    d2y = fma(R(-2.0), u, uN) + uS
    if P.diffusion_only:
        du, dv = fma(cWn, gW, fma(cE, gE, cP * d2y)), np.zeros_like(v)
    elif op.model == co.FHN:
        du = fma(u, fma(-u, u, R(3.0)), fma(cWn, gW, fma(cE, gE, fma(cP, d2y, -v))))
        dv = fma(R(eps), u, rowp)
    else:
        z2 = u * u
        z4, y2 = z2 * z2, v * v
        dA = R(1.0) + z2
        dB = fma(R(1.0 / 500.0), y2, R(4.0 / 500.0)) * fma(z2, z2, R(0.9 ** 4))
        w = fma(R(65.0), z2 * dB, -((y2 * z4) * dA)) * _reciprocal(dA * dB)
        dv = fma(R(-1.0), v, w)
        du = fma(cWn, gW, fma(cE, gE, fma(cP, d2y, fma(R(-10.0), u, rowp - dv))))
    zero = P.zero_rows(t, u.shape[0], j0)
    if plant == "row_n":
        zero[-1] = False
    du[zero] = 0.0
    dv[zero] = 0.0
    return np.stack([du, dv], axis=-1)


def kernel_order_step(op, t, dt, y, R):
    """One RK4 step as the staged kernels take it (crd_kernels.hip): running accumulators, one fused multiply-add per stage input."""
    fma = _fma(R)
    h1, h2, h3, h6 = R(dt), R(0.5 * dt), R(dt / 3.0), R(dt / 6.0)
    y0 = y.astype(R)
    k = kernel_order_rhs(op, t, y0, R)
    acc = fma(h6, k, y0)
    k = kernel_order_rhs(op, t + 0.5 * dt, fma(h2, k, y0), R)
    acc = fma(h3, k, acc)
    k = kernel_order_rhs(op, t + 0.5 * dt, fma(h2, k, y0), R)
    acc = fma(h3, k, acc)
    k = kernel_order_rhs(op, t + dt, fma(h1, k, y0), R)
    return fma(h6, k, acc)


def _float32_problem(op):
    P = eb._Problem(op)
    # the whole grid's geometry formed in float32 from the problem's surface sizes (torus: 2 pi r = W; flat: xmax = W)
    if P.surface == "torus":
        g = cn.geometry("torus", 2 * cn.PI * op.R, 2 * cn.PI * op.r, op.nx, op.ny, dtype=np.float32)
    else:
        g = cn.geometry("flat", op.ymax, op.xmax, op.nx, op.ny, dtype=np.float32)
    return P, g


def reference_order_rhs(op, t, y):
    """The reference's own order (crd_oracle_np in float32)."""
    P, g = _float32_problem(op)
    du, dv = cn.rhs(P.model, P.surface, g, op.diff, t, y[..., 0], y[..., 1], dtype=np.float32, **P.kw)
    return np.stack([du, dv], axis=-1)


def reference_order_step(op, t, dt, y):
    P, g = _float32_problem(op)
    u, v = cn.rk4(P.model, P.surface, g, op.diff, y[..., 0], y[..., 1], t, dt, 1, dtype=np.float32, **P.kw)
    return np.stack([u, v], axis=-1)


def worst_ratio(w):
    return max(w["u"][0], w["v"][0])


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_fp64_reference_is_wider_than_fp64():
    assert np.finfo(np.longdouble).nmant >= 63  # error_bounds.reference_dtype refuses (does not skip) a narrower long double
    assert eb.reference_dtype("f64") is np.longdouble and eb.reference_dtype("f32") is np.float64


def test_precision_generic_oracle_keeps_fp64_and_widens_only_the_arithmetic():
    op = problem(CASES[0], 96)
    y = state(op)
    g = cn.geometry("torus", L, W, 96, 96)
    kw = dict(beta=1.25, vary_beta=1, beta_min=0.3, beta_max=1.4)
    a = cn.rhs("fhn", "torus", g, D, 0.0, y[..., 0], y[..., 1], **kw)
    b = cn.rhs("fhn", "torus", g, D, 0.0, y[..., 0], y[..., 1], dtype=np.float64, **kw)
    assert all(np.array_equal(x, z) and x.dtype == np.float64 for x, z in zip(a, b))
    wide = cn.rhs("fhn", "torus", cn.geometry("torus", L, W, 96, 96, dtype=np.longdouble), D, 0.0, y[..., 0], y[..., 1], dtype=np.longdouble, **kw)
    assert wide[0].dtype == np.longdouble
    assert 0.0 < float(np.max(np.abs(wide[0] - a[0]))) <= 1e-12 * float(np.max(np.abs(a[0])))
    assert cn.geometry("torus", L, W, 96, 96, dtype=np.float32)["dx"].dtype == np.float32


# ---- honest and sharp ----------------------------------------------------------------------------------------------------------
# The reference's own order is checked on the torus only.  Its flat operator, cu1 (uW + uE) + cu2 (uS + uN) + cu3 u
# (src/FHNmodel_flat.cpp:489-500), sums theta neighbour VALUES against cu3 u: its roundings scale with cu1 |u|, not with the
# theta differences the kernels' first-difference form is charged against, and it lands up to ~4x outside this bound on the host
# (fp32 and fp64 alike).  That is the reference's looser arithmetic, not a term the kernels' bound is missing.
def reference_order_applies(op):
    return op.surface == co.TORUS


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fp32_restatements_stay_inside_the_bound(case, n):
    for t_boundary, t in ((0.0, 0.0), (0.5, 0.25)):
        op = problem(case, n, t_boundary)
        y = state(op, n).astype(np.float32)
        bounded = eb.rhs_bound(op, t, y, "f32")
        eb.check("kernel order %s %d t=%g" % (case[0], n, t), kernel_order_rhs(op, t, y, np.float32), bounded)
        if reference_order_applies(op):
            eb.check("reference order %s %d t=%g" % (case[0], n, t), reference_order_rhs(op, t, y), bounded)
        dt = 0.02
        for tb in (0.0, 0.25, 2.0):  # absorbing rows off, switching off after the first stage, on for all four stages
            op.t_boundary = t + tb * dt
            bounded = eb.rk4_step_bound(op, t, dt, y, "f32")
            eb.check("kernel-order step %s %d tB=%g" % (case[0], n, tb), kernel_order_step(op, t, dt, y, np.float32), bounded)
            if reference_order_applies(op):
                eb.check("reference-order step %s %d tB=%g" % (case[0], n, tb), reference_order_step(op, t, dt, y), bounded)


@pytest.mark.parametrize("case", CASES[:3], ids=[c[0] for c in CASES[:3]])
def test_fp32_kernel_order_is_near_the_bound_at_2048(case):
    """Sharp: at 2048^2 the kernel-order restatement reaches >= 0.1 of the RHS bound and >= 0.02 of the one-step bound."""
    op = problem(case, 2048)
    y = state(op).astype(np.float32)
    w = eb.check("kernel order %s 2048" % case[0], kernel_order_rhs(op, 0.0, y, np.float32), eb.rhs_bound(op, 0.0, y, "f32"))
    wr = eb.check("reference order %s 2048" % case[0], reference_order_rhs(op, 0.0, y), eb.rhs_bound(op, 0.0, y, "f32")) if reference_order_applies(op) else None
    dt = 0.8 * 0.25 / (4 * D / (op.dx * op.dx))
    ws = eb.check("kernel-order step %s 2048" % case[0], kernel_order_step(op, 0.0, dt, y, np.float32), eb.rk4_step_bound(op, 0.0, dt, y, "f32"))
    print(eb.describe("RHS kernel order " + case[0], w), "|", wr and eb.describe("reference order", wr), "|", eb.describe("step", ws))
    assert worst_ratio(w) >= 0.1, eb.describe(case[0], w)
    assert worst_ratio(ws) >= 0.02, eb.describe(case[0], ws)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fp64_oracle_stays_inside_the_fp64_bound(case):
    """The C oracle (plain fp64 in the reference's order; torus) and the fp64 kernel-order restatement against the long-double
    reference, RHS and one step."""
    for t_boundary, t in ((0.0, 0.0), (0.5, 0.25)):
        op = problem(case, 192, t_boundary)
        y = state(op, 7)
        eb.check("fp64 kernel order %s t=%g" % (case[0], t), kernel_order_rhs(op, t, y, np.float64), eb.rhs_bound(op, t, y, "f64"))
        if not reference_order_applies(op):
            continue
        eb.check("C oracle %s t=%g" % (case[0], t), co.rhs(op, t, y), eb.rhs_bound(op, t, y, "f64"))
        for tb in (0.0, 0.25):
            op.t_boundary = t + tb * 0.01
            eb.check("C oracle step %s tB=%g" % (case[0], tb), co.rk4(op, y, t, 0.01, 1), eb.rk4_step_bound(op, t, 0.01, y, "f64"))


def test_band_of_rows_is_the_whole_grids_band():
    """rhs_bound / rk4_step_bound on a cropped band starting at global row j0 (phi seam included) give the whole grid's values
    away from the band's edges: the beta ramp and the absorbing rows follow global rows."""
    op = problem(CASES[0], 128, t_boundary=1.0)
    y = state(op)
    whole = eb.rhs_bound(op, 0.5, y, "f32")
    step = eb.rk4_step_bound(op, 0.5, 0.01, y, "f32")
    for j0 in (-6, 40, 120):
        rows = np.arange(j0, j0 + 16) % 128
        band = eb.rhs_bound(op, 0.5, y[rows], "f32", j0=j0 % 128)
        for a, b in zip(band, whole):
            assert np.array_equal(a[1:-1], b[rows[1:-1]])
        band = eb.rk4_step_bound(op, 0.5, 0.01, y[rows], "f32", j0=j0 % 128)
        for a, b in zip(band, step):
            assert np.allclose(a[4:-4], b[rows[4:-4]], rtol=1e-12, atol=0)


# ---- powerful ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fhn_2048():
    op = problem(CASES[0], 2048)
    y = state(op).astype(np.float32)
    return op, y, eb.rhs_bound(op, 0.0, y, "f32"), co.rhs(op, 0.0, y.astype(np.float64))


@pytest.mark.parametrize("plant,where", [("seam", (None, 0)), ("brow", (0, None))])
def test_planted_fp32_mistakes_pass_the_joint_gate_and_fail_the_bound(fhn_2048, plant, where):
    op, y, bounded, want = fhn_2048
    got = kernel_order_rhs(op, 0.0, y, np.float32, plant=plant)
    e = rel_err(got, want)
    w = eb.worst(got, *bounded)
    print("%s: rel_err %.3g (gate 2e-4), %s" % (plant, e, eb.describe(plant, w)))
    assert e <= 2e-4, (plant, e)  # today's gate (tests/test_gpu_parity.py: TOL_F32) lets it through ...
    field = "u" if plant == "seam" else "v"
    ratio, row, col = w[field]
    assert ratio > 100, eb.describe(plant, w)  # ... the per-point bound does not, and names the point
    assert (where[0] is None or row == where[0]) and (where[1] is None or col == where[1]), eb.describe(plant, w)
    with pytest.raises(AssertionError, match=r"worst err/bound .* at \(row \d+, col \d+\)"):
        eb.check("planted " + plant, got, bounded)


def test_planted_fp32_epsilon_in_an_fp64_kernel_fails_the_bound():
    op = problem(CASES[0], 2048)
    y = state(op)
    got = kernel_order_rhs(op, 0.0, y, np.float64, eps=float(np.float32(cn.EPSILON)))
    w = eb.worst(got, *eb.rhs_bound(op, 0.0, y, "f64"))
    e = rel_err(got, co.rhs(op, 0.0, y))
    print("EPSILON as float: rel_err %.3g (gate 1e-12), %s" % (e, eb.describe("eps", w)))
    assert w["v"][0] > 1e6 and w["u"][0] <= 1.0, eb.describe("eps", w)


def test_planted_missing_absorbing_zero_fails_the_bound():
    op = problem(CASES[0], 256, t_boundary=1.0)
    y = state(op).astype(np.float32)
    bounded = eb.rhs_bound(op, 0.5, y, "f32")
    eb.check("absorbing rows", kernel_order_rhs(op, 0.5, y, np.float32), bounded)
    w = eb.worst(kernel_order_rhs(op, 0.5, y, np.float32, plant="row_n"), *bounded)
    assert w["u"][0] == np.inf and w["u"][1] == 255 and w["v"][0] == np.inf, eb.describe("row ny-1", w)


def test_reciprocal_error_is_its_own_term():
    """Goldbeter's bound carries rho |w| beside K u S: without it, a reciprocal of 2^-24 relative error (the bare estimate, no
    Newton step) would hide inside fp64's K u S wherever the Hill terms are large; with it, the bare estimate fails."""
    op = problem(CASES[2], 128)
    y = state(op)
    ref, bu, bv = eb.rhs_bound(op, 0.0, y, "f64")
    u, v = y[..., 0], y[..., 1]
    z2, y2 = u * u, v * v
    w = 65.0 * z2 / (1 + z2) - 500.0 * y2 * z2 * z2 / ((4 + y2) * (0.9 ** 4 + z2 * z2))
    assert np.all(bv >= eb.RHO["f64"] * np.abs(w))
    bare = ref.astype(np.float64).copy()
    bare[..., 1] += 2.0 ** -24.4 * np.abs(w)  # the estimate's own error, as the reciprocal without its Newton step would leave it
    assert eb.worst(bare, ref, bu, bv)["v"][0] > 1.0
