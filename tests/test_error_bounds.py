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


# ---- one error-controlled attempt (Zonneveld 5(3)4): restatements, honest, powerful ----------------------------------------------
ATTEMPT_CONFIGS = [
    ("fhn-torus", co.FHN, co.TORUS, 1.25, {}),
    ("fhn-torus-varybeta", co.FHN, co.TORUS, 1.25, dict(vary_beta=1, beta_min=0.3, beta_max=1.4)),
    ("fhn-flat", co.FHN, co.FLAT, 1.25, {}),
    ("goldbeter-torus", co.GOLDBETER, co.TORUS, 0.4, {}),
    ("goldbeter-flat-varybeta", co.GOLDBETER, co.FLAT, 0.4, dict(vary_beta=1, beta_min=0.0, beta_max=1.0)),
    ("diffusion-only", co.GOLDBETER, co.TORUS, 0.4, dict(just_diffusion=1)),
]  # the six configurations of the device gate (tests/test_gpu_error_bounds.py: CONFIGS), in its order
ATTEMPT_VALID = 54  # columns a wavefront of the attempt kernel stores (64 lanes, an apron of 5 a side)
MODELS = {co.FHN: "fhn", co.GOLDBETER: "goldbeter"}
SURFACES = {co.TORUS: "torus", co.FLAT: "flat"}
# The step of the attempt gates, host and device alike, as a fraction of crd.stable_dt.
ATTEMPT_STEP = 0.9
ATTEMPT_DSM = 0.1  # the norm the tolerances are scaled to: accepted with room to spare, far above the estimate's rounding floor


def attempt_problem(case, nx, ny, t_boundary=0.0, **over):
    _, model, surface, beta, kw = case
    kw = dict(kw, **over)
    return co.make_problem(model, surface, nx, L, W, kw.pop("diff", D), kw.pop("beta", beta), ny=ny, t_boundary=t_boundary, **kw)


def attempt_step(op):
    """ATTEMPT_STEP x crd.stable_dt.  A diffusion-only run takes the bound of its diffusion alone: crd.stable_dt adds Goldbeter's
    reaction rate, which the run does not have, and on a coarse grid that leaves h |lambda| of the diffusion so small that the
    estimate, a fifth-order quantity, is below fp32's rounding.  1 / stable_dt is linear in D plus that constant, so two calls
    isolate the diffusion's part."""
    import crdmodel_amd as crd

    s = lambda diff: crd.stable_dt(crd.make_params(MODELS[op.model], SURFACES[op.surface], op.nx, L, W, diff, 1.0, ny=op.ny))  # noqa: E731
    if op.just_diffusion:
        return ATTEMPT_STEP / (1.0 / s(2 * op.diff) - 1.0 / s(op.diff))
    return ATTEMPT_STEP * s(op.diff)


def attempt_state(op, seed, R=np.float64):
    """state() with grid-scale noise of 0.2 instead of 1e-5: the embedded estimate is a high-order quantity, next to nothing on a
    smooth field; the noise gives every point an estimate of the same order, far above the fp32 floor of 22/3 u |y0|
    (error_bounds: K_Y), so that a single column or row carries its share of the norm wherever it lies.  Rounded to R."""
    y = state(op, seed)
    y += 0.2 * np.random.default_rng(seed + 1000).standard_normal(y.shape)
    if op.model == co.GOLDBETER:
        y = np.abs(y)
    return y.astype(R)


def attempt_bound(op, t, h, y, precision, bound=eb.erk_attempt_bound):
    """(tol, erk_attempt_bound) with rtol = atol = tol scaled on the REFERENCE so that its norm is ATTEMPT_DSM (the norm is
    proportional to 1 / tol when both scale together), asserted to lie in [1e-3, 0.5].  bound: eb.rk43_attempt_bound for the RK4(3) pair."""
    first = bound(op, t, h, y, precision, 1e-4, 1e-4)
    assert np.isfinite(first.dsm) and first.dsm > 0.0, first.dsm
    tol = float(np.float32(1e-4 * first.dsm / ATTEMPT_DSM))  # (a float32 value: the same number in both kernels' precisions ... and in print)
    ab = bound(op, t, h, y, precision, tol, tol)
    assert 1e-3 <= ab.dsm <= 0.5, (tol, ab.dsm)
    return tol, ab


def kernel_order_attempt(op, t, h, y, R, rtol, atol, chunk=4, mutant=None, at=None):
    """fused_item<..., EMBED = 2, ...> in precision R, in its order (crd_fused_impl.h): stage values by one fused multiply-add,
    d_i = y_i - y0, y_new, z5 and e4 out of them at the row's stage 4, k5 at t + 3/4 h, err = fma(fl(16/3) h, k5, e4), the weights
    by one fused multiply-add, a lane's sum of squares in R over its chunk's rows (both fields), everything after that in double.
    Returns (y_new, err, dsm).  mutant (at: its column or row):
      "stale"   stage 5 of column `at` (a strip's last) reads its east neighbour from y0 instead of z5
      "twice"   column `at` (>= nx - 1: nx - 1 itself) is counted twice
      "row"     row `at` (a chunk's first) is not counted
      "time"    stage 5's absorbing flag is decided at t + h
      "five"    16/3 is 5"""
    fma = _fma(R)
    f = lambda ts, z: kernel_order_rhs(op, ts, z, R)  # noqa: E731
    h1, h2, h6 = R(h), R(0.5 * h), R(h / 6.0)
    y0 = y.astype(R)
    k1 = f(t, y0)
    y1 = fma(h2, k1, y0)
    k2 = f(t + 0.5 * h, y1)
    y2 = fma(h2, k2, y0)
    k3 = f(t + 0.5 * h, y2)
    y3 = fma(h1, k3, y0)
    k4 = f(t + h, y3)
    d1, d2, d3 = y1 - y0, y2 - y0, y3 - y0
    ynew = fma(R(1.0 / 3.0), fma(R(2.0), d2, d1 + d3), fma(h6, k4, y0))
    h32, h2m = R(-1.0 / 32.0) * h1, R(-2.0) * h1
    z5 = fma(R(5.0 / 16.0), d1, fma(R(7.0 / 16.0), d2, fma(R(13.0 / 32.0), d3, fma(h32, k4, y0))))
    e4 = fma(R(4.0 / 3.0), d1, fma(R(-4.0), d2, fma(R(-2.0), d3, h2m * k4)))
    k5 = f(t + (1.0 if mutant == "time" else 0.75) * h, z5)
    if mutant == "stale":
        zs = z5.copy()
        zs[:, (at + 1) % op.nx] = y0[:, (at + 1) % op.nx]
        k5[:, at] = f(t + 0.75 * h, zs)[:, at]
    h163 = R(5.0 if mutant == "five" else 16.0 / 3.0) * h1
    err = fma(h163, k5, e4)
    e = err / fma(R(rtol), np.abs(y0), R(atol))
    rows, nx = y0.shape[:2]
    total = 0.0
    for j0 in range(0, rows, chunk):
        acc = np.zeros(nx, dtype=R)
        for j in range(j0, min(j0 + chunk, rows)):
            if mutant == "row" and j == at:
                continue
            acc = fma(e[j, :, 0], e[j, :, 0], fma(e[j, :, 1], e[j, :, 1], acc))
        total += float(np.sum(acc.astype(np.float64)))
        if mutant == "twice":
            total += float(acc[at])
    return ynew, err, float(np.sqrt(total / (2 * rows * nx)))


def reference_order_attempt(op, t, h, y, rtol, atol):
    """oracle/arkode_erk.erk_attempt (the reference's order: stage increments, then h sum (b - b^) k) around the float32
    restatement of the reference's f, and ARKode's WRMS norm, all in float32."""
    from oracle import arkode_erk as ark

    P, g = _float32_problem(op)
    f = lambda ts, z: np.stack(cn.rhs(P.model, P.surface, g, op.diff, ts, z[..., 0], z[..., 1], dtype=np.float32, **P.kw), axis=-1)  # noqa: E731
    tab = {k: ([[np.float32(a) for a in r] for r in v] if k == "A" else v) for k, v in ark.ZONNEVELD_5_3_4.items()}
    h32 = np.float32(h)
    k = []
    for i in range(5):
        z = y
        if i > 0:
            inc = sum(tab["A"][i][j] * k[j] for j in range(i) if tab["A"][i][j] != 0)
            z = y + h32 * inc
        k.append(f(t + tab["c"][i] * h, z))
    f32 = np.float32
    ynew = y + (h32 / f32(6)) * (k[0] + f32(2) * k[1] + f32(2) * k[2] + k[3])
    err = h32 * (f32(2.0 / 3.0) * k[0] - f32(2) * (k[1] + k[2] + k[3]) + f32(16.0 / 3.0) * k[4])
    e = err / (f32(rtol) * np.abs(y) + f32(atol))
    return ynew, err, float(np.sqrt(np.sum(e * e, dtype=np.float32) / f32(e.size)))


ATTEMPT_GRIDS = [(55, 33), (109, 41)]  # strip edges of the attempt kernel (54 columns), a last chunk of one row


def attempt_placements(h):
    """(label, tBoundary - t): absorbing rows off; stage 4 (t + h) free and stage 5 (t + 3/4 h) absorbing; on for all five."""
    return [("off", 0.0), ("between 3/4 h and h", 0.8 * h), ("on", 2.0 * h)]


@pytest.mark.parametrize("case", ATTEMPT_CONFIGS, ids=[c[0] for c in ATTEMPT_CONFIGS])
def test_attempt_restatements_stay_inside_the_state_estimate_and_norm_bounds(case):
    """Honest: the attempt in the kernel's order (fp32 and fp64) and in the reference's (fp32, torus) against erk_attempt_bound --
    y_new and the estimate per point, the WRMS norm as a scalar.  Worst ratios over these cases, as printed (DESIGN.md,
    "Tolerances"): kernel order state 0.29, estimate 0.63 (Goldbeter; FHN 0.46), norm 0.005; reference order 0.17, 0.12, 0.004.
    K_ERR = 8 is the count's: Goldbeter needs no empirical constant of its own beyond the K its stage errors already carry.  (On
    1000 x 65 FHN's v reaches 0.94 of the estimate's bound in the kernel's order: there h k_v is below an ulp of v, every stage value
    rounds back to v itself, and the K_Y u |y0| term is what is left -- the bound is sharp, not slack.)"""
    t = 0.3
    worst = {}
    for nx, ny in ATTEMPT_GRIDS:
        h = attempt_step(attempt_problem(case, nx, ny))
        for label, tb in attempt_placements(h):
            op = attempt_problem(case, nx, ny, t_boundary=t + tb if tb else 0.0)
            for precision, R in (("f64", np.float64), ("f32", np.float32)):
                y = attempt_state(op, nx + ny, R)
                tol, ab = attempt_bound(op, t, h, y, precision)
                runs = [("kernel", kernel_order_attempt(op, t, h, y, R, tol, tol))]
                if precision == "f32" and reference_order_applies(op):
                    runs.append(("reference", reference_order_attempt(op, t, h, y, tol, tol)))
                for order, (ynew, err, dsm) in runs:
                    name = "%s order %s %s %dx%d tB %s" % (order, precision, case[0], nx, ny, label)
                    ws = eb.check(name + " state", ynew, ab.state)
                    we = eb.check(name + " estimate", err, (ab.err, ab.err_bound_u, ab.err_bound_v))
                    rn = abs(dsm - ab.dsm) / ab.dsm_bound
                    assert rn <= 1.0, (name, dsm, ab.dsm, ab.dsm_bound)
                    key = (order, precision)
                    worst[key] = tuple(max(a, b) for a, b in zip(worst.get(key, (0, 0, 0)), (worst_ratio(ws), worst_ratio(we), rn)))
    for key, w in sorted(worst.items()):
        print("BOUND attempt %s order %s %s: worst err/bound state %.3g, estimate %.3g, norm %.3g" % (key + (case[0],) + w))


MUTANT_GRIDS = [(217, 41), (1000, 65)]  # four strips and a ragged fifth; the largest grid of the device gate


@pytest.fixture(scope="module", params=[(g, p) for g in MUTANT_GRIDS for p in ("f64", "f32")], ids=lambda q: "%dx%d-%s" % (q[0] + (q[1],)))
def mutant_case(request):
    (nx, ny), precision = request.param
    R = np.float64 if precision == "f64" else np.float32
    h = attempt_step(attempt_problem(ATTEMPT_CONFIGS[0], nx, ny))
    t = 0.3
    out = {}
    # absorbing rows off, and for "time" tBoundary between stage 5's time and stage 4's (there the two boundary rows, whose estimate
    # is then the first-order -2 h k4, carry most of the norm, and an ordinary row's share is next to nothing)
    for key, tb in (("off", 0.0), ("time", t + 0.8 * h)):
        op = attempt_problem(ATTEMPT_CONFIGS[0], nx, ny, t_boundary=tb)
        y = attempt_state(op, 11, R)
        tol, ab = attempt_bound(op, t, h, y, precision)
        _, _, dsm = kernel_order_attempt(op, t, h, y, R, tol, tol)
        assert abs(dsm - ab.dsm) <= ab.dsm_bound
        out[key] = (op, t, h, y, R, tol, ab, precision)
    return out


@pytest.mark.parametrize("mutant", ["stale", "twice", "row", "time", "five"])
def test_attempt_mutants_exceed_the_norm_bound(mutant_case, mutant):
    """Powerful: five mistakes that leave y_new exact and move only the scalar err_last fail the norm bound -- stage 5 reading a
    stale east neighbour at a strip's last column, column nx - 1 counted twice, a chunk's first row not counted, stage 5's
    absorbing flag decided at t + h, 16/3 replaced by 5 -- on FHN, torus, at the tolerances of the device gate.

    Reach.  fp64: every mutant exceeds the bound by a factor above 1e9 on every grid.  fp32: the bound has a floor, the stage
    values' own rounding carried into the estimate (error_bounds: K_Y u |y0| per point), and a single column's or row's share of
    the norm, about 1 / (2 nx) or 1 / (2 ny) of it, has to stand above that.  At 1000 x 65 (N = 130000 values, the largest grid of
    the device gate) the margins of mutants 1-3 are 13 (stale), 3.2 (twice), 41 (row); a column's share falls with 1 / nx against
    a constant floor, so "twice" reaches to about nx = 3000 on this state, N = 400000: the device gate stays below that.  The
    reach has a lower end too: on narrow grids the step is bound by the reaction rate, h |lambda| of the diffusion is small and
    the estimate, a fifth-order quantity, lies nearer the floor -- at 55 x 33 in fp32 "twice" and "row" come to 0.4 and 0.2 of the
    bound and are not seen there (stale 364, time 2500, five 1600 are), which is why the mutants run from 217 columns on."""
    op, t, h, y, R, tol, ab, precision = mutant_case["time" if mutant == "time" else "off"]
    at = {"stale": min(ATTEMPT_VALID, op.nx) - 1, "twice": op.nx - 1, "row": 4 * (op.ny // 8)}.get(mutant)
    ynew, _, dsm = kernel_order_attempt(op, t, h, y, R, tol, tol, mutant=mutant, at=at)
    eb.check("mutant %s state" % mutant, ynew, ab.state)  # the solution cannot show it
    ratio = abs(dsm - ab.dsm) / ab.dsm_bound
    print("BOUND mutant %s %s %dx%d: |dsm - dsm_ref| / bound %.3g" % (mutant, precision, op.nx, op.ny, ratio))
    assert ratio > 2.0, ratio


def test_attempt_bound_on_a_band_is_the_whole_grids():
    """erk_attempt_bound's per-point parts on a cropped band starting at global row j0, away from the band's edges."""
    op = attempt_problem(ATTEMPT_CONFIGS[1], 64, 48, t_boundary=1.0)
    y = attempt_state(op, 2)
    whole = eb.erk_attempt_bound(op, 0.99, 0.02, y, "f32", 1e-3, 1e-3)
    for j0 in (-7, 20):
        rows = np.arange(j0, j0 + 20) % 48
        band = eb.erk_attempt_bound(op, 0.99, 0.02, y[rows], "f32", 1e-3, 1e-3, j0=j0 % 48)
        for a, b in zip(band.state + (band.err, band.err_bound_u, band.err_bound_v), whole.state + (whole.err, whole.err_bound_u, whole.err_bound_v)):
            assert np.allclose(a[5:-5].astype(np.float64), b[rows[5:-5]].astype(np.float64), rtol=1e-9, atol=0)


# ---- one RK4(3) attempt (CRD_ADAPT_RK43, EMBED = 1): restatements, honest, powerful ------------------------------------------------
def kernel_order_rk43_attempt(op, t, h, y, R, rtol, atol, chunk=4, mutant=None, at=None):
    """fused_item<..., EMBED = 1, ...> in precision R, in its order (crd_fused_impl.h): the staged running accumulators of
    kernel_order_step, k5 = f(t + h, y_new) with stage 4's absorbing flag, e = h6 * (k4 - k5) / fma(rtol, |y0|, atol), a lane's sum of
    squares in R over its chunk's rows (both fields), everything after that in double.  Returns (y_new, err, dsm); err is the
    estimate before the weight, h6 * (k4 - k5).  mutant (at: its column or row):
      "stale"   stage 5 of column `at` (a strip's last) reads its east neighbour from y3 instead of y_new
      "twice"   column `at` (nx - 1) is counted twice
      "row"     row `at` (a chunk's first) is not counted
      "time"    stage 5's absorbing flag is decided at t + 3/4 h
      "third"   h / 3 in place of h / 6"""
    fma = _fma(R)
    f = lambda ts, z: kernel_order_rhs(op, ts, z, R)  # noqa: E731
    h1, h2, h3, h6 = R(h), R(0.5 * h), R(h / 3.0), R(h / 6.0)
    y0 = y.astype(R)
    k = f(t, y0)
    acc = fma(h6, k, y0)
    k = f(t + 0.5 * h, fma(h2, k, y0))
    acc = fma(h3, k, acc)
    k = f(t + 0.5 * h, fma(h2, k, y0))
    acc = fma(h3, k, acc)
    y3 = fma(h1, k, y0)
    k4 = f(t + h, y3)
    ynew = fma(h6, k4, acc)
    k5 = f(t + (0.75 if mutant == "time" else 1.0) * h, ynew)
    if mutant == "stale":
        zs = ynew.copy()
        zs[:, (at + 1) % op.nx] = y3[:, (at + 1) % op.nx]
        k5[:, at] = f(t + h, zs)[:, at]
    err = (R(h / 3.0) if mutant == "third" else h6) * (k4 - k5)
    e = err / fma(R(rtol), np.abs(y0), R(atol))
    rows, nx = y0.shape[:2]
    total = 0.0
    for j0 in range(0, rows, chunk):
        acc = np.zeros(nx, dtype=R)
        for j in range(j0, min(j0 + chunk, rows)):
            if mutant == "row" and j == at:
                continue
            acc = fma(e[j, :, 0], e[j, :, 0], fma(e[j, :, 1], e[j, :, 1], acc))
        total += float(np.sum(acc.astype(np.float64)))
        if mutant == "twice":
            total += float(acc[at])
    return ynew, err, float(np.sqrt(total / (2 * rows * nx)))


def reference_order_rk43_attempt(op, t, h, y, rtol, atol):
    """The pair in the reference's order around the float32 restatement of the reference's f: the oracle's stage inputs
    y + (c h) k, y + h/6 (k1 + 2 k2 + 2 k3 + k4), err = h/6 (k4 - k5), the WRMS norm, all in float32."""
    P, g = _float32_problem(op)
    f = lambda ts, z: np.stack(cn.rhs(P.model, P.surface, g, op.diff, ts, z[..., 0], z[..., 1], dtype=np.float32, **P.kw), axis=-1)  # noqa: E731
    f32 = np.float32
    h32 = f32(h)
    k1 = f(t, y)
    k2 = f(t + 0.5 * h, y + (f32(0.5) * h32) * k1)
    k3 = f(t + 0.5 * h, y + (f32(0.5) * h32) * k2)
    k4 = f(t + h, y + h32 * k3)
    ynew = y + (h32 / f32(6)) * (k1 + f32(2) * k2 + f32(2) * k3 + k4)
    err = (h32 / f32(6)) * (k4 - f(t + h, ynew))
    e = err / (f32(rtol) * np.abs(y) + f32(atol))
    return ynew, err, float(np.sqrt(np.sum(e * e, dtype=np.float32) / f32(e.size)))


def rk43_bound(op, t, h, y, precision):
    return attempt_bound(op, t, h, y, precision, eb.rk43_attempt_bound)


@pytest.mark.parametrize("case", ATTEMPT_CONFIGS, ids=[c[0] for c in ATTEMPT_CONFIGS])
def test_rk43_restatements_stay_inside_the_state_estimate_and_norm_bounds(case):
    """Honest: the RK4(3) attempt in the kernel's order (fp32 and fp64) and in the reference's (fp32, torus) against
    rk43_attempt_bound -- y_new and the estimate per point, the WRMS norm as a scalar -- with tBoundary off, between t + 3/4 h and
    t + h (stages 4 and 5 free, a fifth flag taken at t + 3/4 h would absorb) and on for all five stages.  Worst ratios over these
    cases, as printed ("Tolerances"): kernel order state 0.39, estimate 0.14 (Goldbeter; FHN 0.07), norm 0.029 (diffusion
    only in fp64; every other case 0.007 at most); reference order 0.17, 0.14, 0.025.  K_EST43 = 3 is the count's and has nothing spare;
    the estimate's ratios are small because h/6 (e4 + e5), the stages' worst case, is most of its bound."""
    t = 0.3
    worst = {}
    for nx, ny in ATTEMPT_GRIDS:
        h = attempt_step(attempt_problem(case, nx, ny))
        for label, tb in attempt_placements(h):
            op = attempt_problem(case, nx, ny, t_boundary=t + tb if tb else 0.0)
            for precision, R in (("f64", np.float64), ("f32", np.float32)):
                y = attempt_state(op, nx + ny, R)
                tol, ab = rk43_bound(op, t, h, y, precision)
                runs = [("kernel", kernel_order_rk43_attempt(op, t, h, y, R, tol, tol))]
                if precision == "f32" and reference_order_applies(op):
                    runs.append(("reference", reference_order_rk43_attempt(op, t, h, y, tol, tol)))
                for order, (ynew, err, dsm) in runs:
                    name = "RK4(3) %s order %s %s %dx%d tB %s" % (order, precision, case[0], nx, ny, label)
                    ws = eb.check(name + " state", ynew, ab.state)
                    we = eb.check(name + " estimate", err, (ab.err, ab.err_bound_u, ab.err_bound_v))
                    rn = abs(dsm - ab.dsm) / ab.dsm_bound
                    assert rn <= 1.0, (name, dsm, ab.dsm, ab.dsm_bound)
                    key = (order, precision)
                    worst[key] = tuple(max(a, b) for a, b in zip(worst.get(key, (0, 0, 0)), (worst_ratio(ws), worst_ratio(we), rn)))
    for key, w in sorted(worst.items()):
        print("BOUND RK4(3) attempt %s order %s %s: worst err/bound state %.3g, estimate %.3g, norm %.3g" % (key + (case[0],) + w))


# the narrowest grid of the device gate, one strip edge, two, four strips and a ragged fifth, the largest grid of the gate
RK43_MUTANT_GRIDS = [(5, 59), (55, 33), (109, 41), (217, 41), (1000, 65)]
RK43_MUTANT_CONFIGS = [0, 3, 5]  # FHN, Goldbeter, diffusion only (torus)
RK43_MUTANTS = ["stale", "twice", "row", "time", "third"]


def rk43_mutant_claimed(mutant, precision, k, nx):
    """Where the norm bound is claimed to see a mutant (the docstring of test_rk43_mutants_exceed_the_norm_bound: "Reach")."""
    if mutant == "time" and ATTEMPT_CONFIGS[k][4].get("just_diffusion"):
        return False  # a diffusion-only run has no absorbing rows: the mistake does not exist there
    if precision == "f64":
        return True
    if mutant == "stale":
        return nx >= (217 if ATTEMPT_CONFIGS[k][1] == co.GOLDBETER and not ATTEMPT_CONFIGS[k][4].get("just_diffusion") else 53)
    if mutant == "row":
        return k != 3
    return True


_rk43_mutant_cases = {}


def rk43_mutant_case(nx, ny, precision, k, key):
    """The unmutated attempt of configuration k, shared by its mutants: key "off" (absorbing rows off) or "time" (tBoundary between
    t + 3/4 h and t + h)."""
    q = (nx, ny, precision, k, key)
    if q not in _rk43_mutant_cases:
        R = np.float64 if precision == "f64" else np.float32
        t = 0.3
        h = attempt_step(attempt_problem(ATTEMPT_CONFIGS[k], nx, ny))
        op = attempt_problem(ATTEMPT_CONFIGS[k], nx, ny, t_boundary=t + 0.8 * h if key == "time" else 0.0)
        y = attempt_state(op, 11, R)
        tol, ab = rk43_bound(op, t, h, y, precision)
        _, _, dsm = kernel_order_rk43_attempt(op, t, h, y, R, tol, tol)
        assert abs(dsm - ab.dsm) <= ab.dsm_bound
        _rk43_mutant_cases[q] = (op, t, h, y, R, tol, ab)
    return _rk43_mutant_cases[q]


@pytest.mark.parametrize("nx,ny,precision,k,mutant", [
    pytest.param(nx, ny, p, k, m, id="%dx%d-%s-%s-%s" % (nx, ny, p, ATTEMPT_CONFIGS[k][0], m))
    for nx, ny in RK43_MUTANT_GRIDS for p in ("f64", "f32") for k in RK43_MUTANT_CONFIGS for m in RK43_MUTANTS if rk43_mutant_claimed(m, p, k, nx)])
def test_rk43_mutants_exceed_the_norm_bound(nx, ny, precision, k, mutant):
    """Powerful: five mistakes in the EMBED = 1 path that leave y_new inside its bound and move only the scalar err_last exceed the
    norm bound by more than a factor 2 -- stage 5 reading a stale east neighbour (y3 for y_new) at a strip's last column, column
    nx - 1 counted twice, a chunk's first row not counted, stage 5's absorbing flag decided at t + 3/4 h with tBoundary between that
    and t + h, h / 3 for h / 6 -- on FHN, Goldbeter and diffusion only (torus), at the tolerances and the step (ATTEMPT_STEP x
    crd.stable_dt) of the device gate.

    Reach, measured with this step on 5 x 59, 53 x 26, 55 x 8, 55 x 33, 109 x 41, 163 x 47, 217 x 41, 271 x 38 and 1000 x 65.  The
    estimate is a third-order quantity and the bound 1.4e-5 ... 4.5e-4 of the norm in fp32, 1e-14 ... 4e-13 in fp64.
    fp64: every mutant, every configuration, every grid: factors from 1.3e3 (Goldbeter's row on 5 x 59) and otherwise above 1e6.
    fp32, "twice", "time", "third": every configuration and every grid -- FHN 11 (55 x 8) ... 39 (5 x 59) and 25 (1000 x 65) for
    "twice", above 160 for the other two; Goldbeter 887 ... 14.5 (271 x 38), 19 (1000 x 65); diffusion only 2.2 (5 x 59), 480
    (55 x 33) ... 33 (1000 x 65).  A column's share falls with 1 / nx against a bound that does not: "twice" ends near nx = 10 000.
    fp32, "stale": the stale value differs from the right one by the stage's own increment, and what stage 5 makes of it scales
    with the diffusion's h |lambda|, which a coarse grid does not have.  FHN and diffusion only: seen from 53 columns on (FHN 3.9
    at 55 x 33, 53 at 217 x 41, 8.7 at 1000 x 65; diffusion only 14 ... 259), not on 5 x 59 (0.1, 0.02).  Goldbeter, whose step the
    reaction rate binds: seen from 217 columns on (3.3, 3.1, 9.2 at 1000 x 65), not below (0.005 ... 1.0).  Up to 54 columns there
    is one strip and its last column's east neighbour is the periodic seam's.
    fp32, "row": FHN 22 (55 x 33) ... 458 and diffusion only 26 (5 x 59) ... 2000 on every grid.  NOT claimed for Goldbeter: on this
    state the five rows of the initial front carry the norm (8 to 10 times a row's fair share each; a row elsewhere 0.02 of it), and a
    single uncounted row comes to anything between 0.008 (5 x 59) and 283 (1000 x 65) of the bound according to where it lies.
    So the device gate's norm claim in fp32 is: double counting, the fifth flag's time and the factor at every width and configuration;
    a stale strip-edge neighbour from 55 columns (Goldbeter: 217); an uncounted row on the FHN and diffusion-only configurations,
    which run at every width beside Goldbeter's and share the row rule's code with them."""
    op, t, h, y, R, tol, ab = rk43_mutant_case(nx, ny, precision, k, "time" if mutant == "time" else "off")
    at = {"stale": min(ATTEMPT_VALID, op.nx) - 1, "twice": op.nx - 1, "row": 4 * (op.ny // 8)}.get(mutant)
    ynew, _, dsm = kernel_order_rk43_attempt(op, t, h, y, R, tol, tol, mutant=mutant, at=at)
    eb.check("RK4(3) mutant %s state" % mutant, ynew, ab.state)  # the solution cannot show it
    ratio = abs(dsm - ab.dsm) / ab.dsm_bound
    print("BOUND RK4(3) mutant %s %s %s %dx%d: |dsm - dsm_ref| / bound %.3g" % (mutant, precision, ATTEMPT_CONFIGS[k][0], op.nx, op.ny, ratio))
    assert ratio > 2.0, ratio


def test_rk43_attempt_bound_on_a_band_is_the_whole_grids():
    """rk43_attempt_bound's per-point parts on a cropped band starting at global row j0, away from the band's edges."""
    op = attempt_problem(ATTEMPT_CONFIGS[1], 64, 48, t_boundary=1.0)
    y = attempt_state(op, 2)
    whole = eb.rk43_attempt_bound(op, 0.99, 0.02, y, "f32", 1e-3, 1e-3)
    for j0 in (-7, 20):
        rows = np.arange(j0, j0 + 20) % 48
        band = eb.rk43_attempt_bound(op, 0.99, 0.02, y[rows], "f32", 1e-3, 1e-3, j0=j0 % 48)
        for a, b in zip(band.state + (band.err, band.err_bound_u, band.err_bound_v), whole.state + (whole.err, whole.err_bound_u, whole.err_bound_v)):
            assert np.allclose(a[5:-5].astype(np.float64), b[rows[5:-5]].astype(np.float64), rtol=1e-9, atol=0)
