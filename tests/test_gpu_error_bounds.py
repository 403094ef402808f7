"""Per-point gates of the tiled RHS kernel and the one-step RK4 kernels against a rounding-error bound (oracle/error_bounds.py).

The joint max-norm gate (conftest.rel_err) is dominated by the largest diffusion term on the grid; here every point and field
is held to |kernel - reference| <= K u S (+ the reciprocal's own term) for f(), and to the bound propagated through the four
stages for one step.  The two- and three-step kernels, slab cuts and the ring are tied bit for bit to the one-step kernel by
tests/test_gpu_parity.py, which carries these gates up to them.  Every failure names the case and the worst err/bound per field
with its (row, column).  The error-controlled attempts are gated per point and in norm in tests/test_gpu_attempt_bounds.py (Zonneveld
5(3)4) and tests/test_gpu_rk43_bounds.py (the RK4(3) pair).  theta-block contexts (SlabDesc::wrap_x == 0: ghost-column strips for the
row's wrap) are gated per point, f() and one staged step, in tests/test_gpu_theta_blocks.py, at block widths on both sides of one,
two and three 64-column tiles.
"""
import numpy as np
import pytest

import crdmodel_amd as crd
from conftest import crd_params, golden_names, load_golden, oracle_problem
from oracle import crd_oracle as co
from oracle import error_bounds as eb

pytestmark = pytest.mark.gpu

L, W, D = 80.0, 20.0, 0.12
WIDTHS = [5, 56, 57, 63, 64, 65, 104, 105, 120, 121, 232, 233, 1000]
DTYPE = {"f64": np.float64, "f32": np.float32}

# (label, model, surface, beta, keyword arguments of make_params / make_problem)
CONFIGS = [
    ("fhn-torus", "fhn", "torus", 1.25, {}),
    ("fhn-torus-varybeta", "fhn", "torus", 1.25, dict(vary_beta=1, beta_min=0.3, beta_max=1.4)),
    ("fhn-flat", "fhn", "flat", 1.25, {}),
    ("goldbeter-torus", "goldbeter", "torus", 0.4, {}),
    ("goldbeter-flat-varybeta", "goldbeter", "flat", 0.4, dict(vary_beta=1, beta_min=0.0, beta_max=1.0)),
    ("diffusion-only", "goldbeter", "torus", 0.4, dict(just_diffusion=1)),
]


def check(case, got, bounded, **kw):
    """eb.check, and the worst ratios printed (run with -s to collect them per kernel family)."""
    w = eb.check(case, got, bounded, **kw)
    print("BOUND " + eb.describe(case, w))
    return w


def problem(model, surface, nx, ny, beta, t_boundary=0.0, precision="f64", **kw):
    p = crd.make_params(model, surface, nx, L, W, D, beta, ny=ny, t_boundary=t_boundary, precision=precision, **kw)
    op = co.make_problem({"fhn": co.FHN, "goldbeter": co.GOLDBETER}[model], {"torus": co.TORUS, "flat": co.FLAT}[surface], nx, L, W, D,
                         beta, ny=ny, t_boundary=t_boundary, **kw)
    return p, op


def state(op, seed, precision):
    """The reference's front-style initial state (vary_beta off, so the front exists) with a smooth perturbation, a little noise,
    and for Goldbeter a patch of small z; rounded to the kernel's precision (the reference sees the same, widened)."""
    q = co.Problem.from_buffer_copy(op)
    q.vary_beta = 0
    y = co.initial_conditions(q, 0.1, 0.5, 0)
    ny, nx = y.shape[:2]
    th, ph = np.arange(nx) * op.dx, np.arange(ny) * op.dy
    y[..., 0] += 0.05 * np.sin(th)[None, :] * np.cos(ph)[:, None]
    y[..., 1] += 0.05 * np.cos(th)[None, :] * np.sin(2 * ph)[:, None]
    rng = np.random.default_rng(seed)
    y += 1e-4 * rng.standard_normal(y.shape)
    if op.model == co.GOLDBETER:
        r0, r1, c1 = ny // 2, ny // 2 + max(ny // 4, 1), max(nx // 3, 1)
        y[r0:r1, :c1, 0] = rng.uniform(1e-3, 0.2, (r1 - r0, c1))
    return y.astype(DTYPE[precision])


def ragged(nx):
    return 24 + (nx * 7) % 41


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx", WIDTHS)
def test_rhs_per_point_across_strip_widths(gpu_device, nx, precision):
    ny = ragged(nx)
    for k, (label, model, surface, beta, kw) in enumerate(CONFIGS):
        p, op = problem(model, surface, nx, ny, beta, t_boundary=0.5, precision=precision, **kw)
        y = state(op, nx * 10 + k, precision)
        with crd.Slab(p) as slab:
            for t in (0.25, 0.75):  # both sides of tBoundary
                got = slab.f(t, y)
                check("tiled RHS %s %s %dx%d t=%g" % (precision, label, nx, ny, t), got, eb.rhs_bound(op, t, y, precision))


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", golden_names("rhs_"))
def test_rhs_goldens_per_point(gpu_device, name, precision):
    meta, arr = load_golden(name)
    op = oracle_problem(meta)
    y = arr["y"].astype(DTYPE[precision])
    with crd.Slab(crd_params(meta, precision)) as slab:
        for t in (meta["t_absorbing"], meta["t_free"]):
            check("tiled RHS %s %s t=%g" % (precision, name, t), slab.f(t, y), eb.rhs_bound(op, t, y, precision))


def test_exact_zeros(gpu_device):
    """A uniform field diffuses to exactly zero (crd_device.h: first differences), and diffusion-only Goldbeter has dv == 0."""
    for precision in ("f64", "f32"):
        for surface in ("torus", "flat"):
            p, op = problem("goldbeter", surface, 121, 70, 0.4, precision=precision, just_diffusion=1)
            y = np.empty((70, 121, 2), dtype=DTYPE[precision])
            y[..., 0], y[..., 1] = 0.7312, -1.25
            with crd.Slab(p) as slab:
                got = slab.f(0.0, y)
            assert np.all(got == 0.0), (precision, surface, np.argwhere(got != 0.0)[:3])


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_rhs_per_point_through_slabs_group_and_ring(gpu_device, precision):
    for label, model, surface, beta, kw in CONFIGS[1:2] + CONFIGS[3:5]:
        p, op = problem(model, surface, 200, 96, beta, t_boundary=0.5, precision=precision, **kw)
        y = state(op, 5, precision)
        for t in (0.25, 0.75):
            bounded = eb.rhs_bound(op, t, y, precision)
            with crd.LocalGroup(p, 3) as grp:
                check("group of 3 slabs %s %s t=%g" % (precision, label, t), grp.f(t, y), bounded)
            with crd.Slab(p) as slab:
                slab.init_rccl(crd.rccl_unique_id())
                check("RCCL self-ring %s %s t=%g" % (precision, label, t), slab.f(t, y), bounded)


def full_grid(n, precision):
    """FHN torus n x n from the reference's initial-condition rule (built in row chunks), plus a smooth perturbation."""
    p = crd.make_params("fhn", "torus", n, L, W, D, 1.25, ny=n, precision=precision)
    op = co.make_problem(co.FHN, co.TORUS, n, L, W, D, 1.25, ny=n)
    cfg = crd.run_config(p, wave_length=0.1, wave_width=0.5, wave_inside=0)
    y = np.empty((n, n, 2), dtype=DTYPE[precision])
    th = np.sin(np.arange(n) * op.dx)
    for a in range(0, n, 1024):
        y[a:a + 1024] = crd.initial_conditions(cfg, a, a + 1023)
        y[a:a + 1024, :, 0] += (0.05 * np.cos(np.arange(a, a + 1024) * op.dy)[:, None] * th[None, :]).astype(y.dtype)
    edge = int(np.argmax(y[:, 0, 1] != y[0, 0, 1]))  # first row of the initial rectangle (v is not perturbed)
    assert 0 < edge < n // 4
    return p, op, y, [n - 8, edge - 8, 3 * n // 4]  # the phi seam, the front, the quiet field


@pytest.mark.parametrize("n,precision", [(8192, "f64"), (16384, "f32")])
def test_full_grid_bands_per_point(gpu_device, n, precision):
    """f() and one step of the full grid: 16-row bands (every band holds the theta seam) against the reference on cropped strips."""
    p, op, y, bands = full_grid(n, precision)
    dt = 0.8 * crd.stable_dt(p)
    plan = (0, 0, 1, 0) if precision == "f64" else (0, 0, 2, 0)
    with crd.Slab(p) as slab:
        f = slab.f(0.0, y)
    y1 = one_step(p, y, 0.0, dt, "fused", plan)
    for j0 in bands:
        rows = np.arange(j0 - 1, j0 + 17) % n
        check("tiled RHS %s %d^2 rows %d..%d" % (precision, n, j0, j0 + 15), f[rows], eb.rhs_bound(op, 0.0, y[rows], precision, j0=j0 - 1),
                 rows=slice(1, 17), j0=j0 - 1)
        rows = np.arange(j0 - 4, j0 + 20) % n
        check("one step %s %d^2 rows %d..%d" % (precision, n, j0, j0 + 15), y1[rows], eb.rk4_step_bound(op, 0.0, dt, y[rows], precision, j0=j0 - 4),
                 rows=slice(4, 20), j0=j0 - 4)


STEP_CASES = [  # (label, config index, t_boundary in units of dt: off, all four stages absorbing, switching off after stage 1)
    ("fhn-varybeta-switching", 1, 0.25),
    ("goldbeter-absorbing", 3, 2.0),
    ("diffusion-only", 5, 0.0),
    ("fhn-flat-absorbing-off", 2, 0.0),
]


def plans():
    return sorted({c[:4] for c in crd.launch_plan_candidates()})


def step_cases(nx, ny, precision):
    for label, k, tb in STEP_CASES:
        _, model, surface, beta, kw = CONFIGS[k]
        p0, _ = problem(model, surface, nx, ny, beta, precision=precision, **kw)
        dt = 0.8 * crd.stable_dt(p0)
        t = 3 * dt
        p, op = problem(model, surface, nx, ny, beta, t_boundary=t + tb * dt, precision=precision, **kw)
        y = state(op, nx + ny, precision)
        yield label, p, op, y, t, dt


def one_step(p, y, t, dt, stepper, plan=None):
    with crd.Slab(p) as slab:
        slab.set_stepper(stepper)
        if plan is not None:
            slab.set_launch_plan(*plan, steps_per_launch=1)
        slab.upload(y)
        slab.step_rk4(t, dt, 1)
        if plan is not None:
            lp = slab.launch_plan()
            assert lp["steps_per_launch"] == 1 and (lp["one_round"], lp["xcd_mapping"], lp["columns_per_lane"], lp["nontemporal_stores"]) == plan, lp
        return slab.download(y.dtype)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx", WIDTHS)
def test_one_step_per_point_across_strip_widths(gpu_device, nx, precision):
    """Staged stepper and the one-step kernel with one and with two columns per lane."""
    ny = ragged(nx) + 9
    for label, p, op, y, t, dt in step_cases(nx, ny, precision):
        bounded = eb.rk4_step_bound(op, t, dt, y, precision)
        check("staged step %s %s %dx%d" % (precision, label, nx, ny), one_step(p, y, t, dt, "staged"), bounded)
        for plan in ((0, 0, 1, 0), (1, 1, 2, 1)):
            check("one-step kernel %s %s %dx%d plan %s" % (precision, label, nx, ny, plan), one_step(p, y, t, dt, "fused", plan), bounded)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny", [(233, 300), (1000, 130)])
def test_one_step_per_point_every_launch_plan(gpu_device, nx, ny, precision):
    """Every launch-plan candidate's chunk mode, XCD mapping, columns per lane and store kind, pinned at one step per launch."""
    for label, p, op, y, t, dt in step_cases(nx, ny, precision):
        bounded = eb.rk4_step_bound(op, t, dt, y, precision)
        for plan in plans():
            check("one-step kernel %s %s %dx%d plan %s" % (precision, label, nx, ny, plan), one_step(p, y, t, dt, "fused", plan), bounded)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_one_step_per_point_group_of_three_slabs(gpu_device, precision):
    for label, p, op, y, t, dt in step_cases(200, 150, precision):
        bounded = eb.rk4_step_bound(op, t, dt, y, precision)
        for stepper in ("staged", "fused"):
            with crd.LocalGroup(p, 3) as grp:
                grp.set_stepper(stepper)
                grp.upload(y)
                grp.step_rk4(t, dt, 1)
                check("group of 3 slabs %s step %s %s" % (stepper, precision, label), grp.download(y.dtype), bounded)
