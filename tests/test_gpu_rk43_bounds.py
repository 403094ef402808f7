"""Per-point and norm gates of the RK4(3) attempt (CRD_ADAPT_RK43, fused_item<..., EMBED = 1, ...>) and of its dense output against
the bounds of oracle/error_bounds.py (rk43_attempt_bound, hermite_bound): lone contexts, slab cuts and the RCCL self-ring.

The pair shares the 54-column strips, the extra apron row and the err_lo / err_hi rule with the Zonneveld attempt
(tests/test_gpu_attempt_bounds.py), but the code between stage 4 and the lane's sum is its own: accumulators live beside the fifth
stage, a y_new window in U4, k4 itself in K4U / K4V, h6 * (k4 - k5) / w, a fifth absorbing flag the host decides at t + h, the
context's plan_embed.  tests/test_error_bounds.py: test_rk43_mutants_exceed_the_norm_bound shows that the norm bound sees a stale
neighbour at a strip's last column, a column counted twice, an uncounted row, the fifth flag at the wrong time and a wrong h / 6, and
where: in fp64 at every width and configuration here; in fp32 double counting, the flag's time and the factor at every width and
configuration, a stale strip-edge neighbour from 55 columns on (Goldbeter: from 217), a single uncounted row on the FHN and
diffusion-only configurations (on Goldbeter's state the front's rows carry the norm: not claimed).  Below those sizes the norm gate
still runs; it only is not known to see that mistake there.

Every case is ONE accepted attempt in isolation: integrate_adaptive(T0, T0 + h, h0 = h, method = RK4(3), no dense output, bias = 1) on
a fresh upload.  Without dense output the integrator clips the step to tout - t, so T0 = 0.25 and h is a float32 value:
(T0 + h) - T0 == h exactly (asserted), and err_last is bias = 1 times that attempt's norm.  Tolerances are scaled on the REFERENCE so
that its norm is 0.1 (test_error_bounds.attempt_bound), asserted in [1e-3, 0.5] before the device is touched.  Every failure names
the case, and for the state the worst point; every case prints its BOUND lines.
"""
import numpy as np
import pytest

import crdmodel_amd as crd
from oracle import error_bounds as eb
from test_error_bounds import ATTEMPT_CONFIGS, attempt_problem, attempt_state, attempt_step, rk43_bound
from test_gpu_attempt_bounds import DTYPE, WIDTHS, params_of
from test_gpu_error_bounds import check, ragged

pytestmark = pytest.mark.gpu

T0 = 0.25
RK43 = crd._capi.ADAPT_RK43
# tBoundary - t0 in units of h: off; stages 4 and 5 (both at t + h) free, where a fifth flag taken at t + 3/4 h would absorb; only
# stage 1 absorbing; all five absorbing; t == tBoundary (strict <: nothing absorbing)
PLACEMENTS = [("off", None), ("stages 4 and 5 free, 3/4 h absorbing", 0.8), ("only stage 1 absorbing", 0.3), ("all absorbing", 2.0), ("t == tBoundary", 0.0)]


def case_of(k, nx, ny, precision, placement=None, seed=0, t0=T0):
    """(op, h, y, tol, bound) of configuration k: the reference side of a case, before the device is touched.  h is a float32 value."""
    h = float(np.float32(attempt_step(attempt_problem(ATTEMPT_CONFIGS[k], nx, ny))))
    assert (t0 + h) - t0 == h, (t0, h)  # the step the integrator takes, tout - t, is the step the reference is given
    op = attempt_problem(ATTEMPT_CONFIGS[k], nx, ny, t_boundary=0.0 if placement is None else t0 + placement * h)
    y = attempt_state(op, nx + ny + k + seed, DTYPE[precision])
    tol, ab = rk43_bound(op, t0, h, y, precision)
    return op, h, y, tol, ab


def one_attempt(ctx, h, tol):
    return ctx.integrate_adaptive(T0, T0 + h, h0=h, h_max=-1.0, method=RK43, dense_output=0, bias=1.0, rtol=tol, atol=tol)


def judge(name, st, got, h, ab):
    """One accepted attempt: the state per point, err_last against the reference's norm."""
    assert (st["accepted"], st["rejected"], st["h_last"], st["t"]) == (1, 0, h, T0 + h), (name, st)
    check(name + " state", got, ab.state)
    ratio = abs(st["err_last"] - ab.dsm) / ab.dsm_bound
    print("BOUND %s norm: err_last %.17g, reference %.17g, |difference| / bound %.3g" % (name, st["err_last"], ab.dsm, ratio))
    assert ratio <= 1.0, (name, st["err_last"], ab.dsm, ab.dsm_bound)
    return ratio


def lone_attempt(name, op, h, y, tol, ab, precision):
    with crd.Slab(params_of(op, precision)) as slab:
        slab.upload(y)
        st = one_attempt(slab, h, tol)
        return judge(name, st, slab.download(y.dtype), h, ab)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx", WIDTHS)
def test_rk43_attempt_per_point_and_norm_across_strip_widths(gpu_device, nx, precision):
    """All six configurations at every strip edge of the attempt kernel, ragged ny; the placement of tBoundary rotates with the
    configuration and the width so that every width meets several and every configuration all five."""
    ny = ragged(nx)
    for k, case in enumerate(ATTEMPT_CONFIGS):
        label, placement = PLACEMENTS[(k + WIDTHS.index(nx)) % len(PLACEMENTS)]
        op, h, y, tol, ab = case_of(k, nx, ny, precision, placement)
        lone_attempt("RK4(3) attempt %s %s %dx%d tB %s" % (precision, case[0], nx, ny, label), op, h, y, tol, ab, precision)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("ny", [8, 9, 33])
def test_rk43_attempt_short_grids_and_a_last_chunk_of_one_row(gpu_device, ny, precision):
    """ny = 8, the fewest rows a context takes and fewer than a 16- or 32-row chunk; ny = 9 and 33, one row more than a whole number
    of 4- and 8-row (33: also 16- and 32-row) chunks, whichever rule the launch takes."""
    for nx in (55, 109):
        for k in (1, 3, 5):
            op, h, y, tol, ab = case_of(k, nx, ny, precision, 0.8)
            lone_attempt("RK4(3) attempt %s %s %dx%d" % (precision, ATTEMPT_CONFIGS[k][0], nx, ny), op, h, y, tol, ab, precision)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx", [55, 217])
def test_rk43_attempt_stage_times_around_tboundary_at_edge_widths(gpu_device, nx, precision):
    """All five placements of tBoundary against the stage times, each at a strip-edge width, for one FHN and one Goldbeter
    configuration."""
    ny = ragged(nx)
    for k in (1, 4):
        for label, placement in PLACEMENTS:
            op, h, y, tol, ab = case_of(k, nx, ny, precision, placement)
            lone_attempt("RK4(3) attempt %s %s %dx%d tB %s" % (precision, ATTEMPT_CONFIGS[k][0], nx, ny, label), op, h, y, tol, ab, precision)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_rk43_attempt_through_slabs_and_the_ring(gpu_device, precision):
    """163 x 47 cut into three ragged slabs (16 + 16 + 15 rows) and through the RCCL self-ring, held to the lone context's bound: the
    norm is reduced over the slabs, and err_lo / err_hi decide who counts a ghost-region row."""
    nx, ny = 163, 47
    for k in (1, 3, 5):
        for label, placement in PLACEMENTS[1:3]:
            op, h, y, tol, ab = case_of(k, nx, ny, precision, placement)
            p = params_of(op, precision)
            name = "%s %s %dx%d tB %s" % (precision, ATTEMPT_CONFIGS[k][0], nx, ny, label)
            with crd.LocalGroup(p, 3) as grp:
                grp.upload(y)
                st = one_attempt(grp, h, tol)
                judge("RK4(3) attempt, group of 3 slabs " + name, st, grp.download(y.dtype), h, ab)
            with crd.Slab(p) as slab:
                slab.init_rccl(crd.rccl_unique_id())
                slab.upload(y)
                st = one_attempt(slab, h, tol)
                judge("RK4(3) attempt, RCCL self-ring " + name, st, slab.download(y.dtype), h, ab)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx", [55, 217])
def test_rk43_dense_output_per_point(gpu_device, nx, precision):
    """One accepted step of the pair with dense output on and tout = theta h inside it returns the cubic Hermite interpolant: per
    point against hermite_bound, fed with the pair's AttemptBound.  From t0 = 0 the step the integrator interpolates with,
    t_{n+1} - t_n, and its theta, (tout - t_n) / (t_{n+1} - t_n), are the h and the theta the reference is given, exactly."""
    ny = 33
    for k in (1, 3):
        op, h, y, tol, ab = case_of(k, nx, ny, precision, 0.6, t0=0.0)
        p = params_of(op, precision)
        for theta in (0.25, 0.5, 0.999):
            tout = theta * h
            bounded = eb.hermite_bound(op, 0.0, h, tout / h, y, precision, ab)
            name = "RK4(3) dense output %s %s %dx%d theta %g" % (precision, ATTEMPT_CONFIGS[k][0], nx, ny, theta)
            with crd.Slab(p) as slab:
                slab.upload(y)
                st = slab.integrate_adaptive(0.0, tout, h0=h, h_max=-1.0, method=RK43, dense_output=1, bias=1.0, rtol=tol, atol=tol)
                assert (st["accepted"], st["rejected"], st["h_last"], st["t_internal"], st["t"]) == (1, 0, h, h, tout), (name, st)
                check(name, slab.download(y.dtype), bounded)
