"""Per-point and norm gates of the error-controlled attempt (Zonneveld 5(3)4, fused_item<..., EMBED = 2, ...>) and of the dense
output against the bounds of oracle/error_bounds.py: lone contexts, slab cuts, the RCCL self-ring and ensembles.

The attempt kernel has a geometry of its own -- 54-column strips, one more apron row and column per side, its own rule for the
rows and lanes that count towards the error sum -- and three kinds of mistake in it leave y_new exact and move only the scalar
err_last (tests/test_error_bounds.py: test_attempt_mutants_exceed_the_norm_bound shows that the norm bound sees each of them on
grids up to the largest one here).  Every case is ONE accepted attempt in isolation: integrate_adaptive(t0, t0 + h, h0 = h) on a
fresh upload -- no launch-ahead, no dense output, the downloaded state is y_new and err_last that attempt's norm.  Tolerances are
scaled on the REFERENCE so that its norm is 0.1 (test_error_bounds.attempt_bound), asserted in [1e-3, 0.5] before the device is
touched.  Widths: the edges of one, two, three, four and five 54-column strips; rows: ragged, 8, and 33 (a last chunk of one row
under the 4-row and the 8-row chunk rule alike).  Every failure names the case, and for the state the worst point.
The RK4(3) attempt (CRD_ADAPT_RK43, EMBED = 1) and its dense output are gated the same way in tests/test_gpu_rk43_bounds.py.
"""
import copy

import numpy as np
import pytest

import crdmodel_amd as crd
from oracle import error_bounds as eb
from test_error_bounds import ATTEMPT_CONFIGS, MODELS, SURFACES, L, W, attempt_bound, attempt_problem, attempt_state, attempt_step
from test_gpu_error_bounds import check, ragged

pytestmark = pytest.mark.gpu

WIDTHS = [5, 53, 54, 55, 107, 108, 109, 162, 163, 216, 217, 271, 1000]
DTYPE = {"f64": np.float64, "f32": np.float32}
T0 = 0.3
# tBoundary - t0 in units of h: off; stage 4 (t + h) free with stage 5 (t + 3/4 h) absorbing; stages 4 and 5 free; only stage 1
# absorbing; t == tBoundary (strict <: nothing absorbing)
PLACEMENTS = [("off", None), ("stage 5 absorbing, 4 free", 0.8), ("stages 4 and 5 free", 0.6), ("only stage 1 absorbing", 0.3), ("t == tBoundary", 0.0)]


def params_of(op, precision):
    return crd.make_params(MODELS[op.model], SURFACES[op.surface], op.nx, L, W, op.diff, op.beta, ny=op.ny, beta_min=op.beta_min, beta_max=op.beta_max,
                           vary_beta=op.vary_beta, just_diffusion=op.just_diffusion, t_boundary=op.t_boundary, precision=precision)


def case_of(k, nx, ny, precision, placement=None, seed=0, t0=T0):
    """(op, h, y, tol, bound) of configuration k: the reference side of a case, before the device is touched."""
    h = attempt_step(attempt_problem(ATTEMPT_CONFIGS[k], nx, ny))
    op = attempt_problem(ATTEMPT_CONFIGS[k], nx, ny, t_boundary=0.0 if placement is None else t0 + placement * h)
    y = attempt_state(op, nx + ny + k + seed, DTYPE[precision])
    tol, ab = attempt_bound(op, t0, h, y, precision)
    return op, h, y, tol, ab


def judge(name, st, got, h, ab):
    """One accepted attempt: the state per point, err_last against the reference's norm."""
    assert (st["accepted"], st["rejected"], st["t_internal"]) == (1, 0, T0 + h), (name, st)
    check(name + " state", got, ab.state)
    ratio = abs(st["err_last"] - ab.dsm) / ab.dsm_bound
    print("BOUND %s norm: err_last %.17g, reference %.17g, |difference| / bound %.3g" % (name, st["err_last"], ab.dsm, ratio))
    assert ratio <= 1.0, (name, st["err_last"], ab.dsm, ab.dsm_bound)
    return ratio


def lone_attempt(name, op, h, y, tol, ab, precision):
    with crd.Slab(params_of(op, precision)) as slab:
        slab.upload(y)
        st = slab.integrate_adaptive(T0, T0 + h, h0=h, h_max=-1.0, rtol=tol, atol=tol)
        return judge(name, st, slab.download(y.dtype), h, ab)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx", WIDTHS)
def test_attempt_per_point_and_norm_across_strip_widths(gpu_device, nx, precision):
    """All six configurations at every strip edge of the attempt kernel, ragged ny; the placement of tBoundary rotates with the
    configuration so that every width meets several."""
    ny = ragged(nx)
    for k, case in enumerate(ATTEMPT_CONFIGS):
        label, placement = PLACEMENTS[(k + nx) % len(PLACEMENTS)]
        op, h, y, tol, ab = case_of(k, nx, ny, precision, placement)
        lone_attempt("attempt %s %s %dx%d tB %s" % (precision, case[0], nx, ny, label), op, h, y, tol, ab, precision)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("ny", [8, 9, 33])
def test_attempt_short_grids_and_a_last_chunk_of_one_row(gpu_device, ny, precision):
    """ny = 8, the fewest rows a context takes and fewer than a 16- or 32-row chunk; ny = 9 and 33, one row more than a whole number
    of 4- and 8-row (33: also 16- and 32-row) chunks, whichever rule the launch takes (a grid this small gets 4-row chunks:
    fused_chunk_rows)."""
    for nx in (55, 109):
        for k in (1, 3, 5):
            op, h, y, tol, ab = case_of(k, nx, ny, precision, 0.8)
            lone_attempt("attempt %s %s %dx%d" % (precision, ATTEMPT_CONFIGS[k][0], nx, ny), op, h, y, tol, ab, precision)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx", [55, 217])
def test_attempt_stage_times_around_tboundary_at_edge_widths(gpu_device, nx, precision):
    """The four placements of the five stage times around tBoundary (and absorbing rows off), each at a strip-edge width."""
    ny = ragged(nx)
    for k in (1, 4):
        for label, placement in PLACEMENTS:
            op, h, y, tol, ab = case_of(k, nx, ny, precision, placement)
            lone_attempt("attempt %s %s %dx%d tB %s" % (precision, ATTEMPT_CONFIGS[k][0], nx, ny, label), op, h, y, tol, ab, precision)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_attempt_through_slabs_and_the_ring(gpu_device, precision):
    """163 x 47 cut into three ragged slabs (16 + 16 + 15 rows) and through the RCCL self-ring: the norm is reduced over the slabs,
    and err_lo / err_hi decide who counts a ghost-region row."""
    nx, ny = 163, 47
    for k in (1, 3, 5):
        for label, placement in PLACEMENTS[1:3]:
            op, h, y, tol, ab = case_of(k, nx, ny, precision, placement)
            p = params_of(op, precision)
            name = "%s %s %dx%d tB %s" % (precision, ATTEMPT_CONFIGS[k][0], nx, ny, label)
            with crd.LocalGroup(p, 3) as grp:
                grp.upload(y)
                st = grp.integrate_adaptive(T0, T0 + h, h0=h, h_max=-1.0, rtol=tol, atol=tol)
                judge("attempt, group of 3 slabs " + name, st, grp.download(y.dtype), h, ab)
            with crd.Slab(p) as slab:
                slab.init_rccl(crd.rccl_unique_id())
                slab.upload(y)
                st = slab.integrate_adaptive(T0, T0 + h, h0=h, h_max=-1.0, rtol=tol, atol=tol)
                judge("attempt, RCCL self-ring " + name, st, slab.download(y.dtype), h, ab)


# ---- ensembles -------------------------------------------------------------------------------------------------------------------
def ensemble_members(k, nx, ny, precision, count):
    """Members that differ in beta, diffusion, varyBeta and tBoundary, so that the five absorb flags differ between the members of one
    launch; one step and one tolerance for all (the options are the call's).  Returns (h, tol, [(op, y, bound)])."""
    base = attempt_problem(ATTEMPT_CONFIGS[k], nx, ny)
    variants = [dict(), dict(beta=0.8 * base.beta, diff=0.75 * base.diff), dict(vary_beta=1, beta_min=0.3, beta_max=1.4), dict(diff=0.5 * base.diff),
                dict(beta=1.1 * base.beta, vary_beta=1, beta_min=0.5, beta_max=1.2, diff=0.9 * base.diff)][:count]
    h = attempt_step(base)  # the largest diffusion's bound
    ops = []
    for m, over in enumerate(variants):
        placement = PLACEMENTS[(m + 1) % len(PLACEMENTS)][1]
        ops.append(attempt_problem(ATTEMPT_CONFIGS[k], nx, ny, t_boundary=0.0 if placement is None else T0 + placement * h, **over))
    ys = [attempt_state(op, nx + 7 * m, DTYPE[precision]) for m, op in enumerate(ops)]
    # one tolerance: the geometric mean of the members' own scales
    tols = [attempt_bound(op, T0, h, y, precision)[0] for op, y in zip(ops, ys)]
    tol = float(np.float32(np.exp(np.mean(np.log(tols)))))
    out = []
    for op, y in zip(ops, ys):
        ab = eb.erk_attempt_bound(op, T0, h, y, precision, tol, tol)
        assert 1e-3 <= ab.dsm <= 0.5, (tol, ab.dsm)
        out.append((op, y, ab))
    return h, tol, out


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("count", [1, 5])
@pytest.mark.parametrize("nx", [54, 55, 109, 217, 300, 330])
def test_ensemble_attempt_per_point_and_norm(gpu_device, nx, count, precision):
    """The same gate through Ensemble.integrate_adaptive with every member's own err_last: widths of one, two, three, five, six
    and seven strips -- a last block of the attempt kernel with one, two and three live wavefronts (sw = 4) --, B = 1 and 5.  The
    ensemble sums a member's partials over its own partition of work items, hence a bound and not bit-identity with a lone
    context.  FHN and Goldbeter alternate with the width."""
    k = (0, 3)[nx % 2]
    ny = 33 if nx % 3 else ragged(nx)
    h, tol, members = ensemble_members(k, nx, ny, precision, count)
    with crd.Ensemble([params_of(op, precision) for op, _, _ in members]) as e:
        for m, (_, y, _) in enumerate(members):
            e.upload(m, y)
        sts = e.integrate_adaptive(T0, T0 + h, h0=h, h_max=-1.0, rtol=tol, atol=tol)
        for m, (op, y, ab) in enumerate(members):
            assert sts[m]["status"] == crd._capi.OK, sts[m]
            judge("ensemble attempt %s %s %dx%d member %d of %d" % (precision, ATTEMPT_CONFIGS[k][0], nx, ny, m, count), sts[m], e.download(m, y.dtype), h, ab)


# ---- dense output ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx", [55, 217])
def test_dense_output_per_point_lone_and_ensemble(gpu_device, nx, precision):
    """One accepted step with tout = t0 + theta h inside it returns the cubic Hermite interpolant: per point against the
    reference-precision interpolant of the reference's y_n, y_{n+1}, f_n, f_{n+1} (error_bounds.hermite_bound).  t0 = 0 here: the
    integrator interpolates with the step it took, t_{n+1} - t_n, at (tout - t_n) / (t_{n+1} - t_n), and from t0 = 0 both are the
    h and the theta the reference is given, exactly; from t0 = 0.3 the rounding of t0 + h alone moves h by 80 ulps in fp64."""
    ny = 33
    for k in (1, 3):
        op, h, y, tol, ab = case_of(k, nx, ny, precision, 0.6, t0=0.0)
        p = params_of(op, precision)
        for theta in (0.25, 0.5, 0.999):
            tout = theta * h
            bounded = eb.hermite_bound(op, 0.0, h, tout / h, y, precision, ab)
            name = "dense output %s %s %dx%d theta %g" % (precision, ATTEMPT_CONFIGS[k][0], nx, ny, theta)
            with crd.Slab(p) as slab:
                slab.upload(y)
                st = slab.integrate_adaptive(0.0, tout, h0=h, h_max=-1.0, rtol=tol, atol=tol)
                assert (st["accepted"], st["rejected"], st["t_internal"]) == (1, 0, h), (name, st)
                check(name, slab.download(y.dtype), bounded)
            with crd.Ensemble([p, copy.copy(p)]) as e:
                e.upload(0, y)
                e.upload(1, y)
                sts = e.integrate_adaptive(0.0, tout, h0=h, h_max=-1.0, rtol=tol, atol=tol)
                assert all((s["accepted"], s["rejected"], s["t_internal"]) == (1, 0, h) for s in sts), (name, sts)
                check(name + " ensemble", e.download(1, y.dtype), bounded)
