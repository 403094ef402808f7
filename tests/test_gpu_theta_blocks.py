"""theta-block contexts (crd_create_block with d0 > 1, LocalGroup(..., blocks=(d0, d1))) at block widths beyond one 64-column tile.

Only this layout has SlabDesc::wrap_x == 0: the tile loaders of crd_rk4_stage_kernel and crd_rhs_aos_kernel take the west / east
neighbour of a block's first / last column from the ghost-column strips, crd_cols_extract_kernel packs the edge columns (stride
1 from a plane, stride 2 from var0 of an AoS vector), exchange_block_input / prime_block_halo move them, staged_step_blocks steps
with them, and crd_create_block slices the per-column tables cE / cWn / cP.  tests/test_theta_blocks_host.py shows that a per-tile
slip in the strips' rule cannot be seen by a block of 64 columns or fewer, and states the shape table used here (SHAPES): blocks
of 2 to 131 columns, neighbours one column apart in width, two, three and four blocks across, phi whole and cut.  Every whole
grid of the table is accepted as it stands (none had to be replaced).

Every assertion is bit identity with the whole-domain context (same point function, same stage arithmetic), an exact zero, or a
per-point bound of oracle/error_bounds.py; every gate prints its BOUND line (run with -s to collect them).
"""
import numpy as np
import pytest

import crdmodel_amd as crd
from oracle import error_bounds as eb
from test_gpu_error_bounds import CONFIGS, STEP_CASES, check, one_step, problem, state
from test_theta_blocks_host import SHAPES

pytestmark = pytest.mark.gpu

DTYPE = {"f64": np.float64, "f32": np.float32}
ENTRIES = [s[0] for s in SHAPES]
STEP_ENTRIES = [e for e in ENTRIES if e[:2] in ((5, 2), (129, 2), (193, 3), (260, 2), (391, 3), (258, 4))]
assert len(ENTRIES) == 9 and len(STEP_ENTRIES) == 6


def entry_id(e):
    return "%d/%dx%d/%d" % (e[0], e[1], e[2], e[3])


def blocks_of(p, d0, d1):
    """The LOCAL group of d0 x d1 block contexts, its extents held to the library's split rule before anything runs."""
    grp = crd.LocalGroup(p, 0, blocks=(d0, d1))
    g = crd.grid_of(p)
    want = [crd.block_extents(g.nx, g.ny, c0, d0, c1, d1) for c0 in range(d0) for c1 in range(d1)]
    assert [(s.is_, s.ie, s.js, s.je) for s in grp.slabs] == want and len(want) == d0 * d1, want
    return grp


# ---- (a) f() per point and bit for bit ----
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("entry", ENTRIES, ids=entry_id)
def test_rhs_through_blocks_per_point_and_bit_for_bit(gpu_device, entry, precision):
    """All six configurations (three of them on the torus, where cE / cWn / cP differ column by column and a wrongly sliced table
    shows), both sides of tBoundary: the absorbing rows' exact zeros are part of the bound on every block that owns row 0 or ny - 1."""
    nx, d0, d1, ny = entry
    for k, (label, model, surface, beta, kw) in enumerate(CONFIGS):
        p, op = problem(model, surface, nx, ny, beta, t_boundary=0.5, precision=precision, **kw)
        y = state(op, nx * 10 + k, precision)
        with crd.Slab(p) as one, blocks_of(p, d0, d1) as grp:
            for t in (0.25, 0.75):
                got = grp.f(t, y)
                case = "theta-blocks RHS %s %s %s t=%g" % (precision, label, entry_id(entry), t)
                check(case, got, eb.rhs_bound(op, t, y, precision))
                whole = one.f(t, y)
                assert np.array_equal(got, whole), (case, np.argwhere(got != whole)[:4])


# ---- (b) exact zero across the seams ----
@pytest.mark.parametrize("entry", [e for e in ENTRIES if e[:2] in ((129, 2), (391, 3))], ids=entry_id)
def test_uniform_field_diffuses_to_exact_zero_across_block_seams(gpu_device, entry):
    """test_gpu_error_bounds.test_exact_zeros through blocks: a ghost strip read from the wrong plane, row or field is not 0.7312."""
    nx, d0, d1, ny = entry
    for precision in ("f64", "f32"):
        for surface in ("torus", "flat"):
            p, op = problem("goldbeter", surface, nx, ny, 0.4, precision=precision, just_diffusion=1)
            y = np.empty((ny, nx, 2), dtype=DTYPE[precision])
            y[..., 0], y[..., 1] = 0.7312, -1.25
            with blocks_of(p, d0, d1) as grp:
                got = grp.f(0.0, y)
            assert got.shape == y.shape and np.all(got == 0.0), (precision, surface, np.argwhere(got != 0.0)[:3])


# ---- (c), (d): the staged step ----
def step_problem(k, tb, nx, ny, precision, seed=0):
    """Configuration k with t_boundary = t + tb dt at t = 3 dt, dt = 0.8 stable_dt (as test_gpu_error_bounds.step_cases)."""
    _, model, surface, beta, kw = CONFIGS[k]
    p0, _ = problem(model, surface, nx, ny, beta, precision=precision, **kw)
    dt = 0.8 * crd.stable_dt(p0)
    t = 3 * dt
    p, op = problem(model, surface, nx, ny, beta, t_boundary=t + tb * dt, precision=precision, **kw)
    return p, op, state(op, nx + ny + seed, precision), t, dt


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("entry", STEP_ENTRIES, ids=entry_id)
def test_one_staged_step_through_blocks_per_point(gpu_device, entry, precision):
    nx, d0, d1, ny = entry
    for label, k, tb in STEP_CASES:
        p, op, y, t, dt = step_problem(k, tb, nx, ny, precision)
        with blocks_of(p, d0, d1) as grp:
            grp.upload(y)
            grp.step_rk4(t, dt, 1)
            got = grp.download(y.dtype)
        case = "theta-blocks staged step %s %s %s" % (precision, label, entry_id(entry))
        check(case, got, eb.rk4_step_bound(op, t, dt, y, precision))
        whole = one_step(p, y, t, dt, "staged")
        assert np.array_equal(got, whole), (case, np.argwhere(got != whole)[:4])


def staged_slab(p):
    one = crd.Slab(p)
    one.set_stepper("staged")
    return one


def switching(tb):
    """(d): where STEP_CASES has absorbing rows, they switch off inside step 6 of the nine (after its first stage)."""
    return 5.25 if tb else 0.0


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("entry", STEP_ENTRIES, ids=entry_id)
def test_trajectory_through_blocks_bit_for_bit_across_calls(gpu_device, entry, precision):
    nx, d0, d1, ny = entry
    for label, k, tb in STEP_CASES:
        p, op, y, t0, dt = step_problem(k, switching(tb), nx, ny, precision)
        with staged_slab(p) as one, blocks_of(p, d0, d1) as grp:
            one.upload(y)
            grp.upload(y)
            for t, n in ((t0, 4), (t0 + 4 * dt, 5)):
                one.step_rk4(t, dt, n)
                grp.step_rk4(t, dt, n)
                got, whole = grp.download(y.dtype), one.download(y.dtype)
                assert np.all(np.isfinite(whole)) and not np.array_equal(whole, y)
                assert np.array_equal(got, whole), (precision, label, entry, n, np.argwhere(got != whole)[:4])


@pytest.mark.parametrize("entry,precision", [((260, 2, 1, 24), "f64"), ((258, 4, 3, 50), "f32")], ids=["260/2x1-f64", "258/4x3-f32"])
def test_rhs_calls_and_fresh_uploads_between_stepping_calls(gpu_device, entry, precision):
    """f() has strips of its own (edge_col / ghost_col, packed from the AoS vector) beside the stages' ecol / gcol and must not
    disturb a run; a state uploaded between two calls must have ITS edge columns exchanged by prime_block_halo."""
    nx, d0, d1, ny = entry
    for label, k, tb in STEP_CASES:
        p, op, y, t0, dt = step_problem(k, switching(tb), nx, ny, precision)
        fresh = step_problem(k, switching(tb), nx, ny, precision, seed=1)[2]
        assert not np.array_equal(fresh, y)
        with staged_slab(p) as one, blocks_of(p, d0, d1) as grp:
            def both(what):
                got, whole = what(grp), what(one)
                assert np.array_equal(got, whole), (precision, label, entry, np.argwhere(got != whole)[:4])
                return whole

            for c in (one, grp):
                c.upload(y)
                c.step_rk4(t0, dt, 4)
            now = both(lambda c: c.download(y.dtype))
            f_now = both(lambda c: c.f(t0 + 4 * dt, now))  # between the calls, on the state the run stands at
            assert np.any(f_now != 0.0)
            both(lambda c: c.f(t0 + 4 * dt, fresh))  # ... and on another one
            for c in (one, grp):
                c.step_rk4(t0 + 4 * dt, dt, 5)
            end = both(lambda c: c.download(y.dtype))
            assert not np.array_equal(end, now)
            for c in (one, grp):  # a fresh state between calls
                c.upload(fresh)
                c.step_rk4(t0 + 4 * dt, dt, 5)
            end2 = both(lambda c: c.download(y.dtype))
            assert not np.array_equal(end2, end)
