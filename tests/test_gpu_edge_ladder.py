"""The three-step fp64 block strip taking its neighbours' edge values as each read lands (crd_fused_impl.h: kEdgeLadder; crd_edge_waits.h):
counted `s_waitcnt lgkmcnt(N)` in front of the stages that first need a read, in place of one wait for all six.  A change of schedule:
every test pins plans with crd_set_launch_plan and asserts bit equality (np.array_equal on both fields) against the same problem stepped
one step per launch under the plain plan (0, 0, 1, 1, 1).  FHN fp64 on the torus, the initial state perturbed at every point.

What can go wrong is a stage that runs on an edge value which has not landed -- a wrong count.  It shows only in the columns next to a
wavefront boundary INSIDE a block (places 64 k - 1 and 64 k of a strip), at any of the loop's unrolled positions and in the peeled and
tail code, and it is a race: every comparison runs twice and must give the reference's bits both times.  So:

widths      233 and 489: two strips, the second one's wavefronts but the first all parked lanes (four wide a strip stores 232 columns,
            eight wide 488); 464 and 976: two full strips; 1000.
heights     24 .. 33 at those widths: items of 6 rows, every tail length, last items of one row.
            Plans (1, m, 1, 1, 3) four wide and (3, m, 1, 1, 3) eight wide, m = 0, 1, 2; 3 and 7 steps.
long items  8192 x 250, 262, 281, 293: several trips of the peeled code and of the loop proper.
absorbing   t_boundary inside the first triple: the band around the boundary rows goes out four wide through the kernel with the selects
rows        (which keeps the single wait), the interior eight wide, in the same step.
calls       one state advanced by calls of 3, 5, 1 and 4 steps."""
import functools

import numpy as np
import pytest

import crdmodel_amd as crd

pytestmark = pytest.mark.gpu

PLAIN = (0, 0, 1, 1, 1)
HEIGHTS = tuple(range(24, 34))
WIDTHS = (233, 489, 464, 976, 1000)
PLANS = tuple((mode, m, 1, 1, 3) for mode in (1, 3) for m in (0, 1, 2))
LONG_ITEMS = (250, 262, 281, 293)
APRON = 12  # three steps of four columns a side


def _params(nx, ny, t_boundary=0.0):
    return crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, precision="f64", t_boundary=t_boundary)


@functools.lru_cache(maxsize=None)
def _problem(nx, ny):
    p = _params(nx, ny)
    y0 = np.array(crd.initial_conditions(crd.run_config(p, wave_length=0.1, wave_width=0.5)))
    y0 += 0.05 * np.random.default_rng(7000 * nx + ny).standard_normal(y0.shape)
    y0.setflags(write=False)
    return y0, 0.7 * crd.stable_dt(p)


def _stepped(p, y0, dt, plan, calls, expect=None):
    """The state after each of `calls` (step counts, one call after the other) under `plan`."""
    out = []
    with crd.Slab(p) as s:
        s.set_launch_plan(*plan)
        if expect is not None:
            expect(s)
        s.upload(y0)
        done = 0
        for k in calls:
            s.step_rk4(done * dt, dt, k)
            done += k
            out.append(np.array(s.download()))
    return out


@functools.lru_cache(maxsize=None)
def _reference(nx, ny, calls, tb_in_dt=0.0):
    y0, dt = _problem(nx, ny)
    ref = _stepped(_params(nx, ny, tb_in_dt * dt), y0, dt, PLAIN, calls)
    for r in ref:
        r.setflags(write=False)
    assert not np.array_equal(ref[0], y0)
    return ref


def boundary_columns(nx, waves):
    """The columns on both sides of every wavefront boundary inside a block that stores there: per strip, places 64 k - 1 and 64 k
    (k = 1 .. waves - 1) of its 64 waves lanes, of which the strip stores places APRON .. 64 waves - APRON - 1 from column
    strip x (64 waves - 2 APRON) on."""
    valid = 64 * waves - 2 * APRON
    cols = []
    for strip in range((nx + valid - 1) // valid):
        for k in range(1, waves):
            for place in (64 * k - 1, 64 * k):
                c = strip * valid + place - APRON
                if c < nx:
                    cols.append(c)
    return cols


def _width(plan):
    def expect(s):
        lp, g = s.launch_plan(), s.launch_geometry()
        assert lp["one_round"] == plan[0] and lp["steps_per_launch"] == 3 and g["wavefronts_per_workgroup"] == (8 if plan[0] == 3 else 4), (plan, lp, g)
    return expect


def _check(nx, ny, plan, calls=(3,), tb_in_dt=0.0, expect=None):
    y0, dt = _problem(nx, ny)
    want = _reference(nx, ny, calls, tb_in_dt)
    # the comparison is over every column of the grid: both sides of every interior wavefront boundary are among them
    edges = boundary_columns(nx, 8 if plan[0] == 3 else 4)
    assert edges and all(0 <= c < want[0].shape[1] for c in edges) and want[0].shape[1] == nx, (nx, plan, edges)
    for again in range(2):  # a race that loses only sometimes is still a failure
        got = _stepped(_params(nx, ny, tb_in_dt * dt), y0, dt, plan, calls, expect or _width(plan))
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape
            same = np.array_equal(g[..., 0], w[..., 0]) and np.array_equal(g[..., 1], w[..., 1])
            if not same:
                bad = (g != w).any(axis=2)
                rows, cols = np.unique(np.nonzero(bad)[0]), np.unique(np.nonzero(bad)[1])
                print("nx %d ny %d plan %r call %d of %r, run %d: %d rows differ, first %s; %d columns, first %s; at wavefront boundaries: %s"
                      % (nx, ny, plan, k, calls, again, len(rows), rows[:8], len(cols), cols[:8], sorted(set(cols) & set(edges))[:8]))
            assert same, (nx, ny, plan, calls, k, tb_in_dt, again)


def test_the_widths_put_columns_on_both_sides_of_every_interior_wavefront_boundary():
    # full strips: 2 (waves - 1) columns each, adjacent pairs; the strips of parked wavefronts (233 four wide, 489 eight wide) add none
    for nx, waves, strips, full in ((464, 4, 2, 2), (976, 8, 2, 2), (233, 4, 2, 1), (489, 8, 2, 1), (1000, 4, 5, 4), (1000, 8, 3, 2)):
        valid = 64 * waves - 2 * APRON
        assert (nx + valid - 1) // valid == strips
        cols = boundary_columns(nx, waves)
        assert len(cols) >= 2 * (waves - 1) * full and len(cols) % 2 == 0, (nx, waves, cols)
        assert all(b == a + 1 for a, b in zip(cols[0::2], cols[1::2])), (nx, waves, cols)
        for strip in range(full):
            assert {strip * valid + 64 * k - APRON for k in range(1, waves)} <= set(cols)
    assert 233 - 232 == 1 and 489 - 488 == 1  # (the second strip stores one column: its other wavefronts are parked lanes only)
    last = {ny: ny - 6 * ((ny + 5) // 6 - 1) for ny in HEIGHTS}
    assert set(last.values()) == {1, 2, 3, 4, 5, 6} and {r % 4 for r in last.values()} == {0, 1, 2, 3}, last


@pytest.mark.parametrize("ny", HEIGHTS)
def test_heights_with_every_tail_at_every_width(gpu_device, ny):
    def expect_for(plan):
        def expect(s):
            _width(plan)(s)
            g = s.launch_geometry()
            assert g["chunk_rows"] == 6 and g["chunks"] == (ny + 5) // 6, (ny, plan, g)  # items of 6 rows and a last one of ny mod 6 (or 6)
        return expect
    for nx in WIDTHS:
        for plan in PLANS:
            for steps in (3, 7):
                _check(nx, ny, plan, calls=(steps,), expect=expect_for(plan))


@pytest.mark.parametrize("ny", LONG_ITEMS)
def test_long_items_through_the_peeled_trips_and_the_loop(gpu_device, ny):
    _check(8192, ny, (3, 1, 1, 1, 3))
    _check(8192, ny, (1, 1, 1, 1, 3))


def test_absorbing_rows_switch_off_inside_a_triple(gpu_device):
    off = _reference(489, 64, (3, 4))
    on = _reference(489, 64, (3, 4), 1.6)
    assert not np.array_equal(on[0], off[0])
    for nx in (489, 464):
        for plan in ((3, 1, 1, 1, 3), (1, 1, 1, 1, 3)):
            _check(nx, 64, plan, calls=(3, 4), tb_in_dt=1.6)


def test_one_state_advanced_by_calls_of_unequal_length(gpu_device):
    _check(1000, 33, (3, 0, 1, 1, 3), calls=(3, 5, 1, 4))
    _check(489, 30, (1, 2, 1, 1, 3), calls=(3, 5, 1, 4))
    _check(233, 27, (1, 1, 1, 1, 3), calls=(3, 5, 1, 4))
    _check(976, 29, (3, 2, 1, 1, 3), calls=(3, 5, 1, 4))
