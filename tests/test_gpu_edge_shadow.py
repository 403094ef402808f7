"""The three-step fp64 block strip with its publish and its fill in the shadow of the edge reads (crd_fused_impl.h, kReadAhead): behind an
iteration's barrier the reads of the neighbours' edge values go out, and the NEXT iteration publishes its row, starts its fill and advances its
row scalars before it waits for them; the row's registers land at the barrier's wait (edge_exchange names them), the first row's in front
of the loop (ring_first_row_landed), and the scalar load of the next b(j) goes out behind the wait for the edge values.  A change of
schedule: every test pins plans with crd_set_launch_plan and asserts bit equality (np.array_equal on both fields) against the same problem
stepped one step per launch under the plain plan (0, 0, 1, 1, 1).  FHN fp64 on the torus, the initial state perturbed at every point.

What can go wrong is a publish or a fill that runs ahead of what it depends on -- a row published before it landed (an item's first row,
the first row of a trip of four, the rows of the loop's tail), a slot filled while its row is still being read, a b(j) taken from the wrong
iteration -- at any of the loop's unrolled positions and in the straight-line code in front of and behind it.  So:

heights     24 .. 33 at widths 489 and 1000.  These grids run items of 6 rows (one trip of the loop and two positions of its tail); the
            last item has ny mod 6 rows, or 6: 6, 1, 2, 3, 4, 5, 6, 1, 2, 3 -- every residue mod 4, so the tail takes 0, 1, 2 and 3 positions,
            and last items of ONE row (25, 31), which the loop never sees.
            Plans (1, m, 1, 1, 3) four wide and (3, m, 1, 1, 3) eight wide, m = 0, 1, 2; 3 and 7 steps.
long items  8192 x 250, 262, 281, 293: items of 17, 18, 19, 20 rows and last items of 12, 10, 15, 13 -- several trips of the steady-state
            loop, and behind it the tail at 1, 2, 3, 0 positions (items) and 0, 2, 3, 1 (last items).
absorbing   t_boundary inside the first triple: the band around the boundary rows goes out four wide (the kernel with the selects, which
rows        holds both bodies) while the interior goes out eight wide, in the same step.
calls       one state advanced by calls of 3, 5, 1 and 4 steps."""
import functools

import numpy as np
import pytest

import crdmodel_amd as crd

pytestmark = pytest.mark.gpu

PLAIN = (0, 0, 1, 1, 1)
HEIGHTS = tuple(range(24, 34))
WIDTHS = (489, 1000)
PLANS = tuple((mode, m, 1, 1, 3) for mode in (1, 3) for m in (0, 1, 2))
LONG_ITEMS = {250: (17, 12), 262: (18, 10), 281: (19, 15), 293: (20, 13)}  # ny: rows of an item, of the last item (eight wide, 8192 columns)


def _params(nx, ny, t_boundary=0.0):
    return crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, precision="f64", t_boundary=t_boundary)


@functools.lru_cache(maxsize=None)
def _problem(nx, ny):
    p = _params(nx, ny)
    y0 = np.array(crd.initial_conditions(crd.run_config(p, wave_length=0.1, wave_width=0.5)))
    y0 += 0.05 * np.random.default_rng(1000 * nx + ny).standard_normal(y0.shape)
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


def _width(plan):
    def expect(s):
        lp, g = s.launch_plan(), s.launch_geometry()
        assert lp["one_round"] == plan[0] and lp["steps_per_launch"] == 3 and g["wavefronts_per_workgroup"] == (8 if plan[0] == 3 else 4), (plan, lp, g)
    return expect


def _check(nx, ny, plan, calls=(3,), tb_in_dt=0.0, expect=None):
    y0, dt = _problem(nx, ny)
    want = _reference(nx, ny, calls, tb_in_dt)
    got = _stepped(_params(nx, ny, tb_in_dt * dt), y0, dt, plan, calls, expect or _width(plan))
    for k, (g, w) in enumerate(zip(got, want)):
        same = np.array_equal(g[..., 0], w[..., 0]) and np.array_equal(g[..., 1], w[..., 1])
        if not same:
            bad = (g != w).any(axis=2)
            rows, cols = np.unique(np.nonzero(bad)[0]), np.unique(np.nonzero(bad)[1])
            print("nx %d ny %d plan %r call %d of %r: %d rows differ, first %s; %d columns, first %s" % (nx, ny, plan, k, calls, len(rows), rows[:8], len(cols), cols[:8]))
        assert same, (nx, ny, plan, calls, k, tb_in_dt)


@pytest.mark.parametrize("ny", HEIGHTS)
def test_heights_with_every_last_item(gpu_device, ny):
    def expect_for(plan):
        def expect(s):
            _width(plan)(s)
            g = s.launch_geometry()
            # items of 6 rows and a last one of ny mod 6 (or 6): what the module's text says these heights cover
            assert g["chunk_rows"] == 6 and g["chunks"] == (ny + 5) // 6, (ny, plan, g)
        return expect
    for nx in WIDTHS:
        for plan in PLANS:
            for steps in (3, 7):
                _check(nx, ny, plan, calls=(steps,), expect=expect_for(plan))


def test_the_heights_cover_every_residue_and_last_items_of_one_row():
    last = {ny: ny - 6 * ((ny + 5) // 6 - 1) for ny in HEIGHTS}
    assert set(last.values()) == {1, 2, 3, 4, 5, 6} and {r % 4 for r in last.values()} == {0, 1, 2, 3} and sum(1 for r in last.values() if r == 1) == 2, last
    for col in (0, 1):  # (the loop takes an item's rows four at a time: every number of positions of its tail, items and last items)
        assert {rows[col] % 4 for rows in LONG_ITEMS.values()} == {0, 1, 2, 3}, LONG_ITEMS


@pytest.mark.parametrize("ny", sorted(LONG_ITEMS))
def test_long_items_through_the_loop_and_every_tail(gpu_device, ny):
    rows, last = LONG_ITEMS[ny]

    def expect(s):
        _width((3, 1, 1, 1, 3))(s)
        g = s.launch_geometry()
        assert g["chunk_rows"] == rows and g["chunks"] == 15 and ny - 14 * rows == last, (ny, g)
    _check(8192, ny, (3, 1, 1, 1, 3), expect=expect)
    _check(8192, ny, (1, 1, 1, 1, 3))


def test_absorbing_rows_switch_off_inside_a_triple(gpu_device):
    # t_boundary = 1.6 dt: on for all stages of step 1, for the first stage(s) of step 2, off in step 3 -- the band around rows ny - 1 / 0 is
    # the four-wide kernel's with the selects, the other rows the eight-wide kernel's
    off = _reference(489, 64, (3, 4))
    on = _reference(489, 64, (3, 4), 1.6)
    assert not np.array_equal(on[0], off[0])
    for plan in ((3, 1, 1, 1, 3), (1, 1, 1, 1, 3)):
        _check(489, 64, plan, calls=(3, 4), tb_in_dt=1.6)


def test_one_state_advanced_by_calls_of_unequal_length(gpu_device):
    _check(1000, 33, (3, 0, 1, 1, 3), calls=(3, 5, 1, 4))
    _check(489, 30, (1, 2, 1, 1, 3), calls=(3, 5, 1, 4))
