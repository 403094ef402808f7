"""The three-step fp64 block strip with its rows addressed by ONE buffer resource per field and launch and a running 32-bit scalar byte
offset (crd_fused_impl.h, kScalarRows): the fills and the stores take the row as their scalar offset, the input offset advances by a row
pitch and jumps to the plane's first row behind its last (the periodic seam in phi), holds the item's last row in the tail, the output
offset advances by a pitch per iteration, b(j) is read at a running, clamped byte offset, and the fill phase's shorter wait is
straight-line code in front of the steady-state loop.  A change of addressing and schedule: every test pins plans with
crd_set_launch_plan -- (1, m, 1, nt, 3) four wavefronts wide, (3, m, 1, nt, 3) eight wide -- and asserts bit equality (np.array_equal on
both fields) against the same problem stepped one step per launch under the plain plan (0, 0, 1, 1, 1), as tests/test_gpu_edge_shadow.py
does.  FHN fp64, the initial state perturbed at every point.

What can go wrong: an offset that starts at the wrong row (the item's first row in front of row 0: rows -12 .. -1 are rows ny - 12 ..
ny - 1), that misses the seam or takes it twice, that runs on behind the item's last row, an output offset that is off while the pipeline
fills, a b(j) one row early or late, a lane parked beyond the resource's range that is written after all (the scalar offset is not part
of the range check -- if it were, rows far into the plane would not be stored), the wrong wait in one of the peeled iterations.  So:

heights   24, the least the plan accepts, and 25 .. 31 at width 489: items of 6 rows with last items of 6, 1, 2, 3, 4, 5, 6, 1 rows -- the
          loop's tail at every length, and items whose rows end inside the peeled trips (an item of 6 rows has 30 iterations: one peeled
          trip and two iterations of the tail).
          ONE item: 124441 columns x 24 rows (2048 and more wavefronts in a single chunk: the chunk is not halved) -- its apron rows cross
          the seam at BOTH ends of the plane, rows -12 .. -1 and 24 .. 35.
          TWO items, the last one shorter: 59161 columns x 41 rows, items of 21 and 20 rows.
          A flat surface at 489 x 30 and 233 x 27.  (A single slab wraps in phi on either surface -- Slab::wrap is 1 for every fp64
          three-step launch, fused_steps_supported -- so the kernel's other setting, a plane based at its first ghost row, has no launch
          that reaches it; the flat cases run the same kernel on the other surface's coefficients.)
widths    232 = the columns one four-wide block stores and 488 = one eight-wide block's, each - 1 and + 1; at 233 and 489 the second block
          stores ONE column: wavefronts 1 .. 3 (1 .. 7) of it hold parked lanes only; 242: ten columns in the second block, likewise;
          100: narrower than a block, whose lanes wrap around theta more than twice.  Every first block's apron crosses the theta seam
          (columns -12 .. -1), every last block's lanes beyond nx wrap to column 0.
steps     3, 4, 5, 6, 7 -- a triple, a triple and a single step, a triple and a pair, two triples, and one more.
calls     one state advanced by calls of 2, 5, 1 and 4 steps (every call cuts the sequence of triples).
absorbing t_boundary = 1.6 dt: the rows are held in step 1 and in the first stages of step 2, not in step 3 -- the band around rows
rows      ny - 1 / 0 is the four-wide kernel's body with the selects, also under the eight-wide plan.
stores    non-temporal and plain, under every mapping."""
import functools

import numpy as np
import pytest

import crdmodel_amd as crd

pytestmark = pytest.mark.gpu

PLAIN = (0, 0, 1, 1, 1)
FOUR, EIGHT = (1, 1, 1, 1, 3), (3, 1, 1, 1, 3)
WIDTHS = (100, 231, 232, 233, 242, 487, 488, 489)
HEIGHTS = tuple(range(24, 32))


def _params(nx, ny, t_boundary=0.0, surface="torus"):
    return crd.make_params("fhn", surface, nx, 80.0, 20.0, 0.12, 1.25, ny=ny, precision="f64", t_boundary=t_boundary)


@functools.lru_cache(maxsize=None)
def _problem(nx, ny, surface="torus"):
    p = _params(nx, ny, surface=surface)
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
def _reference(nx, ny, calls, tb_in_dt=0.0, surface="torus"):
    y0, dt = _problem(nx, ny, surface)
    ref = _stepped(_params(nx, ny, tb_in_dt * dt, surface), y0, dt, PLAIN, calls)
    for r in ref:
        r.setflags(write=False)
    assert not np.array_equal(ref[0], y0)
    return ref


def _width(plan):
    def expect(s):
        lp, g = s.launch_plan(), s.launch_geometry()
        assert lp["one_round"] == plan[0] and lp["steps_per_launch"] == 3 and lp["nontemporal_stores"] == plan[3], (plan, lp)
        assert g["wavefronts_per_workgroup"] == (8 if plan[0] == 3 else 4), (plan, g)
    return expect


def _check(nx, ny, plan, calls=(3,), tb_in_dt=0.0, expect=None, surface="torus"):
    y0, dt = _problem(nx, ny, surface)
    want = _reference(nx, ny, calls, tb_in_dt, surface)
    got = _stepped(_params(nx, ny, tb_in_dt * dt, surface), y0, dt, plan, calls, expect or _width(plan))
    for k, (g, w) in enumerate(zip(got, want)):
        same = np.array_equal(g[..., 0], w[..., 0]) and np.array_equal(g[..., 1], w[..., 1])
        if not same:
            bad = (g != w).any(axis=2)
            rows, cols = np.unique(np.nonzero(bad)[0]), np.unique(np.nonzero(bad)[1])
            print("nx %d ny %d plan %r call %d of %r: %d rows differ, first %s; %d columns, first %s" % (nx, ny, plan, k, calls, len(rows), rows[:8], len(cols), cols[:8]))
        assert same, (nx, ny, plan, calls, k, tb_in_dt, surface)


@pytest.mark.parametrize("nx", WIDTHS)
def test_widths_around_one_block_and_blocks_of_parked_wavefronts(gpu_device, nx):
    def expect_for(plan):
        def expect(s):
            _width(plan)(s)
            g = s.launch_geometry()
            valid = 8 * 64 - 24 if plan[0] == 3 else 4 * 64 - 24
            assert g["strips"] == g["wavefronts_per_workgroup"] * (-(-nx // valid)) and g["chunk_rows"] == 6 and g["chunks"] == 5, (nx, plan, g)
        return expect
    for plan in (FOUR, EIGHT):
        for steps in (3, 7):
            _check(nx, 26, plan, calls=(steps,), expect=expect_for(plan))


def test_the_widths_are_what_the_text_says():
    assert 4 * 64 - 24 == 232 and 8 * 64 - 24 == 488
    assert {232 - 1, 232, 232 + 1, 488 - 1, 488, 488 + 1} <= set(WIDTHS)
    # a second block that stores one column (ten): its first wavefront has 64 - 12 lanes for them, the others store nothing
    assert 233 - 232 == 1 and 489 - 488 == 1 and 242 - 232 == 10 and 10 <= 64 - 12
    last = {ny: ny - 6 * ((ny + 5) // 6 - 1) for ny in HEIGHTS}
    assert set(last.values()) == {1, 2, 3, 4, 5, 6} and min(HEIGHTS) == 24, last


@pytest.mark.parametrize("ny", HEIGHTS)
def test_heights_from_the_least_the_plan_accepts(gpu_device, ny):
    def expect_for(plan):
        def expect(s):
            _width(plan)(s)
            g = s.launch_geometry()
            assert g["chunk_rows"] == 6 and g["chunks"] == (ny + 5) // 6, (ny, plan, g)
        return expect
    for plan in (FOUR, EIGHT):
        for steps in (3, 7):
            _check(489, ny, plan, calls=(steps,), expect=expect_for(plan))


def test_one_item_whose_apron_crosses_the_seam_at_both_ends(gpu_device):
    def expect_for(plan):
        def expect(s):
            _width(plan)(s)
            g = s.launch_geometry()
            assert g["chunks"] == 1 and g["chunk_rows"] == 24 and g["rows"] == 24, (plan, g)
        return expect
    for plan in (FOUR, EIGHT):
        _check(124441, 24, plan, expect=expect_for(plan))


def test_two_items_the_last_one_shorter(gpu_device):
    def expect_for(plan):
        def expect(s):
            _width(plan)(s)
            g = s.launch_geometry()
            assert g["chunks"] == 2 and g["chunk_rows"] == 21 and g["rows"] == 41, (plan, g)
        return expect
    for plan in (FOUR, EIGHT):
        _check(59161, 41, plan, expect=expect_for(plan))


def test_a_flat_surface(gpu_device):
    for nx, ny in ((489, 30), (233, 27)):
        for plan in (FOUR, EIGHT):
            _check(nx, ny, plan, calls=(3, 4), surface="flat")


@pytest.mark.parametrize("steps", (3, 4, 5, 6, 7))
def test_step_counts_around_whole_triples(gpu_device, steps):
    for plan in (FOUR, EIGHT):
        _check(489, 30, plan, calls=(steps,))
        _check(1000, 33, plan, calls=(steps,))


def test_calls_that_cut_the_sequence_of_triples(gpu_device):
    _check(1000, 33, EIGHT, calls=(2, 5, 1, 4))
    _check(489, 30, FOUR, calls=(2, 5, 1, 4))


def test_absorbing_rows_switch_off_inside_a_triple(gpu_device):
    off = _reference(489, 64, (3, 4))
    on = _reference(489, 64, (3, 4), 1.6)
    assert not np.array_equal(on[0], off[0])
    for mode in (1, 3):
        for nt in (0, 1):
            _check(489, 64, (mode, 1, 1, nt, 3), calls=(3, 4), tb_in_dt=1.6)


@pytest.mark.parametrize("nt", (0, 1))
def test_plain_and_non_temporal_stores_under_every_mapping(gpu_device, nt):
    for mode in (1, 3):
        for mapping in (0, 1, 2):
            _check(1000, 33, (mode, mapping, 1, nt, 3), calls=(6,))
            _check(233, 27, (mode, mapping, 1, nt, 3), calls=(6,))
