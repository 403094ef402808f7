"""The three-step fp64 block-strip kernel reads row p + 1 out of its LDS ring slot during iteration p (crd_fused_impl.h: kReadAhead,
ring_read_ahead) and takes the registers over at the top of iteration p + 1.  What can go wrong with it shows as wrong bits: a read that
overtakes the LDS-DMA fill of its slot (the hand-counted `s_waitcnt vmcnt`), a read from the wrong slot where a trip of four iterations
ends, a register with a read in flight that something touches, the first row's read in front of the loop, the read behind an item's
last row.  So: three-step plans against one-step plans, by the sha256 of the downloaded state, FHN fp64 on the torus, on the smallest
grids where each of these is exercised.

Widths: 232 and 233 (one block strip, and one column over), 463 / 464 / 465 (two strips), 40 (a block whose last wavefronts lie wholly
beyond nx).  Row counts 8, 9 (the ring's 8 rows and one over: too short for the twelve-row apron each side, such a grid takes single
steps whatever the plan asks for -- the plan's answer is checked, and the bits), 25 (ends inside the 24 filling iterations plus the
ring), 33, 61.  On grids this small the launch heuristic cuts the rows into items of 4 rows; 465 x 345 adds items of 8 rows and a last
item of one.  Step counts 3, 4, 5, 6, 9 from the initial state (a triple; a triple and a single step; a triple and a pair; two triples;
three); everything once without absorbing rows and once with `t_boundary` inside the first triple (held rows: the ABSORB body), under
chunk modes 0 and 1.

Items of those lengths IN the three-step kernel need a launch that fills the device: 2048 resident wavefronts x 58 columns, so
nx = 8192 (36 block strips), where chunk mode 1 cuts the rows into 14 items of ceil(ny / 14) rows and chunk mode 0 into items of 24
(the last one shorter).  The second test runs those: items of 9, 25, 33 and 61 rows, and 17, 18, 24, 27, 30 -- every residue of the
item's iterations mod 4 (the tail behind the unrolled loop: 0 to 3 iterations, each with its own read ahead), items that end inside
the first trips of the steady-state loop and items with ten of them.  `launch_geometry()["chunk_rows"]` is asserted, so the cases
cannot fall back to other items unnoticed.  One upload per context there; the calls of 3, 4, 5, 6 and 9 steps follow one another
(after 3, 7, 12, 18 and 27 steps the state is compared), each call a triple / a triple and a step / a triple and a pair / triples."""
import hashlib

import numpy as np
import pytest

import crdmodel_amd as crd

pytestmark = pytest.mark.gpu

WIDTHS = (232, 233, 463, 464, 465, 40)
ROWS = (8, 9, 25, 33, 61)
STEP_COUNTS = (3, 4, 5, 6, 9)
GRIDS = [(nx, ny) for nx in WIDTHS for ny in ROWS] + [(465, 345)]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _digests(p, y0, dt, plan, want_steps_per_launch=None):
    out = []
    with crd.Slab(p) as s:
        s.set_launch_plan(*plan)
        if want_steps_per_launch is not None:
            assert s.launch_plan()["steps_per_launch"] == want_steps_per_launch, (plan, s.launch_plan())
        for k in STEP_COUNTS:
            s.upload(y0)
            s.step_rk4(0.0, dt, k)
            out.append(_sha(s.download()))
    return out


@pytest.mark.parametrize("nx,ny", GRIDS)
def test_three_step_plans_with_the_row_read_ahead_give_the_one_step_bits(gpu_device, nx, ny):
    p0 = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny)
    dt = 0.7 * crd.stable_dt(p0)
    rng = np.random.default_rng(1000 * nx + ny)
    y0 = np.empty((ny, nx, 2))
    y0[..., 0] = -1.0 + 0.3 * rng.random((ny, nx))
    y0[..., 1] = -1.5 + 0.3 * rng.random((ny, nx))
    per_launch = 3 if ny >= 24 else 2 if ny >= 16 else 1  # (three steps need 24 rows: twelve of apron each side; pairs 16)
    for t_boundary in (0.0, 1.6 * dt):  # 1.6 dt: the absorbing rows switch off inside the first triple, stage by stage
        p = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, t_boundary=t_boundary)
        want = _digests(p, y0, dt, (0, 0, 1, 0, 1), 1)
        assert len(set(want)) == len(want) and _sha(y0) not in want
        for chunk_mode in (0, 1):
            got = _digests(p, y0, dt, (chunk_mode, 1, 1, 1, 3), per_launch)
            print("nx %d ny %d t_boundary %.3g chunk mode %d: %s" % (nx, ny, t_boundary, chunk_mode, ["ok" if g == w else "DIFFERS" for g, w in zip(got, want)]))
            assert got == want, (nx, ny, t_boundary, chunk_mode, [k for k, g, w in zip(STEP_COUNTS, got, want) if g != w])


# (ny, chunk mode, rows per item, rows of the last item)
LONG_ITEMS = [(369, 0, 24, 9), (369, 1, 27, 18), (238, 1, 17, 17), (350, 1, 25, 25), (420, 1, 30, 30), (462, 1, 33, 33), (854, 1, 61, 61)]


def _running_digests(p, y0, dt, plan, chunk_rows=None):
    out = []
    with crd.Slab(p) as s:
        s.set_launch_plan(*plan)
        if chunk_rows is not None:
            lp, g = s.launch_plan(), s.launch_geometry()
            assert lp["steps_per_launch"] == 3 and g["chunk_rows"] == chunk_rows and g["fill_iterations"] == 24 and g["strips"] == 4 * 36, (lp, g)
        s.upload(y0)
        done = 0
        for k in STEP_COUNTS:
            s.step_rk4(done * dt, dt, k)
            done += k
            out.append(_sha(s.download()))
    return out


@pytest.mark.parametrize("ny,chunk_mode,chunk_rows,last_rows", LONG_ITEMS)
def test_items_of_the_lengths_that_matter_give_the_one_step_bits(gpu_device, ny, chunk_mode, chunk_rows, last_rows):
    nx = 8192
    assert ny - (-(-ny // chunk_rows) - 1) * chunk_rows == last_rows
    p0 = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny)
    dt = 0.7 * crd.stable_dt(p0)
    rng = np.random.default_rng(ny)
    y0 = np.empty((ny, nx, 2))
    y0[..., 0] = -1.0 + 0.3 * rng.random((ny, nx))
    y0[..., 1] = -1.5 + 0.3 * rng.random((ny, nx))
    for t_boundary in (0.0, 1.6 * dt):
        p = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, t_boundary=t_boundary)
        want = _running_digests(p, y0, dt, (0, 0, 1, 0, 1))
        assert len(set(want)) == len(want) and _sha(y0) not in want
        got = _running_digests(p, y0, dt, (chunk_mode, 1, 1, 1, 3), chunk_rows)
        print("ny %d chunk mode %d items of %d (last %d) t_boundary %.3g: %s" % (ny, chunk_mode, chunk_rows, last_rows, t_boundary, ["ok" if g == w else "DIFFERS" for g, w in zip(got, want)]))
        assert got == want, (ny, chunk_mode, t_boundary, [k for k, g, w in zip(STEP_COUNTS, got, want) if g != w])
