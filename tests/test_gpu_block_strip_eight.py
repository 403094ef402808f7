"""Launch-plan chunk mode 3: the three-step fp64 FHN block strip with EIGHT wavefronts around one apron (crd_fused_impl.h: kWideWaves; crd_fused_plan.h: choose;
488 valid lanes of 512, one block per CU).  Every test pins plans with crd_set_launch_plan and asserts bit equality (np.array_equal on
both fields) against the same problem stepped one step per launch under the plain plan (0, 0, 1, 1, 1).  FHN fp64 on the torus; the initial
state is the reference rule's travelling wave plus a seeded perturbation of every point (on the wave's flat parts a wrong neighbour
would hold the right value).

What can go wrong is in the theta cut (block strips of 488 columns, wavefronts of 64 lanes, an apron of 12), in the edge exchange between
eight wavefronts (slots and dump area sized by the width), in the barrier of a block whose last wavefronts hold only parked lanes, and in
the host code that switches between the eight-wide kernel and the four-wide one inside a step.  So:

widths      200, 487, 488, 489, 976, 977, 1000: at, just below and just above one and two strips.
hazard      A wavefront of the last block whose lanes are ALL parked (its first storing column, x0 of the wavefront -- x0 + 12 for the
widths      block's first --, lies at or beyond nx) still publishes the edge values its western neighbour's lane 63 reads.  With
            r = nx - 488 (blocks - 1) in 1 .. 488, wavefront w >= 1 is parked iff 64 w - 12 >= r: seven parked wavefronts for r <= 52, six up
            to 116, ... one up to 436, none above (nx = 200: four -- wavefronts 4 .. 7).  HAZARD_WIDTHS has one width inside each of the
            seven runs and the two on each border, in the first block and (for the outer runs) in the second.
heights     24 (= 6 kStepHalo, the least a triple takes), 25, 29 (items of 4 rows and a last one of 1) under every XCD mapping, and
            8192 x 250: the whole-rounds rule's 15 items of 17 rows and a last one of 12, eight wavefronts per block asserted.
steps       1 .. 7 from the initial state (every residue mod 3, with the pair and single tails), and one state advanced by calls of
            3, 5, 1 and 4 steps.
absorbing   t_boundary inside the first triple: rows switch off stage by stage, and the band around the boundary rows goes out four wide
rows        (the ABSORB kernel) while the interior goes out eight wide, in the same step.
repeat      nx = 489 three times in one process.
fallback    on a Goldbeter and on an fp32 context mode 3 is mode 1: crd_get_launch_plan says so, same bits.
geometry    61 valid lanes of 64, the instantiation's own table row (a digest of its own)."""
import functools

import numpy as np
import pytest

import crdmodel_amd as crd

pytestmark = pytest.mark.gpu

PLAIN = (0, 0, 1, 1, 1)
WIDTHS = (200, 487, 488, 489, 976, 977, 1000)
# r = 1 .. 488 by the number of parked wavefronts: [1, 52] seven, [53, 116] six, [117, 180] five, [181, 244] four, [245, 308] three,
# [309, 372] two, [373, 436] one, [437, 488] none (tests/test_block_strip_eight_host.py derives the same from x0)
_BORDERS = (52, 116, 180, 244, 308, 372, 436)
_INSIDE = (30, 84, 150, 212, 280, 340, 400)
HAZARD_WIDTHS = tuple(sorted(set(_INSIDE) | {b + d for b in _BORDERS for d in (0, 1)} | {488 + 30, 488 + 52, 488 + 53, 488 + 400, 488 + 436, 488 + 437}))


def _params(model, nx, ny, precision="f64", t_boundary=0.0):
    return crd.make_params(model, "torus", nx, 80.0, 20.0, 0.12, 1.25 if model == "fhn" else 0.4, ny=ny, precision=precision, t_boundary=t_boundary)


@functools.lru_cache(maxsize=None)
def _problem(nx, ny, model="fhn"):
    p = _params(model, nx, ny)
    y0 = np.array(crd.initial_conditions(crd.run_config(p, wave_length=0.1, wave_width=0.5)))
    rng = np.random.default_rng(1000 * nx + ny)
    if model == "fhn":
        y0 += 0.05 * rng.standard_normal(y0.shape)
    else:
        y0 *= 1.0 + 0.05 * rng.random(y0.shape)  # (concentrations stay positive)
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
    ref = _stepped(_params("fhn", nx, ny, t_boundary=tb_in_dt * dt), y0, dt, PLAIN, calls)
    for r in ref:
        r.setflags(write=False)
    assert not np.array_equal(ref[0], y0)
    return ref


def _wide(s):
    lp, g = s.launch_plan(), s.launch_geometry()
    assert lp["one_round"] == 3 and lp["steps_per_launch"] == 3 and g["wavefronts_per_workgroup"] == 8 and g["lanes_valid"] == 61, (lp, g)


def _check(nx, ny, mapping, calls=(3,), tb_in_dt=0.0, expect=_wide):
    y0, dt = _problem(nx, ny)
    want = _reference(nx, ny, calls, tb_in_dt)
    got = _stepped(_params("fhn", nx, ny, t_boundary=tb_in_dt * dt), y0, dt, (3, mapping, 1, 1, 3), calls, expect)
    for k, (g, w) in enumerate(zip(got, want)):
        same = np.array_equal(g[..., 0], w[..., 0]) and np.array_equal(g[..., 1], w[..., 1])
        if not same:
            cols = np.unique(np.nonzero((g != w).any(axis=(0, 2)))[0])
            print("nx %d ny %d mapping %d call %d of %r: %d columns differ, first %s" % (nx, ny, mapping, k, calls, len(cols), cols[:8]))
        assert same, (nx, ny, mapping, calls, k, tb_in_dt)


@pytest.mark.parametrize("nx", WIDTHS)
def test_widths_around_one_and_two_eight_wide_strips(gpu_device, nx):
    for mapping in (0, 1, 2):
        _check(nx, 40, mapping)


def test_widths_at_which_a_wavefront_of_the_last_block_holds_only_parked_lanes(gpu_device):
    for nx in HAZARD_WIDTHS:
        _check(nx, 24, 1)


@pytest.mark.parametrize("ny", (24, 25, 29))
def test_heights_at_the_minimum_and_with_unequal_items(gpu_device, ny):
    def expect(s):
        _wide(s)
        g = s.launch_geometry()
        if ny == 29:
            assert g["chunks"] >= 2 and ny % g["chunk_rows"] != 0, g
    for mapping in (0, 1, 2):
        _check(489, ny, mapping, expect=expect)


def test_whole_rounds_items_on_the_full_width(gpu_device):
    def expect(s):
        _wide(s)
        g = s.launch_geometry()
        assert g["strips"] == 8 * 17 and g["chunk_rows"] == 17 and g["chunks"] == 15 and g["workgroups"] == 17 * 15, g
    _check(8192, 250, 1, expect=expect)


def test_step_counts(gpu_device):
    for k in range(1, 8):
        _check(489, 40, 1, calls=(k,))
    _check(1000, 40, 0, calls=(3, 5, 1, 4))


@pytest.mark.parametrize("nx", (489, 1000))
def test_absorbing_rows_switch_off_inside_a_triple(gpu_device, nx):
    # t_boundary = 1.6 dt: on for all stages of step 1, for the first stage(s) of step 2, off in step 3 -- the band of 26 rows around
    # rows ny - 1 / 0 is the four-wide ABSORB kernel's, the other 38 rows the eight-wide kernel's
    y0, dt = _problem(nx, 64)
    off = _reference(nx, 64, (3, 4))
    on = _reference(nx, 64, (3, 4), 1.6)
    assert not np.array_equal(on[0], off[0])
    for mapping in (0, 1, 2):
        _check(nx, 64, mapping, calls=(3, 4), tb_in_dt=1.6)


def test_the_same_bits_three_times_in_one_process(gpu_device):
    y0, dt = _problem(489, 40)
    p = _params("fhn", 489, 40)
    runs = [_stepped(p, y0, dt, (3, 1, 1, 1, 3), (6,), _wide)[0] for _ in range(3)]
    assert np.array_equal(runs[0], _reference(489, 40, (6,))[0])
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


@pytest.mark.parametrize("model,precision", (("goldbeter", "f64"), ("fhn", "f32")))
def test_mode_three_is_mode_one_where_the_eight_wide_kernel_does_not_run(gpu_device, model, precision):
    nx, ny = 488, 40
    y0, dt = _problem(nx, ny, model)
    p = _params(model, nx, ny, precision)
    plans = {}

    def note(mode):
        def expect(s):
            plans[mode] = (s.launch_plan(), s.launch_geometry())
        return expect
    one = _stepped(p, y0, dt, (1, 1, 1 if precision == "f64" else 2, 1, 3), (6,), note(1))[0]
    three = _stepped(p, y0, dt, (3, 1, 1 if precision == "f64" else 2, 1, 3), (6,), note(3))[0]
    assert plans[3][0] == plans[1][0] and plans[3][0]["one_round"] == 1, plans
    assert plans[3][1] == plans[1][1] and plans[3][1]["wavefronts_per_workgroup"] == 4, plans
    assert np.array_equal(one[..., 0], three[..., 0]) and np.array_equal(one[..., 1], three[..., 1])


def test_geometry_reports_the_eight_wide_instantiation(gpu_device):
    p = _params("fhn", 8192, 8192)
    with crd.Slab(p) as s:
        s.set_launch_plan(1, 1, 1, 1, 3)
        g4 = s.launch_geometry()
        s.set_launch_plan(3, 1, 1, 1, 3)
        g8 = s.launch_geometry()
        assert s.launch_plan()["one_round"] == 3
    assert g4["lanes_valid"] == 58 and g4["wavefronts_per_workgroup"] == 4
    # 17 block strips x 15 items of 547 rows: 0.996 rounds of the 256 blocks a 256-CU device holds
    assert g8["lanes_valid"] == 61 and g8["wavefronts_per_workgroup"] == 8 and g8["strips"] == 8 * 17 and g8["chunk_rows"] == 547 and g8["workgroups"] == 255, g8
    assert g8["loop_valu"] > 0 and g8["loop_instructions"] > g8["loop_valu"] and g8["wavefronts_per_simd"] == 2 and g8["vgprs"] <= 256 and g8["scratch_bytes"] == 0, g8
    assert g8["lds_bytes"] > g4["lds_bytes"] and g8["exec_skipped_vmem"] == 0
    assert crd.kernel_digest(g8) and crd.kernel_digest(g8) != crd.kernel_digest(g4)
