"""Two RK4 steps per launch on ensembles (crd_ensemble_set_steps_per_launch, Ensemble.set_steps_per_launch, crd_run --ensemble-steps):
every member bit-identical -- np.array_equal, no tolerance -- to (a) the same ensemble stepped with one step per launch and (b) a lone
context of its parameters on the one-launch stepper; across strip and block layouts, both precisions, the block-as-strip Goldbeter
kernel, absorbing rows that switch off between and inside the steps of a pair, observers whose samples a pair must not straddle,
switching between the settings, and the refusals."""
import os
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
from conftest import ROOT
from test_gpu_ensemble import crd_run, lone, params_like, same_files, start_state, two_small_members, write_ini

pytestmark = pytest.mark.gpu

MIN_ROWS = 9  # CRD_ENSEMBLE_PAIR_MIN_ROWS (include/crd.h)
ONE_STEP_PLAN = (0, 0, 1, 0, 1)


def dtype_of(members):
    return np.float64 if members[0].precision == crd._capi.PRECISION_F64 else np.float32


def states(members, seed=0):
    ys = [start_state(p, seed + k) for k, p in enumerate(members)]
    return [y.astype(dtype_of(members)) for y in ys]


def stepped(members, ys, t0, dt, calls, steps_per_launch):
    """The members' states after `calls` = [(first step, count), ...] under the given setting."""
    with crd.Ensemble(members) as e:
        if steps_per_launch != 1:
            e.set_steps_per_launch(steps_per_launch)
        assert e.steps_per_launch == steps_per_launch
        for k, y in enumerate(ys):
            e.upload(k, y)
        for a, b in calls:
            e.step_rk4(t0 + a * dt, dt, b)
        out = [e.download(k, dtype_of(members)) for k in range(len(members))]
        assert all(np.isfinite(m) for m in e.max_abs())
    return out


def check_pairs(members, t0, dt, calls, seed=0):
    """Pairs against (a) singles of the same ensemble and (b) lone contexts on the one-launch stepper: every bit."""
    ys = states(members, seed)
    pairs = stepped(members, ys, t0, dt, calls, 2)
    singles = stepped(members, ys, t0, dt, calls, 1)
    for k, p in enumerate(members):
        assert np.array_equal(pairs[k], singles[k]), ("member", k, "against single steps", float(np.max(np.abs(pairs[k].astype(np.float64) - singles[k]))))
        want = lone(p, ys[k], t0, dt, calls, ONE_STEP_PLAN)
        assert np.array_equal(pairs[k], want), ("member", k, "against a lone context", float(np.max(np.abs(pairs[k].astype(np.float64) - want))))
    return pairs


def fhn_across_hopf(nx, ny, precision="f64", surface="torus"):
    """Three members, beta across the Hopf point (excitable / near it / oscillatory); one varies beta over the rows."""
    base = crd.make_params("fhn", surface, nx, 80.0, 20.0, 0.12, 1.25, ny=ny, beta_min=0.7, beta_max=1.7, precision=precision)
    return [params_like(base, beta=0.6), params_like(base, beta=1.0, diffusion=0.08), params_like(base, beta=1.4, vary_beta=1)]


def safe_dt(members):
    return 0.8 * min(crd.stable_dt(p) for p in members)


@pytest.mark.parametrize("nsteps", [5, 1])
@pytest.mark.parametrize("nx,ny", [(61, 33), (130, 21), (230, 33), (61, MIN_ROWS)])
def test_fhn_fp64_pairs(gpu_device, nx, ny, nsteps):
    """61 x 33: narrower than a strip's 48 valid columns + aprons, odd, wraps in theta; 130 x 21: three strips, one block; 230 x 33: five
    strips, a partly filled second block; 61 x 9: the smallest accepted ny.  5 steps = pair, pair, single; 1 = no pair at all."""
    members = fhn_across_hopf(nx, ny)
    assert crd.grid_of(members[0]).ny == ny
    check_pairs(members, 0.0, safe_dt(members), [(0, nsteps)])


@pytest.mark.parametrize("nx,ny", [(100, 40), (300, 21)])
def test_goldbeter_block_strip_and_diffusion_only(gpu_device, nx, ny):
    """Goldbeter fp64 runs the block as the strip (one apron round the block's wavefronts, edge values through LDS): 100 x 40, one
    block; 300 x 21, two strip blocks, the second partly filled.  Diffusion-only: a strip per wavefront."""
    base = crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, 0.4, ny=ny)
    members = [params_like(base, beta=b) for b in (0.3, 0.5, 0.75)]
    dt = safe_dt(members)
    check_pairs(members, 0.0, dt, [(0, 5)])
    check_pairs(members, 0.0, dt, [(0, 1)])
    check_pairs([params_like(m, just_diffusion=1) for m in members], 0.0, dt, [(0, 5)])


@pytest.mark.parametrize("nx,ny", [(64, 33), (61, 33), (229, 13), (490, 33)])
def test_fp32_pairs(gpu_device, nx, ny):
    """fp32: two columns per lane on an even nx (64; 490: five strips of 112, a partly filled last block), one on an odd one (61; 229:
    five strips of 48)."""
    members = fhn_across_hopf(nx, ny, "f32")
    dt = safe_dt(members)
    check_pairs(members, 0.0, dt, [(0, 5)])
    check_pairs(members, 0.0, dt, [(0, 1)])
    gb = crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, 0.4, ny=ny, precision="f32")
    check_pairs([gb, params_like(gb, beta=0.6)], 0.0, safe_dt([gb]), [(0, 5)])


def test_flat_surface_pairs(gpu_device):
    members = fhn_across_hopf(70, 0, surface="flat")
    check_pairs(members, 0.0, safe_dt(members), [(0, 5)])


def absorbing_members(nx, ny, dt, precision="f64", model="fhn"):
    """tBoundary in units of dt, for a call that starts at t0 = 0 and steps pairs (0, 1), (2, 3), ...: absorbs in both steps of every
    pair; stops between the first and the second step of pair (2, 3) (stage times 2 / 2.5 / 2.5 / 3 | 3 / 3.5 / 3.5 / 4 dt: tBoundary
    3 dt -- strict <, so stage 4 of step 2 at 3 dt itself is already off, the whole second step is); stops inside a step, between
    its stages (2.25 dt: stage 1 of step 2 on, stages 2 - 4 off); never absorbs."""
    if model == "fhn":
        base = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, beta_min=0.7, beta_max=1.7, precision=precision)
    else:
        base = crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, 0.4, ny=ny, precision=precision)
    return [params_like(base, t_boundary=100 * dt), params_like(base, beta=0.9 * base.beta, t_boundary=3 * dt), params_like(base, diffusion=0.08, t_boundary=2.25 * dt),
            params_like(base, t_boundary=0.0), params_like(base, beta=1.1 * base.beta, t_boundary=2.75 * dt)]


@pytest.mark.parametrize("model,precision,nx,ny", [("fhn", "f64", 61, 13), ("fhn", "f64", 130, 200), ("goldbeter", "f64", 100, 40), ("goldbeter", "f64", 100, 200),
                                                    ("fhn", "f32", 64, 13), ("fhn", "f32", 61, 200)])
def test_absorbing_rows_per_member_and_stage(gpu_device, model, precision, nx, ny):
    """One launch holds members that absorb in both steps, stop between the steps of a pair, stop between the stages of a step, and
    never absorb.  ny = 13 / 40: every chunk's rows and aprons meet row 0 or ny - 1 (the body with the selects everywhere); ny = 200:
    interior chunks run the body without them beside boundary chunks that run it with."""
    dt = safe_dt(absorbing_members(nx, ny, 1.0, precision, model))
    members = absorbing_members(nx, ny, dt, precision, model)
    check_pairs(members, 0.0, dt, [(0, 6)])
    check_pairs(members, 0.0, dt, [(0, 3), (3, 4)])  # (the second call's pairs start at an odd step: the switch-offs fall elsewhere in them)


@pytest.mark.parametrize("model,count", [("fhn", 64), ("fhn", 32), ("fhn", 16), ("goldbeter", 64)])
def test_tall_chunks_of_the_plan(gpu_device, model, count):
    """The item heights the plan is meant to run at.  ensemble_pair_plan starts from 128 rows and halves while all members together give
    fewer than two rounds of resident blocks -- 2 x 768 on an MI355X (256 CUs x 3 four-wavefront blocks at three wavefronts per SIMD).
    150 x 4000 members -- four strips of 48 columns, or one block strip of 240: one block per chunk -- keep 128-row chunks at B = 64
    (64 x 32 = 2048 blocks, the last chunk of each member 32 rows), get 64 at B = 32 (32 x 63) and 32 at B = 16 (16 x 125).  Every member
    against single steps of the same ensemble; members from both ends and the middle against lone contexts.  Some members absorb, one
    stops between the steps of the second pair: at these heights most chunks are interior ones beside the two boundary chunks."""
    if model == "fhn":
        base = crd.make_params("fhn", "torus", 150, 80.0, 20.0, 0.12, 1.25, ny=4000, beta_min=0.7, beta_max=1.7)
        betas = np.linspace(0.6, 1.4, count)
    else:
        base = crd.make_params("goldbeter", "torus", 150, 80.0, 20.0, 0.12, 0.4, ny=4000)
        betas = np.linspace(0.3, 0.75, count)
    dt = 0.8 * crd.stable_dt(base)
    members = [params_like(base, beta=float(b), t_boundary=(0.0, 100 * dt, 3 * dt)[k % 3]) for k, b in enumerate(betas)]
    assert crd.grid_of(base).ny == 4000
    rng = np.random.default_rng(7)
    y0 = crd.initial_conditions(crd.run_config(base, wave_length=0.1, wave_width=0.5, wave_inside=0))
    noise = 0.05 * rng.standard_normal(y0.shape)
    ys = [y0 + np.roll(noise, 61 * k, axis=0) for k in range(count)]  # (one draw, shifted per member: no two members start alike)
    calls = [(0, 5)]
    pairs = stepped(members, ys, 0.0, dt, calls, 2)
    singles = stepped(members, ys, 0.0, dt, calls, 1)
    for k in range(count):
        assert np.array_equal(pairs[k], singles[k]), ("member", k, float(np.max(np.abs(pairs[k] - singles[k]))))
    for k in (0, 1, count // 2, count - 1):
        assert np.array_equal(pairs[k], lone(members[k], ys[k], 0.0, dt, calls, ONE_STEP_PLAN)), ("member", k, "against a lone context")


def test_members_are_independent_and_runs_repeat(gpu_device):
    dt = safe_dt(absorbing_members(61, 33, 1.0))
    members = absorbing_members(61, 33, dt)
    ys = states(members)
    first = stepped(members, ys, 0.0, dt, [(0, 7)], 2)
    again = stepped(members, ys, 0.0, dt, [(0, 7)], 2)
    for k in range(len(members)):
        assert np.array_equal(first[k], again[k]), k
    other = list(members)
    other[1] = params_like(members[1], beta=0.8, diffusion=0.2, t_boundary=5 * dt)
    moved = stepped(other, ys, 0.0, dt, [(0, 7)], 2)
    assert not np.array_equal(first[1], moved[1])
    for k in (0, 2, 3, 4):
        assert np.array_equal(first[k], moved[k]), k


def observed(members, ys, dt, nsteps, stride, steps_per_launch, calls):
    with crd.Ensemble(members) as e:
        e.set_steps_per_launch(steps_per_launch)
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.observe(stride=stride, probes=[(3, 4), (17, 11)], maps=True, threshold=0.1, capacity=nsteps, sections=[("column", 5)], cycles=True, cycle_threshold=0.05)
        for a, b in calls:
            e.step_rk4(a * dt, dt, b)
        ob = e.observations()
        out = {"t": ob["t"], "stats": ob["stats"], "probes": ob["probes"], "section": e.observed_section(0)}
        for k in range(len(members)):
            out["maps%d" % k] = np.stack(e.observed_maps(k))
            c = e.observed_cycles(k)
            out["cycles%d" % k] = (c[0], c[1], c[2])
            out["state%d" % k] = e.download(k)
        e.end_observe()
    return out


@pytest.mark.parametrize("stride", [3, 2, 1])
def test_observers_record_what_single_steps_record(gpu_device, stride):
    """12 steps.  Stride 3: pair, single | pair, single | ... (the step that completes a stride goes alone); stride 2: pairs throughout,
    a sample behind each -- and, in two calls of 5 and 7 steps, a single at the end of the first call and one at the start of the second
    (the count carries over); stride 1: singles.  Samples, their times,
    probes, maps, the column section and the cycle maps: the arrays of the steps = 1 run exactly."""
    members = fhn_across_hopf(61, 33)
    dt = safe_dt(members)
    ys = states(members)
    for calls in ([(0, 12)], [(0, 5), (5, 7)]):
        one = observed(members, ys, dt, 12, stride, 1, calls)
        two = observed(members, ys, dt, 12, stride, 2, calls)
        assert len(one["t"]) == 12 // stride
        for key in one:
            if key.startswith("cycles"):
                for a, b in zip(one[key], two[key]):
                    assert np.array_equal(a, b, equal_nan=True), key
            else:
                assert np.array_equal(one[key], two[key], equal_nan=True), key


def test_switching_between_settings(gpu_device):
    members = fhn_across_hopf(130, 21)
    dt = safe_dt(members)
    ys = states(members)
    want = stepped(members, ys, 0.0, dt, [(0, 5)], 1)
    for first, second in ((2, 1), (1, 2)):
        with crd.Ensemble(members) as e:
            for k, y in enumerate(ys):
                e.upload(k, y)
            e.set_steps_per_launch(first)
            e.step_rk4(0.0, dt, 3)
            e.set_steps_per_launch(second)
            assert e.steps_per_launch == second
            e.step_rk4(3 * dt, dt, 2)
            for k in range(len(members)):
                assert np.array_equal(e.download(k), want[k]), (first, second, k)


def test_integrate_adaptive_after_pairs_as_after_singles(gpu_device):
    members = fhn_across_hopf(61, 33)
    dt = safe_dt(members)
    ys = states(members)
    got = {}
    for n in (1, 2):
        with crd.Ensemble(members) as e:
            e.set_steps_per_launch(n)
            for k, y in enumerate(ys):
                e.upload(k, y)
            e.step_rk4(0.0, dt, 4)
            stats = e.integrate_adaptive(4 * dt, 4 * dt + 0.05, rtol=1e-5, atol=1e-8)
            got[n] = (stats, [e.download(k) for k in range(len(members))])
    for k in range(len(members)):
        assert got[1][0][k] == got[2][0][k], (k, got[1][0][k], got[2][0][k])  # (the first-step estimate, every step size and count)
        assert np.array_equal(got[1][1][k], got[2][1][k]), k


def test_refusals_leave_the_ensemble_stepping_singles(gpu_device):
    EINVAL = crd._capi.EINVAL
    L = crd._capi.lib()
    for ny, refused in [(n, True) for n in sorted({8, MIN_ROWS - 1})] + [(MIN_ROWS, False)]:  # (ny = 8, and one row below the bound where that is another)
        members = fhn_across_hopf(61, ny)
        dt = safe_dt(members)
        ys = states(members)
        want = stepped(members, ys, 0.0, dt, [(0, 3)], 1)
        with crd.Ensemble(members) as e:
            for k, y in enumerate(ys):
                e.upload(k, y)
            for bad in (3, 0, -1):
                assert L.crd_ensemble_set_steps_per_launch(e.handle, bad) == EINVAL
                assert "1 or 2" in e.last_error() and str(bad) in e.last_error(), e.last_error()
                assert e.steps_per_launch == 1
            rc = L.crd_ensemble_set_steps_per_launch(e.handle, 2)
            if refused:
                assert rc == EINVAL and str(MIN_ROWS) in e.last_error() and "rows" in e.last_error(), e.last_error()
                with pytest.raises(crd.CrdError):
                    e.set_steps_per_launch(2)
                assert e.steps_per_launch == 1
            else:
                assert rc == 0 and e.steps_per_launch == 2
                assert L.crd_ensemble_set_steps_per_launch(e.handle, 3) == EINVAL and e.steps_per_launch == 2  # (a refusal changes nothing)
                e.set_steps_per_launch(1)
            e.step_rk4(0.0, dt, 3)
            for k in range(len(members)):
                assert np.array_equal(e.download(k), want[k]), (ny, k)
    assert L.crd_ensemble_get_steps_per_launch(None) == EINVAL and L.crd_ensemble_set_steps_per_launch(None, 2) == EINVAL


def test_driver_pairs_write_the_files_single_steps_write(gpu_device, tmp_path):
    ini = write_ini(tmp_path / "base.ini")
    outs = {}
    for name, extra in (("one", []), ("two", ["--ensemble-steps", "2"]), ("explicit_one", ["--ensemble-steps", "1"])):
        (tmp_path / name).mkdir()
        r = crd_run(["--ensemble", "beta=0.9,1.25", "--dt", "0.02", "--outdir", str(tmp_path / name)] + extra + [ini], tmp_path)
        assert r.returncode == 0, r.stderr
        outs[name] = tmp_path / name
    for k in range(2):
        same_files(str(outs["two"] / ("member_%d" % k)), str(outs["one"] / ("member_%d" % k)))
        same_files(str(outs["explicit_one"] / ("member_%d" % k)), str(outs["one"] / ("member_%d" % k)))
    # ... and the run says what it did
    r = subprocess.run([os.path.join(ROOT, "crdmodel_amd", "bin", "crd_run"), "--model", "fhn", "--surface", "torus", "--ensemble", "beta=0.9,1.25", "--ensemble-steps", "2", "--dt",
                        "0.02", "--outdir", str(tmp_path / "two"), ini], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "two steps per launch" in r.stdout, (r.stdout, r.stderr)


SMALL_CASES = [(m, p, nx) for m in ("fhn", "goldbeter", "diffusion_only") for p, nx in (("f64", 131), ("f32", 131), ("f32", 244))]


@pytest.mark.parametrize("model,precision,nx", SMALL_CASES)
def test_smallest_shapes_of_the_shared_setup(gpu_device, model, precision, nx):
    """crd_ensemble_pair_kernel on nx = 131 / 244 by ny = 41: 8-row chunks, chunk 2 clear of the 8-row apron on both sides.  tBoundary =
    1.5 dt: the pair (0, 1) launches the absorbing instantiation with a member that never absorbs beside one that does, the pair (2, 3)
    the plain one."""
    members, dt = two_small_members(model, precision, nx, 41, 1.5)
    check_pairs(members, 0.0, dt, [(0, 5)])
