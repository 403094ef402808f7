"""Ensembles on the GPU (crd_ensemble_*, crdmodel_amd.Ensemble, crd_run --ensemble): every member bit-identical to a context of the
same parameters stepped alone with the one-launch stepper, under a pinned one-step plan and under the measured plan; the oracle on a
small grid; members independent of each other; the driver's files byte-identical to lone runs, a blown-up member stopped alone."""
import copy
import filecmp
import os
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT
from oracle import crd_oracle as co

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
INI = os.path.join(GOLDEN, "ini")


def params_like(p, **kw):
    q = copy.copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def start_state(p, seed):
    """The reference's initial state of p, perturbed per member so that no two members start alike."""
    cfg = crd.run_config(p, wave_length=0.1, wave_width=0.5, wave_inside=0)
    y = crd.initial_conditions(cfg)
    rng = np.random.default_rng(seed)
    return y + 0.05 * rng.standard_normal(y.shape)


def lone(p, y0, t0, dt, steps, plan):
    """A context of p stepped alone: plan None = the measured plan, else a pinned one (chunk mode, mapping, columns, nt, steps)."""
    with crd.Slab(p) as s:
        s.set_stepper("fused")
        if plan is None:
            s.set_autotune(1)
        else:
            s.set_autotune(0)
            s.set_launch_plan(*plan)
        s.upload(y0)
        for a, b in steps:  # (t0 + a dt, b steps) per call
            s.step_rk4(t0 + a * dt, dt, b)
        return s.download(np.float64 if p.precision == crd._capi.PRECISION_F64 else np.float32)


def check_ensemble(members, t0, dt, steps, plans=((0, 0, 1, 0, 1), None), seed=0):
    dtype = np.float64 if members[0].precision == crd._capi.PRECISION_F64 else np.float32
    ys = [start_state(p, seed + k) for k, p in enumerate(members)]
    if dtype == np.float32:
        ys = [y.astype(np.float32) for y in ys]
    with crd.Ensemble(members) as e:
        assert len(e) == len(members)
        for k, y in enumerate(ys):
            e.upload(k, y)
        for a, b in steps:
            e.step_rk4(t0 + a * dt, dt, b)
        got = [e.download(k, dtype) for k in range(len(members))]
        assert all(np.isfinite(m) for m in e.max_abs())
    for plan in plans:
        for k, p in enumerate(members):
            want = lone(p, ys[k], t0, dt, steps, plan)
            assert np.array_equal(got[k], want), ("member", k, "plan", plan, float(np.max(np.abs(got[k].astype(np.float64) - want))))
    return got


def fhn_members(nx, precision="f64", ny=0):
    base = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, beta_min=0.7, beta_max=1.7, precision=precision)
    # beta, varyBeta on / off, diffusion, tBoundary: none, inside the call between two stages of step 5 (t = 0.10: stages at 0.10 /
    # 0.11 / 0.11 / 0.12), beyond the call, at a stage time exactly
    return [params_like(base, t_boundary=0.0), params_like(base, beta=0.9, t_boundary=0.105), params_like(base, vary_beta=1, t_boundary=0.3),
            params_like(base, diffusion=0.05, t_boundary=0.11), params_like(base, diffusion=0.2, beta=1.1, t_boundary=0.17),
            params_like(base, vary_beta=1, diffusion=0.08, beta_min=0.5, beta_max=2.0, t_boundary=0.06)]


@pytest.mark.parametrize("nx", [61, 130])
def test_fhn_members_bit_identical_to_lone_contexts(gpu_device, nx):
    """Ragged nx (61, 130: not multiples of a strip's 56 valid columns), tBoundary inside the calls; two calls (the time carries over)."""
    check_ensemble(fhn_members(nx), 0.0, 0.02, [(0, 5), (5, 7)])


def test_fhn_shipped_grid_400x1600(gpu_device):
    p = crd.load_ini(os.path.join(INI, "fhn_shipped.ini"), "fhn", "torus").params
    g = crd.grid_of(p)
    assert (g.nx, g.ny) == (400, 1600)
    # (dt 0.004: under the grid's RK4 stability bound, 0.0052; tBoundary 0.01 falls between stages 1 and 2 of step 2)
    members = [params_like(p, t_boundary=0.05), params_like(p, beta=0.95, vary_beta=0, t_boundary=0.0), params_like(p, diffusion=0.06, t_boundary=0.01)]
    check_ensemble(members, 0.0, 0.004, [(0, 4), (4, 3)])


def test_goldbeter_members_and_diffusion_only(gpu_device):
    p = crd.load_ini(os.path.join(INI, "goldbeter_shipped.ini"), "goldbeter", "torus").params
    members = [params_like(p, beta=b, t_boundary=tb) for b, tb in ((0.3, 0.0), (0.5, 0.005), (0.75, 1.0))]
    check_ensemble(members, 0.0, 0.002, [(0, 6)])
    just = [params_like(m, just_diffusion=1) for m in members]
    check_ensemble(just, 0.0, 0.002, [(0, 6)])


def test_flat_surface_members(gpu_device):
    base = crd.make_params("fhn", "flat", 70, 80.0, 20.0, 0.12, 1.25, t_boundary=0.05)
    check_ensemble([base, params_like(base, beta=0.8, t_boundary=0.0), params_like(base, diffusion=0.3)], 0.0, 0.01, [(0, 9)])


@pytest.mark.parametrize("nx", [64, 61])
def test_fp32_members_even_and_odd_nx(gpu_device, nx):
    """fp32: two columns per lane on an even nx, one on an odd one -- bit-identical to fp32 contexts either way."""
    check_ensemble(fhn_members(nx, "f32")[:4], 0.0, 0.02, [(0, 8)])
    base = crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, 0.4, precision="f32", t_boundary=0.004)
    check_ensemble([base, params_like(base, beta=0.6)], 0.0, 0.002, [(0, 5)])


def members_in_steps(nx, ny, dt, precision="f64"):
    """fhn_members' variety with tBoundary in units of dt: none; between two stages of step 5 of the call (stages at 5 / 5.5 / 5.5 /
    6 dt); beyond the call; at a stage time exactly; at a step's end."""
    base = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, beta_min=0.7, beta_max=1.7, precision=precision)
    return [params_like(base, t_boundary=0.0), params_like(base, beta=0.9, t_boundary=5.25 * dt), params_like(base, vary_beta=1, t_boundary=15 * dt),
            params_like(base, diffusion=0.05, t_boundary=5.5 * dt), params_like(base, vary_beta=1, diffusion=0.08, beta_min=0.5, beta_max=2.0, t_boundary=3 * dt)]


@pytest.mark.parametrize("nx,ny", [(230, 33), (300, 9), (390, 21)])
def test_partly_filled_last_block_of_strips_fp64(gpu_device, nx, ny):
    """Five, six and seven strips of 56 columns: with sw = 4 wavefronts per block the last block of a row of strips has one, two
    and three live wavefronts, the others return in front of the body's barriers.  Short ny: 33 (one row more than whole chunks of
    4, 8, 16 or 32 rows), 9 and 21 (ny % 4 == 1).  Members differ as fhn_members' do; tBoundary falls inside the calls.
    (ensemble_plan's 32-row chunk is out of reach at test size: it needs B x blocks-per-member >= two rounds of resident blocks,
    upwards of a thousand blocks, i.e. hundreds of members of a grid this small, each of them then stepped alone twice by
    check_ensemble.  The grids here get its 4-row chunks.)"""
    dt = 0.8 * min(crd.stable_dt(p) for p in members_in_steps(nx, ny, 1.0))
    check_ensemble(members_in_steps(nx, ny, dt), 0.0, dt, [(0, 5), (5, 3)])


@pytest.mark.parametrize("nx,ny", [(490, 33), (229, 13)])
def test_partly_filled_last_block_of_strips_fp32(gpu_device, nx, ny):
    """fp32: even nx = 490, five strips of 120 columns with two columns per lane; odd nx = 229, five strips of 56 with one."""
    dt = 0.8 * min(crd.stable_dt(p) for p in members_in_steps(nx, ny, 1.0, "f32"))
    check_ensemble(members_in_steps(nx, ny, dt, "f32"), 0.0, dt, [(0, 5), (5, 3)])


def test_two_members_match_the_oracle(gpu_device):
    nx, dt, n = 32, 0.02, 10
    members = [crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, t_boundary=0.1),
               crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.2, 0.9, t_boundary=0.0)]
    got = check_ensemble(members, 0.0, dt, [(0, n)], plans=())
    for k, (p, y) in enumerate(zip(members, got)):
        op = co.make_problem(co.FHN, co.TORUS, nx, 80.0, 20.0, p.diffusion, p.beta, t_boundary=p.t_boundary)
        want = co.rk4(op, start_state(p, k), 0.0, dt, n)
        assert float(np.max(np.abs(y - want)) / np.max(np.abs(want))) <= 1e-12, k


def test_members_are_independent(gpu_device):
    members = fhn_members(61)
    ys = [start_state(p, k) for k, p in enumerate(members)]
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.step_rk4(0.0, 0.02, 8)
        first = [e.download(k) for k in range(len(members))]
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.upload(2, start_state(members[2], 99))  # a new state for member 2 only
        e.step_rk4(0.0, 0.02, 8)
        second = [e.download(k) for k in range(len(members))]
    for k in range(len(members)):
        if k == 2:
            assert not np.array_equal(first[k], second[k])
        else:
            assert np.array_equal(first[k], second[k]), k


def test_one_member_is_a_context(gpu_device):
    check_ensemble(fhn_members(130)[1:2], 0.0, 0.02, [(0, 9)])


def test_64_goldbeter_members(gpu_device):
    """B = 64 of the shipped 100 x 400 Goldbeter grid: member indices beyond one round of the XCDs; a sample against lone contexts."""
    p = crd.load_ini(os.path.join(INI, "goldbeter_shipped.ini"), "goldbeter", "torus").params
    betas = np.linspace(0.2, 0.9, 64)
    members = [params_like(p, beta=float(b), t_boundary=(0.004 if k % 3 == 0 else 0.0)) for k, b in enumerate(betas)]
    ys = [start_state(m, k) for k, m in enumerate(members)]
    dt, n = 0.002, 5
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.step_rk4(0.0, dt, n)
        for k in (0, 1, 7, 8, 31, 33, 62, 63):
            assert np.array_equal(e.download(k), lone(members[k], ys[k], 0.0, dt, [(0, n)], (0, 0, 1, 0, 1))), k


def write_ini(path, **overrides):
    lines = open(os.path.join(INI, "small_run.ini")).read().splitlines()
    out = []
    for line in lines:
        key = line.split("=")[0].strip()
        out.append("%s = %s" % (key, overrides[key]) if key in overrides else line)
    path.write_text("\n".join(out) + "\n")
    return str(path)


def crd_run(args, cwd):
    return subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus", "--quiet"] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def same_files(a, b):
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b)), (names, sorted(os.listdir(b)))
    _, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


def test_driver_members_write_what_lone_runs_write(gpu_device, tmp_path):
    ini = write_ini(tmp_path / "base.ini")
    (tmp_path / "ens").mkdir()
    r = crd_run(["--ensemble", "beta=0.9,1.25", "--dt", "0.02", "--outdir", str(tmp_path / "ens"), ini], tmp_path)
    assert r.returncode == 0, r.stderr
    for k, beta in enumerate(("0.9", "1.25")):
        lone_dir = tmp_path / ("lone%d" % k)
        lone_dir.mkdir()
        r = crd_run(["--dt", "0.02", "--outdir", str(lone_dir), write_ini(tmp_path / ("m%d.ini" % k), beta=beta)], tmp_path)
        assert r.returncode == 0, r.stderr
        same_files(str(tmp_path / "ens" / ("member_%d" % k)), str(lone_dir))


def test_driver_stops_a_blown_up_member_alone(gpu_device, tmp_path):
    ini = write_ini(tmp_path / "base.ini")
    (tmp_path / "ens").mkdir()
    r = crd_run(["--ensemble", "diffusion=0.12,5000", "--dt", "0.02", "--outdir", str(tmp_path / "ens"), ini], tmp_path)
    assert r.returncode == 1 and "member 1" in r.stderr, (r.returncode, r.stderr)
    for k, d in enumerate(("0.12", "5000")):
        lone_dir = tmp_path / ("lone%d" % k)
        lone_dir.mkdir()
        r = crd_run(["--dt", "0.02", "--outdir", str(lone_dir), write_ini(tmp_path / ("m%d.ini" % k), diffusion=d)], tmp_path)
        assert r.returncode == (0 if k == 0 else 1), r.stderr
        same_files(str(tmp_path / "ens" / ("member_%d" % k)), str(lone_dir))


def two_small_members(model, precision, nx, ny, tb_in_dt):
    """Two members of the smallest shapes that reach every branch of the work-item set-up: one absorbs until tb_in_dt steps into the
    call, one never does, so one launch runs both bodies and later launches take the select-free kernel.  Returns (members, dt)."""
    if model == "fhn":
        base = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, beta_min=0.7, beta_max=1.7, precision=precision)
    else:
        base = crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, 0.4, ny=ny, precision=precision, just_diffusion=int(model == "diffusion_only"))
    dt = 0.8 * crd.stable_dt(base)
    return [params_like(base, t_boundary=tb_in_dt * dt), params_like(base, beta=0.9 * base.beta, t_boundary=0.0)], dt


SMALL_CASES = [(m, p, nx) for m in ("fhn", "goldbeter", "diffusion_only") for p, nx in (("f64", 131), ("f32", 131), ("f32", 244))]


@pytest.mark.parametrize("model,precision,nx", SMALL_CASES)
def test_smallest_shapes_of_the_shared_setup(gpu_device, model, precision, nx):
    """crd_ensemble_step_kernel on nx = 131 (three strips of 56, the last partial, one column per lane) or 244 (fp32: three strips of
    120, two columns per lane) by ny = 21: six 4-row chunks, chunk 2 wholly interior, chunks 0 and 5 at the boundary.  tBoundary = 1.5 dt:
    steps 1 and 2 launch the absorbing instantiation, step 3 the plain one."""
    members, dt = two_small_members(model, precision, nx, 21, 1.5)
    check_ensemble(members, 0.0, dt, [(0, 3)], plans=((0, 0, 1, 0, 1),))
