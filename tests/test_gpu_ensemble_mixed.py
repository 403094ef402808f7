"""Mixed-geometry ensembles on the GPU (crd_ensemble_create_mixed, crdmodel_amd.Ensemble(..., mixed=True)): members of different
surface, nx and ny in one launch, every member's state bit-identical to a context of its parameters stepped alone with the one-launch
stepper -- at one and two steps per launch, in any member order -- and its observer row, probes and maps bit-identical to a uniform
ensemble of that member alone.  Every comparison is np.array_equal.  The shapes are the smallest that reach every branch of the block
mapping: a wavefront holds 56 valid columns in fp64 single steps (120 with two columns per lane), 48 (112) in pairs, a block 240
where it is the strip (Goldbeter fp64 pairs)."""
import copy
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

EINVAL = crd._capi.EINVAL
DT = 0.02


def params_like(p, **kw):
    q = copy.copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def dtype_of(p):
    return np.float64 if p.precision == crd._capi.PRECISION_F64 else np.float32


def start_state(p, seed):
    cfg = crd.run_config(p, wave_length=0.1, wave_width=0.5, wave_inside=0)
    y = crd.initial_conditions(cfg)
    y = y + 0.05 * np.random.default_rng(seed).standard_normal(y.shape)
    return y.astype(dtype_of(p))


def lone(p, y0, calls, observe=False):
    """A context of p stepped alone with the one-launch stepper: calls = [(first step, steps), ...]."""
    with crd.Slab(p) as s:
        s.set_stepper("fused")
        s.set_autotune(0)
        s.set_launch_plan(0, 0, 1, 0, 1)
        s.upload(y0)
        for a, b in calls:
            s.step_rk4(a * DT, DT, b)
        y = s.download(dtype_of(p))
        return (y, s.observe()) if observe else y


_LONE = {}


def lone_cached(key, p, y0, calls):
    k = (key, tuple(calls))
    if k not in _LONE:
        _LONE[k] = lone(p, y0, calls)
    return _LONE[k]


def run_mixed(members, ys, calls, steps_per_launch=1):
    with crd.Ensemble(members, mixed=True) as e:
        for k, y in enumerate(ys):
            assert (e.grid(k).nx, e.grid(k).ny) == (members[k].nx, members[k].ny)
            e.upload(k, y)
        if steps_per_launch != 1:
            e.set_steps_per_launch(steps_per_launch)
        for a, b in calls:
            e.step_rk4(a * DT, DT, b)
        assert all(np.isfinite(m) for m in e.max_abs())
        return [e.download(k, dtype_of(members[k])) for k in range(len(members))]


def fhn_set(precision="f64", t_far=10.0):
    def mk(surface, nx, ny, beta=1.25, **kw):
        return crd.make_params("fhn", surface, nx, 80.0, 20.0, 0.12, beta, ny=ny, beta_min=0.7, beta_max=1.7, precision=precision, **kw)
    # one strip; two strips; five strips (two blocks per chunk row, the second with surplus wavefronts) absorbing throughout; three
    # strips; the smallest member again, last, with another beta
    return [mk("torus", 40, 9), mk("flat", 57, 37, t_boundary=0.05), mk("torus", 230, 70, t_boundary=t_far), mk("flat", 113, 16),
            mk("torus", 40, 9, beta=0.9)]


CALLS = {1: [(0, 1)], 2: [(0, 2)], 5: [(0, 2), (2, 3)], 6: [(0, 5), (5, 1)], 11: [(0, 5), (5, 6)]}


@pytest.fixture(scope="module")
def fhn_case():
    members = fhn_set()
    return members, [start_state(p, k) for k, p in enumerate(members)]


@pytest.mark.parametrize("spl", [1, 2])
@pytest.mark.parametrize("steps", [1, 2, 5, 6])
def test_fhn_fp64_members_bit_identical(gpu_device, fhn_case, steps, spl):
    members, ys = fhn_case
    got = run_mixed(members, ys, CALLS[steps], spl)
    for k, p in enumerate(members):
        want = lone_cached(("fhn", k), p, ys[k], CALLS[steps])
        assert got[k].shape == (p.ny, p.nx, 2)
        assert np.array_equal(got[k], want), ("member", k, float(np.max(np.abs(got[k] - want))))


@pytest.mark.parametrize("spl", [1, 2])
def test_boundary_time_between_the_two_steps_of_a_pair(gpu_device, spl):
    """tBoundary = 0.03: the first step of the pair (stages at 0 .. 0.02) absorbs, the second (0.02 .. 0.04) partly."""
    members = fhn_set(t_far=0.03)
    ys = [start_state(p, 10 + k) for k, p in enumerate(members)]
    got = run_mixed(members, ys, CALLS[6], spl)
    for k, p in enumerate(members):
        assert np.array_equal(got[k], lone(p, ys[k], CALLS[6])), ("member", k)


@pytest.mark.parametrize("spl", [1, 2])
@pytest.mark.parametrize("widths", [(40, 122, 242), (40, 57, 242)])
def test_fp32_two_columns_and_one(gpu_device, widths, spl):
    """Even widths take two columns per lane; one odd width forces one column per lane for all."""
    members = [crd.make_params("fhn", s, nx, 80.0, 20.0, 0.12, 1.25, ny=ny, precision="f32", t_boundary=tb)
               for s, nx, ny, tb in zip(("torus", "flat", "torus"), widths, (9, 37, 70), (0.0, 0.05, 10.0))]
    ys = [start_state(p, 20 + k) for k, p in enumerate(members)]
    got = run_mixed(members, ys, CALLS[5], spl)
    for k, p in enumerate(members):
        assert got[k].dtype == np.float32
        assert np.array_equal(got[k], lone(p, ys[k], CALLS[5])), ("member", k)


@pytest.mark.parametrize("spl", [1, 2])
def test_goldbeter_fp64_block_strip(gpu_device, spl):
    """Pairs run the block as the strip: 240 valid columns of four wavefronts' 256; a 40-wide member's block has three wavefronts wholly
    beyond its nx, a 241-wide one a second block of one column."""
    members = [crd.make_params("goldbeter", s, nx, 80.0, 20.0, 0.12, b, ny=ny, t_boundary=tb)
               for s, nx, ny, b, tb in zip(("torus", "flat", "torus", "flat"), (40, 100, 241, 500), (9, 33, 70, 20), (0.4, 0.5, 0.2, 0.9), (0.0, 10.0, 0.05, 10.0))]
    ys = [start_state(p, 30 + k) for k, p in enumerate(members)]
    got = run_mixed(members, ys, CALLS[5], spl)
    for k, p in enumerate(members):
        assert np.array_equal(got[k], lone(p, ys[k], CALLS[5])), ("member", k)


def test_diffusion_only(gpu_device):
    members = [crd.make_params("goldbeter", s, nx, 80.0, 20.0, d, 0.4, ny=ny, just_diffusion=1) for s, nx, ny, d in (("torus", 61, 12, 0.12), ("flat", 130, 40, 0.2))]
    ys = [start_state(p, 40 + k) for k, p in enumerate(members)]
    got = run_mixed(members, ys, CALLS[5])
    for k, p in enumerate(members):
        assert np.array_equal(got[k], lone(p, ys[k], CALLS[5])), ("member", k)


@pytest.mark.parametrize("spl", [1, 2])
def test_member_order_does_not_matter(gpu_device, fhn_case, spl):
    members, ys = fhn_case
    fwd = run_mixed(members, ys, CALLS[5], spl)
    rev = run_mixed(members[::-1], ys[::-1], CALLS[5], spl)[::-1]
    for k in range(len(members)):
        assert np.array_equal(fwd[k], rev[k]), ("member", k)


def test_equal_shapes_are_an_ordinary_ensemble(gpu_device):
    """Members of one shape through create_mixed: the results of crd.Ensemble(members); integrate_adaptive and sections are accepted."""
    base = crd.make_params("fhn", "torus", 61, 80.0, 20.0, 0.12, 1.25, ny=24, beta_min=0.7, beta_max=1.7)
    members = [base, params_like(base, beta=0.9, t_boundary=0.05), params_like(base, diffusion=0.2)]
    ys = [start_state(p, 50 + k) for k, p in enumerate(members)]
    out = {}
    for mixed in (False, True):
        with crd.Ensemble(members, mixed=mixed) as e:
            for k, y in enumerate(ys):
                e.upload(k, y)
            e.observe(stride=1, sections=[("row", 3), ("theta_mean",)], capacity=8)
            e.step_rk4(0.0, DT, 3)
            sec = e.observed_section(1)
            e.end_observe()
            st = e.integrate_adaptive(3 * DT, 3 * DT + 0.05)
            assert all(d["status"] == crd._capi.OK for d in st)
            out[mixed] = ([e.download(k) for k in range(3)], sec)
    for k in range(3):
        assert np.array_equal(out[True][0][k], out[False][0][k]), ("member", k)
    assert np.array_equal(out[True][1], out[False][1])


def test_tables_are_each_members_own(gpu_device):
    """Torus and flat at one 64 x 32 mesh: one shape, two geometries -- wrong if the tables are built from member 0's grid."""
    members = [crd.make_params("fhn", s, 64, 80.0, 20.0, 0.12, 1.25, ny=32, beta_min=0.7, beta_max=1.7, vary_beta=1) for s in ("torus", "flat")]
    ys = [start_state(p, 60 + k) for k, p in enumerate(members)]
    got = run_mixed(members, ys, CALLS[5])
    for k, p in enumerate(members):
        assert np.array_equal(got[k], lone(p, ys[k], CALLS[5])), ("member", k)
    assert not np.array_equal(got[0], lone(members[1], ys[0], CALLS[5]))  # (the two geometries do differ)


@pytest.mark.parametrize("stride", [1, 3])
def test_observer_rows_probes_and_maps(gpu_device, fhn_case, stride):
    members, ys = fhn_case
    probes, steps, thr = [(3, 2), (39, 8)], 6, 0.1
    with crd.Ensemble(members, mixed=True) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.observe(stride=stride, probes=probes, maps=True, threshold=thr, capacity=8)
        e.step_rk4(0.0, DT, 4)
        e.step_rk4(4 * DT, DT, 2)
        obs = e.observations()
        maps = [e.observed_maps(k) for k in range(len(members))]
        e.end_observe()
    assert obs["stats"].shape[0] == steps // stride
    for k, p in enumerate(members):
        with crd.Ensemble([p]) as one:
            one.upload(0, ys[k])
            one.observe(stride=stride, probes=probes, maps=True, threshold=thr, capacity=8)
            one.step_rk4(0.0, DT, 4)
            one.step_rk4(4 * DT, DT, 2)
            want = one.observations()
            wmaps = one.observed_maps(0)
        assert np.array_equal(obs["t"], want["t"])
        assert np.array_equal(obs["stats"][:, k], want["stats"][:, 0], equal_nan=True), ("member", k)
        assert np.array_equal(obs["probes"][:, k], want["probes"][:, 0]), ("member", k)
        assert np.array_equal(obs["mean"][:, k], want["mean"][:, 0]), ("member", k)
        for q in range(3):
            assert maps[k][q].shape == (p.ny, p.nx)
            assert np.array_equal(maps[k][q], wmaps[q], equal_nan=True), ("member", k, "map", q)
        # ... and the last row is crd_state_observe's of the lone context
        last = (steps // stride) * stride
        _, row = lone(p, ys[k], [(0, last)], observe=True)
        assert np.array_equal(obs["stats"][last // stride - 1, k], row), ("member", k)


def test_refusals_leave_the_ensemble_stepping(gpu_device):
    mk = lambda nx, ny: crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny)
    members = [mk(61, 8), mk(40, 20)]
    ys = [start_state(p, 70 + k) for k, p in enumerate(members)]
    with crd.Ensemble(members, mixed=True) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)

        def refused(call, *words):
            with pytest.raises(crd.CrdError) as err:
                call()
            assert err.value.status == EINVAL, err.value
            for w in words:
                assert w in e.last_error(), (w, e.last_error())

        refused(lambda: e.integrate_adaptive(0.0, 0.1), "members of different shape")
        refused(lambda: e.observe(sections=[("row", 1)]), "members of different shape", "section")
        refused(lambda: e.observe(cycles=True), "members of different shape", "cycle")
        refused(lambda: e.set_steps_per_launch(2), "member 0", "8")
        assert e.steps_per_launch == 1
        refused(lambda: e.observe(probes=[(50, 3)]), "probe 0", "member 1")
        refused(lambda: e.observe(probes=[(3, 3), (3, 10)]), "probe 1", "member 0")
        e.step_rk4(0.0, DT, 3)
        for k, p in enumerate(members):
            assert np.array_equal(e.download(k), lone(p, ys[k], [(0, 3)])), ("member", k)


BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
SMALL_INI = os.path.join(GOLDEN, "ini", "small_run.ini")


def write_ini(path, **overrides):
    out = []
    for line in open(SMALL_INI).read().splitlines():
        key = line.split("=")[0].strip()
        out.append("%s = %s" % (key, overrides[key]) if key in overrides else line)
    path.write_text("\n".join(out) + "\n")
    return str(path)


def crd_run(surface, args, cwd):
    return subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", surface, "--quiet"] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def same_files(a, b):
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b)), (names, sorted(os.listdir(b)))
    _, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


@pytest.mark.parametrize("keys,lone_runs", [
    (["surfaceLength=80,40", "surface=torus,flat"], [("torus", {"surfaceLength": "80"}), ("flat", {"surfaceLength": "40"})]),
    # ... and members of different nx (the ini pins ny by phiMesh): the mixed launches, two steps per launch
    (["xMesh=16,24", "surfaceLength=80,40"], [("torus", {"thetaMesh": "16", "surfaceLength": "80"}), ("torus", {"thetaMesh": "24", "surfaceLength": "40"})]),
])
def test_driver_members_write_what_lone_runs_write(gpu_device, tmp_path, keys, lone_runs):
    (tmp_path / "ens").mkdir()
    args = []
    for k in keys:
        args += ["--ensemble", k]
    if keys[0].startswith("xMesh"):
        args += ["--ensemble-steps", "2"]
    r = crd_run("torus", args + ["--dt", "0.02", "--outdir", str(tmp_path / "ens"), SMALL_INI], tmp_path)
    assert r.returncode == 0, r.stderr
    for k, (surface, overrides) in enumerate(lone_runs):
        lone_dir = tmp_path / ("lone%d" % k)
        lone_dir.mkdir()
        r = crd_run(surface, ["--dt", "0.02", "--outdir", str(lone_dir), write_ini(tmp_path / ("m%d.ini" % k), **overrides)], tmp_path)
        assert r.returncode == 0, r.stderr
        same_files(str(tmp_path / "ens" / ("member_%d" % k)), str(lone_dir))


def small_mixed_set(model, precision, even):
    """131 x 41 (three strips), 60 x 25 (one strip: narrower than the block, surplus wavefronts), 131 x 9 (the pair kernels' minimum
    height); even: 132 wide, so that fp32 takes two columns per lane.  The first member absorbs until 1.5 DT, the others never."""
    w = 132 if even else 131
    def mk(nx, ny, beta, tb):
        if model == "fhn":
            return crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, beta, ny=ny, beta_min=0.7, beta_max=1.7, precision=precision, t_boundary=tb)
        return crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, 0.4 * beta, ny=ny, precision=precision, t_boundary=tb, just_diffusion=int(model == "diffusion_only"))
    return [mk(w, 41, 1.25, 1.5 * DT), mk(60, 25, 1.0, 0.0), mk(w, 9, 0.9, 0.0)]


SMALL_MIXED_CASES = [(m, p, e) for m in ("fhn", "goldbeter", "diffusion_only") for p, e in (("f64", False), ("f32", False), ("f32", True))]


@pytest.mark.parametrize("spl", [1, 2])
@pytest.mark.parametrize("model,precision,even", SMALL_MIXED_CASES)
def test_smallest_shapes_of_the_shared_setup(gpu_device, monkeypatch, model, precision, even, spl):
    """crd_ensemble_step_mixed_kernel (spl = 1) and crd_ensemble_pair_mixed_kernel (spl = 2): the first launches take the absorbing
    instantiation with both bodies in one launch, the later ones the plain one.  Goldbeter's kinetics bound the RK4 step of these grids
    at 0.0066 (crd.stable_dt), so its members step at 0.005: five steps at this module's 0.02 would overflow fp32."""
    if model == "goldbeter":
        monkeypatch.setattr(sys.modules[__name__], "DT", 0.005)
    members = small_mixed_set(model, precision, even)
    ys = [start_state(p, 70 + k) for k, p in enumerate(members)]
    got = run_mixed(members, ys, CALLS[5], spl)
    for k, p in enumerate(members):
        assert np.array_equal(got[k], lone(p, ys[k], CALLS[5])), ("member", k)
