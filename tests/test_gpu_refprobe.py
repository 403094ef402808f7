"""The HIP path against the reference's own compiled f() (tests/golden/refprobe_*.npz), with no oracle in between.

tests/test_refprobe_host.py ties the oracle to these fixtures bit for bit; here the kernels meet the same rows: f() per point in fp64
and fp32 on one slab and on three, one RK4 step of the staged stepper and the one-step kernels from the reference's initial row,
runs to each output time of the reference's fixed-step RK4 runs at one, two and three steps per launch, and the driver's files.
Bounds are oracle/error_bounds.py's; the trajectory gate is tests/test_gpu_parity.py::test_rk4_trajectory's.  Reads committed
fixtures only.

Worst err / bound printed on an MI355X (-s): see DESIGN.md section 2.
"""
import os
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
from conftest import rel_err
from oracle import error_bounds as eb
from test_gpu_error_bounds import DTYPE, check, one_step
from test_gpu_parity import RK4_TOL_F64
from test_refprobe_host import PROBE, RK4, fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ["fhn_torus_121", "fhn_torus_64_vb", "fhn_torus_23"]  # 121-, 64- and 23-wide


def params(fx, precision):
    p = crd._capi.Params.from_buffer_copy(fx.cfg.params)
    p.precision = {"f64": crd._capi.PRECISION_F64, "f32": crd._capi.PRECISION_F32}[precision]
    return p


def check_against_rows(case, got, row, fx, t, y, bounded, cut=None):
    """|got - the reference's row| <= bound + |row - the wide reference| per point and field: the kernel's distance from the wide value
    plus the reference program's own (which tests/test_refprobe_host.py holds inside the fp64 bound).  cut: got, row and bounded
    are a block of the grid and cut(whole) takes that block (tests/test_gpu_refranks.py); y is the whole state either way."""
    wide = eb.rhs_bound(fx.op, t, y, "f64")[0]
    if cut is not None:
        wide = cut(wide)
    worst = []
    for f, b in ((0, bounded[1]), (1, bounded[2])):
        err = np.abs(got[..., f].astype(np.longdouble) - row[..., f])
        room = b + np.abs(row[..., f] - wide[..., f]).astype(np.float64)
        bad = np.argwhere(~(err <= room))
        assert len(bad) == 0, "%s: field %d is outside the bound around the reference's row at %d point(s), first (row %d, column %d): err %.3g, room %.3g" % (
            case, f, len(bad), bad[0][0], bad[0][1], err[tuple(bad[0])], room[tuple(bad[0])])
        worst.append(float(np.max(np.where(room > 0, err / np.where(room > 0, room, 1), 0))))
    print("BOUND %s against the reference's rows: worst err/room u %.3g, v %.3g" % (case, worst[0], worst[1]))


def check_f(fx, precision, evaluate, label):
    for k, t, y64, name in fx.probes():
        y = y64.astype(DTYPE[precision])  # the probe states are float32 values: exact in both precisions
        got = evaluate(t, y)
        bounded = eb.rhs_bound(fx.op, t, y, precision)
        case = "%s %s %s probe %d (%s state, t = %g)" % (label, precision, fx.tag, k, name, t)
        check(case, got, bounded)
        check_against_rows(case, got, fx.rows[k + 1], fx, t, y64, bounded)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("tag", PROBE)
def test_f_per_point_against_the_references_rows(gpu_device, tag, precision):
    fx = fixture(tag)
    with crd.Slab(params(fx, precision)) as slab:
        check_f(fx, precision, slab.f, "tiled RHS")


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("tag", GROUPS)
def test_f_per_point_group_of_three_slabs(gpu_device, tag, precision):
    fx = fixture(tag)
    with crd.LocalGroup(params(fx, precision), 3) as grp:
        check_f(fx, precision, grp.f, "group of 3 slabs")


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("tag", RK4)
def test_one_step_from_the_references_initial_row(gpu_device, tag, precision):
    fx = fixture(tag)
    p, dt = params(fx, precision), float(fx.d["dt"])
    y = fx.rows[0].astype(DTYPE[precision])
    bounded = eb.rk4_step_bound(fx.op, 0.0, dt, y, precision)
    check("staged step %s %s" % (precision, tag), one_step(p, y, 0.0, dt, "staged"), bounded)
    for plan in ((0, 0, 1, 0), (1, 1, 2, 1)):
        check("one-step kernel %s %s plan %s" % (precision, tag, plan), one_step(p, y, 0.0, dt, "fused", plan), bounded)


def trajectory_gate(case, got, ref):
    """tests/test_gpu_parity.py::test_rk4_trajectory's gate, here against the reference's own rows."""
    e = [rel_err(got[..., f], ref[..., f]) for f in (0, 1)]
    print("TRAJECTORY %s: scaled max error u %.3g, v %.3g" % (case, e[0], e[1]))
    assert e[0] <= RK4_TOL_F64 and e[1] <= RK4_TOL_F64, (case, e)
    assert np.allclose(got[..., 0], ref[..., 0], rtol=1e-6, atol=1e-9), case


def output_times(fx):
    """(t, tout, steps) of the reference's output loop: tout += dTout, capped at tFinal."""
    cfg, dt = fx.cfg, float(fx.d["dt"])
    d_out = cfg.t_final / cfg.output_timestep
    t, tout = 0.0, d_out
    for _ in range(cfg.output_timestep):
        yield t, tout, int(round((tout - t) / dt))
        t, tout = tout, min(tout + d_out, cfg.t_final)


@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("tag", RK4)
def test_rk4_runs_land_on_the_references_rows(gpu_device, tag, steps):
    fx = fixture(tag)
    p, dt = params(fx, "f64"), float(fx.d["dt"])
    with crd.Slab(p) as slab:
        slab.set_launch_plan(0, 0, 1, 1, steps)
        # (a plan asking for more steps than the model, precision or grid allows gets what crd_steps_per_launch_on says)
        assert slab.launch_plan()["steps_per_launch"] == crd.steps_per_launch_on(str(fx.d["model"]), "f64", fx.op.nx, fx.op.ny, steps)
        slab.upload(fx.rows[0])
        for k, (t, tout, n) in enumerate(output_times(fx), start=1):
            slab.step_rk4(t, dt, n)
            trajectory_gate("%s output %d, %d step(s) per launch" % (tag, k, steps), slab.download(), fx.rows[k])


def text_row(values):
    return ("".join(" %.16e" % v for v in values.ravel()) + "\n").encode()


def test_driver_writes_the_references_files(gpu_device, tmp_path):
    """`crd_run --model fhn --surface torus --fixed --dt <the fixture's> <ini>` (the program behind bin/FHNmodel_torus, which like the
    reference takes the ini alone): the subdomain file and the initial row are the reference's bytes, the later rows pass the
    trajectory gate."""
    fx = fixture("rk4_fhn_torus_23")
    ini = tmp_path / "case.ini"
    ini.write_text(str(fx.d["ini_text"]))
    exe = os.path.join(ROOT, "crdmodel_amd", "bin", "crd_run")
    r = subprocess.run([exe, "--model", "fhn", "--surface", "torus", "--fixed", "--dt", repr(float(fx.d["dt"])), "--quiet", str(ini)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "FHNmodel_torus_subdomain.000.txt").read_bytes() == fx.d["header"].tobytes()
    for f, name in enumerate(("u", "v")):
        lines = (tmp_path / ("FHNmodel_torus_%s.000.txt" % name)).read_bytes().split(b"\n")
        assert len(lines) == fx.rows.shape[0] + 1 and lines[-1] == b"", (name, len(lines))
        assert lines[0] + b"\n" == text_row(fx.rows[0][..., f]), "initial row of %s" % name
    got = np.stack([np.loadtxt(tmp_path / ("FHNmodel_torus_%s.000.txt" % name)).reshape(fx.rows.shape[:-1]) for name in ("u", "v")], axis=-1)
    for k in range(1, fx.rows.shape[0]):
        trajectory_gate("driver output %d" % k, got[k], fx.rows[k])
