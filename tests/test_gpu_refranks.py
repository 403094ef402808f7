"""The HIP path against TWO- and FOUR-rank runs of the reference's own compiled code (tests/golden/refranks_*.npz), no oracle in between.

tests/test_refranks_host.py ties the oracle and the host side to these fixtures bit for bit; here the kernels meet the same rows:
f() per point in fp64 and fp32 on the reference's own process grids (crd.dims_create: 2 x 1 theta-blocks for two ranks, 2 x 2 for
four) with BLOCK k held to RANK k's rows -- which pins the rank order -- and on two and four phi-slabs (the layout the project
computes on when it writes block files) against the ranks' rows stitched by their headers; the reference's four-rank fixed-step RK4
run through 2 x 2 block contexts (staged stepper) and through four phi-slabs with the one-launch stepper; and the driver's block file
sets.  The only tolerances are oracle/error_bounds.py: rhs_bound, cut to the block, and the trajectory gate of
tests/test_gpu_parity.py (RK4_TOL_F64).  Reads committed fixtures only.

The blocks here are 6 to 12 columns wide; tests/test_gpu_theta_blocks.py holds blocks wider than one 64-column tile to the single
context.  (A fixture with such blocks does not fit the size conditions: every program derives ny >= nx, so a 130-wide grid has
16,900 points or more, 270 KB per frame and rank count.)  libcrd wants 8 rows per context, so four phi-slabs are asked of the grids
with 32 rows or more.

Worst err / bound printed on an MI355X (-s): see DESIGN.md section 2.
"""
import os
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
from oracle import error_bounds as eb
from oracle.ref_build import make_fixtures as mf
from test_gpu_error_bounds import DTYPE, check
from test_gpu_refprobe import check_against_rows, params, text_row, trajectory_gate
from test_refranks_host import PROBE, RANKS, RK4, fixture, output_times

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_ROWS = 8  # of a context (crd_create_block)


def held_to_its_rank(grp, ranks):
    """Context k of the group covers what rank k's own header says: the rank order, before anything is compared."""
    assert [(s.is_, s.ie, s.js, s.je) for s in grp.slabs] == [(r.is_, r.ie, r.js, r.je) for r in ranks]


def stitched(fx, ranks, frame):
    """One frame of the ranks' rows, placed by the extents in their own headers."""
    whole = np.full((fx.op.ny, fx.op.nx, 2), np.nan)
    for r in ranks:
        whole[r.js:r.je + 1, r.is_:r.ie + 1] = r.rows[frame]
    assert np.all(np.isfinite(whole))
    return whole


def check_f_on_parts(fx, precision, grp, parts, label):
    """f() of the group on every probe state; `parts`: the objects with extents and rows (frames, nyl, nxl, 2) each piece is held to."""
    for k, t, y64, name in fx.probes():
        y = y64.astype(DTYPE[precision])  # the probe states are float32 values: exact in both precisions
        got = grp.f(t, y)
        bounded = eb.rhs_bound(fx.op, t, y, precision)
        for q, r in enumerate(parts):
            case = "%s %s %s probe %d (%s state, t = %g), part %d of %d" % (label, precision, fx.tag, k, name, t, q, len(parts))
            cut = tuple(np.ascontiguousarray(r.cut(b[..., None])[..., 0] if b.ndim == 2 else r.cut(b)) for b in bounded)
            mine = np.ascontiguousarray(r.cut(got))
            check(case, mine, cut)
            check_against_rows(case, mine, r.rows[k + 1], fx, t, y64, cut, cut=r.cut)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("tag", PROBE)
def test_f_per_point_block_k_against_rank_k(gpu_device, tag, n, precision):
    fx = fixture(tag)
    ranks = fx.ranks(n)
    with crd.LocalGroup(params(fx, precision), n, blocks=crd.dims_create(n)) as grp:
        held_to_its_rank(grp, ranks)
        check_f_on_parts(fx, precision, grp, ranks, "%d block contexts" % n)


class Whole:
    """The ranks' rows stitched into the whole grid, with the interface of a rank."""

    def __init__(self, fx, ranks):
        self.rows = np.stack([stitched(fx, ranks, frame) for frame in range(fx.one.shape[0])])

    @staticmethod
    def cut(whole):
        return whole


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("tag", PROBE)
def test_f_per_point_phi_slabs_against_the_stitched_ranks(gpu_device, tag, n, precision):
    fx = fixture(tag)
    slabs = n if fx.op.ny >= MIN_ROWS * n else 2  # (the 19- and 26-row grids: two slabs, against the four ranks' rows all the same)
    assert fx.op.ny >= MIN_ROWS * slabs
    with crd.LocalGroup(params(fx, precision), slabs) as grp:
        assert [(s.is_, s.ie) for s in grp.slabs] == [(0, fx.op.nx - 1)] * slabs
        check_f_on_parts(fx, precision, grp, [Whole(fx, fx.ranks(n))], "%d phi-slabs, rows of %d ranks" % (slabs, n))


@pytest.mark.parametrize("layout", ["block-contexts-staged", "four-slabs-fused"])
@pytest.mark.parametrize("tag", RK4)
def test_rk4_run_of_four_ranks(gpu_device, tag, layout):
    """From the reference's initial rows to each of its output times; every block's rows through the trajectory gate by themselves."""
    fx = fixture(tag)
    ranks = fx.ranks(4)
    p, dt = params(fx, "f64"), float(fx.d["dt"])
    grp = crd.LocalGroup(p, 4, blocks=crd.dims_create(4)) if layout == "block-contexts-staged" else crd.LocalGroup(p, 4)
    with grp:
        if layout == "block-contexts-staged":
            held_to_its_rank(grp, ranks)
        else:
            grp.set_exchange_period(3)  # 13-row slabs: 3 steps x 4 ghost rows is what they can lend (before the stepper: it depends on this)
            grp.set_stepper("fused")
        grp.upload(stitched(fx, ranks, 0))
        for k, (t, tout, steps) in enumerate(output_times(fx), start=1):
            grp.step_rk4(t, dt, steps)
            whole = None if layout == "block-contexts-staged" else grp.download()
            for q, r in enumerate(ranks):
                got = grp.slabs[q].download() if whole is None else np.ascontiguousarray(r.cut(whole))
                trajectory_gate("%s %s output %d, rank %d of 4" % (tag, layout, k, q), got, r.rows[k])


@pytest.mark.parametrize("argv,n", [(("--gpus", "2", "--decomp", "mpi"), 2), (("--gpus", "4", "--decomp", "mpi"), 4),
                                    (("--gpus", "4", "--decomp", "2x2", "--block-contexts"), 4)], ids=["mpi-2", "mpi-4", "2x2-block-contexts"])
@pytest.mark.parametrize("tag", RK4)
def test_driver_writes_every_ranks_files(gpu_device, tmp_path, tag, argv, n):
    """`crd_run --fixed --dt <the fixture's> --decomp mpi` on two and on four slabs of one device, and on 2 x 2 block contexts: every
    rank's subdomain file and initial row are the reference's bytes, the later rows pass the trajectory gate, no file for rank np."""
    fx = fixture(tag)
    ranks = fx.ranks(n)
    ini = tmp_path / "case.ini"
    ini.write_text(str(fx.d["ini_text"]))
    exe = os.path.join(ROOT, "crdmodel_amd", "bin", "crd_run")
    r = subprocess.run([exe, "--model", str(fx.d["model"]), "--surface", str(fx.d["surface"]), "--fixed", "--dt", repr(float(fx.d["dt"])), "--quiet", "--devices", "1"]
                       + list(argv) + [str(ini)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    program = fx.program
    for q, rank in enumerate(ranks):
        assert (tmp_path / ("%s_subdomain.%03d.txt" % (program, q))).read_bytes() == rank.header, (q, rank.header)
        got = []
        for f, name in enumerate(mf.PROGRAMS[program][3]):
            lines = (tmp_path / ("%s_%s.%03d.txt" % (program, name, q))).read_bytes().split(b"\n")
            assert len(lines) == rank.rows.shape[0] + 1 and lines[-1] == b"", (name, q, len(lines))
            assert lines[0] + b"\n" == text_row(rank.rows[0][..., f]), "initial row of %s, rank %d of %d" % (name, q, n)
            got.append(np.array([[float(v) for v in line.split()] for line in lines[:-1]]).reshape(rank.rows.shape[:-1]))
        got = np.stack(got, axis=-1)
        for k in range(1, rank.rows.shape[0]):
            trajectory_gate("driver %s output %d, rank %d of %d" % (" ".join(argv), k, q, n), got[k], rank.rows[k])
    assert not any((tmp_path / ("%s_%s.%03d.txt" % (program, name, n))).exists() for name in ("subdomain",) + mf.PROGRAMS[program][3])
