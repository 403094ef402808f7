"""The oracle and libcrd's host side against the reference's OWN compiled code (tests/golden/refprobe_*.npz).

The fixtures hold what the reference's four programs, compiled unmodified against the stand-in headers of oracle/ref_build/, read and
wrote at one rank: their f() on given states (the stand-in ARKode does no arithmetic there), their initial rows, their subdomain
lines, fixed-step RK4 runs through their f(), and two complete run directories.  Everything is compared bit for bit; each check is
also handed arrays with one value moved by one ulp at (0, 0), at the theta seam column, in an absorbing row and at the last point,
and has to fail.  Problem parameters always go ini text -> crd.load_ini -> crd_params -> oracle problem (make_fixtures.load).

Runs with two and four ranks: tests/test_refranks_host.py.  Not pinned, and said so wherever the project speaks of parity: ARKode's
adaptive step sequence.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import crdmodel_amd as crd
from oracle import crd_oracle as co
from oracle import error_bounds as eb
from oracle.ref_build import build_ref
from oracle.ref_build import make_fixtures as mf

TAGS = [os.path.basename(p)[len(mf.PREFIX):-4] for p in mf.fixture_paths()]
PROBE = [t for t in TAGS if t != "geometry" and not t.startswith("rk4_")]
RK4 = [t for t in TAGS if t.startswith("rk4_")]
_cache = {}


class Fixture:
    def __init__(self, tag):
        self.tag = tag
        d = np.load(os.path.join(mf.GOLDEN, mf.PREFIX + tag + ".npz"), allow_pickle=False)
        self.d = {k: d[k] for k in d.files}
        self.program = str(self.d["program"])
        self.cfg, self.op = mf.load(str(self.d["ini_text"]), self.program)
        self.cfg.steady_state_decimals = 8  # the route the reference takes: the printed line (Goldbeter; no effect on FHN)
        self.rows = np.stack([self.d["var0"], self.d["var1"]], axis=-1)  # (rows, ny, nx, 2)
        self.steady = tuple(float(v) for v in self.d["steady_line"]) or None

    def probes(self):
        for k, (t, s) in enumerate(zip(self.d["probe_t"], self.d["probe_state"])):
            yield k, float(t), self.d["states"][s].astype(np.float64), str(self.d["state_names"][s])


def fixture(tag):
    if tag not in _cache:
        _cache[tag] = Fixture(tag)
    return _cache[tag]


def planted_points(ny, nx):
    """(0, 0), the theta seam column, an absorbing row, the last point."""
    return [(0, 0), (ny // 2, nx - 1), (ny - 1, nx // 2), (ny - 1, nx - 1)]


def moved(a, row, col, field):
    """A copy of (..., ny, nx, 2) with one value of the last frame moved to the next double."""
    b = np.array(a, copy=True)
    b[..., row, col, field] = np.nextafter(b[..., row, col, field], np.inf)
    return b


def require_bits(case, got, ref):
    """got and ref, (ny, nx, 2) doubles, are the same bit patterns; a failure names the case, the field and the first (row, column)."""
    got, ref = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (case, got.shape, ref.shape)
    for f in (0, 1):
        bad = np.argwhere(got[..., f].view(np.uint64) != ref[..., f].view(np.uint64))
        if len(bad):
            j, i = bad[0]
            raise AssertionError("%s: field %d differs at %d point(s), first at (row %d, column %d): %r, the reference wrote %r"
                                 % (case, f, len(bad), j, i, got[j, i, f], ref[j, i, f]))


# ---- the checks (each takes the reference's rows as an argument, so that the planted tests can hand it moved ones) -----------------

def check_rhs(fx, rows):
    for k, t, y, name in fx.probes():
        require_bits("%s probe %d (%s state, t = %g): co.rhs" % (fx.tag, k, name, t), co.rhs(fx.op, t, y), rows[k + 1])


def check_initial_conditions(fx, rows):
    cfg = fx.cfg
    if fx.steady is not None:
        assert crd.steady_state_as_printed("goldbeter", cfg.params.beta, 8) == fx.steady, (fx.tag, fx.steady)
    got = co.initial_conditions(fx.op, cfg.wave_length, cfg.wave_width, cfg.wave_inside, cfg.ic_type, steady_state=fx.steady)
    require_bits("%s: co.initial_conditions" % fx.tag, got, rows[0])
    y = np.empty((fx.op.ny, fx.op.nx, 2))
    crd._capi.check(crd._capi.lib().crd_initial_conditions(C.byref(cfg), 0, fx.op.ny - 1, y.ctypes.data), "crd_initial_conditions")
    require_bits("%s: crd_initial_conditions" % fx.tag, y, rows[0])


def check_rk4(fx, rows):
    cfg, dt, per = fx.cfg, float(fx.d["dt"]), int(fx.d["steps_per_output"])
    d_out = (cfg.t_final - 0.0) / cfg.output_timestep  # the reference's output loop: tout += dTout, capped at Tf
    y, t, tout = rows[0], 0.0, 0.0 + d_out
    for k in range(1, cfg.output_timestep + 1):
        n = int(round((tout - t) / dt))
        assert n == per, (fx.tag, k, n)
        y = co.rk4(fx.op, y, t, dt, n)
        require_bits("%s output %d (t = %.17g): co.rk4" % (fx.tag, k, tout), y, rows[k])
        t, tout = tout, min(tout + d_out, cfg.t_final)


def check_bound(fx, rows):
    """The reference's own double evaluation is inside the bound the GPU is held to."""
    for k, t, y, name in fx.probes():
        eb.check("%s probe %d (%s state): the reference's ydot" % (fx.tag, k, name), rows[k + 1], eb.rhs_bound(fx.op, t, y, "f64"))


def check_header(fx, header, cfg=None, tmp_path=None):
    """crd_grid_from_params, crd_slab_extents(..., 0, 1) and crd_writer_open against one subdomain line of the reference."""
    cfg = fx.cfg if cfg is None else cfg
    words = header.split()
    g = crd.grid_of(cfg.params)
    assert (g.nx, g.ny) == (int(words[0]), int(words[1])), ("nx, ny", fx.tag, (g.nx, g.ny), header)
    assert crd.slab_extents(g.ny, 0, 1) == (int(words[4]), int(words[5])), ("js, je", fx.tag, header)
    if tmp_path is not None:
        crd.Writer(cfg, tmp_path).close()
        with open(os.path.join(tmp_path, "%s_subdomain.000.txt" % fx.program), "rb") as f:
            assert f.read() == header, (fx.tag, header)


def check_files(fx, rows, tmp_path):
    """crd_writer_write_row on the parsed rows gives back the reference's complete files."""
    names = mf.PROGRAMS[fx.program][3]
    with crd.Writer(fx.cfg, tmp_path) as w:
        for row in rows:
            w.write_row(row)
    for f, key in zip(names, ("file_var0", "file_var1")):
        with open(os.path.join(tmp_path, "%s_%s.000.txt" % (fx.program, f)), "rb") as fh:
            got = fh.read()
        assert got == fx.d[key].tobytes(), "%s: %s_%s.000.txt differs from the reference's file" % (fx.tag, fx.program, f)


# ---- the fixtures as committed -----------------------------------------------------------------------------------------------------

def test_every_case_has_its_fixture():
    assert sorted(TAGS) == sorted([c["tag"] for c in mf.CASES] + ["geometry"])
    sizes = [os.path.getsize(p) for p in mf.fixture_paths()]
    assert max(sizes) <= mf.MAX_FIXTURE_BYTES and sum(sizes) < mf.MAX_TOTAL_BYTES, (max(sizes), sum(sizes))


def test_goldbeter_torus_fixture_carries_a_beta_range_the_program_never_reads():
    fx = fixture("gb_torus_23_vb")
    ini = str(fx.d["ini_text"])
    assert "betaMin = 0.1" in ini and "betaMax = 0.9" in ini and "varyBeta = 1" in ini
    assert (fx.cfg.params.vary_beta, fx.cfg.params.beta_min, fx.cfg.params.beta_max) == (1, 0.0, 0.0)


@pytest.mark.parametrize("tag", PROBE)
def test_oracle_rhs_is_the_references_f_bit_for_bit(tag):
    fx = fixture(tag)
    check_rhs(fx, fx.rows)


@pytest.mark.parametrize("tag", PROBE + RK4)
def test_initial_conditions_are_the_references_first_row(tag):
    fx = fixture(tag)
    check_initial_conditions(fx, fx.rows)


@pytest.mark.parametrize("tag", PROBE + RK4)
def test_grid_extents_and_subdomain_line(tag, tmp_path):
    fx = fixture(tag)
    check_header(fx, fx.d["header"].tobytes(), tmp_path=str(tmp_path))


def test_geometry_sweep(tmp_path):
    d = np.load(os.path.join(mf.GOLDEN, mf.PREFIX + "geometry.npz"), allow_pickle=False)
    truncating = 0
    assert len(d["header"]) >= 200
    for k, (program, ini, header) in enumerate(zip(d["program"], d["ini_text"], d["header"])):
        fx = type("GeometryCase", (), {"tag": "geometry[%d] %s" % (k, program), "program": str(program)})
        cfg, _ = mf.load(str(ini), str(program))
        check_header(fx, str(header).encode(), cfg, str(tmp_path))
        p = cfg.params
        truncating += int(header.split()[1]) != int(p.nx * p.surface_length / p.surface_width)
    assert truncating >= 50, truncating


@pytest.mark.parametrize("tag", [t for t in PROBE if "file_var0" in fixture(t).d] if TAGS else [])
def test_writer_reproduces_the_references_files(tag, tmp_path):
    fx = fixture(tag)
    check_files(fx, fx.rows, str(tmp_path))


@pytest.mark.parametrize("tag", RK4)
def test_oracle_rk4_is_rk4_through_the_references_f_bit_for_bit(tag):
    fx = fixture(tag)
    check_rk4(fx, fx.rows)


@pytest.mark.parametrize("tag", PROBE)
def test_the_references_ydot_is_inside_the_gpu_bound(tag):
    fx = fixture(tag)
    check_bound(fx, fx.rows)


# ---- every check bites -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("point", range(4))
@pytest.mark.parametrize("tag", ["fhn_torus_23", "gb_torus_23_vb", "gb_flat_23_ic2"])
def test_planted_ulp_fails_the_rhs_and_initial_condition_checks(tag, point):
    fx = fixture(tag)
    j, i = planted_points(fx.op.ny, fx.op.nx)[point]
    for field in (0, 1):
        for frame in range(fx.rows.shape[0]):
            rows = fx.rows.copy()
            rows[frame] = moved(rows[frame], j, i, field)
            with pytest.raises(AssertionError, match=r"field %d differs at 1 point\(s\), first at \(row %d, column %d\)" % (field, j, i)):
                check_initial_conditions(fx, rows) if frame == 0 else check_rhs(fx, rows)


@pytest.mark.parametrize("point", range(4))
@pytest.mark.parametrize("tag", RK4)
def test_planted_ulp_fails_the_rk4_check(tag, point):
    fx = fixture(tag)
    j, i = planted_points(fx.op.ny, fx.op.nx)[point]
    for frame in (1, fx.rows.shape[0] - 1):
        rows = fx.rows.copy()
        rows[frame] = moved(rows[frame], j, i, point % 2)
        with pytest.raises(AssertionError, match=r"output %d .*\(row %d, column %d\)" % (frame, j, i)):
            check_rk4(fx, rows)


@pytest.mark.parametrize("point", range(4))
def test_planted_ulp_fails_the_file_check(point, tmp_path):
    fx = fixture("fhn_torus_5")
    j, i = planted_points(fx.op.ny, fx.op.nx)[point]
    rows = fx.rows.copy()
    rows[-1] = moved(rows[-1], j, i, point % 2)
    with pytest.raises(AssertionError, match="differs from the reference's file"):
        check_files(fx, rows, str(tmp_path))


@pytest.mark.parametrize("point", range(4))
@pytest.mark.parametrize("tag", ["fhn_torus_23", "gb_torus_23"])
def test_planted_error_fails_the_bound_check(tag, point):
    """One ulp is inside a rounding-error bound by construction, so the planted error here is twice the bound at the point -- and one
    ulp where the bound is zero (an absorbing row before tBoundary)."""
    fx = fixture(tag)
    j, i = planted_points(fx.op.ny, fx.op.nx)[point]
    for k, t, y, _ in fx.probes():
        _, bu, bv = eb.rhs_bound(fx.op, t, y, "f64")
        for field, b in ((0, bu), (1, bv)):
            rows = fx.rows.copy()
            step = 2.0 * float(b[j, i])
            rows[k + 1, j, i, field] = rows[k + 1, j, i, field] + step if step > 0.0 else np.nextafter(rows[k + 1, j, i, field], np.inf)
            with pytest.raises(AssertionError):
                check_bound(fx, rows)


def test_a_wrong_subdomain_line_fails_the_header_check(tmp_path):
    fx = fixture("fhn_torus_23_trunc")
    header = fx.d["header"].tobytes()

    def line(w):
        return b"  ".join(w[:6]) + b" " + b" ".join(w[6:]) + b"\n"

    assert line(header.split()) == header
    check_header(fx, header, tmp_path=str(tmp_path))
    for k, wrong in ((1, b"217"), (5, b"216"), (8, b"1.200001")):  # ny, je, tFinal
        words = header.split()
        words[k] = wrong
        with pytest.raises(AssertionError):
            check_header(fx, line(words), tmp_path=str(tmp_path))


# ---- the fixtures are what the recipe makes ----------------------------------------------------------------------------------------

def need_compiled_reference():
    """A reference tree without the binaries is a failure (build() makes them); only a machine with neither skips."""
    if not build_ref.built():
        if build_ref.reference_dir() is not None:
            pytest.fail("a reference tree is present but oracle/_ref/ does not hold its programs: __graft_entry__.build() (oracle/ref_build/build_ref.py) builds them")
        pytest.skip("neither a reference tree nor oracle/_ref/ on this machine")


def test_stand_ins_fail_the_way_the_libraries_would(tmp_path):
    """A short probe file is a solver failure reported by the program (no crash, the initial row written); a missing ini key terminates it."""
    import subprocess

    need_compiled_reference()
    exe = os.path.join(build_ref.OUT, "O0", "FHNmodel_torus")
    ini = mf.ini_text("FHNmodel_torus", 5, 80.0, 20.0)
    (tmp_path / "case.ini").write_text(ini)
    (tmp_path / "probe.bin").write_bytes(np.zeros(3).tobytes())  # t and two of the 200 values
    env = {k: v for k, v in os.environ.items() if k != "CRD_REF_RK4_DT"}
    r = subprocess.run([exe, "case.ini"], cwd=tmp_path, env=dict(env, CRD_REF_PROBE="probe.bin"), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ARKode failed with flag = -1" in r.stderr, (r.returncode, r.stderr)
    assert (tmp_path / "FHNmodel_torus_u.000.txt").read_bytes().count(b"\n") == 1
    (tmp_path / "case.ini").write_text(ini.replace("betaMax = 1.7\n", ""))
    r = subprocess.run([exe, "case.ini"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "No such node (Parameters.betaMax)" in r.stderr, (r.returncode, r.stderr)


def test_fixtures_regenerate_from_the_compiled_reference(tmp_path):
    """With oracle/_ref/ built: run the recipe again and require the committed contents, array by array."""
    need_compiled_reference()
    mf.make_all(str(tmp_path))
    made = [os.path.basename(p) for p in mf.fixture_paths(str(tmp_path))]
    assert made == [os.path.basename(p) for p in mf.fixture_paths()]
    for name in made:
        new, old = np.load(os.path.join(str(tmp_path), name), allow_pickle=False), np.load(os.path.join(mf.GOLDEN, name), allow_pickle=False)
        assert sorted(new.files) == sorted(old.files), name
        for k in new.files:
            if k == "provenance":  # the compiler's version line may differ between machines; the sources and flags may not
                a, b = json.loads(str(new[k])), json.loads(str(old[k]))
                assert (a["sources"], a["flags"]) == (b["sources"], b["flags"]), name
                continue
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (name, k)
