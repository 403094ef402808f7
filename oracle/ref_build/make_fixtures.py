"""Run the reference's own compiled programs (oracle/_ref/, build_ref.py) on the cases below and record what they read and wrote as
tests/golden/refprobe_<tag>.npz.

    python oracle/ref_build/make_fixtures.py [--out DIR]

Every case runs with the -O0 and with the -O2 build; the two must write identical bytes.  A fixture holds data only: the ini text,
the probe records handed to the stand-in ARKode, and the rows and header line the reference wrote (README.md has the schema).
tests/test_refprobe_host.py regenerates every fixture with this module and requires the committed contents.  Run as a script it also
writes the two- and four-rank fixtures, tests/golden/refranks_<tag>.npz (make_rank_fixtures.py).
"""
import io
import itertools
import json
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import crd_oracle as co  # noqa: E402
from oracle.ref_build import build_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PREFIX = "refprobe_"
MAX_FIXTURE_BYTES = 424462  # the largest file tracked under tests/golden/ before these fixtures
MAX_TOTAL_BYTES = 2 * 1000 * 1000

# program -> (model, surface, mesh key, names of the two fields in the file names)
PROGRAMS = {
    "FHNmodel_torus": ("fhn", "torus", "thetaMesh", ("u", "v")),
    "FHNmodel_flat": ("fhn", "flat", "thetaMesh", ("u", "v")),
    "GoldbeterModel_torus": ("goldbeter", "torus", "xMesh", ("Z", "Y")),
    "GoldbeterModel_flat": ("goldbeter", "flat", "xMesh", ("Z", "Y")),
}

# (state, time) of each probe record.  Times: "half" = tBoundary / 2 (rows 0 and ny-1 absorb), "at" = exactly tBoundary (they do not:
# the test is t < TBOUNDARY), "after" = 2 tBoundary + 1.  States: see probe_states().
FULL = (("front", "half"), ("random", "at"), ("uniform", "after"))
# grids of several thousand points: one record with a non-uniform state is what the size conditions leave room for
LARGE = (("front", "half"), ("uniform", "after"))


def _case(tag, program, nx, length, width, probes=FULL, keep_files=False, **kw):
    d = dict(tag=tag, program=program, nx=nx, length=length, width=width, probes=probes, keep_files=keep_files, mode="probe",
             wave_inside=0, vary_beta=0, just_diffusion=0, ic_type=0, t_boundary=0.4)
    d.update(kw)
    return d


FT, FF, GT, GF = "FHNmodel_torus", "FHNmodel_flat", "GoldbeterModel_torus", "GoldbeterModel_flat"
CASES = [
    # FHN torus: waveInside 0 / 1, varyBeta 0 / 1, tBoundary 0 / > 0, spread over the grids
    _case("fhn_torus_5", FT, 5, 80.0, 20.0, wave_inside=1, t_boundary=0.0, keep_files=True),
    _case("fhn_torus_23", FT, 23, 80.0, 20.0),
    _case("fhn_torus_64_vb", FT, 64, 80.0, 20.0, vary_beta=1, probes=LARGE),
    _case("fhn_torus_23_curved_vb", FT, 23, 40.0, 20.0, wave_inside=1, vary_beta=1, t_boundary=0.0),
    _case("fhn_torus_23_trunc", FT, 23, 66.0, 7.0),  # ny = 216 of a quotient 216.86
    _case("fhn_torus_65_vb", FT, 65, 20.5, 20.0, vary_beta=1),
    _case("fhn_torus_121", FT, 121, 20.5, 20.0, probes=LARGE),
    _case("fhn_flat_23", FF, 23, 40.0, 20.0),
    _case("fhn_flat_64_vb", FF, 64, 20.5, 20.0, vary_beta=1, probes=LARGE),
    # Goldbeter torus never reads betaMin / betaMax (the ini carries non-zero ones): varyBeta = 1 is beta = 0 throughout
    _case("gb_torus_23", GT, 23, 40.0, 20.0),
    _case("gb_torus_23_vb", GT, 23, 40.0, 20.0, vary_beta=1, ic_type=1),  # icType is not read by the torus program either
    _case("gb_torus_23_jd", GT, 23, 40.0, 20.0, just_diffusion=1, wave_inside=1),
    _case("gb_torus_65_vb_jd", GT, 65, 20.5, 20.0, vary_beta=1, just_diffusion=1),
    # Goldbeter flat: ny = xMesh * (long)(L / W); icType 0 / 1 / 2 under varyBeta = 1 (2 is the rand() rule)
    _case("gb_flat_23", GF, 23, 20.0, 20.0, keep_files=True),
    _case("gb_flat_23_ic0", GF, 23, 20.0, 20.0, vary_beta=1, ic_type=0),
    _case("gb_flat_23_ic1", GF, 23, 20.0, 20.0, vary_beta=1, ic_type=1),
    _case("gb_flat_23_ic2", GF, 23, 20.0, 20.0, vary_beta=1, ic_type=2),
    # fixed-step RK4 through the reference's f(): 40 steps, 4 output times, tBoundary between stage 1 and stage 2 of step 12
    _case("rk4_fhn_torus_23", FT, 23, 80.0, 20.0, mode="rk4", probes=()),
    _case("rk4_gb_torus_23", GT, 23, 40.0, 20.0, mode="rk4", probes=()),
]
RK4_STEPS, RK4_OUTPUTS, RK4_DT_SAFETY, RK4_BOUNDARY_STEPS = 40, 4, 0.8, 12.25

BETA = {"fhn": 1.25, "goldbeter": 0.4}
BETA_RANGE = {"fhn": (0.7, 1.7), "goldbeter": (0.1, 0.9)}


def ini_text(program, nx, length, width, *, wave_inside=0, vary_beta=0, just_diffusion=0, ic_type=0, t_boundary=0.4, t_final=1.2,
             outputs=3, all_vars=1):
    """One ini with every key any of the four programs reads (each ignores the others'), a comment line and a trailing tab."""
    model, _, mesh_key, _ = PROGRAMS[program]
    lo, hi = BETA_RANGE[model]
    return ("; %s\n[Parameters]\ndiffusion = 0.12\nbeta = %r\t\nsurfaceWidth = %r\nsurfaceLength = %r\nwaveLength = 0.1\nwaveWidth = 0.5\n"
            "waveInside = %d\noutputTimestep = %d\ntBoundary = %r\ntFinal = %r\n%s = %d\nbetaMin = %r\nbetaMax = %r\n\n# switches\n[System]\n"
            "includeAllVars = %d\nvaryBeta = %d\njustDiffusion = %d\nicType = %d\n"
            % (program, BETA[model], width, length, wave_inside, outputs, t_boundary, t_final, mesh_key, nx, lo, hi, all_vars, vary_beta,
               just_diffusion, ic_type))


def load(ini, program):
    """ini text -> (cfg, oracle problem): crd.load_ini -> crd_params -> co.make_problem, the one route the tests take too."""
    import crdmodel_amd as crd

    model, surface = PROGRAMS[program][:2]
    with tempfile.NamedTemporaryFile("w", suffix=".ini", delete=False) as f:
        f.write(ini)
    try:
        cfg = crd.load_ini(f.name, model, surface)
    finally:
        os.unlink(f.name)
    p = cfg.params
    op = co.make_problem({"fhn": co.FHN, "goldbeter": co.GOLDBETER}[model], {"torus": co.TORUS, "flat": co.FLAT}[surface], int(p.nx),
                         p.surface_length, p.surface_width, p.diffusion, p.beta, ny=int(p.ny), beta_min=p.beta_min, beta_max=p.beta_max,
                         vary_beta=p.vary_beta, just_diffusion=p.just_diffusion, t_boundary=p.t_boundary)
    return cfg, op


def steady_line(program, ini):
    """The two numbers the stand-in SolveGoldbeterODE.py prints, as text: the fixed point at numpy's 8 decimals."""
    import crdmodel_amd as crd

    if PROGRAMS[program][0] != "goldbeter":
        return None
    cfg, _ = load(ini, program)
    return tuple(("%.8f" % v).rstrip("0") for v in crd.steady_state_as_printed("goldbeter", cfg.params.beta, 8))


def probe_states(op, seed):
    """The three probe states, every value a float32 (the fp32 kernels and the reference then see the same numbers):
    front = tests/test_gpu_error_bounds.py::state, random = uniform positive noise, uniform = one value per field."""
    from test_gpu_error_bounds import state

    rng = np.random.default_rng(seed)
    shape = (op.ny, op.nx, 2)
    uniform = np.empty(shape, dtype=np.float32)
    uniform[..., 0], uniform[..., 1] = 0.7312, 1.25
    return {"front": state(op, seed, "f32"), "random": rng.uniform(0.05, 1.5, shape).astype(np.float32), "uniform": uniform}


def probe_time(which, t_boundary):
    return {"half": 0.5 * t_boundary, "at": t_boundary, "after": 2.0 * t_boundary + 1.0}[which]


def run_reference(program, ini, env, workdir):
    """Both builds in directories of their own; returns {file name: bytes}, identical for -O0 and -O2."""
    out = {}
    for lv in build_ref.LEVELS:
        d = os.path.join(workdir, lv)
        os.makedirs(d, exist_ok=True)
        for f in os.listdir(d):
            os.unlink(os.path.join(d, f))
        with open(os.path.join(d, "case.ini"), "w") as f:
            f.write(ini)
        e = dict(os.environ, PATH=os.path.join(build_ref.OUT, "bin") + os.pathsep + os.environ.get("PATH", ""))
        for k in ("CRD_REF_PROBE", "CRD_REF_RK4_DT"):
            e.pop(k, None)
        e.update(env)
        r = subprocess.run([os.path.join(build_ref.OUT, lv, program), "case.ini"], cwd=d, env=e, capture_output=True, timeout=120)
        if r.returncode != 0:
            raise RuntimeError("%s (-%s) exited with %d: %s" % (program, lv, r.returncode, r.stderr.decode(errors="replace")[-400:]))
        out[lv] = {}
        for f in sorted(os.listdir(d)):
            if f.startswith(program + "_"):
                with open(os.path.join(d, f), "rb") as fh:
                    out[lv][f] = fh.read()
    a, b = (out[lv] for lv in build_ref.LEVELS)
    if a != b:
        raise RuntimeError("%s: the -O0 and -O2 builds wrote different bytes (%s)" % (program, [k for k in a if a[k] != b.get(k)]))
    return a


def parse_rows(text, ny, nx):
    """The rows of one field's file: (rows, ny, nx) doubles (float() reads "%.16e" back exactly)."""
    rows = [np.array([float(v) for v in line.split()]) for line in text.decode().split("\n") if line.strip()]
    return np.stack(rows).reshape(len(rows), ny, nx) if rows else np.empty((0, ny, nx))


def steady_env(program, ini):
    s = steady_line(program, ini)
    return {} if s is None else {"CRD_REF_STEADY_Z": s[0], "CRD_REF_STEADY_Y": s[1]}


def make_case(case, workdir):
    """One case -> dict of arrays (the fixture's contents)."""
    import crdmodel_amd as crd

    program = case["program"]
    model, surface, _, fields = PROGRAMS[program]
    kw = {k: case[k] for k in ("wave_inside", "vary_beta", "just_diffusion", "ic_type")}
    rec = {}
    if case["mode"] == "probe":
        ini = ini_text(program, case["nx"], case["length"], case["width"], t_boundary=case["t_boundary"], outputs=len(case["probes"]), **kw)
        cfg, op = load(ini, program)
        states = probe_states(op, 1000 + CASES.index(case))
        names = sorted({s for s, _ in case["probes"]})
        times = np.array([probe_time(w, case["t_boundary"]) for _, w in case["probes"]])
        probe = os.path.join(workdir, "probe.bin")
        with open(probe, "wb") as f:
            for (s, _), t in zip(case["probes"], times):
                np.float64(t).tofile(f)
                states[s].astype(np.float64).tofile(f)
        env = {"CRD_REF_PROBE": probe}
        rec.update(probe_t=times, probe_state=np.array([names.index(s) for s, _ in case["probes"]]), state_names=np.array(names),
                   states=np.stack([states[s] for s in names]))
    else:
        pre, _ = load(ini_text(program, case["nx"], case["length"], case["width"], **kw), program)
        dt = RK4_DT_SAFETY * crd.stable_dt(pre.params)
        ini = ini_text(program, case["nx"], case["length"], case["width"], t_boundary=RK4_BOUNDARY_STEPS * dt, t_final=RK4_STEPS * dt,
                       outputs=RK4_OUTPUTS, **kw)
        cfg, op = load(ini, program)
        env = {"CRD_REF_RK4_DT": repr(dt)}
        rec.update(dt=np.float64(dt), steps_per_output=np.int64(RK4_STEPS // RK4_OUTPUTS))
    env.update(steady_env(program, ini))
    files = run_reference(program, ini, env, workdir)
    header = files["%s_subdomain.000.txt" % program]
    nx, ny = (int(v) for v in header.split()[:2])
    if (nx, ny) != (op.nx, op.ny):
        raise RuntimeError("%s: the reference's grid is %d x %d, the oracle's %d x %d" % (case["tag"], nx, ny, op.nx, op.ny))
    var = [files["%s_%s.000.txt" % (program, f)] for f in fields]
    rec.update(tag=np.array(case["tag"]), program=np.array(program), model=np.array(model), surface=np.array(surface), mode=np.array(case["mode"]),
               ini_text=np.array(ini), header=np.frombuffer(header, dtype=np.uint8), var0=parse_rows(var[0], ny, nx), var1=parse_rows(var[1], ny, nx),
               steady_line=np.array(list(steady_line(program, ini) or ())), provenance=np.array(json.dumps(build_ref.provenance(), sort_keys=True)))
    expected = 1 + (len(case["probes"]) if case["mode"] == "probe" else RK4_OUTPUTS)
    if rec["var0"].shape[0] != expected or rec["var1"].shape[0] != expected:
        raise RuntimeError("%s: %d / %d rows written, %d expected" % (case["tag"], rec["var0"].shape[0], rec["var1"].shape[0], expected))
    if case["keep_files"]:
        rec.update(file_var0=np.frombuffer(var[0], dtype=np.uint8), file_var1=np.frombuffer(var[1], dtype=np.uint8))
    return rec


def geometry_cases():
    """(program, nx, L, W) of the header-only sweep: surfaces at least as long as wide (a torus longer), 4 to 600 rows by the plain quotient."""
    meshes = [5, 7, 10, 12, 15, 20, 25, 30]
    lengths = [20.0, 30.0, 42.0, 60.0, 66.0, 80.0, 14.0, 9.9, 20.5]
    widths = [20.0, 10.0, 6.0, 3.0, 7.0, 1.1]
    cases = []
    for k, (nx, length, width) in enumerate(itertools.product(meshes, lengths, widths)):
        program = list(PROGRAMS)[k % 4]
        if length < width or not 4 <= nx * length / width <= 600:
            continue
        if PROGRAMS[program][1] == "torus" and length == width:
            continue  # R = r: the torus closes on its axis; crd_config_load_ini refuses it, the reference divides by R - r
        cases.append((program, nx, length, width))
    # the torus programs once more, on quotients L / W that are not exact in binary: NX * (R / r) often truncates one off int(nx L / W)
    for k, (nx, length, width) in enumerate(itertools.product([5, 7, 10, 12], [35.0, 49.0, 77.0, 54.0, 33.0, 12.0], [7.0, 10.0, 2.1, 4.2, 1.1])):
        if length > width and 4 <= nx * length / width <= 600:
            cases.append((FT if k % 2 == 0 else GT, nx, length, width))
    return cases


def make_geometry(workdir):
    """Header-only runs (no probe file: the stand-in ARKode fails at once, after the subdomain file is written)."""
    inis, headers, programs, plain = [], [], [], 0
    for program, nx, length, width in geometry_cases():
        ini = ini_text(program, nx, length, width, outputs=1, all_vars=0)
        env = {"CRD_REF_STEADY_Z": "0.392", "CRD_REF_STEADY_Y": "1.64562147"}
        files = run_reference(program, ini, env, workdir)
        header = files["%s_subdomain.000.txt" % program].decode()
        plain += int(header.split()[1]) != int(nx * length / width)
        inis.append(ini)
        headers.append(header)
        programs.append(program)
    if len(inis) < 200 or plain < 50:
        raise RuntimeError("geometry sweep: %d cases, %d with ny != int(nx L / W); 200 and 50 are required" % (len(inis), plain))
    return dict(tag=np.array("geometry"), mode=np.array("geometry"), program=np.array(programs), ini_text=np.array(inis), header=np.array(headers),
                provenance=np.array(json.dumps(build_ref.provenance(), sort_keys=True)))


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member order and time stamp: the same contents give the same file."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def fixture_paths(directory=GOLDEN):
    return sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.startswith(PREFIX) and f.endswith(".npz"))


def make_all(out_dir):
    if not build_ref.built():
        raise RuntimeError("oracle/_ref/ does not hold the reference programs: run oracle/ref_build/build_ref.py on a machine with the reference tree")
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as work:
        for case in CASES:
            save_npz(os.path.join(out_dir, PREFIX + case["tag"] + ".npz"), make_case(case, work))
        save_npz(os.path.join(out_dir, PREFIX + "geometry.npz"), make_geometry(work))
    sizes = {os.path.basename(p): os.path.getsize(p) for p in fixture_paths(out_dir)}
    if max(sizes.values()) > MAX_FIXTURE_BYTES or sum(sizes.values()) >= MAX_TOTAL_BYTES:
        raise RuntimeError("fixtures too large: %s, total %d" % (sizes, sum(sizes.values())))
    return sizes


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    from oracle.ref_build import make_rank_fixtures  # the same cases' kin at two and four ranks: refranks_<tag>.npz

    for name, size in sorted(make_all(out).items()) + sorted(make_rank_fixtures.make_all(out).items()):
        print("%8d  %s" % (size, name))
