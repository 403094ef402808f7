"""Run the reference's own compiled programs (oracle/_ref/, build_ref.py) at ONE, TWO and FOUR ranks on the cases below and record what
every rank wrote as tests/golden/refranks_<tag>.npz.

    python oracle/ref_build/make_rank_fixtures.py [--out DIR]        (python oracle/ref_build/make_fixtures.py runs this too)

The ranks are processes of their own, started side by side in one working directory as mpirun would start them; the stand-in mpi.h
(include/mpi.h, CRD_REF_MPI_SIZE / _RANK / _DIR) carries their messages through a directory.  For each case and each np in (2, 4):

  1. a header-only run (no probe file: the stand-in ARKode fails at once, after the subdomain files and initial rows are written).
     The ranks' extents are read from the subdomain lines THE REFERENCE wrote; nothing of this project computes them.
  2. probe cases: rank k's probe file holds its block [js, je] x [is, ie] of the very states and times the one-rank run gets, laid out
     as the reference's index macro lays out a local vector (2 x + 2 y nxl: rows of nxl points, two values per point), and the run
     is repeated with CRD_REF_PROBE set per rank.  RK4 cases: the run is repeated with CRD_REF_RK4_DT.

Every run is made with the -O0 and with the -O2 build; the two must write identical bytes.  A fixture holds data only (README.md
has the schema): what the one-rank run wrote, and per np and rank the subdomain line's bytes and every row of both fields, rank after
rank in one array; for the two smallest cases also the complete text files.  tests/test_refranks_host.py regenerates every fixture
with this module and requires the committed contents.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle.ref_build import build_ref  # noqa: E402
from oracle.ref_build import make_fixtures as mf  # noqa: E402

PREFIX = "refranks_"
RANKS = (2, 4)
MAX_FIXTURE_BYTES = mf.MAX_FIXTURE_BYTES
MAX_TOTAL_BYTES = 600 * 1000
DEADLINE_SECONDS = 60  # of one MPI_Wait; a run lasts milliseconds
RUN_SECONDS = 180

FT, FF, GT, GF = mf.FT, mf.FF, mf.GT, mf.GF
# Every probe case: times half, at and after with tBoundary = 0.4 > 0, so that the held rows of the ranks that own row 0 or ny - 1 are seen.
# own_rows: the cases in which a rank's rows are NOT the cut of the one-rank rows, by the reference's own rule, and why.
CASES = [
    # nx and ny both odd: nx c / d truncates in both directions (11 | 12 columns, 28 | 29 rows; 6 | 7 and 19 | 20)
    mf._case("fhn_torus_23x57", FT, 23, 50.0, 20.0),
    mf._case("gb_flat_13x39", GF, 13, 60.0, 20.0),
    # one per program on 13-wide grids, varyBeta = 1 once per model, waveInside.  No grid has fewer than 16 rows: libcrd wants 8 per
    # block, and the GPU tests put these very grids on 2 x 2 block contexts
    mf._case("fhn_torus_13_vb", FT, 13, 30.0, 20.0, vary_beta=1, wave_inside=1, keep_files=True),  # 13 x 19: 6 | 7 columns, 9 | 10 rows
    mf._case("fhn_flat_13", FF, 13, 40.0, 20.0),  # 13 x 26 (the flat programs: ny = nx (long) (L / W))
    mf._case("gb_torus_13", GT, 13, 30.0, 20.0, wave_inside=1, keep_files=True),  # 13 x 19
    mf._case("gb_flat_13_vb_ic1", GF, 13, 40.0, 20.0, vary_beta=1, ic_type=1),  # 13 x 26
    mf._case("gb_flat_13_vb_ic2", GF, 13, 40.0, 20.0, vary_beta=1, ic_type=2,
             own_rows="icType = 2 draws (float) rand() / RAND_MAX * 1.4 point by point with no srand(): every rank is a process of its own and "
                      "draws the same sequence from the default seed over ITS points, so a rank's initial row is the first 2 nxl nyl values "
                      "of the one-rank initial row, not the cut of it"),
    # fixed-step RK4 through the reference's f() and Exchange(): 40 steps, 4 output times, tBoundary between stage 1 and stage 2 of step 12
    # (13 x 52: four phi-slabs of 13 rows, the shortest the one-launch stepper takes at its shortest exchange period, 3 steps x 4 rows)
    mf._case("rk4_fhn_torus_13x52", FT, 13, 80.0, 20.0, mode="rk4", probes=()),
]
SEED = 2000  # + the case's index: the probe states' seed


def fixture_paths(directory=mf.GOLDEN):
    return sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.startswith(PREFIX) and f.endswith(".npz"))


def run_ranks(program, ini, n, rank_env, rank_files, workdir):
    """n rank processes of each build side by side in a working directory of their own; rank_env(k) -> that rank's extra environment,
    rank_files = {name: bytes} written beside case.ini first.  Returns {file name: bytes}, identical for -O0 and -O2."""
    out = {}
    for lv in build_ref.LEVELS:
        d = tempfile.mkdtemp(prefix="np%d_%s_" % (n, lv), dir=workdir)
        os.mkdir(os.path.join(d, "messages"))
        with open(os.path.join(d, "case.ini"), "w") as f:
            f.write(ini)
        for name, data in rank_files.items():
            with open(os.path.join(d, name), "wb") as f:
                f.write(data)
        base = dict(os.environ, PATH=os.path.join(build_ref.OUT, "bin") + os.pathsep + os.environ.get("PATH", ""))
        for k in [k for k in base if k.startswith("CRD_REF_")]:
            del base[k]
        procs = []
        for k in range(n):
            e = dict(base, **rank_env(k))
            if n > 1:
                e.update(CRD_REF_MPI_SIZE=str(n), CRD_REF_MPI_RANK=str(k), CRD_REF_MPI_DIR=os.path.join(d, "messages"), CRD_REF_MPI_DEADLINE=str(DEADLINE_SECONDS))
            procs.append(subprocess.Popen([os.path.join(build_ref.OUT, lv, program), "case.ini"], cwd=d, env=e, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE))
        errors = []
        try:
            for k, p in enumerate(procs):
                _, err = p.communicate(timeout=RUN_SECONDS)
                if p.returncode != 0:
                    errors.append("rank %d of %d exited with %d: %s" % (k, n, p.returncode, err.decode(errors="replace")[-400:]))
                    break  # the others would wait for it until their deadline
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
                    p.communicate()
        if errors:
            raise RuntimeError("%s (-%s): %s" % (program, lv, errors[0]))
        left = os.listdir(os.path.join(d, "messages"))
        if left:
            raise RuntimeError("%s (-%s), %d ranks: messages left in the directory: %s" % (program, lv, n, left[:4]))
        out[lv] = {}
        for f in sorted(os.listdir(d)):
            if f.startswith(program + "_"):
                with open(os.path.join(d, f), "rb") as fh:
                    out[lv][f] = fh.read()
    a, b = (out[lv] for lv in build_ref.LEVELS)
    if a != b:
        raise RuntimeError("%s, %d ranks: the -O0 and -O2 builds wrote different bytes (%s)" % (program, n, [k for k in a if a[k] != b.get(k)]))
    return a


def check_index_macro(program):
    """The probe files lay a rank's block out as rows of nxl points, two values per point.  Where the reference tree is at hand, its
    own index macro is read from the program's source and evaluated: IDX(x, y) must be 2 x + 2 y nxl.  (Where only oracle/_ref/ is,
    the invariance checks of tests/test_refranks_host.py are what would show another layout.)"""
    ref = build_ref.reference_dir()
    if ref is None:
        return
    with open(os.path.join(ref, "src", program + ".cpp")) as f:
        src = f.read()
    macro = re.search(r"^#define\s+IDX\(\s*x\s*,\s*y\s*\)\s+(.+)$", src, re.M)
    nvars = re.search(r"^#define\s+NVARS\s+(\d+)\s*$", src, re.M)
    if not macro or not nvars:
        raise RuntimeError("%s: no IDX(x, y) / NVARS macro found to check the probe files' layout against" % program)
    expr = macro.group(1).split("//")[0].replace("udata->nxl", "nxl")
    if not re.fullmatch(r"[\sxynlNVARS()*+]+", expr):
        raise RuntimeError("%s: IDX(x, y) is not an expression in x, y, NVARS and nxl: %r" % (program, expr))
    for x, y, nxl in ((0, 0, 7), (1, 0, 7), (0, 1, 7), (5, 3, 6), (11, 28, 12)):
        at = eval(expr, {"__builtins__": {}}, {"x": x, "y": y, "nxl": nxl, "NVARS": int(nvars.group(1))})  # noqa: S307 (characters checked above)
        if at != 2 * x + 2 * y * nxl:
            raise RuntimeError("%s: IDX(%d, %d) with nxl = %d is %d, the probe files assume %d" % (program, x, y, nxl, at, 2 * x + 2 * y * nxl))


def extents_of(header):
    """(nx, ny, is, ie, js, je) of one subdomain line."""
    return tuple(int(v) for v in header.split()[:6])


def rank_rows(text, frames):
    """The rows of one rank's file: (frames, nyl * nxl) doubles, the local vector's own order."""
    rows = [np.array([float(v) for v in line.split()]) for line in text.decode().split("\n") if line.strip()]
    if len(rows) != frames:
        raise RuntimeError("%d rows written, %d expected" % (len(rows), frames))
    return np.stack(rows)


def make_case(case, workdir):
    """One case -> dict of arrays (the fixture's contents)."""
    import crdmodel_amd as crd

    program = case["program"]
    model, surface, _, fields = mf.PROGRAMS[program]
    kw = {k: case[k] for k in ("wave_inside", "vary_beta", "just_diffusion", "ic_type")}
    rec, run_env = {}, {}
    if case["mode"] == "probe":
        ini = mf.ini_text(program, case["nx"], case["length"], case["width"], t_boundary=case["t_boundary"], outputs=len(case["probes"]), **kw)
        cfg, op = mf.load(ini, program)
        states = mf.probe_states(op, SEED + CASES.index(case))
        names = sorted({s for s, _ in case["probes"]})
        times = np.array([mf.probe_time(w, case["t_boundary"]) for _, w in case["probes"]])
        frames = 1 + len(case["probes"])
        rec.update(probe_t=times, probe_state=np.array([names.index(s) for s, _ in case["probes"]]), state_names=np.array(names),
                   states=np.stack([states[s] for s in names]))
    else:
        pre, _ = mf.load(mf.ini_text(program, case["nx"], case["length"], case["width"], **kw), program)
        dt = mf.RK4_DT_SAFETY * crd.stable_dt(pre.params)
        ini = mf.ini_text(program, case["nx"], case["length"], case["width"], t_boundary=mf.RK4_BOUNDARY_STEPS * dt, t_final=mf.RK4_STEPS * dt,
                          outputs=mf.RK4_OUTPUTS, **kw)
        cfg, op = mf.load(ini, program)
        frames = 1 + mf.RK4_OUTPUTS
        run_env = {"CRD_REF_RK4_DT": repr(dt)}
        rec.update(dt=np.float64(dt), steps_per_output=np.int64(mf.RK4_STEPS // mf.RK4_OUTPUTS))
    steady = mf.steady_env(program, ini)
    check_index_macro(program)
    if op.ny < 16:
        raise RuntimeError("%s: %d rows; the GPU tests put every case on 2 x 2 blocks of at least 8 rows" % (case["tag"], op.ny))

    def probe_file(is_, ie, js, je):
        """The block of every probe record as the reference lays out a local vector: IDX(x, y) = 2 x + 2 y nxl."""
        parts = []
        for (s, _), t in zip(case["probes"], times):
            parts.append(np.float64(t).tobytes())
            parts.append(np.ascontiguousarray(states[s][js:je + 1, is_:ie + 1, :], dtype=np.float64).tobytes())
        return b"".join(parts)

    for n in (1,) + RANKS:
        header_only = run_ranks(program, ini, n, lambda k: dict(steady), {}, workdir)
        headers = [header_only["%s_subdomain.%03d.txt" % (program, k)] for k in range(n)]
        if "%s_subdomain.%03d.txt" % (program, n) in header_only:
            raise RuntimeError("%s: a file of rank %d in a run of %d ranks" % (case["tag"], n, n))
        ext = [extents_of(h) for h in headers]
        if any(e[:2] != (op.nx, op.ny) for e in ext):
            raise RuntimeError("%s: the reference's grid is %s, the oracle's %d x %d" % (case["tag"], ext[0][:2], op.nx, op.ny))
        if case["mode"] == "probe":
            files = {"probe.%d.bin" % k: probe_file(*e[2:]) for k, e in enumerate(ext)}
            out = run_ranks(program, ini, n, lambda k: dict(steady, CRD_REF_PROBE="probe.%d.bin" % k), files, workdir)
        else:
            out = run_ranks(program, ini, n, lambda k: dict(steady, **run_env), {}, workdir)
        if [out["%s_subdomain.%03d.txt" % (program, k)] for k in range(n)] != headers:
            raise RuntimeError("%s: the subdomain lines of the two runs at %d ranks differ" % (case["tag"], n))
        text = [[out["%s_%s.%03d.txt" % (program, f, k)] for k in range(n)] for f in fields]
        var = [np.concatenate([rank_rows(t, frames) for t in text[v]], axis=1) for v in (0, 1)]
        for v in (0, 1):
            if var[v].shape != (frames, op.nx * op.ny):
                raise RuntimeError("%s: the %d ranks wrote %s values per row, the grid has %d" % (case["tag"], n, var[v].shape, op.nx * op.ny))
        rec.update({"header_np%d" % n: np.array(headers), "var0_np%d" % n: var[0], "var1_np%d" % n: var[1]})
        if case["keep_files"] and n > 1:
            for v in (0, 1):
                for k in range(n):
                    rec["file_np%d_rank%d_var%d" % (n, k, v)] = np.frombuffer(text[v][k], dtype=np.uint8)
    rec.update(tag=np.array(case["tag"]), program=np.array(program), model=np.array(model), surface=np.array(surface), mode=np.array(case["mode"]),
               ini_text=np.array(ini), own_rows=np.array(case.get("own_rows", "")), steady_line=np.array(list(mf.steady_line(program, ini) or ())),
               provenance=np.array(json.dumps(build_ref.provenance(), sort_keys=True)))
    return rec


def make_all(out_dir):
    if not build_ref.current():
        build_ref.build()  # (compiles only where a reference tree is, and only what is missing or older than the stand-in headers)
    if not build_ref.built():
        raise RuntimeError("oracle/_ref/ does not hold the reference programs: run oracle/ref_build/build_ref.py on a machine with the reference tree")
    if not build_ref.current():
        raise RuntimeError("oracle/_ref/ was compiled against other stand-in headers than oracle/ref_build/include/ holds now (an mpi.h of one rank "
                           "ignores CRD_REF_MPI_SIZE): run oracle/ref_build/build_ref.py on a machine with the reference tree")
    made = {}
    with tempfile.TemporaryDirectory() as work:
        for case in CASES:
            made[PREFIX + case["tag"] + ".npz"] = make_case(case, work)
        # the size conditions hold before anything is written
        sizes = {}
        for name, rec in made.items():
            path = os.path.join(work, name)
            mf.save_npz(path, rec)
            sizes[name] = os.path.getsize(path)
        if max(sizes.values()) > MAX_FIXTURE_BYTES or sum(sizes.values()) >= MAX_TOTAL_BYTES:
            raise RuntimeError("rank fixtures too large, nothing written: %s, total %d" % (sizes, sum(sizes.values())))
        os.makedirs(out_dir, exist_ok=True)
        for name in made:
            with open(os.path.join(work, name), "rb") as src, open(os.path.join(out_dir, name), "wb") as dst:
                dst.write(src.read())
    return sizes


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else mf.GOLDEN
    for name, size in sorted(make_all(out).items()):
        print("%8d  %s" % (size, name))
