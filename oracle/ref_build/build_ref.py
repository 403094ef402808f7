"""Compile the reference's four programs, UNMODIFIED, against the stand-in headers of oracle/ref_build/include into oracle/_ref/.

    python oracle/ref_build/build_ref.py [REFERENCE_DIR] [--force]

The reference tree is the argument, else $CRD_REFERENCE_DIR, else /root/reference.  Where none of these holds the four sources
(a machine without the reference tree) nothing is built and nothing is said.  Each source is compiled twice with
g++ -ffp-contract=off, at -O0 (what the reference's CMakeLists.txt gives: it sets no optimisation level) and at -O2, into
oracle/_ref/O0/ and oracle/_ref/O2/; make_fixtures.py requires the two to write identical bytes.  oracle/_ref/ is never committed.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "_ref")
PROGRAMS = ("FHNmodel_torus", "FHNmodel_flat", "GoldbeterModel_torus", "GoldbeterModel_flat")
LEVELS = ("O0", "O2")
# -fno-builtin-sin -fno-builtin-cos: at -O2 gcc would otherwise merge sin(x) and cos(x) into one sincos(x), whose sine is not glibc's
# sin(x) everywhere (one ulp apart at some theta); with them both levels make the libm calls the sources name (README.md)
FLAGS = ["-ffp-contract=off", "-fno-builtin-sin", "-fno-builtin-cos", "-w"]


def reference_dir(arg=None):
    """The reference tree, or None where there is none."""
    for d in (arg, os.environ.get("CRD_REFERENCE_DIR"), "/root/reference"):
        if d and all(os.path.isfile(os.path.join(d, "src", p + ".cpp")) for p in PROGRAMS):
            return os.path.abspath(d)
    return None


def sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def built():
    """True when oracle/_ref/ holds all eight programs and the provenance record."""
    return (all(os.access(os.path.join(OUT, lv, p), os.X_OK) for lv in LEVELS for p in PROGRAMS)
            and os.path.isfile(os.path.join(OUT, "provenance.json")))


def provenance():
    with open(os.path.join(OUT, "provenance.json")) as f:
        return json.load(f)


def stand_in_hashes():
    """{path under oracle/ref_build: SHA-256} of every stand-in header as it is now."""
    headers = sorted(os.path.join(d, f) for d, _, fs in os.walk(os.path.join(HERE, "include")) for f in fs)
    return {os.path.relpath(h, HERE): sha256(h) for h in headers}


def current():
    """True when oracle/_ref/ is built AND was compiled against the stand-in headers as they are now.  Programs compiled against an
    earlier mpi.h know one rank only: they ignore CRD_REF_MPI_SIZE, and every rank process of a run writes rank 0's files."""
    return built() and provenance().get("stand_ins") == stand_in_hashes()


def build(ref=None, force=False):
    """Returns the output directory, or None where no reference tree exists."""
    ref = reference_dir(ref)
    if ref is None:
        return None
    cxx = shutil.which(os.environ.get("CXX", "g++")) or "g++"
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True, check=True).stdout.splitlines()[0]
    record = {"compiler": version, "flags": {lv: ["-" + lv] + FLAGS for lv in LEVELS},
              "sources": {p + ".cpp": sha256(os.path.join(ref, "src", p + ".cpp")) for p in PROGRAMS},
              "stand_ins": stand_in_hashes()}
    if not force and built() and provenance() == record:
        return OUT
    for lv in LEVELS:
        os.makedirs(os.path.join(OUT, lv), exist_ok=True)
        for p in PROGRAMS:
            subprocess.run([cxx, "-" + lv] + FLAGS + ["-I", os.path.join(HERE, "include"), os.path.join(ref, "src", p + ".cpp"), "-o",
                            os.path.join(OUT, lv, p), "-lm"], check=True)
    os.makedirs(os.path.join(OUT, "bin"), exist_ok=True)
    script = os.path.join(OUT, "bin", "SolveGoldbeterODE.py")
    shutil.copyfile(os.path.join(HERE, "bin", "SolveGoldbeterODE.py"), script)
    os.chmod(script, 0o755)
    with open(os.path.join(OUT, "provenance.json"), "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
    return OUT


if __name__ == "__main__":
    _dirs = [a for a in sys.argv[1:] if not a.startswith("--")]
    build(_dirs[0] if _dirs else None, force="--force" in sys.argv)
