"""What crd_run refuses before any device is asked for, byte for byte: exit status, stdout and stderr of each command line in
tests/golden/driver_refusals.json -- the single faults, and pairs of faults that pin which of the two is reported.  The other host tests
pin a substring per message; this one pins the status, the precedence and the silence of stdout too.  No kernel is launched, so the
test gives the same result with and without a GPU."""
import json
import os
import subprocess

from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
SMALL_INI = os.path.join(GOLDEN, "ini", "small_run.ini")
LAUNCHER_PREFIXES = ("OMPI_", "PMI_", "MV2_")  # (a launcher's rank and size are part of an entry, never inherited)


def test_driver_refusals_match_the_recorded_messages(tmp_path):
    """Each entry: argv0 (crd_run or an alias), args and launcher environment -> status, stdout, stderr, with the paths of the executable
    and of small_run.ini written {EXE} and {INI}.  Run in an empty directory, which must stay empty."""
    entries = json.load(open(os.path.join(GOLDEN, "driver_refusals.json")))
    assert len(entries) >= 36
    clean = {k: v for k, v in os.environ.items() if not k.startswith(LAUNCHER_PREFIXES)}
    for e in entries:
        exe = os.path.join(BIN, e["argv0"])
        r = subprocess.run([exe] + [a.replace("{INI}", SMALL_INI) for a in e["args"]], cwd=tmp_path, env=dict(clean, **e["env"]), capture_output=True, timeout=60)
        got = [r.returncode] + [s.decode().replace(exe, "{EXE}").replace(SMALL_INI, "{INI}") for s in (r.stdout, r.stderr)]
        assert got == [e["status"], e["stdout"], e["stderr"]], (e["argv0"], e["args"], e["env"])
        assert "no HIP device" not in got[2] and "crd_create" not in got[2], e["args"]
    assert os.listdir(tmp_path) == []
