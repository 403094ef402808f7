"""CPU-side checks of the run recorder (crd_recorder_*, crd_run --observe without --ensemble): the header's declarations from plain C,
the ctypes table against the header, the ABI number, and what the driver refuses before any device is asked for.  No kernel is
launched."""
import ctypes as C
import os
import re
import subprocess

import pytest

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
SMALL_INI = os.path.join(GOLDEN, "ini", "small_run.ini")
capi = crd._capi
NAMES = ["crd_recorder_open", "crd_recorder_count", "crd_recorder_info", "crd_recorder_read", "crd_recorder_section_info", "crd_recorder_read_section",
         "crd_recorder_maps", "crd_recorder_cycles", "crd_recorder_close"]


def test_recorder_declarations_link_from_c(tmp_path):
    src = tmp_path / "rec.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "crd.h"
int main(void) {
	crd_recorder *r = (crd_recorder *)0; crd_ctx *none[1] = {(crd_ctx *)0}; crd_observe_options o; crd_observe_extras x;
	int32_t kind = 0, index = 0, slabs = 0, cnt[4]; int64_t n = 0, d = 0, values = 0, cap = 0, length = 0; double v[8];
	memset(&o, 0, sizeof o); memset(&x, 0, sizeof x);
	o.stride = 1;
	if (CRD_ABI_VERSION != 8 || crd_abi_version() != CRD_ABI_VERSION) return 1;
	if (crd_recorder_open((crd_ctx *const *)0, 1, &o, &x, 4, &r) != CRD_EINVAL) return 2;
	if (crd_recorder_open(none, 1, &o, (const crd_observe_extras *)0, 4, &r) != CRD_EINVAL || r) return 3;
	if (crd_recorder_count(r, &n) != CRD_EINVAL) return 4;
	if (crd_recorder_info(r, &d, &values, &slabs, &o, &x, &cap) != CRD_EINVAL) return 5;
	if (crd_recorder_read(r, 0, 0, v, v, v) != CRD_EINVAL) return 6;
	if (crd_recorder_section_info(r, 0, &kind, &index, &length, &d) != CRD_EINVAL) return 7;
	if (crd_recorder_read_section(r, 0, 0, 0, v) != CRD_EINVAL) return 8;
	if (crd_recorder_maps(r, v, v, v) != CRD_EINVAL) return 9;
	if (crd_recorder_cycles(r, cnt, v, v) != CRD_EINVAL) return 10;
	if (crd_recorder_close(r) != CRD_EINVAL) return 11;
	printf("ok\n");
	return 0;
}
''')
    exe = tmp_path / "rec"
    libdir = os.path.join(ROOT, "crdmodel_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lcrd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout, r.stderr)


def test_capi_mirrors_the_header():
    header = open(os.path.join(ROOT, "include", "crd.h")).read()
    assert "#define CRD_ABI_VERSION 8" in header and capi.ABI_VERSION == 8 and capi.lib().crd_abi_version() == 8
    declared = re.findall(r"^int (crd_recorder_\w+)\(([^;]*)\);", header, flags=re.M | re.S)
    assert [name for name, _ in declared] == NAMES
    for name, args in declared:
        res, argtypes = capi._SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == len(args.split(",")), name
        assert hasattr(capi.lib(), name)
    assert "typedef struct crd_recorder crd_recorder;" in header
    assert "No observers on multi-slab runs" not in header


def test_null_handles_are_refused():
    L = capi.lib()
    n, buf, cnt = C.c_int64(), (C.c_double * 8)(), (C.c_int32 * 8)()
    opt = capi.ObserveOptions()
    opt.stride = 1
    h = C.c_void_p()
    assert L.crd_recorder_open(None, 1, C.byref(opt), None, 4, C.byref(h)) == capi.EINVAL and not h
    assert L.crd_recorder_count(None, C.byref(n)) == capi.EINVAL
    assert L.crd_recorder_read(None, 0, 0, buf, buf, buf) == capi.EINVAL
    assert L.crd_recorder_read_section(None, 0, 0, 0, buf) == capi.EINVAL
    assert L.crd_recorder_maps(None, buf, buf, buf) == capi.EINVAL and L.crd_recorder_cycles(None, cnt, buf, buf) == capi.EINVAL
    assert L.crd_recorder_close(None) == capi.EINVAL


def crd_run(*args):
    return subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus"] + list(args) + [SMALL_INI], capture_output=True, text=True,
                          timeout=120)


@pytest.mark.parametrize("args,needles", [
    (["--observe", "2", "--probe", "3,2", "--gpus", "4", "--decomp", "2x2"], ["--observe", "--decomp"]),
    (["--observe", "2", "--probe", "3,2", "--gpus", "2", "--decomp", "mpi"], ["--observe", "--decomp"]),
    (["--observe", "2", "--probe", "3,2", "--block-contexts"], ["--observe", "--block-contexts"]),
    (["--observe", "2", "--section", "phi-mean", "--gpus", "2", "--devices", "1"], ["--section phi-mean", "more than one slab"]),
    (["--observe", "0", "--probe", "3,2"], ["--observe", "stride"]),
    (["--observe", "2", "--probe", "16,0"], ["--probe 16,0", "16 x 40"]),            # small_run.ini: a 16 x 40 grid
    (["--observe", "2", "--section", "row:40"], ["--section row:40", "16 x 40"]),
    (["--observe", "2", "--probe", "1,1"] + ["--section", "theta-mean"] * 9, ["--section", "at most 8"]),
])
def test_driver_refusals_of_a_recorded_run(args, needles, tmp_path):
    """Each exits non-zero naming the reason, before any device is asked for (no "no HIP device" message) and before any file."""
    r = crd_run("--outdir", str(tmp_path), *args)
    assert r.returncode != 0 and "CRD_ERROR" in r.stderr and all(n in r.stderr for n in needles), r.stderr
    assert "no HIP device" not in r.stderr and "crd_create" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []
