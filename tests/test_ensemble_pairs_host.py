"""CPU-side checks of two steps per launch on ensembles: the two entry points in the header and the ctypes table, compiled from plain C;
what crd_run --ensemble-steps refuses before any device is touched; tools/kernel_regs.py --check on the pair unit's kept assembly and
on two hand-written files; the pair kernels' registers against the single-slab two-step kernels'.  No kernel is launched."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
BUILD = os.path.join(ROOT, "crdmodel_amd", "csrc", "build")
PAIR_ASM = os.path.join(BUILD, "crd_ensemble_multi-hip-amdgcn-amd-amdhsa-gfx950.s")
KERNEL_REGS = os.path.join(ROOT, "tools", "kernel_regs.py")
SMALL_INI = os.path.join(GOLDEN, "ini", "small_run.ini")
HEADER = os.path.join(ROOT, "include", "crd.h")

# fp64 / fp32 x FHN (0) / Goldbeter (1) / diffusion-only (2) x plain / absorbing (none for diffusion-only); one column per lane in fp64,
# one or two in fp32
PAIR_KERNELS = sorted([("double", m, a, 1) for m in (0, 1) for a in (False, True)] + [("double", 2, False, 1)] +
                      [("float", m, a, c) for m in (0, 1) for a in (False, True) for c in (1, 2)] + [("float", 2, False, c) for c in (1, 2)])


@pytest.fixture(scope="module")
def pair_asm():
    """The pair unit's device assembly as the build keeps it (the session's build, or this one's)."""
    if not os.path.exists(PAIR_ASM):
        from crdmodel_amd.build import build

        build()
    assert os.path.exists(PAIR_ASM), "the build keeps crd_ensemble_multi's device assembly"
    return PAIR_ASM


def test_entry_points_in_header_and_ctypes_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+crd_ensemble_set_steps_per_launch\s*\(\s*crd_ensemble\s*\*\s*e\s*,\s*int\s+steps\s*\)\s*;", text)
    assert re.search(r"\bint\s+crd_ensemble_get_steps_per_launch\s*\(\s*const\s+crd_ensemble\s*\*\s*e\s*\)\s*;", text)
    sig = crd._capi._SIGNATURES
    assert sig["crd_ensemble_set_steps_per_launch"] == (C.c_int, [C.c_void_p, C.c_int])
    assert sig["crd_ensemble_get_steps_per_launch"] == (C.c_int, [C.c_void_p])
    assert "#define CRD_ABI_VERSION 8" in open(HEADER).read() and crd._capi.ABI_VERSION == 8 and crd._capi.lib().crd_abi_version() == 8
    assert re.search(r"#define CRD_ENSEMBLE_PAIR_MIN_ROWS 9\b", open(HEADER).read())
    L = crd._capi.lib()
    assert L.crd_ensemble_set_steps_per_launch(None, 2) == crd._capi.EINVAL and L.crd_ensemble_get_steps_per_launch(None) == crd._capi.EINVAL


def test_entry_points_compile_and_link_from_c(tmp_path):
    src = tmp_path / "pairs.c"
    src.write_text(r'''
#include <stdio.h>
#include "crd.h"
int main(void) {
	crd_ensemble *e = (crd_ensemble *)0;
	int (*set)(crd_ensemble *, int) = crd_ensemble_set_steps_per_launch;
	int (*get)(const crd_ensemble *) = crd_ensemble_get_steps_per_launch;
	if (CRD_ABI_VERSION != 8 || crd_abi_version() != CRD_ABI_VERSION) return 1;
	if (CRD_ENSEMBLE_PAIR_MIN_ROWS <= 8) return 2;
	if (set(e, 2) != CRD_EINVAL || set(e, 1) != CRD_EINVAL || get(e) != CRD_EINVAL) return 3;
	printf("ok\n");
	return 0;
}
''')
    exe = tmp_path / "pairs"
    libdir = os.path.join(ROOT, "crdmodel_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lcrd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout, r.stderr)


def crd_run(*args, ini=SMALL_INI):
    return subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus"] + list(args) + [ini], capture_output=True, text=True, timeout=120)


def test_driver_refuses_ensemble_steps_without_an_ensemble():
    r = crd_run("--ensemble-steps", "2")
    assert r.returncode != 0 and "--ensemble-steps" in r.stderr and "needs --ensemble" in r.stderr, r.stderr


@pytest.mark.parametrize("value", ["3", "0", "two", "-2", "2.0"])
def test_driver_refuses_a_bad_steps_value(value):
    r = crd_run("--ensemble", "beta=0.9,1.25", "--ensemble-steps", value)
    assert r.returncode != 0 and "--ensemble-steps takes 1 or 2" in r.stderr and value in r.stderr, r.stderr


def test_driver_refuses_ensemble_steps_with_adaptive(tmp_path):
    ini = tmp_path / "adaptive.ini"
    ini.write_text(open(SMALL_INI).read().replace("[Solver]\n", "[Solver]\nadaptive = 1\n"))
    assert "adaptive = 1" in ini.read_text()
    r = crd_run("--ensemble", "beta=0.9,1.25", "--ensemble-steps", "2", "--outdir", str(tmp_path), ini=str(ini))
    assert r.returncode != 0 and "--ensemble-steps" in r.stderr and "adaptive = 1" in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("member_")]  # refused before anything was created
    r = crd_run("--ensemble", "beta=0.9,1.25", "--ensemble-steps", "2", "--adaptive")
    assert r.returncode != 0 and "--adaptive" in r.stderr, r.stderr


def kernel_regs_check(*paths, cwd):
    return subprocess.run([sys.executable, KERNEL_REGS, "--check", "--asm"] + list(paths), capture_output=True, text=True, cwd=cwd, timeout=300)


def test_check_mode_passes_the_pair_unit_and_reports_every_pair_kernel(pair_asm, tmp_path):
    r = kernel_regs_check(pair_asm, cwd=tmp_path)
    assert r.returncode == 0, (r.stdout, r.stderr)
    reported = re.findall(r"^ok\s+crd_ensemble_pair_kernel<(double|float), (\d+), (true|false), (\d+)>\s*$", r.stdout, flags=re.M)
    assert sorted((real, int(m), a == "true", int(c)) for real, m, a, c in reported) == PAIR_KERNELS, r.stdout
    assert "FAIL" not in r.stdout and os.listdir(tmp_path) == []
    # every kernel of the unit is reported, and the unit holds the pair kernels alone: crd_fused_impl.h is device bodies only, the
    # single-slab launcher's error-sum kernel (crd_fused_launch.h) is not this unit's
    assert "crd_sum_partials_kernel" not in r.stdout, r.stdout
    assert len(re.findall(r"^(ok|FAIL)\s", r.stdout, flags=re.M)) == len(PAIR_KERNELS)


def test_check_mode_refuses_a_store_behind_an_exec_branch(tmp_path):
    bad = os.path.join(GOLDEN, "kernel_regs", "exec_skipped_store.s")
    good = os.path.join(GOLDEN, "kernel_regs", "straight_store.s")
    branch = [ln for ln in open(bad) if "s_cbranch_execz" in ln]
    assert len(branch) == 1 and not [ln for ln in open(good) if "s_cbranch" in ln]
    r = kernel_regs_check(bad, cwd=tmp_path)
    assert r.returncode != 0 and "FAIL" in r.stdout and "pair_like_kernel" in r.stderr and "execution mask" in r.stderr, (r.returncode, r.stdout, r.stderr)
    assert os.listdir(tmp_path) == []  # no output file
    r = kernel_regs_check(good, cwd=tmp_path)
    assert r.returncode == 0 and re.search(r"^ok\s+pair_like_kernel", r.stdout, flags=re.M), (r.returncode, r.stdout, r.stderr)
    r = kernel_regs_check(good, bad, cwd=tmp_path)  # one violating file among several
    assert r.returncode != 0
    # --check writes no table: asking for one beside it is an error, and nothing is written
    r = subprocess.run([sys.executable, KERNEL_REGS, "--check", "--asm", good, "--table", str(tmp_path / "t.inc")], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0 and os.listdir(tmp_path) == []


def test_pair_kernels_sit_at_the_single_slab_two_step_kernels_occupancy(pair_asm):
    """No scratch, and the wavefronts per SIMD of crd_rk4_fused_step_kernel<..., STEPS = 2> of the same precision / model / absorb /
    columns (plain stores), from this build's kernel table.  The diffusion-only variant has no single-slab two-step kernel: its pairs are
    held to no scratch and to more wavefronts than the model kernels of their precision and columns."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    pairs = {}
    for k in kernel_regs.parse(open(pair_asm).read()):
        m = re.match(r"crd_ensemble_pair_kernel<(double|float), (\d+), (true|false), (\d+)>", k["name"])
        if m:
            pairs[(m.group(1), int(m.group(2)), m.group(3) == "true", int(m.group(4)))] = k
    assert sorted(pairs) == PAIR_KERNELS
    table = json.load(open(os.path.join(BUILD, "kernel_table.json")))["kernels"]
    single = {("double" if r["precision"] == "f64" else "float", r["model"], bool(r["absorb"]), r["cols"]): r
              for r in table if r["steps"] == 2 and r["embed"] == 0 and r["nt"] == 0}
    for key, k in pairs.items():
        assert k["scratch"] == 0 and k["exec_skipped_vmem"] == 0 and k["async_lds_read_hazards"] == 0, (key, k)
        if key[1] == 2:
            assert key not in single and k["occupancy"] >= pairs[(key[0], 0, False, key[3])]["occupancy"], key
        else:
            assert k["occupancy"] == single[key]["wavefronts_per_simd"], (key, k["vgprs"], single[key]["vgprs"])
            assert k["lds"] == single[key]["lds_bytes"], key
