"""CPU-side checks of the observers (crd_ensemble_observe_*, crd_state_observe, crd_run --observe, post.oscillation_summary): what is
refused before any device is touched, the header's declarations compiled from plain C, and the period / amplitude estimate on a series
whose answer is known.  No kernel is launched."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT
from crdmodel_amd import post

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
SMALL_INI = os.path.join(GOLDEN, "ini", "small_run.ini")


def test_null_handles_are_refused():
    L = crd._capi.lib()
    EINVAL = crd._capi.EINVAL
    opt = crd._capi.ObserveOptions()
    opt.stride = 1
    n, blocks, values, cap = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64()
    buf = (C.c_double * 8)()
    assert L.crd_ensemble_observe_begin(None, C.byref(opt), 4) == EINVAL
    assert L.crd_ensemble_observe_count(None, C.byref(n)) == EINVAL
    assert L.crd_ensemble_observe_read(None, 0, 0, None, None, None) == EINVAL
    assert L.crd_ensemble_observe_maps(None, 0, None, None, None) == EINVAL
    assert L.crd_ensemble_observe_info(None, C.byref(blocks), C.byref(values), C.byref(opt), C.byref(cap)) == EINVAL
    assert L.crd_ensemble_observe_end(None) == EINVAL
    assert L.crd_state_observe(None, buf) == EINVAL


def test_options_struct_matches_the_header():
    """The ctypes mirror of crd_observe_options has the header's probe limit and, through it, the C struct's size (checked from C below)."""
    header = open(os.path.join(ROOT, "include", "crd.h")).read()
    assert "#define CRD_OBSERVE_MAX_PROBES %d" % crd._capi.OBSERVE_MAX_PROBES in header
    assert C.sizeof(crd._capi.ObserveOptions) == 8 + 4 + 4 + 2 * 4 * crd._capi.OBSERVE_MAX_PROBES + 8


def test_observer_declarations_link_from_c(tmp_path):
    src = tmp_path / "obs.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "crd.h"
int main(void) {
	crd_ensemble *e = (crd_ensemble *)0; crd_observe_options o; int64_t n = 0, cap = 0, values = 0; int32_t blocks = 0; double x[8];
	memset(&o, 0, sizeof o);
	o.stride = 1; o.n_probes = 1; o.probe_i[0] = 3; o.probe_j[CRD_OBSERVE_MAX_PROBES - 1] = 0; o.maps = 1; o.threshold = 0.5;
	if (CRD_ABI_VERSION != 8 || crd_abi_version() != CRD_ABI_VERSION) return 1;
	if (crd_ensemble_observe_begin(e, &o, 16) != CRD_EINVAL) return 2;
	if (crd_ensemble_observe_count(e, &n) != CRD_EINVAL) return 3;
	if (crd_ensemble_observe_read(e, 0, 1, x, x, x) != CRD_EINVAL) return 4;
	if (crd_ensemble_observe_maps(e, 0, x, x, x) != CRD_EINVAL) return 5;
	if (crd_ensemble_observe_info(e, &blocks, &values, &o, &cap) != CRD_EINVAL) return 6;
	if (crd_ensemble_observe_end(e) != CRD_EINVAL) return 7;
	if (crd_state_observe((crd_ctx *)0, x) != CRD_EINVAL) return 8;
	printf("ok %d\n", (int)sizeof o);
	return 0;
}
''')
    exe = tmp_path / "obs"
    libdir = os.path.join(ROOT, "crdmodel_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lcrd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stdout.split() == ["ok", str(C.sizeof(crd._capi.ObserveOptions))], r.stdout


def crd_run(*args):
    return subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus"] + list(args) + [SMALL_INI], capture_output=True, text=True,
                          timeout=120)


@pytest.mark.parametrize("args,needle", [
    (["--observe", "2"], "--observe"),                                                      # no --ensemble
    (["--ensemble", "beta=1,1.2", "--observe", "0"], "--observe"),
    (["--ensemble", "beta=1,1.2", "--observe", "-3"], "--observe"),
    (["--ensemble", "beta=1,1.2", "--observe", "x"], "--observe"),
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--probe", "16,0"], "--probe"),         # small_run.ini: a 16 x 40 grid
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--probe", "0,40"], "--probe"),
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--probe", "-1,3"], "--probe"),
    (["--ensemble", "beta=1,1.2", "--probe", "1,3"], "--probe"),                            # no --observe
    (["--ensemble", "beta=1,1.2", "--observe-maps", "0.5"], "--observe-maps"),
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--observe-maps", "high"], "--observe-maps"),
])
def test_driver_usage_errors(args, needle, tmp_path):
    """Each exits non-zero with a message naming the option, before any device is asked for (no "no HIP device" message, no files)."""
    g = crd.grid_of(crd.load_ini(SMALL_INI, "fhn", "torus").params)
    assert (g.nx, g.ny) == (16, 40)  # (what makes the probes above lie outside)
    r = crd_run("--outdir", str(tmp_path), *args)
    assert r.returncode != 0 and "CRD_ERROR" in r.stderr and needle in r.stderr, r.stderr
    assert "device" not in r.stderr and "crd_ensemble_create" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


def test_oscillation_summary_on_a_sampled_sine():
    """x(t) = c + A sin(2 pi t / T + phase), sampled every h over several periods.
    Period: the estimate is the mean spacing of interpolated upward crossings.  A crossing is placed inside the sample interval that
    contains it, so each is off by less than h, and so is the mean spacing of k crossings (2 h / (k - 1) <= h for k >= 3): within one
    sample interval, as asserted.
    Amplitude: the nearest sample to a crest is at most h / 2 away from it, where the sine has dropped by A (1 - cos(pi h / T)); the same
    at the trough.  So 2 A - 2 A (1 - cos(pi h / T)) <= max - min <= 2 A."""
    T, A, c, h, phase = 7.3, 1.7, 0.4, 0.11, 0.37
    t = np.arange(0.0, 5.2 * T, h)
    x = c + A * np.sin(2.0 * math.pi * t / T + phase)
    s = post.oscillation_summary(t, x)
    assert s["crossings"] >= 3
    assert abs(s["period"] - T) <= h, s
    loss = 2.0 * A * (1.0 - math.cos(math.pi * h / T))
    assert 2.0 * A - loss <= s["amplitude"] <= 2.0 * A, (s, loss)


def test_oscillation_summary_without_an_oscillation():
    t = np.linspace(0.0, 10.0, 101)
    s = post.oscillation_summary(t, np.full_like(t, 0.25))
    assert math.isnan(s["period"]) and s["amplitude"] == 0.0
    # one upward crossing is not a period either: a relaxation through its mean and back
    s = post.oscillation_summary(t, np.exp(-t) * np.sin(0.5 * t))
    assert s["crossings"] < 2 and math.isnan(s["period"])
