"""CPU-side checks of the observers' sections and cycle maps (crd_ensemble_observe_begin_with, crd_ensemble_observe_section_info /
_read_section / _cycles, crd_state_section, crd_run --section / --observe-cycles, post.period_map, post.plot_kymograph): the ctypes
mirror of crd_observe_extras against the C struct, what is refused before any device is touched, and the post-processing on made-up
arrays.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT
from crdmodel_amd import post

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
SMALL_INI = os.path.join(GOLDEN, "ini", "small_run.ini")
capi = crd._capi
EINVAL = capi.EINVAL


def extras(sections=(), cycles=0, cycle_threshold=0.0, n_sections=None):
    ex = capi.ObserveExtras()
    ex.n_sections = len(sections) if n_sections is None else n_sections
    ex.cycles, ex.cycle_threshold = cycles, cycle_threshold
    for q, (kind, index) in enumerate(sections):
        ex.kind[q], ex.index[q] = kind, index
    return ex


def test_null_handles_are_refused():
    """Every refusal of the new entry points, on a NULL ensemble / context: CRD_EINVAL, and no HIP call is made to get there (the
    machine that runs this has no device: a HIP call would answer CRD_EHIP)."""
    L = capi.lib()
    opt = capi.ObserveOptions()
    opt.stride = 1
    good = extras([(capi.SECTION_ROW, 0), (capi.SECTION_PHI_MEAN, 0)], cycles=1, cycle_threshold=0.5)
    assert L.crd_ensemble_observe_begin_with(None, C.byref(opt), C.byref(good), 4) == EINVAL
    assert L.crd_ensemble_observe_begin_with(None, C.byref(opt), None, 4) == EINVAL
    for bad in (extras(n_sections=-1), extras(n_sections=capi.OBSERVE_MAX_SECTIONS + 1), extras([(4, 0)]), extras([(-1, 0)]),
                extras([(capi.SECTION_ROW, -1)]), extras([(capi.SECTION_ROW, 1 << 30)]), extras([(capi.SECTION_COLUMN, -1)]),
                extras([(capi.SECTION_COLUMN, 1 << 30)]), extras(cycles=1, cycle_threshold=float("nan")), extras(cycles=1, cycle_threshold=float("inf")),
                extras(cycles=2)):
        assert L.crd_ensemble_observe_begin_with(None, C.byref(opt), C.byref(bad), 4) == EINVAL
    kind, index, length, additions = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    buf = (C.c_double * 8)()
    cnt = (C.c_int32 * 8)()
    assert L.crd_ensemble_observe_section_info(None, 0, C.byref(kind), C.byref(index), C.byref(length), C.byref(additions)) == EINVAL
    assert L.crd_ensemble_observe_read_section(None, 0, 0, 0, buf) == EINVAL
    assert L.crd_ensemble_observe_cycles(None, 0, cnt, buf, buf) == EINVAL
    for k, i in ((capi.SECTION_ROW, 0), (capi.SECTION_THETA_MEAN, 0), (7, 0), (capi.SECTION_COLUMN, -1)):
        assert L.crd_state_section(None, k, i, buf) == EINVAL


def test_extras_struct_matches_the_header():
    header = open(os.path.join(ROOT, "include", "crd.h")).read()
    assert "#define CRD_OBSERVE_MAX_SECTIONS %d" % capi.OBSERVE_MAX_SECTIONS in header
    for name, value in (("ROW", capi.SECTION_ROW), ("COLUMN", capi.SECTION_COLUMN), ("THETA_MEAN", capi.SECTION_THETA_MEAN), ("PHI_MEAN", capi.SECTION_PHI_MEAN)):
        assert "#define CRD_SECTION_%s %d" % (name, value) in header
    assert capi.SECTION_KINDS == {"row": 0, "column": 1, "theta_mean": 2, "phi_mean": 3}
    assert C.sizeof(capi.ObserveExtras) == 4 + 4 + 2 * 4 * capi.OBSERVE_MAX_SECTIONS + 8
    assert "#define CRD_ABI_VERSION 8" in header and capi.ABI_VERSION == 8 and capi.lib().crd_abi_version() == 8


def test_section_declarations_link_from_c(tmp_path):
    """The header's declarations compiled from plain C: the struct's size and field offsets are the ctypes mirror's, the ABI number is
    still 8, crd_observe_options kept its size, and the refusals come back through the C ABI."""
    src = tmp_path / "sec.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "crd.h"
int main(void) {
	crd_ensemble *e = (crd_ensemble *)0; crd_observe_options o; crd_observe_extras x; int32_t kind = 0, index = 0, cnt[4]; int64_t length = 0, d = 0; double v[8];
	memset(&o, 0, sizeof o); memset(&x, 0, sizeof x);
	o.stride = 1;
	x.n_sections = 2; x.kind[0] = CRD_SECTION_COLUMN; x.index[0] = 3; x.kind[CRD_OBSERVE_MAX_SECTIONS - 1] = CRD_SECTION_PHI_MEAN; x.cycles = 1; x.cycle_threshold = 0.5;
	if (CRD_ABI_VERSION != 8 || crd_abi_version() != CRD_ABI_VERSION) return 1;
	if (CRD_SECTION_ROW != 0 || CRD_SECTION_COLUMN != 1 || CRD_SECTION_THETA_MEAN != 2 || CRD_SECTION_PHI_MEAN != 3) return 2;
	if (crd_ensemble_observe_begin_with(e, &o, &x, 16) != CRD_EINVAL) return 3;
	if (crd_ensemble_observe_begin_with(e, &o, (const crd_observe_extras *)0, 16) != CRD_EINVAL) return 4;
	if (crd_ensemble_observe_section_info(e, 0, &kind, &index, &length, &d) != CRD_EINVAL) return 5;
	if (crd_ensemble_observe_read_section(e, 0, 0, 1, v) != CRD_EINVAL) return 6;
	if (crd_ensemble_observe_cycles(e, 0, cnt, v, v) != CRD_EINVAL) return 7;
	if (crd_state_section((crd_ctx *)0, CRD_SECTION_THETA_MEAN, 0, v) != CRD_EINVAL) return 8;
	printf("ok %d %d %d %d %d %d %d\n", (int)sizeof x, (int)offsetof(crd_observe_extras, n_sections), (int)offsetof(crd_observe_extras, cycles),
	       (int)offsetof(crd_observe_extras, kind), (int)offsetof(crd_observe_extras, index), (int)offsetof(crd_observe_extras, cycle_threshold), (int)sizeof o);
	return 0;
}
''')
    exe = tmp_path / "sec"
    libdir = os.path.join(ROOT, "crdmodel_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lcrd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    X = capi.ObserveExtras
    assert r.stdout.split() == ["ok"] + [str(v) for v in (C.sizeof(X), X.n_sections.offset, X.cycles.offset, X.kind.offset, X.index.offset, X.cycle_threshold.offset,
                                                          C.sizeof(capi.ObserveOptions))], r.stdout


def crd_run(*args):
    return subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus"] + list(args) + [SMALL_INI], capture_output=True, text=True,
                          timeout=120)


@pytest.mark.parametrize("args,needle", [
    (["--section", "row:0"], "--section"),                                                            # no --ensemble
    (["--observe-cycles", "0.0"], "--observe-cycles"),
    (["--ensemble", "beta=1,1.2", "--section", "theta-mean"], "--section"),                           # no --observe
    (["--ensemble", "beta=1,1.2", "--observe-cycles", "0.0"], "--observe-cycles"),
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--section", "diagonal"], "--section"),
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--section", "row"], "--section"),
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--section", "row:"], "--section"),
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--section", "column:x"], "--section"),
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--section", "row:40"], "--section"),             # small_run.ini: a 16 x 40 grid
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--section", "row:-1"], "--section"),
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--section", "column:16"], "--section"),
    (["--ensemble", "beta=1,1.2", "--observe", "2"] + ["--section", "phi-mean"] * 9, "--section"),    # one more than CRD_OBSERVE_MAX_SECTIONS
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--observe-cycles", "high"], "--observe-cycles"),
    (["--ensemble", "beta=1,1.2", "--observe", "2", "--observe-cycles", "nan"], "--observe-cycles"),
])
def test_driver_usage_errors(args, needle, tmp_path):
    """Each exits non-zero with a message naming the option, before any device is asked for (no "no HIP device" message, no files)."""
    g = crd.grid_of(crd.load_ini(SMALL_INI, "fhn", "torus").params)
    assert (g.nx, g.ny) == (16, 40)  # (what makes row 40 and column 16 lie outside)
    r = crd_run("--outdir", str(tmp_path), *args)
    assert r.returncode != 0 and "CRD_ERROR" in r.stderr and needle in r.stderr, r.stderr
    assert "device" not in r.stderr and "crd_ensemble_create" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


def test_period_map_on_made_up_planes():
    count = np.array([[0, 1, 2], [3, 5, 2]], dtype=np.int32)
    t_first = np.array([[np.nan, 0.5, 0.25], [1.0, 0.5, 2.0]])
    t_last = np.array([[np.nan, 0.5, 1.0], [2.0, 2.5, 2.0]])
    got = post.period_map(count, t_first, t_last)
    assert got.shape == (2, 3) and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), count < 2)
    assert got[0, 2] == 0.75 and got[1, 0] == 0.5 and got[1, 1] == 0.5 and got[1, 2] == 0.0
    with pytest.raises(ValueError):
        post.period_map(count, t_first[:1], t_last)


def test_kymograph_of_a_made_up_section(tmp_path):
    """A travelling sine as [sample, length, 2]: the image holds the chosen field's values, sample 0 at the bottom, and is written."""
    t = np.linspace(0.0, 3.0, 31)
    x = np.arange(48)
    section = np.stack([np.sin(0.3 * x[None, :] - 2.0 * t[:, None]), np.cos(0.1 * x[None, :] + t[:, None])], axis=-1)
    path = tmp_path / "kymograph.png"
    fig = post.plot_kymograph(section, t, var=1, path=str(path))
    assert path.exists() and path.stat().st_size > 0
    img = fig.axes[0].images[0]
    assert np.array_equal(np.asarray(img.get_array()), section[:, :, 1]) and img.origin == "lower"
    assert list(img.get_extent()) == [0.0, 48.0, 0.0, 3.0]
    with pytest.raises(ValueError):
        post.plot_kymograph(section[:, :, 0], t)
    with pytest.raises(ValueError):
        post.plot_kymograph(section, t[:-1])
