"""Observer sections and cycle maps on the GPU (crd_ensemble_observe_begin_with, Ensemble.observe(sections=, cycles=),
Ensemble.observed_section / observed_cycles, Slab.section, crd_run --section / --observe-cycles).

The reference of every per-sample check is a second, identical run without an observer that downloads every member's state at every
sample.  Rows and columns are compared with ==; a mean against math.fsum(x) / n within D u sum|x| / n, D from
crd_ensemble_observe_section_info (include/crd.h derives it); the cycle planes with == against the rule of include/crd.h evaluated by
numpy on the downloaded states.

Shapes: 61 x 183 -- an odd point count: the second plane does not start on 16 bytes, most rows do not either, nx < 64, short last
group; 64 x 256 -- every row on 16 bytes: the 16-byte loads; 130 x 70 -- more than two wavefronts' worth of columns (three blocks of
the phi-mean, the last with two columns), ny no multiple of 4, nx > ny."""
import copy
import filecmp
import math
import os
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT
from crdmodel_amd import post
from oracle import crd_oracle as co

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
INI = os.path.join(GOLDEN, "ini")
U = 2.0 ** -53
capi = crd._capi
EINVAL = capi.EINVAL


def params_like(p, **kw):
    q = copy.copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def start_state(p, seed):
    y = crd.initial_conditions(crd.run_config(p, wave_length=0.1, wave_width=0.5, wave_inside=0))
    return y + 0.05 * np.random.default_rng(seed).standard_normal(y.shape)


def dtype_of(p):
    return np.float64 if p.precision == capi.PRECISION_F64 else np.float32


def members_of(model, precision, nx, ny):
    """Three members differing in beta, D and tBoundary (the pattern of test_gpu_observe.py)."""
    if model == "fhn":
        base = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, beta_min=0.7, beta_max=1.7, precision=precision, t_boundary=10.0)
        return [base, params_like(base, beta=0.9, diffusion=0.2), params_like(base, vary_beta=1, t_boundary=0.05)]
    base = crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, 0.4, ny=ny, precision=precision, t_boundary=10.0)
    return [base, params_like(base, beta=0.6), params_like(base, diffusion=0.3, t_boundary=0.005)]


def plain_run(members, ys, t0, dt, nsteps, every=1):
    """No observer: `every` steps per call, every member downloaded after every call.  states[sample][member]."""
    dtype = dtype_of(members[0])
    states = []
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        for s in range(nsteps // every):
            e.step_rk4(t0 + (s * every) * dt, dt, every)
            states.append([e.download(k, dtype) for k in range(len(members))])
    return states


def all_sections(nx, ny):
    return [("row", 0), ("row", ny - 1), ("column", 0), ("column", nx - 1), ("row", ny // 3), ("column", nx // 2), ("theta_mean",), ("phi_mean",)]


def expected_exact(section, state):
    """The line [length, 2] of an exact section of a downloaded state [ny, nx, 2]."""
    return state[section[1]].astype(np.float64) if section[0] == "row" else state[:, section[1]].astype(np.float64)


def check_means(kind, line, state, D, worst):
    """A theta_mean / phi_mean line [length, 2] against the downloaded state: |mean - fsum(x) / n| <= D u sum|x| / n."""
    for f in range(2):
        x = state[..., f].astype(np.float64)
        x = x if kind == "theta_mean" else x.T  # one line of x per value of the section
        n = x.shape[1]
        assert line.shape == (x.shape[0], 2)
        for q in range(x.shape[0]):
            err, bound = abs(line[q, f] - math.fsum(x[q]) / n), D * U * math.fsum(np.abs(x[q])) / n
            worst[0] = max(worst[0], err / bound)
            assert err <= bound, (kind, f, q, err, bound)


CONFIGS = [("fhn", "f64", 61, 183), ("goldbeter", "f32", 61, 183), ("fhn", "f32", 64, 0), ("goldbeter", "f64", 64, 0), ("fhn", "f64", 130, 70),
           ("goldbeter", "f32", 130, 70)]


@pytest.mark.parametrize("model,precision,nx,ny", CONFIGS)
def test_sections_match_the_downloaded_states(gpu_device, model, precision, nx, ny):
    """7 steps at stride 1: rows and columns == the state downloaded after the same step of the unobserved run, means within the bound
    D states, final states bit-equal to the unobserved run's."""
    members = members_of(model, precision, nx, ny)
    dtype = dtype_of(members[0])
    dt, nsteps, t0 = (0.02 if model == "fhn" else 0.002), 7, 0.0
    ys = [start_state(p, 3 + k).astype(dtype) for k, p in enumerate(members)]
    g = crd.grid_of(members[0])
    NX, NY = g.nx, g.ny
    sections = all_sections(NX, NY)
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.observe(stride=1, capacity=nsteps, sections=sections)
        e.step_rk4(t0, dt, nsteps, sync=False)
        info = [e.observed_section_info(s) for s in range(len(sections))]
        lines = [e.observed_section(s) for s in range(len(sections))]
        got = [e.download(k, dtype) for k in range(len(members))]
        assert e.observations()["t"].tolist() == [t0 + float(s + 1) * dt for s in range(nsteps)]
        e.end_observe()
    states = plain_run(members, ys, t0, dt, nsteps)
    for k in range(len(members)):
        assert np.array_equal(got[k], states[-1][k]), ("observation perturbed member", k)
    V = 2 if precision == "f64" else 4
    worst = {"theta_mean": [0.0], "phi_mean": [0.0]}
    for q, sec in enumerate(sections):
        length = NX if sec[0] in ("row", "phi_mean") else NY
        assert info[q]["kind"] == capi.SECTION_KINDS[sec[0]] and info[q]["index"] == (sec[1] if len(sec) > 1 else 0) and info[q]["length"] == length
        assert lines[q].shape == (nsteps, len(members), length, 2)
        # D as include/crd.h derives it
        D = {"row": 0, "column": 0, "theta_mean": -(-(-(-NX // V)) // 64) + int(math.log2(V)) + 6 + 3, "phi_mean": -(-NY // 4) + 2 + 3}[sec[0]]
        assert info[q]["additions"] == D, (sec, info[q], D)
        for s in range(nsteps):
            for k in range(len(members)):
                if sec[0] in ("row", "column"):
                    assert np.array_equal(lines[q][s, k], expected_exact(sec, states[s][k])), (sec, s, k)
                else:
                    check_means(sec[0], lines[q][s, k], states[s][k], D, worst[sec[0]])
    print("sections %s %s %dx%d: worst error / bound: theta-mean %.3e, phi-mean %.3e" % (model, precision, NX, NY, worst["theta_mean"][0], worst["phi_mean"][0]))


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_means_of_a_uniform_field_are_its_value(gpu_device, precision):
    """(0.3 rounded to fp32, 1.5): 24 significant bits, so every partial sum of up to 2^29 of them is exact in double, and so is the
    division of n c by n."""
    for nx, ny in ((61, 183), (64, 0), (130, 70)):
        p = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, precision=precision)
        g = crd.grid_of(p)
        y = np.empty((g.ny, g.nx, 2))
        y[..., 0], y[..., 1] = float(np.float32(0.3)), 1.5
        with crd.Slab(p) as s:
            s.upload(y)
            for kind, length in (("theta_mean", g.ny), ("phi_mean", g.nx)):
                line = s.section(kind)
                assert line.shape == (length, 2)
                assert np.all(line[:, 0] == float(np.float32(0.3))) and np.all(line[:, 1] == 1.5), (precision, nx, kind)


def observed(members, ys, t0, dt, calls, sections=(), cycles=False, cycle_threshold=0.0, stride=1, capacity=64):
    """An observed run: the section lines, the cycle planes of every member (or None) and the sample times."""
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.observe(stride=stride, capacity=capacity, sections=sections, cycles=cycles, cycle_threshold=cycle_threshold)
        done = 0
        for n in calls:
            e.step_rk4(t0 + done * dt, dt, n, sync=False)
            done += n
        lines = [e.observed_section(s) for s in range(len(sections))]
        cyc = [e.observed_cycles(k) for k in range(len(members))] if cycles else None
        states = [e.download(k, dtype_of(members[0])) for k in range(len(members))]
        return lines, cyc, e.observations()["t"], states


def test_a_nan_stays_with_its_row_column_and_member(gpu_device):
    """A NaN planted in member 2 (it spreads to the stencil's neighbours during the step): of member 2, exactly the theta-means of the
    rows and the phi-means of the columns that hold a NaN in the downloaded state are NaN, per field; every other value of every member
    is the clean run's, byte for byte."""
    base = crd.make_params("fhn", "torus", 61, 80.0, 20.0, 0.12, 1.25, ny=183, t_boundary=0.05)
    members = [params_like(base, beta=0.9 + 0.1 * k) for k in range(4)]
    ys = [start_state(p, 31 + k) for k, p in enumerate(members)]
    bad = ys[2].copy()
    bad[100, 17, 0] = np.nan
    sections = [("theta_mean",), ("phi_mean",), ("row", 100), ("column", 17)]
    clean, _, _, _ = observed(members, ys, 0.0, 0.02, [1], sections=sections)
    dirty, _, _, states = observed(members, ys[:2] + [bad] + ys[3:], 0.0, 0.02, [1], sections=sections)
    nan = np.isnan(states[2])
    assert nan[100, 17, 0] and 0 < nan.sum() < 200
    for q, axis in ((0, 1), (1, 0)):
        hit = nan.any(axis=axis)  # [rows or columns, field]
        assert hit.any() and not hit.all()
        assert np.array_equal(np.isnan(dirty[q][0, 2]), hit), sections[q]
        assert dirty[q][0, 2][~hit].tobytes() == clean[q][0, 2][~hit].tobytes(), sections[q]
    assert np.array_equal(np.isnan(dirty[2][0, 2]), nan[100]) and np.array_equal(np.isnan(dirty[3][0, 2]), nan[:, 17])
    for q in range(len(sections)):
        for k in (0, 1, 3):
            assert np.all(np.isfinite(dirty[q][:, k])) and dirty[q][:, k].tobytes() == clean[q][:, k].tobytes(), (q, k)


@pytest.mark.parametrize("model,precision,nx,ny", [("fhn", "f64", 61, 183), ("goldbeter", "f32", 130, 70), ("fhn", "f32", 64, 0)])
def test_lines_and_cycle_planes_do_not_depend_on_the_member_count_or_the_run(gpu_device, model, precision, nx, ny):
    base = members_of(model, precision, nx, ny)[0]
    members = [params_like(base, beta=base.beta * (0.8 + 0.1 * k), diffusion=0.1 + 0.02 * k) for k in range(5)]
    dtype = dtype_of(base)
    ys = [start_state(p, 11 + k).astype(dtype) for k, p in enumerate(members)]
    g = crd.grid_of(base)
    sections = all_sections(g.nx, g.ny)
    dt = 0.02 if model == "fhn" else 0.002
    thr = float(np.median(ys[0][..., 0]))
    a = observed(members, ys, 0.0, dt, [3, 2], sections=sections, cycles=True, cycle_threshold=thr)
    b = observed(members, ys, 0.0, dt, [3, 2], sections=sections, cycles=True, cycle_threshold=thr)
    for q in range(len(sections)):
        assert a[0][q].tobytes() == b[0][q].tobytes(), sections[q]
    for k in range(5):
        for x, y in zip(a[1][k], b[1][k]):
            assert x.tobytes() == y.tobytes()
    assert sum(int(a[1][k][0].sum()) for k in range(5)) > 0  # (some crossings: the planes are not trivially alike)
    for k in (0, 2, 4):
        one = observed([members[k]], [ys[k]], 0.0, dt, [3, 2], sections=sections, cycles=True, cycle_threshold=thr)
        for q in range(len(sections)):
            assert one[0][q][:, 0].tobytes() == a[0][q][:, k].tobytes(), (k, sections[q])
        for x, y in zip(one[1][0], a[1][k]):
            assert x.tobytes() == y.tobytes(), k
        # the single-slab counterpart: the ensemble-of-one line of the same state
        with crd.Slab(members[k]) as s:
            s.upload(one[3][0])
            for q, sec in enumerate(sections):
                assert s.section(*sec).tobytes() == one[0][q][-1, 0].tobytes(), (k, sec)
    with crd.LocalGroup(crd.make_params("fhn", "torus", 32, 80.0, 20.0, 0.12, 1.25), 2) as grp:
        with pytest.raises(crd.CrdError) as err:
            grp.slabs[1].section("theta_mean")
        assert err.value.status == EINVAL and "single-slab" in str(err.value)


def cycle_rule(xs, t, thr):
    """The rule of include/crd.h on the activator planes xs[sample] (float64) at times t: count, t_first, t_last."""
    count = np.zeros(xs[0].shape, dtype=np.int32)
    t_first, t_last = np.full(xs[0].shape, np.nan), np.full(xs[0].shape, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(1, len(xs)):
            d0, d1 = xs[s - 1] - thr, xs[s] - thr
            up = (d0 < 0.0) & (d1 >= 0.0)
            tc = t[s - 1] + (t[s] - t[s - 1]) * (-d0 / (d1 - d0))
            t_first = np.where(up & (count == 0), tc, t_first)
            t_last = np.where(up, tc, t_last)
            count += up
    return count, t_first, t_last


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_cycle_maps_equal_the_rule_on_the_downloaded_states(gpu_device, precision):
    """Goldbeter on 61 x 183, beta = 0.5 inside and 0.2, 0.9 outside the oscillatory window 0.28895 .. 0.77427, from (Z, Y) = (0.3, 1.5)
    plus noise of 1e-3 per point; dt = 0.005 (crd_stable_dt: 0.00681), 400 steps, a sample every 10: t = 2, more than two periods of
    0.6996.  Threshold 0.5 on Z.
    The CPU oracle's RK4 (oracle/crd_oracle.py, fp64, same start, dt and sampling) with the rule of include/crd.h counts: beta 0.5 -- 3
    upward crossings at every one of the 11163 points (Z runs between 0.28 and 1.12); beta 0.2 -- 0 at every point (Z stays below
    0.24); beta 0.9 -- 1 at every point (Z rises from 0.3 to its rest value 0.757 through 0.5 once).  So the reference alone has points
    with count >= 2 and points with count <= 1, as asserted of the device below."""
    nx, ny, dt, stride, nsamples, thr = 61, 183, 0.005, 10, 40, 0.5
    members = [crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, b, ny=ny, precision=precision, t_boundary=0.0) for b in (0.5, 0.2, 0.9)]
    assert dt < min(crd.stable_dt(p) for p in members)
    dtype = dtype_of(members[0])
    y0 = np.empty((ny, nx, 2))
    y0[..., 0], y0[..., 1] = 0.3, 1.5
    ys = [(y0 + 1e-3 * np.random.default_rng(7).standard_normal(y0.shape)).astype(dtype) for _ in members]
    _, cyc, t, final = observed(members, ys, 0.0, dt, [stride * nsamples], cycles=True, cycle_threshold=thr, stride=stride, capacity=nsamples)
    assert t.shape == (nsamples,)
    states = plain_run(members, ys, 0.0, dt, stride * nsamples, every=stride)
    some_two = some_few = False
    for k in range(len(members)):
        assert np.array_equal(final[k], states[-1][k])
        count, t_first, t_last = cycle_rule([states[s][k][..., 0].astype(np.float64) for s in range(nsamples)], t, thr)
        assert cyc[k][0].dtype == np.int32 and np.array_equal(cyc[k][0], count), k
        assert np.array_equal(cyc[k][1], t_first, equal_nan=True) and np.array_equal(cyc[k][2], t_last, equal_nan=True), k
        assert np.array_equal(np.isnan(cyc[k][1]), count == 0) and np.array_equal(np.isnan(cyc[k][2]), count == 0)
        assert np.array_equal(cyc[k][3], post.period_map(count, t_first, t_last), equal_nan=True)
        some_two = some_two or bool((count >= 2).any())
        some_few = some_few or bool((count <= 1).any())
        print("cycles %s beta %.1f: counts %s" % (precision, members[k].beta, dict(zip(*[a.tolist() for a in np.unique(count, return_counts=True)]))))
    assert some_two and some_few


def test_cycle_maps_of_the_goldbeter_scan(gpu_device):
    """The 8 x 16 uniform scan of test_goldbeter_beta_scan_oscillates_inside_the_window_only (beta = 0.2, 0.5, 0.9; dt = 0.005, a sample
    every 10 steps, 160 samples), cycles on.  The threshold is the mean of the middle member's probe series, taken from a first run with
    the probe alone: post.oscillation_summary places its crossings at that mean, so with it as cycle_threshold the summary of the probe
    series and the period map evaluate the same expressions on the same numbers, and the map equals the summary's period at every
    point (the field is uniform).  Against the CPU oracle (same dt, sampling and threshold): the same count, and a period within 1e-3,
    the margin of that test (a fiftieth of the sample interval)."""
    nx, ny, dt, stride, nsamples = 8, 16, 0.005, 10, 160
    betas = (0.2, 0.5, 0.9)
    members = [crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, b, ny=ny) for b in betas]
    y0 = np.empty((ny, nx, 2))
    y0[..., 0], y0[..., 1] = 0.3, 1.5

    def run(**kw):
        with crd.Ensemble(members) as e:
            for k in range(3):
                e.upload(k, y0)
            e.observe(stride=stride, probes=[(2, 3)], capacity=nsamples, **kw)
            e.step_rk4(0.0, dt, stride * nsamples, sync=False)
            obs = e.observations()
            return obs, ([e.observed_cycles(k) for k in range(3)] if kw else None)

    first, _ = run()
    thr = float(np.mean(first["probes"][:, 1, 0, 0]))
    obs, cyc = run(cycles=True, cycle_threshold=thr)
    assert obs["probes"].tobytes() == first["probes"].tobytes()
    t = obs["t"]
    mid = post.oscillation_summary(t, obs["probes"][:, 1, 0, 0])
    count, _, _, period = cyc[1]
    assert mid["crossings"] >= 10 and np.all(count == mid["crossings"]), (mid, np.unique(count))
    assert np.all(period == mid["period"]), (mid, np.unique(period))
    for k in (0, 2):
        assert not (cyc[k][0] >= 2).any(), (k, np.unique(cyc[k][0]))
    op = co.make_problem(co.GOLDBETER, co.TORUS, nx, 80.0, 20.0, 0.12, betas[1], ny=ny)
    y, series = y0.copy(), []
    for s in range(nsamples):
        y = co.rk4(op, y, s * stride * dt, dt, stride)
        series.append(y[3, 2, 0])
    ocount, ofirst, olast = cycle_rule([np.array([x]) for x in series], t, thr)
    operiod = post.period_map(ocount, ofirst, olast)[0]
    print("scan cycles: threshold %.6f, count %d (oracle %d), period %.6f (oracle %.6f)" % (thr, count[3, 2], ocount[0], period[3, 2], operiod))
    assert np.all(count == ocount[0])
    assert abs(period[3, 2] - operiod) <= 1e-3


def test_bookkeeping_with_sections(gpu_device):
    """Stride carry-over, the capacity refusal and the refusals of begin_with, read_section and cycles, with sections configured."""
    base = crd.make_params("fhn", "torus", 64, 80.0, 20.0, 0.12, 1.25, t_boundary=0.1)
    members = [base, params_like(base, beta=0.9)]
    ys = [start_state(p, 21 + k) for k, p in enumerate(members)]
    g = crd.grid_of(base)
    t0, dt = 0.5, 0.02
    sections = [("column", 5), ("theta_mean",), ("phi_mean",)]
    every, _, te, _ = observed(members, ys, t0, dt, [2, 5, 4], sections=sections)
    third, _, tt, _ = observed(members, ys, t0, dt, [2, 5, 4], sections=sections, stride=3)
    assert te.shape == (11,) and tt.shape == (3,)
    for q in range(len(sections)):
        assert third[q].shape[0] == 3
        for r, s in enumerate((3, 6, 9)):  # the samples after steps 3, 6 and 9: stride 1's times and bits
            assert tt[r] == te[s - 1] and third[q][r].tobytes() == every[q][s - 1].tobytes(), (q, r)
    L = capi.lib()
    opt = capi.ObserveOptions()
    opt.stride = 1
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        # refused before anything is opened: the observer stays closed
        for secs, cycles, thr in (([(capi.SECTION_ROW, g.ny)], 0, 0.0), ([(capi.SECTION_ROW, -1)], 0, 0.0), ([(capi.SECTION_COLUMN, g.nx)], 0, 0.0), ([(4, 0)], 0, 0.0),
                                  ([(capi.SECTION_PHI_MEAN, 0)] * 9, 0, 0.0), ([], 1, float("nan")), ([], 1, float("inf")), ([], 2, 0.0)):
            ex = capi.ObserveExtras()
            ex.n_sections, ex.cycles, ex.cycle_threshold = len(secs), cycles, thr
            for q, (kind, index) in enumerate(secs[:capi.OBSERVE_MAX_SECTIONS]):
                ex.kind[q], ex.index[q] = kind, index
            assert L.crd_ensemble_observe_begin_with(e.handle, opt, ex, 4) == EINVAL, (secs, cycles, thr)
            assert L.crd_ensemble_observe_end(e.handle) == EINVAL
        # the means ignore their index
        e.observe(capacity=1, sections=[("theta_mean", 10 ** 6), ("phi_mean", -5)])
        e.end_observe()
        e.observe(stride=2, capacity=2, sections=sections)
        e.step_rk4(t0, dt, 3)  # one sample (after step 2), count of steps 3
        before = [e.download(k) for k in range(2)]
        assert e.observed_count() == 1
        assert L.crd_ensemble_step_rk4(e.handle, t0 + 3 * dt, dt, 3) == EINVAL and "room" in e.last_error()  # two samples, room for one
        e.synchronize()
        assert e.observed_count() == 1
        for k in range(2):
            assert np.array_equal(e.download(k), before[k])
        e.step_rk4(t0 + 3 * dt, dt, 2)  # step 4 only: fits
        assert e.observed_count() == 2 and e.observed_section(0).shape == (2, 2, g.ny, 2)
        assert e.observed_section(1, first=1).shape == (1, 2, g.ny, 2)
        buf = np.empty((2, 2, g.nx, 2))
        assert L.crd_ensemble_observe_read_section(e.handle, 3, 0, 1, buf.ctypes.data) == EINVAL and "not configured" in e.last_error()
        assert L.crd_ensemble_observe_read_section(e.handle, -1, 0, 1, buf.ctypes.data) == EINVAL
        assert L.crd_ensemble_observe_read_section(e.handle, 2, 1, 2, buf.ctypes.data) == EINVAL
        assert L.crd_ensemble_observe_section_info(e.handle, 3, None, None, None, None) == EINVAL
        assert L.crd_ensemble_observe_cycles(e.handle, 0, None, None, None) == EINVAL and "cycle" in e.last_error()  # cycles are off
        e.end_observe()
        e.observe(capacity=1)  # no extras: no sections, no cycle maps
        assert L.crd_ensemble_observe_section_info(e.handle, 0, None, None, None, None) == EINVAL
        assert L.crd_ensemble_observe_cycles(e.handle, 0, None, None, None) == EINVAL


def test_an_adaptive_call_records_one_line_per_section(gpu_device):
    p = crd.make_params("fhn", "torus", 61, 80.0, 20.0, 0.12, 1.25, ny=183, t_boundary=0.3)
    members = [p, params_like(p, beta=0.9), params_like(p, diffusion=0.2)]
    ys = [start_state(q, 41 + k) for k, q in enumerate(members)]
    sections = [("column", 60), ("row", 91), ("theta_mean",), ("phi_mean",)]
    touts = [0.1, 0.25]
    worst = [0.0]
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.observe(stride=5, capacity=2, sections=sections, cycles=True, cycle_threshold=0.0)  # (the stride counts fixed steps only)
        D = [e.observed_section_info(q)["additions"] for q in range(4)]
        t0 = 0.0
        for r, tout in enumerate(touts):
            assert all(s["status"] == capi.OK for s in e.integrate_adaptive(t0, tout))
            assert e.observations()["t"].tolist() == touts[:r + 1]
            for k in range(3):
                y = e.download(k)
                for q, sec in enumerate(sections):
                    line = e.observed_section(q)
                    assert line.shape[0] == r + 1
                    if sec[0] in ("row", "column"):
                        assert np.array_equal(line[r, k], expected_exact(sec, y)), (r, k, sec)
                    else:
                        check_means(sec[0], line[r, k], y, D[q], worst)
            t0 = tout
        assert capi.lib().crd_ensemble_integrate_adaptive(e.handle, t0, t0 + 0.1, None, None, None) == EINVAL and "room" in e.last_error()
    # a member that fails alone has lines of NaNs, the others do not
    bad = ys[1].copy()
    bad[5, 7, 0] = np.nan
    with crd.Ensemble(members) as e:
        for k, y in enumerate([ys[0], bad, ys[2]]):
            e.upload(k, y)
        e.observe(capacity=1, sections=sections)
        st = e.integrate_adaptive(0.0, 0.1)
        assert [s["status"] for s in st] == [capi.OK, capi.ESTATE, capi.OK]
        for q in range(4):
            line = e.observed_section(q)
            assert line.shape[0] == 1 and np.all(np.isnan(line[0, 1])) and np.all(np.isfinite(line[0, 0])) and np.all(np.isfinite(line[0, 2])), q
    print("sections adaptive: worst mean error / bound = %.3e" % worst[0])


def test_driver_sections_and_cycles_leave_the_state_files_alone(gpu_device, tmp_path):
    ini = os.path.join(INI, "small_run.ini")
    common = [os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus", "--quiet", "--ensemble", "beta=1.0,1.25,1.4"]
    plain, seen = str(tmp_path / "plain"), str(tmp_path / "seen")
    subprocess.run(common + ["--outdir", plain, ini], check=True, capture_output=True, timeout=300)
    r = subprocess.run(common + ["--outdir", seen, "--observe", "2", "--section", "column:0", "--section", "theta-mean", "--observe-cycles", "0.0", ini], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for k in range(3):
        a, b = os.path.join(plain, "member_%d" % k), os.path.join(seen, "member_%d" % k)
        names = sorted(os.listdir(a))
        assert names and sorted(os.listdir(b)) == sorted(names + ["observables.txt", "section_0.npy", "section_1.npy", "activation_count.npy", "period_map.npy"])
        match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
        assert not mismatch and not errors, (mismatch, errors)
        head = open(os.path.join(b, "observables.txt")).read().splitlines()
        assert head[0].startswith("# t min0 max0 sum0 sumsq0 min1 max1 sum1 sumsq1")
        assert head[1].startswith("# section_0.npy: column 0") and head[2].startswith("# section_1.npy: theta-mean") and head[3].startswith("# sample times:")
        rows = np.loadtxt(os.path.join(b, "observables.txt"), ndmin=2)
        assert rows.shape[1] == 9 and rows.shape[0] >= 1
        assert [float(x) for x in head[3].split(":")[1].split()] == rows[:, 0].tolist()
        s0, s1 = np.load(os.path.join(b, "section_0.npy")), np.load(os.path.join(b, "section_1.npy"))
        assert s0.shape == s1.shape == (rows.shape[0], 40, 2) and s0.dtype == np.float64  # (a 16 x 40 grid: both run along phi)
        assert np.all(np.isfinite(s0)) and np.all(np.isfinite(s1))
        assert np.all(rows[:, 1, None] <= s0[:, :, 0]) and np.all(s0[:, :, 0] <= rows[:, 2, None])  # min0 <= var0 on the column <= max0
        assert np.allclose(s1[:, :, 0].mean(axis=1), rows[:, 3] / (16 * 40), rtol=1e-12, atol=1e-14)  # the mean of the rows' means: sum0 / n
        count, period = np.load(os.path.join(b, "activation_count.npy")), np.load(os.path.join(b, "period_map.npy"))
        assert count.shape == period.shape == (40, 16) and count.dtype == np.int32 and period.dtype == np.float64 and np.all(count >= 0)
        assert np.array_equal(np.isnan(period), count < 2)
