"""The run recorder on the GPU (crd_recorder_*, crd.Recorder, crd_run --observe without --ensemble): statistics, probes, sections, maps
and cycle maps of a Slab or a LocalGroup, sampled inside the stepping calls.

The reference of every per-sample check is the downloaded state: min, max, probes, rows, columns and the maps are compared with ==,
the cycle planes with == against the rule of include/crd.h evaluated by numpy, sums against math.fsum within D u sum|x| (D from
Recorder.info(): include/crd.h derives it; squares (D + 1) u sum x^2), the theta-mean within its section's bound.  A record is the same
bits for a lone Slab and for any LocalGroup cut of the grid, and the state steps exactly as without a recorder.

Shapes (nx x ny): nx = 5 leaves most lanes idle; 127 / 128 / 129 in fp64 and 255 / 256 / 257 in fp32 are one 16-byte group per lane, -1
and +1; 300 gives some lanes a second group; an odd nx takes alternate rows off 16 bytes; ny = 8, 9 and 257 are the finishing stride of
256 rows, +1."""
import filecmp
import math
import os
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
INI = os.path.join(GOLDEN, "ini")
U = 2.0 ** -53
capi = crd._capi
F64, F32 = capi.PRECISION_F64, capi.PRECISION_F32
DT = 0.02


def make(model, precision, nx, ny, t_boundary=10.0):
    if model == "fhn":
        return crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, beta_min=0.7, beta_max=1.7, precision=precision, t_boundary=t_boundary)
    return crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, 0.4, ny=ny, precision=precision, t_boundary=t_boundary)


def start_state(p, seed):
    y = crd.initial_conditions(crd.run_config(p, wave_length=0.1, wave_width=0.5, wave_inside=0))
    return y + 0.05 * np.random.default_rng(seed).standard_normal(y.shape)


def dt_of(p):
    """Half the stability bound of the grid at hand (crd_stable_dt): nothing blows up, whatever the shape."""
    return 0.5 * capi.lib().crd_stable_dt(capi.C.byref(p))


def dtype_of(p):
    return np.float64 if p.precision == F64 else np.float32


def target(p, slabs):
    return crd.Slab(p) if slabs == 1 else crd.LocalGroup(p, slabs)


def step(tgt, t0, dt, n):
    tgt.step_rk4(t0, dt, n)


def sections_of(nx, ny):
    return [("row", 0), ("row", ny - 1), ("column", nx // 2), ("theta_mean",), ("row", ny // 2)]


def probes_of(nx, ny, cuts=(2, 3, 5)):
    """Both sides of every slab boundary of the cuts the tests use, and the grid's corners."""
    pts = {(0, 0), (nx - 1, ny - 1), (nx // 3, ny // 2)}
    for n in cuts:
        for k in range(1, n):
            j = (ny * k) // n
            pts.add((k % nx, j - 1))
            pts.add(((k + 1) % nx, j))
    return sorted(pts)[:capi.OBSERVE_MAX_PROBES]


def full_record(rec):
    t, stats, probes = rec.read()
    out = {"t": t, "stats": stats, "probes": probes}
    info = rec.info()
    for s in range(info["n_sections"]):
        out["section%d" % s] = rec.section(s)
    if info["maps"]:
        out["min"], out["max"], out["t_act"] = rec.maps()
    if info["cycles"]:
        out["count"], out["t_first"], out["t_last"] = rec.cycles()
    return out


def records_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def cycles_by_rule(us, ts, thr):
    """include/crd.h's rule on the samples' var0 planes (float64), every operation rounded once."""
    count = np.zeros(us[0].shape, dtype=np.int32)
    t_first, t_last = np.full(us[0].shape, np.nan), np.full(us[0].shape, np.nan)
    with np.errstate(all="ignore"):
        for k in range(1, len(us)):
            d0, d1 = us[k - 1] - thr, us[k] - thr
            cross = (d0 < 0.0) & (d1 >= 0.0)
            tc = ts[k - 1] + (ts[k] - ts[k - 1]) * (-d0 / (d1 - d0))
            t_first = np.where(cross & (count == 0), tc, t_first)
            t_last = np.where(cross, tc, t_last)
            count = count + cross.astype(np.int32)
    return count, t_first, t_last


def maps_by_rule(us, ts, thr):
    mn, mx, ta = np.full(us[0].shape, np.inf), np.full(us[0].shape, -np.inf), np.full(us[0].shape, np.nan)
    for u, t in zip(us, ts):
        mn, mx = np.minimum(mn, u), np.maximum(mx, u)
        ta = np.where(np.isnan(ta) & (u >= thr), t, ta)
    return mn, mx, ta


def run_recorded(p, y0, slabs, stride, nsamples, dt, t0=0.0, download=True, **kw):
    """Step stride by stride with a recorder open; returns (record, info, section infos, states downloaded at every sample)."""
    states = []
    with target(p, slabs) as tgt:
        tgt.upload(y0)
        with crd.Recorder(tgt, stride=stride, capacity=nsamples, **kw) as rec:
            for s in range(nsamples):
                step(tgt, t0 + (s * stride) * dt, dt, stride)
                if download:
                    states.append(tgt.download(dtype_of(p)))
            assert rec.count() == nsamples
            info = rec.info()
            return full_record(rec), info, [rec.section_info(s) for s in range(info["n_sections"])], states


# ---- recording changes nothing ----------------------------------------------------------------------------------------------------------

CALLS = (7, 4, 3)  # cut inside triples and pairs


@pytest.mark.parametrize("plan", ["three_steps", "default"])
@pytest.mark.parametrize("stride", [1, 2, 5])
@pytest.mark.parametrize("shape", [("fhn", F64, 61, 183), ("fhn", F64, 130, 70), ("fhn", F32, 129, 70)], ids=lambda s: "%s_f%d_%dx%d" % (s[0], 64 if s[1] == F64 else 32, s[2], s[3]))
def test_recording_leaves_the_state_alone(shape, stride, plan):
    model, precision, nx, ny = shape
    p = make(model, precision, nx, ny, t_boundary=0.11)  # the absorbing rows go off between the samples at 0.1 and 0.2
    y0 = start_state(p, 3)
    results, expected_t = [], []
    for recorded in (False, True):
        with crd.Slab(p) as slab:
            if plan == "three_steps":
                slab.set_launch_plan(1, 1, 1, 1, 3)
            slab.upload(y0)
            rec = crd.Recorder(slab, stride=stride, probes=[(1, 2)], maps=True, cycles=True, sections=[("theta_mean",)], capacity=sum(CALLS)) if recorded else None
            done = 0
            for n in CALLS:
                t0 = done * DT
                slab.step_rk4(t0, DT, n)
                if recorded:
                    expected_t += [t0 + (s + 1) * DT for s in range(n) if (done + s + 1) % stride == 0]
                done += n
            if recorded:
                assert rec.count() == sum(CALLS) // stride
                t, stats, _ = rec.read()
                assert np.array_equal(t, np.array(expected_t))
                last = slab.download(dtype_of(p))
                if sum(CALLS) % stride == 0:
                    assert stats[-1, 0, 0] == last[..., 0].min() and stats[-1, 1, 1] == last[..., 1].max()
                rec.close()
            results.append(slab.download(dtype_of(p)))
    assert np.array_equal(results[0], results[1])


def test_recording_leaves_a_group_alone():
    p = make("fhn", F64, 163, 47, t_boundary=0.11)  # 16 + 16 + 15 rows
    y0 = start_state(p, 4)
    results = []
    for recorded in (False, True):
        with crd.LocalGroup(p, 3) as g:
            g.set_exchange_period(3)
            g.upload(y0)
            rec = crd.Recorder(g, stride=2, probes=[(5, 15), (6, 16)], maps=True, sections=[("column", 7)], capacity=16) if recorded else None
            done = 0
            for n in CALLS + (5,):
                g.step_rk4(done * DT, DT, n)
                done += n
            if recorded:
                assert rec.count() == done // 2
                rec.close()
            results.append(g.download())
    assert np.array_equal(results[0], results[1])


# ---- exactness and bounds ---------------------------------------------------------------------------------------------------------------

EDGE_SHAPES = [("fhn", F64, 5, 8), ("fhn", F64, 127, 9), ("goldbeter", F64, 128, 8), ("fhn", F64, 129, 257), ("goldbeter", F64, 300, 9),
               ("fhn", F32, 255, 9), ("goldbeter", F32, 256, 8), ("fhn", F32, 257, 9), ("fhn", F32, 300, 257), ("goldbeter", F32, 5, 9)]


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "%s_f%d_%dx%d" % (s[0], 64 if s[1] == F64 else 32, s[2], s[3]))
def test_record_against_the_downloaded_states(shape):
    model, precision, nx, ny = shape
    p = make(model, precision, nx, ny)
    y0 = start_state(p, 5)
    stride, nsamples = 2, 4
    thr = float(np.median(y0[..., 0]))
    secs, probes = sections_of(nx, ny), probes_of(nx, ny)
    dt = dt_of(p)
    r, info, sinfo, states = run_recorded(p, y0, 1, stride, nsamples, dt, probes=probes, maps=True, threshold=thr, sections=secs, cycles=True, cycle_threshold=thr)
    D = info["additions"]
    V = 2 if precision == F64 else 4
    assert D == -(-(-(-nx // V)) // 64) + (1 if V == 2 else 2) + 6 + -(-ny // 256) + 8
    ts = [(s * stride) * dt + stride * dt for s in range(nsamples)]
    assert np.array_equal(r["t"], np.array(ts))
    worst = {"sum": 0.0, "sumsq": 0.0, "theta_mean": 0.0}
    for k, y in enumerate(states):
        y = y.astype(np.float64)
        for f in range(2):
            x = y[..., f].ravel()
            assert r["stats"][k, f, 0] == x.min() and r["stats"][k, f, 1] == x.max()
            bound = D * U * math.fsum(np.abs(x))
            err = abs(r["stats"][k, f, 2] - math.fsum(x))
            worst["sum"] = max(worst["sum"], err / bound)
            assert err <= bound, (k, f, err, bound)
            sq = x * x
            bound = (D + 1) * U * math.fsum(sq)
            err = abs(r["stats"][k, f, 3] - math.fsum(sq))
            worst["sumsq"] = max(worst["sumsq"], err / bound)
            assert err <= bound, (k, f, err, bound)
        for q, (i, j) in enumerate(probes):
            assert np.array_equal(r["probes"][k, q], y[j, i])
        for s, sec in enumerate(secs):
            line = r["section%d" % s][k]
            if sec[0] == "row":
                assert np.array_equal(line, y[sec[1]])
            elif sec[0] == "column":
                assert np.array_equal(line, y[:, sec[1]])
            else:
                Ds = sinfo[s]["additions"]
                for j in range(ny):
                    for f in range(2):
                        bound = Ds * U * math.fsum(np.abs(y[j, :, f])) / nx
                        err = abs(line[j, f] - math.fsum(y[j, :, f]) / nx)
                        worst["theta_mean"] = max(worst["theta_mean"], err / bound)
                        assert err <= bound, (k, j, f, err, bound)
    print("recorder %s: worst error / bound %s (D = %d)" % (shape, {k: "%.3f" % v for k, v in worst.items()}, D))
    us = [y[..., 0].astype(np.float64) for y in states]
    for got, want in zip((r["min"], r["max"], r["t_act"]), maps_by_rule(us, ts, thr)):
        assert np.array_equal(got, want, equal_nan=True)
    for got, want in zip((r["count"], r["t_first"], r["t_last"]), cycles_by_rule(us, ts, thr)):
        assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("shape", [("fhn", F64, 61, 183), ("fhn", F32, 130, 70), ("goldbeter", F64, 129, 9)], ids=lambda s: "%s_f%d_%dx%d" % (s[0], 64 if s[1] == F64 else 32, s[2], s[3]))
def test_lone_lines_are_the_bits_of_slab_section(shape):
    model, precision, nx, ny = shape
    p = make(model, precision, nx, ny)
    with crd.Slab(p) as slab:
        slab.upload(start_state(p, 6))
        with crd.Recorder(slab, stride=3, sections=[("theta_mean",), ("phi_mean",)], capacity=2) as rec:
            for s in range(2):
                slab.step_rk4(3 * s * dt_of(p), dt_of(p), 3)
                assert np.array_equal(rec.section(0)[s], slab.section("theta_mean"))
                assert np.array_equal(rec.section(1)[s], slab.section("phi_mean"))


# ---- cut invariance ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("grid", [(163, 47), (61, 183)], ids=lambda g: "%dx%d" % g)
def test_a_record_does_not_depend_on_the_cut(grid, precision):
    nx, ny = grid
    p = make("fhn", precision, nx, ny, t_boundary=0.05)
    y0 = start_state(p, 7)
    thr = float(np.median(y0[..., 0]))
    kw = dict(probes=probes_of(nx, ny), maps=True, threshold=thr, sections=sections_of(nx, ny), cycles=True, cycle_threshold=thr)
    lone, info, _, states = run_recorded(p, y0, 1, 2, 4, DT, **kw)
    assert info["slabs"] == 1
    again, _, _, _ = run_recorded(p, y0, 1, 2, 4, DT, download=False, **kw)
    records_equal(lone, again)
    for slabs in (2, 3, 5):
        cut, info, _, cut_states = run_recorded(p, y0, slabs, 2, 4, DT, **kw)
        assert info["slabs"] == slabs
        assert np.array_equal(cut_states[-1], states[-1])
        records_equal(lone, cut)


# ---- error-controlled calls -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slabs", [1, 3])
def test_error_controlled_calls_record_one_sample_at_tout(slabs):
    nx, ny = 64, 192
    p = make("fhn", F64, nx, ny)
    y0 = start_state(p, 8)
    touts = [0.05, 0.1, 0.17]
    secs, probes = [("row", 100), ("column", 3), ("theta_mean",)], [(1, 63), (2, 64), (5, 191)]
    with target(p, slabs) as tgt:
        tgt.upload(y0)
        with crd.Recorder(tgt, stride=7, probes=probes, sections=secs, capacity=len(touts)) as rec:
            t0, states = 0.0, []
            for tout in touts:
                tgt.integrate_adaptive(t0, tout)
                states.append(tgt.download())
                t0 = tout
            assert rec.count() == len(touts)
            with pytest.raises(crd.CrdError) as e:  # no room left: refused before any work
                tgt.integrate_adaptive(t0, t0 + 0.01)
            assert e.value.status == capi.EINVAL and np.array_equal(tgt.download(), states[-1]) and rec.count() == len(touts)
            r, D = full_record(rec), rec.info()["additions"]
    assert np.array_equal(r["t"], np.array(touts))
    for k, y in enumerate(states):
        for f in range(2):
            x = y[..., f].ravel()
            assert r["stats"][k, f, 0] == x.min() and r["stats"][k, f, 1] == x.max()
            assert abs(r["stats"][k, f, 2] - math.fsum(x)) <= D * U * math.fsum(np.abs(x))
        for q, (i, j) in enumerate(probes):
            assert np.array_equal(r["probes"][k, q], y[j, i])
        assert np.array_equal(r["section0"][k], y[100]) and np.array_equal(r["section1"][k], y[:, 3])


# ---- bookkeeping ------------------------------------------------------------------------------------------------------------------------

def test_count_carries_over_calls_and_an_overrun_is_refused_whole():
    p = make("fhn", F64, 64, 64)
    with crd.Slab(p) as slab:
        slab.upload(start_state(p, 9))
        with crd.Recorder(slab, stride=3, capacity=3) as rec:
            slab.step_rk4(0.0, DT, 2)
            assert rec.count() == 0
            slab.step_rk4(2 * DT, DT, 2)  # steps 3 and 4: one sample, behind step 3
            assert rec.count() == 1 and rec.read()[0][0] == 2 * DT + 1 * DT
            slab.step_rk4(4 * DT, DT, 5)  # steps 5 .. 9: samples behind 6 and 9
            assert rec.count() == 3
            before = slab.download()
            with pytest.raises(crd.CrdError) as e:
                slab.step_rk4(9 * DT, DT, 3)  # would record a fourth
            assert e.value.status == capi.EINVAL and "room" in str(e.value)
            assert rec.count() == 3 and np.array_equal(slab.download(), before)
            slab.step_rk4(9 * DT, DT, 2)  # ... two steps fit
            assert rec.count() == 3 and not np.array_equal(slab.download(), before)


def test_phi_mean_second_recorder_and_partial_group():
    p = make("fhn", F64, 64, 64)
    with crd.Slab(p) as slab:
        slab.upload(start_state(p, 10))
        with crd.Recorder(slab, sections=[("phi_mean",)], capacity=1) as rec:
            with pytest.raises(crd.CrdError) as e:
                crd.Recorder(slab)
            assert e.value.status == capi.EINVAL and "already open" in str(e.value)
            slab.step_rk4(0.0, DT, 1)
            assert np.array_equal(rec.section(0)[0], slab.section("phi_mean"))
        crd.Recorder(slab).close()  # closed: another may be opened
    with crd.LocalGroup(p, 2) as g:
        g.upload(start_state(p, 10))
        with pytest.raises(crd.CrdError) as e:
            crd.Recorder(g, sections=[("phi_mean",)])
        assert e.value.status == capi.EINVAL and "phi-mean" in str(e.value)
        with pytest.raises(crd.CrdError) as e:
            crd.Recorder(g.slabs[0])
        assert e.value.status == capi.EINVAL and "whole LOCAL group" in str(e.value)
        with crd.Recorder(g, capacity=4) as rec:
            one = (capi.C.c_void_p * 1)(g.slabs[0].handle)
            assert capi.lib().crd_group_step_rk4(one, 1, 0.0, DT, 1) == capi.ESTATE
            assert capi.lib().crd_step_rk4(g.slabs[1].handle, 0.0, DT, 1) == capi.ESTATE
            assert rec.count() == 0
            g.step_rk4(0.0, DT, 2)
            assert rec.count() == 2
    with crd.LocalGroup(p, 2, blocks=(2, 1)) as g:
        with pytest.raises(crd.CrdError) as e:
            crd.Recorder(g)
        assert e.value.status == capi.EINVAL and "block contexts" in str(e.value)


@pytest.mark.parametrize("slabs", [1, 2])
def test_a_nan_stays_in_its_row_and_field(slabs):
    """Goldbeter with justDiffusion: var1 neither moves nor enters var0, so a NaN planted in var1 is still alone after a step."""
    nx, ny, row = 70, 40, 21
    p = crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, 0.4, ny=ny, just_diffusion=1, t_boundary=10.0)
    y = start_state(p, 11)
    y[row, 17, 1] = np.nan
    with target(p, slabs) as tgt:
        tgt.upload(y)
        with crd.Recorder(tgt, sections=[("theta_mean",)], maps=True, capacity=1) as rec:
            tgt.step_rk4(0.0, dt_of(p), 1)
            after = tgt.download()
            _, stats, _ = rec.read()
            line = rec.section(0)[0]
            mn, mx, _ = rec.maps()
    where = np.argwhere(np.isnan(after))
    assert where.tolist() == [[row, 17, 1]]  # (the premise: the NaN is where it was planted and nowhere else)
    assert np.all(np.isnan(stats[0, 1])) and np.all(np.isfinite(stats[0, 0]))
    assert np.isnan(line[row, 1]) and np.isfinite(line[row, 0])
    others = np.arange(ny) != row
    assert np.all(np.isfinite(line[others]))
    assert np.array_equal(mn, after[..., 0]) and np.array_equal(mx, after[..., 0])


# ---- driver -----------------------------------------------------------------------------------------------------------------------------

RECORDED = ["observables.txt", "section_0.npy", "section_1.npy", "amplitude_map.npy", "activation_time.npy", "activation_count.npy", "period_map.npy"]


def test_driver_records_a_lone_run_and_its_slabs_alike(gpu_device, tmp_path):
    ini = os.path.join(INI, "small_run.ini")  # a 16 x 40 grid, dt = 0.02, three outputs 0.4 apart: 60 steps
    observe = ["--observe", "2", "--probe", "3,2", "--section", "column:3", "--section", "theta-mean", "--observe-maps", "0.5", "--observe-cycles", "0.5"]
    dirs = {}
    for name, layout in (("lone", []), ("slabs", ["--gpus", "2", "--devices", "1"])):
        common = [os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus", "--quiet"] + layout
        plain, seen = str(tmp_path / (name + "_plain")), str(tmp_path / (name + "_seen"))
        os.makedirs(plain), os.makedirs(seen)  # (a run without --ensemble writes into a directory that exists)
        subprocess.run(common + ["--outdir", plain, ini], check=True, capture_output=True, timeout=300)
        r = subprocess.run(common + ["--outdir", seen] + observe + [ini], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        names = sorted(os.listdir(plain))
        assert names and sorted(os.listdir(seen)) == sorted(names + RECORDED)
        match, mismatch, errors = filecmp.cmpfiles(plain, seen, names, shallow=False)  # the state files: as without --observe
        assert not mismatch and not errors, (mismatch, errors)
        dirs[name] = seen
    match, mismatch, errors = filecmp.cmpfiles(dirs["lone"], dirs["slabs"], RECORDED, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)
    b = dirs["lone"]
    head = open(os.path.join(b, "observables.txt")).read().splitlines()
    assert head[0] == "# t min0 max0 sum0 sumsq0 min1 max1 sum1 sumsq1 var0(3,2) var1(3,2)"
    assert head[1].startswith("# section_0.npy: column 3") and head[2].startswith("# section_1.npy: theta-mean") and head[3].startswith("# sample times:")
    rows = np.loadtxt(os.path.join(b, "observables.txt"), ndmin=2)
    assert rows.shape == (30, 11)
    # the sample times of single steps: t0 + (s + 1) dt of each output interval's call, as the driver forms them
    d_out, want = 1.2 / 3, []
    dt = d_out / 20.0
    for iout in range(3):
        want += [iout * d_out + (s + 1) * dt for s in range(20) if (iout * 20 + s + 1) % 2 == 0]
    assert rows[:, 0].tolist() == want
    s0, s1 = np.load(os.path.join(b, "section_0.npy")), np.load(os.path.join(b, "section_1.npy"))
    assert s0.shape == s1.shape == (30, 40, 2) and s0.dtype == np.float64
    assert np.array_equal(s0[:, 2, :], rows[:, 9:11])  # the probe (3, 2) lies on column 3
    for name, dtype in (("amplitude_map.npy", np.float64), ("activation_time.npy", np.float64), ("activation_count.npy", np.int32), ("period_map.npy", np.float64)):
        a = np.load(os.path.join(b, name))
        assert a.shape == (40, 16) and a.dtype == dtype, name
    assert np.all(np.load(os.path.join(b, "amplitude_map.npy")) >= 0.0)
    count, period = np.load(os.path.join(b, "activation_count.npy")), np.load(os.path.join(b, "period_map.npy"))
    assert np.array_equal(np.isnan(period), count < 2)


def test_driver_records_one_sample_per_output_when_error_controlled(gpu_device, tmp_path):
    ini = os.path.join(INI, "small_run.ini")
    out = str(tmp_path / "adaptive")
    os.makedirs(out)
    r = subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus", "--quiet", "--adaptive", "--gpus", "2", "--devices", "1", "--outdir", out,
                        "--observe", "5", "--probe", "0,39", ini], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = np.loadtxt(os.path.join(out, "observables.txt"), ndmin=2)
    assert rows.shape == (3, 11) and rows[:, 0].tolist() == [1 * (1.2 / 3), 2 * (1.2 / 3), 1.2]
