"""Observers on the GPU (crd_ensemble_observe_*, Ensemble.observe, Slab.observe, crd_run --observe): observation does not perturb the
run; min / max / probes / maps equal numpy's on the downloaded states; sums within the bound the partition of the reduction gives;
rows independent of the other members, of the member count and of the run; NaN stays with its member; the error-controlled path; the
Goldbeter scan the feature is for, against the CPU oracle.

The reference of every per-sample check is a second, identical run without an observer that downloads every member's state after every
step (stride 1)."""
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
EINVAL = crd._capi.EINVAL


def params_like(p, **kw):
    q = copy.copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def start_state(p, seed):
    """The reference's initial state of p, perturbed per member so that no two members start alike."""
    y = crd.initial_conditions(crd.run_config(p, wave_length=0.1, wave_width=0.5, wave_inside=0))
    return y + 0.05 * np.random.default_rng(seed).standard_normal(y.shape)


def dtype_of(p):
    return np.float64 if p.precision == crd._capi.PRECISION_F64 else np.float32


def exact_sums(x):
    """fsum(x), fsum(|x|) and the sum of squares of a float64 vector, each correctly rounded: the squares are split into the rounded
    product and its residual (exact in the 64-bit significand of long double for float32 data widened; to 2^-64 relative for float64)."""
    hi = x * x
    lo = (x.astype(np.longdouble) * x.astype(np.longdouble) - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(x), math.fsum(np.abs(x)), math.fsum(np.concatenate([hi, lo]))


def check_row(row, state, G, worst):
    """One member's statistics row [2, 4] against its downloaded state [ny, nx, 2]: min / max ==, the sums within the derived bound
    |sum - exact| <= D u sum|x|, |sumsq - exact| <= (D + 1) u sum x^2, D = ceil(n / (256 G)) + 8 + G.  worst: running max of error / bound."""
    n = state.shape[0] * state.shape[1]
    D = -(-n // (256 * G)) + 8 + G
    for f in range(2):
        x = np.ascontiguousarray(state[..., f], dtype=np.float64).ravel()
        assert row[f, 0] == x.min() and row[f, 1] == x.max(), (f, row[f], x.min(), x.max())
        s, sa, sq = exact_sums(x)
        e1, b1 = abs(row[f, 2] - s), D * U * sa
        e2, b2 = abs(row[f, 3] - sq), (D + 1) * U * sq
        worst[0] = max(worst[0], e1 / b1, e2 / b2)
        assert e1 <= b1, ("sum", f, e1, b1)
        assert e2 <= b2, ("sumsq", f, e2, b2)


def plain_run(members, ys, t0, dt, nsteps):
    """No observer: one step per call, every member downloaded after every step.  states[s][k]."""
    dtype = dtype_of(members[0])
    states = []
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        for s in range(nsteps):
            e.step_rk4(t0 + s * dt, dt, 1)
            states.append([e.download(k, dtype) for k in range(len(members))])
    return states


def members_of(model, precision, nx, ny):
    if model == "fhn":
        base = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, beta_min=0.7, beta_max=1.7, precision=precision, t_boundary=10.0)
        return [base, params_like(base, beta=0.9, diffusion=0.2), params_like(base, vary_beta=1, t_boundary=0.05)]
    base = crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, 0.4, ny=ny, precision=precision, t_boundary=10.0)
    return [base, params_like(base, beta=0.6), params_like(base, diffusion=0.3, t_boundary=0.005)]


# (61 x 183: an odd point count -- the second plane of a state does not start on 16 bytes, every load is element-wise and the last
# group is short; 64 columns: the 16-byte loads)
@pytest.mark.parametrize("model,precision,nx,ny", [("fhn", "f64", 61, 183), ("fhn", "f32", 64, 0), ("goldbeter", "f64", 64, 0), ("goldbeter", "f32", 61, 183)])
def test_observed_run_is_unperturbed_and_matches_numpy(gpu_device, model, precision, nx, ny):
    members = members_of(model, precision, nx, ny)
    dtype = dtype_of(members[0])
    dt, nsteps, t0 = (0.02, 7, 0.0) if model == "fhn" else (0.002, 7, 0.0)
    ys = [start_state(p, 3 + k).astype(dtype) for k, p in enumerate(members)]
    g = crd.grid_of(members[0])
    NX, NY = g.nx, g.ny
    probes = [(0, 0), (NX - 1, 0), (0, NY - 1), (NX - 1, NY - 1), (NX // 2, NY // 3), (5, 7)]  # rows 0 and ny - 1, the theta seam
    u0 = ys[0][..., 0].astype(np.float64)
    threshold = 0.5 * (float(u0.min()) + float(u0.max()))
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        info = e.observe(stride=1, probes=probes, maps=True, threshold=threshold, capacity=nsteps)
        e.step_rk4(t0, dt, nsteps, sync=False)
        obs = e.observations()
        maps = [e.observed_maps(k) for k in range(len(members))]
        got = [e.download(k, dtype) for k in range(len(members))]
        e.end_observe()
    G = info["blocks_per_member"]
    assert 1 <= G <= 256 and info["values_per_field"] == NX * NY
    states = plain_run(members, ys, t0, dt, nsteps)
    for k in range(len(members)):
        assert np.array_equal(got[k], states[-1][k]), ("observation perturbed member", k)
    assert obs["t"].tolist() == [t0 + float(s + 1) * dt for s in range(nsteps)]
    worst = [0.0]
    crossed = never = 0
    for k in range(len(members)):
        lo = np.full((NY, NX), np.inf)
        hi = np.full((NY, NX), -np.inf)
        ta = np.full((NY, NX), np.nan)
        for s in range(nsteps):
            st = states[s][k]
            check_row(obs["stats"][s, k], st, G, worst)
            for q, (i, j) in enumerate(probes):
                assert obs["probes"][s, k, q, 0] == st[j, i, 0] and obs["probes"][s, k, q, 1] == st[j, i, 1], (s, k, q)
            uu = st[..., 0].astype(np.float64)
            lo, hi = np.minimum(lo, uu), np.maximum(hi, uu)
            ta = np.where(np.isnan(ta) & (uu >= threshold), obs["t"][s], ta)
            n = NX * NY
            assert obs["mean"][s, k, 0] == obs["stats"][s, k, 0, 2] / n and obs["variance"][s, k, 1] >= 0.0
        assert np.array_equal(maps[k][0], lo) and np.array_equal(maps[k][1], hi), ("min / max map", k)
        assert np.array_equal(maps[k][2], ta, equal_nan=True), ("activation time", k)
        crossed += int(np.count_nonzero(~np.isnan(ta)))
        never += int(np.count_nonzero(np.isnan(ta)))
    assert crossed > 0 and never > 0, (crossed, never)
    print("observe %s %s %dx%d: G = %d, worst sum error / bound = %.3e" % (model, precision, NX, NY, G, worst[0]))


def observe_rows(members, ys, t0, dt, calls, stride=1, probes=(), capacity=64):
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        info = e.observe(stride=stride, probes=probes, capacity=capacity)
        done = 0
        for n in calls:
            e.step_rk4(t0 + done * dt, dt, n, sync=False)
            done += n
        return info, e.observations()


def test_rows_do_not_depend_on_the_other_members_or_the_run(gpu_device):
    """Member k's rows in an ensemble of 8 are bit-equal to its rows as an ensemble of 1 (G depends on the grid alone), and two identical
    runs give bit-equal records."""
    base = crd.make_params("fhn", "torus", 61, 80.0, 20.0, 0.12, 1.25, ny=183, t_boundary=0.05)
    members = [params_like(base, beta=0.8 + 0.1 * k, diffusion=0.1 + 0.02 * k) for k in range(8)]
    ys = [start_state(p, 11 + k) for k, p in enumerate(members)]
    probes = [(0, 0), (60, 182), (30, 91)]
    info8, a = observe_rows(members, ys, 0.0, 0.02, [3, 2], probes=probes)
    _, b = observe_rows(members, ys, 0.0, 0.02, [3, 2], probes=probes)
    for key in ("t", "stats", "probes"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["stats"].shape == (5, 8, 2, 4) and np.all(np.isfinite(a["stats"]))
    for k in (0, 3, 7):
        info1, one = observe_rows([members[k]], [ys[k]], 0.0, 0.02, [3, 2], probes=probes)
        assert info1["blocks_per_member"] == info8["blocks_per_member"] <= 256
        assert one["stats"][:, 0].tobytes() == a["stats"][:, k].tobytes(), k
        assert one["probes"][:, 0].tobytes() == a["probes"][:, k].tobytes(), k


def test_blocks_per_member_follow_the_grid_only(gpu_device):
    for nx, ny in ((32, 0), (61, 183), (400, 1600)):
        p = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny)
        seen = set()
        for B in (1, 5):
            with crd.Ensemble([p] * B) as e:
                seen.add(e.observe(capacity=1)["blocks_per_member"])
        assert len(seen) == 1 and 1 <= min(seen) <= 256, (nx, ny, seen)


def test_stride_carries_over_calls_and_capacity_is_enforced(gpu_device):
    base = crd.make_params("fhn", "torus", 64, 80.0, 20.0, 0.12, 1.25, t_boundary=0.1)
    members = [base, params_like(base, beta=0.9)]
    ys = [start_state(p, 21 + k) for k, p in enumerate(members)]
    t0, dt = 0.5, 0.02
    probes = [(1, 2)]
    # (the same calls: a sample's time is its call's t0 + (s + 1) dt, and t0 + 7 dt + 2 dt need not round like t0 + 9 dt)
    _, every = observe_rows(members, ys, t0, dt, [2, 5, 4], stride=1, probes=probes)
    assert every["t"].shape == (11,)
    _, third = observe_rows(members, ys, t0, dt, [2, 5, 4], stride=3, probes=probes)
    assert third["t"].shape == (3,)
    for q, s in enumerate((3, 6, 9)):  # the samples after steps 3, 6 and 9: stride 1's times and bits
        assert third["t"][q] == every["t"][s - 1]
        assert third["stats"][q].tobytes() == every["stats"][s - 1].tobytes()
        assert third["probes"][q].tobytes() == every["probes"][s - 1].tobytes()
    # a call that would overrun the capacity: refused whole, state and sample count untouched
    L = crd._capi.lib()
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.observe(stride=2, capacity=2)
        e.step_rk4(t0, dt, 3)  # one sample (after step 2), count of steps 3
        before = [e.download(k) for k in range(2)]
        assert e.observed_count() == 1
        assert L.crd_ensemble_step_rk4(e.handle, t0 + 3 * dt, dt, 3) == EINVAL  # steps 4 and 6: two samples, room for one
        assert "room" in e.last_error()
        e.synchronize()
        assert e.observed_count() == 1
        for k in range(2):
            assert np.array_equal(e.download(k), before[k])
        e.step_rk4(t0 + 3 * dt, dt, 2)  # step 4 only: fits
        assert e.observed_count() == 2
        assert e.observations()["t"].tolist() == [t0 + 2.0 * dt, (t0 + 3 * dt) + 1.0 * dt]
        # reads outside the recorded range, and the refusals of begin
        assert L.crd_ensemble_observe_read(e.handle, 1, 2, None, None, None) == EINVAL
        opt = crd._capi.ObserveOptions()
        opt.stride = 1
        assert L.crd_ensemble_observe_begin(e.handle, opt, 4) == EINVAL and "already open" in e.last_error()
        e.end_observe()
        assert L.crd_ensemble_observe_end(e.handle) == EINVAL
        for stride, cap, n_probes, pi, pj in ((0, 4, 0, 0, 0), (1, 0, 0, 0, 0), (1, 4, 17, 0, 0), (1, 4, 1, 64, 0), (1, 4, 1, 0, -1)):
            opt = crd._capi.ObserveOptions()
            opt.stride, opt.n_probes, opt.probe_i[0], opt.probe_j[0] = stride, n_probes, pi, pj
            assert L.crd_ensemble_observe_begin(e.handle, opt, cap) == EINVAL, (stride, cap, n_probes, pi, pj)
        # with no observer open, stepping goes on as before
        e.step_rk4(t0 + 5 * dt, dt, 1)


def test_a_nan_stays_with_its_member(gpu_device):
    base = crd.make_params("fhn", "torus", 61, 80.0, 20.0, 0.12, 1.25, ny=183, t_boundary=0.05)
    members = [params_like(base, beta=0.9 + 0.1 * k) for k in range(4)]
    ys = [start_state(p, 31 + k) for k, p in enumerate(members)]
    bad = ys[2].copy()
    bad[100, 17, 1] = np.nan  # in var1: var0's neighbours take it up at the first step
    _, clean = observe_rows(members, ys, 0.0, 0.02, [4])
    _, poisoned = observe_rows(members, ys[:2] + [bad] + ys[3:], 0.0, 0.02, [4])
    assert np.all(np.isnan(poisoned["stats"][:, 2])), poisoned["stats"][:, 2]
    assert np.all(np.isnan(poisoned["mean"][:, 2])) and np.all(np.isnan(poisoned["variance"][:, 2]))
    for k in (0, 1, 3):
        assert np.all(np.isfinite(poisoned["stats"][:, k]))
        assert poisoned["stats"][:, k].tobytes() == clean["stats"][:, k].tobytes(), k


def test_adaptive_calls_record_one_sample_each(gpu_device):
    p = crd.make_params("fhn", "torus", 61, 80.0, 20.0, 0.12, 1.25, ny=183, t_boundary=0.3)
    members = [p, params_like(p, beta=0.9), params_like(p, diffusion=0.2), params_like(p, beta=1.1)]
    ys = [start_state(q, 41 + k) for k, q in enumerate(members)]
    touts = [0.1, 0.25, 0.4]
    probes = [(0, 0), (60, 182)]
    worst = [0.0]
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        G = e.observe(stride=5, probes=probes, capacity=3)["blocks_per_member"]  # (the stride counts fixed steps only)
        t0 = 0.0
        for q, tout in enumerate(touts):
            st = e.integrate_adaptive(t0, tout)
            assert all(s["status"] == crd._capi.OK for s in st)
            obs = e.observations()
            assert obs["t"].tolist() == touts[:q + 1]
            for k in range(4):
                y = e.download(k)
                check_row(obs["stats"][q, k], y, G, worst)
                for r, (i, j) in enumerate(probes):
                    assert obs["probes"][q, k, r].tolist() == y[j, i].tolist()
            t0 = tout
        L = crd._capi.lib()
        assert L.crd_ensemble_integrate_adaptive(e.handle, t0, t0 + 0.1, None, None, None) == EINVAL and "room" in e.last_error()
    # a member that fails alone (uploaded with a NaN: the 7-failure exit, CRD_ESTATE) has NaN rows, the others do not
    bad = ys[2].copy()
    bad[5, 7, 0] = np.nan
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys[:2] + [bad] + ys[3:]):
            e.upload(k, y)
        e.observe(probes=probes, capacity=2)
        st = e.integrate_adaptive(0.0, 0.1)
        assert [s["status"] for s in st] == [crd._capi.OK, crd._capi.OK, crd._capi.ESTATE, crd._capi.OK]
        obs = e.observations()
        assert obs["t"].tolist() == [0.1]
        assert np.all(np.isnan(obs["stats"][0, 2])) and np.all(np.isnan(obs["probes"][0, 2]))
        for k in (0, 1, 3):
            assert np.all(np.isfinite(obs["stats"][0, k])) and np.all(np.isfinite(obs["probes"][0, k]))
            check_row(obs["stats"][0, k], e.download(k), G, worst)
    print("observe adaptive: worst sum error / bound = %.3e" % worst[0])


def test_goldbeter_beta_scan_oscillates_inside_the_window_only(gpu_device):
    """The scan the feature is for: Goldbeter on a uniform field, beta = 0.2, 0.5, 0.9 around the oscillatory window 0.28895 .. 0.77427,
    8 x 16 points, from (Z, Y) = (0.3, 1.5), 1600 RK4 steps of 0.005 (t = 8), probe (2, 3) sampled every 10 steps.
    The CPU oracle's RK4 (oracle/crd_oracle.py, same dt, same sampling) gave, on the samples with t > 6 (the last quarter):
        beta 0.2   peak-to-peak 1.60e-4, state at t = 8 (0.24597999, 2.19340242)   [crd_steady_state: (0.246, 2.19355990)]
        beta 0.5   peak-to-peak 0.80421, period over the whole series 0.699639 (12 upward crossings)
        beta 0.9   peak-to-peak 0 to the last digit, state at t = 8 = crd_steady_state = (0.757, 0.79752322)
    Margins, from those: the middle member's tail amplitude within 0.01 of 0.80421 and its period within 1e-3 of 0.699639 (a fiftieth
    of the sample interval; device and oracle see the same sampling, their RK4 differ in rounding only); the outer members' tail
    amplitude <= 1e-3 (six times the larger oracle value) and their final probe values within 1e-3 of crd_steady_state (the oracle's
    largest distance: 1.6e-4); the whole probe series within 1e-6 of the oracle's (rounding differences of a stable limit cycle)."""
    nx, ny, dt, stride, nsamples = 8, 16, 0.005, 10, 160
    betas = (0.2, 0.5, 0.9)
    members = [crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, b, ny=ny) for b in betas]
    y0 = np.empty((ny, nx, 2))
    y0[..., 0], y0[..., 1] = 0.3, 1.5
    with crd.Ensemble(members) as e:
        for k in range(3):
            e.upload(k, y0)
        e.observe(stride=stride, probes=[(2, 3)], capacity=nsamples)
        e.step_rk4(0.0, dt, stride * nsamples, sync=False)
        obs = e.observations()
    t = obs["t"]
    series = obs["probes"][:, :, 0, :]  # [sample, member, field]
    tail = t > 6.0
    assert np.count_nonzero(tail) == 40
    amp = [float(np.ptp(series[tail, k, 0])) for k in range(3)]
    mid = post.oscillation_summary(t, series[:, 1, 0])
    print("scan: tail amplitudes %s, middle period %.6f (%d crossings)" % (amp, mid["period"], mid["crossings"]))
    assert abs(amp[1] - 0.80421) <= 0.01, amp
    assert abs(mid["period"] - 0.699639) <= 1e-3 and mid["crossings"] >= 10, mid
    for k in (0, 2):
        assert amp[k] <= 1e-3 and amp[1] > 100.0 * amp[k], amp
        z, y = crd.steady_state("goldbeter", betas[k])
        assert abs(series[-1, k, 0] - z) <= 1e-3 and abs(series[-1, k, 1] - y) <= 1e-3, (k, series[-1, k], z, y)
    # the field stays uniform: the statistics say so (min == max), and the mean is the probe's value
    assert np.array_equal(obs["stats"][:, :, 0, 0], obs["stats"][:, :, 0, 1])
    assert np.allclose(obs["mean"][:, :, 0], series[:, :, 0], rtol=1e-13, atol=0.0)
    assert np.all(obs["variance"] <= 1e-12)
    for k, b in enumerate(betas):
        op = co.make_problem(co.GOLDBETER, co.TORUS, nx, 80.0, 20.0, 0.12, b, ny=ny)
        y = y0.copy()
        for s in range(nsamples):
            y = co.rk4(op, y, s * stride * dt, dt, stride)
            assert abs(y[3, 2, 0] - series[s, k, 0]) <= 1e-6 and abs(y[3, 2, 1] - series[s, k, 1]) <= 1e-6, (k, s, y[3, 2], series[s, k])


def test_slab_observe_is_the_ensemble_of_one_row(gpu_device):
    for precision, nx, ny in (("f64", 61, 183), ("f32", 64, 0), ("f64", 64, 0)):
        p = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=ny, precision=precision)
        y = start_state(p, 51).astype(dtype_of(p))
        with crd.Ensemble([p]) as e:
            e.upload(0, y)
            e.observe(capacity=1)
            e.step_rk4(0.0, 0.02, 1)
            row = e.observations()["stats"][0, 0]
            after = e.download(0, dtype_of(p))
        with crd.Slab(p) as s:
            s.upload(after)
            got = s.observe()
            assert s.max_abs() == max(abs(got[0, 0]), abs(got[0, 1]))
        assert got.tobytes() == row.tobytes(), (precision, nx, got, row)
    with crd.LocalGroup(crd.make_params("fhn", "torus", 32, 80.0, 20.0, 0.12, 1.25), 2) as grp:
        with pytest.raises(crd.CrdError) as err:
            grp.slabs[1].observe()
        assert err.value.status == EINVAL and "single-slab" in str(err.value)


def test_driver_observe_leaves_the_state_files_alone(gpu_device, tmp_path):
    ini = os.path.join(INI, "small_run.ini")
    common = [os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus", "--quiet", "--ensemble", "beta=1.0,1.25,1.4"]
    plain, seen = str(tmp_path / "plain"), str(tmp_path / "seen")
    subprocess.run(common + ["--outdir", plain, ini], check=True, capture_output=True, timeout=300)
    r = subprocess.run(common + ["--outdir", seen, "--observe", "2", "--probe", "0,0", "--probe", "15,39", "--observe-maps", "0.0", ini], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for k in range(3):
        a, b = os.path.join(plain, "member_%d" % k), os.path.join(seen, "member_%d" % k)
        names = sorted(os.listdir(a))
        assert names and sorted(os.listdir(b)) == sorted(names + ["observables.txt", "amplitude_map.npy", "activation_time.npy"])
        match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
        assert not mismatch and not errors, (mismatch, errors)
        lines = open(os.path.join(b, "observables.txt")).read().splitlines()
        assert lines[0].startswith("# t min0 max0 sum0 sumsq0 min1 max1 sum1 sumsq1 var0(0,0) var1(0,0) var0(15,39) var1(15,39)")
        rows = np.loadtxt(os.path.join(b, "observables.txt"))
        assert rows.ndim == 2 and rows.shape[1] == 1 + 8 + 4 and rows.shape[0] >= 1 and np.all(np.diff(rows[:, 0]) > 0)
        assert np.all(rows[:, 1] <= rows[:, 9]) and np.all(rows[:, 9] <= rows[:, 2])  # min0 <= var0 at a probe <= max0
        amp, act = np.load(os.path.join(b, "amplitude_map.npy")), np.load(os.path.join(b, "activation_time.npy"))
        assert amp.shape == act.shape == (40, 16) and np.all(amp >= 0.0)
        assert np.all(np.isnan(act) | ((act >= rows[0, 0]) & (act <= rows[-1, 0])))
