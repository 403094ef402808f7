"""Ensembles with every member at its own step size (crd_ensemble_step_rk4_own, crd_ensemble_own_steps, Ensemble.step_rk4_own,
crd_run --ensemble-own-dt): member k goes from t0 to t1 in n_k RK4 steps of (t1 - t0) / n_k, one launch per round for the members that
still have steps left.  Every state comparison is np.array_equal against a context of the member's parameters stepped alone with the
one-launch stepper, step_rk4(t0, (t1 - t0) / n_k, n_k).  The shapes are the smallest that reach every branch of the block mapping: a
wavefront holds 56 valid columns in fp64 (120 with two columns per lane in fp32), a block four wavefronts."""
import copy
import filecmp
import math
import os
import re
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

EINVAL = crd._capi.EINVAL


def params_like(p, **kw):
    q = copy.copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def dtype_of(p):
    return np.float64 if p.precision == crd._capi.PRECISION_F64 else np.float32


def start_state(p, seed):
    cfg = crd.run_config(p, wave_length=0.1, wave_width=0.5, wave_inside=0)
    y = crd.initial_conditions(cfg)
    y = y + 0.05 * np.random.default_rng(seed).standard_normal(y.shape)
    return y.astype(dtype_of(p))


def lone(p, y0, calls, observe=False):
    """A context of p stepped alone with the one-launch stepper: calls = [(t0, dt, steps), ...]."""
    with crd.Slab(p) as s:
        s.set_stepper("fused")
        s.set_autotune(0)
        s.set_launch_plan(0, 0, 1, 0, 1)
        s.upload(y0)
        for t0, dt, n in calls:
            s.step_rk4(t0, dt, n)
        y = s.download(dtype_of(p))
        return (y, s.observe()) if observe else y


def own_calls(segments, k):
    """segments = [(t0, t1, counts), ...] -> member k's lone calls."""
    return [(t0, (t1 - t0) / n[k], n[k]) for t0, t1, n in segments]


def run_own(members, ys, segments, mixed=False):
    with crd.Ensemble(members, mixed=mixed) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        for t0, t1, n in segments:
            assert e.step_rk4_own(t0, t1, n) == list(n)
        assert all(np.isfinite(m) for m in e.max_abs())
        return [e.download(k, dtype_of(members[k])) for k in range(len(members))]


def check_members(members, ys, got, segments):
    for k, p in enumerate(members):
        want = lone(p, ys[k], own_calls(segments, k))
        assert got[k].shape == (p.ny, p.nx, 2) and got[k].dtype == dtype_of(p)
        assert np.array_equal(got[k], want), ("member", k, float(np.max(np.abs(got[k] - want))))


def fhn(nx, ny, surface="torus", precision="f64", **kw):
    kw.setdefault("beta", 1.25)
    kw.setdefault("diffusion", 0.12)
    d, b = kw.pop("diffusion"), kw.pop("beta")
    return crd.make_params("fhn", surface, nx, 80.0, 20.0, d, b, ny=ny, beta_min=0.7, beta_max=1.7, precision=precision, **kw)


# ---- 1: uniform, three strips (a block with a surplus wavefront), an active set that is no prefix, a last round of one member ----

@pytest.mark.parametrize("segments", [[(0.0, 0.1, (5, 1, 3, 1, 4))], [(0.0, 0.04, (5, 1, 3, 1, 4)), (0.04, 0.1, (5, 1, 3, 1, 4))]], ids=["one-call", "two-calls"])
def test_uniform_fhn_fp64(gpu_device, segments):
    members = [fhn(113, 16, diffusion=0.06, beta=1.25, t_boundary=0.05), fhn(113, 16, diffusion=0.12, beta=0.9, t_boundary=0.0),
               fhn(113, 16, diffusion=0.24, beta=1.1, t_boundary=10.0), fhn(113, 16, diffusion=0.12, beta=1.4, t_boundary=0.07),
               fhn(113, 16, diffusion=0.06, beta=1.0, t_boundary=0.02)]
    ys = [start_state(p, k) for k, p in enumerate(members)]
    check_members(members, ys, run_own(members, ys, segments), segments)


# ---- 2: widths of two and of five strips (two blocks per chunk row), short and tall ----

@pytest.mark.parametrize("ny", [9, 37])
@pytest.mark.parametrize("nx", [57, 230])
def test_widths(gpu_device, nx, ny):
    members = [fhn(nx, ny, beta=1.25, t_boundary=0.03), fhn(nx, ny, beta=0.9, diffusion=0.2), fhn(nx, ny, beta=1.1, t_boundary=10.0)]
    ys = [start_state(p, 10 + k) for k, p in enumerate(members)]
    segments = [(0.0, 0.06, (2, 3, 1))]
    check_members(members, ys, run_own(members, ys, segments), segments)


# ---- 3: every member decides on its absorbing rows against its own stage times ----

def test_per_member_absorbing_decisions(gpu_device):
    """Over [0, 0.08] with tBoundary = 0.03: the one-step member (stages at 0, 0.04, 0.04, 0.08) absorbs at its first stage only; the
    two-step member (0, 0.02, 0.02, 0.04 | ...) throughout its first step; the four-step member (dt = 0.02) throughout its first step,
    at the first stage of its second (0.02; the half-step stages fall on 0.03 itself: strict <), then no more.  Then a member that never
    absorbs, one that always does, and one whose tBoundary IS t0 + 2 dt_k as the library forms it: its third step does not absorb."""
    t0, t1 = 0.0, 0.08
    counts = (1, 2, 4, 3, 2, 4)
    tbs = [0.03, 0.03, 0.03, 0.0, 10.0, t0 + 2.0 * ((t1 - t0) / 4)]
    assert tbs[5] == 0.04 and 0.02 + 0.5 * 0.02 == 0.03  # (the equality cases are equalities in double)
    members = [fhn(61, 20, beta=b, t_boundary=tb) for b, tb in zip((1.25, 0.9, 1.1, 1.3, 1.0, 1.2), tbs)]
    ys = [start_state(p, 20 + k) for k, p in enumerate(members)]
    segments = [(t0, t1, counts)]
    got = run_own(members, ys, segments)
    check_members(members, ys, got, segments)
    # the decisions matter: the same member with the boundary rows never held ends elsewhere
    for k in (0, 2, 5):
        free = lone(params_like(members[k], t_boundary=0.0), ys[k], own_calls(segments, k))
        assert not np.array_equal(got[k], free), ("member", k)


# ---- 4: fp32, two columns per lane and one ----

@pytest.mark.parametrize("nx", [122, 57])
def test_fp32(gpu_device, nx):
    members = [fhn(nx, 20, precision="f32", beta=b, t_boundary=tb) for b, tb in ((1.25, 0.03), (0.9, 0.0), (1.1, 10.0))]
    ys = [start_state(p, 30 + k) for k, p in enumerate(members)]
    segments = [(0.0, 0.06, (3, 1, 2))]
    check_members(members, ys, run_own(members, ys, segments), segments)


# ---- 5: Goldbeter and the diffusion-only variant ----

@pytest.mark.parametrize("just_diffusion", [0, 1], ids=["goldbeter", "diffusion-only"])
def test_goldbeter_fp64_and_diffusion_only(gpu_device, just_diffusion):
    members = [crd.make_params("goldbeter", "torus", 61, 80.0, 20.0, d, b, ny=20, t_boundary=tb, just_diffusion=just_diffusion)
               for d, b, tb in ((0.12, 0.4, 0.03), (0.2, 0.5, 10.0), (0.06, 0.9, 0.0))]
    ys = [start_state(p, 40 + k) for k, p in enumerate(members)]
    segments = [(0.0, 0.06, (2, 4, 1))]
    check_members(members, ys, run_own(members, ys, segments), segments)


# ---- 6: members of different shape ----

def mixed_fhn_set(precision="f64", t_far=10.0):
    """tests/test_gpu_ensemble_mixed.py's fhn_set: one strip; two strips, absorbing early; five strips absorbing throughout; three
    strips; the smallest member again, last, with another beta."""
    return [fhn(40, 9), fhn(57, 37, "flat", t_boundary=0.05), fhn(230, 70, t_boundary=t_far), fhn(113, 16, "flat"), fhn(40, 9, beta=0.9)]


def test_mixed_shapes_and_their_order(gpu_device):
    """Counts (2, 5, 1, 3, 4): the largest member leaves first, and the prefix of block counts is rebuilt after rounds 1, 2, 3 and 4."""
    members = mixed_fhn_set()
    ys = [start_state(p, 50 + k) for k, p in enumerate(members)]
    counts = (2, 5, 1, 3, 4)
    segments = [(0.0, 0.06, counts)]
    got = run_own(members, ys, segments, mixed=True)
    check_members(members, ys, got, segments)
    perm = [2, 4, 0, 3, 1]
    again = run_own([members[i] for i in perm], [ys[i] for i in perm], [(0.0, 0.06, tuple(counts[i] for i in perm))], mixed=True)
    for slot, i in enumerate(perm):
        assert np.array_equal(again[slot], got[i]), ("member", i)


@pytest.mark.parametrize("widths", [(40, 122, 242), (40, 57, 242)])
def test_mixed_fp32_two_columns_and_one(gpu_device, widths):
    members = [fhn(nx, ny, s, precision="f32", t_boundary=tb) for s, nx, ny, tb in zip(("torus", "flat", "torus"), widths, (9, 37, 70), (0.0, 0.03, 10.0))]
    ys = [start_state(p, 60 + k) for k, p in enumerate(members)]
    segments = [(0.0, 0.06, (3, 1, 2))]
    check_members(members, ys, run_own(members, ys, segments, mixed=True), segments)


# ---- 7: the other calls behind it ----

@pytest.mark.parametrize("mixed", [False, True], ids=["uniform", "mixed"])
def test_call_sequences(gpu_device, mixed):
    members = [fhn(57, 37, "flat", t_boundary=0.05), fhn(113, 16, t_boundary=10.0), fhn(40, 9, beta=0.9)] if mixed else \
              [fhn(61, 12, t_boundary=0.05), fhn(61, 12, beta=0.9, t_boundary=10.0), fhn(61, 12, diffusion=0.2)]
    ys = [start_state(p, 70 + k) for k, p in enumerate(members)]
    dt = 0.02
    n1, n2 = (3, 2, 1), (2, 1, 4)
    walk = [[] for _ in members]  # every member's lone calls so far
    with crd.Ensemble(members, mixed=mixed) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)

        def settled(calls):
            for k in range(len(members)):
                walk[k] += calls(k)
            assert all(np.isfinite(m) for m in e.max_abs())
            return [e.download(k) for k in range(len(members))]

        e.step_rk4_own(0.0, 0.06, n1)  # odd and even counts: members end in different buffers
        settled(lambda k: own_calls([(0.0, 0.06, n1)], k))
        e.step_rk4(0.06, dt, 3)
        settled(lambda k: [(0.06, dt, 3)])
        e.set_steps_per_launch(2)
        e.step_rk4(0.12, dt, 5)
        settled(lambda k: [(0.12, dt, 5)])
        e.step_rk4_own(0.22, 0.28, n2)  # single steps whatever the setting says
        assert e.steps_per_launch == 2
        got = settled(lambda k: own_calls([(0.22, 0.28, n2)], k))
    for k, p in enumerate(members):
        assert np.array_equal(got[k], lone(p, ys[k], walk[k])), ("member", k)


# ---- 8: equal counts are crd_ensemble_step_rk4 ----

def test_equal_counts_are_the_common_step(gpu_device):
    members = [fhn(113, 16, t_boundary=0.05), fhn(113, 16, beta=0.9), fhn(113, 16, diffusion=0.2, t_boundary=10.0)]
    ys = [start_state(p, 80 + k) for k, p in enumerate(members)]
    t0, t1, n = 0.01, 0.09, 4
    got = run_own(members, ys, [(t0, t1, (n, n, n))])
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.step_rk4(t0, (t1 - t0) / n, n)
        for k in range(3):
            assert np.array_equal(got[k], e.download(k)), ("member", k)


# ---- 8b: the step sizes given instead of formed (crd_ensemble_step_rk4_own_dt), and the event-timed form ----

def test_given_step_sizes(gpu_device):
    """Where (t1 - t0) / n_k is what the caller hands over, the call is step_rk4_own itself; where it is not -- a driver's
    dTout / n_k with (t + dTout) - t one bit off dTout -- member k has the bits of the lone context stepped at the size given."""
    members = [fhn(113, 16, t_boundary=0.05), fhn(113, 16, beta=0.9), fhn(113, 16, diffusion=0.2, t_boundary=10.0)]
    ys = [start_state(p, 85 + k) for k, p in enumerate(members)]
    counts = (3, 1, 2)
    t0, t1 = 0.25, 0.75  # exact in double, their difference too
    formed = run_own(members, ys, [(t0, t1, counts)])
    d_out = 1.2 / 3
    t = 2 * d_out
    assert (t + d_out) - t != d_out  # the driver's third output interval of tFinal 1.2 in three outputs
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.step_rk4_own(t0, t1, counts, dt=[(t1 - t0) / n for n in counts])
        for k in range(3):
            assert np.array_equal(e.download(k), formed[k]), ("member", k)
            e.upload(k, ys[k])
        e.step_rk4_own(t, t + d_out, counts, dt=[d_out / n for n in counts])
        for k, p in enumerate(members):
            assert np.array_equal(e.download(k), lone(p, ys[k], [(t, d_out / counts[k], counts[k])])), ("member", k)
        with pytest.raises(crd.CrdError) as err:
            e.step_rk4_own(t0, t1, counts, dt=[0.1, 0.0, 0.1])
        assert err.value.status == EINVAL and "member 1" in e.last_error()


def test_timed_form_is_the_call(gpu_device):
    members = [fhn(61, 12, t_boundary=0.05), fhn(61, 12, beta=0.9)]
    ys = [start_state(p, 88 + k) for k, p in enumerate(members)]
    segments = [(0.0, 0.06, (3, 2))]
    want = run_own(members, ys, segments)
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        ms = e.step_rk4_own_timed(*segments[0])
        assert ms > 0.0
        for k in range(2):
            assert np.array_equal(e.download(k), want[k]), ("member", k)


# ---- 9: the observer ----

def test_observer_one_sample_per_call(gpu_device):
    members = [fhn(61, 37, t_boundary=0.05), fhn(61, 37, beta=0.9, t_boundary=10.0), fhn(61, 37, diffusion=0.2)]
    ys = [start_state(p, 90 + k) for k, p in enumerate(members)]
    probes, column = [(3, 2), (60, 36)], 17
    segments = [(0.0, 0.04, (2, 1, 3)), (0.04, 0.1, (3, 4, 1)), (0.1, 0.12, (1, 2, 2))]
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.observe(stride=2, probes=probes, maps=True, threshold=0.1, capacity=3, sections=[("column", column)], cycles=True, cycle_threshold=0.1)
        states = []
        for t0, t1, n in segments:
            e.step_rk4_own(t0, t1, n)
            states.append([e.download(k) for k in range(3)])
        assert e.observed_count() == 3
        obs, lines = e.observations(), e.observed_section(0)
        maps, cycles = [e.observed_maps(k) for k in range(3)], [e.observed_cycles(k) for k in range(3)]
        # a fourth call finds no room: refused whole, the state where it was
        with pytest.raises(crd.CrdError) as err:
            e.step_rk4_own(0.12, 0.14, (1, 1, 1))
        assert err.value.status == EINVAL and "room" in e.last_error()
        assert e.observed_count() == 3
        for k in range(3):
            assert np.array_equal(e.download(k), states[2][k])
        e.end_observe()
    assert np.array_equal(obs["t"], np.array([s[1] for s in segments]))
    for i in range(3):
        for k, p in enumerate(members):
            y, row = lone(p, ys[k], own_calls(segments[:i + 1], k), observe=True)
            assert np.array_equal(states[i][k], y)
            assert np.array_equal(obs["stats"][i, k], row), ("sample", i, "member", k)
            for q, (pi, pj) in enumerate(probes):
                assert np.array_equal(obs["probes"][i, k, q], states[i][k][pj, pi]), ("sample", i, "member", k, "probe", q)
            assert np.array_equal(lines[i, k], states[i][k][:, column, :]), ("sample", i, "member", k)
    for k in range(3):
        u = np.stack([states[i][k][..., 0] for i in range(3)])
        assert np.array_equal(maps[k][0], u.min(axis=0)) and np.array_equal(maps[k][1], u.max(axis=0))
        count = cycles[k][0]
        up = sum(((u[i - 1] < 0.1) & (u[i] >= 0.1)).astype(np.int32) for i in (1, 2))
        assert np.array_equal(count, up), ("member", k)


def test_observer_mixed_rows_are_an_ensemble_of_ones(gpu_device):
    members = mixed_fhn_set()[:4]
    ys = [start_state(p, 100 + k) for k, p in enumerate(members)]
    probes = [(3, 2), (39, 8)]
    segments = [(0.0, 0.04, (2, 1, 3, 1)), (0.04, 0.06, (1, 2, 1, 3))]
    with crd.Ensemble(members, mixed=True) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.observe(stride=1, probes=probes, capacity=4)
        for t0, t1, n in segments:
            e.step_rk4_own(t0, t1, n)
        obs = e.observations()
        e.end_observe()
    assert obs["stats"].shape[0] == 2
    for k, p in enumerate(members):
        with crd.Ensemble([p]) as one:
            one.upload(0, ys[k])
            one.observe(stride=1, probes=probes, capacity=4)
            for t0, t1, n in segments:
                one.step_rk4_own(t0, t1, (n[k],))
            want = one.observations()
        assert np.array_equal(obs["t"], want["t"])
        assert np.array_equal(obs["stats"][:, k], want["stats"][:, 0]), ("member", k)
        assert np.array_equal(obs["probes"][:, k], want["probes"][:, 0]), ("member", k)


# ---- 10: error control starts afresh behind it ----

def test_adaptive_starts_afresh_behind_own_steps(gpu_device):
    members = [fhn(61, 20, t_boundary=0.05), fhn(61, 20, beta=0.9), fhn(61, 20, diffusion=0.2, t_boundary=10.0)]
    ys = [start_state(p, 110 + k) for k, p in enumerate(members)]
    t1, t2 = 0.06, 0.16
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        e.integrate_adaptive(0.0, 0.02)  # a carry-over for the own steps to end
        e.step_rk4_own(0.02, t1, (3, 2, 1))
        mid = [e.download(k) for k in range(3)]
        st = e.integrate_adaptive(t1, t2)
        got = [e.download(k) for k in range(3)]
    with crd.Ensemble(members) as f:
        for k in range(3):
            f.upload(k, mid[k])
        want_st = f.integrate_adaptive(t1, t2)
        for k in range(3):
            assert st[k] == want_st[k], ("member", k, st[k], want_st[k])
            assert np.array_equal(got[k], f.download(k)), ("member", k)


# ---- 11: the rule ----

def test_own_steps_rule(gpu_device):
    members = [fhn(113, 16, diffusion=d) for d in (0.06, 0.12, 0.24, 0.48)]
    with crd.Ensemble(members) as e:
        for t0, t1, s in ((0.0, 1.0, 0.8), (0.3, 2.7, 0.5), (0.0, 1e-6, 0.8)):
            want = [max(1, math.ceil((t1 - t0) / (s * crd.stable_dt(p)) - 1e-12)) for p in members]
            assert e.own_steps(t0, t1, s) == want, (t0, t1, s)
        counts = e.own_steps(0.0, 1.0, 0.8)
        assert len(set(counts)) == 4 and counts == sorted(counts), counts
        assert e.own_steps(0.0, 1e-6) == [1, 1, 1, 1]
    mixed = mixed_fhn_set()
    with crd.Ensemble(mixed, mixed=True) as e:
        assert e.own_steps(0.0, 2.0, 0.8) == [max(1, math.ceil(2.0 / (0.8 * crd.stable_dt(p)) - 1e-12)) for p in mixed]


# ---- 12: refusals ----

def test_refusals_leave_the_ensemble_stepping(gpu_device):
    members = [fhn(61, 12, t_boundary=0.05), fhn(61, 12, beta=0.9)]
    ys = [start_state(p, 120 + k) for k, p in enumerate(members)]
    L, C = crd._capi.lib(), crd._capi.C
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)

        def refused(call, *words):
            with pytest.raises(crd.CrdError) as err:
                call()
            assert err.value.status == EINVAL, err.value
            for w in words:
                assert w in e.last_error(), (w, e.last_error())

        n = (C.c_int64 * 2)(2, 3)
        assert L.crd_ensemble_step_rk4_own(None, 0.0, 0.1, n) == EINVAL
        assert L.crd_ensemble_step_rk4_own(e.handle, 0.0, 0.1, None) == EINVAL and "null" in e.last_error()
        assert L.crd_ensemble_own_steps(None, 0.0, 0.1, 0.8, n) == EINVAL
        assert L.crd_ensemble_own_steps(e.handle, 0.0, 0.1, 0.8, None) == EINVAL and "null" in e.last_error()
        refused(lambda: e.step_rk4_own(float("nan"), 0.1, (2, 3)), "finite")
        refused(lambda: e.step_rk4_own(0.0, float("inf"), (2, 3)), "finite")
        refused(lambda: e.step_rk4_own(0.1, 0.1, (2, 3)), "t1")
        refused(lambda: e.step_rk4_own(0.1, 0.0, (2, 3)), "t1")
        refused(lambda: e.step_rk4_own(0.0, 0.1, (2, 0)), "member 1", "nsteps")
        refused(lambda: e.step_rk4_own(0.0, 0.1, (-1, 3)), "member 0", "nsteps")
        refused(lambda: e.own_steps(0.1, 0.0), "t1")
        refused(lambda: e.own_steps(float("nan"), 1.0), "finite")
        for k in range(2):
            assert np.array_equal(e.download(k), ys[k]), ("member", k)  # nothing was launched
        segments = [(0.0, 0.06, (2, 3))]
        e.step_rk4_own(*segments[0])
        for k, p in enumerate(members):
            assert np.array_equal(e.download(k), lone(p, ys[k], own_calls(segments, k))), ("member", k)


# ---- 13: the driver ----

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
SMALL_INI = os.path.join(GOLDEN, "ini", "small_run.ini")


def write_ini(path, **overrides):
    out = []
    for line in open(SMALL_INI).read().splitlines():
        key = line.split("=")[0].strip()
        out.append("%s = %s" % (key, overrides[key]) if key in overrides else line)
    path.write_text("\n".join(out) + "\n")
    return str(path)


def crd_run(args, cwd, quiet=True):
    return subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus"] + (["--quiet"] if quiet else []) + args, cwd=cwd,
                          capture_output=True, text=True, timeout=300)


def same_files(a, b):
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b)), (names, sorted(os.listdir(b)))
    _, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


@pytest.mark.parametrize("keys,lone_inis,counts_differ", [
    (["diffusion=0.12,6"], [{"diffusion": "0.12"}, {"diffusion": "6"}], True),
    # ... and members of truly different shape (the ini pins ny by phiMesh): the mixed launches
    (["xMesh=16,24", "surfaceLength=80,40"], [{"thetaMesh": "16", "surfaceLength": "80"}, {"thetaMesh": "24", "surfaceLength": "40"}], False),
])
def test_driver_members_write_what_lone_runs_of_the_plain_ini_write(gpu_device, tmp_path, keys, lone_inis, counts_differ):
    ini = write_ini(tmp_path / "own.ini", dt="0")
    (tmp_path / "ens").mkdir()
    args = []
    for k in keys:
        args += ["--ensemble", k]
    r = crd_run(args + ["--ensemble-own-dt", "--outdir", str(tmp_path / "ens"), ini], tmp_path, quiet=False)
    assert r.returncode == 0, r.stderr
    per_output = [int(n) for n in re.findall(r"member \d+: dt = \S+ \((\d+) steps per output\)", r.stdout)]
    assert len(per_output) == 2 and (per_output[0] != per_output[1] or not counts_differ), r.stdout
    for k, overrides in enumerate(lone_inis):
        lone_dir = tmp_path / ("lone%d" % k)
        lone_dir.mkdir()
        r = crd_run(["--outdir", str(lone_dir), write_ini(tmp_path / ("m%d.ini" % k), dt="0", **overrides)], tmp_path)
        assert r.returncode == 0, r.stderr
        same_files(str(tmp_path / "ens" / ("member_%d" % k)), str(lone_dir))


def test_driver_observes_once_per_output(gpu_device, tmp_path):
    ini = write_ini(tmp_path / "own.ini", dt="0")
    r = crd_run(["--ensemble", "diffusion=0.12,6", "--ensemble-own-dt", "--observe", "1", "--probe", "3,2", "--outdir", str(tmp_path), ini], tmp_path)
    assert r.returncode == 0, r.stderr
    for k in range(2):
        rows = [l for l in open(tmp_path / ("member_%d" % k) / "observables.txt").read().splitlines() if l.strip() and not l.lstrip().startswith("#")]
        assert len(rows) == 3, rows  # outputTimestep = 3


# ---- 9: every instantiation of crd_ensemble_own_kernel on the smallest shapes that reach every branch of the shared set-up ----

def small_own_set(model, precision, even, mixed, tb):
    """Uniform: two members of 131 (132) x 21; mixed: 131 x 41, 60 x 25, 131 x 9.  The first member absorbs until tb, the others never."""
    w = 132 if even else 131
    def mk(nx, ny, beta, tb):
        if model == "fhn":
            return fhn(nx, ny, precision=precision, beta=beta, t_boundary=tb)
        return crd.make_params("goldbeter", "torus", nx, 80.0, 20.0, 0.12, 0.4 * beta, ny=ny, precision=precision, t_boundary=tb, just_diffusion=int(model == "diffusion_only"))
    if mixed:
        return [mk(w, 41, 1.25, tb), mk(60, 25, 1.0, 0.0), mk(w, 9, 0.9, 0.0)], (3, 1, 2)
    return [mk(w, 21, 1.25, tb), mk(w, 21, 0.9, 0.0)], (3, 1)


SMALL_OWN_CASES = [(m, p, e, x) for x in (False, True) for m in ("fhn", "goldbeter", "diffusion_only") for p, e in (("f64", False), ("f32", False), ("f32", True))]


@pytest.mark.parametrize("model,precision,even,mixed", SMALL_OWN_CASES)
def test_smallest_shapes_of_the_shared_setup(gpu_device, model, precision, even, mixed):
    """Over [0, t1] with tBoundary = t1 / 2: the three-step member absorbs through its first step and at the first stage of its second,
    beside members that never absorb; the last round launches the plain instantiation.  t1 = 0.06; 0.015 for Goldbeter, whose kinetics
    bound the RK4 step of these grids at 0.0066 (crd.stable_dt): three steps of 0.02 would overflow fp32."""
    t1 = 0.015 if model == "goldbeter" else 0.06
    members, counts = small_own_set(model, precision, even, mixed, 0.5 * t1)
    ys = [start_state(p, 90 + k) for k, p in enumerate(members)]
    segments = [(0.0, t1, counts)]
    check_members(members, ys, run_own(members, ys, segments, mixed=mixed), segments)
