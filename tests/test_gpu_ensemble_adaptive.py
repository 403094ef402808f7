"""Error-controlled ensembles on the GPU (crd_ensemble_integrate_adaptive, Ensemble.integrate_adaptive, crd_run --ensemble with
[Solver] adaptive = 1): every member against a lone context (crd.Slab) of its parameters running the same calls, the oracle's
restatement of ARKode on a small grid, members independent of each other, carry-over between calls, B = 1 and B = 64, the driver.

Tolerances ("Ensembles"): a member's attempt norm is summed over the ensemble's partition of work items, not a lone
context's, so the norms -- and with them the step sizes -- agree to ~1e-15, not bit for bit.  The first step (arkHin) is computed by
the same arithmetic in the same order: 1e-12.  Accept / reject counts: identical.  Internal time and next step: 1e-6, states: 1e-9 --
the ones the ARKode tests and the ring-versus-single-slab check use."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
from conftest import GOLDEN, ROOT, crd_params, load_golden, oracle_problem, rel_err

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "crdmodel_amd", "bin")
SMALL_INI = os.path.join(GOLDEN, "ini", "small_run.ini")
F32 = crd._capi.PRECISION_F32


def params_like(p, **kw):
    q = copy.copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def start_state(p, seed):
    cfg = crd.run_config(p, wave_length=0.1, wave_width=0.5, wave_inside=0)
    y = crd.initial_conditions(cfg)
    rng = np.random.default_rng(seed)
    y = y + 0.02 * rng.standard_normal(y.shape)
    return y.astype(np.float32) if p.precision == F32 else y


def dtype_of(p):
    return np.float32 if p.precision == F32 else np.float64


def lone_calls(p, y0, calls, **opt):
    """A context of p integrated alone: the stats and state after each call."""
    out = []
    with crd.Slab(p) as s:
        s.upload(y0)
        for t0, tout in calls:
            st = s.integrate_adaptive(t0, tout, **opt)
            out.append((st, s.download(dtype_of(p))))
    return out


def compare(st, y, want_st, want_y, fresh, state_tol=1e-9):
    """One member's call against a lone context's (y None: stats only)."""
    if fresh:
        assert st["h_first"] == pytest.approx(want_st["h_first"], rel=1e-12), (st, want_st)
    else:
        assert st["h_first"] == pytest.approx(want_st["h_first"], rel=1e-6), (st, want_st)
    assert (st["accepted"], st["rejected"]) == (want_st["accepted"], want_st["rejected"]), (st, want_st)
    assert st["t"] == want_st["t"]
    assert st["t_internal"] == pytest.approx(want_st["t_internal"], rel=1e-6)
    assert st["h_next"] == pytest.approx(want_st["h_next"], rel=1e-6)
    if y is not None:
        assert rel_err(y, want_y) <= state_tol, rel_err(y, want_y)


def check_members(members, calls, state_tol=1e-9, seed=0, **opt):
    ys = [start_state(p, seed + k) for k, p in enumerate(members)]
    got = [[] for _ in members]
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        for t0, tout in calls:
            sts = e.integrate_adaptive(t0, tout, **opt)
            for k in range(len(members)):
                assert sts[k]["status"] == crd._capi.OK, sts[k]
                got[k].append((sts[k], e.download(k, dtype_of(members[k]))))
    rejected = 0
    for k, p in enumerate(members):
        want = lone_calls(p, ys[k], calls, **opt)
        for c, ((st, y), (wst, wy)) in enumerate(zip(got[k], want)):
            compare(st, y, wst, wy, fresh=c == 0, state_tol=state_tol)
            rejected += st["rejected"]
    return rejected


TOUTS = [0.5, 1.0, 1.0001, 1.5]
CALLS = list(zip([0.0] + TOUTS[:-1], TOUTS))


@pytest.mark.parametrize("nx", [61, 130])
@pytest.mark.parametrize("h_max", [-1.0, 0.0])
def test_members_follow_lone_contexts(gpu_device, nx, h_max):
    """FHN torus on a ragged nx; members differ in beta, varyBeta, diffusion and tBoundary (some inside a call).  Error control alone
    (h_max = -1) is compared over its first call and one inside the step it ended on: on these diffusion-limited grids the controller
    soon probes the stability bound, where the error estimate is rounding noise of a cancellation -- a difference of one ulp in a
    norm (the member's and the lone context's are summed in another order) gives other noise at the next step, and the step sequences
    drift apart at ~1e-5 after a few dozen steps, as two correct ARKode builds would (test_gpu_parity's oracle comparisons keep to
    such horizons for the same reason).  Capped at the stability bound (h_max = 0) on nx = 61 they stay together over all four calls;
    on nx = 130 the capped run drifts like that in its second call already, and is compared over the same horizon as h_max = -1."""
    p = crd.make_params("fhn", "torus", nx, 80.0, 20.0, 0.12, 1.25, ny=3 * nx, beta_min=0.7, beta_max=1.7)
    members = [p, params_like(p, beta=1.1, t_boundary=0.3), params_like(p, vary_beta=1, diffusion=0.2), params_like(p, diffusion=0.05, t_boundary=1.2),
               params_like(p, beta=1.4, t_boundary=3.0)]
    rejected = check_members(members, CALLS if (h_max == 0.0 and nx == 61) else [(0.0, 0.5), (0.5, 0.5001)], h_max=h_max)
    if h_max < 0:
        assert rejected >= 1  # error control alone on a diffusion-limited grid: the error test does fail now and then


@pytest.mark.parametrize("just_diffusion", [0, 1], ids=["goldbeter", "diffusion-only"])
def test_fp32_goldbeter_and_diffusion_only(gpu_device, just_diffusion):
    """The fp32 attempt kernels of Goldbeter (plain and absorbing) and of the diffusion-only variant on 131 x 21: three strips of 54
    valid columns, the last partial, six 4-row chunks.  One member absorbs until t = 0.02, inside the first call, one never does: the
    first rounds launch the absorbing instantiation with both bodies, the later ones the plain one."""
    p = crd.make_params("goldbeter", "torus", 131, 80.0, 20.0, 0.12, 0.5, ny=21, t_boundary=0.02, precision="f32", just_diffusion=just_diffusion)
    members = [p, params_like(p, beta=0.3, t_boundary=0.0), params_like(p, diffusion=0.2, t_boundary=0.0)]
    # (fp32: the tolerance test_other_models_and_precisions uses for fp32 states)
    check_members(members, [(0.0, 0.05), (0.05, 0.0501)], state_tol=1e-5, h_max=0.0)


@pytest.mark.parametrize("kind", ["goldbeter", "diffusion_only", "flat", "fp32"])
def test_other_models_and_precisions(gpu_device, kind):
    calls = [(0.0, 0.05), (0.05, 0.0501), (0.0501, 0.3)]
    if kind == "goldbeter":
        p = crd.make_params("goldbeter", "torus", 64, 80.0, 20.0, 0.12, 0.5, ny=160, t_boundary=0.1)
        members = [p, params_like(p, beta=0.2), params_like(p, beta=0.9, diffusion=0.3), params_like(p, beta=0.6, t_boundary=0.0)]
    elif kind == "diffusion_only":
        p = crd.make_params("goldbeter", "torus", 64, 80.0, 20.0, 0.12, 0.5, ny=160, just_diffusion=1)
        members = [p, params_like(p, diffusion=0.3), params_like(p, diffusion=0.05)]
    elif kind == "flat":
        p = crd.make_params("fhn", "flat", 70, 80.0, 20.0, 0.12, 1.25, ny=140, t_boundary=0.2)
        members = [p, params_like(p, beta=1.0, t_boundary=0.0), params_like(p, diffusion=0.2)]
        calls = CALLS[:3]
    else:
        p = crd.make_params("fhn", "torus", 61, 80.0, 20.0, 0.12, 1.25, ny=183, t_boundary=0.3, precision="f32")
        members = [p, params_like(p, beta=1.0), params_like(p, diffusion=0.2, t_boundary=0.0)]
        calls = CALLS[:3]
    # (fp32: the states are fp32, and a step size that differs in its last bits of double may round to another fp32 step)
    check_members(members, calls, state_tol=1e-5 if kind == "fp32" else 1e-9, h_max=0.0)


def test_refusals_before_device_work(gpu_device):
    p = crd.make_params("fhn", "torus", 32, 80.0, 20.0, 0.12, 1.25, ny=96)
    with crd.Ensemble([p, p]) as e:
        with pytest.raises(crd.CrdError) as x:
            e.integrate_adaptive(0.0, 1.0, method=crd._capi.ADAPT_RK43)
        assert x.value.status == crd._capi.EINVAL
        with pytest.raises(crd.CrdError) as x:
            e.integrate_adaptive(1.0, 0.5)
        assert x.value.status == crd._capi.EINVAL
        with pytest.raises(crd.CrdError) as x:
            e.integrate_adaptive(0.0, 1.0, rtol=-1.0)
        assert x.value.status == crd._capi.EINVAL


@pytest.mark.parametrize("name,touts,h_max", [("rk4_fhn_torus_outside", [0.5, 1.0, 1.0001, 1.5], -1.0), ("rk4_fhn_torus_outside", [0.7, 2.5], 0.0)])
def test_members_follow_the_oracle(gpu_device, name, touts, h_max):
    """Two members (the golden case and a variant in beta and tBoundary) against oracle/arkode_erk.py around the oracle's f(), as
    test_arkode_method_follows_the_restated_published_algorithm checks a lone context: the same counts, states to 1e-9."""
    from oracle import arkode_erk as ark

    meta, arr = load_golden(name)
    meta2 = dict(meta, beta=meta["beta"] * 0.9, t_boundary=0.8)
    metas = [meta, meta2]
    members = [crd_params(m) for m in metas]
    caps = [float("inf") if h_max < 0 else crd.stable_dt(q) for q in members]  # (each member is capped at its own bound)
    with crd.Ensemble(members) as e:
        for k in range(2):
            e.upload(k, arr["y0"])
        refs, t0 = [None, None], 0.0
        for c, tout in enumerate(touts):
            sts = e.integrate_adaptive(t0, tout, h_max=h_max)
            for k in range(2):
                st = sts[k]
                assert st["status"] == crd._capi.OK
                if c == 0:
                    hin = ark.ArkodeErk(oracle_problem(metas[k]), 0.0, arr["y0"], h_max=caps[k])
                    hin.evolve(touts[0])
                    assert st["h_first"] == pytest.approx(hin.steps[0], rel=1e-6), "arkHin"
                    refs[k] = ark.ArkodeErk(oracle_problem(metas[k]), 0.0, arr["y0"], h_max=caps[k], h0=st["h_first"])
                want, rst = refs[k].evolve(tout)
                assert (st["accepted"], st["rejected"]) == (rst["accepted"], rst["rejected"]), (k, tout, st, rst)
                assert st["t_internal"] == pytest.approx(rst["t_internal"], rel=1e-6)
                assert rel_err(e.download(k), want) <= 1e-9, (k, tout)
            t0 = tout


def test_members_are_independent(gpu_device):
    """At equal B, replacing one member's parameters and state -- once with a state holding a NaN -- changes no bit of any other
    member; the NaN member fails alone (the 7-failure exit) and the call says so; repeated runs are bit-identical."""
    p = crd.make_params("fhn", "torus", 61, 80.0, 20.0, 0.12, 1.25, ny=183, t_boundary=0.3)
    calls = [(0.0, 0.4), (0.4, 0.8)]

    def run(members, ys):
        res = []
        with crd.Ensemble(members) as e:
            for k, y in enumerate(ys):
                e.upload(k, y)
            for t0, tout in calls:
                sts = e.integrate_adaptive(t0, tout, h_max=-1.0)
                res.append((sts, [e.download(k) for k in range(len(members))], e.last_error()))
        return res

    members = [p, params_like(p, beta=1.1), params_like(p, diffusion=0.2), params_like(p, t_boundary=0.0)]
    ys = [start_state(q, k) for k, q in enumerate(members)]
    a = run(members, ys)
    b = run(members, ys)
    for (sa, ya, _), (sb, yb, _) in zip(a, b):
        assert sa == sb
        for u, v in zip(ya, yb):
            assert np.array_equal(u, v)
    other = params_like(p, beta=0.9, diffusion=0.3, t_boundary=1.0)
    c = run(members[:2] + [other] + members[3:], ys[:2] + [start_state(other, 7)] + ys[3:])
    nan_state = ys[2].copy()
    nan_state[5, 7, 0] = np.nan
    d = run(members, ys[:2] + [nan_state] + ys[3:])
    for res in (c, d):
        for (sa, ya, _), (sx, yx, _) in zip(a, res):
            for k in (0, 1, 3):
                assert sa[k] == sx[k]
                assert np.array_equal(ya[k], yx[k])
    sts, _, msg = d[0]
    assert sts[2]["status"] == crd._capi.ESTATE
    assert "member 2" in msg and "failed 7 times" in msg, msg
    assert all(sts[k]["status"] == crd._capi.OK and sts[k]["t"] == 0.4 for k in (0, 1, 3))
    # the call itself reports CRD_ESTATE
    L = crd._capi.lib()
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys[:2] + [nan_state] + ys[3:]):
            e.upload(k, y)
        opt = crd._capi.AdaptiveOptions()
        L.crd_adaptive_defaults(opt)
        assert L.crd_ensemble_integrate_adaptive(e.handle, 0.0, 0.4, opt, None, None) == crd._capi.ESTATE


def test_carry_over_between_calls(gpu_device):
    """A second call resumes (no arkHin; counts as a lone context that resumes); an upload restarts that member only; fixed steps
    after an adaptive call and an adaptive call after fixed steps match a lone context doing the same."""
    p = crd.make_params("fhn", "torus", 61, 80.0, 20.0, 0.12, 1.25, ny=183, t_boundary=0.3)
    members = [p, params_like(p, beta=1.1), params_like(p, diffusion=0.2)]
    ys = [start_state(q, k) for k, q in enumerate(members)]
    y_new = start_state(members[1], 11)
    dt = 0.8 * crd.stable_dt(p)
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        s1 = e.integrate_adaptive(0.0, 0.3)
        s2 = e.integrate_adaptive(0.3, 0.6)
        e.upload(1, y_new)
        s3 = e.integrate_adaptive(0.6, 0.9)
        mid = [e.download(k) for k in range(3)]
        e.step_rk4(0.9, dt, 5)
        s4 = e.integrate_adaptive(0.9 + 5 * dt, 1.2 + 5 * dt)
        end = [e.download(k) for k in range(3)]
    for k, q in enumerate(members):
        with crd.Slab(q) as s:
            s.upload(ys[k])
            w1 = s.integrate_adaptive(0.0, 0.3)
            w2 = s.integrate_adaptive(0.3, 0.6)
            if k == 1:
                s.upload(y_new)
            w3 = s.integrate_adaptive(0.6, 0.9)
            wmid = s.download()
            s.step_rk4(0.9, dt, 5)
            w4 = s.integrate_adaptive(0.9 + 5 * dt, 1.2 + 5 * dt)
            wend = s.download()
        compare(s1[k], None, w1, None, fresh=True)
        assert (s2[k]["accepted"], s2[k]["rejected"]) == (w2["accepted"], w2["rejected"])
        assert s2[k]["h_first"] == pytest.approx(w2["h_first"], rel=1e-6) and s2[k]["h_first"] != s1[k]["h_first"]
        compare(s3[k], mid[k], w3, wmid, fresh=k == 1)
        compare(s4[k], end[k], w4, wend, fresh=True)
    # the restarted member ran arkHin afresh: its first step is a fresh lone context's estimate
    with crd.Slab(members[1]) as s:
        s.upload(y_new)
        fresh = s.integrate_adaptive(0.6, 0.9)
    assert s3[1]["h_first"] == pytest.approx(fresh["h_first"], rel=1e-12)


def test_one_member_and_sixty_four(gpu_device):
    """B = 1 behaves as a context; 64 Goldbeter 100 x 400 members all finish, a spot-checked subset as lone contexts."""
    p = crd.make_params("fhn", "torus", 61, 80.0, 20.0, 0.12, 1.25, ny=183, t_boundary=0.3)
    check_members([p], CALLS[:2], h_max=0.0)
    g = crd.make_params("goldbeter", "torus", 100, 80.0, 20.0, 0.12, 0.5, ny=400, t_boundary=0.05)
    betas = np.linspace(0.2, 0.95, 64)
    members = [params_like(g, beta=float(b), diffusion=0.1 + 0.002 * k) for k, b in enumerate(betas)]
    ys = [start_state(q, k) for k, q in enumerate(members)]
    calls = [(0.0, 0.05), (0.05, 0.1)]
    with crd.Ensemble(members) as e:
        for k, y in enumerate(ys):
            e.upload(k, y)
        res = []
        for t0, tout in calls:
            sts = e.integrate_adaptive(t0, tout)
            assert all(st["status"] == crd._capi.OK and st["t"] == tout for st in sts)
            res.append((sts, {k: e.download(k) for k in (0, 17, 40, 63)}))
    for k in (0, 17, 40, 63):
        want = lone_calls(members[k], ys[k], calls)
        for c, (wst, wy) in enumerate(want):
            compare(res[c][0][k], res[c][1][k], wst, wy, fresh=c == 0)


def test_driver_adaptive_ensemble(gpu_device, tmp_path):
    """crd_run --ensemble beta=... with [Solver] adaptive = 1 in the ini: exit 0; each member's files agree with a lone adaptive run
    of its parameters to 1e-9, and the printed per-member counts with the lone runs'."""
    ini = tmp_path / "adaptive.ini"
    ini.write_text(open(SMALL_INI).read().replace("[Solver]\n", "[Solver]\nadaptive = 1\n"))
    ens_dir = tmp_path / "ens"
    ens_dir.mkdir()
    r = subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus", "--ensemble", "beta=1.25,1.0", "--ensemble", "tBoundary=0.4,0.0",
                        "--outdir", str(ens_dir), str(ini)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    counts = {int(m.group(1)): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"member (\d+): steps = (\d+) \(\+(\d+) rejected\)", r.stdout)}
    assert sorted(counts) == [0, 1], r.stdout
    for k, (beta, tb) in enumerate([(1.25, 0.4), (1.0, 0.0)]):
        text = open(SMALL_INI).read().replace("[Solver]\n", "[Solver]\nadaptive = 1\n").replace("beta = 1.25", "beta = %r" % beta).replace("tBoundary = 0.4", "tBoundary = %r" % tb)
        lone_ini = tmp_path / ("lone_%d.ini" % k)
        lone_ini.write_text(text)
        lone_dir = tmp_path / ("lone_%d" % k)
        lone_dir.mkdir()
        r1 = subprocess.run([os.path.join(BIN, "crd_run"), "--model", "fhn", "--surface", "torus", "--outdir", str(lone_dir), str(lone_ini)], capture_output=True,
                            text=True, timeout=300)
        assert r1.returncode == 0, r1.stderr
        m = re.search(r"steps = (\d+) \(\+(\d+) rejected\)", r1.stdout)
        assert m and (int(m.group(1)), int(m.group(2))) == counts[k], (r1.stdout, counts)
        names = sorted(f for f in os.listdir(ens_dir / ("member_%d" % k)) if f.endswith(".txt"))
        assert names
        for f in names:
            a, b = np.loadtxt(ens_dir / ("member_%d" % k) / f, ndmin=1), np.loadtxt(lone_dir / f, ndmin=1)
            assert a.shape == b.shape and rel_err(a, b) <= 1e-9, f
