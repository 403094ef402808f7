"""The split right-hand side f = f_D + f_R and J(t, y) v on the device (crd_rhs_part_* / crd_jtimes_*, Slab.rhs_part / Slab.jtimes).

Every part and every J v form is held per point and per field to the rounding bound of tests/jacobian_reference.py against the
long-double reference (fp32: float64 on the widened vectors); the identities the header promises are held bit for bit
(np.array_equal); slab cuts and the RCCL ring to self reproduce the single slab bit for bit; the device's Jacobian gives the
reference's two stated stability results; and one linearly implicit Euler step at 20x the explicit bound shows what it is for.

Worst err / bound measured on MI355X (printed with -s as "BOUND ..."): see DESIGN.md section 2.
"""
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
import jacobian_reference as jr
from conftest import GOLDEN
from oracle import error_bounds as eb

pytestmark = pytest.mark.gpu

CONFIG_IDS = [c[0] for c in jr.CONFIGS]
T_ON, T_AT, T_OFF = jr.TIMES  # absorbing rows on; at tBoundary (strict <: off); off


def contexts(config, nx, ny, precision, **kw):
    p, op = jr.case(config, nx, ny, precision, **kw)
    return p, op, jr.start_state(p, 1), jr.direction(p, 2)


def check(case, got, bounded):
    w = eb.check(case, got, bounded)
    print("BOUND " + eb.describe(case, w))
    return max(w["u"][0], w["v"][0])


# ---- bound checks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config", jr.CONFIGS, ids=CONFIG_IDS)
def test_parts_and_jtimes_within_the_bound(gpu_device, config, precision):
    worst = {"part": 0.0, "jtimes": 0.0}
    for nx, ny in jr.GRIDS:
        p, op, y, v = contexts(config, nx, ny, precision)
        with crd.Slab(p) as slab:
            for t in jr.TIMES:
                for part in jr.PARTS:
                    case = "%s %s %dx%d t=%g %s" % (precision, config[0], nx, ny, t, part)
                    worst["part"] = max(worst["part"], check("rhs_part " + case, slab.rhs_part(t, y, part), jr.part_bound(op, t, y, precision, part)))
                    worst["jtimes"] = max(worst["jtimes"], check("jtimes " + case, slab.jtimes(t, y, v, part), jr.jtimes_bound(op, t, y, v, precision, part)))
    print("BOUND WORST %s %s: rhs_part %.3g, jtimes %.3g" % (precision, config[0], worst["part"], worst["jtimes"]))


# ---- bit identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config", jr.CONFIGS, ids=CONFIG_IDS)
def test_bit_identities(gpu_device, config, precision):
    just_diffusion = config[4].get("just_diffusion", 0)
    for nx, ny in jr.GRIDS:
        p, op, y, v = contexts(config, nx, ny, precision)
        other_y = jr.start_state(p, 9)
        uniform = np.empty_like(y)
        uniform[..., 0], uniform[..., 1] = 0.7312, 1.25
        with crd.Slab(p) as slab:
            for t in jr.TIMES:
                case = (config[0], precision, nx, ny, t)
                f = slab.f(t, y)
                assert np.array_equal(slab.rhs_part(t, y, "full"), f), case
                f_d, f_r = slab.rhs_part(t, y, "diffusion"), slab.rhs_part(t, y, "reaction")
                assert not f_d[..., 1].any() and not np.signbit(f_d[..., 1]).any(), case  # dv = +0.0
                if just_diffusion:
                    assert not f_r.any() and np.array_equal(f_d, f), case
                # J_D v = f_D(v), whatever y
                jd = slab.jtimes(t, y, v, "diffusion")
                assert np.array_equal(jd, slab.rhs_part(t, v, "diffusion")) and np.array_equal(jd, slab.jtimes(t, other_y, v, "diffusion")), case
                # J is linear in v: scaling by a power of two commutes with every rounding
                for part in jr.PARTS:
                    jv = slab.jtimes(t, y, v, part)
                    for k in (3, -3):
                        scale = y.dtype.type(2.0 ** k)
                        assert np.array_equal(slab.jtimes(t, y, scale * v, part), scale * jv), case + (part, k)
                assert not slab.jtimes(t, y, uniform, "diffusion").any(), case  # a uniform direction diffuses to exactly zero
                assert np.array_equal(slab.rhs_part(t, uniform, "reaction"), slab.rhs_part(t, uniform, "full")), case  # ... and a uniform state


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_diffusion_part_is_the_diffusion_only_context(gpu_device, precision):
    """DIFFUSION of an FHN context has the bits of f of a Goldbeter just_diffusion context of the same geometry and diffusion.  That
    context has no absorbing rows (the reference skips them with the kinetics), so before tBoundary rows 0 and ny - 1 are left out."""
    for surface, fhn in (("torus", jr.CONFIGS[0]), ("flat", jr.CONFIGS[1])):
        only = ("just-diffusion-" + surface, "goldbeter", surface, 0.4, dict(just_diffusion=1))
        for nx, ny in jr.GRIDS:
            p, _, y, _ = contexts(fhn, nx, ny, precision)
            q, _ = jr.case(only, nx, ny, precision)
            with crd.Slab(p) as a, crd.Slab(q) as b:
                for t in jr.TIMES:
                    got, want = a.rhs_part(t, y, "diffusion"), b.f(t, y)
                    rows = slice(1, ny - 1) if t < jr.T_BOUNDARY else slice(None)
                    assert np.array_equal(got[rows], want[rows]), (surface, nx, ny, t)
                    assert np.array_equal(b.rhs_part(t, y, "diffusion"), want) and np.array_equal(b.jtimes(t, y, y, "full"), want)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config", jr.CONFIGS[:3], ids=CONFIG_IDS[:3])
def test_absorbing_rows(gpu_device, config, precision):
    """Global rows 0 and ny - 1 are zero in every part of f and zero rows of every part of J while t < tBoundary -- strictly: not at
    t == tBoundary -- and in a group only on the slab that owns them: the slabs' own first and last rows are not zero."""
    nx, ny = 130, 33
    p, op, y, v = contexts(config, nx, ny, precision)
    with crd.Slab(p) as slab, crd.LocalGroup(p, 3) as group:
        inner = sorted({r for s in group.slabs for r in (s.js, s.je)} - {0, ny - 1})
        assert len(inner) == 4
        for target in (slab, group):
            for part in jr.PARTS:
                for t in (T_ON, T_AT):
                    for out in (target.rhs_part(t, y, part), target.jtimes(t, y, v, part)):
                        edge = out[[0, ny - 1]]
                        if t < jr.T_BOUNDARY:
                            assert not edge.any(), (config[0], part, t)
                        else:
                            assert edge[..., 0].any(axis=1).all(), (config[0], part, t)
                        assert out[inner][..., 0].any(axis=1).all(), (config[0], part, t)


def test_just_diffusion_has_no_absorbing_rows(gpu_device):
    """A Goldbeter just_diffusion context's f has no absorbing rows; its parts and its J follow f."""
    p, op, y, v = contexts(jr.CONFIGS[3], 130, 33, "f64")
    with crd.Slab(p) as slab:
        f = slab.f(T_ON, y)
        assert f[[0, 32], :, 0].any(axis=1).all()
        assert np.array_equal(slab.rhs_part(T_ON, y, "diffusion"), f) and np.array_equal(slab.rhs_part(T_ON, y, "full"), f)
        assert np.array_equal(slab.jtimes(T_ON, y, y, "diffusion"), f) and not slab.jtimes(T_ON, y, v, "reaction").any()


# ---- slabs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config", jr.CONFIGS, ids=CONFIG_IDS)
def test_slab_cuts_and_self_ring_reproduce_the_single_slab(gpu_device, config, precision):
    """On 130 x 33: a 3-slab LOCAL group on the one device, and the RCCL ring to self, give the single slab's bits in every part and
    every J v form."""
    p, op, y, v = contexts(config, 130, 33, precision)
    with crd.Slab(p) as slab, crd.LocalGroup(p, 3) as group, crd.Slab(p) as ring:
        ring.init_rccl(crd.rccl_unique_id())
        assert ring.comm_info()[0] == "rccl"
        for t in (T_ON, T_OFF):
            for part in jr.PARTS:
                want_f, want_j = slab.rhs_part(t, y, part), slab.jtimes(t, y, v, part)
                for name, other in (("group", group), ("ring", ring)):
                    assert np.array_equal(other.rhs_part(t, y, part), want_f), (name, config[0], part, t)
                    assert np.array_equal(other.jtimes(t, y, v, part), want_j), (name, config[0], part, t)


def test_refusals(gpu_device):
    """A bad part is CRD_EINVAL; LOCAL contexts go through the group entry points for the parts that exchange, and REACTION -- not
    collective -- works on a lone context of a group; theta-blocks are refused with CRD_ESTATE."""
    p, op, y, v = contexts(jr.CONFIGS[0], 130, 33, "f64")
    K = crd._capi
    with crd.Slab(p) as slab:
        for call in (lambda: slab.rhs_part(0.0, y, 3), lambda: slab.jtimes(0.0, y, v, -1)):
            with pytest.raises(K.CrdError) as e:
                call()
            assert e.value.status == K.EINVAL
        whole_r = slab.rhs_part(T_OFF, y, "reaction")
    with crd.LocalGroup(p, 3) as group:
        s = group.slabs[1]
        rows = slice(s.js, s.je + 1)
        for part in ("full", "diffusion"):
            with pytest.raises(K.CrdError) as e:
                s.rhs_part(0.0, y[rows], part)
            assert e.value.status == K.ESTATE and "crd_group_rhs_part" in str(e.value)
            with pytest.raises(K.CrdError) as e:
                s.jtimes(0.0, y[rows], v[rows], part)
            assert e.value.status == K.ESTATE and "crd_group_jtimes" in str(e.value)
        assert np.array_equal(s.rhs_part(T_OFF, y[rows], "reaction"), whole_r[rows])
    with crd.LocalGroup(p, 4, blocks=(2, 2)) as blocks:
        for call in (lambda: blocks.rhs_part(0.0, y, "diffusion"), lambda: blocks.jtimes(0.0, y, v, "reaction")):
            with pytest.raises(K.CrdError) as e:
                call()
            assert e.value.status == K.ESTATE


# ---- known answers ----------------------------------------------------------------------------------------------------------------
def reaction_block(model, beta):
    """The 2x2 block of the kinetics at the uniform steady state, read off the device: J_R applied to uniform (1, 0) and (0, 1)."""
    p = crd.make_params(model, "torus", 61, 80.0, 20.0, 0.12, beta, ny=9)
    s0, s1 = crd.steady_state(model, beta)
    y = np.empty((9, 61, 2))
    y[..., 0], y[..., 1] = s0, s1
    cols = []
    with crd.Slab(p) as slab:
        for e in ((1.0, 0.0), (0.0, 1.0)):
            v = np.empty_like(y)
            v[..., 0], v[..., 1] = e
            jv = slab.jtimes(1.0, y, v, "reaction")
            assert (jv == jv[4, 30]).all()  # pointwise: the same block everywhere
            cols.append(jv[4, 30])
    return np.array(cols).T


def test_known_stability_results(gpu_device):
    """The reference's two stated results, from the device's Jacobian.  FHN: the steady state loses stability where the block's trace
    changes sign, |beta| = 1.  Goldbeter: oscillations inside beta = 0.28895 ... 0.77427."""
    assert np.trace(reaction_block("fhn", 0.9)) > 0 > np.trace(reaction_block("fhn", 1.1))
    growth = {beta: np.linalg.eigvals(reaction_block("goldbeter", beta)).real.max() for beta in (0.2, 0.5, 0.9)}
    assert growth[0.5] > 0 and growth[0.2] < 0 and growth[0.9] < 0, growth


# ---- what it is for ---------------------------------------------------------------------------------------------------------------
def solve(matvec, b, rtol):
    """GMRES (scipy) where it imports, else a plain BiCGStab; returns x."""
    n = b.size
    try:
        from scipy.sparse.linalg import LinearOperator, gmres
    except ImportError:
        x, r = np.zeros(n), b.copy()
        r0, rho, alpha, omega, vv, pp = r.copy(), 1.0, 1.0, 1.0, np.zeros(n), np.zeros(n)
        for _ in range(2000):
            rho1 = r0 @ r
            pp = r + (rho1 / rho) * (alpha / omega) * (pp - omega * vv)
            vv = matvec(pp)
            alpha = rho1 / (r0 @ vv)
            s = r - alpha * vv
            t = matvec(s)
            omega = (t @ s) / (t @ t)
            x, r, rho = x + alpha * pp + omega * s, s - omega * t, rho1
            if np.linalg.norm(r) <= rtol * np.linalg.norm(b):
                break
        return x
    x, info = gmres(LinearOperator((n, n), matvec=matvec, dtype=np.float64), b, rtol=rtol, atol=0.0, restart=400, maxiter=5)
    assert info == 0, info
    return x


def test_linearly_implicit_euler_step(gpu_device):
    """One linearly implicit Euler step of FHN flat 64 x 16 at h = 20 x crd_stable_dt: (I - h J_D) y1 = y0 + h f_R(y0), solved by a Krylov
    method whose matvec is v - h jtimes(DIFFUSION).  Relative tolerance 1e-10: a setting of the solver.  The residual of y1 under the
    long-double operator is within that tolerance plus the rounding of what the solver was given: per point h x (the bound on J_D y1
    + the bound on f_R(y0)) + 2 u (|y1| + h |J_D y1|) + 2 u (|y0| + h |f_R|) for the two host-side combinations.  Fifty explicit RK4
    steps of that size overflow; the implicit step stays finite."""
    p, op = jr.case(jr.CONFIGS[1], 64, 16, "f64", t_boundary=0.0)
    y0 = jr.start_state(p, 1)
    h, rtol, u = 20.0 * crd.stable_dt(p), 1e-10, eb.UNIT["f64"]
    shape = y0.shape
    with crd.Slab(p) as slab:
        f_r = slab.rhs_part(0.0, y0, "reaction")
        b = y0 + h * f_r
        y1 = solve(lambda x: x - h * slab.jtimes(0.0, y0, x.reshape(shape), "diffusion").ravel(), b.ravel(), rtol).reshape(shape)
        slab.upload(y0)
        slab.step_rk4(0.0, h, 50)
        assert not np.isfinite(slab.download()).all()
    assert np.isfinite(y1).all()
    jd, jbu, jbv = jr.jtimes_bound(op, 0.0, y0, y1, "f64", jr.DIFFUSION)
    fr, rbu, rbv = jr.part_bound(op, 0.0, y0, "f64", jr.REACTION)
    L = np.longdouble
    residual = (y1.astype(L) - L(h) * jd) - (y0.astype(L) + L(h) * fr)
    rounding = h * (np.stack([jbu, jbv], -1) + np.stack([rbu, rbv], -1)) + 2 * u * (np.abs(y1) + h * np.abs(jd.astype(np.float64)) + np.abs(y0) + h * np.abs(f_r))
    res, allowed = float(np.linalg.norm(residual.astype(np.float64))), rtol * float(np.linalg.norm(b)) + float(np.linalg.norm(rounding))
    print("BOUND implicit Euler: h = %.3g = 20 x stable dt, residual %.3g, allowed %.3g (solver %.3g + rounding %.3g)" % (
        h, res, allowed, rtol * np.linalg.norm(b), np.linalg.norm(rounding)))
    assert res <= allowed
    assert np.abs(y1 - y0).max() > 1e-3  # the step went somewhere


# ---- the shim ---------------------------------------------------------------------------------------------------------------------
def test_imex_shim(gpu_device, tmp_path):
    """tests/native/shim_imex_selftest.c drives crd_arkode_fe / _fi / _jtimes_fi / _jtimes on host vectors through SUNDIALS-typed function
    pointers: jtimes_fi(v) is fi(v) bit for bit (checked there), and fe + fi is within the sum of the parts' and f's bounds of f."""
    import os

    exe, dump = tmp_path / "shim_imex", tmp_path / "parts.bin"
    build = subprocess.run(jr.shim_build_command(exe), capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    r = subprocess.run([str(exe), os.path.join(GOLDEN, "ini", "small_run.ini"), str(dump)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "shim imex selftest" in r.stdout, (r.returncode, r.stdout, r.stderr)
    nx, ny, t_boundary = 16, 40, 0.4  # tests/golden/ini/small_run.ini
    op = jr.problem_of("fhn", "torus", nx, ny, 1.25, t_boundary=t_boundary)
    data = np.fromfile(dump, dtype=np.float64).reshape(2, 4, ny, nx, 2)
    for k, t in enumerate((0.5 * t_boundary, 2.0 * t_boundary + 1.0)):
        y, f, fe, fi = data[k]
        full = eb.rhs_bound(op, t, y, "f64")
        part_r, part_d = jr.part_bound(op, t, y, "f64", jr.REACTION), jr.part_bound(op, t, y, "f64", jr.DIFFUSION)
        eb.check("shim f t=%g" % t, f, full)
        eb.check("shim fe t=%g" % t, fe, part_r)
        eb.check("shim fi t=%g" % t, fi, part_d)
        gap = np.abs((fe.astype(np.longdouble) + fi) - f).astype(np.float64)
        for field in (0, 1):
            assert np.all(gap[..., field] <= full[1 + field] + part_r[1 + field] + part_d[1 + field]), (t, field)
        if t < t_boundary:
            assert not fe[[0, ny - 1]].any() and not fi[[0, ny - 1]].any()
