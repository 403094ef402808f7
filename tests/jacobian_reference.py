"""Reference and per-point rounding-error bounds for the split right-hand side f = f_D + f_R and for J(t, y) v
(crd_rhs_part_* / crd_jtimes_*, crdmodel_amd/csrc/crd_jacobian.h).  TEST INFRASTRUCTURE ONLY.

Reference
---------
oracle/crd_oracle_np.py's diffusion operator and the kinetics' formulas, evaluated in error_bounds.reference_dtype(precision):
np.longdouble for the fp64 kernels, float64 on the exactly widened fp32 vectors for the fp32 kernels.  The operator is linear, so
J_D v is the operator on v's activator; the reaction block is analytic (tests/test_jacobian_host.py pins the Goldbeter partials to
sympy.diff and the FHN block to a central difference of the numpy right-hand side).

Bound on a part of f
--------------------
error_bounds.rhs_bound's form, K u S + rho |w|, with S restricted to the part's terms:

    diffusion  S_u = |cE gE| + |cWn gW| + |cP| (|uN| + 2 |uC| + |uS|),  S_v = 0 (dv is exactly +0)
    reaction   FHN        S_u = |v| + 3 |u| + |u|^3,                            S_v = eps (|u| + |b|)
               Goldbeter  S_u = |v2| + |v3| + kf |v| + k |u| + |v0 + v1 b|,     S_v = |v2| + |v3| + kf |v|,  + rho |v2 - v3| on both
               Goldbeter with just_diffusion: exact zeros

K = error_bounds.K.  Absorbing rows while t < tBoundary are exact zeros (not for just_diffusion, whose f has none).

Bound on J v
------------
With d = (du, dv) the direction and a the 2x2 block at y,

    |Jv_kernel - Jv_ref|  <=  K_J u S + (K_A u + M rho) A            per point and per field

    u field  S = |cE gE| + |cWn gW| + |cP| (|dN| + 2 |dC| + |dS|) + A_u      (gE, gW, dN, dC, dS: of d's activator; the first
                                                                            line is absent from the reaction part, A_u from the
                                                                            diffusion part)
             A_u = |a11| |du| + |a12| |dv|
    v field  S = A_v = |a21| |du| + |a22| |dv|

where |a_ij| is the sum of the magnitudes of the entry's TERMS, because they cancel: FHN |a11| = 3 + 3 u^2; Goldbeter
w_z = wz2 - wz3 (the Hill terms' partials, of opposite sign), |a11| = |wz2| + |wz3| + k, |a21| = |wz2| + |wz3|,
|a12| = |a22| = |w_y| + kf.

K_J, derived from jac_point's operation sequence as error_bounds derives K = 8: count the roundings a term passes through on its
way into the result.  FULL, u field: r0 = a12 dv (1; FHN's -dv: 0); d2y = fma(-2, dC, dN) + dS (2); fma(cP, d2y, r0),
fma(cE, gE, .), fma(cWn, gW, .), fma(a11, du, .) (1 each).  The phi term passes d2y's two, a rounded table and four fused
multiply-adds: 7.  The east term passes its difference's rounding (a first difference of arbitrary values is correct to half an
ulp, not exact), a rounded table and three fused multiply-adds: 5; the west term 4; a12 dv 5; a11 du 1.  v field:
fma(a21, du, a22 dv): 2.  The largest count is 7, K_J = 8 leaves one spare -- the same constant as K, for the same chain.

K_A and M, the roundings and reciprocals inside a Goldbeter block entry (jac_block).  z2 = z z carries 1 u, y2 = y y 1, z4 = z2 z2 3.
The denominators are sums of positive terms: K2^2 + z2 carries 2 u, KR^2 + y2 2, fma(z2, z2, ka4) 4 (z2 twice, the rounded ka4 or
the fma, each on a positive term).  A reciprocal adds rho: rA rho + 2 u, rC rho + 2 u, rD rho + 4 u.
    t2 = (65 rA) rA                          2 rho + 6 u
    q3 = ((y2 rC) (z2 rD)) rD                (rho + 4 u) + (rho + 6 u) + 1 + (rho + 4 u) + 1 = 3 rho + 16 u
    c4 q3, c4 = (-2 VM3) ka4 in the device precision (2 u), inside fma(c4, q3, t2) (1 u): 3 rho + 19 u
    w_z = (2 z) (.)                          + 1: 3 rho + 20 u on the wz3 term, 2 rho + 8 u on wz2; a11 = -w_z - k: + 1
    w_y = (-4000 y) ((z4 rD) (rC rC))        1 + (3 + rho + 4 + 1) + (2 rho + 4 + 1) + 1 + 1 = 3 rho + 16 u; a22 = w_y - kf: + 1
The largest count is 21 u and 3 rho: K_A = 24 leaves three spare, M = 3.  FHN: a11 = fma(-3 u, u, 3) rounds twice, the other
entries are constants (eps rounded to the device precision: 1): K_A_FHN = 2, M = 0.

The reference's own error (2^-64 or 2^-53 of the same terms) is ignored, as in error_bounds.
"""
import os

import numpy as np

from oracle import crd_oracle as co
from oracle import crd_oracle_np as cn
from oracle import error_bounds as eb
from oracle.error_bounds import RHO, UNIT

FULL, DIFFUSION, REACTION = "full", "diffusion", "reaction"
PARTS = (FULL, DIFFUSION, REACTION)
K_J = 8.0
K_A = 24.0
M_RCP = 3.0
K_A_FHN = 2.0
KF, KK, V0, V1, VM2, VM3, K2, KR, KA, EPS = eb.KF, eb.KK, eb.V0, eb.V1, eb.VM2, eb.VM3, eb.K2, eb.KR, eb.KA, eb.EPS


def _zero_rows(P, t, rows):
    return P.zero_rows(t, rows, 0)


def _beta(P, dtype, rows):
    return cn.beta_rows(P.g, P.kw["beta"], P.kw["vary_beta"], P.kw["beta_min"], P.kw["beta_max"], dtype, 0, rows)[:, None]


def goldbeter_partials(z, y, ka4=None):
    """(wz2, wz3, w_y) of w = v2(z) - v3(z, y) in the dtype of z: w_z = wz2 - wz3."""
    c = z.dtype.type
    ka4 = c(KA ** 4.0) if ka4 is None else ka4  # the fp64 constant, as crd_oracle_np and the host form it
    z2, y2 = z * z, y * y
    z4 = z2 * z2
    wz2 = c(VM2) * 2 * z * c(K2 * K2) / (c(K2 * K2) + z2) ** 2
    wz3 = c(VM3) * y2 / (c(KR * KR) + y2) * 4 * z * z2 * ka4 / (ka4 + z4) ** 2
    w_y = -c(VM3) * z4 / (ka4 + z4) * 2 * y * c(KR * KR) / (c(KR * KR) + y2) ** 2
    return wz2, wz3, w_y


def block(P, u, v):
    """((a11, a12, a21, a22), (|a11|, |a12|, |a21|, |a22|)): the reaction block at (u, v) in their dtype, and the entries' term
    magnitudes in float64 (module docstring)."""
    c = u.dtype.type
    one, zero = np.ones_like(u), np.zeros_like(u)
    f = lambda x: np.abs(np.asarray(x, dtype=np.float64))
    if P.diffusion_only:
        return (zero, zero, zero, zero), (f(zero),) * 4
    if P.model == "fhn":
        return (3 - 3 * u * u, -one, c(EPS) * one, zero), (3 + 3 * f(u) ** 2, f(one), EPS * f(one), f(zero))
    wz2, wz3, w_y = goldbeter_partials(u, v)
    w_z = wz2 - wz3
    mz = f(wz2) + f(wz3)
    return (-w_z - c(KK), -w_y + c(KF), w_z, w_y - c(KF)), (mz + KK, f(w_y) + KF, mz, f(w_y) + KF)


def _reaction(P, u, v):
    c = u.dtype.type
    if P.diffusion_only:
        return np.zeros_like(u), np.zeros_like(v)
    b = _beta(P, c, u.shape[0])
    if P.model == "fhn":
        return 3 * u - u * u * u - v, c(EPS) * (u + b)
    z2, y2 = u * u, v * v
    z4 = z2 * z2
    v2 = c(VM2) * z2 / (c(K2 * K2) + z2)
    v3 = c(VM3) * y2 * z4 / ((c(KR * KR) + y2) * (c(KA ** 4.0) + z4))
    return c(V0) + c(V1) * b - v2 + v3 + c(KF) * v - c(KK) * u, v2 - v3 - c(KF) * v


def _diffusion_sizes(P, u):
    u = np.asarray(u, dtype=np.float64)
    uW, uE = np.roll(u, 1, axis=1), np.roll(u, -1, axis=1)
    uS, uN = np.roll(u, 1, axis=0), np.roll(u, -1, axis=0)
    cE, cWn, cP = P.cE[None, :], P.cWn[None, :], P.cP[None, :]
    return np.abs(cE * (uE - u)) + np.abs(cWn * (u - uW)) + np.abs(cP) * (np.abs(uN) + 2 * np.abs(u) + np.abs(uS))


def _split(y, dtype):
    y = np.asarray(y)
    assert y.ndim == 3 and y.shape[2] == 2, y.shape
    return y[..., 0].astype(dtype), y[..., 1].astype(dtype)


def part_bound(op, t, y, precision, part):
    """(ref, bound_u, bound_v) of one part of f(t, y) on the whole grid, as error_bounds.rhs_bound's."""
    P = eb._Problem(op)
    rd = eb.reference_dtype(precision)
    u, v = _split(y, rd)
    un = UNIT[precision]
    du, dv = np.zeros_like(u), np.zeros_like(v)
    bu, bv = np.zeros(u.shape), np.zeros(u.shape)
    if part in (FULL, DIFFUSION):
        du = du + cn.diffusion(P.surface, P.g, P.D, u, rd)
        bu = bu + eb.K * un * _diffusion_sizes(P, u)
    if part in (FULL, REACTION) and not P.diffusion_only:
        ru, rv = _reaction(P, u, v)
        du, dv = du + ru, dv + rv
        u64, v64 = u.astype(np.float64), v.astype(np.float64)
        b = _beta(P, np.float64, u.shape[0])
        if P.model == "fhn":
            Su, Sv, w = np.abs(v64) + 3 * np.abs(u64) + np.abs(u64) ** 3, EPS * (np.abs(u64) + np.abs(b)), 0.0
        else:
            z2, y2 = u64 * u64, v64 * v64
            v2 = VM2 * z2 / (K2 * K2 + z2)
            v3 = VM3 * y2 * z2 * z2 / ((KR * KR + y2) * (KA ** 4.0 + z2 * z2))
            Sv = np.abs(v2) + np.abs(v3) + KF * np.abs(v64)
            Su, w = Sv + KK * np.abs(u64) + np.abs(V0 + V1 * b), np.abs(v2 - v3)
        bu = bu + eb.K * un * Su + RHO[precision] * w
        bv = bv + eb.K * un * Sv + RHO[precision] * w
    zero = _zero_rows(P, t, u.shape[0])
    for a in (du, dv, bu, bv):
        a[zero] = 0.0
    return np.stack([du, dv], axis=-1), bu, bv


def jtimes_bound(op, t, y, v, precision, part):
    """(ref, bound_u, bound_v) of J_part(t, y) v on the whole grid (module docstring)."""
    P = eb._Problem(op)
    rd = eb.reference_dtype(precision)
    yu, yv = _split(y, rd)
    du, dv = _split(v, rd)
    un = UNIT[precision]
    ju, jv = np.zeros_like(du), np.zeros_like(dv)
    Su, Au, Av = np.zeros(du.shape), np.zeros(du.shape), np.zeros(du.shape)
    if part in (FULL, DIFFUSION):
        ju = ju + cn.diffusion(P.surface, P.g, P.D, du, rd)
        Su = Su + _diffusion_sizes(P, du)
    if part in (FULL, REACTION):
        (a11, a12, a21, a22), (m11, m12, m21, m22) = block(P, yu, yv)
        ju = ju + a11 * du + a12 * dv
        jv = jv + a21 * du + a22 * dv
        adu, adv = np.abs(du.astype(np.float64)), np.abs(dv.astype(np.float64))
        Au, Av = m11 * adu + m12 * adv, m21 * adu + m22 * adv
    entry = K_A_FHN * un if P.model == "fhn" else K_A * un + M_RCP * RHO[precision]
    bu = K_J * un * (Su + Au) + entry * Au
    bv = K_J * un * Av + entry * Av
    zero = _zero_rows(P, t, du.shape[0])
    for a in (ju, jv, bu, bv):
        a[zero] = 0.0
    return np.stack([ju, jv], axis=-1), bu, bv


# ---- the kernels' own order in a working precision (the bound is honest: these stay inside it; and sharp: mutants do not) ---------
def _fma(R):
    """Fused multiply-add of the precision R, emulated one size up (exact product for float32; 64-bit significand for float64)."""
    wide = np.float64 if R == np.float32 else np.longdouble
    return lambda a, b, c: (np.asarray(a, wide) * np.asarray(b, wide) + np.asarray(c, wide)).astype(R)


def _reciprocal(x):
    """The device's 1/x: an estimate (here the correctly rounded value) refined by one Newton step."""
    fma = _fma(x.dtype.type)
    r = (1 / x.astype(np.longdouble)).astype(x.dtype)
    return fma(r, fma(-x, r, x.dtype.type(1)), r)


def _tables(P, R, rows):
    b = _beta(P, np.float64, rows)
    rowp = cn.EPSILON * b if P.model == "fhn" else (np.longdouble(7.3) * b.astype(np.longdouble) + 1).astype(np.float64)  # host: fma(v1, b, v0)
    return tuple(c.astype(R)[None, :] for c in (P.cE, P.cWn, P.cP)) + (rowp.astype(R),)


def _stencil(x, R, mutant):
    """(gW, gE, d2y) of the activator plane x as the kernels form them; mutant "seam" / "nowrap" plants a wrong neighbour."""
    fma = _fma(R)
    xW, xE = np.roll(x, 1, axis=1), np.roll(x, -1, axis=1)
    xS, xN = np.roll(x, 1, axis=0), np.roll(x, -1, axis=0)
    if mutant == "seam":
        xW[:, 0] = x[:, -2]  # column 0 takes its west neighbour one column off the seam
    if mutant == "nowrap":
        xS[0] = x[0]  # row 0's southern neighbour is not the last row
    return x - xW, xE - x, fma(R(-2.0), x, xN) + xS


def kernel_order_part(op, t, y, R, part):
    """crd_jacobian.h's rhs_point_diffusion / rhs_point_reaction in precision R (FULL: tests/test_error_bounds.kernel_order_rhs)."""
    assert part in (DIFFUSION, REACTION)
    fma = _fma(R)
    P = eb._Problem(op)
    u, v = y[..., 0].astype(R), y[..., 1].astype(R)
    cE, cWn, cP, rowp = _tables(P, R, u.shape[0])
    if part == DIFFUSION:
        gW, gE, d2y = _stencil(u, R, None)
        du, dv = fma(cWn, gW, fma(cE, gE, cP * d2y)), np.zeros_like(v)
    elif P.diffusion_only:
        du, dv = np.zeros_like(u), np.zeros_like(v)
    elif P.model == "fhn":
        du, dv = fma(u, fma(-u, u, R(3.0)), -v), fma(R(EPS), u, rowp)
    else:
        z2 = u * u
        z4, y2 = z2 * z2, v * v
        dA = R(1.0) + z2
        dB = fma(R(1.0 / 500.0), y2, R(4.0 / 500.0)) * fma(z2, z2, R(0.9 ** 4))
        w = fma(R(65.0), z2 * dB, -((y2 * z4) * dA)) * _reciprocal(dA * dB)
        dv = fma(R(-1.0), v, w)
        du = fma(R(-10.0), u, rowp - dv)
    zero = _zero_rows(P, t, u.shape[0])
    du[zero] = 0.0
    dv[zero] = 0.0
    return np.stack([du, dv], axis=-1)


def kernel_order_jtimes(op, t, y, v, R, part, mutant=None):
    """crd_jacobian.h's jac_point in precision R.  mutant: "seam", "nowrap" (a wrong stencil neighbour), "a11" (3 - u^2 for
    3 - 3 u^2), "transpose" (the off-diagonal entries exchanged)."""
    fma = _fma(R)
    P = eb._Problem(op)
    yu, yv = y[..., 0].astype(R), y[..., 1].astype(R)
    du, dv = v[..., 0].astype(R), v[..., 1].astype(R)
    cE, cWn, cP, _ = _tables(P, R, du.shape[0])
    gW, gE, d2y = _stencil(du, R, mutant)
    if part == DIFFUSION or (P.diffusion_only and part == FULL):
        ju, jv = fma(cWn, gW, fma(cE, gE, cP * d2y)), np.zeros_like(dv)
    elif P.diffusion_only:
        ju, jv = np.zeros_like(du), np.zeros_like(dv)
    else:
        if P.model == "fhn":
            a11 = fma((R(-1.0) if mutant == "a11" else R(-3.0)) * yu, yu, R(3.0))
            a12, a21, a22 = np.full_like(yu, -1.0), np.full_like(yu, R(EPS)), np.zeros_like(yu)
        else:
            ka4 = R(0.9 ** 4)
            z2 = yu * yu
            z4, y2 = z2 * z2, yv * yv
            rA, rC, rD = _reciprocal(R(1.0) + z2), _reciprocal(R(4.0) + y2), _reciprocal(fma(z2, z2, ka4))
            t2 = (R(65.0) * rA) * rA
            q3 = ((y2 * rC) * (z2 * rD)) * rD
            w_z = (R(2.0) * yu) * fma(R(-1000.0) * ka4, q3, t2)
            w_y = (R(-4000.0) * yv) * ((z4 * rD) * (rC * rC))
            a11, a12, a21, a22 = -w_z - R(10.0), R(1.0) - w_y, w_z, w_y - R(1.0)
        if mutant == "transpose":
            a12, a21 = a21, a12
        r = a12 * dv
        if part == FULL:
            r = fma(cWn, gW, fma(cE, gE, fma(cP, d2y, r)))
        ju = fma(a11, du, r)
        jv = fma(a21, du, a22 * dv)
    zero = _zero_rows(P, t, du.shape[0])
    ju[zero] = 0.0
    jv[zero] = 0.0
    return np.stack([ju, jv], axis=-1)


def problem_of(model, surface, nx, ny, beta, L=80.0, W=20.0, D=0.12, **kw):
    return co.make_problem({"fhn": co.FHN, "goldbeter": co.GOLDBETER}[model], {"torus": co.TORUS, "flat": co.FLAT}[surface], nx, L, W, D, beta, ny=ny, **kw)


# ---- the cases tests/test_jacobian_host.py and tests/test_gpu_jacobian.py share ---------------------------------------------------
GRIDS = [(61, 9), (64, 16), (130, 33)]  # (nx, ny): ragged and under one tile; exactly one tile; two tiles and a ragged third, rows not a multiple of 16
T_BOUNDARY = 0.5
TIMES = (0.25, 0.5, 0.75)  # before, at and after tBoundary
# (label, model, surface, beta, keyword arguments of make_params / make_problem)
CONFIGS = [
    ("fhn-torus-varybeta", "fhn", "torus", 1.25, dict(vary_beta=1, beta_min=0.3, beta_max=1.4)),
    ("fhn-flat", "fhn", "flat", 1.25, {}),
    ("goldbeter-torus", "goldbeter", "torus", 0.4, {}),
    ("goldbeter-just-diffusion", "goldbeter", "torus", 0.4, dict(just_diffusion=1)),
]


def case(config, nx, ny, precision="f64", t_boundary=T_BOUNDARY):
    """(crd_params, oracle Problem) of one configuration on one grid."""
    import crdmodel_amd as crd

    _, model, surface, beta, kw = config
    p = crd.make_params(model, surface, nx, 80.0, 20.0, 0.12, beta, ny=ny, t_boundary=t_boundary, precision=precision, **kw)
    return p, problem_of(model, surface, nx, ny, beta, t_boundary=t_boundary, **kw)


def start_state(p, seed):
    """The state of tests/test_gpu_ensemble_adaptive.py: start_state -- the reference's initial conditions plus noise -- in the
    context's precision; Goldbeter states stay positive."""
    import crdmodel_amd as crd

    cfg = crd.run_config(p, wave_length=0.1, wave_width=0.5, wave_inside=0)
    y = crd.initial_conditions(cfg)
    rng = np.random.default_rng(seed)
    y = y + 0.02 * rng.standard_normal(y.shape)
    if p.model == crd._capi.MODEL_GOLDBETER:
        assert y.min() > 0.0, y.min()
    return y.astype(np.float32) if p.precision == crd._capi.PRECISION_F32 else y


def direction(p, seed):
    """A standard normal direction in the context's precision."""
    import crdmodel_amd as crd

    g = crd.grid_of(p)
    v = np.random.default_rng(seed).standard_normal((g.ny, g.nx, 2))
    return v.astype(np.float32) if p.precision == crd._capi.PRECISION_F32 else v


def shim_build_command(exe):
    """gcc command line of tests/native/shim_imex_selftest.c + integration/crd_arkode_shim.c against the test double."""
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.join(ROOT, "crdmodel_amd")
    return ["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "integration"),
            "-I", os.path.join(ROOT, "tests", "native"), '-DCRD_SHIM_NVECTOR_HEADER="mock_nvector.h"', os.path.join(ROOT, "integration", "crd_arkode_shim.c"),
            os.path.join(ROOT, "tests", "native", "shim_imex_selftest.c"), "-o", str(exe), "-L", lib_dir, "-lcrd", "-Wl,-rpath," + lib_dir,
            "-Wl,-rpath,/opt/rocm/lib", "-lm"]
