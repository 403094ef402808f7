"""Reference for the IMEX stepper (crd_step_imex / Slab.step_imex, crdmodel_amd/csrc/crd_imex*.{h,cpp,hip}).  TEST INFRASTRUCTURE ONLY.

The schemes
-----------
`exact(scheme)` holds the three tableaux as the issue states them, in Fractions (ARS222: floats, gamma = 1 - 1/sqrt(2) is irrational);
`tableau(scheme)` the doubles crd_imex_tables.h forms -- a Fraction p/q becomes the correctly rounded quotient, which is what the C++
expression p.0 / q.0 gives, and ARS222's entries are formed by the header's own expressions.  tests/test_imex_host.py checks the order
conditions on the first and holds the second to the header's values bit for bit (tests/native/imex_tables_selftest.cpp prints them).

Layout: stage 0 is Y_0 = y_n; AE[i][j] (j < i) and AI[i][j] (1 <= j <= i) are full (s + 1) x (s + 1) matrices, c has s + 1 entries, the
weights are the last rows.

The dense restatement
---------------------
`Dense(op)` assembles L(t), the matrix of the oracle's diffusion operator on the activator (oracle/crd_oracle_np.diffusion applied to
unit vectors, rows held at zero while t < tBoundary), and evaluates the kinetics by jacobian_reference._reaction; `dense_step` is the
step of include/crd.h in float64 with numpy.linalg.solve for (I - dt gamma L(t_i)) k_i = L(t_i) R_i.  Mutants of it (MUTANTS) each
fail an assertion of tests/test_imex_host.py.

The allowance of a device step against the dense one
----------------------------------------------------
`step_allowance` bounds || y_device - y_dense ||_2 after one step to first order in the errors, given the bound e0 on the two
states' distance before it: G e0 + d, with G = || d y_{n+1} / d y_n ||_2 of the dense step (`step_gain`: the chain rule through the
step with the dense matrices) and d what the step's own errors leave from a common start (e0 = 0 below).  Per stage, with u the unit roundoff, A_i = I - dt gamma L(t_i) and, FROM THE DENSE MATRIX on the CPU,
kappa_i = ||A_i^-1||_2 and lambda_i = ||A_i^-1 L(t_i)||_2 (singular values: the torus operator is not symmetric and these norms have no
closed form), Lip = the largest 2-norm of the kinetics' 2 x 2 block over the grid at the dense stage value:

    solve    the device's k_i satisfies A k = r_dev - rho with ||rho|| <= krylov_reference.residual_allowance's bound at the solve's rtol
             (its stopping rule plus the rounding of its own residual), and r_dev = f_D(R_dev) is off by L dR plus f_D's rounding bound
             (jacobian_reference.part_bound):         a_i = lambda_i r_i + kappa_i (|| bound_D(R_i) || + rho_i)
    Y_i      = fma(dt gamma, k_i, R_i), one rounding; dY = A^-1 dR + dt gamma A^-1 (f_D's error - rho), because I + dt gamma A^-1 L = A^-1:
                                                       y_i = kappa_i r_i + dt gamma kappa_i (|| bound_D(R_i) || + rho_i) + u ||Y_i||
    FR_i     f_i = Lip y_i + || bound_R(Y_i) ||
    R_{i+1}  = y_n + m terms, one fma and so one rounding each, every partial sum at most S = |y_n| + sum |coef| |vector|:
             r_{i+1} = sum_j |hE| f_j + sum_j |hI| a_j + m u ||S||

and the step's error is y_s.  Nothing in it is fitted to a device result: the constants are norms of the dense matrices, the bounds of
the parts of f are those tests/test_gpu_jacobian.py holds the kernels to, and the solve's is the one tests/test_gpu_krylov.py holds
crd_lsolve_* to.  `steps_allowance` chains it over several steps.
"""
import math
import os
from fractions import Fraction as Fr

import numpy as np

import jacobian_reference as jr
import krylov_reference as kr
from oracle import crd_oracle_np as cn
from oracle import error_bounds as eb

SCHEMES = ("euler", "ars222", "ars443")
ORDER = {"euler": 1, "ars222": 2, "ars443": 3}
MUTANTS = ("swapped_coefficient", "rows_exchanged", "stage_time", "dropped_term")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _full(rows_e, rows_i, c):
    """(s, c, AE, AI) with full (s + 1) x (s + 1) matrices from the issue's rows: A^E columns 0 .. i - 1, A^I columns 1 .. i."""
    s = len(rows_e)
    zero = type(c[0])(0)
    AE = [[zero] * (s + 1) for _ in range(s + 1)]
    AI = [[zero] * (s + 1) for _ in range(s + 1)]
    for i in range(1, s + 1):
        assert len(rows_e[i - 1]) == i and len(rows_i[i - 1]) == i
        for j in range(i):
            AE[i][j] = rows_e[i - 1][j]
            AI[i][j + 1] = rows_i[i - 1][j]
    return s, list(c), AE, AI


def exact(scheme):
    """(s, c, AE, AI, gamma): Fractions for euler and ars443, floats for ars222."""
    if scheme == "euler":
        return _full([[Fr(1)]], [[Fr(1)]], [Fr(0), Fr(1)]) + (Fr(1),)
    if scheme == "ars222":
        g = 1.0 - 1.0 / math.sqrt(2.0)
        d = 1.0 - 1.0 / (2.0 * g)
        return _full([[g], [d, 1.0 - d]], [[g], [1.0 - g, g]], [0.0, g, 1.0]) + (g,)
    assert scheme == "ars443", scheme
    F = Fr
    rows_e = [[F(1, 2)], [F(11, 18), F(1, 18)], [F(5, 6), F(-5, 6), F(1, 2)], [F(1, 4), F(7, 4), F(3, 4), F(-7, 4)]]
    rows_i = [[F(1, 2)], [F(1, 6), F(1, 2)], [F(-1, 2), F(1, 2), F(1, 2)], [F(3, 2), F(-3, 2), F(1, 2), F(1, 2)]]
    return _full(rows_e, rows_i, [F(0), F(1, 2), F(2, 3), F(1, 2), F(1)]) + (F(1, 2),)


def tableau(scheme):
    """(s, c, AE, AI, gamma) in the doubles of crd_imex_tables.h."""
    s, c, AE, AI, g = exact(scheme)
    f = lambda rows: [[float(x) for x in row] for row in rows]
    return s, [float(x) for x in c], f(AE), f(AI), float(g)


def order_residuals(scheme):
    """{condition: residual} of every order condition up to order 3 of the additive pair, coupling conditions included: the row sums
    (A e = c for both matrices), b.e, b.c, b.c^2 and b.A.c for every pairing of b^E / b^I with A^E / A^I; b is the last row."""
    s, c, AE, AI, _ = exact(scheme)
    n = s + 1
    out = {}
    for name, A in (("E", AE), ("I", AI)):
        for i in range(n):
            out["row sum %s %d" % (name, i)] = sum(A[i]) - c[i]
    for bn, B in (("E", AE), ("I", AI)):
        b = B[s]
        out["b%s.e" % bn] = sum(b) - 1
        out["b%s.c" % bn] = sum(b[j] * c[j] for j in range(n)) - Fr(1, 2)
        out["b%s.c^2" % bn] = sum(b[j] * c[j] * c[j] for j in range(n)) - Fr(1, 3)
        for an, A in (("E", AE), ("I", AI)):
            out["b%s.A%s.c" % (bn, an)] = sum(b[i] * A[i][j] * c[j] for i in range(n) for j in range(n)) - Fr(1, 6)
    return out


def condition_order(name):
    """The order at which a condition of order_residuals enters: 1 (row sums, b.e), 2 (b.c) or 3 (b.c^2, b.A.c)."""
    if name.startswith("row sum") or name.endswith(".e"):
        return 1
    return 2 if name in ("bE.c", "bI.c") else 3


def row_terms(scheme, nxt, dt, R):
    """[(j, "E" or "I", coefficient in R)] of R_{nxt} in the kernel's order: j ascending, explicit then implicit; zeros left out."""
    s, c, AE, AI, g = tableau(scheme)
    out = []
    for j in range(nxt):
        e = R(dt * AE[nxt][j])
        if e != 0:
            out.append((j, "E", e))
        if j >= 1:
            i = R(dt * AI[nxt][j])
            if i != 0:
                out.append((j, "I", i))
    return out


# ---- the dense restatement --------------------------------------------------------------------------------------------------------
class Dense:
    def __init__(self, op):
        self.op, self.P = op, eb._Problem(op)
        self.ny, self.nx = op.ny, op.nx
        n = self.ny * self.nx
        L = np.empty((n, n))
        e = np.zeros(n)
        for q in range(n):
            e[q] = 1.0
            L[:, q] = cn.diffusion(self.P.surface, self.P.g, self.P.D, e.reshape(self.ny, self.nx), np.float64).ravel()
            e[q] = 0.0
        self.L_free = L
        self._cache = {}

    def held(self, t):
        return bool(self.P.zero_rows(t, self.ny, 0).any())

    def L(self, t):
        if not self.held(t):
            return self.L_free
        if "held" not in self._cache:
            L = self.L_free.copy()
            L[np.repeat(self.P.zero_rows(t, self.ny, 0), self.nx)] = 0.0
            self._cache["held"] = L
        return self._cache["held"]

    def f_R(self, t, y):
        u, v = y[..., 0].astype(np.float64), y[..., 1].astype(np.float64)
        du, dv = jr._reaction(self.P, u, v)
        zero = self.P.zero_rows(t, self.ny, 0)
        du[zero] = 0.0
        dv[zero] = 0.0
        return np.stack([du, dv], axis=-1)

    def f(self, t, y):
        out = self.f_R(t, y)
        out[..., 0] += (self.L(t) @ y[..., 0].ravel()).reshape(self.ny, self.nx)
        return out

    def norms(self, t, hg):
        """(kappa, lam, ||L||) = (||A^-1||_2, ||A^-1 L||_2, ||L||_2) of A = I - hg L(t)."""
        key = (self.held(t), hg)
        if key not in self._cache:
            L = self.L(t)
            Ainv = np.linalg.inv(np.eye(L.shape[0]) - hg * L)
            self._cache[key] = (float(np.linalg.norm(Ainv, 2)), float(np.linalg.norm(Ainv @ L, 2)), float(np.linalg.norm(L, 2)))
        return self._cache[key]


def _mutated(scheme, mutant):
    s, c, AE, AI, g = tableau(scheme)
    AE, AI = [row[:] for row in AE], [row[:] for row in AI]
    if mutant == "swapped_coefficient":  # the last row's first two explicit coefficients change places
        assert s >= 2
        AE[s][0], AE[s][1] = AE[s][1], AE[s][0]
    if mutant == "rows_exchanged":  # the last stage's explicit and implicit rows: FR_j takes A^I_sj, k_j takes A^E_sj (j < s)
        assert s >= 2
        for j in range(1, s):
            AE[s][j], AI[s][j] = AI[s][j], AE[s][j]
    if mutant == "dropped_term":  # the last implicit term of the last row
        assert s >= 2
        AI[s][s - 1] = 0.0
    return s, c, AE, AI, g


def dense_step(D, scheme, t, dt, y, mutant=None, stages=None):
    """One step in float64; `stages` (a list) receives (t_i, R_i, k_i, Y_i, FR_i) per stage i >= 1 and (t, None, None, y, FR_0) first."""
    assert mutant is None or mutant in MUTANTS, mutant
    s, c, AE, AI, g = _mutated(scheme, mutant)
    y = np.asarray(y, dtype=np.float64)
    n = D.ny * D.nx
    FR, k = [D.f_R(t, y)], [None]
    if stages is not None:
        stages.append((t, None, None, y, FR[0]))
    R = y + dt * AE[1][0] * FR[0]
    Y = y
    for i in range(1, s + 1):
        ti = t if mutant == "stage_time" else t + c[i] * dt
        L = D.L(ti)
        ku = np.linalg.solve(np.eye(n) - (dt * g) * L, L @ R[..., 0].ravel()).reshape(D.ny, D.nx)
        ki = np.stack([ku, np.zeros_like(ku)], axis=-1)
        k.append(ki)
        Y = R + (dt * g) * ki
        Fi = D.f_R(ti, Y)
        FR.append(Fi)
        if stages is not None:
            stages.append((ti, R, ki, Y, Fi))
        if i < s:
            R = y.copy()
            for j in range(i + 1):
                R = R + dt * AE[i + 1][j] * FR[j]
                if j >= 1:
                    R = R + dt * AI[i + 1][j] * k[j]
    return Y


def dense_steps(D, scheme, t0, dt, nsteps, y, mutant=None):
    for n in range(nsteps):
        y = dense_step(D, scheme, t0 + n * dt, dt, y, mutant)
    return y


def rk4_steps(D, t0, dt, nsteps, y):
    """Classical RK4 on the oracle's f (oracle/crd_oracle_np.rk4), float64."""
    u, v = cn.rk4(D.P.model, D.P.surface, D.P.g, D.P.D, y[..., 0], y[..., 1], t0, dt, nsteps, **D.P.kw)
    return np.stack([u, v], axis=-1)


def lipschitz(D, y):
    """The largest 2-norm of the kinetics' block d f_R / d (u, v) over the grid at the state y."""
    (a11, a12, a21, a22), _ = jr.block(D.P, y[..., 0].astype(np.float64), y[..., 1].astype(np.float64))
    blocks = np.stack([np.stack([a11, a12], -1), np.stack([a21, a22], -1)], -2).reshape(-1, 2, 2)
    return float(np.linalg.norm(blocks, 2, axis=(1, 2)).max())


def _block_matrices(D, t, y):
    """The kinetics' block at y as four diagonals (a11, a12, a21, a22), rows held at t zeroed: d f_R(t, .) / d (u, v)."""
    (a11, a12, a21, a22), _ = jr.block(D.P, y[..., 0].astype(np.float64), y[..., 1].astype(np.float64))
    zero = D.P.zero_rows(t, D.ny, 0)
    out = []
    for a in (a11, a12, a21, a22):
        a = np.array(a, dtype=np.float64)
        a[zero] = 0.0
        out.append(a.ravel())
    return out


def step_gain(D, scheme, dt, stages):
    """||d y_{n+1} / d y_n||_2 of the dense step, from its stage values: the chain rule through the step with dense matrices, unknowns
    ordered (u; v).  dk_i = A_i^-1 L_i dR_i on u, dY_i = dR_i + dt gamma dk_i, dFR_i = J_R(Y_i) dY_i, dR_{i+1} = dy + sum hE dFR_j + hI dk_j."""
    s, c, AE, AI, g = tableau(scheme)
    n = D.ny * D.nx
    I2 = np.eye(2 * n)

    def kinetics(t, y, M):
        a11, a12, a21, a22 = _block_matrices(D, t, y)
        return np.vstack([a11[:, None] * M[:n] + a12[:, None] * M[n:], a21[:, None] * M[:n] + a22[:, None] * M[n:]])

    MF, Mk = [kinetics(stages[0][0], stages[0][3], I2)], [None]
    MR = I2 + dt * AE[1][0] * MF[0]
    MY = I2
    for i in range(1, s + 1):
        ti, _, _, Yi, _ = stages[i]
        L = D.L(ti)
        B = np.linalg.solve(np.eye(n) - dt * g * L, L)
        Mk.append(np.vstack([B @ MR[:n], np.zeros((n, 2 * n))]))
        MY = MR + dt * g * Mk[i]
        MF.append(kinetics(ti, Yi, MY))
        if i < s:
            MR = I2.copy()
            for j in range(i + 1):
                MR += dt * AE[i + 1][j] * MF[j]
                if j >= 1:
                    MR += dt * AI[i + 1][j] * Mk[j]
    return float(np.linalg.norm(MY, 2))


def step_allowance(D, scheme, t, dt, y, e0, rtol, precision="f64", atol=0.0):
    """(bound on ||y_device - y_dense||_2 after the step from (t, y), the dense step's result): gain x e0 + the module docstring's
    recursion from a common start."""
    u = eb.UNIT[precision]
    R_ = kr.DTYPES[precision]
    s, c, AE, AI, g = tableau(scheme)
    hg = float(R_(dt * g))
    stages = []
    y1 = dense_step(D, scheme, t, dt, y, stages=stages)
    nrm = lambda x: float(np.linalg.norm(np.asarray(x, dtype=np.float64)))
    part = lambda ti, x, which: nrm(np.stack(jr.part_bound(D.op, ti, x, precision, which)[1:], -1))
    f = [part(t, y, jr.REACTION)]
    a = [0.0]
    r = abs(dt * AE[1][0]) * f[0] + u * nrm(np.abs(y) + abs(dt * AE[1][0]) * np.abs(stages[0][4]))
    y_err = 0.0
    for i in range(1, s + 1):
        ti, Ri, ki, Yi, Fi = stages[i]
        kappa, lam, _ = D.norms(ti, hg)
        rhs = np.stack([(D.L(ti) @ Ri[..., 0].ravel()).reshape(D.ny, D.nx), np.zeros((D.ny, D.nx))], -1)
        _, rho = kr.residual_allowance(D.op, ti, hg, None, ki, rhs, precision, jr.DIFFUSION, rtol, atol)
        inject = kappa * (part(ti, Ri, jr.DIFFUSION) + rho)
        a.append(lam * r + inject)
        y_err = kappa * r + hg * inject + u * nrm(Yi)  # dY = A^-1 dR + dt gamma A^-1 (the solve's own errors): I + dt gamma A^-1 L = A^-1
        f.append(lipschitz(D, Yi) * y_err + part(ti, Yi, jr.REACTION))
        if i < s:
            S, m, r = np.abs(y), 0, 0.0
            for j in range(i + 1):
                for coef, vec, err in ((dt * AE[i + 1][j], stages[j][4], f[j]),) + (((dt * AI[i + 1][j], stages[j][2], a[j]),) if j >= 1 else ()):
                    if coef != 0.0:
                        S, m, r = S + abs(coef) * np.abs(vec), m + 1, r + abs(coef) * err
            r += m * u * nrm(S)
    gain = step_gain(D, scheme, dt, stages) if e0 > 0.0 else 0.0
    return gain * e0 + y_err, y1


def steps_allowance(D, scheme, t0, dt, nsteps, y, rtol, precision="f64"):
    """(bound after nsteps steps from an exact common start, the dense result)."""
    e = 0.0
    for n in range(nsteps):
        e, y = step_allowance(D, scheme, t0 + n * dt, dt, y, e, rtol, precision)
    return e, y


# ---- the step of include/crd.h from the public pieces: what Slab.step_imex must equal bit for bit -----------------------------------
# jacobian_reference._fma forms a b + c one size up and rounds the result a second time: right for a bound, but about one float64 result
# in 2^11 lands on the other side of a tie (the 64-bit significand of np.longdouble does not hold the 106-bit product), and a
# bit-for-bit comparison over some 10^5 operations would fail on the reference's own account.  fma_exact is correctly rounded for every
# finite input away from overflow and underflow: error-free transformations and one rounding to odd (Boldo and Melquiond, "Emulation of
# a FMA and correctly rounded sums: proved algorithms using rounding to odd", IEEE Trans. Computers 57, 2008).  tests/test_imex_host.py
# holds it to exact rational arithmetic, ties included, and to _fma wherever _fma is right.
def _two_sum(x, y):
    s = x + y
    b = s - x
    return s, (x - (s - b)) + (y - b)


def _sum_to_odd(x, y):
    """x + y in float64 rounded to odd: the neighbour of the exact sum whose last significand bit is set, unless the sum is exact."""
    s, e = _two_sum(x, y)
    even = (s.view(np.int64) & 1) == 0
    return np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)


def _two_product(a, b):
    """(p, e) with p + e = a b exactly (Dekker, with Veltkamp's splitting), float64."""
    split = 134217729.0  # 2^27 + 1
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    p = a * b
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma_exact(R):
    """The correctly rounded a b + c of the precision R (np.float32 or np.float64) on arrays."""
    def f64(a, b, c):
        a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
        a, b, c = np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c)
        uh, ul = _two_product(a, b)
        th, tl = _two_sum(c, uh)
        return th + _sum_to_odd(tl, ul)

    def f32(a, b, c):
        a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
        return _sum_to_odd(np.ascontiguousarray(a * b), np.ascontiguousarray(c)).astype(np.float32)  # the product of two floats is exact in float64

    return f32 if R == np.float32 else f64


def composed_step(slab, scheme, t, dt, y, **lsolve_options):
    """(y_new, [lsolve stats]) of one step as a loop over Slab.rhs_part, Slab.lsolve and fma_exact (jacobian_reference._fma without its
    second rounding) in the slab's precision; y_new is None behind a solve that did not converge."""
    R_ = slab.dtype
    fma = fma_exact(R_)
    s, c, AE, AI, g = tableau(scheme)
    hg = R_(dt * g)
    y = np.ascontiguousarray(y, dtype=R_)
    FR, k, stats = [slab.rhs_part(t, y, "reaction")], [None], []
    R = fma(R_(dt * AE[1][0]), FR[0], y)
    for i in range(1, s + 1):
        ti = t + c[i] * dt
        r = slab.rhs_part(ti, R, "diffusion")
        ki, st = slab.lsolve(ti, float(hg), r, **lsolve_options)
        stats.append(st)
        if not st.converged:
            return None, stats
        k.append(ki)
        Y = fma(hg, ki, R)
        if i == s:
            return Y, stats
        FR.append(slab.rhs_part(ti, Y, "reaction"))
        R = y
        for j, which, coef in row_terms(scheme, i + 1, dt, R_):
            R = fma(coef, FR[j] if which == "E" else k[j], R)


def composed_steps(slab, scheme, t0, dt, nsteps, y, **lsolve_options):
    stats = []
    for n in range(nsteps):
        y, st = composed_step(slab, scheme, t0 + n * dt, dt, y, **lsolve_options)
        stats += st
        if y is None:
            break
    return y, stats


def smooth_state(op, amplitude=0.5):
    """A smooth FHN state around the steady state of beta = 1.25: one Fourier mode in each direction."""
    th = 2 * np.pi * np.arange(op.nx) / op.nx
    ph = 2 * np.pi * np.arange(op.ny) / op.ny
    u = -1.25 + amplitude * np.cos(ph)[:, None] * (1 + 0.5 * np.sin(th)[None, :])
    v = -1.25 * (3 - 1.25 ** 2) + 0.3 * amplitude * np.sin(ph)[:, None] * np.cos(th)[None, :]
    return np.stack([u, v], axis=-1)


def selftest_build_command(exe, sanitizers=None):
    """g++ command line of tests/native/imex_tables_selftest.cpp (plain C++17 against crd_imex_tables.h, nothing of HIP)."""
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "crdmodel_amd", "csrc"), os.path.join(ROOT, "tests", "native", "imex_tables_selftest.cpp"),
           "-o", str(exe)]
    if sanitizers:
        cmd[4:4] = ["-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizers, "-fno-sanitize-recover=all"]
    return cmd
