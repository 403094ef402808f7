"""Reference, kernel-order restatement and bounds of the linear solve (I - gamma J_part(t, y)) z = r by restarted, right-preconditioned
GMRES on the device (crd_lsolve_*, crdmodel_amd/csrc/crd_krylov.cpp / crd_krylov.hip / crd_krylov_host.h).  TEST INFRASTRUCTURE ONLY.

The algorithm (include/crd.h states it; this module restates it twice through one driver, `gmres`)
--------------------------------------------------------------------------------------------------
z = 0; per cycle: res = r - A z (the first cycle: r), beta = ||res||, stop if beta <= tol = rtol ||r|| + atol; V_0 = res / beta;
inner iteration j: w = A M V_j; h1 = V^T w, w -= V h1, h2 = V^T w, w -= V h2 (classical Gram-Schmidt twice), column = (h1 + h2, ||w||);
breakdown when ||w|| <= 2 u ||column||_2 -- the column is final, no new vector; else Givens rotation j, residual estimate |g_{j+1}|,
V_{j+1} = w / ||w||; the cycle ends at `restart` columns, at max_iters inner iterations in total, on a breakdown or when the estimate is
<= tol, with z += M (V y), y the least-squares solution.  A v = v - gamma J_part v; M is the multigrid cycle on var0 and the identity on
var1, or the identity.  DIFFUSION: var1 of the residual is masked to 0 (every Krylov vector has var1 = 0) and z_var1 = r_var1 at the end.

Reference (reference_solve): that driver in error_bounds.reference_dtype(precision) -- np.longdouble for the fp64 kernels, float64 on the
exactly widened vectors for the fp32 kernels -- with the operator from multigrid_reference.operator (FULL: jacobian_reference's J v in the
same dtype) and M from multigrid_reference.reference_vcycle.  Returns the iterate and the residual history.

Kernel order (kernel_order_solve): the driver in the device precision R with jacobian_reference.kernel_order_jtimes,
multigrid_reference.kernel_order_vcycle and the reductions in the kernels' own summation order (kernel_order_dots).

The multi-dot's summation tree and its bound (dot_roundings, dots_bound)
------------------------------------------------------------------------
<V_i, w> over n reals, G = min(512, ceil(n / 256)) blocks of 256 threads, accumulators double in both precisions:
  thread   element q = block 256 + thread + k (256 G), k = 0 .. trips - 1, trips = ceil(n / (256 G)): a chain acc = fma(V_i[q], w[q], acc).
           The first term passes through `trips` roundings (in fp32 the product of two floats is exact in double; in fp64 the fused
           multiply-add rounds product and sum once).
  wave     six shuffle steps, lane l += lane l + off, off = 32 .. 1: 6 additions.
  block    ((p0 + p1) + p2) + p3 over the four wavefronts: 3 additions.
  final    one wavefront per vector: lane l adds partials l, l + 64, ... in order -- ceil(G / 64) additions -- then six shuffle steps.
A term passes through at most K = trips + 6 + 3 + ceil(G / 64) + 6 additions, each of relative error <= u64 = 2^-53, so
    |h_i - <V_i, w>| <= gamma_K sum_q |V_i[q] w[q]|,   gamma_K = K u64 / (1 - K u64)
(Higham, Accuracy and Stability of Numerical Algorithms, 4.2: any summation order, K the longest path).  Nothing more in fp32: the
products are exact.  19 x 27 (n = 1026, G = 5): K = 1 + 15 + 1 = 17; 264 x 250 (n = 132000, G = 512): K = 2 + 15 + 8 = 25; 8192^2: 1047.
The long-double reference's own rounding (2^-64 of the same sums) is ignored, as in error_bounds.

Orthogonality (orthogonality_allowance)
---------------------------------------
Classical Gram-Schmidt applied twice: the second pass starts from a w that the first has already made orthogonal to V up to u kappa
(Giraud, Langou, Rozloznik, van den Eshof, Numer. Math. 101 (2005): "twice is enough" while the Krylov matrix is numerically of full
rank), so it barely changes ||w||, and what it leaves of V_i in w is its own rounding: the coefficient's error, gamma_K ||w|| by
Cauchy-Schwarz (||V_i|| = 1), the j + 1 fused multiply-adds and the store's rounding of the update, (j + 2) u ||w||, and the rounding of
the quotient in the scale, u.  Per entry of V^T V - I, with a factor 2 for ||w|| before over ||w|| after the second pass:
    2 (K u64 + (columns + 3) u),   u the unit roundoff of the vectors' precision.
Applied once, Gram-Schmidt loses orthogonality like u kappa^2, kappa about ||r|| over the current residual: all of it by the time the
residual has fallen by 1 / sqrt(u).

Allowance for the solver (residual_allowance)
---------------------------------------------
tests/test_gpu_multigrid.py: test_gmres_with_the_device_preconditioner's: the residual r - (z - gamma J z) under the reference operator may
be  rtol ||r|| + atol + || gamma B_J + 2 u (|z| + gamma |J z|) ||  with B_J jacobian_reference.jtimes_bound's per-point bound on J z.
"""
import numpy as np

import jacobian_reference as jr
import multigrid_reference as mg
from oracle import error_bounds as eb
from oracle.error_bounds import UNIT

THREADS, BLOCKS, GROUP = 256, 512, 8  # crd_krylov.h: kKrylovThreads, kKrylovBlocks, kKrylovGroup
DTYPES = {"f64": np.float64, "f32": np.float32}
DOT_MUTANTS = ("last_element", "tail_block", "first_trip", "var0_only", "slot_shift")
SOLVE_MUTANTS = ("one_pass", "no_final_m", "givens_sign")
MUTANTS = DOT_MUTANTS + SOLVE_MUTANTS
# the gate that claims each mutant
MUTANT_GATES = dict({m: "dots" for m in DOT_MUTANTS}, one_pass="orthogonality", no_final_m="solve", givens_sign="solve")
U64 = 2.0 ** -53


def grid(n):
    return min(BLOCKS, max(1, -(-n // THREADS)))


def dot_roundings(n):
    """K of the module docstring."""
    G = grid(n)
    trips = -(-n // (G * THREADS))
    return trips + 6 + 3 + -(-G // 64) + 6


def dots_bound(V, w):
    """(ref, bound, sizes) of h_i = <V_i, w>: V (count, n), w (n,) in either precision; ref in long double."""
    L = np.longdouble
    V, w = np.asarray(V), np.asarray(w)
    prod = V.astype(L) * w.astype(L)[None, :]
    sizes = np.abs(prod).sum(axis=1).astype(np.float64)
    K = dot_roundings(w.size)
    return prod.sum(axis=1), K * U64 / (1 - K * U64) * sizes, sizes


_fma64 = jr._fma(np.float64)


def _wave(a):
    for off in (32, 16, 8, 4, 2, 1):
        a = a[..., :off] + a[..., off:2 * off]
    return a[..., 0]


def kernel_order_sums(x, y, mutant=None):
    """sum_q x[i, q] y[q] in the multi-dot's order (module docstring): x (count, n) and y (n,) float64 (widened exactly from the device
    precision), result float64 (count,).  mutant: one of DOT_MUTANTS."""
    assert mutant is None or mutant in DOT_MUTANTS, mutant
    x, y = np.array(x, dtype=np.float64, ndmin=2), np.asarray(y, dtype=np.float64)
    count, n = x.shape
    G = grid(n)
    step = G * THREADS
    trips = -(-n // step)
    if mutant == "last_element":
        x[:, n - 1] = 0
    if mutant == "var0_only":
        x[:, 1::2] = 0
    X = np.pad(x, ((0, 0), (0, trips * step - n))).reshape(count, trips, G, THREADS // 64, 64)
    Y = np.pad(y, (0, trips * step - n)).reshape(trips, G, THREADS // 64, 64)
    acc = np.zeros((count, G, THREADS // 64, 64))
    for k in range(1 if mutant == "first_trip" else trips):
        acc = _fma64(X[:, k], Y[k][None], acc)
    p = _wave(acc)
    partials = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]  # (count, G)
    if mutant == "tail_block":
        partials[:, G - 1] = 0
    rows = -(-G // 64)
    P = np.pad(partials, ((0, 0), (0, rows * 64 - G))).reshape(count, rows, 64)
    lane = np.zeros((count, 64))
    for k in range(rows):
        lane = lane + P[:, k]
    h = _wave(lane)
    return np.roll(h, -1) if mutant == "slot_shift" else h


def kernel_order_dots(V, w, mutant=None):
    return kernel_order_sums(np.asarray(V, dtype=np.float64), np.asarray(w, dtype=np.float64), mutant)


def planted(n, count, positions, R, seed=7):
    """(V, w, where): noise of size 1e-3 and, per vector i, ONE element at where[i] = positions[i % len] whose product with w carries the
    sum: V_i[q] = 1 + i / 64, w[q] = 1 at every planted q (the other vectors have noise there)."""
    rng = np.random.default_rng(seed)
    V = (1e-3 * rng.standard_normal((count, n))).astype(R)
    w = (1e-3 * rng.standard_normal(n)).astype(R)
    where = [positions[i % len(positions)] for i in range(count)]
    for q in set(where):
        w[q] = 1
    for i, q in enumerate(where):
        V[i, q] = R(1 + i / 64.0)
    return V, w, where


def plant_positions(n):
    """Index 0, 63 | 64, 255 | 256, the last index of the first grid-stride trip and the first of the second (where the vector has a
    second), and n - 1: var0 (even) and var1 (odd) both occur."""
    first = grid(n) * THREADS
    p = [0, 63, 64, 255, 256] + ([first - 1, first] if n > first else []) + [n - 1]
    return [q for q in p if q < n]


# ---- the small least-squares problem (crd_krylov_host.h: LeastSquares) ------------------------------------------------------------
class LeastSquares:
    def __init__(self, restart, beta, dtype=np.float64, mutant=None):
        self.m, self.k, self.dt, self.mutant, self.breakdown = restart, 0, dtype, mutant, False
        self.R = np.zeros((restart, restart), dtype=dtype)  # [row, column]
        self.c, self.s = np.ones(restart, dtype=dtype), np.zeros(restart, dtype=dtype)
        self.g = np.zeros(restart + 1, dtype=dtype)
        self.g[0] = beta

    def full(self):
        return self.k >= self.m or self.breakdown

    def residual(self):
        return abs(self.g[self.k])

    def push(self, h, unit):
        k = self.k
        h = np.asarray(h, dtype=self.dt)
        nxt = h[k + 1]
        self.breakdown = not (nxt > 2 * unit * np.sqrt(np.sum(h[:k + 2] * h[:k + 2])))
        col = h[:k + 1].copy()
        for i in range(k):
            a, b = col[i], col[i + 1]
            col[i], col[i + 1] = self.c[i] * a + self.s[i] * b, -self.s[i] * a + self.c[i] * b
        if self.breakdown:
            self.g[k + 1] = 0
        else:
            a = col[k]
            r = np.hypot(a, nxt)
            self.c[k], self.s[k] = a / r, nxt / r
            col[k] = r
            self.g[k + 1] = (self.s[k] if self.mutant == "givens_sign" else -self.s[k]) * self.g[k]
            self.g[k] = self.c[k] * self.g[k]
        self.R[:k + 1, k] = col
        self.k = k + 1

    def solve(self):
        y = np.zeros(self.k, dtype=self.dt)
        for i in range(self.k - 1, -1, -1):
            a = self.g[i] - np.sum(self.R[i, i + 1:self.k] * y[i + 1:])
            y[i] = a / self.R[i, i] if self.R[i, i] != 0 else 0
        return y


# ---- one driver, two sets of operations -------------------------------------------------------------------------------------------
class Result:
    def __init__(self):
        self.converged, self.iterations, self.restarts, self.matvecs, self.psolves, self.breakdown = 0, 0, 0, 0, 0, 0
        self.r_norm = self.res_norm = 0.0
        self.history, self.z, self.basis = [], None, None


def gmres(ops, r, gamma, diffusion, restart, max_iters, rtol, atol, unit, mutant=None):
    """The algorithm of the module docstring on AoS arrays (ny, nx, 2).  ops: A(x), M(x), dots(V list, w) -> coefficients,
    update(V list, h, w) -> (w, ||w||^2), scale(w, norm2), combine(V list, y), add(z, d), sub(r, a), ls_dtype.  Returns a Result: history
    is [beta, the estimate after every inner iteration ...] of every cycle in order, basis the last cycle's vectors."""
    out = Result()
    out.r_norm = float(np.sqrt(ops.dots([r], r)[0]))
    if gamma == 0 or out.r_norm == 0:
        out.z, out.converged = r.copy(), 1
        return out
    tol = rtol * out.r_norm + atol
    mask = lambda x: np.stack([x[..., 0], np.zeros_like(x[..., 1])], axis=-1) if diffusion else x
    z, res = np.zeros_like(r), mask(r)
    cycle = 0
    while out.iterations < max_iters:
        if cycle > 0:
            out.restarts += 1
            res = mask(ops.sub(r, ops.A(z)))
            out.matvecs += 1
        cycle += 1
        sq = ops.dots([res], res)[0]
        beta = np.sqrt(sq)
        out.res_norm = float(beta)
        out.history.append(float(beta))
        if not beta > tol:
            out.converged = int(beta <= tol)
            break
        V = [ops.scale(res, sq)]
        ls = LeastSquares(restart, beta, ops.ls_dtype, mutant)
        while not ls.full() and out.iterations < max_iters:
            j = ls.k
            w = ops.A(ops.M(V[j]))
            out.matvecs, out.psolves = out.matvecs + 1, out.psolves + 1
            col = np.zeros(j + 2, dtype=ops.ls_dtype)
            norm2 = None
            for _ in range(1 if mutant == "one_pass" else 2):
                h = ops.dots(V, w)
                w, norm2 = ops.update(V, h, w)
                col[:j + 1] += h
            col[j + 1] = np.sqrt(norm2)
            ls.push(col, unit)
            out.iterations += 1
            out.res_norm = float(ls.residual())
            out.history.append(out.res_norm)
            if ls.breakdown:
                out.breakdown = 1
            if out.res_norm <= tol:
                break
            if not ls.full() and out.iterations < max_iters:
                V.append(ops.scale(w, norm2))
        x = ops.combine(V[:ls.k], ls.solve())
        z = ops.add(z, x if mutant == "no_final_m" else ops.M(x))
        out.psolves += 1
        out.basis = V
        if out.res_norm <= tol:
            out.converged = 1
            break
    if diffusion:
        z = np.stack([z[..., 0], r[..., 1]], axis=-1)
    out.z = z
    return out


class _Operators:
    """A and M of a problem in the dtype dt: the reference's (kernel = False) or the kernels' own order in the device precision."""

    def __init__(self, op, t, gamma, y, part, precondition, dt, kernel, psolve):
        self.op, self.t, self.gamma, self.y, self.part, self.pre, self.dt, self.kernel, self.psolve = op, t, gamma, y, part, precondition, dt, kernel, psolve
        self.fma = jr._fma(dt) if kernel else None
        self.precision = "f64" if dt in (np.float64, np.longdouble) and not (kernel and dt == np.float32) else "f32"

    def J(self, x):
        y = np.zeros(x.shape) if self.y is None else self.y
        if self.kernel:
            return jr.kernel_order_jtimes(self.op, self.t, y.astype(self.dt), x, self.dt, self.part)
        if self.part == jr.DIFFUSION:
            jx = (x[..., 0] - mg.operator(self.op, self.t, 1.0, x[..., 0], dtype=self.dt)).astype(self.dt)  # I - (I - J_D)
            return np.stack([jx, np.zeros_like(jx)], axis=-1)
        return jr.jtimes_bound(self.op, self.t, y, x, "f64" if self.dt == np.longdouble else "f32", self.part)[0].astype(self.dt)

    def A(self, x):
        if self.kernel:
            return self.fma(self.dt(-self.gamma), self.J(x), x)
        if self.part == jr.DIFFUSION:
            return np.stack([mg.operator(self.op, self.t, self.gamma, x[..., 0], dtype=self.dt), x[..., 1]], axis=-1)
        return x - self.dt(self.gamma) * self.J(x)

    def M(self, x):
        if not self.pre:
            return x
        if self.kernel:
            return mg.kernel_order_vcycle(self.op, self.t, self.gamma, x, self.dt, **self.psolve)
        return np.stack([mg.reference_vcycle(self.op, self.t, self.gamma, x[..., 0], dtype=self.dt, **self.psolve), x[..., 1]], axis=-1)


class ReferenceOps(_Operators):
    def __init__(self, op, t, gamma, y, part, precondition, dt, psolve):
        super().__init__(op, t, gamma, y, part, precondition, dt, False, psolve)
        self.ls_dtype = dt

    def dots(self, V, w):
        return np.array([np.sum(v * w) for v in V], dtype=self.dt)

    def update(self, V, h, w):
        for hi, v in zip(h, V):
            w = w - hi * v
        return w, np.sum(w * w)

    def scale(self, w, norm2):
        return w / np.sqrt(norm2)

    def combine(self, V, y):
        return sum(yi * v for yi, v in zip(y, V))

    def add(self, z, d):
        return z + d

    def sub(self, r, a):
        return r - a


class KernelOps(_Operators):
    def __init__(self, op, t, gamma, y, part, precondition, R, psolve, mutant=None):
        super().__init__(op, t, gamma, y, part, precondition, R, True, psolve)
        self.ls_dtype, self.mutant = np.float64, mutant if mutant in DOT_MUTANTS else None

    def dots(self, V, w):
        return kernel_order_sums(np.array([v.ravel() for v in V], dtype=np.float64), w.ravel().astype(np.float64), self.mutant)

    def update(self, V, h, w):
        a = w.astype(np.float64)
        for hi, v in zip(h, V):
            a = _fma64(-hi, v.astype(np.float64), a)
        o = a.astype(self.dt)
        f = o.ravel().astype(np.float64)
        return o, kernel_order_sums(f[None, :], f)[0]

    def scale(self, w, norm2):
        return (w.astype(np.float64) / np.sqrt(norm2)).astype(self.dt)

    def combine(self, V, y):
        a = np.zeros(V[0].shape)
        for yi, v in zip(y, V):
            a = _fma64(yi, v.astype(np.float64), a)
        return a.astype(self.dt)

    def add(self, z, d):
        return z + d

    def sub(self, r, a):
        return r - a


DEFAULTS = dict(part=jr.DIFFUSION, precondition=True, restart=30, max_iters=200, rtol=1e-8, atol=0.0)


def _options(kw):
    o = dict(DEFAULTS)
    psolve = {k: kw.pop(k) for k in list(kw) if k in mg.DEFAULTS}
    for k, v in kw.items():
        assert k in o, k
        o[k] = v
    return o, psolve


def reference_solve(op, t, gamma, r, precision, y=None, **kw):
    """Result of the solve in the reference's dtype; z (ny, nx, 2)."""
    o, psolve = _options(kw)
    rd = eb.reference_dtype(precision)
    ops = ReferenceOps(op, t, gamma, y, o["part"], o["precondition"], rd, psolve)
    return gmres(ops, np.asarray(r).astype(rd), gamma, o["part"] == jr.DIFFUSION, o["restart"], o["max_iters"], o["rtol"], o["atol"], UNIT[precision])


def kernel_order_solve(op, t, gamma, r, R, y=None, mutant=None, **kw):
    """Result of the solve in the device precision R in the kernels' order; mutant: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS, mutant
    o, psolve = _options(kw)
    ops = KernelOps(op, t, gamma, y, o["part"], o["precondition"], R, psolve, mutant)
    precision = "f64" if R == np.float64 else "f32"
    return gmres(ops, np.asarray(r).astype(R), gamma, o["part"] == jr.DIFFUSION, o["restart"], o["max_iters"], o["rtol"], o["atol"], UNIT[precision], mutant)


def tolerance_between(history, r_norm, floor=0.0, near=1e-8):
    """(rtol, iterations): rtol the geometric mean of two successive entries of a single cycle's residual history (relative to ||r||) whose
    ratio is at least 4, both >= floor ||r||, the pair nearest `near`; iterations the count at which the estimate first falls below it.
    None when no such pair exists."""
    rel = np.asarray(history, dtype=np.float64) / r_norm
    best = None
    for k in range(1, len(rel)):
        if rel[k] > 0 and rel[k] >= floor and rel[k - 1] / rel[k] >= 4:
            mid = float(np.sqrt(rel[k - 1] * rel[k]))
            if best is None or abs(np.log(mid / near)) < abs(np.log(best[0] / near)):
                best = (mid, k)
    return best


def residual_allowance(op, t, gamma, y, z, r, precision, part, rtol, atol=0.0):
    """(||r - (z - gamma J z)|| under the reference operator, what it may be): the module docstring's allowance."""
    rd, u = eb.reference_dtype(precision), UNIT[precision]
    y = np.zeros(np.shape(z)) if y is None else y
    jz, bu, bv = jr.jtimes_bound(op, t, y, z, precision, part)
    residual = (np.asarray(z).astype(rd) - rd(gamma) * jz) - np.asarray(r).astype(rd)
    rounding = gamma * np.stack([bu, bv], -1) + 2 * u * (np.abs(np.asarray(z, dtype=np.float64)) + gamma * np.abs(jz.astype(np.float64)))
    r64 = np.asarray(r, dtype=np.float64)
    return float(np.linalg.norm(residual.astype(np.float64))), rtol * float(np.linalg.norm(r64)) + atol + float(np.linalg.norm(rounding))


def orthogonality_allowance(columns, n, precision):
    return 2 * (dot_roundings(n) * U64 + (columns + 3) * UNIT[precision])


def orthogonality(basis):
    """max |<V_i, V_j> - delta_ij| in long double."""
    Q = np.array([v.ravel() for v in basis]).astype(np.longdouble)
    return float(np.abs(Q @ Q.T - np.eye(len(basis))).max())


def selftest_build_command(exe, sanitizers=None):
    """g++ command line of tests/native/krylov_host_selftest.cpp (plain C++17 against crd_krylov_host.h, nothing of HIP)."""
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(root, "crdmodel_amd", "csrc"), os.path.join(root, "tests", "native", "krylov_host_selftest.cpp"),
           "-o", str(exe)]
    if sanitizers:
        cmd[4:4] = ["-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizers, "-fno-sanitize-recover=all"]
    return cmd
