"""Reference, kernel-order restatement and bounds of the BiCGStab solve (I - gamma J_part(t, y)) z = r on the device (crd_bicgstab_*,
crdmodel_amd/csrc/crd_bicgstab.cpp / crd_bicgstab.hip / crd_bicgstab_host.h).  TEST INFRASTRUCTURE ONLY.

The algorithm (include/crd.h states it; this module restates it twice through one driver, `bicgstab`)
----------------------------------------------------------------------------------------------------
x = 0, res = r (var1 masked for DIFFUSION) -- or x = the guess, res = r - A x --, rhat = p = res, rho = <rhat, res>; per iteration:
phat = M p; v = A phat; alpha = rho / <rhat, v>; s = res - alpha v; ||s|| <= tol: x += alpha phat, half exit; shat = M s; t = A shat;
omega = <t, s> / <t, t>; x += alpha phat + omega shat; res = s - omega t; ||res|| <= tol: done; beta = (rho' / rho)(alpha / omega);
p = res + beta (p - omega v).  tol = rtol ||r|| + atol.  The scalar decisions are `Recurrence`, the restatement of crd_bicgstab_host.h.
`history` is interleaved: ||res_0||, ||s_1||, ||res_1||, ||s_2||, ...

Reference (reference_solve): the driver in error_bounds.reference_dtype(precision) -- np.longdouble for the fp64 kernels, float64 on the
exactly widened vectors for the fp32 kernels -- with krylov_reference.ReferenceOps' A and M; scalars are not rounded.

Kernel order (kernel_order_solve): the driver in the device precision with krylov_reference.KernelOps' A = fma(-gamma, J x, x) and M, every
vector update an imex_reference.fma_exact composition as the kernels spell it, the scalars rounded once to the device precision, and the
reductions in the kernels' own summation order (kernel_order_sum).

The sums' tree and its bound (sum_roundings, sum_bound)
-------------------------------------------------------
A vector of n reals is U = ceil(n / P) units of 16 bytes, P = 2 reals (fp64) or 4 (fp32); G = min(2048, ceil(U / 256)) blocks of 256
threads; accumulators double in both precisions:
  thread   unit q = block 256 + thread + k (256 G), k = 0 .. trips - 1, trips = ceil(U / (256 G)): a chain acc = fma(a[e], b[e], acc)
           over the unit's P reals in order, then the next trip's.  The first term passes through trips x P roundings.
  wave     six shuffle steps, lane l += lane l + off, off = 32 .. 1: 6 additions.
  block    ((p0 + p1) + p2) + p3 over the four wavefronts: 3 additions.
  final    one wavefront per sum: lane l adds partials l, l + 64, ... in order -- ceil(G / 64) additions -- then six shuffle steps.
K = trips P + 6 + 3 + ceil(G / 64) + 6, and |sum - exact| <= gamma_K sum |a b|, gamma_K = K u64 / (1 - K u64) (Higham, Accuracy and
Stability of Numerical Algorithms, 4.2).  19 x 27 (n = 1026): fp64 U = 513, G = 3, K = 2 + 15 + 1 = 18; fp32 U = 257, G = 2, K = 20.
"""
import os

import numpy as np

import imex_reference as ir
import jacobian_reference as jr
import krylov_reference as kr
from oracle import error_bounds as eb
from oracle.error_bounds import UNIT

THREADS, BLOCKS = 256, 2048  # crd_bicgstab.h: kBcgThreads, kBcgBlocks
REALS = {"f64": 2, "f32": 4}  # reals in a thread's 16 bytes
DTYPES = kr.DTYPES
U64 = 2.0 ** -53
NONE, D, TT, OMEGA, RHO = 0, 1, 2, 3, 4  # CRD_BICGSTAB_BREAKDOWN_*
SUM_MUTANTS = ("last_element", "tail_block", "first_trip")
SOLVE_MUTANTS = ("x_without_omega", "half_exit_without_x", "beta_without_ratio", "p_without_v", "omega_over_ss", "var1_unmasked")
MUTANTS = SUM_MUTANTS + SOLVE_MUTANTS
# (var1_unmasked: the diffusion part without its var1 handling -- no mask on res, v and t, no z_var1 = r_var1 at the end: var1 is then
# iterated on like var0, and comes out near r_var1 instead of equal to it)
# the gate that claims each mutant
MUTANT_GATES = dict({m: "sums" for m in SUM_MUTANTS}, x_without_omega="true_residual", half_exit_without_x="true_residual", beta_without_ratio="count",
                    p_without_v="count", omega_over_ss="count", var1_unmasked="var1")


def units(n, precision):
    return -(-n // REALS[precision])


def grid(n, precision):
    return min(BLOCKS, max(1, -(-units(n, precision) // THREADS)))


def trips(n, precision):
    return -(-units(n, precision) // (grid(n, precision) * THREADS))


def sum_roundings(n, precision):
    """K of the module docstring."""
    return trips(n, precision) * REALS[precision] + 6 + 3 + -(-grid(n, precision) // 64) + 6


def sum_bound(a, b, precision):
    """(ref, bound, size) of <a, b>: ref in long double, size = sum |a b|."""
    L = np.longdouble
    prod = np.asarray(a).ravel().astype(L) * np.asarray(b).ravel().astype(L)
    size = float(np.abs(prod).sum())
    K = sum_roundings(prod.size, precision)
    return prod.sum(), K * U64 / (1 - K * U64) * size, size


_fma64 = ir.fma_exact(np.float64)


def kernel_order_sum(a, b, precision, mutant=None):
    """<a, b> in the kernels' order (module docstring): a, b of the device precision, any shape; the result a float64."""
    assert mutant is None or mutant in SUM_MUTANTS, mutant
    a, b = np.array(a, dtype=np.float64).ravel(), np.array(b, dtype=np.float64).ravel()
    n, P = a.size, REALS[precision]
    G, T = grid(n, precision), trips(n, precision)
    if mutant == "last_element":
        a[n - 1] = 0
    pad = T * G * THREADS * P - n
    A = np.pad(a, (0, pad)).reshape(T, G, THREADS // 64, 64, P)
    B = np.pad(b, (0, pad)).reshape(T, G, THREADS // 64, 64, P)
    acc = np.zeros((G, THREADS // 64, 64))
    for k in range(1 if mutant == "first_trip" else T):
        for e in range(P):
            acc = _fma64(A[k, ..., e], B[k, ..., e], acc)
    p = kr._wave(acc)
    partials = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
    if mutant == "tail_block":
        partials[G - 1] = 0
    rows = -(-G // 64)
    Pm = np.pad(partials, (0, rows * 64 - G)).reshape(rows, 64)
    lane = np.zeros(64)
    for k in range(rows):
        lane = lane + Pm[k]
    return float(kr._wave(lane))


def plant_positions(n, precision):
    """Real indices: 0; the last of a wavefront and the first of the next; the last of a block and the first of the next; the last real
    of the first grid-stride trip and the first of the second (where the vector has a second); n - 1.  var0 (even) and var1 (odd) both
    occur."""
    P = REALS[precision]
    first = grid(n, precision) * THREADS * P
    p = [0, 64 * P - 1, 64 * P, THREADS * P - 1, THREADS * P] + ([first - 1, first] if n > first else []) + [n - 1]
    return [q for q in p if q < n]


def smallest_grid_above_one_trip(precision):
    """(nx, ny) of the smallest grid 1030 wide whose vector takes a second grid-stride trip (1030: the last block is ragged)."""
    points = BLOCKS * THREADS * REALS[precision] // 2
    return 1030, points // 1030 + 1


# ---- the scalar recurrences (crd_bicgstab_host.h: Recurrence) ---------------------------------------------------------------------
class Recurrence:
    """dtype float64 with f32 = True / False restates the header bit for bit; dtype longdouble (round nothing) is the reference's."""

    def __init__(self, tol, max_iters, f32=False, dtype=np.float64, mutant=None):
        self.tol, self.max_iters, self.f32, self.dt, self.mutant = dtype(tol), max_iters, f32, dtype, mutant
        z = dtype(0)
        self.rho, self.alpha, self.omega, self.beta, self.res_norm = z, z, z, z, z
        self.iterations = self.half_exit = self.breakdown = self.converged = 0

    def rounded(self, x):
        return self.dt(np.float32(x)) if self.f32 else self.dt(x)

    @staticmethod
    def usable(x):
        return bool(np.isfinite(x)) and x != 0

    def start(self, res_sq):
        res_sq = self.dt(res_sq)
        with np.errstate(all="ignore"):
            self.rho, self.res_norm = res_sq, np.sqrt(res_sq)
        if not np.isfinite(res_sq):
            return False
        if self.res_norm <= self.tol:
            self.converged = 1
            return False
        return self.max_iters > 0

    def take_d(self, d):
        d = self.dt(d)
        with np.errstate(all="ignore"):
            if self.usable(d):
                self.alpha = self.rounded(self.rho / d)
        if not self.usable(d) or not self.usable(self.alpha):
            self.breakdown = D
            return False
        return True

    def take_s(self, s_sq):
        with np.errstate(all="ignore"):
            self.res_norm = np.sqrt(self.dt(s_sq))
        if self.res_norm <= self.tol:
            self.converged, self.half_exit = 1, 1
            self.iterations += 1
            return False
        return True

    def take_t(self, ts, tt):
        ts, tt = self.dt(ts), self.dt(tt)
        if not self.usable(tt):
            self.breakdown = TT
        else:
            with np.errstate(all="ignore"):
                self.omega = self.rounded(ts / tt)
            if not self.usable(self.omega):
                self.breakdown = OMEGA
        if self.breakdown != NONE:
            self.half_exit = 1
            self.iterations += 1
            return False
        return True

    def take_res(self, res_sq, rho_new):
        rho_new = self.dt(rho_new)
        self.iterations += 1
        with np.errstate(all="ignore"):
            self.res_norm = np.sqrt(self.dt(res_sq))
        if self.res_norm <= self.tol:
            self.converged = 1
            return False
        if self.iterations >= self.max_iters:
            return False
        with np.errstate(all="ignore"):
            if self.usable(rho_new):
                ratio = self.dt(1) if self.mutant == "beta_without_ratio" else self.alpha / self.omega
                self.beta = self.rounded((rho_new / self.rho) * ratio)
        if not self.usable(rho_new) or not np.isfinite(self.beta):
            self.breakdown = RHO
            return False
        self.rho = rho_new
        return True


class Result:
    def __init__(self):
        self.converged = self.iterations = self.half_exit = self.matvecs = self.psolves = self.breakdown = 0
        self.r_norm = self.res_norm = self.true_res_norm = 0.0
        self.history, self.z, self.coefficients = [], None, []


# ---- one driver, two sets of operations -------------------------------------------------------------------------------------------
class _Arithmetic:
    """fma(a, x, y) = a x + y elementwise, dot(a, b), and the operators A, J, M of krylov_reference."""

    def __init__(self, ops, kernel, precision, mutant=None):
        self.ops, self.kernel, self.precision = ops, kernel, precision
        self.sum_mutant = mutant if mutant in SUM_MUTANTS else None
        self._fma = ir.fma_exact(DTYPES[precision]) if kernel else None

    def fma(self, a, x, y):
        if self.kernel:
            return self._fma(DTYPES[self.precision](a), x, y).astype(DTYPES[self.precision]).reshape(np.shape(x))
        return a * x + y

    def dot(self, a, b):
        if self.kernel:
            return kernel_order_sum(a, b, self.precision, self.sum_mutant)
        return np.sum(a * b)

    def A(self, x):
        if self.kernel:  # fma(-gamma, J x, x), as the apply-dot kernel spells it
            return self.fma(-self.ops.gamma, self.ops.J(x), x)
        return self.ops.A(x)

    def M(self, x):
        return self.ops.M(x)


def bicgstab(ar, r, gamma, diffusion, max_iters, rtol, atol, guess=None, mutant=None):
    """The algorithm of the module docstring on AoS arrays (ny, nx, 2); ar an _Arithmetic.  Returns a Result."""
    out = Result()
    kernel = ar.kernel
    dt = np.float64 if kernel else r.dtype.type
    mask = (lambda x: np.stack([x[..., 0], np.zeros_like(x[..., 1])], axis=-1)) if diffusion and mutant != "var1_unmasked" else (lambda x: x)
    with np.errstate(all="ignore"):
        out.r_norm = float(np.sqrt(ar.dot(r, r)))
    if gamma == 0:
        out.z, out.converged = r.copy(), 1
        return out
    if out.r_norm == 0:
        out.z, out.converged = np.zeros_like(r), 1
        return out
    if guess is None:
        x, res = np.zeros_like(r), mask(r)
    else:
        x = guess.astype(r.dtype)
        res = mask(r - ar.A(x))
        out.matvecs += 1
    rhat, p = res.copy(), res.copy()
    res_sq = ar.dot(res, res)
    with np.errstate(all="ignore"):
        out.res_norm = out.true_res_norm = float(np.sqrt(res_sq))
    if not np.isfinite(out.r_norm):
        out.z = np.stack([x[..., 0], r[..., 1]], axis=-1) if diffusion else x
        return out
    k = Recurrence(dt(rtol) * dt(out.r_norm) + dt(atol), max_iters, f32=kernel and ar.precision == "f32", dtype=dt, mutant=mutant)
    go = k.start(res_sq)
    out.history.append(float(k.res_norm))

    def precondition(v):
        if ar.ops.pre:
            out.psolves += 1
        return ar.M(v)

    while go:
        phat = precondition(p)
        v = mask(ar.A(phat))
        out.matvecs += 1
        if not k.take_d(ar.dot(rhat, v)):
            break
        s = ar.fma(-k.alpha, v, res)
        half = not k.take_s(ar.dot(s, s))
        out.history.append(float(k.res_norm))
        if half:
            if mutant != "half_exit_without_x":
                x = ar.fma(k.alpha, phat, x)
            break
        shat = precondition(s)
        t = mask(ar.A(shat))
        out.matvecs += 1
        ts, tt = ar.dot(t, s), ar.dot(t, t)
        if not k.take_t(ts, ar.dot(s, s) if mutant == "omega_over_ss" else tt):
            x = ar.fma(k.alpha, phat, x)
            break
        x = ar.fma(k.alpha, phat, x)
        if mutant != "x_without_omega":
            x = ar.fma(k.omega, shat, x)
        res = ar.fma(-k.omega, t, s)
        go = k.take_res(ar.dot(res, res), ar.dot(rhat, res))
        out.history.append(float(k.res_norm))
        out.coefficients.append((float(k.alpha), float(k.omega), float(k.beta) if go else None))
        if go:
            p = ar.fma(k.beta, p if mutant == "p_without_v" else ar.fma(-k.omega, v, p), res)
    out.converged, out.iterations, out.half_exit, out.breakdown, out.res_norm = k.converged, k.iterations, k.half_exit, k.breakdown, float(k.res_norm)
    if diffusion and mutant != "var1_unmasked":
        x = np.stack([x[..., 0], r[..., 1]], axis=-1)
    true = mask(r - ar.A(x))
    out.matvecs += 1
    out.true_res_norm = float(np.sqrt(ar.dot(true, true)))
    out.z = x
    return out


DEFAULTS = dict(part=jr.DIFFUSION, precondition=True, max_iters=200, rtol=1e-8, atol=0.0)


def _options(kw):
    o = dict(DEFAULTS)
    psolve = {k: kw.pop(k) for k in list(kw) if k in kr.mg.DEFAULTS}
    for k, v in kw.items():
        assert k in o, k
        o[k] = v
    return o, psolve


def reference_solve(op, t, gamma, r, precision, y=None, guess=None, mutant=None, **kw):
    """Result of the solve in the reference's dtype; z (ny, nx, 2)."""
    o, psolve = _options(kw)
    rd = eb.reference_dtype(precision)
    ops = kr.ReferenceOps(op, t, gamma, y, o["part"], o["precondition"], rd, psolve)
    g = None if guess is None else np.asarray(guess).astype(rd)
    return bicgstab(_Arithmetic(ops, False, precision), np.asarray(r).astype(rd), rd(gamma), o["part"] == jr.DIFFUSION, o["max_iters"], o["rtol"], o["atol"], g, mutant)


def kernel_order_solve(op, t, gamma, r, precision, y=None, guess=None, mutant=None, **kw):
    """Result of the solve in the device precision in the kernels' order; mutant: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS, mutant
    o, psolve = _options(kw)
    R = DTYPES[precision]
    ops = kr.KernelOps(op, t, float(R(gamma)), y, o["part"], o["precondition"], R, psolve)
    g = None if guess is None else np.asarray(guess).astype(R)
    return bicgstab(_Arithmetic(ops, True, precision, mutant), np.asarray(r).astype(R), float(R(gamma)), o["part"] == jr.DIFFUSION, o["max_iters"], o["rtol"], o["atol"], g, mutant)


def half_steps(result):
    """Where the solve stopped, in half-steps: 2 iterations, less one for a half exit."""
    return 2 * result.iterations - result.half_exit


def implied_counts(iterations, half_exit, precondition=True, guess=False):
    """(matvecs, psolves) the algorithm implies: two of each per full iteration, one for a half exit, one matvec for a guess and one
    for the true residual."""
    halves = 2 * iterations - half_exit
    return halves + 1 + int(guess), halves if precondition else 0


def selftest_build_command(exe, sanitizers=None):
    """g++ command line of tests/native/bicgstab_host_selftest.cpp (plain C++17 against crd_bicgstab_host.h, nothing of HIP)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(root, "crdmodel_amd", "csrc"), os.path.join(root, "tests", "native", "bicgstab_host_selftest.cpp"),
           "-o", str(exe)]
    if sanitizers:
        cmd[4:4] = ["-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizers, "-fno-sanitize-recover=all"]
    return cmd


# ---- each fused kernel alone (crd_bicgstab_probe) -----------------------------------------------------------------------------------
# kernel -> (inputs, scalars, outputs, sums)
KERNELS = {"apply_dot": (3, 1, 1, 1), "apply_dot2": (3, 1, 1, 2), "s_update": (2, 1, 1, 1), "xr_update": (6, 2, 2, 2), "p_update": (3, 2, 1, 0), "x_half": (2, 1, 1, 0)}
SCALARS = {"apply_dot": (0.37,), "apply_dot2": (0.37,), "s_update": (0.81,), "xr_update": (0.81, 0.43), "p_update": (-0.29, 0.43), "x_half": (0.81,)}


def kernel_reference(kernel, ins, scalars, precision, var0_only=False):
    """(outs, pairs) of one fused kernel as the fma_exact composition crd_bicgstab.hip spells: ins flat vectors of the device precision,
    scalars rounded once to it; pairs the (a, b) whose dot each sum of the kernel is, over the STORED outputs."""
    R = DTYPES[precision]
    fma = ir.fma_exact(R)
    f = lambda a, x, y: fma(R(a), x, y).astype(R)
    c = [R(s) for s in scalars]
    if kernel in ("apply_dot", "apply_dot2"):
        jv, x, b = ins
        out = f(-c[0], jv, x)
        if var0_only:
            out[1::2] = 0
        return [out], ([(b, out)] if kernel == "apply_dot" else [(out, b), (out, out)])
    if kernel == "s_update":
        v, res = ins
        s = f(-c[0], v, res)
        return [s], [(s, s)]
    if kernel == "xr_update":
        x, phat, shat, t, s, rhat = ins
        xn = f(c[1], shat, f(c[0], phat, x))
        rn = f(-c[1], t, s)
        return [xn, rn], [(rn, rn), (rhat, rn)]
    if kernel == "p_update":
        p, v, res = ins
        return [f(c[0], f(-c[1], v, p), res)], []
    x, phat = ins
    return [f(c[0], phat, x)], []


def sum_pairs(kernel, ins, outs):
    """The (a, b) whose dot each sum of `kernel` is, from its inputs and its STORED outputs (the device's own, for instance)."""
    if kernel == "apply_dot":
        return [(ins[2], outs[0])]
    if kernel == "apply_dot2":
        return [(outs[0], ins[2]), (outs[0], outs[0])]
    if kernel == "s_update":
        return [(outs[0], outs[0])]
    if kernel == "xr_update":
        return [(outs[1], outs[1]), (ins[5], outs[1])]
    return []


def planted_case(kernel, n, precision, q1, q2, seed=7):
    """Inputs of one kernel: noise of size 1e-4 and planted elements so that ONE element carries each sum -- the first sum at real q1,
    the second (where the kernel leaves two) at q2 != q1: the vector the output starts from is 1 at q1 and 4 at q2, the vector the
    first sum pairs it with is 1 at q1."""
    R = DTYPES[precision]
    n_in = KERNELS[kernel][0]
    rng = np.random.default_rng(seed)
    ins = [(1e-4 * rng.standard_normal(n)).astype(R) for _ in range(n_in)]
    base, pair = {"apply_dot": (1, 2), "apply_dot2": (1, 2), "s_update": (1, None), "xr_update": (4, 5), "p_update": (2, None), "x_half": (0, None)}[kernel]
    ins[base][q1] = 1
    if pair is not None:
        ins[pair][q1] = 1
    if KERNELS[kernel][3] == 2:
        ins[base][q2] = 4
    return ins


def carriers(kernel, q1, q2):
    """The real that carries each sum of planted_case's inputs, in the order the kernel leaves its sums."""
    return {"apply_dot": [q1], "apply_dot2": [q1, q2], "s_update": [q1], "xr_update": [q2, q1]}.get(kernel, [])


def sums_gate(got, pairs, precision):
    """Largest |sum - ref| / bound over a kernel's sums (0 where it leaves none)."""
    worst = 0.0
    for g, (a, b) in zip(got, pairs):
        ref, bound, _ = sum_bound(a, b, precision)
        worst = max(worst, float(abs(np.longdouble(g) - ref)) / bound)
    return worst


# ---- the IMEX step composed from the public calls (crd_step_imex with CRD_IMEX_SOLVER_BICGSTAB / _WARM) -----------------------------
def composed_steps(slab, scheme, t0, dt, nsteps, y, warm=False, **solve_options):
    """(y_new, [bicgstab stats]) of nsteps steps as a loop over Slab.rhs_part, Slab.lsolve_bicgstab and imex_reference.fma_exact in the
    slab's precision -- imex_reference.composed_step with the other solver.  warm: every solve starts from the k of the solve before
    (the first of the call from zero).  y_new is None behind a solve that did not converge."""
    R_ = slab.dtype
    fma = ir.fma_exact(R_)
    s, c, AE, AI, g = ir.tableau(scheme)
    hg = R_(dt * g)
    y = np.ascontiguousarray(y, dtype=R_)
    stats, last_k = [], None
    for n in range(nsteps):
        t = t0 + n * dt
        FR, k = [slab.rhs_part(t, y, "reaction")], [None]
        R = fma(R_(dt * AE[1][0]), FR[0], y)
        for i in range(1, s + 1):
            ti = t + c[i] * dt
            r = slab.rhs_part(ti, R, "diffusion")
            ki, st = slab.lsolve_bicgstab(ti, float(hg), r, guess=last_k if warm else None, **solve_options)
            stats.append(st)
            if not st.converged:
                return None, stats
            k.append(ki)
            last_k = ki
            Y = fma(hg, ki, R)
            if i == s:
                y = np.ascontiguousarray(Y, dtype=R_)
                break
            FR.append(slab.rhs_part(ti, Y, "reaction"))
            R = y
            for j, which, coef in ir.row_terms(scheme, i + 1, dt, R_):
                R = fma(coef, FR[j] if which == "E" else k[j], R)
    return y, stats


def kernel_order_imex_steps(op, scheme, t0, dt, nsteps, y, precision, warm=False, **solve_options):
    """(y_new, [Result]) of nsteps IMEX steps on the CPU in the device precision: jacobian_reference.kernel_order_part for f_D and f_R,
    kernel_order_solve for every stage (warm: from the k of the solve before), imex_reference.fma_exact between them -- composed_steps
    without a device."""
    R_ = DTYPES[precision]
    fma = ir.fma_exact(R_)
    s, c, AE, AI, g = ir.tableau(scheme)
    hg = R_(dt * g)
    y = np.ascontiguousarray(y, dtype=R_)
    results, last_k = [], None
    for n in range(nsteps):
        t = t0 + n * dt
        FR, k = [jr.kernel_order_part(op, t, y, R_, jr.REACTION)], [None]
        R = fma(R_(dt * AE[1][0]), FR[0], y).astype(R_)
        for i in range(1, s + 1):
            ti = t + c[i] * dt
            r = jr.kernel_order_part(op, ti, R, R_, jr.DIFFUSION)
            res = kernel_order_solve(op, ti, float(hg), r, precision, guess=last_k if warm else None, **solve_options)
            results.append(res)
            assert res.converged, (n, i, res.iterations, res.breakdown)
            k.append(res.z)
            last_k = res.z
            Y = fma(hg, res.z, R).astype(R_)
            if i == s:
                y = Y
                break
            FR.append(jr.kernel_order_part(op, ti, Y, R_, jr.REACTION))
            R = y
            for j, which, coef in ir.row_terms(scheme, i + 1, dt, R_):
                R = fma(coef, FR[j] if which == "E" else k[j], R).astype(R_)
    return y, results
