"""Reference, kernel-order restatement and per-point rounding-error bound of the preconditioner solve z = M r, M one geometric
multigrid V-cycle for P = I - gamma J_D(t) on var0 (crd_psolve_*, crdmodel_amd/csrc/crd_multigrid.hip).  TEST INFRASTRUCTURE ONLY.

The cycle (include/crd.h states it; this module restates it twice)
-------------------------------------------------------------------
Level l: L x (j, i) = cE[i] (x[j, i+1] - x[j, i]) + cWn[i] (x[j, i] - x[j, i-1]) + cP[i] (x[j+1, i] - 2 x[j, i] + x[j-1, i]), periodic in both
directions, zero rows at held rows; A = I - gamma L; d[i] = 1 + gamma (2 cX + 2 cP[i]).  Level 0 is the problem's grid and tables; level
l + 1 exists while nx_l and ny_l are both even and both halves are >= 4, up to max_levels; coarse (J, I) is fine (2 J, 2 I); coarse tables
cX / 4, cA[2 I] / 2, cP[2 I] / 4.  Held rows (t < tBoundary strictly, never for just_diffusion): rows 0 and ny - 1 of level 0, row 0 of
every coarser level.  Sweep: z <- z + omega (r - (z - gamma L z)) / d from the old z, then z = r on held rows.  Cycle: the coarsest
level takes `coarse` sweeps from z = 0 (a single-level cycle is therefore `coarse` sweeps); any other level `pre` sweeps from z = 0,
s = r - A z, full weighting 1/16 [1 2 1; 2 4 2; 1 2 1] of s, 0 on the coarse held row, the cycle below, bilinear prolongation,
0 on this level's held rows, z += correction, `post` sweeps.  var1 of z is var1 of r.

Reference: reference_vcycle / vcycle_bound evaluate that in error_bounds.reference_dtype(precision) -- np.longdouble for the fp64
kernels, float64 on the exactly widened vector for the fp32 kernels -- with the host's fp64 tables.

Kernel order: kernel_order_vcycle evaluates it in the device precision R, operation by operation as crd_multigrid.hip does, fused
multiply-adds emulated by jacobian_reference._fma, tables and gamma, omega, 2 cX rounded once to R:
    w    = omega / fma(gamma, fma(2, cP, 2cX), 1)
    A z  = fma(-gamma, fma(cWn, z - zW, fma(cE, zE - z, cP (fma(-2, z, zN) + zS))), z)          (a held row: z)
    sweep: from z = 0 w r, else fma(w, r - A z, z); held rows r
    restriction of s = r - A z: 0.0625 fma(4, s, fma(2, (sW + sE) + (sS + sN), (sSW + sSE) + (sNW + sNE)))
    prolongation: 0.25 ((e[J, I] + e[J, I']) + (e[J', I] + e[J', I'])), I' = I + (i odd), J' = J + (j odd), wrapped; z + that.

Bound (vcycle_bound)
--------------------
An error field E is carried through the reference cycle beside the values: a bound on |kernel value - reference value| per point.
With u the unit roundoff of the device precision, every operation adds  k u (sum of the magnitudes of its terms)  with k the number of
roundings the term that passes through most of them meets in the kernel's sequence, and every linear operator passes the incoming
field on with the magnitudes of its coefficients.

  sweep      T = |r| + |z| + gamma S_L,  S_L = |cE gE| + |cWn gW| + cP (|zN| + 2 |z| + |zS|)  (jacobian_reference._diffusion_sizes).
             On the way to the final fused multiply-add the phi term meets: d2y 2, the rounded cP, its product, the two fused
             multiply-adds of L, the rounded gamma, A z's fused multiply-add, the subtraction from r: 9; then w's 7 (cP, 2cX, gamma
             and omega rounded, two fused multiply-adds of positive terms, the quotient): 16.  K_SWEEP = 17 leaves one spare:
                 local = u (|z| + w T) + K_SWEEP u w T          (the first term: the final fused multiply-add's own rounding)
             From z = 0 the same expression covers w r (8 roundings).  Propagation, with M = I - w A the Jacobi matrix:
                 E' = (1 - omega) E + w gamma (|cE| E_E + |cWn| E_W + cP (E_N + E_S)) + w E_r + local;   held rows E' = E_r exactly.
             Its row sums are 1 - omega / d < 1 because cE > 0 > cWn: a sweep does not amplify E.
  residual   s = r - A z: the phi term meets 9 roundings, K_RES = 10:  local = K_RES u T;
                 E_s = E_r + d E + gamma (|cE| E_E + |cWn| E_W + cP (E_N + E_S)) + local;   held rows: u (|r| + |z|) + E_r + E.
             This is the one operator of norm above 1 (about 2 d): a coarse sweep's w E_r undoes it, since d_coarse is about d / 4.
  restrict   edge and corner terms meet two additions and two fused multiply-adds: local = 4 u R(|s|), E_rc = R(E_s) + local, R the
             full weighting (non-negative weights of sum 1: no amplification); the coarse held row is exactly 0.
  prolong    two additions inside the mean (the factor 0.25 is exact) and the correction's own:
                 local = 3 u P(|e|) + u |z|,  E' = E + P(E_e) + local, P the bilinear interpolation (weights of sum 1); held rows keep E.
  var1       bit for bit r's: bound 0.
The reference's own error (2^-64 or 2^-53 of the same terms) is ignored, as in error_bounds.  `unit` overrides u: with 2^-64 the
same fields bound the long-double reference's own rounding (the symmetry test of tests/test_multigrid_host.py).
"""
import numpy as np

import jacobian_reference as jr
from oracle import error_bounds as eb
from oracle.error_bounds import UNIT

DEFAULTS = dict(pre=2, post=2, coarse=8, max_levels=16, omega=0.8)
K_SWEEP = 17.0
K_RES = 10.0
MUTANTS = ("seam", "injection", "prolong_row", "coarse_held_rhs", "cA4", "coarse_rowN")


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in o, k
        o[k] = v
    return o


def level_shapes(nx, ny, max_levels=16):
    """[(nx, ny)] per level."""
    out = [(nx, ny)]
    while len(out) < max_levels and nx % 2 == 0 and ny % 2 == 0 and nx // 2 >= 4 and ny // 2 >= 4:
        nx, ny = nx // 2, ny // 2
        out.append((nx, ny))
    return out


def host_coefficients(op):
    """(cX, cA[nx], cP[nx]) in float64 as crd_host.cpp: build_coefficients forms them (error_bounds._Problem's formulas)."""
    D, dx, dy = op.diff, op.dx, op.dy
    P = eb._Problem(op)
    if P.surface == "torus":
        theta = op.xmin + np.arange(op.nx, dtype=np.float64) * dx
        rho = op.R + op.r * np.cos(theta)
        return D * (1 / (op.r * op.r)) / (dx * dx), D * (-np.sin(theta) / (op.r * rho)) / (2 * dx), D * (1 / (rho * rho)) / (dy * dy)
    return D / dx / dx, np.zeros(op.nx), np.full(op.nx, D / dy / dy)


class Level:
    def __init__(self, nx, ny, cX, cA, cP, held):
        self.nx, self.ny, self.cX, self.cA, self.cP = nx, ny, cX, cA, cP
        self.cE, self.cWn = cX + cA, cA - cX  # in double, as the host forms them
        self.held = held  # bool per row


def build_levels(op, t, max_levels=16, mutant=None):
    P = eb._Problem(op)
    hold = bool(P.zero_rows(t, op.ny, 0).any())
    cX, cA, cP = host_coefficients(op)
    out = []
    for l, (nx, ny) in enumerate(level_shapes(op.nx, op.ny, max_levels)):
        if l > 0:
            cX, cA, cP = cX / 4, cA[::2] / (4 if mutant == "cA4" else 2), cP[::2] / 4
        held = np.zeros(ny, dtype=bool)
        if hold:
            held[0] = True
            if l == 0 or mutant == "coarse_rowN":
                held[ny - 1] = True
        out.append(Level(nx, ny, cX, cA, cP, held))
    return out


def _nb(x):
    """(W, E, S, N) neighbours of every point, periodic: S is row j - 1, N row j + 1."""
    return np.roll(x, 1, axis=1), np.roll(x, -1, axis=1), np.roll(x, 1, axis=0), np.roll(x, -1, axis=0)


def _weights(x):
    """Full weighting 1/16 [1 2 1; 2 4 2; 1 2 1] around the even / even points, periodic (any dtype, non-negative weights)."""
    W, E, S, N = _nb(x)
    SW, SE, NW, NE = np.roll(S, 1, axis=1), np.roll(S, -1, axis=1), np.roll(N, 1, axis=1), np.roll(N, -1, axis=1)
    return ((4 * x + 2 * (W + E + S + N) + (SW + SE + NW + NE)) / 16)[::2, ::2]


def _interp_index(ny, nx):
    j, i = np.arange(ny)[:, None], np.arange(nx)[None, :]
    J, I = j >> 1, i >> 1
    return J, I, (J + (j & 1)) % (ny // 2), (I + (i & 1)) % (nx // 2)


def _interp(e, ny, nx):
    """Bilinear prolongation, periodic: e at even / even points, the mean of two or four coarse neighbours elsewhere."""
    J, I, Jp, Ip = _interp_index(ny, nx)
    return (e[J, I] + e[J, Ip] + e[Jp, I] + e[Jp, Ip]) / 4


class _Reference:
    """The cycle in the dtype rd with the error field of the module docstring (unit roundoff un) beside the values."""

    def __init__(self, levels, gamma, o, rd, un):
        self.levels, self.gamma, self.o, self.rd, self.un = levels, gamma, o, rd, un

    def _parts(self, lv, z):
        rd = self.rd
        cE, cWn, cP = (c.astype(rd)[None, :] for c in (lv.cE, lv.cWn, lv.cP))
        W, E, S, N = _nb(z)
        Lz = cE * (E - z) + cWn * (z - W) + cP * (N - 2 * z + S)
        Lz[lv.held] = 0
        return Lz, jr_sizes(lv, z)

    def _spread(self, lv, E):
        W, Ee, S, N = _nb(E)
        return np.abs(lv.cE)[None, :] * Ee + np.abs(lv.cWn)[None, :] * W + lv.cP[None, :] * (N + S)

    def sweep(self, lv, z, Ez, r, Er):
        rd, g, om, un = self.rd, self.gamma, self.o["omega"], self.un
        d = 1 + g * (2 * lv.cX + 2 * lv.cP)[None, :]
        Lz, SL = self._parts(lv, z)
        zn = z + rd(om) * (r - (z - rd(g) * Lz)) / d.astype(rd)
        w = om / d
        T = np.abs(r.astype(np.float64)) + np.abs(z.astype(np.float64)) + g * SL
        En = (1 - om) * Ez + w * g * self._spread(lv, Ez) + w * Er + un * (np.abs(z.astype(np.float64)) + w * T) + K_SWEEP * un * w * T
        zn[lv.held] = r[lv.held]
        En[lv.held] = Er[lv.held]
        return zn, En

    def residual(self, lv, z, Ez, r, Er):
        rd, g, un = self.rd, self.gamma, self.un
        d = 1 + g * (2 * lv.cX + 2 * lv.cP)[None, :]
        Lz, SL = self._parts(lv, z)
        s = r - (z - rd(g) * Lz)
        az, ar = np.abs(z.astype(np.float64)), np.abs(r.astype(np.float64))
        Es = Er + d * Ez + g * self._spread(lv, Ez) + K_RES * un * (ar + az + g * SL)
        Es[lv.held] = (un * (ar + az) + Er + Ez)[lv.held]
        return s, Es

    def cycle(self, l, r, Er):
        lv, o, un = self.levels[l], self.o, self.un
        last = l == len(self.levels) - 1
        z, Ez = np.zeros_like(r), np.zeros(r.shape)
        for _ in range(o["coarse"] if last else o["pre"]):
            z, Ez = self.sweep(lv, z, Ez, r, Er)
        if last:
            return z, Ez
        s, Es = self.residual(lv, z, Ez, r, Er)
        lc = self.levels[l + 1]
        rc, Erc = _weights(s), _weights(Es) + 4 * un * _weights(np.abs(s.astype(np.float64)))
        rc[lc.held] = 0
        Erc[lc.held] = 0
        e, Ee = self.cycle(l + 1, rc, Erc)
        corr, Ecorr = _interp(e, lv.ny, lv.nx), _interp(Ee, lv.ny, lv.nx) + 3 * un * _interp(np.abs(e.astype(np.float64)), lv.ny, lv.nx) + un * np.abs(z.astype(np.float64))
        corr[lv.held] = 0
        Ecorr[lv.held] = 0
        z, Ez = z + corr, Ez + Ecorr
        for _ in range(o["post"]):
            z, Ez = self.sweep(lv, z, Ez, r, Er)
        return z, Ez


def jr_sizes(lv, z):
    """jacobian_reference._diffusion_sizes on a level's tables."""
    u = np.asarray(z, dtype=np.float64)
    W, E, S, N = _nb(u)
    return np.abs(lv.cE[None, :] * (E - u)) + np.abs(lv.cWn[None, :] * (u - W)) + np.abs(lv.cP)[None, :] * (np.abs(N) + 2 * np.abs(u) + np.abs(S))


def vcycle_bound(op, t, gamma, r, precision, unit=None, dtype=None, **opts):
    """(ref, bound_u, bound_v) of z = M r on the whole grid: ref (ny, nx, 2) in the reference's dtype (dtype overrides it), the per-point
    bound of the module docstring on var0 and zeros on var1."""
    o = options(**opts)
    rd = dtype or eb.reference_dtype(precision)
    un = UNIT[precision] if unit is None else unit
    r = np.asarray(r)
    r0 = r[..., 0].astype(rd)
    if gamma == 0:
        z, Ez = r0.copy(), np.zeros(r0.shape)
    else:
        z, Ez = _Reference(build_levels(op, t, o["max_levels"]), float(gamma), o, rd, un).cycle(0, r0, np.zeros(r0.shape))
    return np.stack([z, r[..., 1].astype(rd)], axis=-1), Ez, np.zeros(r0.shape)


def reference_vcycle(op, t, gamma, r0, dtype=np.float64, **opts):
    """M applied to a var0 plane in `dtype` (what a Krylov method on var0 alone takes as its preconditioner)."""
    o = options(**opts)
    r0 = np.asarray(r0, dtype=dtype)
    return _Reference(build_levels(op, t, o["max_levels"]), float(gamma), o, dtype, 0.0).cycle(0, r0, np.zeros(r0.shape))[0]


def operator(op, t, gamma, x0, dtype=np.float64):
    """(I - gamma J_D(t)) on a var0 plane in `dtype`: rows of J_D are zero where the rows are held."""
    lv = build_levels(op, t, 1)[0]
    x0 = np.asarray(x0, dtype=dtype)
    W, E, S, N = _nb(x0)
    Lx = lv.cE.astype(dtype)[None, :] * (E - x0) + lv.cWn.astype(dtype)[None, :] * (x0 - W) + lv.cP.astype(dtype)[None, :] * (N - 2 * x0 + S)
    Lx[lv.held] = 0
    return x0 - dtype(gamma) * Lx


# ---- the kernels' own order in the device precision -------------------------------------------------------------------------------
class _KernelOrder:
    def __init__(self, levels, gamma, o, R, mutant):
        self.levels, self.R, self.o, self.mutant = levels, R, o, mutant
        self.fma = jr._fma(R)
        self.gamma, self.omega = R(gamma), R(o["omega"])

    def tables(self, lv):
        R = self.R
        return lv.cE.astype(R)[None, :], lv.cWn.astype(R)[None, :], lv.cP.astype(R)[None, :], R(2 * lv.cX)

    def apply(self, lv, z):
        R, fma = self.R, self.fma
        cE, cWn, cP, _ = self.tables(lv)
        W, E, S, N = _nb(z)
        d2y = fma(R(-2.0), z, N) + S
        lz = fma(cWn, z - W, fma(cE, E - z, cP * d2y))
        az = fma(-self.gamma, lz, z)
        az[lv.held] = z[lv.held]
        return az

    def sweep(self, lv, z, r, first):
        R, fma = self.R, self.fma
        _, _, cP, cX2 = self.tables(lv)
        w = self.omega / fma(self.gamma, fma(R(2.0), cP, cX2), R(1.0))
        zn = (w * r).astype(R) if first else fma(w, r - self.apply(lv, z), z)
        zn[lv.held] = r[lv.held]
        return zn

    def restrict(self, lv, lc, z, r):
        R, fma = self.R, self.fma
        s = r - self.apply(lv, z)
        if self.mutant == "injection":
            rc = s[::2, ::2].copy()
        else:
            W, E, S, N = _nb(s)
            SW, SE, NW, NE = np.roll(S, 1, axis=1), np.roll(S, -1, axis=1), np.roll(N, 1, axis=1), np.roll(N, -1, axis=1)
            if self.mutant == "seam":  # column 0's western neighbours one column off the seam
                W, SW, NW = W.copy(), SW.copy(), NW.copy()
                W[:, 0], SW[:, 0], NW[:, 0] = s[:, -2], S[:, -2], N[:, -2]
            edge, corner = (W + E) + (S + N), (SW + SE) + (NW + NE)
            rc = (R(0.0625) * fma(R(4.0), s, fma(R(2.0), edge, corner)))[::2, ::2].copy()
        if self.mutant != "coarse_held_rhs":
            rc[lc.held] = 0
        return rc

    def prolong(self, lv, z, e):
        R = self.R
        J, I, Jp, Ip = _interp_index(lv.ny, lv.nx)
        corr = R(0.25) * ((e[J, I] + e[J, Ip]) + (e[Jp, I] + e[Jp, Ip]))
        if self.mutant == "prolong_row":
            corr = np.roll(corr, 1, axis=0)
        zn = z + corr
        zn[lv.held] = z[lv.held]
        return zn

    def cycle(self, l, r):
        lv, o = self.levels[l], self.o
        last = l == len(self.levels) - 1
        z = np.zeros_like(r)
        for k in range(o["coarse"] if last else o["pre"]):
            z = self.sweep(lv, z, r, k == 0)
        if last:
            return z
        e = self.cycle(l + 1, self.restrict(lv, self.levels[l + 1], z, r))
        z = self.prolong(lv, z, e)
        for _ in range(o["post"]):
            z = self.sweep(lv, z, r, False)
        return z


def kernel_order_vcycle(op, t, gamma, r, R, mutant=None, **opts):
    """z = M r in the device precision R in crd_multigrid.hip's operation order, (ny, nx, 2).  mutant: one of MUTANTS --
    "seam" a theta-seam slip in the restriction, "injection" for full weighting, "prolong_row" the prolongation one row off,
    "coarse_held_rhs" the coarse held row's right-hand side not zeroed, "cA4" cA / 4 for cA / 2 in the coarse tables,
    "coarse_rowN" row ny - 1 held on the coarse levels too."""
    assert mutant is None or mutant in MUTANTS, mutant
    o = options(**opts)
    r = np.asarray(r).astype(R)
    if gamma == 0:
        return r.copy()
    z = _KernelOrder(build_levels(op, t, o["max_levels"], mutant), gamma, o, R, mutant).cycle(0, r[..., 0].copy())
    return np.stack([z, r[..., 1]], axis=-1)


# ---- the cases tests/test_multigrid_host.py and tests/test_gpu_multigrid.py share -------------------------------------------------
# (nx, ny) -> levels: coarse levels 4 wide; 17 wide (136, 68, 34, 17); 6 x 5; one tile exactly; two tiles and a ragged third / under
# one tile: one level only; and the largest
LEVEL_CASES = [((32, 128), 4), ((136, 72), 4), ((48, 40), 4), ((64, 16), 3), ((130, 33), 1), ((61, 9), 1)]
GRIDS = [g for g, _ in LEVEL_CASES] + [(96, 384)]
GAMMAS = (20.0, 2000.0)  # multiples of the explicit bound
OPTION_SETS = [dict(), dict(pre=1, post=3, coarse=2, max_levels=2)]
# the issue's table: (nx, ny, surface, held, gamma multiple, GMRES iterations without / with the cycle in the prototype)
GMRES_TABLE = [
    (32, 128, "torus", False, 20.0, 82, 9),
    (32, 128, "torus", True, 500.0, 298, 13),
    (48, 192, "torus", False, 2000.0, 379, 13),
    (48, 192, "torus", True, 2000.0, 624, 19),
    (48, 192, "flat", True, 2000.0, 432, 19),
    (96, 384, "torus", True, 8000.0, 1514, 20),
]


def shim_build_command(exe):
    """gcc command line of tests/native/shim_psolve_selftest.c + integration/crd_arkode_shim.c against the test double."""
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.join(root, "crdmodel_amd")
    return ["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "integration"),
            "-I", os.path.join(root, "tests", "native"), '-DCRD_SHIM_NVECTOR_HEADER="mock_nvector.h"', os.path.join(root, "integration", "crd_arkode_shim.c"),
            os.path.join(root, "tests", "native", "shim_psolve_selftest.c"), "-o", str(exe), "-L", lib_dir, "-lcrd", "-Wl,-rpath," + lib_dir,
            "-Wl,-rpath,/opt/rocm/lib", "-lm"]


def explicit_bound(op):
    """2.785 / (4 cX + 4 max cP): the diffusion operator's explicit step bound, the unit gamma is given in."""
    cX, _, cP = host_coefficients(op)
    return 2.785 / (4 * cX + 4 * np.max(cP))


def gmres_iterations(matvec, b, M=None, rtol=1e-10, restart=None):
    """(x, inner iterations) of scipy gmres with a restart length beyond the iteration count (the problem's size, capped at 2000).
    scipy ends a preconditioned inner loop on the preconditioned residual and then looks at the true one: where that is still a
    shade above the tolerance it starts a second cycle of a few iterations, which the count includes."""
    from scipy.sparse.linalg import LinearOperator, gmres

    n = b.size
    count = [0]

    def tick(_):
        count[0] += 1

    A = LinearOperator((n, n), matvec=matvec, dtype=np.float64)
    Mop = None if M is None else LinearOperator((n, n), matvec=M, dtype=np.float64)
    x, info = gmres(A, b, M=Mop, rtol=rtol, atol=0.0, restart=min(n, 2000) if restart is None else restart, maxiter=5, callback=tick, callback_type="pr_norm")
    assert info == 0, info
    return x, count[0]
