"""Per-point rounding-error bounds for the HIP right-hand side, one RK4 step and one error-controlled attempt.  TEST INFRASTRUCTURE ONLY.

Only tests/ may import this module.  It states, point by point and field by field, how far a correct kernel in a given
precision may land from a high-precision reference, so that a mistake that is large where it happens fails even when it is
small next to the largest term on the grid (the joint max-norm gate of tests/conftest.py: rel_err).

Reference
---------
fp64 kernels: oracle/crd_oracle_np.py in np.longdouble (64-bit significand; refused, not skipped, where the platform's long
double is narrower).  fp32 kernels: the same restatement in float64, evaluated on the fp32 state widened exactly, so that
rounding the input is never counted as kernel error.  The reference's own error (2^-64 or 2^-53 of the same terms) is at
most 1/2048 of the bound and ignored.

Right-hand side
---------------
With u the unit roundoff of the kernel's precision (2^-53 or 2^-24), every point's result is a short chain of products
and sums.  The standard model fl(a op b) = (a op b)(1 + d), |d| <= u, bounds the error of ANY evaluation order of a sum of
terms t_i, fused or not, by (n - 1) u sum |t_i| + O(u^2): each rounding is relative to a partial sum, and every partial
sum is at most sum |t_i|.  So

    |f_kernel - f_ref| <= K u S + rho |w|       per point and per field,

where S sums the absolute values of every term and product the point function combines:

    S_u = |cE gE| + |cWn gW| + |cP| (|uN| + 2|uC| + |uS|) + kinetics_u
          FHN        kinetics_u = |v| + 3|u| + |u|^3,            S_v = eps (|u| + |b|)
          Goldbeter  kinetics_u = |v2| + |v3| + kf |v| + k |u| + |v0 + v1 b|,   S_v = |v2| + |v3| + kf |v|
          diffusion only: S_v = 0 (dv is exactly zero)

with gE = uE - uC, gW = uC - uW (the theta differences are exact or correct to half an ulp of u, so the theta part is
charged against the differences; the phi second difference is formed from values and charged against the values), and
cE, cWn, cP the host's fp64 coefficient tables (crdmodel_amd/csrc/crd_host.cpp: build_coefficients).  The two Hill terms
v2 and v3 are taken separately because they cancel in w = v2 - v3.  Rounding a table (cE, cWn, cP, the row parameter
eps b or v0 + v1 b) to the device precision is one more relative u on a term already in S.

The Goldbeter reciprocal (hardware estimate + one Newton step, crd_device.h: reciprocal) is not correctly rounded.  Its
relative error rho multiplies the quotient w and is charged as its own term, rho |w|, so a change to the reciprocal (or
to CRD_RCP_NEWTON) moves this bound rather than hiding inside K.

The torus coefficients' own conditioning.  theta_i = i dx, rho = R + r cos(theta), cA ~ sin(theta) / rho and cP ~ 1 / rho^2 are
formed in fp64 by the host's tables and by the reference program alike, while this module's reference forms them in its own, wider
type.  In fp64 theta_i carries the product's rounding, |d theta| <= u64 theta, so |d cos| <= u64 (theta |sin| + |cos|) and, with the
product r cos and the sum,

    |d rho| / |rho| <= u64 kappa,    kappa = r (theta |sin theta| + 2 |cos theta|) / |rho| + 1:

a cancellation when the torus nearly closes on its axis (R -> r: rho -> 0 at theta = pi).  kappa <= 2.4 on an 80 x 20 torus, which
the spare rounding in K used to cover unnoticed; at 20.5 x 20 (R / r = 1.025) it reaches 83 and the reference's own compiled f() -- a correct fp64
evaluation by definition -- left the old bound by a factor 2.2 (tests/test_refprobe_host.py).  So the coefficients' errors are
charged as their own term, against the exact differences they multiply and in u64 whatever the kernel's precision:

    u64 [ (|cA| (kappa + 3) + D theta |cos theta| / (2 dx r |rho|)) |uE - uW| + |cP| (2 kappa + 3) |uN - 2 uC + uS| ]

(the second summand of the first bracket is sin(theta)'s absolute error, theta |cos theta| u64, which is not small next to
sin(theta) near theta = 0 and pi; the 3 are the remaining products and quotients of each table entry).  Zero on the flat surface.

Absorbing rows while t < tBoundary, dv of diffusion-only Goldbeter, and a uniform field's diffusion are exact zeros: the
bound there is 0 and any nonzero result fails.

One RK4 step
------------
Stages Y1 = y0, Y2 = y0 + dt/2 k1, Y3 = y0 + dt/2 k2, Y4 = y0 + dt k3 at times t, t + dt/2, t + dt/2, t + dt (the oracle's).
With dY_s the bound on the stage input's error, the stage derivative's error is

    e_s = K u S(Y_s) + rho |w(Y_s)| + |J(Y_s)| dY_s

where |J| is the absolute Jacobian of f as a 5-point stencil: |cE| on the east neighbour, |cWn| on the west, |cP| on north
and south, |cWn - cE - 2 cP + dg/du| on the centre, |dg/dv| on v; and |dh/du|, |dh/dv| for the v equation (kinetic partials
analytic).  Stage inputs are one fused multiply-add with a rounded coefficient c dt:

    dY_{s+1} = c dt e_s + 2 u (|y0| + c dt |k_s|)

and the step's result, formed from y0 and the four k_s in any order (running accumulators on the device, the reference's
y0 + dt/6 (k1 + 2 k2 + 2 k3 + k4) on the host):

    bound = dt/6 (e1 + 2 e2 + 2 e3 + e4) + K_ACC u (|y0| + dt/6 sum w_s |k_s|).

A stage at a time before tBoundary has exact zeros on the absorbing rows: e_s = 0 there.  The bound is evaluated at the
reference's stage values; the kernel's differ by dY_s, which moves S and |J| by O(u) of themselves (second order).

One error-controlled attempt (Zonneveld 5(3)4, fused_item<..., EMBED = 2, ...>)
----------------------------------------------------------------------------
The propagated solution is classical RK4 (b5 = 0): its reference and per-point bound are the ones above.  The EMBED = 2 body keeps
no running sums; with d_i = y_i - y0 taken from the stage values y_i = fl(y0 + c_i h k_i) still in registers it forms

    y_new = fma(1/3, fma(2, d2, d1 + d3), fma(h/6, k4, y0)).

Each d_i carries the rounding of its y_i, u (|y0| + c_i h |k_i|), one more u c_i h |k_i| for the rounded step size and one for the
subtraction where it is not exact; weighted (1, 2, 1)/3 that is 4/3 u |y0| + 3 u h/6 (|k1| + 2 |k2| + 2 |k3|).  On top: d1 + d3, the inner
fma, the rounded 1/3 and the outer fma round the k1..k3 sum 4 times (7 in all); fma(h/6, k4, y0), the rounded h/6 and the outer fma
round the k4 term 3 times and y0 twice (10/3 with the 4/3).  The largest count is 7 <= K_ACC = 8: the same constant holds, with one
spare instead of two.

Fifth stage, at t + 3h/4 (its absorbing flag decided at that time), from
z5 = fma(5/16, d1, fma(7/16, d2, fma(13/32, d3, fma(-h/32, k4, y0)))) = y0 + h (5/32 k1 + 7/32 k2 + 13/32 k3 - 1/32 k4):

    dY5 = h sum |a5i| e_i + C5 u (|y0| + h sum |a5i| |k_i|),       e5 = stage_error(..., dY5).

C5: y0 takes the innermost fma's rounding, the three outer ones and (5/16 + 7/16 + 13/32) u through the d_i: 5.2; a k_i term takes its
d_i's three roundings and up to three fmas (k3: 6), k4 the rounded h and four fmas (5).  C5 = 6.

The estimate.  Reference: err = h (2/3 k1 - 2 k2 - 2 k3 - 2 k4 + 16/3 k5) = h sum beta_i k_i, beta = b - b^ of
oracle/arkode_erk.ZONNEVELD_5_3_4.  Device: e4 = fma(4/3, d1, fma(-4, d2, fma(-2, d3, (-2 h) k4))) when the row's stage 4 runs, and
err = fma(fl(16/3) h, k5, e4) one iteration later:

    d_err = h sum |beta_i| e_i + K_ERR u h sum |beta_i| |k_i| + K_Y u |y0|.

K_ERR: a term takes its d_i's three roundings (above), the rounded 4/3 (k1 only), the fmas of e4 it sits inside (k1: 1, k2: 2, k3: 3;
k4: the rounded h, its product and three fmas) and the last fma: k1 6, k2 6, k3 7, k4 6; k5 the rounded 16/3, its product with the
rounded h and the last fma: 4.  K_ERR = 8 leaves one spare.  K_Y = sum_{i<=3} |beta_i| / c_i = 4/3 + 4 + 2 = 22/3 is the price of
forming the estimate from stage VALUES: d_i inherits u |y_i| from y_i, an error of the size of y0 in a quantity of the size of h k,
multiplied by beta_i / c_i.  (The kernel's header names it: "a rounding of y_i itself ... in quantities that are compared with
rtol |y| + atol".  In fp32 it is the floor of the estimate: 22/3 2^-24 |y0| = 4.4e-7 |y0| per point.)  The reference's order,
h (2/3 k1 - 2 (k2 + k3 + k4) + 16/3 k5) in the kernel's precision, has no such term and at most 7 roundings per k.

The norm.  dsm_ref = sqrt(sum (err w)^2 / N), w = 1 / (rtol |y0| + atol), over both fields.  The device forms
fma(rtol, |y0|, atol) from rtol and atol rounded to its precision (positive terms: 3 u) and divides (1 u): K_W = 4, so per point

    delta = w d_err + K_W u |err| w,

and by the triangle inequality of the RMS norm |dsm_gpu - dsm_ref| <= D + sigma (dsm_ref + D), D = sqrt(sum delta^2 / N).
sigma is the summation: a lane adds its rows' squares in the KERNEL's precision, err2 = fma(eu, eu, fma(ev, ev, err2)), over at most
one chunk's rows -- 32 at most (fused_chunk_rows without the one-round and 64-row plans, which an attempt does not use;
ensemble_attempt_plan), so N_ACC = 64 additions of non-negative terms: the sum is off by at most 64 u of itself, the norm by
32 u.  In fp32 that is 1.9e-6 of dsm (4.8e-7 with the 4-row chunks of a test-sized grid): stated here because nothing else does.
Then fp64 throughout: the lane's value widened (exact), a 6-level butterfly, one partial per work item, thread t of 256 adding items
t, t + 256, ..., an 8-level tree, the slabs' sums, the division by N and the root: K_RED = 24 roundings of 2^-53 cover a launch of up
to 2048 items on 4 slabs, 1.3e-15 of dsm.  Negligible beside 32 u in fp32; of its size in fp64, so it is in the bound:

    sigma = (N_ACC u + K_RED 2^-53) / 2.

One RK4(3) attempt (CRD_ADAPT_RK43, fused_item<..., EMBED = 1, ...>)
------------------------------------------------------------------
The propagated solution is classical RK4 formed by the running accumulators of the plain step (ACC_U / ACC_V stay live beside the
fifth stage): reference and per-point bound B are "One RK4 step"'s, K_ACC included.  The fifth stage is k5 = f(t + h, y_new) on the
y_new the lane has just formed (U4 / V4 hold a window of it, K4U / K4V hold k4 itself), its absorbing flag the host's absorb[3],
decided at t + h like stage 4's (crd_adaptive.cpp: launch_attempt).  The device's y_new is within B of the reference's, so

    e5 = stage_error(t + h, y_new; dY = B)

-- the construction f_new_bound uses for the interpolant's f_{n+1}.  The estimate.  Reference: err = h/6 (k4 - k5) (the pair's
third-order weights are (1/6, 1/3, 1/3, 0, 1/6): y_new - yhat).  Device: `h6 * (K4U - du) / wu`:

    d_err = h/6 (e4 + e5) + K_EST43 u h/6 (|k4| + |k5|),

K_EST43 = 3: the rounded h6 = fl(h / 6), the subtraction, the product (each relative to h/6 |k4 - k5| <= h/6 (|k4| + |k5|)); the
quotient is K_W's.  No K_Y term: nothing here is formed from stage values.  k4 - k5 = O(h) k, so the estimate is a third-order
quantity in h |lambda|, orders above the rounding floor the Zonneveld estimate has in fp32, and the norm bound is accordingly a
smaller fraction of the norm: 5e-6 ... 1e-4 in fp32, 1e-14 ... 4e-13 in fp64 on the grids of the tests.

The norm: as above, delta = w d_err + K_W u |err| w, |dsm_gpu - dsm_ref| <= D + sigma (dsm_ref + D), with the same reduction
(K_RED).  Only N_ACC differs.  An EMBED = 1 launch takes the launch plan the context keeps for it, plan_embed; on a grid of 2^20
points or more that plan is measured on the first launch (autotune is on by default), and two of its chunk modes make chunks
taller than 32 rows: 64 rows (mode 2) and "one round" (mode 1), stretched to at most 96 (fused_chunk_rows: `need <= 96`).  A lane
can therefore add 96 rows' squares, both fields: N_ACC_RK43 = 192, sigma = 96 u + 12 2^-53 (5.7e-6 in fp32).  The grids of the
tests are below 2^20 points and get 4- to 32-row chunks; the bound is stated for what the path can do, not for what the tests meet.
(plan_arkode is measured by the same code, so the Zonneveld section's "32 at most" holds for unmeasured plans only -- every grid
its gates run on; its N_ACC is left as it is, erk_attempt_bound's results being pinned by those gates.)

Dense output (Hermite, ARK_NORMAL)
----------------------------------
theta = (tout - t_n) / h in (0, 1):  y(theta) = h00 y_n + h01 y_{n+1} + h (h10 f_n + h11 f_{n+1}) with the cubic Hermite basis
(oracle/arkode_erk.hermite_arkode with tau = theta - 1).  y_n is exact input and f_n = f(t_n, y_n) has the RHS bound; the device's
y_{n+1} is within the attempt's bound B, so its f_{n+1} = f(t_{n+1}, y_{n+1}) is within stage_error(f_{n+1}; dY = B):

    bound = |h01| B + h |h10| e(f_n) + h |h11| stage_error(f_{n+1}; B) + K_HERM u (|h00 y_n| + |h01 y_{n+1}| + h |h10 f_n| + h |h11 f_{n+1}|)

K_HERM = 4 + 2: the kernel's four roundings (h11 f_{n+1}'s product and three fused multiply-adds around it), and two for a
coefficient, which the host forms in double -- a cubic in theta, times h -- and rounds to the kernel's precision.
"""
import numpy as np

from oracle import crd_oracle as co
from oracle import crd_oracle_np as cn

UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}  # unit roundoff of the kernel's precision (round to nearest)
# K: FHN's longest chain sums 7 terms (u: east, west, three phi values, v, kinetics), 6 roundings, plus one for a table or row
# parameter rounded to the device precision: 7, and 8 leaves one spare.  Goldbeter's u chain is longer (Hill quotients several
# roundings deep), so there K is empirical: the host's fp32 restatements reach 0.37 (kernel order) and 0.78 (reference order) of it.
K = 8.0
# K_ACC: the reference's order rounds 6 times on the way to y (three sums of k, the rounded dt/6, its product, + y0); the
# device's running sums 5 times (four fused multiply-adds, a rounded coefficient); 8 leaves two spare.
K_ACC = 8.0
# rho: relative error of the Goldbeter reciprocal.  fp64: v_rcp_f64 (2^-24.4) + one Newton step, 2.2e-15 as measured over
# [2.6, 1e6] (crd_device.h: reciprocal; relative, so the range's scale does not matter).  fp32: the estimate's error squared
# (2^-46) plus the refined value's rounding and the residual's, 3 u.
RHO = {"f64": 2.2e-15, "f32": 3.0 * 2.0 ** -24}
# The attempt's constants: counted in the docstring ("One error-controlled attempt"), from crd_fused_impl.h: fused_item, EMBED = 2.
C5 = 6.0          # roundings on the fifth stage's input
K_ERR = 8.0       # roundings on a term h beta_i k_i of the estimate (largest count 7)
K_Y = 22.0 / 3.0  # sum_{i<=3} |beta_i| / c_i: the stage values' own rounding, u |y0|, carried into the estimate by d_i = y_i - y0
K_W = 4.0         # the weight's three roundings and the quotient's
N_ACC = 64        # additions into a lane's sum of squares in the kernel's precision: 32 rows at most, both fields
K_RED = 24.0      # fp64 roundings between a lane's sum and dsm
K_HERM = 6.0      # the interpolant's four roundings + two on a coefficient
# The RK4(3) attempt's constants: counted in the docstring ("One RK4(3) attempt"), from crd_fused_impl.h: fused_item, EMBED = 1.
# K_EST43: the roundings of `eu = h6 * (K4U[S5 & 1] - du) / wu` (and ev alike) on h/6 (k4 - k5), the quotient apart (that one is K_W's):
# h6 = (Real)(dt / 6.0) rounded to the kernel's precision (launch_fused_t), the subtraction k4 - k5, the product with h6.  K4U holds
# k4 as stage 4 left it (`K4U[S4 & 1] = du`): no rounding of its own.  Three, none spare.
K_EST43 = 3.0
# N_ACC_RK43: additions into a lane's sum of squares, both fields, over the tallest chunk an EMBED = 1 launch can take under plan_embed:
# 96 rows (fused_chunk_rows: a measured plan's one-round chunks, `need <= 96`; its 64-row mode and the plain 32 lie below).
N_ACC_RK43 = 192
KF, KK, V0, V1, VM2, VM3, K2, KR, KA, EPS = 1.0, 10.0, 1.0, 7.3, 65.0, 500.0, 1.0, 2.0, 0.9, cn.EPSILON


def reference_dtype(precision):
    if precision == "f64":
        assert np.finfo(np.longdouble).nmant >= 63, (
            "the fp64 kernels' reference needs an 80-bit (or wider) np.longdouble; this platform's has %d mantissa bits"
            % np.finfo(np.longdouble).nmant)
        return np.longdouble
    assert precision == "f32", precision
    return np.float64


class _Problem:
    """The oracle Problem's whole-grid description in the numpy restatement's terms, plus the fp64 coefficient tables."""

    def __init__(self, p):
        self.model = {co.FHN: "fhn", co.GOLDBETER: "goldbeter"}[p.model]
        self.surface = {co.TORUS: "torus", co.FLAT: "flat"}[p.surface]
        self.g = dict(nx=p.nx, ny=p.ny, dx=p.dx, dy=p.dy, xmin=p.xmin, xmax=p.xmax, ymin=p.ymin, ymax=p.ymax, R=p.R, r=p.r)
        self.D = p.diff
        self.kw = dict(beta=p.beta, vary_beta=p.vary_beta, beta_min=p.beta_min, beta_max=p.beta_max, t_boundary=p.t_boundary,
                       just_diffusion=p.just_diffusion)
        self.diffusion_only = self.model == "goldbeter" and p.just_diffusion != 0
        D, dx, dy = p.diff, p.dx, p.dy
        if self.surface == "torus":  # the host's tables, as crd_host.cpp: build_coefficients forms them
            theta = p.xmin + np.arange(p.nx, dtype=np.float64) * dx
            rho = p.R + p.r * np.cos(theta)
            cX = D * (1 / (p.r * p.r)) / (dx * dx)
            cA = D * (-np.sin(theta) / (p.r * rho)) / (2 * dx)
            cP = D * (1 / (rho * rho)) / (dy * dy)
            # the coefficients' own fp64 errors, per column (module docstring: "The torus coefficients' own conditioning")
            kappa = p.r * (theta * np.abs(np.sin(theta)) + 2 * np.abs(np.cos(theta))) / np.abs(rho) + 1
            self.dcA = UNIT["f64"] * (np.abs(cA) * (kappa + 3) + D * theta * np.abs(np.cos(theta)) / (2 * dx * p.r * np.abs(rho)))
            self.dcP = UNIT["f64"] * np.abs(cP) * (2 * kappa + 3)
        else:
            cX = D / dx / dx
            cA = np.zeros(p.nx)
            cP = np.full(p.nx, D / dy / dy)
            self.dcA = self.dcP = np.zeros(p.nx)
        self.cE, self.cWn, self.cP = cX + cA, cA - cX, cP

    def rhs(self, t, u, v, dtype, j0):
        return cn.rhs(self.model, self.surface, self.g, self.D, t, u, v, dtype=dtype, j0=j0, **self.kw)

    def zero_rows(self, t, rows, j0):
        """Rows (of a band starting at global row j0) whose derivative is exactly zero at time t."""
        if self.diffusion_only or not t < self.kw["t_boundary"]:
            return np.zeros(rows, dtype=bool)
        return np.isin((j0 + np.arange(rows)) % self.g["ny"], (0, self.g["ny"] - 1))

    def terms(self, u, v, j0):
        """(S_u, S_v, |w|, centre, dg/dv, dh/du, dh/dv) per point, in float64, at the state (u, v) of a band from row j0."""
        u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
        uW, uE = np.roll(u, 1, axis=1), np.roll(u, -1, axis=1)
        uS, uN = np.roll(u, 1, axis=0), np.roll(u, -1, axis=0)
        cE, cWn, cP = self.cE[None, :], self.cWn[None, :], self.cP[None, :]
        S_u = np.abs(cE * (uE - u)) + np.abs(cWn * (u - uW)) + np.abs(cP) * (np.abs(uN) + 2 * np.abs(u) + np.abs(uS))
        centre_lin = cWn - cE - 2 * cP
        zero = np.zeros_like(u)
        if self.diffusion_only:
            return S_u, zero, zero, np.abs(centre_lin + zero), zero, zero, zero
        b = cn.beta_rows(self.g, self.kw["beta"], self.kw["vary_beta"], self.kw["beta_min"], self.kw["beta_max"], np.float64, j0,
                         u.shape[0])[:, None]
        if self.model == "fhn":
            S_u = S_u + np.abs(v) + 3 * np.abs(u) + np.abs(u) ** 3
            S_v = EPS * (np.abs(u) + np.abs(b))
            gu, gv, hu, hv = 3 - 3 * u * u, -1.0 + zero, EPS + zero, zero
            w = zero
        else:
            z2, y2 = u * u, v * v
            z4 = z2 * z2
            ka4 = KA ** 4
            v2 = VM2 * z2 / (K2 * K2 + z2)
            v3 = VM3 * y2 * z4 / ((KR * KR + y2) * (ka4 + z4))
            hill = np.abs(v2) + np.abs(v3) + KF * np.abs(v)
            S_u = S_u + hill + KK * np.abs(u) + np.abs(V0 + V1 * b)
            S_v = hill
            w_z = VM2 * 2 * u * K2 * K2 / (K2 * K2 + z2) ** 2 - VM3 * y2 / (KR * KR + y2) * 4 * u * z2 * ka4 / (ka4 + z4) ** 2
            w_y = -VM3 * z4 / (ka4 + z4) * 2 * v * KR * KR / (KR * KR + y2) ** 2
            gu, gv, hu, hv = -w_z - KK, -w_y + KF, w_z, w_y - KF
            w = np.abs(v2 - v3)
        return S_u, S_v, w, np.abs(centre_lin + gu), np.abs(gv), np.abs(hu), np.abs(hv)

    def stage_error(self, precision, t, u, v, j0, du=None, dv=None):
        """Bounds (e_u, e_v) on the error of f at a state known to within (du, dv) per point (None: exact input)."""
        S_u, S_v, w, centre, gv, hu, hv = self.terms(u, v, j0)
        rcp = RHO[precision] * w
        u64 = np.asarray(u, dtype=np.float64)
        tables = (self.dcA[None, :] * np.abs(np.roll(u64, -1, axis=1) - np.roll(u64, 1, axis=1))
                  + self.dcP[None, :] * np.abs(np.roll(u64, -1, axis=0) - 2 * u64 + np.roll(u64, 1, axis=0)))
        eu = K * UNIT[precision] * S_u + rcp + tables
        ev = K * UNIT[precision] * S_v + rcp
        if du is not None:
            cE, cWn, cP = np.abs(self.cE)[None, :], np.abs(self.cWn)[None, :], np.abs(self.cP)[None, :]
            eu = eu + (cE * np.roll(du, -1, axis=1) + cWn * np.roll(du, 1, axis=1) + cP * (np.roll(du, -1, axis=0) + np.roll(du, 1, axis=0))
                       + centre * du + gv * dv)
            ev = ev + hu * du + hv * dv
        zero = self.zero_rows(t, u.shape[0], j0)
        eu[zero] = 0.0
        ev[zero] = 0.0
        return eu, ev


def _split(y, dtype):
    y = np.asarray(y)
    assert y.ndim == 3 and y.shape[2] == 2, y.shape
    return y[..., 0].astype(dtype), y[..., 1].astype(dtype)


def rhs_bound(problem, t, y, precision, j0=0):
    """(ref, bound_u, bound_v) for f(t, y) of a kernel in `precision` ("f64" / "f32").  problem: the whole grid's oracle Problem
    (co.make_problem); y: (rows, nx, 2), the whole grid or a band of whole rows starting at global row j0 (a band's first and
    last rows wrap inside the band and are not meaningful).  ref has the reference's dtype (np.longdouble for f64)."""
    P = _Problem(problem)
    rd = reference_dtype(precision)
    u, v = _split(y, rd)
    fu, fv = P.rhs(t, u, v, rd, j0)
    bu, bv = P.stage_error(precision, t, u, v, j0)
    return np.stack([fu, fv], axis=-1), bu, bv


def _rk4_stages(P, t, dt, y0u, y0v, precision, j0):
    """The four classical stages from (t, y0) in the reference's dtype: (ks, es, ref, bounds) -- the stage derivatives, the bounds on
    the device's errors in them, the step's reference result and its per-point bounds (the docstring's "One RK4 step")."""
    rd = y0u.dtype.type
    un = UNIT[precision]
    a0u, a0v = np.abs(y0u.astype(np.float64)), np.abs(y0v.astype(np.float64))
    h = rd(dt)
    cs, ws = (0.0, 0.5, 0.5, 1.0), (1.0, 2.0, 2.0, 1.0)
    Yu, Yv, du, dv = y0u, y0v, None, None
    ks, es = [], []
    for s in range(4):
        ts = t + cs[s] * float(dt)
        ku, kv = P.rhs(ts, Yu, Yv, rd, j0)
        eu, ev = P.stage_error(precision, ts, Yu, Yv, j0, du, dv)
        ks.append((ku, kv))
        es.append((eu, ev))
        if s < 3:
            c = cs[s + 1]
            Yu, Yv = y0u + (rd(c) * h) * ku, y0v + (rd(c) * h) * kv  # the oracle's stage inputs (crd_oracle_np.rk4)
            du = c * float(dt) * eu + 2 * un * (a0u + c * float(dt) * np.abs(ku.astype(np.float64)))
            dv = c * float(dt) * ev + 2 * un * (a0v + c * float(dt) * np.abs(kv.astype(np.float64)))
    (k1u, k1v), (k2u, k2v), (k3u, k3v), (k4u, k4v) = ks
    ref = np.stack([y0u + (h / 6) * (k1u + 2 * k2u + 2 * k3u + k4u), y0v + (h / 6) * (k1v + 2 * k2v + 2 * k3v + k4v)], axis=-1)
    h6 = float(dt) / 6.0
    bounds = []
    for f, a0 in ((0, a0u), (1, a0v)):
        prop = h6 * sum(w * e[f] for w, e in zip(ws, es))
        size = a0 + h6 * sum(w * np.abs(k[f].astype(np.float64)) for w, k in zip(ws, ks))
        bounds.append(prop + K_ACC * un * size)
    return ks, es, ref, bounds


def rk4_step_bound(problem, t, dt, y, precision, j0=0):
    """(ref, bound_u, bound_v) for one classical RK4 step of size dt from (t, y), as rhs_bound (a band's first and last 4 rows
    are not meaningful)."""
    P = _Problem(problem)
    y0u, y0v = _split(y, reference_dtype(precision))
    _, _, ref, bounds = _rk4_stages(P, t, dt, y0u, y0v, precision, j0)
    return ref, bounds[0], bounds[1]


class AttemptBound:
    """erk_attempt_bound's and rk43_attempt_bound's result.  state: (ref, bound_u, bound_v) of y_new, as rk4_step_bound's (for check()); err: the reference's
    per-point estimate (rows, nx, 2) with its per-point bounds err_bound_u / err_bound_v (not weighted); dsm, dsm_bound: the
    reference's WRMS norm and the bound on |dsm_device - dsm|; f_new_bound(): see hermite_bound."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def erk_attempt_bound(problem, t, h, y, precision, rtol, atol, j0=0):
    """One Zonneveld 5(3)4 attempt of size h from (t, y): the propagated state's reference and per-point bound, the reference's
    per-point error estimate and the bound on the device's, and the WRMS norm dsm_ref with the bound on |dsm_device - dsm_ref|
    (module docstring).  y as rk4_step_bound's; the norm is over all rows given (the whole grid: a band's edge rows are not
    meaningful).  Returns an AttemptBound."""
    from oracle.arkode_erk import ZONNEVELD_5_3_4 as tab

    P = _Problem(problem)
    rd = reference_dtype(precision)
    un = UNIT[precision]
    y0u, y0v = _split(y, rd)
    ks, es, ref, bounds = _rk4_stages(P, t, h, y0u, y0v, precision, j0)
    hh, hf = rd(h), float(h)
    a5 = tab["A"][4][:4]
    beta = [b - b2 for b, b2 in zip(tab["b"], tab["b2"])]
    t5 = t + tab["c"][4] * hf
    y0 = (y0u, y0v)
    a0 = [np.abs(v.astype(np.float64)) for v in y0]
    ak = [[np.abs(k[f].astype(np.float64)) for f in (0, 1)] for k in ks]
    Y5 = [y0[f] + hh * sum(rd(a) * k[f] for a, k in zip(a5, ks)) for f in (0, 1)]
    dY5 = [hf * sum(abs(a) * e[f] for a, e in zip(a5, es)) + C5 * un * (a0[f] + hf * sum(abs(a) * k[f] for a, k in zip(a5, ak))) for f in (0, 1)]
    k5 = P.rhs(t5, Y5[0], Y5[1], rd, j0)
    e5 = P.stage_error(precision, t5, Y5[0], Y5[1], j0, dY5[0], dY5[1])
    ks5, es5 = ks + [k5], es + [e5]
    ak.append([np.abs(k5[f].astype(np.float64)) for f in (0, 1)])
    # beta as exact rationals of the reference's dtype: 2/3 and 16/3 are not binary fractions
    bw = [rd(2) / rd(3), rd(-2), rd(-2), rd(-2), rd(16) / rd(3)]
    assert all(abs(float(a) - b) <= 1e-15 for a, b in zip(bw, beta)), (bw, beta)
    err, d_err = [], []
    for f in (0, 1):
        err.append(hh * sum(b * k[f] for b, k in zip(bw, ks5)))
        d_err.append(hf * sum(abs(b) * e[f] for b, e in zip(beta, es5)) + K_ERR * un * hf * sum(abs(b) * k[f] for b, k in zip(beta, ak)) + K_Y * un * a0[f])
    return _attempt_result(P, precision, j0, y0, ref, bounds, err, d_err, rtol, atol, N_ACC)


def _attempt_result(P, precision, j0, y0, ref, bounds, err, d_err, rtol, atol, n_acc):
    """The AttemptBound of an embedded pair from its per-point parts: y0 = (u, v) in the reference's dtype, the step's reference and
    bounds, err / d_err the reference's estimate and the bound on the device's per field; n_acc: additions into a lane's sum of
    squares in the kernel's precision.  The norm and its bound are the module docstring's ("The norm")."""
    rd = y0[0].dtype.type
    un = UNIT[precision]
    delta2, e2 = 0.0, rd(0)
    for f in (0, 1):
        a0 = np.abs(y0[f].astype(np.float64))
        w = 1.0 / (rtol * a0 + atol)
        delta = w * d_err[f] + K_W * un * np.abs(err[f].astype(np.float64)) * w
        wr = rd(1) / (rd(rtol) * np.abs(y0[f]) + rd(atol))
        e2 = e2 + np.sum((err[f] * wr) ** 2)
        delta2 += float(np.sum(delta * delta))
    n = 2 * y0[0].size
    dsm = float(np.sqrt(e2 / n))
    D = float(np.sqrt(delta2 / n))
    sigma = 0.5 * (n_acc * un + K_RED * UNIT["f64"])
    dsm_bound = D + sigma * (dsm + D)

    def f_new_bound(t_new):
        """f(t_new, y_new) in the reference's dtype and the bound on the device's f at ITS y_new: (f, e_u, e_v)."""
        fu, fv = P.rhs(t_new, ref[..., 0], ref[..., 1], rd, j0)
        eu, ev = P.stage_error(precision, t_new, ref[..., 0], ref[..., 1], j0, bounds[0], bounds[1])
        return np.stack([fu, fv], axis=-1), eu, ev

    return AttemptBound(state=(ref, bounds[0], bounds[1]), err=np.stack(err, axis=-1), err_bound_u=d_err[0], err_bound_v=d_err[1], dsm=dsm,
                        dsm_bound=dsm_bound, rms_delta=D, sigma=sigma, f_new_bound=f_new_bound)


def rk43_attempt_bound(problem, t, h, y, precision, rtol, atol, j0=0):
    """One RK4(3) attempt of size h from (t, y) (CRD_ADAPT_RK43; fused_item<..., EMBED = 1, ...>): as erk_attempt_bound, an AttemptBound
    with the propagated state's reference and per-point bound, the reference's estimate err = h/6 (k4 - k5), k5 = f(t + h, y_new), the
    per-point bound on the device's, and the WRMS norm with the bound on |dsm_device - dsm_ref| (module docstring, "One RK4(3)
    attempt").  The lane's sum is charged N_ACC_RK43 = 192 additions, not N_ACC = 64: an EMBED = 1 launch goes out under the context's
    plan_embed, which on grids of 2^20 points and more may be measured, and a measured plan's one-round chunks are up to 96 rows
    high (crd_fused_impl.h: fused_chunk_rows) -- 192 additions of both fields' squares per lane."""
    P = _Problem(problem)
    rd = reference_dtype(precision)
    un = UNIT[precision]
    y0 = _split(y, rd)
    ks, es, ref, bounds = _rk4_stages(P, t, h, y0[0], y0[1], precision, j0)
    hf = float(h)
    t5 = t + hf
    k5 = P.rhs(t5, ref[..., 0], ref[..., 1], rd, j0)
    e5 = P.stage_error(precision, t5, ref[..., 0], ref[..., 1], j0, bounds[0], bounds[1])  # (f_new_bound's construction: the device's y_new is within B)
    h6r, h6 = rd(h) / rd(6), hf / 6.0
    err, d_err = [], []
    for f in (0, 1):
        k4 = ks[3][f]
        err.append(h6r * (k4 - k5[f]))
        d_err.append(h6 * (es[3][f] + e5[f]) + K_EST43 * un * h6 * (np.abs(k4.astype(np.float64)) + np.abs(k5[f].astype(np.float64))))
    return _attempt_result(P, precision, j0, y0, ref, bounds, err, d_err, rtol, atol, N_ACC_RK43)


def hermite_bound(problem, t, h, theta, y, precision, attempt, j0=0):
    """(ref, bound_u, bound_v) of the dense output at t + theta h inside the accepted step `attempt` (erk_attempt_bound's result for
    the same t, h, y): the reference-precision cubic Hermite interpolant of the reference's y_n, y_{n+1}, f_n, f_{n+1} and the bound
    of the module docstring ("Dense output")."""
    from oracle.arkode_erk import hermite_arkode

    rd = reference_dtype(precision)
    un = UNIT[precision]
    f0, e0u, e0v = rhs_bound(problem, t, y, precision, j0)
    f1, e1u, e1v = attempt.f_new_bound(t + float(h))
    y0 = np.stack(_split(y, rd), axis=-1)
    y1, b1u, b1v = attempt.state
    tau = rd(theta) - rd(1)
    ref = hermite_arkode(tau, rd(h), y0, y1, f0, f1)
    th = float(theta)
    h00, h01 = 1 - (3 * th * th - 2 * th ** 3), 3 * th * th - 2 * th ** 3
    h10, h11 = th * (1 - th) ** 2, th * th * (th - 1)
    out = []
    for f, b1, e0, e1 in ((0, b1u, e0u, e1u), (1, b1v, e0v, e1v)):
        size = (abs(h00) * np.abs(y0[..., f]) + abs(h01) * np.abs(y1[..., f]) + float(h) * (abs(h10) * np.abs(f0[..., f]) + abs(h11) * np.abs(f1[..., f]))).astype(np.float64)
        out.append(abs(h01) * b1 + float(h) * (abs(h10) * e0 + abs(h11) * e1) + K_HERM * un * size)
    return ref, out[0], out[1]


def worst(got, ref, bound_u, bound_v, rows=None, j0=0):
    """{"u": (ratio, row, column), "v": ...}: the largest err / bound per field (inf where a zero bound is missed, or where a
    result is not finite), with its grid row (j0 + band row) and column.  rows: a slice of the band to judge (default all)."""
    rows = slice(None) if rows is None else rows
    start = rows.start or 0
    out = {}
    for f, name, b in ((0, "u", bound_u), (1, "v", bound_v)):
        g = np.asarray(got)[rows, :, f]
        err = np.abs(g.astype(ref.dtype) - ref[rows, :, f]).astype(np.float64)
        bb = np.asarray(b, dtype=np.float64)[rows]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0.0, 0.0, err / bb)
        r[~np.isfinite(g)] = np.inf
        r = np.nan_to_num(r, nan=np.inf, posinf=np.inf)
        j, i = np.unravel_index(int(np.argmax(r)), r.shape)
        out[name] = (float(r[j, i]), j0 + start + int(j), int(i))
    return out


def describe(case, w):
    return "%s: worst err/bound u %.3g at (row %d, col %d), v %.3g at (row %d, col %d)" % ((case,) + w["u"] + w["v"])


def check(case, got, bounded, rows=None, j0=0):
    """Assert got is inside the bound everywhere (bounded = rhs_bound / rk4_step_bound's result); returns worst()."""
    ref, bu, bv = bounded
    w = worst(got, ref, bu, bv, rows, j0)
    assert w["u"][0] <= 1.0 and w["v"][0] <= 1.0, describe(case, w)
    return w
