"""Reference for the error-controlled IMEX integrator (crd_integrate_imex / Slab.integrate_imex; crd_imex_tables.h: the embedded data,
crd_imex_control.h: the controller, crd_imex.hip: the estimating last close).  TEST INFRASTRUCTURE ONLY.

The pair
--------
ARS(4,4,3) with ONE embedded weight vector for both parts, BHAT = (0, 5/2, 0, -3/2, 0), in Fractions; DE, DI = b - BHAT per part.
`estimate_terms(dt, R)` lists the estimate's terms as crd_imex_tables.h: estimate_terms does (j ascending, explicit before implicit,
coefficients dt d rounded once to R, zeros left out).

The dense restatement
---------------------
`dense_estimate(stages, dt)` forms e = dt sum dE_j FR_j + dt sum dI_j k_j from imex_reference.dense_step(..., stages=); `wrms` is the
norm of include/crd.h with the weights 1 / (rtol |y_n| + atol); `integrate_dense` is the integrator around `Control`.  Mutants of the
estimate and of the norm (MUTANTS) each fail one named gate of tests/test_imex_adaptive_host.py.

The controller
--------------
`Control` restates crd_imex_control.h (and, inside it, crd_arkode.h's pid_eta / reject / accept with the embedding order 2) in Python
floats: the same operations in the same order, so it reaches the C++ step sizes up to pow's last bits.

The close in the kernel's arithmetic
------------------------------------
`close_reference` gives the estimating close's out, e and q bit for bit (imex_reference.fma_exact; q in plain float64 operations, each
rounded once), and `sum_bound` the allowance of the device's sum of q against its long-double sum: gamma_K sum q with K counted from the
reduction tree as tests/bicgstab_reference.py counts it (the tree is the same; the thread's chain adds q where that one fuses a
product).
"""
import math
import os
from fractions import Fraction as Fr

import numpy as np

import bicgstab_reference as br
import imex_reference as ir

ROOT = ir.ROOT
SCHEME = "ars443"
EMBEDDED_ORDER = 2
BHAT = [Fr(0), Fr(5, 2), Fr(0), Fr(-3, 2), Fr(0)]
MUTANTS = ("swapped_dI", "dropped_term", "weights_from_ynew", "bhat_for_b")
# the gate that claims each mutant
MUTANT_GATES = dict(swapped_dI="estimate_order", dropped_term="estimate_order", weights_from_ynew="norm_weights", bhat_for_b="solution_order")

K1, K2, K3 = 0.58, 0.21, 0.1
ETAMX1, ETAMXF = 10000.0, 0.3
SMALL_NEF, MAX_NEF = 2, 7
LBOUND, UBOUND, ONEPSM, ONEMSM = 1.0, 1.5, 1.000001, 0.999999
TINY = 1.0e-10
TOO_MUCH_WORK = "adaptive integration: max_steps steps taken before reaching tout (ARK_TOO_MUCH_WORK)"
UNDERFLOW = "adaptive integration: step size underflow"
ERR_FAILURE = "adaptive integration: the error test failed 7 times on one step (ARK_ERR_FAILURE)"


def differences():
    """(dE, dI) in Fractions: b - BHAT with b the last rows of the exact tableau; dI[0] is 0 (there is no k_0)."""
    s, c, AE, AI, g = ir.exact(SCHEME)
    return [AE[s][j] - BHAT[j] for j in range(s + 1)], [AI[s][j] - BHAT[j] if j >= 1 else Fr(0) for j in range(s + 1)]


def estimate_terms(dt, R, mutant=None):
    """[(j, "E" or "I", coefficient in R)] in the kernel's order."""
    dE, dI = differences()
    dE, dI = [float(x) for x in dE], [float(x) for x in dI]
    if mutant == "swapped_dI":
        dI[1], dI[2] = dI[2], dI[1]
    if mutant == "dropped_term":
        dI[4] = 0.0
    out = []
    for j in range(5):
        e = R(dt * dE[j])
        if e != 0:
            out.append((j, "E", e))
        if j >= 1:
            i = R(dt * dI[j])
            if i != 0:
                out.append((j, "I", i))
    return out


def dense_estimate(stages, dt, mutant=None):
    """e of the step whose stages imex_reference.dense_step recorded, in float64."""
    e = 0.0
    for j, which, coef in estimate_terms(dt, np.float64, mutant):
        e = e + coef * (stages[j][4] if which == "E" else stages[j][2])
    return e


def wrms(e, y, rtol, atol):
    r = np.asarray(e, dtype=np.float64) / (rtol * np.abs(np.asarray(y, dtype=np.float64)) + atol)
    return float(math.sqrt(float(np.sum(r * r)) / r.size))


def dense_attempt(D, t, h, y, rtol, atol, mutant=None):
    """(y_new, norm) of one attempt of the dense restatement."""
    stages = []
    y1 = ir.dense_step(D, SCHEME, t, h, y, stages=stages)
    e = dense_estimate(stages, h, mutant)
    if mutant == "bhat_for_b":  # the step returns the embedded solution
        y1 = y1 - dense_estimate(stages, h)
    return y1, wrms(e, y1 if mutant == "weights_from_ynew" else y, rtol, atol)


# ---- the controller ---------------------------------------------------------------------------------------------------------------
def pid_eta(h, e, etamax, safety, etamin, h_cap, order):
    e1, e2, e3 = (max(x, TINY) for x in e)
    h_acc = h * math.pow(e1, -K1 / order) * math.pow(e2, K2 / order) * math.pow(e3, -K3 / order)
    h_acc *= safety
    h_acc = min(abs(h_acc), abs(etamax * h))
    h_acc = max(abs(h_acc), abs(etamin * h))
    if abs(h_acc) > abs(h * LBOUND * ONEMSM) and abs(h_acc) < abs(h * UBOUND * ONEPSM):
        h_acc = h
    eta = h_acc / h
    if math.isfinite(h_cap):
        eta /= max(1.0, abs(h) * eta / h_cap)
    return eta


class Control:
    """crd_imex_control.h: Control."""

    def __init__(self, t0, tout, h_first, h_max=0.0, safety=0.96, bias=1.5, growth=20.0, shrink=0.1, max_steps=200000, order=EMBEDDED_ORDER):
        self.safety, self.bias, self.growth, self.shrink, self.max_steps, self.order = safety, bias, growth, shrink, max_steps, order
        self.h_cap = h_max if h_max > 0.0 else math.inf
        self.t, self.tout = t0, tout
        self.h = min(h_first, self.h_cap)
        self.hprime, self.eta, self.etamax, self.nst = self.h, 1.0, ETAMX1, 0
        self.ehist = [1.0, 1.0, 1.0]
        self.attempts = self.accepted = self.rejected = self.nef = 0
        self.in_step = self.clipped = False
        self.wanted = self.h
        self.err_last = 0.0

    def done(self):
        return not self.t < self.tout

    def next(self):
        """(t_n, h) of the attempt to make, or the refusal's message (a str)."""
        if self.attempts >= self.max_steps:
            return TOO_MUCH_WORK
        if not self.in_step:
            if self.nst > 0 and self.hprime != self.h:
                self.h *= self.eta
            self.nef = 0
        if not self.h > 1e-14 * max(abs(self.t), 1e-300) and not (self.t == 0.0 and self.h > 0.0):
            return UNDERFLOW
        self.in_step = True
        self.wanted = self.h
        self.clipped = self.t + self.h >= self.tout or self.tout - (self.t + self.h) < 1e-12 * abs(self.tout)
        if self.clipped:
            self.h = self.tout - self.t
        self.attempts += 1
        return self.t, self.h

    def verdict(self, norm):
        self.err_last = self.bias * norm
        if not norm <= 1.0:
            self.nef += 1
            self.rejected += 1
            if self.nef == MAX_NEF:
                return -1
            self.etamax = 1.0
            e = [norm * self.bias if math.isfinite(norm) else 1e300, self.ehist[0], self.ehist[1]]
            eta = pid_eta(self.h, e, self.etamax, self.safety, self.shrink, self.h_cap, self.order)
            if self.nef >= SMALL_NEF:
                eta = min(eta, ETAMXF)
            self.h *= eta
            return 0
        self.ehist = [norm * self.bias, self.ehist[0], self.ehist[1]]
        if self.etamax == 1.0:
            self.hprime, self.eta = self.h, 1.0
        else:
            self.eta = pid_eta(self.h, self.ehist, self.etamax, self.safety, self.shrink, self.h_cap, self.order)
            self.hprime = self.h * self.eta
        self.etamax = self.growth
        self.t = self.tout if self.clipped else self.t + self.h
        self.nst += 1
        self.accepted += 1
        self.in_step = False
        return 1

    def h_next(self):
        if self.in_step or self.nst == 0:
            return min(self.h, self.h_cap)
        return min(max(self.wanted, self.hprime) if self.clipped else self.hprime, self.h_cap)


def ulps(a, b):
    """The distance of two finite doubles of one sign in units of the last place."""
    ia, ib = np.float64(a).view(np.int64), np.float64(b).view(np.int64)
    return abs(int(ia) - int(ib))


def integrate_dense(D, t0, tout, y, rtol, atol, h0, mutant=None, **control):
    """(y, Control, [(t, h, norm, accepted)]) of the dense restatement of the integrator."""
    K = Control(t0, tout, h0, **control)
    record = []
    while not K.done():
        nxt = K.next()
        if isinstance(nxt, str):
            raise RuntimeError(nxt)
        t, h = nxt
        y1, norm = dense_attempt(D, t, h, y, rtol, atol, mutant)
        if not (np.isfinite(y1).all() and math.isfinite(norm)):
            norm = math.nan
        verdict = K.verdict(norm)
        record.append((t, h, norm, verdict == 1))
        if verdict < 0:
            raise RuntimeError(ERR_FAILURE)
        if verdict == 1:
            y = y1
    return y, K, record


# ---- the close in the kernel's arithmetic -----------------------------------------------------------------------------------------
STORED = ((0, "E"), (1, "E"), (1, "I"), (2, "E"), (2, "I"), (3, "E"), (3, "I"))  # the probe's seven stored vectors, in the estimate's order


def close_reference(R, k, yn, stored, hg, dt, rtol, atol, precision, mutant=None):
    """(out, e, q) of the estimating close bit for bit: out and e in the device precision, q in float64, all shaped like R."""
    R_ = br.DTYPES[precision]
    fma = ir.fma_exact(R_)
    out = fma(R_(hg), k, R)
    vec = dict(zip(STORED, stored))
    vec[(4, "I")] = k
    e = None
    for j, which, coef in estimate_terms(dt, R_, mutant):
        x = np.asarray(vec[(j, which)], dtype=R_)
        e = (R_(coef) * x).astype(R_) if e is None else fma(coef, x, e)
    w = rtol * np.abs(np.asarray(yn, dtype=np.float64)) + atol
    r = np.asarray(e, dtype=np.float64) / w
    return out, e, r * r


def sum_bound(q, precision):
    """(ref, bound) of the device's sum of q: the long-double sum and gamma_K sum q."""
    L = np.longdouble
    ref = np.asarray(q).ravel().astype(L).sum()
    K = br.sum_roundings(np.asarray(q).size, precision)
    return ref, K * br.U64 / (1 - K * br.U64) * float(ref)


def selftest_build_command(exe, sanitizers=None):
    """g++ command line of tests/native/imex_control_selftest.cpp (plain C++17 against crd_imex_tables.h, crd_imex_control.h, crd_arkode.h)."""
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "crdmodel_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "imex_control_selftest.cpp"), "-o", str(exe)]
    if sanitizers:
        cmd[4:4] = ["-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizers, "-fno-sanitize-recover=all"]
    return cmd
