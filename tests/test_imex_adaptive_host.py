"""The error-controlled IMEX integrator's host side, without a GPU (crd_integrate_imex; tests/imex_adaptive_reference.py):

1. the embedded weights of ARS(4,4,3) in Fractions: order 2 and not 3, the difference rows, damping at infinity;
2. tests/native/imex_control_selftest.cpp as a program, plain and under ASan + UBSan: the header's doubles and estimate_terms' order and
   omissions against the Python restatement bit for bit, the order-3 controller unchanged bit for bit, and scripted norm sequences through
   the order-2 controller against the Python restatement to 4 ulps;
3. the dense restatement: the estimate's observed order, runs to T = 2 at four tolerances against a small-step RK4 solution, and
   mutants that each fail the gate imex_adaptive_reference.MUTANT_GATES names;
4. what can be refused without a device: the driver's option parser, a call without a context, the ctypes mirror's layout.
"""
import ctypes as C
import functools
import math
import os
import subprocess
from fractions import Fraction as Fr

import numpy as np
import pytest

import crdmodel_amd as crd
import imex_adaptive_reference as ar
import imex_reference as ir
from test_imex_host import DRIVER_REFUSALS, INI, run_driver, smooth_problem

ROOT = ar.ROOT
K = crd._capi


# ---- 1. the weights ---------------------------------------------------------------------------------------------------------------
def test_embedded_weights_are_of_order_two_and_not_three():
    s, c, AE, AI, g = ir.exact("ars443")
    b = ar.BHAT
    # both matrices have row sums c, so sum bhat = 1 and bhat.c = 1/2 are all four additive second-order conditions
    for A in (AE, AI):
        assert all(sum(A[i]) == c[i] for i in range(s + 1))
    assert sum(b) == 1 and sum(b[j] * c[j] for j in range(s + 1)) == Fr(1, 2)
    for A in (AE, AI):  # the same two, written with each matrix: bhat.(A e)
        assert sum(b[i] * sum(A[i]) for i in range(s + 1)) == Fr(1, 2)
    assert sum(b[j] * c[j] ** 2 for j in range(s + 1)) == Fr(1, 4) != Fr(1, 3)
    assert b[0] == 0 and b[s] == 0  # one vector serves both parts (there is no k_0), and FR_4 is not needed


def test_difference_rows():
    s, c, AE, AI, g = ir.exact("ars443")
    dE, dI = ar.differences()
    assert dE == [Fr(1, 4), Fr(-3, 4), Fr(3, 4), Fr(-1, 4), 0] and dI == [0, Fr(-1), Fr(-3, 2), Fr(2), Fr(1, 2)]
    for d, A in ((dE, AE), (dI, AI)):
        assert d == [A[s][j] - ar.BHAT[j] for j in range(s + 1)]
        assert sum(d) == 0 and sum(d[j] * c[j] for j in range(s + 1)) == 0
    # every coefficient is exact in binary: a power-of-two denominator
    assert all(x.denominator & (x.denominator - 1) == 0 for x in dE + dI + ar.BHAT)


def solve_exact(A, rhs):
    """A^-1 rhs in Fractions by Gaussian elimination."""
    n = len(A)
    M = [list(A[i]) + [rhs[i]] for i in range(n)]
    for col in range(n):
        piv = next(r for r in range(col, n) if M[r][col] != 0)
        M[col], M[piv] = M[piv], M[col]
        M[col] = [x / M[col][col] for x in M[col]]
        for r in range(n):
            if r != col and M[r][col] != 0:
                M[r] = [x - M[r][col] * y for x, y in zip(M[r], M[col])]
    return [M[i][n] for i in range(n)]


def test_damped_at_infinity():
    s, c, AE, AI, g = ir.exact("ars443")
    block = [[AI[i][j] for j in range(1, s + 1)] for i in range(1, s + 1)]
    z = solve_exact(block, [Fr(1)] * s)
    damping = lambda w: 1 - sum(w[j] * z[j] for j in range(s))
    assert damping(ar.BHAT[1:]) == 0
    assert damping(AI[s][1:]) == 0  # b itself: stiffly accurate
    # the one-parameter family of the issue: x = 1/2 is b, x = 0 the embedded weights
    family = lambda x: [Fr(5, 2) - 2 * x, -3 * x, 4 * x - Fr(3, 2), x]
    assert family(Fr(1, 2)) == AI[s][1:] and family(Fr(0)) == ar.BHAT[1:]
    for x in (Fr(1, 3), Fr(-2), Fr(7, 5)):
        assert damping(family(x)) == 0 and sum(family(x)) == 1 and sum(w * cj for w, cj in zip(family(x), c[1:])) == Fr(1, 2)
    # "the obvious one" for ARS(2,2,2) is not damped: first-order weights (1, 0) on its implicit block amplify stiff modes
    s2, c2, AE2, AI2, g2 = ir.exact("ars222")
    z2 = np.linalg.solve(np.array([[AI2[i][j] for j in (1, 2)] for i in (1, 2)]), np.ones(2))
    assert abs(abs(1 - z2[0]) - 2.4) < 0.02


# ---- 2. the native self-test ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def selftest_output(tmp, sanitizers):
    exe = os.path.join(tmp, "imex_control_selftest" + ("_san" if sanitizers else ""))
    build = subprocess.run(ar.selftest_build_command(exe, sanitizers), capture_output=True, text=True)
    if sanitizers and build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        return None
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "imex control selftest ok" in run.stdout
    return run.stdout


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("imex_control"))


@pytest.mark.parametrize("sanitizers", [None, "address,undefined"])
def test_selftest_tables_bit_for_bit(build_dir, sanitizers):
    out = selftest_output(build_dir, sanitizers)
    if out is None:
        pytest.skip("sanitizer runtimes not installed")
    dE, dI = ar.differences()
    seen, want, terms = 0, None, None
    for line in out.splitlines():
        w = line.split()
        if w[0] == "embedded":
            assert int(w[1]) == ar.EMBEDDED_ORDER
        elif w[0] in ("bhat", "dE", "dI"):
            exact = {"bhat": ar.BHAT, "dE": dE, "dI": dI}[w[0]]
            assert float.fromhex(w[2]) == float(exact[int(w[1])]), line
            seen += 1
        elif w[0] == "terms":
            assert not want, (want, "terms left over")
            R = np.float32 if int(w[1]) else np.float64
            want = ar.estimate_terms(float.fromhex(w[2]), R)
            assert int(w[3]) == len(want)
        elif w[0] == "term":
            j, which, coef = want.pop(0)
            assert (int(w[1]), w[2], float.fromhex(w[3])) == (j, which, float(coef)), line
        elif w[0] == "order3":
            assert int(w[1]) > 1000 and w[2] == "identical"
    assert seen == 5 + 5 + 4 and not want
    # the order and the omissions themselves
    assert [(j, which) for j, which, _ in ar.estimate_terms(0.3, np.float64)] == list(ar.STORED) + [(4, "I")]
    assert ar.estimate_terms(1e-60, np.float32) == [] and len(ar.estimate_terms(1e-60, np.float64)) == 8


def scenarios(out):
    """[(name, header floats, max_steps, [(t, h, norm, verdict)], (t, h_next, accepted, rejected, attempts, why))]"""
    found, cur = [], None
    for line in out.splitlines():
        w = line.split()
        if w[0] == "scenario":
            cur = [w[1], [float.fromhex(x) for x in w[2:7]], int(w[7]), [], None]
            found.append(cur)
        elif w[0] == "attempt":
            cur[3].append((float.fromhex(w[1]), float.fromhex(w[2]), float.fromhex(w[3]) if w[3] != "nan" else math.nan, int(w[4])))
        elif w[0] == "end":
            cur[4] = (float.fromhex(w[1]), float.fromhex(w[2]), int(w[3]), int(w[4]), int(w[5]), " ".join(w[6:]))
    return found


def test_controller_scenarios_against_the_restatement(build_dir):
    """Every attempt's t and h of the C++ controller within 4 ulps of the Python restatement's fed the same norms (pow may differ in its
    last bit; everything else is the same operations), the verdicts and the counts equal; and each scenario shows what it is named for."""
    found = {s[0]: s for s in scenarios(selftest_output(build_dir, None))}
    assert set(found) == {"accept", "reject", "second_failure", "seventh_failure", "growth_cap", "h_max", "shortened_last_step", "stretched_last_step", "one_exact_step",
                          "max_steps_1", "no_interval"}
    for name, (t0, tout, h_first, h_max, growth), max_steps, attempts, end in found.values():
        P = ar.Control(t0, tout, h_first, h_max=h_max, growth=growth, max_steps=max_steps)
        failed = False
        for t, h, norm, verdict in attempts:
            assert not P.done()
            nxt = P.next()
            assert not isinstance(nxt, str), (name, nxt)
            assert ar.ulps(nxt[0], t) <= 4 and ar.ulps(nxt[1], h) <= 4, (name, nxt, (t, h))
            assert P.verdict(norm) == verdict, (name, t, h, norm)
            failed = verdict < 0
        assert ar.ulps(P.t, end[0]) <= 4 and ar.ulps(P.h_next(), end[1]) <= 4 and (P.accepted, P.rejected, P.attempts) == end[2:5], (name, end)
        if P.done():
            why = "done"
        elif failed:
            why = ar.ERR_FAILURE
        else:  # the script ran out, or the controller refuses the next attempt
            nxt = P.next()
            why = nxt if isinstance(nxt, str) else "script"
        assert why == end[5], (name, why, end[5])
    hs = lambda name: [a[1] for a in found[name][3]]
    verdicts = lambda name: [a[3] for a in found[name][3]]
    # accept: the first step may grow by 10000 (it grows by what the PID rule gives), then the dead band holds h
    assert all(v == 1 for v in verdicts("accept")) and hs("accept")[-1] == hs("accept")[-2]
    # reject: a smaller retry, and the step after a failed one keeps its size
    assert verdicts("reject")[:2] == [0, 1] and hs("reject")[1] < hs("reject")[0] and hs("reject")[2] == hs("reject")[1]
    # second failure: at most 0.3 of the step before
    assert verdicts("second_failure")[:3] == [0, 0, 1] and hs("second_failure")[2] <= 0.3 * hs("second_failure")[1] * (1 + 1e-15)
    # seventh failure: the call ends; a NaN norm is a failed test
    assert verdicts("seventh_failure") == [1, 0, 0, 0, 0, 0, 0, -1] and found["seventh_failure"][4][5] == ar.ERR_FAILURE
    # growth cap: 10000 on the first step at most, 20 afterwards; h_max caps it
    g = hs("growth_cap")
    assert g[1] / g[0] <= 10000 * (1 + 1e-15) and g[1] / g[0] > 20 and all(abs(g[k + 1] / g[k] - 20.0) < 1e-12 for k in range(1, 5))
    assert max(hs("h_max")) == 0.75 == found["h_max"][4][1]
    # the last step lands on tout exactly, shortened or stretched; h_next is not less than the step that was shortened
    for name in ("shortened_last_step", "stretched_last_step", "one_exact_step"):
        tout = found[name][1][1]
        assert found[name][4][0] == tout and found[name][4][5] == "done"
    assert hs("shortened_last_step")[-1] < hs("shortened_last_step")[-2] == found["shortened_last_step"][4][1]
    assert hs("stretched_last_step")[-1] > hs("stretched_last_step")[0] and len(hs("stretched_last_step")) == 2
    assert hs("one_exact_step") == [0.125]
    # max_steps counts attempts: one rejected attempt and the call is over, h_next the smaller step
    assert verdicts("max_steps_1") == [0] and found["max_steps_1"][4][5] == ar.TOO_MUCH_WORK and found["max_steps_1"][4][1] < 0.5
    assert found["no_interval"][3] == [] and found["no_interval"][4][:2] == (3.0, 0.5)


def test_order_three_controller_is_the_oracles():
    """The Python restatement at order 3 is oracle/arkode_erk.pid_eta, which the existing integrator is held to: same expression, same bits."""
    from oracle import arkode_erk as ae

    for h in (1e-3, 0.37):
        for e in ([0.3, 1.0, 1.0], [2.5, 0.4, 0.1], [1e-12, 0.02, 0.7]):
            for etamax in (1.0, 20.0, 10000.0):
                assert ar.pid_eta(h, e, etamax, ae.SAFETY, ae.ETAMIN, math.inf, 3) == ae.pid_eta(h, e, etamax)
                assert ar.pid_eta(h, e, etamax, ae.SAFETY, ae.ETAMIN, 0.5, 3) == ae.pid_eta(h, e, etamax, 0.5)


def test_the_control_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "crdmodel_amd", "csrc", "crd_imex_control.h")).read()
    assert [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")] == ["<cmath>", "<cstdint>", '"crd_arkode.h"']
    assert not [word for word in ("hip/", "hipError_t", "hipStream_t", "__global__", "__device__") if word in text]


# ---- 3. the dense restatement -----------------------------------------------------------------------------------------------------
# The estimate is the local error of the second-order solution, so its size falls with dt^3 and the observed slope tends to 3; 2 and 4
# are the neighbours it has to be told from: (2.5, 3.5).  Halvings: one step from t = 0 of T / 16, T / 32, T / 64 with T = 0.4 (dt =
# 0.025, 0.0125, 0.00625); coarser ones are not yet in the bracket (2.27, 2.57 at T / 4 -> T / 8 -> T / 16 on the flat surface).
HALVINGS = (16, 32, 64)


def estimate_slopes(D, y0, T, mutant=None):
    sizes = []
    for n in HALVINGS:
        stages = []
        ir.dense_step(D, "ars443", 0.0, T / n, y0, stages=stages)
        sizes.append(float(np.linalg.norm(ar.dense_estimate(stages, T / n, mutant))))
    return [float(np.log2(sizes[k] / sizes[k + 1])) for k in range(2)], sizes


def gate_estimate_order(D, y0, T, mutant=None):
    got, sizes = estimate_slopes(D, y0, T, mutant)
    return all(2.5 < s < 3.5 for s in got), got, sizes


@pytest.mark.parametrize("surface", ["flat", "torus"])
def test_estimate_order(surface):
    D, y0, T, _ = smooth_problem(surface)
    ok, got, sizes = gate_estimate_order(D, y0, T)
    print("ESTIMATE ORDER %s: sizes %s, slopes %s" % (surface, ["%.3g" % e for e in sizes], ["%.2f" % s for s in got]))
    assert ok, got
    # the sizes the issue records at dt = 0.025 and 0.0125
    want = {"flat": (0.00166, 0.000245), "torus": (0.00210, 0.000326)}[surface]
    assert all(abs(a - b) <= 0.01 * b for a, b in zip(sizes[:2], want))


def gate_solution_order(D, y0, T, ref, mutant=None):
    """The accepted solution is the third-order one: fixed steps T / 4, T / 8, T / 16 against the reference, slopes in (2.5, 3.5)."""
    errs = []
    for n in (4, 8, 16):
        y = y0
        for i in range(n):
            y, _ = ar.dense_attempt(D, i * T / n, T / n, y, 1e-4, 1e-6, mutant)
        errs.append(float(np.linalg.norm(y - ref)))
    got = [float(np.log2(errs[k] / errs[k + 1])) for k in range(2)]
    return all(2.5 < s < 3.5 for s in got), got


def gate_norm_weights(D, y0, mutant=None):
    """The attempt's norm is formed with the weights of the step's START: written out by hand from the recorded stages."""
    rtol, atol, h = 1e-4, 1e-6, 0.2
    stages = []
    ir.dense_step(D, "ars443", 0.0, h, y0, stages=stages)
    e = ar.dense_estimate(stages, h)
    want = math.sqrt(sum((x / (rtol * abs(y) + atol)) ** 2 for x, y in zip(e.ravel(), y0.ravel())) / e.size)
    _, got = ar.dense_attempt(D, 0.0, h, y0, rtol, atol, mutant)
    return abs(got - want) <= 1e-12 * want, got, want


def test_solution_order_and_norm_weights():
    D, y0, T, ref = smooth_problem("flat")
    assert gate_solution_order(D, y0, T, ref)[0]
    assert gate_norm_weights(D, y0)[0]


@functools.lru_cache(maxsize=None)
def long_reference(surface):
    """RK4 of the oracle's f at T / 16384 to T = 2 (the issue's reference)."""
    D, y0, _, _ = smooth_problem(surface)
    return ir.rk4_steps(D, 0.0, 2.0 / 16384, 16384, y0)


@pytest.mark.parametrize("surface", ["flat", "torus"])
def test_runs_follow_the_tolerance(surface):
    """The restated integrator to T = 2 at rtol = 1e-3 .. 1e-6, atol = rtol / 100, h0 = 1e-3: the error against RK4 at T / 16384 is within
    10 rtol in the 2-norm, and the accepted counts rise as the tolerance tightens.  Measured here with the PID controller: 13 / 26 / 55 /
    115 accepted steps (flat), 13 / 27 / 57 / 120 (torus), no rejections, errors 1.9 / 2.6 / 2.5 / 3.0 x rtol (flat), 2.8 / 2.5 / 2.8 /
    3.3 x rtol (torus); the largest steps 0.30 / 0.21 / 0.087 / 0.059 (flat) against crd_stable_dt = 0.029."""
    D, y0, _, _ = smooth_problem(surface)
    ref = long_reference(surface)
    counts = []
    for rtol in (1e-3, 1e-4, 1e-5, 1e-6):
        y, C_, record = ar.integrate_dense(D, 0.0, 2.0, y0, rtol, rtol / 100, 1e-3)
        err = float(np.linalg.norm(y - ref))
        print("RUN %s rtol %.0e: %d accepted, %d rejected, error %.3g = %.2f rtol, largest step %.3g" % (surface, rtol, C_.accepted, C_.rejected, err, err / rtol,
                                                                                                         max(r[1] for r in record)))
        assert C_.t == 2.0 and err <= 10 * rtol, (rtol, err)
        counts.append(C_.accepted)
    assert counts == sorted(counts) and len(set(counts)) == 4, counts


@pytest.mark.parametrize("mutant", ar.MUTANTS)
def test_mutants_fail_their_gate(mutant):
    D, y0, T, ref = smooth_problem("flat")
    gate = ar.MUTANT_GATES[mutant]
    if gate == "estimate_order":
        assert not gate_estimate_order(D, y0, T, mutant)[0]
    elif gate == "norm_weights":
        assert not gate_norm_weights(D, y0, mutant)[0]
    else:
        assert gate == "solution_order" and not gate_solution_order(D, y0, T, ref, mutant)[0]


# ---- 4. refusals without a device, and the mirror ---------------------------------------------------------------------------------
ADAPTIVE_REFUSALS = [
    (["--imex-adaptive"], "--imex-adaptive controls the error of ARS(4,4,3), the one scheme with an embedded solution: only with --imex ars443"),
    (["--imex", "ars222", "--imex-adaptive"], "--imex-adaptive controls the error of ARS(4,4,3), the one scheme with an embedded solution: only with --imex ars443"),
    (["--imex-adaptive", "--imex", "euler"], "--imex-adaptive controls the error of ARS(4,4,3), the one scheme with an embedded solution: only with --imex ars443"),
    (["--imex", "ars443", "--imex-adaptive", "--adaptive"], "--imex steps at the run's fixed dt: not with --adaptive / --adaptive-rk43"),
    (["--imex", "ars443", "--imex-adaptive", "--adaptive-rk43"], "--imex steps at the run's fixed dt: not with --adaptive / --adaptive-rk43"),
    (["--imex", "ars443", "--imex-adaptive", "--gpus", "2"], "--imex steps a lone single-slab run: not with --gpus 2"),
    (["--imex", "ars443", "--imex-adaptive", "--ensemble", "beta=1.0,1.5"], "--imex steps a lone single-slab run: not with --ensemble"),
    (["--imex", "ars443", "--imex-adaptive", "--observe", "2", "--probe", "1,1"], "--imex takes no recorder samples: not with --observe"),
]


@pytest.mark.parametrize("args,message", ADAPTIVE_REFUSALS, ids=[" ".join(a) for a, _ in ADAPTIVE_REFUSALS])
def test_driver_refuses_with_a_message(args, message, tmp_path):
    r = run_driver(args, INI, tmp_path)
    assert r.returncode == 1 and r.stdout == "" and r.stderr == "\nCRD_ERROR: " + message + "\n\n", (r.stdout, r.stderr)
    assert not os.listdir(tmp_path)


def test_driver_still_refuses_a_fixed_imex_run_without_a_step(tmp_path):
    """--imex without --imex-adaptive at dt = 0 is refused as before; and the ini's adaptive = 1 is refused with --imex-adaptive too."""
    assert any("--adaptive" in a for a, _ in DRIVER_REFUSALS)  # (the unchanged refusals themselves: tests/test_imex_host.py)
    text = open(INI).read()
    for line, args, needle in (("dt = 0", ["--imex", "ars443"], "--imex needs the run's fixed step"),
                               ("dt = 0.02\nadaptive = 1", ["--imex", "ars443", "--imex-adaptive"], "[Solver] adaptive = 1 (pass --fixed)")):
        ini = tmp_path / ("run%d.ini" % len(line))
        ini.write_text(text.replace("dt = 0.02\ngpus = 1", line + "\ngpus = 1"))
        out = tmp_path / ("out%d" % len(line))
        out.mkdir()
        r = run_driver(args, ini, out)
        assert r.returncode == 1 and needle in r.stderr and r.stderr.startswith("\nCRD_ERROR: --imex"), r.stderr
        assert not os.listdir(out)


def test_calls_without_a_context_and_the_mirror():
    L = K.lib()
    opt, st = K.ImexAdaptiveOptions(), K.ImexAdaptiveStats()
    assert L.crd_imex_adaptive_defaults(None) == K.EINVAL and L.crd_imex_adaptive_defaults(C.byref(opt)) == K.OK
    assert (opt.imex.scheme, opt.imex.solver) == (K.IMEX_SCHEMES["ars443"], K.IMEX_SOLVERS["gmres"])
    assert (opt.rtol, opt.atol, opt.h0, opt.h_max, opt.safety, opt.bias, opt.growth, opt.shrink, opt.max_steps) == (1e-5, 1e-10, 0.0, 0.0, 0.96, 1.5, 20.0, 0.1, 200000)
    assert L.crd_integrate_imex(None, 0.0, 1.0, C.byref(opt), C.byref(st), None, 0) == K.EINVAL
    assert L.crd_imex_estimate_probe(None, None, None, None, None) == K.EINVAL
    assert C.sizeof(K.ImexAdaptiveOptions) == C.sizeof(K.ImexOptions) + 8 * 8 + 8
    assert C.sizeof(K.ImexAdaptiveStats) == C.sizeof(K.ImexStats) + 4 * 8 + 7 * 8 and C.sizeof(K.ImexAttempt) == 3 * 8 + 2 * 4
    header = open(os.path.join(ROOT, "include", "crd.h")).read()
    for name in ("crd_imex_adaptive_options", "crd_imex_adaptive_stats", "crd_imex_attempt", "crd_integrate_imex", "crd_imex_estimate_probe", "crd_imex_adaptive_defaults"):
        assert name in header
    assert "bhat = (0, 5/2, 0, -3/2, 0)" in header and "dE = (1/4, -3/4, 3/4, -1/4)" in header and "dI = (-1, -3/2, 2, 1/2)" in header
