"""The gates of the step controller's reductions (tests/controller_reference.py) on the host: the oracle's arkHin trace is arkHin, every
input the device test runs isolates the scalar it is meant to, and the checks have the power claimed for them -- fed what a wrong
reduction would return (controller_reference.MUTANTS) they fail, fed the unmutated restatement they pass.  No kernel has to be broken
on a device to show that tests/test_gpu_controller_reductions.py would notice."""
import math

import numpy as np
import pytest

import controller_reference as cr
from conftest import load_golden, oracle_problem
from oracle import arkode_erk as ark
from oracle import crd_oracle as co
from oracle import error_bounds as eb


def initial_step_before_the_trace(rhs, t0, y0, f0, tout, rtol, atol):
    """oracle/arkode_erk.initial_step as it stood before initial_step_trace took over its body: the bits the wrapper has to return."""
    tdist = abs(tout - t0)
    tround = ark.UROUND * max(abs(t0), abs(tout))
    hlb = ark.H0_LBFACTOR * tround
    hub_inv = float(np.max(np.abs(f0) / (ark.H0_UBFACTOR * np.abs(y0) + (rtol * np.abs(y0) + atol))))
    hub = ark.H0_UBFACTOR * tdist
    if hub * hub_inv > 1.0:
        hub = 1.0 / hub_inv
    hg = math.sqrt(hlb * hub)
    if hub < hlb:
        return hg
    w = ark.error_weights(y0, rtol, atol)
    hnew_ok, hnew = False, hg
    for count in range(1, ark.H0_ITERS + 1):
        ydd = (rhs(t0 + hg, y0 + hg * f0) - f0) * (1.0 / hg)
        yddnrm = ark.wrms(ydd, w)
        if hnew_ok or count == ark.H0_ITERS:
            hnew = hg
            break
        hnew = math.sqrt(2.0 / yddnrm) if yddnrm * hub * hub > 2.0 else math.sqrt(hg * hub)
        hrat = hnew / hg
        if 0.5 < hrat < 2.0:
            hnew_ok = True
        if count > 1 and hrat > 2.0:
            hnew, hnew_ok = hg, True
        hg = hnew
    return min(max(ark.H0_BIAS * hnew, hlb), hub)


def slab_extents():
    import crdmodel_amd as crd  # (host arithmetic of libcrd: no device)

    return [crd.slab_extents(cr.GROUP_GRID[1], k, cr.GROUP_SLABS) for k in range(cr.GROUP_SLABS)]


@pytest.mark.parametrize("name", ["rk4_fhn_torus_outside", "rk4_goldbeter_torus"])
def test_trace_reproduces_initial_step_bit_for_bit(name):
    meta, arr = load_golden(name)
    op = oracle_problem(meta)
    rhs = lambda t, y: co.rhs(op, t, y)  # noqa: E731
    y0 = arr["y0"]
    f0 = rhs(0.0, y0)
    planted = y0.copy()
    planted[3, 5, 0] = 0.0
    fp = rhs(0.0, planted)
    for y, f, tout, rtol, atol in ((y0, f0, 0.5, 1e-5, 1e-10), (y0, f0, 0.05, 1e-5, 1e-10), (y0, f0, 0.5, 1e-2, 1e-4), (planted, fp, 0.5, 1e-2, 1e-4),
                                   (planted, fp, 0.5, 1e-2, 1e-30), (y0, f0, 0.5, 0.0, 1e-6)):
        want = initial_step_before_the_trace(rhs, 0.0, y, f, tout, rtol, atol)
        tr = ark.initial_step_trace(rhs, 0.0, y, f, tout, rtol, atol)
        assert tr["h0"] == want and ark.initial_step(rhs, 0.0, y, f, tout, rtol, atol) == want
        # the trace says what it did
        ratio = np.abs(f) / (0.1 * np.abs(y) + (rtol * np.abs(y) + atol))
        assert tr["hub_inv"] == float(np.max(ratio)) and ratio.ravel()[tr["argmax"]] == tr["hub_inv"]
        assert tr["clamped"] == (tr["hub"] != 0.1 * tout) and tr["hlb"] == 100.0 * ark.UROUND * tout
        assert tr["count"] == len(tr["iterations"]) and (tr["count"] == 0) == (tr["hub"] < tr["hlb"])
        if tr["count"]:
            assert [it["formula"] for it in tr["iterations"]].count(None) == 1 and tr["iterations"][-1]["formula"] is None
            assert tr["ydd_terms"].shape == y.shape
            assert math.sqrt(float(np.sum(tr["ydd_terms"])) / y.size) == tr["iterations"][-1]["yddnrm"]
            assert tr["iterations"][0]["hg"] == math.sqrt(tr["hlb"] * tr["hub"])
    with pytest.raises(ValueError):
        ark.initial_step_trace(rhs, 1.0, y0, f0, 1.0, 1e-5, 1e-10)


def test_default_tolerances_hide_the_bound():
    """Why the regimes are needed: at the defaults, on the goldens and first output times the suite runs (tests/test_gpu_parity.py), a
    bound reduction that returns nothing moves the first step by less than the rel = 1e-6 it is compared at, or barely more."""
    for name, tout, most in (("rk4_fhn_torus_outside", 0.5, 1e-6), ("rk4_goldbeter_torus", 0.05, 2e-6)):
        meta, arr = load_golden(name)
        op = oracle_problem(meta)
        y0 = arr["y0"]
        f0 = co.rhs(op, 0.0, y0)
        ay = np.abs(y0)
        want = ark.initial_step(lambda t, y: co.rhs(op, t, y), 0.0, y0, f0, tout, 1e-5, 1e-10)
        got = cr.hin_scalar(0.0, tout, 0.0, lambda hg: ark.wrms((co.rhs(op, hg, y0 + hg * f0) - f0) * (1.0 / hg), 1.0 / (1e-5 * ay + 1e-10)))
        assert abs(got - want) <= most * want, (name, got, want)


def test_f_at_the_plant_is_the_whole_grids():
    nx, ny = cr.SMALL
    for precision in ("f64", "f32"):
        for model in cr.MODELS:
            op = cr.problem(model, nx, ny)
            y = cr.state(nx, ny, 5, precision)
            ref, bu, bv = eb.rhs_bound(op, cr.T0, y, precision)
            for q in cr.small_positions(nx * ny) + [nx, nx * (ny - 1) - 1]:
                j, i = divmod(q, nx)
                f, u, v = cr.f_at(op, y, precision, j, i)
                assert np.array_equal(f, ref[j, i]) and u == bu[j, i] and v == bv[j, i], (precision, model, q)


def every_arkhin_case():
    sets = [cr.lone_bound_cases(), cr.lone_exit_cases(), cr.lone_ydd_cases(), cr.group_cases(slab_extents()), cr.compaction_set()]
    return [c for s in sets for c in s] + [c for _, members in cr.ensemble_sets() for c in members]


def test_every_device_input_meets_its_regime():
    """argmax at the plant, runner-up at most half, no y'' formula (bound regime); every formula y'' and one term at least half the
    sum (y'' regime); hub < hlb (exit) -- for every input of the device test, and the tolerance it is given is a rounding bound."""
    cases = every_arkhin_case()
    planted = [c for c in cases if c.q is not None]
    assert len(planted) >= 100
    for c in cases:
        r = cr.reference(c)
        r.assert_regime()
        if c.q is not None and c.regime != "ydd":
            assert 8 * cr.U64 <= r.allowed <= (2e-14 if c.precision == "f64" else 2e-6), (cr.case_name(c), r.allowed)
    # the unplanted members of the compaction set tell their states apart; in the bound regime they would not
    a, _, b = [cr.reference(c).h0 for c in cr.compaction_set()]
    assert abs(a - b) > 1e-3 * a


# ---- the power of the checks -----------------------------------------------------------------------------------------------------
def rejected(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def lone_gate(cases, extents=None):
    def run(mutant):
        return [rejected(cr.reference(c).check, cr.h_first_model(c, mutant, extents)) for c in cases]
    return run


def ensemble_gate(sets):
    def run(mutant):
        out = []
        for _, members in sets:
            h = cr.ensemble_model(members, mutant)
            out.append(any(rejected(cr.reference(c).check, hk) for c, hk in zip(members, h)))
        return out
    return run


def max_abs_gate(sets, cap):
    def run(mutant):
        return [rejected(cr.check_max_abs, fields, cr.max_abs_model(fields, cap, mutant)) for fields in sets]
    return run


KERNEL_MUTANTS = ["drop_last", "drop_tail_block", "first_trip", "first_wavefront"]


def gates():
    """(name, run(mutant) -> [rejected per input], the mutants this gate must reject on at least one of its inputs)."""
    ens = cr.ensemble_sets()
    ens_max = [f for precision in ("f64", "f32") for mixed in (False, True) for _, _, f in cr.max_abs_sets(precision, mixed)]
    return [
        ("lone bound", lone_gate(cr.lone_bound_cases(("f64",))), KERNEL_MUTANTS + ["var0_only"]),
        ("lone exit", lone_gate(cr.lone_exit_cases()), ["drop_last", "drop_tail_block", "var0_only"]),
        ("lone y''", lone_gate(cr.lone_ydd_cases()), KERNEL_MUTANTS),
        ("group", lone_gate(cr.group_cases(slab_extents()), slab_extents()), ["slab0_only", "var0_only"]),
        ("ensemble bound", ensemble_gate([s for s in ens if s[0].startswith("bound")]), KERNEL_MUTANTS + ["var0_only", "slot_shift"]),
        ("ensemble y''", ensemble_gate([s for s in ens if s[0].startswith("ydd")]), KERNEL_MUTANTS + ["slot_shift"]),
        ("ensemble compaction", ensemble_gate([("", cr.compaction_set())]), ["slot_shift"]),
        ("ensemble max-abs", max_abs_gate(ens_max, cr.ENS_MAXABS_CAP), KERNEL_MUTANTS + ["slot_shift", "no_abs", "var1_counted"]),
        ("lone max-abs", max_abs_gate([[f] for precision in ("f64", "f32") for _, f in cr.lone_max_abs_fields(precision)], cr.LONE_CAP),
         ["drop_last", "first_trip", "first_wavefront", "no_abs", "var1_counted"]),
    ]


@pytest.fixture(scope="module")
def all_gates():
    return gates()


def test_the_unmutated_restatement_passes_every_gate(all_gates):
    for name, run, _ in all_gates:
        verdicts = run(None)
        assert verdicts and not any(verdicts), (name, [k for k, v in enumerate(verdicts) if v])


@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_every_mutant_is_rejected(all_gates, mutant):
    """... by every gate that claims it, on at least one of the gate's planted inputs; and each of the listed mutants is claimed."""
    claimed = [(name, run) for name, run, mutants in all_gates if mutant in mutants]
    assert claimed, mutant
    for name, run in claimed:
        verdicts = run(mutant)
        assert any(verdicts), (mutant, "passes the gate", name)
        print("MUTANT %s: gate '%s' rejects it on %d of %d inputs" % (mutant, name, sum(verdicts), len(verdicts)))


def test_max_abs_check_is_exact_and_nan_aware():
    nx, ny = cr.SMALL
    fields = [cr.max_abs_fields(nx, ny, "f32", 1, 7), cr.max_abs_fields(nx, ny, "f32", 2, 9, -1.0, nan_at=100)]
    good = cr.max_abs_model(fields, cr.ENS_MAXABS_CAP)
    assert good[0] == cr.MAXABS_EXTREME and math.isnan(good[1])
    cr.check_max_abs(fields, good)
    assert rejected(cr.check_max_abs, fields, [float(np.nextafter(good[0], 8.0)), good[1]])
    assert rejected(cr.check_max_abs, fields, [good[0], cr.MAXABS_EXTREME])  # a NaN that did not propagate
    assert rejected(cr.check_max_abs, fields, [float("nan"), good[1]])      # ... or that leaked into a neighbour
