"""The step controller's reductions on the device: the arkHin bound, the y'' norm and max |u| of lone contexts, slab groups, the RCCL
self-ring and ensembles, each made to decide h_first (or the guard's value) alone and held to a derived tolerance.

tests/controller_reference.py has the regimes, the planted positions, the tolerances and the checks; tests/test_controller_reductions_host.py
shows on the host that these checks reject what a wrong reduction would return.  Every h_first here comes from
integrate_adaptive(0, 0.5, rtol, atol, h_max = -1) on a fresh upload; what the call does after its first attempt is not looked at (an
ensemble is stopped after one step, max_steps = 1: its members' stats come back with their status; a context's stats come back only
from a call that ends well, so it runs on to tout).  Only the crd Python API is used, and no torch (see tests/test_gpu_multigrid.py).

Worst observed / allowed measured on MI355X (printed with -s as "BOUND ..."): see DESIGN.md section 2.
"""
import numpy as np
import pytest

import controller_reference as cr
import crdmodel_amd as crd
from oracle import arkode_erk as ark
from oracle import crd_oracle as co

pytestmark = pytest.mark.gpu

K = crd._capi


def params_of(model, nx, ny, precision):
    return crd.make_params(model, "torus", nx, cr.L, cr.W, cr.D, cr.MODELS[model][1], ny=ny, precision=precision)


def case_params(c):
    return params_of(c.model, c.nx, c.ny, c.precision)


def options(c, **more):
    rtol, atol = cr.REGIMES[c.regime]
    return dict(rtol=rtol, atol=atol, h_max=-1.0, **more)


def h_first_of(ctx, c, y=None):
    """h_first of a fresh upload of case c's state on a Slab or a LocalGroup."""
    ctx.upload(cr.planted_state(c) if y is None else y)
    return ctx.integrate_adaptive(cr.T0, cr.TOUT, **options(c))["h_first"]


def report(name, ratios):
    print("BOUND %s: worst observed / allowed relative error of h_first %.3g over %d inputs" % (name, max(ratios), len(ratios)))


def run_lone(name, cases):
    """Cases that share a grid and a precision share a context."""
    ratios = []
    slabs = {}
    try:
        for c in cases:
            r = cr.reference(c)
            r.assert_regime()
            key = (c.model, c.nx, c.ny, c.precision)
            if key not in slabs:
                slabs[key] = crd.Slab(case_params(c))
            ratios.append(r.check(h_first_of(slabs[key], c)))
    finally:
        for s in slabs.values():
            s.close()
    report(name, ratios)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_lone_bound_regime_every_position(gpu_device, precision):
    """crd_hin_bound_kernel: FHN and Goldbeter, var0 and var1, the zero planted at 0, 63 | 64, 255 | 256 and n - 1 of 19 x 27 and around
    the second grid-stride trip of 1024 x 513 (also crd_axpy_kernel's and the RHS's: the bound is taken of f on every point)."""
    run_lone("lone bound regime " + precision, cr.lone_bound_cases((precision,)))


def test_lone_exit_when_hub_is_below_hlb(gpu_device):
    """atol = 1e-30 and a planted zero: hub < hlb, no y'' pass, h0 = sqrt(hlb hub)."""
    run_lone("lone hub < hlb exit", cr.lone_exit_cases())


def test_lone_ydd_regime_every_position(gpu_device):
    """crd_ydd_sumsq_kernel + crd_sum_blocks_kernel and the trial state of crd_axpy_kernel: fp64, 19 x 27, 264 x 250 -- just above the
    65536 points the norm's 256 blocks cover in one trip -- and 1024 x 513, where crd_axpy_kernel takes its second."""
    run_lone("lone y'' regime", cr.lone_ydd_cases())


@pytest.mark.parametrize("kind", ["group of 3 slabs", "RCCL self-ring"])
def test_slab_groups_and_the_ring(gpu_device, kind):
    """Three uneven slabs (the host takes the maximum / the sum over them) and the one-rank RCCL ring (ncclAllReduce of the scalar):
    the plant in each slab's first and last owned row, both regimes, against the lone context's reference."""
    nx, ny = cr.GROUP_GRID
    extents = [crd.slab_extents(ny, k, cr.GROUP_SLABS) for k in range(cr.GROUP_SLABS)]
    ratios = {"bound": [], "ydd": []}
    ctxs = {}
    try:
        for c in cr.group_cases(extents):
            r = cr.reference(c)
            r.assert_regime()
            key = (c.model, c.precision)
            if key not in ctxs:
                if kind.startswith("group"):
                    ctxs[key] = crd.LocalGroup(case_params(c), cr.GROUP_SLABS)
                    assert [(s.js, s.je) for s in ctxs[key].slabs] == extents
                else:
                    ctxs[key] = crd.Slab(case_params(c))
                    ctxs[key].init_rccl(crd.rccl_unique_id())
            ratios[c.regime].append(r.check(h_first_of(ctxs[key], c)))
    finally:
        for ctx in ctxs.values():
            ctx.close()
    for regime, v in ratios.items():
        report("%s, %s regime" % (kind, regime), v)


# ---- ensembles -------------------------------------------------------------------------------------------------------------------
def ensemble_h_first(e, members, y=None):
    """h_first per member of one call on fresh uploads, stopped after its first step."""
    for k, c in enumerate(members):
        e.upload(k, cr.planted_state(c) if y is None else y[k])
    sts = e.integrate_adaptive(cr.T0, cr.TOUT, **options(members[0], max_steps=1))
    assert all(s["status"] in (K.OK, K.ESTATE) for s in sts), sts
    return [s["h_first"] for s in sts]


def test_ensemble_members_each_take_their_own_scalars(gpu_device):
    """Three members, the plant in each in turn: the planted member against the reference and against a lone context (rel = 1e-12, the
    suite's bar for a fresh member), the other two bit-identical to a run of the same ensemble with no plant anywhere.  19 x 27 at every
    position; 512 x 513, where the hin bound's and the axpy's loops over [var0 | var1] start their second trip inside var1; 264 x 250
    for the y'' norm."""
    ensembles, lone, plain = {}, {}, {}
    ratios = {}
    try:
        for label, members in cr.ensemble_sets():
            c0 = members[0]
            key = (c0.model, c0.nx, c0.ny, c0.precision)
            if key not in ensembles:
                ensembles[key] = crd.Ensemble([case_params(c) for c in members])
                lone[key] = crd.Slab(case_params(c0))
            e = ensembles[key]
            bare = tuple(c._replace(q=None, var=0) for c in members)
            if bare not in plain:
                plain[bare] = ensemble_h_first(e, bare)
            got = ensemble_h_first(e, members)
            for k, c in enumerate(members):
                if c.q is None:
                    assert got[k] == plain[bare][k], (label, cr.case_name(members[[m.q is not None for m in members].index(True)]), "moved member", k, got[k], plain[bare][k])
                    continue
                r = cr.reference(c)
                ratios.setdefault(label, []).append(r.check(got[k]))
                assert got[k] == pytest.approx(h_first_of(lone[key], c), rel=1e-12), (label, cr.case_name(c))
                assert got[k] != plain[bare][k]
    finally:
        for ctx in list(ensembles.values()) + list(lone.values()):
            ctx.close()
    for label, v in ratios.items():
        report("ensemble, " + label, v)


def test_ensemble_compacted_op_lists_map_back_to_their_members(gpu_device):
    """atol = 1e-30 and a zero planted in member 1 alone: member 1 is done after the bound, members 0 and 2 iterate (open = [0, 2]: op 1
    of every y'' launch is member 2).  Then a call in which member 0 resumes and members 1 and 2 are fresh: hin = [1, 2], op 0 is member
    1, and after the bound open = [2], op 0 is member 2."""
    members = cr.compaction_set()
    opt = options(members[0])
    ys = [cr.planted_state(c) for c in members]
    refs = [cr.reference(c) for c in members]
    for r in refs:
        r.assert_regime()
    assert [r.trace["count"] for r in refs] == [3, 0, 3]
    lone = []
    for k, (c, y) in enumerate(zip(members, ys)):  # each member's two calls on a lone context (member 2's second on a fresh upload)
        with crd.Slab(case_params(c)) as s:
            s.upload(y)
            first = s.integrate_adaptive(0.0, cr.TOUT, **opt)
            if k == 2:
                s.upload(y)
            # (member 1's second call has no lone twin: its first step, ~1e-22 at t = 0.5, is a step size underflow, which a context
            # raises and an ensemble reports in the member's status beside its stats)
            lone.append((first, None if k == 1 else s.integrate_adaptive(cr.TOUT, 1.0, **opt)))
    with crd.Ensemble([case_params(c) for c in members]) as e:
        got = ensemble_h_first(e, members)
        ratios = [r.check(h) for r, h in zip(refs, got)]
        for k in range(3):
            assert got[k] == pytest.approx(lone[k][0]["h_first"], rel=1e-12), k
        assert got[0] != got[2]
        report("ensemble, compacted op lists", ratios)
        # a finished call, then: member 0 resumes, members 1 and 2 start afresh
        for k, y in enumerate(ys):
            e.upload(k, y)
        sts = e.integrate_adaptive(0.0, cr.TOUT, **opt)
        assert all(s["status"] == K.OK for s in sts), sts
        assert [s["h_first"] for s in sts] == got
        for k in (1, 2):
            e.upload(k, ys[k])
        sts = e.integrate_adaptive(cr.TOUT, 1.0, **dict(opt, max_steps=1))
        assert sts[0]["h_first"] == pytest.approx(lone[0][1]["h_first"], rel=1e-6) and sts[0]["h_first"] != got[0]  # (a resumed call: the suite's bar)
        for k in (1, 2):
            op = cr.problem(members[k].model, members[k].nx, members[k].ny)
            rhs = lambda t, y: co.rhs(op, t, y)  # noqa: E731
            y64 = ys[k].astype(np.float64)
            want = ark.initial_step(rhs, cr.TOUT, y64, rhs(cr.TOUT, y64), 1.0, opt["rtol"], opt["atol"])
            assert sts[k]["h_first"] == pytest.approx(want, rel=1e-6), k
        assert sts[2]["h_first"] == pytest.approx(lone[2][1]["h_first"], rel=1e-12)


@pytest.mark.parametrize("mixed", [False, True], ids=["uniform", "mixed"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_ensemble_max_abs_is_exact_per_member(gpu_device, precision, mixed):
    """Ensemble.max_abs(), the blow-up guard of crd_run's ensemble path: np.max(np.abs(var0)) of each member, exactly, with the extreme
    (positive and negative) at every position of 19 x 27 and around the second trip of 130 x 127 (64 blocks cover 16384 points), var1
    ten times larger everywhere, and a NaN in one member alone."""
    ensembles = {}
    sets = cr.max_abs_sets(precision, mixed)
    assert len(sets) == 10
    try:
        for label, shapes, fields in sets:
            key = tuple(shapes)
            if key not in ensembles:
                ensembles[key] = crd.Ensemble([params_of("fhn", nx, ny, precision) for nx, ny in shapes], mixed=mixed)
            e = ensembles[key]
            for k, y in enumerate(fields):
                e.upload(k, y)
            got = e.max_abs()
            try:
                cr.check_max_abs(fields, got)
            except AssertionError as x:
                raise AssertionError("%s %s %s: %s" % (precision, "mixed" if mixed else "uniform", label, x))
    finally:
        for e in ensembles.values():
            e.close()
    print("BOUND ensemble max-abs %s %s: exact on %d sets of three members" % (precision, "mixed" if mixed else "uniform", len(sets)))


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_lone_max_abs_is_exact_beyond_one_trip(gpu_device, precision):
    """Slab.max_abs() on 1024 x 513, the first size at which crd_max_abs_kernel strides (2048 blocks cover 524288 points)."""
    nx, ny = cr.LONE_CAP_GRID
    with crd.Slab(params_of("fhn", nx, ny, precision)) as s:
        for label, y in cr.lone_max_abs_fields(precision):
            s.upload(y)
            try:
                cr.check_max_abs([y], [s.max_abs()])
            except AssertionError as x:
                raise AssertionError("%s %s: %s" % (precision, label, x))
        y = cr.max_abs_fields(nx, ny, precision, 96, 7, nan_at=nx * ny - 1)
        s.upload(y)
        cr.check_max_abs([y], [s.max_abs()])
    print("BOUND lone max-abs %s: exact on %d states of %d x %d, and NaN for a NaN" % (precision, len(cr.lone_max_abs_fields(precision)), nx, ny))
