"""The step controller's reductions, restated in numpy for the tests: inputs, planted positions, checks and mutants.  No GPU here.

What is under test: the scalars that decide the first step of an error-controlled run (arkHin) and the blow-up guard --
crd_hin_bound_kernel, crd_axpy_kernel, crd_ydd_sumsq_kernel, crd_sum_blocks_kernel (crd_kernels.hip), their per-member twins
(crd_ensemble_adaptive.hip), crd_max_abs_kernel and member_max_abs (crd_ensemble_item.h).  All of them are grid-stride loops of 256-thread
blocks, four 64-lane wavefronts each, under a cap on the number of blocks; the host takes the maximum / the sum over the slabs of a
group and maps the ops of a batched launch back to members.  A wrong one moves h_first by far less than the suite's rel = 1e-6 at
the default tolerances, where the y'' norm alone decides.  Two regimes make each scalar decide alone:

Bound regime.  rtol = 1e-2, atol = 1e-4, tout = 0.5, states uniform in [0.5, 1.5] with ONE component set to exactly 0.  There the
quotient |f| / (0.1 |y| + rtol |y| + atol) is |f_q| / atol, thousands of times every other; hub = atol / |f_q| is clamped, both deciding
passes of arkHin take hnew = sqrt(hg hub), and h0 = 0.5 hlb^(1/4) hub^(3/4): a function of the bound alone, with relative
sensitivity 3/4 to f_q.  With atol = 1e-30 the same plant gives hub < hlb: the loop is skipped and h0 = sqrt(hlb hub), sensitivity 1/2.
Tolerance: the device's f_q is within oracle/error_bounds.rhs_bound of the reference's, so h_first is within
3/4 (1/2) bound_q / |f_q| + 8 unit roundoffs of float64 (the quotient, the reciprocal, two or three roots and the products on the host).

y'' regime (fp64, FHN).  rtol = 0, atol = 1e-6 and +50 on one var0 component: f_u = -u^3 + ... there is ~1e5, its y'' ~1e9, and the
point alone carries over 0.97 of sum (ydd_i w_i)^2 on every grid used (all but 1e-4 up to 264 x 250); every deciding pass takes hnew = sqrt(2 / yddnrm).  Tolerance:
rel = 1e-6, the suite's bar for arkHin (tests/test_gpu_parity.py) -- y'' is a difference quotient over hg ~ 1e-9.  Goldbeter has no such
plant (its kinetics saturate: the same +50 leaves the planted term at 0.013 of the sum) and is left to the bound regime.  fp32 is left
out: the trial state y + hg f with hg ~ 1e-8 rounds back to y in float32, so a float64 reference says nothing about the fp32 norm.
The regime cannot single out var1 (a planted v moves y''_v by eps only): a y'' norm that skipped var1 is left to the default-tolerance
comparisons, where var1 carries a material share.

The conditions are asserted on the reference (Reference.assert_regime) before a device value is looked at.  One combination does
not meet them and is left out: FHN's var1 on the half-million-point grids.  f_v = eps (u + b - ...) is ~0.02 whatever the grid, while the
diffusion of grid-scale noise grows with 1 / dy^2, and on 1024 x 513 and 512 x 513 some var0 quotient exceeds the planted 0.02 / atol.  The
kernels are instantiated per precision, not per model: Goldbeter's var1 (f_v ~ 10) takes the second trip of the same code there.

Positions.  A plant is a flat index q = j nx + i of a field of n points, in var0 or var1.  SMALL = 19 x 27 has n = 513 = 2 * 256 + 1:
0, 63 | 64 (wavefront edge), 255 | 256 (block edge), n - 1 (a tail block of one element).  The grids "just above a cap" come from the
launch caps in the source, 256 elements per block:
    lone hin / axpy / max-abs          grid_for: 2048 blocks      second trip above 524288 points     LONE_CAP_GRID  = 1024 x 513
    ensemble hin / axpy (over 2n)      grid_for: 2048 blocks      above 524288 elements               ENS_CAP_GRID   = 512 x 513
    y'' norms, lone and ensemble       kNormBlocks = 256          above 65536 points                  YDD_CAP_GRID   = 264 x 250
    ensemble max-abs, both launches    grid_for(n, 64)            above 16384 points                  MAXABS_CAP_GRID = 130 x 127
with three plants each: the last index of the first trip, the first of the second, n - 1.  The y'' regime also runs on LONE_CAP_GRID and
once on ENS_CAP_GRID: the trial state y + hg f is the axpy kernels' work, and its second trip shows in the y'' norm alone.

Mutants.  seen(), fold() and grouped() restate how the kernels and the host visit and combine; with a mutant they return what a wrong
kernel or wrong host code would: MUTANTS.  tests/test_controller_reductions_host.py
shows that the checks reject every one of them on at least one planted input and accept the unmutated restatement on all.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from oracle import arkode_erk as ark
from oracle import crd_oracle as co
from oracle import error_bounds as eb

L, W, D = 80.0, 20.0, 0.12
MODELS = {"fhn": (co.FHN, 1.25), "goldbeter": (co.GOLDBETER, 0.4)}
DTYPE = {"f64": np.float64, "f32": np.float32}
T0, TOUT = 0.0, 0.5
BLOCK, WAVE = 256, 64
LONE_CAP, YDD_CAP, ENS_MAXABS_CAP = 2048, 256, 64  # blocks: grid_for, kNormBlocks / kEnsembleNormBlocks, grid_for(n, 64)
SMALL = (19, 27)
LONE_CAP_GRID, ENS_CAP_GRID, YDD_CAP_GRID, MAXABS_CAP_GRID = (1024, 513), (512, 513), (264, 250), (130, 127)
GROUP_GRID, GROUP_SLABS = (19, 29), 3  # 29 rows in three slabs: 10 + 10 + 9
U64 = 2.0 ** -53
HOST_ROUNDINGS = 8

REGIMES = {  # rtol, atol
    "bound": (1e-2, 1e-4),
    "exit": (1e-2, 1e-30),
    "compaction": (1e-5, 1e-30),  # the exit for a planted member; an unplanted one decides by its y'' norm, which depends on its state
    "ydd": (0.0, 1e-6),
}
YDD_PLANT = 50.0
SENSITIVITY = {"bound": 0.75, "exit": 0.5, "compaction": 0.5}

for _nx, _ny in (SMALL,):
    assert (_nx * _ny) % BLOCK == 1
assert LONE_CAP_GRID[0] * LONE_CAP_GRID[1] > LONE_CAP * BLOCK >= ENS_CAP_GRID[0] * ENS_CAP_GRID[1]
assert 2 * ENS_CAP_GRID[0] * ENS_CAP_GRID[1] > LONE_CAP * BLOCK
assert YDD_CAP_GRID[0] * YDD_CAP_GRID[1] > YDD_CAP * BLOCK
assert MAXABS_CAP_GRID[0] * MAXABS_CAP_GRID[1] > ENS_MAXABS_CAP * BLOCK


def problem(model, nx, ny):
    m, beta = MODELS[model]
    return co.make_problem(m, co.TORUS, nx, L, W, D, beta, ny=ny)


def state(nx, ny, seed, precision="f64"):
    """uniform in [0.5, 1.5]: f is non-zero everywhere.  Rounded to the device's precision, so that the upload is exact."""
    return np.random.default_rng(seed).uniform(0.5, 1.5, (ny, nx, 2)).astype(DTYPE[precision])


def small_positions(n):
    return [0, WAVE - 1, WAVE, BLOCK - 1, BLOCK, n - 1]


def trip_positions(n, cap_blocks):
    """Last index of the first grid-stride trip, first of the second, n - 1."""
    edge = cap_blocks * BLOCK
    assert n > edge
    return [edge - 1, edge, n - 1]


# A case: one input of an arkHin gate.  q: flat index in the field `var`; seed: of the unplanted state.
Case = namedtuple("Case", "regime model nx ny precision var q seed")


def case_name(c):
    plant = "no plant (seed %d)" % c.seed if c.q is None else "var%d q=%d" % (c.var, c.q)
    return "%s %s %s %dx%d %s" % (c.regime, c.precision, c.model, c.nx, c.ny, plant)


def planted_state(c):
    y = state(c.nx, c.ny, c.seed, c.precision)
    if c.q is None:
        return y
    j, i = divmod(c.q, c.nx)
    if c.regime == "ydd":
        y[j, i, c.var] += YDD_PLANT
    else:
        y[j, i, c.var] = 0.0
    return y


def f_at(op, y, precision, j, i):
    """(f_ref, bound_u, bound_v) of error_bounds.rhs_bound at point (j, i), from the five rows around it (the torus wraps in phi):
    the whole grid's values at that point (tests/test_controller_reductions_host.py compares) at a fraction of the cost."""
    rows = [(j + d) % op.ny for d in (-2, -1, 0, 1, 2)]
    ref, bu, bv = eb.rhs_bound(op, T0, np.ascontiguousarray(y[rows]), precision, j0=rows[0])
    return ref[2, i], bu[2, i], bv[2, i]


class Reference:
    """The reference side of a case: the trace of oracle/arkode_erk.initial_step_trace on the (widened) state, the step the regime
    predicts from the high-precision f at the plant, and the relative error allowed to a device."""

    def __init__(self, c):
        self.case = c
        self.rtol, self.atol = REGIMES[c.regime]
        self.op = problem(c.model, c.nx, c.ny)
        y = self.y
        y64 = y.astype(np.float64)
        rhs = lambda t, v: co.rhs(self.op, t, v)  # noqa: E731
        f0 = rhs(T0, y64)
        tr = self.trace = ark.initial_step_trace(rhs, T0, y64, f0, TOUT, self.rtol, self.atol)
        self.component = None if c.q is None else 2 * c.q + c.var  # in the AoS vector the trace indexes
        # what assert_regime needs of the arrays, so that none is kept (the cases above a cap hold half a million points)
        terms = tr.pop("ydd_terms")
        if terms is not None:
            self.ydd_argmax, self.ydd_share = int(np.argmax(terms)), float(np.max(terms)) / float(np.sum(terms))
        if c.q is not None and c.regime != "ydd":
            ratio = (np.abs(f0) / (0.1 * np.abs(y64) + (self.rtol * np.abs(y64) + self.atol))).ravel()
            self.runner_up = float(np.max(np.delete(ratio, self.component)))
        if c.regime == "ydd" or c.q is None:
            self.h0, self.allowed = tr["h0"], 1e-6
            return
        j, i = divmod(c.q, c.nx)
        f, bu, bv = f_at(self.op, y, c.precision, j, i)
        fq, bq = abs(f[c.var]), (bu, bv)[c.var]
        self.fq, self.rel_f = float(fq), float(bq / fq)
        hub = np.longdouble(self.atol) / fq
        hlb = np.longdouble(tr["hlb"])
        if c.regime == "bound":
            self.h0 = float(np.longdouble(0.5) * np.sqrt(np.sqrt(hlb * hub * hub * hub)))
        else:
            self.h0 = float(np.sqrt(hlb * hub))
        self.allowed = SENSITIVITY[c.regime] * self.rel_f + HOST_ROUNDINGS * U64

    @property
    def y(self):
        """The case's state in the device's precision (formed anew: nothing of a grid's size is kept)."""
        return planted_state(self.case)

    def assert_regime(self):
        """The conditions under which the case isolates its reduction, on the reference alone."""
        c, tr = self.case, self.trace
        name = case_name(c)
        if c.q is None:  # an unplanted member: compared with the trace at the suite's bar, nothing to isolate
            return
        deciding = [it for it in tr["iterations"] if it["formula"] is not None]
        if c.regime == "ydd":
            assert deciding and all(it["formula"] == "ydd" for it in deciding), (name, tr["iterations"])
            assert self.ydd_share >= 0.5, (name, self.ydd_share)
            assert self.ydd_argmax == self.component, (name, self.ydd_argmax)
            return
        assert tr["argmax"] == self.component, (name, tr["argmax"], self.component)
        assert self.runner_up <= 0.5 * tr["hub_inv"], (name, self.runner_up, tr["hub_inv"])
        assert tr["clamped"], name
        if c.regime in ("exit", "compaction"):
            assert tr["count"] == 0 and tr["hub"] < tr["hlb"], (name, tr)
        else:
            assert len(deciding) == 2 and all(it["formula"] == "geometric" for it in deciding), (name, tr["iterations"])
            # ... with room: a device norm within a factor 8 of the reference's (fp32: the trial step is a few ulps of y, its y'' a
            # rounded quotient of the right size at best) takes the same branch
            assert all(8.0 * it["yddnrm"] * tr["hub"] ** 2 <= 2.0 for it in deciding), (name, tr["iterations"], tr["hub"])
        # the f64 restatement is itself an evaluation within the bound: the trace and the prediction agree
        assert abs(tr["h0"] - self.h0) <= self.allowed * self.h0, (name, tr["h0"], self.h0, self.allowed)

    def check(self, h_first):
        """observed / allowed relative error of a device's (or a mutant's) h_first; AssertionError above 1."""
        self.assert_regime()
        ratio = abs(h_first - self.h0) / self.h0 / self.allowed
        assert ratio <= 1.0, (case_name(self.case), h_first, self.h0, "relative error / allowed = %.3g" % ratio)
        return ratio


@functools.lru_cache(maxsize=None)
def reference(case):
    return Reference(case)


def check_max_abs(fields, got):
    """got[k] == max |var0| of member k exactly; a NaN in var0 makes the member's value NaN.  fields: the members' states (ny, nx, 2)."""
    assert len(got) == len(fields)
    for k, (y, g) in enumerate(zip(fields, got)):
        u = np.asarray(y[..., 0], dtype=np.float64)
        want = float(np.max(np.abs(u)))  # (np.max propagates NaN)
        assert (math.isnan(g) and math.isnan(want)) or g == want, ("member %d" % k, g, want)


# ---- the reductions as the kernels make them, and wrong ones ---------------------------------------------------------------------
MUTANTS = [
    "drop_last",        # the loop ends one element early
    "drop_tail_block",  # the grid is n / 256 blocks, rounded down
    "var0_only",        # the second field is never launched / the loop runs to n instead of 2n
    "first_trip",       # no grid stride: every thread looks at one element
    "first_wavefront",  # only wavefront 0's partial of each block is kept
    "slab0_only",       # the group's scalar is slab 0's, not the max / sum over the slabs
    "slot_shift",       # member k's result lands in slot k - 1
    "no_abs",           # max u instead of max |u|
    "var1_counted",     # max-abs looks at both fields
]


def seen(n, cap_blocks, mutant=None):
    """Which of n consecutive elements a grid-stride loop of 256-thread blocks under `cap_blocks` folds into its result."""
    idx = np.arange(n)
    keep = np.ones(n, dtype=bool)
    if mutant == "drop_last":
        keep[n - 1] = False
    elif mutant == "drop_tail_block":
        keep = idx < (n // BLOCK) * BLOCK
    elif mutant == "first_trip":
        keep = idx < cap_blocks * BLOCK
    elif mutant == "first_wavefront":
        keep = idx % BLOCK < WAVE
    return keep


def fold(values, cap_blocks, mutant, op, layout):
    """max or sum of one trajectory's per-component values (ny, nx, 2), visited as `layout` says: "planes" -- a launch (or loop) per
    field over n points, the lone kernels and the ensemble's y'' norm; "flat" -- one loop over the 2n elements of [var0 | var1], the
    ensemble's hin bound."""
    fields = [values[..., 0].ravel(), values[..., 1].ravel()]
    if mutant == "var0_only":
        fields = fields[:1]
    if layout == "flat" and len(fields) == 2:
        flat = np.concatenate(fields)
        fields = [flat]
    out = 0.0
    for f in fields:
        part = f[seen(f.size, cap_blocks, mutant)]
        if part.size:
            out = max(out, float(np.max(part))) if op == "max" else out + float(np.sum(part))
    return out


def grouped(values, extents, cap_blocks, mutant, op, layout="planes"):
    """The scalar of a run cut into slabs of rows [js, je]: each slab folds its own rows, the host combines (extents None: one slab)."""
    if extents is None:
        extents = [(0, values.shape[0] - 1)]
    parts = [fold(values[js:je + 1], cap_blocks, mutant, op, layout) for js, je in extents]
    if mutant == "slab0_only":
        return parts[0]
    return max(parts) if op == "max" else sum(parts)


def hin_scalar(t0, tout, hub_inv, yddnrm_of):
    """The host's side of arkHin (crd_arkode.h: hin_start, hin_bound, hin_ydd) around the two device scalars."""
    tdist = abs(tout - t0)
    hlb = ark.H0_LBFACTOR * ark.UROUND * max(abs(t0), abs(tout))
    hub = ark.H0_UBFACTOR * tdist
    if hub * hub_inv > 1.0:
        hub = 1.0 / hub_inv
    hg = math.sqrt(hlb * hub)
    if hub < hlb:
        return hg
    hnew_ok, count = False, 0
    while True:
        yddnrm = yddnrm_of(hg)
        count += 1
        if hnew_ok or count == ark.H0_ITERS:
            return min(max(ark.H0_BIAS * hg, hlb), hub)
        hnew = math.sqrt(2.0 / yddnrm) if yddnrm * hub * hub > 2.0 else math.sqrt(hg * hub)
        hrat = hnew / hg
        if 0.5 < hrat < 2.0:
            hnew_ok = True
        if count > 1 and hrat > 2.0:
            hnew, hnew_ok = hg, True
        hg = hnew


def h_first_model(c, mutant=None, extents=None, ensemble=False):
    """h_first of case c as the device forms it -- float64 throughout, f from the oracle --, or as a mutant would."""
    r = reference(c)
    y = r.y.astype(np.float64)
    ay, f0 = np.abs(y), co.rhs(r.op, T0, y)
    layout = "flat" if ensemble else "planes"
    hub_inv = grouped(np.abs(f0) / (0.1 * ay + (r.rtol * ay + r.atol)), extents, LONE_CAP, mutant, "max", layout)

    def yddnrm_of(hg):
        e = (co.rhs(r.op, T0 + hg, y + hg * f0) - f0) * (1.0 / hg) / (r.rtol * ay + r.atol)
        return math.sqrt(grouped(e * e, extents, YDD_CAP, mutant, "sum") / y.size)

    return hin_scalar(T0, TOUT, hub_inv, yddnrm_of)


def ensemble_model(cases, mutant=None):
    """h_first per member of an ensemble whose member k holds case k's state."""
    h = [h_first_model(c, None if mutant == "slot_shift" else mutant, ensemble=True) for c in cases]
    if mutant == "slot_shift":
        h = h[1:] + [0.0]
    return h


def max_abs_model(fields, cap_blocks, mutant=None):
    """max |var0| per member as member_max_abs / crd_max_abs_kernel fold it, or as a mutant would."""
    out = []
    for y in fields:
        v = np.asarray(y, dtype=np.float64)
        v = v if mutant == "no_abs" else np.abs(v)
        cols = [v[..., 0].ravel()] + ([v[..., 1].ravel()] if mutant == "var1_counted" else [])
        m = 0.0
        for f in cols:
            part = f[seen(f.size, cap_blocks, mutant)]
            if part.size:
                m = float("nan") if np.isnan(part).any() or math.isnan(m) else max(m, float(np.max(part)))
        out.append(m)
    if mutant == "slot_shift":
        out = out[1:] + [0.0]
    return out


# ---- the inputs of the gates (the GPU test runs them, the host test shows the regime conditions and the mutants on them) ---------
def lone_bound_cases(precisions=("f64", "f32")):
    out = []
    for precision in precisions:
        for model in MODELS:
            nx, ny = SMALL
            for var in (0, 1):
                out += [Case("bound", model, nx, ny, precision, var, q, 11) for q in small_positions(nx * ny)]
            nx, ny = LONE_CAP_GRID
            for var in (0, 1) if model == "goldbeter" else (0,):  # (see the docstring: FHN's var1 above the cap)
                out += [Case("bound", model, nx, ny, precision, var, q, 12) for q in trip_positions(nx * ny, LONE_CAP)]
    return out


def lone_exit_cases():
    nx, ny = SMALL
    return [Case("exit", model, nx, ny, precision, var, q, 13) for precision in ("f64", "f32") for model in MODELS for var in (0, 1) for q in (0, nx * ny - 1)]


def lone_ydd_cases():
    nx, ny = SMALL
    out = [Case("ydd", "fhn", nx, ny, "f64", 0, q, 14) for q in small_positions(nx * ny)]
    nx, ny = YDD_CAP_GRID
    out += [Case("ydd", "fhn", nx, ny, "f64", 0, q, 15) for q in trip_positions(nx * ny, YDD_CAP)]
    # crd_axpy_kernel's second trip: a trial state it left unwritten is a stale plane, off by O(1) where hg f is ~1e-9 -- a y'' of 1e9
    nx, ny = LONE_CAP_GRID
    return out + [Case("ydd", "fhn", nx, ny, "f64", 0, q, 18) for q in trip_positions(nx * ny, LONE_CAP)]


def group_cases(extents):
    """The plant in each slab in turn, in its first owned row and its last; var0 and var1 alternate with the column."""
    nx, ny = GROUP_GRID
    assert extents[0][0] == 0 and extents[-1][1] == ny - 1 and len({je - js for js, je in extents}) > 1, extents
    out = []
    for s, (js, je) in enumerate(extents):
        for j, i in ((js, 3 + s), (je, nx - 2 - s)):
            q = j * nx + i
            out += [Case("bound", "fhn", nx, ny, "f64", s % 2, q, 16), Case("bound", "goldbeter", nx, ny, "f32", (s + 1) % 2, q, 16),
                    Case("ydd", "fhn", nx, ny, "f64", 0, q, 17)]
    return out


def ensemble_sets():
    """[(label, [case of member 0, 1, 2])]: the plant in each member in turn (the other two hold unplanted states of their own, q None)
    -- every position of SMALL, then the grids just above the ensemble's caps."""
    out = []

    def members(regime, model, nx, ny, precision, var, q, planted, seed):
        return [Case(regime, model, nx, ny, precision, var if k == planted else 0, q if k == planted else None, seed + k) for k in range(3)]

    nx, ny = SMALL
    n = nx * ny
    for m, q in enumerate(small_positions(n)):
        out.append(("bound small", members("bound", "fhn", nx, ny, "f64", m % 2, q, m % 3, 20)))
        out.append(("bound small", members("bound", "goldbeter", nx, ny, "f32", (m + 1) % 2, q, (m + 1) % 3, 30)))
        out.append(("ydd small", members("ydd", "fhn", nx, ny, "f64", 0, q, (m + 2) % 3, 40)))
    nx, ny = ENS_CAP_GRID  # the hin bound strides [var0 | var1]: the second trip starts inside var1
    n = nx * ny
    for m, e in enumerate(trip_positions(2 * n, LONE_CAP)):
        out.append(("bound above the cap", members("bound", "goldbeter", nx, ny, ("f64", "f32")[m % 2], 1, e - n, m, 50)))
    nx, ny = YDD_CAP_GRID
    for m, q in enumerate(trip_positions(nx * ny, YDD_CAP)):
        out.append(("ydd above the cap", members("ydd", "fhn", nx, ny, "f64", 0, q, m, 60)))
    nx, ny = ENS_CAP_GRID  # the ensemble's axpy strides [var0 | var1] like its hin bound: the trial state's second trip (see lone_ydd_cases)
    out.append(("ydd above the axpy cap", members("ydd", "fhn", nx, ny, "f64", 0, nx * ny - 1, 1, 65)))
    return out


def compaction_set():
    """atol = 1e-30 and a zero planted in member 1 alone: member 1 is done after the bound (hub < hlb), members 0 and 2 iterate, so the
    second op of every y'' launch is member 2.  rtol = 1e-5: the two that iterate take their steps from their own y'' norms (in the
    bound regime an unplanted member's hub is 0.1 |tout - t0| and its step the same number whatever its state)."""
    nx, ny = SMALL
    return [Case("compaction", "fhn", nx, ny, "f64", 0, None, 70), Case("compaction", "fhn", nx, ny, "f64", 0, 200, 71),
            Case("compaction", "fhn", nx, ny, "f64", 0, None, 72)]


MAXABS_EXTREME = 7.5


def max_abs_fields(nx, ny, precision, seed, q=None, sign=1.0, nan_at=None):
    """A member's state for the max-abs gate: var0 uniform in [0.5, 1.5] with +-7.5 planted at q, var1 ten times larger everywhere
    (it must not count), optionally a NaN at flat index nan_at of var0."""
    y = state(nx, ny, seed, precision)
    y[..., 1] *= 10.0
    if q is not None:
        y[q // nx, q % nx, 0] = sign * MAXABS_EXTREME
    if nan_at is not None:
        y[nan_at // nx, nan_at % nx, 0] = np.nan
    return y


def max_abs_sets(precision, mixed):
    """[(label, [(nx, ny), ...], [state per member])] of three members; mixed: the members differ in size.  The extreme sits in each
    position class in turn, negative every other time, in the member that rotates with it; one set holds a NaN in one member."""
    big, small = MAXABS_CAP_GRID, SMALL
    shapes = [small, big, (33, 21)] if mixed else None
    out = []
    for grid, positions in ((small, small_positions(small[0] * small[1])), (big, trip_positions(big[0] * big[1], ENS_MAXABS_CAP))):
        for m, q in enumerate(positions):
            sh = shapes if mixed else [grid] * 3
            k = sh.index(grid) if mixed else m % 3
            fields = [max_abs_fields(nx, ny, precision, 80 + j, q if j == k else None, -1.0 if m % 2 else 1.0) for j, (nx, ny) in enumerate(sh)]
            out.append(("%dx%d q=%d member %d" % (grid + (q, k)), sh, fields))
    sh = shapes if mixed else [small] * 3
    fields = [max_abs_fields(nx, ny, precision, 90 + j, 5, nan_at=(nx * ny - 1 if j == 1 else None)) for j, (nx, ny) in enumerate(sh)]
    out.append(("NaN in member 1", sh, fields))
    return out


def lone_max_abs_fields(precision):
    nx, ny = LONE_CAP_GRID
    pos = trip_positions(nx * ny, LONE_CAP) + small_positions(nx * ny)[:5]
    return [("%dx%d q=%d" % (nx, ny, q), max_abs_fields(nx, ny, precision, 95, q, -1.0 if m % 2 else 1.0)) for m, q in enumerate(pos)]
