"""Host-side mirror of the reference's interface for the RHS path, on top of the libcrd C ABI.

Names follow the reference (/root/reference/src/FHNmodel_torus.cpp): a `Slab` is one subdomain (UserData) living
on one GPU; `Slab.f(t, y)` is the ARKRhsFn `f(t, y, ydot, user_data)` (:504); `Slab.step_rk4` replaces the
`ARKode(...)` call (:423).  Vectors are numpy arrays in the reference's layout, shape (nyl, nx, 2) = AoS [var0, var1],
theta fastest.  All arithmetic happens in the HIP kernels; nothing here computes on the CPU.
"""
import ctypes as C

import numpy as np

from . import _capi as capi
from .post import period_map
from ._capi import (MODELS, SURFACES, STEPPERS, PRECISION_F32, PRECISION_F64, CrdError, Grid, Params,  # noqa: F401
                    RunConfig, check, lib)


def make_params(model, surface, nx, surface_length, surface_width, diffusion, beta, *, ny=0, beta_min=0.0, beta_max=0.0,
                vary_beta=0, just_diffusion=0, t_boundary=0.0, precision="f64"):
    p = Params()
    p.model = MODELS[model] if isinstance(model, str) else model
    p.surface = SURFACES[surface] if isinstance(surface, str) else surface
    p.nx, p.ny = nx, ny
    p.surface_length, p.surface_width = surface_length, surface_width
    p.diffusion, p.beta, p.beta_min, p.beta_max = diffusion, beta, beta_min, beta_max
    p.vary_beta, p.just_diffusion = vary_beta, just_diffusion
    p.t_boundary = t_boundary
    p.precision = {"f64": PRECISION_F64, "f32": PRECISION_F32}[precision] if isinstance(precision, str) else precision
    return p


def _part(part):
    return capi.PARTS[part] if isinstance(part, str) else int(part)


def grid_of(params):
    g = Grid()
    check(lib().crd_grid_from_params(C.byref(params), C.byref(g)), "crd_grid_from_params")
    return g


def slab_extents(ny, slab, n_slabs):
    js, je = C.c_int64(), C.c_int64()
    check(lib().crd_slab_extents(ny, slab, n_slabs, C.byref(js), C.byref(je)), "crd_slab_extents")
    return js.value, je.value


def dims_create(nprocs):
    """MPI_Dims_create(nprocs, 2): the reference's process grid (d0 theta-blocks x d1 phi-blocks)."""
    d0, d1 = C.c_int(), C.c_int()
    check(lib().crd_dims_create(nprocs, C.byref(d0), C.byref(d1)), "crd_dims_create")
    return d0.value, d1.value


def block_extents(nx, ny, c0, d0, c1, d1):
    """(is, ie, js, je) of block (c0, c1) of a d0 x d1 decomposition (SetupDecomp)."""
    v = [C.c_int64() for _ in range(4)]
    check(lib().crd_block_extents(nx, ny, c0, d0, c1, d1, *[C.byref(x) for x in v]), "crd_block_extents")
    return tuple(x.value for x in v)


def halo_plan(slab, n_slabs, nyl, depth=1):
    """The four ordered point-to-point operations of one halo exchange: [(is_send, peer, row_begin, row_count)]."""
    ops = (capi.HaloOp * 4)()
    check(lib().crd_halo_plan(slab, n_slabs, nyl, depth, ops), "crd_halo_plan")
    return [(bool(o.is_send), o.peer, o.row_begin, o.row_count) for o in ops]


def cycle_vote(pos):
    """What a rank standing at position `pos` of the exchange cycle (-1: ghost rows not trusted) contributes to the agreement."""
    v = (C.c_double * 2)()
    check(lib().crd_cycle_vote(pos, v), "crd_cycle_vote")
    return [v[0], v[1]]


def cycle_agreed(reduced):
    """The ring's common cycle position from the element-wise MIN of the ranks' votes, or -1 (start with an exchange)."""
    return lib().crd_cycle_agreed((C.c_double * 2)(*reduced))


def steady_state(model, beta):
    a, b = C.c_double(), C.c_double()
    m = MODELS[model] if isinstance(model, str) else model
    check(lib().crd_steady_state(m, beta, C.byref(a), C.byref(b)), "crd_steady_state")
    return a.value, b.value


def steady_state_as_printed(model, beta, decimals=8):
    """The stable state as the reference's Goldbeter programs read it from SolveGoldbeterODE.py's print (numpy: 8 decimals)."""
    a, b = C.c_double(), C.c_double()
    m = MODELS[model] if isinstance(model, str) else model
    check(lib().crd_steady_state_as_printed(m, beta, decimals, C.byref(a), C.byref(b)), "crd_steady_state_as_printed")
    return a.value, b.value


def stable_dt(params):
    return lib().crd_stable_dt(C.byref(params))


def load_ini(path, model, surface):
    cfg = RunConfig()
    err = C.create_string_buffer(512)
    m = MODELS[model] if isinstance(model, str) else model
    s = SURFACES[surface] if isinstance(surface, str) else surface
    rc = lib().crd_config_load_ini(str(path).encode(), m, s, C.byref(cfg), err, len(err))
    if rc != capi.OK:
        raise CrdError(rc, "crd_config_load_ini", err.value.decode())
    return cfg


def run_config(params, *, wave_length=0.1, wave_width=0.5, wave_inside=0, output_timestep=1, t_final=1.0,
               include_all_vars=0, ic_type=0, dt=0.0, dt_safety=0.8, n_gpus=1, stepper=capi.STEPPER_AUTO, adaptive=0, rtol=1e-5, atol=1e-10,
               steady_state_decimals=0):
    cfg = RunConfig()
    cfg.params = params
    cfg.wave_length, cfg.wave_width, cfg.wave_inside = wave_length, wave_width, wave_inside
    cfg.output_timestep, cfg.t_final = output_timestep, t_final
    cfg.include_all_vars, cfg.ic_type = include_all_vars, ic_type
    cfg.dt, cfg.dt_safety, cfg.n_gpus, cfg.stepper = dt, dt_safety, n_gpus, stepper
    cfg.adaptive, cfg.rtol, cfg.atol = adaptive, rtol, atol
    cfg.steady_state_decimals = steady_state_decimals
    return cfg


def initial_conditions(cfg, js=None, je=None, is_=None, ie=None):
    """Rows [js, je] (and columns [is_, ie]) of the reference's initial state as float64 (nyl, nxl, 2)."""
    g = grid_of(cfg.params)
    js = 0 if js is None else js
    je = g.ny - 1 if je is None else je
    is_ = 0 if is_ is None else is_
    ie = g.nx - 1 if ie is None else ie
    y = np.empty((je - js + 1, ie - is_ + 1, 2), dtype=np.float64)
    check(lib().crd_initial_conditions_block(C.byref(cfg), is_, ie, js, je, y.ctypes.data), "crd_initial_conditions_block")
    return y


class Writer:
    """Per-subdomain text files in the reference's format (/root/reference/src/FHNmodel_torus.cpp:376-410,438-455)."""

    def __init__(self, cfg, directory, slab=0, n_slabs=1, block=None):
        self._h = C.c_void_p()
        if block is None:
            check(lib().crd_writer_open(C.byref(cfg), str(directory).encode(), slab, n_slabs, C.byref(self._h)), "crd_writer_open")
        else:  # block = (c0, d0, c1, d1); the file number is the block's rank
            c0, d0, c1, d1 = block
            check(lib().crd_writer_open_block(C.byref(cfg), str(directory).encode(), c0 * d1 + c1, c0, d0, c1, d1, C.byref(self._h)), "crd_writer_open_block")

    def write_row(self, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        check(lib().crd_writer_write_row(self._h, y.ctypes.data), "crd_writer_write_row")

    def close(self):
        if self._h:
            h, self._h = self._h, None
            check(lib().crd_writer_close(h), "crd_writer_close")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _adaptive_options(options):
    opt = capi.AdaptiveOptions()
    check(lib().crd_adaptive_defaults(C.byref(opt)), "crd_adaptive_defaults")
    for k, v in options.items():
        if not hasattr(opt, k):
            raise TypeError("unknown adaptive option %r" % k)
        setattr(opt, k, v)
    return opt


def _adaptive_result(rc, st, where, handle):
    stats = {f: getattr(st, f) for f, _ in st._fields_}
    if rc != capi.OK:
        raise CrdError(rc, where, lib().crd_last_error(handle).decode() + " %r" % stats)
    return stats


class Slab:
    """One phi-slab of the grid resident on one GPU (crd_ctx)."""

    def __init__(self, params, slab=0, n_slabs=1, device=0, block=None):
        self._h = C.c_void_p()
        self.params = params
        if block is None:
            rc = lib().crd_create(C.byref(params), slab, n_slabs, device, C.byref(self._h))
        else:  # block = (c0, d0, c1, d1) of a 2-D decomposition
            c0, d0, c1, d1 = block
            slab, n_slabs = c0 * d1 + c1, d0 * d1
            rc = lib().crd_create_block(C.byref(params), c0, d0, c1, d1, device, C.byref(self._h))
        if rc != capi.OK:
            self._h = None
            raise CrdError(rc, "crd_create", lib().crd_last_error(None).decode())
        g = Grid()
        check(lib().crd_get_grid(self._h, C.byref(g)), "crd_get_grid", self._h)
        self.grid = g
        js, je = C.c_int64(), C.c_int64()
        check(lib().crd_get_slab(self._h, C.byref(js), C.byref(je)), "crd_get_slab", self._h)
        self.js, self.je = js.value, je.value
        blk = [C.c_int64() for _ in range(4)]
        check(lib().crd_get_block(self._h, *[C.byref(x) for x in blk]), "crd_get_block", self._h)
        self.is_, self.ie = blk[0].value, blk[1].value
        self.nx, self.nyl = self.ie - self.is_ + 1, je.value - js.value + 1
        self.slab, self.n_slabs = slab, n_slabs
        self.dtype = np.float64 if params.precision == PRECISION_F64 else np.float32

    # -- lifecycle ---------------------------------------------------------------------------------------------
    def close(self):
        if self._h:
            lib().crd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    def _check(self, rc, where):
        check(rc, where, self._h)

    # -- state -------------------------------------------------------------------------------------------------
    def upload(self, y):
        y = np.ascontiguousarray(y)
        assert y.shape == (self.nyl, self.nx, 2), (y.shape, (self.nyl, self.nx, 2))
        if y.dtype == np.float64:
            self._check(lib().crd_state_upload(self._h, y.ctypes.data, 1), "crd_state_upload")
        elif y.dtype == np.float32 and self.dtype == np.float32:
            self._check(lib().crd_state_upload(self._h, y.ctypes.data, 0), "crd_state_upload")
        else:
            raise TypeError("state must be float64, or float32 for an f32 context")

    def download(self, dtype=np.float64):
        y = np.empty((self.nyl, self.nx, 2), dtype=dtype)
        self._check(lib().crd_state_download(self._h, y.ctypes.data, 1 if y.dtype == np.float64 else 0), "crd_state_download")
        return y

    def download_rows(self, var, row_begin, row_count):
        """Rows [row_begin, row_begin + row_count) of one field of the resident state, ghost rows included (device precision)."""
        rows = np.empty((row_count, self.nx), dtype=self.dtype)
        self._check(lib().crd_state_download_rows(self._h, var, row_begin, row_count, rows.ctypes.data), "crd_state_download_rows")
        return rows

    # -- the RHS callback --------------------------------------------------------------------------------------
    def f(self, t, y, out=None):
        """ydot = f(t, y) for this slab's AoS vector (host arrays in the device precision).  With y and `out` both over
        pinned memory (PinnedArray) the call streams the slab band by band over the host link."""
        y = np.ascontiguousarray(y, dtype=self.dtype)
        assert y.shape == (self.nyl, self.nx, 2)
        ydot = np.empty_like(y) if out is None else out
        assert ydot.shape == y.shape and ydot.dtype == y.dtype and ydot.flags["C_CONTIGUOUS"]
        self._check(lib().crd_rhs_host(self._h, t, y.ctypes.data, ydot.ctypes.data), "crd_rhs_host")
        return ydot

    def _vector(self, y):
        y = np.ascontiguousarray(y, dtype=self.dtype)
        assert y.shape == (self.nyl, self.nx, 2), (y.shape, (self.nyl, self.nx, 2))
        return y

    def rhs_part(self, t, y, part):
        """One part of f(t, y) = f_D + f_R for this slab's AoS vector: part "full", "diffusion" or "reaction" (or a CRD_PART_* value)."""
        y = self._vector(y)
        ydot = np.empty_like(y)
        self._check(lib().crd_rhs_part_host(self._h, t, _part(part), y.ctypes.data, ydot.ctypes.data), "crd_rhs_part_host")
        return ydot

    def jtimes(self, t, y, v, part="full"):
        """J_part(t, y) v: the action of the Jacobian of f, or of one part of it, on the direction v (laid out like y)."""
        y, v = self._vector(y), self._vector(v)
        jv = np.empty_like(y)
        self._check(lib().crd_jtimes_host(self._h, t, _part(part), y.ctypes.data, v.ctypes.data, jv.ctypes.data), "crd_jtimes_host")
        return jv

    @staticmethod
    def _psolve_options(pre, post, coarse, max_levels, omega):
        opt = capi.PsolveOptions()
        opt.pre, opt.post, opt.coarse, opt.max_levels, opt.omega = pre, post, coarse, max_levels, omega
        return opt

    def psolve(self, t, gamma, r, pre=2, post=2, coarse=8, max_levels=16, omega=0.8):
        """z = M r, M one multigrid V-cycle for (I - gamma J_D(t)) z = r: the preconditioner solve of an implicit stage (crd_psolve_host).
        r is laid out like y; var1 of z is var1 of r."""
        r = self._vector(r)
        z = np.empty_like(r)
        opt = self._psolve_options(pre, post, coarse, max_levels, omega)
        self._check(lib().crd_psolve_host(self._h, t, gamma, C.byref(opt), r.ctypes.data, z.ctypes.data), "crd_psolve_host")
        return z

    def psolve_info(self, pre=2, post=2, coarse=8, max_levels=16, omega=0.8):
        """(levels, [(nx, ny) per level], workspace bytes) of Slab.psolve with these options (crd_psolve_info)."""
        opt = self._psolve_options(pre, post, coarse, max_levels, omega)
        levels, nbytes = C.c_int32(), C.c_int64()
        nx, ny = (C.c_int32 * 16)(), (C.c_int32 * 16)()
        self._check(lib().crd_psolve_info(self._h, C.byref(opt), C.byref(levels), nx, ny, C.byref(nbytes)), "crd_psolve_info")
        return levels.value, [(nx[k], ny[k]) for k in range(levels.value)], nbytes.value

    @classmethod
    def _lsolve_options(cls, part="diffusion", precondition=True, restart=30, max_iters=200, rtol=1e-8, atol=0.0, **psolve_options):
        opt = capi.LsolveOptions()
        opt.part, opt.precondition, opt.restart, opt.max_iters, opt.rtol, opt.atol = _part(part), int(precondition), restart, max_iters, rtol, atol
        opt.psolve = cls._psolve_options(**dict(dict(pre=2, post=2, coarse=8, max_levels=16, omega=0.8), **psolve_options))
        return opt

    def lsolve(self, t, gamma, r, y=None, part="diffusion", precondition=True, restart=30, max_iters=200, rtol=1e-8, atol=0.0, **psolve_options):
        """(z, stats) of (I - gamma J_part(t, y)) z = r by restarted GMRES on the device, right-preconditioned with the cycle of
        Slab.psolve (crd_lsolve_host).  r and y are laid out like the state; y is needed for part "full" only.  stats is the
        crd_lsolve_stats structure: converged, iterations, restarts, matvecs, psolves, breakdown, r_norm, res_norm.  Running out of
        max_iters is not an error: stats.converged is 0 and z the last iterate."""
        r = self._vector(r)
        y = None if y is None else self._vector(y)
        z, st = np.empty_like(r), capi.LsolveStats()
        opt = self._lsolve_options(part, precondition, restart, max_iters, rtol, atol, **psolve_options)
        self._check(lib().crd_lsolve_host(self._h, t, gamma, C.byref(opt), None if y is None else y.ctypes.data, r.ctypes.data, z.ctypes.data, C.byref(st)),
                    "crd_lsolve_host")
        return z, st

    def lsolve_info(self, part="diffusion", precondition=True, restart=30, max_iters=200, rtol=1e-8, atol=0.0, **psolve_options):
        """Device bytes of the workspace Slab.lsolve with these options keeps on the context (crd_lsolve_info)."""
        opt, nbytes = self._lsolve_options(part, precondition, restart, max_iters, rtol, atol, **psolve_options), C.c_int64()
        self._check(lib().crd_lsolve_info(self._h, C.byref(opt), C.byref(nbytes)), "crd_lsolve_info")
        return nbytes.value

    @classmethod
    def _bicgstab_options(cls, part="diffusion", precondition=True, max_iters=200, guess=False, rtol=1e-8, atol=0.0, **psolve_options):
        opt = capi.BicgstabOptions()
        opt.part, opt.precondition, opt.max_iters, opt.guess, opt.rtol, opt.atol = _part(part), int(precondition), max_iters, int(guess), rtol, atol
        opt.psolve = cls._psolve_options(**dict(dict(pre=2, post=2, coarse=8, max_levels=16, omega=0.8), **psolve_options))
        return opt

    def lsolve_bicgstab(self, t, gamma, r, y=None, guess=None, part="diffusion", precondition=True, max_iters=200, rtol=1e-8, atol=0.0, **psolve_options):
        """(z, stats) of (I - gamma J_part(t, y)) z = r by right-preconditioned BiCGStab on the device (crd_bicgstab_host): a short
        recurrence with eight work vectors, one iteration two matvecs and two cycles.  guess: a vector laid out like r to start from
        (None: from zero).  stats is the crd_bicgstab_stats structure: converged, iterations, half_exit, matvecs, psolves, breakdown,
        r_norm, res_norm (the recurrence's), true_res_norm (||r - A z|| by one more matvec).  Neither max_iters nor a breakdown is an
        error: stats.converged is 0 and z the last consistent iterate."""
        r = self._vector(r)
        y = None if y is None else self._vector(y)
        z = np.empty_like(r) if guess is None else np.array(self._vector(guess), copy=True)
        st = capi.BicgstabStats()
        opt = self._bicgstab_options(part, precondition, max_iters, guess is not None, rtol, atol, **psolve_options)
        self._check(lib().crd_bicgstab_host(self._h, t, gamma, C.byref(opt), None if y is None else y.ctypes.data, r.ctypes.data, z.ctypes.data, C.byref(st)),
                    "crd_bicgstab_host")
        return z, st

    def lsolve_bicgstab_info(self, part="diffusion", precondition=True, max_iters=200, rtol=1e-8, atol=0.0, **psolve_options):
        """Device bytes of the workspace Slab.lsolve_bicgstab keeps on the context (crd_bicgstab_info)."""
        opt, nbytes = self._bicgstab_options(part, precondition, max_iters, False, rtol, atol, **psolve_options), C.c_int64()
        self._check(lib().crd_bicgstab_info(self._h, C.byref(opt), C.byref(nbytes)), "crd_bicgstab_info")
        return nbytes.value

    # -- time stepping -----------------------------------------------------------------------------------------
    def set_stepper(self, stepper):
        s = STEPPERS[stepper] if isinstance(stepper, str) else stepper
        self._check(lib().crd_set_stepper(self._h, s), "crd_set_stepper")

    def step_rk4(self, t0, dt, nsteps, sync=True):
        self._check(lib().crd_step_rk4(self._h, t0, dt, nsteps), "crd_step_rk4")
        if sync:
            self.synchronize()

    def _imex_options(self, scheme, lsolve_options, solver="gmres"):
        opt = capi.ImexOptions()
        opt.scheme = capi.IMEX_SCHEMES[scheme] if isinstance(scheme, str) else scheme
        opt.solver = capi.IMEX_SOLVERS[solver] if isinstance(solver, str) else solver
        opt.lsolve = self._lsolve_options(**lsolve_options)
        return opt

    def step_imex(self, t0, dt, nsteps, scheme="ars222", solver="gmres", **lsolve_options):
        """nsteps IMEX steps of size dt on the resident state, the diffusion part implicit (crd_step_imex): scheme "euler", "ars222" or
        "ars443" (or a CRD_IMEX_* value); solver "gmres", "bicgstab" or "bicgstab-warm" (each stage's solve started from the one before;
        or a CRD_IMEX_SOLVER_* value); lsolve_options are Slab.lsolve's and reach every stage's solve.  Returns the crd_imex_stats
        structure: steps, t, solves, iterations, max_iterations, failed_step, failed_stage, worst_residual, max_abs_u.  A solve that
        does not converge raises CrdError (CRD_ESTATE) with that structure as its `stats`; the state is the last completed step's."""
        opt, st = self._imex_options(scheme, lsolve_options, solver), capi.ImexStats()
        rc = lib().crd_step_imex(self._h, t0, dt, nsteps, C.byref(opt), C.byref(st))
        if rc != capi.OK:
            err = CrdError(rc, "crd_step_imex", lib().crd_last_error(self._h).decode())
            err.stats = st
            raise err
        return st

    def imex_info(self, scheme="ars222", solver="gmres", **lsolve_options):
        """Device bytes crd_step_imex with these options keeps on the context, the chosen solver's workspace included (crd_imex_info)."""
        opt, nbytes = self._imex_options(scheme, lsolve_options, solver), C.c_int64()
        self._check(lib().crd_imex_info(self._h, C.byref(opt), C.byref(nbytes)), "crd_imex_info")
        return nbytes.value

    def integrate_imex(self, t0, tout, rtol=1e-5, atol=1e-10, h0=0.0, h_max=0.0, safety=0.96, bias=1.5, growth=20.0, shrink=0.1, max_steps=200000, scheme="ars443",
                       solver="gmres", history=False, lsolve_rtol=1e-8, lsolve_atol=0.0, **lsolve_options):
        """Error-controlled IMEX integration of the resident state from t0 to tout (crd_integrate_imex): ARS(4,4,3) with its embedded
        second-order solution, the step sizes found from rtol and atol.  h0: the first step (0: crd_stable_dt); h_max > 0 caps the step;
        max_steps bounds the attempts, rejected ones included; solver and lsolve_options as Slab.step_imex, but for the solves' own
        tolerances, which are lsolve_rtol and lsolve_atol here (rtol and atol are the integrator's).  Returns the
        crd_imex_adaptive_stats structure (imex: crd_step_imex's figures; accepted, rejected, attempts, recorded, h_first, h_last,
        h_next -- the next call's h0 --, h_min, h_max, err_last, t), and with history=True (or a capacity) the pair (stats, [attempt
        records: t, h, err = bias x norm, accepted, iterations]).  A call that stops short of tout raises CrdError (CRD_ESTATE) with
        that structure as its `stats` and the records as its `history`; the state is the last accepted step's."""
        opt = capi.ImexAdaptiveOptions()
        opt.imex = self._imex_options(scheme, dict(lsolve_options, rtol=lsolve_rtol, atol=lsolve_atol), solver)
        opt.rtol, opt.atol, opt.h0, opt.h_max, opt.safety, opt.bias, opt.growth, opt.shrink, opt.max_steps = rtol, atol, h0, h_max, safety, bias, growth, shrink, max_steps
        cap = 0 if not history else (4096 if history is True else int(history))
        records = (capi.ImexAttempt * cap)() if cap else None
        st = capi.ImexAdaptiveStats()
        rc = lib().crd_integrate_imex(self._h, t0, tout, C.byref(opt), C.byref(st), records, cap)
        taken = [records[i] for i in range(st.recorded)] if cap else []
        if rc != capi.OK:
            err = CrdError(rc, "crd_integrate_imex", lib().crd_last_error(self._h).decode())
            err.stats, err.history = st, taken
            raise err
        return (st, taken) if history else st

    def imex_estimate_probe(self, R, k, yn, stored, hg, dt, rtol, atol):
        """(out, e, sum, max |var0|) of the estimating last close of crd_integrate_imex run alone (crd_imex_estimate_probe): R, k, yn and
        the seven `stored` vectors FR_0, FR_1, k_1, FR_2, k_2, FR_3, k_3 are laid out like the state, in the slab's precision."""
        assert len(stored) == 7
        vecs = np.ascontiguousarray(np.stack([self._vector(x) for x in [R, k, yn] + list(stored)]))
        out = np.empty((2,) + vecs.shape[1:], dtype=vecs.dtype)
        scalars, result = (C.c_double * 4)(hg, dt, rtol, atol), (C.c_double * 2)()
        self._check(lib().crd_imex_estimate_probe(self._h, scalars, vecs.ctypes.data, out.ctypes.data, result), "crd_imex_estimate_probe")
        return out[0], out[1], result[0], result[1]

    def step_rk4_timed(self, t0, dt, nsteps):
        ms, kms, lps = C.c_double(), C.c_double(), C.c_int()
        self._check(lib().crd_step_rk4_timed(self._h, t0, dt, nsteps, C.byref(ms), C.byref(kms), C.byref(lps)), "crd_step_rk4_timed")
        return ms.value, kms.value, lps.value

    def integrate_adaptive(self, t0, tout, **options):
        """Error-controlled integration from t0 to tout; options override crd_adaptive_defaults (rtol, atol, h0, method, ...): by
        default the reference's integrator (ARKode's Zonneveld 5(3)4 pair + PID controller, ARK_NORMAL output); method=0 with
        dense_output=0/1 is the RK4(3) pair of earlier rounds.  Returns stats."""
        opt, st = _adaptive_options(options), capi.AdaptiveStats()
        rc = lib().crd_integrate_adaptive(self._h, t0, tout, C.byref(opt), C.byref(st))
        return _adaptive_result(rc, st, "crd_integrate_adaptive", self._h)

    def synchronize(self):
        self._check(lib().crd_synchronize(self._h), "crd_synchronize")

    def set_diagnostics(self, on):
        """Per-exchange event pairs in the next step_rk4_timed calls (RCCL contexts): see step_timing()."""
        self._check(lib().crd_set_diagnostics(self._h, 1 if on else 0), "crd_set_diagnostics")

    def set_halo_slack(self, sweeps):
        """1 or 2 sweeps of owned-only rows between an exchange and the wait for its halo (crd_set_halo_slack)."""
        self._check(lib().crd_set_halo_slack(self._h, sweeps), "crd_set_halo_slack")

    def set_exchange_period(self, steps):
        """Fused steps between two deep-halo exchanges (crd_set_exchange_period): 3 .. 16, the same on every slab / rank of a run."""
        self._check(lib().crd_set_exchange_period(self._h, steps), "crd_set_exchange_period")

    def exchange_period(self):
        return lib().crd_get_exchange_period(self._h)

    def step_timing(self):
        """What the last step_rk4_timed call measured (crd_step_timing) as a dict."""
        tm = capi.StepTiming()
        self._check(lib().crd_get_step_timing(self._h, C.byref(tm)), "crd_get_step_timing")
        return {f: getattr(tm, f) for f, _ in tm._fields_ if f != "reserved"}

    def dominant_kernel_rows(self):
        v = C.c_int64()
        self._check(lib().crd_dominant_kernel_rows(self._h, C.byref(v)), "crd_dominant_kernel_rows")
        return v.value

    def dominant_kernel(self):
        return lib().crd_dominant_kernel_name(self._h).decode()

    def set_autotune(self, on):
        """0 / False: never measure a launch plan; 1 / True: measure on the first full-size launch; 2: ... and print the timings."""
        self._check(lib().crd_set_autotune(self._h, int(on)), "crd_set_autotune")

    def set_launch_plan(self, chunk_mode, xcd_mapping, columns_per_lane, nontemporal_stores=0, steps_per_launch=1):
        """Pin the launch plan of the fixed-step kernel (crd_set_launch_plan) instead of having it measured."""
        self._check(lib().crd_set_launch_plan(self._h, chunk_mode, xcd_mapping, columns_per_lane, nontemporal_stores, steps_per_launch), "crd_set_launch_plan")

    def plan_launches(self):
        """Measure the fused step kernel's launch plan now (state not advanced) rather than inside the first step_rk4."""
        self._check(lib().crd_plan_launches(self._h), "crd_plan_launches")

    def launch_plan(self):
        """The fused step kernel's launch plan as a dict (crd_launch_plan)."""
        lp = capi.LaunchPlan()
        self._check(lib().crd_get_launch_plan(self._h, C.byref(lp)), "crd_get_launch_plan")
        return {f: getattr(lp, f) for f, _ in lp._fields_ if f != "reserved"}

    def launch_geometry(self):
        """The full-height launch under the current plan + what the build's kernel table says about its kernel (crd_launch_geometry)."""
        g = capi.LaunchGeometry()
        self._check(lib().crd_get_launch_geometry(self._h, C.byref(g)), "crd_get_launch_geometry")
        return {f: getattr(g, f) for f, _ in g._fields_ if f != "reserved"}

    def max_abs(self):
        v = C.c_double()
        self._check(lib().crd_state_max_abs(self._h, C.byref(v)), "crd_state_max_abs")
        return v.value

    def observe(self):
        """min, max, sum and sum of squares of both fields of a single-slab context's state, [2, 4] (crd_state_observe): the row an
        Ensemble of one holding this state records, bit for bit."""
        v = np.empty((2, 4))
        self._check(lib().crd_state_observe(self._h, v.ctypes.data_as(C.POINTER(C.c_double))), "crd_state_observe")
        return v

    def section(self, kind, index=0):
        """One section of a single-slab context's state, [length, 2] (crd_state_section): kind "row" (along theta at row `index`),
        "column" (along phi at column `index`), "theta_mean" (the axial profile) or "phi_mean" (the profile around the tube) -- the
        line an Ensemble of one holding this state records, bit for bit."""
        kind = _section_kind(kind)
        g = self.grid
        length = g.nx if kind in (capi.SECTION_ROW, capi.SECTION_PHI_MEAN) else g.ny
        v = np.empty((length, 2))
        self._check(lib().crd_state_section(self._h, kind, int(index), v.ctypes.data), "crd_state_section")
        return v

    # -- RCCL wiring -------------------------------------------------------------------------------------------
    def init_rccl(self, unique_id):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(lib().crd_comm_init_rccl(self._h, buf), "crd_comm_init_rccl")

    def comm_info(self):
        """(transport, ranks, rank): transport is 'self' / 'local' / 'rccl'; for RCCL the last two come from the communicator."""
        halo, ranks, rank = C.c_int(), C.c_int(), C.c_int()
        self._check(lib().crd_comm_info(self._h, C.byref(halo), C.byref(ranks), C.byref(rank)), "crd_comm_info")
        return {0: "self", 1: "local", 2: "rccl"}.get(halo.value, "unwired"), ranks.value, rank.value

    def halo_exchange(self, depth=32):
        """One exchange of `depth` ghost rows of both fields with the ring neighbours, outside any step; waits for it."""
        self._check(lib().crd_halo_exchange(self._h, depth), "crd_halo_exchange")


def _section_kind(kind):
    if isinstance(kind, str):
        name = kind.replace("-", "_")
        if name not in capi.SECTION_KINDS:
            raise ValueError("a section is one of %s (got %r)" % (", ".join(sorted(capi.SECTION_KINDS)), kind))
        return capi.SECTION_KINDS[name]
    return int(kind)


class Ensemble:
    """B independent single-slab problems on one GPU, stepped by one launch per RK4 step (crd_ensemble).  params_list: one Params per
    member; by default members share model, surface, nx, ny, surface length / width, precision and justDiffusion, and may differ in diffusion,
    beta, betaMin, betaMax, varyBeta and tBoundary.  Each member's result is bit-identical to a Slab of the same params stepped alone.
    mixed=True (crd_ensemble_create_mixed): members share model, precision and justDiffusion only and may also differ in surface, nx, ny
    and the surface's length and width; grid(member) is each member's own grid, and upload, download and observed_maps are shaped by it.
    Members of different nx or ny take fixed steps (one or two per launch) and the basic observer; integrate_adaptive, sections and
    cycle maps raise CrdError for them."""

    def __init__(self, params_list, device=0, mixed=False):
        self._h = C.c_void_p()
        self.params = list(params_list)
        arr = (Params * max(len(self.params), 1))(*self.params)
        create, name = (lib().crd_ensemble_create_mixed, "crd_ensemble_create_mixed") if mixed else (lib().crd_ensemble_create, "crd_ensemble_create")
        rc = create(arr, len(self.params), device, C.byref(self._h))
        if rc != capi.OK:
            self._h = None
            raise CrdError(rc, name, lib().crd_ensemble_last_error(None).decode())
        n, g = C.c_int(), Grid()
        self._check(lib().crd_ensemble_info(self._h, C.byref(n), C.byref(g)), "crd_ensemble_info")
        self.n_members = n.value
        self.nx, self.ny = g.nx, g.ny  # member 0's
        self.grids = []
        for k in range(self.n_members):
            gk = Grid()
            self._check(lib().crd_ensemble_member_grid(self._h, k, C.byref(gk)), "crd_ensemble_member_grid")
            self.grids.append(gk)
        self.dtype = np.float64 if self.params[0].precision == PRECISION_F64 else np.float32

    def __len__(self):
        return self.n_members

    def grid(self, member=0):
        """Member `member`'s grid (crd_ensemble_member_grid); without mixed=True every member's is member 0's.  (Before mixed
        geometry `grid` was an attribute holding the common Grid: `e.grid.nx` is now `e.grid().nx`, or `e.nx`.)"""
        return self.grids[member]

    def _shape(self, member):
        g = self.grids[member]
        return (g.ny, g.nx)

    # -- lifecycle ---------------------------------------------------------------------------------------------
    def close(self):
        if self._h:
            lib().crd_ensemble_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    def _check(self, rc, where):
        if rc != capi.OK:
            raise CrdError(rc, where, lib().crd_ensemble_last_error(self._h).decode())

    # -- state -------------------------------------------------------------------------------------------------
    def upload(self, member, y):
        y = np.ascontiguousarray(y)
        assert y.shape == self._shape(member) + (2,), (y.shape, self._shape(member) + (2,))
        if y.dtype == np.float64:
            self._check(lib().crd_ensemble_upload(self._h, member, y.ctypes.data, 1), "crd_ensemble_upload")
        elif y.dtype == np.float32 and self.dtype == np.float32:
            self._check(lib().crd_ensemble_upload(self._h, member, y.ctypes.data, 0), "crd_ensemble_upload")
        else:
            raise TypeError("state must be float64, or float32 for an f32 ensemble")

    def download(self, member, dtype=np.float64):
        y = np.empty(self._shape(member) + (2,), dtype=dtype)
        self._check(lib().crd_ensemble_download(self._h, member, y.ctypes.data, 1 if y.dtype == np.float64 else 0), "crd_ensemble_download")
        return y

    # -- time stepping -----------------------------------------------------------------------------------------
    def step_rk4(self, t0, dt, nsteps, sync=True):
        self._check(lib().crd_ensemble_step_rk4(self._h, t0, dt, nsteps), "crd_ensemble_step_rk4")
        if sync:
            self.synchronize()

    def step_rk4_timed(self, t0, dt, nsteps):
        """Device time of the batch in ms (blocks until done)."""
        ms = C.c_double()
        self._check(lib().crd_ensemble_step_rk4_timed(self._h, t0, dt, nsteps, C.byref(ms)), "crd_ensemble_step_rk4_timed")
        return ms.value

    def own_steps(self, t0, t1, dt_safety=0.8):
        """The steps each member takes from t0 to t1 at its own bound (crd_ensemble_own_steps): per member
        ceil((t1 - t0) / (dt_safety * stable_dt(params)) - 1e-12), at least 1 -- a lone crd_run's rule per output interval."""
        n = (C.c_int64 * self.n_members)()
        self._check(lib().crd_ensemble_own_steps(self._h, t0, t1, dt_safety, n), "crd_ensemble_own_steps")
        return list(n)

    def step_rk4_own(self, t0, t1, nsteps=None, dt_safety=0.8, sync=True, dt=None):
        """Every member from t0 to t1 at its own step size (crd_ensemble_step_rk4_own): member k takes nsteps[k] RK4 steps of
        (t1 - t0) / nsteps[k], bit-identical to a Slab of its params taking them alone; one launch per round for the members that still
        have steps left.  nsteps=None: own_steps(t0, t1, dt_safety).  With an observer open, one sample at t1.  dt: the members' step
        sizes given instead of formed (crd_ensemble_step_rk4_own_dt; t1 is then the sample's time only).  Returns the counts used."""
        counts = self.own_steps(t0, t1, dt_safety) if nsteps is None else [int(n) for n in nsteps]
        if len(counts) != self.n_members:
            raise ValueError("nsteps needs one count per member (%d), got %d" % (self.n_members, len(counts)))
        arr = (C.c_int64 * self.n_members)(*counts)
        if dt is None:
            self._check(lib().crd_ensemble_step_rk4_own(self._h, t0, t1, arr), "crd_ensemble_step_rk4_own")
        else:
            if len(dt) != self.n_members:
                raise ValueError("dt needs one step size per member (%d), got %d" % (self.n_members, len(dt)))
            self._check(lib().crd_ensemble_step_rk4_own_dt(self._h, t0, t1, (C.c_double * self.n_members)(*[float(h) for h in dt]), arr), "crd_ensemble_step_rk4_own_dt")
        if sync:
            self.synchronize()
        return counts

    def step_rk4_own_timed(self, t0, t1, nsteps):
        """step_rk4_own bracketed by events: device time of the call in ms (blocks until done)."""
        arr = (C.c_int64 * self.n_members)(*[int(n) for n in nsteps])
        ms = C.c_double()
        self._check(lib().crd_ensemble_step_rk4_own_timed(self._h, t0, t1, arr, C.byref(ms)), "crd_ensemble_step_rk4_own_timed")
        return ms.value

    def synchronize(self):
        self._check(lib().crd_ensemble_synchronize(self._h), "crd_ensemble_synchronize")

    def set_steps_per_launch(self, n):
        """RK4 steps one launch of step_rk4 takes: 1 (the default) or 2 -- pairs, with the bits of single steps
        (crd_ensemble_set_steps_per_launch).  CrdError for anything else, and for 2 on members of fewer than
        CRD_ENSEMBLE_PAIR_MIN_ROWS rows; the setting is then unchanged."""
        self._check(lib().crd_ensemble_set_steps_per_launch(self._h, int(n)), "crd_ensemble_set_steps_per_launch")

    @property
    def steps_per_launch(self):
        return int(lib().crd_ensemble_get_steps_per_launch(self._h))

    def max_abs(self):
        """max |var0| per member (a list; non-finite for a member that blew up)."""
        v = (C.c_double * self.n_members)()
        self._check(lib().crd_ensemble_max_abs(self._h, v), "crd_ensemble_max_abs")
        return list(v)

    def integrate_adaptive(self, t0, tout, **options):
        """Error-controlled integration of every member from t0 to tout (crd_ensemble_integrate_adaptive): each member steps as a Slab of
        its params would with Slab.integrate_adaptive and the same options (CRD_ADAPT_ARKODE only).  Returns one stats dict per member,
        each with a `status` entry (OK, or ESTATE for a member that failed alone -- the others still reach tout); raises CrdError only for
        failures of the call itself."""
        opt = _adaptive_options(options)
        st = (capi.AdaptiveStats * self.n_members)()
        status = (C.c_int32 * self.n_members)()
        rc = lib().crd_ensemble_integrate_adaptive(self._h, t0, tout, C.byref(opt), st, status)
        if rc not in (capi.OK, capi.ESTATE):
            raise CrdError(rc, "crd_ensemble_integrate_adaptive", lib().crd_ensemble_last_error(self._h).decode())
        out = []
        for k in range(self.n_members):
            d = {f: getattr(st[k], f) for f, _ in st[k]._fields_}
            d["status"] = status[k]
            out.append(d)
        return out

    # -- observers ---------------------------------------------------------------------------------------------
    def observe(self, stride=1, probes=(), maps=False, threshold=0.0, capacity=1024, sections=(), cycles=False, cycle_threshold=0.0):
        """Open the observer (crd_ensemble_observe_begin): from now on step_rk4 records a sample of every member after each stride-th
        step and integrate_adaptive one per call -- field statistics, both fields at the `probes` (i, j) = (theta, phi index) and, with
        maps, the running minimum / maximum of var0 and the activation time (first sample with var0 >= threshold) per grid point -- on
        the device, without a synchronisation.  capacity: samples the record buffer holds.  Returns the observer's info: the sampling
        blocks per member and the values per field, which state the sums' rounding bound.
        sections: up to 8 of ("row", j), ("column", i), ("theta_mean",), ("phi_mean",) -- a line of both fields per sample and member
        (observed_section).  cycles: also count, per grid point, the upward crossings of cycle_threshold by var0 between consecutive
        samples and keep the times of the first and the last (observed_cycles).  Without either this is crd_ensemble_observe_begin."""
        probes = list(probes)
        opt = capi.ObserveOptions()
        opt.stride, opt.n_probes, opt.maps, opt.threshold = int(stride), len(probes), 1 if maps else 0, float(threshold)
        if len(probes) > capi.OBSERVE_MAX_PROBES:
            raise ValueError("at most %d probes" % capi.OBSERVE_MAX_PROBES)
        for q, (i, j) in enumerate(probes):
            opt.probe_i[q], opt.probe_j[q] = int(i), int(j)
        sections = [tuple(s) if isinstance(s, (tuple, list)) else (s,) for s in sections]
        if not sections and not cycles:
            self._check(lib().crd_ensemble_observe_begin(self._h, C.byref(opt), int(capacity)), "crd_ensemble_observe_begin")
            return self.observe_info()
        if len(sections) > capi.OBSERVE_MAX_SECTIONS:
            raise ValueError("at most %d sections" % capi.OBSERVE_MAX_SECTIONS)
        ex = capi.ObserveExtras()
        ex.n_sections, ex.cycles, ex.cycle_threshold = len(sections), 1 if cycles else 0, float(cycle_threshold)
        for q, sec in enumerate(sections):
            ex.kind[q], ex.index[q] = _section_kind(sec[0]), int(sec[1]) if len(sec) > 1 else 0
        self._check(lib().crd_ensemble_observe_begin_with(self._h, C.byref(opt), C.byref(ex), int(capacity)), "crd_ensemble_observe_begin_with")
        return self.observe_info()

    def observed_section_info(self, section):
        """Section `section` of the open observer: kind, index, length and D -- a mean of n values x lies within D 2^-53 sum|x| / n of
        the exact mean (0 for the exact kinds)."""
        kind, index, length, additions = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self._check(lib().crd_ensemble_observe_section_info(self._h, int(section), C.byref(kind), C.byref(index), C.byref(length), C.byref(additions)),
                    "crd_ensemble_observe_section_info")
        return {"kind": kind.value, "index": index.value, "length": length.value, "additions": additions.value}

    def observed_section(self, section, first=0, count=None):
        """The recorded lines of section `section`, [sample, member, length, 2] (default: every sample).  Synchronises; one copy."""
        length = self.observed_section_info(section)["length"]
        if count is None:
            count = self.observed_count() - first
        v = np.empty((count, self.n_members, length, 2))
        self._check(lib().crd_ensemble_observe_read_section(self._h, int(section), first, count, v.ctypes.data), "crd_ensemble_observe_read_section")
        return v

    def observed_cycles(self, member):
        """Member `member`'s cycle maps as they stand, [ny, nx] each: (count of upward crossings, time of the first, time of the last,
        period map = (t_last - t_first) / (count - 1) where count >= 2, NaN elsewhere)."""
        count = np.empty((self.ny, self.nx), dtype=np.int32)
        t_first, t_last = np.empty((self.ny, self.nx)), np.empty((self.ny, self.nx))
        self._check(lib().crd_ensemble_observe_cycles(self._h, member, count.ctypes.data, t_first.ctypes.data, t_last.ctypes.data), "crd_ensemble_observe_cycles")
        return count, t_first, t_last, period_map(count, t_first, t_last)

    def observe_info(self):
        blocks, values, opt, cap = C.c_int32(), C.c_int64(), capi.ObserveOptions(), C.c_int64()
        self._check(lib().crd_ensemble_observe_info(self._h, C.byref(blocks), C.byref(values), C.byref(opt), C.byref(cap)), "crd_ensemble_observe_info")
        return {"blocks_per_member": blocks.value, "values_per_field": values.value, "stride": opt.stride, "maps": bool(opt.maps), "threshold": opt.threshold,
                "probes": [(opt.probe_i[q], opt.probe_j[q]) for q in range(opt.n_probes)], "capacity": cap.value}

    def observed_count(self):
        n = C.c_int64()
        self._check(lib().crd_ensemble_observe_count(self._h, C.byref(n)), "crd_ensemble_observe_count")
        return n.value

    def observations(self, first=0, count=None):
        """The recorded samples first .. first + count - 1 (default: all): a dict of numpy arrays -- t [samples], stats [samples, members,
        2 fields, 4: min, max, sum, sum of squares], probes [samples, members, probes, 2 fields] -- and, derived here, mean and variance
        [samples, members, 2] (the population variance sum x^2 / n - mean^2, clipped at 0).  Synchronises; one copy."""
        info = self.observe_info()
        if count is None:
            count = self.observed_count() - first
        P = len(info["probes"])
        t = np.empty(count)
        stats = np.empty((count, self.n_members, 2, 4))
        probes = np.empty((count, self.n_members, P, 2))
        self._check(lib().crd_ensemble_observe_read(self._h, first, count, t.ctypes.data, stats.ctypes.data, probes.ctypes.data), "crd_ensemble_observe_read")
        n = np.array([float(g.nx) * float(g.ny) for g in self.grids])[None, :, None]  # values per field, per member
        mean = stats[..., 2] / n
        with np.errstate(invalid="ignore"):
            variance = np.maximum(stats[..., 3] / n - mean * mean, 0.0)
        variance[np.isnan(mean)] = np.nan
        return {"t": t, "stats": stats, "probes": probes, "mean": mean, "variance": variance}

    def observed_maps(self, member):
        """Member `member`'s maps as they stand: (running minimum of var0, running maximum, activation time), [ny, nx] each."""
        out = [np.empty(self._shape(member)) for _ in range(3)]
        self._check(lib().crd_ensemble_observe_maps(self._h, member, *[a.ctypes.data for a in out]), "crd_ensemble_observe_maps")
        return tuple(out)

    def end_observe(self):
        self._check(lib().crd_ensemble_observe_end(self._h), "crd_ensemble_observe_end")

    def last_error(self):
        return lib().crd_ensemble_last_error(self._h).decode()


class PinnedArray:
    """A numpy array over page-locked host memory from crd_host_alloc (freed with the object)."""

    def __init__(self, shape, dtype=np.float64):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = lib().crd_host_alloc(self.nbytes)
        if not self._p:
            raise MemoryError("crd_host_alloc(%d) failed" % self.nbytes)
        self.array = np.frombuffer((C.c_char * self.nbytes).from_address(self._p), dtype=dtype).reshape(shape)

    def close(self):
        if self._p:
            self.array = None
            lib().crd_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def launch_plan_candidates(eight_wide=False):
    """The plans the launch-plan measurement chooses among, as (chunk_mode, xcd_mapping, columns_per_lane, nontemporal_stores, steps per launch).

    By default the plans whose kernel is named by (precision, model, columns, store hint, steps) alone -- how the profile records and
    the kernel table are keyed.  eight_wide=True: the chunk-mode-3 plans (eight wavefronts per block strip) alone, whose kernel is a
    further instantiation under the same five (the table rows with "waves": 8): their records carry that kernel's digest
    (tests/test_block_strip_eight_host.py checks them)."""
    out, k = [], 0
    while True:
        lp = capi.LaunchPlan()
        if lib().crd_launch_plan_candidate(k, C.byref(lp)) != 0:
            return out
        if (lp.one_round == 3) == bool(eight_wide):
            out.append((lp.one_round, lp.xcd_mapping, lp.columns_per_lane, lp.nontemporal_stores, lp.steps_per_launch))
        k += 1


def steps_per_launch_on(model, precision, nx, nyl, steps_wanted, single_slab=True):
    """crd_steps_per_launch_on: the steps per launch a plan asking for `steps_wanted` gets on a slab of nx x nyl points (no device needed)."""
    rc = lib().crd_steps_per_launch_on(MODELS[model] if isinstance(model, str) else model,
                                       {"f64": PRECISION_F64, "f32": PRECISION_F32}[precision] if isinstance(precision, str) else precision,
                                       nx, nyl, 1 if single_slab else 0, steps_wanted)
    check(min(rc, 0), "crd_steps_per_launch_on")
    return rc


def rows_addressable(nx, rows, real_bytes=8):
    """crd_rows_addressable: `rows` rows of nx reals span less than 2^32 bytes minus one row (the three-step fp64 kernel's 32-bit row offsets)."""
    return bool(lib().crd_rows_addressable(nx, rows, real_bytes))


def plan_key(model, precision, plan):
    """Key of a launch plan in profiles/pmc_traffic.json / profiles/plan_stats.json: plan = (chunk_mode, mapping, columns, nt[, steps per
    launch]) or the dict Slab.launch_plan() returns."""
    if isinstance(plan, dict):
        plan = (plan["one_round"], plan["xcd_mapping"], plan["columns_per_lane"], plan["nontemporal_stores"], plan.get("steps_per_launch", 1))
    key = "fused/%s/%s/chunk%d/map%d/cols%d/%s" % (model, precision, plan[0], plan[1], plan[2], "nt" if plan[3] else "plain")
    return key + ("/steps%d" % plan[4] if len(plan) > 4 and plan[4] >= 2 else "")


def kernel_table_digest():
    """crd_kernel_table_digest: 16 hex digits over the step kernels of the loaded library ("" for a build without the table)."""
    return lib().crd_kernel_table_digest().decode()


def kernel_digest(geometry):
    """16 hex digits over what the build's kernel table says about ONE kernel -- the one `geometry` (Slab.launch_geometry()) describes:
    registers, LDS, scratch, occupancy and the instruction mix of its steady-state loop.  profiles/pmc_traffic.json and plan_stats.json
    stamp every entry with the digest of the kernel it was measured on; bench.py quotes an entry only while the loaded library's kernel
    still has that digest (a changed kernel makes its own entries stale, not the other kernels')."""
    import hashlib

    fields = ("vgprs", "sgprs", "lds_bytes", "scratch_bytes", "wavefronts_per_simd", "loop_valu", "loop_salu", "loop_vmem", "loop_lds", "loop_instructions", "exec_skipped_vmem")
    if not geometry or not geometry.get("vgprs"):
        return ""
    return hashlib.sha256(",".join("%s=%d" % (f, int(geometry[f])) for f in fields).encode()).hexdigest()[:16]


def kernel_digest_of_table_row(row):
    """The same digest from a row of csrc/build/kernel_table.json (tools/kernel_regs.py --json): what a build's kernel would report
    through crd_get_launch_geometry, without a device (tests/test_profiles.py)."""
    lp = row["loop"]
    return kernel_digest({"vgprs": row["vgprs"], "sgprs": row["sgprs"], "lds_bytes": row["lds_bytes"], "scratch_bytes": row["scratch_bytes"], "wavefronts_per_simd": row["wavefronts_per_simd"],
                          "loop_valu": lp["valu"], "loop_salu": lp["salu"], "loop_vmem": lp["vmem"], "loop_lds": lp["lds"], "loop_instructions": lp["total"],
                          "exec_skipped_vmem": row.get("exec_skipped_vmem", 0)})


def rccl_unique_id():
    buf = C.create_string_buffer(128)
    check(lib().crd_comm_unique_id(buf), "crd_comm_unique_id")
    return buf.raw


class LocalGroup:
    """All slabs of one run inside this process (one host thread drives every GPU, or several slabs on one GPU).  blocks = (d0, d1):
    the reference's 2-D decomposition instead of phi-slabs, d0 theta-blocks x d1 phi-blocks, in rank order c0 d1 + c1."""

    def __init__(self, params, n_slabs, devices=None, blocks=None):
        if blocks is not None:
            d0, d1 = blocks
            n_slabs = d0 * d1
        devices = devices or [0] * n_slabs
        if blocks is None:
            self.slabs = [Slab(params, k, n_slabs, devices[k]) for k in range(n_slabs)]
        else:
            self.slabs = [Slab(params, device=devices[c0 * d1 + c1], block=(c0, d0, c1, d1)) for c0 in range(d0) for c1 in range(d1)]
        self._arr = (C.c_void_p * n_slabs)(*[s.handle for s in self.slabs])
        check(lib().crd_comm_attach_local(self._arr, n_slabs), "crd_comm_attach_local", self.slabs[0].handle)
        self.grid = self.slabs[0].grid

    def upload(self, y):
        for s in self.slabs:
            s.upload(y[s.js:s.je + 1, s.is_:s.ie + 1])

    def _assemble(self, parts, dtype):
        out = np.empty((self.grid.ny, self.grid.nx, 2), dtype=dtype)
        for s, q in zip(self.slabs, parts):
            out[s.js:s.je + 1, s.is_:s.ie + 1] = q
        return out

    def download(self, dtype=np.float64):
        return self._assemble([s.download(dtype) for s in self.slabs], dtype)

    def f(self, t, y):
        """ydot = f(t, y) on the whole grid, evaluated block by block with halos exchanged between the blocks' vectors."""
        n = len(self.slabs)
        parts = [np.ascontiguousarray(y[s.js:s.je + 1, s.is_:s.ie + 1], dtype=s.dtype) for s in self.slabs]
        outs = [np.empty_like(q) for q in parts]
        ins = (C.c_void_p * n)(*[q.ctypes.data for q in parts])
        out = (C.c_void_p * n)(*[q.ctypes.data for q in outs])
        check(lib().crd_group_rhs_host(self._arr, n, t, ins, out), "crd_group_rhs_host", self.slabs[0].handle)
        return self._assemble(outs, outs[0].dtype)

    def _split(self, y):
        parts = [np.ascontiguousarray(y[s.js:s.je + 1, s.is_:s.ie + 1], dtype=s.dtype) for s in self.slabs]
        return parts, (C.c_void_p * len(parts))(*[q.ctypes.data for q in parts])

    def rhs_part(self, t, y, part):
        """One part of f(t, y) on the whole grid (Slab.rhs_part), slab by slab with the halos of y exchanged between the slabs' vectors."""
        n = len(self.slabs)
        ys, ins = self._split(y)
        outs, out = self._split(np.empty((self.grid.ny, self.grid.nx, 2), dtype=ys[0].dtype))
        check(lib().crd_group_rhs_part_host(self._arr, n, t, _part(part), ins, out), "crd_group_rhs_part_host", self.slabs[0].handle)
        return self._assemble(outs, outs[0].dtype)

    def jtimes(self, t, y, v, part="full"):
        """J_part(t, y) v on the whole grid (Slab.jtimes): the halos exchanged are those of v."""
        n = len(self.slabs)
        ys, ins = self._split(y)
        vs, vins = self._split(v)
        outs, out = self._split(np.empty((self.grid.ny, self.grid.nx, 2), dtype=ys[0].dtype))
        check(lib().crd_group_jtimes_host(self._arr, n, t, _part(part), ins, vins, out), "crd_group_jtimes_host", self.slabs[0].handle)
        return self._assemble(outs, outs[0].dtype)

    def step_rk4(self, t0, dt, nsteps):
        check(lib().crd_group_step_rk4(self._arr, len(self.slabs), t0, dt, nsteps), "crd_group_step_rk4", self.slabs[0].handle)
        for s in self.slabs:
            s.synchronize()

    def step_rk4_timed(self, t0, dt, nsteps):
        """crd_group_step_rk4_timed: the group call with event pairs on every slab; returns each slab's step_timing()."""
        check(lib().crd_group_step_rk4_timed(self._arr, len(self.slabs), t0, dt, nsteps), "crd_group_step_rk4_timed", self.slabs[0].handle)
        return [s.step_timing() for s in self.slabs]

    def set_stepper(self, stepper):
        for s in self.slabs:
            s.set_stepper(stepper)

    def set_halo_slack(self, sweeps):
        for s in self.slabs:
            s.set_halo_slack(sweeps)

    def set_exchange_period(self, steps):
        for s in self.slabs:
            s.set_exchange_period(steps)

    def set_threads(self, threads):
        """Host threads issuing the group's work in step_rk4 (crd_group_set_threads): 0 = one per device."""
        check(lib().crd_group_set_threads(self._arr, len(self.slabs), threads), "crd_group_set_threads", self.slabs[0].handle)

    def integrate_adaptive(self, t0, tout, **options):
        opt, st = _adaptive_options(options), capi.AdaptiveStats()
        rc = lib().crd_group_integrate_adaptive(self._arr, len(self.slabs), t0, tout, C.byref(opt), C.byref(st))
        stats = _adaptive_result(rc, st, "crd_group_integrate_adaptive", self.slabs[0].handle)
        for s in self.slabs:
            s.synchronize()
        return stats

    def close(self):
        for s in self.slabs:
            s.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Recorder:
    """The run recorder (crd_recorder_open) of a Slab or of a LocalGroup: while the target steps, statistics, probes, sections, maps
    and cycle maps are recorded on the device -- a sample after every stride-th fixed step (the count carries over calls), one per
    integrate_adaptive call at tout.  Probes (i, j), ("row", j) and ("column", i) are indices on the global grid.  Every recorded bit is
    the same for a lone Slab and for any LocalGroup cut of the same grid.  The state steps exactly as without a recorder.  A context
    manager; closing the target closes the recorder too."""

    def __init__(self, target, stride=1, probes=(), maps=False, threshold=0.0, sections=(), cycles=False, cycle_threshold=0.0, capacity=1024):
        self._h = None
        self._slabs = list(target.slabs) if hasattr(target, "slabs") else [target]
        self.grid = self._slabs[0].grid
        probes = list(probes)
        if len(probes) > capi.OBSERVE_MAX_PROBES:
            raise ValueError("at most %d probes" % capi.OBSERVE_MAX_PROBES)
        sections = [tuple(s) if isinstance(s, (tuple, list)) else (s,) for s in sections]
        if len(sections) > capi.OBSERVE_MAX_SECTIONS:
            raise ValueError("at most %d sections" % capi.OBSERVE_MAX_SECTIONS)
        opt = capi.ObserveOptions()
        opt.stride, opt.n_probes, opt.maps, opt.threshold = int(stride), len(probes), 1 if maps else 0, float(threshold)
        for q, (i, j) in enumerate(probes):
            opt.probe_i[q], opt.probe_j[q] = int(i), int(j)
        ex = capi.ObserveExtras()
        ex.n_sections, ex.cycles, ex.cycle_threshold = len(sections), 1 if cycles else 0, float(cycle_threshold)
        for q, sec in enumerate(sections):
            ex.kind[q], ex.index[q] = _section_kind(sec[0]), int(sec[1]) if len(sec) > 1 else 0
        n = len(self._slabs)
        arr = (C.c_void_p * n)(*[s.handle for s in self._slabs])
        h = C.c_void_p()
        check(lib().crd_recorder_open(arr, n, C.byref(opt), C.byref(ex), int(capacity), C.byref(h)), "crd_recorder_open", self._slabs[0].handle)
        self._h = h
        self.n_probes, self.n_sections = len(probes), len(sections)

    def _check(self, rc, where):
        check(rc, where, self._slabs[0].handle)

    def _alive(self):
        if not self._h or any(s.handle is None for s in self._slabs):  # (crd_destroy of a recorded context has closed it)
            self._h = None
            raise RuntimeError("the recorder is closed")
        return self._h

    def close(self):
        if self._h and all(s.handle is not None for s in self._slabs):
            lib().crd_recorder_close(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def count(self):
        n = C.c_int64()
        self._check(lib().crd_recorder_count(self._alive(), C.byref(n)), "crd_recorder_count")
        return n.value

    def info(self):
        """additions: D of the statistics' bound, |sum - exact| <= D 2^-53 sum|x| (sums of squares: D + 1); values_per_field; slabs;
        stride, n_probes, maps, n_sections, cycles, capacity."""
        d, values, slabs, cap = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64()
        opt, ex = capi.ObserveOptions(), capi.ObserveExtras()
        self._check(lib().crd_recorder_info(self._alive(), C.byref(d), C.byref(values), C.byref(slabs), C.byref(opt), C.byref(ex), C.byref(cap)), "crd_recorder_info")
        return {"additions": d.value, "values_per_field": values.value, "slabs": slabs.value, "stride": opt.stride, "n_probes": opt.n_probes, "maps": opt.maps,
                "threshold": opt.threshold, "n_sections": ex.n_sections, "cycles": ex.cycles, "cycle_threshold": ex.cycle_threshold, "capacity": cap.value}

    def read(self, first=0, count=None):
        """(t[count], stats[count, 2, 4], probes[count, n_probes, 2]): min, max, sum, sum of squares per field.  Synchronises."""
        if count is None:
            count = self.count() - first
        t, stats, probes = np.empty(count), np.empty((count, 2, 4)), np.empty((count, self.n_probes, 2))
        self._check(lib().crd_recorder_read(self._alive(), first, count, t.ctypes.data, stats.ctypes.data, probes.ctypes.data), "crd_recorder_read")
        return t, stats, probes

    def section_info(self, section):
        kind, index, length, additions = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self._check(lib().crd_recorder_section_info(self._alive(), int(section), C.byref(kind), C.byref(index), C.byref(length), C.byref(additions)), "crd_recorder_section_info")
        return {"kind": kind.value, "index": index.value, "length": length.value, "additions": additions.value}

    def section(self, section, first=0, count=None):
        """The recorded lines of section `section`, [sample, length, 2] (default: every sample).  Synchronises; one copy."""
        length = self.section_info(section)["length"]
        if count is None:
            count = self.count() - first
        v = np.empty((count, length, 2))
        self._check(lib().crd_recorder_read_section(self._alive(), int(section), first, count, v.ctypes.data), "crd_recorder_read_section")
        return v

    def maps(self):
        """(min, max, activation time) of var0 over the samples so far, whole-grid [ny, nx] planes gathered from the slabs."""
        out = [np.empty((self.grid.ny, self.grid.nx)) for _ in range(3)]
        self._check(lib().crd_recorder_maps(self._alive(), *[a.ctypes.data for a in out]), "crd_recorder_maps")
        return tuple(out)

    def cycles(self):
        """(count, t_first, t_last) of the upward crossings of cycle_threshold, whole-grid [ny, nx] planes."""
        count = np.empty((self.grid.ny, self.grid.nx), dtype=np.int32)
        t_first, t_last = np.empty((self.grid.ny, self.grid.nx)), np.empty((self.grid.ny, self.grid.nx))
        self._check(lib().crd_recorder_cycles(self._alive(), count.ctypes.data, t_first.ctypes.data, t_last.ctypes.data), "crd_recorder_cycles")
        return count, t_first, t_last
