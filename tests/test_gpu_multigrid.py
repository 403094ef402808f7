"""The preconditioner solve on the device (crd_psolve_* / Slab.psolve): one multigrid V-cycle for (I - gamma J_D(t)) z = r.

Every cycle is held per point to the rounding bound of tests/multigrid_reference.py against the long-double reference (fp32: float64 on
the widened vector); the identities the header promises are held bit for bit; as the preconditioner of scipy's GMRES with the device's
own J_D v it needs no more iterations than the reference cycle does and at most a quarter of the unpreconditioned count; the ARKode
shim's callback gives the device entry point's bits; and what the entry points refuse, they refuse with a message.

Worst err / bound measured on MI355X (printed with -s as "BOUND ..."): see DESIGN.md section 2.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import crdmodel_amd as crd
import jacobian_reference as jr
import multigrid_reference as mg
from conftest import GOLDEN
from oracle import error_bounds as eb

pytestmark = pytest.mark.gpu

CONFIG_IDS = [c[0] for c in jr.CONFIGS]
T_ON, T_AT, T_OFF = jr.TIMES  # rows held; at tBoundary (strict <: free); free
K = crd._capi


def right_hand_side(p, seed=3):
    g = crd.grid_of(p)
    r = np.random.default_rng(seed).standard_normal((g.ny, g.nx, 2))
    return r.astype(np.float32) if p.precision == K.PRECISION_F32 else r


@functools.lru_cache(maxsize=None)
def bounded(config_index, nx, ny, precision, t, multiple, opts):
    """(ref, bound_u, bound_v) of one case, computed once and shared by the tests that need it; gamma = multiple x crd.stable_dt."""
    p, op = jr.case(jr.CONFIGS[config_index], nx, ny, precision)
    return mg.vcycle_bound(op, t, multiple * crd.stable_dt(p), right_hand_side(p), precision, **dict(opts))


class Device:
    """The *_device entry points on device memory of the process's own HIP runtime (the one libcrd is bound to): one input and one
    output vector of the slab's size, written by up(), read by down().  Not torch tensors: by the time this file runs the suite's ring
    tests have made libcrd load the system's RCCL globally, and torch imported after that resolves its own bundled libraries of the
    same SONAME against it -- a mixed set in one process (the pytest process then ended in a double free at exit)."""

    H2D, D2H = 1, 2  # hipMemcpyHostToDevice, hipMemcpyDeviceToHost

    def __init__(self, slab):
        self.slab, self.L = slab, K.lib()
        self.hip = C.CDLL(None)  # libcrd.so is loaded RTLD_GLOBAL: its HIP runtime's symbols are the process's
        self.hip.hipMalloc.argtypes, self.hip.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
        self.hip.hipFree.argtypes, self.hip.hipFree.restype = [C.c_void_p], C.c_int
        self.hip.hipMemcpy.argtypes, self.hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
        self.shape = (slab.nyl, slab.nx, 2)
        self.nbytes = int(np.prod(self.shape)) * np.dtype(slab.dtype).itemsize
        self.vin, self.vout = C.c_void_p(), C.c_void_p()
        for v in (self.vin, self.vout):
            assert self.hip.hipMalloc(C.byref(v), self.nbytes) == 0 and v.value

    def close(self):
        self.slab.synchronize()
        for v in (self.vin, self.vout):
            if v.value:
                assert self.hip.hipFree(v) == 0
                v.value = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def up(self, x):
        x = np.ascontiguousarray(x, dtype=self.slab.dtype)
        assert x.shape == self.shape
        self.slab.synchronize()  # nothing still reads the input vector
        assert self.hip.hipMemcpy(self.vin, x.ctypes.data, self.nbytes, self.H2D) == 0
        return self.vin

    def down(self, v):
        out = np.empty(self.shape, dtype=self.slab.dtype)
        self.slab.synchronize()
        assert self.hip.hipMemcpy(out.ctypes.data, v, self.nbytes, self.D2H) == 0
        return out

    def psolve(self, t, gamma, r, **opts):
        opt = crd.Slab._psolve_options(**mg.options(**opts))
        self.slab._check(self.L.crd_psolve_device(self.slab.handle, t, gamma, C.byref(opt), r, self.vout), "crd_psolve_device")
        return self.vout

    def jtimes_diffusion(self, t, v):
        self.slab._check(self.L.crd_jtimes_device(self.slab.handle, t, K.PART_DIFFUSION, v, v, self.vout), "crd_jtimes_device")
        return self.vout


# ---- the per-point gate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config_index", range(len(jr.CONFIGS)), ids=CONFIG_IDS)
def test_cycle_within_the_bound(gpu_device, config_index, precision):
    config, worst = jr.CONFIGS[config_index], 0.0
    for nx, ny in mg.GRIDS:
        p, op = jr.case(config, nx, ny, precision)
        r = right_hand_side(p)
        with crd.Slab(p) as slab:
            for opts in mg.OPTION_SETS:
                levels, shapes, nbytes = slab.psolve_info(**opts)
                assert shapes == mg.level_shapes(nx, ny, mg.options(**opts)["max_levels"]) and levels == len(shapes)
                planes = sum(3 * a * b for a, b in mg.level_shapes(nx, ny)) * r.itemsize
                assert planes <= nbytes <= planes + 6 * 256 * len(mg.level_shapes(nx, ny)) + 3 * 2 * nx * r.itemsize
            for t in jr.TIMES:
                for multiple in mg.GAMMAS:
                    for opts in mg.OPTION_SETS:
                        case = "psolve %s %s %dx%d t=%g gamma=%gx %s" % (precision, config[0], nx, ny, t, multiple, opts or "defaults")
                        z = slab.psolve(t, multiple * crd.stable_dt(p), r, **opts)
                        w = eb.check(case, z, bounded(config_index, nx, ny, precision, t, multiple, tuple(sorted(opts.items()))))
                        print("BOUND " + eb.describe(case, w))
                        worst = max(worst, w["u"][0])
    print("BOUND WORST %s %s: psolve %.3g" % (precision, config[0], worst))


# ---- bit identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("config_index", [0, 1, 3], ids=[CONFIG_IDS[k] for k in (0, 1, 3)])
def test_bit_identities(gpu_device, config_index, precision):
    config = jr.CONFIGS[config_index]
    R = np.float64 if precision == "f64" else np.float32
    for nx, ny in [(48, 40), (136, 72), (130, 33), (64, 16)]:
        p, op = jr.case(config, nx, ny, precision)
        r = right_hand_side(p)
        with crd.Slab(p) as slab, Device(slab) as dev:
            r_dev = dev.up(r)
            for t in (T_ON, T_OFF):
                for multiple in mg.GAMMAS:
                    gamma, case = multiple * crd.stable_dt(p), (config[0], precision, nx, ny, t, multiple)
                    z = slab.psolve(t, gamma, r)
                    assert np.array_equal(z[..., 1], r[..., 1]), case  # var1 is r's
                    assert np.array_equal(slab.psolve(t, gamma, r), z), case  # the same bits from run to run
                    assert np.array_equal(dev.down(dev.psolve(t, gamma, r_dev)), z), case  # _host is _device
                    assert np.array_equal(slab.psolve(t, gamma, R(4.0) * r), R(4.0) * z), case  # a fixed linear map: powers of two commute with every rounding
                    assert np.array_equal(slab.psolve(t, 0.0, r), r), case  # gamma = 0: P = I
                    # one level: `coarse` sweeps (here coarse = pre + post) of the kernel-order restatement's single level, within the bound
                    one = dict(pre=2, post=2, coarse=4, max_levels=1)
                    z1 = slab.psolve(t, gamma, r, **one)
                    ref, bound, _ = mg.vcycle_bound(op, t, gamma, r, precision, **one)
                    eb.check("one level %r" % (case,), z1, (ref, bound, np.zeros_like(bound)))
                    restated = mg.kernel_order_vcycle(op, t, gamma, r, R, **one)
                    assert np.all(np.abs(z1[..., 0].astype(ref.dtype) - restated[..., 0]) <= bound), case
                    assert np.array_equal(slab.psolve_info(**one)[1], [(nx, ny)])


def test_options_without_a_pre_or_a_post_sweep(gpu_device):
    """pre = 0 (the residual of z = 0 is r, read from the caller's vector) and post = 0 (the prolongation writes the caller's vector)
    take launch paths of their own: both inside the bound."""
    for precision in ("f64", "f32"):
        for nx, ny in [(48, 40), (136, 72)]:
            p, op = jr.case(jr.CONFIGS[0], nx, ny, precision)
            r = right_hand_side(p)
            with crd.Slab(p) as slab:
                for t in (T_ON, T_OFF):
                    for opts in (dict(pre=0, post=2), dict(pre=2, post=0), dict(pre=0, post=1, coarse=1), dict(pre=1, post=0, max_levels=2)):
                        gamma = 20.0 * crd.stable_dt(p)
                        z = slab.psolve(t, gamma, r, **opts)
                        eb.check("psolve %s %dx%d t=%g %s" % (precision, nx, ny, t, opts), z, mg.vcycle_bound(op, t, gamma, r, precision, **opts))


# ---- what it is for ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,held,multiple", [(32, 128, True, 500.0), (48, 192, False, 2000.0)], ids=["32x128-held-500x", "48x192-free-2000x"])
def test_gmres_with_the_device_preconditioner(gpu_device, nx, ny, held, multiple):
    """(I - gamma J_D) z = r on the FHN torus in scipy gmres (rtol 1e-10), matvec from crd_jtimes_device(CRD_PART_DIFFUSION), M from
    crd_psolve_device: no more iterations than with the reference cycle as M on the reference operator (+ 2: rounding can move a
    count by one or two), at most a quarter of the device's own unpreconditioned count, and the residual under the long-double operator
    within the solver's tolerance plus the rounding of what it was given (test_gpu_jacobian.test_linearly_implicit_euler_step's
    allowance: per point gamma x the bound on J_D z + 2 u (|z| + gamma |J_D z|))."""
    p, op = jr.case(jr.CONFIGS[0], nx, ny, "f64")
    t = T_ON if held else T_OFF
    gamma, rtol, u = multiple * crd.stable_dt(p), 1e-10, eb.UNIT["f64"]
    b = right_hand_side(p, seed=5)
    shape = b.shape
    y_any = np.zeros(shape)
    with crd.Slab(p) as slab, Device(slab) as dev:

        def matvec(x):
            v = dev.up(x.reshape(shape))
            return x - gamma * dev.down(dev.jtimes_diffusion(t, v)).ravel()

        def precondition(x):
            return dev.down(dev.psolve(t, gamma, dev.up(x.reshape(shape)))).ravel()

        z, with_m = mg.gmres_iterations(matvec, b.ravel(), precondition, rtol=rtol)
        _, plain = mg.gmres_iterations(matvec, b.ravel(), rtol=rtol)

    def ref_matvec(x):
        x = x.reshape(shape)
        return np.stack([mg.operator(op, t, gamma, x[..., 0]), x[..., 1]], axis=-1).ravel()

    def ref_precondition(x):
        x = x.reshape(shape)
        return np.stack([mg.reference_vcycle(op, t, gamma, x[..., 0]), x[..., 1]], axis=-1).ravel()

    _, with_ref = mg.gmres_iterations(ref_matvec, b.ravel(), ref_precondition, rtol=rtol)
    print("GMRES %dx%d %s %gx: %d iterations with crd_psolve_device, %d with the reference cycle, %d without" % (nx, ny, "held" if held else "free", multiple, with_m, with_ref, plain))
    assert with_m <= with_ref + 2, (with_m, with_ref)
    assert 4 * with_m <= plain, (with_m, plain)
    z = z.reshape(shape)
    jd, jbu, jbv = jr.jtimes_bound(op, t, y_any, z, "f64", jr.DIFFUSION)
    L = np.longdouble
    residual = (z.astype(L) - L(gamma) * jd) - b.astype(L)
    rounding = gamma * np.stack([jbu, jbv], -1) + 2 * u * (np.abs(z) + gamma * np.abs(jd.astype(np.float64)))
    res, allowed = float(np.linalg.norm(residual.astype(np.float64))), rtol * float(np.linalg.norm(b)) + float(np.linalg.norm(rounding))
    print("BOUND gmres residual %.3g, allowed %.3g" % (res, allowed))
    assert res <= allowed


# ---- the shim ---------------------------------------------------------------------------------------------------------------------
def test_psolve_shim(gpu_device, tmp_path):
    """tests/native/shim_psolve_selftest.c drives crd_arkode_psolve on host vectors through a SUNDIALS-typed function pointer (there: the
    bits of crd_psolve_host with either lr); here its z has the bits of crd_psolve_device on the same r."""
    exe, dump = tmp_path / "shim_psolve", tmp_path / "psolve.bin"
    ini = os.path.join(GOLDEN, "ini", "small_run.ini")
    build = subprocess.run(mg.shim_build_command(exe), capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    r = subprocess.run([str(exe), ini, str(dump)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "shim psolve selftest" in r.stdout, (r.returncode, r.stdout, r.stderr)
    nx, ny, t_boundary, gamma = 16, 40, 0.4, 0.0625  # tests/golden/ini/small_run.ini; SELFTEST_GAMMA
    data = np.fromfile(dump, dtype=np.float64).reshape(2, 2, ny, nx, 2)
    p = crd.load_ini(ini, "fhn", "torus").params
    op = jr.problem_of("fhn", "torus", nx, ny, 1.25, t_boundary=t_boundary)
    with crd.Slab(p) as slab, Device(slab) as dev:
        for k, t in enumerate((0.5 * t_boundary, 2.0 * t_boundary + 1.0)):
            rhs, z = data[k]
            assert np.array_equal(dev.down(dev.psolve(t, gamma, dev.up(rhs))), z), t
            eb.check("shim psolve t=%g" % t, z, mg.vcycle_bound(op, t, gamma, rhs, "f64"))
            if t < t_boundary:
                assert np.array_equal(z[[0, ny - 1]], rhs[[0, ny - 1]])  # held rows: z = r


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_device):
    """Each CRD_EINVAL of the header, a member of a two-slab LOCAL group and a theta-block context (CRD_ESTATE), each with a message."""
    p, op = jr.case(jr.CONFIGS[0], 48, 40, "f64")
    r = right_hand_side(p)
    L = K.lib()

    def refused(call, status):
        with pytest.raises(K.CrdError) as e:
            call()
        assert e.value.status == status, e.value
        return str(e.value)

    with crd.Slab(p) as slab:
        bad = [dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(pre=0, post=0), dict(pre=-1, post=2), dict(coarse=0), dict(max_levels=0),
               dict(max_levels=17), dict(omega=0.0), dict(omega=1.5), dict(omega=float("nan"))]
        for kw in bad:
            gamma = kw.pop("gamma", 1.0)
            refused(lambda: slab.psolve(0.0, gamma, r, **kw), K.EINVAL)
            assert "psolve" in L.crd_last_error(slab.handle).decode(), kw
        refused(lambda: slab.psolve_info(max_levels=0), K.EINVAL)
        same = np.ascontiguousarray(r)
        rc = L.crd_psolve_host(slab.handle, 0.0, 1.0, None, same.ctypes.data, same.ctypes.data)  # z == r
        assert rc == K.EINVAL and "z must not be r" in L.crd_last_error(slab.handle).decode()
        assert L.crd_psolve_device(slab.handle, 0.0, 1.0, None, same.ctypes.data, same.ctypes.data) == K.EINVAL
        assert np.array_equal(slab.psolve(0.0, 1.0, r, omega=1.0)[..., 1], r[..., 1])  # the ends of the ranges are inside
    with crd.LocalGroup(p, 2) as group:
        s = group.slabs[1]
        msg = refused(lambda: s.psolve(0.0, 1.0, r[s.js:s.je + 1]), K.ESTATE)
        assert "whole grid" in msg
        refused(lambda: s.psolve_info(), K.ESTATE)
    with crd.LocalGroup(p, 4, blocks=(2, 2)) as blocks:
        s = blocks.slabs[0]
        msg = refused(lambda: s.psolve(0.0, 1.0, r[s.js:s.je + 1, s.is_:s.ie + 1]), K.ESTATE)
        assert "theta-blocks" in msg
