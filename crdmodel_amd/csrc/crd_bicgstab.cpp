// crd_bicgstab.cpp -- entry points of the BiCGStab solve (crd_bicgstab_*, include/crd.h).  This file owns the workspace kept on the
// context and the order of launches -- J v (crd_jtimes_device), the multigrid cycle (crd_psolve_device), the fused kernels of
// crd_bicgstab.hip -- and reads the reductions of each; what the scalars mean for the iteration is crd_bicgstab_host.h's.  Host code only.
#include <cmath>
#include <cstring>

#include "crd_bicgstab.h"
#include "crd_bicgstab_host.h"
#include "crd_ctx.h"
#include "crd_krylov.h"

namespace crd {

// Eight vectors, the reductions' partials and a page-locked block the sums land in: one allocation (and the block), made by the first
// crd_bicgstab_* call, freed by crd_destroy.  Never the workspace of crd_lsolve_*.
struct BicgstabWorkspace {
	void *base = nullptr;
	void *res = nullptr, *rhat = nullptr, *p = nullptr, *v = nullptr, *s = nullptr, *t = nullptr, *phat = nullptr, *shat = nullptr;
	double *partials = nullptr;
	double *host = nullptr;  // page-locked, device-visible: the sums of the launch at hand
};

void bicgstab_release(crd_ctx *c)
{
	if (!c || !c->bicgstab) return;
	if (c->bicgstab->base) (void)hipFree(c->bicgstab->base);
	if (c->bicgstab->host) (void)hipHostFree(c->bicgstab->host);
	delete c->bicgstab;
	c->bicgstab = nullptr;
}

}  // namespace crd

using namespace crd;

namespace {

constexpr size_t kAlign = 256;
constexpr int kVectors = 8;
size_t aligned(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }
size_t vector_reals(const crd_ctx *c) { return 2 * (size_t)c->nx * (size_t)c->nyl; }
size_t vector_bytes(const crd_ctx *c) { return vector_reals(c) * c->real_size; }
size_t workspace_bytes(const crd_ctx *c) { return kVectors * aligned(vector_bytes(c)) + aligned((size_t)kBcgSlots * kBcgBlocks * sizeof(double)); }

int ensure_workspace(crd_ctx *c)
{
	if (c->bicgstab) return CRD_OK;
	void *base = nullptr;
	hipError_t e = hipMalloc(&base, workspace_bytes(c));
	if (e != hipSuccess) {
		(void)hipGetLastError();
		return fail(c, e == hipErrorOutOfMemory ? CRD_ENOMEM : CRD_EHIP, std::string("hipMalloc(bicgstab workspace): ") + hipGetErrorString(e));
	}
	double *host = nullptr;
	e = hipHostMalloc((void **)&host, 8 * sizeof(double), hipHostMallocPortable | hipHostMallocMapped);
	if (e != hipSuccess) {  // nothing is kept on the context: the next call starts over
		(void)hipGetLastError();
		(void)hipFree(base);
		return fail(c, CRD_EHIP, std::string("hipHostMalloc(bicgstab scalars): ") + hipGetErrorString(e));
	}
	BicgstabWorkspace *w = new BicgstabWorkspace;
	w->base = base;
	w->host = host;
	char *at = static_cast<char *>(base);
	const size_t vec = aligned(vector_bytes(c));
	for (void **q : {&w->res, &w->rhat, &w->p, &w->v, &w->s, &w->t, &w->phat, &w->shat}) {
		*q = at;
		at += vec;
	}
	w->partials = reinterpret_cast<double *>(at);
	c->bicgstab = w;  // complete, and only now the context's
	return CRD_OK;
}

int check_ctx(crd_ctx *c)
{
	if (c->d0 > 1) return fail(c, CRD_ESTATE, "theta-blocks have no linear solve");
	if (c->n_slabs > 1) return fail(c, CRD_ESTATE, "crd_bicgstab works on a context that holds the whole grid: its preconditioner and its reductions do not span slabs");
	return CRD_OK;
}

int check_options(crd_ctx *c, const crd_bicgstab_options *opt, crd_bicgstab_options *o)
{
	if (opt) *o = *opt;
	else (void)crd_bicgstab_defaults(o);
	if (o->part != CRD_PART_DIFFUSION && o->part != CRD_PART_FULL) return fail(c, CRD_EINVAL, "bicgstab: part must be CRD_PART_DIFFUSION or CRD_PART_FULL");
	if (o->precondition != 0 && o->precondition != 1) return fail(c, CRD_EINVAL, "bicgstab: precondition must be 0 or 1");
	if (o->max_iters < 1) return fail(c, CRD_EINVAL, "bicgstab: max_iters must be at least 1");
	if (o->guess != 0 && o->guess != 1) return fail(c, CRD_EINVAL, "bicgstab: guess must be 0 or 1");
	if (!std::isfinite(o->rtol) || o->rtol < 0.0 || !std::isfinite(o->atol) || o->atol < 0.0) return fail(c, CRD_EINVAL, "bicgstab: rtol and atol must be finite and not negative");
	if (int rc = check_ctx(c)) return rc;
	if (int rc = crd_psolve_info(c, &o->psolve, nullptr, nullptr, nullptr, nullptr)) {
		const std::string why = c->err;
		return fail(c, rc, "bicgstab: " + why);
	}
	return CRD_OK;
}

int check_call(crd_ctx *c, double gamma, const crd_bicgstab_options *opt, const void *y, const void *r, const void *z, crd_bicgstab_options *o)
{
	if (!c) return fail(nullptr, CRD_EINVAL, "bicgstab: no context");
	if (!r || !z) return fail(c, CRD_EINVAL, "bicgstab: r and z must not be null");
	if (!std::isfinite(gamma) || gamma < 0.0) return fail(c, CRD_EINVAL, "bicgstab: gamma must be finite and not negative");
	if (int rc = check_options(c, opt, o)) return rc;
	if (z == r || z == y) return fail(c, CRD_EINVAL, "bicgstab: z must not be r or y (both are read after z is written)");
	if (!y && o->part == CRD_PART_FULL) return fail(c, CRD_EINVAL, "bicgstab: CRD_PART_FULL needs y");
	return CRD_OK;
}

// One solve's state and its launches on the compute stream.
struct Solve {
	crd_ctx *c;
	const crd_bicgstab_options &o;
	double t, gamma;
	const void *y, *r;
	void *z;
	crd_bicgstab_stats st{};
	BicgstabWorkspace *w = nullptr;
	size_t n = 0;
	int precision = 0, var0_only = 0;

	// waits for everything launched so far: the sums of the last reducing launch are in w->host
	int wait() { HIP_TRY(c, hipStreamSynchronize(c->compute)); return CRD_OK; }

	// out = J x
	int jtimes(const void *x, void *out)
	{
		if (int rc = crd_jtimes_device(c, t, o.part, y ? y : x, x, out)) return rc;
		st.matvecs++;
		return CRD_OK;
	}

	// *out = M x (the cycle into `store`), or x itself without a preconditioner
	int precondition(const void *x, void *store, const void **out)
	{
		if (!o.precondition) {
			*out = x;
			return CRD_OK;
		}
		if (int rc = crd_psolve_device(c, t, gamma, &o.psolve, x, store)) return rc;
		st.psolves++;
		*out = store;
		return CRD_OK;
	}

	int finish_trivial(bool copy_r)
	{
		if (copy_r) HIP_TRY(c, hipMemcpyAsync(z, r, vector_bytes(c), hipMemcpyDeviceToDevice, c->compute));
		else {
			HIP_TRY(c, hipMemsetAsync(z, 0, vector_bytes(c), c->compute));
			if (var0_only) HIP_TRY(c, launch_kr_add(precision, z, nullptr, r, n, c->compute));
		}
		st.converged = 1;
		return wait();
	}

	// z_var1 = r_var1 (the diffusion part), then ||r - A z|| through one more matvec
	int finish()
	{
		if (var0_only) HIP_TRY(c, launch_kr_add(precision, z, nullptr, r, n, c->compute));
		if (int rc = jtimes(z, w->v)) return rc;
		HIP_TRY(c, launch_bcg_start(precision, r, z, w->v, gamma, var0_only, w->t, nullptr, nullptr, n, w->partials, w->host, c->compute));
		if (int rc = wait()) return rc;
		st.true_res_norm = std::sqrt(w->host[1]);
		return CRD_OK;
	}

	int run()
	{
		precision = c->p.precision;
		n = vector_reals(c);
		var0_only = o.part == CRD_PART_DIFFUSION;
		if (int rc = set_device(c)) return rc;
		if (int rc = ensure_workspace(c)) return rc;
		w = c->bicgstab;
		const bool warm = o.guess == 1 && gamma != 0.0;
		if (warm) {
			if (int rc = jtimes(z, w->v)) return rc;
		} else if (gamma != 0.0) {
			HIP_TRY(c, hipMemsetAsync(z, 0, vector_bytes(c), c->compute));
		}
		// res = rhat = p = the first residual, ||r||^2 and ||res||^2 from the same pass
		HIP_TRY(c, launch_bcg_start(precision, r, warm ? z : nullptr, warm ? w->v : nullptr, gamma, var0_only, w->res, w->rhat, w->p, n, w->partials, w->host, c->compute));
		if (int rc = wait()) return rc;
		st.r_norm = std::sqrt(w->host[0]);
		const double res_sq = w->host[1];
		st.res_norm = st.true_res_norm = std::sqrt(res_sq);
		if (gamma == 0.0) {  // A = I
			st.res_norm = st.true_res_norm = 0.0;
			return finish_trivial(true);
		}
		if (st.r_norm == 0.0) {
			st.res_norm = st.true_res_norm = 0.0;
			return finish_trivial(false);
		}
		if (!std::isfinite(st.r_norm)) {  // nothing to iterate on: z is the start (var1 as everywhere)
			if (var0_only) HIP_TRY(c, launch_kr_add(precision, z, nullptr, r, n, c->compute));
			return wait();
		}
		bicgstab::Recurrence k;
		k.f32 = precision != CRD_PRECISION_F64;
		k.tol = o.rtol * st.r_norm + o.atol;
		k.max_iters = o.max_iters;
		bool go = k.start(res_sq);
		while (go) {
			const void *phat = nullptr, *shat = nullptr;
			if (int rc = precondition(w->p, w->phat, &phat)) return rc;
			if (int rc = jtimes(phat, w->v)) return rc;
			HIP_TRY(c, launch_bcg_apply_dot(precision, w->v, phat, w->rhat, gamma, var0_only, 0, n, w->partials, w->host, c->compute));
			if (int rc = wait()) return rc;
			if (!k.take_d(w->host[0])) break;
			HIP_TRY(c, launch_bcg_s_update(precision, w->s, w->v, w->res, k.alpha, n, w->partials, w->host, c->compute));
			if (int rc = wait()) return rc;
			if (!k.take_s(w->host[0])) {
				HIP_TRY(c, launch_bcg_x_half(precision, z, phat, k.alpha, n, c->compute));
				break;
			}
			if (int rc = precondition(w->s, w->shat, &shat)) return rc;
			if (int rc = jtimes(shat, w->t)) return rc;
			HIP_TRY(c, launch_bcg_apply_dot(precision, w->t, shat, w->s, gamma, var0_only, 1, n, w->partials, w->host, c->compute));
			if (int rc = wait()) return rc;
			if (!k.take_t(w->host[0], w->host[1])) {
				HIP_TRY(c, launch_bcg_x_half(precision, z, phat, k.alpha, n, c->compute));  // s is the residual of this x
				break;
			}
			HIP_TRY(c, launch_bcg_xr_update(precision, z, phat, shat, w->t, w->s, w->rhat, w->res, k.alpha, k.omega, n, w->partials, w->host, c->compute));
			if (int rc = wait()) return rc;
			go = k.take_res(w->host[0], w->host[1]);
			if (go) HIP_TRY(c, launch_bcg_p_update(precision, w->p, w->v, w->res, k.beta, k.omega, n, c->compute));
		}
		st.converged = k.converged;
		st.iterations = k.iterations;
		st.half_exit = k.half_exit;
		st.breakdown = k.breakdown;
		st.res_norm = k.res_norm;
		return finish();
	}
};

int solve_device(crd_ctx *c, double t, double gamma, const crd_bicgstab_options &o, const void *y, const void *r, void *z, crd_bicgstab_stats *stats)
{
	Solve s{c, o, t, gamma, o.part == CRD_PART_FULL ? y : nullptr, r, z};
	const int rc = s.run();
	if (stats) *stats = s.st;
	return rc;
}

// the direction buffer of crd_jtimes_host serves as the staging of y
int stage_y(crd_ctx *c, const void *y)
{
	if (c->stage_v_bytes < vector_bytes(c)) {
		if (c->stage_v) (void)hipFree(c->stage_v);
		c->stage_v = nullptr;
		c->stage_v_bytes = 0;
		HIP_TRY(c, hipMalloc(&c->stage_v, vector_bytes(c)));
		c->stage_v_bytes = vector_bytes(c);
	}
	HIP_TRY(c, hipMemcpyAsync(c->stage_v, y, vector_bytes(c), hipMemcpyHostToDevice, c->compute));
	return CRD_OK;
}

}  // namespace

extern "C" {

int crd_bicgstab_defaults(crd_bicgstab_options *opt)
{
	if (!opt) return CRD_EINVAL;
	opt->part = CRD_PART_DIFFUSION;
	opt->precondition = 1;
	opt->max_iters = 200;
	opt->guess = 0;
	opt->rtol = 1e-8;
	opt->atol = 0.0;
	return crd_psolve_defaults(&opt->psolve);
}

int crd_bicgstab_info(crd_ctx *c, const crd_bicgstab_options *opt, int64_t *bytes)
{
	if (!c) return fail(nullptr, CRD_EINVAL, "bicgstab: no context");
	crd_bicgstab_options o;
	if (int rc = check_options(c, opt, &o)) return rc;
	if (bytes) *bytes = (int64_t)workspace_bytes(c);
	return CRD_OK;
}

int crd_bicgstab_device(crd_ctx *c, double t, double gamma, const crd_bicgstab_options *opt, const void *y, const void *r, void *z, crd_bicgstab_stats *stats)
{
	crd_bicgstab_options o;
	if (int rc = check_call(c, gamma, opt, y, r, z, &o)) return rc;
	return solve_device(c, t, gamma, o, y, r, z, stats);
}

int crd_bicgstab_host(crd_ctx *c, double t, double gamma, const crd_bicgstab_options *opt, const void *y, const void *r, void *z, crd_bicgstab_stats *stats)
{
	crd_bicgstab_options o;
	if (int rc = check_call(c, gamma, opt, y, r, z, &o)) return rc;
	if (int rc = set_device(c)) return rc;
	if (int rc = ensure_staging(c, 2 * (size_t)c->nx * (size_t)c->nyl * 8)) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->stage_in, r, vector_bytes(c), hipMemcpyHostToDevice, c->compute));
	if (o.guess) HIP_TRY(c, hipMemcpyAsync(c->stage_out, z, vector_bytes(c), hipMemcpyHostToDevice, c->compute));
	const bool with_y = y && o.part == CRD_PART_FULL;
	if (with_y)
		if (int rc = stage_y(c, y)) return rc;
	if (int rc = solve_device(c, t, gamma, o, with_y ? c->stage_v : nullptr, c->stage_in, c->stage_out, stats)) return rc;
	HIP_TRY(c, hipMemcpyAsync(z, c->stage_out, vector_bytes(c), hipMemcpyDeviceToHost, c->compute));
	HIP_TRY(c, hipStreamSynchronize(c->compute));
	return CRD_OK;
}

int crd_bicgstab_probe(crd_ctx *c, int kernel, int var0_only, const double *scalars, const void *in, void *out, double *sums)
{
	if (!c) return fail(nullptr, CRD_EINVAL, "bicgstab_probe: no context");
	if (kernel < CRD_BICGSTAB_KERNEL_APPLY_DOT || kernel > CRD_BICGSTAB_KERNEL_X_HALF) return fail(c, CRD_EINVAL, "bicgstab_probe: kernel must be a CRD_BICGSTAB_KERNEL_* value");
	if (!scalars || !in || !out || (var0_only != 0 && var0_only != 1)) return fail(c, CRD_EINVAL, "bicgstab_probe: no pointer null besides sums, var0_only 0 or 1");
	if (int rc = check_ctx(c)) return rc;
	if (int rc = set_device(c)) return rc;
	if (int rc = ensure_workspace(c)) return rc;
	BicgstabWorkspace *w = c->bicgstab;
	const int precision = c->p.precision;
	const bool f32 = precision != CRD_PRECISION_F64;
	const size_t vb = vector_bytes(c), n = vector_reals(c);
	void *slot[7] = {w->res, w->rhat, w->p, w->v, w->s, w->t, w->phat};
	static const int n_in[6] = {3, 3, 2, 6, 3, 2}, n_out[6] = {1, 1, 1, 2, 1, 1}, n_sums[6] = {1, 2, 1, 2, 0, 0};
	for (int i = 0; i < n_in[kernel]; i++) HIP_TRY(c, hipMemcpyAsync(slot[i], static_cast<const char *>(in) + (size_t)i * vb, vb, hipMemcpyHostToDevice, c->compute));
	const double a = bicgstab::rounded(scalars[0], f32), b = n_in[kernel] == 6 || kernel == CRD_BICGSTAB_KERNEL_P_UPDATE ? bicgstab::rounded(scalars[1], f32) : 0.0;
	w->host[0] = w->host[1] = 0.0;
	void *result[2] = {slot[0], nullptr};
	switch (kernel) {
	case CRD_BICGSTAB_KERNEL_APPLY_DOT:
	case CRD_BICGSTAB_KERNEL_APPLY_DOT2:
		HIP_TRY(c, launch_bcg_apply_dot(precision, slot[0], slot[1], slot[2], a, var0_only, kernel == CRD_BICGSTAB_KERNEL_APPLY_DOT2, n, w->partials, w->host, c->compute));
		break;
	case CRD_BICGSTAB_KERNEL_S_UPDATE:
		HIP_TRY(c, launch_bcg_s_update(precision, slot[6], slot[0], slot[1], a, n, w->partials, w->host, c->compute));
		result[0] = slot[6];
		break;
	case CRD_BICGSTAB_KERNEL_XR_UPDATE:
		HIP_TRY(c, launch_bcg_xr_update(precision, slot[0], slot[1], slot[2], slot[3], slot[4], slot[5], slot[6], a, b, n, w->partials, w->host, c->compute));
		result[1] = slot[6];
		break;
	case CRD_BICGSTAB_KERNEL_P_UPDATE:
		HIP_TRY(c, launch_bcg_p_update(precision, slot[0], slot[1], slot[2], a, b, n, c->compute));
		break;
	default:
		HIP_TRY(c, launch_bcg_x_half(precision, slot[0], slot[1], a, n, c->compute));
		break;
	}
	for (int i = 0; i < n_out[kernel]; i++) HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(out) + (size_t)i * vb, result[i], vb, hipMemcpyDeviceToHost, c->compute));
	HIP_TRY(c, hipStreamSynchronize(c->compute));
	for (int i = 0; sums && i < n_sums[kernel]; i++) sums[i] = w->host[i];
	return CRD_OK;
}

}  // extern "C"
