// crd_krylov.cpp -- entry points of the linear solve (crd_lsolve_*, include/crd.h): restarted, right-preconditioned GMRES whose
// vectors stay on the device.  This file owns the workspace kept on the context and the order of launches -- J v (crd_jtimes_device),
// the multigrid cycle (crd_psolve_device), the kernels of crd_krylov.hip -- and reads one Hessenberg column per inner iteration;
// the small least-squares problem is crd_krylov_host.h's.  Host code only.
#include <cmath>
#include <cstring>

#include "crd_ctx.h"
#include "crd_krylov.h"
#include "crd_krylov_host.h"

namespace crd {

// restart + 1 basis vectors, two work vectors, the reductions' scalars: one allocation, made by the first crd_lsolve_* call, made
// again when a call asks for a longer restart, freed by crd_destroy.
struct LsolveWorkspace {
	int restart = 0;
	void *base = nullptr;
	size_t bytes = 0;
	size_t stride = 0;  // reals from one basis vector to the next
	char *V = nullptr;
	void *work[2] = {nullptr, nullptr};
	double *partials = nullptr, *norm_partials = nullptr, *h_cur = nullptr, *h_col = nullptr, *y = nullptr;
	double *host = nullptr;  // page-locked: [0, 80) the column read back, [80, 160) the coefficients sent up
};

void lsolve_release(crd_ctx *c)
{
	if (!c || !c->lsolve) return;
	if (c->lsolve->base) (void)hipFree(c->lsolve->base);
	if (c->lsolve->host) (void)hipHostFree(c->lsolve->host);
	delete c->lsolve;
	c->lsolve = nullptr;
}

}  // namespace crd

using namespace crd;

namespace {

constexpr size_t kAlign = 256;
constexpr int kHostSlots = 80;
size_t aligned(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }
size_t vector_reals(const crd_ctx *c) { return 2 * (size_t)c->nx * (size_t)c->nyl; }
size_t vector_bytes(const crd_ctx *c) { return vector_reals(c) * c->real_size; }
// doubles: the multi-dot's partials, the norm's, h of the pass at hand, the column (and the norm behind it), the cycle's coefficients
constexpr size_t kScalarDoubles = (size_t)kKrylovMaxBasis * kKrylovBlocks + kKrylovBlocks + 3 * 128;
size_t workspace_bytes(const crd_ctx *c, int restart) { return ((size_t)restart + 3) * aligned(vector_bytes(c)) + aligned(kScalarDoubles * sizeof(double)); }

int ensure_workspace(crd_ctx *c, int restart)
{
	if (c->lsolve && c->lsolve->restart >= restart) return CRD_OK;
	HIP_TRY(c, hipStreamSynchronize(c->compute));
	lsolve_release(c);
	const size_t bytes = workspace_bytes(c, restart), vec = aligned(vector_bytes(c));
	void *base = nullptr;
	hipError_t e = hipMalloc(&base, bytes);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		return fail(c, e == hipErrorOutOfMemory ? CRD_ENOMEM : CRD_EHIP, std::string("hipMalloc(lsolve workspace): ") + hipGetErrorString(e));
	}
	LsolveWorkspace *w = new LsolveWorkspace;
	w->restart = restart;
	w->base = base;
	w->bytes = bytes;
	c->lsolve = w;
	HIP_TRY(c, hipHostMalloc((void **)&w->host, 2 * kHostSlots * sizeof(double), hipHostMallocDefault));
	char *at = static_cast<char *>(base);
	w->stride = vec / c->real_size;
	w->V = at;
	at += ((size_t)restart + 1) * vec;
	w->work[0] = at;
	w->work[1] = at + vec;
	at += 2 * vec;
	w->partials = reinterpret_cast<double *>(at);
	w->norm_partials = w->partials + (size_t)kKrylovMaxBasis * kKrylovBlocks;
	w->h_cur = w->norm_partials + kKrylovBlocks;
	w->h_col = w->h_cur + 128;
	w->y = w->h_col + 128;
	return CRD_OK;
}

int check_ctx(crd_ctx *c)
{
	if (c->d0 > 1) return fail(c, CRD_ESTATE, "theta-blocks have no linear solve");
	if (c->n_slabs > 1) return fail(c, CRD_ESTATE, "crd_lsolve works on a context that holds the whole grid: its preconditioner and its reductions do not span slabs");
	return CRD_OK;
}

int check_options(crd_ctx *c, const crd_lsolve_options *opt, crd_lsolve_options *o)
{
	if (opt) *o = *opt;
	else (void)crd_lsolve_defaults(o);
	if (o->part != CRD_PART_DIFFUSION && o->part != CRD_PART_FULL) return fail(c, CRD_EINVAL, "lsolve: part must be CRD_PART_DIFFUSION or CRD_PART_FULL");
	if (o->precondition != 0 && o->precondition != 1) return fail(c, CRD_EINVAL, "lsolve: precondition must be 0 or 1");
	if (o->restart < 1 || o->restart > krylov::kMaxRestart) return fail(c, CRD_EINVAL, "lsolve: restart must be in 1 .. 64");
	if (o->max_iters < 1) return fail(c, CRD_EINVAL, "lsolve: max_iters must be at least 1");
	if (!std::isfinite(o->rtol) || o->rtol < 0.0 || !std::isfinite(o->atol) || o->atol < 0.0) return fail(c, CRD_EINVAL, "lsolve: rtol and atol must be finite and not negative");
	if (int rc = check_ctx(c)) return rc;
	if (int rc = crd_psolve_info(c, &o->psolve, nullptr, nullptr, nullptr, nullptr)) {
		const std::string why = c->err;
		return fail(c, rc, "lsolve: " + why);
	}
	return CRD_OK;
}

int check_call(crd_ctx *c, double gamma, const crd_lsolve_options *opt, const void *y, const void *r, const void *z, crd_lsolve_options *o)
{
	if (!c) return fail(nullptr, CRD_EINVAL, "lsolve: no context");
	if (!r || !z) return fail(c, CRD_EINVAL, "lsolve: r and z must not be null");
	if (!std::isfinite(gamma) || gamma < 0.0) return fail(c, CRD_EINVAL, "lsolve: gamma must be finite and not negative");
	if (int rc = check_options(c, opt, o)) return rc;
	if (z == r || z == y) return fail(c, CRD_EINVAL, "lsolve: z must not be r or y (both are read after z is written)");
	if (!y && o->part == CRD_PART_FULL) return fail(c, CRD_EINVAL, "lsolve: CRD_PART_FULL needs y");
	return CRD_OK;
}

// One solve's state and its launches on the compute stream.
struct Solve {
	crd_ctx *c;
	const crd_lsolve_options &o;
	double t, gamma;
	const void *y, *r;
	void *z;
	crd_lsolve_stats st{};
	LsolveWorkspace *w = nullptr;
	size_t n = 0;
	int precision = 0, var0_only = 0;

	void *basis(int i) const { return w->V + (size_t)i * w->stride * c->real_size; }

	// `count` doubles from device memory, waiting for everything launched so far
	int read(const double *dev, int count, double *out)
	{
		HIP_TRY(c, hipMemcpyAsync(w->host, dev, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, c->compute));
		HIP_TRY(c, hipStreamSynchronize(c->compute));
		std::memcpy(out, w->host, (size_t)count * sizeof(double));
		return CRD_OK;
	}

	// out = A x = x - gamma J x (or r - A x), through work[1]
	int apply(const void *x, void *out, bool residual)
	{
		if (int rc = crd_jtimes_device(c, t, o.part, y ? y : x, x, w->work[1])) return rc;
		st.matvecs++;
		HIP_TRY(c, launch_kr_apply(precision, out, x, w->work[1], residual ? r : nullptr, gamma, var0_only, n, c->compute));
		return CRD_OK;
	}

	// *out = M x (the cycle), or x itself without a preconditioner
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

	// h_col[slot] = ||v||^2 read back as a norm
	int norm_of(const void *v, double *out)
	{
		HIP_TRY(c, launch_kr_dots(precision, v, w->stride, 1, v, n, w->partials, w->h_cur, nullptr, 0, c->compute));
		double sq = 0.0;
		if (int rc = read(w->h_cur, 1, &sq)) return rc;
		*out = std::sqrt(sq);
		return CRD_OK;
	}

	int finish_trivial(bool copy_r)
	{
		if (copy_r) HIP_TRY(c, hipMemcpyAsync(z, r, vector_bytes(c), hipMemcpyDeviceToDevice, c->compute));
		else {
			HIP_TRY(c, hipMemsetAsync(z, 0, vector_bytes(c), c->compute));
			if (var0_only) HIP_TRY(c, launch_kr_add(precision, z, nullptr, r, n, c->compute));
		}
		HIP_TRY(c, hipStreamSynchronize(c->compute));
		st.converged = 1;
		return CRD_OK;
	}

	int run()
	{
		precision = c->p.precision;
		n = vector_reals(c);
		var0_only = o.part == CRD_PART_DIFFUSION;
		const double unit = precision == CRD_PRECISION_F64 ? 0x1p-53 : 0x1p-24;
		if (int rc = set_device(c)) return rc;
		if (int rc = ensure_workspace(c, o.restart)) return rc;
		w = c->lsolve;
		if (int rc = norm_of(r, &st.r_norm)) return rc;
		if (gamma == 0.0) return finish_trivial(true);  // A = I
		if (st.r_norm == 0.0) return finish_trivial(false);
		const double tol = o.rtol * st.r_norm + o.atol;
		// the first cycle's residual is r itself (on var0 alone for the diffusion part: var1 is solved by z_var1 = r_var1)
		HIP_TRY(c, launch_kr_apply(precision, basis(0), r, nullptr, nullptr, 0.0, var0_only, n, c->compute));
		HIP_TRY(c, hipMemsetAsync(z, 0, vector_bytes(c), c->compute));
		krylov::LeastSquares ls;
		double col[krylov::kMaxRestart + 2], coef[krylov::kMaxRestart];
		for (int cycle = 0; st.iterations < o.max_iters; cycle++) {
			if (cycle > 0) {
				st.restarts++;
				if (int rc = apply(z, basis(0), true)) return rc;
			}
			// beta = ||residual||, V_0 = residual / beta
			HIP_TRY(c, launch_kr_dots(precision, basis(0), w->stride, 1, basis(0), n, w->partials, w->h_cur, w->h_col, 0, c->compute));
			double sq = 0.0;
			if (int rc = read(w->h_col, 1, &sq)) return rc;
			const double beta = std::sqrt(sq);
			st.res_norm = beta;
			if (!(beta > tol)) {  // (also a residual that is not a number: nothing to iterate on)
				st.converged = beta <= tol;
				break;
			}
			HIP_TRY(c, launch_kr_scale(precision, basis(0), basis(0), n, w->h_col, 0, c->compute));
			ls.start(o.restart, beta);
			while (!ls.full() && st.iterations < o.max_iters) {
				const int j = ls.columns();
				const void *u = nullptr;
				if (int rc = precondition(basis(j), w->work[0], &u)) return rc;
				if (int rc = apply(u, basis(j + 1), false)) return rc;
				// Gram-Schmidt twice: the column is the sum of the two coefficient sets, its last entry ||w||^2 until the host takes the root
				for (int pass = 0; pass < 2; pass++) {
					HIP_TRY(c, launch_kr_dots(precision, basis(0), w->stride, j + 1, basis(j + 1), n, w->partials, w->h_cur, w->h_col, pass, c->compute));
					HIP_TRY(c, launch_kr_update(precision, basis(0), w->stride, j + 1, basis(j + 1), n, w->h_cur, w->norm_partials, w->h_col + j + 1, c->compute));
				}
				if (int rc = read(w->h_col, j + 2, col)) return rc;
				col[j + 1] = std::sqrt(col[j + 1]);
				ls.push(col, unit);
				st.iterations++;
				st.res_norm = ls.residual();
				if (ls.breakdown()) st.breakdown = 1;
				if (st.res_norm <= tol) break;
				// the next basis vector, if the cycle goes on (never after a breakdown: the cycle is full then)
				if (!ls.full() && st.iterations < o.max_iters) HIP_TRY(c, launch_kr_scale(precision, basis(j + 1), basis(j + 1), n, w->h_col + j + 1, 0, c->compute));
			}
			// z += M (sum_i y_i V_i): one M for the cycle
			const int k = ls.columns();
			ls.solve(coef);
			std::memcpy(w->host + kHostSlots, coef, (size_t)k * sizeof(double));
			HIP_TRY(c, hipMemcpyAsync(w->y, w->host + kHostSlots, (size_t)k * sizeof(double), hipMemcpyHostToDevice, c->compute));
			HIP_TRY(c, launch_kr_combine(precision, basis(0), w->stride, k, w->y, w->work[0], n, c->compute));
			const void *mx = nullptr;
			if (int rc = precondition(w->work[0], w->work[1], &mx)) return rc;
			HIP_TRY(c, launch_kr_add(precision, z, mx, nullptr, n, c->compute));
			HIP_TRY(c, hipStreamSynchronize(c->compute));  // the coefficients' host buffer is free again
			if (st.res_norm <= tol) {
				st.converged = 1;
				break;
			}
		}
		if (var0_only) HIP_TRY(c, launch_kr_add(precision, z, nullptr, r, n, c->compute));
		HIP_TRY(c, hipStreamSynchronize(c->compute));
		return CRD_OK;
	}
};

int lsolve_device(crd_ctx *c, double t, double gamma, const crd_lsolve_options &o, const void *y, const void *r, void *z, crd_lsolve_stats *stats)
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

int crd_lsolve_defaults(crd_lsolve_options *opt)
{
	if (!opt) return CRD_EINVAL;
	opt->part = CRD_PART_DIFFUSION;
	opt->precondition = 1;
	opt->restart = 30;
	opt->max_iters = 200;
	opt->rtol = 1e-8;
	opt->atol = 0.0;
	return crd_psolve_defaults(&opt->psolve);
}

int crd_lsolve_info(crd_ctx *c, const crd_lsolve_options *opt, int64_t *bytes)
{
	if (!c) return fail(nullptr, CRD_EINVAL, "lsolve: no context");
	crd_lsolve_options o;
	if (int rc = check_options(c, opt, &o)) return rc;
	if (bytes) *bytes = (int64_t)workspace_bytes(c, o.restart);
	return CRD_OK;
}

int crd_lsolve_device(crd_ctx *c, double t, double gamma, const crd_lsolve_options *opt, const void *y, const void *r, void *z, crd_lsolve_stats *stats)
{
	crd_lsolve_options o;
	if (int rc = check_call(c, gamma, opt, y, r, z, &o)) return rc;
	return lsolve_device(c, t, gamma, o, y, r, z, stats);
}

int crd_lsolve_host(crd_ctx *c, double t, double gamma, const crd_lsolve_options *opt, const void *y, const void *r, void *z, crd_lsolve_stats *stats)
{
	crd_lsolve_options o;
	if (int rc = check_call(c, gamma, opt, y, r, z, &o)) return rc;
	if (int rc = set_device(c)) return rc;
	if (int rc = ensure_staging(c, 2 * (size_t)c->nx * (size_t)c->nyl * 8)) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->stage_in, r, vector_bytes(c), hipMemcpyHostToDevice, c->compute));
	const bool with_y = y && o.part == CRD_PART_FULL;
	if (with_y)
		if (int rc = stage_y(c, y)) return rc;
	if (int rc = lsolve_device(c, t, gamma, o, with_y ? c->stage_v : nullptr, c->stage_in, c->stage_out, stats)) return rc;
	HIP_TRY(c, hipMemcpyAsync(z, c->stage_out, vector_bytes(c), hipMemcpyDeviceToHost, c->compute));
	HIP_TRY(c, hipStreamSynchronize(c->compute));
	return CRD_OK;
}

int crd_krylov_probe_dots(crd_ctx *c, const void *vectors, int count, const void *wv, double *out)
{
	if (!c) return fail(nullptr, CRD_EINVAL, "probe_dots: no context");
	if (!vectors || !wv || !out || count < 1 || count > kKrylovMaxBasis) return fail(c, CRD_EINVAL, "probe_dots: count must be in 1 .. 65 and no pointer null");
	if (int rc = check_ctx(c)) return rc;
	if (int rc = set_device(c)) return rc;
	if (int rc = ensure_workspace(c, count > 1 ? count - 1 : 1)) return rc;
	LsolveWorkspace *w = c->lsolve;
	const size_t vb = vector_bytes(c);
	for (int i = 0; i < count; i++)
		HIP_TRY(c, hipMemcpyAsync(w->V + (size_t)i * w->stride * c->real_size, static_cast<const char *>(vectors) + (size_t)i * vb, vb, hipMemcpyHostToDevice, c->compute));
	HIP_TRY(c, hipMemcpyAsync(w->work[0], wv, vb, hipMemcpyHostToDevice, c->compute));
	HIP_TRY(c, launch_kr_dots(c->p.precision, w->V, w->stride, count, w->work[0], vector_reals(c), w->partials, w->h_cur, nullptr, 0, c->compute));
	HIP_TRY(c, hipMemcpyAsync(out, w->h_cur, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, c->compute));
	HIP_TRY(c, hipStreamSynchronize(c->compute));
	return CRD_OK;
}

}  // extern "C"
