// crd_imex.cpp -- crd_step_imex (include/crd.h): IMEX additive Runge-Kutta steps with the diffusion part implicit.  This file owns the
// step's vectors, kept on the context, and the order of launches: f_D (crd_rhs_part_device), the linear solve (crd_lsolve_device, or
// crd_bicgstab_device where the options ask for it) and the stage close (crd_imex.hip) that carries everything else.  The schemes are crd_imex_tables.h's.
// crd_integrate_imex makes attempts of the same stages behind the estimating last close; its step sizes are crd_imex_control.h's.  Host code only.
#include <cmath>

#include "crd_ctx.h"
#include "crd_imex.h"
#include "crd_imex_control.h"
#include "crd_imex_tables.h"

namespace crd {

// y_n, R, k_1 .. k_s, FR_0 .. FR_{s-1} and r (the solve's right-hand side, in the slot of FR_s), the last close's partial maxima: one
// allocation, made by the first crd_step_imex call, made again when a call's scheme has more stages, freed by crd_destroy.
struct ImexWorkspace {
	int stages = 0;
	void *base = nullptr;
	void *yn = nullptr, *R = nullptr, *k[imex::kMaxStages + 1] = {}, *FR[imex::kMaxStages + 1] = {};
	double *partials = nullptr;
};

void imex_release(crd_ctx *c)
{
	if (!c || !c->imex) return;
	if (c->imex->base) (void)hipFree(c->imex->base);
	delete c->imex;
	c->imex = nullptr;
}

}  // namespace crd

using namespace crd;

namespace {

constexpr size_t kAlign = 256;
size_t aligned(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }
size_t vector_bytes(const crd_ctx *c) { return 2 * (size_t)c->nx * (size_t)c->nyl * c->real_size; }
size_t workspace_bytes(const crd_ctx *c, int stages) { return (2 * (size_t)stages + 3) * aligned(vector_bytes(c)) + aligned(kImexBlocks * sizeof(double)); }

int ensure_workspace(crd_ctx *c, int stages)
{
	if (c->imex && c->imex->stages >= stages) return CRD_OK;
	HIP_TRY(c, hipStreamSynchronize(c->compute));
	imex_release(c);
	void *base = nullptr;
	hipError_t e = hipMalloc(&base, workspace_bytes(c, stages));
	if (e != hipSuccess) {
		(void)hipGetLastError();
		return fail(c, e == hipErrorOutOfMemory ? CRD_ENOMEM : CRD_EHIP, std::string("hipMalloc(imex workspace): ") + hipGetErrorString(e));
	}
	ImexWorkspace *w = new ImexWorkspace;
	w->stages = stages;
	w->base = base;
	c->imex = w;
	char *at = static_cast<char *>(base);
	const size_t vec = aligned(vector_bytes(c));
	auto take = [&] {
		void *p = at;
		at += vec;
		return p;
	};
	w->yn = take();
	w->R = take();
	for (int i = 1; i <= stages; i++) w->k[i] = take();
	for (int i = 0; i <= stages; i++) w->FR[i] = take();
	w->partials = reinterpret_cast<double *>(at);
	return CRD_OK;
}

// the BiCGStab options that `lsolve` stands for (restart is not read)
crd_bicgstab_options bicgstab_options(const crd_lsolve_options &l, int guess)
{
	crd_bicgstab_options b;
	b.part = l.part;
	b.precondition = l.precondition;
	b.max_iters = l.max_iters;
	b.guess = guess;
	b.rtol = l.rtol;
	b.atol = l.atol;
	b.psolve = l.psolve;
	return b;
}

// the chosen solver's own check of its options and of the context, and its workspace
int solver_info(crd_ctx *c, const crd_imex_options &o, int64_t *bytes)
{
	if (o.solver == CRD_IMEX_SOLVER_GMRES) return crd_lsolve_info(c, &o.lsolve, bytes);
	const crd_bicgstab_options b = bicgstab_options(o.lsolve, 0);
	return crd_bicgstab_info(c, &b, bytes);
}

// What the call refuses before any device work; *o the options it runs with, *T their scheme.
int check_call(crd_ctx *c, double t0, double dt, int64_t nsteps, const crd_imex_options *opt, crd_imex_options *o, imex::Tableau *T)
{
	if (opt) *o = *opt;
	else (void)crd_imex_defaults(o);
	if (!imex::tableau(o->scheme, T)) return fail(c, CRD_EINVAL, "imex: scheme must be CRD_IMEX_EULER, CRD_IMEX_ARS222 or CRD_IMEX_ARS443");
	if (o->solver != CRD_IMEX_SOLVER_GMRES && o->solver != CRD_IMEX_SOLVER_BICGSTAB && o->solver != CRD_IMEX_SOLVER_BICGSTAB_WARM)
		return fail(c, CRD_EINVAL, "imex: solver must be CRD_IMEX_SOLVER_GMRES, CRD_IMEX_SOLVER_BICGSTAB or CRD_IMEX_SOLVER_BICGSTAB_WARM");
	if (o->lsolve.part != CRD_PART_DIFFUSION) return fail(c, CRD_EINVAL, "imex: lsolve.part must be CRD_PART_DIFFUSION (the implicit part is the diffusion operator)");
	if (!(dt > 0.0) || !std::isfinite(dt) || !std::isfinite(t0)) return fail(c, CRD_EINVAL, "imex: dt must be positive and finite, t0 finite");
	if (nsteps < 0) return fail(c, CRD_EINVAL, "imex: nsteps must not be negative");
	if (int rc = solver_info(c, *o, nullptr)) {  // its options, and the contexts it refuses: several slabs, theta-blocks
		const std::string why = c->err;
		return fail(c, rc, "imex: " + why);
	}
	if (c->recorder) return fail(c, CRD_ESTATE, "imex: a run recorder is open on this context; crd_step_imex takes no samples");
	return CRD_OK;
}

struct Stepper {
	crd_ctx *c;
	const crd_imex_options &o;
	const imex::Tableau &T;
	double dt;  // of the step at hand
	crd_imex_stats st{};
	ImexWorkspace *w = nullptr;
	bool f32 = false;
	const void *last_k = nullptr;  // the k of the solve before (CRD_IMEX_SOLVER_BICGSTAB_WARM starts the next one from it)

	int absorb_at(double t) const { return absorbing(c, t) && !c->desc.just_diffusion ? 1 : 0; }

	// the close of stage i at time t: FR_i and R_{i+1}, or (i = s) Y_s into R
	int close(int i, double t)
	{
		ImexClose a;
		a.R = i == 0 ? w->yn : w->R;
		a.k = i == 0 ? nullptr : w->k[i];
		a.yn = w->yn;
		a.hg = imex::rounded(dt * T.gamma, f32);
		a.absorb = absorb_at(t);
		if (i == T.stages) {
			a.last = 1;
			a.out = w->R;
			a.partials = w->partials;
			a.max_out = c->scalar_sink();
		} else {
			a.FR = w->FR[i];
			a.Rnext = w->R;
			imex::Term terms[2 * imex::kMaxStages];
			const int n = imex::row_terms(T, i + 1, dt, f32, terms);
			for (int q = 0; q < n; q++) {
				const imex::Term &m = terms[q];
				if (m.j < i) {
					if (a.nterms >= kImexMaxTerms) return fail(c, CRD_EINVAL, "imex: a row with more stored terms than the stage close takes");
					a.term[a.nterms] = m.explicit_part ? w->FR[m.j] : w->k[m.j];
					a.coef[a.nterms++] = m.coef;
				} else if (m.explicit_part) {
					a.cE = m.coef;
				} else {
					a.cI = m.coef;
				}
			}
		}
		HIP_TRY(c, launch_imex_close(c->p.precision, c->desc, a, c->compute));
		return CRD_OK;
	}

	int stopped(int64_t n, int stage, const std::string &why)
	{
		st.failed_step = n;
		st.failed_stage = stage;
		return fail(c, CRD_ESTATE, "imex: step " + std::to_string(n) + ", stage " + std::to_string(stage) + ": " + why);
	}

	// stage 0 .. the solve of stage s: everything of a step but its last close
	int stages(int64_t n, double t, int64_t *iterations_out = nullptr)
	{
		if (int rc = close(0, t)) return rc;
		const double hg = imex::rounded(dt * T.gamma, f32);
		for (int i = 1; i <= T.stages; i++) {
			const double ti = t + T.c[i] * dt;
			void *r = w->FR[T.stages];
			if (int rc = crd_rhs_part_device(c, ti, CRD_PART_DIFFUSION, w->R, r)) return rc;
			// what the stage's solve reports: {converged, iterations, ||r||, its residual}
			int converged = 0, iterations = 0;
			double r_norm = 0.0, res_norm = 0.0;
			if (o.solver == CRD_IMEX_SOLVER_GMRES) {
				crd_lsolve_stats ls{};
				if (int rc = crd_lsolve_device(c, ti, hg, &o.lsolve, nullptr, r, w->k[i], &ls)) return rc;
				converged = ls.converged, iterations = ls.iterations, r_norm = ls.r_norm, res_norm = ls.res_norm;
			} else {
				const bool warm = o.solver == CRD_IMEX_SOLVER_BICGSTAB_WARM && last_k;
				if (warm && last_k != w->k[i]) HIP_TRY(c, hipMemcpyAsync(w->k[i], last_k, vector_bytes(c), hipMemcpyDeviceToDevice, c->compute));
				const crd_bicgstab_options b = bicgstab_options(o.lsolve, warm ? 1 : 0);
				crd_bicgstab_stats bs{};
				if (int rc = crd_bicgstab_device(c, ti, hg, &b, nullptr, r, w->k[i], &bs)) return rc;
				converged = bs.converged, iterations = bs.iterations, r_norm = bs.r_norm, res_norm = bs.true_res_norm;
				last_k = w->k[i];
			}
			st.solves++;
			st.iterations += iterations;
			if (iterations_out) *iterations_out += iterations;
			if (iterations > st.max_iterations) st.max_iterations = iterations;
			if (r_norm > 0.0 && !(res_norm / r_norm <= st.worst_residual)) st.worst_residual = res_norm / r_norm;
			if (!converged) return stopped(n, i, "the linear solve did not converge in " + std::to_string(iterations) + " iterations");
			if (i < T.stages)
				if (int rc = close(i, ti)) return rc;
		}
		return CRD_OK;
	}

	int step(int64_t n, double t)
	{
		if (int rc = stages(n, t)) return rc;
		if (int rc = close(T.stages, t + T.c[T.stages] * dt)) return rc;
		double *sink = c->scalar_sink();
		if (sink != c->scalar_host) HIP_TRY(c, hipMemcpyAsync(c->scalar_host, sink, sizeof(double), hipMemcpyDeviceToHost, c->compute));
		HIP_TRY(c, hipStreamSynchronize(c->compute));
		const double m = c->scalar_host[0];
		if (!std::isfinite(m)) return stopped(n, T.stages, "the new state is not finite");
		st.max_abs_u = m;
		std::swap(w->yn, w->R);  // Y_s is y_{n+1}
		return CRD_OK;
	}

	int run(double t0, int64_t nsteps)
	{
		f32 = c->p.precision != CRD_PRECISION_F64;
		st.failed_step = -1;
		st.failed_stage = -1;
		st.t = t0;
		if (int rc = set_device(c)) return rc;
		if (nsteps == 0) return crd_state_max_abs(c, &st.max_abs_u);
		if (int rc = ensure_workspace(c, T.stages)) return rc;
		w = c->imex;
		arkode::drop(c->dense, c->ark);  // stepping on from the state handed back, not from the integrator's internal one
		c->cycle_pos = -1;
		HIP_TRY(c, launch_planes_to_aos(c->p.precision, f32 ? 0 : 1, c->planes(crd_ctx::Y), w->yn, c->nx, c->nyl, c->compute));
		int rc = CRD_OK;
		for (int64_t n = 0; n < nsteps && rc == CRD_OK; n++) {
			rc = step(n, t0 + (double)n * dt);
			if (rc == CRD_OK) st.steps = n + 1;
		}
		st.t = t0 + (double)st.steps * dt;
		// the resident state: that of the last completed step
		const std::string why = c->err;
		if (st.steps > 0) {
			hipError_t e = launch_aos_to_planes(c->p.precision, f32 ? 0 : 1, w->yn, c->planes(crd_ctx::Y), c->nx, c->nyl, c->compute);
			if (e == hipSuccess) e = hipStreamSynchronize(c->compute);
			if (e != hipSuccess && rc == CRD_OK) return fail(c, CRD_EHIP, std::string("imex: storing the state: ") + hipGetErrorString(e));
		}
		if (rc != CRD_OK) c->err = why;
		return rc;
	}

	// ---- crd_integrate_imex ----
	// The estimating last close of the step from y_n of size dt: Y_s into R, max |var0| and the sum of the weighted squares into result.
	// The sum's partials lie in the vector of r, which nothing reads behind the last solve.
	int estimate_close(double hg, double rtol, double atol, void *e_out, double *result)
	{
		ImexEstimate a;
		a.R = w->R;
		a.k = w->k[T.stages];
		a.yn = w->yn;
		a.out = w->R;
		a.e_out = e_out;
		a.hg = hg;
		a.rtol = rtol;
		a.atol = atol;
		imex::Term terms[imex::kMaxEstimateTerms];
		const int n = imex::estimate_terms(T, dt, f32, terms);
		for (int q = 0; q < n; q++) {
			const imex::Term &m = terms[q];
			if (!m.explicit_part && m.j == T.stages) {
				a.ck = m.coef;
			} else if (m.j >= T.stages || a.nterms >= kImexEstimateTerms) {
				return fail(c, CRD_EINVAL, "imex: an estimate with a term the estimating close does not take");
			} else {
				a.term[a.nterms] = m.explicit_part ? w->FR[m.j] : w->k[m.j];
				a.coef[a.nterms++] = m.coef;
			}
		}
		a.max_partials = w->partials;
		a.sum_partials = static_cast<double *>(w->FR[T.stages]);
		a.result = result;
		HIP_TRY(c, launch_imex_estimate(c->p.precision, c->desc, a, c->compute));
		return CRD_OK;
	}

	// One attempt from (t, y_n) of size h: *norm is the WRMS norm of the estimate, NaN when it or the new state is not finite.  y_n is
	// not written; Y_s is in R.
	int attempt(int64_t n, double t, double h, double rtol, double atol, double *norm, int64_t *iterations)
	{
		dt = h;
		last_k = nullptr;  // as a crd_step_imex call of one step: the first solve starts from x = 0
		if (int rc = stages(n, t, iterations)) return rc;
		double *sink = c->scalar_sink();
		if (int rc = estimate_close(imex::rounded(dt * T.gamma, f32), rtol, atol, nullptr, sink)) return rc;
		if (sink != c->scalar_host) HIP_TRY(c, hipMemcpyAsync(c->scalar_host, sink, 2 * sizeof(double), hipMemcpyDeviceToHost, c->compute));
		HIP_TRY(c, hipStreamSynchronize(c->compute));
		const double m = c->scalar_host[0], sum = c->scalar_host[1];
		*norm = std::isfinite(m) && std::isfinite(sum) ? std::sqrt(sum / (2.0 * (double)c->nx * (double)c->nyl)) : NAN;
		if (std::isfinite(m)) st.max_abs_u = m;
		return CRD_OK;
	}

	int integrate(double t0, double tout, const crd_imex_adaptive_options &ao, crd_imex_adaptive_stats *as, crd_imex_attempt *history, int64_t history_cap)
	{
		f32 = c->p.precision != CRD_PRECISION_F64;
		st.failed_step = -1;
		st.failed_stage = -1;
		st.t = t0;
		imex::Control K;
		K.start(t0, tout, ao.h0 > 0.0 ? ao.h0 : crd_stable_dt(&c->p), imex::control_options(ao.rtol, ao.atol, ao.h0, ao.h_max, ao.safety, ao.bias, ao.growth, ao.shrink, ao.max_steps));
		auto figures = [&] {
			st.steps = K.st.accepted;
			st.t = K.t;
			as->imex = st;
			as->accepted = K.st.accepted, as->rejected = K.st.rejected, as->attempts = K.attempts;
			as->h_first = K.st.h_first, as->h_last = K.st.h_last, as->h_min = K.st.h_min, as->h_max = K.st.h_max;
			as->err_last = K.st.err_last, as->t = K.t, as->h_next = K.h_next();
		};
		as->recorded = 0;
		if (int rc = set_device(c)) return rc;
		if (K.done()) {
			const int rc = crd_state_max_abs(c, &st.max_abs_u);
			figures();
			return rc;
		}
		if (int rc = ensure_workspace(c, T.stages)) return rc;
		w = c->imex;
		arkode::drop(c->dense, c->ark);
		c->cycle_pos = -1;
		HIP_TRY(c, launch_planes_to_aos(c->p.precision, f32 ? 0 : 1, c->planes(crd_ctx::Y), w->yn, c->nx, c->nyl, c->compute));
		int rc = CRD_OK;
		while (rc == CRD_OK && !K.done()) {
			double t = 0.0, h = 0.0, norm = NAN;
			if (const char *why = K.next(&t, &h)) {
				rc = fail(c, CRD_ESTATE, std::string("imex: ") + why);
				break;
			}
			int64_t iterations = 0;
			rc = attempt(K.attempts - 1, t, h, ao.rtol, ao.atol, &norm, &iterations);
			if (rc != CRD_OK) break;
			const int verdict = K.verdict(norm);
			if (verdict == 1) std::swap(w->yn, w->R);  // Y_s is y_{n+1}
			if (history && as->recorded < history_cap) history[as->recorded++] = crd_imex_attempt{t, h, K.st.err_last, verdict == 1, (int32_t)iterations};
			if (verdict < 0) rc = fail(c, CRD_ESTATE, std::string("imex: ") + arkode::kErrFailure);
		}
		figures();
		const std::string why = c->err;
		if (K.st.accepted > 0) {
			hipError_t e = launch_aos_to_planes(c->p.precision, f32 ? 0 : 1, w->yn, c->planes(crd_ctx::Y), c->nx, c->nyl, c->compute);
			if (e == hipSuccess) e = hipStreamSynchronize(c->compute);
			if (e != hipSuccess && rc == CRD_OK) return fail(c, CRD_EHIP, std::string("imex: storing the state: ") + hipGetErrorString(e));
		}
		if (rc != CRD_OK) c->err = why;
		return rc;
	}
};

const char *check_adaptive(const crd_imex_adaptive_options &o, double t0, double tout, const crd_imex_attempt *history, int64_t history_cap)
{
	if (o.imex.scheme != CRD_IMEX_ARS443)
		return "imex: error control needs CRD_IMEX_ARS443: Euler and ARS(2,2,2) have no embedded solution that is both damped at infinity and able to see the diffusion error";
	if (!std::isfinite(o.rtol) || !std::isfinite(o.atol) || o.rtol < 0.0 || o.atol < 0.0 || !(o.rtol + o.atol > 0.0)) return "imex: rtol and atol must be finite, not negative and not both zero";
	if (!std::isfinite(t0) || !std::isfinite(tout) || tout < t0) return "imex: t0 and tout must be finite and tout not before t0";
	if (!(o.h0 >= 0.0) || !std::isfinite(o.h0)) return "imex: h0 must be finite and not negative (0: crd_stable_dt)";
	if (std::isnan(o.h_max)) return "imex: h_max must not be NaN";
	if (!(o.safety > 0.0) || !(o.bias > 0.0) || !(o.growth >= 1.0) || !(o.shrink > 0.0) || !(o.shrink < 1.0)) return "imex: safety and bias must be positive, growth at least 1, shrink inside (0, 1)";
	if (o.max_steps < 1) return "imex: max_steps must be at least 1";
	if (history_cap < 0 || (history_cap > 0 && !history)) return "imex: history_cap must not be negative, and history not null with it positive";
	return nullptr;
}

}  // namespace

extern "C" {

int crd_imex_defaults(crd_imex_options *opt)
{
	if (!opt) return CRD_EINVAL;
	opt->scheme = CRD_IMEX_ARS222;
	opt->solver = CRD_IMEX_SOLVER_GMRES;
	return crd_lsolve_defaults(&opt->lsolve);
}

int crd_imex_info(crd_ctx *c, const crd_imex_options *opt, int64_t *bytes)
{
	if (!c) return fail(nullptr, CRD_EINVAL, "imex: no context");
	crd_imex_options o;
	imex::Tableau T;
	if (int rc = check_call(c, 0.0, 1.0, 0, opt, &o, &T)) return rc;
	int64_t solve = 0;
	if (int rc = solver_info(c, o, &solve)) return rc;
	if (bytes) *bytes = (int64_t)workspace_bytes(c, T.stages) + solve;
	return CRD_OK;
}

int crd_step_imex(crd_ctx *c, double t0, double dt, int64_t nsteps, const crd_imex_options *opt, crd_imex_stats *stats)
{
	if (!c) return fail(nullptr, CRD_EINVAL, "imex: no context");
	crd_imex_options o;
	imex::Tableau T;
	if (int rc = check_call(c, t0, dt, nsteps, opt, &o, &T)) return rc;
	TraceRange range("crd_step_imex");
	Stepper s{c, o, T, dt};
	const int rc = s.run(t0, nsteps);
	if (stats) *stats = s.st;
	return rc;
}

int crd_imex_adaptive_defaults(crd_imex_adaptive_options *opt)
{
	if (!opt) return CRD_EINVAL;
	if (int rc = crd_imex_defaults(&opt->imex)) return rc;
	opt->imex.scheme = CRD_IMEX_ARS443;
	crd_adaptive_options a;
	(void)crd_adaptive_defaults(&a);
	opt->rtol = a.rtol, opt->atol = a.atol, opt->h0 = 0.0, opt->h_max = 0.0;
	opt->safety = a.safety, opt->bias = a.bias, opt->growth = a.growth, opt->shrink = a.shrink;
	opt->max_steps = a.max_steps;
	return CRD_OK;
}

int crd_integrate_imex(crd_ctx *c, double t0, double tout, const crd_imex_adaptive_options *opt, crd_imex_adaptive_stats *stats, crd_imex_attempt *history, int64_t history_cap)
{
	if (!c) return fail(nullptr, CRD_EINVAL, "imex: no context");
	crd_imex_adaptive_options ao;
	if (opt) ao = *opt;
	else (void)crd_imex_adaptive_defaults(&ao);
	crd_imex_options o;
	imex::Tableau T;
	if (int rc = check_call(c, std::isfinite(t0) ? t0 : 0.0, 1.0, 0, &ao.imex, &o, &T)) return rc;
	if (const char *why = check_adaptive(ao, t0, tout, history, history_cap)) return fail(c, CRD_EINVAL, why);
	TraceRange range("crd_integrate_imex");
	Stepper s{c, o, T, 0.0};
	crd_imex_adaptive_stats as{};
	const int rc = s.integrate(t0, tout, ao, &as, history, history_cap);
	if (stats) *stats = as;
	return rc;
}

int crd_imex_estimate_probe(crd_ctx *c, const double *scalars, const void *in, void *out, double *result)
{
	if (!c) return fail(nullptr, CRD_EINVAL, "imex_estimate_probe: no context");
	if (!scalars || !in || !out || !result) return fail(c, CRD_EINVAL, "imex_estimate_probe: no pointer may be null");
	crd_imex_options o;
	(void)crd_imex_defaults(&o);
	o.scheme = CRD_IMEX_ARS443;
	imex::Tableau T;
	if (int rc = check_call(c, 0.0, 1.0, 0, &o, &o, &T)) return rc;
	const double hg = scalars[0], dt = scalars[1], rtol = scalars[2], atol = scalars[3];
	if (!std::isfinite(hg) || !std::isfinite(dt)) return fail(c, CRD_EINVAL, "imex_estimate_probe: hg and dt must be finite");
	if (int rc = set_device(c)) return rc;
	if (int rc = ensure_workspace(c, T.stages)) return rc;
	if (int rc = ensure_staging(c, 2 * (size_t)c->nx * (size_t)c->nyl * 8)) return rc;
	Stepper s{c, o, T, dt};
	s.f32 = c->p.precision != CRD_PRECISION_F64;
	s.w = c->imex;
	ImexWorkspace *w = c->imex;
	const size_t vb = vector_bytes(c);
	void *slot[10] = {w->R, w->k[4], w->yn, w->FR[0], w->FR[1], w->k[1], w->FR[2], w->k[2], w->FR[3], w->k[3]};
	for (int i = 0; i < 10; i++) HIP_TRY(c, hipMemcpyAsync(slot[i], static_cast<const char *>(in) + (size_t)i * vb, vb, hipMemcpyHostToDevice, c->compute));
	// the close as an attempt launches it, but for hg, which is the caller's
	double *sink = c->scalar_sink();
	if (int rc = s.estimate_close(imex::rounded(hg, s.f32), rtol, atol, c->stage_out, sink)) return rc;
	if (sink != c->scalar_host) HIP_TRY(c, hipMemcpyAsync(c->scalar_host, sink, 2 * sizeof(double), hipMemcpyDeviceToHost, c->compute));
	HIP_TRY(c, hipMemcpyAsync(out, w->R, vb, hipMemcpyDeviceToHost, c->compute));
	HIP_TRY(c, hipMemcpyAsync(static_cast<char *>(out) + vb, c->stage_out, vb, hipMemcpyDeviceToHost, c->compute));
	HIP_TRY(c, hipStreamSynchronize(c->compute));
	result[0] = c->scalar_host[1];
	result[1] = c->scalar_host[0];
	return CRD_OK;
}

}  // extern "C"
