// crd_multigrid.cpp -- entry points of the preconditioner solve (crd_psolve_*, include/crd.h): the level rule, the levels' coefficient
// tables and planes kept on the context, and the order of one V-cycle's launches (crd_multigrid.hip).  Host code only.
#include <cmath>
#include <cstring>
#include <vector>

#include "crd_ctx.h"
#include "crd_multigrid.h"

namespace crd {

// The levels of a context: planes and tables in one allocation, made at the first crd_psolve_* call for every level the grid has
// (whatever max_levels that call asks for), freed by crd_destroy.
struct PsolveWorkspace {
	int levels = 0;
	MgLevel level[kMgMaxLevels];  // held_lo / held_hi are a call's, not kept here
	void *base = nullptr;
	size_t bytes = 0;
};

void psolve_release(crd_ctx *c)
{
	if (!c || !c->psolve) return;
	if (c->psolve->base) (void)hipFree(c->psolve->base);
	delete c->psolve;
	c->psolve = nullptr;
}

}  // namespace crd

using namespace crd;

namespace {

constexpr size_t kAlign = 256;
size_t aligned(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

// Level l + 1 exists while nx and ny of level l are both even and both halves are at least 4.
int level_rule(int64_t nx, int64_t ny, int max_levels, int32_t *nxs, int32_t *nys)
{
	int n = 0;
	for (;;) {
		nxs[n] = (int32_t)nx;
		nys[n] = (int32_t)ny;
		n++;
		if (n >= max_levels || nx % 2 || ny % 2 || nx / 2 < 4 || ny / 2 < 4) return n;
		nx /= 2;
		ny /= 2;
	}
}

// Bytes of the workspace of a grid: three planes per level, three tables per level below the first (level 0 reads the context's).
size_t workspace_bytes(int levels, const int32_t *nxs, const int32_t *nys, size_t real)
{
	size_t total = 0;
	for (int l = 0; l < levels; l++) {
		total += 3 * aligned((size_t)nxs[l] * (size_t)nys[l] * real);
		if (l > 0) total += 3 * aligned((size_t)nxs[l] * real);
	}
	return total;
}

int check_ctx(crd_ctx *c)
{
	if (c->d0 > 1) return fail(c, CRD_ESTATE, "theta-blocks have no preconditioner solve");
	if (c->n_slabs > 1) return fail(c, CRD_ESTATE, "crd_psolve works on a context that holds the whole grid: a multi-slab cycle would exchange halos on every level");
	return CRD_OK;
}

int check_options(crd_ctx *c, const crd_psolve_options *opt, crd_psolve_options *o)
{
	if (opt) *o = *opt;
	else (void)crd_psolve_defaults(o);
	if (o->pre < 0 || o->post < 0 || (int64_t)o->pre + (int64_t)o->post < 1) return fail(c, CRD_EINVAL, "psolve: pre and post must be non-negative with pre + post >= 1");
	if (o->coarse < 1) return fail(c, CRD_EINVAL, "psolve: coarse must be at least 1");
	if (o->max_levels < 1 || o->max_levels > kMgMaxLevels) return fail(c, CRD_EINVAL, "psolve: max_levels must be in 1 .. 16");
	if (!(o->omega > 0.0 && o->omega <= 1.0)) return fail(c, CRD_EINVAL, "psolve: omega must be in (0, 1]");
	return CRD_OK;
}

int upload_level_table(crd_ctx *c, const std::vector<double> &src, void *dst)
{
	if (c->p.precision == CRD_PRECISION_F64) {
		HIP_TRY(c, hipMemcpy(dst, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice));
		return CRD_OK;
	}
	std::vector<float> f(src.size());
	for (size_t i = 0; i < src.size(); i++) f[i] = (float)src[i];
	HIP_TRY(c, hipMemcpy(dst, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
	return CRD_OK;
}

// The coarse tables are the fine formulas at doubled spacing: cX / 4, cA[2 I] / 2, cP[2 I] / 4, in double; cE = cX + cA and
// cWn = cA - cX are formed in double and rounded once to the context's precision.
int ensure_workspace(crd_ctx *c)
{
	if (c->psolve) return CRD_OK;
	int32_t nxs[kMgMaxLevels], nys[kMgMaxLevels];
	const int levels = level_rule(c->nx, c->nyl, kMgMaxLevels, nxs, nys);
	const size_t real = c->real_size, bytes = workspace_bytes(levels, nxs, nys, real);
	void *base = nullptr;
	hipError_t e = hipMalloc(&base, bytes);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		return fail(c, e == hipErrorOutOfMemory ? CRD_ENOMEM : CRD_EHIP, std::string("hipMalloc(psolve workspace): ") + hipGetErrorString(e));
	}
	PsolveWorkspace *w = new PsolveWorkspace;
	w->levels = levels;
	w->base = base;
	w->bytes = bytes;
	c->psolve = w;  // the context's from here on; a table upload that fails below releases it again
	Coefficients co;
	build_coefficients(c->p, c->g, &co);
	char *at = static_cast<char *>(base);
	auto take = [&](size_t n) {
		void *q = at;
		at += aligned(n);
		return q;
	};
	for (int l = 0; l < levels; l++) {
		MgLevel &m = w->level[l];
		m.nx = nxs[l];
		m.ny = nys[l];
		m.held_lo = m.held_hi = 0;
		const size_t plane = (size_t)m.nx * (size_t)m.ny * real;
		m.r = take(plane);
		m.z[0] = take(plane);
		m.z[1] = take(plane);
		if (l == 0) {
			m.cE = c->cE;
			m.cWn = c->cWn;
			m.cP = c->cP;
		} else {
			Coefficients next;
			next.cX = co.cX / 4;
			next.cA.resize((size_t)m.nx);
			next.cP.resize((size_t)m.nx);
			next.cE.resize((size_t)m.nx);
			next.cWn.resize((size_t)m.nx);
			for (int i = 0; i < m.nx; i++) {
				next.cA[(size_t)i] = co.cA[(size_t)(2 * i)] / 2;
				next.cP[(size_t)i] = co.cP[(size_t)(2 * i)] / 4;
				next.cE[(size_t)i] = next.cX + next.cA[(size_t)i];
				next.cWn[(size_t)i] = next.cA[(size_t)i] - next.cX;
			}
			co = next;
			void *cE = take((size_t)m.nx * real), *cWn = take((size_t)m.nx * real), *cP = take((size_t)m.nx * real);
			int rc;
			if ((rc = upload_level_table(c, co.cE, cE)) || (rc = upload_level_table(c, co.cWn, cWn)) || (rc = upload_level_table(c, co.cP, cP))) {
				psolve_release(c);
				return rc;
			}
			m.cE = cE;
			m.cWn = cWn;
			m.cP = cP;
		}
		m.cX2 = 2 * co.cX;
	}
	return CRD_OK;
}

size_t vector_bytes(const crd_ctx *c) { return 2 * (size_t)c->nx * (size_t)c->nyl * c->real_size; }

// One V-cycle's launches on the compute stream: down the levels (sweeps from z = 0, residual and restriction), `coarse` sweeps on
// the last, and up again (prolongation and correction, sweeps).  On level 0 the right-hand side is the caller's AoS vector until a
// sweep has left it as a plane, and the last sweep -- or, with post = 0, the prolongation -- writes the caller's AoS z.
struct Cycle {
	crd_ctx *c;
	const crd_psolve_options &o;
	double gamma;
	int levels;
	const void *r_aos;
	void *z_aos;
	MgLevel lv[kMgMaxLevels];
	int cur[kMgMaxLevels] = {};  // the plane of level l that holds its z
	bool rhs_plane = false;      // level 0's right-hand side has been stored as a plane

	int sweeps(int l, int n, bool from_zero, bool to_aos)
	{
		const int precision = c->p.precision;
		if (from_zero && n == 0) {
			HIP_TRY(c, hipMemsetAsync(lv[l].z[0], 0, (size_t)lv[l].nx * (size_t)lv[l].ny * c->real_size, c->compute));
			cur[l] = 0;
		}
		for (int k = 0; k < n; k++) {
			const bool first = from_zero && k == 0, out_aos = to_aos && k == n - 1;
			int flags = first ? kMgFirst : 0;
			if (l == 0 && (!rhs_plane || out_aos)) {
				flags |= kMgRhsAos;
				if (!rhs_plane && !out_aos) {
					flags |= kMgStoreRhs;
					rhs_plane = true;
				}
			}
			if (out_aos) flags |= kMgOutAos;
			const int dst = first ? 0 : 1 - cur[l];
			HIP_TRY(c, launch_mg_sweep(precision, lv[l], gamma, o.omega, flags, r_aos, first ? nullptr : lv[l].z[cur[l]], out_aos ? nullptr : lv[l].z[dst], z_aos, c->compute));
			cur[l] = dst;
		}
		return CRD_OK;
	}

	int run()
	{
		const int precision = c->p.precision;
		for (int l = 0; l < levels; l++) {
			const bool last = l == levels - 1;
			if (int rc = sweeps(l, last ? o.coarse : o.pre, true, last && l == 0)) return rc;
			if (last) break;
			HIP_TRY(c, launch_mg_restrict(precision, lv[l], lv[l + 1], gamma, l == 0 && !rhs_plane, r_aos, lv[l].z[cur[l]], c->compute));
		}
		for (int l = levels - 2; l >= 0; l--) {
			const bool to_aos = l == 0;
			HIP_TRY(c, launch_mg_prolong(precision, lv[l], lv[l + 1], lv[l + 1].z[cur[l + 1]], lv[l].z[cur[l]], to_aos && o.post == 0 ? r_aos : nullptr,
			                             to_aos && o.post == 0 ? z_aos : nullptr, c->compute));
			if (int rc = sweeps(l, o.post, false, to_aos)) return rc;
		}
		return CRD_OK;
	}
};

int psolve_device(crd_ctx *c, double t, double gamma, const crd_psolve_options &o, const void *r, void *z)
{
	if (int rc = set_device(c)) return rc;
	if (gamma == 0.0) {  // P = I
		HIP_TRY(c, hipMemcpyAsync(z, r, vector_bytes(c), hipMemcpyDeviceToDevice, c->compute));
		return CRD_OK;
	}
	if (int rc = ensure_workspace(c)) return rc;
	const PsolveWorkspace &w = *c->psolve;
	Cycle cy{c, o, gamma, w.levels < o.max_levels ? w.levels : o.max_levels, r, z, {}, {}, false};
	// rows are held when J has zero rows at t: the rule of crd_jtimes_* (crd_jacobian.cpp: absorb_flag)
	const int held = absorbing(c, t) && !c->desc.just_diffusion ? 1 : 0;
	for (int l = 0; l < cy.levels; l++) {
		cy.lv[l] = w.level[l];
		cy.lv[l].held_lo = held;
		cy.lv[l].held_hi = l == 0 ? held : 0;  // fine row ny - 1 has no coarse counterpart
	}
	return cy.run();
}

int check_call(crd_ctx *c, double gamma, const crd_psolve_options *opt, const void *r, void *z, crd_psolve_options *o)
{
	if (!c) return fail(nullptr, CRD_EINVAL, "psolve: no context");
	if (!r || !z) return fail(c, CRD_EINVAL, "psolve: r and z must not be null");
	if (!std::isfinite(gamma) || gamma < 0.0) return fail(c, CRD_EINVAL, "psolve: gamma must be finite and not negative");
	if (int rc = check_options(c, opt, o)) return rc;
	if (z == r) return fail(c, CRD_EINVAL, "psolve: z must not be r (a sweep reads r after z is written)");
	return check_ctx(c);
}

}  // namespace

extern "C" {

int crd_psolve_defaults(crd_psolve_options *opt)
{
	if (!opt) return CRD_EINVAL;
	opt->pre = opt->post = 2;
	opt->coarse = 8;
	opt->max_levels = kMgMaxLevels;
	opt->omega = 0.8;
	return CRD_OK;
}

int crd_psolve_info(crd_ctx *c, const crd_psolve_options *opt, int32_t *levels, int32_t nx[16], int32_t ny[16], int64_t *bytes)
{
	if (!c) return fail(nullptr, CRD_EINVAL, "psolve: no context");
	crd_psolve_options o;
	if (int rc = check_options(c, opt, &o)) return rc;
	if (int rc = check_ctx(c)) return rc;
	int32_t nxs[kMgMaxLevels] = {}, nys[kMgMaxLevels] = {};
	const int all = level_rule(c->nx, c->nyl, kMgMaxLevels, nxs, nys);
	if (bytes) *bytes = (int64_t)workspace_bytes(all, nxs, nys, c->real_size);  // the workspace holds every level the grid has
	const int n = all < o.max_levels ? all : o.max_levels;
	if (levels) *levels = n;
	for (int l = 0; l < kMgMaxLevels; l++) {
		if (nx) nx[l] = l < n ? nxs[l] : 0;
		if (ny) ny[l] = l < n ? nys[l] : 0;
	}
	return CRD_OK;
}

int crd_psolve_device(crd_ctx *c, double t, double gamma, const crd_psolve_options *opt, const void *r, void *z)
{
	crd_psolve_options o;
	if (int rc = check_call(c, gamma, opt, r, z, &o)) return rc;
	return psolve_device(c, t, gamma, o, r, z);
}

int crd_psolve_host(crd_ctx *c, double t, double gamma, const crd_psolve_options *opt, const void *r, void *z)
{
	crd_psolve_options o;
	if (int rc = check_call(c, gamma, opt, r, z, &o)) return rc;
	if (int rc = set_device(c)) return rc;
	if (int rc = ensure_staging(c, 2 * (size_t)c->nx * (size_t)c->nyl * 8)) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->stage_in, r, vector_bytes(c), hipMemcpyHostToDevice, c->compute));
	if (int rc = psolve_device(c, t, gamma, o, c->stage_in, c->stage_out)) return rc;
	HIP_TRY(c, hipMemcpyAsync(z, c->stage_out, vector_bytes(c), hipMemcpyDeviceToHost, c->compute));
	HIP_TRY(c, hipStreamSynchronize(c->compute));
	return CRD_OK;
}

}  // extern "C"
