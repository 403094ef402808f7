// crd_ensemble.cpp -- ensembles behind the C ABI (include/crd.h, crd_ensemble_*): B independent single-slab problems of one geometry,
// stepped by one launch per RK4 step (crd_ensemble.hip).  Host code only.  A member owns its tables and two state buffers; the
// members' descriptors sit in a device table the step kernel reads.
#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "crd_ctx.h"
#include "crd_device.h"
#include "crd_ensemble.h"

using namespace crd;

struct crd_ensemble {
	std::vector<crd_params> p;
	crd_grid g{};
	int n = 0, device = 0, precision = CRD_PRECISION_F64, model = CRD_MODEL_FHN;  // model: kernel_model's (diffusion-only is its own)
	int nx = 0, ny = 0;
	size_t real_size = 8;
	EnsemblePlan plan;
	std::vector<EnsembleMember> members;   // host copy of the descriptor table
	EnsembleMember *table = nullptr;       // ... on the device
	std::vector<void *> allocs;            // every device allocation but the table
	int cur = 0;                           // the buffer holding every member's current state
	void *stage = nullptr;                 // AoS staging of upload / download (nx * ny pairs of doubles)
	double *max_dev = nullptr, *max_host = nullptr;  // n doubles each; max_host page-locked
	hipStream_t stream = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	std::string err;
};

namespace {

thread_local std::string g_create_error;  // crd_ensemble_last_error(NULL)

int efail(crd_ensemble *e, int code, const std::string &msg)
{
	if (e) e->err = msg;
	else g_create_error = msg;
	return code;
}

#define ENS_TRY(e, expr)                                                                                                   \
	do {                                                                                                                    \
		hipError_t r_ = (expr);                                                                                             \
		if (r_ != hipSuccess)                                                                                               \
			return efail((e), r_ == hipErrorOutOfMemory ? CRD_ENOMEM : CRD_EHIP, std::string(#expr) + ": " + hipGetErrorString(r_)); \
	} while (0)

// The first field in which member k differs from member 0 where members must agree, or nullptr.
const char *disagreement(const crd_params &a, const crd_grid &ga, const crd_params &b, const crd_grid &gb)
{
	if (a.model != b.model) return "model";
	if (a.surface != b.surface) return "surface";
	if (a.nx != b.nx) return "nx";
	if (a.surface_length != b.surface_length) return "surface_length";
	if (a.surface_width != b.surface_width) return "surface_width";
	if (a.precision != b.precision) return "precision";
	if (a.just_diffusion != b.just_diffusion) return "just_diffusion";
	if (ga.ny != gb.ny) return "ny";  // (the derived row count: after the fields it derives from)
	return nullptr;
}

int check_member(crd_ensemble *e, int member)
{
	if (member < 0 || member >= e->n) return efail(e, CRD_EINVAL, "member index out of range");
	return CRD_OK;
}

}  // namespace

extern "C" {

int crd_ensemble_create(const crd_params *members, int n_members, int device, crd_ensemble **out)
{
	if (!out) return CRD_EINVAL;
	*out = nullptr;
	// Everything that can be refused without a device is refused first.
	if (!members) return efail(nullptr, CRD_EINVAL, "null members");
	if (n_members < 1) return efail(nullptr, CRD_EINVAL, "an ensemble needs at least one member (n_members = " + std::to_string(n_members) + ")");
	std::vector<crd_grid> grids((size_t)n_members);
	for (int k = 0; k < n_members; k++) {
		std::string why;
		if (!validate_params(members[k], &why)) return efail(nullptr, CRD_EINVAL, "member " + std::to_string(k) + ": " + why);
		if (int rc = crd_grid_from_params(&members[k], &grids[(size_t)k])) return efail(nullptr, rc, "member " + std::to_string(k) + ": bad geometry");
		if (const char *f = disagreement(members[0], grids[0], members[k], grids[(size_t)k]))
			return efail(nullptr, CRD_EINVAL, "member " + std::to_string(k) + " differs from member 0 in " + f + " (members may differ in diffusion, beta, beta_min, beta_max, vary_beta and t_boundary only)");
	}
	if (grids[0].ny < 2 * kStepHalo) return efail(nullptr, CRD_EINVAL, "every member needs at least 8 rows");
	if (grids[0].ny > INT32_MAX / 2) return efail(nullptr, CRD_EINVAL, "members too tall");
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
		(void)hipGetLastError();
		return efail(nullptr, CRD_EHIP, "no HIP device available (libcrd has no CPU fallback)");
	}
	if (device < 0 || device >= ndev) return efail(nullptr, CRD_EINVAL, "device ordinal out of range");

	crd_ensemble *e = new (std::nothrow) crd_ensemble;
	if (!e) return efail(nullptr, CRD_ENOMEM, "host allocation failed");
	auto bail = [&](int rc) {
		g_create_error = e->err;
		crd_ensemble_destroy(e);
		return rc;
	};
	e->p.assign(members, members + n_members);
	e->g = grids[0];
	e->n = n_members;
	e->device = device;
	e->precision = members[0].precision;
	e->real_size = e->precision == CRD_PRECISION_F64 ? 8 : 4;
	e->nx = (int)e->g.nx;
	e->ny = (int)e->g.ny;
	e->model = (members[0].model == CRD_MODEL_GOLDBETER && members[0].just_diffusion) ? dev::kModelDiffusionOnly : members[0].model;
	const size_t points = (size_t)e->nx * (size_t)e->ny, plane = points * e->real_size;
	// (block ids are 32-bit: at most one block per strip of 56 columns and chunk of 4 rows per member)
	if ((long)n_members * ((e->nx + 55) / 56) * ((e->ny + 3) / 4) > INT32_MAX) return bail(efail(e, CRD_EINVAL, "too many work items for one launch"));

	auto step = [&](hipError_t r, const char *what) {
		if (r != hipSuccess) efail(e, r == hipErrorOutOfMemory ? CRD_ENOMEM : CRD_EHIP, std::string(what) + ": " + hipGetErrorString(r));
		return r == hipSuccess;
	};
	auto device_alloc = [&](size_t bytes, void **q) {
		*q = nullptr;
		const bool ok = step(hipMalloc(q, bytes), "hipMalloc");
		if (ok) e->allocs.push_back(*q);
		return ok;
	};
	if (!step(hipSetDevice(device), "hipSetDevice") || !step(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking), "hipStreamCreateWithFlags") ||
	    !step(hipEventCreate(&e->ev0), "hipEventCreate") || !step(hipEventCreate(&e->ev1), "hipEventCreate"))
		return bail(CRD_EHIP);
	void *q = nullptr;
	if (!device_alloc(2 * points * sizeof(double), &e->stage) || !device_alloc((size_t)n_members * sizeof(double), &q)) return bail(CRD_ENOMEM);
	e->max_dev = static_cast<double *>(q);
	if (!step(hipHostMalloc((void **)&e->max_host, (size_t)n_members * sizeof(double), hipHostMallocPortable), "hipHostMalloc")) return bail(CRD_ENOMEM);

	e->members.resize((size_t)n_members);
	for (int k = 0; k < n_members; k++) {
		EnsembleMember &m = e->members[(size_t)k];
		m = EnsembleMember{};
		// two state buffers, each both fields: u then v, nx * ny reals apiece
		for (int b = 0; b < 2; b++) {
			if (!device_alloc(2 * plane, &q)) return bail(e->err.empty() ? CRD_ENOMEM : CRD_EHIP);
			if (!step(hipMemsetAsync(q, 0, 2 * plane, e->stream), "hipMemsetAsync")) return bail(CRD_EHIP);
			m.u[b] = q;
			m.v[b] = static_cast<char *>(q) + plane;
		}
		Coefficients co;
		std::vector<double> brow;
		build_step_tables(members[k], e->g, -kGhost, e->g.ny + kGhost, &co, &brow);
		void *tables[4] = {nullptr, nullptr, nullptr, nullptr};
		const std::vector<double> *src[4] = {&co.cE, &co.cWn, &co.cP, &brow};
		for (int t = 0; t < 4; t++) {
			const hipError_t r = upload_reals(e->precision, *src[t], &tables[t]);
			if (tables[t]) e->allocs.push_back(tables[t]);
			if (!step(r, "table upload")) return bail(r == hipErrorOutOfMemory ? CRD_ENOMEM : CRD_EHIP);
		}
		m.cE = tables[0];
		m.cWn = tables[1];
		m.cP = tables[2];
		m.brow = tables[3];
		m.t_boundary = members[k].t_boundary;
	}
	if (!step(hipMalloc((void **)&e->table, (size_t)n_members * sizeof(EnsembleMember)), "hipMalloc(table)") ||
	    !step(hipMemcpy(e->table, e->members.data(), (size_t)n_members * sizeof(EnsembleMember), hipMemcpyHostToDevice), "hipMemcpy(table)"))
		return bail(CRD_EHIP);
	if (!step(ensemble_plan(e->precision, e->model, e->nx, e->ny, n_members, &e->plan), "ensemble_plan") ||
	    !step(hipStreamSynchronize(e->stream), "device initialisation"))
		return bail(CRD_EHIP);
	*out = e;
	return CRD_OK;
}

void crd_ensemble_destroy(crd_ensemble *e)
{
	if (!e) return;
	(void)hipSetDevice(e->device);
	if (e->stream) (void)hipStreamSynchronize(e->stream);
	for (void *q : e->allocs) (void)hipFree(q);
	if (e->table) (void)hipFree(e->table);
	if (e->max_host) (void)hipHostFree(e->max_host);
	for (hipEvent_t ev : {e->ev0, e->ev1})
		if (ev) (void)hipEventDestroy(ev);
	if (e->stream) (void)hipStreamDestroy(e->stream);
	(void)hipGetLastError();
	delete e;
}

const char *crd_ensemble_last_error(const crd_ensemble *e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int crd_ensemble_info(const crd_ensemble *e, int *n_members, crd_grid *g)
{
	if (!e) return CRD_EINVAL;
	if (n_members) *n_members = e->n;
	if (g) *g = e->g;
	return CRD_OK;
}

int crd_ensemble_upload(crd_ensemble *e, int member, const void *y, int host_is_f64)
{
	if (!e || !y) return CRD_EINVAL;
	if (int rc = check_member(e, member)) return rc;
	if (e->precision == CRD_PRECISION_F64 && !host_is_f64) return efail(e, CRD_EINVAL, "an fp64 ensemble takes double host buffers");
	TraceRange range("crd_ensemble_upload");
	ENS_TRY(e, hipSetDevice(e->device));
	const size_t points = (size_t)e->nx * (size_t)e->ny;
	const EnsembleMember &m = e->members[(size_t)member];
	ENS_TRY(e, hipMemcpyAsync(e->stage, y, 2 * points * (host_is_f64 ? 8 : 4), hipMemcpyHostToDevice, e->stream));
	ENS_TRY(e, launch_ensemble_aos_to_planes(e->precision, host_is_f64, e->stage, m.u[e->cur], m.v[e->cur], points, e->stream));
	ENS_TRY(e, hipStreamSynchronize(e->stream));
	return CRD_OK;
}

int crd_ensemble_download(crd_ensemble *e, int member, void *y, int host_is_f64)
{
	if (!e || !y) return CRD_EINVAL;
	if (int rc = check_member(e, member)) return rc;
	if (e->precision == CRD_PRECISION_F64 && !host_is_f64) return efail(e, CRD_EINVAL, "an fp64 ensemble fills double host buffers");
	TraceRange range("crd_ensemble_download");
	ENS_TRY(e, hipSetDevice(e->device));
	const size_t points = (size_t)e->nx * (size_t)e->ny;
	const EnsembleMember &m = e->members[(size_t)member];
	ENS_TRY(e, launch_ensemble_planes_to_aos(e->precision, host_is_f64, m.u[e->cur], m.v[e->cur], e->stage, points, e->stream));
	ENS_TRY(e, hipMemcpyAsync(y, e->stage, 2 * points * (host_is_f64 ? 8 : 4), hipMemcpyDeviceToHost, e->stream));
	ENS_TRY(e, hipStreamSynchronize(e->stream));
	return CRD_OK;
}

int crd_ensemble_step_rk4(crd_ensemble *e, double t0, double dt, int64_t nsteps)
{
	if (!e) return CRD_EINVAL;
	if (nsteps < 0 || !(dt > 0.0) || !std::isfinite(t0)) return efail(e, CRD_EINVAL, "bad t0 / dt / nsteps");
	TraceRange range("crd_ensemble_step_rk4");
	ENS_TRY(e, hipSetDevice(e->device));
	EnsembleStep st{};
	// the step's constants as launch_fused_t forms them
	st.h1 = dt;
	st.h2 = 0.5 * dt;
	st.h3 = dt / 3.0;
	st.h6 = dt / 6.0;
	st.ka4 = std::pow(kGbKa, 4.0);  // pow(KA, p), src/GoldbeterModel_torus.cpp:695
	st.nx = e->nx;
	st.ny = e->ny;
	st.nstrips = e->plan.nstrips;
	st.sw = e->plan.sw;
	st.nsb = e->plan.nsb;
	st.chunk = e->plan.chunk;
	st.nchunks = e->plan.nchunks;
	st.member_blocks = st.nsb * st.nchunks;
	st.nblocks = st.member_blocks * e->n;
	const double cs[4] = {0.0, 0.5, 0.5, 1.0};
	double latest_boundary = -INFINITY;  // the absorbing rows are on at stage time t exactly when t < some member's tBoundary
	for (const crd_params &p : e->p) latest_boundary = std::max(latest_boundary, p.t_boundary);
	for (int64_t s = 0; s < nsteps; s++) {
		const double t = t0 + (double)s * dt;  // as run_steps forms it
		bool absorb = false;
		for (int k = 0; k < 4; k++) {
			st.t_stage[k] = t + cs[k] * dt;  // as make_fused_call forms it
			absorb = absorb || st.t_stage[k] < latest_boundary;
		}
		st.src = e->cur;
		ENS_TRY(e, launch_ensemble_step(e->precision, e->model, e->plan.cols, absorb && e->model != dev::kModelDiffusionOnly, e->table, st, e->stream));
		e->cur = 1 - e->cur;
	}
	return CRD_OK;
}

int crd_ensemble_step_rk4_timed(crd_ensemble *e, double t0, double dt, int64_t nsteps, double *ms_total)
{
	if (!e) return CRD_EINVAL;
	ENS_TRY(e, hipSetDevice(e->device));
	ENS_TRY(e, hipEventRecord(e->ev0, e->stream));
	if (int rc = crd_ensemble_step_rk4(e, t0, dt, nsteps)) return rc;
	ENS_TRY(e, hipEventRecord(e->ev1, e->stream));
	ENS_TRY(e, hipEventSynchronize(e->ev1));
	float ms = 0.f;
	ENS_TRY(e, hipEventElapsedTime(&ms, e->ev0, e->ev1));
	if (ms_total) *ms_total = ms;
	return CRD_OK;
}

int crd_ensemble_synchronize(crd_ensemble *e)
{
	if (!e) return CRD_EINVAL;
	ENS_TRY(e, hipSetDevice(e->device));
	ENS_TRY(e, hipStreamSynchronize(e->stream));
	return CRD_OK;
}

int crd_ensemble_max_abs(crd_ensemble *e, double *per_member)
{
	if (!e || !per_member) return CRD_EINVAL;
	ENS_TRY(e, hipSetDevice(e->device));
	ENS_TRY(e, launch_ensemble_max_abs(e->precision, e->table, e->n, e->cur, (size_t)e->nx * (size_t)e->ny, e->max_dev, e->stream));
	ENS_TRY(e, hipMemcpyAsync(e->max_host, e->max_dev, (size_t)e->n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
	ENS_TRY(e, hipStreamSynchronize(e->stream));
	for (int k = 0; k < e->n; k++) per_member[k] = e->max_host[k];
	return CRD_OK;
}

}  // extern "C"
