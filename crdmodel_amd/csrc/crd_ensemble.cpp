// crd_ensemble.cpp -- ensembles behind the C ABI (include/crd.h, crd_ensemble_*): B independent single-slab problems of one geometry,
// stepped by one launch per RK4 step (crd_ensemble.hip).  Host code only.  A member owns its tables and two state buffers; the
// members' descriptors sit in a device table the step kernel reads.  crd_ensemble_create_mixed lets the members differ in surface and
// grid: each has its own crd_grid; where nx or ny truly differ (`mixed`) the fixed steps and the basic observer go through the
// per-member block mapping (crd_ensemble_mixed.hip, crd_ensemble_mixed_multi.hip), and everything else is refused.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "crd_arkode.h"
#include "crd_ctx.h"
#include "crd_device.h"
#include "crd_ensemble.h"

using namespace crd;

struct crd_ensemble {
	std::vector<crd_params> p;
	crd_grid g{};
	int n = 0, device = 0, precision = CRD_PRECISION_F64, model = CRD_MODEL_FHN;  // model: kernel_model's (diffusion-only is its own)
	int nx = 0, ny = 0;                    // member 0's (every member's unless `mixed`)
	std::vector<crd_grid> grids;           // every member's own grid
	bool mixed = false;                    // members differ in nx or ny (crd_ensemble_create_mixed only)
	size_t max_points = 0;                 // nx * ny of the largest member
	int min_ny = 0;
	std::vector<EnsembleShape> shapes, pair_shapes;  // mixed: the members' shapes under the step plan and under the pair plan (n + 1 entries)
	EnsembleShape *shapes_dev = nullptr, *pair_shapes_dev = nullptr;  // ... on the device (in allocs)
	size_t real_size = 8;
	EnsemblePlan plan;
	int steps_per_launch = 1;              // crd_ensemble_set_steps_per_launch: 1, or 2 (pairs, crd_ensemble_multi.hip)
	bool pair_planned = false;
	EnsemblePlan pair_plan;                // the pair launches' plan: fixed at the first crd_ensemble_set_steps_per_launch(e, 2)
	std::vector<EnsembleMember> members;   // host copy of the descriptor table
	EnsembleMember *table = nullptr;       // ... on the device
	std::vector<void *> allocs;            // every device allocation but the table
	int cur = 0;                           // the buffer holding every member's current state
	void *stage = nullptr;                 // AoS staging of upload / download (nx * ny pairs of doubles of the largest member)
	double *max_dev = nullptr, *max_host = nullptr;  // n doubles each; max_host page-locked
	hipStream_t stream = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	std::string err;

	// Error-controlled integration (crd_ensemble_integrate_adaptive): allocated at the first such call, empty before.
	struct Adaptive {
		void *buf[5];             // the member's five state buffers: its two (EnsembleMember::u) and three for the dense output
		void *role[5];            // buffer of each role (arkode::Y .. OUT), as a context's planes; role[Y] is the state handed back
		arkode::Memory ark;       // the controller's memory between calls (crd_ctx::ark)
		arkode::Dense dense;      // the finished step a next call may resume from (crd_ctx::dense)
	};
	std::vector<Adaptive> adapt;
	EnsemblePlan aplan;                        // the attempt kernel's plan: fixed at the first adaptive call
	double *partials = nullptr;                // n x member_items error partials
	double *ydd_partials = nullptr;            // n x kEnsembleNormBlocks
	double *sums_dev = nullptr, *sums_host = nullptr;  // n doubles each; sums_host page-locked
	EnsembleAttempt *att_dev = nullptr, *att_host = nullptr;  // n entries each; att_host page-locked
	EnsembleOp *ops_dev = nullptr, *ops_host = nullptr;  // kOpSets x n entries each; ops_host page-locked
	static constexpr int kOpSets = 3;          // batched launches enqueued between two waits, each with an operand set of its own

	// Own step sizes (crd_ensemble_step_rk4_own): allocated at the first such call, empty before.  The slot table on the device holds
	// one version at a time -- 2 (n + 1) entries: the active slots and the prefix's last entry, once per parity of the round -- and is
	// rewritten in stream order; the host keeps kOwnVersions page-locked copies, so that a version is not overwritten while its copy
	// may still be under way (after that many the stream is waited for), and beside each a copy of the member table for the call's end.
	static constexpr int kOwnVersions = 16;
	EnsembleOwnSlot *own_dev = nullptr, *own_host = nullptr;
	EnsembleMember *own_members_host = nullptr;
	int own_versions = 0;                      // versions written since the stream was last waited for

	// Observer (crd_ensemble_observe_*): empty unless one is open.
	struct Observer {
		bool open = false;
		crd_observe_options opt{};
		ObserveProbes probes{};
		int64_t capacity = 0, count = 0;       // samples: room, recorded (enqueued)
		int64_t steps = 0;                     // fixed steps taken since begin (the stride's count, carried over calls)
		int blocks = 0, row_doubles = 0;       // sampling blocks per member (mixed: of the largest; the partials' stride); doubles per member and sample: 8 + 2 n_probes
		size_t map_plane = 0;                  // doubles per map plane (nx * ny of the largest member, rounded up to an even count: 16-byte planes)
		double *records = nullptr;             // capacity x n x row_doubles
		double *partials = nullptr;            // n x blocks x 8
		double *maps = nullptr;                // n x 3 x map_plane (minimum, maximum, activation time), or null
		std::vector<double> t;                 // the samples' times
		// sections and cycle maps (crd_ensemble_observe_begin_with): none unless asked for
		ObserveSections sections{};            // kinds, indices, lengths, blocks; out[] is set per sample
		int64_t section_additions[kObserveMaxSections] = {};  // D of each section's bound
		size_t section_base[kObserveMaxSections] = {};        // section s: section_records + section_base[s], capacity x n x length x 2
		double *section_records = nullptr;
		bool cycles = false;
		double cycle_threshold = 0.0;
		double *cycle_planes = nullptr;        // n x 4 x map_plane (previous var0, t_first, t_last, int32 count), or null
	} obs;
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

// The geometry a launch over `count` members (slots, attempts) takes from a plan: G is EnsembleStep or EnsembleAttemptLaunch.  shapes:
// the plan's shape table where the members differ in shape -- strips and chunks are then the members' own (the plan's are zero) and
// the launch's block count is the table's last entry.
template <typename G>
void plan_geometry(G &g, const crd_ensemble *e, const EnsemblePlan &plan, int count, const std::vector<EnsembleShape> *shapes = nullptr)
{
	g.nx = e->nx;
	g.ny = e->ny;
	g.nstrips = plan.nstrips;
	g.sw = plan.sw;
	g.nsb = plan.nsb;
	g.chunk = plan.chunk;
	g.nchunks = plan.nchunks;
	g.member_blocks = plan.nsb * plan.nchunks;
	g.nblocks = shapes ? (*shapes)[(size_t)count].first_block : g.member_blocks * count;
}

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

// The first field in which member k differs from member 0 where members of a mixed-geometry ensemble must agree, or nullptr.
const char *mixed_disagreement(const crd_params &a, const crd_params &b)
{
	if (a.model != b.model) return "model";
	if (a.precision != b.precision) return "precision";
	if (a.just_diffusion != b.just_diffusion) return "just_diffusion";
	return nullptr;
}

size_t member_points(const crd_ensemble *e, int member) { return (size_t)e->grids[(size_t)member].nx * (size_t)e->grids[(size_t)member].ny; }

// the reaction block of a diffusion-only run is skipped, absorbing rows included: no launch of it takes the instantiation with the selects
bool can_absorb(const crd_ensemble *e) { return e->model != dev::kModelDiffusionOnly; }

// The fixed steps go on from the states handed back, not from the integrator's own (run_steps): no member has anything to resume.
void drop_adaptive(crd_ensemble *e) { for (auto &a : e->adapt) arkode::drop(a.dense, a.ark); }

// `call` between the ensemble's two timing events: its elapsed time on the stream in *ms_total (the *_timed entry points).
template <typename Call>
int timed_call(crd_ensemble *e, double *ms_total, Call call)
{
	if (!e) return CRD_EINVAL;
	ENS_TRY(e, hipSetDevice(e->device));
	ENS_TRY(e, hipEventRecord(e->ev0, e->stream));
	if (int rc = call()) return rc;
	ENS_TRY(e, hipEventRecord(e->ev1, e->stream));
	ENS_TRY(e, hipEventSynchronize(e->ev1));
	float ms = 0.f;
	ENS_TRY(e, hipEventElapsedTime(&ms, e->ev0, e->ev1));
	if (ms_total) *ms_total = ms;
	return CRD_OK;
}

constexpr const char *kMixedRefusal = "members of different shape";

int check_member(crd_ensemble *e, int member)
{
	if (member < 0 || member >= e->n) return efail(e, CRD_EINVAL, "member index out of range");
	return CRD_OK;
}

void observer_release(crd_ensemble *e)
{
	for (void *q : {(void *)e->obs.records, (void *)e->obs.partials, (void *)e->obs.maps, (void *)e->obs.section_records, (void *)e->obs.cycle_planes})
		if (q) (void)hipFree(q);
	e->obs = crd_ensemble::Observer{};
}

// Sample `sample`'s lines of section s: n members x length x 2 doubles.
double *section_lines(crd_ensemble *e, int s, int64_t sample)
{
	return e->obs.section_records + e->obs.section_base[s] + (size_t)sample * (size_t)e->n * (size_t)e->obs.sections.length[s] * 2;
}

// One sample of every member's current state at time t, behind whatever the stream holds: the sampling pass, then the finishing
// launch into the sample's rows.  The caller has checked that there is room.
int observer_sample(crd_ensemble *e, double t)
{
	crd_ensemble::Observer &ob = e->obs;
	const size_t n = (size_t)e->nx * (size_t)e->ny;
	double *const row = ob.records + (size_t)ob.count * (size_t)e->n * (size_t)ob.row_doubles;
	if (e->mixed) {  // (no sections, no cycle maps: refused when the observer was opened)
		ENS_TRY(e, launch_observe_sample_mixed(e->precision, e->table, e->shapes_dev, e->n, e->cur, ob.blocks, ob.partials, ob.maps, ob.map_plane, ob.opt.threshold, t, e->stream));
		ENS_TRY(e, launch_observe_finish_mixed(e->precision, e->table, e->shapes_dev, e->n, e->cur, ob.blocks, ob.partials, ob.probes, row, ob.row_doubles, e->stream));
		ob.t.push_back(t);
		ob.count++;
		return CRD_OK;
	}
	if (ob.cycles) {
		const ObserveCycles cy{ob.cycle_planes, ob.map_plane, ob.cycle_threshold, ob.t.empty() ? 0.0 : ob.t.back(), ob.t.empty() ? 1 : 0};
		ENS_TRY(e, launch_observe_sample_cycles(e->precision, e->table, e->n, e->cur, n, ob.partials, ob.maps, ob.map_plane, ob.opt.threshold, t, cy, e->stream));
	} else {
		ENS_TRY(e, launch_observe_sample(e->precision, e->table, e->n, e->cur, n, ob.partials, ob.maps, ob.map_plane, ob.opt.threshold, t, e->stream));
	}
	ENS_TRY(e, launch_observe_finish(e->precision, e->table, e->n, e->cur, n, ob.partials, ob.probes, e->nx, row, ob.row_doubles, e->stream));
	if (ob.sections.n > 0) {
		for (int s = 0; s < ob.sections.n; s++) ob.sections.out[s] = section_lines(e, s, ob.count);
		ENS_TRY(e, launch_observe_sections(e->precision, e->table, e->n, e->cur, e->nx, e->ny, ob.sections, e->stream));
	}
	ob.t.push_back(t);
	ob.count++;
	return CRD_OK;
}

void member_extents(const crd_ensemble *e, std::vector<int> *nx, std::vector<int> *ny)
{
	nx->clear();
	ny->clear();
	for (const crd_grid &g : e->grids) {
		nx->push_back((int)g.nx);
		ny->push_back((int)g.ny);
	}
}

// The first own-steps call's allocations: the slot table and its page-locked versions.
int ensure_own(crd_ensemble *e)
{
	if (e->own_dev) return CRD_OK;
	const size_t entries = 2 * ((size_t)e->n + 1);
	void *slots = nullptr, *members = nullptr, *dev = nullptr;  // (into locals: a failure leaves the ensemble without any of them)
	hipError_t r = hipHostMalloc(&slots, crd_ensemble::kOwnVersions * entries * sizeof(EnsembleOwnSlot), hipHostMallocPortable);
	if (r == hipSuccess) r = hipHostMalloc(&members, crd_ensemble::kOwnVersions * (size_t)e->n * sizeof(EnsembleMember), hipHostMallocPortable);
	if (r == hipSuccess) r = hipMalloc(&dev, entries * sizeof(EnsembleOwnSlot));
	if (r != hipSuccess) {
		if (slots) (void)hipHostFree(slots);
		if (members) (void)hipHostFree(members);
		(void)hipGetLastError();
		return efail(e, r == hipErrorOutOfMemory ? CRD_ENOMEM : CRD_EHIP, std::string("own-steps tables: ") + hipGetErrorString(r));
	}
	e->allocs.push_back(dev);
	e->own_host = static_cast<EnsembleOwnSlot *>(slots);
	e->own_members_host = static_cast<EnsembleMember *>(members);
	e->own_dev = static_cast<EnsembleOwnSlot *>(dev);
	e->own_versions = 0;
	return CRD_OK;
}

// crd_ensemble_create (mixed_entry false: members of one geometry, today's refusals and messages) and crd_ensemble_create_mixed
// (members agree on model, precision and just_diffusion only).
int create_ensemble(const crd_params *members, int n_members, int device, bool mixed_entry, crd_ensemble **out)
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
		if (mixed_entry) {
			if (const char *f = mixed_disagreement(members[0], members[k]))
				return efail(nullptr, CRD_EINVAL, "member " + std::to_string(k) + " differs from member 0 in " + f + " (members of a mixed-geometry ensemble must agree on model, precision and just_diffusion)");
		} else if (const char *f = disagreement(members[0], grids[0], members[k], grids[(size_t)k])) {
			return efail(nullptr, CRD_EINVAL, "member " + std::to_string(k) + " differs from member 0 in " + f + " (members may differ in diffusion, beta, beta_min, beta_max, vary_beta and t_boundary only)");
		}
	}
	bool mixed = false;
	if (mixed_entry) {
		// (block ids are 32-bit: at most one block per strip of 48 columns -- the pairs' -- and chunk of 4 rows, over all members together)
		long blocks = 0;
		for (int k = 0; k < n_members; k++) {
			const crd_grid &g = grids[(size_t)k];
			if (g.ny < 2 * kStepHalo)
				return efail(nullptr, CRD_EINVAL, "member " + std::to_string(k) + " has ny = " + std::to_string(g.ny) + " rows: every member needs at least 8 rows");
			if (g.ny > INT32_MAX / 2) return efail(nullptr, CRD_EINVAL, "member " + std::to_string(k) + " is too tall (ny = " + std::to_string(g.ny) + ")");
			if (g.nx > INT32_MAX / 2) return efail(nullptr, CRD_EINVAL, "member " + std::to_string(k) + " is too wide (nx = " + std::to_string(g.nx) + ")");
			blocks += (long)((g.nx + 47) / 48) * (long)((g.ny + 3) / 4);
			if (blocks > INT32_MAX)
				return efail(nullptr, CRD_EINVAL, "member " + std::to_string(k) + ": with its nx = " + std::to_string(g.nx) + " and ny = " + std::to_string(g.ny) +
				                                      " the block ids of members 0 .. " + std::to_string(k) + " together overflow 32 bits (too many work items for one launch)");
			mixed = mixed || g.nx != grids[0].nx || g.ny != grids[0].ny;
		}
	} else {
		if (grids[0].ny < 2 * kStepHalo) return efail(nullptr, CRD_EINVAL, "every member needs at least 8 rows");
		if (grids[0].ny > INT32_MAX / 2) return efail(nullptr, CRD_EINVAL, "members too tall");
	}
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
	e->grids = grids;
	e->mixed = mixed;
	e->n = n_members;
	e->device = device;
	e->precision = members[0].precision;
	e->real_size = e->precision == CRD_PRECISION_F64 ? 8 : 4;
	e->nx = (int)e->g.nx;
	e->ny = (int)e->g.ny;
	e->min_ny = e->ny;
	for (int k = 0; k < n_members; k++) {
		e->max_points = std::max(e->max_points, member_points(e, k));
		e->min_ny = std::min(e->min_ny, (int)grids[(size_t)k].ny);
	}
	e->model = (members[0].model == CRD_MODEL_GOLDBETER && members[0].just_diffusion) ? dev::kModelDiffusionOnly : members[0].model;
	// (block ids are 32-bit: at most one block per strip of 56 columns and chunk of 4 rows per member)
	if (!mixed_entry && (long)n_members * ((e->nx + 55) / 56) * ((e->ny + 3) / 4) > INT32_MAX) return bail(efail(e, CRD_EINVAL, "too many work items for one launch"));

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
	if (!device_alloc(2 * e->max_points * sizeof(double), &e->stage) || !device_alloc((size_t)n_members * sizeof(double), &q)) return bail(CRD_ENOMEM);
	e->max_dev = static_cast<double *>(q);
	if (!step(hipHostMalloc((void **)&e->max_host, (size_t)n_members * sizeof(double), hipHostMallocPortable), "hipHostMalloc")) return bail(CRD_ENOMEM);

	e->members.resize((size_t)n_members);
	for (int k = 0; k < n_members; k++) {
		EnsembleMember &m = e->members[(size_t)k];
		m = EnsembleMember{};
		const crd_grid &gk = e->grids[(size_t)k];
		const size_t plane = member_points(e, k) * e->real_size;
		// two state buffers, each both fields: u then v, nx * ny reals apiece
		for (int b = 0; b < 2; b++) {
			if (!device_alloc(2 * plane, &q)) return bail(e->err.empty() ? CRD_ENOMEM : CRD_EHIP);
			if (!step(hipMemsetAsync(q, 0, 2 * plane, e->stream), "hipMemsetAsync")) return bail(CRD_EHIP);
			m.u[b] = q;
			m.v[b] = static_cast<char *>(q) + plane;
		}
		Coefficients co;
		std::vector<double> brow;
		build_step_tables(members[k], gk, -kGhost, gk.ny + kGhost, &co, &brow);  // (the member's own grid: its surface, lengths and mesh)
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
	if (e->mixed) {
		std::vector<int> nxs, nys;
		member_extents(e, &nxs, &nys);
		e->shapes.resize((size_t)n_members + 1);
		if (!step(ensemble_plan_mixed(e->precision, e->model, nxs.data(), nys.data(), n_members, &e->plan, e->shapes.data()), "ensemble_plan_mixed")) return bail(CRD_EHIP);
		if (const int k = mixed_overflow_member(e->shapes.data(), n_members); k >= 0)  // (refused above on a coarser count: not reached)
			return bail(efail(e, CRD_EINVAL, "too many work items for one launch: the block ids overflow 32 bits at member " + std::to_string(k)));
		if (!device_alloc(e->shapes.size() * sizeof(EnsembleShape), &q)) return bail(CRD_ENOMEM);
		e->shapes_dev = static_cast<EnsembleShape *>(q);
		if (!step(hipMemcpy(e->shapes_dev, e->shapes.data(), e->shapes.size() * sizeof(EnsembleShape), hipMemcpyHostToDevice), "hipMemcpy(shapes)")) return bail(CRD_EHIP);
	} else if (!step(ensemble_plan(e->precision, e->model, e->nx, e->ny, n_members, &e->plan), "ensemble_plan")) {
		return bail(CRD_EHIP);
	}
	if (!step(hipStreamSynchronize(e->stream), "device initialisation")) return bail(CRD_EHIP);
	*out = e;
	return CRD_OK;
}

}  // namespace

extern "C" {

int crd_ensemble_create(const crd_params *members, int n_members, int device, crd_ensemble **out) { return create_ensemble(members, n_members, device, false, out); }

int crd_ensemble_create_mixed(const crd_params *members, int n_members, int device, crd_ensemble **out) { return create_ensemble(members, n_members, device, true, out); }

void crd_ensemble_destroy(crd_ensemble *e)
{
	if (!e) return;
	(void)hipSetDevice(e->device);
	if (e->stream) (void)hipStreamSynchronize(e->stream);
	observer_release(e);
	for (void *q : e->allocs) (void)hipFree(q);
	if (e->table) (void)hipFree(e->table);
	if (e->max_host) (void)hipHostFree(e->max_host);
	for (void *q : {(void *)e->sums_host, (void *)e->att_host, (void *)e->ops_host, (void *)e->own_host, (void *)e->own_members_host})
		if (q) (void)hipHostFree(q);
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

int crd_ensemble_member_grid(const crd_ensemble *e, int member, crd_grid *g)
{
	if (!e || !g || member < 0 || member >= e->n) return CRD_EINVAL;
	*g = e->grids[(size_t)member];
	return CRD_OK;
}

int crd_ensemble_upload(crd_ensemble *e, int member, const void *y, int host_is_f64)
{
	if (!e || !y) return CRD_EINVAL;
	if (int rc = check_member(e, member)) return rc;
	if (e->precision == CRD_PRECISION_F64 && !host_is_f64) return efail(e, CRD_EINVAL, "an fp64 ensemble takes double host buffers");
	TraceRange range("crd_ensemble_upload");
	ENS_TRY(e, hipSetDevice(e->device));
	const size_t points = member_points(e, member);
	const EnsembleMember &m = e->members[(size_t)member];
	ENS_TRY(e, hipMemcpyAsync(e->stage, y, 2 * points * (host_is_f64 ? 8 : 4), hipMemcpyHostToDevice, e->stream));
	if (!e->adapt.empty()) arkode::drop(e->adapt[(size_t)member].dense, e->adapt[(size_t)member].ark);  // this member starts afresh
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
	const size_t points = member_points(e, member);
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
	crd_ensemble::Observer &ob = e->obs;
	if (ob.open) {  // a call that would overrun the record buffer is refused whole
		const int64_t stride = ob.opt.stride, samples = (ob.steps + nsteps) / stride - ob.steps / stride;
		if (samples > ob.capacity - ob.count)
			return efail(e, CRD_EINVAL, "the observer has room for " + std::to_string(ob.capacity - ob.count) + " more samples; this call would record " + std::to_string(samples));
	}
	TraceRange range("crd_ensemble_step_rk4");
	drop_adaptive(e);
	ENS_TRY(e, hipSetDevice(e->device));
	EnsembleStep st{};
	const step::Sizes hs(dt);
	st.h1 = hs.h[0];
	st.h2 = hs.h[1];
	st.h3 = hs.h[2];
	st.h6 = hs.h[3];
	st.ka4 = std::pow(kGbKa, 4.0);  // pow(KA, p), src/GoldbeterModel_torus.cpp:695
	plan_geometry(st, e, e->plan, e->n, e->mixed ? &e->shapes : nullptr);
	const bool pairs = e->steps_per_launch == 2;
	EnsemblePair pr{};  // the same constants on the pair launches' own plan
	if (pairs) {
		pr.step = st;
		plan_geometry(pr.step, e, e->pair_plan, e->n, e->mixed ? &e->pair_shapes : nullptr);
	}
	double latest_boundary = -INFINITY;  // the absorbing rows are on at stage time t exactly when t < some member's tBoundary
	for (const crd_params &p : e->p) latest_boundary = std::max(latest_boundary, p.t_boundary);
	// the stage times of a step at t, which the kernel compares with each member's tBoundary; true: some member has its absorbing rows on
	auto stage_times = [&](double t, double *ts) {
		bool any = false;
		for (int k = 0; k < 4; k++) any = step::absorbing_at(ts[k] = step::stage_time(t, dt, k), latest_boundary) || any;
		return any && can_absorb(e);
	};
	for (int64_t s = 0; s < nsteps;) {
		bool absorb = stage_times(t0 + (double)s * dt, st.t_stage);  // (the step's time as run_steps forms it)
		// Two steps in one launch where the setting asks for pairs, two steps are left, and -- an observer open -- the first of them does
		// not complete a stride: a pair never straddles a sample.
		int taken = 1;
		if (pairs && s + 2 <= nsteps && !(ob.open && (ob.steps + 1) % ob.opt.stride == 0)) {
			std::copy(st.t_stage, st.t_stage + 4, pr.step.t_stage);
			absorb = stage_times(t0 + (double)(s + 1) * dt, pr.t_stage2) || absorb;  // the second step's t as the next single step's is formed
			pr.step.src = e->cur;
			if (e->mixed) ENS_TRY(e, launch_ensemble_pair_mixed(e->precision, e->model, e->pair_plan.cols, absorb, e->table, e->pair_shapes_dev, e->n, e->min_ny, pr, e->stream));
			else ENS_TRY(e, launch_ensemble_pair(e->precision, e->model, e->pair_plan.cols, absorb, e->table, pr, e->stream));
			taken = 2;
		} else {
			st.src = e->cur;
			if (e->mixed) ENS_TRY(e, launch_ensemble_step_mixed(e->precision, e->model, e->plan.cols, absorb, e->table, e->shapes_dev, e->n, st, e->stream));
			else ENS_TRY(e, launch_ensemble_step(e->precision, e->model, e->plan.cols, absorb, e->table, st, e->stream));
		}
		e->cur = 1 - e->cur;  // (a pair flips once: its first step's state never reaches memory)
		s += taken;
		if (ob.open && (ob.steps += taken) % ob.opt.stride == 0)
			if (int rc = observer_sample(e, t0 + (double)s * dt)) return rc;  // the time as the next step's t is formed
	}
	return CRD_OK;
}

int crd_ensemble_set_steps_per_launch(crd_ensemble *e, int steps)
{
	if (!e) return CRD_EINVAL;
	if (steps != 1 && steps != 2) return efail(e, CRD_EINVAL, "steps per launch must be 1 or 2 (got " + std::to_string(steps) + ")");
	if (steps == 2) {
		static_assert(CRD_ENSEMBLE_PAIR_MIN_ROWS == kEnsemblePairMinRows, "crd.h states the pair kernels' bound");
		if (e->mixed) {
			for (int k = 0; k < e->n; k++)
				if (e->grids[(size_t)k].ny < kEnsemblePairMinRows)
					return efail(e, CRD_EINVAL, "two steps per launch need members of at least " + std::to_string(kEnsemblePairMinRows) + " rows (CRD_ENSEMBLE_PAIR_MIN_ROWS); member " +
					                                std::to_string(k) + " has " + std::to_string(e->grids[(size_t)k].ny));
		} else if (e->ny < kEnsemblePairMinRows)
			return efail(e, CRD_EINVAL, "two steps per launch need members of at least " + std::to_string(kEnsemblePairMinRows) + " rows (CRD_ENSEMBLE_PAIR_MIN_ROWS); these have " +
			                                std::to_string(e->ny));
#ifdef CRD_NO_ENSEMBLE_PAIRS
		return efail(e, CRD_EINVAL, "this build of libcrd carries no pair kernels (built without the check of their assembly: make KERNEL_TABLE=0)");
#else
		if (!e->pair_planned && e->mixed) {
			ENS_TRY(e, hipSetDevice(e->device));
			EnsemblePlan plan;
			std::vector<int> nxs, nys;
			member_extents(e, &nxs, &nys);
			std::vector<EnsembleShape> shapes((size_t)e->n + 1);
			ENS_TRY(e, ensemble_pair_plan_mixed(e->precision, e->model, nxs.data(), nys.data(), e->n, &plan, shapes.data()));
			if (const int k = mixed_overflow_member(shapes.data(), e->n); k >= 0)
				return efail(e, CRD_EINVAL, "too many work items for one launch: the pair launches' block ids overflow 32 bits at member " + std::to_string(k));
			void *q = nullptr;
			ENS_TRY(e, hipMalloc(&q, shapes.size() * sizeof(EnsembleShape)));
			e->allocs.push_back(q);
			ENS_TRY(e, hipMemcpy(q, shapes.data(), shapes.size() * sizeof(EnsembleShape), hipMemcpyHostToDevice));
			e->pair_shapes_dev = static_cast<EnsembleShape *>(q);
			e->pair_shapes = shapes;
			e->pair_plan = plan;
			e->pair_planned = true;
		} else if (!e->pair_planned) {
			ENS_TRY(e, hipSetDevice(e->device));
			EnsemblePlan plan;
			ENS_TRY(e, ensemble_pair_plan(e->precision, e->model, e->nx, e->ny, e->n, &plan));
			if ((long)e->n * plan.nsb * plan.nchunks > INT32_MAX) return efail(e, CRD_EINVAL, "too many work items for one launch");
			e->pair_plan = plan;
			e->pair_planned = true;
		}
#endif
	}
	e->steps_per_launch = steps;
	return CRD_OK;
}

int crd_ensemble_get_steps_per_launch(const crd_ensemble *e) { return e ? e->steps_per_launch : CRD_EINVAL; }

int crd_ensemble_step_rk4_timed(crd_ensemble *e, double t0, double dt, int64_t nsteps, double *ms_total)
{
	return timed_call(e, ms_total, [&] { return crd_ensemble_step_rk4(e, t0, dt, nsteps); });
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
	if (e->mixed) ENS_TRY(e, launch_ensemble_max_abs_mixed(e->precision, e->table, e->shapes_dev, e->n, e->cur, e->max_points, e->max_dev, e->stream));
	else ENS_TRY(e, launch_ensemble_max_abs(e->precision, e->table, e->n, e->cur, (size_t)e->nx * (size_t)e->ny, e->max_dev, e->stream));
	ENS_TRY(e, hipMemcpyAsync(e->max_host, e->max_dev, (size_t)e->n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
	ENS_TRY(e, hipStreamSynchronize(e->stream));
	for (int k = 0; k < e->n; k++) per_member[k] = e->max_host[k];
	return CRD_OK;
}

int crd_ensemble_own_steps(const crd_ensemble *e, double t0, double t1, double dt_safety, int64_t *nsteps)
{
	if (!e) return CRD_EINVAL;
	crd_ensemble *const w = const_cast<crd_ensemble *>(e);  // (the message only)
	if (!nsteps) return efail(w, CRD_EINVAL, "crd_ensemble_own_steps: null nsteps");
	if (!std::isfinite(t0) || !std::isfinite(t1)) return efail(w, CRD_EINVAL, "crd_ensemble_own_steps: t0 and t1 must be finite");
	if (!(t1 > t0)) return efail(w, CRD_EINVAL, "crd_ensemble_own_steps: t1 must lie after t0");
	if (!(dt_safety > 0.0) || !std::isfinite(dt_safety)) return efail(w, CRD_EINVAL, "crd_ensemble_own_steps: dt_safety must be positive and finite");
	for (int k = 0; k < e->n; k++) {
		const double n = std::ceil((t1 - t0) / (dt_safety * crd_stable_dt(&e->p[(size_t)k])) - 1e-12);  // crd_run's rule for a lone run
		if (!(n < 0x1p62)) return efail(w, CRD_EINVAL, "crd_ensemble_own_steps: member " + std::to_string(k) + " would take too many steps");
		nsteps[k] = n >= 1.0 ? (int64_t)n : 1;
	}
	return CRD_OK;
}

}  // extern "C"

namespace {

// crd_ensemble_step_rk4_own (dt == nullptr: member k's step size formed here, (t1 - t0) / nsteps[k]) and crd_ensemble_step_rk4_own_dt
// (given).  Everything is refused before anything is launched.
int step_own(crd_ensemble *e, double t0, double t1, const double *dt, const int64_t *nsteps, const char *where)
{
	if (!e) return CRD_EINVAL;
	const std::string w = std::string(where) + ": ";
	if (!nsteps) return efail(e, CRD_EINVAL, w + "null nsteps");
	if (!std::isfinite(t0) || !std::isfinite(t1)) return efail(e, CRD_EINVAL, w + "t0 and t1 must be finite");
	if (!(t1 > t0)) return efail(e, CRD_EINVAL, w + "t1 must lie after t0");
	const int B = e->n;
	int64_t rounds = 0;
	for (int k = 0; k < B; k++) {
		if (nsteps[k] < 1)
			return efail(e, CRD_EINVAL, w + "member " + std::to_string(k) + " has nsteps = " + std::to_string(nsteps[k]) + " (every member takes at least one step)");
		if (dt && !(dt[k] > 0.0 && std::isfinite(dt[k]))) return efail(e, CRD_EINVAL, w + "member " + std::to_string(k) + " has a step size that is not positive and finite");
		rounds = std::max(rounds, nsteps[k]);
	}
	crd_ensemble::Observer &ob = e->obs;
	if (ob.open && ob.count >= ob.capacity) return efail(e, CRD_EINVAL, "the observer has no room for this call's sample");  // refused whole
	TraceRange range(where);
	ENS_TRY(e, hipSetDevice(e->device));
	if (int rc = ensure_own(e)) return rc;
	drop_adaptive(e);

	// What the rounds share: the plan made for all B members when the ensemble was created (no re-planning as members finish).
	EnsembleStep st{};
	st.ka4 = std::pow(kGbKa, 4.0);  // pow(KA, p), src/GoldbeterModel_torus.cpp:695
	plan_geometry(st, e, e->plan, 0);  // (nblocks: the active slots', set with each slot table)
	// Per member, once: its step size (own[k].h[0]), the constants formed from it, and its blocks.
	std::vector<step::Sizes> own;
	std::vector<int> blocks;
	for (int k = 0; k < B; k++) {
		own.emplace_back(dt ? dt[k] : (t1 - t0) / (double)nsteps[k]);
		blocks.push_back(e->mixed ? e->shapes[(size_t)k].nsb * e->shapes[(size_t)k].nchunks : st.member_blocks);
	}
	const size_t version_entries = 2 * ((size_t)B + 1);
	// Round s steps every member with nsteps[k] > s, in member order.  The slot table is rewritten only when that set, or a member's
	// absorbing decision at one of its stages, differs from the round before: at most B + 1 + 3 B times a call.
	std::vector<int> active, flags, now_active, now_flags;
	bool absorb = false;
	int version = -1;  // the page-locked copy the device table was last written from
	int64_t launched = 0;  // rounds launched
	auto run_rounds = [&]() -> int {
	for (int64_t s = 0; s < rounds; s++) {
		now_active.clear();
		now_flags.clear();
		bool now_absorb = false;
		for (int k = 0; k < B; k++) {
			if (nsteps[k] <= s) continue;
			now_active.push_back(k);
			const double dt_k = own[(size_t)k].h[0];
			int f[4] = {0, 0, 0, 0};
			if (can_absorb(e)) now_absorb = step::stage_flags(t0 + (double)s * dt_k, dt_k, e->p[(size_t)k].t_boundary, 4, f) || now_absorb;  // (the step's time as run_steps forms it)
			now_flags.insert(now_flags.end(), f, f + 4);
		}
		const int count = (int)now_active.size();
		if (s == 0 || now_active != active || now_flags != flags) {
			if (e->own_versions == crd_ensemble::kOwnVersions) {  // every page-locked copy may still be waiting to be read
				ENS_TRY(e, hipStreamSynchronize(e->stream));
				e->own_versions = 0;
			}
			version = e->own_versions++;
			EnsembleOwnSlot *const host = e->own_host + (size_t)version * version_entries;
			for (int parity = 0; parity < 2; parity++) {
				EnsembleOwnSlot *const slots = host + (size_t)parity * ((size_t)count + 1);
				int first = 0;
				for (int i = 0; i < count; i++) {
					const int k = now_active[(size_t)i];
					const EnsembleMember &m = e->members[(size_t)k];
					EnsembleOwnSlot &sl = slots[i];
					sl = EnsembleOwnSlot{};
					sl.in = m.u[e->cur ^ parity];  // every active member has taken s steps: one parity for the round
					sl.out = m.u[e->cur ^ parity ^ 1];
					std::copy(own[(size_t)k].h, own[(size_t)k].h + 4, sl.h);
					std::copy(own[(size_t)k].hf, own[(size_t)k].hf + 4, sl.hf);
					std::copy(&now_flags[(size_t)(4 * i)], &now_flags[(size_t)(4 * i)] + 4, sl.absorb);
					sl.member = k;
					sl.first_block = first;
					first += blocks[(size_t)k];
				}
				slots[count] = EnsembleOwnSlot{};
				slots[count].first_block = first;
			}
			ENS_TRY(e, hipMemcpyAsync(e->own_dev, host, 2 * ((size_t)count + 1) * sizeof(EnsembleOwnSlot), hipMemcpyHostToDevice, e->stream));
			st.nblocks = host[count].first_block;
			active.swap(now_active);
			flags.swap(now_flags);
			absorb = now_absorb;
		}
		ENS_TRY(e, launch_ensemble_own_step(e->precision, e->model, e->plan.cols, absorb, e->table, e->mixed ? e->shapes_dev : nullptr,
		                                    e->own_dev + (size_t)(s & 1) * ((size_t)count + 1), count, st, e->stream));
		launched = s + 1;
	}
	return CRD_OK;
	};
	const int rounds_rc = run_rounds();
	// A member that took an odd number of steps ends in its other buffer: re-point its descriptor, so that buffer e->cur is every
	// member's current state (nothing is copied; the error-controlled path does the same).  Where a round failed to launch, for the
	// steps each member did take: the descriptors still name every member's latest state, though the members are at different times.
	bool repoint = false;
	for (int k = 0; k < B; k++)
		if (std::min(nsteps[k], launched) & 1) {
			EnsembleMember &m = e->members[(size_t)k];
			std::swap(m.u[0], m.u[1]);
			std::swap(m.v[0], m.v[1]);
			repoint = true;
		}
	hipError_t table_r = hipSuccess;
	if (repoint) {  // (version >= 0: a round was launched)
		EnsembleMember *const host = e->own_members_host + (size_t)version * (size_t)B;  // (beside the call's last slot version: not rewritten before the stream is waited for)
		std::copy(e->members.begin(), e->members.end(), host);
		table_r = hipMemcpyAsync(e->table, host, (size_t)B * sizeof(EnsembleMember), hipMemcpyHostToDevice, e->stream);
	}
	if (rounds_rc != CRD_OK) {
		const std::string cause = e->err;
		return efail(e, rounds_rc, w + cause + "; " + std::to_string(launched) + " of " + std::to_string(rounds) + " rounds were launched: member k has taken min(nsteps[k], " +
		                               std::to_string(launched) + ") steps, the members no longer share a time -- upload every member before stepping on" +
		                               (table_r != hipSuccess ? std::string("; the member table could not be rewritten (") + hipGetErrorString(table_r) + "): destroy the ensemble" : std::string()));
	}
	ENS_TRY(e, table_r);
	if (ob.open)
		if (int rc = observer_sample(e, t1)) return rc;  // one sample per call, at t1 (crd_ensemble_integrate_adaptive's rule); the stride's count does not move
	return CRD_OK;
}

}  // namespace

extern "C" {

int crd_ensemble_step_rk4_own(crd_ensemble *e, double t0, double t1, const int64_t *nsteps) { return step_own(e, t0, t1, nullptr, nsteps, "crd_ensemble_step_rk4_own"); }

int crd_ensemble_step_rk4_own_dt(crd_ensemble *e, double t0, double t1, const double *dt, const int64_t *nsteps)
{
	if (e && !dt) return efail(e, CRD_EINVAL, "crd_ensemble_step_rk4_own_dt: null dt");
	return step_own(e, t0, t1, dt, nsteps, "crd_ensemble_step_rk4_own_dt");
}

int crd_ensemble_step_rk4_own_timed(crd_ensemble *e, double t0, double t1, const int64_t *nsteps, double *ms_total)
{
	return timed_call(e, ms_total, [&] { return crd_ensemble_step_rk4_own(e, t0, t1, nsteps); });
}

}  // extern "C"

namespace {

// The first adaptive call's allocations: three more state buffers per member, the error partials, the per-member scalars and the
// attempt / operand tables.  An ensemble that only takes fixed steps never makes them.
int ensure_adaptive(crd_ensemble *e)
{
	if (!e->adapt.empty()) return CRD_OK;
	const size_t B = (size_t)e->n, plane = (size_t)e->nx * (size_t)e->ny * e->real_size;
	EnsemblePlan plan;
	ENS_TRY(e, ensemble_attempt_plan(e->precision, e->model, e->nx, e->ny, e->n, &plan));
	const long member_blocks = (long)plan.nsb * plan.nchunks;
	if (member_blocks * e->n > INT32_MAX) return efail(e, CRD_EINVAL, "too many work items for one attempt launch");
	const size_t member_items = (size_t)plan.nstrips * (size_t)plan.nchunks;
	std::vector<crd_ensemble::Adaptive> adapt(B);
	std::vector<void *> fresh;  // (freed again if a later allocation fails)
	auto dev_alloc = [&](size_t bytes, void **q) {
		*q = nullptr;
		const hipError_t r = hipMalloc(q, bytes);
		if (r == hipSuccess) fresh.push_back(*q);
		return r;
	};
	auto undo = [&](int rc, const std::string &what) {
		for (void *q : fresh) (void)hipFree(q);
		if (e->sums_host) (void)hipHostFree(e->sums_host);
		if (e->att_host) (void)hipHostFree(e->att_host);
		if (e->ops_host) (void)hipHostFree(e->ops_host);
		e->sums_host = nullptr;
		e->att_host = nullptr;
		e->ops_host = nullptr;
		return efail(e, rc, what);
	};
	void *q = nullptr;
	for (size_t k = 0; k < B; k++) {
		const EnsembleMember &m = e->members[k];
		adapt[k].buf[0] = m.u[e->cur];
		adapt[k].buf[1] = m.u[1 - e->cur];
		for (int b = 2; b < 5; b++) {
			if (hipError_t r = dev_alloc(2 * plane, &q); r != hipSuccess) return undo(CRD_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(r));
			adapt[k].buf[b] = q;
		}
	}
	void *p[5] = {};
	const size_t sizes[5] = {B * member_items * sizeof(double), B * kEnsembleNormBlocks * sizeof(double), B * sizeof(double), B * sizeof(EnsembleAttempt),
	                         crd_ensemble::kOpSets * B * sizeof(EnsembleOp)};
	for (int i = 0; i < 5; i++)
		if (hipError_t r = dev_alloc(sizes[i], &p[i]); r != hipSuccess) return undo(CRD_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(r));
	if (hipHostMalloc((void **)&e->sums_host, B * sizeof(double), hipHostMallocPortable) != hipSuccess ||
	    hipHostMalloc((void **)&e->att_host, B * sizeof(EnsembleAttempt), hipHostMallocPortable) != hipSuccess ||
	    hipHostMalloc((void **)&e->ops_host, crd_ensemble::kOpSets * B * sizeof(EnsembleOp), hipHostMallocPortable) != hipSuccess)
		return undo(CRD_ENOMEM, "hipHostMalloc failed");
	e->partials = static_cast<double *>(p[0]);
	e->ydd_partials = static_cast<double *>(p[1]);
	e->sums_dev = static_cast<double *>(p[2]);
	e->att_dev = static_cast<EnsembleAttempt *>(p[3]);
	e->ops_dev = static_cast<EnsembleOp *>(p[4]);
	e->allocs.insert(e->allocs.end(), fresh.begin(), fresh.end());
	e->aplan = plan;
	e->adapt = std::move(adapt);
	return CRD_OK;
}

// What one member does during one call (crd_adaptive.cpp: what AdaptiveRun keeps for a context's call).
struct MemberRun {
	crd_adaptive_stats st{};
	double t = 0.0, t_prev = 0.0, h_cap = 0.0, t_boundary = 0.0;
	arkode::Rotation rot;  // its state buffers' turns, by role
	int nef = 0, dst = -1;
	int64_t steps = 0;
	bool new_step = true, reinterpolate = false, failed = false;
	arkode::Hin hin;
	std::string why;
	// does the call end with an output for this member: has its last step (t_prev -> t) reached or passed tout?
	bool output(double tout) const { return !failed && rot.prev >= 0 && t >= tout; }
};

// Operand set `set` (0 .. kOpSets) of the batched element-wise launches: host entries, then one copy to the device.
EnsembleOp *op_set(crd_ensemble *e, int set) { return e->ops_host + (size_t)set * (size_t)e->n; }
hipError_t upload_ops(crd_ensemble *e, int set, int count)
{
	if (count <= 0) return hipSuccess;
	return hipMemcpyAsync(e->ops_dev + (size_t)set * (size_t)e->n, op_set(e, set), (size_t)count * sizeof(EnsembleOp), hipMemcpyHostToDevice, e->stream);
}
EnsembleOp make_op(int member, const void *x0, const void *x1, const void *x2, const void *x3, void *out)
{
	EnsembleOp o{};
	o.x[0] = x0;
	o.x[1] = x1;
	o.x[2] = x2;
	o.x[3] = x3;
	o.out = out;
	o.member = member;
	return o;
}
// the scalars of `count` members, written to sums_dev by work already enqueued, into sums_host (one wait)
hipError_t fetch_sums(crd_ensemble *e, int count)
{
	if (hipError_t r = hipMemcpyAsync(e->sums_host, e->sums_dev, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, e->stream); r != hipSuccess) return r;
	return hipStreamSynchronize(e->stream);
}

}  // namespace

extern "C" {

int crd_ensemble_integrate_adaptive(crd_ensemble *e, double t0, double tout, const crd_adaptive_options *opt, crd_adaptive_stats *stats, int32_t *status)
{
	if (!e) return CRD_EINVAL;
	if (e->mixed) return efail(e, CRD_EINVAL, std::string("crd_ensemble_integrate_adaptive: ") + kMixedRefusal + " integrate with fixed steps only");
	crd_adaptive_options o;
	crd_adaptive_defaults(&o);
	if (opt) o = *opt;
	if (!arkode::options_valid(o, t0, tout)) return efail(e, CRD_EINVAL, "bad adaptive options / time interval");
	if (o.method != CRD_ADAPT_ARKODE) return efail(e, CRD_EINVAL, "an ensemble integrates with CRD_ADAPT_ARKODE only");
	if (e->obs.open && e->obs.count >= e->obs.capacity) return efail(e, CRD_EINVAL, "the observer has no room for this call's sample");
	const int B = e->n;
	// Which members resume (a context's rule, per member: t0 is the output time its previous call handed back, and nothing has replaced
	// its state since), and -- before any device work -- whether a fresh member's first-step estimate can be made at all.
	std::vector<char> resume((size_t)B, 0);
	bool estimate = false;
	for (int k = 0; k < B; k++) {
		if (!e->adapt.empty()) resume[(size_t)k] = arkode::resumes(e->adapt[(size_t)k].dense, e->adapt[(size_t)k].ark, t0, true);
		estimate = estimate || (!resume[(size_t)k] && !(o.h0 > 0.0) && tout > t0);
	}
	arkode::Hin probe;
	if (estimate && !arkode::hin_start(probe, t0, tout)) return efail(e, CRD_EINVAL, arkode::kHinTooClose);
	TraceRange range("crd_ensemble_integrate_adaptive");
	ENS_TRY(e, hipSetDevice(e->device));
	if (int rc = ensure_adaptive(e)) return rc;
	const size_t points = (size_t)e->nx * (size_t)e->ny, plane = points * e->real_size;
	const double n_components = 2.0 * (double)e->nx * (double)e->ny;  // WRMS norm over the whole grid
	const double ka4 = std::pow(kGbKa, 4.0);

	std::vector<MemberRun> run((size_t)B);
	std::vector<int> hin, active;  // members that estimate their first step / that take steps
	for (int k = 0; k < B; k++) {
		MemberRun &r = run[(size_t)k];
		auto &a = e->adapt[(size_t)k];
		const crd_params &p = e->p[(size_t)k];
		r.h_cap = arkode::h_cap(o, p);  // (h_max = 0: the member's own stability bound)
		r.t_boundary = p.t_boundary;
		r.t = r.t_prev = t0;
		if (!resume[(size_t)k]) {
			// the member's state is in its descriptor's current buffer; its other four buffers are free
			void *y = e->members[(size_t)k].u[e->cur];
			a.role[arkode::Y] = y;
			int next = arkode::SA;
			for (void *b : a.buf)
				if (b != y) a.role[next++] = b;
			a.dense.pending = false;
			arkode::init(a.ark, t0, o.h0);
			if (arkode::needs_estimate(a.ark, t0, tout)) {
				arkode::hin_start(r.hin, t0, tout);
				hin.push_back(k);
			}
			continue;
		}
		r.t = a.dense.t_np1;
		if (tout <= a.dense.t_np1) {  // still inside the step already taken: that step (t_prev -> t) again, to interpolate again
			r.reinterpolate = true;
			r.t_prev = a.dense.t_n;
			r.rot.reinterpolate();
			continue;
		}
		r.rot.resume();
	}

	// arkHin of the fresh members, batched: f0 -> SB, the trial state -> SA, f(trial) -> ACC
	if (!hin.empty()) {
		const int nh = (int)hin.size();
		for (int i = 0; i < nh; i++) {
			const int k = hin[(size_t)i];
			auto &a = e->adapt[(size_t)k];
			op_set(e, 0)[i] = make_op(k, a.role[arkode::Y], nullptr, nullptr, nullptr, a.role[arkode::SB]);
			op_set(e, 0)[i].absorb = step::absorbing_at(t0, run[(size_t)k].t_boundary) ? 1 : 0;
			op_set(e, 1)[i] = make_op(k, a.role[arkode::Y], a.role[arkode::SB], nullptr, nullptr, nullptr);
		}
		ENS_TRY(e, upload_ops(e, 0, nh));
		ENS_TRY(e, upload_ops(e, 1, nh));
		ENS_TRY(e, launch_ensemble_rhs(e->precision, e->model, e->table, e->ops_dev, nh, e->nx, e->ny, ka4, e->stream));
		ENS_TRY(e, launch_ensemble_hin_bound(e->precision, e->ops_dev + B, nh, points, o.rtol, o.atol, e->sums_dev, e->stream));
		ENS_TRY(e, fetch_sums(e, nh));
		std::vector<int> open;
		for (int i = 0; i < nh; i++) {
			arkode::hin_bound(run[(size_t)hin[(size_t)i]].hin, e->sums_host[i]);
			if (!run[(size_t)hin[(size_t)i]].hin.done) open.push_back(hin[(size_t)i]);
		}
		while (!open.empty()) {
			const int no = (int)open.size();
			for (int i = 0; i < no; i++) {
				const int k = open[(size_t)i];
				auto &a = e->adapt[(size_t)k];
				const double hg = run[(size_t)k].hin.hg;
				EnsembleOp &ax = op_set(e, 0)[i];
				ax = make_op(k, a.role[arkode::Y], a.role[arkode::SB], nullptr, nullptr, a.role[arkode::SA]);
				ax.c[0] = hg;
				ax.cf[0] = (float)hg;
				op_set(e, 1)[i] = make_op(k, a.role[arkode::SA], nullptr, nullptr, nullptr, a.role[arkode::ACC]);
				op_set(e, 1)[i].absorb = step::absorbing_at(t0 + hg, run[(size_t)k].t_boundary) ? 1 : 0;
				op_set(e, 2)[i] = make_op(k, a.role[arkode::Y], a.role[arkode::SB], a.role[arkode::ACC], nullptr, nullptr);
				op_set(e, 2)[i].c[0] = 1.0 / hg;
			}
			for (int set = 0; set < 3; set++) ENS_TRY(e, upload_ops(e, set, no));
			ENS_TRY(e, launch_ensemble_axpy(e->precision, e->ops_dev, no, points, e->stream));
			ENS_TRY(e, launch_ensemble_rhs(e->precision, e->model, e->table, e->ops_dev + B, no, e->nx, e->ny, ka4, e->stream));
			ENS_TRY(e, launch_ensemble_ydd_sumsq(e->precision, e->ops_dev + 2 * B, no, points, o.rtol, o.atol, e->ydd_partials, e->sums_dev, e->stream));
			ENS_TRY(e, fetch_sums(e, no));
			std::vector<int> still;
			for (int i = 0; i < no; i++) {
				arkode::Hin &H = run[(size_t)open[(size_t)i]].hin;
				arkode::hin_ydd(H, std::sqrt(e->sums_host[i] / n_components));
				if (!H.done) still.push_back(open[(size_t)i]);
			}
			open.swap(still);
		}
		for (int k : hin) e->adapt[(size_t)k].ark.h = run[(size_t)k].hin.h0;
	}
	for (int k = 0; k < B; k++) {
		MemberRun &r = run[(size_t)k];
		if (r.reinterpolate) continue;
		auto &A = e->adapt[(size_t)k].ark;
		if (!resume[(size_t)k]) arkode::first_step(A, r.h_cap);
		r.st.h_first = arkode::first_attempt(A);
		if (r.t < tout) active.push_back(k);
	}

	// Rounds: one attempt of every active member in one launch, the per-member sums, one wait, then each member's controller.
	const EnsemblePlan &pl = e->aplan;
	EnsembleAttemptLaunch l{};
	l.rtol = o.rtol;
	l.atol = o.atol;
	l.ka4 = ka4;
	l.partials = e->partials;
	plan_geometry(l, e, pl, 0);  // (nblocks: the active members', set with each round)
	l.member_items = pl.nstrips * pl.nchunks;
	std::vector<int> slot_member;
	while (!active.empty()) {
		slot_member.clear();
		bool absorb = false;
		for (int k : active) {
			MemberRun &r = run[(size_t)k];
			auto &a = e->adapt[(size_t)k];
			if (r.new_step) {
				if (const char *why = arkode::begin_step(a.ark, r.t, r.steps, o.max_steps)) {
					r.failed = true;
					r.why = why;
					continue;
				}
				r.new_step = false;
				r.nef = 0;
				r.dst = r.rot.spare;
			}
			const step::Sizes hs(a.ark.h);
			EnsembleAttempt &at = e->att_host[slot_member.size()];
			at = EnsembleAttempt{};
			at.in = a.role[r.rot.cur];
			at.out = a.role[r.dst];
			std::copy(hs.h, hs.h + 4, at.h);
			std::copy(hs.hf, hs.hf + 4, at.hf);
			at.member = k;
			absorb = step::stage_flags(r.t, a.ark.h, r.t_boundary, 5, at.absorb) || absorb;  // the four stages and Zonneveld's fifth
			slot_member.push_back(k);
		}
		const int count = (int)slot_member.size();
		if (count > 0) {
			l.nblocks = l.member_blocks * count;
			ENS_TRY(e, hipMemcpyAsync(e->att_dev, e->att_host, (size_t)count * sizeof(EnsembleAttempt), hipMemcpyHostToDevice, e->stream));
			ENS_TRY(e, launch_ensemble_attempts(e->precision, e->model, absorb && can_absorb(e), e->table, e->att_dev, count, l, e->sums_dev, e->stream));
			ENS_TRY(e, fetch_sums(e, count));
		}
		for (int i = 0; i < count; i++) {
			const int k = slot_member[(size_t)i];
			MemberRun &r = run[(size_t)k];
			auto &A = e->adapt[(size_t)k].ark;
			const double dsm = std::sqrt(e->sums_host[i] / n_components);
			r.st.err_last = dsm;
			if (dsm <= 1.0) {  // (a NaN fails the test)
				r.t_prev = r.t;
				arkode::accept(A, dsm, o, r.h_cap, r.t, r.st);
				r.steps++;
				r.rot.accept(r.dst, true);
				r.new_step = true;
			} else if (!arkode::reject(A, dsm, &r.nef, o, r.h_cap, r.st)) {
				r.failed = true;
				r.why = arkode::kErrFailure;
			}
		}
		std::vector<int> still;
		for (int k : active)
			if (!run[(size_t)k].failed && run[(size_t)k].t < tout) still.push_back(k);
		active.swap(still);
	}

	// ARK_NORMAL output: f at both ends of each finished member's last step, then the cubic Hermite interpolant at tout (members that
	// interpolate again inside a step already taken need the interpolant only).  Three batched launches; the buffers are re-labelled.
	int nd = 0, nhm = 0;
	for (int k = 0; k < B; k++) {
		MemberRun &r = run[(size_t)k];
		auto &a = e->adapt[(size_t)k];
		if (!r.output(tout)) continue;
		const double hstep = r.t - r.t_prev;
		EnsembleOp &op = op_set(e, 2)[nhm++];
		op = make_op(k, a.role[r.rot.prev], a.role[r.rot.cur], a.role[arkode::SB], a.role[arkode::ACC], a.role[r.rot.interpolant()]);
		ensemble_hermite_coefficients((tout - r.t_prev) / hstep, hstep, op.c, op.cf);
		if (r.reinterpolate) continue;
		op_set(e, 0)[nd] = make_op(k, a.role[r.rot.prev], nullptr, nullptr, nullptr, a.role[arkode::SB]);
		op_set(e, 0)[nd].absorb = step::absorbing_at(r.t_prev, r.t_boundary) ? 1 : 0;
		op_set(e, 1)[nd] = make_op(k, a.role[r.rot.cur], nullptr, nullptr, nullptr, a.role[arkode::ACC]);
		op_set(e, 1)[nd].absorb = step::absorbing_at(r.t, r.t_boundary) ? 1 : 0;
		nd++;
	}
	for (int set = 0; set < 3; set++) ENS_TRY(e, upload_ops(e, set, set < 2 ? nd : nhm));
	ENS_TRY(e, launch_ensemble_rhs(e->precision, e->model, e->table, e->ops_dev, nd, e->nx, e->ny, ka4, e->stream));
	ENS_TRY(e, launch_ensemble_rhs(e->precision, e->model, e->table, e->ops_dev + B, nd, e->nx, e->ny, ka4, e->stream));
	ENS_TRY(e, launch_ensemble_hermite(e->precision, e->ops_dev + 2 * B, nhm, points, e->stream));

	int rc = CRD_OK;
	std::string failures;
	for (int k = 0; k < B; k++) {
		MemberRun &r = run[(size_t)k];
		auto &a = e->adapt[(size_t)k];
		// an output at tout, or -- a zero-length interval, a failure -- the state reached handed back
		arkode::end_of_call(r.rot, r.output(tout), a.dense, tout, r.t_prev, r.t).apply(a.role);
		r.st.t_internal = r.t;
		r.st.t = r.output(tout) ? tout : r.t;
		if (!r.reinterpolate) a.ark.live = !r.failed && a.dense.pending;
		r.st.h_next = a.ark.hprime;
		if (r.failed) {
			rc = CRD_ESTATE;
			failures += (failures.empty() ? "" : "; ") + std::string("member ") + std::to_string(k) + ": " + r.why;
		}
		if (stats) stats[k] = r.st;
		if (status) status[k] = r.failed ? CRD_ESTATE : CRD_OK;
		// the descriptor: the state handed back is the current buffer; the other one (overwritten only by a fixed step, which ends the
		// carry-over) the integrator's own state
		EnsembleMember &m = e->members[(size_t)k];
		m.u[e->cur] = a.role[arkode::Y];
		m.v[e->cur] = static_cast<char *>(a.role[arkode::Y]) + plane;
		m.u[1 - e->cur] = a.role[arkode::SA];
		m.v[1 - e->cur] = static_cast<char *>(a.role[arkode::SA]) + plane;
	}
	ENS_TRY(e, hipMemcpyAsync(e->table, e->members.data(), (size_t)B * sizeof(EnsembleMember), hipMemcpyHostToDevice, e->stream));
	if (e->obs.open) {
		// one sample per call, of the states handed back; a member that failed gets a row of NaNs (every byte 0xff is one)
		const int64_t sample = e->obs.count;
		double *const row = e->obs.records + (size_t)sample * (size_t)B * (size_t)e->obs.row_doubles;
		if (int orc = observer_sample(e, tout)) return orc;
		for (int k = 0; k < B; k++)
			if (run[(size_t)k].failed) {
				ENS_TRY(e, hipMemsetAsync(row + (size_t)k * (size_t)e->obs.row_doubles, 0xff, (size_t)e->obs.row_doubles * sizeof(double), e->stream));
				for (int s = 0; s < e->obs.sections.n; s++) {  // ... and lines of NaNs
					const size_t line = (size_t)e->obs.sections.length[s] * 2;
					ENS_TRY(e, hipMemsetAsync(section_lines(e, s, sample) + (size_t)k * line, 0xff, line * sizeof(double), e->stream));
				}
			}
	}
	ENS_TRY(e, hipStreamSynchronize(e->stream));
	if (rc != CRD_OK) return efail(e, rc, "adaptive integration failed for " + failures);
	return CRD_OK;
}

}  // extern "C"

// ---- observers ----

extern "C" {

int crd_ensemble_observe_begin(crd_ensemble *e, const crd_observe_options *opt, int64_t capacity) { return crd_ensemble_observe_begin_with(e, opt, nullptr, capacity); }

int crd_ensemble_observe_begin_with(crd_ensemble *e, const crd_observe_options *opt, const crd_observe_extras *extras, int64_t capacity)
{
	if (!e) return CRD_EINVAL;
	if (!opt) return efail(e, CRD_EINVAL, "null observer options");
	if (e->obs.open) return efail(e, CRD_EINVAL, "an observer is already open (crd_ensemble_observe_end closes it)");
	if (opt->stride < 1) return efail(e, CRD_EINVAL, "observer stride must be at least 1 (got " + std::to_string(opt->stride) + ")");
	if (capacity < 1) return efail(e, CRD_EINVAL, "observer capacity must be at least 1 sample (got " + std::to_string(capacity) + ")");
	if (opt->n_probes < 0 || opt->n_probes > CRD_OBSERVE_MAX_PROBES)
		return efail(e, CRD_EINVAL, "an observer takes 0 .. " + std::to_string(CRD_OBSERVE_MAX_PROBES) + " probes (got " + std::to_string(opt->n_probes) + ")");
	if (e->mixed && extras && (extras->n_sections != 0 || extras->cycles != 0))
		return efail(e, CRD_EINVAL, std::string("crd_ensemble_observe_begin_with: ") + kMixedRefusal + " take " + (extras->n_sections != 0 ? "no sections" : "no cycle maps") +
		                                " (statistics, probes and maps only)");
	for (int q = 0; q < opt->n_probes; q++)
		for (int k = 0; k < (e->mixed ? e->n : 1); k++) {  // (members of one shape: member 0 stands for all, with today's message)
			const int nx = (int)e->grids[(size_t)k].nx, ny = (int)e->grids[(size_t)k].ny;
			if (opt->probe_i[q] < 0 || opt->probe_i[q] >= nx || opt->probe_j[q] < 0 || opt->probe_j[q] >= ny)
				return efail(e, CRD_EINVAL, "probe " + std::to_string(q) + " (i = " + std::to_string(opt->probe_i[q]) + ", j = " + std::to_string(opt->probe_j[q]) +
				                                ") is outside the " + std::to_string(nx) + " x " + std::to_string(ny) + " grid" + (e->mixed ? " of member " + std::to_string(k) : std::string()));
		}
	if (opt->maps != 0 && opt->maps != 1) return efail(e, CRD_EINVAL, "observer maps is 0 or 1");
	if (opt->maps && !std::isfinite(opt->threshold)) return efail(e, CRD_EINVAL, "observer maps need a finite threshold");
	static_assert(CRD_OBSERVE_MAX_PROBES == kObserveMaxProbes, "the header's probe limit is the kernels'");
	static_assert(CRD_OBSERVE_MAX_SECTIONS == kObserveMaxSections, "the header's section limit is the kernels'");
	const size_t n = e->max_points, B = (size_t)e->n;  // (the partials' stride and the map planes are sized for the largest member)
	crd_ensemble::Observer ob;
	size_t section_doubles = 0;  // of the whole section buffer
	if (extras) {
		if (extras->n_sections < 0 || extras->n_sections > CRD_OBSERVE_MAX_SECTIONS)
			return efail(e, CRD_EINVAL, "an observer takes 0 .. " + std::to_string(CRD_OBSERVE_MAX_SECTIONS) + " sections (got " + std::to_string(extras->n_sections) + ")");
		if (extras->cycles != 0 && extras->cycles != 1) return efail(e, CRD_EINVAL, "observer cycles is 0 or 1");
		if (extras->cycles && !std::isfinite(extras->cycle_threshold)) return efail(e, CRD_EINVAL, "cycle maps need a finite cycle_threshold");
		ObserveSections &sc = ob.sections;
		sc.n = extras->n_sections;
		for (int s = 0; s < sc.n; s++) {
			int blocks = 0;
			if (!observe_section_shape(e->precision, extras->kind[s], e->nx, e->ny, &sc.length[s], &blocks, &ob.section_additions[s]))
				return efail(e, CRD_EINVAL, "section " + std::to_string(s) + ": unknown kind " + std::to_string(extras->kind[s]));
			sc.kind[s] = extras->kind[s];
			sc.index[s] = 0;
			if (sc.kind[s] == CRD_SECTION_ROW || sc.kind[s] == CRD_SECTION_COLUMN) {
				const int limit = sc.kind[s] == CRD_SECTION_ROW ? e->ny : e->nx;
				if (extras->index[s] < 0 || extras->index[s] >= limit)
					return efail(e, CRD_EINVAL, "section " + std::to_string(s) + ": " + (sc.kind[s] == CRD_SECTION_ROW ? "row " : "column ") + std::to_string(extras->index[s]) +
					                                " is outside the " + std::to_string(e->nx) + " x " + std::to_string(e->ny) + " grid");
				sc.index[s] = extras->index[s];
			}
			sc.first_block[s + 1] = sc.first_block[s] + blocks;
			if ((double)capacity * (double)B * (double)sc.length[s] * 16.0 > 0x1p46) return efail(e, CRD_EINVAL, "observer capacity too large");
			ob.section_base[s] = section_doubles;
			section_doubles += (size_t)(capacity > 0 ? capacity : 0) * B * (size_t)sc.length[s] * 2;
		}
		ob.cycles = extras->cycles == 1;
		ob.cycle_threshold = extras->cycle_threshold;
	}
	ob.opt = *opt;
	ob.probes.n = opt->n_probes;
	for (int q = 0; q < opt->n_probes; q++) {
		ob.probes.i[q] = opt->probe_i[q];
		ob.probes.j[q] = opt->probe_j[q];
	}
	ob.capacity = capacity;
	ob.blocks = observe_blocks(n);
	ob.row_doubles = 8 + 2 * opt->n_probes;
	ob.map_plane = (n + 1) & ~(size_t)1;
	if ((double)capacity * (double)B * (double)ob.row_doubles * 8.0 > 0x1p46) return efail(e, CRD_EINVAL, "observer capacity too large");
	TraceRange range("crd_ensemble_observe_begin");
	ENS_TRY(e, hipSetDevice(e->device));
	e->obs = ob;  // (observer_release frees whatever a failed allocation leaves behind)
	auto fail = [&](hipError_t r, const char *what) {
		observer_release(e);
		return efail(e, r == hipErrorOutOfMemory ? CRD_ENOMEM : CRD_EHIP, std::string(what) + ": " + hipGetErrorString(r));
	};
	if (hipError_t r = hipMalloc((void **)&e->obs.records, (size_t)capacity * B * (size_t)ob.row_doubles * sizeof(double)); r != hipSuccess) return fail(r, "hipMalloc(records)");
	if (hipError_t r = hipMalloc((void **)&e->obs.partials, B * (size_t)ob.blocks * 8 * sizeof(double)); r != hipSuccess) return fail(r, "hipMalloc(partials)");
	if (opt->maps) {
		if (hipError_t r = hipMalloc((void **)&e->obs.maps, B * 3 * ob.map_plane * sizeof(double)); r != hipSuccess) return fail(r, "hipMalloc(maps)");
		for (size_t k = 0; k < B; k++) {
			const double init[3] = {INFINITY, -INFINITY, NAN};
			for (int q = 0; q < 3; q++)
				if (hipError_t r = launch_observe_fill(e->obs.maps + (k * 3 + (size_t)q) * ob.map_plane, ob.map_plane, init[q], e->stream); r != hipSuccess)
					return fail(r, "map initialisation");
		}
	}
	if (section_doubles)
		if (hipError_t r = hipMalloc((void **)&e->obs.section_records, section_doubles * sizeof(double)); r != hipSuccess) return fail(r, "hipMalloc(section records)");
	if (ob.cycles) {
		if (hipError_t r = hipMalloc((void **)&e->obs.cycle_planes, B * 4 * ob.map_plane * sizeof(double)); r != hipSuccess) return fail(r, "hipMalloc(cycle planes)");
		for (size_t k = 0; k < B; k++) {  // previous var0: anything (the first sample stores it); t_first, t_last: NaN; count: 0
			double *const planes = e->obs.cycle_planes + k * 4 * ob.map_plane;
			if (hipError_t r = launch_observe_fill(planes + ob.map_plane, 2 * ob.map_plane, NAN, e->stream); r != hipSuccess) return fail(r, "cycle map initialisation");
			if (hipError_t r = hipMemsetAsync(planes, 0, ob.map_plane * sizeof(double), e->stream); r != hipSuccess) return fail(r, "cycle map initialisation");
			if (hipError_t r = hipMemsetAsync(planes + 3 * ob.map_plane, 0, ob.map_plane * sizeof(double), e->stream); r != hipSuccess) return fail(r, "cycle map initialisation");
		}
	}
	e->obs.open = true;
	return CRD_OK;
}

int crd_ensemble_observe_count(const crd_ensemble *e, int64_t *n_samples)
{
	if (!e || !n_samples || !e->obs.open) return CRD_EINVAL;
	*n_samples = e->obs.count;
	return CRD_OK;
}

int crd_ensemble_observe_info(const crd_ensemble *e, int32_t *blocks_per_member, int64_t *values_per_field, crd_observe_options *opt, int64_t *capacity)
{
	if (!e || !e->obs.open) return CRD_EINVAL;
	if (blocks_per_member) *blocks_per_member = e->mixed ? observe_blocks(member_points(e, 0)) : e->obs.blocks;  // (member 0's, as crd_ensemble_info)
	if (values_per_field) *values_per_field = (int64_t)e->nx * (int64_t)e->ny;
	if (opt) *opt = e->obs.opt;
	if (capacity) *capacity = e->obs.capacity;
	return CRD_OK;
}

int crd_ensemble_observe_read(crd_ensemble *e, int64_t first, int64_t count, double *t, double *stats, double *probes)
{
	if (!e) return CRD_EINVAL;
	const crd_ensemble::Observer &ob = e->obs;
	if (!ob.open) return efail(e, CRD_EINVAL, "no observer is open");
	if (first < 0 || count < 0 || first > ob.count || count > ob.count - first) return efail(e, CRD_EINVAL, "sample range outside the " + std::to_string(ob.count) + " recorded");
	TraceRange range("crd_ensemble_observe_read");
	ENS_TRY(e, hipSetDevice(e->device));
	const size_t B = (size_t)e->n, R = (size_t)ob.row_doubles, P = (size_t)ob.probes.n, rows = (size_t)count * B;
	std::vector<double> host(rows * R);
	if (rows) ENS_TRY(e, hipMemcpyAsync(host.data(), ob.records + (size_t)first * B * R, rows * R * sizeof(double), hipMemcpyDeviceToHost, e->stream));
	ENS_TRY(e, hipStreamSynchronize(e->stream));
	for (size_t r = 0; r < rows; r++) {
		if (stats) std::copy(host.begin() + (ptrdiff_t)(r * R), host.begin() + (ptrdiff_t)(r * R + 8), stats + r * 8);
		if (probes) std::copy(host.begin() + (ptrdiff_t)(r * R + 8), host.begin() + (ptrdiff_t)(r * R + R), probes + r * 2 * P);
	}
	if (t) std::copy(ob.t.begin() + (ptrdiff_t)first, ob.t.begin() + (ptrdiff_t)(first + count), t);
	return CRD_OK;
}

int crd_ensemble_observe_maps(crd_ensemble *e, int member, double *min_u, double *max_u, double *t_act)
{
	if (!e) return CRD_EINVAL;
	if (!e->obs.open || !e->obs.maps) return efail(e, CRD_EINVAL, "no observer with maps is open");
	if (int rc = check_member(e, member)) return rc;
	ENS_TRY(e, hipSetDevice(e->device));
	const size_t n = member_points(e, member);
	double *const out[3] = {min_u, max_u, t_act};
	for (int q = 0; q < 3; q++)
		if (out[q]) ENS_TRY(e, hipMemcpyAsync(out[q], e->obs.maps + ((size_t)member * 3 + (size_t)q) * e->obs.map_plane, n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
	ENS_TRY(e, hipStreamSynchronize(e->stream));
	return CRD_OK;
}

int crd_ensemble_observe_section_info(const crd_ensemble *e, int section, int32_t *kind, int32_t *index, int64_t *length, int64_t *additions)
{
	if (!e || !e->obs.open || section < 0 || section >= e->obs.sections.n) return CRD_EINVAL;
	if (kind) *kind = e->obs.sections.kind[section];
	if (index) *index = e->obs.sections.index[section];
	if (length) *length = e->obs.sections.length[section];
	if (additions) *additions = e->obs.section_additions[section];
	return CRD_OK;
}

int crd_ensemble_observe_read_section(crd_ensemble *e, int section, int64_t first, int64_t count, double *values)
{
	if (!e) return CRD_EINVAL;
	const crd_ensemble::Observer &ob = e->obs;
	if (!ob.open) return efail(e, CRD_EINVAL, "no observer is open");
	if (section < 0 || section >= ob.sections.n) return efail(e, CRD_EINVAL, "section " + std::to_string(section) + " was not configured (the observer has " + std::to_string(ob.sections.n) + ")");
	if (first < 0 || count < 0 || first > ob.count || count > ob.count - first) return efail(e, CRD_EINVAL, "sample range outside the " + std::to_string(ob.count) + " recorded");
	if (count > 0 && !values) return efail(e, CRD_EINVAL, "null values");
	TraceRange range("crd_ensemble_observe_read_section");
	ENS_TRY(e, hipSetDevice(e->device));
	const size_t doubles = (size_t)count * (size_t)e->n * (size_t)ob.sections.length[section] * 2;
	if (doubles) ENS_TRY(e, hipMemcpyAsync(values, section_lines(e, section, first), doubles * sizeof(double), hipMemcpyDeviceToHost, e->stream));
	ENS_TRY(e, hipStreamSynchronize(e->stream));
	return CRD_OK;
}

int crd_ensemble_observe_cycles(crd_ensemble *e, int member, int32_t *count, double *t_first, double *t_last)
{
	if (!e) return CRD_EINVAL;
	if (!e->obs.open || !e->obs.cycles) return efail(e, CRD_EINVAL, "no observer with cycle maps is open");
	if (int rc = check_member(e, member)) return rc;
	ENS_TRY(e, hipSetDevice(e->device));
	const size_t n = (size_t)e->nx * (size_t)e->ny, plane = e->obs.map_plane;
	const double *const planes = e->obs.cycle_planes + (size_t)member * 4 * plane;
	if (t_first) ENS_TRY(e, hipMemcpyAsync(t_first, planes + plane, n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
	if (t_last) ENS_TRY(e, hipMemcpyAsync(t_last, planes + 2 * plane, n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
	if (count) ENS_TRY(e, hipMemcpyAsync(count, planes + 3 * plane, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
	ENS_TRY(e, hipStreamSynchronize(e->stream));
	return CRD_OK;
}

int crd_ensemble_observe_end(crd_ensemble *e)
{
	if (!e) return CRD_EINVAL;
	if (!e->obs.open) return efail(e, CRD_EINVAL, "no observer is open");
	ENS_TRY(e, hipSetDevice(e->device));
	ENS_TRY(e, hipStreamSynchronize(e->stream));
	observer_release(e);
	return CRD_OK;
}

}  // extern "C"
