// crd_recorder.cpp -- the run recorder behind crd_recorder_*: statistics, probes, sections, maps and cycle maps of a single-slab
// context or of the slabs of a LOCAL group, sampled inside the stepping calls (crd_steppers.cpp asks recorder_* below).  Host code only;
// the kernels are crd_record.hip's.
//
// Per sample every slab runs the row pass and the gather on its own compute stream, behind the step it samples.  Slab 0 -- the lead --
// writes its row records and its block of extras (probes, row lines) straight into the lead's buffers; every other slab writes into
// buffers of its own device and sends them with at most two peer copies.  The finishing launch runs on the lead's compute stream behind
// an event of every other slab's stream; the other slabs wait for the finishing launch of the previous sample before they overwrite
// what it read.  No host wait anywhere.
#include <cmath>
#include <cstring>

#include "crd_ctx.h"
#include "crd_record.h"

struct crd_recorder {
	std::vector<crd_ctx *> ctxs;
	crd_ctx *lead = nullptr;
	crd_observe_options opt{};
	crd_observe_extras ex{};
	int64_t capacity = 0, count = 0, steps = 0;  // samples there is room for / recorded; fixed steps since open
	int nx = 0, ny = 0, precision = 0;
	int n_columns = 0, n_rows = 0, stride = 0, row_doubles = 0;  // stride: doubles per row record; row_doubles: 8 + 2 n_probes
	size_t extras_doubles = 0;                                     // one slab's block: 2 n_probes + 2 nx n_rows
	int length[CRD_OBSERVE_MAX_SECTIONS] = {};
	int64_t additions[CRD_OBSERVE_MAX_SECTIONS] = {};
	crd::RecordFinish finish{};  // (out[] is set per sample)
	// on the lead's device
	double *records = nullptr;                                  // capacity x row_doubles
	double *section_records[CRD_OBSERVE_MAX_SECTIONS] = {};     // capacity x length x 2
	double *rows = nullptr;                                     // ny x stride: the row records by global row
	double *extras = nullptr;                                   // n_slabs x extras_doubles
	hipEvent_t ev_finish = nullptr;
	struct Slab {
		double *rows = nullptr, *extras = nullptr;  // where this slab's kernels write (the lead: inside the buffers above)
		bool own_buffers = false, sends_extras = false;
		double *maps = nullptr, *cycles = nullptr;  // 3 / 4 planes of `plane` doubles
		size_t plane = 0;
		crd::RecordGather gather{};
		hipEvent_t ev_sample = nullptr;
	};
	std::vector<Slab> slabs;
	std::vector<double> times;
	std::vector<double> staging;  // host side of the read calls' one copy per slab
};

namespace crd {

namespace {

int rfail(crd_ctx *c, int code, const std::string &msg) { return fail(c, code, "recorder: " + msg); }

void release(crd_recorder *r)
{
	for (size_t k = 0; k < r->ctxs.size(); k++) {
		crd_ctx *c = r->ctxs[k];
		if (hipSetDevice(c->device) != hipSuccess) continue;
		if (c->compute) (void)hipStreamSynchronize(c->compute);
	}
	for (size_t k = 0; k < r->slabs.size(); k++) {
		crd_recorder::Slab &s = r->slabs[k];
		(void)hipSetDevice(r->ctxs[k]->device);
		if (s.own_buffers) {
			if (s.rows) (void)hipFree(s.rows);
			if (s.extras) (void)hipFree(s.extras);
		}
		if (s.maps) (void)hipFree(s.maps);
		if (s.cycles) (void)hipFree(s.cycles);
		if (s.ev_sample) (void)hipEventDestroy(s.ev_sample);
	}
	if (r->lead) (void)hipSetDevice(r->lead->device);
	for (double *p : {r->records, r->rows, r->extras})
		if (p) (void)hipFree(p);
	for (double *p : r->section_records)
		if (p) (void)hipFree(p);
	if (r->ev_finish) (void)hipEventDestroy(r->ev_finish);
	for (crd_ctx *c : r->ctxs)
		if (c->recorder == r) c->recorder = nullptr;
	delete r;
}

}  // namespace

int recorder_of_call(crd_ctx *const *cs, int n, crd_recorder **out)
{
	*out = nullptr;
	if (!cs) return CRD_OK;
	crd_recorder *r = nullptr;
	for (int k = 0; k < n; k++)
		if (cs[k] && cs[k]->recorder) r = cs[k]->recorder;
	if (!r) return CRD_OK;
	bool whole = (size_t)n == r->ctxs.size();
	for (int k = 0; whole && k < n; k++) whole = cs[k] == r->ctxs[(size_t)k];
	if (!whole) return rfail(cs[0] ? cs[0] : r->lead, CRD_ESTATE, "a recorded context steps in a call that covers the recorder's whole group (" + std::to_string(r->ctxs.size()) + " slabs)");
	*out = r;
	return CRD_OK;
}

int64_t recorder_stride(const crd_recorder *r) { return r->opt.stride; }
int64_t recorder_steps(const crd_recorder *r) { return r->steps; }
void recorder_advance(crd_recorder *r, int64_t nsteps) { r->steps += nsteps; }

int recorder_room(crd_recorder *r, int64_t samples)
{
	if (samples <= r->capacity - r->count) return CRD_OK;
	return rfail(r->lead, CRD_EINVAL, "the call would record " + std::to_string(samples) + " samples and there is room for " + std::to_string(r->capacity - r->count) + " (capacity " +
	                                      std::to_string(r->capacity) + "): refused whole, nothing launched");
}

int recorder_sample(crd_recorder *r, int plane_index, double t)
{
	if (r->count >= r->capacity) return rfail(r->lead, CRD_EINVAL, "no room for another sample");
	crd_ctx *lead = r->lead;
	const int n = (int)r->ctxs.size();
	ObserveCycles cy{};
	cy.plane = 0;
	cy.threshold = r->ex.cycle_threshold;
	cy.t_prev = r->times.empty() ? 0.0 : r->times.back();
	cy.first = r->count == 0 ? 1 : 0;
	for (int k = 0; k < n; k++) {
		crd_ctx *c = r->ctxs[(size_t)k];
		crd_recorder::Slab &s = r->slabs[(size_t)k];
		if (int rc = set_device(c)) return rc;
		const void *u = c->row_ptr(c->plane[plane_index][0], 0), *v = c->row_ptr(c->plane[plane_index][1], 0);
		// (this slab's buffers were read by the previous sample's peer copies -- this stream -- and its finishing launch -- the lead's)
		if (s.own_buffers && r->count > 0) HIP_TRY(c, hipStreamWaitEvent(c->compute, r->ev_finish, 0));
		cy.planes = s.cycles;
		cy.plane = s.plane;
		HIP_TRY(c, launch_record_rows(r->precision, u, v, c->nx, c->nyl, s.rows, r->stride, s.maps, s.plane, r->opt.threshold, t, s.cycles ? &cy : nullptr, c->compute));
		HIP_TRY(c, launch_record_gather(r->precision, u, v, c->nx, c->nyl, s.rows, r->stride, s.extras, s.gather, c->compute));
		if (s.own_buffers) {
			HIP_TRY(c, hipMemcpyPeerAsync(r->rows + (size_t)c->js * (size_t)r->stride, lead->device, s.rows, c->device, (size_t)c->nyl * (size_t)r->stride * sizeof(double), c->compute));
			if (s.sends_extras)
				HIP_TRY(c, hipMemcpyPeerAsync(r->extras + (size_t)k * r->extras_doubles, lead->device, s.extras, c->device, r->extras_doubles * sizeof(double), c->compute));
			HIP_TRY(c, hipEventRecord(s.ev_sample, c->compute));
		}
	}
	if (int rc = set_device(lead)) return rc;
	for (int k = 0; k < n; k++)
		if (r->slabs[(size_t)k].own_buffers) HIP_TRY(lead, hipStreamWaitEvent(lead->compute, r->slabs[(size_t)k].ev_sample, 0));
	RecordFinish f = r->finish;
	for (int q = 0; q < f.n_sections; q++) f.out[q] = r->section_records[q] + (size_t)r->count * (size_t)r->length[q] * 2;
	HIP_TRY(lead, launch_record_finish(r->rows, r->stride, r->nx, r->ny, r->extras, r->extras_doubles, f, r->records + (size_t)r->count * (size_t)r->row_doubles, lead->compute));
	for (int q = 0; q < f.n_sections; q++)
		if (f.kind[q] == CRD_SECTION_PHI_MEAN)  // (a lone context only)
			HIP_TRY(lead, launch_record_phi_mean(r->precision, lead->row_ptr(lead->plane[plane_index][0], 0), lead->row_ptr(lead->plane[plane_index][1], 0), r->nx, r->ny, f.out[q],
			                                     lead->compute));
	if (n > 1) HIP_TRY(lead, hipEventRecord(r->ev_finish, lead->compute));
	r->times.push_back(t);
	r->count++;
	return CRD_OK;
}

void recorder_detach(crd_ctx *c)
{
	if (c && c->recorder) release(c->recorder);
}

}  // namespace crd

using namespace crd;

extern "C" {

int crd_recorder_open(crd_ctx *const *ctxs, int n_slabs, const crd_observe_options *opt, const crd_observe_extras *extras, int64_t capacity, crd_recorder **out)
{
	if (out) *out = nullptr;
	if (!ctxs || n_slabs < 1 || !ctxs[0] || !out) return rfail(ctxs && n_slabs >= 1 ? ctxs[0] : nullptr, CRD_EINVAL, "null argument");
	crd_ctx *lead = ctxs[0];
	for (int k = 0; k < n_slabs; k++)
		if (!ctxs[k]) return rfail(lead, CRD_EINVAL, "null context");
	// ---- what a recorder does not take ----
	for (int k = 0; k < n_slabs; k++) {
		const crd_ctx *c = ctxs[k];
		if (c->recorder) return rfail(lead, CRD_EINVAL, "a recorder is already open on this context (slab " + std::to_string(c->slab) + ")");
		if (c->d0 > 1) return rfail(lead, CRD_EINVAL, "block contexts (crd_create_block with a theta split) are not recorded: a row's record needs the whole row");
		if (c->halo == CRD_HALO_RCCL && c->n_slabs > 1)
			return rfail(lead, CRD_EINVAL, "a context wired through RCCL with more than one rank is not recorded (the finishing pass needs an ordered reduction over the ranks)");
	}
	if (n_slabs != lead->n_slabs) return rfail(lead, CRD_EINVAL, "the context list is not the whole LOCAL group: " + std::to_string(n_slabs) + " of " + std::to_string(lead->n_slabs) + " slabs");
	for (int k = 0; k < n_slabs; k++) {
		const crd_ctx *c = ctxs[k];
		if (c->n_slabs != n_slabs || c->slab != k) return rfail(lead, CRD_EINVAL, "the context list is not the whole LOCAL group in slab order");
		if (n_slabs > 1 && (c->halo != CRD_HALO_LOCAL || c->group.size() != (size_t)n_slabs || c->group[(size_t)k] != c || c->group[0] != lead))
			return rfail(lead, CRD_EINVAL, "the context list is not the whole LOCAL group (crd_comm_attach_local)");
	}
	// ---- what crd_ensemble_observe_begin_with refuses ----
	const int nx = (int)lead->g.nx, ny = (int)lead->g.ny;
	if (!opt) return rfail(lead, CRD_EINVAL, "null options");
	if (opt->stride < 1) return rfail(lead, CRD_EINVAL, "stride must be >= 1");
	if (capacity < 1) return rfail(lead, CRD_EINVAL, "capacity must be >= 1");
	if (opt->n_probes < 0 || opt->n_probes > CRD_OBSERVE_MAX_PROBES)
		return rfail(lead, CRD_EINVAL, "a recorder takes 0 .. " + std::to_string(CRD_OBSERVE_MAX_PROBES) + " probes (got " + std::to_string(opt->n_probes) + ")");
	for (int q = 0; q < opt->n_probes; q++)
		if (opt->probe_i[q] < 0 || opt->probe_i[q] >= nx || opt->probe_j[q] < 0 || opt->probe_j[q] >= ny)
			return rfail(lead, CRD_EINVAL, "probe " + std::to_string(q) + " (i = " + std::to_string(opt->probe_i[q]) + ", j = " + std::to_string(opt->probe_j[q]) + ") is outside the " +
			                                   std::to_string(nx) + " x " + std::to_string(ny) + " grid");
	if (opt->maps != 0 && opt->maps != 1) return rfail(lead, CRD_EINVAL, "maps is 0 or 1");
	if (opt->maps && !std::isfinite(opt->threshold)) return rfail(lead, CRD_EINVAL, "maps need a finite threshold");
	crd_observe_extras ex{};
	if (extras) ex = *extras;
	if (ex.n_sections < 0 || ex.n_sections > CRD_OBSERVE_MAX_SECTIONS)
		return rfail(lead, CRD_EINVAL, "a recorder takes 0 .. " + std::to_string(CRD_OBSERVE_MAX_SECTIONS) + " sections (got " + std::to_string(ex.n_sections) + ")");
	if (ex.cycles != 0 && ex.cycles != 1) return rfail(lead, CRD_EINVAL, "cycles is 0 or 1");
	if (ex.cycles && !std::isfinite(ex.cycle_threshold)) return rfail(lead, CRD_EINVAL, "cycle maps need a finite cycle_threshold");
	auto *r = new crd_recorder;
	r->lead = lead;  // (not yet attached to any context: release() below frees it)
	auto refuse = [&](const std::string &msg) {
		delete r;
		return rfail(lead, CRD_EINVAL, msg);
	};
	r->finish.n_probes = opt->n_probes;
	r->finish.n_sections = ex.n_sections;
	double record_bytes = (double)capacity * (double)(8 + 2 * opt->n_probes) * 8.0;
	for (int s = 0; s < ex.n_sections; s++) {
		if (!observe_section_shape(lead->p.precision, ex.kind[s], nx, ny, &r->length[s], nullptr, &r->additions[s])) return refuse("section " + std::to_string(s) + ": unknown kind " + std::to_string(ex.kind[s]));
		r->finish.kind[s] = ex.kind[s];
		if (ex.kind[s] == CRD_SECTION_ROW || ex.kind[s] == CRD_SECTION_COLUMN) {
			const int limit = ex.kind[s] == CRD_SECTION_ROW ? ny : nx;
			if (ex.index[s] < 0 || ex.index[s] >= limit)
				return refuse("section " + std::to_string(s) + ": " + (ex.kind[s] == CRD_SECTION_ROW ? "row " : "column ") + std::to_string(ex.index[s]) + " is outside the " + std::to_string(nx) +
				              " x " + std::to_string(ny) + " grid");
			r->finish.slot[s] = ex.kind[s] == CRD_SECTION_ROW ? r->n_rows++ : r->n_columns++;
		} else {
			ex.index[s] = 0;
			if (ex.kind[s] == CRD_SECTION_PHI_MEAN && n_slabs > 1)
				return refuse("section " + std::to_string(s) + ": phi-mean on more than one slab is not recorded (a column's sum crosses the slabs); it is on a lone context");
		}
		record_bytes += (double)capacity * (double)r->length[s] * 16.0;
	}
	if (record_bytes > 0x1p46) return refuse("capacity too large");
	r->ctxs.assign(ctxs, ctxs + n_slabs);
	r->opt = *opt;
	r->ex = ex;
	r->capacity = capacity;
	r->nx = nx;
	r->ny = ny;
	r->precision = lead->p.precision;
	r->stride = kRecordRowFixed + 2 * r->n_columns;
	r->row_doubles = 8 + 2 * opt->n_probes;
	r->extras_doubles = 2 * (size_t)opt->n_probes + 2 * (size_t)nx * (size_t)r->n_rows;
	r->slabs.resize((size_t)n_slabs);
	auto owner_of_row = [&](int j) {
		for (int k = 0; k < n_slabs; k++)
			if (j >= ctxs[k]->js && j <= ctxs[k]->je) return k;
		return 0;
	};
	for (int q = 0; q < opt->n_probes; q++) r->finish.probe_owner[q] = owner_of_row(opt->probe_j[q]);
	for (int s = 0; s < ex.n_sections; s++)
		if (ex.kind[s] == CRD_SECTION_ROW) r->finish.owner[s] = owner_of_row(ex.index[s]);
	for (int k = 0; k < n_slabs; k++) {
		crd_recorder::Slab &sl = r->slabs[(size_t)k];
		RecordGather &g = sl.gather;
		g.n_probes = opt->n_probes;
		g.n_columns = r->n_columns;
		g.n_rows = r->n_rows;
		for (int q = 0; q < opt->n_probes; q++) {
			g.probe_i[q] = opt->probe_i[q];
			g.probe_j[q] = r->finish.probe_owner[q] == k ? (int)(opt->probe_j[q] - ctxs[k]->js) : -1;
			sl.sends_extras = sl.sends_extras || g.probe_j[q] >= 0;
		}
		for (int s = 0; s < ex.n_sections; s++) {
			if (ex.kind[s] == CRD_SECTION_COLUMN) g.column_i[r->finish.slot[s]] = ex.index[s];
			if (ex.kind[s] == CRD_SECTION_ROW) {
				g.row_j[r->finish.slot[s]] = r->finish.owner[s] == k ? (int)(ex.index[s] - ctxs[k]->js) : -1;
				sl.sends_extras = sl.sends_extras || r->finish.owner[s] == k;
			}
		}
		sl.plane = ((size_t)ctxs[k]->nx * (size_t)ctxs[k]->nyl + 1) & ~(size_t)1;
	}
	// ---- device work ----
	TraceRange range("crd_recorder_open");
	auto dfail = [&](crd_ctx *c, hipError_t e, const char *what) {
		release(r);
		return rfail(c, e == hipErrorOutOfMemory ? CRD_ENOMEM : CRD_EHIP, std::string(what) + ": " + hipGetErrorString(e));
	};
#define REC_TRY(c, expr, what)                                 \
	do {                                                       \
		if (hipError_t e_ = (expr); e_ != hipSuccess) return dfail((c), e_, (what)); \
	} while (0)
	REC_TRY(lead, hipSetDevice(lead->device), "hipSetDevice");
	REC_TRY(lead, hipMalloc((void **)&r->records, (size_t)capacity * (size_t)r->row_doubles * sizeof(double)), "hipMalloc(records)");
	for (int s = 0; s < ex.n_sections; s++)
		REC_TRY(lead, hipMalloc((void **)&r->section_records[s], (size_t)capacity * (size_t)r->length[s] * 2 * sizeof(double)), "hipMalloc(section records)");
	REC_TRY(lead, hipMalloc((void **)&r->rows, (size_t)ny * (size_t)r->stride * sizeof(double)), "hipMalloc(row records)");
	if (r->extras_doubles) {
		REC_TRY(lead, hipMalloc((void **)&r->extras, (size_t)n_slabs * r->extras_doubles * sizeof(double)), "hipMalloc(extras)");
		REC_TRY(lead, hipMemsetAsync(r->extras, 0, (size_t)n_slabs * r->extras_doubles * sizeof(double), lead->compute), "hipMemsetAsync(extras)");
	}
	if (n_slabs > 1) REC_TRY(lead, hipEventCreateWithFlags(&r->ev_finish, hipEventDisableTiming), "hipEventCreate");
	for (int k = 0; k < n_slabs; k++) {
		crd_ctx *c = ctxs[k];
		crd_recorder::Slab &sl = r->slabs[(size_t)k];
		REC_TRY(c, hipSetDevice(c->device), "hipSetDevice");
		if (k == 0) {
			sl.rows = r->rows + (size_t)c->js * (size_t)r->stride;
			sl.extras = r->extras;
		} else {
			sl.own_buffers = true;
			REC_TRY(c, hipMalloc((void **)&sl.rows, (size_t)c->nyl * (size_t)r->stride * sizeof(double)), "hipMalloc(row records)");
			if (r->extras_doubles) {
				REC_TRY(c, hipMalloc((void **)&sl.extras, r->extras_doubles * sizeof(double)), "hipMalloc(extras)");
				REC_TRY(c, hipMemsetAsync(sl.extras, 0, r->extras_doubles * sizeof(double), c->compute), "hipMemsetAsync(extras)");
			}
			REC_TRY(c, hipEventCreateWithFlags(&sl.ev_sample, hipEventDisableTiming), "hipEventCreate");
		}
		if (opt->maps) {
			REC_TRY(c, hipMalloc((void **)&sl.maps, 3 * sl.plane * sizeof(double)), "hipMalloc(maps)");
			const double init[3] = {INFINITY, -INFINITY, NAN};
			for (int q = 0; q < 3; q++) REC_TRY(c, launch_observe_fill(sl.maps + (size_t)q * sl.plane, sl.plane, init[q], c->compute), "map initialisation");
		}
		if (ex.cycles) {  // previous var0: anything (the first sample stores it); t_first, t_last: NaN; count: 0
			REC_TRY(c, hipMalloc((void **)&sl.cycles, 4 * sl.plane * sizeof(double)), "hipMalloc(cycle planes)");
			REC_TRY(c, launch_observe_fill(sl.cycles + sl.plane, 2 * sl.plane, NAN, c->compute), "cycle map initialisation");
			REC_TRY(c, hipMemsetAsync(sl.cycles, 0, sl.plane * sizeof(double), c->compute), "cycle map initialisation");
			REC_TRY(c, hipMemsetAsync(sl.cycles + 3 * sl.plane, 0, sl.plane * sizeof(double), c->compute), "cycle map initialisation");
		}
	}
#undef REC_TRY
	for (int k = 0; k < n_slabs; k++) ctxs[k]->recorder = r;
	*out = r;
	return CRD_OK;
}

int crd_recorder_close(crd_recorder *r)
{
	if (!r) return CRD_EINVAL;
	release(r);
	return CRD_OK;
}

int crd_recorder_count(const crd_recorder *r, int64_t *n_samples)
{
	if (!r || !n_samples) return CRD_EINVAL;
	*n_samples = r->count;
	return CRD_OK;
}

int crd_recorder_info(const crd_recorder *r, int64_t *additions, int64_t *values_per_field, int32_t *n_slabs, crd_observe_options *opt, crd_observe_extras *extras, int64_t *capacity)
{
	if (!r) return CRD_EINVAL;
	if (additions) *additions = record_additions(r->precision, r->nx, r->ny);
	if (values_per_field) *values_per_field = (int64_t)r->nx * (int64_t)r->ny;
	if (n_slabs) *n_slabs = (int32_t)r->ctxs.size();
	if (opt) *opt = r->opt;
	if (extras) *extras = r->ex;
	if (capacity) *capacity = r->capacity;
	return CRD_OK;
}

int crd_recorder_read(crd_recorder *r, int64_t first, int64_t count, double *t, double *stats, double *probes)
{
	if (!r) return CRD_EINVAL;
	crd_ctx *lead = r->lead;
	if (first < 0 || count < 0 || first + count > r->count) return rfail(lead, CRD_EINVAL, "samples " + std::to_string(first) + " .. " + std::to_string(first + count - 1) + " are outside the " + std::to_string(r->count) + " recorded");
	if (count == 0) return CRD_OK;
	if (int rc = set_device(lead)) return rc;
	const size_t rd = (size_t)r->row_doubles;
	r->staging.resize((size_t)count * rd);
	HIP_TRY(lead, hipMemcpyAsync(r->staging.data(), r->records + (size_t)first * rd, (size_t)count * rd * sizeof(double), hipMemcpyDeviceToHost, lead->compute));
	HIP_TRY(lead, hipStreamSynchronize(lead->compute));
	const size_t np2 = 2 * (size_t)r->opt.n_probes;
	for (int64_t s = 0; s < count; s++) {
		if (t) t[s] = r->times[(size_t)(first + s)];
		if (stats) std::memcpy(stats + (size_t)s * 8, r->staging.data() + (size_t)s * rd, 8 * sizeof(double));
		if (probes && np2) std::memcpy(probes + (size_t)s * np2, r->staging.data() + (size_t)s * rd + 8, np2 * sizeof(double));
	}
	return CRD_OK;
}

int crd_recorder_section_info(const crd_recorder *r, int section, int32_t *kind, int32_t *index, int64_t *length, int64_t *additions)
{
	if (!r || section < 0 || section >= r->ex.n_sections) return CRD_EINVAL;
	if (kind) *kind = r->ex.kind[section];
	if (index) *index = r->ex.index[section];
	if (length) *length = r->length[section];
	if (additions) *additions = r->additions[section];
	return CRD_OK;
}

int crd_recorder_read_section(crd_recorder *r, int section, int64_t first, int64_t count, double *values)
{
	if (!r || !values) return CRD_EINVAL;
	crd_ctx *lead = r->lead;
	if (section < 0 || section >= r->ex.n_sections) return rfail(lead, CRD_EINVAL, "section " + std::to_string(section) + " was not configured");
	if (first < 0 || count < 0 || first + count > r->count) return rfail(lead, CRD_EINVAL, "samples " + std::to_string(first) + " .. " + std::to_string(first + count - 1) + " are outside the " + std::to_string(r->count) + " recorded");
	if (count == 0) return CRD_OK;
	if (int rc = set_device(lead)) return rc;
	const size_t line = (size_t)r->length[section] * 2;
	HIP_TRY(lead, hipMemcpyAsync(values, r->section_records[section] + (size_t)first * line, (size_t)count * line * sizeof(double), hipMemcpyDeviceToHost, lead->compute));
	HIP_TRY(lead, hipStreamSynchronize(lead->compute));
	return CRD_OK;
}

// `planes` planes of every slab, from plane `from` on, in ONE copy per slab; out[q]: whole-grid ny x nx arrays of `bytes[q]` per value.
static int gather_planes(crd_recorder *r, bool cycles, int from, int planes, void *const *out, const size_t *bytes)
{
	for (size_t k = 0; k < r->ctxs.size(); k++) {
		crd_ctx *c = r->ctxs[k];
		const crd_recorder::Slab &sl = r->slabs[k];
		if (int rc = set_device(c)) return rc;
		r->staging.resize((size_t)planes * sl.plane);
		const double *src = (cycles ? sl.cycles : sl.maps) + (size_t)from * sl.plane;
		HIP_TRY(c, hipMemcpyAsync(r->staging.data(), src, (size_t)planes * sl.plane * sizeof(double), hipMemcpyDeviceToHost, c->compute));
		HIP_TRY(c, hipStreamSynchronize(c->compute));
		const size_t points = (size_t)c->nx * (size_t)c->nyl, at = (size_t)c->js * (size_t)r->nx;
		for (int q = 0; q < planes; q++)
			if (out[q]) std::memcpy(static_cast<char *>(out[q]) + at * bytes[q], r->staging.data() + (size_t)q * sl.plane, points * bytes[q]);
	}
	return CRD_OK;
}

int crd_recorder_maps(crd_recorder *r, double *min_u, double *max_u, double *t_act)
{
	if (!r) return CRD_EINVAL;
	if (!r->opt.maps) return rfail(r->lead, CRD_EINVAL, "maps are off");
	void *const out[3] = {min_u, max_u, t_act};
	const size_t bytes[3] = {8, 8, 8};
	return gather_planes(r, false, 0, 3, out, bytes);
}

int crd_recorder_cycles(crd_recorder *r, int32_t *count, double *t_first, double *t_last)
{
	if (!r) return CRD_EINVAL;
	if (!r->ex.cycles) return rfail(r->lead, CRD_EINVAL, "cycle maps are off");
	void *const out[3] = {t_first, t_last, count};  // planes 1, 2, 3: the count as int32 in the first half of its plane
	const size_t bytes[3] = {8, 8, 4};
	return gather_planes(r, true, 1, 3, out, bytes);
}

}  // extern "C"
