// crd_adaptive.cpp -- the error-controlled integrator of a context or of the slabs of a run behind the C ABI: ARKode's controller on
// Zonneveld 5(3)4 (CRD_ADAPT_ARKODE) or the RK4(3) pair with an I-controller, attempts launched with the fused kernels, dense output.
// The controller's arithmetic and the plane rotation are crd_arkode.h's (shared with the ensemble's integrator).  Host code only.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "crd_ctx.h"

using namespace crd;

namespace {

// f(t, plane src) -> plane dst on every slab (bare RHS with the stage kernel; multi-slab: one ghost row of var0 first).
int rhs_on_planes(crd_ctx *const *cs, int n, double t, int src, int dst)
{
	const bool multi = cs[0]->halo != CRD_HALO_SELF;
	if (multi)
		if (int rc = prime_halo(cs, n, src, 1, false)) return rc;
	for (int k = 0; k < n; k++) {
		crd_ctx *c = cs[k];
		if (int rc = set_device(c)) return rc;
		StageCall call{};
		call.stage = 0;
		call.absorb = absorbing(c, t) ? 1 : 0;
		call.yin = c->planes(src);
		call.yout = c->planes(dst);
		if (multi) HIP_TRY(c, hipStreamWaitEvent(c->compute, c->ev_halo, 0));
		HIP_TRY(c, launch_stage(c->p.precision, c->desc, call, 0, c->nyl, c->compute));
	}
	return CRD_OK;
}

// One scalar per slab (left in c->scalar_dev by work already enqueued on the compute streams) combined over the run: the sum or
// the maximum, identical on every rank (RCCL: ncclAllReduce; LOCAL groups: added / compared on the host in slab order).
int collect_scalar(crd_ctx *const *cs, int n, bool take_max, double *out)
{
	// The producers wrote to scalar_sink(): host memory, or -- RCCL runs -- device memory that is reduced over the ranks first and
	// copied to the page-locked buffer (a copy to pageable memory goes through the runtime's staging buffer: ~10 us per attempt of an
	// error-controlled run on a small grid).  Every slab's work is enqueued before the first one is waited for.
	for (int k = 0; k < n; k++) {
		crd_ctx *c = cs[k];
		if (c->scalar_sink() == c->scalar_host) continue;
		if (int rc = set_device(c)) return rc;
		if (c->halo == CRD_HALO_RCCL) NCCL_TRY(c, g_rccl.AllReduce(c->scalar_dev, c->scalar_dev, 1, ncclDouble, take_max ? ncclMax : ncclSum, c->nccl, c->compute));
		HIP_TRY(c, hipMemcpyAsync(c->scalar_host, c->scalar_dev, sizeof(double), hipMemcpyDeviceToHost, c->compute));
	}
	double acc = 0.0;
	for (int k = 0; k < n; k++) {
		crd_ctx *c = cs[k];
		if (int rc = set_device(c)) return rc;
		HIP_TRY(c, hipStreamSynchronize(c->compute));
		const double part = c->scalar_host[0];
		if (take_max) acc = (part > acc || part != part) ? part : acc;
		else acc += part;
	}
	*out = acc;
	return CRD_OK;
}

// ARKode's step-size controller (CRD_ADAPT_ARKODE) and its bookkeeping: crd_arkode.h (shared with the ensemble's integrator).

// arkHin: ARKode's estimate of the first step from y'' along a forward Euler trial step, on the planes: f0 -> SB, trial state ->
// SA, f(trial) -> ACC (all three are scratch on a fresh state).
int arkode_initial_step(crd_ctx *const *cs, int n, double t0, double tout, int cur, const crd_adaptive_options &o, double n_components, double *h0)
{
	crd_ctx *lead = cs[0];
	arkode::Hin H;
	if (!arkode::hin_start(H, t0, tout)) return fail(lead, CRD_EINVAL, arkode::kHinTooClose);
	if (int rc = rhs_on_planes(cs, n, t0, cur, crd_ctx::SB)) return rc;
	for (int k = 0; k < n; k++) {
		crd_ctx *c = cs[k];
		if (int rc = set_device(c)) return rc;
		HIP_TRY(c, launch_hin_bound(c->p.precision, c->planes(cur), c->planes(crd_ctx::SB), c->nx, c->nyl, o.rtol, o.atol, c->scalar_sink(), c->compute));
	}
	double hub_inv = 0.0;
	if (int rc = collect_scalar(cs, n, true, &hub_inv)) return rc;
	arkode::hin_bound(H, hub_inv);
	while (!H.done) {
		const double hg = H.hg;
		for (int k = 0; k < n; k++) {
			crd_ctx *c = cs[k];
			if (int rc = set_device(c)) return rc;
			HIP_TRY(c, launch_axpy_planes(c->p.precision, c->planes(cur), c->planes(crd_ctx::SB), hg, c->planes(crd_ctx::SA), c->nx, c->nyl, c->compute));
		}
		if (int rc = rhs_on_planes(cs, n, t0 + hg, crd_ctx::SA, crd_ctx::ACC)) return rc;
		for (int k = 0; k < n; k++) {
			crd_ctx *c = cs[k];
			if (int rc = set_device(c)) return rc;
			HIP_TRY(c, launch_ydd_sumsq(c->p.precision, c->planes(cur), c->planes(crd_ctx::SB), c->planes(crd_ctx::ACC), hg, o.rtol, o.atol, c->nx, c->nyl, c->err_partials,
			                            c->scalar_sink(), c->compute));
		}
		double sum = 0.0;
		if (int rc = collect_scalar(cs, n, false, &sum)) return rc;
		arkode::hin_ydd(H, std::sqrt(sum / n_components));
	}
	*h0 = H.h0;
	return CRD_OK;
}

constexpr int kEmbedHalo = kStepHalo + 1;  // the fifth stage reads one more row
// The two attempt slots (an attempt and the one launched ahead of its verdict) have scalars of their own -- elements 2 and 3; 0 is
// collect_scalar's / crd_state_max_abs's, which run on the compute stream with no ordering against a slot's second-stream work.
constexpr int kAttemptScalar = 2;

// One call's error-controlled integration of all slabs of a run (n = 1: a single-slab or RCCL context; n > 1: a LOCAL group): what
// the call keeps from attempt to attempt, and its parts.
struct AdaptiveRun {
	crd_ctx *const *cs;
	const int n;
	crd_ctx *const lead;
	const double t0, tout;
	const crd_adaptive_options o;
	const bool multi, arkode_method, dense;  // (dense: ARKode's ARK_NORMAL never shortens a step for an output time)
	const double h_cap, n_components;        // (the WRMS norm is over the whole grid)
	// Three state planes take turns as y_n, y_{n+1} and scratch: Y and SA (and OUT with dense output).
	arkode::Rotation R;
	arkode::Memory &A;  // (every context of the run gets a copy at the end)
	crd_adaptive_stats st{};
	double t, t_prev, h = 0.0;
	// Ghost rows of each plane's present content that are still valid (multi-slab; a single slab wraps in the kernel).  The
	// integrator exchanges kAdaptGhost rows of the state it is about to step from when fewer than the attempt's five are left, and
	// every attempt produces its rows AND the ghost-region rows its input still covers -- the deep halo of the fixed stepper, by
	// attempts: one exchange per kAdaptGhost / 5 accepted steps instead of one per attempt (a rejected attempt re-runs on the same
	// input).  Only owned rows count towards the error norm (FusedArgs::err_lo / err_hi), so every rank still sees the same sum.
	int kAdaptGhost = 0;  // 60 rows: 12 attempts
	int ext_of[crd_ctx::NPLANES];
	bool in_flight[2] = {false, false};  // the attempt slots: launched and not yet waited for

	AdaptiveRun(crd_ctx *const *cs_, int n_, double t0_, double tout_, const crd_adaptive_options &o_)
	    : cs(cs_), n(n_), lead(cs_[0]), t0(t0_), tout(tout_), o(o_), multi(lead->halo != CRD_HALO_SELF), arkode_method(o.method == CRD_ADAPT_ARKODE),
	      dense(o.dense_output != 0 || arkode_method), h_cap(arkode::h_cap(o, lead->p)), n_components(2.0 * (double)lead->g.nx * (double)lead->g.ny),
	      R(arkode::Rotation::fresh(dense)), A(lead->ark), t(t0_), t_prev(t0_)
	{
		int shortest = lead->nyl;
		for (int k = 0; k < lead->d1; k++) {
			int64_t a0, a1;
			if (crd_slab_extents(lead->g.ny, k, lead->d1, &a0, &a1) == CRD_OK) shortest = (int)std::min<int64_t>(shortest, a1 - a0 + 1);
		}
		kAdaptGhost = kEmbedHalo * std::max(1, std::min((kGhost - kStepHalo) / kEmbedHalo, shortest / kEmbedHalo));
		for (int &e : ext_of) e = multi ? 0 : (1 << 20);
	}

	// The attempts' buffers and events, and the third state plane of dense output (all lazy).
	int prepare_contexts()
	{
		for (int k = 0; k < n; k++) {
			crd_ctx *c = cs[k];
			if (!fused_step_supported(c->p.precision, c->desc)) return fail(lead, CRD_EINVAL, "slab too small for the fused step kernel");
			if (int rc = set_device(c)) return rc;
			if (!c->err_partials) {  // two slots: an attempt and the one launched ahead of its verdict
				c->err_capacity = std::max(fused_max_items(c->desc), 256);  // (256: the block partials of the initial-step norm)
				HIP_TRY(c, hipMalloc((void **)&c->err_partials, 2 * sizeof(double) * (size_t)c->err_capacity));
				for (int q = 0; q < 2; q++) {
					HIP_TRY(c, hipEventCreateWithFlags(&c->ev_attempt[q], hipEventDisableTiming));
					HIP_TRY(c, hipEventCreateWithFlags(&c->ev_norm[q], hipEventDisableTiming));
				}
			}
			if (dense)
				for (int f = 0; f < 2; f++)
					if (!c->plane[crd_ctx::OUT][f])
						if (int rc = alloc_plane(c, crd_ctx::OUT, f)) return rc;
		}
		for (int k = 0; k < n; k++) cs[k]->cycle_pos = -1;  // the integrator exchanges as it needs; a fixed-step call afterwards starts afresh
		return CRD_OK;
	}

	// The interpolant of the step R.prev -> R.cur (t_n -> t_np1; SB = f_n, ACC = f_{n+1}) at tout into the remaining state plane; then
	// the step is recorded and the planes are re-labelled (arkode::end_of_call).
	int hand_back(double t_n, double t_np1)
	{
		const double hstep = t_np1 - t_n;
		for (int k = 0; k < n; k++) {
			crd_ctx *c = cs[k];
			if (int rc = set_device(c)) return rc;
			HIP_TRY(c, launch_hermite(c->p.precision, c->planes(R.prev), c->planes(R.cur), c->planes(crd_ctx::SB), c->planes(crd_ctx::ACC), c->planes(R.interpolant()), c->nx,
			                          c->nyl, (tout - t_n) / hstep, hstep, c->compute));
		}
		for (int k = 0; k < n; k++) arkode::end_of_call(R, true, cs[k]->dense, tout, t_n, t_np1).apply(cs[k]->plane);
		return CRD_OK;
	}

	// Where the call starts -- from the step the previous one left pending, or afresh -- and with which step size; *done: tout lies
	// inside the step already taken, and the state is handed back.
	int start(bool *done)
	{
		bool resume = dense && arkode::resumes(lead->dense, lead->ark, t0, arkode_method);
		for (int k = 0; k < n; k++)  // (every slab of a group must still hold the step: an upload to one of them alone ends the carry-over for all)
			resume = resume && cs[k]->dense.pending && cs[k]->dense.t_out == lead->dense.t_out && cs[k]->dense.t_np1 == lead->dense.t_np1;
		// Under RCCL that decision has to be the RING's (round-3 advice): crd_state_upload on one rank only is allowed between calls, and a
		// rank that alone started afresh would run arkHin's exchanges and reductions while its neighbours skip them -- the ring's
		// collectives would no longer pair.  One ncclAllReduce(min) of the ranks' votes: every rank resumes, or none does.
		if (lead->halo == CRD_HALO_RCCL && n == 1) {
			int all = 0;
			if (int rc = begin_cycle_agreement(lead, resume ? 0 : -1)) return rc;
			if (int rc = finish_cycle_agreement(lead, &all)) return rc;
			if (resume && all != 0) lead->agreement_restarts++;
			resume = resume && all == 0;
		}
		for (int k = 0; k < n; k++)
			if (!resume) cs[k]->dense.pending = false;
		if (resume) {
			st.t_internal = lead->dense.t_np1;
			if (tout <= lead->dense.t_np1) {  // still inside the step the integrator has already taken: interpolate again
				R.reinterpolate();
				if (int rc = hand_back(lead->dense.t_n, lead->dense.t_np1)) return rc;
				st.t = tout;
				st.h_next = arkode_method ? A.hprime : std::fmin(o.h0 > 0.0 ? o.h0 : 0.8 * crd_stable_dt(&lead->p), h_cap);
				*done = true;
				return CRD_OK;
			}
			t = lead->dense.t_np1;
			R.resume();
		}
		if (arkode_method) {
			if (!resume) {  // a fresh state: ARKodeInit
				arkode::init(A, t0, o.h0);
				if (arkode::needs_estimate(A, t0, tout))
					if (int rc = arkode_initial_step(cs, n, t0, tout, R.cur, o, n_components, &A.h)) return rc;
				arkode::first_step(A, h_cap);
			}
			h = A.h;
		} else {
			h = std::fmin(o.h0 > 0.0 ? o.h0 : 0.8 * crd_stable_dt(&lead->p), h_cap);
		}
		st.h_first = arkode_method ? arkode::first_attempt(A) : h;
		return CRD_OK;
	}

	// One attempt of size hh at time tt from plane `src` into plane `dst`, enqueued only: the kernel, the fixed-order sum of its
	// partials, and -- on the second stream, behind an event -- the reduction over the ranks and the copy of the scalar to
	// page-locked memory.  `slot` (0 / 1) names the buffers; finish_attempt(slot) waits for the scalar.
	int launch_attempt(double tt, double hh, int src, int dst, int slot)
	{
		// The attempt behind an exchange is cut in two (round 5): its rows that read owned rows only, [5, nyl - 5), are launched straight
		// behind the exchange's release and run UNDER it; the rest -- the edge rows and the ghost-region rows -- follow behind the halo
		// event as one small launch, and the one sum kernel behind that adds both launches' partials.  (Uncut, the 2 x 7.9 MB of an
		// 8192-column slab's 60 ghost rows travelled with nothing to hide under: 167 us per exchange, 13 us per attempt.)
		bool under_exchange = false;
		if (ext_of[src] < kEmbedHalo) {
			if (int rc = prime_halo(cs, n, src, kAdaptGhost, true)) return rc;
			under_exchange = true;
			for (int k = 0; k < n; k++) under_exchange = under_exchange && cs[k]->nyl >= 8 * kEmbedHalo;
			if (!under_exchange)
				for (int k = 0; k < n; k++) {
					if (int rc = set_device(cs[k])) return rc;
					HIP_TRY(cs[k], hipStreamWaitEvent(cs[k]->compute, cs[k]->ev_halo, 0));
				}
			ext_of[src] = kAdaptGhost;
		}
		const int e = multi ? ext_of[src] - kEmbedHalo : 0;
		for (int k = 0; k < n; k++) {
			crd_ctx *c = cs[k];
			if (int rc = set_device(c)) return rc;
			FusedCall call = make_fused_call(c, tt, hh, src, dst);
			call.embed = arkode_method ? 2 : 1;
			if (arkode_method) step::stage_flags(tt, hh, c->p.t_boundary, 5, call.absorb);  // the fifth stage's time: t + 3/4 h (Zonneveld); RK4(3)'s is t + h, the fourth's
			call.plan = arkode_method ? &c->plan_arkode : &c->plan_embed;
			call.rtol = o.rtol;
			call.atol = o.atol;
			call.err_partials = c->err_partials + (size_t)slot * (size_t)c->err_capacity;
			call.err_capacity = c->err_capacity;
			const bool reduce_on_device = c->halo == CRD_HALO_RCCL;
			// (the slot's previous user may have been launched ahead and never waited for: its sum and reduction on the second stream must be
			// through with the slot's partials and scalar before this attempt writes them -- only then: a slot whose attempt the host has
			// waited for (finish_attempt) is quiet, and a cross-stream wait in front of every attempt is a bubble of its own)
			if (in_flight[slot]) HIP_TRY(c, hipStreamWaitEvent(c->compute, c->ev_norm[slot], 0));
			// The sum of the partials runs on the SECOND stream behind the step kernel's own completion signal, so that the compute stream
			// carries step kernels only, back to back: a one-block kernel between two sweeps cost its 8 us and 5 more of dispatch latency
			// it is too short to hide (kernel-trace timelines, profiles/r05/adaptive_attempt_timeline_kernel_trace.txt).
			// (The RK4(3) pair launches nothing ahead of a verdict: there the hop to the second stream is latency added to every attempt --
			// 76 -> 86 us measured -- and the sum stays behind its sweep on the compute stream.)
			const bool sum_off_stream = arkode_method;
			double *const sum_to = reduce_on_device ? c->scalar_dev + kAttemptScalar + slot : c->scalar_host + kAttemptScalar + slot;
			call.err_sum = sum_to;
			call.err_defer_sum = sum_off_stream;
			call.done_event = sum_off_stream || reduce_on_device ? c->ev_attempt[slot] : c->ev_norm[slot];
			int items = 0, inner_items = 0;
			call.err_items_out = &items;
			if (under_exchange) {
				FusedCall inner = call;
				inner.done_event = nullptr;
				inner.err_defer_sum = true;  // (the second launch, or the second stream, sums both launches' partials)
				inner.err_items_out = &inner_items;
				HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, inner, kEmbedHalo, c->nyl - kEmbedHalo, 0, 0, c->compute));
				HIP_TRY(c, hipStreamWaitEvent(c->compute, c->ev_halo, 0));
				call.err_offset = inner_items;
				HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call, -e, kEmbedHalo, c->nyl - kEmbedHalo, c->nyl + e, c->compute));
			} else {
				HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call, -e, c->nyl + e, 0, 0, c->compute));
			}
			if (sum_off_stream || reduce_on_device) HIP_TRY(c, hipStreamWaitEvent(c->comm, c->ev_attempt[slot], 0));
			if (reduce_on_device) {
				if (sum_off_stream) HIP_TRY(c, launch_sum_partials(call.err_partials, inner_items + items, sum_to, nullptr, c->comm));
				NCCL_TRY(c, g_rccl.AllReduce(c->scalar_dev + kAttemptScalar + slot, c->scalar_dev + kAttemptScalar + slot, 1, ncclDouble, ncclSum, c->nccl, c->comm));  // (every rank gets the same bits, hence takes the same decision)
				HIP_TRY(c, launch_scalar_to_host(c->scalar_dev + kAttemptScalar + slot, c->scalar_host + kAttemptScalar + slot, c->ev_norm[slot], c->comm));
			} else if (sum_off_stream) {
				HIP_TRY(c, launch_sum_partials(call.err_partials, inner_items + items, sum_to, c->ev_norm[slot], c->comm));  // (straight into page-locked memory)
			}
		}
		ext_of[dst] = multi ? e : (1 << 20);
		in_flight[slot] = true;
		return CRD_OK;
	}

	int finish_attempt(int slot, double *sum)
	{
		double acc = 0.0;
		for (int k = 0; k < n; k++) {  // (LOCAL groups: the slabs' sums added on the host in slab order)
			crd_ctx *c = cs[k];
			if (int rc = set_device(c)) return rc;
			HIP_TRY(c, hipEventSynchronize(c->ev_norm[slot]));
			acc += c->scalar_host[kAttemptScalar + slot];
		}
		in_flight[slot] = false;
		*sum = acc;
		return CRD_OK;
	}

	// CRD_ADAPT_ARKODE: one step = attempts until the error test passes (arkStep), then arkPrepareNextStep / arkCompleteStep.
	int arkode_loop()
	{
		int64_t steps_this_call = 0;
		struct {
			bool live;
			double h;
			int src, dst, slot;
		} ahead = {false, 0.0, -1, -1, 0};  // the attempt launched ahead of its predecessor's verdict
		int next_slot = 0;
		while (t < tout) {
			if (const char *why = arkode::begin_step(A, t, steps_this_call, o.max_steps)) return fail(lead, CRD_ESTATE, why);
			const int dst = R.spare;
			double dsm = 0.0;
			for (int nef = 0;;) {
				// This attempt -- unless it is already in flight: the previous step launched it ahead of its own verdict (below).
				int my_slot;
				if (ahead.live && ahead.h == A.h && ahead.src == R.cur && ahead.dst == dst) {
					my_slot = ahead.slot;
					st.launched_ahead++;
				} else {
					my_slot = next_slot;
					next_slot ^= 1;
					if (int rc = launch_attempt(t, A.h, R.cur, dst, my_slot)) return rc;
				}
				ahead.live = false;
				// The step after this one, launched BEFORE this one's error norm is known, on the assumption the integrator makes most of
				// the time on these grids: the attempt passes and the step size stays (the controller's dead band, or the cap).  If that
				// turns out wrong the launch is void -- it wrote a plane nobody needs (the one that becomes scratch once this step is
				// accepted; if this step is rejected, y_{n-1} in it is not needed either: the interpolant is built on the LAST step) --
				// and the next attempt is simply issued afresh.  The host's wait for the norm (reduction over the ranks, copy, wake-up)
				// then hides under a kernel that is already running.  No exchange is ever issued ahead.
				const int after = R.ahead();
				if (after >= 0 && t + A.h < tout && steps_this_call + 1 < o.max_steps && ext_of[dst] >= kEmbedHalo) {
					if (int rc = launch_attempt(t + A.h, A.h, dst, after, next_slot)) return rc;
					ahead = {true, A.h, dst, after, next_slot};
					next_slot ^= 1;
				}
				double sum = 0.0;
				if (int rc = finish_attempt(my_slot, &sum)) return rc;
				dsm = std::sqrt(sum / n_components);
				st.err_last = dsm;
#ifdef CRD_TUNING_BUILD
				if (std::getenv("CRD_ADAPT_TRACE")) std::fprintf(stderr, "libcrd attempt: t %.17g h %.17g sum %.17g\n", t, A.h, sum);
#endif
				if (dsm <= 1.0) break;  // (a NaN fails the test)
				ahead.live = false;     // a failed step: what was launched ahead of it is void
				if (!arkode::reject(A, dsm, &nef, o, h_cap, st)) return fail(lead, CRD_ESTATE, arkode::kErrFailure);
			}
			t_prev = t;
			arkode::accept(A, dsm, o, h_cap, t, st);
			steps_this_call++;
			R.accept(dst, dense);
		}
		return CRD_OK;
	}

	// CRD_ADAPT_RK43: the embedded pair and I-controller of rounds 1-2; every attempt is launched and waited for.
	int rk43_loop()
	{
		bool after_reject = false;
		while (t < tout) {
			if (st.accepted + st.rejected >= o.max_steps) return fail(lead, CRD_ESTATE, "adaptive integration: max_steps attempts taken before reaching tout");
			double hh = h;
			bool clipped = false;
			if (!dense && (t + hh >= tout || tout - (t + hh) < 1e-12 * std::fabs(tout))) {  // land on tout exactly; absorb a sliver of a last step
				hh = tout - t;
				clipped = true;
			}
			if (!(hh > 1e-14 * std::fmax(std::fabs(t), 1e-300)) && !(t == 0.0 && hh > 0.0)) return fail(lead, CRD_ESTATE, "adaptive integration: step size underflow");
			const int dst = R.spare;
			double sum = 0.0;
			if (int rc = launch_attempt(t, hh, R.cur, dst, 0)) return rc;
			if (int rc = finish_attempt(0, &sum)) return rc;
			const double err = o.bias * std::sqrt(sum / n_components);
			st.err_last = err;
			double eta;
			if (!(err == err) || std::isinf(err)) eta = o.shrink;  // NaN / inf: the step blew up
			else if (err <= 0.0) eta = o.growth;
			else eta = std::fmin(o.growth, std::fmax(o.shrink, o.safety * std::pow(err, -0.25)));
			if (err <= 1.0) {
				t_prev = t;
				t = clipped ? tout : t + hh;
				R.accept(dst, dense);
				st.accepted++;
				if (after_reject) eta = std::fmin(eta, 1.0);  // no growth right after a rejection
				after_reject = false;
				if (!clipped || st.accepted == 1) {
					st.h_last = hh;
					st.h_min = (st.h_min == 0.0) ? hh : std::fmin(st.h_min, hh);
					st.h_max = std::fmax(st.h_max, hh);
				}
				if (!clipped) h = hh * eta;
				else h = std::fmax(h, hh * eta);  // a step shortened to hit tout says nothing against the step it replaced
				h = std::fmin(h, h_cap);
			} else {
				st.rejected++;
				after_reject = true;
				h = hh * std::fmin(eta, 0.9);
			}
		}
		return CRD_OK;
	}

	// The end of the call, with the loop's return code: the state handed back, the controller's memory on every context, the figures.
	int end_of_call(int rc)
	{
		// No launch outlives the call -- neither a void one (issued ahead of a verdict that then went the other way) nor, on an error exit,
		// the attempt that was being waited for: their reductions and copies on the second stream still write the slots' scalars.
		for (int slot = 0; slot < 2; slot++)
			if (in_flight[slot]) {
				double ignored;
				(void)finish_attempt(slot, &ignored);
			}
		st.t_internal = t;
		if (rc == CRD_OK && dense && R.prev >= 0 && t >= tout) {
			// ARK_NORMAL: the step t_prev -> t has reached or passed tout.  f at both ends, then the cubic Hermite interpolant at tout.
			if ((rc = rhs_on_planes(cs, n, t_prev, R.prev, crd_ctx::SB)) == CRD_OK && (rc = rhs_on_planes(cs, n, t, R.cur, crd_ctx::ACC)) == CRD_OK &&
			    (rc = hand_back(t_prev, t)) == CRD_OK)
				t = tout;
		} else {  // no dense output (or a zero-length interval, or an error): hand back the state reached
			for (int k = 0; k < n; k++) arkode::end_of_call(R, false, cs[k]->dense, tout, t_prev, t).apply(cs[k]->plane);
		}
		if (arkode_method) {
			A.live = rc == CRD_OK && lead->dense.pending;
			for (int k = 1; k < n; k++) cs[k]->ark = A;
			h = A.hprime;
		}
		st.t = t;
		st.h_next = h;
		return rc;
	}
};

int integrate_adaptive_impl(crd_ctx *const *cs, int n, double t0, double tout, const crd_adaptive_options *opt_in, crd_adaptive_stats *stats)
{
	crd_ctx *lead = cs[0];
	TraceRange range("crd_integrate_adaptive");
	crd_adaptive_options o;
	crd_adaptive_defaults(&o);
	if (opt_in) o = *opt_in;
	if (!arkode::options_valid(o, t0, tout))
		return fail(lead, CRD_EINVAL, "bad adaptive options / time interval");
	if (lead->d0 > 1) return fail(lead, CRD_EINVAL, "the error-controlled integrators need phi-slabs (theta-blocks step with the staged RK4 only)");
	AdaptiveRun run(cs, n, t0, tout, o);
	bool done = false;
	if (int rc = run.prepare_contexts()) return rc;
	if (int rc = run.start(&done)) return rc;
	const int rc = done ? CRD_OK : run.end_of_call(run.arkode_method ? run.arkode_loop() : run.rk43_loop());
	if (stats) *stats = run.st;
	return rc;
}

// With a run recorder open: one sample per call, at tout, of the state handed back (plane Y) -- the ensembles' rule; a call for which
// there is no room is refused before any work.
int integrate_adaptive_recorded(crd_ctx *const *cs, int n, double t0, double tout, const crd_adaptive_options *opt, crd_adaptive_stats *stats)
{
	crd_recorder *rec = nullptr;
	if (int rc = recorder_of_call(cs, n, &rec)) return rc;
	if (rec)
		if (int rc = recorder_room(rec, 1)) return rc;
	if (int rc = integrate_adaptive_impl(cs, n, t0, tout, opt, stats)) return rc;
	return rec ? recorder_sample(rec, crd_ctx::Y, tout) : CRD_OK;
}

}  // namespace

extern "C" {

int crd_adaptive_defaults(crd_adaptive_options *o)
{
	if (!o) return CRD_EINVAL;
	o->rtol = 1.e-5;   // src/FHNmodel_torus.cpp:197
	o->atol = 1.e-10;  // :198
	o->h0 = 0.0;
	o->safety = 0.96;
	o->bias = 1.5;
	o->growth = 20.0;
	o->shrink = 0.1;
	o->max_steps = 200000;  // :372
	o->h_max = 0.0;         // automatic: the diffusion-stability bound
	o->dense_output = 1;    // ARK_NORMAL, :423
	o->method = CRD_ADAPT_ARKODE;  // the reference's integrator: ARKodeInit(mem, f, NULL, ...) = default explicit table, order 4 (:362)
	return CRD_OK;
}

int crd_integrate_adaptive(crd_ctx *c, double t0, double tout, const crd_adaptive_options *opt, crd_adaptive_stats *stats)
{
	if (!c) return CRD_EINVAL;
	if (c->halo < 0) return fail(c, CRD_ESTATE, "multi-slab context is not wired (crd_comm_attach_local / crd_comm_init_rccl)");
	if (c->halo == CRD_HALO_LOCAL) return fail(c, CRD_ESTATE, "LOCAL groups integrate through crd_group_integrate_adaptive");
	crd_ctx *one[1] = {c};
	return integrate_adaptive_recorded(one, 1, t0, tout, opt, stats);
}

int crd_group_integrate_adaptive(crd_ctx *const *ctxs, int n, double t0, double tout, const crd_adaptive_options *opt, crd_adaptive_stats *stats)
{
	if (int rc = check_group(ctxs, n)) return rc;
	if (n > 1)
		for (int k = 0; k < n; k++)
			if (ctxs[k]->halo != CRD_HALO_LOCAL) return fail(ctxs[0], CRD_ESTATE, "group is not attached");
	return integrate_adaptive_recorded(ctxs, n, t0, tout, opt, stats);
}

}  // extern "C"
