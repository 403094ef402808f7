// crd_steppers.cpp -- the time-stepping drivers behind the C ABI: classical RK4 with the staged or the fused kernels on one
// slab or on the slabs of a run (deep-halo exchange cycles), the setters and the timed entry points.  Which launch comes next is
// crd_schedule.h's; the error-controlled integrator is crd_adaptive.cpp.  Host code only.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "crd_ctx.h"
#include "crd_schedule.h"

namespace crd {

namespace {

struct StagePlan {
	int in, out;
};
const StagePlan kStages[4] = {{crd_ctx::Y, crd_ctx::SA}, {crd_ctx::SA, crd_ctx::SB}, {crd_ctx::SB, crd_ctx::SA}, {crd_ctx::SA, crd_ctx::Y}};

StageCall make_stage_call(const crd_ctx *c, int stage, double t, double dt)
{
	const StagePlan &sp = kStages[stage - 1];
	StageCall call{};
	call.stage = stage;
	call.dt = dt;
	call.absorb = absorbing(c, step::stage_time(t, dt, stage - 1)) ? 1 : 0;
	call.yin = c->planes(sp.in);
	call.y0 = c->planes(crd_ctx::Y);
	call.acc = c->planes(crd_ctx::ACC);
	call.yout = c->planes(sp.out);
	return call;
}

// Single slab: four launches per step, phi wrap inside the kernel.
int staged_step_self(crd_ctx *c, double t, double dt, hipEvent_t *k_begin, hipEvent_t *k_end)
{
	for (int stage = 1; stage <= 4; stage++) {
		const StageCall call = make_stage_call(c, stage, t, dt);
		if (stage == 2 && k_begin) HIP_TRY(c, hipEventRecord(*k_begin, c->compute));
		HIP_TRY(c, launch_stage(c->p.precision, c->desc, call, 0, c->nyl, c->compute));
		if (stage == 2 && k_end) HIP_TRY(c, hipEventRecord(*k_end, c->compute));
	}
	return CRD_OK;
}

int fused_step_self(crd_ctx *c, double t, double dt, int src, int dst, hipEvent_t *k_begin, hipEvent_t *k_end, int steps = 1)
{
	FusedCall call = make_fused_call(c, t, dt, src, dst);
	call.steps = steps;  // 2: this one launch takes the state from t to t + 2 dt
	// a sampled launch is timed by events bound to the kernel itself (start / completion), not recorded around it: a record is a barrier
	// packet, and ten of them in a 20-step timed region were 2 % of it
	if (k_begin) call.start_event = *k_begin;
	if (k_end) call.done_event = *k_end;
	HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call, 0, c->nyl, 0, 0, c->compute));
	return CRD_OK;
}

// Several slabs (LOCAL group driven by one thread, or this rank's slab under RCCL).  Per stage:
//   compute: [wait halo(in)] boundary rows 0 and nyl-1 -> record edges(out) -> interior rows
//   comm:    wait edges(out) -> exchange one ghost row of out.u -> record halo(out)
// so the exchange of stage s+1's input overlaps stage s's interior sweep.  The step's first input (Y) has its
// halo exchanged at the end of the previous step's stage 4 (or by prime_halo before the first step).
int staged_step_multi(crd_ctx *const *cs, int n, double t, double dt, bool timed_step)
{
	for (int stage = 1; stage <= 4; stage++) {
		const StagePlan &sp = kStages[stage - 1];
		for (int k = 0; k < n; k++) {
			crd_ctx *c = cs[k];
			if (int rc = set_device(c)) return rc;
			const StageCall call = make_stage_call(c, stage, t, dt);
			HIP_TRY(c, hipStreamWaitEvent(c->compute, c->ev_halo, 0));
			HIP_TRY(c, launch_stage(c->p.precision, c->desc, call, 0, 1, c->compute));
			HIP_TRY(c, launch_stage(c->p.precision, c->desc, call, c->nyl - 1, c->nyl, c->compute));
			HIP_TRY(c, hipEventRecord(c->ev_edges, c->compute));
		}
		// start moving the edge rows of `out` while the interiors run
		if (int rc = exchange_stage_input(cs, n, sp.out, 1, false)) return rc;
		for (int k = 0; k < n; k++) {
			crd_ctx *c = cs[k];
			if (int rc = set_device(c)) return rc;
			const StageCall call = make_stage_call(c, stage, t, dt);
			const bool timed = timed_step && stage == 2 && !c->ev_k.empty();
			if (timed) c->timed_steps = 1;
			if (timed) HIP_TRY(c, hipEventRecord(c->ev_k[0], c->compute));
			HIP_TRY(c, launch_stage(c->p.precision, c->desc, call, 1, c->nyl - 1, c->compute));
			if (timed) HIP_TRY(c, hipEventRecord(c->ev_k[1], c->compute));
		}
	}
	return CRD_OK;
}

// 2-D blocks (theta split: a LOCAL group driven by one thread).  Per stage: [wait halo(in)] all rows of the block -> pack the
// output's edge columns -> record edges; then every block pulls one ghost row / column strip of the output from its neighbours.
// No boundary / interior overlap here: the layout exists to reproduce the reference's `-np 4` file for file, the fast layout on
// one node is phi-slabs.
int staged_step_blocks(crd_ctx *const *cs, int n, double t, double dt)
{
	for (int stage = 1; stage <= 4; stage++) {
		const StagePlan &sp = kStages[stage - 1];
		for (int k = 0; k < n; k++) {
			crd_ctx *c = cs[k];
			if (int rc = set_device(c)) return rc;
			StageCall call = make_stage_call(c, stage, t, dt);
			call.gcol_w = c->gcol[sp.in][0];
			call.gcol_e = c->gcol[sp.in][1];
			HIP_TRY(c, hipStreamWaitEvent(c->compute, c->ev_halo, 0));
			HIP_TRY(c, launch_stage(c->p.precision, c->desc, call, 0, c->nyl, c->compute));
			if (c->d0 > 1)
				HIP_TRY(c, launch_plane_cols_extract(c->p.precision, c->plane[sp.out][0], c->ecol[sp.out][0], c->ecol[sp.out][1], c->nx, c->nyl, c->compute));
			HIP_TRY(c, hipEventRecord(c->ev_edges, c->compute));
		}
		if (int rc = exchange_block_input(cs, n, sp.out)) return rc;
	}
	return CRD_OK;
}

// Fused stepper on several slabs: ONE exchange every E = exchange_every steps (crd_set_exchange_period; by default 8, 10 where every slab has 256 rows or more: crd_create), G = 4 E ghost
// rows of both fields.  Step q of a cycle (q = 0 right after an exchange) produces rows [-e, nyl + e) with e = 4 (E-1-q): the
// still-valid part of the ghost region is recomputed redundantly (same kernel, same inputs, so bit-identical to what the owning
// slab computes) instead of being communicated.  The last step of a cycle (e = 0) is split
//   compute: edge bands [0, B) and [nyl-B, nyl) in one small launch -> record edges        (B = max(32, G): every row the exchange sends)
//   comm:    wait edges -> exchange G rows of u and v with the ring neighbours -> record halo
//   compute: interior [B, nyl-B) (needs neither ghost rows nor the bands)
// and so is the first step of the next cycle
//   compute: rows [4, nyl-4), which read owned rows only, straight after the interior sweep
//   compute: [wait halo] rows [-e, 4) and [nyl-4, nyl+e), the ones that read ghost rows, in one small launch (e = G - 4)
// so the exchange has two sweeps to hide under (three with crd_set_halo_slack(ctx, 2)).  Per step that is 1 + 2 / E launches and
// 1 / E of an RCCL group on the host, against 3 launches + 1 group for a per-step exchange.
inline int cycle_steps(const crd_ctx *c) { return c->exchange_every; }
inline int cycle_ghost(const crd_ctx *c) { return kStepHalo * c->exchange_every; }
inline int cycle_band(const crd_ctx *c) { return std::max(32, cycle_ghost(c)); }

// The compute stream's wait for the halo of the exchange just made (and, in a LOCAL group, for the neighbours to have pulled
// theirs out of this context's planes), with the diagnostics' event pair around it.
int wait_for_halo(crd_ctx *c)
{
	// (diagnostics: how long does the compute stream stand at this wait?  Zero when the exchange hid under the sweeps)
	const bool diag = c->diag_active && 4 * c->diag_waits + 1 < (int)c->ev_diag.size();
	if (diag) HIP_TRY(c, hipEventRecord(c->ev_diag[(size_t)(4 * c->diag_waits)], c->compute));
	HIP_TRY(c, hipStreamWaitEvent(c->compute, c->ev_halo, 0));
	if (diag) HIP_TRY(c, hipEventRecord(c->ev_diag[(size_t)(4 * c->diag_waits++ + 1)], c->compute));
	if (c->halo == CRD_HALO_LOCAL) {
		// LOCAL halos are PULLED by the neighbours from this context's planes: the next launch that overwrites those rows must not
		// start before both neighbours have finished copying them
		HIP_TRY(c, hipStreamWaitEvent(c->compute, c->group[(size_t)((c->slab + c->n_slabs - 1) % c->n_slabs)]->ev_halo, 0));
		HIP_TRY(c, hipStreamWaitEvent(c->compute, c->group[(size_t)((c->slab + 1) % c->n_slabs)]->ev_halo, 0));
	}
	return CRD_OK;
}

// One launch of the cycle on every context of the call: `nsub` steps (1, or 2 / 3 with a plan of several steps per launch: the launch
// must not straddle an exchange, q + nsub <= E) from cycle position q.  What the launch's three cases share:
struct CycleLaunch {
	double t, dt;
	int src, dst, q, nsub, max_nsub;
	bool timed_step, last_launch_of_call;
	int E, G, B;
	int H() const { return kStepHalo * nsub; }              // rows consumed beyond the rows produced
	int ext() const { return kStepHalo * (E - q - nsub); }  // ghost rows still valid once this launch has run
	FusedCall call(const crd_ctx *c, double tt, int from, int to, int steps) const
	{
		FusedCall call = make_fused_call(c, tt, dt, from, to);
		call.steps = steps;
		return call;
	}
	FusedCall call(const crd_ctx *c) const { return call(c, t, src, dst, nsub); }
};

// Middle of the cycle: one full-height sweep (nothing to record: the next launch runs on the same stream).
int cycle_middle(crd_ctx *c, const CycleLaunch &L)
{
	const FusedCall call = L.call(c);
	const bool timed = L.timed_step && !c->ev_k.empty();
	if (timed) HIP_TRY(c, hipEventRecord(c->ev_k[0], c->compute));
	HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call, -L.ext(), c->nyl + L.ext(), 0, 0, c->compute));
	if (timed) HIP_TRY(c, hipEventRecord(c->ev_k[1], c->compute));
	if (timed) c->timed_rows = c->nyl + 2 * L.ext();  // what crd_dominant_kernel_rows reports for this launch
	if (timed) c->timed_steps = L.nsub;
	return CRD_OK;
}

// First launch after an exchange.  Output rows [H, nyl - H) read owned rows only, so they are launched straight behind the interior
// sweep of the previous launch: the exchange gets this sweep as extra time to land.
int cycle_first(crd_ctx *c, const CycleLaunch &L)
{
	const FusedCall call = L.call(c);
	const int H = L.H(), ext = L.ext();
	const bool split = c->nyl >= 4 * L.B;
	if (split) HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call, H, c->nyl - H, 0, 0, c->compute));
	if (split && c->halo_slack >= 2 && !L.last_launch_of_call && L.q + L.nsub + L.max_nsub < L.E) {  // (whatever the next launch takes -- up to max_nsub steps --, it is not the cycle's last)
		c->ghost_deferred = true;  // the wait and the rows that read ghost rows follow behind the NEXT launch's owned-only rows
		c->deferred_t = L.t;
		c->deferred_nsub = L.nsub;
		return CRD_OK;
	}
	if (int rc = wait_for_halo(c)) return rc;
	// the rows that read ghost rows: [-ext, H) and [nyl - H, nyl + ext) in one launch
	if (split) HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call, -ext, H, c->nyl - H, c->nyl + ext, c->compute));
	else HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call, -ext, c->nyl + ext, 0, 0, c->compute));
	return CRD_OK;
}

// ... its deferred form.  Halo slack 2 (crd_set_halo_slack): the exchange gets a THIRD sweep to land under.  The cycle's first launch
// has only produced its rows that read owned rows; this one does the same -- rows [B, nyl - B) only, B = the band the exchange sends
// from / the neighbours pull from, which nobody may overwrite before the exchange is through -- and only then the compute stream
// waits, finishes the first launch (the rows that read ghost rows) and this one (its edges).
int cycle_first_deferred(crd_ctx *c, const CycleLaunch &L)
{
	const FusedCall call = L.call(c);
	const int B = L.B, ext = L.ext(), n0 = c->deferred_nsub, H0 = kStepHalo * n0, ext0 = kStepHalo * (L.E - n0);
	const FusedCall call0 = L.call(c, c->deferred_t, L.dst, L.src, n0);  // the first launch read this launch's output plane and wrote its input plane
	HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call, B, c->nyl - B, 0, 0, c->compute));
	if (int rc = wait_for_halo(c)) return rc;
	HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call0, -ext0, H0, c->nyl - H0, c->nyl + ext0, c->compute));
	HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call, -ext, B, c->nyl - B, c->nyl + ext, c->compute));
	c->ghost_deferred = false;
	return CRD_OK;
}

// Last launch of the cycle: edge bands, exchange released behind them, interior under the exchange.
int cycle_last(crd_ctx *const *cs, int n, const CycleLaunch &L)
{
	const int B = L.B;
	for (int k = 0; k < n; k++) {
		crd_ctx *c = cs[k];
		if (int rc = set_device(c)) return rc;
		FusedCall call = L.call(c);
		call.done_event = c->ev_edges;  // (set by the launch's own completion: no record, no bubble in front of the interior launch)
		if (c->nyl >= 4 * B) HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call, 0, B, c->nyl - B, c->nyl, c->compute));
		else HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call, 0, c->nyl, 0, 0, c->compute));
	}
	if (int rc = exchange_stage_input(cs, n, L.dst, L.G, true)) return rc;
	for (int k = 0; k < n; k++) {
		crd_ctx *c = cs[k];
		if (int rc = set_device(c)) return rc;
		if (c->nyl >= 4 * B) HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, L.call(c), B, c->nyl - B, 0, 0, c->compute));
	}
	return CRD_OK;
}

int fused_launch_multi(crd_ctx *const *cs, int n, const CycleLaunch &L)
{
	if (L.q + L.nsub >= L.E) return cycle_last(cs, n, L);
	for (int k = 0; k < n; k++) {
		crd_ctx *c = cs[k];
		if (int rc = set_device(c)) return rc;
		if (int rc = c->ghost_deferred ? cycle_first_deferred(c, L) : L.q > 0 ? cycle_middle(c, L) : cycle_first(c, L)) return rc;
	}
	return CRD_OK;
}

// Step of an exchange cycle whose single full-slab launch is the one timed in a multi-slab fused run (step 0 is split in two).
constexpr int kTimedCycleStep = 1;

int ensure_timing_events(crd_ctx *c)
{
	while ((int)c->ev_k.size() < 2 * step::kMaxTimedLaunches) {
		hipEvent_t e;
		HIP_TRY(c, hipEventCreate(&e));
		c->ev_k.push_back(e);
	}
	return CRD_OK;
}

}  // namespace

// RCCL runs: one decision for the whole ring on where in the exchange cycle the call starts (see crd_ctx::agree_dev).  begin_
// enqueues the reduction on the comm stream and returns; finish_ waits for it.  Every rank of the run makes both calls in every
// fused stepping call, before any other RCCL operation of that call.
int begin_cycle_agreement(crd_ctx *c, int mine)
{
	if (!c->agree_dev) {
		HIP_TRY(c, hipMalloc((void **)&c->agree_dev, 2 * sizeof(double)));
		HIP_TRY(c, hipHostMalloc((void **)&c->agree_host, 4 * sizeof(double), hipHostMallocDefault));
		HIP_TRY(c, hipEventCreateWithFlags(&c->ev_agree, hipEventDisableTiming));
	}
	if (crd_cycle_vote(mine, c->agree_host) != CRD_OK) return fail(c, CRD_ESTATE, "exchange-cycle position out of range");
	HIP_TRY(c, hipMemcpyAsync(c->agree_dev, c->agree_host, 2 * sizeof(double), hipMemcpyHostToDevice, c->comm));
	NCCL_TRY(c, g_rccl.AllReduce(c->agree_dev, c->agree_dev, 2, ncclDouble, ncclMin, c->nccl, c->comm));
	HIP_TRY(c, hipMemcpyAsync(c->agree_host + 2, c->agree_dev, 2 * sizeof(double), hipMemcpyDeviceToHost, c->comm));
	HIP_TRY(c, hipEventRecord(c->ev_agree, c->comm));
	return CRD_OK;
}

int finish_cycle_agreement(crd_ctx *c, int *agreed)
{
	HIP_TRY(c, hipEventSynchronize(c->ev_agree));
	*agreed = crd_cycle_agreed(c->agree_host + 2);
	return CRD_OK;
}

void decide_cycle_start(crd_ctx *const *all, int n_all)
{
	int q0 = all[0]->cycle_pos;
	for (int k = 0; k < n_all; k++)
		if (all[k]->cycle_pos != q0 || all[k]->cycle_pos < 0) q0 = -1;
	for (int k = 0; k < n_all; k++) all[k]->cycle_start = q0;
}

FusedCall make_fused_call(const crd_ctx *c, double t, double dt, int src, int dst)
{
	FusedCall call{};
	call.dt = dt;
	step::stage_flags(t, dt, c->p.t_boundary, 4, call.absorb);
	step::stage_flags(t + dt, dt, c->p.t_boundary, 4, call.absorb2);         // the step after this one, as the stepping loop forms its time
	step::stage_flags((t + dt) + dt, dt, c->p.t_boundary, 4, call.absorb3);  // ... and the one after that (three-step launches)
	call.absorb[4] = call.absorb[3];  // (the embedded pairs' fifth stage: set by the adaptive integrator)
	call.y0 = c->planes(src);
	call.yout = c->planes(dst);
	call.plan = const_cast<FusedPlan *>(&c->plan);
	// (ACC is the staged stepper's accumulator and a temporary of arkHin / the Hermite output: free whenever a one-launch step runs)
	if (src != crd_ctx::ACC && dst != crd_ctx::ACC) call.tune_scratch = c->planes(crd_ctx::ACC);
	return call;
}

namespace {

// What a stepping call was asked for, and the run recorder's part in it (rec_stride 0: none).  With a recorder only the grouping of
// steps into launches changes: no pair, triple or deferred launch straddles a sample -- `lim(s)` is where the steps that may share a
// launch with step s end.  Times are formed from t0 and the step's index in the call as ever.
struct StepCall {
	crd_ctx *const *cs;
	int n;
	double t0, dt;
	int64_t nsteps;
	bool timing;
	crd_recorder *rec;
	int64_t rec_stride, rec_steps;
	int stepper;
	double time(int64_t s) const { return t0 + (double)s * dt; }
	int64_t lim(int64_t s) const { return step::sample_limit(s, nsteps, rec_stride, rec_steps); }
	int sample(int64_t s, int plane) const { return step::sample_due(s, rec_stride, rec_steps) ? recorder_sample(rec, plane, time(s)) : CRD_OK; }  // s: steps taken so far
};

// A call that ends on an odd number of fused launches has its result in SA: swap the plane pointers.
void result_into_Y(crd_ctx *const *cs, int n, int cur)
{
	for (int k = 0; k < n && cur != crd_ctx::Y; k++) {
		std::swap(cs[k]->plane[crd_ctx::Y][0], cs[k]->plane[crd_ctx::SA][0]);
		std::swap(cs[k]->plane[crd_ctx::Y][1], cs[k]->plane[crd_ctx::SA][1]);
	}
}

// theta-blocks: staged kernels, every block of the run in this one call
int run_blocks(const StepCall &a)
{
	crd_ctx *const *cs = a.cs;
	if (cs[0]->halo != CRD_HALO_LOCAL || a.n != cs[0]->n_slabs) return fail(cs[0], CRD_ESTATE, "theta-blocks step as a LOCAL group holding every block of the run");
	for (int k = 0; k < a.n; k++) cs[k]->cycle_pos = -1;
	if (a.nsteps > 0)
		if (int rc = prime_block_halo(cs, a.n, crd_ctx::Y)) return rc;
	for (int64_t s = 0; s < a.nsteps; s++)
		if (int rc = staged_step_blocks(cs, a.n, a.time(s), a.dt)) return rc;
	for (int k = 0; k < a.n; k++) {
		if (int rc = set_device(cs[k])) return rc;
		HIP_TRY(cs[k], hipStreamWaitEvent(cs[k]->compute, cs[k]->ev_halo, 0));
	}
	return CRD_OK;
}

int run_single(const StepCall &a, int *timed_out)
{
	crd_ctx *c = a.cs[0];
	if (int rc = set_device(c)) return rc;
	const bool f64 = c->p.precision == CRD_PRECISION_F64;  // (its three-step kernel has the instantiation with the absorbing rows' selects)
	int cur = crd_ctx::Y, timed = 0;
	for (int64_t s = 0; s < a.nsteps;) {
		const double t = a.time(s);
		hipEvent_t *kb = nullptr, *ke = nullptr;
		// The plan may say "two steps per launch" (measured -- by this call's first launch, perhaps --, or pinned): pairs while two steps
		// are left, a single-step launch for an odd last one; a three-step plan: triples while three steps are left, then a pair or a
		// single step (crd_schedule.h).
		const int per_launch = (a.stepper == CRD_STEPPER_FUSED && c->plan.tuned) ? fused_steps_supported(c->p.precision, c->desc, c->plan.steps) : 1;
		int rc, took = step::launch_steps(per_launch, f64, a.t0, a.dt, c->p.t_boundary, s, a.lim(s));
		if (a.timing && step::timed_here(step::timed_kind(per_launch, f64, a.t0, a.dt, c->p.t_boundary, a.nsteps), took, s, a.nsteps, timed)) {
			kb = &c->ev_k[(size_t)(2 * timed)];
			ke = &c->ev_k[(size_t)(2 * timed + 1)];
			timed++;
			c->timed_steps = took;
		}
		if (a.stepper == CRD_STEPPER_STAGED) {
			rc = staged_step_self(c, t, a.dt, kb, ke);
		} else {
			const int dst = (cur == crd_ctx::Y) ? crd_ctx::SA : crd_ctx::Y;
			rc = fused_step_self(c, t, a.dt, cur, dst, kb, ke, took);
			cur = dst;
		}
		if (rc) return rc;
		s += took;
		if (int rs = a.sample(s, a.stepper == CRD_STEPPER_STAGED ? (int)crd_ctx::Y : cur)) return rs;
	}
	result_into_Y(a.cs, 1, cur);
	*timed_out = timed;
	return CRD_OK;
}

// Where in the exchange cycle does the resident state stand?  If the previous call left it mid-cycle (or right after an exchange) the
// ghost rows are as good as they need to be and this call carries on from there; otherwise -- new state, staged stepper, slabs that
// disagree -- it starts with an exchange.  (A 20-step call on an 8192 x 1024 slab is 1.2 ms: an exposed exchange in front of it is
// several per cent.)
// Under RCCL (`ring`) that decision has to be the RING's, not this rank's: a rank that alone holds a new state (an upload on that
// rank only, a failed call) would prime its halo while its neighbours carry on, and the ring's send / receive sequences would no
// longer pair.  So the ranks reduce their positions first.  The reduction (and the host's wait for it) hides under the call's first
// step wherever that step involves no exchange of its own (q0 = 0 .. E - 4: the step is issued speculatively into the scratch planes
// and simply issued again, behind an exchange, if the ring turns out to disagree): *agreement_pending.
int resolve_cycle_start(const StepCall &a, bool fused, bool ring, int E, int *q0_out, bool *agreement_pending)
{
	crd_ctx *const *cs = a.cs;
	crd_ctx *lead = cs[0];
	int q0 = fused ? lead->cycle_start : -1;  // (decide_cycle_start: one decision for every slab of the run)
	if (a.nsteps > 0) {
		for (int k = 0; k < a.n; k++) cs[k]->cycle_pos = -1;  // until this call has gone through
		for (int k = 0; k < a.n; k++) cs[k]->ghost_deferred = false;  // (a call always finishes what its last step deferred)
		if (ring) {
			if (int rc = begin_cycle_agreement(lead, q0)) return rc;
			*agreement_pending = true;
			if (q0 < 0 || q0 >= E - 3) {  // nothing to issue ahead of the answer (the call's first launch may be the cycle's last: a pair, or -- fp32 -- a triple)
				if (int rc = finish_cycle_agreement(lead, &q0)) return rc;
				*agreement_pending = false;
			}
		}
		if (q0 < 0) {
			if (ring && lead->cycle_start >= 0) lead->agreement_restarts++;
			if (int rc = prime_halo(cs, a.n, crd_ctx::Y, fused ? cycle_ghost(lead) : 1, fused)) return rc;
			q0 = 0;
		}
	}
	*q0_out = q0;
	return CRD_OK;
}

// The ring disagreed with the position the call's first launch was issued from: some rank holds a new state, every rank starts
// afresh.  The launch just issued wrote the scratch planes only (plane Y is untouched) and is overwritten by the one the caller
// issues again from step 0, in stream order.
int start_afresh(const StepCall &a)
{
	a.cs[0]->agreement_restarts++;
	for (int k = 0; k < a.n; k++) a.cs[k]->ghost_deferred = false;  // (the launch issued ahead of the answer is void, and so is what it deferred)
	return prime_halo(a.cs, a.n, crd_ctx::Y, cycle_ghost(a.cs[0]), true);
}

int run_slabs(const StepCall &a, int *timed_out)
{
	crd_ctx *const *cs = a.cs;
	crd_ctx *lead = cs[0];
	const int n = a.n;
	const bool fused = (a.stepper == CRD_STEPPER_FUSED);
	const int E = cycle_steps(lead);
	for (int k = 0; k < n; k++)
		if (cs[k]->exchange_every != E) return fail(lead, CRD_EINVAL, "contexts of one run disagree on the exchange period");
	int q0 = -1;
	bool agreement_pending = false;
	if (int rc = resolve_cycle_start(a, fused, fused && n == 1 && lead->halo == CRD_HALO_RCCL, E, &q0, &agreement_pending)) return rc;
	int cur = crd_ctx::Y, timed = 0;
	// Two steps per launch where the lead context's plan says so (measured, or pinned): pairs that do not straddle an exchange.
	// Where the exchanges fall in the step sequence does not depend on the pairing, so the ranks of a ring / the threads of a group
	// may pair differently (each by its own plan) and still meet at the same collectives.
	// Three where the three-step kernel takes slabs (fp32: a strip per wavefront; fp64's block strip measured nothing on a rank's
	// share and keeps pairs: fused_steps_supported), by the same rule -- a triple never straddles an exchange either.
	bool pairs = fused && lead->plan.tuned && lead->plan.steps >= 2;
	for (int k = 0; k < n; k++) pairs = pairs && fused_two_steps_supported(cs[k]->desc);
	bool triples = pairs && lead->plan.steps == 3;
	for (int k = 0; k < n; k++) triples = triples && fused_steps_supported(cs[k]->p.precision, cs[k]->desc, 3) == 3;
	for (int64_t s = 0; s < a.nsteps;) {
		const int q = (int)((s + q0) % E);
		const int64_t end = a.lim(s);
		const int nsub = step::launch_steps(triples ? 3 : pairs ? 2 : 1, false, a.t0, a.dt, lead->p.t_boundary, s, end, q, E);
		bool finishes_deferred = false;
		for (int k = 0; k < n; k++) finishes_deferred = finishes_deferred || cs[k]->ghost_deferred;
		const bool timed_step = a.timing && !timed && step::timed_slab_launch(fused, q, nsub, E, finishes_deferred, s, a.nsteps);
		if (fused) {
			const int dst = (cur == crd_ctx::Y) ? crd_ctx::SA : crd_ctx::Y;
			const CycleLaunch L{a.time(s), a.dt, cur, dst, q, nsub, triples ? 3 : 2, timed_step, s + nsub == end, E, cycle_ghost(lead), cycle_band(lead)};
			if (int rc = fused_launch_multi(cs, n, L)) return rc;
			cur = dst;
		} else if (int rc = staged_step_multi(cs, n, a.time(s), a.dt, timed_step)) {
			return rc;
		}
		if (timed_step) timed = 1;
		s += nsub;
		if (agreement_pending) {  // the first launch is on its way: now hear what the ring says
			int agreed = -1;
			if (int rc = finish_cycle_agreement(lead, &agreed)) return rc;
			agreement_pending = false;
			if (agreed != q0) {
				if (int rc = start_afresh(a)) return rc;
				q0 = 0, cur = crd_ctx::Y, timed = 0, s = 0;
			}
		}
		// (the sample reads owned rows, which only this compute stream writes: it is behind the cycle's last step wherever that step
		// was split around an exchange, and the exchange itself -- the second stream -- writes ghost rows only)
		if (int rs = a.sample(s, fused ? cur : (int)crd_ctx::Y)) return rs;
	}
	// (several issuing threads: the neighbours read this thread's plane pointers while they enqueue their pulls)
	if (lead->bar && !lead->bar->wait()) return fail(lead, CRD_ESTATE, "another slab's issuing thread failed");
	result_into_Y(cs, n, cur);
	// leave the compute stream of every context ordered behind its last band launch and exchange
	for (int k = 0; k < n; k++) {
		if (int rc = set_device(cs[k])) return rc;
		HIP_TRY(cs[k], hipStreamWaitEvent(cs[k]->compute, cs[k]->ev_edges, 0));
		HIP_TRY(cs[k], hipStreamWaitEvent(cs[k]->compute, cs[k]->ev_halo, 0));
	}
	if (fused && a.nsteps > 0)
		for (int k = 0; k < n; k++) cs[k]->cycle_pos = (int)((q0 + a.nsteps) % E);
	*timed_out = timed;
	return CRD_OK;
}

}  // namespace

// The stepping loop shared by crd_step_rk4 / crd_step_rk4_timed / the group call: validation and the recorder's room here, then the
// run by layout.  A call that would overrun the recorder is refused whole, before anything is launched.
int run_steps(crd_ctx *const *cs, int n, double t0, double dt, int64_t nsteps, int *timed_launches, crd_recorder *rec)
{
	crd_ctx *lead = cs[0];
	if (nsteps < 0 || !(dt > 0.0) || !std::isfinite(t0)) return fail(lead, CRD_EINVAL, "bad t0 / dt / nsteps");
	const int64_t rec_stride = rec ? recorder_stride(rec) : 0, rec_steps = rec ? recorder_steps(rec) : 0;
	if (rec)
		if (int rc = recorder_room(rec, (rec_steps + nsteps) / rec_stride - rec_steps / rec_stride)) return rc;
	const int stepper = resolve_stepper(lead);
	if (stepper < 0) return fail(lead, CRD_EINVAL, "fused stepper not available for this configuration");
	for (int k = 0; k < n; k++) arkode::drop(cs[k]->dense, cs[k]->ark);  // stepping on from the state handed back, not from the integrator's internal one
	if (nsteps > 0)
		for (int k = 0; k < n; k++) cs[k]->last_step_t = t0 + (double)(nsteps - 1) * dt, cs[k]->last_step_dt = dt;
	if (stepper != CRD_STEPPER_FUSED)
		for (int k = 0; k < n; k++) cs[k]->cycle_pos = -1;  // the staged stepper keeps one ghost row of one field current, not the deep halo
	for (int k = 0; k < n; k++)
		if (resolve_stepper(cs[k]) != stepper) return fail(lead, CRD_EINVAL, "contexts of one run disagree on the stepper");
	const StepCall a{cs, n, t0, dt, nsteps, timed_launches != nullptr, rec, rec_stride, rec_steps, stepper};
	int timed = 0;
	if (lead->d0 > 1) {
		if (int rc = run_blocks(a)) return rc;
		if (timed_launches) *timed_launches = 0;
		return CRD_OK;
	}
	if (int rc = lead->halo == CRD_HALO_SELF ? run_single(a, &timed) : run_slabs(a, &timed)) return rc;
	if (timed_launches) *timed_launches = timed;
	if (rec) recorder_advance(rec, nsteps);
	return CRD_OK;
}

}  // namespace crd

using namespace crd;

extern "C" {

int crd_set_stepper(crd_ctx *c, int stepper)
{
	if (!c) return CRD_EINVAL;
	if (stepper != CRD_STEPPER_AUTO && stepper != CRD_STEPPER_STAGED && stepper != CRD_STEPPER_FUSED) return fail(c, CRD_EINVAL, "unknown stepper");
	const int before = c->stepper;
	c->stepper = stepper;
	if (stepper == CRD_STEPPER_FUSED && resolve_stepper(c) < 0) {
		c->stepper = before;
		return fail(c, CRD_EINVAL, "fused stepper not available for this configuration (slab too short)");
	}
	return CRD_OK;
}

int crd_step_rk4(crd_ctx *c, double t0, double dt, int64_t nsteps)
{
	if (!c) return CRD_EINVAL;
	if (c->halo < 0) return fail(c, CRD_ESTATE, "multi-slab context is not wired (crd_comm_attach_local / crd_comm_init_rccl)");
	if (c->halo == CRD_HALO_LOCAL) return fail(c, CRD_ESTATE, "LOCAL groups step through crd_group_step_rk4");
	crd_ctx *one[1] = {c};
	crd_recorder *rec = nullptr;
	if (int rc = recorder_of_call(one, 1, &rec)) return rc;
	decide_cycle_start(one, 1);
	TraceRange range("crd_step_rk4");
	return run_steps(one, 1, t0, dt, nsteps, nullptr, rec);
}

// LOCAL groups spread over several devices get one issuing thread per device: a single thread that enqueues every launch, event
// and peer copy of every GPU becomes the bottleneck once a GPU's share of a step is short (an 8192 x 1024 slab steps in ~60 us,
// a thread needs a good part of that to issue one GPU's work).  The threads run the same step loop on their own contexts and meet
// at the group's rendezvous around every halo exchange.  crd_group_set_threads(ctxs, n, k) forces k threads (also on one device:
// how the tests exercise the rendezvous on a one-GPU box), k = 1 the single-thread path.
static int group_step(crd_ctx *const *ctxs, int n, double t0, double dt, int64_t nsteps, bool timed)
{
	crd_recorder *rec = nullptr;
	if (ctxs && n >= 1 && ctxs[0])
		if (int rc = recorder_of_call(ctxs, n, &rec)) return rc;  // (a recorded group steps whole: CRD_ESTATE for a part of it)
	if (int rc = check_group(ctxs, n)) return rc;
	if (n > 1)
		for (int k = 0; k < n; k++)
			if (ctxs[k]->halo != CRD_HALO_LOCAL) return fail(ctxs[0], CRD_ESTATE, "group is not attached");
	// contiguous runs of slabs per thread: by device, or by the knob
	std::vector<int> first{0};
	const int forced = ctxs[0]->group_threads;  // crd_group_set_threads: 0 = one per device
	if (forced > 1) {
		const int t = std::min(forced, n);
		for (int q = 1; q < t; q++) first.push_back((int)((long)n * q / t));
	} else if (forced == 0) {
		for (int k = 1; k < n; k++)
			if (ctxs[k]->device != ctxs[k - 1]->device) first.push_back(k);
	}
	if (ctxs[0]->d0 > 1) first.assign(1, 0);  // theta-blocks: one issuing thread
	if (rec) first.assign(1, 0);              // a recorded group: one thread issues the steps and, between them, the samples
	const int nthreads = (int)first.size();
	decide_cycle_start(ctxs, n);
	TraceRange range("crd_group_step_rk4");
	std::vector<int> timed_of((size_t)nthreads, 0);
	if (nthreads <= 1 || nsteps <= 0) return run_steps(ctxs, n, t0, dt, nsteps, timed ? &timed_of[0] : nullptr, rec);
	first.push_back(n);
	GroupBarrier bar;
	bar.members = nthreads;
	for (int k = 0; k < n; k++) ctxs[k]->bar = &bar;
	std::vector<int> rcs((size_t)nthreads, CRD_OK);
	auto work = [&](int q) {
		rcs[(size_t)q] = run_steps(ctxs + first[(size_t)q], first[(size_t)q + 1] - first[(size_t)q], t0, dt, nsteps, timed ? &timed_of[(size_t)q] : nullptr, nullptr);  // (a recorded group runs on one thread, above)
		if (rcs[(size_t)q] != CRD_OK) bar.leave_failed();
	};
	std::vector<std::thread> pool;
	for (int q = 1; q < nthreads; q++) pool.emplace_back(work, q);
	work(0);
	for (auto &th : pool) th.join();
	for (int k = 0; k < n; k++) ctxs[k]->bar = nullptr;
	for (int q = 0; q < nthreads; q++)
		if (rcs[(size_t)q] != CRD_OK) {
			if (q > 0 && ctxs[0]->err.empty()) ctxs[0]->err = ctxs[first[(size_t)q]]->err;  // the caller asks the first context for the text
			return rcs[(size_t)q];
		}
	return CRD_OK;
}

int crd_plan_launches(crd_ctx *c)
{
	if (!c) return CRD_EINVAL;
	if (int rc = set_device(c)) return rc;
	if (int rc = ensure_timing_events(c)) return rc;  // (a first crd_step_rk4_timed would otherwise create its 128 events inside the region it times)
	if (resolve_stepper(c) != CRD_STEPPER_FUSED || c->plan.tuned || !c->plan.autotune) return CRD_OK;
	// After a dense-output call the "scratch" plane SA holds the integrator's own state y_{n+1}, which a resumed
	// crd_integrate_adaptive continues from: leave it alone (the plan is then measured by the first fixed-step launch instead).
	if (c->dense.pending) return CRD_OK;
	// One step of the resident state into the scratch planes, discarded: its first launch is where the plan is measured.  The
	// state itself (plane Y) is only read; ghost rows may be stale, which only matters to results nobody keeps.
	FusedCall call = make_fused_call(c, 0.0, 1e-9 * crd_stable_dt(&c->p), crd_ctx::Y, crd_ctx::SA);
	for (int k = 0; k < 5; k++) call.absorb[k] = 0;
	const int lo = c->halo == CRD_HALO_SELF ? 0 : kStepHalo, hi = c->halo == CRD_HALO_SELF ? c->nyl : c->nyl - kStepHalo;
	HIP_TRY(c, launch_fused_step(c->p.precision, c->desc, call, lo, hi, 0, 0, c->compute));
	HIP_TRY(c, hipStreamSynchronize(c->compute));
	return CRD_OK;
}

int crd_group_set_threads(crd_ctx *const *ctxs, int n, int threads)
{
	if (int rc = check_group(ctxs, n)) return rc;
	if (threads < 0) return fail(ctxs[0], CRD_EINVAL, "issuing threads: 0 = one per device, k >= 1 = exactly k");
	ctxs[0]->group_threads = threads;
	return CRD_OK;
}

int crd_set_exchange_period(crd_ctx *c, int steps)
{
	if (!c) return CRD_EINVAL;
	if (steps < kMinExchangeEvery || steps > kMaxExchangeEvery) return fail(c, CRD_EINVAL, "exchange period: 3 .. 16 steps");
	if (c->exchange_every != steps) c->cycle_pos = -1;  // the ghost rows were exchanged for another cycle length
	c->exchange_every = steps;
	return CRD_OK;
}

int crd_get_exchange_period(const crd_ctx *c) { return c ? c->exchange_every : CRD_EINVAL; }

int crd_set_halo_slack(crd_ctx *c, int sweeps)
{
	if (!c) return CRD_EINVAL;
	if (sweeps != 1 && sweeps != 2) return fail(c, CRD_EINVAL, "halo slack is 1 or 2 sweeps");
	c->halo_slack = sweeps;
	return CRD_OK;
}

int crd_set_diagnostics(crd_ctx *c, int on)
{
	if (!c) return CRD_EINVAL;
	c->diagnostics = on != 0;
	return CRD_OK;
}

int crd_get_step_timing(const crd_ctx *c, crd_step_timing *out)
{
	if (!c || !out) return CRD_EINVAL;
	*out = c->timing;
	out->agreement_restarts = c->agreement_restarts;
	return CRD_OK;
}

int crd_group_step_rk4(crd_ctx *const *ctxs, int n, double t0, double dt, int64_t nsteps) { return group_step(ctxs, n, t0, dt, nsteps, false); }

// The group call with the clocks of crd_step_rk4_timed on every slab: an event pair around the batch on each context's compute stream
// and one around ONE full-height launch of the dominant kernel per context, mid-run (a launch of the exchange cycle that is neither
// its split first nor its split last).  Returns when every slab's last step is done; crd_get_step_timing(ctxs[k]) has slab k's figures.
int crd_group_step_rk4_timed(crd_ctx *const *ctxs, int n, double t0, double dt, int64_t nsteps)
{
	if (int rc = check_group(ctxs, n)) return rc;
	for (int k = 0; k < n; k++) {
		crd_ctx *c = ctxs[k];
		if (int rc = set_device(c)) return rc;
		if (int rc = ensure_timing_events(c)) return rc;
		c->timed_rows = c->timed_steps = 0;
		c->timing = crd_step_timing{};
		HIP_TRY(c, hipEventRecord(c->ev_t0, c->compute));
	}
	if (int rc = group_step(ctxs, n, t0, dt, nsteps, true)) return rc;
	for (int k = 0; k < n; k++) {
		crd_ctx *c = ctxs[k];
		if (int rc = set_device(c)) return rc;
		HIP_TRY(c, hipEventRecord(c->ev_t1, c->compute));
	}
	for (int k = 0; k < n; k++) {
		crd_ctx *c = ctxs[k];
		if (int rc = set_device(c)) return rc;
		HIP_TRY(c, hipEventSynchronize(c->ev_t1));
		HIP_TRY(c, hipStreamSynchronize(c->comm));
		float ms = 0.f, km = 0.f;
		HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1));
		if (c->timed_steps > 0) HIP_TRY(c, hipEventElapsedTime(&km, c->ev_k[0], c->ev_k[1]));  // (set where a launch of this context was timed)
		c->timing.ms_total = ms;
		c->timing.kernel_ms = km;
		c->timing.steps = nsteps;
		c->timing.halo_slack = c->halo_slack;
		c->timing.timed_steps_per_launch = c->timed_steps;
	}
	return CRD_OK;
}

int crd_step_rk4_timed(crd_ctx *c, double t0, double dt, int64_t nsteps, double *ms_total, double *kernel_ms, int *launches_per_step)
{
	if (!c) return CRD_EINVAL;
	if (c->halo < 0 || c->halo == CRD_HALO_LOCAL) return fail(c, CRD_ESTATE, "timed stepping needs a single-slab or RCCL context");
	if (int rc = set_device(c)) return rc;
	if (int rc = ensure_timing_events(c)) return rc;
	constexpr int kMaxDiagExchanges = 64;
	if (c->diagnostics)
		while ((int)c->ev_diag.size() < 4 * kMaxDiagExchanges) {
			hipEvent_t e;
			HIP_TRY(c, hipEventCreate(&e));
			c->ev_diag.push_back(e);
		}
	crd_ctx *one[1] = {c};
	crd_recorder *rec = nullptr;
	if (int rc = recorder_of_call(one, 1, &rec)) return rc;
	decide_cycle_start(one, 1);
	int timed = 0;
	c->timed_rows = c->timed_steps = 0;
	c->diag_waits = c->diag_exchanges = 0;
	c->diag_active = c->diagnostics && c->halo == CRD_HALO_RCCL;
	c->timing = crd_step_timing{};
	HIP_TRY(c, hipEventRecord(c->ev_t0, c->compute));
	trace_push("crd_step_rk4_timed");
	const int rc_steps = run_steps(one, 1, t0, dt, nsteps, &timed, rec);
	trace_pop();
	c->diag_active = false;
	if (rc_steps) return rc_steps;
	HIP_TRY(c, hipEventRecord(c->ev_t1, c->compute));
	HIP_TRY(c, hipEventSynchronize(c->ev_t1));
	HIP_TRY(c, hipStreamSynchronize(c->comm));
	float ms = 0.f;
	HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1));
	if (ms_total) *ms_total = ms;
	double sum = 0.0;
	for (int k = 0; k < timed; k++) {
		float m = 0.f;
		HIP_TRY(c, hipEventElapsedTime(&m, c->ev_k[(size_t)(2 * k)], c->ev_k[(size_t)(2 * k + 1)]));
		sum += m;
	}
	if (kernel_ms) *kernel_ms = timed ? sum / timed : 0.0;
	if (launches_per_step) *launches_per_step = (resolve_stepper(c) == CRD_STEPPER_FUSED) ? 1 : 2;
	crd_step_timing &tm = c->timing;
	tm.ms_total = ms;
	tm.kernel_ms = timed ? sum / timed : 0.0;
	tm.steps = nsteps;
	tm.halo_slack = c->halo_slack;
	tm.timed_steps_per_launch = timed ? c->timed_steps : 0;
	tm.halo_waits = c->diag_waits;
	tm.exchanges = c->diag_exchanges;
	for (int k = 0; k < c->diag_waits; k++) {
		float m = 0.f;
		HIP_TRY(c, hipEventElapsedTime(&m, c->ev_diag[(size_t)(4 * k)], c->ev_diag[(size_t)(4 * k + 1)]));
		tm.exposed_halo_ms += m;
	}
	for (int k = 0; k < c->diag_exchanges; k++) {
		float m = 0.f;
		HIP_TRY(c, hipEventElapsedTime(&m, c->ev_diag[(size_t)(4 * k + 2)], c->ev_diag[(size_t)(4 * k + 3)]));
		tm.exchange_ms += m;
	}
	return CRD_OK;
}

int crd_dominant_kernel_rows(const crd_ctx *c, int64_t *rows)
{
	if (!c || !rows) return CRD_EINVAL;
	const int stepper = resolve_stepper(c);
	if (c->halo == CRD_HALO_SELF) *rows = c->nyl;
	else if (stepper == CRD_STEPPER_FUSED)  // the launch crd_step_rk4_timed last timed (before any: the second step of an exchange cycle)
		*rows = c->timed_rows > 0 ? c->timed_rows : c->nyl + 2 * kStepHalo * (c->exchange_every - 1 - kTimedCycleStep);
	else *rows = c->nyl - 2;
	return CRD_OK;
}

const char *crd_dominant_kernel_name(const crd_ctx *c)
{
	if (!c) return "";
	return resolve_stepper(c) == CRD_STEPPER_FUSED ? fused_kernel_name(c->p.precision, c->p.model) : stage_kernel_name(c->p.precision, c->p.model);
}

}  // extern "C"
