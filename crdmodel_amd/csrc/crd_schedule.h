// crd_schedule.h -- which launch comes next in a fixed-step call: how many steps it takes (1, 2 or 3 by the plan, never across a
// recorder sample or a halo exchange, and only where a multi-step launch takes the single steps' absorbing-row decisions) and which
// launches a timed call puts its events around.  Plain functions of numbers: host code only, no HIP include, no context, so that
// tests/native/schedule_selftest.cpp walks whole calls on a CPU.  Both stepping loops of crd_steppers.cpp ask here.  Not part of the ABI.
#pragma once

#include <algorithm>
#include <cstdint>

#include "crd_step.h"

namespace crd {
namespace step {

// May steps s and s + 1 of a call go out as ONE two-step launch?  The kernel takes the second step's absorbing-row flags from
// t + dt (make_fused_call); the stepping loops form that step's time as t0 + (s + 1) dt, which may differ by a rounding -- which
// matters only where a stage time lands within an ulp of tBoundary.  Such a pair is stepped singly, so that paired and unpaired
// stepping take the same decisions.
static inline bool same_flags(double t_boundary, double ta, double tb, double dt)  // do steps of size dt at ta and at tb take the same absorbing decisions?
{
	int fa[4], fb[4];
	stage_flags(ta, dt, t_boundary, 4, fa);
	stage_flags(tb, dt, t_boundary, 4, fb);
	return std::equal(fa, fa + 4, fb);
}
static inline bool pair_is_exact(double t_boundary, double t0, int64_t s, double dt)
{
	const double t = t0 + (double)s * dt;
	return same_flags(t_boundary, t0 + (double)(s + 1) * dt, t + dt, dt);
}
// Does any stage of the three steps from t on have the absorbing rows on?  (The fp32 three-step kernel has no instantiation with the
// selects -- it would not fit the registers: 256 + scratch --; such triples are stepped as a pair and a single step.)
static inline bool triple_absorbs(double t_boundary, double t, double dt)
{
	int f[4];
	for (double tk : {t, t + dt, (t + dt) + dt})
		if (stage_flags(tk, dt, t_boundary, 4, f)) return true;
	return false;
}
// ... and steps s, s + 1, s + 2 as one three-step launch: the third step's flags come from (t + dt) + dt.
static inline bool triple_is_exact(double t_boundary, double t0, int64_t s, double dt)
{
	const double t = t0 + (double)s * dt;
	return pair_is_exact(t_boundary, t0, s, dt) && same_flags(t_boundary, t0 + (double)(s + 2) * dt, (t + dt) + dt, dt);
}

// A run recorder of stride rec_stride (0: none) that has seen rec_steps steps takes a sample behind every step whose count since it
// was opened is a multiple of the stride.  sample_limit: where the steps that may share a launch with step s of the call end.
static inline int64_t sample_limit(int64_t s, int64_t nsteps, int64_t rec_stride, int64_t rec_steps)
{
	return rec_stride ? std::min<int64_t>(nsteps, s + (rec_stride - (rec_steps + s) % rec_stride)) : nsteps;
}
static inline bool sample_due(int64_t s, int64_t rec_stride, int64_t rec_steps) { return rec_stride && s > 0 && (rec_steps + s) % rec_stride == 0; }  // s: steps of this call taken so far

constexpr int kNoCycle = 0;  // E of a run without exchange cycles (one slab)

// The steps the launch at step s takes: the most of max_steps (the plan's: 1, 2 or 3) that end by `end` (sample_limit(s)) and, at
// position q of an exchange cycle of E steps, by the cycle's end; a launch is the cycle's first -- which waits for the halo -- or
// its last -- which sends the next --, never both (at E = 3 a triple from q = 0 would be; found by tests/long_oracle_sweep.py).
// A triple with the absorbing rows on needs absorbing_triples (the fp64 kernel on one slab).
static inline int launch_steps(int max_steps, bool absorbing_triples, double t0, double dt, double t_boundary, int64_t s, int64_t end, int q = 0, int E = kNoCycle)
{
	const auto fits = [&](int k) { return s + k <= end && (E == kNoCycle || q + k <= E); };
	if (max_steps >= 3 && fits(3) && (E == kNoCycle || q > 0 || E > 3) && triple_is_exact(t_boundary, t0, s, dt) &&
	    (absorbing_triples || !triple_absorbs(t_boundary, t0 + (double)s * dt, dt)))
		return 3;
	return (max_steps >= 2 && fits(2) && pair_is_exact(t_boundary, t0, s, dt)) ? 2 : 1;
}

constexpr int kMaxTimedLaunches = 64;

// One slab, timed call.  Only launches of the plan's own kind are timed (a pairing plan's odd last step, or a pair stepped singly,
// goes out as a one-step launch: another kernel, which must not enter the average; runs too short to hold a pair time what there
// is).  The kind is that of the launch the call starts with.
static inline int timed_kind(int max_steps, bool absorbing_triples, double t0, double dt, double t_boundary, int64_t nsteps)
{
	const bool triples_here = max_steps == 3 && nsteps >= 3 && (absorbing_triples || !triple_absorbs(t_boundary, t0, dt));
	return triples_here ? 3 : (max_steps >= 2 && nsteps >= 2) ? 2 : 1;
}
// ... and every fourth step at most: an event pair around EVERY launch of a short run would sit inside the region being timed.
// `timed`: launches timed so far; `took`: the steps of the launch at s.
static inline bool timed_here(int kind, int took, int64_t s, int64_t nsteps, int timed)
{
	const int64_t want = std::min<int64_t>(kMaxTimedLaunches, std::max<int64_t>(1, nsteps / 4));
	return timed < want && took == kind && (s * want / std::max<int64_t>(nsteps, 1)) >= timed && ((s % 4) >= 1 || nsteps < 4);
}
// Slabs: one launch of the dominant kernel mid-run (fused: a launch of the cycle that is one full-height sweep, i.e. neither the
// split first nor the split last one, nor the one that finishes a first whose ghost readers were deferred -- whatever the two
// launches take, one step or two).  Asked until one launch has been timed.
static inline bool timed_slab_launch(bool fused, int q, int nsub, int E, bool finishes_deferred, int64_t s, int64_t nsteps)
{
	const bool middle = q >= 1 && q + nsub < E && !finishes_deferred;
	return fused ? (middle && (s >= nsteps / 2 || s + E >= nsteps)) : s >= nsteps / 2;
}

}  // namespace step
}  // namespace crd
