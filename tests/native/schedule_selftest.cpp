// Self-test of the launch schedule of the fixed-step calls (crd_schedule.h): how many steps each launch of a call takes -- by the plan,
// never across a recorder sample or a halo exchange, never the first and the last launch of a cycle at once, and a multi-step launch
// only where it takes the single steps' absorbing-row decisions -- and which launches a timed call times.  Plain C++, no device: the
// program walks whole calls with the rule, as the stepping loops do, and compares with sequences written out here by hand; then it
// sweeps small ranges and checks the rule's properties against a restatement of its own.
// Built and run by tests/test_schedule_host.py (also under AddressSanitizer + UndefinedBehaviorSanitizer).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "crd_schedule.h"

using namespace crd;
using step::kNoCycle;

static int g_failures = 0;
#define CHECK(cond)                                                      \
	do {                                                                 \
		if (!(cond)) {                                                   \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			g_failures++;                                                \
		}                                                                \
	} while (0)

struct Call {
	int max_steps;           // the plan's steps per launch
	bool absorbing_triples;  // fp64 on one slab
	double t0, dt, t_boundary;
	int64_t nsteps, rec_stride, rec_steps;  // rec_stride 0: no recorder
	int E, q0;                              // E = kNoCycle: one slab
};
using Seq = std::vector<int>;

// The call's launches, as run_single / run_slabs walk them.
static Seq walk(const Call &c)
{
	Seq out;
	for (int64_t s = 0; s < c.nsteps;) {
		const int q = c.E == kNoCycle ? 0 : (int)((s + c.q0) % c.E);
		const int k = step::launch_steps(c.max_steps, c.absorbing_triples, c.t0, c.dt, c.t_boundary, s, step::sample_limit(s, c.nsteps, c.rec_stride, c.rec_steps), q, c.E);
		CHECK(k >= 1 && k <= 3);
		if (k < 1) break;
		out.push_back(k);
		s += k;
	}
	return out;
}
static Call one_slab(int max_steps, int64_t nsteps) { return Call{max_steps, true, 0.0, 0.1, 0.0, nsteps, 0, 0, kNoCycle, 0}; }
static Call slabs(int max_steps, int64_t nsteps, int E, int q0) { return Call{max_steps, false, 0.0, 0.1, 0.0, nsteps, 0, 0, E, q0}; }

// a. Whole calls, written out.
static void test_sequences()
{
	CHECK(walk(one_slab(3, 8)) == (Seq{3, 3, 2}));
	CHECK(walk(one_slab(3, 7)) == (Seq{3, 3, 1}));
	CHECK(walk(one_slab(3, 4)) == (Seq{3, 1}));
	CHECK(walk(one_slab(3, 5)) == (Seq{3, 2}));
	CHECK(walk(one_slab(2, 5)) == (Seq{2, 2, 1}));
	CHECK(walk(one_slab(1, 3)) == (Seq{1, 1, 1}));
	CHECK(walk(one_slab(3, 0)).empty());
	CHECK(walk(slabs(3, 8, 8, 0)) == (Seq{3, 3, 2}));
	CHECK(walk(slabs(3, 9, 9, 0)) == (Seq{3, 3, 3}));
	CHECK(walk(slabs(3, 3, 3, 0)) == (Seq{2, 1}));  // never a triple that is the cycle's first and last launch
	CHECK(walk(slabs(3, 6, 3, 0)) == (Seq{2, 1, 2, 1}));
	CHECK(walk(slabs(3, 4, 4, 1)) == (Seq{3, 1}));   // (from q = 1 a triple may end the cycle; the next launch starts the next one)
	CHECK(walk(slabs(2, 7, 8, 6)) == (Seq{2, 2, 2, 1}));  // the pair that ends the cycle, then the next cycle from q = 0
	CHECK(walk(slabs(2, 5, 8, 7)) == (Seq{1, 2, 2}));     // no pair across the exchange
	CHECK(walk(slabs(3, 10, 10, 0)) == (Seq{3, 3, 3, 1}));
	CHECK(walk(slabs(1, 4, 8, 6)) == (Seq{1, 1, 1, 1}));
}

// b. Triples with the absorbing rows on: fp32 (and every slab run) steps them as a pair and a single step.
static void test_absorbing_triples()
{
	Call c = one_slab(3, 3);
	c.t_boundary = 0.05;  // only the first stage of the first step lies before it
	c.absorbing_triples = false;
	CHECK(walk(c) == (Seq{2, 1}));
	c.absorbing_triples = true;
	CHECK(walk(c) == (Seq{3}));
	c.t_boundary = 0.25;  // the third step's first two stages... (0.2, 0.25 is not < 0.25): its first stage
	c.absorbing_triples = false;
	CHECK(walk(c) == (Seq{2, 1}));
	// the rows switch off inside the call: triples from the first one no stage of which absorbs
	c = one_slab(3, 6);
	c.t_boundary = 0.15;
	c.absorbing_triples = false;
	CHECK(walk(c) == (Seq{2, 3, 1}));
	c.absorbing_triples = true;
	CHECK(walk(c) == (Seq{3, 3}));
	Call m = slabs(3, 6, 9, 0);  // slabs: never, whatever the precision
	m.t_boundary = 0.15;
	CHECK(walk(m) == (Seq{2, 3, 1}));
}

// c. A rounding: 6 * 0.1 = 0.6000000000000001 is the time of step 6 as the loops form it, (0.5 + 0.1) = 0.6 as a launch that starts at
// step 5 (or at step 4, a triple) forms it.  With tBoundary = 6 * 0.1 the first stage of step 6 absorbs in the second form only.
static void test_rounding()
{
	const double tb = 6 * 0.1;
	CHECK(tb == 0x1.3333333333334p-1 && 0.5 + 0.1 == 0x1.3333333333333p-1 && 5 * 0.1 == 0.5 && 4 * 0.1 + 0.1 == 0.5);
	CHECK(!step::pair_is_exact(tb, 0.0, 5, 0.1));
	CHECK(step::pair_is_exact(tb, 0.0, 4, 0.1) && !step::triple_is_exact(tb, 0.0, 4, 0.1));
	CHECK(step::pair_is_exact(0.0, 0.0, 5, 0.1) && step::triple_is_exact(0.0, 0.0, 4, 0.1));
	CHECK(step::same_flags(tb, 0.6, 0.6, 0.1) && !step::same_flags(tb, tb, 0.6, 0.1));
	Call c{2, true, 0.0, 0.1, tb, 10, 5, 0, kNoCycle, 0};  // a recorder of stride 5 makes step 5 the start of a launch
	CHECK(walk(c) == (Seq{2, 2, 1, 1, 2, 2}));
	c.t_boundary = 0.0;
	CHECK(walk(c) == (Seq{2, 2, 1, 2, 2, 1}));
	Call d{3, true, 0.0, 0.1, tb, 8, 4, 0, kNoCycle, 0};  // ... of stride 4, step 4: the triple is inexact, the pair is not
	CHECK(walk(d) == (Seq{3, 1, 2, 2}));
	d.t_boundary = 0.0;
	CHECK(walk(d) == (Seq{3, 1, 3, 1}));
}

// d. The recorder's limit and its samples.
static void test_sample_limit()
{
	CHECK(step::sample_limit(0, 10, 0, 0) == 10 && step::sample_limit(7, 10, 0, 3) == 10);
	CHECK(step::sample_limit(0, 10, 4, 0) == 4 && step::sample_limit(3, 10, 4, 0) == 4 && step::sample_limit(4, 10, 4, 0) == 8 && step::sample_limit(8, 10, 4, 0) == 10);
	CHECK(step::sample_limit(0, 10, 4, 3) == 1 && step::sample_limit(1, 10, 4, 3) == 5);  // three steps of earlier calls count
	CHECK(step::sample_limit(0, 10, 1, 0) == 1);
	CHECK(!step::sample_due(0, 4, 0) && !step::sample_due(0, 4, 4) && step::sample_due(4, 4, 0) && !step::sample_due(3, 4, 0) && step::sample_due(1, 4, 3));
	CHECK(!step::sample_due(4, 0, 0));
	Call c = one_slab(3, 10);
	c.rec_stride = 4, c.rec_steps = 3;
	CHECK(walk(c) == (Seq{1, 3, 1, 3, 1, 1}));  // samples behind steps 1, 5, 9 of the call
}

// e. Every call of a small range: the rule against its properties, restated here.
static long sweep_one(const Call &c)
{
	long launches = 0;
	int64_t s = 0;
	for (int k : walk(c)) {
		const int q = c.E == kNoCycle ? 0 : (int)((s + c.q0) % c.E);
		int64_t lim = c.nsteps;  // the first step count beyond s at which a sample is due
		for (int64_t v = s + 1; c.rec_stride && v < c.nsteps; v++)
			if ((c.rec_steps + v) % c.rec_stride == 0) {
				lim = v;
				break;
			}
		CHECK(s + k <= lim);
		if (c.E != kNoCycle) CHECK(q + k <= c.E && !(q == 0 && q + k == c.E));
		if (k >= 2) CHECK(step::pair_is_exact(c.t_boundary, c.t0, s, c.dt));
		if (k == 3) CHECK(step::triple_is_exact(c.t_boundary, c.t0, s, c.dt));
		if (k == 3 && !c.absorbing_triples) CHECK(!step::triple_absorbs(c.t_boundary, c.t0 + (double)s * c.dt, c.dt));
		// the largest size the conditions allow
		int best = 1;
		for (int j = 2; j <= c.max_steps; j++) {
			bool ok = s + j <= lim && (j == 2 ? step::pair_is_exact(c.t_boundary, c.t0, s, c.dt) : step::triple_is_exact(c.t_boundary, c.t0, s, c.dt));
			if (c.E != kNoCycle) ok = ok && q + j <= c.E && !(q == 0 && q + j == c.E);
			if (j == 3 && !c.absorbing_triples) ok = ok && !step::triple_absorbs(c.t_boundary, c.t0 + (double)s * c.dt, c.dt);
			if (ok) best = j;
		}
		CHECK(k == best);
		s += k;
		launches++;
	}
	CHECK(s == c.nsteps);
	return launches;
}
static void test_sweep()
{
	long launches = 0, inexact = 0;
	const int Es[6] = {kNoCycle, 3, 4, 8, 9, 16};
	const int strides[5] = {0, 1, 2, 3, 5};
	const double tbs[4] = {0.0, 6 * 0.1 /* inside, on a rounding */, 0.35 /* inside */, 100.0};
	for (int max_steps = 1; max_steps <= 3; max_steps++)
		for (int64_t nsteps = 0; nsteps <= 13; nsteps++)
			for (int E : Es)
				for (int q0 = 0; q0 < (E == kNoCycle ? 1 : E); q0++)
					for (int stride : strides)
						for (int rec_steps = 0; rec_steps < (stride ? stride : 1); rec_steps++)
							for (double tb : tbs)
								for (int absorbing_triples = 0; absorbing_triples <= (E == kNoCycle ? 1 : 0); absorbing_triples++)
									launches += sweep_one(Call{max_steps, absorbing_triples != 0, 0.0, 0.1, tb, nsteps, stride, rec_steps, E, q0});
	for (int64_t s = 0; s <= 13; s++) inexact += !step::pair_is_exact(6 * 0.1, 0.0, s, 0.1);
	CHECK(launches > 100000 && inexact >= 1);
}

// f. Which launches a timed call times.  One slab: launches of the kind the call STARTS with, none at a step that is a multiple of 4
// (calls of 4 steps and more), one per quarter of the call at most.  Today's answers are pinned as they are: a three-step plan over
// 4 or 5 steps times nothing (the triple sits at step 0, the rest is of another kind), and a call whose absorbing rows switch off
// early (fp32) keeps timing pairs.  That is a known weakness of `kind`; changing it is a change of behaviour, not this test's.
static Seq timed_steps_of(const Call &c)
{
	Seq at;
	int timed = 0;
	const int kind = step::timed_kind(c.max_steps, c.absorbing_triples, c.t0, c.dt, c.t_boundary, c.nsteps);
	int64_t s = 0;
	for (int k : walk(c)) {
		if (step::timed_here(kind, k, s, c.nsteps, timed)) at.push_back((int)s), timed++;
		s += k;
	}
	return at;
}
static void test_timed_choice()
{
	CHECK(timed_steps_of(one_slab(3, 4)).empty());
	CHECK(timed_steps_of(one_slab(3, 5)).empty());
	CHECK(timed_steps_of(one_slab(3, 20)) == (Seq{3, 6, 9, 15}));
	CHECK(timed_steps_of(one_slab(3, 3)) == (Seq{0}));  // (shorter than 4 steps: step 0 counts)
	CHECK(timed_steps_of(one_slab(2, 20)) == (Seq{2, 6, 10, 14, 18}));
	CHECK(timed_steps_of(one_slab(1, 20)) == (Seq{1, 5, 9, 13, 17}));
	CHECK(step::timed_kind(3, true, 0.0, 0.1, 0.0, 2) == 2 && step::timed_kind(3, true, 0.0, 0.1, 0.0, 1) == 1 && step::timed_kind(2, true, 0.0, 0.1, 0.0, 1) == 1);
	Call c = one_slab(3, 20);
	c.absorbing_triples = false;
	c.t_boundary = 0.15;  // the call starts with a pair: kind 2, and the triples that make up the rest are not timed
	CHECK(step::timed_kind(3, false, 0.0, 0.1, 0.15, 20) == 2);
	CHECK(walk(c) == (Seq{2, 3, 3, 3, 3, 3, 3}));
	CHECK(timed_steps_of(c).empty());
	CHECK(step::kMaxTimedLaunches == 64);
	// Slabs: a launch in the middle of a cycle, in the call's second half or its last cycle; staged runs: any step of the second half.
	CHECK(!step::timed_slab_launch(true, 0, 2, 8, false, 10, 20) && !step::timed_slab_launch(true, 6, 2, 8, false, 14, 20));  // first, last
	CHECK(step::timed_slab_launch(true, 2, 2, 8, false, 10, 20) && !step::timed_slab_launch(true, 2, 2, 8, true, 10, 20));   // middle; finishing a deferred first
	CHECK(!step::timed_slab_launch(true, 2, 2, 8, false, 2, 20) && step::timed_slab_launch(true, 2, 2, 8, false, 12, 20) && step::timed_slab_launch(true, 2, 1, 8, false, 2, 10));
	CHECK(step::timed_slab_launch(true, 1, 1, 3, false, 1, 2) && !step::timed_slab_launch(true, 1, 2, 3, false, 1, 3));
	CHECK(!step::timed_slab_launch(false, 0, 1, 8, false, 9, 20) && step::timed_slab_launch(false, 0, 1, 8, false, 10, 20));
}

int main()
{
	test_sequences();
	test_absorbing_triples();
	test_rounding();
	test_sample_limit();
	test_sweep();
	test_timed_choice();
	if (g_failures) {
		std::printf("%d checks failed\n", g_failures);
		return 1;
	}
	std::printf("schedule selftest ok\n");
	return 0;
}
