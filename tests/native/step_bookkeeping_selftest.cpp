// Self-test of the host-side step bookkeeping that contexts and ensembles share: crd_step.h (step sizes, stage times, absorbing
// flags) and the part of crd_arkode.h around the controller (dense-output record, plane rotation, relabelling, resume predicate).
// Plain C++, no device.  Every expectation below is written out here, not taken from the code under test.
// Built and run by tests/test_step_bookkeeping_host.py (also under AddressSanitizer + UndefinedBehaviorSanitizer).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "crd.h"
#include "crd_arkode.h"
#include "crd_step.h"

using namespace crd;
using arkode::ACC;
using arkode::OUT;
using arkode::Rotation;
using arkode::SA;
using arkode::SB;
using arkode::Y;

static int g_failures = 0;
#define CHECK(cond)                                                      \
	do {                                                                 \
		if (!(cond)) {                                                   \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			g_failures++;                                                \
		}                                                                \
	} while (0)

static bool is(const Rotation &r, int cur, int spare, int third, int prev) { return r.cur == cur && r.spare == spare && r.third == third && r.prev == prev; }

// a. The step sizes: dt, 0.5 dt, dt / 3.0, dt / 6.0 in double, and those rounded to float -- byte for byte.
static void test_sizes()
{
	const double dts[5] = {0.1, 1.0 / 3.0, 1e-3, 0.8 * 0.12527608469584325 /* crd_stable_dt of FHN on a 61-column torus, D = 0.12 */, 0x1.fffffffffffffp-3};
	int reciprocal_differs = 0;
	for (double dt : dts) {
		const double h[4] = {dt, 0.5 * dt, dt / 3.0, dt / 6.0};
		const float hf[4] = {(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
		const step::Sizes s(dt);
		CHECK(sizeof s.h == sizeof h && std::memcmp(s.h, h, sizeof h) == 0);
		CHECK(sizeof s.hf == sizeof hf && std::memcmp(s.hf, hf, sizeof hf) == 0);
		if (dt / 3.0 != dt * (1.0 / 3.0)) reciprocal_differs++;
	}
	CHECK(reciprocal_differs >= 1);  // (the last one: a multiplication by the reciprocal would not pass the memcmp above)
}

// b. The flags: strict <, the fifth stage at 3/4, the "any" return, and stage times formed as t + c * h.
static void test_flags()
{
	const double tb = 0.2;
	CHECK(!step::absorbing_at(tb, tb));
	CHECK(step::absorbing_at(std::nextafter(tb, -INFINITY), tb));
	CHECK(!step::absorbing_at(std::nextafter(tb, INFINITY), tb));

	int f[5];
	// t = 0, h = 1: stage times 0, 1/2, 1/2, 1, 3/4
	CHECK(step::stage_flags(0.0, 1.0, 0.8, 5, f) && f[0] == 1 && f[1] == 1 && f[2] == 1 && f[3] == 0 && f[4] == 1);
	CHECK(step::stage_flags(0.0, 1.0, 0.75, 5, f) && f[0] == 1 && f[1] == 1 && f[2] == 1 && f[3] == 0 && f[4] == 0);  // 3/4 == tBoundary: off
	CHECK(step::stage_flags(0.0, 1.0, std::nextafter(0.75, 1.0), 5, f) && f[4] == 1);
	CHECK(step::stage_flags(0.0, 1.0, 0.7, 5, f) && f[1] == 1 && f[4] == 0);  // (a fifth stage at 1/2 or at 1 would not give 1, 0 here and 0, 1 above)
	// n = 4 leaves the fifth flag alone
	f[4] = 7;
	CHECK(step::stage_flags(0.0, 1.0, 0.8, 4, f) && f[4] == 7);
	// "any": no flag set, and exactly one
	CHECK(!step::stage_flags(0.0, 1.0, -1.0, 5, f) && f[0] == 0 && f[1] == 0 && f[2] == 0 && f[3] == 0 && f[4] == 0);
	CHECK(!step::stage_flags(0.0, 1.0, 0.0, 4, f) && f[0] == 0);  // t == tBoundary
	CHECK(step::stage_flags(0.0, 1.0, 0.25, 4, f) && f[0] == 1 && f[1] == 0 && f[2] == 0 && f[3] == 0);
	CHECK(step::stage_flags(-1.0, 0.5, -0.6, 4, f) && f[0] == 1 && f[1] == 1 && f[2] == 1 && f[3] == 0);

	// The time is t + c * h.  c = 1: t + 1.0 * h is t + h whatever the doubles, so the last stage is the next step's first.
	const double t = 0x1.a104fe1e5e850p+2, h = 0x1.93ef3d52081b8p-1;
	CHECK(step::stage_time(t, h, 0) == t);
	CHECK(step::stage_time(t, h, 3) == t + h);
	// c = 1/2: a multiplication by a power of two is exact, so t + h[1] of the step sizes IS t + 0.5 * h for every double: no form to
	// tell apart.  c = 3/4 has one: t + 0.75 * h rounds once after the product, (t + 0.5 * h) + 0.25 * h twice.
	CHECK(step::stage_time(t, h, 1) == t + 0.5 * h && step::stage_time(t, h, 2) == t + 0.5 * h);
	const double direct = t + 0.75 * h, in_two = (t + 0.5 * h) + 0.25 * h;
	CHECK(direct == 0x1.c6e36bde0f479p+2 && in_two == 0x1.c6e36bde0f47ap+2);  // (the case was chosen for this)
	CHECK(step::stage_time(t, h, 4) == direct);
	// ... and the flag follows the time: a boundary between the two forms
	CHECK(step::stage_flags(t, h, in_two, 5, f) && f[4] == 1);
	CHECK(step::stage_flags(t, h, direct, 5, f) && f[4] == 0);
}

// The relabelling at an output from state r, on five distinct tokens: Y <- the interpolant's, SA <- cur's, OUT <- prev's.
static void check_output_relabel(const Rotation &r, int interpolant)
{
	CHECK(r.interpolant() == interpolant);
	int tok[5] = {10, 11, 12, 13, 14}, was[5];
	std::memcpy(was, tok, sizeof tok);
	arkode::Dense d;
	arkode::end_of_call(r, true, d, 2.0, 1.5, 2.5).apply(tok);
	CHECK(tok[Y] == was[interpolant] && tok[SA] == was[r.cur] && tok[OUT] == was[r.prev] && tok[SB] == was[SB] && tok[ACC] == was[ACC]);
	CHECK(d.pending && d.t_out == 2.0 && d.t_n == 1.5 && d.t_np1 == 2.5);
}

// c. The rotation, against the written-out table.
static void test_rotation_table()
{
	CHECK(Y == 0 && SA == 1 && SB == 2 && ACC == 3 && OUT == 4 && arkode::NPLANES == 5);
	Rotation r = Rotation::fresh(true);
	CHECK(is(r, Y, SA, OUT, -1));
	CHECK(r.ahead() == OUT);
	r.accept(r.spare, true);
	CHECK(is(r, SA, OUT, -1, Y));
	check_output_relabel(r, OUT);
	CHECK(r.ahead() == Y);
	r.accept(r.spare, true);
	CHECK(is(r, OUT, Y, -1, SA));
	check_output_relabel(r, Y);
	r.accept(r.spare, true);
	CHECK(is(r, Y, SA, -1, OUT));
	check_output_relabel(r, SA);

	Rotation s = Rotation::fresh(true);
	s.resume();
	CHECK(is(s, SA, OUT, Y, -1));
	CHECK(s.ahead() == Y);
	s.accept(s.spare, true);
	CHECK(is(s, OUT, Y, -1, SA));

	Rotation q = Rotation::fresh(true);
	q.reinterpolate();
	CHECK(q.prev == OUT && q.cur == SA);
	check_output_relabel(q, Y);

	Rotation n = Rotation::fresh(false);
	CHECK(is(n, Y, SA, -1, -1));
	CHECK(n.ahead() == -1);
	n.accept(n.spare, false);
	CHECK(is(n, SA, Y, -1, -1));
	n.accept(n.spare, false);
	CHECK(is(n, Y, SA, -1, -1));

	// no output: the state reached is handed back (Y <-> cur), nothing is left to resume
	Rotation b = Rotation::fresh(true);
	b.accept(b.spare, true);  // cur = SA
	int tok[5] = {10, 11, 12, 13, 14};
	arkode::Dense d;
	d.pending = true;
	arkode::end_of_call(b, false, d, 2.0, 1.5, 2.5).apply(tok);
	CHECK(tok[Y] == 11 && tok[SA] == 10 && tok[SB] == 12 && tok[ACC] == 13 && tok[OUT] == 14 && !d.pending);
	const Rotation z = Rotation::fresh(true);  // (a zero-length interval: cur is Y already)
	arkode::end_of_call(z, false, d, 2.0, 2.0, 2.0).apply(tok);
	CHECK(tok[Y] == 11 && tok[SA] == 10 && tok[OUT] == 14);
}

// d. Invariants over every sequence of up to 6 operations: 0 = accept, 1 = output + relabel + resume, 2 = output + relabel +
// re-interpolate (an output needs a step taken: sequences that ask for one before any are cut there).
static bool state_ok(const Rotation &r, const int tok[5])
{
	const auto state_plane = [](int p) { return p == Y || p == SA || p == OUT; };
	bool ok = state_plane(r.cur) && state_plane(r.spare) && r.cur != r.spare;
	if (r.prev >= 0) ok = ok && state_plane(r.prev) && r.prev != r.cur && r.prev != r.spare;
	int seen = 0;
	for (int k = 0; k < 5; k++)
		if (tok[k] >= 10 && tok[k] <= 14) seen |= 1 << (tok[k] - 10);
	return ok && seen == 31;  // the five tokens are still a permutation
}
static void test_rotation_invariants()
{
	long checked = 0;
	for (int len = 1; len <= 6; len++) {
		int total = 1;
		for (int k = 0; k < len; k++) total *= 3;
		for (int code = 0; code < total; code++) {
			Rotation r = Rotation::fresh(true);
			int tok[5] = {10, 11, 12, 13, 14};
			int c = code;
			for (int k = 0; k < len; k++, c /= 3) {
				const int op = c % 3;
				if (op == 0) {
					r.accept(r.spare, true);
				} else {
					if (r.prev < 0) break;
					int was[5];
					std::memcpy(was, tok, sizeof tok);
					const int out = Y + SA + OUT - r.prev - r.cur;
					arkode::Dense d;
					arkode::end_of_call(r, true, d, 1.0, 0.5, 1.5).apply(tok);
					CHECK(tok[Y] == was[out] && tok[SA] == was[r.cur] && tok[OUT] == was[r.prev] && tok[SB] == was[SB] && tok[ACC] == was[ACC]);
					r = Rotation::fresh(true);  // the next call
					if (op == 1) r.resume();
					else r.reinterpolate();
				}
				CHECK(state_ok(r, tok));
				checked++;
			}
		}
	}
	CHECK(checked > 1000);
}

// e. Dropping the finished step, and the resume predicate.
static void test_drop_and_resume()
{
	arkode::Dense d;
	arkode::Memory A;
	d.pending = true;
	d.t_out = 0.5;
	A.live = true;
	CHECK(arkode::resumes(d, A, 0.5, true));
	CHECK(arkode::resumes(d, A, 0.5, false));
	CHECK(!arkode::resumes(d, A, 0.5001, true));
	CHECK(!arkode::resumes(d, A, std::nextafter(0.5, 1.0), false));
	A.live = false;
	CHECK(!arkode::resumes(d, A, 0.5, true));
	CHECK(arkode::resumes(d, A, 0.5, false));  // RK4(3) keeps no controller memory
	A.live = true;
	arkode::drop(d, A);
	CHECK(!d.pending && !A.live);
	CHECK(!arkode::resumes(d, A, 0.5, true) && !arkode::resumes(d, A, 0.5, false));
}

int main()
{
	test_sizes();
	test_flags();
	test_rotation_table();
	test_rotation_invariants();
	test_drop_and_resume();
	if (g_failures) {
		std::printf("%d checks failed\n", g_failures);
		return 1;
	}
	std::printf("step bookkeeping selftest ok\n");
	return 0;
}
