// Self-test of the counted waits of the three-step block strip's edge values (crd_edge_waits.h): the constants the kernels wait with,
// against a literal enumeration of one iteration's operations on the LGKM counter.  Plain C++, no device.  The list below is written out
// here, operation by operation, not taken from the header under test.
// Built and run by tests/test_edge_ladder_host.py.
#include <cstdio>
#include <cstring>

#include "crd_edge_waits.h"

using namespace crd::edge_waits;

static int g_failures = 0;
#define CHECK(cond)                                                      \
	do {                                                                 \
		if (!(cond)) {                                                   \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			g_failures++;                                                \
		}                                                                \
	} while (0)

// One iteration behind the fill, in program order.  "rK": edge read K (issued behind the previous iteration's barrier); "pub": a publish
// (ds_write_b64); "ahead": one ds_read_b64 of the read ahead; "N.S": stage S of step N starts here -- not an operation, a place.
static const char *const kThreeSteps[] = {
    "r0", "r1", "r2", "r3", "r4", "r5",                       // the exchange
    "pub",                                                      // u0: the row the iteration takes
    "0.1", "pub", "0.2", "pub", "0.3", "pub", "0.4",          // step 0
    "ahead", "ahead",                                           // the next row, behind step 0
    "pub", "1.1", "pub", "1.2", "pub", "1.3", "pub", "1.4",   // step 1: its input row, then its stages
    "pub", "2.1", "pub", "2.2", "pub", "2.3", "pub", "2.4",   // step 2
};
static const char *const kTwoSteps[] = {
    "r0", "r1", "r2", "r3",
    "pub",
    "0.1", "pub", "0.2", "pub", "0.3", "pub", "0.4",
    "ahead", "ahead",
    "pub", "1.1", "pub", "1.2", "pub", "1.3", "pub", "1.4",
};

// Operations issued behind read `k` and in front of the place `where`: what may be outstanding when read k has to have landed there.
static int behind(const char *const *ops, int n, int k, const char *where)
{
	char read[8];
	std::snprintf(read, sizeof read, "r%d", k);
	int count = -1;
	for (int i = 0; i < n; i++) {
		if (std::strcmp(ops[i], where) == 0) return count;
		const bool place = std::strchr(ops[i], '.') != nullptr;
		if (count >= 0 && !place) count++;
		if (std::strcmp(ops[i], read) == 0) count = 0;
	}
	return -1000;
}

static void check_steps(const char *const *ops, int n, int steps)
{
	CHECK(edge_reads(steps) == 2 * steps);
	for (int s = 0; s < steps; s++) {
		char first[8], third[8];
		std::snprintf(first, sizeof first, "%d.1", s);
		std::snprintf(third, sizeof third, "%d.3", s);
		// the full ladder: read 2 s in front of the step's stage 1, read 2 s + 1 in front of its stage 3
		CHECK(ladder_wait(steps, s, 0) == behind(ops, n, 2 * s, first));
		CHECK(ladder_wait(steps, s, 1) == behind(ops, n, 2 * s + 1, third));
		// one wait per step: both reads in front of its stage 1
		CHECK(step_wait(steps, s) == behind(ops, n, 2 * s + 1, first));
		CHECK(ladder_wait(steps, s, 0) <= kLgkmcntMax && ladder_wait(steps, s, 1) <= kLgkmcntMax && step_wait(steps, s) <= kLgkmcntMax);
	}
	// two waits: the last read in front of step 0's stage 3
	CHECK(rest_wait(steps) == behind(ops, n, 2 * steps - 1, "0.3"));
}

int main()
{
	check_steps(kThreeSteps, (int)(sizeof kThreeSteps / sizeof *kThreeSteps), 3);
	check_steps(kTwoSteps, (int)(sizeof kTwoSteps / sizeof *kTwoSteps), 2);
	// ... and the numbers themselves, three steps: counted by hand from the list above
	CHECK(ladder_wait(3, 0, 0) == 6 && ladder_wait(3, 0, 1) == 7 && ladder_wait(3, 1, 0) == 10 && ladder_wait(3, 1, 1) == 11 && ladder_wait(3, 2, 0) == 12 &&
	      ladder_wait(3, 2, 1) == 13);
	CHECK(step_wait(3, 0) == 5 && step_wait(3, 1) == 9 && step_wait(3, 2) == 11);
	CHECK(rest_wait(3) == 3);
	CHECK(kLgkmcntMax == 15);
	static_assert(ladder_wait(3, 2, 1) <= kLgkmcntMax, "constexpr: usable in the kernels' static_asserts");
	if (g_failures) {
		std::printf("%d check(s) failed\n", g_failures);
		return 1;
	}
	std::printf("edge ladder selftest ok\n");
	return 0;
}
