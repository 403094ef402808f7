// The counted waits of the three-step block strip's edge values (crd_fused_impl.h: kEdgeLadder, edge_landed): how many operations on a
// wavefront's LGKM counter may still be outstanding when the k-th edge read of the previous iteration's exchange has to have landed.
// Plain constexpr arithmetic, no device code: the kernels include it, and so does tests/native/edge_ladder_selftest.cpp, which checks
// it against a written-out list of an iteration's LDS operations.
//
// The operations of one iteration behind the fill, in program order (all of them `asm volatile`: the order is fixed):
//   r0 .. r(R-1)   the edge reads, R = 2 STEPS ds_read_b128 of two quantities each, issued behind the PREVIOUS iteration's barrier
//   publish u0     the row the iteration takes
//   step 0:        stage 1, publish U1, stage 2, publish U2, stage 3, publish U3, stage 4
//   read ahead     the two ds_read_b64 of the next row, behind step kEdgeReadAheadStep
//   step n > 0:    publish nu, stage 1, publish U1, stage 2, publish U2, stage 3, publish U3, stage 4
// Stages 1 and 2 of step n take their neighbour values from read 2 n, stages 3 and 4 from read 2 n + 1.  LDS operations return in
// issue order, so `s_waitcnt lgkmcnt(N)` retires all but the newest N: in front of stage 1 + 2 h of step n, read k has landed once
// at most (R - 1 - k) + (the iteration's own operations issued so far) are outstanding.  That holds only while no scalar memory load
// is in flight -- SMEM returns out of order on the same counter: the load of b(j) goes out behind the iteration's last counted wait,
// and the wait in front of the barrier retires it.
#pragma once

namespace crd {
namespace edge_waits {

constexpr int kStagePublishes = 3;    // publishes a step issues behind its stages 1, 2 and 3
constexpr int kReadAheadReads = 2;    // ds_read_b64 of u and v of the next row
constexpr int kEdgeReadAheadStep = 0; // the step the read ahead sits behind

constexpr int edge_reads(int steps) { return 2 * steps; }
// publishes a step issues in all: its input row (step 0's is the iteration's first operation) and its three stage values
constexpr int kStepPublishes = 1 + kStagePublishes;
// LDS operations the iteration has issued in front of stage 1 + 2 h of step n (h = 0, 1)
constexpr int issued_before(int n, int h)
{
	int ops = 0;
	for (int s = 0; s < n; s++) ops += kStepPublishes + (s == kEdgeReadAheadStep ? kReadAheadReads : 0);
	return ops + 1 /* the step's input row */ + 2 * h /* U1, U2 */;
}
// `s_waitcnt lgkmcnt(N)` in front of stage 1 + 2 h of step n that retires edge read k (and every read before it)
constexpr int outstanding_allowed(int steps, int k, int n, int h) { return (edge_reads(steps) - 1 - k) + issued_before(n, h); }
// (C) the full ladder: read 2 n + h in front of stage 1 + 2 h of step n -- the place that first needs it
constexpr int ladder_wait(int steps, int n, int h) { return outstanding_allowed(steps, 2 * n + h, n, h); }
// (B) one wait per step: reads 2 n and 2 n + 1 in front of its stage 1
constexpr int step_wait(int steps, int n) { return outstanding_allowed(steps, 2 * n + 1, n, 0); }
// (A) two waits: read 0 in front of step 0's stage 1 (ladder_wait(steps, 0, 0)), every other read in front of its stage 3
constexpr int rest_wait(int steps) { return outstanding_allowed(steps, edge_reads(steps) - 1, 0, 1); }
constexpr int kLgkmcntMax = 15;  // gfx9: the field is four bits

}  // namespace edge_waits
}  // namespace crd
