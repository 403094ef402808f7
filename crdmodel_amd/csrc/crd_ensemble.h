// crd_ensemble.h -- launch interface between the ensemble host code (crd_ensemble.cpp) and its kernels (crd_ensemble.hip).  Not part of
// the ABI.  An ensemble is B independent single-slab problems of one geometry and model that differ in their tables (diffusion, beta)
// and in tBoundary; one launch advances every member by one classical RK4 step.
#pragma once

#include <hip/hip_runtime.h>

namespace crd {

// One member as the step kernel sees it: an entry of a table in device memory, written once when the ensemble is created and read
// through the constant address space (scalar loads).  Every pointer is a device pointer on the ensemble's device.
struct EnsembleMember {
	void *u[2], *v[2];              // the two state buffers (ping-pong): field planes of nx * ny reals each, row 0 first, no ghost rows
	const void *cE, *cWn, *cP;      // nx: the member's diffusion tables (crd_kernels.h: SlabDesc)
	const void *brow;               // ny + 2 kGhost: the kinetics' row parameter, index j + kGhost
	double t_boundary;              // absorbing rows while t_stage < t_boundary
	double reserved;
};

// What one launch of the ensemble step shares over its members.
struct EnsembleStep {
	double h1, h2, h3, h6;  // dt, dt/2, dt/3, dt/6 in double (crd_step.h: step::Sizes); the kernel rounds them to its precision
	double t_stage[4];      // the four stages' times (step::stage_time; t = t0 + s dt, as run_steps forms it)
	double ka4;             // Goldbeter pow(KA, 4)
	int src;                // buffer holding the input; the step writes buffer 1 - src
	int nx, ny;
	int nstrips;            // strips of columns per member (a wavefront each)
	int sw;                 // wavefronts per block = adjacent strips a block takes
	int nsb;                // blocks across one chunk of rows: ceil(nstrips / sw)
	int chunk, nchunks;     // rows per work item, items per strip
	int member_blocks;      // nsb * nchunks
	int nblocks;            // member_blocks * members
};

// The plan of an ensemble's launches: fixed when the ensemble is created (no measurement).
struct EnsemblePlan {
	int cols = 1;           // grid columns per lane (fp32 on an even nx: 2)
	int nstrips = 0, sw = 0, nsb = 0, chunk = 0, nchunks = 0;
	long resident_blocks = 0;  // workgroups of the step kernel the device holds at once
};

// Fixed plan of an ensemble of `members` members of an nx x ny grid (crd_ensemble.hip; DESIGN.md, "Ensembles").  Needs the device
// (occupancy of the kernel).
hipError_t ensemble_plan(int precision, int model, int nx, int ny, int members, EnsemblePlan *plan);
// One RK4 step of every member: `absorb` selects the instantiation with the absorbing-row selects (some member has t_stage < tBoundary
// at some stage of this step).  `model` is kernel_model's: CRD_MODEL_FHN, CRD_MODEL_GOLDBETER or the diffusion-only variant.
hipError_t launch_ensemble_step(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleStep &e, hipStream_t s);
// AoS (host layout, doubles or the device precision) <-> the two field planes of one buffer, n = nx * ny points.
hipError_t launch_ensemble_aos_to_planes(int precision, int src_is_f64, const void *aos, void *u, void *v, size_t n, hipStream_t s);
hipError_t launch_ensemble_planes_to_aos(int precision, int dst_is_f64, const void *u, const void *v, void *aos, size_t n, hipStream_t s);
// max |u| of buffer `src` of every member into out_dev[0 .. members) (NaN propagates: a blown-up member reads non-finite).
hipError_t launch_ensemble_max_abs(int precision, const EnsembleMember *table, int members, int src, size_t n, double *out_dev, hipStream_t s);


// ---- two steps per launch (crd_ensemble_multi.hip; crd_ensemble.cpp: crd_ensemble_set_steps_per_launch) ----

// What one launch of the ensemble pair shares over its members: the first step's constants and geometry (the pair's own plan), and the
// second step's stage times, t + dt + c_k dt with t + dt formed as the next single step's t is (t0 + (s + 1) dt).
struct EnsemblePair {
	EnsembleStep step;
	double t_stage2[4];
};
// The smallest member height a pair runs on: the two-step body's own conditions (a row index wraps at most once: ny >= 8; an item's
// pipeline -- its chunk and 16 apron rows -- touches fewer than 2 ny rows: a one-row chunk from ny = 9 on).  CRD_ENSEMBLE_PAIR_MIN_ROWS.
constexpr int kEnsemblePairMinRows = 9;
// Fixed plan of the pair launches (the two-step apron: 48 valid columns per wavefront, 112 with two columns per lane, the block as the
// strip for Goldbeter in fp64).  Needs the device.  hipErrorInvalidValue below kEnsemblePairMinRows rows.
hipError_t ensemble_pair_plan(int precision, int model, int nx, int ny, int members, EnsemblePlan *plan);
// Two RK4 steps of every member: `absorb` selects the instantiation with the absorbing-row selects (some member has t_stage < tBoundary
// at some of the pair's eight stages).
hipError_t launch_ensemble_pair(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsemblePair &e, hipStream_t s);


// ---- members of different shape (crd_ensemble_mixed.hip, crd_ensemble_mixed_multi.hip; crd_ensemble.cpp: crd_ensemble_create_mixed) ----

// One member's shape under one plan: an entry of a second device table beside EnsembleMember's, written once when the plan is made
// and read through the constant address space (scalar loads).  The table has members + 1 entries: first_block is the prefix of the
// members' block counts (nsb * nchunks) in member-major order, the last entry's the launch's block count (its other fields are zero).
struct EnsembleShape {
	int nx, ny;
	int nstrips, nsb, nchunks;  // strips of columns, blocks across one chunk of rows, chunks of rows: the member's own
	int first_block;
};
typedef const __attribute__((address_space(4))) EnsembleShape ConstShape;  // (as the kernels read the table)
// Both plans below mark a prefix that leaves 32 bits with first_block = -1 from the first member past it on (the last entry too);
// such a plan must not be launched.  The member at which the block ids overflow, or -1 where they fit.
inline int mixed_overflow_member(const EnsembleShape *shapes, int members)
{
	if (shapes[members].first_block >= 0) return -1;
	int k = 0;
	while (k + 1 < members && shapes[k + 1].first_block >= 0) k++;
	return k;
}
// Fixed plan over a list of shapes: plan->cols, sw, chunk and resident_blocks hold for the launch (nstrips, nsb, nchunks stay zero:
// they are per member, in shapes[0 .. members]).  cols = 2 only in fp32 with every nx even; strips are cut per member as ensemble_plan
// cuts them; sw = min(4, the most strips of any member); ONE chunk height, ensemble_plan's halving rule over the members' blocks
// together, never above the smallest ny.  Needs the device.
hipError_t ensemble_plan_mixed(int precision, int model, const int *nx, const int *ny, int members, EnsemblePlan *plan, EnsembleShape *shapes);
// launch_ensemble_step over members of different shape: e.sw, e.chunk, e.nblocks (the shapes' total), e.src and the step's constants
// are the launch's; nx, ny, strips and chunks come from shapes (a device table of members + 1 entries).
hipError_t launch_ensemble_step_mixed(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleShape *shapes, int members,
                                      const EnsembleStep &e, hipStream_t s);
// launch_ensemble_max_abs, each member over its own nx * ny points; max_n: the largest member's.
hipError_t launch_ensemble_max_abs_mixed(int precision, const EnsembleMember *table, const EnsembleShape *shapes, int members, int src, size_t max_n, double *out_dev,
                                         hipStream_t s);
// The pair launches' plan over a list of shapes (ensemble_pair_plan's rule; the chunk never above 2 min ny - 17), and the launch.
// hipErrorInvalidValue where a member has fewer than kEnsemblePairMinRows rows.
hipError_t ensemble_pair_plan_mixed(int precision, int model, const int *nx, const int *ny, int members, EnsemblePlan *plan, EnsembleShape *shapes);
hipError_t launch_ensemble_pair_mixed(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleShape *shapes, int members, int min_ny,
                                      const EnsemblePair &e, hipStream_t s);


// ---- every member at its own step size (crd_ensemble_own.hip; crd_ensemble.cpp: crd_ensemble_step_rk4_own) ----

// One active member's step of a round: an entry of a table in device memory, written by the host whenever the set of active members
// or one of their absorbing decisions changes, and read through the constant address space.  What crd_ensemble_step_kernel takes from
// the launch's arguments for all members alike -- buffers, step size, absorbing stages -- is here per slot.  A launch over `count`
// slots reads count + 1 entries: first_block is the prefix of the active members' block counts (members of different shape only), the
// last entry's the launch's block count (its other fields are zero).
struct EnsembleOwnSlot {
	const void *in;         // the member's input: a state buffer (u plane, then v plane), row 0 first, no ghost rows
	void *out;              // ... and the buffer its step writes
	double h[4];            // dt_k, dt_k/2, dt_k/3, dt_k/6 in double (crd_step.h: step::Sizes of dt_k; fp64 kernels)
	float hf[4];            // ... rounded to fp32 on the host (fp32 kernels)
	int member;             // index into the member table (and the shape table)
	int absorb[4];          // t_stage < tBoundary at the member's own t + (0, 1/2, 1/2, 1) dt_k
	int first_block;
	int reserved[2];
};
// One RK4 step of each of slots[0 .. count): e gives the plan (members of one shape, shapes == nullptr: all of EnsembleStep's
// geometry, nblocks = member_blocks * count; of different shape: sw, chunk and nblocks = slots[count].first_block, strips and chunks
// from shapes[member]) and ka4; its step constants, stage times and src are not read.  absorb: some slot has a flag set.
hipError_t launch_ensemble_own_step(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleShape *shapes, const EnsembleOwnSlot *slots,
                                    int count, const EnsembleStep &e, hipStream_t s);


// ---- error-controlled integration (crd_ensemble_adaptive.hip; crd_ensemble.cpp: crd_ensemble_integrate_adaptive) ----

// One member's attempt of a round: an entry of a table in device memory, written by the host before each round's launch and read
// through the constant address space.  Members take their own step sizes, so what a context's attempt gets as kernel arguments is here.
struct EnsembleAttempt {
	const void *in;         // y_n: a state buffer (u plane, then v plane), row 0 first, no ghost rows
	void *out;              // the attempt's y_{n+1}
	double h[4];            // h, h/2, h/3, h/6 in double (crd_step.h: step::Sizes of h; fp64 kernels)
	float hf[4];            // ... rounded to fp32 on the host (fp32 kernels: a conversion in the kernel would cost registers)
	int member;             // index into the member table and into the error partials' segments
	int absorb[5];          // t_stage < tBoundary at t + (0, 1/2, 1/2, 1, 3/4) h: the four stages and Zonneveld's fifth
};

// What one attempt launch shares over its members.
struct EnsembleAttemptLaunch {
	double rtol, atol, ka4;
	double *partials;       // member k's error partials: [k * member_items, (k + 1) * member_items)
	int nx, ny;
	int nstrips, sw, nsb, chunk, nchunks;  // the attempt plan (fixed at the first adaptive call)
	int member_blocks;      // nsb * nchunks
	int member_items;       // nstrips * nchunks: the partials of one member's attempt
	int nblocks;            // member_blocks * attempts
};

// One member's operands of a batched element-wise operation (arkHin's, the dense output's): buffer base pointers as in
// EnsembleAttempt, a scalar set in double and in fp32 (rounded on the host), and the member's absorbing flag at the operation's time.
struct EnsembleOp {
	const void *x[4];
	void *out;
	double c[4];
	float cf[4];
	int member;
	int absorb;
};

// The attempt kernel's plan: one column per lane, the embedded apron (54 valid columns per wavefront), the ensemble's chunk rule.
hipError_t ensemble_attempt_plan(int precision, int model, int nx, int ny, int members, EnsemblePlan *plan);
// One Zonneveld 5(3)4 attempt of each of `count` members (attempts[0 .. count)), and the fixed-order sum of each one's partials into
// sums_dev[slot].  absorb: some entry has an absorbing flag set.
hipError_t launch_ensemble_attempts(int precision, int model, bool absorb, const EnsembleMember *table, const EnsembleAttempt *attempts, int count,
                                    const EnsembleAttemptLaunch &l, double *sums_dev, hipStream_t s);
// Batched over ops[0 .. count), n = nx * ny points per field, out_dev[slot] where a scalar comes out:
//   rhs        out = f(t, x0) with the member's tables and absorb flag (the bare RHS of rhs_on_planes: the same bits)
//   hin_bound  out_dev = max_i |x1_i| / (0.1 |x0_i| + rtol |x0_i| + atol)
//   axpy       out = x0 + c0 x1
//   ydd_sumsq  out_dev = sum_i (((x2_i - x1_i) c0) / (rtol |x0_i| + atol))^2 in launch_ydd_sumsq's order (c0 = 1 / h)
//   hermite    out = c0 x0 + c1 x2 + c2 x1 + c3 x3 (yn, yp, fn, fp: launch_hermite's coefficients)
hipError_t launch_ensemble_rhs(int precision, int model, const EnsembleMember *table, const EnsembleOp *ops, int count, int nx, int ny, double ka4, hipStream_t s);
hipError_t launch_ensemble_hin_bound(int precision, const EnsembleOp *ops, int count, size_t n, double rtol, double atol, double *out_dev, hipStream_t s);
hipError_t launch_ensemble_axpy(int precision, const EnsembleOp *ops, int count, size_t n, hipStream_t s);
hipError_t launch_ensemble_ydd_sumsq(int precision, const EnsembleOp *ops, int count, size_t n, double rtol, double atol, double *partials_dev, double *out_dev,
                                     hipStream_t s);
hipError_t launch_ensemble_hermite(int precision, const EnsembleOp *ops, int count, size_t n, hipStream_t s);
constexpr int kEnsembleNormBlocks = 256;
// launch_hermite's coefficients h00, h10, h01, h11 of the interpolant at t_n + theta h, formed as it forms them, in double and rounded to
// fp32 (in the kernels' unit, under its floating-point contraction setting).
void ensemble_hermite_coefficients(double theta, double h, double c[4], float cf[4]);  // blocks per member of the ydd norm (crd_kernels.hip: kNormBlocks); partials_dev: count x that


// ---- observers (crd_observe.hip; crd_ensemble.cpp: crd_ensemble_observe_*, crd_context.cpp: crd_state_observe) ----

constexpr int kObserveMaxProbes = 16;           // CRD_OBSERVE_MAX_PROBES
constexpr int kObserveMaxBlocks = 256;          // sampling blocks per member, at most
constexpr size_t kObservePointsPerBlock = 4096; // ... one per this many points of a plane: 16 points per lane of 256
// The probes' grid points, the same for every member: a kernel argument of the finishing launch.
struct ObserveProbes {
	int n;
	int i[kObserveMaxProbes], j[kObserveMaxProbes];
};
// Sampling blocks per member, G: a function of the plane's size alone -- never of the member count -- so a member's partition, and
// with it every bit of its row, is the same in any ensemble.
int observe_blocks(size_t n);
// Sampling: the partial records of buffer `src` of every member, n = nx * ny points per field, into partials_dev[members x G x 8]
// (min, max, sum, sum of squares of u, then of v).  maps_dev non-null: also fold u into member k's three planes at
// maps_dev + 3 k map_plane (running minimum, running maximum, time of the first sample with u >= threshold -- set to t where it is
// still NaN), each of map_plane >= n doubles.
hipError_t launch_observe_sample(int precision, const EnsembleMember *table, int members, int src, size_t n, double *partials_dev, double *maps_dev, size_t map_plane,
                                 double threshold, double t, hipStream_t s);
// Finishing: member k's G partials added in index order into row_dev[k * row_doubles .. + 8), the probes' (u, v) behind them.
hipError_t launch_observe_finish(int precision, const EnsembleMember *table, int members, int src, size_t n, const double *partials_dev, const ObserveProbes &probes, int nx,
                                 double *row_dev, int row_doubles, hipStream_t s);
hipError_t launch_observe_fill(double *x, size_t n, double value, hipStream_t s);
// ... over members of different shape: n_k = nx_k * ny_k from shapes, G_k = observe_blocks(n_k) as ever, so a member's row is the bits
// it has in any ensemble.  The sampling grid is (max_blocks = max G_k, members), blocks beyond G_k return; member k's partials sit at
// partials_dev + k * max_blocks * 8, its map planes at maps_dev + 3 k map_plane (map_plane >= the largest n_k).
hipError_t launch_observe_sample_mixed(int precision, const EnsembleMember *table, const EnsembleShape *shapes, int members, int src, int max_blocks, double *partials_dev,
                                       double *maps_dev, size_t map_plane, double threshold, double t, hipStream_t s);
hipError_t launch_observe_finish_mixed(int precision, const EnsembleMember *table, const EnsembleShape *shapes, int members, int src, int max_blocks,
                                       const double *partials_dev, const ObserveProbes &probes, double *row_dev, int row_doubles, hipStream_t s);

// Cycle maps: what the sampling pass needs besides the sample's time.  Member k's four planes of `plane` >= n doubles each at
// planes + 4 k plane: the previous sample's var0, the time of the first and of the last upward crossing of `threshold` (NaN where
// there was none), and -- as int32, in the first half of its plane -- the count of crossings.
struct ObserveCycles {
	double *planes;
	size_t plane;
	double threshold;
	double t_prev;          // the previous sample's time
	int first;              // the first sample since begin: only stores var0
};
// launch_observe_sample with the cycle maps folded in the same pass over the state.
hipError_t launch_observe_sample_cycles(int precision, const EnsembleMember *table, int members, int src, size_t n, double *partials_dev, double *maps_dev, size_t map_plane,
                                        double threshold, double t, const ObserveCycles &cy, hipStream_t s);

// Sections: lines of both fields along a row or a column, and the means over theta and over phi, the same for every member: a kernel
// argument of the sections launch.
constexpr int kObserveMaxSections = 8;          // CRD_OBSERVE_MAX_SECTIONS
struct ObserveSections {
	int n;
	int kind[kObserveMaxSections], index[kObserveMaxSections], length[kObserveMaxSections];
	int first_block[kObserveMaxSections + 1];   // blocks per member before section s; [n]: blocks per member
	double *out[kObserveMaxSections];           // this sample's lines of section s: member k's at out[s] + 2 k length[s], (var0, var1) per point
};
// A section's values per field, its blocks per member and D, the additions a value of a mean passes through (+ 3: crd.h; 0 for the
// exact kinds): functions of the kind, the precision (values per 16-byte load) and the grid alone.  false: unknown kind.
bool observe_section_shape(int precision, int kind, int nx, int ny, int *length, int *blocks, int64_t *additions);
hipError_t launch_observe_sections(int precision, const EnsembleMember *table, int members, int src, int nx, int ny, const ObserveSections &sc, hipStream_t s);

}  // namespace crd
