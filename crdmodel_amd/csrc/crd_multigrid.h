// crd_multigrid.h -- launch interface between crd_multigrid.cpp (crd_psolve_*: levels, workspace, the V-cycle's order) and the
// kernels of crd_multigrid.hip.  One geometric multigrid V-cycle for P = I - gamma J_D(t) on var0 (include/crd.h has the definition).
// Every pointer is a device pointer on the context's device; planes are var0 only, ny rows of nx reals, theta fastest, no ghost rows:
// phi wraps inside a level as theta does.
#pragma once

#include <hip/hip_runtime.h>

namespace crd {

constexpr int kMgMaxLevels = 16;

// One level as a call sees it.  held_lo / held_hi: row 0 / row ny - 1 is held at the call's time (level 0: both or neither; coarser
// levels: row 0 only).
struct MgLevel {
	const void *cE, *cWn, *cP;  // nx reals each, the level's tables in the context's precision
	double cX2;                 // 2 cX of the level (the theta part of the diagonal), rounded to the context's precision by the launcher
	int nx, ny;
	int held_lo, held_hi;
	void *r, *z[2];             // the level's right-hand side and the two planes the sweeps alternate between
};

// What a smoothing sweep reads and writes besides z_in -> z_out.
enum {
	kMgFirst = 1,     // from z = 0: z_out = (omega / d) r, z_in is not read
	kMgRhsAos = 2,    // r is var0 of the AoS vector r_aos (level 0), not the plane L.r
	kMgStoreRhs = 4,  // ... and is stored to the plane L.r for the kernels behind this one
	kMgOutAos = 8,    // z_out is the AoS vector z_aos: var0 the sweep's result, var1 copied from r_aos (needs kMgRhsAos)
};

// One damped Jacobi sweep on a level: z_out = z_in + omega (r - (z_in - gamma L z_in)) / d, then z_out = r on held rows.
hipError_t launch_mg_sweep(int precision, const MgLevel &L, double gamma, double omega, int flags, const void *r_aos, const void *z_in, void *z_out, void *z_aos,
                           hipStream_t s);
// coarse.r = full weighting of the residual r - A z of the fine level (never stored), 0 on the coarse held row.  rhs_aos: the fine
// right-hand side is var0 of r_aos.
hipError_t launch_mg_restrict(int precision, const MgLevel &fine, const MgLevel &coarse, double gamma, int rhs_aos, const void *r_aos, const void *z, hipStream_t s);
// z += bilinear prolongation of the coarse plane e, except on the fine level's held rows; in place.  With z_aos (a cycle without
// post-sweeps, level 0) the sum goes to the AoS vector z_aos instead, var1 copied from r_aos.
hipError_t launch_mg_prolong(int precision, const MgLevel &fine, const MgLevel &coarse, const void *e, void *z, const void *r_aos, void *z_aos, hipStream_t s);

}  // namespace crd
