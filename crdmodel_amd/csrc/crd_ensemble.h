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
	double h1, h2, h3, h6;  // dt, dt/2, dt/3, dt/6, formed in double as launch_fused_t forms them; the kernel rounds them to its precision
	double t_stage[4];      // t + c_k dt of the four stages (t = t0 + s dt, as run_steps forms it)
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

}  // namespace crd
