// crd_ensemble_mixed.h -- block id -> (member, chunk of rows, strips of columns) for ensembles whose members differ in shape: shared
// by the mixed step kernels (crd_ensemble_mixed.hip) and the mixed pair kernels (crd_ensemble_mixed_multi.hip), and what their two
// plans share on the host.  For those two units only.
#pragma once

#include <cstdint>

#include "crd_ensemble.h"

namespace crd {

typedef const __attribute__((address_space(4))) EnsembleShape ConstShape;

// The member whose blocks hold block `blk` of the member-major order: the last entry of the prefix shapes[0 .. members].first_block
// that is <= blk.  blk is uniform over the block, so the bisection runs on scalar registers and scalar loads; the result goes
// through readfirstlane so the compiler sees it so.  Every member has at least one block: the prefix rises strictly.
static __device__ __forceinline__ int mixed_member(ConstShape *shapes, int members, int blk)
{
	int lo = 0, hi = members;  // first_block[lo] <= blk < first_block[hi]
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (shapes[mid].first_block <= blk) lo = mid;
		else hi = mid;
	}
	return __builtin_amdgcn_readfirstlane(lo);
}

// ---- host side: what the two plans over a list of shapes (ensemble_plan_mixed, ensemble_pair_plan_mixed) share ----

// shapes[k].nx, ny and nstrips = ceil(nx_k / valid) of every member (`valid`: the columns a wavefront stores); returns the most strips
// of any member, which sets the launch's block size.
static inline int mixed_cut_strips(const int *nx, const int *ny, int members, int valid, EnsembleShape *shapes)
{
	int most_strips = 0;
	for (int k = 0; k < members; k++) {
		shapes[k] = EnsembleShape{};
		shapes[k].nx = nx[k];
		shapes[k].ny = ny[k];
		shapes[k].nstrips = (nx[k] + valid - 1) / valid;
		most_strips = most_strips > shapes[k].nstrips ? most_strips : shapes[k].nstrips;
	}
	return most_strips;
}

// The blocks of all members together at `chunk` rows per work item (nsb set): what the plans' halving rules weigh.
static inline long mixed_blocks(const EnsembleShape *shapes, int members, int chunk)
{
	long b = 0;
	for (int k = 0; k < members; k++) b += (long)shapes[k].nsb * ((shapes[k].ny + chunk - 1) / chunk);
	return b;
}

// nchunks of every member at the launch's chunk height and the prefix of block counts, shapes[members] included.  A prefix that leaves
// 32 bits is stored as -1 from the first member past it on (the last entry too): such a plan must not be launched, and
// mixed_overflow_member (crd_ensemble.h) names the member for the caller's refusal.
static inline void mixed_fill_prefix(int chunk, int members, EnsembleShape *shapes)
{
	long first = 0;
	shapes[members] = EnsembleShape{};
	for (int k = 0; k < members; k++) {
		shapes[k].nchunks = (shapes[k].ny + chunk - 1) / chunk;
		shapes[k].first_block = first > INT32_MAX ? -1 : (int)first;
		first += (long)shapes[k].nsb * shapes[k].nchunks;
	}
	shapes[members].first_block = first > INT32_MAX ? -1 : (int)first;
}

}  // namespace crd
