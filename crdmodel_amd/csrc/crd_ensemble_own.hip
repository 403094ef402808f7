// crd_ensemble_own.hip -- the ensemble step with every member at its OWN step size (crd_ensemble.cpp drives it:
// crd_ensemble_step_rk4_own).  One classical RK4 step of every member that still has steps left, in one launch: a block is a work item
// of one active SLOT, and the slot table says which member a slot is, between which buffers it steps, with which step size, and at
// which of its four stages its rows absorb -- all decided on the host against the member's own stage times.  The work item runs
// fused_item, the one-step body of the single-slab kernel (crd_fused_impl.h), as crd_ensemble_step_kernel does, so every point of a
// member goes through the arithmetic it goes through in a context stepped alone with that step size: bit-identical under any plan
// and any set of active slots.  Members of one shape: slot = block / member_blocks (crd_ensemble_attempt_kernel's mapping); members
// of different shape: a scalar search of the prefix of block counts over the ACTIVE slots (mixed_member's, crd_ensemble_mixed.h), the
// member's geometry from its entry of the shape table.  A unit of its own, compiled as crd_ensemble.hip is: the kernels of
// crd_ensemble_step_rk4 keep their code and registers.  DESIGN.md, "Ensembles" (own step sizes).
#include "crd_ensemble.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"  // (the header's error-sum kernel: this unit launches none)
#include "crd_fused_impl.h"
#pragma clang diagnostic pop
#include "crd_ensemble_mixed.h"

namespace crd {

namespace {

typedef const __attribute__((address_space(4))) EnsembleMember ConstMember;
typedef const __attribute__((address_space(4))) EnsembleOwnSlot ConstSlot;

// What a launch passes to the kernel: the geometry and chunking of EnsembleStep (members of one shape: all of it; of different shape:
// sw, chunk and nblocks, the rest being the member's), Goldbeter's constant in the kernel's precision, and the count of active slots.
template <typename Real>
struct EnsembleOwnArgs {
	Real ka4;
	EnsembleStep e;
	int slots;
};

// The slot whose blocks hold block `blk`: mixed_member's bisection over slots[0 .. count].first_block -- on scalar registers and
// scalar loads, blk being uniform over the block.  Every slot has at least one block: the prefix rises strictly.
static __device__ __forceinline__ int own_slot(ConstSlot *slots, int count, int blk)
{
	int lo = 0, hi = count;  // first_block[lo] <= blk < first_block[hi]
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (slots[mid].first_block <= blk) lo = mid;
		else hi = mid;
	}
	return __builtin_amdgcn_readfirstlane(lo);
}

// Wavefronts per SIMD the allocator is held to: the step kernels' (kMinWaves<..., STEPS = 1, ...>).
template <typename Real, int MODEL, bool ABSORB, int COLS, bool MIXED>
__global__ void __launch_bounds__(kLanes *kMaxWavesPerBlock) __attribute__((amdgpu_waves_per_eu(kMinWaves<Real, MODEL, COLS, 1, ABSORB>)))
crd_ensemble_own_kernel(const EnsembleMember *members, const EnsembleShape *shapes, const EnsembleOwnSlot *slots, EnsembleOwnArgs<Real> ea)
{
	const EnsembleStep &e = ea.e;
	// slot-major block order through xcd_remap, as crd_ensemble_step_kernel: a member's blocks share one L2
	const int blk = xcd_remap((int)blockIdx.x, e.nblocks);
	int slot, rest, nx, ny, nstrips, nsb, nchunks;
	if constexpr (MIXED) {
		slot = own_slot((ConstSlot *)slots, ea.slots, blk);
		rest = blk - ((ConstSlot *)slots)[slot].first_block;
	} else {
		slot = __builtin_amdgcn_readfirstlane(blk / e.member_blocks);
		rest = blk - slot * e.member_blocks;
	}
	ConstSlot *const sl = (ConstSlot *)slots + slot;
	const int member = sl->member;
	if constexpr (MIXED) {
		ConstShape *const sh = (ConstShape *)shapes + member;
		nx = sh->nx, ny = sh->ny, nstrips = sh->nstrips, nsb = sh->nsb, nchunks = sh->nchunks;
	} else {
		nx = e.nx, ny = e.ny, nstrips = e.nstrips, nsb = e.nsb, nchunks = e.nchunks;
	}
	const int cblk = rest / nsb;
	const int strip = __builtin_amdgcn_readfirstlane((rest - cblk * nsb) * e.sw + (int)(threadIdx.x >> 6));
	const int chunk = __builtin_amdgcn_readfirstlane(cblk);
	if (strip >= nstrips) return;  // (surplus wavefronts; a barrier waits for the surviving wavefronts of the workgroup only)
	ConstMember *const m = (ConstMember *)members + member;
	const size_t plane = (size_t)nx * (size_t)ny;

	Slab<Real> s;
	s.cE = static_cast<const Real *>(m->cE);
	s.cWn = static_cast<const Real *>(m->cWn);
	s.cP = static_cast<const Real *>(m->cP);
	s.brow = static_cast<const Real *>(m->brow) + kGhost;  // index by row
	s.ka4 = ea.ka4;
	s.nx = nx;
	s.nyl = ny;
	s.wrap = 1;  // a member is a single slab: phi wraps inside it
	s.has_row0 = s.has_rowN = 1;
	s.just_diffusion = MODEL == kModelDiffusionOnly;
	s.wrap_x = 1;
	FusedArgs<Real> a{};
	a.in_u = static_cast<const Real *>(sl->in);  // a state buffer: the u plane, then the v plane
	a.in_v = a.in_u + plane;
	a.out_u = static_cast<Real *>(sl->out);
	a.out_v = a.out_u + plane;
	if constexpr (sizeof(Real) == 8) {
		a.h1 = sl->h[0];
		a.h2 = sl->h[1];
		a.h3 = sl->h[2];
		a.h6 = sl->h[3];
	} else {
		a.h1 = sl->hf[0];
		a.h2 = sl->hf[1];
		a.h3 = sl->hf[2];
		a.h6 = sl->hf[3];
	}
	bool absorbs = false;
	if constexpr (ABSORB) {
		for (int k = 0; k < 4; k++) {
			a.absorb[k] = sl->absorb[k];
			absorbs = absorbs || a.absorb[k];
		}
	}
	a.js = 0;
	a.ny = ny;
	a.r_begin[0] = a.r_begin[1] = 0;
	a.r_end[0] = a.r_end[1] = ny;
	a.chunk = e.chunk;
	a.first2 = a.nchunks = nchunks;
	a.nstrips = nstrips;
	a.nitems = nstrips * nchunks;
	a.nblocks = e.nblocks;
	a.sw = e.sw;
	if constexpr (ABSORB) {
		// crd_ensemble_step_kernel's per-item rule on the member's own ny: the selects only where this member absorbs at some stage AND
		// the chunk's rows plus apron reach row 0 or row ny - 1.
		const int j0 = chunk * e.chunk, j1 = (j0 + e.chunk < ny) ? j0 + e.chunk : ny;
		if (absorbs && (j0 - kApron <= 0 || j1 + kApron >= ny)) {
			fused_item<Real, MODEL, true, 0, COLS, false>(s, a, strip, chunk);
			return;
		}
	}
	fused_item<Real, MODEL, false, 0, COLS, false>(s, a, strip, chunk);
}

template <typename Real, int MODEL, bool ABSORB, int COLS>
void fire(const EnsembleMember *table, const EnsembleShape *shapes, const EnsembleOwnSlot *slots, int count, const EnsembleStep &e, hipStream_t s)
{
	EnsembleOwnArgs<Real> a;
	a.ka4 = (Real)e.ka4;
	a.e = e;
	a.slots = count;
	if (shapes) crd_ensemble_own_kernel<Real, MODEL, ABSORB, COLS, true><<<e.nblocks, kLanes * e.sw, 0, s>>>(table, shapes, slots, a);
	else crd_ensemble_own_kernel<Real, MODEL, ABSORB, COLS, false><<<e.nblocks, kLanes * e.sw, 0, s>>>(table, shapes, slots, a);
}

template <typename Real, int MODEL>
hipError_t launch_model(int cols, bool absorb, const EnsembleMember *table, const EnsembleShape *shapes, const EnsembleOwnSlot *slots, int count, const EnsembleStep &e,
                        hipStream_t s)
{
	// (the diffusion-only variant skips the reaction block, absorbing rows included: no instantiation with the selects)
	constexpr bool kCanAbsorb = MODEL != kModelDiffusionOnly;
	if (cols == 2) {
		if constexpr (sizeof(Real) == 4) {
			if (kCanAbsorb && absorb) fire<Real, MODEL, kCanAbsorb, 2>(table, shapes, slots, count, e, s);
			else fire<Real, MODEL, false, 2>(table, shapes, slots, count, e, s);
			return hipSuccess;
		}
		return hipErrorInvalidValue;  // (fp64: one column per lane)
	}
	if (kCanAbsorb && absorb) fire<Real, MODEL, kCanAbsorb, 1>(table, shapes, slots, count, e, s);
	else fire<Real, MODEL, false, 1>(table, shapes, slots, count, e, s);
	return hipSuccess;
}

template <typename Real>
hipError_t launch_real(int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleShape *shapes, const EnsembleOwnSlot *slots, int count,
                       const EnsembleStep &e, hipStream_t s)
{
	switch (model) {
	case CRD_MODEL_FHN: return launch_model<Real, CRD_MODEL_FHN>(cols, absorb, table, shapes, slots, count, e, s);
	case CRD_MODEL_GOLDBETER: return launch_model<Real, CRD_MODEL_GOLDBETER>(cols, absorb, table, shapes, slots, count, e, s);
	default: return launch_model<Real, kModelDiffusionOnly>(cols, absorb, table, shapes, slots, count, e, s);
	}
}

}  // namespace

hipError_t launch_ensemble_own_step(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleShape *shapes, const EnsembleOwnSlot *slots,
                                    int count, const EnsembleStep &e, hipStream_t s)
{
	clear_launch_status();
	if (count < 1 || e.nblocks <= 0) return hipSuccess;  // (no block without a member)
	if (!slots || e.sw < 1 || e.sw > kMaxWavesPerBlock || e.chunk < 1) return hipErrorInvalidValue;
	const hipError_t r = precision == CRD_PRECISION_F64 ? launch_real<double>(model, cols, absorb, table, shapes, slots, count, e, s)
	                                                    : launch_real<float>(model, cols, absorb, table, shapes, slots, count, e, s);
	return r != hipSuccess ? r : launch_status();
}

}  // namespace crd
