// crd_ensemble_own.hip -- the ensemble step with every member at its OWN step size (crd_ensemble.cpp drives it:
// crd_ensemble_step_rk4_own).  One classical RK4 step of every member that still has steps left, in one launch: a block is a work item
// of one active SLOT, and the slot table says which member a slot is, between which buffers it steps, with which step size, and at
// which of its four stages its rows absorb -- all decided on the host against the member's own stage times.  Members of one shape:
// slot = block / member_blocks (crd_ensemble_attempt_kernel's mapping); members of different shape: the scalar search of the prefix of
// block counts over the ACTIVE slots, the member's geometry from its entry of the shape table.  The work item is set up by
// crd_ensemble_item.h, so a member goes through the arithmetic of a context stepped alone with that step size: bit-identical under any
// plan and any set of active slots.  A unit of its own, compiled as crd_ensemble.hip is: the kernels of crd_ensemble_step_rk4 keep
// their code and registers.  DESIGN.md, "Ensembles" (own step sizes).
#include "crd_ensemble.h"
#include "crd_fused_impl.h"
#include "crd_ensemble_item.h"

namespace crd {

namespace {

typedef const __attribute__((address_space(4))) EnsembleOwnSlot ConstSlot;

// What a launch passes to the kernel: the geometry and chunking of EnsembleStep (members of one shape: all of it; of different shape:
// sw, chunk and nblocks, the rest being the member's), Goldbeter's constant in the kernel's precision, and the count of active slots.
template <typename Real>
struct EnsembleOwnArgs {
	Real ka4;
	EnsembleStep e;
	int slots;
};

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
		slot = prefix_entry((ConstSlot *)slots, ea.slots, blk);
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

	const Slab<Real> s = member_slab<Real, MODEL>(m, ea.ka4, nx, ny);
	FusedArgs<Real> a{};
	member_planes(a, sl->in, sl->out, (size_t)nx * (size_t)ny);
	entry_step_sizes(a, sl);
	bool absorbs = false;
	if constexpr (ABSORB) {
		for (int k = 0; k < 4; k++) {
			a.absorb[k] = sl->absorb[k];
			absorbs = absorbs || a.absorb[k];
		}
	}
	item_geometry(a, ny, nstrips, nchunks, nstrips * nchunks, e.chunk, e.sw, e.nblocks);
	step_item<Real, MODEL, ABSORB, COLS>(s, a, absorbs, strip, chunk);
}

}  // namespace

hipError_t launch_ensemble_own_step(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleShape *shapes, const EnsembleOwnSlot *slots,
                                    int count, const EnsembleStep &e, hipStream_t s)
{
	clear_launch_status();
	if (count < 1 || e.nblocks <= 0) return hipSuccess;  // (no block without a member)
	if (!slots || e.sw < 1 || e.sw > kMaxWavesPerBlock || e.chunk < 1) return hipErrorInvalidValue;
	const hipError_t r = with_instantiation(precision, model, cols, absorb, [&](auto k) {
		using K = decltype(k);
		const EnsembleOwnArgs<typename K::Real> a{(typename K::Real)e.ka4, e, count};
		if (shapes) crd_ensemble_own_kernel<typename K::Real, K::kModel, K::kAbsorb, K::kCols, true><<<e.nblocks, kLanes * e.sw, 0, s>>>(table, shapes, slots, a);
		else crd_ensemble_own_kernel<typename K::Real, K::kModel, K::kAbsorb, K::kCols, false><<<e.nblocks, kLanes * e.sw, 0, s>>>(table, shapes, slots, a);
	});
	return r != hipSuccess ? r : launch_status();
}

}  // namespace crd
