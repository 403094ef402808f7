// crd_ensemble_mixed_multi.hip -- the ensemble pair over members of DIFFERENT shape: TWO classical RK4 steps of B members in one
// launch (crd_ensemble.cpp drives it; crd_ensemble_create_mixed with crd_ensemble_set_steps_per_launch(e, 2)).
// crd_ensemble_pair_kernel (crd_ensemble_multi.hip) with every size taken from the member's entry of the shape table, the block found
// by the scalar search of crd_ensemble_item.h, which also sets the work item up.  The block size is the launch's: where the block is
// the strip (Goldbeter in fp64) a narrow member's block has wavefronts wholly beyond its nx, as the uniform kernel's last block has --
// they run on (every member's strip count is a multiple of sw there), so the stores' vmcnt contract and the barrier hold.  A unit of
// its own, its device assembly kept and checked by tools/kernel_regs.py --check before libcrd.so links, as crd_ensemble_multi.hip's.
// DESIGN.md, "Ensembles".
#include "crd_ensemble.h"
#include "crd_fused_impl.h"
#include "crd_ensemble_item.h"

#ifndef CRD_NO_ENSEMBLE_PAIRS  // (make KERNEL_TABLE=0: nothing checks this unit's assembly, so it ships no kernel; Makefile)
namespace crd {

namespace {

template <typename Real>
struct EnsembleMixedPairArgs {
	StepConstants<Real> k;
	EnsemblePair e;
	int members;
};

// Wavefronts per SIMD the allocator is held to: the uniform pair kernel's (kMinWaves<..., STEPS = 2, ...>).
template <typename Real, int MODEL, bool ABSORB, int COLS>
__global__ void __launch_bounds__(kLanes *kMaxWavesPerBlock) __attribute__((amdgpu_waves_per_eu(kMinWaves<Real, MODEL, COLS, 2, ABSORB>)))
crd_ensemble_pair_mixed_kernel(const EnsembleMember *members, const EnsembleShape *shapes, EnsembleMixedPairArgs<Real> ea)
{
	const EnsembleStep &e = ea.e.step;
	// block id -> (member, chunk, strip block): crd_ensemble_step_mixed_kernel's mapping
	const int blk = xcd_remap((int)blockIdx.x, e.nblocks);
	const int member = prefix_entry((ConstShape *)shapes, ea.members, blk);
	ConstShape *const sh = (ConstShape *)shapes + member;
	const int nx = sh->nx, ny = sh->ny, nstrips = sh->nstrips, nsb = sh->nsb, nchunks = sh->nchunks;
	const int rest = blk - sh->first_block;
	const int cblk = rest / nsb;
	const int sblk = __builtin_amdgcn_readfirstlane(rest - cblk * nsb);
	const int strip = __builtin_amdgcn_readfirstlane(sblk * e.sw + (int)(threadIdx.x >> 6));
	const int chunk = __builtin_amdgcn_readfirstlane(cblk);
	if (strip >= nstrips) return;  // (never where the block is the strip; a barrier waits for the surviving wavefronts only)
	ConstMember *const m = (ConstMember *)members + member;

	// member_slab's fill (crd_ensemble_item.h), written out: behind the helper one instantiation of this kernel -- fp32 Goldbeter,
	// absorbing, two columns -- keeps one scalar value fewer in vector lanes, and the resource rows are held equal
	Slab<Real> s;
	s.cE = static_cast<const Real *>(m->cE);
	s.cWn = static_cast<const Real *>(m->cWn);
	s.cP = static_cast<const Real *>(m->cP);
	s.brow = static_cast<const Real *>(m->brow) + kGhost;  // index by row (kGhost >= 2 kApron entries either side: the pair's aprons)
	s.ka4 = ea.k.ka4;
	s.nx = nx;
	s.nyl = ny;
	s.wrap = 1;  // a member is a single slab: phi wraps inside it
	s.has_row0 = s.has_rowN = 1;
	s.just_diffusion = MODEL == kModelDiffusionOnly;
	s.wrap_x = 1;
	FusedArgs<Real> a{};
	member_planes(a, m, e.src);
	step_sizes(a, ea.k);
	bool absorbs = false;
	if constexpr (ABSORB) {
		const double tb = m->t_boundary;
		for (int k = 0; k < 4; k++) {
			a.absorb[k] = e.t_stage[k] < tb ? 1 : 0;  // strict <, as absorbing() (crd_ctx.h)
			a.absorb2[k] = ea.e.t_stage2[k] < tb ? 1 : 0;
			absorbs = absorbs || a.absorb[k] || a.absorb2[k];
		}
	}
	item_geometry(a, ny, nstrips, nchunks, nstrips * nchunks, e.chunk, e.sw, e.nblocks);
	// the rings (and, the block as the strip, the edge area) of this block's wavefronts: sized as crd_ensemble_pair_kernel sizes them
	__shared__ __attribute__((aligned(16))) char rings[kRingBytes<Real, COLS, 2>];
	lds_char *const block_rings = (lds_char *)rings;
	__shared__ __attribute__((aligned(16))) char edges[kCoop<Real, MODEL, COLS, 2> ? kEdgeBytes<2> + kEdgeDumpBytes<2> : 16];
	lds_char *const block_edges = (lds_char *)edges;
	if constexpr (ABSORB) {
		// crd_ensemble_pair_kernel's per-item rule on the member's own ny, and its form: an if / else on a scalar between the two bodies.
		// The flag goes through a scalar register the compiler cannot look into: behind this kernel's mapping it otherwise lays the two
		// bodies out one behind the other with a flag between them (two regions, the form crd_ensemble_pair_kernel's comment warns of),
		// on which the lint cannot tell that the first body's last edge reads never meet the second body.  With it the branch is the
		// uniform kernel's plain one.
		constexpr int APRON = 2 * kApron;
		const int j0 = chunk * e.chunk, j1 = (j0 + e.chunk < ny) ? j0 + e.chunk : ny;
		int touches;
		asm volatile("s_mov_b32 %0, %1" : "=s"(touches) : "s"(__builtin_amdgcn_readfirstlane((int)(absorbs && (j0 - APRON <= 0 || j1 + APRON >= ny)))));
		if (touches) fused_item_multi_step<Real, MODEL, true, COLS, false, 2>(s, a, strip, chunk, block_rings, sblk, block_edges);
		else fused_item_multi_step<Real, MODEL, false, COLS, false, 2>(s, a, strip, chunk, block_rings, sblk, block_edges);
	} else {
		fused_item_multi_step<Real, MODEL, false, COLS, false, 2>(s, a, strip, chunk, block_rings, sblk, block_edges);
	}
}

}  // namespace

hipError_t ensemble_pair_plan_mixed(int precision, int model, const int *nx, const int *ny, int members, EnsemblePlan *plan, EnsembleShape *shapes)
{
	clear_launch_status();
	if (members < 1) return hipErrorInvalidValue;
	const bool f64 = precision == CRD_PRECISION_F64;
	constexpr int kPairApron = 2 * kApron;
	*plan = EnsemblePlan{};
	plan->cols = f64 ? 1 : 2;  // as ensemble_plan_mixed
	int min_ny = ny[0];
	for (int k = 0; k < members; k++) {
		if (ny[k] < kEnsemblePairMinRows) return hipErrorInvalidValue;
		if (nx[k] % 2 != 0) plan->cols = 1;
		min_ny = std::min(min_ny, ny[k]);
	}
	// 48 columns per wavefront, 112 with two columns per lane; one block size per launch; Goldbeter in fp64: the block as the strip
	plan->sw = cut_strips(nx, ny, members, plan->cols, kPairApron, f64 && model == CRD_MODEL_GOLDBETER, shapes);
	const int per_cu = resident_blocks_per_cu(precision, model, plan->cols, plan->sw, [](auto k) {
		using K = decltype(k);
		return crd_ensemble_pair_mixed_kernel<typename K::Real, K::kModel, K::kAbsorb, K::kCols>;
	});
	plan->resident_blocks = (long)device_cus() * per_cu;
	// ensemble_pair_plan's rule over the blocks of all members together; never more than the body allows on the shortest member
	// (chunk + 16 < 2 ny)
	auto blocks = [&](int chunk) { return mixed_blocks(shapes, members, chunk); };
	const int chunk = std::min(ensemble_chunk_rows(CRD_ENSEMBLE_PAIR_CHUNK, blocks, plan->resident_blocks, 0), 2 * min_ny - 4 * kApron - 1);
	plan->chunk = std::min(chunk, min_ny);
	mixed_fill_prefix(plan->chunk, members, shapes);
	return launch_status();
}

hipError_t launch_ensemble_pair_mixed(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleShape *shapes, int members, int min_ny,
                                      const EnsemblePair &e, hipStream_t s)
{
	clear_launch_status();
	if (e.step.nblocks <= 0) return hipSuccess;
	if (members < 1 || !shapes || e.step.sw < 1 || e.step.sw > kMaxWavesPerBlock || e.step.chunk < 1) return hipErrorInvalidValue;
	if (min_ny < kEnsemblePairMinRows || e.step.chunk + 4 * kApron >= 2 * min_ny) return hipErrorInvalidValue;
	const hipError_t r = with_instantiation(precision, model, cols, absorb, [&](auto k) {
		using K = decltype(k);
		const EnsembleMixedPairArgs<typename K::Real> a{StepConstants<typename K::Real>(e.step), e, members};
		crd_ensemble_pair_mixed_kernel<typename K::Real, K::kModel, K::kAbsorb, K::kCols><<<e.step.nblocks, kLanes * e.step.sw, 0, s>>>(table, shapes, a);
	});
	return r != hipSuccess ? r : launch_status();
}

}  // namespace crd
#else
namespace crd {
// (no pair kernels in this build: crd_ensemble_set_steps_per_launch refuses 2 before either is reached)
hipError_t ensemble_pair_plan_mixed(int, int, const int *, const int *, int, EnsemblePlan *, EnsembleShape *) { return hipErrorNotSupported; }
hipError_t launch_ensemble_pair_mixed(int, int, int, bool, const EnsembleMember *, const EnsembleShape *, int, int, const EnsemblePair &, hipStream_t) { return hipErrorNotSupported; }
}  // namespace crd
#endif
