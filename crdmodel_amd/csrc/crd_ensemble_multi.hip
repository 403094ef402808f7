// crd_ensemble_multi.hip -- the ensemble pair: TWO classical RK4 steps of B independent members in ONE launch (crd_ensemble.cpp drives
// it; crd_ensemble_set_steps_per_launch).  The block mapping is crd_ensemble.hip's and the work item is set up by crd_ensemble_item.h;
// it runs fused_item_multi_step<..., STEPS = 2>, the two-step body of the single-slab kernel (crd_fused_impl.h): rows through LDS-DMA
// rings, the second step fed from the first one's registers, the state across memory once per two steps.  Per point the arithmetic is
// the sequence of two single steps exactly, so a pair's results are two single launches' bit for bit.  A unit of its own: the one-step
// ensemble kernels keep their code and registers.  Its device assembly is kept and checked by tools/kernel_regs.py --check (the body's
// two contracts: no vector-memory instruction skipped on the execution mask, no register touched with an LDS read in flight) before
// libcrd.so links.  DESIGN.md, "Ensembles".
#include "crd_ensemble.h"
#include "crd_fused_impl.h"
#include "crd_ensemble_item.h"

#ifndef CRD_NO_ENSEMBLE_PAIRS  // (make KERNEL_TABLE=0: nothing checks this unit's assembly, so it ships no kernel; Makefile)
namespace crd {

namespace {

// What a launch passes to the kernel: the pair's constants in the kernel's precision and EnsemblePair.
template <typename Real>
struct EnsemblePairArgs {
	StepConstants<Real> k;
	EnsemblePair e;
};

// Wavefronts per SIMD the allocator is held to: what the single-slab two-step kernel is held to (kMinWaves<..., STEPS = 2, ...>).
template <typename Real, int MODEL, bool ABSORB, int COLS>
__global__ void __launch_bounds__(kLanes *kMaxWavesPerBlock) __attribute__((amdgpu_waves_per_eu(kMinWaves<Real, MODEL, COLS, 2, ABSORB>)))
crd_ensemble_pair_kernel(const EnsembleMember *members, EnsemblePairArgs<Real> ea)
{
	const EnsembleStep &e = ea.e.step;
	// block id -> (member, chunk, strip block), member-major through xcd_remap: crd_ensemble_step_kernel's mapping
	const int blk = xcd_remap((int)blockIdx.x, e.nblocks);
	const int member = __builtin_amdgcn_readfirstlane(blk / e.member_blocks);
	const int rest = blk - member * e.member_blocks;
	const int cblk = rest / e.nsb;
	const int sblk = __builtin_amdgcn_readfirstlane(rest - cblk * e.nsb);
	const int strip = __builtin_amdgcn_readfirstlane(sblk * e.sw + (int)(threadIdx.x >> 6));
	const int chunk = __builtin_amdgcn_readfirstlane(cblk);
	if (strip >= e.nstrips) return;  // (a barrier waits for the surviving wavefronts of the workgroup only)
	ConstMember *const m = (ConstMember *)members + member;

	const Slab<Real> s = member_slab<Real, MODEL>(m, ea.k.ka4, e.nx, e.ny);
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
	item_geometry(a, e.ny, e.nstrips, e.nchunks, e.nstrips * e.nchunks, e.chunk, e.sw, e.nblocks);
	// the rings (and, the block as the strip, the edge area) of this block's wavefronts: sized as crd_rk4_fused_step_kernel sizes them
	__shared__ __attribute__((aligned(16))) char rings[kRingBytes<Real, COLS, 2>];
	lds_char *const block_rings = (lds_char *)rings;
	__shared__ __attribute__((aligned(16))) char edges[kCoop<Real, MODEL, COLS, 2> ? kEdgeBytes<2> + kEdgeDumpBytes<2> : 16];
	lds_char *const block_edges = (lds_char *)edges;
	if constexpr (ABSORB) {
		// The selects only where this member absorbs at some of the eight stages AND the chunk's pipeline -- rows [j0 - 2 kApron,
		// j1 + 2 kApron) -- can meet global row 0 or ny - 1: touches_boundary's rule (crd_ensemble_item.h) with the two steps' apron.
		// The decision is the wavefront's, and the compiler must see that (readfirstlane: the stage-time compares are vector compares
		// of uniform values): an if / else on a scalar, as in the single-slab kernel, not two regions under execution masks with a flag
		// between them -- on that form the lint cannot tell that the first body's last edge reads never meet the second body.
		constexpr int APRON = 2 * kApron;
		const int j0 = chunk * e.chunk, j1 = (j0 + e.chunk < e.ny) ? j0 + e.chunk : e.ny;
		const bool touches = __builtin_amdgcn_readfirstlane((int)(absorbs && (j0 - APRON <= 0 || j1 + APRON >= e.ny))) != 0;
		if (touches) fused_item_multi_step<Real, MODEL, true, COLS, false, 2>(s, a, strip, chunk, block_rings, sblk, block_edges);
		else fused_item_multi_step<Real, MODEL, false, COLS, false, 2>(s, a, strip, chunk, block_rings, sblk, block_edges);
	} else {
		fused_item_multi_step<Real, MODEL, false, COLS, false, 2>(s, a, strip, chunk, block_rings, sblk, block_edges);
	}
}

}  // namespace

static_assert(kGhost >= 2 * kApron, "the row parameter's table covers the pair's aprons");
// The body's own conditions (fused_item_multi_step): a row index wraps at most once -- rows [j0 - 8, j1 + 8) inside [-ny, 2 ny), which
// any chunk meets from ny = 8 on -- and an item's pipeline touches fewer than 2 ny rows: chunk + 16 < 2 ny, which a chunk of ONE row
// meets from ny = 9 on.
static_assert(kEnsemblePairMinRows == 2 * kApron + 1 && 1 + 4 * kApron < 2 * kEnsemblePairMinRows && 1 + 4 * kApron >= 2 * (kEnsemblePairMinRows - 1),
              "the smallest ny on which a legal pair chunk exists");

hipError_t ensemble_pair_plan(int precision, int model, int nx, int ny, int members, EnsemblePlan *plan)
{
	clear_launch_status();
	if (ny < kEnsemblePairMinRows) return hipErrorInvalidValue;
	const bool f64 = precision == CRD_PRECISION_F64;
	constexpr int kPairApron = 2 * kApron;
	plan->cols = (!f64 && nx % 2 == 0) ? 2 : 1;  // as ensemble_plan
	static_assert(kCoop<double, CRD_MODEL_GOLDBETER, 1, 2> && !kCoop<double, CRD_MODEL_FHN, 1, 2> && !kCoop<double, kModelDiffusionOnly, 1, 2>, "which pairs run the block as the strip");
	cut_strips(nx, ny, plan->cols, kPairApron, f64 && model == CRD_MODEL_GOLDBETER, plan);  // 48 columns per wavefront, 112 with two columns per lane
	const int per_cu = resident_blocks_per_cu(precision, model, plan->cols, plan->sw, [](auto k) {
		using K = decltype(k);
		return crd_ensemble_pair_kernel<typename K::Real, K::kModel, K::kAbsorb, K::kCols>;
	});
	plan->resident_blocks = (long)device_cus() * per_cu;
	// (The count is the SELECT-FREE instantiation's.  The absorbing Goldbeter pairs -- fp64, and fp32 with two columns per lane -- hold one
	// wavefront per SIMD fewer (2, not 3), so while some member of such a scan still absorbs a round is two thirds of this; the plan must
	// not depend on time, and which instantiation a launch takes does.)
	// Rows per work item: a pair pays 16 filling iterations per item, so the halving rule starts from CRD_ENSEMBLE_PAIR_CHUNK rows and
	// has no floor for small launches; never more than the body allows on a short member (chunk + 16 < 2 ny).
	auto blocks = [&](int chunk) { return (long)members * plan->nsb * ((ny + chunk - 1) / chunk); };
	const int chunk = std::min(ensemble_chunk_rows(CRD_ENSEMBLE_PAIR_CHUNK, blocks, plan->resident_blocks, 0), 2 * ny - 4 * kApron - 1);
	plan->chunk = std::min(chunk, ny);
	plan->nchunks = (ny + plan->chunk - 1) / plan->chunk;
	return launch_status();
}

hipError_t launch_ensemble_pair(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsemblePair &e, hipStream_t s)
{
	clear_launch_status();
	if (e.step.nblocks <= 0) return hipSuccess;
	if (e.step.ny < kEnsemblePairMinRows || e.step.chunk + 4 * kApron >= 2 * e.step.ny) return hipErrorInvalidValue;
	const hipError_t r = with_instantiation(precision, model, cols, absorb, [&](auto k) {
		using K = decltype(k);
		const EnsemblePairArgs<typename K::Real> a{StepConstants<typename K::Real>(e.step), e};
		crd_ensemble_pair_kernel<typename K::Real, K::kModel, K::kAbsorb, K::kCols><<<e.step.nblocks, kLanes * e.step.sw, 0, s>>>(table, a);
	});
	return r != hipSuccess ? r : launch_status();
}

}  // namespace crd
#else
namespace crd {
// (no pair kernels in this build: crd_ensemble_set_steps_per_launch refuses 2 before either is reached)
hipError_t ensemble_pair_plan(int, int, int, int, int, EnsemblePlan *) { return hipErrorNotSupported; }
hipError_t launch_ensemble_pair(int, int, int, bool, const EnsembleMember *, const EnsemblePair &, hipStream_t) { return hipErrorNotSupported; }
}  // namespace crd
#endif
