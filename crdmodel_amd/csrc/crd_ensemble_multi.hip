// crd_ensemble_multi.hip -- the ensemble pair: TWO classical RK4 steps of B independent members in ONE launch (crd_ensemble.cpp drives
// it; crd_ensemble_set_steps_per_launch).  The block mapping and the member descriptors are crd_ensemble.hip's; the work item runs
// fused_item_multi_step<..., STEPS = 2>, the two-step body of the single-slab kernel (crd_fused_impl.h): rows through LDS-DMA rings, the
// second step fed from the first one's registers, the state across memory once per two steps.  Per point the arithmetic is the sequence
// of two single steps exactly, so a pair's results are two single launches' bit for bit.  A unit of its own: the one-step ensemble
// kernels (crd_ensemble.hip) keep their code and registers.  Its device assembly is kept and checked by tools/kernel_regs.py --check
// (the body's two contracts: no vector-memory instruction skipped on the execution mask, no register touched with an LDS read in
// flight) before libcrd.so links.  DESIGN.md, "Ensembles".
#include "crd_ensemble.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"  // (the header's error-sum kernel: this unit launches none)
#include "crd_fused_impl.h"
#pragma clang diagnostic pop

#ifndef CRD_NO_ENSEMBLE_PAIRS  // (make KERNEL_TABLE=0: nothing checks this unit's assembly, so it ships no kernel; Makefile)
namespace crd {

namespace {

typedef const __attribute__((address_space(4))) EnsembleMember ConstMember;

// Rows per work item the pair's plan starts from (ensemble_pair_plan): what fused_chunk_rows uses for the single slab's two-step launches.
// UNMEASURED on ensembles -- a build with -DCRD_ENSEMBLE_PAIR_CHUNK=32 / 64 is the other arm of an A/B that has still to be run.
#ifndef CRD_ENSEMBLE_PAIR_CHUNK
#define CRD_ENSEMBLE_PAIR_CHUNK 128
#endif

// What a launch passes to the kernel: the pair's constants in the kernel's precision, rounded on the host as crd_ensemble.hip's fire
// rounds them for a single step.
template <typename Real>
struct EnsemblePairArgs {
	Real h1, h2, h3, h6, ka4;
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

	Slab<Real> s;
	s.cE = static_cast<const Real *>(m->cE);
	s.cWn = static_cast<const Real *>(m->cWn);
	s.cP = static_cast<const Real *>(m->cP);
	s.brow = static_cast<const Real *>(m->brow) + kGhost;  // index by row (kGhost >= 2 kApron entries either side: the pair's aprons)
	s.ka4 = ea.ka4;
	s.nx = e.nx;
	s.nyl = e.ny;
	s.wrap = 1;  // a member is a single slab: phi wraps inside it
	s.has_row0 = s.has_rowN = 1;
	s.just_diffusion = MODEL == kModelDiffusionOnly;
	s.wrap_x = 1;
	FusedArgs<Real> a{};
	a.in_u = static_cast<const Real *>(m->u[e.src]);
	a.in_v = static_cast<const Real *>(m->v[e.src]);
	a.out_u = static_cast<Real *>(m->u[1 - e.src]);
	a.out_v = static_cast<Real *>(m->v[1 - e.src]);
	a.h1 = ea.h1;
	a.h2 = ea.h2;
	a.h3 = ea.h3;
	a.h6 = ea.h6;
	bool absorbs = false;
	if constexpr (ABSORB) {
		const double tb = m->t_boundary;
		for (int k = 0; k < 4; k++) {
			a.absorb[k] = e.t_stage[k] < tb ? 1 : 0;  // strict <, as absorbing() (crd_ctx.h)
			a.absorb2[k] = ea.e.t_stage2[k] < tb ? 1 : 0;
			absorbs = absorbs || a.absorb[k] || a.absorb2[k];
		}
	}
	a.js = 0;
	a.ny = e.ny;
	a.r_begin[0] = a.r_begin[1] = 0;
	a.r_end[0] = a.r_end[1] = e.ny;
	a.chunk = e.chunk;
	a.first2 = a.nchunks = e.nchunks;
	a.nstrips = e.nstrips;
	a.nitems = e.nstrips * e.nchunks;
	a.nblocks = e.nblocks;
	a.sw = e.sw;
	// the rings (and, the block as the strip, the edge area) of this block's wavefronts: sized as crd_rk4_fused_step_kernel sizes them
	__shared__ __attribute__((aligned(16))) char rings[kRingBytes<Real, COLS, 2>];
	lds_char *const block_rings = (lds_char *)rings;
	__shared__ __attribute__((aligned(16))) char edges[kCoop<Real, MODEL, COLS, 2> ? kEdgeBytes<2> + kEdgeDumpBytes<2> : 16];
	lds_char *const block_edges = (lds_char *)edges;
	if constexpr (ABSORB) {
		// The selects only where this member absorbs at some of the eight stages AND the chunk's pipeline -- rows [j0 - 2 kApron,
		// j1 + 2 kApron) -- can meet global row 0 or ny - 1: the single-slab kernel's per-chunk `touches` with js = 0 and one range
		// (rows 0 and ny - 1 are neighbours; the rows contain one of them exactly when they reach 0 from above or ny from below).
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

template <typename Real, int MODEL, bool ABSORB, int COLS>
void fire(const EnsembleMember *table, const EnsemblePair &e, hipStream_t s)
{
	EnsemblePairArgs<Real> a;
	a.h1 = (Real)e.step.h1;
	a.h2 = (Real)e.step.h2;
	a.h3 = (Real)e.step.h3;
	a.h6 = (Real)e.step.h6;
	a.ka4 = (Real)e.step.ka4;
	a.e = e;
	crd_ensemble_pair_kernel<Real, MODEL, ABSORB, COLS><<<e.step.nblocks, kLanes * e.step.sw, 0, s>>>(table, a);
}

template <typename Real, int MODEL>
hipError_t launch_model(int cols, bool absorb, const EnsembleMember *table, const EnsemblePair &e, hipStream_t s)
{
	// (the diffusion-only variant skips the reaction block, absorbing rows included: no instantiation with the selects)
	constexpr bool kCanAbsorb = MODEL != kModelDiffusionOnly;
	if (cols == 2) {
		if constexpr (sizeof(Real) == 4) {
			if (kCanAbsorb && absorb) fire<Real, MODEL, kCanAbsorb, 2>(table, e, s);
			else fire<Real, MODEL, false, 2>(table, e, s);
			return hipSuccess;
		}
		return hipErrorInvalidValue;  // (fp64: one column per lane)
	}
	if (kCanAbsorb && absorb) fire<Real, MODEL, kCanAbsorb, 1>(table, e, s);
	else fire<Real, MODEL, false, 1>(table, e, s);
	return hipSuccess;
}

template <typename Real>
hipError_t launch_real(int model, int cols, bool absorb, const EnsembleMember *table, const EnsemblePair &e, hipStream_t s)
{
	switch (model) {
	case CRD_MODEL_FHN: return launch_model<Real, CRD_MODEL_FHN>(cols, absorb, table, e, s);
	case CRD_MODEL_GOLDBETER: return launch_model<Real, CRD_MODEL_GOLDBETER>(cols, absorb, table, e, s);
	default: return launch_model<Real, kModelDiffusionOnly>(cols, absorb, table, e, s);
	}
}

template <typename Real, int MODEL>
int resident_blocks_per_cu(int cols, int sw)
{
	int per_cu = 0;
	hipError_t r;
	if constexpr (sizeof(Real) == 4)
		if (cols == 2) r = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, crd_ensemble_pair_kernel<Real, MODEL, false, 2>, kLanes * sw, 0);
		else r = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, crd_ensemble_pair_kernel<Real, MODEL, false, 1>, kLanes * sw, 0);
	else
		r = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, crd_ensemble_pair_kernel<Real, MODEL, false, 1>, kLanes * sw, 0);
	return (r == hipSuccess && per_cu >= 1) ? per_cu : 1;
}

template <typename Real>
int resident_blocks_per_cu(int model, int cols, int sw)
{
	switch (model) {
	case CRD_MODEL_FHN: return resident_blocks_per_cu<Real, CRD_MODEL_FHN>(cols, sw);
	case CRD_MODEL_GOLDBETER: return resident_blocks_per_cu<Real, CRD_MODEL_GOLDBETER>(cols, sw);
	default: return resident_blocks_per_cu<Real, kModelDiffusionOnly>(cols, sw);
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
	const int valid = plan->cols * kLanes - 2 * kPairApron;  // 48 columns per wavefront, 112 with two columns per lane
	plan->nstrips = (nx + valid - 1) / valid;
	plan->sw = std::min(kWavesPerBlock, plan->nstrips);
	plan->nsb = (plan->nstrips + plan->sw - 1) / plan->sw;
	if (f64 && model == CRD_MODEL_GOLDBETER) {
		// kCoop: the block as the strip, one apron around its sw wavefronts (240 valid columns of four wavefronts' 256)
		static_assert(kCoop<double, CRD_MODEL_GOLDBETER, 1, 2> && !kCoop<double, CRD_MODEL_FHN, 1, 2> && !kCoop<double, kModelDiffusionOnly, 1, 2>, "which pairs run the block as the strip");
		const int block_valid = plan->sw * kLanes - 2 * kPairApron;
		plan->nsb = (nx + block_valid - 1) / block_valid;
		plan->nstrips = plan->sw * plan->nsb;
	}
	const int per_cu = f64 ? resident_blocks_per_cu<double>(model, plan->cols, plan->sw) : resident_blocks_per_cu<float>(model, plan->cols, plan->sw);
	plan->resident_blocks = (long)device_cus() * per_cu;
	// (The count is the SELECT-FREE instantiation's.  The absorbing Goldbeter pairs -- fp64, and fp32 with two columns per lane -- hold one
	// wavefront per SIMD fewer (2, not 3), so while some member of such a scan still absorbs a round is two thirds of this; the plan must
	// not depend on time, and which instantiation a launch takes does.)
	// Rows per work item, a fixed rule ("Ensembles"): a pair pays 16 filling iterations per item, so it starts from
	// CRD_ENSEMBLE_PAIR_CHUNK rows -- the single slab's two-step height, not yet measured on ensembles -- halved while all members together would not give
	// two rounds of resident blocks, down to 8; never more than the body allows on a short member (chunk + 16 < 2 ny).
	auto blocks = [&](int chunk) { return (long)members * plan->nsb * ((ny + chunk - 1) / chunk); };
	int chunk = CRD_ENSEMBLE_PAIR_CHUNK;
	while (chunk > 8 && blocks(chunk) < 2 * plan->resident_blocks) chunk /= 2;
	chunk = std::min(chunk, 2 * ny - 4 * kApron - 1);
	plan->chunk = std::min(chunk, ny);
	plan->nchunks = (ny + plan->chunk - 1) / plan->chunk;
	return launch_status();
}

hipError_t launch_ensemble_pair(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsemblePair &e, hipStream_t s)
{
	clear_launch_status();
	if (e.step.nblocks <= 0) return hipSuccess;
	if (e.step.ny < kEnsemblePairMinRows || e.step.chunk + 4 * kApron >= 2 * e.step.ny) return hipErrorInvalidValue;
	const hipError_t r = precision == CRD_PRECISION_F64 ? launch_real<double>(model, cols, absorb, table, e, s) : launch_real<float>(model, cols, absorb, table, e, s);
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
