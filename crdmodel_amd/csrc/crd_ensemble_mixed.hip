// crd_ensemble_mixed.hip -- the ensemble step over members of DIFFERENT shape (surface, nx, ny): one classical RK4 step of B members
// in one launch (crd_ensemble.cpp drives it; crd_ensemble_create_mixed).  crd_ensemble_step_kernel (crd_ensemble.hip) with every size
// taken from the member's entry of a second device table (EnsembleShape): a block finds its member by a scalar search of the prefix
// of block counts, the rest of the mapping is the uniform kernel's arithmetic on the member's own nsb and nchunks.  The work item's
// set-up is written out here (crd_ensemble_item.h's header explains why); the search, the ladder and the plan are that header's.  A unit of its own: the uniform kernels keep their code and registers and stay the path of every
// ensemble whose members share nx and ny.  DESIGN.md, "Ensembles" (mixed geometry).
#include "crd_ensemble.h"
#include "crd_fused_impl.h"
#include "crd_ensemble_item.h"

namespace crd {

namespace {

// What a launch passes to the kernel: crd_ensemble.hip's EnsembleArgs and the member count (the length of the prefix).  Of e, the
// kernel reads src, the stage times, sw, chunk and nblocks: what the launch shares; the geometry is the member's.
template <typename Real>
struct EnsembleMixedArgs {
	StepConstants<Real> k;
	EnsembleStep e;
	int members;
};

// Wavefronts per SIMD the allocator is held to: the uniform kernel's (kMinWaves<..., STEPS = 1, ...>).
template <typename Real, int MODEL, bool ABSORB, int COLS>
__global__ void __launch_bounds__(kLanes *kMaxWavesPerBlock) __attribute__((amdgpu_waves_per_eu(kMinWaves<Real, MODEL, COLS, 1, ABSORB>)))
crd_ensemble_step_mixed_kernel(const EnsembleMember *members, const EnsembleShape *shapes, EnsembleMixedArgs<Real> ea)
{
	const EnsembleStep &e = ea.e;
	// member-major block order through xcd_remap, as crd_ensemble_step_kernel: a member's blocks share one L2
	const int blk = xcd_remap((int)blockIdx.x, e.nblocks);
	const int member = prefix_entry((ConstShape *)shapes, ea.members, blk);
	ConstShape *const sh = (ConstShape *)shapes + member;
	const int nx = sh->nx, ny = sh->ny, nstrips = sh->nstrips, nsb = sh->nsb, nchunks = sh->nchunks;
	const int rest = blk - sh->first_block;
	const int cblk = rest / nsb;
	const int strip = __builtin_amdgcn_readfirstlane((rest - cblk * nsb) * e.sw + (int)(threadIdx.x >> 6));
	const int chunk = __builtin_amdgcn_readfirstlane(cblk);
	if (strip >= nstrips) return;  // (surplus wavefronts of a member narrower than the block; a barrier waits for the survivors only)
	ConstMember *const m = (ConstMember *)members + member;

	// (written out, not through crd_ensemble_item.h's helpers: timed against the hand-written kernel this one lay outside the noise of the
	// measurement in one case, profiles/ensemble/refactor_ab.txt, and the rule is then the hand-written form)
	Slab<Real> s;
	s.cE = static_cast<const Real *>(m->cE);
	s.cWn = static_cast<const Real *>(m->cWn);
	s.cP = static_cast<const Real *>(m->cP);
	s.brow = static_cast<const Real *>(m->brow) + kGhost;  // index by row
	s.ka4 = ea.k.ka4;
	s.nx = nx;
	s.nyl = ny;
	s.wrap = 1;  // a member is a single slab: phi wraps inside it
	s.has_row0 = s.has_rowN = 1;
	s.just_diffusion = MODEL == kModelDiffusionOnly;
	s.wrap_x = 1;
	FusedArgs<Real> a{};
	a.in_u = static_cast<const Real *>(m->u[e.src]);
	a.in_v = static_cast<const Real *>(m->v[e.src]);
	a.out_u = static_cast<Real *>(m->u[1 - e.src]);
	a.out_v = static_cast<Real *>(m->v[1 - e.src]);
	a.h1 = ea.k.h1;
	a.h2 = ea.k.h2;
	a.h3 = ea.k.h3;
	a.h6 = ea.k.h6;
	bool absorbs = false;
	if constexpr (ABSORB) {
		const double tb = m->t_boundary;
		for (int k = 0; k < 4; k++) {
			a.absorb[k] = e.t_stage[k] < tb ? 1 : 0;  // strict <, as absorbing() (crd_ctx.h)
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

// blockIdx.y = member, over its own nx * ny points
template <typename Real>
__global__ void __launch_bounds__(256) crd_ensemble_max_abs_mixed_kernel(const EnsembleMember *members, const EnsembleShape *shapes, int src, double *out)
{
	ConstMember *const mem = (ConstMember *)members + blockIdx.y;
	ConstShape *const sh = (ConstShape *)shapes + blockIdx.y;
	member_max_abs(static_cast<const Real *>(mem->u[src]), (size_t)sh->nx * (size_t)sh->ny, out);
}

}  // namespace

hipError_t ensemble_plan_mixed(int precision, int model, const int *nx, const int *ny, int members, EnsemblePlan *plan, EnsembleShape *shapes)
{
	clear_launch_status();
	if (members < 1) return hipErrorInvalidValue;
	const bool f64 = precision == CRD_PRECISION_F64;
	*plan = EnsemblePlan{};
	plan->cols = f64 ? 1 : 2;  // the packed arithmetic for fp32 where no member's pairs straddle the seam
	int min_ny = ny[0];
	for (int k = 0; k < members; k++) {
		if (nx[k] % 2 != 0) plan->cols = 1;
		min_ny = std::min(min_ny, ny[k]);
	}
	// strips per member, as ensemble_plan cuts them; one block size per launch
	plan->sw = cut_strips(nx, ny, members, plan->cols, kApron, false, shapes);
	const int per_cu = resident_blocks_per_cu(precision, model, plan->cols, plan->sw, [](auto k) {
		using K = decltype(k);
		return crd_ensemble_step_mixed_kernel<typename K::Real, K::kModel, K::kAbsorb, K::kCols>;
	});
	plan->resident_blocks = (long)device_cus() * per_cu;
	// ensemble_plan's rule for the rows per work item, over the blocks of all members together; one height for the launch
	auto blocks = [&](int chunk) { return mixed_blocks(shapes, members, chunk); };
	plan->chunk = std::min(ensemble_chunk_rows(32, blocks, plan->resident_blocks, device_cus() / 2), min_ny);
	mixed_fill_prefix(plan->chunk, members, shapes);
	return launch_status();
}

hipError_t launch_ensemble_step_mixed(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleShape *shapes, int members,
                                      const EnsembleStep &e, hipStream_t s)
{
	clear_launch_status();
	if (e.nblocks <= 0) return hipSuccess;
	if (members < 1 || !shapes || e.sw < 1 || e.sw > kMaxWavesPerBlock || e.chunk < 1) return hipErrorInvalidValue;
	const hipError_t r = with_instantiation(precision, model, cols, absorb, [&](auto k) {
		using K = decltype(k);
		const EnsembleMixedArgs<typename K::Real> a{StepConstants<typename K::Real>(e), e, members};
		crd_ensemble_step_mixed_kernel<typename K::Real, K::kModel, K::kAbsorb, K::kCols><<<e.nblocks, kLanes * e.sw, 0, s>>>(table, shapes, a);
	});
	return r != hipSuccess ? r : launch_status();
}

hipError_t launch_ensemble_max_abs_mixed(int precision, const EnsembleMember *table, const EnsembleShape *shapes, int members, int src, size_t max_n, double *out_dev,
                                         hipStream_t s)
{
	clear_launch_status();
	if (members < 1) return hipSuccess;
	if (hipError_t e = hipMemsetAsync(out_dev, 0, (size_t)members * sizeof(double), s); e != hipSuccess || max_n == 0) return e;
	const size_t g = (max_n + 255) / 256;
	const dim3 grid((unsigned)(g < 64 ? g : 64), (unsigned)members);
	if (precision == CRD_PRECISION_F64) crd_ensemble_max_abs_mixed_kernel<double><<<grid, 256, 0, s>>>(table, shapes, src, out_dev);
	else crd_ensemble_max_abs_mixed_kernel<float><<<grid, 256, 0, s>>>(table, shapes, src, out_dev);
	return launch_status();
}

}  // namespace crd
