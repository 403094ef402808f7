// crd_ensemble_mixed.hip -- the ensemble step over members of DIFFERENT shape (surface, nx, ny): one classical RK4 step of B members
// in one launch (crd_ensemble.cpp drives it; crd_ensemble_create_mixed).  The body of crd_ensemble_step_kernel (crd_ensemble.hip) with
// every size taken from the member's entry of a second device table (EnsembleShape): a block finds its member by a scalar search of the
// prefix of block counts, the rest of the mapping is the uniform kernel's arithmetic on the member's own nsb and nchunks.  The work
// item runs fused_item on that member's planes and tables, so the results stay bit-identical to a context stepped alone, under any
// plan.  A unit of its own: the uniform kernels (crd_ensemble.hip) keep their code and registers and stay the path of every ensemble
// whose members share nx and ny.  DESIGN.md, "Ensembles" (mixed geometry).
#include "crd_ensemble.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"  // (the header's error-sum kernel: this unit launches none)
#include "crd_fused_impl.h"
#pragma clang diagnostic pop
#include "crd_ensemble_mixed.h"

namespace crd {

namespace {

typedef const __attribute__((address_space(4))) EnsembleMember ConstMember;

// What a launch passes to the kernel: crd_ensemble.hip's EnsembleArgs and the member count (the length of the prefix).  Of e, the
// kernel reads src, the stage times, sw, chunk and nblocks: what the launch shares; the geometry is the member's.
template <typename Real>
struct EnsembleMixedArgs {
	Real h1, h2, h3, h6, ka4;
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
	const int member = mixed_member((ConstShape *)shapes, ea.members, blk);
	ConstShape *const sh = (ConstShape *)shapes + member;
	const int nx = sh->nx, ny = sh->ny, nstrips = sh->nstrips, nsb = sh->nsb, nchunks = sh->nchunks;
	const int rest = blk - sh->first_block;
	const int cblk = rest / nsb;
	const int strip = __builtin_amdgcn_readfirstlane((rest - cblk * nsb) * e.sw + (int)(threadIdx.x >> 6));
	const int chunk = __builtin_amdgcn_readfirstlane(cblk);
	if (strip >= nstrips) return;  // (surplus wavefronts of a member narrower than the block; a barrier waits for the survivors only)
	ConstMember *const m = (ConstMember *)members + member;

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

// blockIdx.y = member, over its own nx * ny points; NaN propagates (crd_ensemble_max_abs_kernel)
template <typename Real>
__global__ void __launch_bounds__(256) crd_ensemble_max_abs_mixed_kernel(const EnsembleMember *members, const EnsembleShape *shapes, int src, double *out)
{
	__shared__ double part[4];
	ConstMember *const mem = (ConstMember *)members + blockIdx.y;
	ConstShape *const sh = (ConstShape *)shapes + blockIdx.y;
	const size_t n = (size_t)sh->nx * (size_t)sh->ny;
	const Real *const u = static_cast<const Real *>(mem->u[src]);
	double m = 0.0;
	for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
		const double a = fabs((double)u[q]);
		m = (a > m || a != a) ? a : m;
	}
	for (int off = 32; off > 0; off >>= 1) {
		const double o = __shfl_down(m, off, 64);
		m = (o > m || o != o) ? o : m;
	}
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < 4; w++) m = (part[w] > m || part[w] != part[w]) ? part[w] : m;
		// non-negative doubles order like their bit patterns; NaN (0x7ff8...) sorts above every finite value
		atomicMax(reinterpret_cast<unsigned long long *>(out + blockIdx.y), (unsigned long long)__double_as_longlong(m));
	}
}

template <typename Real, int MODEL, bool ABSORB, int COLS>
void fire(const EnsembleMember *table, const EnsembleShape *shapes, int members, const EnsembleStep &e, hipStream_t s)
{
	EnsembleMixedArgs<Real> a;
	a.h1 = (Real)e.h1;
	a.h2 = (Real)e.h2;
	a.h3 = (Real)e.h3;
	a.h6 = (Real)e.h6;
	a.ka4 = (Real)e.ka4;
	a.e = e;
	a.members = members;
	crd_ensemble_step_mixed_kernel<Real, MODEL, ABSORB, COLS><<<e.nblocks, kLanes * e.sw, 0, s>>>(table, shapes, a);
}

template <typename Real, int MODEL>
hipError_t launch_model(int cols, bool absorb, const EnsembleMember *table, const EnsembleShape *shapes, int members, const EnsembleStep &e, hipStream_t s)
{
	// (the diffusion-only variant skips the reaction block, absorbing rows included: no instantiation with the selects)
	constexpr bool kCanAbsorb = MODEL != kModelDiffusionOnly;
	if (cols == 2) {
		if constexpr (sizeof(Real) == 4) {
			if (kCanAbsorb && absorb) fire<Real, MODEL, kCanAbsorb, 2>(table, shapes, members, e, s);
			else fire<Real, MODEL, false, 2>(table, shapes, members, e, s);
			return hipSuccess;
		}
		return hipErrorInvalidValue;  // (fp64: one column per lane)
	}
	if (kCanAbsorb && absorb) fire<Real, MODEL, kCanAbsorb, 1>(table, shapes, members, e, s);
	else fire<Real, MODEL, false, 1>(table, shapes, members, e, s);
	return hipSuccess;
}

template <typename Real>
hipError_t launch_real(int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleShape *shapes, int members, const EnsembleStep &e, hipStream_t s)
{
	switch (model) {
	case CRD_MODEL_FHN: return launch_model<Real, CRD_MODEL_FHN>(cols, absorb, table, shapes, members, e, s);
	case CRD_MODEL_GOLDBETER: return launch_model<Real, CRD_MODEL_GOLDBETER>(cols, absorb, table, shapes, members, e, s);
	default: return launch_model<Real, kModelDiffusionOnly>(cols, absorb, table, shapes, members, e, s);
	}
}

template <typename Real, int MODEL>
int resident_blocks_per_cu(int cols, int sw)
{
	int per_cu = 0;
	hipError_t r;
	if constexpr (sizeof(Real) == 4)
		if (cols == 2) r = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, crd_ensemble_step_mixed_kernel<Real, MODEL, false, 2>, kLanes * sw, 0);
		else r = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, crd_ensemble_step_mixed_kernel<Real, MODEL, false, 1>, kLanes * sw, 0);
	else
		r = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, crd_ensemble_step_mixed_kernel<Real, MODEL, false, 1>, kLanes * sw, 0);
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
	plan->sw = std::min(kWavesPerBlock, mixed_cut_strips(nx, ny, members, plan->cols * kLanes - 2 * kApron, shapes));
	for (int k = 0; k < members; k++) shapes[k].nsb = (shapes[k].nstrips + plan->sw - 1) / plan->sw;
	const int per_cu = f64 ? resident_blocks_per_cu<double>(model, plan->cols, plan->sw) : resident_blocks_per_cu<float>(model, plan->cols, plan->sw);
	plan->resident_blocks = (long)device_cus() * per_cu;
	// ensemble_plan's rule for the rows per work item, over the blocks of all members together; one height for the launch
	int chunk = 32;
	while (chunk > 8 && mixed_blocks(shapes, members, chunk) < 2 * plan->resident_blocks) chunk /= 2;
	if (chunk == 8 && mixed_blocks(shapes, members, 8) < device_cus() / 2) chunk = 4;
	plan->chunk = std::min(chunk, min_ny);
	mixed_fill_prefix(plan->chunk, members, shapes);
	return launch_status();
}

hipError_t launch_ensemble_step_mixed(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleShape *shapes, int members,
                                      const EnsembleStep &e, hipStream_t s)
{
	clear_launch_status();
	if (e.nblocks <= 0) return hipSuccess;
	if (members < 1 || !shapes || e.sw < 1 || e.sw > kMaxWavesPerBlock || e.chunk < 1) return hipErrorInvalidValue;
	const hipError_t r = precision == CRD_PRECISION_F64 ? launch_real<double>(model, cols, absorb, table, shapes, members, e, s)
	                                                    : launch_real<float>(model, cols, absorb, table, shapes, members, e, s);
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
