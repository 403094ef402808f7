// crd_ensemble.hip -- the ensemble step: one classical RK4 step of B independent members in ONE launch (crd_ensemble.cpp drives it).
// A block is a work item of one member: block id -> (member, chunk of rows, strips of columns).  The work item runs fused_item, the
// one-step body of the single-slab kernel (crd_fused_impl.h), on that member's planes and tables, so every point of a member goes
// through the arithmetic it goes through in a context stepped alone: the results are bit-identical to crd_step_rk4 with the one-launch
// stepper, under any plan.  The members' descriptors are read through the constant address space (scalar loads); what the members
// share -- step size, stage times, geometry, chunking -- comes in the kernel arguments.  DESIGN.md, "Ensembles".
#include "crd_ensemble.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"  // (the header's error-sum kernel: this unit launches none)
#include "crd_fused_impl.h"
#pragma clang diagnostic pop

namespace crd {

namespace {

typedef const __attribute__((address_space(4))) EnsembleMember ConstMember;

// What a launch passes to the kernel: EnsembleStep with the step's constants in the kernel's precision, rounded on the host as
// launch_fused_t rounds them (a conversion in the kernel would be a vector instruction, its result held in vector registers).
template <typename Real>
struct EnsembleArgs {
	Real h1, h2, h3, h6, ka4;
	EnsembleStep e;
};

// Wavefronts per SIMD the allocator is held to: what the single-slab one-step kernel is held to (kMinWaves<..., STEPS = 1, ...>).
template <typename Real, int MODEL, bool ABSORB, int COLS>
__global__ void __launch_bounds__(kLanes *kMaxWavesPerBlock) __attribute__((amdgpu_waves_per_eu(kMinWaves<Real, MODEL, COLS, 1, ABSORB>)))
crd_ensemble_step_kernel(const EnsembleMember *members, EnsembleArgs<Real> ea)
{
	const EnsembleStep &e = ea.e;
	// Workgroups are dealt round-robin over the XCDs; xcd_remap hands each XCD a contiguous run of the member-major block order, so a
	// member's blocks share one L2 (two where a member straddles runs; with fewer than eight members a member spans 8 / B XCDs).
	const int blk = xcd_remap((int)blockIdx.x, e.nblocks);
	const int member = __builtin_amdgcn_readfirstlane(blk / e.member_blocks);
	const int rest = blk - member * e.member_blocks;
	const int cblk = rest / e.nsb;
	const int strip = __builtin_amdgcn_readfirstlane((rest - cblk * e.nsb) * e.sw + (int)(threadIdx.x >> 6));
	const int chunk = __builtin_amdgcn_readfirstlane(cblk);
	if (strip >= e.nstrips) return;  // (a barrier waits for the surviving wavefronts of the workgroup only)
	ConstMember *const m = (ConstMember *)members + member;

	Slab<Real> s;
	s.cE = static_cast<const Real *>(m->cE);
	s.cWn = static_cast<const Real *>(m->cWn);
	s.cP = static_cast<const Real *>(m->cP);
	s.brow = static_cast<const Real *>(m->brow) + kGhost;  // index by row
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
			absorbs = absorbs || a.absorb[k];
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
	if constexpr (ABSORB) {
		// The selects only where this member absorbs at some stage AND the chunk's pipeline -- rows [j0 - kApron, j1 + kApron) -- can
		// meet global row 0 or ny - 1 (the single-slab kernel's per-chunk rule, crd_rk4_fused_step_kernel; with js = 0 and ny >= 8 the
		// rows reach row 0 exactly when j0 - kApron <= 0 and row ny - 1 exactly when j1 + kApron >= ny).
		const int j0 = chunk * e.chunk, j1 = (j0 + e.chunk < e.ny) ? j0 + e.chunk : e.ny;
		if (absorbs && (j0 - kApron <= 0 || j1 + kApron >= e.ny)) {
			fused_item<Real, MODEL, true, 0, COLS, false>(s, a, strip, chunk);
			return;
		}
	}
	fused_item<Real, MODEL, false, 0, COLS, false>(s, a, strip, chunk);
}

template <typename Src, typename Real>
__global__ void __launch_bounds__(256) crd_ensemble_aos_to_planes_kernel(const Src *__restrict__ aos, Real *__restrict__ u, Real *__restrict__ v, size_t n)
{
	for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
		u[q] = (Real)aos[2 * q];
		v[q] = (Real)aos[2 * q + 1];
	}
}

template <typename Dst, typename Real>
__global__ void __launch_bounds__(256) crd_ensemble_planes_to_aos_kernel(const Real *__restrict__ u, const Real *__restrict__ v, Dst *__restrict__ aos, size_t n)
{
	for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
		aos[2 * q] = (Dst)u[q];
		aos[2 * q + 1] = (Dst)v[q];
	}
}

// blockIdx.y = member; NaN propagates (the blow-up guard of crd_max_abs_kernel, crd_kernels.hip)
template <typename Real>
__global__ void __launch_bounds__(256) crd_ensemble_max_abs_kernel(const EnsembleMember *members, int src, size_t n, double *out)
{
	__shared__ double part[4];
	ConstMember *const mem = (ConstMember *)members + blockIdx.y;
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

inline int grid_for(size_t n, size_t cap = 2048) { return (int)((n + 255) / 256 < cap ? (n + 255) / 256 : cap); }

template <typename Real, int MODEL, bool ABSORB, int COLS>
void fire(const EnsembleMember *table, const EnsembleStep &e, hipStream_t s)
{
	EnsembleArgs<Real> a;
	a.h1 = (Real)e.h1;
	a.h2 = (Real)e.h2;
	a.h3 = (Real)e.h3;
	a.h6 = (Real)e.h6;
	a.ka4 = (Real)e.ka4;
	a.e = e;
	crd_ensemble_step_kernel<Real, MODEL, ABSORB, COLS><<<e.nblocks, kLanes * e.sw, 0, s>>>(table, a);
}

template <typename Real, int MODEL>
hipError_t launch_model(int cols, bool absorb, const EnsembleMember *table, const EnsembleStep &e, hipStream_t s)
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
hipError_t launch_real(int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleStep &e, hipStream_t s)
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
		if (cols == 2) r = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, crd_ensemble_step_kernel<Real, MODEL, false, 2>, kLanes * sw, 0);
		else r = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, crd_ensemble_step_kernel<Real, MODEL, false, 1>, kLanes * sw, 0);
	else
		r = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, crd_ensemble_step_kernel<Real, MODEL, false, 1>, kLanes * sw, 0);
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

hipError_t ensemble_plan(int precision, int model, int nx, int ny, int members, EnsemblePlan *plan)
{
	clear_launch_status();
	const bool f64 = precision == CRD_PRECISION_F64;
	plan->cols = (!f64 && nx % 2 == 0) ? 2 : 1;  // fused_default_columns: the packed arithmetic for fp32 where the pairs do not straddle the seam
	const int valid = plan->cols * kLanes - 2 * kApron;
	plan->nstrips = (nx + valid - 1) / valid;
	plan->sw = std::min(kWavesPerBlock, plan->nstrips);  // (a block of narrow members: no wavefronts that only return)
	plan->nsb = (plan->nstrips + plan->sw - 1) / plan->sw;
	const int per_cu = f64 ? resident_blocks_per_cu<double>(model, plan->cols, plan->sw) : resident_blocks_per_cu<float>(model, plan->cols, plan->sw);
	plan->resident_blocks = (long)device_cus() * per_cu;
	// Rows per work item, a fixed rule ("Ensembles"): 32 -- the single slab's chunk where a launch fills the device -- halved
	// while all members together would not give two rounds of resident blocks, down to 8; 4 where even 8-row chunks leave half the CUs
	// without a block (fused_chunk_rows' rule for tiny launches).
	auto blocks = [&](int chunk) { return (long)members * plan->nsb * ((ny + chunk - 1) / chunk); };
	int chunk = 32;
	while (chunk > 8 && blocks(chunk) < 2 * plan->resident_blocks) chunk /= 2;
	if (chunk == 8 && blocks(8) < device_cus() / 2) chunk = 4;
	plan->chunk = std::min(chunk, ny);
	plan->nchunks = (ny + plan->chunk - 1) / plan->chunk;
	return launch_status();
}

hipError_t launch_ensemble_step(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleStep &e, hipStream_t s)
{
	clear_launch_status();
	if (e.nblocks <= 0) return hipSuccess;
	const hipError_t r = precision == CRD_PRECISION_F64 ? launch_real<double>(model, cols, absorb, table, e, s) : launch_real<float>(model, cols, absorb, table, e, s);
	return r != hipSuccess ? r : launch_status();
}

hipError_t launch_ensemble_aos_to_planes(int precision, int src_is_f64, const void *aos, void *u, void *v, size_t n, hipStream_t s)
{
	clear_launch_status();
	if (n == 0) return hipSuccess;
	const int g = grid_for(n);
	if (precision == CRD_PRECISION_F64) {
		if (!src_is_f64) return hipErrorInvalidValue;
		crd_ensemble_aos_to_planes_kernel<double, double><<<g, 256, 0, s>>>(static_cast<const double *>(aos), static_cast<double *>(u), static_cast<double *>(v), n);
	} else if (src_is_f64) {
		crd_ensemble_aos_to_planes_kernel<double, float><<<g, 256, 0, s>>>(static_cast<const double *>(aos), static_cast<float *>(u), static_cast<float *>(v), n);
	} else {
		crd_ensemble_aos_to_planes_kernel<float, float><<<g, 256, 0, s>>>(static_cast<const float *>(aos), static_cast<float *>(u), static_cast<float *>(v), n);
	}
	return launch_status();
}

hipError_t launch_ensemble_planes_to_aos(int precision, int dst_is_f64, const void *u, const void *v, void *aos, size_t n, hipStream_t s)
{
	clear_launch_status();
	if (n == 0) return hipSuccess;
	const int g = grid_for(n);
	if (precision == CRD_PRECISION_F64) {
		if (!dst_is_f64) return hipErrorInvalidValue;
		crd_ensemble_planes_to_aos_kernel<double, double><<<g, 256, 0, s>>>(static_cast<const double *>(u), static_cast<const double *>(v), static_cast<double *>(aos), n);
	} else if (dst_is_f64) {
		crd_ensemble_planes_to_aos_kernel<double, float><<<g, 256, 0, s>>>(static_cast<const float *>(u), static_cast<const float *>(v), static_cast<double *>(aos), n);
	} else {
		crd_ensemble_planes_to_aos_kernel<float, float><<<g, 256, 0, s>>>(static_cast<const float *>(u), static_cast<const float *>(v), static_cast<float *>(aos), n);
	}
	return launch_status();
}

hipError_t launch_ensemble_max_abs(int precision, const EnsembleMember *table, int members, int src, size_t n, double *out_dev, hipStream_t s)
{
	clear_launch_status();
	if (members < 1) return hipSuccess;
	if (hipError_t e = hipMemsetAsync(out_dev, 0, (size_t)members * sizeof(double), s); e != hipSuccess || n == 0) return e;
	const dim3 grid((unsigned)grid_for(n, 64), (unsigned)members);
	if (precision == CRD_PRECISION_F64) crd_ensemble_max_abs_kernel<double><<<grid, 256, 0, s>>>(table, src, n, out_dev);
	else crd_ensemble_max_abs_kernel<float><<<grid, 256, 0, s>>>(table, src, n, out_dev);
	return launch_status();
}

}  // namespace crd
