// crd_ensemble.hip -- the ensemble step: one classical RK4 step of B independent members in ONE launch (crd_ensemble.cpp drives it).
// A block is a work item of one member: block id -> (member, chunk of rows, strips of columns).  The work item runs fused_item, the
// one-step body of the single-slab kernel (crd_fused_impl.h), on that member's planes and tables, so every point of a member goes
// through the arithmetic it goes through in a context stepped alone: the results are bit-identical to crd_step_rk4 with the one-launch
// stepper, under any plan.  The members' descriptors are read through the constant address space (scalar loads); what the members
// share -- step size, stage times, geometry, chunking -- comes in the kernel arguments.  The work item is set up by
// crd_ensemble_item.h, as in every ensemble step unit.  DESIGN.md, "Ensembles".
#include "crd_ensemble.h"
#include "crd_fused_impl.h"
#include "crd_ensemble_item.h"

namespace crd {

namespace {

// What a launch passes to the kernel: the step's constants in the kernel's precision and EnsembleStep.
template <typename Real>
struct EnsembleArgs {
	StepConstants<Real> k;
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

	const Slab<Real> s = member_slab<Real, MODEL>(m, ea.k.ka4, e.nx, e.ny);
	FusedArgs<Real> a{};
	member_planes(a, m, e.src);
	step_sizes(a, ea.k);
	bool absorbs = false;
	if constexpr (ABSORB) absorbs = stage_absorbs(a, e.t_stage, m->t_boundary);
	item_geometry(a, e.ny, e.nstrips, e.nchunks, e.nstrips * e.nchunks, e.chunk, e.sw, e.nblocks);
	step_item<Real, MODEL, ABSORB, COLS>(s, a, absorbs, strip, chunk);
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

// blockIdx.y = member
template <typename Real>
__global__ void __launch_bounds__(256) crd_ensemble_max_abs_kernel(const EnsembleMember *members, int src, size_t n, double *out)
{
	ConstMember *const mem = (ConstMember *)members + blockIdx.y;
	member_max_abs(static_cast<const Real *>(mem->u[src]), n, out);
}

inline int grid_for(size_t n, size_t cap = 2048) { return (int)((n + 255) / 256 < cap ? (n + 255) / 256 : cap); }

}  // namespace

hipError_t ensemble_plan(int precision, int model, int nx, int ny, int members, EnsemblePlan *plan)
{
	clear_launch_status();
	const bool f64 = precision == CRD_PRECISION_F64;
	plan->cols = (!f64 && nx % 2 == 0) ? 2 : 1;  // fused_default_columns: the packed arithmetic for fp32 where the pairs do not straddle the seam
	cut_strips(nx, ny, plan->cols, kApron, false, plan);
	const int per_cu = resident_blocks_per_cu(precision, model, plan->cols, plan->sw, [](auto k) {
		using K = decltype(k);
		return crd_ensemble_step_kernel<typename K::Real, K::kModel, K::kAbsorb, K::kCols>;
	});
	plan->resident_blocks = (long)device_cus() * per_cu;
	// 32 rows -- the single slab's chunk where a launch fills the device -- under the ensembles' halving rule
	auto blocks = [&](int chunk) { return (long)members * plan->nsb * ((ny + chunk - 1) / chunk); };
	plan->chunk = std::min(ensemble_chunk_rows(32, blocks, plan->resident_blocks, device_cus() / 2), ny);
	plan->nchunks = (ny + plan->chunk - 1) / plan->chunk;
	return launch_status();
}

hipError_t launch_ensemble_step(int precision, int model, int cols, bool absorb, const EnsembleMember *table, const EnsembleStep &e, hipStream_t s)
{
	clear_launch_status();
	if (e.nblocks <= 0) return hipSuccess;
	const hipError_t r = with_instantiation(precision, model, cols, absorb, [&](auto k) {
		using K = decltype(k);
		const EnsembleArgs<typename K::Real> a{StepConstants<typename K::Real>(e), e};
		crd_ensemble_step_kernel<typename K::Real, K::kModel, K::kAbsorb, K::kCols><<<e.nblocks, kLanes * e.sw, 0, s>>>(table, a);
	});
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
