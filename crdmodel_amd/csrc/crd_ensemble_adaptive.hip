// crd_ensemble_adaptive.hip -- the kernels of an ensemble's error-controlled integration (crd_ensemble.cpp drives them): one
// Zonneveld 5(3)4 attempt of every active member in ONE launch, the per-member sums of its error partials, and the per-member
// counterparts of the element-wise operations a context's integrator runs for arkHin and the dense output.  Every member goes through
// the arithmetic a lone single-slab context goes through: the attempt runs fused_item with EMBED = 2 (the body of a context's attempt),
// the RHS calls rhs_point_values with the stage kernel's operands, and the element-wise operations and the ydd norm are those of
// crd_kernels.hip, per member.  Only the attempt's error norm is summed over another partition of work items.  The attempt kernel
// sets its work item up itself (hand-written, as crd_ensemble_item.h's header explains); its instantiation ladder and its plan are
// that header's.  DESIGN.md, "Ensembles".
#include "crd_ensemble.h"
#include "crd_fused_impl.h"
#include "crd_ensemble_item.h"

namespace crd {

namespace {

typedef const __attribute__((address_space(4))) EnsembleAttempt ConstAttempt;
typedef const __attribute__((address_space(4))) EnsembleOp ConstOp;

template <typename Real>
struct AttemptArgs {
	Real rtol, atol, ka4;  // rounded on the host as launch_fused_t rounds them
	EnsembleAttemptLaunch l;
};

// One attempt per active member.  A block is a work item of one attempt: block id -> (slot, chunk of rows, strips of columns), with
// the step kernel's XCD remap; the attempt table says which member a slot is and with which step size it runs.  Held to the
// wavefronts per SIMD of the single-slab attempt kernel (kMinWaves<..., STEPS = 1, ...>).
template <typename Real, int MODEL, bool ABSORB>
__global__ void __launch_bounds__(kLanes *kMaxWavesPerBlock) __attribute__((amdgpu_waves_per_eu(kMinWaves<Real, MODEL, 1, 1, ABSORB>)))
crd_ensemble_attempt_kernel(const EnsembleMember *members, const EnsembleAttempt *attempts, AttemptArgs<Real> aa)
{
	const EnsembleAttemptLaunch &l = aa.l;
	const int blk = xcd_remap((int)blockIdx.x, l.nblocks);
	const int slot = __builtin_amdgcn_readfirstlane(blk / l.member_blocks);
	const int rest = blk - slot * l.member_blocks;
	const int cblk = rest / l.nsb;
	const int strip = __builtin_amdgcn_readfirstlane((rest - cblk * l.nsb) * l.sw + (int)(threadIdx.x >> 6));
	const int chunk = __builtin_amdgcn_readfirstlane(cblk);
	if (strip >= l.nstrips) return;  // (a barrier waits for the surviving wavefronts of the workgroup only)
	ConstAttempt *const at = (ConstAttempt *)attempts + slot;
	const int member = at->member;
	ConstMember *const m = (ConstMember *)members + member;
	// (written out, not through crd_ensemble_item.h's helpers: timed against the hand-written kernel this one lay outside the noise of the
	// measurement in one case, profiles/ensemble/refactor_ab.txt, and the rule is then the hand-written form)
	const size_t plane = (size_t)l.nx * (size_t)l.ny;

	Slab<Real> s;
	s.cE = static_cast<const Real *>(m->cE);
	s.cWn = static_cast<const Real *>(m->cWn);
	s.cP = static_cast<const Real *>(m->cP);
	s.brow = static_cast<const Real *>(m->brow) + kGhost;  // index by row
	s.ka4 = aa.ka4;
	s.nx = l.nx;
	s.nyl = l.ny;
	s.wrap = 1;  // a member is a single slab: phi wraps inside it
	s.has_row0 = s.has_rowN = 1;
	s.just_diffusion = MODEL == kModelDiffusionOnly;
	s.wrap_x = 1;
	FusedArgs<Real> a{};
	a.in_u = static_cast<const Real *>(at->in);
	a.in_v = a.in_u + plane;
	a.out_u = static_cast<Real *>(at->out);
	a.out_v = a.out_u + plane;
	if constexpr (sizeof(Real) == 8) {
		a.h1 = at->h[0];
		a.h2 = at->h[1];
		a.h3 = at->h[2];
		a.h6 = at->h[3];
	} else {
		a.h1 = at->hf[0];
		a.h2 = at->hf[1];
		a.h3 = at->hf[2];
		a.h6 = at->hf[3];
	}
	bool absorbs = false;
	if constexpr (ABSORB) {
		for (int k = 0; k < 5; k++) {
			a.absorb[k] = at->absorb[k];
			absorbs = absorbs || a.absorb[k];
		}
	}
	a.js = 0;
	a.ny = l.ny;
	a.r_begin[0] = a.r_begin[1] = 0;
	a.r_end[0] = a.r_end[1] = l.ny;
	a.chunk = l.chunk;
	a.first2 = a.nchunks = l.nchunks;
	a.nstrips = l.nstrips;
	a.nitems = l.member_items;
	a.nblocks = l.nblocks;
	a.sw = l.sw;
	a.err_partials = l.partials + (size_t)member * (size_t)l.member_items;
	a.rtol = aa.rtol;
	a.atol = aa.atol;
	a.err_lo = INT32_MIN;  // a single slab: every row it produces is its own
	a.err_hi = INT32_MAX;
	if constexpr (ABSORB) {
		// The selects only where this member absorbs at some stage AND the chunk's pipeline -- rows [j0 - kApron - 1, j1 + kApron + 1)
		// with the fifth stage's row -- can meet global row 0 or ny - 1 (crd_rk4_fused_step_kernel's per-chunk rule with EMBED's apron).
		constexpr int kEmbedApron = kApron + 1;
		const int j0 = chunk * l.chunk, j1 = (j0 + l.chunk < l.ny) ? j0 + l.chunk : l.ny;
		if (absorbs && (j0 - kEmbedApron <= 0 || j1 + kEmbedApron >= l.ny)) {
			fused_item<Real, MODEL, true, 2, 1, false>(s, a, strip, chunk);
			return;
		}
	}
	fused_item<Real, MODEL, false, 2, 1, false>(s, a, strip, chunk);
}

// One workgroup per slot: the member's partials added in crd_sum_partials_kernel's fixed order (thread t takes items t, t + 256, ...;
// then a fixed LDS tree).
__global__ void __launch_bounds__(256) crd_ensemble_sum_partials_kernel(const EnsembleAttempt *attempts, const double *__restrict__ partials, int n,
                                                                        double *__restrict__ out)
{
	__shared__ double part[256];
	ConstAttempt *const at = (ConstAttempt *)attempts + blockIdx.x;
	const double *const p = partials + (size_t)at->member * (size_t)n;
	double sum = 0.0;
	for (int q = threadIdx.x; q < n; q += 256) sum += p[q];
	part[threadIdx.x] = sum;
	__syncthreads();
	for (int w = 128; w > 0; w >>= 1) {
		if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
		__syncthreads();
	}
	if (threadIdx.x == 0) out[blockIdx.x] = part[0];
}

// f(t, x0) -> out, blockIdx.y = op: one thread per point, neighbours straight from memory (theta and phi wrap), the point function
// with the operands crd_rk4_stage_kernel's STAGE 0 gives it.
template <typename Real, int MODEL>
__global__ void __launch_bounds__(256) crd_ensemble_rhs_kernel(const EnsembleMember *members, const EnsembleOp *ops, int nx, int ny, Real ka4)
{
	ConstOp *const op = (ConstOp *)ops + blockIdx.y;
	ConstMember *const m = (ConstMember *)members + op->member;
	const Real *const cEt = static_cast<const Real *>(m->cE);
	const Real *const cWnt = static_cast<const Real *>(m->cWn);
	const Real *const cPt = static_cast<const Real *>(m->cP);
	const Real *const brow = static_cast<const Real *>(m->brow) + kGhost;
	const size_t n = (size_t)nx * (size_t)ny;
	const Real *const u = static_cast<const Real *>(op->x[0]);
	const Real *const v = u + n;
	Real *const du_out = static_cast<Real *>(op->out);
	Real *const dv_out = du_out + n;
	const bool absorb = op->absorb != 0;
	for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
		const int j = (int)(q / (size_t)nx), i = (int)(q - (size_t)j * (size_t)nx);
		const int iw = i == 0 ? nx - 1 : i - 1, ie = i == nx - 1 ? 0 : i + 1;
		const int js = j == 0 ? ny - 1 : j - 1, jn = j == ny - 1 ? 0 : j + 1;
		const size_t row = (size_t)j * nx;
		const bool zero = absorb && (j == 0 || j == ny - 1);
		Real du, dv;
		rhs_point_values<Real, MODEL>(u[q], u[row + iw], u[row + ie], u[(size_t)js * nx + i], u[(size_t)jn * nx + i], v[q], cEt[i], cWnt[i], cPt[i], brow[j], ka4, zero,
		                              du, dv);
		du_out[q] = du;
		dv_out[q] = dv;
	}
}

// crd_hin_bound_kernel per op: both fields, folded into out[op] with an atomic max on the bit pattern (exact in any order)
template <typename Real>
__global__ void __launch_bounds__(256) crd_ensemble_hin_bound_kernel(const EnsembleOp *ops, size_t n, double rtol, double atol, double *out)
{
	__shared__ double part[4];
	ConstOp *const op = (ConstOp *)ops + blockIdx.y;
	const Real *const y = static_cast<const Real *>(op->x[0]);
	const Real *const f = static_cast<const Real *>(op->x[1]);
	double m = 0.0;
	for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < 2 * n; q += (size_t)gridDim.x * blockDim.x) {
		const double ay = fabs((double)y[q]);
		const double r = fabs((double)f[q]) / (0.1 * ay + (rtol * ay + atol));
		m = (r > m || r != r) ? r : m;
	}
	for (int off = 32; off > 0; off >>= 1) {
		const double o = __shfl_down(m, off, 64);
		m = (o > m || o != o) ? o : m;
	}
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < 4; w++) m = (part[w] > m || part[w] != part[w]) ? part[w] : m;
		atomicMax(reinterpret_cast<unsigned long long *>(out + blockIdx.y), (unsigned long long)__double_as_longlong(m));
	}
}

// crd_axpy_kernel per op over both fields: out = x0 + h x1
template <typename Real>
__global__ void __launch_bounds__(256) crd_ensemble_axpy_kernel(const EnsembleOp *ops, size_t n)
{
	ConstOp *const op = (ConstOp *)ops + blockIdx.y;
	const Real *const y = static_cast<const Real *>(op->x[0]);
	const Real *const f = static_cast<const Real *>(op->x[1]);
	Real *const out = static_cast<Real *>(op->out);
	Real h;
	if constexpr (sizeof(Real) == 8) h = op->c[0];
	else h = op->cf[0];
	for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < 2 * n; q += (size_t)gridDim.x * blockDim.x) out[q] = fmadd(h, f[q], y[q]);
}

// crd_ydd_sumsq_kernel per op: kEnsembleNormBlocks blocks stride each field in the lone kernel's pattern, u first, and the block's
// partial is (0 + sum over u) + sum over v, as the lone launch pair leaves it.
template <typename Real>
__global__ void __launch_bounds__(256) crd_ensemble_ydd_sumsq_kernel(const EnsembleOp *ops, size_t n, double rtol, double atol, double *__restrict__ partials)
{
	__shared__ double part[256];
	ConstOp *const op = (ConstOp *)ops + blockIdx.y;
	const double inv_h = op->c[0];
	double acc = 0.0;
	for (int f = 0; f < 2; f++) {
		const Real *const y = static_cast<const Real *>(op->x[0]) + (size_t)f * n;
		const Real *const f0 = static_cast<const Real *>(op->x[1]) + (size_t)f * n;
		const Real *const f2 = static_cast<const Real *>(op->x[2]) + (size_t)f * n;
		double sum = 0.0;
		for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
			const double e = ((double)f2[q] - (double)f0[q]) * inv_h / (rtol * fabs((double)y[q]) + atol);
			sum = fma(e, e, sum);
		}
		part[threadIdx.x] = sum;
		__syncthreads();
		for (int w = 128; w > 0; w >>= 1) {
			if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
			__syncthreads();
		}
		acc = (f ? acc : 0.0) + part[0];
		__syncthreads();  // (part is reused by the next field)
	}
	if (threadIdx.x == 0) partials[(size_t)blockIdx.y * kEnsembleNormBlocks + blockIdx.x] = acc;
}

// crd_sum_blocks_kernel per op
__global__ void __launch_bounds__(kEnsembleNormBlocks) crd_ensemble_sum_blocks_kernel(const double *__restrict__ partials, double *__restrict__ out)
{
	__shared__ double part[kEnsembleNormBlocks];
	part[threadIdx.x] = partials[(size_t)blockIdx.x * kEnsembleNormBlocks + threadIdx.x];
	__syncthreads();
	for (int w = kEnsembleNormBlocks / 2; w > 0; w >>= 1) {
		if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
		__syncthreads();
	}
	if (threadIdx.x == 0) out[blockIdx.x] = part[0];
}

// crd_hermite_kernel per op over both fields: x0 = y_n, x1 = y_{n+1}, x2 = f_n, x3 = f_{n+1}; c = h00, h10, h01, h11
template <typename Real>
__global__ void __launch_bounds__(256) crd_ensemble_hermite_kernel(const EnsembleOp *ops, size_t n)
{
	ConstOp *const op = (ConstOp *)ops + blockIdx.y;
	const Real *const yn = static_cast<const Real *>(op->x[0]);
	const Real *const yp = static_cast<const Real *>(op->x[1]);
	const Real *const fn = static_cast<const Real *>(op->x[2]);
	const Real *const fp = static_cast<const Real *>(op->x[3]);
	Real *const out = static_cast<Real *>(op->out);
	Real h00, h10, h01, h11;
	if constexpr (sizeof(Real) == 8) {
		h00 = op->c[0];
		h10 = op->c[1];
		h01 = op->c[2];
		h11 = op->c[3];
	} else {
		h00 = op->cf[0];
		h10 = op->cf[1];
		h01 = op->cf[2];
		h11 = op->cf[3];
	}
	for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < 2 * n; q += (size_t)gridDim.x * blockDim.x)
		out[q] = fmadd(h00, yn[q], fmadd(h10, fn[q], fmadd(h01, yp[q], h11 * fp[q])));
}

inline unsigned grid_for(size_t n, size_t cap = 2048) { return (unsigned)((n + 255) / 256 < cap ? (n + 255) / 256 : cap); }

template <typename Real>
void rhs_real(int model, const EnsembleMember *table, const EnsembleOp *ops, int count, int nx, int ny, Real ka4, hipStream_t s)
{
	const dim3 grid(grid_for((size_t)nx * (size_t)ny), (unsigned)count);
	switch (model) {
	case CRD_MODEL_FHN: crd_ensemble_rhs_kernel<Real, CRD_MODEL_FHN><<<grid, 256, 0, s>>>(table, ops, nx, ny, ka4); break;
	case CRD_MODEL_GOLDBETER: crd_ensemble_rhs_kernel<Real, CRD_MODEL_GOLDBETER><<<grid, 256, 0, s>>>(table, ops, nx, ny, ka4); break;
	default: crd_ensemble_rhs_kernel<Real, kModelDiffusionOnly><<<grid, 256, 0, s>>>(table, ops, nx, ny, ka4); break;
	}
}

}  // namespace

hipError_t ensemble_attempt_plan(int precision, int model, int nx, int ny, int members, EnsemblePlan *plan)
{
	clear_launch_status();
	plan->cols = 1;  // (the embedded pairs run one column per lane)
	cut_strips(nx, ny, 1, kApron + 1, false, plan);  // the embedded apron: 54 valid columns per wavefront
	const int per_cu = resident_blocks_per_cu(precision, model, 1, plan->sw, [](auto k) {
		using K = decltype(k);
		return crd_ensemble_attempt_kernel<typename K::Real, K::kModel, K::kAbsorb>;
	});
	plan->resident_blocks = (long)device_cus() * per_cu;
	// ensemble_plan's chunk rule, over all B members
	auto blocks = [&](int chunk) { return (long)members * plan->nsb * ((ny + chunk - 1) / chunk); };
	plan->chunk = std::min(ensemble_chunk_rows(32, blocks, plan->resident_blocks, device_cus() / 2), ny);
	plan->nchunks = (ny + plan->chunk - 1) / plan->chunk;
	return launch_status();
}

hipError_t launch_ensemble_attempts(int precision, int model, bool absorb, const EnsembleMember *table, const EnsembleAttempt *attempts, int count,
                                    const EnsembleAttemptLaunch &l, double *sums_dev, hipStream_t s)
{
	clear_launch_status();
	if (count <= 0) return hipSuccess;
	if (l.nblocks != l.member_blocks * count) return hipErrorInvalidValue;
	(void)with_instantiation(precision, model, 1, absorb, [&](auto k) {
		using Real = typename decltype(k)::Real;
		const AttemptArgs<Real> a{(Real)l.rtol, (Real)l.atol, (Real)l.ka4, l};  // rounded on the host as launch_fused_t rounds them
		crd_ensemble_attempt_kernel<Real, decltype(k)::kModel, decltype(k)::kAbsorb><<<l.nblocks, kLanes * l.sw, 0, s>>>(table, attempts, a);
	});
	crd_ensemble_sum_partials_kernel<<<count, 256, 0, s>>>(attempts, l.partials, l.member_items, sums_dev);
	return launch_status();
}

hipError_t launch_ensemble_rhs(int precision, int model, const EnsembleMember *table, const EnsembleOp *ops, int count, int nx, int ny, double ka4, hipStream_t s)
{
	clear_launch_status();
	if (count <= 0) return hipSuccess;
	if (precision == CRD_PRECISION_F64) rhs_real<double>(model, table, ops, count, nx, ny, (double)ka4, s);
	else rhs_real<float>(model, table, ops, count, nx, ny, (float)ka4, s);
	return launch_status();
}

hipError_t launch_ensemble_hin_bound(int precision, const EnsembleOp *ops, int count, size_t n, double rtol, double atol, double *out_dev, hipStream_t s)
{
	clear_launch_status();
	if (count <= 0) return hipSuccess;
	if (hipError_t e = hipMemsetAsync(out_dev, 0, (size_t)count * sizeof(double), s); e != hipSuccess) return e;
	const dim3 grid(grid_for(2 * n), (unsigned)count);
	if (precision == CRD_PRECISION_F64) crd_ensemble_hin_bound_kernel<double><<<grid, 256, 0, s>>>(ops, n, rtol, atol, out_dev);
	else crd_ensemble_hin_bound_kernel<float><<<grid, 256, 0, s>>>(ops, n, rtol, atol, out_dev);
	return launch_status();
}

hipError_t launch_ensemble_axpy(int precision, const EnsembleOp *ops, int count, size_t n, hipStream_t s)
{
	clear_launch_status();
	if (count <= 0) return hipSuccess;
	const dim3 grid(grid_for(2 * n), (unsigned)count);
	if (precision == CRD_PRECISION_F64) crd_ensemble_axpy_kernel<double><<<grid, 256, 0, s>>>(ops, n);
	else crd_ensemble_axpy_kernel<float><<<grid, 256, 0, s>>>(ops, n);
	return launch_status();
}

hipError_t launch_ensemble_ydd_sumsq(int precision, const EnsembleOp *ops, int count, size_t n, double rtol, double atol, double *partials_dev, double *out_dev,
                                     hipStream_t s)
{
	clear_launch_status();
	if (count <= 0) return hipSuccess;
	const dim3 grid(kEnsembleNormBlocks, (unsigned)count);
	if (precision == CRD_PRECISION_F64) crd_ensemble_ydd_sumsq_kernel<double><<<grid, 256, 0, s>>>(ops, n, rtol, atol, partials_dev);
	else crd_ensemble_ydd_sumsq_kernel<float><<<grid, 256, 0, s>>>(ops, n, rtol, atol, partials_dev);
	crd_ensemble_sum_blocks_kernel<<<count, kEnsembleNormBlocks, 0, s>>>(partials_dev, out_dev);
	return launch_status();
}

void ensemble_hermite_coefficients(double theta, double h, double c[4], float cf[4])
{
	const double t2 = theta * theta, t3 = t2 * theta;
	c[0] = 2.0 * t3 - 3.0 * t2 + 1.0;
	c[1] = (t3 - 2.0 * t2 + theta) * h;
	c[2] = -2.0 * t3 + 3.0 * t2;
	c[3] = (t3 - t2) * h;
	for (int k = 0; k < 4; k++) cf[k] = (float)c[k];
}

hipError_t launch_ensemble_hermite(int precision, const EnsembleOp *ops, int count, size_t n, hipStream_t s)
{
	clear_launch_status();
	if (count <= 0) return hipSuccess;
	const dim3 grid(grid_for(2 * n), (unsigned)count);
	if (precision == CRD_PRECISION_F64) crd_ensemble_hermite_kernel<double><<<grid, 256, 0, s>>>(ops, n);
	else crd_ensemble_hermite_kernel<float><<<grid, 256, 0, s>>>(ops, n);
	return launch_status();
}

}  // namespace crd
