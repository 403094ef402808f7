// crd_imex.hip -- the stage close of crd_step_imex (include/crd.h): everything between two linear solves of an IMEX step in ONE
// pointwise pass over the AoS vectors.  Templated on Real and model.
//
//   crd_imex_close_kernel   Y_i = fma(dt gamma, k_i, R_i); FR_i = f_R(Y_i) by rhs_point_reaction of crd_jacobian.h, unchanged -- the
//                           bits of crd_rhs_part_*(CRD_PART_REACTION) on Y_i; R_{i+1} = y_n + the row's terms, one explicit fma each, in
//                           the order crd_imex.h states.  Y_i itself is never stored.  Stage 0 is the same kernel without k; the LAST
//                           instantiation (stage s) stores Y_s and leaves per-block partials of max |var0|, NaN propagating.
//   crd_imex_max_kernel     the partials' maximum in a fixed order (one wavefront), as crd_krylov.hip sums its partials.
//   crd_imex_estimate_kernel  the last close of an error-controlled step (crd_integrate_imex): Y_s as above and, in the same pass, the
//                           embedded pair's error estimate and the sum of its weighted squares in double, reduced as crd_bicgstab.hip
//                           reduces its dots; crd_imex_max_sum_kernel finishes both reductions, one wavefront each.
// A thread takes 16 bytes of every vector per grid-stride trip (one fp64 point, two fp32 points: global_load_dwordx4 either way) and
// issues all its loads before the first use.  Coefficients and pointers arrive in one by-value struct; no atomics, no scratch, no LDS
// besides the block's four maxima.
//
// Traffic in vector crossings, counted from the loop below: a close at stage i of an s-stage step reads R_i, k_i, y_n and the
// 2 i - 1 stored vectors of the row whose coefficients are not zero, and writes FR_i and R_{i+1}: ARS443's last-but-one close (i = 3)
// reads 8 and writes 2.  From single axpys (y = a x + y: 2 reads, 1 write) the same close takes Y_i (3), FR_i (2), a copy of y_n (2)
// and 7 axpys (21): 28 crossings.  The last close reads 2 and writes 1; stage 0 reads 1 and writes 2.
#include <hip/hip_runtime.h>

#include "crd_imex.h"
#include "crd_jacobian.h"

namespace crd {

namespace {

using namespace dev;

constexpr int kWaves = kImexThreads / 64;

template <typename Real> struct Unit;
template <> struct Unit<double> {
	typedef double type __attribute__((ext_vector_type(2)));
	static constexpr int kPoints = 1;
};
template <> struct Unit<float> {
	typedef float type __attribute__((ext_vector_type(4)));
	static constexpr int kPoints = 2;
};

// the 16 bytes at unit q; `full` is false only for the single point behind an odd number of fp32 points
template <typename Real>
__device__ __forceinline__ typename Unit<Real>::type load_unit(const void *p, size_t q, bool full)
{
	using V = typename Unit<Real>::type;
	if (full) return *(static_cast<const V *>(p) + q);
	const Real *e = static_cast<const Real *>(p) + q * (2 * Unit<Real>::kPoints);
	V x = (V)((Real)0);
	x[0] = e[0];
	x[1] = e[1];
	return x;
}
template <typename Real>
__device__ __forceinline__ void store_unit(void *p, size_t q, bool full, typename Unit<Real>::type x)
{
	using V = typename Unit<Real>::type;
	if (full) {
		*(static_cast<V *>(p) + q) = x;
		return;
	}
	Real *e = static_cast<Real *>(p) + q * (2 * Unit<Real>::kPoints);
	e[0] = x[0];
	e[1] = x[1];
}

template <typename V, typename Real>
__device__ __forceinline__ V fma_unit(double coef, V x, V acc)
{
	return __builtin_elementwise_fma((V)((Real)coef), x, acc);
}

// a row the absorbing boundary holds at zero while t < tBoundary (crd_jacobian.hip: absorbing_row)
template <typename Real>
__device__ __forceinline__ bool held_row(const Slab<Real> &s, int absorb, int j)
{
	return absorb && ((s.has_row0 && j == 0) || (s.has_rowN && j == s.nyl - 1));
}

__device__ __forceinline__ double max_nan(double m, double a) { return (a > m || a != a) ? a : m; }  // NaN propagates

template <typename Real, int MODEL, bool LAST>
__global__ void __launch_bounds__(kImexThreads) crd_imex_close_kernel(Slab<Real> s, ImexClose a, size_t npoints)
{
	using V = typename Unit<Real>::type;
	constexpr int PTS = Unit<Real>::kPoints;
	const size_t units = (npoints + PTS - 1) / PTS, step = (size_t)gridDim.x * kImexThreads;
	const bool narrow = npoints <= 0xffffffffull;  // rows by a 32-bit division wherever the point index fits
	double m = 0.0;
	for (size_t q = (size_t)blockIdx.x * kImexThreads + threadIdx.x; q < units; q += step) {
		const bool full = (q + 1) * PTS <= npoints;
		const V R = load_unit<Real>(a.R, q, full);
		V k = (V)((Real)0), Y = R;
		if (a.k) k = load_unit<Real>(a.k, q, full);
		if constexpr (LAST) {
			Y = fma_unit<V, Real>(a.hg, k, R);
			store_unit<Real>(a.out, q, full, Y);
#pragma unroll
			for (int e = 0; e < PTS; e++) m = max_nan(m, fabs((double)Y[2 * e]));  // (the tail's absent point is +0)
		} else {
			V acc = R, x[kImexMaxTerms];
			if (a.yn != a.R) acc = load_unit<Real>(a.yn, q, full);
#pragma unroll
			for (int t = 0; t < kImexMaxTerms; t++)
				if (t < a.nterms) x[t] = load_unit<Real>(a.term[t], q, full);
			if (a.k) Y = fma_unit<V, Real>(a.hg, k, R);
			V F;
#pragma unroll
			for (int e = 0; e < PTS; e++) {
				const size_t p = q * PTS + e;
				int j = narrow ? (int)((unsigned)p / (unsigned)s.nx) : (int)(p / (size_t)s.nx);
				if (j > s.nyl - 1) j = s.nyl - 1;  // (the tail's absent point)
				Real du, dv;
				rhs_point_reaction<Real, MODEL>(Y[2 * e], Y[2 * e + 1], s.brow[j], s.ka4, held_row(s, a.absorb, j), du, dv);
				F[2 * e] = du;
				F[2 * e + 1] = dv;
			}
			store_unit<Real>(a.FR, q, full, F);
#pragma unroll
			for (int t = 0; t < kImexMaxTerms; t++)
				if (t < a.nterms) acc = fma_unit<V, Real>(a.coef[t], x[t], acc);
			if (a.cE != 0.0) acc = fma_unit<V, Real>(a.cE, F, acc);
			if (a.k && a.cI != 0.0) acc = fma_unit<V, Real>(a.cI, k, acc);
			store_unit<Real>(a.Rnext, q, full, acc);
		}
	}
	if constexpr (LAST) {
		__shared__ double part[kWaves];
		for (int off = 32; off > 0; off >>= 1) m = max_nan(m, __shfl_down(m, off, 64));
		if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
		__syncthreads();
		if (threadIdx.x == 0) {
			for (int w = 1; w < kWaves; w++) m = max_nan(m, part[w]);
			a.partials[blockIdx.x] = m;
		}
	}
}

// *out = the maximum of `blocks` partials: a chain over every 64th, six shuffle steps.
__global__ void __launch_bounds__(64) crd_imex_max_kernel(const double *__restrict__ partials, int blocks, double *__restrict__ out)
{
	double m = 0.0;
	for (int b = (int)threadIdx.x; b < blocks; b += 64) m = max_nan(m, partials[b]);
	for (int off = 32; off > 0; off >>= 1) m = max_nan(m, __shfl_down(m, off, 64));
	if (threadIdx.x == 0) *out = m;
}

// acc + q of one real: the weighted square of crd_imex.h, every operation rounded once (nothing here contracts into an fma).
__device__ __forceinline__ double add_weighted_square(double acc, double e, double yn, double rtol, double atol)
{
#pragma clang fp contract(off)
	const double w = rtol * fabs(yn) + atol;
	const double r = e / w;
	const double q = r * r;
	return acc + q;
}

__device__ __forceinline__ double wave_sum(double a)
{
	for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
	return a;
}

// The last close with the embedded pair's estimate (crd_imex.h: ImexEstimate).  The first half of the loop body is the LAST branch of
// crd_imex_close_kernel; no kinetics, so no model.  Reads R_s, k_s, y_n and the stored vectors of the estimate (seven for ARS(4,4,3)),
// writes one: 11 crossings; a twelfth when e is stored.
template <typename Real>
__global__ void __launch_bounds__(kImexThreads) crd_imex_estimate_kernel(ImexEstimate a, size_t npoints)
{
	using V = typename Unit<Real>::type;
	constexpr int PTS = Unit<Real>::kPoints;
	const size_t units = (npoints + PTS - 1) / PTS, step = (size_t)gridDim.x * kImexThreads;
	double m = 0.0, acc = 0.0;
	for (size_t q = (size_t)blockIdx.x * kImexThreads + threadIdx.x; q < units; q += step) {
		const bool full = (q + 1) * PTS <= npoints;
		const V R = load_unit<Real>(a.R, q, full), k = load_unit<Real>(a.k, q, full), yn = load_unit<Real>(a.yn, q, full);
		V x[kImexEstimateTerms];
#pragma unroll
		for (int t = 0; t < kImexEstimateTerms; t++)
			if (t < a.nterms) x[t] = load_unit<Real>(a.term[t], q, full);
		const V Y = fma_unit<V, Real>(a.hg, k, R);
		store_unit<Real>(a.out, q, full, Y);
#pragma unroll
		for (int e = 0; e < PTS; e++) m = max_nan(m, fabs((double)Y[2 * e]));  // (the tail's absent point is +0)
		V e = (V)((Real)0);
		if (a.nterms > 0) e = (V)((Real)a.coef[0]) * x[0];
		else e = (V)((Real)a.ck) * k;
#pragma unroll
		for (int t = 1; t < kImexEstimateTerms; t++)
			if (t < a.nterms) e = fma_unit<V, Real>(a.coef[t], x[t], e);
		if (a.nterms > 0 && a.ck != 0.0) e = fma_unit<V, Real>(a.ck, k, e);
		if (a.e_out) store_unit<Real>(a.e_out, q, full, e);
#pragma unroll
		for (int i = 0; i < 2 * PTS; i++)
			if (full || i < 2) acc = add_weighted_square(acc, (double)e[i], (double)yn[i], a.rtol, a.atol);  // (the tail's absent point does not count)
	}
	__shared__ double part[2][kWaves];
	for (int off = 32; off > 0; off >>= 1) m = max_nan(m, __shfl_down(m, off, 64));
	acc = wave_sum(acc);
	if ((threadIdx.x & 63) == 0) {
		part[0][threadIdx.x >> 6] = m;
		part[1][threadIdx.x >> 6] = acc;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < kWaves; w++) m = max_nan(m, part[0][w]);
		a.max_partials[blockIdx.x] = m;
	} else if (threadIdx.x == 64) {
		a.sum_partials[blockIdx.x] = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
	}
}

// result[0] = the maximum of the blocks' maxima as crd_imex_max_kernel forms it (block 0); result[1] = the sum of the blocks' sums,
// lane l adding partials l, l + 64, ... in order, then six shuffle steps (block 1).  One wavefront each.
__global__ void __launch_bounds__(64) crd_imex_max_sum_kernel(const double *__restrict__ max_partials, const double *__restrict__ sum_partials, int blocks,
                                                              double *__restrict__ result)
{
	if (blockIdx.x == 0) {
		double m = 0.0;
		for (int b = (int)threadIdx.x; b < blocks; b += 64) m = max_nan(m, max_partials[b]);
		for (int off = 32; off > 0; off >>= 1) m = max_nan(m, __shfl_down(m, off, 64));
		if (threadIdx.x == 0) result[0] = m;
	} else {
		double s = 0.0;
		for (int b = (int)threadIdx.x; b < blocks; b += 64) s += sum_partials[b];
		s = wave_sum(s);
		if (threadIdx.x == 0) result[1] = s;
	}
}

template <typename Real>
hipError_t estimate_t(const SlabDesc &d, const ImexEstimate &a, hipStream_t st)
{
	constexpr int PTS = Unit<Real>::kPoints;
	const size_t npoints = (size_t)d.nx * (size_t)d.nyl, units = (npoints + PTS - 1) / PTS;
	const size_t want = (units + kImexThreads - 1) / kImexThreads;
	const int blocks = want < (size_t)kImexBlocks ? (int)(want ? want : 1) : kImexBlocks;
	crd_imex_estimate_kernel<Real><<<blocks, kImexThreads, 0, st>>>(a, npoints);
	crd_imex_max_sum_kernel<<<2, 64, 0, st>>>(a.max_partials, a.sum_partials, blocks, a.result);
	return launch_status();
}

template <typename Real, int MODEL>
hipError_t close_t(const SlabDesc &d, const ImexClose &a, hipStream_t st)
{
	constexpr int PTS = Unit<Real>::kPoints;
	const Slab<Real> s = typed<Real>(d);
	const size_t npoints = (size_t)d.nx * (size_t)d.nyl, units = (npoints + PTS - 1) / PTS;
	const size_t want = (units + kImexThreads - 1) / kImexThreads;
	const int blocks = want < (size_t)kImexBlocks ? (int)(want ? want : 1) : kImexBlocks;
	if (a.last) {
		crd_imex_close_kernel<Real, MODEL, true><<<blocks, kImexThreads, 0, st>>>(s, a, npoints);
		crd_imex_max_kernel<<<1, 64, 0, st>>>(a.partials, blocks, a.max_out);
	} else {
		crd_imex_close_kernel<Real, MODEL, false><<<blocks, kImexThreads, 0, st>>>(s, a, npoints);
	}
	return launch_status();
}

template <typename Real>
hipError_t close_r(const SlabDesc &d, const ImexClose &a, hipStream_t st)
{
	switch (kernel_model(d)) {
	case CRD_MODEL_FHN: return close_t<Real, CRD_MODEL_FHN>(d, a, st);
	case CRD_MODEL_GOLDBETER: return close_t<Real, CRD_MODEL_GOLDBETER>(d, a, st);
	default: return close_t<Real, kModelDiffusionOnly>(d, a, st);
	}
}

}  // namespace

hipError_t launch_imex_close(int precision, const SlabDesc &d, const ImexClose &a, hipStream_t s)
{
	clear_launch_status();
	if (!a.R || !a.yn || a.nterms < 0 || a.nterms > kImexMaxTerms || d.nx < 1 || d.nyl < 1) return hipErrorInvalidValue;
	if (a.last ? (!a.k || !a.out || !a.partials || !a.max_out) : (!a.FR || !a.Rnext)) return hipErrorInvalidValue;
	for (int t = 0; t < a.nterms; t++)
		if (!a.term[t]) return hipErrorInvalidValue;
	return precision == CRD_PRECISION_F64 ? close_r<double>(d, a, s) : close_r<float>(d, a, s);
}

hipError_t launch_imex_estimate(int precision, const SlabDesc &d, const ImexEstimate &a, hipStream_t s)
{
	clear_launch_status();
	if (!a.R || !a.k || !a.yn || !a.out || !a.max_partials || !a.sum_partials || !a.result || d.nx < 1 || d.nyl < 1) return hipErrorInvalidValue;
	if (a.nterms < 0 || a.nterms > kImexEstimateTerms) return hipErrorInvalidValue;
	for (int t = 0; t < a.nterms; t++)
		if (!a.term[t]) return hipErrorInvalidValue;
	return precision == CRD_PRECISION_F64 ? estimate_t<double>(d, a, s) : estimate_t<float>(d, a, s);
}

}  // namespace crd
