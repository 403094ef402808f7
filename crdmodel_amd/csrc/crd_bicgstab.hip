// crd_bicgstab.hip -- the vector kernels of right-preconditioned BiCGStab for (I - gamma J) z = r (crd_bicgstab_*, include/crd.h):
// everything between two launches of J v or of the multigrid cycle in ONE pass over the AoS vectors, the reductions the host needs
// next leaving the same pass.  All templated on Real, all on whole vectors of n reals.
//
//   crd_bcg_apply_dot_kernel   out = fma(-gamma, jv, x) in place over the J v buffer, var1 masked for the diffusion part, and the dots
//                              of the stored out against a second vector: <rhat, v>, or <t, s> and <t, t>.
//   crd_bcg_s_update_kernel    s = fma(-alpha, v, res) and ||s||^2.
//   crd_bcg_xr_update_kernel   x = fma(omega, shat, fma(alpha, phat, x)), res = fma(-omega, t, s), ||res||^2 and <rhat, res>.
//   crd_bcg_p_update_kernel    p = fma(beta, fma(-omega, v, p), res).
//   crd_bcg_x_half_kernel      x = fma(alpha, phat, x): the half exit.
//   crd_bcg_start_kernel       once per solve, and once more for the true residual: r, or r - (x - gamma J x), masked, into up to three
//                              vectors, with ||r||^2 and the squared norm of what it stored.
//   crd_bcg_sum_kernel         the partials of each sum in a fixed order (one wavefront per sum), as crd_krylov.hip sums its own.
// Shape: that of the IMEX stage close (crd_imex.hip).  A thread takes 16 bytes of every vector per grid-stride trip (two fp64 reals,
// four fp32 reals: global_load_dwordx4 either way) and issues all its loads before the first use; scalars arrive by value; no atomics,
// no scratch, no LDS besides the block's partials, and no kernel waits on anything.
//
// The sums' tree: a thread's chain acc = fma(a, b, acc) over the reals of its unit in order and over its trips (accumulators double in
// both precisions: the product of two floats is exact), the wavefront's six shuffle steps, the block's four wavefronts added in order,
// then one wavefront over the blocks: lane l adds partials l, l + 64, ... in order, six shuffle steps.  A term passes through at most
// trips x (reals per unit) + 6 + 3 + ceil(blocks / 64) + 6 additions.
//
// Traffic of one iteration in vector crossings, counted from the loops below: apply-dot 3 + 1 twice, s-update 2 + 1, xr-update 6 + 2,
// p-update 3 + 1: 23.
#include <hip/hip_runtime.h>

#include "crd_bicgstab.h"
#include "crd_device.h"
#include "crd_kernels.h"

namespace crd {

namespace {

using namespace dev;

constexpr int kWaves = kBcgThreads / 64;

template <typename Real> struct Unit;
template <> struct Unit<double> {
	typedef double type __attribute__((ext_vector_type(2)));
	static constexpr int kReals = 2;
};
template <> struct Unit<float> {
	typedef float type __attribute__((ext_vector_type(4)));
	static constexpr int kReals = 4;
};

// the 16 bytes at unit q; `full` is false only for the two reals behind an odd number of fp32 points (the absent two read as +0)
template <typename Real>
__device__ __forceinline__ typename Unit<Real>::type load_unit(const void *p, size_t q, bool full)
{
	using V = typename Unit<Real>::type;
	if (full) return *(static_cast<const V *>(p) + q);
	const Real *e = static_cast<const Real *>(p) + q * Unit<Real>::kReals;
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
	Real *e = static_cast<Real *>(p) + q * Unit<Real>::kReals;
	e[0] = x[0];
	e[1] = x[1];
}

template <typename V, typename Real>
__device__ __forceinline__ V fma_unit(Real coef, V x, V acc)
{
	return __builtin_elementwise_fma((V)(coef), x, acc);
}

// var1 (the odd reals) to +0
template <typename Real>
__device__ __forceinline__ typename Unit<Real>::type var0_of(typename Unit<Real>::type x)
{
#pragma unroll
	for (int e = 1; e < Unit<Real>::kReals; e += 2) x[e] = (Real)0;
	return x;
}

// acc = fma(a[e], b[e], acc) over the unit's reals in order
template <typename Real>
__device__ __forceinline__ double dot_unit(typename Unit<Real>::type a, typename Unit<Real>::type b, double acc)
{
#pragma unroll
	for (int e = 0; e < Unit<Real>::kReals; e++) acc = __builtin_fma((double)a[e], (double)b[e], acc);
	return acc;
}

__device__ __forceinline__ double wave_sum(double a)
{
	for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
	return a;
}

// partials[i * kBcgBlocks + block] = the block's share of sum i, i < S
template <int S>
__device__ __forceinline__ void leave_partials(const double (&acc)[S], double *__restrict__ partials)
{
	__shared__ double part[S][kWaves];
#pragma unroll
	for (int i = 0; i < S; i++) {
		const double a = wave_sum(acc[i]);
		if ((threadIdx.x & 63) == 0) part[i][threadIdx.x >> 6] = a;
	}
	__syncthreads();
	const int i = (int)threadIdx.x;
	if (i < S) partials[(size_t)i * kBcgBlocks + blockIdx.x] = ((part[i][0] + part[i][1]) + part[i][2]) + part[i][3];
}

// One wavefront per sum: out[i] = the sum of its `blocks` partials.
__global__ void __launch_bounds__(64) crd_bcg_sum_kernel(const double *__restrict__ partials, int blocks, double *__restrict__ out)
{
	const int i = (int)blockIdx.x;
	double a = 0.0;
	for (int b = (int)threadIdx.x; b < blocks; b += 64) a += partials[(size_t)i * kBcgBlocks + b];
	a = wave_sum(a);
	if (threadIdx.x == 0) out[i] = a;
}

template <typename Real>
__global__ void __launch_bounds__(kBcgThreads) crd_bcg_start_kernel(const void *r, const void *x, const void *jv, Real gamma, int var0_only, void *out0, void *out1, void *out2,
                                                                    size_t n, double *__restrict__ partials)
{
	using V = typename Unit<Real>::type;
	constexpr int RPU = Unit<Real>::kReals;
	const size_t units = (n + RPU - 1) / RPU, step = (size_t)gridDim.x * kBcgThreads;
	double acc[2] = {0.0, 0.0};
	for (size_t q = (size_t)blockIdx.x * kBcgThreads + threadIdx.x; q < units; q += step) {
		const bool full = (q + 1) * RPU <= n;
		const V R = load_unit<Real>(r, q, full);
		V a = R;
		if (x) {
			const V X = load_unit<Real>(x, q, full), J = load_unit<Real>(jv, q, full);
			a = R - fma_unit<V, Real>(-gamma, J, X);
		}
		if (var0_only) a = var0_of<Real>(a);
		store_unit<Real>(out0, q, full, a);
		if (out1) store_unit<Real>(out1, q, full, a);
		if (out2) store_unit<Real>(out2, q, full, a);
		acc[0] = dot_unit<Real>(R, R, acc[0]);
		acc[1] = dot_unit<Real>(a, a, acc[1]);
	}
	leave_partials<2>(acc, partials);
}

template <typename Real, bool TWO>
__global__ void __launch_bounds__(kBcgThreads) crd_bcg_apply_dot_kernel(void *jv_out, const void *x, const void *b, Real gamma, int var0_only, size_t n,
                                                                        double *__restrict__ partials)
{
	using V = typename Unit<Real>::type;
	constexpr int RPU = Unit<Real>::kReals;
	const size_t units = (n + RPU - 1) / RPU, step = (size_t)gridDim.x * kBcgThreads;
	double acc[TWO ? 2 : 1] = {};
	for (size_t q = (size_t)blockIdx.x * kBcgThreads + threadIdx.x; q < units; q += step) {
		const bool full = (q + 1) * RPU <= n;
		const V J = load_unit<Real>(jv_out, q, full), X = load_unit<Real>(x, q, full), B = load_unit<Real>(b, q, full);
		V o = fma_unit<V, Real>(-gamma, J, X);
		if (var0_only) o = var0_of<Real>(o);
		store_unit<Real>(jv_out, q, full, o);
		acc[0] = dot_unit<Real>(o, B, acc[0]);
		if constexpr (TWO) acc[1] = dot_unit<Real>(o, o, acc[1]);
	}
	leave_partials<TWO ? 2 : 1>(acc, partials);
}

template <typename Real>
__global__ void __launch_bounds__(kBcgThreads) crd_bcg_s_update_kernel(void *__restrict__ s_out, const void *__restrict__ v, const void *__restrict__ res, Real alpha, size_t n,
                                                                       double *__restrict__ partials)
{
	using V = typename Unit<Real>::type;
	constexpr int RPU = Unit<Real>::kReals;
	const size_t units = (n + RPU - 1) / RPU, step = (size_t)gridDim.x * kBcgThreads;
	double acc[1] = {0.0};
	for (size_t q = (size_t)blockIdx.x * kBcgThreads + threadIdx.x; q < units; q += step) {
		const bool full = (q + 1) * RPU <= n;
		const V Vv = load_unit<Real>(v, q, full), R = load_unit<Real>(res, q, full);
		const V o = fma_unit<V, Real>(-alpha, Vv, R);
		store_unit<Real>(s_out, q, full, o);
		acc[0] = dot_unit<Real>(o, o, acc[0]);
	}
	leave_partials<1>(acc, partials);
}

template <typename Real>
__global__ void __launch_bounds__(kBcgThreads) crd_bcg_xr_update_kernel(void *x, const void *phat, const void *shat, const void *t, const void *sv, const void *rhat,
                                                                        void *res, Real alpha, Real omega, size_t n, double *__restrict__ partials)
{
	using V = typename Unit<Real>::type;
	constexpr int RPU = Unit<Real>::kReals;
	const size_t units = (n + RPU - 1) / RPU, step = (size_t)gridDim.x * kBcgThreads;
	double acc[2] = {0.0, 0.0};
	for (size_t q = (size_t)blockIdx.x * kBcgThreads + threadIdx.x; q < units; q += step) {
		const bool full = (q + 1) * RPU <= n;
		const V X = load_unit<Real>(x, q, full), P = load_unit<Real>(phat, q, full), Sh = load_unit<Real>(shat, q, full);
		const V T = load_unit<Real>(t, q, full), S = load_unit<Real>(sv, q, full), Rh = load_unit<Real>(rhat, q, full);
		const V xn = fma_unit<V, Real>(omega, Sh, fma_unit<V, Real>(alpha, P, X));
		const V rn = fma_unit<V, Real>(-omega, T, S);
		store_unit<Real>(x, q, full, xn);
		store_unit<Real>(res, q, full, rn);
		acc[0] = dot_unit<Real>(rn, rn, acc[0]);
		acc[1] = dot_unit<Real>(Rh, rn, acc[1]);
	}
	leave_partials<2>(acc, partials);
}

template <typename Real>
__global__ void __launch_bounds__(kBcgThreads) crd_bcg_p_update_kernel(void *p, const void *__restrict__ v, const void *__restrict__ res, Real beta, Real omega, size_t n)
{
	using V = typename Unit<Real>::type;
	constexpr int RPU = Unit<Real>::kReals;
	const size_t units = (n + RPU - 1) / RPU, step = (size_t)gridDim.x * kBcgThreads;
	for (size_t q = (size_t)blockIdx.x * kBcgThreads + threadIdx.x; q < units; q += step) {
		const bool full = (q + 1) * RPU <= n;
		const V P = load_unit<Real>(p, q, full), Vv = load_unit<Real>(v, q, full), R = load_unit<Real>(res, q, full);
		store_unit<Real>(p, q, full, fma_unit<V, Real>(beta, fma_unit<V, Real>(-omega, Vv, P), R));
	}
}

template <typename Real>
__global__ void __launch_bounds__(kBcgThreads) crd_bcg_x_half_kernel(void *x, const void *__restrict__ phat, Real alpha, size_t n)
{
	using V = typename Unit<Real>::type;
	constexpr int RPU = Unit<Real>::kReals;
	const size_t units = (n + RPU - 1) / RPU, step = (size_t)gridDim.x * kBcgThreads;
	for (size_t q = (size_t)blockIdx.x * kBcgThreads + threadIdx.x; q < units; q += step) {
		const bool full = (q + 1) * RPU <= n;
		const V X = load_unit<Real>(x, q, full), P = load_unit<Real>(phat, q, full);
		store_unit<Real>(x, q, full, fma_unit<V, Real>(alpha, P, X));
	}
}

template <typename Real> int blocks_for(size_t n) { return bcg_blocks((n + Unit<Real>::kReals - 1) / Unit<Real>::kReals); }

template <typename Real>
hipError_t start_t(const void *r, const void *x, const void *jv, double gamma, int var0_only, void *out0, void *out1, void *out2, size_t n, double *partials, double *sums,
                   hipStream_t s)
{
	const int blocks = blocks_for<Real>(n);
	crd_bcg_start_kernel<Real><<<blocks, kBcgThreads, 0, s>>>(r, x, jv, (Real)gamma, var0_only, out0, out1, out2, n, partials);
	crd_bcg_sum_kernel<<<2, 64, 0, s>>>(partials, blocks, sums);
	return launch_status();
}

template <typename Real>
hipError_t apply_dot_t(void *jv_out, const void *x, const void *b, double gamma, int var0_only, int two, size_t n, double *partials, double *sums, hipStream_t s)
{
	const int blocks = blocks_for<Real>(n);
	if (two) crd_bcg_apply_dot_kernel<Real, true><<<blocks, kBcgThreads, 0, s>>>(jv_out, x, b, (Real)gamma, var0_only, n, partials);
	else crd_bcg_apply_dot_kernel<Real, false><<<blocks, kBcgThreads, 0, s>>>(jv_out, x, b, (Real)gamma, var0_only, n, partials);
	crd_bcg_sum_kernel<<<two ? 2 : 1, 64, 0, s>>>(partials, blocks, sums);
	return launch_status();
}

template <typename Real>
hipError_t s_update_t(void *s_out, const void *v, const void *res, double alpha, size_t n, double *partials, double *sums, hipStream_t s)
{
	const int blocks = blocks_for<Real>(n);
	crd_bcg_s_update_kernel<Real><<<blocks, kBcgThreads, 0, s>>>(s_out, v, res, (Real)alpha, n, partials);
	crd_bcg_sum_kernel<<<1, 64, 0, s>>>(partials, blocks, sums);
	return launch_status();
}

template <typename Real>
hipError_t xr_update_t(void *x, const void *phat, const void *shat, const void *t, const void *sv, const void *rhat, void *res, double alpha, double omega, size_t n,
                       double *partials, double *sums, hipStream_t s)
{
	const int blocks = blocks_for<Real>(n);
	crd_bcg_xr_update_kernel<Real><<<blocks, kBcgThreads, 0, s>>>(x, phat, shat, t, sv, rhat, res, (Real)alpha, (Real)omega, n, partials);
	crd_bcg_sum_kernel<<<2, 64, 0, s>>>(partials, blocks, sums);
	return launch_status();
}

}  // namespace

hipError_t launch_bcg_start(int precision, const void *r, const void *x, const void *jv, double gamma, int var0_only, void *out0, void *out1, void *out2, size_t n,
                            double *partials, double *sums, hipStream_t s)
{
	clear_launch_status();
	if (!r || !out0 || !partials || !sums || n == 0 || (n & 1) || (x && !jv)) return hipErrorInvalidValue;
	return precision == CRD_PRECISION_F64 ? start_t<double>(r, x, jv, gamma, var0_only, out0, out1, out2, n, partials, sums, s)
	                                      : start_t<float>(r, x, jv, gamma, var0_only, out0, out1, out2, n, partials, sums, s);
}

hipError_t launch_bcg_apply_dot(int precision, void *jv_out, const void *x, const void *b, double gamma, int var0_only, int two, size_t n, double *partials, double *sums,
                                hipStream_t s)
{
	clear_launch_status();
	if (!jv_out || !x || !b || !partials || !sums || n == 0 || (n & 1)) return hipErrorInvalidValue;
	return precision == CRD_PRECISION_F64 ? apply_dot_t<double>(jv_out, x, b, gamma, var0_only, two, n, partials, sums, s)
	                                      : apply_dot_t<float>(jv_out, x, b, gamma, var0_only, two, n, partials, sums, s);
}

hipError_t launch_bcg_s_update(int precision, void *s_out, const void *v, const void *res, double alpha, size_t n, double *partials, double *sums, hipStream_t s)
{
	clear_launch_status();
	if (!s_out || !v || !res || !partials || !sums || n == 0 || (n & 1)) return hipErrorInvalidValue;
	return precision == CRD_PRECISION_F64 ? s_update_t<double>(s_out, v, res, alpha, n, partials, sums, s) : s_update_t<float>(s_out, v, res, alpha, n, partials, sums, s);
}

hipError_t launch_bcg_xr_update(int precision, void *x, const void *phat, const void *shat, const void *t, const void *sv, const void *rhat, void *res, double alpha,
                                double omega, size_t n, double *partials, double *sums, hipStream_t s)
{
	clear_launch_status();
	if (!x || !phat || !shat || !t || !sv || !rhat || !res || !partials || !sums || n == 0 || (n & 1)) return hipErrorInvalidValue;
	return precision == CRD_PRECISION_F64 ? xr_update_t<double>(x, phat, shat, t, sv, rhat, res, alpha, omega, n, partials, sums, s)
	                                      : xr_update_t<float>(x, phat, shat, t, sv, rhat, res, alpha, omega, n, partials, sums, s);
}

hipError_t launch_bcg_p_update(int precision, void *p, const void *v, const void *res, double beta, double omega, size_t n, hipStream_t s)
{
	clear_launch_status();
	if (!p || !v || !res || n == 0 || (n & 1)) return hipErrorInvalidValue;
	if (precision == CRD_PRECISION_F64) crd_bcg_p_update_kernel<double><<<blocks_for<double>(n), kBcgThreads, 0, s>>>(p, v, res, beta, omega, n);
	else crd_bcg_p_update_kernel<float><<<blocks_for<float>(n), kBcgThreads, 0, s>>>(p, v, res, (float)beta, (float)omega, n);
	return launch_status();
}

hipError_t launch_bcg_x_half(int precision, void *x, const void *phat, double alpha, size_t n, hipStream_t s)
{
	clear_launch_status();
	if (!x || !phat || n == 0 || (n & 1)) return hipErrorInvalidValue;
	if (precision == CRD_PRECISION_F64) crd_bcg_x_half_kernel<double><<<blocks_for<double>(n), kBcgThreads, 0, s>>>(x, phat, alpha, n);
	else crd_bcg_x_half_kernel<float><<<blocks_for<float>(n), kBcgThreads, 0, s>>>(x, phat, (float)alpha, n);
	return launch_status();
}

}  // namespace crd
