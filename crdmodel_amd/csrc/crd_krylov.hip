// crd_krylov.hip -- the vector kernels of restarted GMRES for (I - gamma J) z = r (crd_lsolve_*, include/crd.h): the orthogonalisation
// of one new Krylov vector w against the basis V_0 .. V_j, classical Gram-Schmidt applied twice, and the few whole-vector operations
// around it.  All templated on Real, all on whole AoS vectors of n reals, one thread per element per grid-stride trip.
//
//   crd_kr_dots_kernel     multi-dot: <V_i, w> for a group of up to kKrylovGroup = 8 basis vectors in ONE pass over w -- w is read once
//                          per group, every V_i once.  Eight double accumulators per thread (the width is what the registers carry
//                          without scratch: profiles/krylov/kernel_resources.txt); products of floats are exact in double.  At most
//                          kKrylovBlocks = 512 blocks each leave one partial per vector: the thread's chain over its grid-stride trips,
//                          the wavefront's six shuffle steps, the block's four wavefronts added in order.
//   crd_kr_sum_kernel      sums the partials of each vector in a fixed order (one wavefront per vector: a chain over every 64th
//                          block, six shuffle steps) into device memory, and adds the result to the Hessenberg column's entry.
//   crd_kr_update_kernel   multi-axpy with fused norm: w <- w - sum_i h[i] V_i for ALL i <= j in one pass, h read from device memory
//                          (into LDS), a double chain per element rounded once to Real; the same pass leaves the per-block partials
//                          of ||w||^2 of the stored values.
//   crd_kr_scale_kernel    V_{j+1} = w / ||w||, the squared norm read from device memory.
//   crd_kr_combine_kernel  x = sum_i y[i] V_i, y read from device memory.
//   crd_kr_apply_kernel    u - gamma (J u) and r - (z - gamma (J z)) around the J v of crd_jacobian.hip; crd_kr_add_kernel  z += M x.
// No atomics, no scratch, no cooperative launch, and no kernel waits on anything: every result is one fixed sequence of operations
// on fixed inputs, so the bits repeat from run to run.
//
// Traffic of one inner iteration j (c = j + 1 basis vectors), in vector crossings counted from the loops below: a multi-dot reads
// c + ceil(c / 8) vectors, an update reads c + 1 and writes 1; Gram-Schmidt twice is 2 (2 c + ceil(c / 8) + 2) = 4 (j + 2) +
// 2 ceil((j + 1) / 8) crossings -- 46 at j = 9, 132 at j = 29 -- where separate dots and axpys take 2 (2 c + 3 c) = 10 (j + 1).
// Around it: apply 3, scale 2 (in place).
#include <hip/hip_runtime.h>

#include "crd_device.h"
#include "crd_krylov.h"

namespace crd {

namespace {

using namespace dev;

constexpr int kWaves = kKrylovThreads / 64;

// sum over the wavefront into lane 0: six steps, the same pairs every time
__device__ __forceinline__ double wave_sum(double a)
{
	for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
	return a;
}

template <typename Real, int W, bool FULL>
__device__ __forceinline__ void dots_trips(const Real *__restrict__ V, size_t stride, int count, const Real *__restrict__ w, size_t n, double (&acc)[W])
{
	const size_t step = (size_t)gridDim.x * kKrylovThreads;
	for (size_t q = (size_t)blockIdx.x * kKrylovThreads + threadIdx.x; q < n; q += step) {
		const double wq = (double)w[q];
#pragma unroll
		for (int i = 0; i < W; i++)
			if (FULL || i < count) acc[i] = __builtin_fma((double)V[(size_t)i * stride + q], wq, acc[i]);
	}
}

// partials[i * kKrylovBlocks + block] = the block's share of <V_i, w>, i < count <= W
template <typename Real, int W>
__global__ void __launch_bounds__(kKrylovThreads) crd_kr_dots_kernel(const Real *__restrict__ V, size_t stride, int count, const Real *__restrict__ w, size_t n,
                                                                     double *__restrict__ partials)
{
	__shared__ double part[W][kWaves];
	double acc[W];
#pragma unroll
	for (int i = 0; i < W; i++) acc[i] = 0.0;
	if (count == W) dots_trips<Real, W, true>(V, stride, count, w, n, acc);
	else dots_trips<Real, W, false>(V, stride, count, w, n, acc);
#pragma unroll
	for (int i = 0; i < W; i++) {
		const double a = wave_sum(acc[i]);
		if ((threadIdx.x & 63) == 0) part[i][threadIdx.x >> 6] = a;
	}
	__syncthreads();
	const int i = (int)threadIdx.x;
	if (i < W && i < count) partials[(size_t)i * kKrylovBlocks + blockIdx.x] = ((part[i][0] + part[i][1]) + part[i][2]) + part[i][3];
}

// One wavefront per vector: cur[i] = the sum of its `blocks` partials, sum[i] (+)= cur[i].
__global__ void __launch_bounds__(64) crd_kr_sum_kernel(const double *__restrict__ partials, int blocks, double *__restrict__ cur, double *__restrict__ sum, int accumulate)
{
	const int i = (int)blockIdx.x;
	double a = 0.0;
	for (int b = (int)threadIdx.x; b < blocks; b += 64) a += partials[(size_t)i * kKrylovBlocks + b];
	a = wave_sum(a);
	if (threadIdx.x == 0) {
		if (cur) cur[i] = a;
		if (sum) sum[i] = accumulate ? sum[i] + a : a;
	}
}

template <typename Real>
__global__ void __launch_bounds__(kKrylovThreads) crd_kr_update_kernel(const Real *__restrict__ V, size_t stride, int count, Real *__restrict__ w, size_t n,
                                                                       const double *__restrict__ h, double *__restrict__ partials)
{
	__shared__ double hs[kKrylovMaxBasis];
	__shared__ double part[kWaves];
	if ((int)threadIdx.x < count) hs[threadIdx.x] = -h[threadIdx.x];
	__syncthreads();
	double sum = 0.0;
	const size_t step = (size_t)gridDim.x * kKrylovThreads;
	for (size_t q = (size_t)blockIdx.x * kKrylovThreads + threadIdx.x; q < n; q += step) {
		double a = (double)w[q];
#pragma unroll 4
		for (int i = 0; i < count; i++) a = __builtin_fma(hs[i], (double)V[(size_t)i * stride + q], a);
		const Real o = (Real)a;
		w[q] = o;
		sum = __builtin_fma((double)o, (double)o, sum);
	}
	sum = wave_sum(sum);
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
	__syncthreads();
	if (threadIdx.x == 0) partials[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

template <typename Real>
__global__ void __launch_bounds__(kKrylovThreads) crd_kr_scale_kernel(const Real *w, Real *out, size_t n, const double *__restrict__ norm2, int var0_only)
{
	const double norm = sqrt(*norm2);
	const size_t step = (size_t)gridDim.x * kKrylovThreads;
	for (size_t q = (size_t)blockIdx.x * kKrylovThreads + threadIdx.x; q < n; q += step) out[q] = (var0_only && (q & 1)) ? (Real)0 : (Real)((double)w[q] / norm);
}

template <typename Real>
__global__ void __launch_bounds__(kKrylovThreads) crd_kr_combine_kernel(const Real *__restrict__ V, size_t stride, int count, const double *__restrict__ y, Real *__restrict__ x,
                                                                        size_t n)
{
	__shared__ double ys[kKrylovMaxBasis];
	if ((int)threadIdx.x < count) ys[threadIdx.x] = y[threadIdx.x];
	__syncthreads();
	const size_t step = (size_t)gridDim.x * kKrylovThreads;
	for (size_t q = (size_t)blockIdx.x * kKrylovThreads + threadIdx.x; q < n; q += step) {
		double a = 0.0;
#pragma unroll 4
		for (int i = 0; i < count; i++) a = __builtin_fma(ys[i], (double)V[(size_t)i * stride + q], a);
		x[q] = (Real)a;
	}
}

template <typename Real>
__global__ void __launch_bounds__(kKrylovThreads) crd_kr_apply_kernel(Real *out, const Real *x, const Real *jv, const Real *r, Real gamma, int var0_only, size_t n)
{
	const size_t step = (size_t)gridDim.x * kKrylovThreads;
	for (size_t q = (size_t)blockIdx.x * kKrylovThreads + threadIdx.x; q < n; q += step) {
		Real a = jv ? fmadd(-gamma, jv[q], x[q]) : x[q];
		if (r) a = r[q] - a;
		out[q] = (var0_only && (q & 1)) ? (Real)0 : a;
	}
}

template <typename Real>
__global__ void __launch_bounds__(kKrylovThreads) crd_kr_add_kernel(Real *z, const Real *d, const Real *var1_from, size_t n)
{
	const size_t step = (size_t)gridDim.x * kKrylovThreads;
	for (size_t q = (size_t)blockIdx.x * kKrylovThreads + threadIdx.x; q < n; q += step) {
		if (var1_from && (q & 1)) z[q] = var1_from[q];
		else if (d) z[q] = z[q] + d[q];
	}
}

// blocks of the whole-vector kernels that reduce nothing: enough to fill the device, grid-stride beyond
int stream_blocks(size_t n)
{
	const size_t b = (n + kKrylovThreads - 1) / kKrylovThreads;
	return b < 4096 ? (int)(b ? b : 1) : 4096;
}

template <typename Real>
hipError_t dots_t(const void *V, size_t stride, int count, const void *w, size_t n, double *partials, double *h_cur, double *h_sum, int accumulate, hipStream_t s)
{
	const int blocks = krylov_blocks(n);
	for (int first = 0; first < count; first += kKrylovGroup) {
		const int c = count - first < kKrylovGroup ? count - first : kKrylovGroup;
		crd_kr_dots_kernel<Real, kKrylovGroup><<<blocks, kKrylovThreads, 0, s>>>(static_cast<const Real *>(V) + (size_t)first * stride, stride, c, static_cast<const Real *>(w), n,
		                                                                         partials + (size_t)first * kKrylovBlocks);
	}
	crd_kr_sum_kernel<<<count, 64, 0, s>>>(partials, blocks, h_cur, h_sum, accumulate);
	return launch_status();
}

}  // namespace

hipError_t launch_kr_dots(int precision, const void *V, size_t stride, int count, const void *w, size_t n, double *partials, double *h_cur, double *h_sum, int accumulate,
                          hipStream_t s)
{
	if (count < 1 || count > kKrylovMaxBasis) return hipErrorInvalidValue;
	clear_launch_status();
	return precision == CRD_PRECISION_F64 ? dots_t<double>(V, stride, count, w, n, partials, h_cur, h_sum, accumulate, s)
	                                      : dots_t<float>(V, stride, count, w, n, partials, h_cur, h_sum, accumulate, s);
}

hipError_t launch_kr_update(int precision, const void *V, size_t stride, int count, void *w, size_t n, const double *h, double *partials, double *norm2, hipStream_t s)
{
	if (count < 1 || count > kKrylovMaxBasis) return hipErrorInvalidValue;
	clear_launch_status();
	const int blocks = krylov_blocks(n);
	if (precision == CRD_PRECISION_F64)
		crd_kr_update_kernel<double><<<blocks, kKrylovThreads, 0, s>>>(static_cast<const double *>(V), stride, count, static_cast<double *>(w), n, h, partials);
	else crd_kr_update_kernel<float><<<blocks, kKrylovThreads, 0, s>>>(static_cast<const float *>(V), stride, count, static_cast<float *>(w), n, h, partials);
	crd_kr_sum_kernel<<<1, 64, 0, s>>>(partials, blocks, nullptr, norm2, 0);
	return launch_status();
}

hipError_t launch_kr_scale(int precision, const void *w, void *out, size_t n, const double *norm2, int var0_only, hipStream_t s)
{
	clear_launch_status();
	if (precision == CRD_PRECISION_F64) crd_kr_scale_kernel<double><<<stream_blocks(n), kKrylovThreads, 0, s>>>(static_cast<const double *>(w), static_cast<double *>(out), n, norm2, var0_only);
	else crd_kr_scale_kernel<float><<<stream_blocks(n), kKrylovThreads, 0, s>>>(static_cast<const float *>(w), static_cast<float *>(out), n, norm2, var0_only);
	return launch_status();
}

hipError_t launch_kr_combine(int precision, const void *V, size_t stride, int count, const double *y, void *x, size_t n, hipStream_t s)
{
	if (count < 1 || count >= kKrylovMaxBasis) return hipErrorInvalidValue;
	clear_launch_status();
	if (precision == CRD_PRECISION_F64) crd_kr_combine_kernel<double><<<stream_blocks(n), kKrylovThreads, 0, s>>>(static_cast<const double *>(V), stride, count, y, static_cast<double *>(x), n);
	else crd_kr_combine_kernel<float><<<stream_blocks(n), kKrylovThreads, 0, s>>>(static_cast<const float *>(V), stride, count, y, static_cast<float *>(x), n);
	return launch_status();
}

hipError_t launch_kr_apply(int precision, void *out, const void *x, const void *jv, const void *r, double gamma, int var0_only, size_t n, hipStream_t s)
{
	clear_launch_status();
	if (precision == CRD_PRECISION_F64)
		crd_kr_apply_kernel<double><<<stream_blocks(n), kKrylovThreads, 0, s>>>(static_cast<double *>(out), static_cast<const double *>(x), static_cast<const double *>(jv),
		                                                                       static_cast<const double *>(r), gamma, var0_only, n);
	else
		crd_kr_apply_kernel<float><<<stream_blocks(n), kKrylovThreads, 0, s>>>(static_cast<float *>(out), static_cast<const float *>(x), static_cast<const float *>(jv),
		                                                                      static_cast<const float *>(r), (float)gamma, var0_only, n);
	return launch_status();
}

hipError_t launch_kr_add(int precision, void *z, const void *d, const void *var1_from, size_t n, hipStream_t s)
{
	clear_launch_status();
	if (precision == CRD_PRECISION_F64)
		crd_kr_add_kernel<double><<<stream_blocks(n), kKrylovThreads, 0, s>>>(static_cast<double *>(z), static_cast<const double *>(d), static_cast<const double *>(var1_from), n);
	else crd_kr_add_kernel<float><<<stream_blocks(n), kKrylovThreads, 0, s>>>(static_cast<float *>(z), static_cast<const float *>(d), static_cast<const float *>(var1_from), n);
	return launch_status();
}

}  // namespace crd
