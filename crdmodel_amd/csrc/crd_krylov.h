// crd_krylov.h -- launch interface between crd_krylov.cpp (crd_lsolve_*: restarted GMRES, its workspace and its order of launches)
// and the kernels of crd_krylov.hip.  Every pointer is a device pointer on the context's device.  Vectors are whole AoS vectors of
// n = 2 nx nyl reals in the context's precision; a basis is an array of such vectors `stride` reals apart; every scalar the kernels
// read or leave (coefficients, partial sums, norms) is a double in device memory.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace crd {

constexpr int kKrylovThreads = 256;  // per block
constexpr int kKrylovBlocks = 512;   // the reductions' block cap: a vector beyond 512 x 256 = 131072 reals takes a second grid-stride trip
constexpr int kKrylovGroup = 8;      // basis vectors per pass of the multi-dot over w
constexpr int kKrylovMaxBasis = 65;  // restart <= 64: V[0 .. 64]

inline int krylov_blocks(size_t n)
{
	const size_t b = (n + kKrylovThreads - 1) / kKrylovThreads;
	return b < (size_t)kKrylovBlocks ? (int)(b ? b : 1) : kKrylovBlocks;
}

// Multi-dot: h_cur[i] = <V_i, w>, i < count <= kKrylovMaxBasis, and h_sum[i] = (accumulate ? h_sum[i] : 0) + h_cur[i] (h_sum may be
// null).  ceil(count / kKrylovGroup) passes over w, each reading its group's vectors once; per-block partials (partials: count x
// kKrylovBlocks doubles), then one launch that sums them in a fixed order.
hipError_t launch_kr_dots(int precision, const void *V, size_t stride, int count, const void *w, size_t n, double *partials, double *h_cur, double *h_sum, int accumulate,
                          hipStream_t s);
// Multi-axpy with fused norm: w <- w - sum_i h[i] V_i in one pass, *norm2 = ||w||^2 of the stored w (partials: kKrylovBlocks doubles).
hipError_t launch_kr_update(int precision, const void *V, size_t stride, int count, void *w, size_t n, const double *h, double *partials, double *norm2, hipStream_t s);
// Scale: out = w / sqrt(*norm2) (out may be w); var0_only: var1 of out is +0.
hipError_t launch_kr_scale(int precision, const void *w, void *out, size_t n, const double *norm2, int var0_only, hipStream_t s);
// Combine: x = sum_i y[i] V_i, i < count <= kKrylovMaxBasis - 1.
hipError_t launch_kr_combine(int precision, const void *V, size_t stride, int count, const double *y, void *x, size_t n, hipStream_t s);
// The operator's own arithmetic around J v: a = jv ? fma(-gamma, jv, x) : x;  out = r ? r - a : a;  var0_only: var1 of out is +0.
hipError_t launch_kr_apply(int precision, void *out, const void *x, const void *jv, const void *r, double gamma, int var0_only, size_t n, hipStream_t s);
// z += d (d may be null); var1_from: var1 of z is var1 of that vector instead.
hipError_t launch_kr_add(int precision, void *z, const void *d, const void *var1_from, size_t n, hipStream_t s);

}  // namespace crd
