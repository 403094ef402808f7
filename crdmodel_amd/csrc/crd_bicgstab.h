// crd_bicgstab.h -- launch interface between crd_bicgstab.cpp (crd_bicgstab_*: the workspace, the order of launches, the entry points)
// and the kernels of crd_bicgstab.hip.  Every vector pointer is a device pointer on the context's device: a whole AoS vector of
// n = 2 nx nyl reals in the context's precision (n is even: the launches refuse an odd one), 16-byte aligned: a thread loads and stores
// 16 bytes at a time.  Scalars are doubles that hold values of the context's precision, passed by value.
// `partials` is kBcgSlots x kBcgBlocks doubles in device memory; `sums` (kBcgSlots doubles) may be page-locked host memory that the
// device can write: the launch that reduces also launches the one wavefront per sum that adds the partials in a fixed order.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace crd {

constexpr int kBcgThreads = 256;  // per block; a thread takes 16 bytes of a vector per grid-stride trip: two fp64 reals, four fp32 reals
constexpr int kBcgBlocks = 2048;  // block cap, as the IMEX stage close: beyond 2048 x 256 = 524288 such units a block takes a second trip
constexpr int kBcgSlots = 2;      // sums one launch leaves at most

inline size_t bcg_units(int precision_is_f64, size_t n) { return precision_is_f64 ? (n + 1) / 2 : (n + 3) / 4; }
inline int bcg_blocks(size_t units)
{
	const size_t b = (units + kBcgThreads - 1) / kBcgThreads;
	return b < (size_t)kBcgBlocks ? (int)(b ? b : 1) : kBcgBlocks;
}

// Start (and the true residual): a = x ? r - fma(-gamma, jv, x) : r;  var0_only: var1 of a is +0;  a -> out0 and, where not null,
// out1 and out2.  sums[0] = ||r||^2 over the whole of r, sums[1] = ||a||^2 of the stored a.
hipError_t launch_bcg_start(int precision, const void *r, const void *x, const void *jv, double gamma, int var0_only, void *out0, void *out1, void *out2, size_t n,
                            double *partials, double *sums, hipStream_t s);
// Apply-dot: out = fma(-gamma, jv, x) IN PLACE over jv (var0_only: var1 of out is +0).  two == 0: sums[0] = <b, out>;
// two == 1: sums[0] = <out, b>, sums[1] = <out, out>.  Reads 3, writes 1.
hipError_t launch_bcg_apply_dot(int precision, void *jv_out, const void *x, const void *b, double gamma, int var0_only, int two, size_t n, double *partials, double *sums,
                                hipStream_t s);
// s-update: s = fma(-alpha, v, res);  sums[0] = ||s||^2 of the stored s.  Reads 2, writes 1.
hipError_t launch_bcg_s_update(int precision, void *s_out, const void *v, const void *res, double alpha, size_t n, double *partials, double *sums, hipStream_t s);
// xr-update: x = fma(omega, shat, fma(alpha, phat, x)) in place;  res = fma(-omega, t, sv);  sums[0] = ||res||^2, sums[1] = <rhat, res>
// of the stored res.  Reads 6, writes 2.  phat, shat may be p, sv (no preconditioner); res is none of the inputs.
hipError_t launch_bcg_xr_update(int precision, void *x, const void *phat, const void *shat, const void *t, const void *sv, const void *rhat, void *res, double alpha,
                                double omega, size_t n, double *partials, double *sums, hipStream_t s);
// p-update: p = fma(beta, fma(-omega, v, p), res) in place.  Reads 3, writes 1.
hipError_t launch_bcg_p_update(int precision, void *p, const void *v, const void *res, double beta, double omega, size_t n, hipStream_t s);
// x-half: x = fma(alpha, phat, x) in place.  Reads 2, writes 1.
hipError_t launch_bcg_x_half(int precision, void *x, const void *phat, double alpha, size_t n, hipStream_t s);

}  // namespace crd
