// crd_imex.h -- launch interface between crd_imex.cpp (crd_step_imex: the IMEX stepper, its workspace and its order of launches) and
// the stage-close kernel of crd_imex.hip.  Every pointer is a device pointer on the context's device; vectors are whole AoS vectors
// of 2 nx nyl reals in the context's precision.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "crd_kernels.h"

namespace crd {

constexpr int kImexThreads = 256;  // per block; a thread takes 16 bytes of a vector per grid-stride trip: one fp64 point, two fp32 points
constexpr int kImexBlocks = 2048;  // block cap: beyond 2048 x 256 = 524288 such units a block takes a second trip
constexpr int kImexMaxTerms = 6;   // stored vectors in one R_{i+1} besides y_n: FR_0 .. FR_{i-1}, k_1 .. k_{i-1}, i <= 3

// One stage close (stage i of a step, 0 <= i <= s), by value to the kernel.
//   Y   = k ? fma(hg, k, R) : R                                  (stage 0: k == nullptr, R is y_n itself)
//   last:  Y -> out; the partials of max |var0 of Y| -> partials, their maximum -> *max_out.  Nothing else.
//   else:  F = f_R(Y) with the held rows of `absorb` -> FR
//          acc = y_n; acc = fma(coef[t], term[t], acc) for t = 0 .. nterms - 1; then fma(cE, F, acc) unless cE == 0; then
//          fma(cI, k, acc) unless k == nullptr or cI == 0;  acc -> Rnext
// Rnext may be R, out may be R: a thread reads its own elements of every input before it writes any.  Coefficients are doubles that
// hold values of the context's precision.
struct ImexClose {
	const void *R = nullptr, *k = nullptr, *yn = nullptr;
	void *FR = nullptr, *Rnext = nullptr, *out = nullptr;
	double hg = 0.0, cE = 0.0, cI = 0.0;
	int nterms = 0, last = 0, absorb = 0;
	const void *term[kImexMaxTerms] = {};
	double coef[kImexMaxTerms] = {};
	double *partials = nullptr;  // kImexBlocks doubles (last stage)
	double *max_out = nullptr;   // device-visible double (last stage)
};

hipError_t launch_imex_close(int precision, const SlabDesc &d, const ImexClose &a, hipStream_t s);

constexpr int kImexEstimateTerms = 7;  // stored vectors of one error estimate: FR_0 .. FR_3, k_1 .. k_3 of ARS(4,4,3); k_4 comes from its register

// The last stage close of an error-controlled step (crd_integrate_imex), by value to its kernel: the last close above and, in the
// same pass, the estimate e of the embedded pair and the sum of its weighted squares.
//   Y   = fma(hg, k, R) -> out; the partials of max |var0 of Y| -> max_partials, their maximum -> result[0]: ImexClose's last close.
//   e   = coef[0] term[0], one rounded product; then e = fma(coef[t], term[t], e) for t = 1 .. nterms - 1; then e = fma(ck, k, e)
//         unless ck == 0 (the k that formed Y, from its register); all in the context's precision.  (nterms == 0: e = ck k.)
//         -> e_out when e_out is given.
//   q   = r r, r = (double)e / w, w = rtol |(double)y_n| + atol: a product, a sum, a quotient and a product in double, each rounded
//         once, none contracted.  Every real of the vector counts, var0 and var1.
//   sum of q: a thread's chain acc = acc + q over the reals of its unit in order and over its trips, then the tree of
//         crd_bicgstab.hip -- six shuffle steps, the block's four wavefronts in order, one partial per block -> sum_partials, one
//         wavefront over the blocks in a fixed order -> result[1].  No atomics: the bits repeat.
// out may be R.  out and e_out may be none of the vectors read besides R.
struct ImexEstimate {
	const void *R = nullptr, *k = nullptr, *yn = nullptr;
	void *out = nullptr, *e_out = nullptr;
	double hg = 0.0, ck = 0.0, rtol = 0.0, atol = 0.0;
	int nterms = 0;
	const void *term[kImexEstimateTerms] = {};
	double coef[kImexEstimateTerms] = {};
	double *max_partials = nullptr, *sum_partials = nullptr;  // kImexBlocks doubles each
	double *result = nullptr;                                 // two device-visible doubles: max |var0|, sum of q
};

hipError_t launch_imex_estimate(int precision, const SlabDesc &d, const ImexEstimate &a, hipStream_t s);

}  // namespace crd
