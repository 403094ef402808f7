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

}  // namespace crd
