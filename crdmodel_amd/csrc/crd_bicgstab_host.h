// crd_bicgstab_host.h -- the host's share of crd_bicgstab_* (crd_bicgstab.cpp): the scalar recurrences of BiCGStab, the breakdown and
// exit decisions, and the rounding of the coefficients.  The device hands over reductions (doubles); this forms alpha, omega and beta
// in double, rounds each ONCE to the vectors' precision, and says after every reduction whether the next kernel may be launched.
// Plain C++17, nothing of HIP: tests/native/bicgstab_host_selftest.cpp exercises it on the CPU.
//
//   start(||res_0||^2)           rho = <rhat, res_0> = ||res_0||^2;  not finite: stop, converged = 0;  ||res_0|| <= tol: stop, converged
//   take_d(d)                    d zero or not finite, or alpha = rho / d zero or not finite once rounded: breakdown kD (the
//                                iteration does not count: x is untouched)
//   take_s(||s||^2)              ||s|| <= tol: the half exit -- the caller applies x = fma(alpha, phat, x); the iteration counts
//   take_t(<t, s>, <t, t>)       <t, t> zero or not finite: kTT;  omega = <t, s> / <t, t> zero or not finite once rounded: kOmega.
//                                Either way the caller applies the half update first (s is its residual): half_exit, the iteration counts
//   take_res(||res||^2, rho')    the iteration counts;  ||res|| <= tol: converged;  else max_iters reached: stop;  else rho' zero or
//                                not finite, or beta = (rho' / rho) (alpha / omega) not finite once rounded: kRho;  else rho = rho'
// Every take_* returns true when the iteration goes on to the kernel that uses the scalar it has just formed.
#pragma once

#include <cmath>

namespace crd {
namespace bicgstab {

enum Breakdown { kNone = 0, kD = 1, kTT = 2, kOmega = 3, kRho = 4 };

// the value of the vectors' precision nearest x, as a double
inline double rounded(double x, bool f32) { return f32 ? (double)(float)x : x; }
inline bool usable(double x) { return std::isfinite(x) && x != 0.0; }

struct Recurrence {
	bool f32 = false;
	double tol = 0.0;
	int max_iters = 1;
	double rho = 0.0, alpha = 0.0, omega = 0.0, beta = 0.0, res_norm = 0.0;
	int iterations = 0, half_exit = 0, breakdown = kNone, converged = 0;

	bool start(double res_sq)
	{
		rho = res_sq;
		res_norm = std::sqrt(res_sq);
		if (!std::isfinite(res_sq)) return false;
		if (res_norm <= tol) {
			converged = 1;
			return false;
		}
		return max_iters > 0;
	}

	bool take_d(double d)
	{
		if (usable(d)) alpha = rounded(rho / d, f32);
		if (!usable(d) || !usable(alpha)) {
			breakdown = kD;
			return false;
		}
		return true;
	}

	// true: go on to shat = M s;  false: the half exit
	bool take_s(double s_sq)
	{
		res_norm = std::sqrt(s_sq);
		if (res_norm <= tol) {
			converged = 1;
			half_exit = 1;
			iterations++;
			return false;
		}
		return true;
	}

	bool take_t(double ts, double tt)
	{
		if (!usable(tt)) breakdown = kTT;
		else {
			omega = rounded(ts / tt, f32);
			if (!usable(omega)) breakdown = kOmega;
		}
		if (breakdown != kNone) {
			half_exit = 1;
			iterations++;
			return false;
		}
		return true;
	}

	bool take_res(double res_sq, double rho_new)
	{
		iterations++;
		res_norm = std::sqrt(res_sq);
		if (res_norm <= tol) {
			converged = 1;
			return false;
		}
		if (iterations >= max_iters) return false;
		if (usable(rho_new)) beta = rounded((rho_new / rho) * (alpha / omega), f32);
		if (!usable(rho_new) || !std::isfinite(beta)) {
			breakdown = kRho;
			return false;
		}
		rho = rho_new;
		return true;
	}
};

}  // namespace bicgstab
}  // namespace crd
