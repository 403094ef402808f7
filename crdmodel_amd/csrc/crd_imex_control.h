// crd_imex_control.h -- the step-size control of crd_integrate_imex (include/crd.h): crd_arkode.h's PID controller on the embedding
// order 2 of ARS(4,4,3)'s pair, and the three rules that are this integrator's own -- the first step, the attempts' budget and the last
// step, shortened to land on tout.  Plain C++: nothing of HIP, driven with scripted norms on the host
// (tests/native/imex_control_selftest.cpp); tests/imex_adaptive_reference.py restates it.
//
//   start(t0, tout, h_first, o)    h_first > 0: the caller's h0, or crd_stable_dt.  The first step may grow by arkode::kEtamx1.
//   while (!done())
//       next(&t_n, &h)             the attempt to make, or the CRD_ESTATE message: attempts == max_steps (every attempt counts, a
//                                  rejected one too), or a step size below 1e-14 |t|.
//                                  h = the controller's step, unless t_n + h >= tout or the rest behind it is below 1e-12 |tout|: then
//                                  h = tout - t_n (`clipped`), and the accepted step ends at tout itself.
//       verdict(norm)              norm: the WRMS norm of the estimate, NaN for an attempt that left something not finite.  Passed
//                                  (norm <= 1): 1.  Failed: 0, the next attempt is smaller; -1 on the 7th failure of one step.
//   h_next()                       what the caller passes as the next call's h0: the step the controller would take now -- after a
//                                  clipped last step not less than the step that was clipped, which nothing has spoken against.
#pragma once

#include <cmath>
#include <cstdint>

#include "crd_arkode.h"

namespace crd {
namespace imex {

constexpr int kEmbeddedOrder = 2;

struct Control {
	arkode::Memory A;
	crd_adaptive_options o{};
	crd_adaptive_stats st{};
	double h_cap = INFINITY, t = 0.0, tout = 0.0, wanted = 0.0;
	int64_t attempts = 0;
	int nef = 0;
	bool clipped = false, in_step = false;

	void start(double t0, double tout_, double h_first, const crd_adaptive_options &opt)
	{
		o = opt;
		st = crd_adaptive_stats{};
		h_cap = o.h_max > 0.0 ? o.h_max : INFINITY;
		t = t0;
		tout = tout_;
		attempts = 0;
		in_step = false;
		arkode::init(A, t0, h_first);
		arkode::first_step(A, h_cap);
		st.h_first = wanted = A.h;
		st.t = st.t_internal = t0;
	}
	bool done() const { return !(t < tout); }

	const char *next(double *t_n, double *h)
	{
		if (attempts >= o.max_steps) return arkode::kTooMuchWork;
		if (!in_step) {
			if (const char *why = arkode::begin_step(A, t, 0, 1)) return why;
			in_step = true;
			nef = 0;
		} else if (!(A.h > 1e-14 * std::fmax(std::fabs(t), 1e-300)) && !(t == 0.0 && A.h > 0.0)) {
			return arkode::kUnderflow;
		}
		wanted = A.h;
		clipped = t + A.h >= tout || tout - (t + A.h) < 1e-12 * std::fabs(tout);
		if (clipped) A.h = tout - t;
		if (attempts == 0) st.h_first = A.h;
		attempts++;
		*t_n = t;
		*h = A.h;
		return nullptr;
	}

	int verdict(double norm)
	{
		st.err_last = o.bias * norm;
		if (!(norm <= 1.0)) return arkode::reject(A, norm, &nef, o, h_cap, st, kEmbeddedOrder) ? 0 : -1;
		arkode::accept(A, norm, o, h_cap, t, st, kEmbeddedOrder);
		if (clipped) t = A.tn = tout;
		st.t = st.t_internal = t;
		in_step = false;
		return 1;
	}

	double h_next() const
	{
		if (in_step || A.nst == 0) return std::fmin(A.h, h_cap);  // a call that stopped inside a step, or took none
		return std::fmin(clipped ? std::fmax(wanted, A.hprime) : A.hprime, h_cap);
	}
};

// crd_imex_adaptive_options' controller fields as the crd_adaptive_options arkode::reject / accept read.
inline crd_adaptive_options control_options(double rtol, double atol, double h0, double h_max, double safety, double bias, double growth, double shrink, int64_t max_steps)
{
	crd_adaptive_options o{};
	o.rtol = rtol, o.atol = atol, o.h0 = h0, o.h_max = h_max, o.safety = safety, o.bias = bias, o.growth = growth, o.shrink = shrink, o.max_steps = max_steps;
	o.dense_output = 0;
	o.method = CRD_ADAPT_ARKODE;
	return o;
}

}  // namespace imex
}  // namespace crd
