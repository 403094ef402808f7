// crd_arkode.h -- ARKode's step-size controller (CRD_ADAPT_ARKODE) and its per-step bookkeeping, restated from its documentation;
// oracle/arkode_erk.py has the same rules with the same names, and the tests compare the two attempt by attempt.  Host code only,
// shared by the single-context integrator (crd_adaptive.cpp: AdaptiveRun) and the ensemble's (crd_ensemble.cpp), so that
// both take the same decisions from the same norms -- and, at the end, what both keep around the controller: the dense-output record,
// the rotation of the state planes and their relabelling when a call ends.  Not part of the ABI.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>

#include "crd.h"

namespace crd {
namespace arkode {

constexpr double kK1 = 0.58, kK2 = 0.21, kK3 = 0.1;  // ARK_ADAPT_PID gains
constexpr int kEmbeddingOrder = 3;                   // Zonneveld 5(3)4; "pq = 0": the embedding's order enters the exponents
constexpr double kEtamx1 = 10000.0, kEtamxf = 0.3;   // growth bound of the very first step; bound from the second failure of a step on
constexpr int kSmallNef = 2, kMaxNef = 7;
constexpr double kLbound = 1.0, kUbound = 1.5, kOnePsm = 1.000001, kOneMsm = 0.999999;  // no change of h for lbound <= eta <= ubound
constexpr double kTiny = 1.0e-10, kUround = 2.220446049250313e-16;
constexpr double kH0LbFactor = 100.0, kH0UbFactor = 0.1, kH0Bias = 0.5;
constexpr int kH0Iters = 4;

constexpr const char *kTooMuchWork = "adaptive integration: max_steps steps taken before reaching tout (ARK_TOO_MUCH_WORK)";
constexpr const char *kUnderflow = "adaptive integration: step size underflow";
constexpr const char *kErrFailure = "adaptive integration: the error test failed 7 times on one step (ARK_ERR_FAILURE)";

// arkAdapt with the PID method and no explicit-stability function: eta = h_new / h.  e = (this step's biased error, the previous
// accepted step's, the one before that).
// `order`: the embedding's (an int divides the gains exactly as kEmbeddingOrder does: the order-3 call keeps its bits).
inline double pid_eta(double h, const double e[3], double etamax, double safety, double etamin, double h_cap, int order)
{
	const double e1 = std::fmax(e[0], kTiny), e2 = std::fmax(e[1], kTiny), e3 = std::fmax(e[2], kTiny);
	double h_acc = h * std::pow(e1, -kK1 / order) * std::pow(e2, kK2 / order) * std::pow(e3, -kK3 / order);
	h_acc *= safety;
	h_acc = std::fmin(std::fabs(h_acc), std::fabs(etamax * h));
	h_acc = std::fmax(std::fabs(h_acc), std::fabs(etamin * h));
	if (std::fabs(h_acc) > std::fabs(h * kLbound * kOneMsm) && std::fabs(h_acc) < std::fabs(h * kUbound * kOnePsm)) h_acc = h;
	double eta = h_acc / h;
	if (std::isfinite(h_cap)) eta /= std::fmax(1.0, std::fabs(h) * eta / h_cap);  // hmax_inv
	return eta;
}
inline double pid_eta(double h, const double e[3], double etamax, double safety, double etamin, double h_cap) { return pid_eta(h, e, etamax, safety, etamin, h_cap, kEmbeddingOrder); }

// The controller's memory between calls, as ARKodeMem keeps it between ARKode() calls: valid while the resident state is the one the
// integrator left (`live`), dropped by whatever replaces that state.
struct Memory {
	bool live = false;
	int64_t nst = 0;  // steps taken since the state was new
	double tn = 0.0;  // time the integrator has reached
	double h = 0.0, hprime = 0.0, eta = 1.0, etamax = 0.0;
	double ehist[3] = {1.0, 1.0, 1.0};
};

// ARKodeInit on a fresh state at t0, with the user's first step h0 (0: to be estimated -- needs_estimate -- before first_step).
inline void init(Memory &A, double t0, double h0)
{
	A.live = false;
	A.nst = 0;
	A.tn = t0;
	A.eta = 1.0;
	A.etamax = kEtamx1;
	A.ehist[0] = A.ehist[1] = A.ehist[2] = 1.0;
	A.h = h0;
}
inline bool needs_estimate(const Memory &A, double t0, double tout) { return !(A.h > 0.0) && tout > t0; }
inline void first_step(Memory &A, double h_cap)  // (after the estimate, if any)
{
	A.h = std::fmin(A.h, h_cap);
	A.hprime = A.h;
}
// The size of the call's first attempt (crd_adaptive_stats::h_first).
inline double first_attempt(const Memory &A) { return (A.nst > 0 && A.hprime != A.h) ? A.h * A.eta : A.h; }

// Start of a step at time t (arkStep): the step size the controller chose after the previous step, and the two exits before an
// attempt.  nullptr, or the CRD_ESTATE message.
inline const char *begin_step(Memory &A, double t, int64_t steps_this_call, int64_t max_steps)
{
	if (steps_this_call >= max_steps) return kTooMuchWork;
	if (A.nst > 0 && A.hprime != A.h) A.h *= A.eta;
	if (!(A.h > 1e-14 * std::fmax(std::fabs(t), 1e-300)) && !(t == 0.0 && A.h > 0.0)) return kUnderflow;
	return nullptr;
}

// A failed error test (dsm > 1 or NaN) of the step's attempt number *nef: false on the kMaxNef-th failure (ARK_ERR_FAILURE), else
// the smaller step to try next is in A.h.
inline bool reject(Memory &A, double dsm, int *nef, const crd_adaptive_options &o, double h_cap, crd_adaptive_stats &st, int order = kEmbeddingOrder)
{
	++*nef;
	st.rejected++;
	if (*nef == kMaxNef) return false;
	A.etamax = 1.0;  // no growth for the rest of this step, and none after it
	const double e[3] = {std::isfinite(dsm) ? dsm * o.bias : 1e300, A.ehist[0], A.ehist[1]};
	double eta = pid_eta(A.h, e, A.etamax, o.safety, o.shrink, h_cap, order);
	if (*nef >= kSmallNef) eta = std::fmin(eta, kEtamxf);
	A.h *= eta;
	return true;
}

// A passed error test: arkPrepareNextStep / arkCompleteStep.  t advances to the end of the step.
inline void accept(Memory &A, double dsm, const crd_adaptive_options &o, double h_cap, double &t, crd_adaptive_stats &st, int order = kEmbeddingOrder)
{
	A.ehist[2] = A.ehist[1];
	A.ehist[1] = A.ehist[0];
	A.ehist[0] = dsm * o.bias;
	if (A.etamax == 1.0) {  // the step failed its test at least once: keep its size for the next one
		A.hprime = A.h;
		A.eta = 1.0;
	} else {
		A.eta = pid_eta(A.h, A.ehist, A.etamax, o.safety, o.shrink, h_cap, order);
		A.hprime = A.h * A.eta;
	}
	A.etamax = o.growth;
	t += A.h;
	A.tn = t;
	A.nst++;
	st.accepted++;
	st.h_last = A.h;
	st.h_min = (st.h_min == 0.0) ? A.h : std::fmin(st.h_min, A.h);
	st.h_max = std::fmax(st.h_max, A.h);
}

// arkHin: ARKode's estimate of the first step from y'' along a forward Euler trial step -- its scalar side; the vector operations
// (f(t0, y0), the bound, the trial state, f at it, the norm of the difference) are the caller's.  Use: start; the bound max_i |f_i| /
// (0.1 |y_i| + rtol |y_i| + atol) into bound(); then, until done, the WRMS norm of (f(t0 + hg, y0 + hg f0) - f0) / hg into ydd().
struct Hin {
	double tdist = 0.0, hlb = 0.0, hub = 0.0, hg = 0.0, hnew = 0.0, h0 = 0.0;
	bool hnew_ok = false, done = false;
	int count = 0;
};
inline bool hin_start(Hin &H, double t0, double tout)  // false: tout too close to t0 (CRD_EINVAL)
{
	H = Hin{};
	const double tdist = std::fabs(tout - t0), tround = kUround * std::fmax(std::fabs(t0), std::fabs(tout));
	if (tdist < 2.0 * tround) return false;
	H.tdist = tdist;
	H.hlb = kH0LbFactor * tround;
	return true;
}
constexpr const char *kHinTooClose = "adaptive integration: tout too close to t0 to estimate a first step";
inline void hin_bound(Hin &H, double hub_inv)
{
	H.hub = kH0UbFactor * H.tdist;
	if (H.hub * hub_inv > 1.0) H.hub = 1.0 / hub_inv;
	H.hg = std::sqrt(H.hlb * H.hub);
	H.hnew = H.hg;
	if (H.hub < H.hlb) {
		H.h0 = H.hg;
		H.done = true;
	}
}
inline void hin_ydd(Hin &H, double yddnrm)
{
	H.count++;
	if (H.hnew_ok || H.count == kH0Iters) {
		H.hnew = H.hg;
		H.h0 = std::fmin(std::fmax(kH0Bias * H.hnew, H.hlb), H.hub);
		H.done = true;
		return;
	}
	H.hnew = (yddnrm * H.hub * H.hub > 2.0) ? std::sqrt(2.0 / yddnrm) : std::sqrt(H.hg * H.hub);
	const double hrat = H.hnew / H.hg;
	if (hrat > 0.5 && hrat < 2.0) H.hnew_ok = true;
	if (H.count > 1 && hrat > 2.0) {
		H.hnew = H.hg;
		H.hnew_ok = true;
	}
	H.hg = H.hnew;
}

// The checks of crd_integrate_adaptive's options and interval (CRD_EINVAL when they fail).
inline bool options_valid(const crd_adaptive_options &o, double t0, double tout)
{
	return o.rtol >= 0.0 && o.atol >= 0.0 && o.rtol + o.atol > 0.0 && o.safety > 0.0 && o.bias > 0.0 && o.growth >= 1.0 && o.shrink > 0.0 && o.shrink < 1.0 &&
	       o.max_steps >= 1 && o.h0 >= 0.0 && !std::isnan(o.h_max) && std::isfinite(t0) && std::isfinite(tout) && !(tout < t0) &&
	       (o.method == CRD_ADAPT_RK43 || o.method == CRD_ADAPT_ARKODE);
}

// ---- Around the controller: what both error-controlled integrators (RK4(3) too) keep of a trajectory between and during calls ----

// The state planes of a trajectory by role -- a context's plane[role], an ensemble member's role[]: Y the state handed back, SA / SB the
// staged stepper's ping-pong, ACC its accumulator, OUT the third state plane of a dense output.
enum Role { Y = 0, SA = 1, SB = 2, ACC = 3, OUT = 4, NPLANES = 5 };

// Dense output (ARK_NORMAL): after a call that overshot tout, Y holds the interpolant at t_out, SA the integrator's own state y_{n+1}
// at t_np1, OUT y_n at t_n, SB / ACC f(t_n, y_n) / f(t_{n+1}, y_{n+1}).
struct Dense {
	bool pending = false;
	double t_out = 0.0, t_n = 0.0, t_np1 = 0.0;
};
// Whatever replaces the resident state (an upload, a fixed step) drops the finished step and the controller's memory with it.
inline void drop(Dense &d, Memory &A) { d.pending = A.live = false; }
// A call continues the previous one when it starts at the output time that one handed back and nothing has replaced the state since
// (ARKode keeps its memory between ARKode() calls the same way); the ARKode-style controller also needs its own memory.
inline bool resumes(const Dense &d, const Memory &A, double t0, bool arkode_method) { return d.pending && t0 == d.t_out && (!arkode_method || A.live); }
// The cap on the step size: the caller's, the trajectory's own diffusion-stability bound (h_max = 0), or none (h_max < 0).
inline double h_cap(const crd_adaptive_options &o, const crd_params &p) { return o.h_max > 0.0 ? o.h_max : (o.h_max == 0.0 ? crd_stable_dt(&p) : INFINITY); }

// Three state planes -- Y, SA and, with dense output, OUT -- take turns as y_n (prev), y_{n+1} (cur) and the next attempt's target (spare).
struct Rotation {
	int cur = Y, spare = SA, third = OUT, prev = -1;  // a fresh state with dense output; third: a plane nothing has been stepped into yet

	static Rotation fresh(bool dense) { return dense ? Rotation{} : Rotation{Y, SA, -1, -1}; }
	// A resumed call steps on from the integrator's own state; y_n of the finished step and the interpolant handed back are free.
	void resume() { cur = SA, spare = OUT, third = Y; }
	// A resumed call whose tout lies inside the step already taken: that step again (nothing is stepped; the interpolant overwrites Y).
	void reinterpolate() { prev = OUT, cur = SA, spare = Y, third = -1; }
	// An accepted step into dst: the old state becomes y_n (kept for the interpolant), the old y_n / the untouched plane the next target.
	void accept(int dst, bool dense)
	{
		spare = dense ? ahead() : cur;
		if (dense && prev < 0) third = -1;
		if (dense) prev = cur;
		cur = dst;
	}
	int interpolant() const { return Y + SA + OUT - prev - cur; }  // the state plane that is neither y_n nor y_{n+1}
	int ahead() const { return prev >= 0 ? prev : third; }         // where a step after the one being attempted may go before the verdict (-1: nowhere)
};

// A relabelling of a trajectory's planes at the end of a call: role r gets the storage that had role from[r].
struct Relabel {
	int from[NPLANES];
	template <typename T>
	void apply(T (&slot)[NPLANES]) const  // T: a plane's handle(s), trivially copyable (void *, void *[2])
	{
		T old[NPLANES];
		std::memcpy(old, slot, sizeof old);
		for (int r = 0; r < NPLANES; r++) std::memcpy(&slot[r], &old[from[r]], sizeof(T));
	}
};
// The end of a call.  output: the step t_n -> t_np1 (r.prev -> r.cur) has reached or passed tout and the interpolant at tout is in
// r.interpolant() -- Y <- that, SA <- y_{n+1}, OUT <- y_n, and the step is recorded for the next call.  Otherwise (no dense output, a
// zero-length interval, a failure) the state reached is handed back: Y <-> r.cur, nothing to resume.
inline Relabel end_of_call(const Rotation &r, bool output, Dense &d, double tout, double t_n, double t_np1)
{
	if (output) {
		d = Dense{true, tout, t_n, t_np1};
		return Relabel{{r.interpolant(), r.cur, SB, ACC, r.prev}};
	}
	d.pending = false;
	Relabel p{{Y, SA, SB, ACC, OUT}};
	std::swap(p.from[Y], p.from[r.cur]);
	return p;
}

}  // namespace arkode
}  // namespace crd
