// crd_step.h -- what the host forms for one Runge-Kutta step before it launches it: the step sizes the kernels take, the stage times and
// the absorbing-row flags.  Host code only and no HIP include, shared by every stepper of contexts and of ensembles (.cpp and .hip units
// alike): a member of an ensemble goes through a lone context's arithmetic bit by bit, and on the host that is these expressions and
// no others.  The step's own time is the caller's (t0 + s dt, (t + dt) + ..., ((t + dt) + dt) + ...): those forms differ by roundings
// the steppers rely on (crd_schedule.h: pair_is_exact).  Not part of the ABI.
#pragma once

namespace crd {
namespace step {

// dt, dt/2, dt/3, dt/6 in double -- these expressions, not dt * (1.0 / 3.0) -- and rounded to fp32 (what the fp32 kernels take).
struct Sizes {
	double h[4];
	float hf[4];
	explicit Sizes(double dt) : h{dt, 0.5 * dt, dt / 3.0, dt / 6.0}, hf{(float)h[0], (float)h[1], (float)h[2], (float)h[3]} {}
};

// Stage times are t + c_k h: classical RK4's four (Zonneveld 5(3)4 shares them), then Zonneveld's fifth stage.
constexpr double kStageC[5] = {0.0, 0.5, 0.5, 1.0, 0.75};
inline double stage_time(double t, double h, int k) { return t + kStageC[k] * h; }

// The absorbing rows are on at a stage exactly while its time lies before tBoundary: strict <, src/FHNmodel_torus.cpp:643.
inline bool absorbing_at(double t_stage, double t_boundary) { return t_stage < t_boundary; }

// The flags of the first n (4 or 5) stages of a step of size h at t; true when any of them is set.
inline bool stage_flags(double t, double h, double t_boundary, int n, int *flags)
{
	bool any = false;
	for (int k = 0; k < n; k++) any = (flags[k] = absorbing_at(stage_time(t, h, k), t_boundary) ? 1 : 0) || any;
	return any;
}

}  // namespace step
}  // namespace crd
