// bicgstab_host_selftest.cpp -- crd_bicgstab_host.h on the CPU: the scalar recurrences of crd_bicgstab_* driven through scripted
// sequences of reductions -- a normal run, a half exit, each breakdown, scalars that are not finite, max_iters -- with the decisions and
// coefficients checked here and printed as hexadecimal floats, so that tests/test_bicgstab_host.py can hold its Python restatement to
// the same bits.  Plain C++17, nothing of HIP: g++ -std=c++17 -Wall -Werror -I crdmodel_amd/csrc, once more with
// -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "crd_bicgstab_host.h"

using namespace crd::bicgstab;

namespace {

int failures = 0;

void expect(bool ok, const char *what, int line)
{
	if (ok) return;
	std::printf("FAIL line %d: %s\n", line, what);
	failures++;
}
#define EXPECT(x) expect((x), #x, __LINE__)

// one reduction handed over: 's'tart, 'd', 'n' (||s||^2), 't' (<t, s>, <t, t>), 'r' (||res||^2, rho')
struct Op {
	char kind;
	double a, b;
};

// Runs the script until a step says stop (or the script ends); prints every step and the state behind it.
Recurrence run(const char *name, bool f32, double tol, int max_iters, const std::vector<Op> &ops)
{
	Recurrence k;
	k.f32 = f32;
	k.tol = tol;
	k.max_iters = max_iters;
	std::printf("script %s %d %a %d\n", name, f32 ? 1 : 0, tol, max_iters);
	for (const Op &op : ops) {
		bool go = false;
		switch (op.kind) {
		case 's': go = k.start(op.a); break;
		case 'd': go = k.take_d(op.a); break;
		case 'n': go = k.take_s(op.a); break;
		case 't': go = k.take_t(op.a, op.b); break;
		default: go = k.take_res(op.a, op.b); break;
		}
		std::printf("op %c %a %a -> %d %a %a %a %a %a %d %d %d %d\n", op.kind, op.a, op.b, go ? 1 : 0, k.rho, k.alpha, k.omega, k.beta, k.res_norm, k.iterations, k.half_exit,
		            k.breakdown, k.converged);
		if (!go) break;
	}
	return k;
}

const double kInf = std::numeric_limits<double>::infinity();
const double kNaN = std::numeric_limits<double>::quiet_NaN();

void test_scripts()
{
	// two full iterations, converged at the end of the second
	Recurrence k = run("normal", false, 1e-3, 10, {{'s', 4.0, 0}, {'d', 8.0, 0}, {'n', 1.0, 0}, {'t', 0.5, 2.0}, {'r', 0.25, 0.3}, {'d', 0.7, 0}, {'n', 0.01, 0},
	                                                {'t', 0.004, 0.008}, {'r', 1e-8, 1e-5}});
	EXPECT(k.converged == 1 && k.iterations == 2 && k.half_exit == 0 && k.breakdown == kNone);
	EXPECT(k.omega == 0.5 && k.res_norm == 1e-4);
	EXPECT(k.beta == (0.3 / 4.0) * (0.5 / 0.25));  // of the first iteration: alpha = 4 / 8, omega = 0.5 / 2
	// the same reductions in fp32: every coefficient is a float's value
	k = run("normal_f32", true, 1e-3, 10, {{'s', 4.0, 0}, {'d', 7.0, 0}, {'n', 1.0, 0}, {'t', 0.3, 1.1}, {'r', 0.25, 0.3}, {'d', 0.7, 0}});
	EXPECT(k.alpha == (double)(float)k.alpha && k.omega == (double)(float)k.omega && k.beta == (double)(float)k.beta);
	EXPECT(k.omega == (double)(float)(0.3 / 1.1) && k.alpha == (double)(float)(0.3 / 0.7));
	// converged before the first iteration; a start that is not finite
	k = run("start_converged", false, 3.0, 10, {{'s', 4.0, 0}, {'d', 1.0, 0}});
	EXPECT(k.converged == 1 && k.iterations == 0 && k.res_norm == 2.0);
	k = run("start_nan", false, 3.0, 10, {{'s', kNaN, 0}, {'d', 1.0, 0}});
	EXPECT(k.converged == 0 && k.iterations == 0 && k.breakdown == kNone);
	k = run("start_inf", false, 3.0, 10, {{'s', kInf, 0}, {'d', 1.0, 0}});
	EXPECT(k.converged == 0 && k.iterations == 0);
	// half exit in the first iteration
	k = run("half_exit", false, 0.5, 10, {{'s', 4.0, 0}, {'d', 8.0, 0}, {'n', 0.04, 0}, {'t', 1.0, 1.0}});
	EXPECT(k.converged == 1 && k.iterations == 1 && k.half_exit == 1 && k.breakdown == kNone && k.alpha == 0.5 && k.res_norm == 0.2);
	// each breakdown
	k = run("breakdown_d_zero", false, 1e-3, 10, {{'s', 4.0, 0}, {'d', 0.0, 0}, {'n', 1.0, 0}});
	EXPECT(k.breakdown == kD && k.iterations == 0 && k.converged == 0 && k.half_exit == 0 && k.alpha == 0.0);
	k = run("breakdown_d_nan", false, 1e-3, 10, {{'s', 4.0, 0}, {'d', kNaN, 0}, {'n', 1.0, 0}});
	EXPECT(k.breakdown == kD && k.iterations == 0);
	k = run("breakdown_alpha_overflow", false, 1e-3, 10, {{'s', 1e300, 0}, {'d', 1e-300, 0}, {'n', 1.0, 0}});
	EXPECT(k.breakdown == kD && k.iterations == 0);
	k = run("breakdown_alpha_underflow_f32", true, 0.0, 10, {{'s', 1e-30, 0}, {'d', 1e30, 0}, {'n', 1.0, 0}});
	EXPECT(k.breakdown == kD && k.alpha == 0.0);
	k = run("breakdown_tt", false, 1e-3, 10, {{'s', 4.0, 0}, {'d', 8.0, 0}, {'n', 1.0, 0}, {'t', 0.5, 0.0}, {'r', 1.0, 1.0}});
	EXPECT(k.breakdown == kTT && k.iterations == 1 && k.half_exit == 1 && k.converged == 0 && k.res_norm == 1.0);
	k = run("breakdown_tt_inf", false, 1e-3, 10, {{'s', 4.0, 0}, {'d', 8.0, 0}, {'n', 1.0, 0}, {'t', 0.5, kInf}, {'r', 1.0, 1.0}});
	EXPECT(k.breakdown == kTT);
	k = run("breakdown_omega_zero", false, 1e-3, 10, {{'s', 4.0, 0}, {'d', 8.0, 0}, {'n', 1.0, 0}, {'t', 0.0, 2.0}, {'r', 1.0, 1.0}});
	EXPECT(k.breakdown == kOmega && k.iterations == 1 && k.half_exit == 1 && k.omega == 0.0);
	k = run("breakdown_omega_nan", false, 1e-3, 10, {{'s', 4.0, 0}, {'d', 8.0, 0}, {'n', 1.0, 0}, {'t', kNaN, 2.0}, {'r', 1.0, 1.0}});
	EXPECT(k.breakdown == kOmega);
	k = run("breakdown_rho_zero", false, 1e-3, 10, {{'s', 4.0, 0}, {'d', 8.0, 0}, {'n', 1.0, 0}, {'t', 0.5, 2.0}, {'r', 0.25, 0.0}, {'d', 1.0, 0}});
	EXPECT(k.breakdown == kRho && k.iterations == 1 && k.half_exit == 0 && k.converged == 0 && k.rho == 4.0);
	k = run("breakdown_rho_nan", false, 1e-3, 10, {{'s', 4.0, 0}, {'d', 8.0, 0}, {'n', 1.0, 0}, {'t', 0.5, 2.0}, {'r', 0.25, kNaN}, {'d', 1.0, 0}});
	EXPECT(k.breakdown == kRho);
	k = run("breakdown_beta_overflow", false, 0.0, 10, {{'s', 1e-200, 0}, {'d', 1e-200, 0}, {'n', 1.0, 0}, {'t', 1e-150, 1.0}, {'r', 0.25, 1e200}, {'d', 1.0, 0}});
	EXPECT(k.breakdown == kRho);
	// a residual that is not a number neither converges nor loops: the next scalar ends it
	k = run("nan_residual", false, 1e-3, 10, {{'s', 4.0, 0}, {'d', 8.0, 0}, {'n', kNaN, 0}, {'t', kNaN, kNaN}});
	EXPECT(k.breakdown == kTT && k.converged == 0 && k.iterations == 1);
	// convergence at the full step wins over a rho' that would be a breakdown; max_iters wins over it too
	k = run("converged_despite_rho", false, 1.0, 10, {{'s', 4.0, 0}, {'d', 8.0, 0}, {'n', 2.0, 0}, {'t', 0.5, 2.0}, {'r', 0.25, 0.0}});
	EXPECT(k.converged == 1 && k.breakdown == kNone && k.iterations == 1);
	k = run("max_iters", false, 1e-6, 2, {{'s', 4.0, 0}, {'d', 8.0, 0}, {'n', 1.0, 0}, {'t', 0.5, 2.0}, {'r', 0.25, 0.3}, {'d', 0.7, 0}, {'n', 0.01, 0}, {'t', 0.004, 0.008},
	                                      {'r', 1e-4, 0.0}, {'d', 1.0, 0}});
	EXPECT(k.converged == 0 && k.iterations == 2 && k.breakdown == kNone && k.half_exit == 0);
	k = run("max_iters_one", false, 1e-6, 1, {{'s', 4.0, 0}, {'d', 8.0, 0}, {'n', 1.0, 0}, {'t', 0.5, 2.0}, {'r', 0.25, 0.3}, {'d', 0.7, 0}});
	EXPECT(k.iterations == 1 && k.converged == 0);
}

void test_rounding()
{
	EXPECT(rounded(0.1, false) == 0.1 && rounded(0.1, true) == (double)0.1f);
	EXPECT(usable(1.0) && usable(-1e-300) && !usable(0.0) && !usable(-0.0) && !usable(kInf) && !usable(kNaN));
	EXPECT(rounded(1e-60, true) == 0.0 && std::isinf(rounded(1e60, true)));
}

}  // namespace

int main()
{
	test_scripts();
	test_rounding();
	if (failures) {
		std::printf("bicgstab host selftest: %d failure(s)\n", failures);
		return 1;
	}
	std::printf("bicgstab host selftest ok\n");
	return 0;
}
