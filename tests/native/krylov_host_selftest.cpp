// krylov_host_selftest.cpp -- crd_krylov_host.h on the CPU: the Givens rotations and the back substitution of crd_lsolve_*'s small
// least-squares problem against Hessenberg matrices whose solutions are known, a breakdown column, restart = 1 and the bounds of a
// cycle.  Plain C++17, nothing of HIP: g++ -std=c++17 -Wall -Werror -I crdmodel_amd/csrc, once more with -fsanitize=address,undefined
// (tests/test_krylov_host.py).
#include <cmath>
#include <cstdio>
#include <vector>

#include "crd_krylov_host.h"

using crd::krylov::LeastSquares;

namespace {

int failures = 0;

void expect(bool ok, const char *what, int line)
{
	if (ok) return;
	std::printf("FAIL line %d: %s\n", line, what);
	failures++;
}
#define EXPECT(x) expect((x), #x, __LINE__)

bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }

// || beta e_1 - H y ||_2 for the (k + 1) x k Hessenberg H given column by column (column j: j + 2 entries)
double residual_of(const std::vector<std::vector<double>> &H, double beta, const std::vector<double> &y)
{
	const size_t k = H.size();
	std::vector<double> r(k + 1, 0.0);
	r[0] = beta;
	for (size_t j = 0; j < k; j++)
		for (size_t i = 0; i < H[j].size(); i++) r[i] -= H[j][i] * y[j];
	double s = 0.0;
	for (double x : r) s += x * x;
	return std::sqrt(s);
}

void test_one_column()
{
	// min || 5 e_1 - (3, 4)^T y ||: y = 15 / 25, residual 5 * 4 / 5 = 4
	LeastSquares ls;
	ls.start(4, 5.0);
	const double h[2] = {3.0, 4.0};
	EXPECT(ls.push(h, 0x1p-53));
	EXPECT(ls.columns() == 1 && !ls.breakdown() && !ls.full());
	EXPECT(near(ls.residual(), 4.0, 1e-15));
	double y[1];
	ls.solve(y);
	EXPECT(near(y[0], 0.6, 1e-15));
}

void test_known_solution()
{
	// H = [[2, 1, 0.5], [1, 3, 1], [0, 2, 1], [0, 0, 0.5]], beta = 3: the normal equations' solution, and the estimate equals the residual
	const std::vector<std::vector<double>> H = {{2.0, 1.0}, {1.0, 3.0, 2.0}, {0.5, 1.0, 1.0, 0.5}};
	LeastSquares ls;
	ls.start(3, 3.0);
	std::vector<double> estimates;
	for (const auto &col : H) {
		EXPECT(ls.push(col.data(), 0x1p-53));
		estimates.push_back(ls.residual());
	}
	EXPECT(ls.full() && ls.columns() == 3 && !ls.breakdown());
	EXPECT(estimates[0] >= estimates[1] && estimates[1] >= estimates[2]);  // the residual of a growing space cannot grow
	std::vector<double> y(3);
	ls.solve(y.data());
	EXPECT(near(residual_of(H, 3.0, y), ls.residual(), 1e-14));
	// H^T (beta e_1 - H y) = 0
	std::vector<double> r(4, 0.0);
	r[0] = 3.0;
	for (size_t j = 0; j < 3; j++)
		for (size_t i = 0; i < H[j].size(); i++) r[i] -= H[j][i] * y[j];
	for (size_t j = 0; j < 3; j++) {
		double g = 0.0;
		for (size_t i = 0; i < H[j].size(); i++) g += H[j][i] * r[i];
		EXPECT(near(g, 0.0, 1e-13));
	}
	// a perturbed y is worse
	for (size_t j = 0; j < 3; j++) {
		std::vector<double> q = y;
		q[j] += 1e-3;
		EXPECT(residual_of(H, 3.0, q) > ls.residual());
	}
	// a column pushed into a full cycle is refused and changes nothing
	const double extra[5] = {1, 1, 1, 1, 1};
	EXPECT(!ls.push(extra, 0x1p-53) && ls.columns() == 3);
}

void test_square_system_is_solved()
{
	// last subdiagonal entry tiny but above the breakdown bound: no breakdown, residual tiny
	LeastSquares ls;
	ls.start(2, 1.0);
	const double c0[2] = {1.0, 1.0}, c1[3] = {1.0, -1.0, 1e-9};
	EXPECT(ls.push(c0, 0x1p-53) && ls.push(c1, 0x1p-53));
	EXPECT(!ls.breakdown());
	double y[2];
	ls.solve(y);
	EXPECT(near(y[0], 0.5, 1e-8) && near(y[1], 0.5, 1e-8));
	EXPECT(ls.residual() < 1e-8);
}

void test_breakdown()
{
	// A v_0 = 2 v_0: the column is (2, 0): final, residual 0, y = beta / 2, nothing divided by the zero
	LeastSquares ls;
	ls.start(30, 7.0);
	const double h[2] = {2.0, 0.0};
	EXPECT(ls.push(h, 0x1p-53));
	EXPECT(ls.breakdown() && ls.full() && ls.columns() == 1);
	EXPECT(ls.residual() == 0.0);
	double y[1];
	ls.solve(y);
	EXPECT(y[0] == 3.5 && std::isfinite(y[0]));
	// a norm of rounding size counts as zero, in the second column too; one a little above does not
	ls.start(30, 1.0);
	const double a0[2] = {1.0, 1.0}, a1[3] = {1.0, 2.0, 2.0 * 0x1p-53};
	EXPECT(ls.push(a0, 0x1p-53) && !ls.breakdown());
	EXPECT(ls.push(a1, 0x1p-53) && ls.breakdown() && ls.residual() == 0.0);
	double y2[2];
	ls.solve(y2);
	EXPECT(std::isfinite(y2[0]) && std::isfinite(y2[1]));
	// (1, 1; 1, 2) y = (1, 0) rotated: y = (2, -1) solves H y = e_1 on its first two rows
	EXPECT(near(y2[0], 2.0, 1e-14) && near(y2[1], -1.0, 1e-14));
	ls.start(30, 1.0);
	const double b0[2] = {1.0, 8.0 * 0x1p-53};
	EXPECT(ls.push(b0, 0x1p-53) && !ls.breakdown());
	// the bound scales with the precision's unit roundoff
	ls.start(30, 1.0);
	const double f0[2] = {1.0, 1e-8};
	EXPECT(ls.push(f0, 0x1p-24) && ls.breakdown());
	// a singular pivot met by a breakdown: the unknown is 0, not a quotient by zero
	ls.start(4, 1.0);
	const double z0[2] = {0.0, 0.0};
	EXPECT(ls.push(z0, 0x1p-53) && ls.breakdown());
	double y3[1];
	ls.solve(y3);
	EXPECT(y3[0] == 0.0);
	// a column that is not a number ends the cycle as a breakdown does: every loop stays bounded
	ls.start(4, 1.0);
	const double n0[2] = {1.0, std::nan("")};
	EXPECT(ls.push(n0, 0x1p-53) && ls.full());
}

void test_restart_one()
{
	LeastSquares ls;
	ls.start(1, 2.0);
	EXPECT(!ls.full() && ls.columns() == 0 && ls.residual() == 2.0);
	const double h[2] = {4.0, 3.0};
	EXPECT(ls.push(h, 0x1p-53));
	EXPECT(ls.full() && !ls.breakdown());
	EXPECT(near(ls.residual(), 2.0 * 3.0 / 5.0, 1e-15));
	double y[1];
	ls.solve(y);
	EXPECT(near(y[0], 2.0 * 4.0 / 25.0, 1e-15));
	EXPECT(!ls.push(h, 0x1p-53));
	// restart outside 1 .. 64 is clamped: the arrays never grow beyond the header's bound
	ls.start(0, 1.0);
	EXPECT(ls.push(h, 0x1p-53) && ls.full());
	ls.start(1000, 1.0);
	int pushed = 0;
	std::vector<double> col(crd::krylov::kMaxRestart + 2, 0.0);
	for (int j = 0; j < 200 && !ls.full(); j++) {
		for (int i = 0; i <= j + 1; i++) col[(size_t)i] = 1.0 / (1.0 + i + j);
		col[(size_t)j + 1] = 1.0;
		if (ls.push(col.data(), 0x1p-53)) pushed++;
	}
	EXPECT(pushed == crd::krylov::kMaxRestart && ls.full());
	std::vector<double> y64((size_t)crd::krylov::kMaxRestart);
	ls.solve(y64.data());
	for (double v : y64) EXPECT(std::isfinite(v));
}

}  // namespace

int main()
{
	test_one_column();
	test_known_solution();
	test_square_system_is_solved();
	test_breakdown();
	test_restart_one();
	if (failures) {
		std::printf("krylov host selftest: %d failure(s)\n", failures);
		return 1;
	}
	std::printf("krylov host selftest ok\n");
	return 0;
}
