// crd_imex_tables.h -- the built-in IMEX additive Runge-Kutta schemes of crd_step_imex (include/crd.h), and the coefficient rows a
// step hands to the stage-close kernel (crd_imex.h).  Plain C++: nothing of HIP, self-tested on the host
// (tests/native/imex_tables_selftest.cpp).
//
// All three are of the Ascher-Ruuth-Spiteri type (Appl. Numer. Math. 25, 1997): s implicit stages behind the explicit stage 0,
//   Y_0 = y_n,   Y_i = y_n + dt sum_{j<i} A^E_ij f_R(Y_j) + dt sum_{1<=j<=i} A^I_ij f_D(Y_j),   i = 1 .. s,   y_{n+1} = Y_s,
// the first column of the implicit matrix zero, ONE diagonal value gamma, stiffly accurate (b = the last row, of both matrices), c shared.
// Rows are stored by stage i = 1 .. s at index i - 1: AE[i - 1][j] for j = 0 .. i - 1, AI[i - 1][j - 1] for j = 1 .. i; the rest is zero.
#pragma once

#include <cmath>

namespace crd {
namespace imex {

constexpr int kSchemeEuler = 0, kSchemeArs222 = 1, kSchemeArs443 = 2;  // CRD_IMEX_EULER / _ARS222 / _ARS443
constexpr int kMaxStages = 4;

struct Tableau {
	int stages = 0, order = 0;
	double gamma = 0.0;
	double c[kMaxStages + 1] = {};
	double AE[kMaxStages][kMaxStages] = {};  // [i - 1][j], j = 0 .. i - 1
	double AI[kMaxStages][kMaxStages] = {};  // [i - 1][j - 1], j = 1 .. i
};

inline bool tableau(int scheme, Tableau *out)
{
	Tableau T;
	if (scheme == kSchemeEuler) {
		T.stages = 1, T.order = 1, T.gamma = 1.0;
		T.c[1] = 1.0;
		T.AE[0][0] = 1.0;
		T.AI[0][0] = 1.0;
	} else if (scheme == kSchemeArs222) {
		const double g = 1.0 - 1.0 / std::sqrt(2.0), d = 1.0 - 1.0 / (2.0 * g);
		T.stages = 2, T.order = 2, T.gamma = g;
		T.c[1] = g, T.c[2] = 1.0;
		T.AE[0][0] = g;
		T.AE[1][0] = d, T.AE[1][1] = 1.0 - d;
		T.AI[0][0] = g;
		T.AI[1][0] = 1.0 - g, T.AI[1][1] = g;
	} else if (scheme == kSchemeArs443) {
		T.stages = 4, T.order = 3, T.gamma = 0.5;
		T.c[1] = 0.5, T.c[2] = 2.0 / 3.0, T.c[3] = 0.5, T.c[4] = 1.0;
		T.AE[0][0] = 0.5;
		T.AE[1][0] = 11.0 / 18.0, T.AE[1][1] = 1.0 / 18.0;
		T.AE[2][0] = 5.0 / 6.0, T.AE[2][1] = -5.0 / 6.0, T.AE[2][2] = 0.5;
		T.AE[3][0] = 0.25, T.AE[3][1] = 1.75, T.AE[3][2] = 0.75, T.AE[3][3] = -1.75;
		T.AI[0][0] = 0.5;
		T.AI[1][0] = 1.0 / 6.0, T.AI[1][1] = 0.5;
		T.AI[2][0] = -0.5, T.AI[2][1] = 0.5, T.AI[2][2] = 0.5;
		T.AI[3][0] = 1.5, T.AI[3][1] = -1.5, T.AI[3][2] = 0.5, T.AI[3][3] = 0.5;
	} else {
		return false;
	}
	*out = T;
	return true;
}

// A coefficient as the kernels use it: formed in double, rounded once to the context's precision.
inline double rounded(double x, bool f32) { return f32 ? (double)(float)x : x; }

// One term of R_{i+1} = y_n + sum: coefficient x (FR_j when `explicit_part`, else k_j).
struct Term {
	int j;
	bool explicit_part;
	double coef;
};

// The terms of R_{next}, next = 1 .. s, in the order the kernel adds them: j ascending, at each j the explicit term and then the
// implicit one; terms whose rounded coefficient is exactly zero are left out.  Returns their number (at most 2 next - 1).
inline int row_terms(const Tableau &T, int next, double dt, bool f32, Term *out)
{
	int n = 0;
	for (int j = 0; j < next; j++) {
		const double e = rounded(dt * T.AE[next - 1][j], f32);
		if (e != 0.0) out[n++] = Term{j, true, e};
		if (j == 0) continue;
		const double i = rounded(dt * T.AI[next - 1][j - 1], f32);
		if (i != 0.0) out[n++] = Term{j, false, i};
	}
	return n;
}

}  // namespace imex
}  // namespace crd
