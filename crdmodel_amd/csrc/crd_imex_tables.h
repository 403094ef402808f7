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
	// The embedded solution yhat = y_n + dt sum_j bhat_j (FR_j + k_j), ONE weight vector for both parts (embedded_order 0: the scheme
	// has none), and the error estimate's rows e = y_{n+1} - yhat = dt sum_j dE_j FR_j + dt sum_j dI_j k_j, d = b - bhat per part.
	int embedded_order = 0;
	double bhat[kMaxStages + 1] = {};  // [j], j = 0 .. s
	double dE[kMaxStages + 1] = {};    // [j], j = 0 .. s
	double dI[kMaxStages] = {};        // [j - 1], j = 1 .. s
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
		// order 2 (sum bhat = 1, bhat.c = 1/2; both matrices have row sums c), not 3 (bhat.c^2 = 1/4), damped at infinity
		// (1 - bhat_I^T A_I^-1 e = 0); bhat_4 = 0, so FR_4 is never formed.  Every entry is exact in binary.
		T.embedded_order = 2;
		T.bhat[1] = 2.5, T.bhat[3] = -1.5;
		T.dE[0] = 0.25, T.dE[1] = -0.75, T.dE[2] = 0.75, T.dE[3] = -0.25;
		T.dI[0] = -1.0, T.dI[1] = -1.5, T.dI[2] = 2.0, T.dI[3] = 0.5;
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

// The terms of the error estimate e = sum coefficient x (FR_j or k_j), in the order the kernel adds them: as row_terms -- j ascending
// over 0 .. s, at each j the explicit term and then the implicit one, each coefficient dt d formed in double and rounded once; terms
// whose rounded coefficient is exactly zero are left out.  Returns their number (at most kMaxEstimateTerms); 0 for a scheme without
// an embedded solution.
constexpr int kMaxEstimateTerms = 2 * kMaxStages + 1;
inline int estimate_terms(const Tableau &T, double dt, bool f32, Term *out)
{
	int n = 0;
	if (T.embedded_order == 0) return n;
	for (int j = 0; j <= T.stages; j++) {
		const double e = rounded(dt * T.dE[j], f32);
		if (e != 0.0) out[n++] = Term{j, true, e};
		if (j == 0) continue;
		const double i = rounded(dt * T.dI[j - 1], f32);
		if (i != 0.0) out[n++] = Term{j, false, i};
	}
	return n;
}

}  // namespace imex
}  // namespace crd
