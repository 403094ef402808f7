// Self-test of crd_imex_tables.h on the host: plain C++17, nothing of HIP (tests/test_imex_host.py builds it with -Wall -Werror, and
// again under ASan + UBSan).  Checks the tableaux' structure -- zero first implicit column (by layout), one diagonal value, row sums
// equal to c, stiff accuracy by construction -- and the coefficient rows a step hands to the stage-close kernel, then prints every
// coefficient as a hexadecimal float so that the Python restatement can be held to the same bits.
#include <cstdio>
#include <cstdlib>

#include "crd_imex_tables.h"

using namespace crd::imex;

#define CHECK(cond)                                                         \
	do {                                                                    \
		if (!(cond)) {                                                      \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			std::exit(1);                                                   \
		}                                                                   \
	} while (0)

static double absd(double x) { return x < 0 ? -x : x; }

int main()
{
	const char *names[3] = {"euler", "ars222", "ars443"};
	const int stages[3] = {1, 2, 4}, orders[3] = {1, 2, 3};
	Tableau T;
	CHECK(!tableau(-1, &T) && !tableau(3, &T));
	for (int scheme = 0; scheme < 3; scheme++) {
		CHECK(tableau(scheme, &T));
		CHECK(T.stages == stages[scheme] && T.order == orders[scheme] && T.stages <= kMaxStages);
		CHECK(T.c[0] == 0.0 && T.c[T.stages] == 1.0);
		for (int i = 1; i <= T.stages; i++) {
			double se = 0.0, si = 0.0;
			for (int j = 0; j < kMaxStages; j++) {
				se += T.AE[i - 1][j];
				si += T.AI[i - 1][j];
				if (j >= i) CHECK(T.AE[i - 1][j] == 0.0 && T.AI[i - 1][j] == 0.0);  // nothing above the diagonal
			}
			CHECK(T.AI[i - 1][i - 1] == T.gamma);  // one diagonal value
			CHECK(absd(se - T.c[i]) <= 4e-16 && absd(si - T.c[i]) <= 4e-16);
		}
		for (int i = T.stages; i < kMaxStages; i++)
			for (int j = 0; j < kMaxStages; j++) CHECK(T.AE[i][j] == 0.0 && T.AI[i][j] == 0.0);
		std::printf("%s %d %d %a\n", names[scheme], T.stages, T.order, T.gamma);
		for (int i = 0; i <= T.stages; i++) std::printf("c %d %a\n", i, T.c[i]);
		for (int i = 1; i <= T.stages; i++)
			for (int j = 0; j < i; j++) std::printf("A %d %d %a %a\n", i, j, T.AE[i - 1][j], T.AI[i - 1][j]);
		// the rows of a step: j ascending, explicit before implicit, no k_0, zeros left out, at most 2 next - 1 terms
		for (int f32 = 0; f32 < 2; f32++)
			for (int next = 1; next <= T.stages; next++) {
				Term terms[2 * kMaxStages];
				const double dt = 0.3;
				const int n = row_terms(T, next, dt, f32 != 0, terms);
				CHECK(n >= 1 && n <= 2 * next - 1);
				for (int q = 0; q < n; q++) {
					CHECK(terms[q].j >= 0 && terms[q].j < next && (terms[q].explicit_part || terms[q].j >= 1) && terms[q].coef != 0.0);
					if (q > 0) CHECK(terms[q].j > terms[q - 1].j || (terms[q].j == terms[q - 1].j && terms[q - 1].explicit_part && !terms[q].explicit_part));
					const double a = terms[q].explicit_part ? T.AE[next - 1][terms[q].j] : T.AI[next - 1][terms[q].j - 1];
					CHECK(terms[q].coef == rounded(dt * a, f32 != 0));
					if (f32) CHECK((double)(float)terms[q].coef == terms[q].coef);
				}
			}
	}
	// a coefficient that rounds to zero is skipped
	CHECK(tableau(kSchemeArs443, &T));
	Term terms[2 * kMaxStages];
	CHECK(row_terms(T, 4, 1e-60, true, terms) == 0 && row_terms(T, 4, 1e-60, false, terms) == 7);
	CHECK(rounded(0.1, false) == 0.1 && rounded(0.1, true) == (double)0.1f);
	std::printf("imex tables selftest ok\n");
	return 0;
}
