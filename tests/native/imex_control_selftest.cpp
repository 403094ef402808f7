// Self-test of the error-controlled IMEX integrator's host side: plain C++17, nothing of HIP (tests/test_imex_adaptive_host.py builds it
// with -Wall -Werror, and again under ASan + UBSan, and runs it as a program).
//   1. crd_imex_tables.h: the embedded data of ARS(4,4,3) and estimate_terms -- order, omissions, rounding -- printed as hexadecimal
//      floats so that the Python restatement can be held to the same bits; the three schemes' own rows are untouched
//      (tests/native/imex_tables_selftest.cpp still passes).
//   2. crd_arkode.h: pid_eta with the embedding order 3 against the expression it had before it took an order, bit for bit.
//   3. crd_imex_control.h: scripted norm sequences through the order-2 controller, every attempt printed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "crd_imex_control.h"
#include "crd_imex_tables.h"

using namespace crd;
using namespace crd::imex;

#define CHECK(cond)                                                         \
	do {                                                                    \
		if (!(cond)) {                                                      \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			std::exit(1);                                                   \
		}                                                                   \
	} while (0)

// pid_eta as crd_arkode.h had it, the embedding order a constant
static double pid_eta_before(double h, const double e[3], double etamax, double safety, double etamin, double h_cap)
{
	using namespace crd::arkode;
	constexpr int kOrder = 3;
	const double e1 = std::fmax(e[0], kTiny), e2 = std::fmax(e[1], kTiny), e3 = std::fmax(e[2], kTiny);
	double h_acc = h * std::pow(e1, -kK1 / kOrder) * std::pow(e2, kK2 / kOrder) * std::pow(e3, -kK3 / kOrder);
	h_acc *= safety;
	h_acc = std::fmin(std::fabs(h_acc), std::fabs(etamax * h));
	h_acc = std::fmax(std::fabs(h_acc), std::fabs(etamin * h));
	if (std::fabs(h_acc) > std::fabs(h * kLbound * kOneMsm) && std::fabs(h_acc) < std::fabs(h * kUbound * kOnePsm)) h_acc = h;
	double eta = h_acc / h;
	if (std::isfinite(h_cap)) eta /= std::fmax(1.0, std::fabs(h) * eta / h_cap);
	return eta;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void tables()
{
	Tableau T;
	for (int scheme : {kSchemeEuler, kSchemeArs222}) {
		CHECK(tableau(scheme, &T) && T.embedded_order == 0);
		Term none[kMaxEstimateTerms];
		CHECK(estimate_terms(T, 0.3, false, none) == 0);
	}
	CHECK(tableau(kSchemeArs443, &T) && T.embedded_order == 2 && T.order == 3 && T.stages == 4);
	std::printf("embedded %d\n", T.embedded_order);
	for (int j = 0; j <= T.stages; j++) std::printf("bhat %d %a\n", j, T.bhat[j]);
	for (int j = 0; j <= T.stages; j++) std::printf("dE %d %a\n", j, T.dE[j]);
	for (int j = 1; j <= T.stages; j++) std::printf("dI %d %a\n", j, T.dI[j - 1]);
	// d = b - bhat on both parts, exactly (b: the last rows)
	for (int j = 0; j <= T.stages; j++) CHECK(T.dE[j] == (j < T.stages ? T.AE[T.stages - 1][j] : 0.0) - T.bhat[j]);
	for (int j = 1; j <= T.stages; j++) CHECK(T.dI[j - 1] == T.AI[T.stages - 1][j - 1] - T.bhat[j]);
	CHECK(T.bhat[T.stages] == 0.0 && T.dE[T.stages] == 0.0);  // no FR_4
	const double dts[3] = {0.3, 0.0125, 1e-60};
	for (int f32 = 0; f32 < 2; f32++)
		for (double dt : dts) {
			Term terms[kMaxEstimateTerms];
			const int n = estimate_terms(T, dt, f32 != 0, terms);
			CHECK(n <= kMaxEstimateTerms);
			std::printf("terms %d %a %d\n", f32, dt, n);
			for (int q = 0; q < n; q++) {
				const Term &m = terms[q];
				CHECK(m.coef != 0.0 && m.j >= 0 && m.j <= T.stages && (m.explicit_part || m.j >= 1));
				if (q > 0) CHECK(m.j > terms[q - 1].j || (m.j == terms[q - 1].j && terms[q - 1].explicit_part && !m.explicit_part));
				CHECK(m.coef == rounded(dt * (m.explicit_part ? T.dE[m.j] : T.dI[m.j - 1]), f32 != 0));
				if (f32) CHECK((double)(float)m.coef == m.coef);
				std::printf("term %d %c %a\n", m.j, m.explicit_part ? 'E' : 'I', m.coef);
			}
			// FR_0, FR_1, k_1, FR_2, k_2, FR_3, k_3, k_4; in fp32 1e-60 rounds every coefficient to zero
			CHECK(n == (f32 && dt == 1e-60 ? 0 : 8));
			if (n == 8) CHECK(terms[0].j == 0 && terms[0].explicit_part && terms[7].j == 4 && !terms[7].explicit_part && terms[2].j == 1 && !terms[2].explicit_part);
		}
}

static void order_three_keeps_its_bits()
{
	const double hs[3] = {1e-3, 0.37, 41.0}, errs[6] = {0.0, 1e-12, 0.02, 0.7, 1.6, 1e300}, caps[2] = {INFINITY, 0.5};
	const double etamaxes[3] = {1.0, 20.0, 10000.0};
	int n = 0;
	for (double h : hs)
		for (double a : errs)
			for (double b : errs)
				for (double c : errs)
					for (double cap : caps)
						for (double etamax : etamaxes) {
							const double e[3] = {a, b, c};
							const double before = pid_eta_before(h, e, etamax, 0.96, 0.1, cap);
							CHECK(same_bits(arkode::pid_eta(h, e, etamax, 0.96, 0.1, cap), before));
							CHECK(same_bits(arkode::pid_eta(h, e, etamax, 0.96, 0.1, cap, arkode::kEmbeddingOrder), before));
							n++;
						}
	// and through reject / accept with their default order
	crd_adaptive_options o = control_options(1e-4, 1e-6, 0.0, 0.0, 0.96, 1.5, 20.0, 0.1, 100);
	crd_adaptive_stats s3{}, s3b{};
	arkode::Memory A, B;
	arkode::init(A, 0.0, 0.01), arkode::init(B, 0.0, 0.01);
	arkode::first_step(A, INFINITY), arkode::first_step(B, INFINITY);
	double ta = 0.0, tb = 0.0;
	int nefa = 0, nefb = 0;
	CHECK(arkode::reject(A, 3.0, &nefa, o, INFINITY, s3) && arkode::reject(B, 3.0, &nefb, o, INFINITY, s3b, 3) && same_bits(A.h, B.h));
	arkode::accept(A, 0.2, o, INFINITY, ta, s3), arkode::accept(B, 0.2, o, INFINITY, tb, s3b, 3);
	CHECK(same_bits(A.hprime, B.hprime) && same_bits(ta, tb));
	std::printf("order3 %d identical\n", n);
}

// One scripted run: norms[k] answers attempt k; ends when the controller is done, refuses, or the script runs out.
static void scenario(const char *name, double t0, double tout, double h_first, double h_max, double growth, long long max_steps, const double *norms, int n_norms)
{
	Control K;
	K.start(t0, tout, h_first, control_options(1e-4, 1e-6, h_first, h_max, 0.96, 1.5, growth, 0.1, max_steps));
	std::printf("scenario %s %a %a %a %a %a %lld\n", name, t0, tout, h_first, h_max, growth, max_steps);
	const char *why = "script";
	int k = 0;
	while (!K.done() && k < n_norms) {
		double t = 0.0, h = 0.0;
		if (const char *stop = K.next(&t, &h)) {
			why = stop;
			break;
		}
		const int verdict = K.verdict(norms[k]);
		std::printf("attempt %a %a %a %d\n", t, h, norms[k], verdict);
		k++;
		if (verdict < 0) {
			why = arkode::kErrFailure;
			break;
		}
	}
	if (K.done()) why = "done";
	std::printf("end %a %a %lld %lld %lld %s\n", K.t, K.h_next(), (long long)K.st.accepted, (long long)K.st.rejected, (long long)K.attempts, why);
}

int main()
{
	tables();
	order_three_keeps_its_bits();
	const double accept[] = {0.3, 0.05, 0.6, 0.9, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2};
	scenario("accept", 0.0, 2.0, 1e-3, 0.0, 20.0, 1000, accept, 12);
	const double reject[] = {2.5, 0.4, 0.1, 0.1};
	scenario("reject", 0.5, 0.9, 0.2, 0.0, 20.0, 1000, reject, 4);
	const double second[] = {4.0, 1.2, 0.8, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3};
	scenario("second_failure", 0.0, 1.0, 0.25, 0.0, 20.0, 1000, second, 10);
	const double seventh[] = {0.5, 9.0, 9.0, NAN, 9.0, 1.01, 9.0, 9.0, 0.1};
	scenario("seventh_failure", 0.0, 10.0, 0.5, 0.0, 20.0, 1000, seventh, 9);
	const double growth[] = {1e-9, 1e-9, 1e-9, 1e-9, 1e-9, 1e-9};
	scenario("growth_cap", 0.0, 1e9, 1e-3, 0.0, 20.0, 1000, growth, 6);
	scenario("h_max", 0.0, 100.0, 1e-3, 0.75, 20.0, 1000, growth, 6);
	const double last[] = {0.5, 0.5, 0.5, 0.5};
	scenario("shortened_last_step", 1.0, 1.35, 0.1, 0.0, 20.0, 1000, last, 4);
	scenario("stretched_last_step", 0.0, 0.2 + 1e-14, 0.1, 0.0, 1.0, 1000, last, 4);
	scenario("one_exact_step", 0.25, 0.375, 0.125, 0.0, 20.0, 1000, last, 4);
	const double budget[] = {3.0, 0.5, 0.5};
	scenario("max_steps_1", 0.0, 1.0, 0.5, 0.0, 20.0, 1, budget, 3);
	scenario("no_interval", 3.0, 3.0, 0.5, 0.0, 20.0, 10, budget, 2);
	std::printf("imex control selftest ok\n");
	return 0;
}
