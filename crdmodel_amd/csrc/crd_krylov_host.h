// crd_krylov_host.h -- the host's share of crd_lsolve_* (crd_krylov.cpp): the small least-squares problem of restarted GMRES.  The
// device hands over one Hessenberg column per inner iteration (j + 2 doubles); this keeps the triangular factor, the Givens rotations
// and the rotated right-hand side, says when a column is a breakdown, and solves for the cycle's coefficients.  Plain C++17, nothing
// of HIP: tests/native/krylov_host_selftest.cpp exercises it on the CPU.
//
//   min_y || beta e_1 - H y ||,  H (k + 1) x k upper Hessenberg, column j arriving as h[0 .. j + 1].
//   Rotation j turns (R[j][j], h[j + 1]) into (r, 0): r = hypot(a, b), c = a / r, s = b / r;  g[j + 1] = -s g[j], g[j] = c g[j].
//   |g[k]| is the residual norm of the system after k columns (right preconditioning: of the system itself).
//   Breakdown: h[j + 1] <= 2 unit ||h[0 .. j + 1]||_2.  The column's norm stands for ||A M v_j|| (Pythagoras: the orthogonalisation
//   splits that vector into the column's entries), so no further reduction is asked of the device.  The column is then final: its
//   last entry counts as zero, no rotation is formed, nothing is divided by it, the residual estimate is zero.
#pragma once

#include <cmath>
#include <vector>

namespace crd {
namespace krylov {

constexpr int kMaxRestart = 64;

class LeastSquares {
public:
	// a cycle of at most `restart` columns (1 .. kMaxRestart) from a residual of norm beta
	void start(int restart, double beta)
	{
		m_ = restart < 1 ? 1 : (restart > kMaxRestart ? kMaxRestart : restart);
		k_ = 0;
		breakdown_ = false;
		R_.assign((size_t)m_ * (size_t)m_, 0.0);
		c_.assign((size_t)m_, 1.0);
		s_.assign((size_t)m_, 0.0);
		g_.assign((size_t)m_ + 1, 0.0);
		g_[0] = beta;
	}

	int columns() const { return k_; }
	bool full() const { return k_ >= m_ || breakdown_; }
	bool breakdown() const { return breakdown_; }
	double residual() const { return std::fabs(g_[(size_t)k_]); }

	// Column k = columns(): h[0 .. k + 1], the last entry the norm the next basis vector would be divided by.  `unit`: the unit
	// roundoff of the vectors' precision.  Returns false when the cycle is full already (the column is ignored).
	bool push(const double *h, double unit)
	{
		if (full()) return false;
		const int k = k_;
		double sq = 0.0;
		for (int i = 0; i <= k + 1; i++) sq += h[i] * h[i];
		const double next = h[k + 1];
		breakdown_ = !(next > 2.0 * unit * std::sqrt(sq));
		double *col = &R_[(size_t)k * (size_t)m_];
		for (int i = 0; i <= k; i++) col[i] = h[i];
		for (int i = 0; i < k; i++) {  // the rotations so far
			const double a = col[i], b = col[i + 1];
			col[i] = c_[(size_t)i] * a + s_[(size_t)i] * b;
			col[i + 1] = -s_[(size_t)i] * a + c_[(size_t)i] * b;
		}
		if (breakdown_) {
			g_[(size_t)k + 1] = 0.0;
		} else {
			const double a = col[k], r = std::hypot(a, next);
			c_[(size_t)k] = a / r;
			s_[(size_t)k] = next / r;
			col[k] = r;
			g_[(size_t)k + 1] = -s_[(size_t)k] * g_[(size_t)k];
			g_[(size_t)k] = c_[(size_t)k] * g_[(size_t)k];
		}
		k_ = k + 1;
		return true;
	}

	// y[0 .. columns()): R y = g by back substitution.  A zero pivot (a singular system met by a breakdown) gives that unknown 0.
	void solve(double *y) const
	{
		for (int i = k_ - 1; i >= 0; i--) {
			double a = g_[(size_t)i];
			for (int j = i + 1; j < k_; j++) a -= R_[(size_t)j * (size_t)m_ + (size_t)i] * y[j];
			const double d = R_[(size_t)i * (size_t)m_ + (size_t)i];
			y[i] = d != 0.0 ? a / d : 0.0;
		}
	}

private:
	int m_ = 1, k_ = 0;
	bool breakdown_ = false;
	std::vector<double> R_, c_, s_, g_;  // R column by column, m_ entries each
};

}  // namespace krylov
}  // namespace crd
