// crd_multigrid.hip -- the kernels of one geometric multigrid V-cycle for P = I - gamma J_D(t) on var0 (crd_psolve_*, include/crd.h).
//
// Three kernels, each templated on Real, each on var0-only planes of a level (ny rows of nx reals, periodic in theta and in phi):
//   crd_mg_sweep_kernel     one damped Jacobi sweep.  The geometry of crd_rhs_part_aos_kernel (crd_jacobian.hip): one thread per
//                           point, 64 x 4 blocks on 64 x 16 tiles dealt to the XCDs in runs, z and its one-point halo ring in LDS
//                           (18 x 66), theta wrap by index arithmetic, phi wrap by row index.  On level 0 its first form reads var0
//                           straight from the caller's AoS r (from z = 0 the sweep is (omega / d) r: no tile) and leaves r as a plane
//                           for the kernels behind it; its last form writes the caller's AoS z, var1 copied from r.
//   crd_mg_restrict_kernel  residual and full weighting in one: a block forms the residual r - A z of the 17 x 65 fine points around
//                           its 8 x 32 coarse points in LDS (z with two rings, 19 x 67, staged first) and weights it; the residual
//                           never reaches memory.
//   crd_mg_prolong_kernel   z += bilinear prolongation of the coarse correction, held rows left alone; in place, pointwise in z, the
//                           coarse plane (a quarter of the points) read through the caches.
// No atomics, no reductions: a point's result is one fixed sequence of operations on fixed inputs, so the bits repeat from run to
// run.  Contraction is off (crd_device.h) and every multiply-add is spelled with fmadd.  Every width works: a tile's columns beyond
// nx are masked, the neighbours of column 0 and nx - 1 are fetched by index, so the coarse levels' 17, 6 or 4 columns are one
// ragged tile.
//
// Traffic of a default cycle on level 0, reals per point: first sweep 2 (AoS r) + 1 (z) + 1 (r plane); second 3 (z, r in, z out);
// restrict 2 + 1/4; prolong 2 + 1/4; third sweep 3; last 1 (z) + 2 (AoS r) + 2 (AoS z): 19.5, and about a third more for the
// coarse levels together.
#include <hip/hip_runtime.h>

#include "crd_device.h"
#include "crd_multigrid.h"

namespace crd {

namespace {

using namespace dev;

constexpr int kTX = 64;          // tile width = one wavefront along theta
constexpr int kBY = 4;           // waves per block
constexpr int kRPT = 4;          // rows per thread
constexpr int kTY = kBY * kRPT;  // tile height
constexpr int kCX = 32, kCY = 8;                        // coarse points per block of the restriction: 256
constexpr int kSR = 2 * kCY + 1, kSC = 2 * kCX + 1;     // the fine residuals they weight
constexpr int kZR = kSR + 2, kZC = kSC + 2;             // ... and the z those read

template <typename Real>
struct Level {
	const Real *cE, *cWn, *cP;
	Real cX2, gamma, omega;
	int nx, ny, held_lo, held_hi;
};

template <typename Real>
Level<Real> typed_level(const MgLevel &m, double gamma, double omega)
{
	Level<Real> l;
	l.cE = static_cast<const Real *>(m.cE);
	l.cWn = static_cast<const Real *>(m.cWn);
	l.cP = static_cast<const Real *>(m.cP);
	l.cX2 = (Real)m.cX2;
	l.gamma = (Real)gamma;
	l.omega = (Real)omega;
	l.nx = m.nx;
	l.ny = m.ny;
	l.held_lo = m.held_lo;
	l.held_hi = m.held_hi;
	return l;
}

template <typename Real>
__device__ __forceinline__ bool held_row(const Level<Real> &l, int j)
{
	return (l.held_lo && j == 0) || (l.held_hi && j == l.ny - 1);
}

// c in [-n, 2 n) into [0, n)
__device__ __forceinline__ int wrap_index(int c, int n) { return c < 0 ? c + n : (c >= n ? c - n : c); }

// (A z) at a point: z - gamma L z with L's chain of rhs_point_diffusion (crd_jacobian.h); a held row of A is the identity's.
template <typename Real>
__device__ __forceinline__ Real apply_point(const Level<Real> &l, Real uC, Real uW, Real uE, Real uS, Real uN, Real cE, Real cWn, Real cP, bool held)
{
	const Real d2y = fmadd((Real)-2.0, uC, uN) + uS;
	const Real lz = fmadd(cWn, uC - uW, fmadd(cE, uE - uC, cP * d2y));
	return held ? uC : fmadd(-l.gamma, lz, uC);
}

// Where a thread stands: its tile, its column, the columns beside the tile (crd_jacobian.hip: tile_pos).
struct TilePos {
	int tx, ty, i, j0, iw, ie;
	bool col_ok, last_col;
};
__device__ __forceinline__ TilePos tile_pos(int nx, int nbx, int nblocks)
{
	TilePos p;
	const int tid = xcd_remap((int)blockIdx.x, nblocks);
	const int by = tid / nbx, bx = tid - by * nbx;
	p.tx = threadIdx.x;
	p.ty = threadIdx.y;
	const int i0 = bx * kTX;
	p.i = i0 + p.tx;
	p.j0 = by * kTY;
	p.col_ok = p.i < nx;
	p.iw = (i0 == 0) ? nx - 1 : i0 - 1;  // theta wrap: column -1 is column nx - 1
	p.last_col = p.col_ok && (p.tx == kTX - 1 || p.i == nx - 1);
	p.ie = (p.i == nx - 1) ? 0 : p.i + 1;
	return p;
}

template <typename Real>
__global__ void __launch_bounds__(kTX *kBY) crd_mg_sweep_kernel(Level<Real> l, int flags, const typename Pair<Real>::type *__restrict__ r_aos,
                                                                const Real *__restrict__ r_plane, Real *__restrict__ r_store, const Real *__restrict__ z_in,
                                                                Real *__restrict__ z_out, typename Pair<Real>::type *__restrict__ z_aos, int nbx, int nblocks)
{
	using P = typename Pair<Real>::type;
	__shared__ Real tile[kTY + 2][kTX + 2];
	const TilePos p = tile_pos(l.nx, nbx, nblocks);
	const int nx = l.nx, ny = l.ny;
	const bool first = (flags & kMgFirst) != 0;  // uniform over the launch: every thread of a block takes the same side
	Real own[kRPT];
#pragma unroll
	for (int r = 0; r < kRPT; r++) own[r] = (Real)0;
	if (!first) {
#pragma unroll
		for (int r = 0; r < kRPT; r++) {
			const int j = p.j0 + p.ty + kBY * r;
			if (j < ny && p.col_ok) {
				const Real *row = z_in + (size_t)j * nx;
				own[r] = row[p.i];
				if (p.tx == 0) tile[p.ty + kBY * r + 1][0] = row[p.iw];
				if (p.last_col) tile[p.ty + kBY * r + 1][p.tx + 2] = row[p.ie];
				tile[p.ty + kBY * r + 1][p.tx + 1] = own[r];
			}
		}
		// halo rows j0 - 1 (wave 0) and min(j0 + kTY, ny) (wave 1), wrapped in phi
		if (p.ty < 2 && p.col_ok) {
			const int jt = (p.ty == 0) ? p.j0 - 1 : ((p.j0 + kTY < ny) ? p.j0 + kTY : ny);
			const int tr = (p.ty == 0) ? 0 : jt - p.j0 + 1;
			tile[tr][p.tx + 1] = z_in[(size_t)wrap_index(jt, ny) * nx + p.i];
		}
		__syncthreads();
	}
	const Real cE = p.col_ok ? l.cE[p.i] : (Real)0;
	const Real cWn = p.col_ok ? l.cWn[p.i] : (Real)0;
	const Real cP = p.col_ok ? l.cP[p.i] : (Real)0;
	const Real w = l.omega / fmadd(l.gamma, fmadd((Real)2.0, cP, l.cX2), (Real)1.0);  // omega / d, d = 1 + gamma (2 cX + 2 cP)
#pragma unroll
	for (int r = 0; r < kRPT; r++) {
		const int j = p.j0 + p.ty + kBY * r;
		if (!(j < ny && p.col_ok)) continue;
		const size_t o = (size_t)j * nx + p.i;
		Real rhs, var1 = (Real)0;
		if (flags & kMgRhsAos) {
			const P q = r_aos[o];
			rhs = q.x;
			var1 = q.y;
		} else {
			rhs = r_plane[o];
		}
		if (flags & kMgStoreRhs) r_store[o] = rhs;
		Real zn;
		if (first) {
			zn = w * rhs;
		} else {
			const int tr = p.ty + kBY * r + 1;
			const Real az = apply_point<Real>(l, own[r], tile[tr][p.tx], tile[tr][p.tx + 2], tile[tr - 1][p.tx + 1], tile[tr + 1][p.tx + 1], cE, cWn, cP, false);
			zn = fmadd(w, rhs - az, own[r]);
		}
		if (held_row(l, j)) zn = rhs;
		if (flags & kMgOutAos) {
			P out;
			out.x = zn;
			out.y = var1;
			z_aos[o] = out;
		} else {
			z_out[o] = zn;
		}
	}
}

template <typename Real>
__global__ void __launch_bounds__(kTX *kBY) crd_mg_restrict_kernel(Level<Real> l, int nxc, int nyc, int held_coarse, int rhs_aos,
                                                                   const typename Pair<Real>::type *__restrict__ r_aos, const Real *__restrict__ r_plane,
                                                                   const Real *__restrict__ z, Real *__restrict__ rc, int nbx, int nblocks)
{
	__shared__ Real zt[kZR][kZC + 1];
	__shared__ Real st[kSR][kSC + 1];
	const int nx = l.nx, ny = l.ny;
	const int bid = xcd_remap((int)blockIdx.x, nblocks);
	const int by = bid / nbx, bx = bid - by * nbx;
	const int I0 = bx * kCX, J0 = by * kCY, fi0 = 2 * I0, fj0 = 2 * J0;
	const int t = (int)threadIdx.y * kTX + (int)threadIdx.x;
	// z at fine rows fj0 - 2 .. fj0 + 2 kCY, columns fi0 - 2 .. fi0 + 2 kCX, as far as the grid (and one wrapped row / column) goes
	for (int q = t; q < kZR * kZC; q += kTX * kBY) {
		const int rr = q / kZC, cc = q - rr * kZC;
		const int fj = fj0 - 2 + rr, fi = fi0 - 2 + cc;
		Real v = (Real)0;
		if (fj <= ny && fi <= nx) v = z[(size_t)wrap_index(fj, ny) * nx + wrap_index(fi, nx)];
		zt[rr][cc] = v;
	}
	__syncthreads();
	// the residual at fine rows fj0 - 1 .. fj0 + 2 kCY - 1, columns fi0 - 1 .. fi0 + 2 kCX - 1
	for (int q = t; q < kSR * kSC; q += kTX * kBY) {
		const int rr = q / kSC, cc = q - rr * kSC;
		const int fj = fj0 - 1 + rr, fi = fi0 - 1 + cc;
		Real s = (Real)0;
		if (fj < ny && fi < nx) {
			const int jw = wrap_index(fj, ny), iw = wrap_index(fi, nx);
			const size_t o = (size_t)jw * nx + iw;
			const Real rhs = rhs_aos ? r_aos[o].x : r_plane[o];
			const Real az = apply_point<Real>(l, zt[rr + 1][cc + 1], zt[rr + 1][cc], zt[rr + 1][cc + 2], zt[rr][cc + 1], zt[rr + 2][cc + 1], l.cE[iw], l.cWn[iw],
			                                  l.cP[iw], held_row(l, jw));
			s = rhs - az;
		}
		st[rr][cc] = s;
	}
	__syncthreads();
	const int lj = t / kCX, li = t - lj * kCX;
	const int J = J0 + lj, I = I0 + li;
	if (J < nyc && I < nxc) {
		const int a = 2 * lj + 1, b = 2 * li + 1;  // coarse (J, I) is fine (2 J, 2 I)
		const Real edge = (st[a][b - 1] + st[a][b + 1]) + (st[a - 1][b] + st[a + 1][b]);
		const Real corner = (st[a - 1][b - 1] + st[a - 1][b + 1]) + (st[a + 1][b - 1] + st[a + 1][b + 1]);
		Real out = (Real)0.0625 * fmadd((Real)4.0, st[a][b], fmadd((Real)2.0, edge, corner));
		if (held_coarse && J == 0) out = (Real)0;
		rc[(size_t)J * nxc + I] = out;
	}
}

template <typename Real>
__global__ void __launch_bounds__(kTX *kBY) crd_mg_prolong_kernel(int nx, int ny, int held_lo, int held_hi, int nxc, int nyc, const Real *__restrict__ e,
                                                                  Real *__restrict__ z, const typename Pair<Real>::type *__restrict__ r_aos,
                                                                  typename Pair<Real>::type *__restrict__ z_aos, int nbx, int nblocks)
{
	const TilePos p = tile_pos(nx, nbx, nblocks);
	if (!p.col_ok) return;
	const int I = p.i >> 1;
	int Ip = I + (p.i & 1);
	if (Ip == nxc) Ip = 0;
#pragma unroll
	for (int r = 0; r < kRPT; r++) {
		const int j = p.j0 + p.ty + kBY * r;
		if (j >= ny) continue;
		const size_t o = (size_t)j * nx + p.i;
		if ((held_lo && j == 0) || (held_hi && j == ny - 1)) {  // the correction is zero on a held row
			if (z_aos) {
				typename Pair<Real>::type out = r_aos[o];
				out.x = z[o];
				z_aos[o] = out;
			}
			continue;
		}
		const int J = j >> 1;
		int Jp = J + (j & 1);
		if (Jp == nyc) Jp = 0;
		const Real *lo = e + (size_t)J * nxc, *hi = e + (size_t)Jp * nxc;
		// one form for all four parities: where an index pair coincides the sum is an exact doubling, so an even / even point takes
		// e itself and an edge point the mean of its two neighbours
		const Real corr = (Real)0.25 * ((lo[I] + lo[Ip]) + (hi[I] + hi[Ip]));
		if (z_aos) {
			typename Pair<Real>::type out = r_aos[o];
			out.x = z[o] + corr;
			z_aos[o] = out;
		} else {
			z[o] = z[o] + corr;
		}
	}
}

bool level_ok(const MgLevel &m) { return m.nx >= 1 && m.ny >= 1 && m.cE && m.cWn && m.cP; }

template <typename Real>
hipError_t sweep_t(const MgLevel &m, double gamma, double omega, int flags, const void *r_aos, const void *z_in, void *z_out, void *z_aos, hipStream_t st)
{
	using P = typename Pair<Real>::type;
	const int nbx = (m.nx + kTX - 1) / kTX, nby = (m.ny + kTY - 1) / kTY;
	crd_mg_sweep_kernel<Real><<<nbx * nby, dim3(kTX, kBY), 0, st>>>(typed_level<Real>(m, gamma, omega), flags, static_cast<const P *>(r_aos),
	                                                                static_cast<const Real *>(m.r), static_cast<Real *>(m.r), static_cast<const Real *>(z_in),
	                                                                static_cast<Real *>(z_out), static_cast<P *>(z_aos), nbx, nbx * nby);
	return launch_status();
}

template <typename Real>
hipError_t restrict_t(const MgLevel &f, const MgLevel &c, double gamma, int rhs_aos, const void *r_aos, const void *z, hipStream_t st)
{
	using P = typename Pair<Real>::type;
	const int nbx = (c.nx + kCX - 1) / kCX, nby = (c.ny + kCY - 1) / kCY;
	crd_mg_restrict_kernel<Real><<<nbx * nby, dim3(kTX, kBY), 0, st>>>(typed_level<Real>(f, gamma, 1.0), c.nx, c.ny, c.held_lo, rhs_aos, static_cast<const P *>(r_aos),
	                                                                   static_cast<const Real *>(f.r), static_cast<const Real *>(z), static_cast<Real *>(c.r), nbx,
	                                                                   nbx * nby);
	return launch_status();
}

template <typename Real>
hipError_t prolong_t(const MgLevel &f, const MgLevel &c, const void *e, void *z, const void *r_aos, void *z_aos, hipStream_t st)
{
	using P = typename Pair<Real>::type;
	const int nbx = (f.nx + kTX - 1) / kTX, nby = (f.ny + kTY - 1) / kTY;
	crd_mg_prolong_kernel<Real><<<nbx * nby, dim3(kTX, kBY), 0, st>>>(f.nx, f.ny, f.held_lo, f.held_hi, c.nx, c.ny, static_cast<const Real *>(e), static_cast<Real *>(z),
	                                                                  static_cast<const P *>(r_aos), static_cast<P *>(z_aos), nbx, nbx * nby);
	return launch_status();
}

}  // namespace

hipError_t launch_mg_sweep(int precision, const MgLevel &L, double gamma, double omega, int flags, const void *r_aos, const void *z_in, void *z_out, void *z_aos,
                           hipStream_t s)
{
	clear_launch_status();
	if (!level_ok(L)) return hipErrorInvalidValue;
	const bool rhs_aos = (flags & kMgRhsAos) != 0, out_aos = (flags & kMgOutAos) != 0;
	if (rhs_aos ? !r_aos : !L.r) return hipErrorInvalidValue;
	if ((flags & kMgStoreRhs) && (!rhs_aos || !L.r)) return hipErrorInvalidValue;
	if (out_aos ? (!z_aos || !rhs_aos) : !z_out) return hipErrorInvalidValue;
	if (!(flags & kMgFirst) && (!z_in || z_in == z_out)) return hipErrorInvalidValue;  // a sweep reads the old z everywhere
	return precision == CRD_PRECISION_F64 ? sweep_t<double>(L, gamma, omega, flags, r_aos, z_in, z_out, z_aos, s)
	                                      : sweep_t<float>(L, gamma, omega, flags, r_aos, z_in, z_out, z_aos, s);
}

hipError_t launch_mg_restrict(int precision, const MgLevel &fine, const MgLevel &coarse, double gamma, int rhs_aos, const void *r_aos, const void *z, hipStream_t s)
{
	clear_launch_status();
	if (!level_ok(fine) || coarse.nx < 1 || coarse.ny < 1 || !coarse.r || !z) return hipErrorInvalidValue;
	if (fine.nx != 2 * coarse.nx || fine.ny != 2 * coarse.ny || coarse.nx < 4 || coarse.ny < 4) return hipErrorInvalidValue;  // the kernel's index ranges
	if (rhs_aos ? !r_aos : !fine.r) return hipErrorInvalidValue;
	return precision == CRD_PRECISION_F64 ? restrict_t<double>(fine, coarse, gamma, rhs_aos, r_aos, z, s) : restrict_t<float>(fine, coarse, gamma, rhs_aos, r_aos, z, s);
}

hipError_t launch_mg_prolong(int precision, const MgLevel &fine, const MgLevel &coarse, const void *e, void *z, const void *r_aos, void *z_aos, hipStream_t s)
{
	clear_launch_status();
	if (fine.nx != 2 * coarse.nx || fine.ny != 2 * coarse.ny || coarse.nx < 1 || coarse.ny < 1 || !e || !z || (z_aos && !r_aos)) return hipErrorInvalidValue;
	return precision == CRD_PRECISION_F64 ? prolong_t<double>(fine, coarse, e, z, r_aos, z_aos, s) : prolong_t<float>(fine, coarse, e, z, r_aos, z_aos, s);
}

}  // namespace crd
