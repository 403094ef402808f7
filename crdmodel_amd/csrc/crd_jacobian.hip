// crd_jacobian.hip -- the split right-hand side and the Jacobian's action on a vector, on the reference's AoS vectors
// (crd_rhs_part_* / crd_jtimes_*: what an implicit or IMEX integrator asks of a problem besides f).
//
// Both kernels have the geometry of crd_rhs_aos_kernel (crd_kernels.hip): one thread per grid point, 64 x 4 blocks sweeping 64 x 16
// tiles dealt to the XCDs in contiguous runs; var0 of the stencil's vector plus its one-point halo ring in LDS (18 x 66); theta wraps
// by index arithmetic, phi neighbours of the slab's first / last row come from the ghost strips or wrap inside a single slab;
// results go out with the non-temporal hint on large slabs.  Memory-bound like that kernel: 32 B per point in fp64 (a part: y in,
// ydot out), 48 B for J v (y and v in, Jv out).  theta-blocks are refused before a launch (crd_jacobian.cpp), so column -1 is
// always column nx - 1 here.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "crd_jacobian.h"

namespace crd {

namespace {

using namespace dev;

constexpr int kTX = 64;          // tile width = one wavefront along theta
constexpr int kBY = 4;           // waves per block
constexpr int kRPT = 4;          // rows per thread
constexpr int kTY = kBY * kRPT;  // tile height

template <bool NT, typename Real, typename P>
__device__ __forceinline__ void pair_store(P *p, const P &k)
{
	if constexpr (NT) {
		typedef Real vec2 __attribute__((ext_vector_type(2)));
		const vec2 v = {k.x, k.y};
		__builtin_nontemporal_store(v, reinterpret_cast<vec2 *>(p));
	} else {
		*p = k;
	}
}
inline bool stores_nontemporal(const SlabDesc &d, size_t real_bytes) { return (size_t)d.nx * (size_t)d.nyl * real_bytes >= ((size_t)32 << 20); }

// Where a thread stands: its tile, its column, the columns beside the tile.
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

// The thread's own pairs of `x` (rows j0 + ty + 4 r) into own[], var0 of the tile and of its halo ring into LDS: the loads of
// crd_rhs_aos_kernel, row for row.  Ends with the barrier.
template <typename Real>
__device__ __forceinline__ void stage_var0(Real (&tile)[kTY + 2][kTX + 2], const Slab<Real> &s, const TilePos &p, const typename Pair<Real>::type *__restrict__ x,
                                           const Real *__restrict__ ghost_lo, const Real *__restrict__ ghost_hi, typename Pair<Real>::type (&own)[kRPT])
{
	const int nx = s.nx, nyl = s.nyl;
#pragma unroll
	for (int r = 0; r < kRPT; r++) {
		const int j = p.j0 + p.ty + kBY * r;
		own[r].x = own[r].y = (Real)0;
		if (j < nyl && p.col_ok) {
			const typename Pair<Real>::type *row = x + (size_t)j * nx;
			own[r] = row[p.i];
			if (p.tx == 0) tile[p.ty + kBY * r + 1][0] = row[p.iw].x;
			if (p.last_col) tile[p.ty + kBY * r + 1][p.tx + 2] = row[p.ie].x;
			tile[p.ty + kBY * r + 1][p.tx + 1] = own[r].x;
		}
	}
	// halo rows j0 - 1 (wave 0) and min(j0 + kTY, nyl) (wave 1): a row of the slab, the wrapped row, or a ghost strip
	if (p.ty < 2 && p.col_ok) {
		const int jt = (p.ty == 0) ? p.j0 - 1 : ((p.j0 + kTY < nyl) ? p.j0 + kTY : nyl);
		const int tr = (p.ty == 0) ? 0 : jt - p.j0 + 1;
		Real val;
		if (jt >= 0 && jt < nyl) val = x[(size_t)jt * nx + p.i].x;
		else if (s.wrap) val = x[(size_t)(jt < 0 ? nyl - 1 : 0) * nx + p.i].x;
		else val = (jt < 0) ? ghost_lo[p.i] : ghost_hi[p.i];
		tile[tr][p.tx + 1] = val;
	}
	__syncthreads();
}

template <typename Real>
__device__ __forceinline__ bool absorbing_row(const Slab<Real> &s, int absorb, int j)
{
	return absorb && ((s.has_row0 && j == 0) || (s.has_rowN && j == s.nyl - 1));
}

// One part of f.  PART = kPartDiffusion: the operator on var0 of y (MODEL plays no role: instantiated once, as
// kModelDiffusionOnly); PART = kPartReaction: the kinetics, pointwise -- no tile, no neighbour is read.
template <typename Real, int MODEL, int PART, bool NT>
__global__ void __launch_bounds__(kTX *kBY) crd_rhs_part_aos_kernel(Slab<Real> s, const typename Pair<Real>::type *__restrict__ y,
                                                                    typename Pair<Real>::type *__restrict__ ydot, const Real *__restrict__ ghost_lo,
                                                                    const Real *__restrict__ ghost_hi, int absorb, int nbx, int nblocks)
{
	using P = typename Pair<Real>::type;
	static_assert(PART == kPartDiffusion || PART == kPartReaction, "the full f is crd_rhs_aos_kernel");
	const TilePos p = tile_pos(s.nx, nbx, nblocks);
	const int nx = s.nx, nyl = s.nyl;
	if constexpr (PART == kPartDiffusion) {
		__shared__ Real tile[kTY + 2][kTX + 2];
		P own[kRPT];
		stage_var0<Real>(tile, s, p, y, ghost_lo, ghost_hi, own);
		const Real cE = p.col_ok ? s.cE[p.i] : (Real)0;
		const Real cWn = p.col_ok ? s.cWn[p.i] : (Real)0;
		const Real cP = p.col_ok ? s.cP[p.i] : (Real)0;
#pragma unroll
		for (int r = 0; r < kRPT; r++) {
			const int j = p.j0 + p.ty + kBY * r;
			if (!(j < nyl && p.col_ok)) continue;
			const int tr = p.ty + kBY * r + 1;
			const Real uC = own[r].x;
			P k;
			rhs_point_diffusion<Real>(uC, uC - tile[tr][p.tx], tile[tr][p.tx + 2] - uC, tile[tr - 1][p.tx + 1], tile[tr + 1][p.tx + 1], cE, cWn, cP,
			                          absorbing_row(s, absorb, j), k.x, k.y);
			pair_store<NT, Real>(&ydot[(size_t)j * nx + p.i], k);
		}
	} else {
#pragma unroll
		for (int r = 0; r < kRPT; r++) {
			const int j = p.j0 + p.ty + kBY * r;
			if (!(j < nyl && p.col_ok)) continue;
			const size_t o = (size_t)j * nx + p.i;
			P own;
			own.x = own.y = (Real)0;
			if (MODEL != kModelDiffusionOnly) own = y[o];
			P k;
			rhs_point_reaction<Real, MODEL>(own.x, own.y, s.brow[j], s.ka4, absorbing_row(s, absorb, j), k.x, k.y);
			pair_store<NT, Real>(&ydot[o], k);
		}
	}
}

// J(t, y) v.  PART = kPartFull: var0 of v is staged in LDS, y and var1 of v are read at the own point only; PART = kPartReaction:
// pointwise.  (J_D v is crd_rhs_part_aos_kernel<kPartDiffusion> on v: the operator is linear.)
template <typename Real, int MODEL, int PART, bool NT>
__global__ void __launch_bounds__(kTX *kBY) crd_jtimes_aos_kernel(Slab<Real> s, const typename Pair<Real>::type *__restrict__ y,
                                                                  const typename Pair<Real>::type *__restrict__ v, typename Pair<Real>::type *__restrict__ jv,
                                                                  const Real *__restrict__ ghost_lo, const Real *__restrict__ ghost_hi, int absorb, int nbx,
                                                                  int nblocks)
{
	using P = typename Pair<Real>::type;
	const TilePos p = tile_pos(s.nx, nbx, nblocks);
	const int nx = s.nx, nyl = s.nyl;
	if constexpr (PART == kPartFull) {
		__shared__ Real tile[kTY + 2][kTX + 2];
		P own[kRPT], at[kRPT];
#pragma unroll
		for (int r = 0; r < kRPT; r++) {
			const int j = p.j0 + p.ty + kBY * r;
			at[r].x = at[r].y = (Real)0;
			if (j < nyl && p.col_ok) at[r] = y[(size_t)j * nx + p.i];
		}
		stage_var0<Real>(tile, s, p, v, ghost_lo, ghost_hi, own);
		const Real cE = p.col_ok ? s.cE[p.i] : (Real)0;
		const Real cWn = p.col_ok ? s.cWn[p.i] : (Real)0;
		const Real cP = p.col_ok ? s.cP[p.i] : (Real)0;
#pragma unroll
		for (int r = 0; r < kRPT; r++) {
			const int j = p.j0 + p.ty + kBY * r;
			if (!(j < nyl && p.col_ok)) continue;
			const int tr = p.ty + kBY * r + 1;
			const Real dC = own[r].x;
			P k;
			jac_point<Real, MODEL, kPartFull>(at[r].x, at[r].y, dC, own[r].y, dC - tile[tr][p.tx], tile[tr][p.tx + 2] - dC, tile[tr - 1][p.tx + 1],
			                                  tile[tr + 1][p.tx + 1], cE, cWn, cP, s.ka4, absorbing_row(s, absorb, j), k.x, k.y);
			pair_store<NT, Real>(&jv[(size_t)j * nx + p.i], k);
		}
	} else {
#pragma unroll
		for (int r = 0; r < kRPT; r++) {
			const int j = p.j0 + p.ty + kBY * r;
			if (!(j < nyl && p.col_ok)) continue;
			const size_t o = (size_t)j * nx + p.i;
			const P at = y[o], d = v[o];
			const Real z = (Real)0;
			P k;
			jac_point<Real, MODEL, kPartReaction>(at.x, at.y, d.x, d.y, z, z, z, z, z, z, z, s.ka4, absorbing_row(s, absorb, j), k.x, k.y);
			pair_store<NT, Real>(&jv[o], k);
		}
	}
}

struct Launch {
	int nbx, nblocks;
	bool nt;
};
template <typename Real>
Launch launch_of(const SlabDesc &d)
{
	const int nbx = (d.nx + kTX - 1) / kTX, nby = (d.nyl + kTY - 1) / kTY;
	return Launch{nbx, nbx * nby, stores_nontemporal(d, sizeof(Real))};
}

template <typename Real, int MODEL, int PART>
hipError_t launch_part_t(const SlabDesc &d, int absorb, const void *y, void *ydot, const void *glo, const void *ghi, hipStream_t st)
{
	using P = typename Pair<Real>::type;
	const Slab<Real> s = typed<Real>(d);
	const Launch l = launch_of<Real>(d);
	auto fire = [&](auto nt_c) {
		crd_rhs_part_aos_kernel<Real, MODEL, PART, decltype(nt_c)::value><<<l.nblocks, dim3(kTX, kBY), 0, st>>>(
		    s, static_cast<const P *>(y), static_cast<P *>(ydot), static_cast<const Real *>(glo), static_cast<const Real *>(ghi), absorb, l.nbx, l.nblocks);
	};
	if (l.nt) fire(std::true_type{});
	else fire(std::false_type{});
	return launch_status();
}

template <typename Real, int MODEL, int PART>
hipError_t launch_jtimes_t(const SlabDesc &d, int absorb, const void *y, const void *v, void *jv, const void *glo, const void *ghi, hipStream_t st)
{
	using P = typename Pair<Real>::type;
	const Slab<Real> s = typed<Real>(d);
	const Launch l = launch_of<Real>(d);
	auto fire = [&](auto nt_c) {
		crd_jtimes_aos_kernel<Real, MODEL, PART, decltype(nt_c)::value><<<l.nblocks, dim3(kTX, kBY), 0, st>>>(
		    s, static_cast<const P *>(y), static_cast<const P *>(v), static_cast<P *>(jv), static_cast<const Real *>(glo), static_cast<const Real *>(ghi), absorb,
		    l.nbx, l.nblocks);
	};
	if (l.nt) fire(std::true_type{});
	else fire(std::false_type{});
	return launch_status();
}

template <typename Real>
hipError_t launch_part_r(const SlabDesc &d, int part, int absorb, const void *y, void *ydot, const void *glo, const void *ghi, hipStream_t st)
{
	if (part == kPartDiffusion) return launch_part_t<Real, kModelDiffusionOnly, kPartDiffusion>(d, absorb, y, ydot, glo, ghi, st);
	switch (kernel_model(d)) {
	case CRD_MODEL_FHN: return launch_part_t<Real, CRD_MODEL_FHN, kPartReaction>(d, absorb, y, ydot, glo, ghi, st);
	case CRD_MODEL_GOLDBETER: return launch_part_t<Real, CRD_MODEL_GOLDBETER, kPartReaction>(d, absorb, y, ydot, glo, ghi, st);
	default: return launch_part_t<Real, kModelDiffusionOnly, kPartReaction>(d, absorb, y, ydot, glo, ghi, st);
	}
}

template <typename Real>
hipError_t launch_jtimes_r(const SlabDesc &d, int part, int absorb, const void *y, const void *v, void *jv, const void *glo, const void *ghi, hipStream_t st)
{
	const int model = kernel_model(d);
	// the linear part, and all there is of a diffusion-only context: f_D on v; that context's block is zero: its f_R
	if (part == kPartDiffusion || (model == kModelDiffusionOnly && part == kPartFull)) return launch_part_r<Real>(d, kPartDiffusion, absorb, v, jv, glo, ghi, st);
	if (model == kModelDiffusionOnly) return launch_part_r<Real>(d, kPartReaction, absorb, v, jv, glo, ghi, st);
	if (model == CRD_MODEL_FHN) {
		if (part == kPartFull) return launch_jtimes_t<Real, CRD_MODEL_FHN, kPartFull>(d, absorb, y, v, jv, glo, ghi, st);
		return launch_jtimes_t<Real, CRD_MODEL_FHN, kPartReaction>(d, absorb, y, v, jv, glo, ghi, st);
	}
	if (part == kPartFull) return launch_jtimes_t<Real, CRD_MODEL_GOLDBETER, kPartFull>(d, absorb, y, v, jv, glo, ghi, st);
	return launch_jtimes_t<Real, CRD_MODEL_GOLDBETER, kPartReaction>(d, absorb, y, v, jv, glo, ghi, st);
}

bool launchable(const SlabDesc &d, int part)
{
	if (part != kPartDiffusion && part != kPartReaction && part != kPartFull) return false;
	if (!d.wrap_x || d.nx < 1) return false;  // theta-blocks: no ghost-column strips here
	return true;
}

}  // namespace

hipError_t launch_rhs_part_aos(int precision, const SlabDesc &d, int part, int absorb, const void *y, void *ydot, const void *ghost_lo, const void *ghost_hi,
                               hipStream_t s)
{
	clear_launch_status();
	if (part == kPartFull) return launch_rhs_aos(precision, d, absorb, y, ydot, ghost_lo, ghost_hi, 0, d.nyl, s);
	if (!launchable(d, part) || !y || !ydot) return hipErrorInvalidValue;
	if (part == kPartDiffusion && !d.wrap && (!ghost_lo || !ghost_hi)) return hipErrorInvalidValue;
	if (d.nyl <= 0) return hipSuccess;
	return precision == CRD_PRECISION_F64 ? launch_part_r<double>(d, part, absorb, y, ydot, ghost_lo, ghost_hi, s)
	                                      : launch_part_r<float>(d, part, absorb, y, ydot, ghost_lo, ghost_hi, s);
}

hipError_t launch_jtimes_aos(int precision, const SlabDesc &d, int part, int absorb, const void *y, const void *v, void *jv, const void *ghost_lo,
                             const void *ghost_hi, hipStream_t s)
{
	clear_launch_status();
	if (!launchable(d, part) || !y || !v || !jv) return hipErrorInvalidValue;
	if (part != kPartReaction && !d.wrap && (!ghost_lo || !ghost_hi)) return hipErrorInvalidValue;
	if (d.nyl <= 0) return hipSuccess;
	return precision == CRD_PRECISION_F64 ? launch_jtimes_r<double>(d, part, absorb, y, v, jv, ghost_lo, ghost_hi, s)
	                                      : launch_jtimes_r<float>(d, part, absorb, y, v, jv, ghost_lo, ghost_hi, s);
}

}  // namespace crd
