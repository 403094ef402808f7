// crd_ensemble_item.h -- where an ensemble work item is set up: what the six ensemble step units (crd_ensemble.hip, _mixed, _own,
// _adaptive, _multi, _mixed_multi) share around the two bodies of crd_fused_impl.h, fused_item and fused_item_multi_step.  Device side:
// a member's Slab and FusedArgs, the absorbing decision per stage and per item, the search of a prefix of block counts.  Host side:
// the ladder from (precision, model, columns, absorb) to an instantiation, the step's constants in the kernel's precision, and the rules
// the plans share (strips, blocks of strips, rows per work item).  Included after crd_fused_impl.h, by those units only.
//
// The rule for when a block takes the absorbing body has to stay the single-slab kernel's in every unit -- bit-identity with a context
// stepped alone rests on it -- so it is written here (touches_boundary).  The kernels themselves, their names and template
// arguments, the block -> (member, chunk, strip) arithmetic and the __shared__ arrays stay in the units: separate units are what keeps
// each kernel's code and registers apart.  What is shared is held to one bar: every instantiation's VGPRs, scratch, LDS, wavefronts
// per SIMD and count of scalar values kept in vector lanes equal to the hand-written kernel's (profiles/ensemble/kernel_resources.txt).
// A step that moved one of them behind a helper stays written out in its kernel, with a comment there; so does the whole set-up of
// crd_ensemble_step_mixed_kernel and crd_ensemble_attempt_kernel, which a timing against the hand-written kernels did not clear
// (profiles/ensemble/refactor_ab.txt).  DESIGN.md, "Ensembles".
#pragma once

#include <algorithm>
#include <cstdint>

#include "crd_ensemble.h"

namespace crd {

typedef const __attribute__((address_space(4))) EnsembleMember ConstMember;

// ---- device side ----

// A member as the bodies see a slab: its tables, the launch's (or its own) nx and ny.
template <typename Real, int MODEL>
static __device__ __forceinline__ Slab<Real> member_slab(ConstMember *m, Real ka4, int nx, int ny)
{
	Slab<Real> s;
	s.cE = static_cast<const Real *>(m->cE);
	s.cWn = static_cast<const Real *>(m->cWn);
	s.cP = static_cast<const Real *>(m->cP);
	s.brow = static_cast<const Real *>(m->brow) + kGhost;  // index by row (kGhost >= 2 kApron entries either side: the pair's aprons too)
	s.ka4 = ka4;
	s.nx = nx;
	s.nyl = ny;
	s.wrap = 1;  // a member is a single slab: phi wraps inside it
	s.has_row0 = s.has_rowN = 1;
	s.just_diffusion = MODEL == kModelDiffusionOnly;
	s.wrap_x = 1;
	return s;
}

// The rows and work items of one member: one range, all ny rows, in chunks of `chunk`.
template <typename Real>
static __device__ __forceinline__ void item_geometry(FusedArgs<Real> &a, int ny, int nstrips, int nchunks, int nitems, int chunk, int sw, int nblocks)
{
	a.js = 0;
	a.ny = ny;
	a.r_begin[0] = a.r_begin[1] = 0;
	a.r_end[0] = a.r_end[1] = ny;
	a.chunk = chunk;
	a.first2 = a.nchunks = nchunks;
	a.nstrips = nstrips;
	a.nitems = nitems;
	a.nblocks = nblocks;
	a.sw = sw;
}

// The state a step reads and writes: the member's ping-pong planes ...
template <typename Real>
static __device__ __forceinline__ void member_planes(FusedArgs<Real> &a, ConstMember *m, int src)
{
	a.in_u = static_cast<const Real *>(m->u[src]);
	a.in_v = static_cast<const Real *>(m->v[src]);
	a.out_u = static_cast<Real *>(m->u[1 - src]);
	a.out_v = static_cast<Real *>(m->v[1 - src]);
}

// ... or two state buffers of a slot or attempt table: the u plane, then the v plane.
template <typename Real>
static __device__ __forceinline__ void member_planes(FusedArgs<Real> &a, const void *in, void *out, size_t plane)
{
	a.in_u = static_cast<const Real *>(in);
	a.in_v = a.in_u + plane;
	a.out_u = static_cast<Real *>(out);
	a.out_v = a.out_u + plane;
}

// The step's constants: the launch's, rounded on the host (StepConstants below) ...
template <typename Real, typename Constants>
static __device__ __forceinline__ void step_sizes(FusedArgs<Real> &a, const Constants &k)
{
	a.h1 = k.h1;
	a.h2 = k.h2;
	a.h3 = k.h3;
	a.h6 = k.h6;
}

// ... or an entry's own (EnsembleOwnSlot, EnsembleAttempt: h in double, hf rounded to fp32 on the host).
template <typename Real, typename ConstEntry>
static __device__ __forceinline__ void entry_step_sizes(FusedArgs<Real> &a, ConstEntry *en)
{
	if constexpr (sizeof(Real) == 8) {
		a.h1 = en->h[0];
		a.h2 = en->h[1];
		a.h3 = en->h[2];
		a.h6 = en->h[3];
	} else {
		a.h1 = en->hf[0];
		a.h2 = en->hf[1];
		a.h3 = en->hf[2];
		a.h6 = en->hf[3];
	}
}

// At which stages the member's rows absorb, and whether at any: the launch's stage times against the member's t_boundary (strict <,
// as absorbing(), crd_ctx.h).  The one-step kernels' four; the pair kernels compare their eight themselves (behind any helper their
// absorbing instantiations came out with other registers), as the slot kernel copies the flags the host decided.
template <typename Real>
static __device__ __forceinline__ bool stage_absorbs(FusedArgs<Real> &a, const double *t_stage, double tb)
{
	bool absorbs = false;
	for (int k = 0; k < 4; k++) {
		a.absorb[k] = t_stage[k] < tb ? 1 : 0;
		absorbs = absorbs || a.absorb[k];
	}
	return absorbs;
}

// The per-item rule, the single-slab kernel's per-chunk one (crd_rk4_fused_step_kernel): the selects only where the member absorbs at
// some stage AND the chunk's pipeline -- rows [j0 - apron, j1 + apron) -- can meet global row 0 or ny - 1.  With js = 0, one range and
// ny >= 8 the rows reach row 0 exactly when j0 - apron <= 0 and row ny - 1 exactly when j1 + apron >= ny.  apron: kApron for a step.
// The pair kernels spell the same rule out with 2 kApron, as a value they pass
// through readfirstlane: behind this helper their absorbing instantiations came out with other registers.
static __device__ __forceinline__ bool touches_boundary(bool absorbs, int chunk, int chunk_rows, int ny, int apron)
{
	const int j0 = chunk * chunk_rows, j1 = (j0 + chunk_rows < ny) ? j0 + chunk_rows : ny;
	// (`if (...) return true;`, not `return ...;`: the compiler then keeps the short-circuit branches of the kernels this rule was
	// written out in, and with them every absorbing instantiation's registers; as one boolean value the one-step kernels came out with
	// other register counts and, in fp32, another occupancy)
	if (absorbs && (j0 - apron <= 0 || j1 + apron >= ny)) return true;
	return false;
}

// One step of the work item: fused_item with the selects where touches_boundary says so, without them elsewhere.
template <typename Real, int MODEL, bool ABSORB, int COLS>
static __device__ __forceinline__ void step_item(const Slab<Real> &s, const FusedArgs<Real> &a, bool absorbs, int strip, int chunk)
{
	if constexpr (ABSORB) {
		if (touches_boundary(absorbs, chunk, a.chunk, a.ny, kApron)) {
			fused_item<Real, MODEL, true, 0, COLS, false>(s, a, strip, chunk);
			return;
		}
	}
	fused_item<Real, MODEL, false, 0, COLS, false>(s, a, strip, chunk);
}

// The entry whose blocks hold block `blk` of the entry-major order: the last of table[0 .. count].first_block that is <= blk
// (EnsembleShape: members; EnsembleOwnSlot: active slots).  blk is uniform over the block, so the bisection runs on scalar registers
// and scalar loads; the result goes through readfirstlane so the compiler sees it so.  Every entry has at least one block: the prefix
// rises strictly.
template <typename ConstEntry>
static __device__ __forceinline__ int prefix_entry(ConstEntry *table, int count, int blk)
{
	int lo = 0, hi = count;  // first_block[lo] <= blk < first_block[hi]
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (table[mid].first_block <= blk) lo = mid;
		else hi = mid;
	}
	return __builtin_amdgcn_readfirstlane(lo);
}

// max |u| over u[0 .. n) of member blockIdx.y, folded into out[blockIdx.y]; blocks of 256 threads.  The 32 bytes of LDS are declared
// here on purpose, unlike the step kernels' rings and edges: they are this body's alone, and its two kernels are nothing but it.  NaN propagates (the blow-up guard
// of crd_max_abs_kernel, crd_kernels.hip).
template <typename Real>
static __device__ __forceinline__ void member_max_abs(const Real *u, size_t n, double *out)
{
	__shared__ double part[4];
	double m = 0.0;
	for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
		const double a = fabs((double)u[q]);
		m = (a > m || a != a) ? a : m;
	}
	for (int off = 32; off > 0; off >>= 1) {
		const double o = __shfl_down(m, off, 64);
		m = (o > m || o != o) ? o : m;
	}
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < 4; w++) m = (part[w] > m || part[w] != part[w]) ? part[w] : m;
		// non-negative doubles order like their bit patterns; NaN (0x7ff8...) sorts above every finite value
		atomicMax(reinterpret_cast<unsigned long long *>(out + blockIdx.y), (unsigned long long)__double_as_longlong(m));
	}
}

// ---- host side: from a launch's settings to a kernel instantiation ----

// What the kernels' argument structs begin with: the step's constants in the kernel's precision, rounded on the host as launch_fused_t
// rounds them (a conversion in the kernel would be a vector instruction, its result held in vector registers).
template <typename Real>
struct StepConstants {
	Real h1, h2, h3, h6, ka4;
	explicit StepConstants(const EnsembleStep &e) : h1((Real)e.h1), h2((Real)e.h2), h3((Real)e.h3), h6((Real)e.h6), ka4((Real)e.ka4) {}
};

// One instantiation of a unit's kernel, as a value a generic lambda takes.
template <typename R, int MODEL, bool ABSORB, int COLS>
struct Instantiation {
	using Real = R;
	static constexpr int kModel = MODEL;
	static constexpr bool kAbsorb = ABSORB;
	static constexpr int kCols = COLS;
};

template <typename Real, int MODEL, typename F>
hipError_t with_instantiation_of(int cols, bool absorb, F &f)
{
	// (the diffusion-only variant skips the reaction block, absorbing rows included: no instantiation with the selects)
	constexpr bool kCanAbsorb = MODEL != kModelDiffusionOnly;
	if (cols == 2) {
		if constexpr (sizeof(Real) == 4) {
			if (kCanAbsorb && absorb) f(Instantiation<Real, MODEL, kCanAbsorb, 2>{});
			else f(Instantiation<Real, MODEL, false, 2>{});
			return hipSuccess;
		}
		return hipErrorInvalidValue;  // (fp64: one column per lane)
	}
	if (kCanAbsorb && absorb) f(Instantiation<Real, MODEL, kCanAbsorb, 1>{});
	else f(Instantiation<Real, MODEL, false, 1>{});
	return hipSuccess;
}

// f(Instantiation<Real, MODEL, ABSORB, COLS>{}) for the launch's precision, model (kernel_model's), columns per lane and absorb flag.
template <typename F>
hipError_t with_instantiation(int precision, int model, int cols, bool absorb, F &&f)
{
	if (precision == CRD_PRECISION_F64) {
		switch (model) {
		case CRD_MODEL_FHN: return with_instantiation_of<double, CRD_MODEL_FHN>(cols, absorb, f);
		case CRD_MODEL_GOLDBETER: return with_instantiation_of<double, CRD_MODEL_GOLDBETER>(cols, absorb, f);
		default: return with_instantiation_of<double, kModelDiffusionOnly>(cols, absorb, f);
		}
	}
	switch (model) {
	case CRD_MODEL_FHN: return with_instantiation_of<float, CRD_MODEL_FHN>(cols, absorb, f);
	case CRD_MODEL_GOLDBETER: return with_instantiation_of<float, CRD_MODEL_GOLDBETER>(cols, absorb, f);
	default: return with_instantiation_of<float, kModelDiffusionOnly>(cols, absorb, f);
	}
}

// Workgroups of sw wavefronts a CU holds of the unit's select-free kernel: kernel_of(Instantiation) names it.
template <typename F>
int resident_blocks_per_cu(int precision, int model, int cols, int sw, F &&kernel_of)
{
	int per_cu = 0;
	hipError_t r = hipErrorInvalidValue;
	(void)with_instantiation(precision, model, cols, false,
	                         [&](auto k) { r = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(kernel_of(k)), kLanes * sw, 0); });
	return (r == hipSuccess && per_cu >= 1) ? per_cu : 1;
}

// ---- host side: what the plans share ----

// Strip cutting, for every member of a launch: shapes[k].nx, ny, nstrips and nsb; returns sw, the wavefronts per block of the launch.
// A wavefront stores cols * kLanes columns less an apron either side; sw = min(4, the most strips of any member) (a block of narrow
// members: no wavefronts that only return); nsb = ceil(nstrips / sw) blocks across one chunk of rows.  block_is_strip (kCoop: the pair
// kernels of Goldbeter in fp64): the block as the strip, ONE apron around its sw wavefronts (240 valid columns of four wavefronts' 256),
// every member's strips a multiple of sw.
static inline int cut_strips(const int *nx, const int *ny, int members, int cols, int apron, bool block_is_strip, EnsembleShape *shapes)
{
	const int valid = cols * kLanes - 2 * apron;
	int most_strips = 0;
	for (int k = 0; k < members; k++) {
		shapes[k] = EnsembleShape{};
		shapes[k].nx = nx[k];
		shapes[k].ny = ny[k];
		shapes[k].nstrips = (nx[k] + valid - 1) / valid;
		most_strips = std::max(most_strips, shapes[k].nstrips);
	}
	const int sw = std::min(kWavesPerBlock, most_strips);
	const int block_valid = sw * kLanes - 2 * apron;
	for (int k = 0; k < members; k++) {
		if (block_is_strip) {
			shapes[k].nsb = (nx[k] + block_valid - 1) / block_valid;
			shapes[k].nstrips = sw * shapes[k].nsb;
		} else {
			shapes[k].nsb = (shapes[k].nstrips + sw - 1) / sw;
		}
	}
	return sw;
}

// ... of members of one shape, into their plan.
static inline void cut_strips(int nx, int ny, int cols, int apron, bool block_is_strip, EnsemblePlan *plan)
{
	EnsembleShape sh;
	plan->sw = cut_strips(&nx, &ny, 1, cols, apron, block_is_strip, &sh);
	plan->nstrips = sh.nstrips;
	plan->nsb = sh.nsb;
}

// Rows per work item, a fixed rule ("Ensembles"): `start` rows halved while all members together -- blocks_at(chunk) blocks
// -- would not give two rounds of resident blocks, down to 8; 4 where even 8-row chunks give fewer than small_launch_floor blocks
// (fused_chunk_rows' rule for tiny launches, device_cus() / 2; 0: no such floor).
template <typename F>
int ensemble_chunk_rows(int start, F &&blocks_at, long resident_blocks, int small_launch_floor)
{
	int chunk = start;
	while (chunk > 8 && blocks_at(chunk) < 2 * resident_blocks) chunk /= 2;
	if (chunk == 8 && blocks_at(8) < small_launch_floor) chunk = 4;
	return chunk;
}

// Rows per work item the pair plans start from: what fused_chunk_rows uses for the single slab's two-step launches.  UNMEASURED on
// ensembles -- a build with -DCRD_ENSEMBLE_PAIR_CHUNK=32 / 64 is the other arm of an A/B that has still to be run.
#ifndef CRD_ENSEMBLE_PAIR_CHUNK
#define CRD_ENSEMBLE_PAIR_CHUNK 128
#endif

// ---- host side: plans over a list of shapes (ensemble_plan_mixed, ensemble_pair_plan_mixed) ----

// The blocks of all members together at `chunk` rows per work item (nsb set): what the plans' halving rules weigh.
static inline long mixed_blocks(const EnsembleShape *shapes, int members, int chunk)
{
	long b = 0;
	for (int k = 0; k < members; k++) b += (long)shapes[k].nsb * ((shapes[k].ny + chunk - 1) / chunk);
	return b;
}

// nchunks of every member at the launch's chunk height and the prefix of block counts, shapes[members] included.  A prefix that leaves
// 32 bits is stored as -1 from the first member past it on (the last entry too): such a plan must not be launched, and
// mixed_overflow_member (crd_ensemble.h) names the member for the caller's refusal.
static inline void mixed_fill_prefix(int chunk, int members, EnsembleShape *shapes)
{
	long first = 0;
	shapes[members] = EnsembleShape{};
	for (int k = 0; k < members; k++) {
		shapes[k].nchunks = (shapes[k].ny + chunk - 1) / chunk;
		shapes[k].first_block = first > INT32_MAX ? -1 : (int)first;
		first += (long)shapes[k].nsb * shapes[k].nchunks;
	}
	shapes[members].first_block = first > INT32_MAX ? -1 : (int)first;
}

}  // namespace crd
