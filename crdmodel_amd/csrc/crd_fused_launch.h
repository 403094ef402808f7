#pragma once
// crd_fused_launch.h -- the host side of the one-launch RK4 step: the step kernel around the device bodies of crd_fused_impl.h, the
// kernel selection, the launcher and the launch-plan measurement.  Included by crd_fused.hip (the fp64 instantiations) and
// crd_fused_f32.hip (the fp32 ones) only: two translation units so that the two halves of the instantiation matrix compile side by side.
// The plan's integer arithmetic -- steps per launch, strips, chunks, XCD mapping, band cut, candidates -- is crd_fused_plan.h's.
#include <atomic>

#include "crd_fused_impl.h"
#include "crd_fused_plan.h"

namespace crd {

namespace {

static_assert(plan::kApron == kApron && plan::kLanes == kLanes && plan::kWavesPerBlock == kWavesPerBlock && plan::kMaxWavesPerBlock == kMaxWavesPerBlock &&
                  plan::kWideWaves == kWideWaves && plan::kNumXcd == kNumXcd,
              "crd_fused_plan.h plans with the kernels' own constants");

// ABSORB = false: no stage of the step has t < tBoundary (every launch after the switch-off time, every launch of a run with
// tBoundary = 0) -- the absorbing-row selects are compiled out.  ABSORB = true: the items that can meet a global phi boundary row
// (src/FHNmodel_torus.cpp:643-653) run the body with the selects, all others the body without (see fused_item).
// EMBED, COLS, NT: see FusedArgs / fused_item above.
// STEPS = 2: two steps per launch (fused_item_two_steps).
// WAVES: the wavefronts of a block -- kMaxWavesPerBlock everywhere but in the eight-wide three-step block strip (kWideWaves).
template <typename Real, int MODEL, bool ABSORB, int EMBED, int COLS, bool NT = false, int STEPS = 1, int WAVES = kMaxWavesPerBlock>
__global__ void __launch_bounds__(kLanes *WAVES) __attribute__((amdgpu_waves_per_eu(kMinWaves<Real, MODEL, COLS, STEPS, ABSORB>))) crd_rk4_fused_step_kernel(Slab<Real> s, FusedArgs<Real> a)
{
	static_assert(STEPS == 1 || ((STEPS == 2 || STEPS == 3) && EMBED == 0), "several steps per launch: the plain step only");
	static_assert(WAVES == kMaxWavesPerBlock || (WAVES == kWideWaves && kCanWide<Real, MODEL, COLS, STEPS> && !ABSORB), "eight wavefronts per block: the three-step fp64 FHN block strip without the selects only");
	// The work item is a property of the wavefront: keep it (and everything derived from it: rows, trip counts, the
	// per-row table reads, the boundary-row tests) in scalar registers.
	// Optional remap: blocks are dealt round-robin over the 8 XCDs; the remap gives each XCD one contiguous run of items.
	// A block's wavefronts take adjacent strips of ONE chunk, blocks walk theta first.  The wavefronts of a block therefore
	// run the same trip counts, and in lockstep (one barrier per pipeline iteration) their row reads reach the memory system
	// together as one contiguous, overlapping run of a.sw x 448 B per row instead of drifting apart.
	const int nsb = (a.nstrips + a.sw - 1) / a.sw;
	int sblk, cblk;
	{
		const int b0 = (int)blockIdx.x;
		const int blk = a.remap == 1 ? xcd_remap(b0, a.nblocks) : b0;
		sblk = blk % nsb;
		cblk = blk / nsb;
		if (a.remap == 2) {
			// Succession in phi: XCD x owns a contiguous run of chunks; its resident workgroups form `xs_lanes` lanes per strip
			// block, and the workgroup that takes a finished one's place (ids are dispatched in order, 8 apart on one XCD) continues
			// that lane with the NEXT chunk in phi -- whose first rows are the rows its predecessor has just read into this L2.
			const int x = blk % kNumXcd, p = blk / kNumXcd, width = nsb * a.xs_lanes;
			const int d = p / width, sl = p - d * width;
			const int c0 = (int)((long)a.nchunks * x / kNumXcd), c1 = (int)((long)a.nchunks * (x + 1) / kNumXcd);
			const int depth = (c1 - c0 + a.xs_lanes - 1) / a.xs_lanes, lane_id = sl / nsb;
			sblk = sl - lane_id * nsb;
			cblk = (d < depth && c0 + lane_id * depth + d < c1) ? c0 + lane_id * depth + d : a.nchunks;  // nchunks: nothing to do
		}
	}
	const int strip = __builtin_amdgcn_readfirstlane(sblk * a.sw + (int)(threadIdx.x >> 6));
	const int chunk = __builtin_amdgcn_readfirstlane(cblk);
	if (strip >= a.nstrips || chunk >= a.nchunks) return;  // (a barrier waits for the surviving wavefronts of the workgroup only)
	// the row rings of a two-step launch's wavefronts (fused_item_two_steps)
	__shared__ __attribute__((aligned(16))) char rings[STEPS >= 2 ? kRingBytes<Real, COLS, STEPS, WAVES> : 16];
	lds_char *const block_rings = (lds_char *)rings;
	__shared__ __attribute__((aligned(16))) char edges[(STEPS >= 2 && kCoop<Real, MODEL, COLS, STEPS>) ? kEdgeBytes<STEPS, WAVES> + kEdgeDumpBytes<STEPS, WAVES> : 16];
	lds_char *const block_edges = (lds_char *)edges;
	if constexpr (ABSORB) {
		// Does any row this chunk's pipeline touches -- [j0 - APRON, j1 + APRON) -- map to global row 0 or ny - 1?  The two are
		// neighbours on the periodic grid: the rows contain one of them exactly when [lo, hi + 1] contains a multiple of ny.
		constexpr int APRON = STEPS * (EMBED != 0 ? kApron + 1 : kApron);
		const int range = chunk >= a.first2 ? 1 : 0;
		const int j0 = a.r_begin[range] + (chunk - (range ? a.first2 : 0)) * a.chunk;
		const int j1 = (j0 + a.chunk < a.r_end[range]) ? j0 + a.chunk : a.r_end[range];
		const int lo = a.js + j0 - APRON, hi1 = a.js + j1 + APRON;  // (lo > -ny and hi1 < 3 ny: a slab is at most the grid, ghost rows at most a slab)
		const bool touches = (lo <= 0 && 0 <= hi1) || (lo <= a.ny && a.ny <= hi1) || (lo <= 2 * a.ny && 2 * a.ny <= hi1);
		if constexpr (STEPS >= 2) {
			if (touches) fused_item_multi_step<Real, MODEL, true, COLS, NT, STEPS, kMaxWavesPerBlock, false>(s, a, strip, chunk, block_rings, sblk, block_edges);
			else fused_item_multi_step<Real, MODEL, false, COLS, NT, STEPS, kMaxWavesPerBlock, false>(s, a, strip, chunk, block_rings, sblk, block_edges);
		} else {
			if (touches) fused_item<Real, MODEL, true, EMBED, COLS, NT>(s, a, strip, chunk);
			else fused_item<Real, MODEL, false, EMBED, COLS, NT>(s, a, strip, chunk);
		}
	} else if constexpr (STEPS >= 2) {
		fused_item_multi_step<Real, MODEL, false, COLS, NT, STEPS, WAVES>(s, a, strip, chunk, block_rings, sblk, block_edges);
	} else {
		fused_item<Real, MODEL, false, EMBED, COLS, NT>(s, a, strip, chunk);
	}
}

// Adds the per-item error sums in a fixed order (thread t takes items t, t+256, ...; then a fixed LDS tree), so the error
// norm, and with it every accept / reject decision of the adaptive stepper, is reproducible from run to run.
__global__ void __launch_bounds__(256) crd_sum_partials_kernel(const double *__restrict__ partials, int n, double *__restrict__ out)
{
	__shared__ double part[256];
	double sum = 0.0;
	for (int q = threadIdx.x; q < n; q += 256) sum += partials[q];
	part[threadIdx.x] = sum;
	__syncthreads();
	for (int w = 128; w > 0; w >>= 1) {
		if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
		__syncthreads();
	}
	if (threadIdx.x == 0) *out = part[0];
}

// Three steps per launch (round 6), for the kernels whose two-step launch is bound by its memory path rather than by issue (DESIGN.md
// 4c, 4d): FHN in fp64 with one column per lane and the block as the strip (232 valid lanes of 256), and FHN in fp32 with two columns
// per lane and a strip per wavefront (104 valid columns of 128 -- no exchange between wavefronts).  kThreeStepCols: the columns per
// lane of the model's three-step kernel, 0 where there is none.
#ifdef CRD_THREE_STEPS_GOLDBETER  // (probe build: the three-step pipeline for Goldbeter fp64 too -- profiles/r06/goldbeter_floor.txt)
template <typename Real, int MODEL>
constexpr int kThreeStepCols = (MODEL == CRD_MODEL_FHN || (MODEL == CRD_MODEL_GOLDBETER && sizeof(Real) == 8)) ? (sizeof(Real) == 8 ? 1 : 2) : 0;
#else
template <typename Real, int MODEL>
constexpr int kThreeStepCols = MODEL == CRD_MODEL_FHN ? (sizeof(Real) == 8 ? 1 : 2) : 0;
#endif
template <typename Real, int MODEL>
constexpr bool kCanThreeSteps = kThreeStepCols<Real, MODEL> != 0;
// Two steps per launch: not the diffusion-only variant (no instantiation: that model is a plumbing case); nor has it absorbing rows --
// the reaction block of a diffusion-only run is skipped, absorbing rows included (src/GoldbeterModel_torus.cpp:668).
template <int MODEL>
constexpr bool kCanTwoSteps = MODEL != kModelDiffusionOnly;
template <int MODEL>
constexpr bool kCanAbsorb = MODEL != kModelDiffusionOnly;

// What crd_fused_plan.h is told about the kernels of one precision and model.
template <typename Real, int MODEL>
constexpr plan::KernelTraits kTraits = {(int)sizeof(Real), kCanTwoSteps<MODEL>, kThreeStepCols<Real, MODEL>, kCoop<Real, MODEL, 1, 2>, kCoop<Real, MODEL, 1, 3>,
                                        kCanWide<Real, MODEL, 1, 3>, kScalarRows<Real, MODEL, kThreeStepCols<Real, MODEL>, 3>};

// ---- kernel selection: run-time choices -> the instantiation ---------------------------------------------------------------------
struct KernelKey {
	bool absorb;  // the body with the absorbing-row selects (decided per chunk)
	int embed;    // 0: plain step; 1 / 2: the embedded pairs (one column per lane, one step)
	int cols;
	bool nt;
	int steps;
	int waves;    // wavefronts per block of the launch: up to kMaxWavesPerBlock, or kWideWaves
};
template <typename Real>
using StepKernel = void (*)(Slab<Real>, FusedArgs<Real>);

// The kernel of a key: absorbing rows x store hint x (embedded pair | columns per lane x steps per launch), all compile-time; nullptr where
// no kernel takes blocks of key.waves wavefronts.
// (The order of the branches -- true before false, two columns before one, three steps before two before one -- is the order in which
// the compiler meets the instantiations, and with it the order of the kernels in the objects and in the build's kernel table.)
template <typename Real, int MODEL>
StepKernel<Real> step_kernel(const KernelKey &k)
{
	constexpr std::true_type yes{};
	constexpr std::false_type no{};
	auto embedded = [&](auto absorb_c, auto nt_c) -> StepKernel<Real> {
		constexpr bool kAbsorb = decltype(absorb_c)::value && kCanAbsorb<MODEL>, kNt = decltype(nt_c)::value;
		if (k.embed == 2) return crd_rk4_fused_step_kernel<Real, MODEL, kAbsorb, 2, 1, kNt>;
		return crd_rk4_fused_step_kernel<Real, MODEL, kAbsorb, 1, 1, kNt>;
	};
	auto plain = [&](auto absorb_c, auto nt_c, auto cols_c) -> StepKernel<Real> {
		constexpr bool kAbsorb = decltype(absorb_c)::value && kCanAbsorb<MODEL>, kNt = decltype(nt_c)::value;
		constexpr int kCols = decltype(cols_c)::value;
		// (three steps where the model has no such kernel, or not with these columns, or in fp32 with the selects -- the three-step pipeline
		// with them does not fit the registers --, and pairs of the diffusion-only variant: never asked for, steps_per_launch)
		constexpr int kThree = (kCanThreeSteps<Real, MODEL> && kCols == kThreeStepCols<Real, MODEL> && !(sizeof(Real) == 4 && kAbsorb)) ? 3 : 1;
		constexpr int kTwo = kCanTwoSteps<MODEL> ? 2 : 1;
		if constexpr (kThree == 3 && kCanWide<Real, MODEL, kCols, 3> && !kAbsorb)
			if (k.steps == 3 && k.waves == kWideWaves) return crd_rk4_fused_step_kernel<Real, MODEL, false, 0, 1, kNt, 3, kWideWaves>;
		if (k.waves > kMaxWavesPerBlock) return nullptr;  // (choose() and the band cut keep the eight-wide blocks to their own kernel)
		if (k.steps == 3) return crd_rk4_fused_step_kernel<Real, MODEL, kAbsorb, 0, kCols, kNt, kThree>;
		if (k.steps == 2) return crd_rk4_fused_step_kernel<Real, MODEL, kAbsorb, 0, kCols, kNt, kTwo>;
		return crd_rk4_fused_step_kernel<Real, MODEL, kAbsorb, 0, kCols, kNt, 1>;
	};
	auto embedded_nt = [&](auto absorb_c) { return k.nt ? embedded(absorb_c, yes) : embedded(absorb_c, no); };
	auto plain_cols = [&](auto absorb_c, auto nt_c) {
		return k.cols == 2 ? plain(absorb_c, nt_c, std::integral_constant<int, 2>{}) : plain(absorb_c, nt_c, std::integral_constant<int, 1>{});
	};
	auto plain_nt = [&](auto absorb_c) { return k.nt ? plain_cols(absorb_c, yes) : plain_cols(absorb_c, no); };
	if (k.embed != 0) return k.absorb ? embedded_nt(yes) : embedded_nt(no);
	return k.absorb ? plain_nt(yes) : plain_nt(no);
}

// Resident wavefronts, on a device of this node, of the kernel a plan of (cols, steps) runs.  Asked once per kernel; the issuing threads
// of a LOCAL group may arrive together: they are told the same number.
template <typename Real, int MODEL>
int resident_wavefronts(int cols, int steps)
{
	static std::atomic<int> known[2][3];
	steps = (steps == 3 && kCanThreeSteps<Real, MODEL>) ? 3 : (steps == 2 && kCanTwoSteps<MODEL>) ? 2 : 1;  // (the diffusion-only variant has no two-step instantiation)
	cols = steps == 3 ? kThreeStepCols<Real, MODEL> : cols == 2 ? 2 : 1;
	std::atomic<int> &slots = known[cols - 1][steps - 1];
	if (const int v = slots.load(std::memory_order_relaxed)) return v;
	int blocks_per_cu = 4;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, step_kernel<Real, MODEL>({false, 0, cols, false, steps, kMaxWavesPerBlock}), kLanes * kWavesPerBlock, 0) != hipSuccess ||
	    blocks_per_cu < 1)
		blocks_per_cu = 4;
	(void)hipGetLastError();
	slots.store(device_cus() * blocks_per_cu * kWavesPerBlock, std::memory_order_relaxed);
	return slots.load(std::memory_order_relaxed);
}

// ---- one call of the launcher ----------------------------------------------------------------------------------------------------
// The call, the kernel arguments it fills, and the plan's choices as the launch takes them (plan::Choice).  configure() fixes the
// choices and lays the caller's rows out accordingly; the fire_* functions launch.
template <typename Real, int MODEL>
struct FusedLaunch {
	const SlabDesc &d;
	const FusedCall &c;
	hipStream_t st;
	Slab<Real> s;
	FusedArgs<Real> a;
	plan::StepSite site;
	int want[4];       // the caller's rows
	int sw_plain;      // wavefronts per block where the eight-wide kernel does not run
	int cols_default;  // columns per lane where nothing has been measured
	bool absorb1, absorb12;  // absorbing rows on in a stage of the first step / of any step of the launch
	plan::Choice ch;
};

template <typename Real, int MODEL>
void set_io(FusedLaunch<Real, MODEL> &L, const Planes &in, const Planes &out)
{
	L.a.in_u = row0<Real>(in.u, L.d.nx);
	L.a.in_v = row0<Real>(in.v, L.d.nx);
	L.a.out_u = row0<Real>(out.u, L.d.nx);
	L.a.out_v = row0<Real>(out.v, L.d.nx);
}

// Everything of the kernel arguments but the geometry.
template <typename Real, int MODEL>
void fill_args(FusedLaunch<Real, MODEL> &L, int js, int ny)
{
	const FusedCall &c = L.c;
	FusedArgs<Real> &a = L.a;
	set_io(L, c.y0, c.yout);
	const step::Sizes hs(c.dt);
	a.h1 = (Real)hs.h[0];
	a.h2 = (Real)hs.h[1];
	a.h3 = (Real)hs.h[2];
	a.h6 = (Real)hs.h[3];
	for (int k = 0; k < 5; k++) a.absorb[k] = c.absorb[k];
	for (int k = 0; k < 4; k++) a.absorb2[k] = c.absorb2[k];
	for (int k = 0; k < 4; k++) a.absorb3[k] = c.absorb3[k];
	a.js = js;
	a.ny = ny;
	a.err_partials = c.err_partials ? c.err_partials + c.err_offset : nullptr;
	a.err_lo = L.d.wrap ? INT32_MIN : 0;
	a.err_hi = L.d.wrap ? INT32_MAX : L.d.nyl;
	a.rtol = (Real)c.rtol;
	a.atol = (Real)c.atol;
}

// Cuts rows R into items under the launch's choices, in blocks of `sw` wavefronts, into the geometry fields of `a`.
template <typename Real, int MODEL>
void lay_out(const FusedLaunch<Real, MODEL> &L, FusedArgs<Real> &a, const int R[4], int sw, int chunk_override)
{
	const plan::Geometry g = plan::layout(kTraits<Real, MODEL>, resident_wavefronts<Real, MODEL>(L.ch.cols, L.ch.steps), device_cus(), L.d.nx, L.c.embed != 0, R, L.ch, sw, chunk_override);
	a.sw = g.sw;
	a.nstrips = g.nstrips;
	a.chunk = g.chunk;
	a.nchunks = g.nchunks;
	a.first2 = g.first2;
	for (int r = 0; r < 2; r++) a.r_begin[r] = g.r_begin[r], a.r_end[r] = g.r_end[r];
	a.nitems = g.nitems;
	a.nblocks = g.nblocks;
	a.remap = g.remap;
	a.xs_lanes = g.xs_lanes;
}

// The launch's geometry in two layers: configure() fixes the plan's choices, lay_out() cuts rows -- the caller's, or a part of them
// (fire_banded) -- into items accordingly.
template <typename Real, int MODEL>
void configure(FusedLaunch<Real, MODEL> &L, int mode, int remap, int want_cols, int want_nt = 0, int want_steps = 1)
{
	L.ch = plan::choose(kTraits<Real, MODEL>, L.site, L.sw_plain, mode, remap, want_cols, want_nt, want_steps);
	lay_out(L, L.a, L.want, L.ch.sw, 0);
}

// One kernel with arguments `a`; e0 / e1: events bound to its start / its own completion (hipExtLaunchKernel), or null.
template <typename Real, int MODEL>
hipError_t launch_kernel(const FusedLaunch<Real, MODEL> &L, const FusedArgs<Real> &a, const KernelKey &key, hipEvent_t e0, hipEvent_t e1)
{
	const StepKernel<Real> kernel = step_kernel<Real, MODEL>(key);
	if (!kernel) return hipErrorInvalidConfiguration;
	if (e0 || e1) hipExtLaunchKernelGGL(kernel, dim3(a.nblocks), dim3(kLanes * a.sw), 0, L.st, e0, e1, 0, L.s, a);
	else kernel<<<a.nblocks, dim3(kLanes * a.sw), 0, L.st>>>(L.s, a);
	return hipSuccess;
}

// The embedded pairs: the step kernel, and behind it the fixed-order sum of its items' error partials.
template <typename Real, int MODEL>
hipError_t fire_embedded(const FusedLaunch<Real, MODEL> &L)
{
	const FusedCall &c = L.c;
	const FusedArgs<Real> &a = L.a;
	if (!c.err_partials || c.err_capacity < c.err_offset + a.nitems || !c.err_sum) return hipErrorInvalidValue;
	// (the sum deferred to the caller -- another stream, launch_sum_partials: the event is this kernel's own completion)
	if (hipError_t e = launch_kernel(L, a, {L.absorb1, c.embed == 2 ? 2 : 1, 1, L.ch.nt, 1, a.sw}, nullptr, c.err_defer_sum ? c.done_event : nullptr); e != hipSuccess) return e;
	if (c.err_items_out) *c.err_items_out = a.nitems;
	if (c.err_defer_sum) return launch_status();  // (the second launch of a cut attempt sums both launches' partials)
	if (c.done_event) hipExtLaunchKernelGGL(crd_sum_partials_kernel, dim3(1), dim3(256), 0, L.st, nullptr, c.done_event, 0, (const double *)c.err_partials, c.err_offset + a.nitems, c.err_sum);
	else crd_sum_partials_kernel<<<1, 256, 0, L.st>>>(c.err_partials, c.err_offset + a.nitems, c.err_sum);
	return launch_status();
}

// A plain step's kernel over the rows `a` is laid out for.
template <typename Real, int MODEL>
hipError_t launch_rows(const FusedLaunch<Real, MODEL> &L, const FusedArgs<Real> &a, bool with_selects, hipEvent_t e0, hipEvent_t e1)
{
	return launch_kernel(L, a, {with_selects, 0, L.ch.cols, L.ch.nt, L.ch.steps, a.sw}, e0, e1);
}

// Pieces of the band cut, two row ranges to a launch.  The call's start event is bound to the first launch of the first pieces, its done
// event to the last launch of the final ones.
template <typename Real, int MODEL>
hipError_t launch_pieces(const FusedLaunch<Real, MODEL> &L, const int (*piece)[2], int count, bool selects, int item_rows, bool first_pieces, bool final_pieces)
{
	FusedArgs<Real> a = L.a;
	for (int q = 0; q < count; q += 2) {
		const int R[4] = {piece[q][0], piece[q][1], q + 1 < count ? piece[q + 1][0] : 0, q + 1 < count ? piece[q + 1][1] : 0};
		// (the eight-wide block strip has no body with the selects: those launches go out four wide, the select-free ones eight wide)
		lay_out(L, a, R, selects ? L.sw_plain : L.ch.sw, item_rows);
		if (hipError_t e = launch_rows(L, a, selects, (first_pieces && q == 0) ? L.c.start_event : nullptr, (final_pieces && q + 2 >= count) ? L.c.done_event : nullptr); e != hipSuccess)
			return e;
	}
	return hipSuccess;
}

// Several steps per launch with absorbing rows on.
// (Three steps per launch alike: ONE launch of the kernel with the selects -- 246 registers against 244, two wavefronts per
// SIMD either way -- measured 0.2579 ms per step against 0.2180 with the cut and 0.2049 without absorbing rows: it is
// the kernel that holds both bodies that is slow, not its occupancy.)
// Two steps per launch with absorbing rows on.  The ABSORB kernel holds the body with the selects AND the one without
// (it decides per chunk), and the former's scalar registers spill into two vector registers of the whole kernel: 170
// VGPRs, two wavefronts per SIMD instead of three for EVERY item of the launch (+20 ... 38 % measured).  So the rows are
// cut: those whose pipeline can meet a global boundary row -- within 2 kApron rows of rows ny - 1 / 0, a band of 18 --
// go out first as a launch of their own (ABSORB kernel, 3-row items: it is the items' length, not their number, that
// sets such a launch's duration), the rest as launches of the select-free kernel.  Same arithmetic, same bits.
template <typename Real, int MODEL>
hipError_t fire_banded(const FusedLaunch<Real, MODEL> &L)
{
	const plan::BandCut cut = plan::cut_bands(L.want, L.a.js, L.a.ny, L.ch.steps);
	if (!cut.fits || cut.n_with == 0) {
		if (L.ch.sw == L.sw_plain) return launch_rows(L, L.a, true, L.c.start_event, L.c.done_event);
		FusedArgs<Real> a = L.a;
		lay_out(L, a, L.want, L.sw_plain, 0);
		return launch_rows(L, a, true, L.c.start_event, L.c.done_event);
	}
	if (hipError_t e = launch_pieces(L, cut.with_sel, cut.n_with, true, 3, true, cut.n_without == 0); e != hipSuccess) return e;
	return launch_pieces(L, cut.without, cut.n_without, false, 0, false, true);
}

template <typename Real, int MODEL>
hipError_t fire(const FusedLaunch<Real, MODEL> &L)
{
	if (L.c.embed) return fire_embedded(L);
	hipError_t e;
	if (L.ch.steps >= 2 && L.absorb12) e = fire_banded(L);
	else e = launch_rows(L, L.a, L.ch.steps >= 2 ? L.absorb12 : L.absorb1, L.c.start_event, L.c.done_event);
	return e != hipSuccess ? e : launch_status();
}

// ---- the launch-plan measurement -------------------------------------------------------------------------------------------------
struct PlanTimer {
	hipEvent_t e0, e1;
	hipStream_t st;
	bool verbose;
	int nx, rows;
};
// What configuring a candidate came to (for the tuner's report and its liveness rules).
struct Configured {
	bool live;
	int mode, chunk, remap, cols, steps;
	bool nt;
};

// A warm-up launch of the variant at hand, then `reps` launches between two events: their time in ms.
template <typename Fire>
hipError_t time_launches(const PlanTimer &t, Fire &fire, int reps, float *ms)
{
	hipError_t err = fire();
	if (err == hipSuccess) err = hipEventRecord(t.e0, t.st);
	for (int r = 0; err == hipSuccess && r < reps; r++) err = fire();
	if (err == hipSuccess) err = hipEventRecord(t.e1, t.st);
	if (err == hipSuccess) err = hipEventSynchronize(t.e1);
	if (err == hipSuccess) err = hipEventElapsedTime(ms, t.e0, t.e1);
	return err;
}

inline void report_timing(const PlanTimer &t, const char *stage, int round, const Configured &k, float ms, int reps)
{
	if (!t.verbose) return;
	std::fprintf(stderr, "libcrd autotune: %d x %d rows, %s %d, chunk mode %d (%d rows), mapping %d, %d column(s) per lane, %s stores, %d step(s) per launch: %.4f ms per step (%d launches timed)\n",
	             t.nx, t.rows, stage, round, k.mode, k.chunk, k.remap, k.cols, k.nt ? "non-temporal" : "plain", k.steps, ms, reps);
}

// Times the candidates -- configure(k) sets candidate k up and says what became of it, fire() launches what is set up -- and picks one:
// *best_k, with the plain plan's time per step and its own.
// Candidates are timed round-robin, kRounds times, and each keeps its best round: a device's clock drifts while the
// measurement runs (a Goldbeter launch sequence lost 15 % over five candidates timed one after the other), and a
// candidate must not win or lose by its place in the queue.
// Final: with two dozen candidates a few per cent apart, the fastest of the short bursts above is as often the luckiest as
// the best, and a burst runs at clocks a sustained run does not keep.  The plain plan and the three fastest candidates are
// therefore timed again, ~16 ms each and twice round, and the final alone decides between them.
template <typename Configure, typename Fire>
hipError_t tune_plan(const PlanTimer &t, Configure &&configure, Fire &&fire, int *best_k, float *base, float *best)
{
	constexpr int kCandidates = plan::kNumPlanCandidates, kRounds = 3, kFinalists = 4, kFinalRounds = 2;
	hipError_t err = hipSuccess;
	float t_best[kCandidates];
	bool live[kCandidates];
	int reps = 3;
	for (int k = 0; k < kCandidates; k++) {
		t_best[k] = 0.f;
		live[k] = configure(k).live;
	}
	for (int round = 0; round < kRounds && err == hipSuccess; round++)
		for (int k = 0; err == hipSuccess && k < kCandidates; k++) {
			if (!live[k]) continue;
			const Configured cfg = configure(k);
			float ms = 0.f;
			for (int pass = 0; pass < 2 && err == hipSuccess; pass++) {
				err = time_launches(t, fire, reps, &ms);
				if (round > 0 || k > 0 || reps > 3 || ms >= 4.0f || ms <= 0.f) break;
				reps = (int)(12.0f / ms) + 1 < 40 ? (int)(12.0f / ms) + 1 : 40;  // time about four milliseconds' worth per candidate and round, then again
			}
			if (err != hipSuccess) break;
			ms /= (float)(reps * cfg.steps);  // per STEP: a two-step launch does twice the work
			report_timing(t, "round", round, cfg, ms, reps);
			if (t_best[k] == 0.f || ms < t_best[k]) t_best[k] = ms;
		}
	int finalist[kFinalists] = {0, -1, -1, -1};
	for (int f = 1; f < kFinalists; f++)
		for (int k = 1; k < kCandidates; k++) {
			if (!live[k] || t_best[k] <= 0.f || k == finalist[1] || k == finalist[2]) continue;
			if (finalist[f] < 0 || t_best[k] < t_best[finalist[f]]) finalist[f] = k;
		}
	float t_final[kFinalists] = {0.f, 0.f, 0.f, 0.f};
	for (int round = 0; round < kFinalRounds && err == hipSuccess; round++)
		for (int f = 0; err == hipSuccess && f < kFinalists; f++) {
			const int k = finalist[f];
			if (k < 0 || t_best[k] <= 0.f) continue;
			const Configured cfg = configure(k);
			const int reps2 = (int)(16.0f / t_best[k]) + 1 < 400 ? (int)(16.0f / t_best[k]) + 1 : 400;
			float ms = 0.f;
			err = time_launches(t, fire, reps2, &ms);
			if (err != hipSuccess) break;
			ms /= (float)(reps2 * cfg.steps);
			report_timing(t, "final", round, cfg, ms, reps2);
			if (t_final[f] == 0.f || ms < t_final[f]) t_final[f] = ms;
		}
	*best_k = 0;
	*base = *best = t_best[0];
	if (t_final[0] > 0.f) {
		*base = *best = t_final[0];
		for (int f = 1; f < kFinalists; f++)
			if (finalist[f] >= 0 && t_final[f] > 0.f && t_final[f] < *best) {
				*best = t_final[f];
				*best_k = finalist[f];
			}
	}
	return err;
}

// Launch plan: measured once per context on the first full-size launch (a launch reads one plane set and writes another, so
// repeating it is harmless: every candidate writes the same values), then reused for every launch of similar height.
template <typename Real, int MODEL>
hipError_t measure_plan(FusedLaunch<Real, MODEL> &L, FusedPlan *plan)
{
	const FusedCall &c = L.c;
	const int rows = L.want[1] - L.want[0];
	PlanTimer t{nullptr, nullptr, L.st, plan->autotune >= 2 || tuning::verbose(), L.d.nx, rows};
	// (nothing else may run on the device while candidates are timed: a halo exchange still in flight on the second stream
	// made a ring context pick a different -- worse -- plan than a plain slab of the same shape)
	hipError_t err = hipDeviceSynchronize();
	if (err == hipSuccess) err = hipEventCreate(&t.e0);
	if (err == hipSuccess) err = hipEventCreate(&t.e1);
	// What a candidate is timed on: with a scratch plane set, launches that step yout -> scratch -> yout -> ... (each reads what
	// its predecessor wrote, as consecutive steps do); without, repetitions of y0 -> yout.  The difference matters on slabs
	// small enough for the memory-side cache: an input that is never overwritten stays there, and a plan that keeps its output
	// out of the caches (non-temporal stores) then looks better than it steps.
	const bool pingpong = c.tune_scratch.u != nullptr && c.tune_scratch.v != nullptr;
	int flip = 0;
	auto fire_timed = [&L, &c, &flip, pingpong]() -> hipError_t {
		if (pingpong) {
			if (flip) set_io(L, c.tune_scratch, c.yout);
			else set_io(L, c.yout, c.tune_scratch);
			flip ^= 1;
		}
		return fire(L);
	};
	if (pingpong && err == hipSuccess) {
		configure(L, 0, 0, L.cols_default, 0);
		err = fire(L);  // yout holds a state to step on from
	}
	// (a candidate that takes more steps per launch than the call reads more rows beyond the launch's: they must exist -- a launch of
	// a multi-slab cycle that reaches far into the ghost region is measured with the candidates of its own step count only; the caller
	// steps pairs, or triples, once the plan says so)
	int steps_ok = 1;
	for (int n = 2; n <= 3 && c.steps == 1; n++)
		if (steps_ok == n - 1 && plan::steps_per_launch(kTraits<Real, MODEL>, L.site, n) == n && plan::rows_in_reach(L.d.wrap, L.want[0], L.want[1], L.d.nyl, n)) steps_ok = n;
	auto configure_k = [&L, steps_ok, rows](int k) -> Configured {
		const plan::PlanCandidate &p = plan::kPlanCandidates[k];
		configure(L, p.one_round, p.remap, p.cols, p.nt, p.steps);
		const plan::Geometry g{L.a.nstrips, L.a.chunk, L.a.nchunks, L.a.first2, {0, 0}, {0, 0}, L.a.nitems, L.a.nblocks, L.a.remap, L.a.xs_lanes, L.a.sw};
		const int chunk_plain = plan::fused_chunk_rows(resident_wavefronts<Real, MODEL>(L.ch.cols, L.ch.steps), device_cus(), L.a.nstrips, rows, 0, L.ch.steps);
		return {plan::candidate_live(k, kTraits<Real, MODEL>, L.ch, g, chunk_plain, steps_ok), p.one_round, L.a.chunk, L.a.remap, L.ch.cols, L.ch.steps, L.ch.nt};
	};
	int best_k = 0;
	float base = 0.f, best = 0.f;
	if (err == hipSuccess) err = tune_plan(t, configure_k, fire_timed, &best_k, &base, &best);
	if (t.e0) (void)hipEventDestroy(t.e0);
	if (t.e1) (void)hipEventDestroy(t.e1);
	set_io(L, c.y0, c.yout);  // (the launch this call was made for follows)
	if (err != hipSuccess) return err;
	if (best > 0.985f * base) best_k = 0;  // a candidate has to beat the plain plan by more than timing noise
	plan->tuned = 1;
	plan->one_round = plan::kPlanCandidates[best_k].one_round;
	plan->remap = plan::kPlanCandidates[best_k].remap;
	plan->cols = plan::kPlanCandidates[best_k].cols;
	plan->nt = plan::kPlanCandidates[best_k].nt;
	plan->steps = plan::kPlanCandidates[best_k].steps;
	plan->rows = rows;
	plan->ms_default = base;
	plan->ms_best = best_k ? best : base;
	return hipSuccess;
}

// What the configured launch would launch (FusedCall::geometry).
template <typename Real, int MODEL>
void report_geometry(const FusedLaunch<Real, MODEL> &L, FusedGeometry &g)
{
	const FusedArgs<Real> &a = L.a;
	const int cols = L.ch.cols, steps = L.ch.steps, sw = a.sw;
	const int apron = steps * (L.c.embed ? kApron + 1 : kApron);
	g.real_bytes = (int)sizeof(Real);
	g.model = MODEL;
	g.absorb = steps >= 2 ? 0 : (L.absorb1 ? 1 : 0);  // (several steps with absorbing rows on: the bulk goes out as the select-free kernel)
	g.embed = L.c.embed;
	g.cols = cols;
	g.nt = L.ch.nt ? 1 : 0;
	g.steps = steps;
	g.strips = a.nstrips;
	g.chunk_rows = a.chunk;
	g.chunks = a.nchunks;
	g.blocks = a.nblocks;
	g.waves_per_block = sw;
	g.chunk_mode = L.ch.mode;
	g.fill_iterations = 2 * apron;
	g.iterations_per_trip = L.c.embed ? CRD_EMBED_SLOTS : 4;
	g.lanes = kLanes;
	g.lanes_valid = (cols * kLanes - 2 * apron) / cols;
	if (plan::block_is_strip(kTraits<Real, MODEL>, cols, steps)) g.lanes_valid = (sw * kLanes - 2 * apron) / sw;  // the block as the strip: 60 (58) of 64 on average
	g.mapping = a.remap;
	g.wave_iterations = (long)a.nstrips * ((long)(L.want[1] - L.want[0] + L.want[3] - L.want[2]) + (long)a.nchunks * 2 * apron);
}

// The events a caller bound to a launch of no rows are recorded on the stream instead, so that a wait on them sees this call and not an
// earlier one.
inline hipError_t record_events_of_empty_launch(const FusedCall &c, hipStream_t st)
{
	if (c.geometry) return hipSuccess;
	if (c.start_event)
		if (hipError_t e = hipEventRecord(c.start_event, st); e != hipSuccess) return e;
	if (c.done_event)
		if (hipError_t e = hipEventRecord(c.done_event, st); e != hipSuccess) return e;
	return hipSuccess;
}

template <typename Real, int MODEL>
hipError_t launch_fused_t(const SlabDesc &d, const FusedCall &c, int row_begin, int row_end, int row_begin2, int row_end2, int js, int ny,
                          hipStream_t st)
{
	clear_launch_status();
	if (row_end <= row_begin) return record_events_of_empty_launch(c, st);
	if (row_end2 < row_begin2) row_end2 = row_begin2;
	const bool absorb1 = kCanAbsorb<MODEL> && (c.absorb[0] || c.absorb[1] || c.absorb[2] || c.absorb[3] || (c.embed && c.absorb[4]));
	const bool absorb12 = absorb1 || (kCanAbsorb<MODEL> && (c.absorb2[0] || c.absorb2[1] || c.absorb2[2] || c.absorb2[3])) ||
	                      (kCanAbsorb<MODEL> && c.steps == 3 && (c.absorb3[0] || c.absorb3[1] || c.absorb3[2] || c.absorb3[3]));  // (any stage of any step of the launch)
	// (the kernels that address rows by 32-bit offsets into the plane: fused_steps_supported keeps such a launch from being asked for)
	const plan::StepSite site{d.nx, d.nyl, d.wrap != 0, c.embed != 0, fused_scalar_rows_addressable(d.nx, fused_addressed_rows(d), (long)sizeof(Real)), absorb12};
	if (plan::steps_per_launch(kTraits<Real, MODEL>, site, c.steps) != c.steps) return hipErrorInvalidValue;
	if (!plan::rows_in_reach(d.wrap != 0, row_begin, row_end, d.nyl, c.steps)) return hipErrorInvalidValue;
	// two columns per lane need an even nx; where nothing has been measured: the packed arithmetic for fp32, one column for fp64 -- fused_default_columns
	const bool cols2_ok = !c.embed && d.nx % 2 == 0;
	int cols_default = (cols2_ok && sizeof(Real) == 4) ? 2 : 1;
	if (const char *e = tuning::knob("CRD_FUSED_COLS")) cols_default = (std::atoi(e) == 2 && cols2_ok) ? 2 : 1;
	// Four adjacent strips per block marching in lockstep: 0.417 ms on 8192^2 fp64 against 0.441 without the barriers and
	// 0.4205 with one barrier per four iterations (tools/tune_fused.py, interleaved in one process; fp32 0.219 vs 0.232,
	// Goldbeter -- instruction-bound -- unchanged); 2 or 8 strips per block lose half of the gain, 3 / 5 / 6 more.
	int sw_plain = kWavesPerBlock;
	if (const char *e = tuning::knob("CRD_FUSED_STRIPS")) {
		const int v = std::atoi(e);
		if (v >= 1 && v <= kMaxWavesPerBlock) sw_plain = v;
	}
	FusedLaunch<Real, MODEL> L{d, c, st, typed<Real>(d), {}, site, {row_begin, row_end, row_begin2, row_end2}, sw_plain, cols_default, absorb1, absorb12, {}};
	fill_args(L, js, ny);
	const int rows = row_end - row_begin, rows2 = row_end2 - row_begin2;
	FusedPlan *plan = c.plan;
	const bool plannable = plan && rows2 == 0 && (long)rows * d.nx >= (1L << 20) && !tuning::enabled();  // (under CRD_TUNING the knobs decide)
	if (plannable && !plan->tuned && plan->autotune && !c.geometry)
		if (hipError_t e = measure_plan(L, plan); e != hipSuccess) return e;
	// A measured plan applies to the launches it was measured on (heights within a tenth of it: the sweeps of a deep-halo cycle are).
	// Launches it was not measured on -- edge bands, short ranges -- still take its columns per lane: that choice is about the
	// kernel's arithmetic, not about the launch's shape.  A PINNED plan (crd_set_launch_plan) is an instruction, not a measurement:
	// every single-range launch of the context takes all of it, of whatever size (chunk mode and mapping fall back inside configure
	// where the launch is too small for them), two-range launches its columns per lane and store hint.
	const bool pinned = plan && plan->tuned && plan->pinned && !tuning::enabled();
	const bool use_plan = (plannable && plan->tuned && 10L * rows >= 9L * plan->rows && 10L * rows <= 11L * plan->rows) || (pinned && rows2 == 0);
	configure(L, use_plan ? plan->one_round : 0, use_plan ? plan->remap : 0, (plan && plan->tuned) ? plan->cols : cols_default, (use_plan || pinned) ? plan->nt : 0, c.steps);
	if (c.geometry) {
		report_geometry(L, *c.geometry);
		return hipSuccess;
	}
	return fire(L);
}

}  // namespace

// the fp32 half of launch_fused_step (crd_fused_f32.hip)
hipError_t launch_fused_step_f32(const SlabDesc &d, const FusedCall &c, int row_begin, int row_end, int row_begin2, int row_end2, hipStream_t s);

}  // namespace crd
