#pragma once
// crd_fused_impl.h -- the device bodies of the one-launch RK4 step, fused_item and fused_item_multi_step, with the constants and LDS
// sizes they share.  Device code only: the single-slab step kernel around them, its launcher and the launch-plan measurement are
// crd_fused_launch.h's (crd_fused.hip, crd_fused_f32.hip); the ensemble units wrap the same bodies in kernels of their own.
// One classical RK4 step of the whole slab in ONE kernel launch: all four RHS evaluations and the
// stage updates happen on chip, so a grid-point-step costs one read and one write of the state (32 B in fp64) instead
// of the 256 B the four stage kernels of crd_kernels.hip move.  Same arithmetic per point as the staged stepper.
//
// Structure (no LDS, no MFMA; no data passes between wavefronts -- the one barrier per iteration only keeps the four
// wavefronts of a block in step): every WAVEFRONT is an independent work item.  It owns a strip of 64
// consecutive theta columns -- one column per lane, 56 valid outputs in the middle and a 4-column apron on each side
// that is recomputed redundantly -- and marches along phi through a chunk of rows as a 4-deep software pipeline:
//   iteration m:  take row p        (state y0, fetched four iterations earlier)
//                 stage 1 on row p-1 (needs y0 rows p-2..p)          -> y1 row p-1, acc row p-1
//                 stage 2 on row p-2 (needs y1 rows p-3..p-1)        -> y2 row p-2
//                 stage 3 on row p-3 (needs y2 rows p-4..p-2)        -> y3 row p-3
//                 stage 4 on row p-4 (needs y3 rows p-5..p-3)        -> new state row p-4, stored
// The phi neighbours of a row are the lane's own registers from neighbouring iterations; the theta neighbours are the
// adjacent lanes' registers, fetched with DPP wavefront shifts (v_mov_b32_dpp wave_shr:1 / wave_shl:1).  Each stage
// invalidates one more apron column per side, hence 4 + 4 of 64; chunks start 4 rows early and end 4 rows late for the
// same reason in phi (rows come from the slab's ghost rows, or wrap for a single slab).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "crd_device.h"
#include "crd_edge_waits.h"
#include "crd_step.h"
#include "crd_tuning.h"

namespace crd {

namespace {

using namespace dev;

constexpr int kApron = 4;                    // RK4 stages = halo depth
constexpr int kLanes = 64;
constexpr int kValid = kLanes - 2 * kApron;  // 56 output columns per wavefront
constexpr int kWavesPerBlock = 4;     // default; the launch may use 1 .. kMaxWavesPerBlock (tuning knob)
constexpr int kMaxWavesPerBlock = 4;  // (8 strips per workgroup never measured faster than 4 -- with a strip, and an apron, per WAVEFRONT; the one kernel whose block shares ONE apron and is bound by issue, the three-step fp64 block strip, has an eight-wide form: kWideWaves, profiles/r08/block_strip_eight_ab.txt)
// Rows in flight per wavefront (a divisor of the unroll factor, so slots stay static).  Tuning builds override per model.
#ifndef CRD_PREFETCH_FHN
#define CRD_PREFETCH_FHN 4
#endif
#ifndef CRD_PREFETCH_GB
#define CRD_PREFETCH_GB 4
#endif
#ifndef CRD_EMBED_SLOTS
#define CRD_EMBED_SLOTS 6
#endif
#ifndef CRD_PREFETCH_EMBED
#define CRD_PREFETCH_EMBED 3
#endif

// Value held by lane-1 / lane+1 of this wavefront (the edge lane gets 0: it is apron garbage by design).  `old` = 0 with
// bound_ctrl lets the DPP move write its destination without a tied input, i.e. without a copy in front of it.
__device__ __forceinline__ double from_lane_below(double x)
{
	int lo = __double2loint(x), hi = __double2hiint(x);
	lo = __builtin_amdgcn_update_dpp(0, lo, 0x138 /* wave_shr:1 */, 0xf, 0xf, true);
	hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, true);
	return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double from_lane_above(double x)
{
	int lo = __double2loint(x), hi = __double2hiint(x);
	lo = __builtin_amdgcn_update_dpp(0, lo, 0x130 /* wave_shl:1 */, 0xf, 0xf, true);
	hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, true);
	return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float from_lane_below(float x)
{
	const int v = __float_as_int(x);
	return __int_as_float(__builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float from_lane_above(float x)
{
	const int v = __float_as_int(x);
	return __int_as_float(__builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, true));
}
// Two columns per lane, (x, y) = columns (2 lane, 2 lane + 1): the western neighbours of the pair are (lane-1's y, own x), the
// eastern ones (own y, lane+1's x) -- one DPP move per direction for two columns instead of one per column.
template <typename V2>
__device__ __forceinline__ V2 pair_from_below(V2 v)
{
	V2 r;
	r.x = from_lane_below(v.y);
	r.y = v.x;
	return r;
}
template <typename V2>
__device__ __forceinline__ V2 pair_from_above(V2 v)
{
	V2 r;
	r.x = v.y;
	r.y = from_lane_above(v.x);
	return r;
}
__device__ __forceinline__ float2v from_lane_below(float2v v) { return pair_from_below(v); }
__device__ __forceinline__ float2v from_lane_above(float2v v) { return pair_from_above(v); }
__device__ __forceinline__ double2v from_lane_below(double2v v) { return pair_from_below(v); }
__device__ __forceinline__ double2v from_lane_above(double2v v) { return pair_from_above(v); }

// The point function on a lane of the marching wavefront: the theta neighbours are the adjacent lanes.  ONE first difference per
// point, gE = u(lane + 1) - u(lane); the other one, gW = u(lane) - u(lane - 1), is the gE of the lane below, fetched with the second
// shift (crd_device.h: rhs_point).  Edge lanes get apron garbage by design.
template <typename V, int MODEL>
__device__ __forceinline__ void rhs_lane(V uC, V uS, V uN, V v, V cE, V cWn, V cP, typename ScalarOf<V>::type rowp, typename ScalarOf<V>::type ka4, bool zero,
                                         V &du, V &dv)
{
#ifndef CRD_NO_PAIR_SHIFTS_FOLDED  // (experiment switch)
	if constexpr (std::is_same<V, float2v>::value) {
		// Packed fp32, two columns (x, y) per lane (round 6): the shifted PAIRS are never assembled.  pair_from_above / pair_from_below cost a
		// DPP move AND a plain move each (the packed instructions want both halves in one register pair): 100 plain moves per trip of the
		// three-step kernel's 797 vector instructions.  Written per column, the lane shift folds into the instruction that consumes it
		// (VOP2 with a DPP operand): gE.y = shl(u.x) - u.y is one v_sub_f32_dpp, the western term of column x one v_fmac_f32_dpp on gE.y
		// of the lane below, that of column y a plain multiply-add on gE.x.  Same operations on the same operands: same bits.
		V gE;
		gE.x = uC.y - uC.x;
		gE.y = from_lane_above(uC.x) - uC.y;
		rhs_point_west<V, MODEL>(uC, gE, uS, uN, v, cE, cP, rowp, ka4, zero, du, dv, [&](V X) {
			V r;
			r.x = fmadd(cWn.x, from_lane_below(gE.y), X.x);
			r.y = fmadd(cWn.y, gE.x, X.y);
			return r;
		});
		return;
	}
#endif
	const V gE = from_lane_above(uC) - uC;
	rhs_point<V, MODEL>(uC, from_lane_below(gE), gE, uS, uN, v, cE, cWn, cP, rowp, ka4, zero, du, dv);
}

// ---- the BLOCK as the strip (two-step Goldbeter pipeline, fp64; round 5) ----------------------------------------------------------
// The wavefronts of a block hold adjacent runs of 64 columns with ONE apron around all of them -- 240 valid columns of 256 instead of
// 4 x 48 of 4 x 64 -- and a wavefront's edge lanes take their theta neighbour from the wavefront next door through LDS.  Every value
// that is the centre of a later stage is published when it is formed (the lanes' 8 bytes at a per-lane address: lane 0 into its
// wavefront's western slot, lane 63 into the eastern one, the 62 in between into a dump area -- switching them off costs two writes
// of exec per value and measured more than the full-width write), the iteration ends with the block's barrier, and behind it the
// reads of what the neighbours published go out -- they land while the next iteration waits for its row.  Slots are double-buffered
// by the iteration's parity (a wavefront can be one barrier ahead of its neighbour, not two).  The neighbour's value enters the DPP
// shift as its `old` operand (bound_ctrl off: a lane without a source keeps `old`), so no instruction merges it; the western first
// difference of lane 0 is one subtraction more per stage-point.  Same arithmetic per point, same bits.
// What it buys is instructions: (603 / 563) x (48 / 60) = 0.86 of the vector work per useful column; what it costs is the barrier and
// eight LDS writes per iteration, which measured 12 - 15 % of an FHN iteration (150 vector instructions) and half that of a Goldbeter
// one (280).  So: Goldbeter, bound by issue, runs 6 - 8 % faster (4096^2: 0.111 -> 0.102 ms per step); FHN, bound by its memory
// traffic, does not (8192^2 0.2200 -> 0.2195; 4096^2 2 % slower) and keeps a strip per wavefront.
// profiles/r05/block_strip_ab.txt; round 4 tried the same at 173 VGPRs -- two wavefronts per SIMD -- and lost 13 %.
// THREE steps per launch (round 6) run the block as the strip in FHN too: with a strip per wavefront the apron would be 12 columns a
// side, 40 valid lanes of 64; around a block it is 232 of 256.
#if defined(CRD_COOP_ALL)  // (experiment switches: every fp64 one-column multi-step pipeline / none)
template <typename Real, int MODEL, int COLS, int STEPS = 2>
constexpr bool kCoop = sizeof(Real) == 8 && COLS == 1;
#elif defined(CRD_NO_COOP)
template <typename Real, int MODEL, int COLS, int STEPS = 2>
constexpr bool kCoop = false;
#else
template <typename Real, int MODEL, int COLS, int STEPS = 2>
constexpr bool kCoop = sizeof(Real) == 8 && COLS == 1 && (MODEL == CRD_MODEL_GOLDBETER || STEPS == 3);
#endif
// The three-step block strip reads row p + 1 out of its ring slot DURING iteration p (ring_read_ahead below) instead of at the top of
// iteration p + 1, where the wavefront stood still for the reads' LDS latency in front of its first stage -- at two wavefronts per SIMD
// only one other wavefront can cover that: 8192^2 0.2041 -> 0.2005 ms per step, 4096^2 0.0625 -> 0.0618, same bits
// (profiles/r07/ring_read_ahead_ab.txt).  The two-step Goldbeter block strip keeps the read at the top (not measured there).
#if defined(CRD_NO_READ_AHEAD)  // (experiment switch: the row read at the top of its iteration, as in the two-step pipelines)
template <typename Real, int MODEL, int COLS, int STEPS>
constexpr bool kReadAhead = false;
#else
template <typename Real, int MODEL, int COLS, int STEPS>
constexpr bool kReadAhead = kCoop<Real, MODEL, COLS, STEPS> && STEPS == 3;
#endif
// ... and addresses its rows by ONE buffer resource per field and launch -- based at the lowest row a launch can address: row 0 of a
// single slab, the first ghost row elsewhere -- with the row as a 32-bit byte offset in scalar registers, handed to the fills and the
// stores as their scalar offset.  The offsets RUN (one add per row, a select at the periodic seam) where every row used to rebuild a
// 64-bit base and a four-register resource per field; b(j) is read at a running, clamped byte offset likewise, and the fill phase's
// shorter wait is peeled out of the steady-state loop (fused_item_multi_step).  About 50 scalar instructions per iteration down to
// about 25; a wavefront issues one instruction per turn of its SIMD whatever its kind, and at two wavefronts per SIMD behind a barrier
// per iteration nothing covers them (profiles/r10/scalar_rows_ab.txt).  The scalar offset is not part of a raw buffer's range check:
// lanes parked at kStoreNowhere stay dropped.  The host keeps such launches to planes whose addressed span fits 32 bits
// (crd_kernels.h: fused_scalar_rows_addressable).
#if defined(CRD_NO_SCALAR_ROWS)  // (experiment switch: a resource per row, as in the two-step pipelines)
template <typename Real, int MODEL, int COLS, int STEPS>
constexpr bool kScalarRows = false;
#else
template <typename Real, int MODEL, int COLS, int STEPS>
constexpr bool kScalarRows = kReadAhead<Real, MODEL, COLS, STEPS>;
#endif
// ... and takes the neighbours' edge values AS EACH READ LANDS (round 11).  Behind an iteration's barrier every wavefront of the block
// issues its six ds_read_b128 in the same few cycles against the CU's one LDS; one `s_waitcnt lgkmcnt(0)` in front of the iteration's
// first stage held every wavefront until its LAST read was back, though step 0's stages 1 and 2 need only the first.  LDS operations
// return in issue order, so a counted wait retires all but the newest N (crd_edge_waits.h has the counting): 0 = the single wait,
// 1 = two waits (read 0; the rest in front of step 0's stage 3), 2 = one wait per step, 3 = one wait per read, each in front of the
// stage that first needs it.  profiles/r11/edge_ladder_ab.txt has the three measured against the single wait.
// (The probe builds that drop publishes or stages issue other operations than the counts assume: they keep the single wait.)
#if defined(CRD_NO_EDGE_LADDER) || defined(CRD_PROBE_NOPUBLISH) || defined(CRD_PROBE_NOMATH) || defined(CRD_PROBE_HALFMATH)  // (experiment switch: the single wait for all six reads)
#undef CRD_EDGE_LADDER
#define CRD_EDGE_LADDER 0
#elif !defined(CRD_EDGE_LADDER)  // (experiment switch: -DCRD_EDGE_LADDER=1 / 2 / 3)
#define CRD_EDGE_LADDER 3
#endif
template <typename Real, int MODEL, int COLS, int STEPS>
constexpr int kEdgeLadder = kReadAhead<Real, MODEL, COLS, STEPS> ? CRD_EDGE_LADDER : 0;
// The eight-wide block strip (launch-plan chunk mode 3): the three-step fp64 FHN kernel with EIGHT wavefronts around one apron -- 488 valid
// lanes of 512 instead of 232 of 256 -- as the only block of its CU (244 VGPRs: eight wavefronts per CU).
constexpr int kWideWaves = 8;
template <typename Real, int MODEL, int COLS, int STEPS>
constexpr bool kCanWide = sizeof(Real) == 8 && MODEL == CRD_MODEL_FHN && COLS == 1 && STEPS == 3 && kCoop<Real, MODEL, COLS, STEPS>;
// An edge slot holds the 4 STEPS quantities of an iteration (each step's input row and its three stage values): 64 B at two steps,
// 96 of 128 at three.
// (Round 6 tried slots placed on the LDS banks lanes 0 / 63 would have had in the dump area -- lane 63's slot shares its banks with lane
// 48's dump address, SQ_LDS_BANK_CONFLICT 13.5 % of the LDS cycles; the eastern slot is then 8- but not 16-byte aligned and the readers
// need ds_read2_b64, eight LDS cycles each instead of four: the three-step launch 3.8 % SLOWER (0.2040 -> 0.2118 ms per step).  A store's
// cost is the transfer of its operands to the LDS, six cycles whatever the banks do; profiles/r06/three_step_ab.txt.)
template <int STEPS>
constexpr int kEdgeSlotBytes = STEPS == 3 ? 128 : 64;
// (WAVES: the wavefronts of the block -- kMaxWavesPerBlock, or 8 in the eight-wide three-step block strip, kWideWaves below)
template <int STEPS, int WAVES = 4 /* kMaxWavesPerBlock */>
constexpr int kEdgeParityBytes = WAVES * 2 * kEdgeSlotBytes<STEPS>;  // [wavefront][side]
template <int STEPS, int WAVES = 4>
constexpr int kEdgeBytes = 2 * kEdgeParityBytes<STEPS, WAVES>;       // [parity]
template <int STEPS, int WAVES = 4>
constexpr int kEdgeDumpBytes = WAVES * 64 * 8 + kEdgeBytes<STEPS, WAVES>;  // where the lanes in between drop their values (+ the largest slot offset)
__device__ __forceinline__ double from_lane_below_old(double x, double old)
{
	int lo = __double2loint(x), hi = __double2hiint(x);
	lo = __builtin_amdgcn_update_dpp(__double2loint(old), lo, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
	hi = __builtin_amdgcn_update_dpp(__double2hiint(old), hi, 0x138, 0xf, 0xf, false);
	return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double from_lane_above_old(double x, double old)
{
	int lo = __double2loint(x), hi = __double2hiint(x);
	lo = __builtin_amdgcn_update_dpp(__double2loint(old), lo, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
	hi = __builtin_amdgcn_update_dpp(__double2hiint(old), hi, 0x130, 0xf, 0xf, false);
	return __hiloint2double(hi, lo);
}
// X: lane 63 holds the eastern neighbour wavefront's value of lane 0, lane 0 the western one's value of lane 63 (other lanes: anything)
template <int MODEL>
__device__ __forceinline__ void rhs_lane_edge(double uC, double X, double uS, double uN, double v, double cE, double cWn, double cP, double rowp, double ka4, bool zero,
                                              double &du, double &dv)
{
	const double t = uC - X;  // lane 0: its western first difference
	const double gE = from_lane_above_old(uC, X) - uC;
	rhs_point<double, MODEL>(uC, from_lane_below_old(gE, t), gE, uS, uN, v, cE, cWn, cP, rowp, ka4, zero, du, dv);
}
template <int OFF>
__device__ __forceinline__ void edge_publish(unsigned pub, double val)
{
#ifndef CRD_PROBE_NOPUBLISH  // (probe build: what the publishes cost -- results are wrong without them)
	asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(pub), "v"(val), "n"(OFF) : "memory");
#endif
}
typedef double double2r __attribute__((ext_vector_type(2)));
#ifdef CRD_PROBE_NOBARRIER  // (probe build: what the iteration's barrier costs -- results are wrong without it)
#define CRD_EDGE_BARRIER "s_nop 0"
#else
#define CRD_EDGE_BARRIER "s_barrier"
#endif
constexpr unsigned long kEdgeLanes = 0x8000000000000001ul;  // exec mask: lanes 0 and 63
// The barrier of an iteration (this wavefront's own publishes have landed: lgkmcnt(0)), and behind it the reads -- issued, not waited
// for: ring_read_with_edges does that -- of the 4 STEPS quantities the neighbours published during it: 16 N bytes from OFF on, into
// lanes 0 and 63.
template <int OFF>
__device__ __forceinline__ void edge_exchange(unsigned con, double2r (&e)[4])
{
	asm volatile("s_waitcnt lgkmcnt(0)\n\t" CRD_EDGE_BARRIER "\n\ts_mov_b64 exec, %5\n\tds_read_b128 %0, %4 offset:%6\n\tds_read_b128 %1, %4 offset:%7\n\t"
	             "ds_read_b128 %2, %4 offset:%8\n\tds_read_b128 %3, %4 offset:%9\n\ts_mov_b64 exec, -1"
	             : "=&v"(e[0]), "=&v"(e[1]), "=&v"(e[2]), "=&v"(e[3]) : "v"(con), "s"(kEdgeLanes), "n"(OFF), "n"(OFF + 16), "n"(OFF + 32), "n"(OFF + 48) : "memory");
}
template <int OFF>
__device__ __forceinline__ void edge_exchange(unsigned con, double2r (&e)[6])
{
	asm volatile("s_waitcnt lgkmcnt(0)\n\t" CRD_EDGE_BARRIER "\n\ts_mov_b64 exec, %7\n\tds_read_b128 %0, %6 offset:%8\n\tds_read_b128 %1, %6 offset:%9\n\t"
	             "ds_read_b128 %2, %6 offset:%10\n\tds_read_b128 %3, %6 offset:%11\n\tds_read_b128 %4, %6 offset:%12\n\tds_read_b128 %5, %6 offset:%13\n\t"
	             "s_mov_b64 exec, -1"
	             : "=&v"(e[0]), "=&v"(e[1]), "=&v"(e[2]), "=&v"(e[3]), "=&v"(e[4]), "=&v"(e[5])
	             : "v"(con), "s"(kEdgeLanes), "n"(OFF), "n"(OFF + 16), "n"(OFF + 32), "n"(OFF + 48), "n"(OFF + 64), "n"(OFF + 80)
	             : "memory");
}
// ... of the read-ahead form (kReadAhead above): the wait in front of the barrier is also what retires the read of the NEXT row, issued
// earlier in the same iteration (ring_read_ahead).  The row's registers are operands of THIS statement, so that they are tied to the place
// where they land: behind it the next iteration publishes the row and starts its fill at once, while the edge reads are still in flight.
template <int OFF>
__device__ __forceinline__ void edge_exchange(unsigned con, double2r (&e)[6], double &u, double &v)
{
	asm volatile("s_waitcnt lgkmcnt(0)\n\t" CRD_EDGE_BARRIER "\n\ts_mov_b64 exec, %9\n\tds_read_b128 %0, %8 offset:%10\n\tds_read_b128 %1, %8 offset:%11\n\t"
	             "ds_read_b128 %2, %8 offset:%12\n\tds_read_b128 %3, %8 offset:%13\n\tds_read_b128 %4, %8 offset:%14\n\tds_read_b128 %5, %8 offset:%15\n\t"
	             "s_mov_b64 exec, -1"
	             : "=&v"(e[0]), "=&v"(e[1]), "=&v"(e[2]), "=&v"(e[3]), "=&v"(e[4]), "=&v"(e[5]), "+v"(u), "+v"(v)
	             : "v"(con), "s"(kEdgeLanes), "n"(OFF), "n"(OFF + 16), "n"(OFF + 32), "n"(OFF + 48), "n"(OFF + 64), "n"(OFF + 80)
	             : "memory");
}

// f(integral_constant<int, 0>{}), f(integral_constant<int, 1>{}), ... in order: a compile-time unrolled loop.
template <typename F, int... Is>
__device__ __forceinline__ void for_sequence(F &&f, std::integer_sequence<int, Is...>)
{
	(f(std::integral_constant<int, Is>{}), ...);
}

// row base (uniform) + this lane's byte offset
template <typename T>
__device__ __forceinline__ T *at_lane(T *row, unsigned byte_offset)
{
	using Bytes = std::conditional_t<std::is_const<T>::value, const char, char>;
	// (the empty asm keeps the compiler from hoisting `constant pointer + lane offset` out of the row loop as a 64-bit vector
	// base, which would cost a 64-bit vector add per access to put the row offset back in)
	asm volatile("" : "+v"(byte_offset));
	return reinterpret_cast<T *>(reinterpret_cast<Bytes *>(row) + byte_offset);
}

// ... the same address as a pointer to the lane's value (one Real, or two adjacent ones: an 8- or 16-byte access)
template <typename V, typename T>
__device__ __forceinline__ auto at_lane_as(T *row, unsigned byte_offset)
{
	using P = std::conditional_t<std::is_const<T>::value, const V, V>;
	return reinterpret_cast<P *>(at_lane(row, byte_offset));
}

// a lane's value(s) added up in double
__device__ __forceinline__ double lane_total(double x) { return x; }
__device__ __forceinline__ double lane_total(float x) { return (double)x; }
template <typename V2>
__device__ __forceinline__ double lane_total(V2 v)
{
	return (double)v.x + (double)v.y;
}

// A value known to be identical in every lane, moved to scalar registers.
__device__ __forceinline__ double uniform(double x)
{
	return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
__device__ __forceinline__ float uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

// (non-temporal row loads measured 19 % slower, fp64 and fp32 alike: the apron rows and columns two items share come from cache)
#define CRD_ROW_LOAD(p) (*(p))
// The new state is written once and not read again by this launch.  NT = true gives its stores the non-temporal hint
// (`global_store ... nt`): the lines do not stay in L2 at the expense of the apron rows and columns neighbouring items share --
// a launch-plan choice (FusedPlan::nt), measured like the others: -6.5 % on 8192^2 fp64 under the plain mapping, -8 % at 4096^2,
// +1 % on some two-column plans (profiles/r03/nt_stores.txt).
template <bool NT, typename T>
__device__ __forceinline__ void row_store(T *p, T v)
{
	if constexpr (NT) __builtin_nontemporal_store(v, p);
	else *p = v;
}

template <typename Real>
struct FusedArgs {
	const Real *in_u, *in_v;  // y0, pointers to local row 0 (ghost rows at negative offsets)
	Real *out_u, *out_v;      // new state, local row 0
	Real h2, h3, h6, h1;      // dt/2, dt/3, dt/6, dt
	int absorb[5];            // t_stage < tBoundary for the four stages (+ the embedded pair's fifth)
	int absorb2[4];           // two steps per launch: the second step's stages
	int absorb3[4];           // three: the third's
	int js, ny;               // global index of local row 0, global row count (absorbing rule is by global row)
	// Rows this launch produces: one or two ranges, cut into work items ("chunks") of `chunk` rows; chunk ids run through the
	// ranges in order (range 1 starts at id `first2`).  One range: an ordinary sweep.  Two: the rows of a step that read ghost
	// rows, below and above the slab, or the two edge bands of a cycle's last step.
	int r_begin[2], r_end[2], chunk, first2;
	int nstrips, nitems, nblocks, remap;
	int xs_lanes;             // remap 2: phi-lanes of chunk sequences per strip block and XCD
	int nchunks;              // chunks of both ranges
	int sw;                   // wavefronts per block = adjacent strips a block covers
	double *err_partials;     // EMBED: one weighted square sum per work item
	Real rtol, atol;          // EMBED: error weights 1 / (rtol |y_n| + atol)
	int err_lo, err_hi;       // EMBED: rows whose error counts (a multi-slab attempt also produces ghost-region rows: the owner counts those)
};

// EMBED adds a fifth pipeline stage and with it a local error estimate whose weighted square sum
//   sum_i (err_i / (rtol |y_n,i| + atol))^2
// over this work item's outputs is written to err_partials[item] (ARKode's WRMS norm, src/FHNmodel_torus.cpp:365, is
// sqrt(sum / N)).  The propagated solution is classical RK4 either way.  The pipeline is then five rows / columns deep
// (apron 5, 54 valid lanes) and uses 6 register slots per array, the loop being unrolled 6 times.
//   EMBED = 1  the RK4(3) pair of rounds 1-2: k5 = f(t + dt, y_new), yhat = y + dt (k1/6 + k2/3 + k3/3 + k5/6), err = dt (k4 - k5)/6.
//   EMBED = 2  ARKode's default fourth-order explicit table, Zonneveld 5(3)4 (what the reference integrates with,
//              src/FHNmodel_torus.cpp:356-372; table and order conditions in oracle/arkode_erk.py): the fifth stage is
//              k5 = f(t + 3/4 dt, y + dt (5/32 k1 + 7/32 k2 + 13/32 k3 - 1/32 k4)) and
//              err = y_new - yhat = dt (2/3 k1 - 2 k2 - 2 k3 - 2 k4 + 16/3 k5).
//              No accumulators in this variant: when stage 4 of a row runs, the row's stage values y1 = y + dt/2 k1,
//              y2 = y + dt/2 k2, y3 = y + dt k3 are still in their register slots (six rows deep), so with
//              d_i = y_i - y the three combinations the row needs come out of d1, d2, d3 and dt k4 there and then,
//                y_new = y + (d1 + 2 d2 + d3)/3 + dt k4/6,   z5 = y + 5/16 d1 + 7/16 d2 + 13/32 d3 - dt k4/32,
//                e4 = 4/3 d1 - 4 d2 - 2 d3 - 2 dt k4        (err = e4 + 16/3 dt k5 one iteration later);
//              the subtractions are exact (y_i is within a factor 2 of y wherever it matters), so what this costs against running
//              sums is a rounding of y_i itself, 1e-16 |y| in quantities that are compared with rtol |y| + atol.
// COLS = 2: two adjacent grid columns per lane -- a wavefront's strip is 128 columns, 120 valid (the apron is two whole lanes a
// side), rows are read and written with one 8-byte (fp32) or 16-byte (fp64) access per lane, a stage needs ONE DPP move per
// direction for two columns, and the fp32 arithmetic is the packed instructions (v_pk_fma_f32 ...).  Needs an even nx (the
// pair must not straddle the periodic seam); results are the one-column kernel's bit for bit.
// NT = true: the new state is stored with the non-temporal hint (row_store above).
// One work item: strip `strip` (a wavefront's columns) of chunk `chunk` (its rows).  ABSORB as a template argument of the ITEM: a
// launch some stage of which has t < tBoundary runs the selects only in the items whose rows (aprons included) contain a global
// phi boundary row -- two chunks per boundary of a launch; every other item runs the body without them (the kernel below decides
// per chunk, uniformly for the block).  With the selects in every item the absorbing-rows run cost 5.4 % at 8192^2 (round 3).
template <typename Real, int MODEL, bool ABSORB, int EMBED, int COLS, bool NT>
__device__ __forceinline__ void fused_item(const Slab<Real> &s, const FusedArgs<Real> &a, const int strip, const int chunk)
{
	static_assert(COLS == 1 || (COLS == 2 && EMBED == 0), "the embedded pairs run one column per lane");
	using V = typename LaneValue<Real, COLS>::type;
	constexpr bool ZONN = EMBED == 2;
	constexpr int APRON = EMBED != 0 ? kApron + 1 : kApron;
	static_assert(APRON % COLS == 0, "the apron is whole lanes");
	constexpr int VALID = COLS * kLanes - 2 * APRON;
	// Register slots per pipeline array = unroll factor: the rows alive at once (4, or 6 with the fifth stage) -- even, because
	// the two-deep arrays below are addressed with the slot's parity.
	constexpr int M = EMBED != 0 ? CRD_EMBED_SLOTS : 4;
	static_assert(M % 2 == 0 && M >= (EMBED != 0 ? 6 : 4) && (EMBED != 2 || M % 3 == 0), "slot count");
	constexpr int kPrefetch = EMBED != 0 ? ((MODEL == CRD_MODEL_GOLDBETER && sizeof(Real) == 8) ? 2 : CRD_PREFETCH_EMBED) : (MODEL == CRD_MODEL_GOLDBETER) ? CRD_PREFETCH_GB : CRD_PREFETCH_FHN;
	static_assert(M % kPrefetch == 0, "prefetch slots are addressed with the unrolled iteration index");
	const int lane = threadIdx.x & (kLanes - 1);
	const int item = chunk * a.nstrips + strip;
	const int nx = s.nx;

	int x = strip * VALID - APRON + COLS * lane;  // this lane's (first) column, wrapped periodically (nx may be smaller than a strip)
	x %= nx;
	if (x < 0) x += nx;
	// lane offsets in bytes, unsigned 32-bit: with a scalar row base the accesses take the `global_load v, v_off, s[base]` form and
	// no 64-bit vector add is spent per access
	const unsigned xb = (unsigned)x * (unsigned)sizeof(Real);  // (a lane that stores has x == out_col: its column is inside [0, nx) unwrapped, so xb serves the stores too)
	const int out_col = strip * VALID + (COLS * lane - APRON);
	const bool lane_stores = COLS * lane >= APRON && COLS * lane < COLS * kLanes - APRON && out_col < nx;  // (two columns: nx is even, so is out_col)

	const int range = chunk >= a.first2 ? 1 : 0;  // (an unused second range starts at nchunks)
	const int range_end = a.r_end[range];
	const int j0 = a.r_begin[range] + (chunk - (range ? a.first2 : 0)) * a.chunk;
	const int j1 = (j0 + a.chunk < range_end) ? j0 + a.chunk : range_end;
	const int jbase = j0 - APRON;
	const int niter = (j1 - j0) + 2 * APRON;
	const int jlast = j1 + APRON - 1;  // last row the pipeline consumes

	const V cE = *reinterpret_cast<const V *>(s.cE + x), cWn = *reinterpret_cast<const V *>(s.cWn + x), cP = *reinterpret_cast<const V *>(s.cP + x);
	const Real ka4 = s.ka4;
	const V h1 = (V)a.h1, h2 = (V)a.h2, h3 = (V)a.h3, h6 = (V)a.h6;
	// b(j) is read-only for the whole launch and its index is uniform: through the constant address space the reads become
	// scalar-cache loads into SGPRs (s_load_dwordx2), no vector registers and no vector-memory instruction
	const __attribute__((address_space(4))) Real *const brow = (const __attribute__((address_space(4))) Real *)(s.brow);

	// Row base pointers are scalar; a single slab wraps rows outside [0, nyl).  Branch-free: this runs once per pipeline
	// iteration in every wavefront's instruction stream (scalar work is not free: ~40 of the ~140 instructions of an iteration
	// were scalar before the row bookkeeping was pared down).
	const int wrap_nyl = s.wrap ? s.nyl : 0;
	auto row_base = [&](int j) -> ptrdiff_t {
		j += wrap_nyl & (j >> 31);
		j -= (j >= s.nyl) ? wrap_nyl : 0;
		return (ptrdiff_t)j * nx;
	};
	// Global phi boundary rows (src/FHNmodel_torus.cpp:643-653), also when they are recomputed as another slab's ghost rows.
	auto boundary_row = [&](int j) -> bool {
		int gj = a.js + j;
		if (gj < 0) gj += a.ny;
		else if (gj >= a.ny) gj -= a.ny;
		return gj == 0 || gj == a.ny - 1;
	};

	// Pipeline registers.  Row jbase+m of an array lives in slot m mod M (m & 1 for the two-deep v arrays), so with the
	// loop unrolled M times every access has a compile-time slot and no value is ever moved between registers.
	// (Zonneveld variant: the local field's stage values stay until the row's stage 4 has used them -- y1 four rows, y2 three)
	constexpr int NV1 = ZONN ? M : 2, NV2 = ZONN ? 3 : 2;
	V u0[M], v0[M], U1[M], U2[M], U3[M], V1[NV1], V2[NV2], V3[2], aU[M], aV[M];
	// (Keeping aU / aV in LDS instead -- 90 VGPRs, five wavefronts per SIMD -- measured 3-5 % SLOWER on every grid: the twelve LDS
	// accesses per iteration cost more than the fifth wavefront brings.)
#define ACC_U(S) aU[S]
#define ACC_V(S) aV[S]
	V U4[M], V4[2], K4U[2], K4V[2];  // EMBED 1: y_new window and k4 of the last two rows; EMBED 2: z5 window (three rows deep) and e4
	const V zero_v = splat<V>(0.0);
	V err2 = zero_v;
#pragma unroll
	for (int k = 0; k < M; k++) u0[k] = v0[k] = U1[k] = U2[k] = U3[k] = aU[k] = aV[k] = U4[k] = zero_v;
#pragma unroll
	for (int k = 0; k < NV1; k++) V1[k] = zero_v;
#pragma unroll
	for (int k = 0; k < NV2; k++) V2[k] = zero_v;
	V3[0] = V3[1] = V4[0] = V4[1] = K4U[0] = K4U[1] = K4V[0] = K4V[1] = zero_v;

	// Rows are fetched kPrefetch iterations before they enter the pipeline: with ~16 wavefronts per CU one row in flight
	// per wavefront is far too little to cover HBM latency (Little's law), four rows (8 loads, 4 KiB per wavefront) is enough.
	// The per-row reaction parameter b(j) rides along: a plain `s.brow[c]` at the point of use is a VECTOR load whose
	// full latency the stage then waits for (four exposed L2 round trips per iteration, 60 % of the wave's lifetime when
	// measured); fetched with the row and moved to scalar registers on arrival it costs nothing.
	V pu[kPrefetch], pv[kPrefetch];
	Real pb[kPrefetch], bq[M];
#pragma unroll
	for (int k = 0; k < kPrefetch; k++) {
		const int jr = (jbase + k < jlast) ? jbase + k : jlast;
		const ptrdiff_t rb = row_base(jr);
		pu[k] = CRD_ROW_LOAD(at_lane_as<V>(a.in_u + rb, xb));
		pv[k] = CRD_ROW_LOAD(at_lane_as<V>(a.in_v + rb, xb));
		pb[k] = brow[jr];
	}
#pragma unroll
	for (int k = 0; k < M; k++) bq[k] = (Real)0;
	// running scalars of the row loop: the row the next prefetch takes (the tail re-reads the last valid row instead of running
	// past the plane) and the output rows of stage 4 (row jbase + m - 4 at iteration m)
	int jn = (jbase + kPrefetch < jlast) ? jbase + kPrefetch : jlast;
	Real *out_row_u = a.out_u + (ptrdiff_t)(jbase - 4) * nx, *out_row_v = a.out_v + (ptrdiff_t)(jbase - 4) * nx;

	// One pipeline iteration at m == K (mod M).  GUARDED: the first iterations of a chunk, where stage k's inputs exist only
	// from iteration 2k on.
	auto iteration = [&](int m, auto kk, auto guarded) {
		constexpr int K = decltype(kk)::value;
		constexpr bool GUARDED = decltype(guarded)::value;
#ifndef CRD_NO_LOCKSTEP  // (an experiment switch: -DCRD_NO_LOCKSTEP lets a block's wavefronts drift)
		__builtin_amdgcn_s_barrier();  // lockstep; uniform over the block: its wavefronts share the chunk, hence niter
#endif
		// slots of rows p, p-1, ... p-6 (with M = 4, row p-4 shares its slot with row p)
		constexpr int S0 = K % M, S1 = (K + M - 1) % M, S2 = (K + M - 2) % M, S3 = (K + M - 3) % M, S4 = (K + 2 * M - 4) % M;
		constexpr int S5 = (K + 2 * M - 5) % M, S6 = (K + 2 * M - 6) % M;
		// slots of the local field's stage values (two deep; in the Zonneveld variant as deep as they have to live) and of the z5 window
		constexpr int A1 = ZONN ? S1 : (S1 & 1), A2 = ZONN ? S2 : (S2 & 1), A4 = ZONN ? S4 : (S4 & 1);              // y1 rows p-1, p-2, p-4
		constexpr int B2 = ZONN ? S2 % 3 : (S2 & 1), B3 = ZONN ? S3 % 3 : (S3 & 1), B4 = ZONN ? S4 % 3 : (S4 & 1);  // y2 rows p-2, p-3, p-4
		constexpr int Z4 = ZONN ? S4 % 3 : S4, Z5 = ZONN ? S5 % 3 : S5, Z6 = ZONN ? S6 % 3 : S6;                    // z5 / y_new rows p-4, p-5, p-6
		constexpr int P = K % kPrefetch;
		const int p = jbase + m;
		const Real b4 = bq[S4];  // b of row p-4 (stage 4), read before row p takes over the slot when M = 4
		u0[S0] = pu[P];
		v0[S0] = pv[P];
		bq[S0] = uniform(pb[P]);
		{
			const ptrdiff_t rb = row_base(jn);
			pu[P] = CRD_ROW_LOAD(at_lane_as<V>(a.in_u + rb, xb));
			pv[P] = CRD_ROW_LOAD(at_lane_as<V>(a.in_v + rb, xb));
			pb[P] = brow[jn];
			jn = (jn < jlast) ? jn + 1 : jlast;
		}
		V du, dv;
		// ---- stage 1, centre row p-1: y0 rows p-2, p-1, p -----------------------------------------------------
		if (!GUARDED || m >= 2) {
			const int c = p - 1;
			rhs_lane<V, MODEL>(u0[S1], u0[S2], u0[S0], v0[S1], cE, cWn, cP, bq[S1], ka4,
			                       ABSORB && a.absorb[0] && boundary_row(c), du, dv);
			U1[S1] = fmadd(h2, du, u0[S1]);
			V1[A1] = fmadd(h2, dv, v0[S1]);
			if (!ZONN) {
				ACC_U(S1) = fmadd(h6, du, u0[S1]);
				ACC_V(S1) = fmadd(h6, dv, v0[S1]);
			}
		}
		// ---- stage 2, centre row p-2: y1 rows p-3, p-2, p-1 ---------------------------------------------------
		if (!GUARDED || m >= 4) {
			const int c = p - 2;
			rhs_lane<V, MODEL>(U1[S2], U1[S3], U1[S1], V1[A2], cE, cWn, cP, bq[S2], ka4,
			                       ABSORB && a.absorb[1] && boundary_row(c), du, dv);
			U2[S2] = fmadd(h2, du, u0[S2]);
			V2[B2] = fmadd(h2, dv, v0[S2]);
			if (!ZONN) {
				ACC_U(S2) = fmadd(h3, du, ACC_U(S2));
				ACC_V(S2) = fmadd(h3, dv, ACC_V(S2));
			}
		}
		// ---- stage 3, centre row p-3: y2 rows p-4, p-3, p-2 ---------------------------------------------------
		if (!GUARDED || m >= 6) {
			const int c = p - 3;
			rhs_lane<V, MODEL>(U2[S3], U2[S4], U2[S2], V2[B3], cE, cWn, cP, bq[S3], ka4,
			                       ABSORB && a.absorb[2] && boundary_row(c), du, dv);
			U3[S3] = fmadd(h1, du, u0[S3]);
			V3[S3 & 1] = fmadd(h1, dv, v0[S3]);
			if (!ZONN) {
				ACC_U(S3) = fmadd(h3, du, ACC_U(S3));
				ACC_V(S3) = fmadd(h3, dv, ACC_V(S3));
			}
		}
		// ---- stage 4, centre row p-4: y3 rows p-5, p-4, p-3 -> the new state ----------------------------------
		if (!GUARDED || m >= 8) {
			const int c = p - 4;
			rhs_lane<V, MODEL>(U3[S4], U3[S5], U3[S3], V3[S4 & 1], cE, cWn, cP, b4, ka4,
			                       ABSORB && a.absorb[3] && boundary_row(c), du, dv);
			V nu, nv;
			if (ZONN) {
				// everything the row still needs, from its stage values (see the kernel's header comment)
				const V yu = u0[S4], yv = v0[S4];
				const V d1u = U1[S4] - yu, d2u = U2[S4] - yu, d3u = U3[S4] - yu, d1v = V1[A4] - yv, d2v = V2[B4] - yv, d3v = V3[S4 & 1] - yv;
				nu = fmadd(splat<V>(1.0 / 3.0), fmadd(splat<V>(2.0), d2u, d1u + d3u), fmadd(h6, du, yu));
				nv = fmadd(splat<V>(1.0 / 3.0), fmadd(splat<V>(2.0), d2v, d1v + d3v), fmadd(h6, dv, yv));
				const V h32 = splat<V>(-1.0 / 32.0) * h1, h2m = splat<V>(-2.0) * h1;
				U4[Z4] = fmadd(splat<V>(5.0 / 16.0), d1u, fmadd(splat<V>(7.0 / 16.0), d2u, fmadd(splat<V>(13.0 / 32.0), d3u, fmadd(h32, du, yu))));
				V4[S4 & 1] = fmadd(splat<V>(5.0 / 16.0), d1v, fmadd(splat<V>(7.0 / 16.0), d2v, fmadd(splat<V>(13.0 / 32.0), d3v, fmadd(h32, dv, yv))));
				K4U[S4 & 1] = fmadd(splat<V>(4.0 / 3.0), d1u, fmadd(splat<V>(-4.0), d2u, fmadd(splat<V>(-2.0), d3u, h2m * du)));
				K4V[S4 & 1] = fmadd(splat<V>(4.0 / 3.0), d1v, fmadd(splat<V>(-4.0), d2v, fmadd(splat<V>(-2.0), d3v, h2m * dv)));
			} else {
				nu = fmadd(h6, du, ACC_U(S4));
				nv = fmadd(h6, dv, ACC_V(S4));
			}
			// Without the fifth stage rows j0 <= c < j1 are exactly iterations 8 .. niter-1; with it (one more apron row each side)
			// the first and the last iteration of the range fall outside.
			if ((EMBED == 0 || (c >= j0 && c < j1)) && lane_stores) {
				row_store<NT>(at_lane_as<V>(out_row_u, xb), nu);
				row_store<NT>(at_lane_as<V>(out_row_v, xb), nv);
			}
			if (EMBED == 1) {
				U4[S4] = nu;
				V4[S4 & 1] = nv;
				K4U[S4 & 1] = du;
				K4V[S4 & 1] = dv;
			}
		}
		// ---- stage 5 (EMBED), centre row p-5: y_new rows p-6, p-5, p-4 -> k5 and the error of row p-5 ----------
		if (EMBED != 0 && (!GUARDED || m >= 10)) {
			const int c = p - 5;
			rhs_lane<V, MODEL>(U4[Z5], U4[Z6], U4[Z4], V4[S5 & 1], cE, cWn, cP, bq[S5], ka4,
			                       ABSORB && a.absorb[4] && boundary_row(c), du, dv);  // k5 at t + dt like k4 (EMBED 1) or at t + 3/4 dt (Zonneveld)
			if (lane_stores && c >= a.err_lo && c < a.err_hi) {  // rows j0 .. j1-1 exactly (stage 5 starts at iteration 10, row j0, and the loop ends at row j1-1), owned rows only
				const V au = __builtin_elementwise_abs(u0[S5]), av = __builtin_elementwise_abs(v0[S5]);
				const V wu = fmadd((V)a.rtol, au, (V)a.atol), wv = fmadd((V)a.rtol, av, (V)a.atol);
				V eu, ev;
				if (ZONN) {
					const V h163 = splat<V>(16.0 / 3.0) * h1;
					eu = fmadd(h163, du, K4U[S5 & 1]) / wu;
					ev = fmadd(h163, dv, K4V[S5 & 1]) / wv;
				} else {
					eu = h6 * (K4U[S5 & 1] - du) / wu;
					ev = h6 * (K4V[S5 & 1] - dv) / wv;
				}
				err2 = fmadd(eu, eu, fmadd(ev, ev, err2));
			}
		}
		out_row_u += nx;
		out_row_v += nx;
	};
	using std::integral_constant;
	// guarded prologue: up to the first multiple of M at or beyond 2 * APRON, so the steady-state loop starts at slot 0
	constexpr int PRO = ((2 * APRON + M - 1) / M) * M;
	for_sequence(
	    [&](auto k) {
		    constexpr int I = decltype(k)::value;
		    if (I < niter) iteration(I, integral_constant<int, I % M>{}, std::true_type{});
	    },
	    std::make_integer_sequence<int, PRO>{});
	int m = PRO;
	for (; m + M - 1 < niter; m += M)  // steady state: M iterations per trip, every register slot a compile-time constant
		for_sequence([&](auto k) { iteration(m + decltype(k)::value, k, std::false_type{}); }, std::make_integer_sequence<int, M>{});
	for_sequence(
	    [&](auto k) {
		    if (m + decltype(k)::value < niter) iteration(m + decltype(k)::value, k, std::false_type{});
	    },
	    std::make_integer_sequence<int, M - 1>{});
	if constexpr (EMBED != 0) {
		// wavefront sum in a fixed order (butterfly over lane distances 32 .. 1), one partial per work item: the host-side
		// reduction adds them in item order, so the norm is reproducible run to run
		double sum = lane_total(err2);
		for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
		if (lane == 0) a.err_partials[item] = sum;
	}
}

// y + h k of the stage updates as the three-address v_fma_f64, spelled out: left to itself the compiler forms a third of them as
// v_mov_b64 + v_fmac_f64 (the addend is still needed, and its two-address form wants it in the destination) -- ten moves per iteration
// of the two-step pipeline, 7 % of its vector instructions.  Same operation, same rounding.
#ifndef CRD_NO_ASM_FMA
__device__ __forceinline__ double stage_fma(double h, double k, double y)
{
	double d;
	asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "s"(h), "v"(k), "v"(y));
	return d;
}
#else
__device__ __forceinline__ double stage_fma(double h, double k, double y) { return fmadd(h, k, y); }
#endif
template <typename V>
__device__ __forceinline__ V stage_fma(V h, V k, V y)
{
	return fmadd(h, k, y);
}

// ---- the two-step pipeline's memory path (round 5) ----------------------------------------------------------------------------
// Rows enter through LDS, fetched by LDS-DMA (buffer_load_dword ... lds) kRingRows iterations ahead of their use: the data of a
// load in flight needs no vector register, so the depth of the prefetch is a matter of LDS (a wavefront's ring: kRingRows x
// 1 KiB in fp64), not of the 168-register line the pipeline sits at.  (Round 4 held two rows per field in registers; under the
// counter's in-order rule -- vmcnt counts loads and stores together -- the wait in front of a row's first use also waited for
// the previous iteration's stores and loads: a wavefront took 2400 cycles per iteration of which it issued 590, and three
// wavefronts per SIMD could not cover that.)  A buffer resource per row (scalar base) + a lane offset: no 64-bit vector
// address arithmetic, and the stores take the same form.
#ifndef CRD_RING_ROWS
#define CRD_RING_ROWS 4
#endif
constexpr int kRingRowsWanted = CRD_RING_ROWS;  // a multiple of the unroll factor 4; rows in flight per wavefront
// ... as far as the six bits of vmcnt allow (a row of 1 KiB per field takes eight LDS-DMA instructions)
#ifndef CRD_RING_ROWS_THREE
#define CRD_RING_ROWS_THREE 8
#endif
// (three steps per launch: two wavefronts per SIMD -- eight rows in flight per wavefront for the bytes in flight twelve wavefronts of four had)
template <typename V, int STEPS = 2>
constexpr int kRingRowsOf = (kLanes * (int)sizeof(V) / 256 >= 4 && (STEPS == 3 ? CRD_RING_ROWS_THREE : kRingRowsWanted) > 4) ? 4 : (STEPS == 3 ? CRD_RING_ROWS_THREE : kRingRowsWanted);
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char lds_char;
constexpr unsigned kRowResourceBytes = 0x7fffffffu;  // num_records of a row's buffer resource
constexpr unsigned kStoreNowhere = 0x80000000u;      // a byte offset out of its range: the hardware drops the write
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_resource(const void *row)
{
	// raw buffer (stride 0) over the bytes from `row` on: offsets are a lane's byte offset within its row (< 2 GiB)
	return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(row), 0, (int)kRowResourceBytes, 0x00020000);
}
// (kScalarRows) What a work item keeps to address its rows by scalar offsets: the four planes' resources, based at local row `row_lo`,
// the row pitch and the seam (all in bytes), the running offsets of the next fill's row, of the next stores' row and of the next b(j) --
// the latter from the table's entry of the item's first row on, up to its last row's.  Empty where rows build their own resources.
template <bool ON>
struct ScalarRows {
};
template <>
struct ScalarRows<true> {
	__amdgpu_buffer_rsrc_t in_u, in_v, out_u, out_v;
	unsigned pitch, seam, in_off, out_off, b_off, b_last;
	int row_lo;
	const __attribute__((address_space(4))) char *b_first;
};
template <bool NT, typename V>
__device__ __forceinline__ void buffer_row_store(__amdgpu_buffer_rsrc_t r, unsigned byte_offset, V v, unsigned row_offset = 0)
{
	// (row_offset: uniform, the instruction's scalar offset -- added to the address, not to what the range check sees; kScalarRows)
	constexpr int aux = NT ? 2 : 0;  // (2 = nt)
	if constexpr (sizeof(V) == 4) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, byte_offset, row_offset, aux);
	else if constexpr (sizeof(V) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, byte_offset, row_offset, aux);
	else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, byte_offset, row_offset, aux);
}
// Both fields of a ring slot into registers: waits until at most VMCNT vector-memory operations of this wavefront are outstanding
// (the slot's LDS-DMA has landed then: the counter retires in issue order), reads, waits for the reads.  One asm statement, so no
// instruction of the compiler's can come between a read and its wait.
template <int VMCNT, int OFF_U, int OFF_V, typename V>
__device__ __forceinline__ void ring_read(unsigned lds_lane, V &u, V &v)
{
	if constexpr (sizeof(V) == 4)
		asm volatile("s_waitcnt vmcnt(%3)\n\tds_read_b32 %0, %2 offset:%4\n\tds_read_b32 %1, %2 offset:%5\n\ts_waitcnt lgkmcnt(0)"
		             : "=&v"(u), "=&v"(v) : "v"(lds_lane), "n"(VMCNT), "n"(OFF_U), "n"(OFF_V) : "memory");
	else if constexpr (sizeof(V) == 8)
		asm volatile("s_waitcnt vmcnt(%3)\n\tds_read_b64 %0, %2 offset:%4\n\tds_read_b64 %1, %2 offset:%5\n\ts_waitcnt lgkmcnt(0)"
		             : "=&v"(u), "=&v"(v) : "v"(lds_lane), "n"(VMCNT), "n"(OFF_U), "n"(OFF_V) : "memory");
	else
		asm volatile("s_waitcnt vmcnt(%3)\n\tds_read_b128 %0, %2 offset:%4\n\tds_read_b128 %1, %2 offset:%5\n\ts_waitcnt lgkmcnt(0)"
		             : "=&v"(u), "=&v"(v) : "v"(lds_lane), "n"(VMCNT), "n"(OFF_U), "n"(OFF_V) : "memory");
}
// ... and the wait covers the edge reads in flight too (edge_exchange): they pass through as operands, so that nothing uses them before it
template <int VMCNT, int OFF_U, int OFF_V>
__device__ __forceinline__ void ring_read_with_edges(unsigned lds_lane, double &u, double &v, double2r (&e)[4])
{
#ifdef CRD_PROBE_NORINGREAD  // (probe build: what the row's LDS reads and their wait cost at the top of an iteration -- the stages run on whatever the registers held)
	asm volatile("s_waitcnt vmcnt(%6)" : "+v"(u), "+v"(v), "+v"(e[0]), "+v"(e[1]), "+v"(e[2]), "+v"(e[3]) : "n"(VMCNT) : "memory");
	return;
#endif
	asm volatile("s_waitcnt vmcnt(%7)\n\tds_read_b64 %0, %6 offset:%8\n\tds_read_b64 %1, %6 offset:%9\n\ts_waitcnt lgkmcnt(0)"
	             : "=&v"(u), "=&v"(v), "+v"(e[0]), "+v"(e[1]), "+v"(e[2]), "+v"(e[3]) : "v"(lds_lane), "n"(VMCNT), "n"(OFF_U), "n"(OFF_V) : "memory");
}
template <int VMCNT, int OFF_U, int OFF_V>
__device__ __forceinline__ void ring_read_with_edges(unsigned lds_lane, double &u, double &v, double2r (&e)[6])
{
#ifdef CRD_PROBE_NORINGREAD
	asm volatile("s_waitcnt vmcnt(%8)" : "+v"(u), "+v"(v), "+v"(e[0]), "+v"(e[1]), "+v"(e[2]), "+v"(e[3]), "+v"(e[4]), "+v"(e[5]) : "n"(VMCNT) : "memory");
	return;
#endif
	asm volatile("s_waitcnt vmcnt(%9)\n\tds_read_b64 %0, %8 offset:%10\n\tds_read_b64 %1, %8 offset:%11\n\ts_waitcnt lgkmcnt(0)"
	             : "=&v"(u), "=&v"(v), "+v"(e[0]), "+v"(e[1]), "+v"(e[2]), "+v"(e[3]), "+v"(e[4]), "+v"(e[5]) : "v"(lds_lane), "n"(VMCNT), "n"(OFF_U), "n"(OFF_V) : "memory");
}
template <int VMCNT, int OFF_U, int OFF_V, typename V, int N>
__device__ __forceinline__ void ring_read_with_edges(unsigned, V &, V &, double2r (&)[N]) {}  // (COOP is fp64, one column per lane)
// The read of the NEXT iteration's row (kReadAhead), issued and not waited for: the wait on vmcnt is the slot's.  What retires the read
// is the `s_waitcnt lgkmcnt(0)` in front of the barrier of the SAME iteration (edge_exchange); up to there nothing may name the registers
// (tools/kernel_regs.py: async_lds_read_hazards stops the build if something does).
template <int VMCNT, int OFF_U, int OFF_V>
__device__ __forceinline__ void ring_read_ahead(unsigned lds_lane, double &u, double &v)
{
	asm volatile("s_waitcnt vmcnt(%3)\n\tds_read_b64 %0, %2 offset:%4\n\tds_read_b64 %1, %2 offset:%5" : "=&v"(u), "=&v"(v) : "v"(lds_lane), "n"(VMCNT), "n"(OFF_U), "n"(OFF_V) : "memory");
}
// ... and the next iteration's wait for the edge reads in flight (edge_exchange), in front of its first stage.  The row's data landed at the
// previous iteration's barrier wait, where its registers are operands; here only the six edge registers are, and nothing that reads them
// may sit above this statement.
__device__ __forceinline__ void ring_row_landed(double2r (&e)[6])
{
	asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(e[0]), "+v"(e[1]), "+v"(e[2]), "+v"(e[3]), "+v"(e[4]), "+v"(e[5]) : : "memory");
}
// (kEdgeLadder) ... or the counted waits in its place: at most N operations of the LGKM counter outstanding, which retires the reads
// named -- exactly the ones the statement releases, so that nothing reads them above it (tools/kernel_regs.py: async_lds_read_hazards
// counts the LDS instructions behind each read along every path and stops the build where a wait is too lax for its place).
template <int N>
__device__ __forceinline__ void edge_landed(double2r &e0)
{
	static_assert(N >= 0 && N <= edge_waits::kLgkmcntMax, "lgkmcnt is four bits");
	asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(e0) : "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void edge_landed(double2r &e0, double2r &e1)
{
	static_assert(N >= 0 && N <= edge_waits::kLgkmcntMax, "lgkmcnt is four bits");
	asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(e0), "+v"(e1) : "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void edge_landed(double2r &e0, double2r &e1, double2r &e2, double2r &e3, double2r &e4)
{
	static_assert(N >= 0 && N <= edge_waits::kLgkmcntMax, "lgkmcnt is four bits");
	asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(e0), "+v"(e1), "+v"(e2), "+v"(e3), "+v"(e4) : "n"(N) : "memory");
}
// (what the stages call in front of stage 1 and stage 3 where no counted wait sits: nothing, and no state)
struct NoEdgeWait {
	template <typename H>
	__device__ __forceinline__ void operator()(H) const {}
};
// (the first row, read in front of the loop: no barrier wait has seen it)
__device__ __forceinline__ void ring_first_row_landed(double &u, double &v)
{
	asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(u), "+v"(v) : : "memory");
}
template <int VMCNT, int OFF_U, int OFF_V, typename V>
__device__ __forceinline__ void ring_read_ahead(unsigned, V &, V &) {}  // (kReadAhead is fp64, one column per lane, three steps)
template <int N>
__device__ __forceinline__ void ring_row_landed(double2r (&)[N]) {}
template <typename V>
__device__ __forceinline__ void ring_first_row_landed(V &, V &) {}
// (kEdgeLadder) ... and the b(j) the iteration loaded behind its last counted wait: an operand too, so that the compiler's own wait for the
// loaded value -- an `s_waitcnt lgkmcnt(0)` in front of its first use, wherever the scheduler puts that -- stands HERE, beside the wait
// this statement begins with, and not between the next iteration's edge reads and its counted waits, which it would undo.
template <int OFF>
__device__ __forceinline__ void edge_exchange(unsigned con, double2r (&e)[6], double &u, double &v, double &sb)
{
	asm volatile("s_waitcnt lgkmcnt(0)\n\t" CRD_EDGE_BARRIER "\n\ts_mov_b64 exec, %10\n\tds_read_b128 %0, %9 offset:%11\n\tds_read_b128 %1, %9 offset:%12\n\t"
	             "ds_read_b128 %2, %9 offset:%13\n\tds_read_b128 %3, %9 offset:%14\n\tds_read_b128 %4, %9 offset:%15\n\tds_read_b128 %5, %9 offset:%16\n\t"
	             "s_mov_b64 exec, -1"
	             : "=&v"(e[0]), "=&v"(e[1]), "=&v"(e[2]), "=&v"(e[3]), "=&v"(e[4]), "=&v"(e[5]), "+v"(u), "+v"(v), "+s"(sb)
	             : "v"(con), "s"(kEdgeLanes), "n"(OFF), "n"(OFF + 16), "n"(OFF + 32), "n"(OFF + 48), "n"(OFF + 64), "n"(OFF + 80)
	             : "memory");
}
template <int OFF, typename V, int N>
__device__ __forceinline__ void edge_exchange(unsigned, double2r (&)[N], V &, V &) {}
template <int OFF, typename V, typename S, int N>
__device__ __forceinline__ void edge_exchange(unsigned, double2r (&)[N], V &, V &, S &) {}
// LDS bytes of a block's rings
template <typename Real, int COLS, int STEPS = 2, int WAVES = kMaxWavesPerBlock>
constexpr int kRingBytes = WAVES * kRingRowsOf<typename LaneValue<Real, COLS>::type, STEPS> * 2 * kLanes * COLS * (int)sizeof(Real);

// TWO classical RK4 steps of the item's rows in one pass over memory (STEPS = 2): the pipeline of fused_item twice over, eight stages
// deep -- iteration m takes row p (out of its LDS ring slot), runs stages 1..4 of step n on rows p-1 .. p-4, hands the new row p-4
// to a second, identical pipeline as ITS input row, which runs stages 1..4 of step n+1 on rows p-5 .. p-8 and stores row p-8.
// The state crosses memory once per TWO steps: 8 B (fp32) / 16 B (fp64) per grid-point-step instead of 16 / 32.  What it costs:
// the apron is 8 columns and 8 rows a side (48 valid columns of 64; 112 of 128 with two columns per lane), 16 filling iterations per
// chunk -- which run only the stages that have inputs, straight-line code in front of the loop -- and twice the pipeline registers
// (three wavefronts per SIMD instead of four).  What bounds the launch is its memory traffic, with vector issue close behind
// (profiles/r05/two_step_memory_path_ab.txt).
// (Goldbeter in fp64 runs the BLOCK as the strip -- kCoop above: one apron around four wavefronts' 256 lanes, 240 valid columns.)
// Slot arithmetic: row r of either pipeline lives in slot r mod 4; the second pipeline's rows are the first one's shifted by 4,
// i.e. the SAME slots -- the stage code is one lambda applied to two sets of arrays.  Per point the arithmetic is the sequence of
// two single steps exactly (same fused multiply-adds, same constants), so the result is theirs bit for bit.
// (COUNTED: the kernel may take its edge values by counted waits, kEdgeLadder above.  The kernel with the absorbing-row selects, which
// holds both bodies, may not: at its 106 scalar registers the compiler reloads kernel arguments where it likes -- an `s_load` between
// the edge reads and a counted wait in the tail's code, which the build's contract check refuses -- and keeps the single wait in both.)
template <typename Real, int MODEL, bool ABSORB, int COLS, bool NT, int STEPS = 2, int WAVES = kMaxWavesPerBlock, bool COUNTED = true>
__device__ __forceinline__ void fused_item_multi_step(const Slab<Real> &s, const FusedArgs<Real> &a, const int strip, const int chunk, lds_char *const block_rings,
                                                      const int sblk = 0, lds_char *const block_edges = nullptr)
{
	static_assert(STEPS == 2 || STEPS == 3, "two or three steps per launch");
	constexpr bool COOP = kCoop<Real, MODEL, COLS, STEPS>;
#ifdef CRD_NO_SETPRIO
	constexpr bool PRIO = false;
#else
#ifdef CRD_PRIO_THREE  // (experiment switch: the three-step pipeline's memory operations at raised priority too)
	constexpr bool PRIO = sizeof(Real) == 8 && COLS == 1 && MODEL == CRD_MODEL_FHN;
#else
	constexpr bool PRIO = sizeof(Real) == 8 && COLS == 1 && MODEL == CRD_MODEL_FHN && STEPS == 2;
#endif
#endif
	using V = typename LaneValue<Real, COLS>::type;
	constexpr int APRON = STEPS * kApron;
	constexpr int FILL = 2 * APRON;  // iterations of a chunk before rows come out: stage k of step n has inputs from iteration 8 n + 2 k on
	static_assert(APRON % COLS == 0, "the apron is whole lanes");
	constexpr int VALID = COLS * kLanes - 2 * APRON;
	constexpr int M = 4;
	// the ring: kRingRows slots of [u row segment | v row segment], RB bytes each, filled 256 B (64 lanes x one dword) per LDS-DMA
	constexpr int RB = kLanes * (int)sizeof(V), SLOT = 2 * RB, G1 = RB / 256, kRingRows = kRingRowsOf<V, STEPS>;
	static_assert(kRingRows % M == 0 && kRingRows >= M && (kRingRows & (kRingRows - 1)) == 0, "ring slots are addressed with the unrolled iteration index");
	// vector-memory operations a wavefront issues per iteration: 2 G1 LDS-DMA loads, and 2 stores once rows come out.  When the slot
	// of iteration m is read, the operations issued after its fill (at iteration m - kRingRows) are the fills of kRingRows - 1
	// iterations and the stores of kRingRows iterations -- none of the latter while the pipeline still fills.
	constexpr int kWaitFill = (kRingRows - 1) * 2 * G1, kWaitSteady = kWaitFill + 2 * kRingRows;
	static_assert(kWaitSteady <= 63, "vmcnt is six bits");
	// (kReadAhead) Row p + 1 is read in iteration p, behind that iteration's fill (and its first step's stages) and in front of its stores.  Its slot was filled at iteration
	// p + 1 - kRingRows (or, for the first kRingRows rows, in front of the loop); issued after that fill are the stores of that iteration,
	// fill and stores of the kRingRows - 2 iterations p + 2 - kRingRows .. p - 1, and the fill of iteration p: kRingRows - 1 fills as before,
	// and the stores of kRingRows - 1 iterations, one fewer than at the top of iteration p + 1 -- this iteration's own are not out yet.
	// While fewer than kRingRows - 1 of those iterations stored (p + 1 - kRingRows < FILL) the count is the fills alone, kWaitFill.
	constexpr bool AHEAD = kReadAhead<Real, MODEL, COLS, STEPS>;
	constexpr int kWaitAhead = kWaitFill + 2 * (kRingRows - 1);
	static_assert(kWaitAhead <= 63, "vmcnt is six bits");
	// (kEdgeLadder) The same argument on the LGKM counter for the edge reads, which come back in issue order like the fills: behind edge
	// read k of the previous iteration's exchange lie the 5 - k later reads and what this iteration has issued so far -- the publish of
	// u0, per step the publish of its input row (steps 1 and 2) and of its three stage values, the two reads of the read ahead behind
	// step 0.  In front of stage 1 / stage 3 of steps 0, 1, 2 that is 5 + 1 = 6, 4 + 3 = 7, 3 + 7 = 10, 2 + 9 = 11, 1 + 11 = 12 and
	// 0 + 13 = 13 operations: `s_waitcnt lgkmcnt(N)` with that N leaves at most those outstanding, so read k is back.  The numbers are
	// edge_waits::ladder_wait(STEPS, n, h), computed from the same quantities (crd_edge_waits.h), none above the field's 15; they hold
	// while no scalar memory load is in flight, which returns out of order on the same counter (next_b, below).
	// (kReadAhead, the fill in the shadow of the edge reads) Publish, fill and row scalars of an iteration sit between the reads the previous
	// iteration's barrier released (edge_exchange) and the wait for them (ring_row_landed) instead of behind that wait.  The fill was the
	// first vector-memory operation of its iteration before and is so now, the stores the last: a wavefront's sequence -- fill q, stores q,
	// fill q + 1 -- is what it was, and so are both counts above.  Re-derived for the read ahead of iteration p: behind the fill of its slot
	// (iteration p + 1 - kRingRows) lie that iteration's stores, fills and stores of iterations p + 2 - kRingRows .. p - 1 and the fill of
	// iteration p, kRingRows - 1 fills and kRingRows - 1 store pairs = kWaitAhead; nothing moved across a vector-memory operation.
	// (kScalarRows) ... nor does the row's address moving from the resource's base into the instruction's scalar offset: the same fills and
	// stores in the same order.  The iterations that wait for kWaitFill behind the fill -- the first kRingRows - 1 of them -- are
	// straight-line code of their own (below), so that the loop proper carries neither the compare nor the branch around that wait.
	constexpr bool SROWS = kScalarRows<Real, MODEL, COLS, STEPS>;
	static_assert(!SROWS || AHEAD, "scalar row offsets: the read-ahead block strip");
	const int lane = threadIdx.x & (kLanes - 1);
	const int nx = s.nx;
	// column of lane 0 (before wrapping), and this lane's place in what the apron surrounds: the wavefront's 64 lanes -- or the block's
	const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const int x0 = COOP ? sblk * (a.sw * kLanes - 2 * APRON) - APRON + wave * kLanes : strip * VALID - APRON;
	const int place = COOP ? wave * kLanes + lane : COLS * lane, span = COOP ? a.sw * kLanes : COLS * kLanes;
	int x = x0 + COLS * lane;
	x %= nx;
	if (x < 0) x += nx;
	const unsigned xb = (unsigned)x * (unsigned)sizeof(Real);  // (a lane that stores has x == out_col: its column is inside [0, nx) unwrapped, so xb serves the stores too)
	const int out_col = x0 + COLS * lane;
	const bool lane_stores = place >= APRON && place < span - APRON && out_col < nx;
	// ... and where its stores go: its column's bytes, or beyond the range of the row's buffer resource (row_resource: 0x7fffffff bytes),
	// where a write is dropped -- the store instructions themselves are issued by every lane (see the stores below)
	const unsigned xb_store = lane_stores ? xb : kStoreNowhere;

	const int range = chunk >= a.first2 ? 1 : 0;
	const int range_end = a.r_end[range];
	const int j0 = a.r_begin[range] + (chunk - (range ? a.first2 : 0)) * a.chunk;
	const int j1 = (j0 + a.chunk < range_end) ? j0 + a.chunk : range_end;
	const int jbase = j0 - APRON;
	const int niter = (j1 - j0) + 2 * APRON;
	const int jlast = j1 + APRON - 1;

	const V cE = *reinterpret_cast<const V *>(s.cE + x), cWn = *reinterpret_cast<const V *>(s.cWn + x), cP = *reinterpret_cast<const V *>(s.cP + x);
	const Real ka4 = s.ka4;
	const V h1 = (V)a.h1, h2 = (V)a.h2, h3 = (V)a.h3, h6 = (V)a.h6;
	const __attribute__((address_space(4))) Real *const brow = (const __attribute__((address_space(4))) Real *)(s.brow);
	const int wrap_nyl = s.wrap ? s.nyl : 0;
	auto row_base = [&](int j) -> ptrdiff_t {
		j += wrap_nyl & (j >> 31);
		j -= (j >= s.nyl) ? wrap_nyl : 0;
		return (ptrdiff_t)j * nx;
	};
	// (kScalarRows) A row as a byte offset from the lowest row a launch can address -- row 0 where phi wraps inside the slab, the first
	// ghost row elsewhere -- in 32 bits (the host's rule: fused_scalar_rows_addressable), and the four planes' resources based there.
	// row_offset is the arithmetic of row_base, once per item; from there the offsets run (take_row, the stores).
	// (All of it lives in `sr`, which is empty in every other kernel: their code is what it was, to the instruction.)
	[[maybe_unused]] ScalarRows<SROWS> sr;
	[[maybe_unused]] auto row_offset = [&](int j, auto &rows) -> unsigned {
		j += wrap_nyl & (j >> 31);
		j -= (j >= s.nyl) ? wrap_nyl : 0;
		return (unsigned)(j - rows.row_lo) * rows.pitch;
	};
	if constexpr (SROWS) {
		sr.pitch = (unsigned)nx * (unsigned)sizeof(Real);
		sr.row_lo = s.wrap ? 0 : -kGhost;
		sr.seam = s.wrap ? (unsigned)s.nyl * sr.pitch : 0xffffffffu;  // one row beyond the last: the next row is the plane's first (no wrap: never reached)
		const ptrdiff_t lo = (ptrdiff_t)sr.row_lo * nx;
		sr.in_u = row_resource(a.in_u + lo);
		sr.in_v = row_resource(a.in_v + lo);
		sr.out_u = row_resource(a.out_u + lo);
		sr.out_v = row_resource(a.out_v + lo);
	}
	// Global phi boundary rows (src/FHNmodel_torus.cpp:643-653).  Rows ny - 1 and 0 are neighbours on the periodic grid: within the rows
	// this item's pipeline touches (fewer than 2 ny of them) they are local rows jb, jb + 1 and possibly jb + ny, jb + ny + 1.  Two
	// scalars and a bit mask of the 4 STEPS stage flags instead of js, ny and as many flag words: the body with the selects must not need
	// more registers than the one without (168 VGPRs = three wavefronts per SIMD), or the launch's kernel, which holds both, runs
	// every item at two.
	int jb = 0, amask = 0;
	if (ABSORB) {
		int g0 = (a.js + jbase) % a.ny;  // global row of the first row the pipeline takes
		if (g0 < 0) g0 += a.ny;
		jb = jbase + (a.ny - 1 - g0);
#pragma unroll
		for (int k = 0; k < 4; k++) amask |= (a.absorb[k] ? 1 << k : 0) | (a.absorb2[k] ? 16 << k : 0) | ((STEPS == 3 && a.absorb3[k]) ? 256 << k : 0);
		jb = __builtin_amdgcn_readfirstlane(jb);
		amask = __builtin_amdgcn_readfirstlane(amask);
	}
	const int ny_rows = a.ny;
	auto boundary_row = [&](int j) -> bool { return (unsigned)(j - jb) <= 1u || (unsigned)(j - jb - ny_rows) <= 1u; };

	struct Pipe {
		V u0[M], v0[M], U1[M], U2[M], U3[M], V1[2], V2[2], V3[2], aU[M], aV[M];
		Real bq[M];
	};
	Pipe P[STEPS];  // P[n]: the pipeline of step n of the launch; its input rows are P[n - 1]'s output rows
	const V zero_v = splat<V>(0.0);
#pragma unroll
	for (int n = 0; n < STEPS; n++) {
#pragma unroll
		for (int k = 0; k < M; k++) {
			P[n].u0[k] = P[n].v0[k] = P[n].U1[k] = P[n].U2[k] = P[n].U3[k] = P[n].aU[k] = P[n].aV[k] = zero_v;
			P[n].bq[k] = (Real)0;
		}
		P[n].V1[0] = P[n].V1[1] = P[n].V2[0] = P[n].V2[1] = P[n].V3[0] = P[n].V3[1] = zero_v;
	}

	// This wavefront's ring, and where its lanes read: lane l takes the l-th value (of sizeof(V) bytes) of a row segment.
	lds_char *const ring = block_rings + wave * (kRingRows * SLOT);
	// (COOP) where lanes 0 / 63 publish their values -- the wavefront's western / eastern slot -- and where they find their neighbours':
	// lane 0 the eastern slot of the wavefront to the west, lane 63 the western slot of the one to the east (the block's outer edges:
	// any slot, they are apron)
	unsigned edge_pub = 0, edge_con = 0;
	if constexpr (COOP) {
		const unsigned base = (unsigned)(uintptr_t)block_edges;
		edge_pub = (lane == 0 || lane == kLanes - 1) ? base + (unsigned)((wave * 2 + (lane == 0 ? 0 : 1)) * kEdgeSlotBytes<STEPS>)
		                                             : base + (unsigned)(kEdgeBytes<STEPS, WAVES> + (wave * kLanes + lane) * 8);
		edge_con = base + (unsigned)((lane == 0 ? (wave > 0 ? wave - 1 : wave) * 2 + 1 : (wave + 1 < a.sw ? wave + 1 : wave) * 2) * kEdgeSlotBytes<STEPS>);
	}
	const unsigned ring_lane = (unsigned)(uintptr_t)ring + (unsigned)lane * (unsigned)sizeof(V);
	// ... and what they fetch: LDS-DMA instruction h of a row moves dwords 64 h + lane of the segment; the column of a dword's
	// element wraps periodically like x above
	unsigned doff[G1];
#pragma unroll
	for (int h = 0; h < G1; h++) {
		const int q = 4 * (kLanes * h + lane), e = q / (int)sizeof(Real);
		int col = (x0 + e) % nx;
		if (col < 0) col += nx;
		doff[h] = (unsigned)col * (unsigned)sizeof(Real) + (unsigned)(q % (int)sizeof(Real));
	}
	// the row at byte `row_off` (uniform) of both fields' resources -> the ring slot at byte `slot_byte` (uniform)
	[[maybe_unused]] auto fill_from = [&](const auto ru, const auto rv, unsigned row_off, int slot_byte) {  // (kScalarRows)
#pragma unroll
		for (int h = 0; h < G1; h++) __builtin_amdgcn_raw_ptr_buffer_load_lds(ru, ring + (slot_byte + 256 * h), 4, doff[h], row_off, 0, 0);
#pragma unroll
		for (int h = 0; h < G1; h++) __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, ring + (slot_byte + RB + 256 * h), 4, doff[h], row_off, 0, 0);
	};
	auto fill = [&](int jrow, int slot_byte) {  // row jrow of both fields -> the ring slot at byte `slot_byte` (uniform)
		if constexpr (SROWS) {
			fill_from(sr.in_u, sr.in_v, row_offset(jrow, sr), slot_byte);
		} else {
			const ptrdiff_t rb = row_base(jrow);
			const __amdgpu_buffer_rsrc_t ru = row_resource(a.in_u + rb), rv = row_resource(a.in_v + rb);
#pragma unroll
			for (int h = 0; h < G1; h++) __builtin_amdgcn_raw_ptr_buffer_load_lds(ru, ring + (slot_byte + 256 * h), 4, doff[h], 0, 0, 0);
#pragma unroll
			for (int h = 0; h < G1; h++) __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, ring + (slot_byte + RB + 256 * h), 4, doff[h], 0, 0, 0);
		}
	};
#pragma unroll
	for (int k = 0; k < kRingRows; k++) fill((jbase + k < jlast) ? jbase + k : jlast, k * SLOT);
	int jn = (jbase + kRingRows < jlast) ? jbase + kRingRows : jlast;  // the row the next fill takes (the tail re-reads the last valid row)
	// (kScalarRows) ... as its running byte offset; where the stores of the next iteration go (modulo 2^32 while the pipeline fills: the
	// rows in front of the item's first are not stored); b(j) of the next row, from the table's entry of the item's first row on
	if constexpr (SROWS) {
		sr.in_off = row_offset(jn, sr);
		sr.out_off = (unsigned)(jbase - APRON - sr.row_lo) * sr.pitch;
		sr.b_first = (const __attribute__((address_space(4))) char *)(brow + jbase);
		sr.b_off = 0;
		sr.b_last = (unsigned)(jlast - jbase) * (unsigned)sizeof(Real);
	}
	// (kReadAhead) the first row's reads go out here: kRingRows - 1 fills behind its own
	if constexpr (AHEAD) ring_read_ahead<kWaitFill, 0, RB>(ring_lane, P[0].u0[0], P[0].v0[0]);
	Real pb = brow[jbase];                                            // b(j) of the row the next iteration takes
	int trip_byte = 0;                                                // ring byte offset of the slots of this trip of four iterations
	unsigned ring_trip = ring_lane;
	// (the rows that come out of the last pipeline at iteration m: row jbase + m - 4 STEPS)
	Real *out_row_u = a.out_u + (ptrdiff_t)(jbase - APRON) * nx, *out_row_v = a.out_v + (ptrdiff_t)(jbase - APRON) * nx;
	// (kReadAhead) ... and have landed here: the first iteration publishes the row before it waits for anything
	if constexpr (AHEAD) ring_first_row_landed(P[0].u0[0], P[0].v0[0]);

	// Stages 1..4 of one step on the pipeline P whose newest row is `p` (slot S0): new state of row p - 4 in (nu, nv).
	// flag_bit: where the step's four stage flags start in amask; b4: b(j) of row p - 4 (read by the caller before row p took over its slot).
	// `live`: the iterations this pipeline has been fed for (m for the first, m - 8 n for the n-th; 8 and more: all stages run).  In the
	// chunk's first 8 STEPS iterations stage k has complete inputs only from the pipeline's iteration 2 k on -- the stages before that are
	// skipped (their rows lie outside what the chunk's outputs depend on: nothing downstream reads what they would have written).  Half
	// the work of those iterations, which is a tenth of a 61-row item's -- one rank's share of an 8-GPU run -- and a third of an edge band's.
	[[maybe_unused]] double2r edge[2 * STEPS];  // (COOP) the neighbours' edge values, lanes 0 and 63: quantity q of an iteration in edge[q / 2]
#pragma unroll
	for (int q = 0; q < 2 * STEPS; q++) edge[q] = double2r{0.0, 0.0};
	auto point = [&](V uC, V uS, V uN, V v, Real rowp, bool zero, [[maybe_unused]] V X, V &du, V &dv) {
		if constexpr (COOP) rhs_lane_edge<MODEL>(uC, X, uS, uN, v, cE, cWn, cP, rowp, ka4, zero, du, dv);
		else rhs_lane<V, MODEL>(uC, uS, uN, v, cE, cWn, cP, rowp, ka4, zero, du, dv);
	};
	auto stages = [&](Pipe &Q, const int p, auto kk, auto live_c, const int flag_bit, const Real b4, V &nu, V &nv, [[maybe_unused]] const V (&E)[4], auto qbase_c, [[maybe_unused]] auto landed) {
		constexpr int K = decltype(kk)::value;
		[[maybe_unused]] constexpr int PUB = (K & 1) * kEdgeParityBytes<STEPS, WAVES> + decltype(qbase_c)::value * 8;
		constexpr int live = decltype(live_c)::value;  // (compile-time: the filling iterations are so many pieces of straight-line code)
		constexpr int S0 = K % M, S1 = (K + M - 1) % M, S2 = (K + M - 2) % M, S3 = (K + M - 3) % M, S4 = (K + 2 * M - 4) % M, S5 = (K + 2 * M - 5) % M;
		V du, dv;
		landed(std::integral_constant<int, 0>{});  // (kEdgeLadder: E[0], E[1] -- or nothing)
		if constexpr (live >= 2) {
			point(Q.u0[S1], Q.u0[S2], Q.u0[S0], Q.v0[S1], Q.bq[S1], ABSORB && ((amask >> (flag_bit + 0)) & 1) && boundary_row(p - 1), E[0], du, dv);
			Q.U1[S1] = stage_fma(h2, du, Q.u0[S1]);
			if constexpr (COOP) edge_publish<PUB + 8>(edge_pub, Q.U1[S1]);
			Q.V1[S1 & 1] = stage_fma(h2, dv, Q.v0[S1]);
			Q.aU[S1] = stage_fma(h6, du, Q.u0[S1]);
			Q.aV[S1] = stage_fma(h6, dv, Q.v0[S1]);
		}
		if constexpr (live >= 4) {
			point(Q.U1[S2], Q.U1[S3], Q.U1[S1], Q.V1[S2 & 1], Q.bq[S2], ABSORB && ((amask >> (flag_bit + 1)) & 1) && boundary_row(p - 2), E[1], du, dv);
			Q.U2[S2] = stage_fma(h2, du, Q.u0[S2]);
			if constexpr (COOP) edge_publish<PUB + 16>(edge_pub, Q.U2[S2]);
			Q.V2[S2 & 1] = stage_fma(h2, dv, Q.v0[S2]);
			Q.aU[S2] = stage_fma(h3, du, Q.aU[S2]);
			Q.aV[S2] = stage_fma(h3, dv, Q.aV[S2]);
		}
		landed(std::integral_constant<int, 1>{});  // (kEdgeLadder: E[2], E[3] -- or nothing)
		if constexpr (live >= 6) {
			point(Q.U2[S3], Q.U2[S4], Q.U2[S2], Q.V2[S3 & 1], Q.bq[S3], ABSORB && ((amask >> (flag_bit + 2)) & 1) && boundary_row(p - 3), E[2], du, dv);
			Q.U3[S3] = stage_fma(h1, du, Q.u0[S3]);
			if constexpr (COOP) edge_publish<PUB + 24>(edge_pub, Q.U3[S3]);
			Q.V3[S3 & 1] = stage_fma(h1, dv, Q.v0[S3]);
			Q.aU[S3] = stage_fma(h3, du, Q.aU[S3]);
			Q.aV[S3] = stage_fma(h3, dv, Q.aV[S3]);
		}
		nu = nv = zero_v;
		if constexpr (live >= 8) {
			point(Q.U3[S4], Q.U3[S5], Q.U3[S3], Q.V3[S4 & 1], b4, ABSORB && ((amask >> (flag_bit + 3)) & 1) && boundary_row(p - 4), E[3], du, dv);
			nu = stage_fma(h6, du, Q.aU[S4]);
			nv = stage_fma(h6, dv, Q.aV[S4]);
		}
	};
	auto next_trip = [&]() {
		if constexpr (kRingRows > M) {
			trip_byte = (trip_byte + M * SLOT) & (kRingRows * SLOT - 1);
			ring_trip = ring_lane + (unsigned)trip_byte;
		}
	};
	auto iteration = [&](int m, auto kk, auto fed_c, auto steady_c) {
		constexpr int FED = decltype(fed_c)::value;  // iterations before this one, if fewer than FILL
		constexpr bool STEADY = decltype(steady_c)::value;  // (kScalarRows) an iteration of the loop proper: m + 1 >= FILL + kRingRows, known where it is written
		constexpr int K = decltype(kk)::value;
		constexpr int S0 = K % M, S4 = (K + 2 * M - 4) % M;
#if !defined(CRD_NO_LOCKSTEP) && !defined(CRD_NO_LOCKSTEP_TWO)
		// Lockstep of the block's wavefronts: fp32 only.  With the rows coming through the rings, the fp64 pipelines run 1 - 5 % faster
		// when their wavefronts drift (8192^2 FHN 0.2292 -> 0.2251 ms per step, 4096^2 0.0683 -> 0.0663, Goldbeter 4096^2 0.1212 -> 0.1148),
		// the packed fp32 one 2 % slower (16384^2 0.4230 -> 0.4308; profiles/r05/two_step_memory_path_ab.txt).
		// (round 6: ... and of the fp32 kernels only the two-step one: the three-step launch, bound by issue at two wavefronts per SIMD, runs
		// 2 % faster without -- C5 0.3689 -> 0.3625 ms per step, 8192^2 0.0998 -> 0.0975; the two-step one 3 % slower, as before)
		if constexpr (sizeof(Real) == 4 && STEPS == 2) __builtin_amdgcn_s_barrier();
#endif
		const int p = jbase + m;
		Real b4[STEPS];  // b(j) of the rows stage 4 of each step works on, read before row p takes over the slot
#pragma unroll
		for (int n = 0; n < STEPS; n++) b4[n] = P[n].bq[S4];
		// row p out of its ring slot (filled kRingRows iterations ago) ...
		if (!AHEAD && m < FILL + kRingRows) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kWaitFill) : "memory");  // (fewer operations in flight while no rows come out yet)
		V E[STEPS][4];
		// b(j) of row p into its slot, row p + kRingRows into the ring slot row p came out of, and the row the next fill takes
		// (kEdgeLadder) An iteration behind the fill takes the edge values read by read (LADDER: 1, 2 or 3 -- kEdgeLadder above); the
		// filling iterations skip stages and publishes, their counts differ, and they keep the single wait.
		constexpr int LADDER = (FED >= FILL && COUNTED) ? kEdgeLadder<Real, MODEL, COLS, STEPS> : 0;
		auto take_row = [&]() {
			if constexpr (LADDER == 0) P[0].bq[S0] = uniform(pb);  // (kEdgeLadder: behind the iteration's last counted wait, see there)
#ifndef CRD_PROBE_NOLOAD  // (probe builds, tools/build_variant.sh: what a launch costs without its row reads / its later steps / its stores)
			if constexpr (SROWS) fill_from(sr.in_u, sr.in_v, sr.in_off, trip_byte + S0 * SLOT);
			else fill(jn, trip_byte + S0 * SLOT);  // ... and row p + kRingRows into it
#endif
			if constexpr (SROWS) {
				// one pitch on, unless the tail holds the last row; behind the plane's last row comes its first (periodic single slab)
				sr.in_off += (jn < jlast) ? sr.pitch : 0u;
				sr.in_off = (sr.in_off == sr.seam) ? 0u : sr.in_off;
			}
			jn = (jn < jlast) ? jn + 1 : jlast;
		};
		// b(j) of the row the next iteration takes: row p + 1, the item's last row at the most
		[[maybe_unused]] auto next_b = [&]() {
			if constexpr (SROWS) {
				sr.b_off = (sr.b_off + (unsigned)sizeof(Real) < sr.b_last) ? sr.b_off + (unsigned)sizeof(Real) : sr.b_last;
				pb = *(const __attribute__((address_space(4))) Real *)(sr.b_first + sr.b_off);
			} else {
				pb = brow[(p < jlast) ? p + 1 : jlast];
			}
		};
		if constexpr (AHEAD) {
			// ... which the previous iteration read ahead: it landed at that iteration's barrier wait (edge_exchange), and behind the barrier the
			// reads of the neighbours' edge values went out.  What this iteration can do without them sits HERE, between those reads and the
			// wait for them -- the publish of this row, its fill and the next fill's row: LDS, memory and scalar issue, which a wavefront fresh
			// out of a barrier issues at full rate, in the time the edge reads of the block's eight (or four) wavefronts take to come back from
			// the one LDS.  (The row's stores stay in front of the barrier; deferring them to this place was measured and not kept,
			// profiles/r09/edge_shadow_ab.txt.)
			edge_publish<(K & 1) * kEdgeParityBytes<STEPS, WAVES>>(edge_pub, P[0].u0[S0]);
			take_row();
			if constexpr (K == M - 1) next_trip();  // (the read ahead below is the next trip's first slot)
			// ... and only now the wait for the neighbours' edge values
			if constexpr (LADDER == 0) {
				ring_row_landed(edge);
				// The scalar load of the next b(j) goes out BEHIND that wait: it returns on the same counter as the edge reads, and in front of the
				// wait the wavefront would stand for its latency as well.  The barrier's wait is the next to see it, a whole iteration later.
				next_b();
#pragma unroll
				for (int n = 0; n < STEPS; n++) E[n][0] = edge[2 * n].x, E[n][1] = edge[2 * n].y, E[n][2] = edge[2 * n + 1].x, E[n][3] = edge[2 * n + 1].y;
			}
			// (kEdgeLadder: ... read by read, in front of the stages -- `landed` below)
		} else if constexpr (COOP) {
			// ... together with the neighbours' edge values, whose reads the previous iteration issued behind its barrier
			ring_read_with_edges<kWaitSteady, S0 * SLOT, S0 * SLOT + RB>(ring_trip, P[0].u0[S0], P[0].v0[S0], edge);
#pragma unroll
			for (int n = 0; n < STEPS; n++) E[n][0] = edge[2 * n].x, E[n][1] = edge[2 * n].y, E[n][2] = edge[2 * n + 1].x, E[n][3] = edge[2 * n + 1].y;
			edge_publish<(K & 1) * kEdgeParityBytes<STEPS, WAVES>>(edge_pub, P[0].u0[S0]);
		} else {
			ring_read<kWaitSteady, S0 * SLOT, S0 * SLOT + RB>(ring_trip, P[0].u0[S0], P[0].v0[S0]);
#pragma unroll
			for (int n = 0; n < STEPS; n++) E[n][0] = E[n][1] = E[n][2] = E[n][3] = zero_v;
		}
		if constexpr (!AHEAD) {
			take_row();
			pb = brow[(p < jlast) ? p + 1 : jlast];
		}
		V nu, nv;
		if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);  // (see the stores below)
		// (kReadAhead) Row p + 1 out of its ring slot -- the next one of this trip, or the first of the next -- straight into the registers it
		// lives in: the first step's stages are the last to need row p - 3, whose slot that is, so the read goes out behind them, costs no
		// second register set, and lands under the stages of the later steps (this iteration's barrier wait, edge_exchange, retires it).  (Behind the item's last row it reads the slot the tail's
		// fills keep rewriting: one read per iteration, whatever the row.)
		[[maybe_unused]] auto read_ahead = [&]() {
			if constexpr (!STEADY)
				if (m + 1 < FILL + kRingRows) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kWaitFill) : "memory");
			ring_read_ahead<kWaitAhead, ((K + 1) % M) * SLOT, ((K + 1) % M) * SLOT + RB>(ring_trip, P[0].u0[(K + 1) % M], P[0].v0[(K + 1) % M]);
		};
#ifdef CRD_PROBE_NOMATH  // (probe build: the launch as a copy -- its memory traffic alone)
		nu = P[0].u0[S0] + (V)b4[0];
		nv = P[0].v0[S0] + (V)b4[STEPS - 1];
		if constexpr (AHEAD) read_ahead();
#else
		// step n of the launch: the new row p - 4 (n + 1), which is the next pipeline's newest row (same slot: rows shifted by 4)
		for_sequence(
		    [&](auto nn) {
			    constexpr int N = decltype(nn)::value;
#ifdef CRD_PROBE_HALFMATH
			    if constexpr (N > 0) return;
#endif
			    if constexpr (N > 0) {
				    P[N].u0[S0] = nu;
				    P[N].v0[S0] = nv;
				    P[N].bq[S0] = b4[N - 1];
				    if constexpr (COOP) edge_publish<(K & 1) * kEdgeParityBytes<STEPS, WAVES> + 32 * N>(edge_pub, nu);
			    }
			    constexpr int live = FED - 8 * N < 0 ? 0 : (FED - 8 * N > 8 ? 8 : FED - 8 * N);
			    // (kEdgeLadder) What the stages call in front of stage 1 (H = 0) and stage 3 (H = 1): the counted wait for the edge reads that
			    // have to be back there, and only behind it the values out of their registers.  The counts: crd_edge_waits.h, from the
			    // iteration's operations as they are written here -- u0's publish in take_row's place, then per step the publish of its input
			    // row, stages and stage publishes, the read ahead behind step 0.  Behind the iteration's LAST counted wait sit the two
			    // things that must not come between an edge read and a counted wait: the first use of the b(j) loaded an iteration ago --
			    // the compiler puts its own `s_waitcnt lgkmcnt(0)` in front of it, which above would undo every counted wait -- and the
			    // scalar load of the next one, which returns out of order on the same counter (the barrier's wait retires it).
			    [[maybe_unused]] auto landed = [&](auto hh) {
				    [[maybe_unused]] constexpr int H = decltype(hh)::value;
				    static_assert(LADDER == 0 || (STEPS == 3 && live == 8), "the counted waits: three steps, every stage and publish of the iteration");
				    if constexpr (LADDER != 0) {
					    using namespace edge_waits;
					    bool last = false;
					    if constexpr (LADDER == 3) {
						    edge_landed<ladder_wait(STEPS, N, H)>(edge[2 * N + H]);
						    E[N][2 * H] = edge[2 * N + H].x, E[N][2 * H + 1] = edge[2 * N + H].y;
						    last = N == STEPS - 1 && H == 1;
					    } else if constexpr (LADDER == 2) {
						    if constexpr (H == 0) {
							    edge_landed<step_wait(STEPS, N)>(edge[2 * N], edge[2 * N + 1]);
							    E[N][0] = edge[2 * N].x, E[N][1] = edge[2 * N].y, E[N][2] = edge[2 * N + 1].x, E[N][3] = edge[2 * N + 1].y;
							    last = N == STEPS - 1;
						    }
					    } else if constexpr (N == 0 && H == 0) {
						    edge_landed<ladder_wait(STEPS, 0, 0)>(edge[0]);
						    E[0][0] = edge[0].x, E[0][1] = edge[0].y;
					    } else if constexpr (N == 0) {
						    edge_landed<rest_wait(STEPS)>(edge[1], edge[2], edge[3], edge[4], edge[5]);
						    E[0][2] = edge[1].x, E[0][3] = edge[1].y;
#pragma unroll
						    for (int n = 1; n < STEPS; n++) E[n][0] = edge[2 * n].x, E[n][1] = edge[2 * n].y, E[n][2] = edge[2 * n + 1].x, E[n][3] = edge[2 * n + 1].y;
						    last = true;
					    }
					    if (last) {
						    P[0].bq[S0] = uniform(pb);
						    next_b();
					    }
				    }
			    };
			    if constexpr (LADDER != 0) stages(P[N], p - kApron * N, kk, std::integral_constant<int, live>{}, 4 * N, b4[N], nu, nv, E[N], std::integral_constant<int, 4 * N>{}, landed);
			    else stages(P[N], p - kApron * N, kk, std::integral_constant<int, live>{}, 4 * N, b4[N], nu, nv, E[N], std::integral_constant<int, 4 * N>{}, NoEdgeWait{});
			    if constexpr (AHEAD && N == 0) read_ahead();
		    },
		    std::make_integer_sequence<int, STEPS>{});
#endif
		// (FHN fp64) From its stores to the next row's fill a wavefront issues ahead of its SIMD's other wavefronts (which are in their
		// arithmetic): its memory operations go out when it reaches them instead of waiting their turn among vector instructions.
		// Nothing on 8192^2, -1 % on 4096^2, -2 % on a rank's 8192 x 1024 share; 1 - 2 % SLOWER in fp32 and 0 - 1 % in Goldbeter, which
		// do without (profiles/r05/two_step_memory_path_ab.txt, K).  Non-temporal row LOADS, tried beside it, cost 15 %: the rows' reuse
		// by the neighbouring items is what keeps the traffic at 1.06 x compulsory.
		if constexpr (PRIO) __builtin_amdgcn_s_setprio(2);
		// Rows j0 .. j1 - 1 exactly: every iteration behind the filling ones.  BOTH store instructions go out in every such iteration of
		// every wavefront, with all lanes on -- the waits of ring_read COUNT them (kWaitSteady).  A lane that has nothing to store (apron,
		// or a column beyond nx) is parked on an offset beyond the buffer resource's range, where the hardware drops its write; under an
		// `if (lane_stores)` the compiler puts a skip branch (s_cbranch_execz) in front of the stores, a wavefront without a storing lane
		// then has fewer operations in flight than the wait assumes, and its ring read can overtake the LDS-DMA fill of its slot.
		if constexpr (FED >= FILL) {
#if defined(CRD_PROBE_BRANCHY_STORES)  // (probe build: round 5's form, stores under the lanes' condition -- what the parked lanes cost; NOT safe, see above)
			static_assert(!SROWS, "the probe stores through the row pointers: build it with -DCRD_NO_SCALAR_ROWS");
			if (lane_stores) {
				buffer_row_store<NT>(row_resource(out_row_u), xb, nu);
				buffer_row_store<NT>(row_resource(out_row_v), xb, nv);
			}
#elif !defined(CRD_PROBE_NOSTORE)
			if constexpr (SROWS) {
				buffer_row_store<NT>(sr.out_u, xb_store, nu, sr.out_off);
				buffer_row_store<NT>(sr.out_v, xb_store, nv, sr.out_off);
			} else {
				buffer_row_store<NT>(row_resource(out_row_u), xb_store, nu);
				buffer_row_store<NT>(row_resource(out_row_v), xb_store, nv);
			}
#else
			if (a.nchunks < 0) {  // (never: keeps the arithmetic alive)
				buffer_row_store<NT>(row_resource(out_row_u), xb_store, nu);
				buffer_row_store<NT>(row_resource(out_row_v), xb_store, nv);
			}
#endif
		}
		if constexpr (SROWS) {
			sr.out_off += sr.pitch;
		} else {
			out_row_u += nx;
			out_row_v += nx;
		}
		// (COOP) what the block's wavefronts published during this iteration is complete beyond the barrier; the reads of what the next
		// iteration needs of it go out at once and land while that iteration waits for its row
		// (kReadAhead: ... and its wait retires the read of the next row, whose registers it names)
		if constexpr (LADDER != 0) edge_exchange<(K & 1) * kEdgeParityBytes<STEPS, WAVES>>(edge_con, edge, P[0].u0[(K + 1) % M], P[0].v0[(K + 1) % M], pb);
		else if constexpr (AHEAD) edge_exchange<(K & 1) * kEdgeParityBytes<STEPS, WAVES>>(edge_con, edge, P[0].u0[(K + 1) % M], P[0].v0[(K + 1) % M]);
		else if constexpr (COOP) edge_exchange<(K & 1) * kEdgeParityBytes<STEPS, WAVES>>(edge_con, edge);
	};
	int m = 0;
	for_sequence(  // the pipeline fills (a chunk has at least one row: FILL iterations and more)
	    [&](auto i) {
		    constexpr int I = decltype(i)::value;
		    iteration(I, std::integral_constant<int, I % M>{}, i, std::false_type{});
		    if constexpr (!AHEAD && I % M == M - 1) next_trip();  // (kReadAhead: the trip's last iteration moves on itself, in front of its read ahead)
	    },
	    std::make_integer_sequence<int, FILL>{});
	m = FILL;
	if constexpr (SROWS) {
		// The first kRingRows iterations behind the fill, trip by trip as far as the item has them: m is a constant in each, and so is which
		// wait its read ahead takes (kWaitFill while m + 1 < FILL + kRingRows).  The loop proper starts behind them.
		bool whole = true;
		for_sequence(
		    [&](auto t) {
			    constexpr int M0 = FILL + M * decltype(t)::value;
			    whole = whole && M0 + M - 1 < niter;
			    if (whole) {
				    for_sequence([&](auto k) { iteration(M0 + decltype(k)::value, k, std::integral_constant<int, FILL>{}, std::false_type{}); }, std::make_integer_sequence<int, M>{});
				    m = M0 + M;
			    }
		    },
		    std::make_integer_sequence<int, kRingRows / M>{});
		// (an item that ended inside those trips has fewer than M iterations left: the loop's condition is false for it)
		for (; m + M - 1 < niter; m += M)
			for_sequence([&](auto k) { iteration(m + decltype(k)::value, k, std::integral_constant<int, FILL>{}, std::true_type{}); }, std::make_integer_sequence<int, M>{});
	} else {
		for (; m + M - 1 < niter; m += M) {
			for_sequence([&](auto k) { iteration(m + decltype(k)::value, k, std::integral_constant<int, FILL>{}, std::false_type{}); }, std::make_integer_sequence<int, M>{});
			if constexpr (!AHEAD) next_trip();
		}
	}
	// (the tail: up to M - 1 iterations, of an item of any length -- the wait of their read ahead is decided at run time)
	for_sequence(
	    [&](auto k) {
		    if (m + decltype(k)::value < niter) iteration(m + decltype(k)::value, k, std::integral_constant<int, FILL>{}, std::false_type{});
	    },
	    std::make_integer_sequence<int, M - 1>{});
	// the fills still in flight write LDS: they must have landed before the wavefront ends and its LDS goes to the next workgroup
	// (... and the last read ahead, which no iteration takes: its registers pass through here, or the compiler would hand them to something
	// else while the read is in flight)
	if constexpr (AHEAD)
		asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)"
		             : "+v"(P[0].u0[0]), "+v"(P[0].u0[1]), "+v"(P[0].u0[2]), "+v"(P[0].u0[3]), "+v"(P[0].v0[0]), "+v"(P[0].v0[1]), "+v"(P[0].v0[2]), "+v"(P[0].v0[3])
		             :
		             : "memory");
	else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Wavefronts per SIMD the register allocator is held to: the two-step pipelines live at the 168-register line (three wavefronts).
template <typename Real, int MODEL, int COLS, int STEPS, bool ABSORB>
constexpr int kMinWaves = (STEPS == 2 && COLS * (int)sizeof(Real) == 8 && MODEL == CRD_MODEL_FHN && !ABSORB) ? 3 : (STEPS == 3 ? 2 : 1);

}  // namespace

}  // namespace crd

