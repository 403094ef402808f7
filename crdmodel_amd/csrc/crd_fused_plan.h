// crd_fused_plan.h -- the integer arithmetic of the one-launch step's launch plan: how many steps a launch can take, how the columns are
// cut into strips and the rows into work items, how the items are dealt to the XCDs, where a multi-step launch with absorbing rows is cut
// into bands, and which plan candidates the tuner times.  Plain C++17, nothing from HIP: what the device reports (compute units, resident
// wavefront slots of the kernel in question) and what the kernels' templates decide (KernelTraits) come in as arguments.  The launcher
// (crd_fused_launch.h) is the one user in the library; tests/native/fused_plan_selftest.cpp checks the rules on the CPU.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "crd_internal.h"
#include "crd_tuning.h"

namespace crd {
namespace plan {

// (the kernels' own constants, crd_fused_impl.h / crd_device.h: the launcher asserts that they agree)
constexpr int kApron = 4;             // columns and rows a step consumes per side: one per RK4 stage
constexpr int kLanes = 64;
constexpr int kWavesPerBlock = 4;     // wavefronts, i.e. adjacent strips, per block
constexpr int kMaxWavesPerBlock = 4;  // ... at most, but for
constexpr int kWideWaves = 8;         // the eight-wide three-step block strip (chunk mode 3)
constexpr int kNumXcd = 8;

// What the kernels' templates decide for one precision and model (crd_fused_launch.h: kTraits).
struct KernelTraits {
	int real_bytes;        // 8 / 4
	bool can_two_steps;    // the model has two-step instantiations (all but the diffusion-only variant)
	int three_step_cols;   // columns per lane of the model's three-step kernel, 0 where there is none (kThreeStepCols)
	bool block_strip_two;  // the block is the strip of the one-column two-step kernel (kCoop<Real, MODEL, 1, 2>)
	bool block_strip_three;  // ... of the three-step kernel (kCoop<Real, MODEL, 1, 3>)
	bool can_wide;         // the three-step kernel has the eight-wide form (kCanWide<Real, MODEL, 1, 3>)
	bool scalar_rows;      // the three-step kernel addresses rows by 32-bit offsets into the plane (kScalarRows)
};

// Where a launch is asked for: the slab, and what of the call bears on the steps it can take.
struct StepSite {
	int nx, nyl;
	bool wrap;         // single slab: phi wraps inside it
	bool embed;        // an embedded error estimate: single steps
	bool addressable;  // fused_scalar_rows_addressable(nx, fused_addressed_rows(d), real_bytes)
	bool absorbing;    // some stage of some step of the launch has the absorbing rows on
};

// THE rule for the steps one launch can take where `want` (1 .. 3) are asked for: three only where the three-step kernel exists (FHN: fp64
// with one column per lane, fp32 with two -- an even nx) and on a single slab (rows wrap; the exchange cycles of multi-slab runs step
// pairs) -- in fp32, a strip per wavefront, the slabs of a multi-slab run too, inside their exchange cycles: the fp64 block strip
// measured nothing on a rank's share and keeps pairs there --, else two where the two-step kernels do, else one.
// (The fp64 block strip addresses its rows by 32-bit offsets into the plane, kScalarRows: beyond that span, pairs.  fp32: the three-step
// pipeline with the absorbing-row selects does not fit the registers -- 256 and scratch; the steppers step such triples as a pair and a
// single step, crd_schedule.h: launch_steps.)
inline int steps_per_launch(const KernelTraits &k, const StepSite &s, int want)
{
	if (s.embed) return 1;  // (several steps per launch: plain steps only)
	const bool three = k.three_step_cols != 0 && (k.three_step_cols == 1 || s.nx % 2 == 0) && (!k.scalar_rows || s.addressable) && (s.wrap || k.real_bytes == 4) &&
	                   s.nyl >= 6 * kStepHalo && !(k.real_bytes == 4 && s.absorbing);
	if (want >= 3 && three) return 3;
	return (want >= 2 && k.can_two_steps && s.nyl >= 4 * kStepHalo) ? 2 : 1;
}

// Rows may extend into the ghost region (deep-halo steps), but the pipeline reads kStepHalo rows per step beyond them: they must exist.
inline bool rows_in_reach(bool wrap, int row_begin, int row_end, int nyl, int steps)
{
	return wrap || (row_begin >= -(kGhost - steps * kStepHalo) && row_end <= nyl + (kGhost - steps * kStepHalo));
}

// Rows per work item.  Every item pays 8 apron rows, which argues for long chunks; but the wavefronts of a launch run in
// "rounds" of (resident wavefront slots) items, a partly filled last round idles most of the chip, unequal wavefront
// speeds cost about half a round at the end whatever the count, and short chunks keep the rows two phi-neighbouring items
// share in L2.  Measured on 8192^2 fp64 (147 strips, 4096 slots; 200-step medians, one process, tools/tune_fused.py):
// chunk 32 0.434 ms, 24 0.451, 50 0.463, 60 0.477, 75 0.494, 128 0.51, 1024 0.62 -- many short items win.  So: 32 rows,
// halved while the launch would not fill every slot once (an 8192 x 1024 slab, one rank's share of 8 GPUs, sweeps in
// 58.4 us with 32-row chunks and 60.5 with 16; the edge-band launches of a multi-slab step end up with 8-row chunks).
// `one_round` (a launch-plan choice, see FusedPlan): a launch that needs more than one round of resident blocks but would
// fit into one with chunks of up to 96 rows gets those longer chunks -- no tail round on an almost idle chip.
// `slots`: the resident wavefronts of the launch's kernel on the device, `cus`: its compute units.
inline int fused_chunk_rows(int slots, int cus, int nstrips, int rows, int chunk_mode, int steps = 1, int sw = kWavesPerBlock)  // 0: 32 rows, 1: one round, 2: 64 rows (two steps per launch: twice that), 3: as 1, blocks of `sw` = kWideWaves wavefronts
{
	bool one_round = chunk_mode == 1 || chunk_mode == 3;
	// Two steps per launch: 16 fill rows per chunk instead of 8, and a pipeline bound by issue, not by the memory system: 128-row
	// chunks (8192^2 fp64: 48 rows 0.301 ms per step, 64 0.289, 96 0.278, 128 0.267, 192 0.276, 256 0.276; fp32 alike,
	// profiles/r04/two_step_tune.txt); chunk mode 2 is the 64-row alternative there.
	int chunk = steps == 3 ? (chunk_mode == 2 ? 96 : 192) : steps == 2 ? (chunk_mode == 2 ? 64 : 128) : 32;  // (three steps: 24 fill rows per chunk)
	while (chunk > 8 && (long)nstrips * ((rows + chunk - 1) / chunk) < (long)slots) chunk /= 2;
	// Tiny launches: where even 8-row chunks make fewer blocks than half the CUs, 4-row chunks put twice as many CUs to work (256^2:
	// 7.3 -> 6.4 us per step; the reference's 100 x 400 Goldbeter grid: 8.2 -> 6.5).  With more blocks than that the extra apron rows
	// cost more than they bring (512^2: 8.9 -> 9.8 us, 400 x 1600: 11.1 -> 12.9; the edge bands of a ring share: no change).
	if (chunk == 8 && (long)((nstrips + kWavesPerBlock - 1) / kWavesPerBlock) * ((rows + 7) / 8) < cus / 2) chunk = 4;
	if (const char *e = tuning::knob("CRD_FUSED_ONEROUND")) one_round = std::atoi(e) != 0;  // tuning knob
	if (steps == 1 && chunk_mode == 2 && chunk == 32 && (long)nstrips * ((rows + 63) / 64) >= 2L * slots) chunk = 64;  // fewer apron rows recomputed: pays where fp64 issue binds (Goldbeter)
	if (one_round && steps == 1) {
		const long strip_blocks = (nstrips + kWavesPerBlock - 1) / kWavesPerBlock, fit = (slots / kWavesPerBlock) / strip_blocks;
		const long need = fit >= 1 ? (rows + fit - 1) / fit : 0;
		if (need > chunk && need <= 96) chunk = (int)need;
	}
	if (one_round && steps >= 2) {
		// Two steps per launch are bound by issue, and what a launch loses is its last, partly filled round of resident blocks: chunks
		// such that the launch is just under a WHOLE NUMBER of rounds -- the fewest rounds whose chunks stay within 288 rows (longer
		// ones have fewer fill rows per row; 8192^2 fp64: 128 rows = 3.6 rounds 0.2667 ms per step, 155 = 2.97 rounds 0.2617, 235 =
		// 1.96 rounds 0.2618, but 161 = 2.86 rounds 0.2669 and 241 = 1.90 rounds 0.2697; 16384^2 fp32: 128 rows 0.4948, 274 rows 0.4830;
		// a rank's share of 1024 rows: one round of 61 rows; profiles/r04/whole_rounds.txt).
		const long strip_blocks = (nstrips + sw - 1) / sw, resident_blocks = slots / sw;  // (sw: kWavesPerBlock, or the eight-wide block strip's kWideWaves)
		for (long k = 1; k <= 8; k++) {
			const long chunks = k * resident_blocks / strip_blocks;
			if (chunks < 1) continue;
			const long need = (rows + chunks - 1) / chunks;
			// (The eight-wide block strip, one block per CU: 576 rows.  8192^2 is 17 strip blocks x 15 chunks of 547 rows = 0.996 rounds of 256
			// resident blocks, 0.1954 ms per step; two rounds of 274-row chunks measured 0.2012, the four-wide plan's time -- what the wider block
			// saves in apron lanes the second round's fill rows and tail give back; profiles/r08/block_strip_eight_ab.txt.)
			if (need <= (sw == kWideWaves ? 576 : steps == 3 ? 432 : 288)) {
				if (need >= 16) chunk = (int)need;
				break;
			}
		}
	}
	if (const char *e = tuning::knob("CRD_FUSED_CHUNK")) {  // tuning knob
		const int v = std::atoi(e);
		if (v >= 1) chunk = v;
	}
	return chunk < rows ? chunk : rows;
}

// A launch plan's choices as a launch takes them (choose() below resolves what a plan asks for on the kernel and slab at hand).
struct Choice {
	int mode = 0;   // chunk mode: 0 = 32 rows, 1 = stretched to whole rounds, 2 = 64 rows, 3 = as 1 with eight wavefronts per block strip
	int remap = 0;  // block -> item mapping asked for (layout() may fall back to dispatch order)
	int cols = 1;   // grid columns per lane
	int steps = 1;  // RK4 steps per launch
	bool nt = false;  // the new state stored with the non-temporal hint
	int sw = kWavesPerBlock;  // wavefronts per block
};

// Is the block the strip -- one apron around its sw wavefronts -- in the kernel of this choice?
inline bool block_is_strip(const KernelTraits &k, int cols, int steps) { return (steps == 2 && cols == 1 && k.block_strip_two) || (steps == 3 && k.block_strip_three); }

// Strips of a launch over nx columns: a strip per wavefront of cols x 64 lanes less the apron of every step on both sides (the embedded
// estimators' fifth stage costs one more apron column per side), or, the block as the strip, per block of sw wavefronts.
inline int strip_count(const KernelTraits &k, int nx, int cols, int steps, bool embed, int sw)
{
	if (block_is_strip(k, cols, steps)) {
		const int block_valid = sw * kLanes - 2 * steps * kApron;
		return sw * ((nx + block_valid - 1) / block_valid);
	}
	const int valid = cols * kLanes - 2 * steps * (embed ? kApron + 1 : kApron);
	return (nx + valid - 1) / valid;
}

// What a plan's (chunk mode, mapping, columns, store hint, steps) become on this kernel and slab; sw_plain: the block's width where the
// eight-wide kernel does not run (kWavesPerBlock, or a tuning knob's).
inline Choice choose(const KernelTraits &k, const StepSite &site, int sw_plain, int mode, int remap, int want_cols, int want_nt, int want_steps)
{
	// two columns per lane need an even nx (a pair must not straddle the periodic seam; rows then are 8- / 16-byte aligned too)
	const bool cols2_ok = !site.embed && site.nx % 2 == 0;
	Choice c;
	c.steps = steps_per_launch(k, site, want_steps);
	c.nt = want_nt != 0;
	if (const char *e = tuning::knob("CRD_FUSED_NT")) c.nt = std::atoi(e) != 0;
	c.cols = (want_cols == 2 && cols2_ok) ? 2 : 1;
	if (const char *e = tuning::knob("CRD_FUSED_COLS")) c.cols = (std::atoi(e) == 2 && cols2_ok) ? 2 : 1;
	if (c.steps == 3) c.cols = k.three_step_cols;  // (the three-step pipeline has ONE form per model and precision)
	// Chunk mode 3, the eight-wide block strip: where the launch is the three-step fp64 FHN kernel's (kCanWide); everywhere else mode 1.
	const bool wide = mode == 3 && k.can_wide && c.steps == 3 && c.cols == 1 && !site.embed && sw_plain == kWavesPerBlock;
	c.mode = (mode == 3 && !wide) ? 1 : mode;
	c.remap = remap;
	c.sw = wide ? kWideWaves : sw_plain;
	return c;
}

// The geometry fields of the kernels' FusedArgs.
struct Geometry {
	int nstrips, chunk, nchunks, first2;
	int r_begin[2], r_end[2];
	int nitems, nblocks;
	int remap;     // the mapping the launch runs: 2 falls back to 0 where its lanes cannot be formed
	int xs_lanes;  // mapping 2: phi-lanes of chunk sequences per strip block and XCD
	int sw;
};

// Cuts the rows R = [R[0], R[1]) and, if non-empty, [R[2], R[3]) into items as the choice says, in blocks of `sw` wavefronts (the choice's,
// or the band cut's for one of its launches).  `slots`: resident wavefronts of the choice's kernel; chunk_override > 0: that many rows per item.
inline Geometry layout(const KernelTraits &k, int slots, int cus, int nx, bool embed, const int R[4], const Choice &c, int sw, int chunk_override)
{
	Geometry g;
	g.sw = sw;
	g.nstrips = strip_count(k, nx, c.cols, c.steps, embed, sw);
	const int rows_a = R[1] - R[0], rows_b = R[3] - R[2];
	const int nsb = (g.nstrips + sw - 1) / sw;
	g.chunk = chunk_override > 0 ? std::min(chunk_override, rows_a + rows_b) : fused_chunk_rows(slots, cus, g.nstrips, rows_a + rows_b, c.mode, c.steps, sw);
	const int n1 = (rows_a + g.chunk - 1) / g.chunk, n2 = (rows_b + g.chunk - 1) / g.chunk;
	g.nchunks = n1 + n2;
	g.first2 = n2 > 0 ? n1 : g.nchunks;
	g.r_begin[0] = R[0];
	g.r_end[0] = R[1];
	g.r_begin[1] = R[2];
	g.r_end[1] = R[3];
	g.nitems = g.nstrips * g.nchunks;
	g.nblocks = nsb * g.nchunks;
	g.remap = c.remap;
	if (const char *e = tuning::knob("CRD_FUSED_REMAP")) g.remap = std::atoi(e);
	g.xs_lanes = 1;
	if (g.remap == 2) {
		const int per_xcd = slots / sw / kNumXcd;
		if (rows_b > 0 || g.nchunks < 2 * kNumXcd || per_xcd < nsb) {
			g.remap = 0;  // two row ranges, or too few chunks / slots for lanes: plain order
		} else {
			g.xs_lanes = per_xcd / nsb;
			const int most = (g.nchunks + kNumXcd - 1) / kNumXcd;  // chunks of the best-served XCD
			g.nblocks = kNumXcd * ((most + g.xs_lanes - 1) / g.xs_lanes) * nsb * g.xs_lanes;
		}
	}
	return g;
}

// Several steps per launch with absorbing rows on: the rows whose pipeline can meet a global boundary row -- within steps x kApron rows of
// global rows ny - 1 / 0, one period down, here, or one period up -- go out as launches of the kernel with the selects, the rest as
// launches of the select-free one (crd_fused_launch.h: fire_banded has the measurements).  Pieces are [begin, end) in local rows, in order.
struct BandCut {
	int with_sel[4][2], without[6][2];
	int n_with = 0, n_without = 0;
	bool fits = true;  // false: more than 4 / 6 pieces would be needed (the caller launches the kernel with the selects over everything)
};
inline BandCut cut_bands(const int want[4], int js, int ny, int steps)
{
	BandCut b;
	for (int r = 0; r < 2 && b.fits; r++) {
		int cursor = want[2 * r];
		const int end = want[2 * r + 1];
		for (int g = -1; g <= 1 && cursor < end; g++) {  // local rows of global rows ny - 1 and 0, one period down / here / one up
			const int jb = (ny - 1 - js) + g * ny, lo = std::max(cursor, jb - steps * kApron), hi = std::min(end, jb + 2 + steps * kApron);
			if (lo >= hi) continue;
			if (cursor < lo) {
				if (b.n_without == 6) b.fits = false;
				else b.without[b.n_without][0] = cursor, b.without[b.n_without++][1] = lo;
			}
			if (b.n_with == 4) b.fits = false;
			else b.with_sel[b.n_with][0] = lo, b.with_sel[b.n_with++][1] = hi;
			cursor = hi;
		}
		if (cursor < end) {
			if (b.n_without == 6) b.fits = false;
			else b.without[b.n_without][0] = cursor, b.without[b.n_without++][1] = end;
		}
	}
	return b;
}

// Launch-plan candidates the autotuner times: (chunks stretched to one round?, block -> item mapping).  Workgroups are dealt
// round-robin to the 8 XCDs, each with its own L2.  Mapping 0 walks the items theta-first in dispatch order: neighbouring
// items land on different XCDs and every apron column and row is fetched from beyond L2 by both items that need it (PMC:
// 39.5 B per point, reads 1.47 x the plane).  Mapping 1 gives each XCD one contiguous run of items, i.e. a contiguous band of
// the slab: theta-neighbours share an L2 and the apron columns are fetched once (36.6 B per point, reads 1.29 x).  Mapping 2
// adds succession in phi -- the workgroup that takes a finished one's place continues with the next chunk in phi, whose first
// rows its predecessor has just pulled into that L2 (34.9 B per point, reads 1.18 x).  Which plan is fastest depends on the
// grid shape AND on the device: on 8192^2 fp64 mapping 1 measured -6.3 %, -0.7 % and +1.7 % against mapping 0 on three
// MI355X of the same pool, mapping 2 -4.4 % on a fourth; one-round chunks -10 % (4096 x 1024) to +2 % (16384 x 2048 fp32) --
// hence measured at run time, on the device and the shape at hand.  Every candidate computes bit-identical results.
// Third dimension (round 3): columns per lane.  Two columns per lane halve the DPP moves and the apron share of a strip (8 of 128
// columns instead of 8 of 64) and, in fp32, use the packed arithmetic; they also halve the wavefronts in flight for the same
// bytes.  Which wins is again a matter of the kernel (fp32 / Goldbeter are issue-bound, FHN fp64 is not) and of the device.
// Fourth dimension (round 3, late): non-temporal stores of the new state (row_store).  They keep L2 for what items share; which
// mapping is fastest changes with them (the plain mapping gains most), so they are timed in combination.
struct PlanCandidate {
	int one_round, remap, cols, nt;  // one_round: the chunk mode -- 0 = 32 rows, 1 = stretched to one round, 2 = 64 rows, 3 = as 1 with eight wavefronts per block strip (kWideWaves)
	int steps = 1;                   // RK4 steps per launch (2: fused_item_two_steps)
};
// (round 4: 64-row chunks also under mappings 1 / 2 and with two columns per lane -- where fp64 issue binds, Goldbeter, the recompute
// factor of the apron rows is what is left to cut: (64 + 8) / 64 x 128 / 120 = 1.20 against (32 + 8) / 32 x 64 / 56 = 1.43)
constexpr PlanCandidate kPlanCandidates[] = {
    {0, 0, 1, 0}, {0, 1, 1, 0}, {0, 2, 1, 0}, {1, 0, 1, 0}, {1, 1, 1, 0}, {2, 0, 1, 0}, {2, 1, 1, 0}, {2, 2, 1, 0},
    {0, 0, 2, 0}, {0, 1, 2, 0}, {0, 2, 2, 0}, {1, 0, 2, 0}, {1, 1, 2, 0}, {2, 0, 2, 0}, {2, 1, 2, 0}, {2, 2, 2, 0},
    {0, 0, 1, 1}, {0, 1, 1, 1}, {0, 2, 1, 1}, {1, 0, 1, 1}, {1, 1, 1, 1}, {2, 0, 1, 1}, {2, 1, 1, 1}, {2, 2, 1, 1},
    {0, 0, 2, 1}, {0, 1, 2, 1}, {0, 2, 2, 1}, {1, 0, 2, 1}, {1, 1, 2, 1}, {2, 0, 2, 1}, {2, 1, 2, 1}, {2, 2, 2, 1},
    // fifth dimension (round 4): two steps per launch (128-row chunks, or 64), non-temporal stores
    {0, 0, 1, 1, 2}, {0, 1, 1, 1, 2}, {0, 2, 1, 1, 2}, {1, 0, 1, 1, 2}, {1, 1, 1, 1, 2}, {2, 1, 1, 1, 2},
    {0, 0, 2, 1, 2}, {0, 1, 2, 1, 2}, {0, 2, 2, 1, 2}, {1, 0, 2, 1, 2}, {1, 1, 2, 1, 2}, {2, 1, 2, 1, 2},
    // sixth (round 6): three steps per launch, the block as the strip (FHN fp64: kCanThreeSteps), non-temporal stores
    // (whole-rounds chunks win by 7 % -- 293 rows = two rounds of resident blocks on 8192^2 against 192 rows = three and a bit --, plain
    // stores by half a per cent on some boxes)
    {0, 0, 1, 1, 3}, {0, 1, 1, 1, 3}, {0, 2, 1, 1, 3}, {1, 0, 1, 1, 3}, {1, 1, 1, 1, 3}, {1, 0, 1, 0, 3}, {1, 1, 1, 0, 3},
    // (round 8) ... and its eight-wide form, chunk mode 3: 488 valid lanes of 512, one block per CU, whole rounds of 256 resident blocks
    // (8192^2: -2.9 / -3.3 % against the best four-wide plan in two runs; 4096^2, where 9 x 488 columns waste what 18 x 232 do: +2.4 / +3.0 %.  Plain stores: +0.5 %,
    // no candidate.  profiles/r08/block_strip_eight_ab.txt)
    {3, 0, 1, 1, 3}, {3, 1, 1, 1, 3}, {3, 2, 1, 1, 3},
    // ... and in fp32: two columns per lane, a strip per wavefront (kThreeStepCols)
    {0, 0, 2, 1, 3}, {0, 1, 2, 1, 3}, {0, 2, 2, 1, 3}, {1, 0, 2, 1, 3}, {1, 1, 2, 1, 3}, {2, 1, 2, 1, 3}};
constexpr int kNumPlanCandidates = (int)(sizeof kPlanCandidates / sizeof kPlanCandidates[0]);

// Is candidate k worth timing on this launch?  c, g: what choose() and layout() made of it; chunk_plain: the rows per item of a 32-row plan
// (chunk mode 0) with c's strips, columns and steps; steps_ok: the steps per launch the tuner may try here (1 .. 3).
inline bool candidate_live(int k, const KernelTraits &t, const Choice &c, const Geometry &g, int chunk_plain, int steps_ok)
{
	const PlanCandidate &p = kPlanCandidates[k];
	if (k == 0) return true;
	if (p.one_round && g.chunk == chunk_plain) return false;  // (same as a 32-row plan)
	if (p.one_round != c.mode) return false;                  // (chunk mode 3 where the eight-wide kernel does not run: that is mode 1's candidate)
	if (p.steps != (p.steps <= steps_ok ? c.steps : 1)) return false;  // (several steps per launch: plain steps)
	if (c.steps == 2 && c.cols == 2 && t.real_bytes == 8) return false;  // (256 VGPRs, one wavefront per SIMD: measured 0.347 against 0.312 ms)
	if (p.remap != g.remap) return false;                     // (the mapping fell back to dispatch order)
	if (p.cols != c.cols) return false;                       // (two columns per lane not possible here, or pinned by a knob)
	if ((p.nt != 0) != c.nt) return false;                    // (pinned by a knob)
	return true;
}

}  // namespace plan
}  // namespace crd
