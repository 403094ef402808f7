// The launch-plan arithmetic of the one-launch step (crdmodel_amd/csrc/crd_fused_plan.h) against expectations written out here: the
// project's recorded plans (docs/HISTORY.md), the band cut, the strip count, the XCD mapping's fallback, the one rule for the
// steps a launch can take against the four statements it replaced, and the ghost-row reach.  Plain C++17, no device.
#include <cstdio>
#include <set>

#include "crd_fused_plan.h"

using namespace crd;
using namespace crd::plan;

static int failures = 0;
#define CHECK(cond)                                                        \
	do {                                                                   \
		if (!(cond)) {                                                     \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			failures++;                                                    \
		}                                                                  \
	} while (0)

// the kernels' traits as crd_fused_launch.h fills them (kCoop, kCanWide, kThreeStepCols, kScalarRows)
static const KernelTraits kFhn64{8, true, 1, false, true, true, true}, kFhn32{4, true, 2, false, false, false, false};
static const KernelTraits kGb64{8, true, 0, true, true, false, false}, kGb32{4, true, 0, false, false, false, false};
static const KernelTraits kDiff64{8, false, 0, false, true, false, false};
constexpr int kCus = 256;  // an MI355X; slots = 256 CUs x 4 SIMDs x wavefronts per SIMD

static void recorded_plans()
{
	// 8192^2 fp64 FHN, three steps, four wide: 144 strips, 293-row chunks = two rounds of resident blocks
	CHECK(strip_count(kFhn64, 8192, 1, 3, false, 4) == 144);
	CHECK(fused_chunk_rows(2048, kCus, 144, 8192, 1, 3, 4) == 293);
	// ... eight wide: 17 strip blocks x 15 chunks of 547 rows
	CHECK(strip_count(kFhn64, 8192, 1, 3, false, 8) == 17 * 8);
	CHECK(fused_chunk_rows(2048, kCus, 136, 8192, 3, 3, 8) == 547);
	{
		const int R[4] = {0, 8192, 0, 0};
		const StepSite site{8192, 8192, true, false, true, false};
		const Choice c = choose(kFhn64, site, 4, 3, 0, 1, 1, 3);
		CHECK(c.mode == 3 && c.sw == 8 && c.steps == 3 && c.cols == 1 && c.nt);
		const Geometry g = layout(kFhn64, 2048, kCus, 8192, false, R, c, c.sw, 0);
		CHECK(g.chunk == 547 && g.nchunks == 15 && g.nblocks == 17 * 15 && g.nitems == 136 * 15 && g.first2 == 15 && g.remap == 0);
	}
	// 4096^2, three steps, four wide
	CHECK(fused_chunk_rows(2048, kCus, strip_count(kFhn64, 4096, 1, 3, false, 4), 4096, 1, 3, 4) == 147);
	// 8192^2 fp64, two steps, one round: 171 strips, 235 rows
	CHECK(strip_count(kFhn64, 8192, 1, 2, false, 4) == 171);
	CHECK(fused_chunk_rows(3072, kCus, 171, 8192, 1, 2, 4) == 235);
	// a rank's share, 8192 x 1024: one round of 61-row chunks, 43 x 17 = 731 blocks
	{
		const int R[4] = {0, 1024, 0, 0};
		const Choice c = choose(kFhn64, StepSite{8192, 1024, false, false, true, false}, 4, 1, 0, 1, 1, 2);
		const Geometry g = layout(kFhn64, 3072, kCus, 8192, false, R, c, c.sw, 0);
		CHECK(c.steps == 2 && g.nstrips == 171 && g.chunk == 61 && g.nchunks == 17 && g.nblocks == 43 * 17 && g.nblocks == 731);
	}
	// 8192^2 fp64, one step: 147 strips, 32 rows
	CHECK(strip_count(kFhn64, 8192, 1, 1, false, 4) == 147);
	CHECK(fused_chunk_rows(4096, kCus, 147, 8192, 0, 1, 4) == 32);
	// tiny launches: 256^2 takes 4-row chunks (2 strip blocks x 32 items of 8 rows < 128), 512^2 does not (3 x 64)
	CHECK(fused_chunk_rows(4096, kCus, strip_count(kFhn64, 256, 1, 1, false, 4), 256, 0, 1, 4) == 4);
	CHECK(fused_chunk_rows(4096, kCus, strip_count(kFhn64, 512, 1, 1, false, 4), 512, 0, 1, 4) == 8);
}

// ---- band cut ----
static bool near_boundary(int j, int js, int ny, int steps)
{
	// within steps x kApron rows of a global row ny - 1 or 0, one period down, here, or one period up
	for (int g = -1; g <= 1; g++) {
		const int last = (ny - 1 - js) + g * ny, first = last + 1;  // local rows of global rows ny - 1 and (the next period's) 0
		if (j >= last - steps * kApron && j <= first + steps * kApron) return true;
	}
	return false;
}

static void check_cut(const int want[4], int js, int ny, int steps)
{
	const BandCut b = cut_bands(want, js, ny, steps);
	// pieces needed, counted on the rows themselves: a with-select piece per (range, period) whose band has rows no earlier band took;
	// a select-free piece per maximal run of rows away from every boundary
	int need_with = 0, need_without = 0;
	for (int r = 0; r < 2; r++) {
		std::set<int> taken;
		for (int g = -1; g <= 1; g++) {
			bool fresh = false;
			const int last = (ny - 1 - js) + g * ny;
			for (int j = want[2 * r]; j < want[2 * r + 1]; j++)
				if (j >= last - steps * kApron && j <= last + 1 + steps * kApron && taken.insert(j).second) fresh = true;
			need_with += fresh;
		}
		for (int j = want[2 * r]; j < want[2 * r + 1]; j++)
			if (!near_boundary(j, js, ny, steps) && (j == want[2 * r] || near_boundary(j - 1, js, ny, steps))) need_without++;
	}
	CHECK(b.fits == (need_with <= 4 && need_without <= 6));
	if (!b.fits) return;
	CHECK(b.n_with == need_with && b.n_without == need_without);
	// the pieces partition the requested rows exactly and in order
	// (walking the rows: the next row is the head of the next piece of one of the two lists, each in order, and no piece crosses a range's end)
	int w = 0, p = 0;
	for (int r = 0; r < 2; r++)
		for (int j = want[2 * r]; j < want[2 * r + 1];) {
			const bool with = w < b.n_with && b.with_sel[w][0] == j, without = !with && p < b.n_without && b.without[p][0] == j;
			CHECK(with || without);
			if (!with && !without) return;
			const int end = with ? b.with_sel[w++][1] : b.without[p++][1];
			CHECK(end > j && end <= want[2 * r + 1]);
			if (end <= j) return;
			for (; j < end; j++) CHECK(near_boundary(j, js, ny, steps) == with);  // every row near a boundary goes out with the selects, no other row
		}
	CHECK(w == b.n_with && p == b.n_without);
}

static void band_cut()
{
	{
		const int want[4] = {0, 1024, 0, 0};
		const BandCut b = cut_bands(want, 0, 1024, 2);
		CHECK(b.fits && b.n_with == 2 && b.n_without == 1);
		CHECK(b.with_sel[0][0] == 0 && b.with_sel[0][1] == 9 && b.with_sel[1][0] == 1015 && b.with_sel[1][1] == 1024);
		CHECK(b.with_sel[0][1] - b.with_sel[0][0] + b.with_sel[1][1] - b.with_sel[1][0] == 18);
		CHECK(b.without[0][0] == 9 && b.without[0][1] == 1015);
	}
	int cases = 0, misfits = 0;
	for (int ny : {24, 25, 64, 1024})
		for (int steps = 2; steps <= 3; steps++)
			for (int nyl : {ny, ny / 2})
				for (int js = 0; js < ny; js += (ny == 1024 ? 61 : 1)) {
					const int reach = std::min(kGhost, nyl);  // (ghost rows are at most a slab)
					const int ranges[][4] = {{0, nyl, 0, 0}, {-reach, nyl + reach, 0, 0}, {-reach, 0, nyl, nyl + reach}, {-reach / 2, 3, nyl - 3, nyl + reach / 2},
					                         {-nyl, nyl, 0, 2 * nyl}, {-nyl, 2 * nyl, -nyl, 2 * nyl}};  // (the last two: as many bands as fit, and more)
					for (const auto &want : ranges) {
						check_cut(want, js, ny, steps);
						misfits += !cut_bands(want, js, ny, steps).fits;
						cases++;
					}
				}
	CHECK(cases > 1000);
	CHECK(misfits > 0 && misfits < cases);  // (the sweep meets both answers)
}

static void strip_counts()
{
	for (int nx = 24; nx <= 2048; nx++) {
		for (int waves : {4, 8}) {
			const int valid2 = waves * 64 - 2 * 2 * 4, valid3 = waves * 64 - 2 * 3 * 4;
			CHECK(strip_count(kGb64, nx, 1, 2, false, waves) == waves * ((nx + valid2 - 1) / valid2));
			CHECK(strip_count(kFhn64, nx, 1, 3, false, waves) == waves * ((nx + valid3 - 1) / valid3));
		}
		for (int cols = 1; cols <= 2; cols++)
			for (int steps = 1; steps <= 3; steps++) {
				const int valid = cols * 64 - 2 * steps * 4;
				CHECK(strip_count(kFhn32, nx, cols, steps, false, 4) == (nx + valid - 1) / valid);
				if (!(steps == 2 && cols == 1)) CHECK(strip_count(kGb32, nx, cols, steps, false, 4) == (nx + valid - 1) / valid);
			}
		CHECK(strip_count(kFhn64, nx, 1, 2, false, 4) == (nx + 47) / 48);  // (FHN pairs keep a strip per wavefront)
		CHECK(strip_count(kFhn64, nx, 1, 1, true, 4) == (nx + 53) / 54);   // the embedded kernels: an apron of 5
		CHECK(strip_count(kGb32, nx, 1, 1, true, 4) == (nx + 53) / 54);
	}
}

static void mapping_two()
{
	const StepSite site{8192, 8192, true, false, true, false};
	const Choice c = choose(kFhn64, site, 4, 0, 2, 1, 0, 1);
	CHECK(c.remap == 2 && c.steps == 1 && c.cols == 1 && c.sw == 4);
	const int one[4] = {0, 8192, 0, 0}, two[4] = {0, 4096, 4096, 8192}, few[4] = {0, 15 * 32, 0, 0}, enough[4] = {0, 16 * 32, 0, 0};
	// 147 strips = 37 strip blocks, 4096 slots: 128 blocks per XCD, 3 lanes; 256 chunks, 32 of each XCD
	Geometry g = layout(kFhn64, 4096, kCus, 8192, false, one, c, 4, 0);
	CHECK(g.remap == 2 && g.xs_lanes == 3 && g.nchunks == 256 && g.nblocks == 8 * ((32 + 2) / 3) * 37 * 3);
	g = layout(kFhn64, 4096, kCus, 8192, false, two, c, 4, 0);  // two row ranges: plain order
	CHECK(g.remap == 0 && g.xs_lanes == 1 && g.nblocks == 37 * g.nchunks && g.first2 == 128);
	g = layout(kFhn64, 4096, kCus, 8192, false, few, c, 4, 32);  // fewer than 16 chunks
	CHECK(g.nchunks == 15 && g.remap == 0 && g.nblocks == 37 * 15);
	g = layout(kFhn64, 4096, kCus, 8192, false, enough, c, 4, 32);
	CHECK(g.nchunks == 16 && g.remap == 2 && g.nblocks == 8 * 1 * 37 * 3);
	g = layout(kFhn64, 1024, kCus, 8192, false, one, c, 4, 0);  // 32 resident blocks per XCD < 37 strip blocks
	CHECK(g.remap == 0 && g.xs_lanes == 1);
	for (int slots : {1024, 2048, 3072, 4096})
		for (int nx : {232, 2048, 8192})
			for (int rows : {64, 1024, 8192}) {
				const int R[4] = {0, rows, 0, 0};
				g = layout(kFhn64, slots, kCus, nx, false, R, c, 4, 0);
				const int nsb = (g.nstrips + 3) / 4, per_xcd = slots / 4 / 8;
				if (g.nchunks < 16 || per_xcd < nsb) {
					CHECK(g.remap == 0 && g.nblocks == nsb * g.nchunks);
				} else {
					const int most = (g.nchunks + 7) / 8;
					CHECK(g.remap == 2 && g.xs_lanes == per_xcd / nsb && g.nblocks == 8 * ((most + g.xs_lanes - 1) / g.xs_lanes) * nsb * g.xs_lanes);
				}
			}
}

// ---- steps per launch: the four statements the one rule replaced, as they stood ----
struct Row {
	int precision_bytes, model;  // model: 0 FHN, 1 Goldbeter, 2 diffusion only
	int nx, nyl;
	bool wrap, addressable, absorbing;
};
static bool can3(const Row &r) { return r.model == 0; }
static int cols3(const Row &r) { return r.model == 0 ? (r.precision_bytes == 8 ? 1 : 2) : 0; }
static int old_supported(const Row &r, int want)  // crd_fused.hip: fused_steps_supported
{
	bool three = r.model == 0 && (r.precision_bytes == 8 || r.nx % 2 == 0);
	if (r.precision_bytes == 8 && !r.addressable) three = false;
	if (want >= 3 && three && (r.wrap || r.precision_bytes != 8) && r.nyl >= 6 * kStepHalo) return 3;
	return (want >= 2 && r.nyl >= 4 * kStepHalo && r.model != 2) ? 2 : 1;
}
static bool old_validation_accepts(const Row &r, int steps, bool embed)  // the top of launch_fused_t
{
	if (steps != 1 && (embed || !((steps == 2 && r.model != 2) || (steps == 3 && can3(r) && (cols3(r) == 1 || r.nx % 2 == 0))))) return false;
	if (steps == 3 && r.precision_bytes == 8 && r.model != 2 && !r.addressable) return false;
	if (steps == 3 && r.precision_bytes == 4 && r.absorbing) return false;
	return true;
}
static int old_configure(const Row &r, int want, bool embed)  // configure
{
	const bool cols2_ok = !embed && r.nx % 2 == 0;
	return (want == 3 && can3(r) && (cols3(r) == 1 || cols2_ok)) ? 3 : (want >= 2 && r.model != 2) ? 2 : 1;
}
static int old_tuner_steps(const Row &r, bool embed, int call_steps)  // two_steps_ok / three_steps_ok, with room for the rows
{
	const bool cols2_ok = !embed && r.nx % 2 == 0;
	const bool two = r.model != 2 && !embed && call_steps == 1 && r.nyl >= 4 * kStepHalo;
	const bool three = two && can3(r) && (cols3(r) == 1 || cols2_ok) && r.nyl >= 6 * kStepHalo && (r.wrap || r.precision_bytes == 4) &&
	                   (!(r.precision_bytes == 8 && r.model == 0) || r.addressable) && !(r.precision_bytes == 4 && r.absorbing);
	return three ? 3 : two ? 2 : 1;
}

static void steps_and_reach()
{
	const KernelTraits *traits[2][3] = {{&kFhn64, &kGb64, &kDiff64}, {&kFhn32, &kGb32, nullptr}};
	int rows = 0;
	for (int p = 0; p < 2; p++)
		for (int model = 0; model < 3; model++)
			for (int nx : {232, 233})
				for (int wrap = 0; wrap < 2; wrap++)
					for (int nyl : {7, 8, 15, 16, 23, 24})
						for (int addressable = 0; addressable < 2; addressable++)
							for (int absorbing = 0; absorbing < 2; absorbing++) {
								if (!traits[p][model]) continue;
								const KernelTraits &k = *traits[p][model];
								const Row r{p == 0 ? 8 : 4, model, nx, nyl, wrap != 0, addressable != 0, absorbing != 0};
								const StepSite site{nx, nyl, wrap != 0, false, addressable != 0, absorbing != 0}, quiet{nx, nyl, wrap != 0, false, addressable != 0, false};
								StepSite embedded = site;
								embedded.embed = true;
								rows++;
								for (int want = 1; want <= 3; want++) {
									const int got = steps_per_launch(k, site, want);
									CHECK(steps_per_launch(k, quiet, want) == old_supported(r, want));
									CHECK(steps_per_launch(k, embedded, want) == 1 && old_validation_accepts(r, want, true) == (want == 1));
									// what the rule grants, the old validation accepted and the old configure took as asked; and what the steppers
									// ask for (old_supported) the old validation refused only where the rule refuses too
									if (got == want) CHECK(old_validation_accepts(r, want, false) && old_configure(r, want, false) == want);
									if (old_supported(r, want) == want && old_validation_accepts(r, want, false)) CHECK(got == want);
								}
								int tuner = 1;
								for (int n = 2; n <= 3; n++)
									if (tuner == n - 1 && steps_per_launch(k, site, n) == n) tuner = n;
								CHECK(tuner == old_tuner_steps(r, false, 1));
								CHECK(old_tuner_steps(r, true, 1) == 1);
							}
	CHECK(rows == 5 * 2 * 2 * 6 * 2 * 2);
	// The recorded fault: a two-step candidate on the first launch of a 16-step cycle, rows from -60: it reads row -68 of 64 ghost rows.
	CHECK(rows_in_reach(false, -60, 1024 + 60, 1024, 1));
	CHECK(!rows_in_reach(false, -60, 1024 + 60, 1024, 2));
	CHECK(rows_in_reach(false, -56, 1024 + 56, 1024, 2) && !rows_in_reach(false, -57, 1024 + 56, 1024, 2) && !rows_in_reach(false, -56, 1024 + 57, 1024, 2));
	CHECK(rows_in_reach(false, -52, 1024 + 52, 1024, 3) && !rows_in_reach(false, -53, 1024 + 52, 1024, 3));
	CHECK(rows_in_reach(true, -60, 1024 + 60, 1024, 3));  // (a single slab wraps)
}

static void candidates()
{
	CHECK(kNumPlanCandidates == 60);
	CHECK(kPlanCandidates[0].one_round == 0 && kPlanCandidates[0].remap == 0 && kPlanCandidates[0].cols == 1 && kPlanCandidates[0].nt == 0 && kPlanCandidates[0].steps == 1);
	CHECK(kPlanCandidates[51].one_round == 3 && kPlanCandidates[51].steps == 3 && kPlanCandidates[59].cols == 2 && kPlanCandidates[59].steps == 3);
	// 8192^2 fp64 FHN: what the tuner times
	const StepSite site{8192, 8192, true, false, true, false};
	const int R[4] = {0, 8192, 0, 0}, slots_of_steps[4] = {0, 4096, 3072, 2048};
	int live = 0, live_wide = 0, live_two_cols_pairs = 0;
	for (int k = 0; k < kNumPlanCandidates; k++) {
		const PlanCandidate &p = kPlanCandidates[k];
		const Choice c = choose(kFhn64, site, 4, p.one_round, p.remap, p.cols, p.nt, p.steps);
		const int slots = slots_of_steps[c.steps];
		const Geometry g = layout(kFhn64, slots, kCus, 8192, false, R, c, c.sw, 0);
		const bool is_live = candidate_live(k, kFhn64, c, g, fused_chunk_rows(slots, kCus, g.nstrips, 8192, 0, c.steps), 3);
		live += is_live;
		live_wide += is_live && p.one_round == 3;
		live_two_cols_pairs += is_live && p.steps == 2 && p.cols == 2;
		if (p.steps == 3 && p.cols == 2) CHECK(!is_live);  // (fp64 triples have one column per lane: the fp32 candidates are not this kernel's)
		if (p.steps >= 2) CHECK(!candidate_live(k, kFhn64, choose(kFhn64, site, 4, p.one_round, p.remap, p.cols, p.nt, 1), g, 0, 1));  // (no room, or a call of several steps)
	}
	// (eight wide under mapping 2 is not timed here: 15 chunks are fewer than two per XCD, the mapping falls back to dispatch order, which
	// is candidate 51's; fp64 pairs with two columns per lane never are)
	CHECK(live_wide == 2 && live_two_cols_pairs == 0 && live > 20 && live < kNumPlanCandidates);
}

int main()
{
	recorded_plans();
	band_cut();
	strip_counts();
	mapping_two();
	steps_and_reach();
	candidates();
	if (failures) {
		std::printf("%d check(s) failed\n", failures);
		return 1;
	}
	std::printf("fused plan selftest ok\n");
	return 0;
}
