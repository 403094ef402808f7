// crd_observe.hip -- observers: per-member statistics, probes and maps of an ensemble's current state, recorded on the device
// (crd_ensemble.cpp drives them; crd_state_observe runs the same sampling kernel on a single-slab context).  Two launches per sample:
//   sampling   grid (G blocks per member, B members): a block strides over its member's two planes and writes ONE partial record
//              (min, max, sum, sum of squares of each field, in fp64 whatever the state's precision); with maps on, the same pass
//              folds the activator it has just read into the member's three map planes;
//   finishing  one workgroup per member: adds the member's G partials in index order into the sample's row of the record buffer and
//              gathers the probe values into the same row.
// No floating-point atomics and no "last block" ticket: which lane takes which point, and the order of every addition, depend on
// the plane's size alone -- not on the member count, not on the alignment of the planes (the 16-byte and the element-wise loads
// serve the same points to the same lanes) -- so a row is the same bits from run to run, in an ensemble of 1 and of 64, and from
// crd_state_observe.  Reads the state and nothing else of the stepping: the step kernels do not know observers exist.
// With cycle maps the sampling pass also folds the activator into four more planes per member (previous sample, count of upward
// crossings of a threshold, time of the first and of the last): further instantiations of the same body, so the state is still read once.
// With sections a third launch follows the finishing one: lines of both fields along a row or a column, and the means over theta of
// every row and over phi of every column, written as doubles behind the sample's rows (crd_observe_sections_kernel below; the same
// rule: the partition of a mean is a function of nx and ny alone).
// DESIGN.md, "Ensembles" (observers).
#include "crd_device.h"
#include "crd_ensemble.h"

namespace crd {

using dev::clear_launch_status;
using dev::launch_status;

namespace {

typedef const __attribute__((address_space(4))) EnsembleMember ConstMember;

constexpr int kObserveThreads = 256;

template <typename Real> struct Wide;
template <> struct Wide<double> { using type = double2; static constexpr int n = 2; };
template <> struct Wide<float> { using type = float4; static constexpr int n = 4; };

// NaN propagates through both (the rule of crd_max_abs_kernel): once an operand is NaN the result is, whichever side it is on.
__device__ __forceinline__ double nan_min(double m, double x) { return (x < m || x != x) ? x : m; }
__device__ __forceinline__ double nan_max(double m, double x) { return (x > m || x != x) ? x : m; }

// One field's statistics in a lane: V interleaved accumulators (element e of every 16-byte group goes to accumulator e), so that a
// point passes through at most ceil(points / (V lanes G)) - 1 additions here and log2 V in fold().
template <int V>
struct FieldStats {
	double mn, mx, s[V], q[V];
	__device__ __forceinline__ void clear()
	{
		mn = INFINITY;
		mx = -INFINITY;
		for (int e = 0; e < V; e++) s[e] = q[e] = 0.0;
	}
	__device__ __forceinline__ void take(int e, double x)
	{
		mn = nan_min(mn, x);
		mx = nan_max(mx, x);
		s[e] += x;
		q[e] = fma(x, x, q[e]);
	}
	__device__ __forceinline__ void fold()  // pairwise: (0 + 1) + (2 + 3)
	{
		for (int w = 1; w < V; w *= 2)
			for (int e = 0; e + w < V; e += 2 * w) {
				s[e] += s[e + w];
				q[e] += q[e + w];
			}
	}
};

// Running minimum / maximum of the activator (np.minimum / np.maximum: NaN propagates) and the time of the first sample at which
// it is >= threshold.  A plane entry is rewritten only when it changes.
__device__ __forceinline__ void map_update(double *__restrict__ mmin, double *__restrict__ mmax, double *__restrict__ tact, size_t p, double x, double threshold,
                                           double t)
{
	const double lo = mmin[p], hi = mmax[p], ta = tact[p];
	if (x < lo || x != x) mmin[p] = x;
	if (x > hi || x != x) mmax[p] = x;
	if (ta != ta && x >= threshold) tact[p] = t;
}

// Cycle maps: upward crossings of cy.threshold by the activator between two consecutive samples, in fp64, every operation rounded once
// (contraction is off in this unit: crd_device.h).  d0 = x_prev - thr, d1 = x - thr; a crossing is d0 < 0 && d1 >= 0, at
// tc = t_prev + (t - t_prev) (-d0 / (d1 - d0)).  A NaN compares false: no crossing, and it becomes the next x_prev.  The first sample
// after begin only stores x_prev.
__device__ __forceinline__ void cycle_update(double *__restrict__ prev, double *__restrict__ tfirst, double *__restrict__ tlast, int *__restrict__ count, size_t p, double x,
                                             const ObserveCycles &cy, double t)
{
	if (!cy.first) {
		const double d0 = prev[p] - cy.threshold, d1 = x - cy.threshold;
		if (d0 < 0.0 && d1 >= 0.0) {
			const double tc = cy.t_prev + (t - cy.t_prev) * (-d0 / (d1 - d0));
			const int c = count[p];
			count[p] = c + 1;
			if (c == 0) tfirst[p] = tc;
			tlast[p] = tc;
		}
	}
	prev[p] = x;
}

// grid (G, members), kObserveThreads lanes.  Group c of V consecutive points belongs to lane (c mod 256) of block ((c / 256) mod G);
// partial record of (member, block): min u, max u, sum u, sum u^2, then v's four.  The body of every instantiation of the sampling kernel.
// G: the member's sampling blocks; slots: partial records between two members (the launch's gridDim.x; members of one shape: both).
template <typename Real, bool MAPS, bool CYCLES>
__device__ __forceinline__ void observe_sample_body(const EnsembleMember *members, int src, size_t n, double *__restrict__ partials, double *__restrict__ maps,
                                                    size_t map_plane, double threshold, double t, const ObserveCycles &cy, unsigned G, unsigned slots)
{
	constexpr int V = Wide<Real>::n;
	using Vec = typename Wide<Real>::type;
	__shared__ double part[kObserveThreads / 64][8];
	const int member = blockIdx.y;
	ConstMember *const mem = (ConstMember *)members + member;
	const Real *__restrict__ const u = static_cast<const Real *>(mem->u[src]);
	const Real *__restrict__ const v = static_cast<const Real *>(mem->v[src]);
	double *const mmin = MAPS ? maps + (size_t)member * 3 * map_plane : nullptr;
	double *const mmax = MAPS ? mmin + map_plane : nullptr;
	double *const tact = MAPS ? mmax + map_plane : nullptr;
	double *const cprev = CYCLES ? cy.planes + (size_t)member * 4 * cy.plane : nullptr;
	double *const cfirst = CYCLES ? cprev + cy.plane : nullptr;
	double *const clast = CYCLES ? cfirst + cy.plane : nullptr;
	int *const ccount = CYCLES ? reinterpret_cast<int *>(clast + cy.plane) : nullptr;
	// 16 bytes per lane and load where both of this member's planes allow it (decided per block; the result does not depend on it)
	const bool wide = (((uintptr_t)u | (uintptr_t)v) & 15) == 0;
	const size_t groups = (n + V - 1) / V, stride = (size_t)G * kObserveThreads;

	FieldStats<V> a, b;
	a.clear();
	b.clear();
	// a lane takes its groups in rising order whichever loop serves them
	auto take_group = [&](size_t p0, const Real *xu, const Real *xv, int count) {
		for (int e = 0; e < V; e++)
			if (e < count) {
				a.take(e, (double)xu[e]);
				b.take(e, (double)xv[e]);
				if constexpr (MAPS) map_update(mmin, mmax, tact, p0 + e, (double)xu[e], threshold, t);
				if constexpr (CYCLES) cycle_update(cprev, cfirst, clast, ccount, p0 + e, (double)xu[e], cy, t);
			}
	};
	size_t c = (size_t)blockIdx.x * kObserveThreads + threadIdx.x;
	if (wide) {
		const size_t full = n / V;  // groups that lie wholly inside the plane
		constexpr int kAhead = 8 / V;  // 16-byte loads in flight per lane and field: 4 in fp64, 2 in fp32
		for (; c + (kAhead - 1) * stride < full; c += kAhead * stride) {
			Vec wu[kAhead], wv[kAhead];
			for (int i = 0; i < kAhead; i++) {
				wu[i] = *reinterpret_cast<const Vec *>(u + (c + i * stride) * V);
				wv[i] = *reinterpret_cast<const Vec *>(v + (c + i * stride) * V);
			}
			for (int i = 0; i < kAhead; i++) take_group((c + i * stride) * V, reinterpret_cast<const Real *>(&wu[i]), reinterpret_cast<const Real *>(&wv[i]), V);
		}
		for (; c < full; c += stride) {
			const Vec wu = *reinterpret_cast<const Vec *>(u + c * V), wv = *reinterpret_cast<const Vec *>(v + c * V);
			take_group(c * V, reinterpret_cast<const Real *>(&wu), reinterpret_cast<const Real *>(&wv), V);
		}
	}
	for (; c < groups; c += stride) {  // planes that do not sit on 16 bytes, and the last, short group of any plane
		const size_t p0 = c * V;
		const int count = p0 + V <= n ? V : (int)(n - p0);
		Real xu[V] = {}, xv[V] = {};
		for (int e = 0; e < V; e++)
			if (e < count) {
				xu[e] = u[p0 + e];
				xv[e] = v[p0 + e];
			}
		take_group(p0, xu, xv, count);
	}
	a.fold();
	b.fold();
	double r[8] = {a.mn, a.mx, a.s[0], a.q[0], b.mn, b.mx, b.s[0], b.q[0]};
	for (int off = 32; off > 0; off >>= 1)
		for (int k = 0; k < 8; k++) {
			const double o = __shfl_down(r[k], off, 64);
			r[k] = (k & 3) == 0 ? nan_min(r[k], o) : (k & 3) == 1 ? nan_max(r[k], o) : r[k] + o;
		}
	if ((threadIdx.x & 63) == 0)
		for (int k = 0; k < 8; k++) part[threadIdx.x >> 6][k] = r[k];
	__syncthreads();
	if (threadIdx.x < 8) {
		const int k = threadIdx.x;
		const double w0 = part[0][k], w1 = part[1][k], w2 = part[2][k], w3 = part[3][k];  // pairwise: (0 + 1) + (2 + 3)
		const double out = (k & 3) == 0 ? nan_min(nan_min(w0, w1), nan_min(w2, w3)) : (k & 3) == 1 ? nan_max(nan_max(w0, w1), nan_max(w2, w3)) : (w0 + w1) + (w2 + w3);
		partials[((size_t)member * slots + blockIdx.x) * 8 + k] = out;
	}
}

template <typename Real, bool MAPS>
__global__ void __launch_bounds__(kObserveThreads) crd_observe_sample_kernel(const EnsembleMember *members, int src, size_t n, double *__restrict__ partials,
                                                                             double *__restrict__ maps, size_t map_plane, double threshold, double t)
{
	observe_sample_body<Real, MAPS, false>(members, src, n, partials, maps, map_plane, threshold, t, ObserveCycles{}, gridDim.x, gridDim.x);
}

// ... with the cycle maps folded in the same pass.
template <typename Real, bool MAPS>
__global__ void __launch_bounds__(kObserveThreads) crd_observe_sample_cycles_kernel(const EnsembleMember *members, int src, size_t n, double *__restrict__ partials,
                                                                                    double *__restrict__ maps, size_t map_plane, double threshold, double t, ObserveCycles cy)
{
	observe_sample_body<Real, MAPS, true>(members, src, n, partials, maps, map_plane, threshold, t, cy, gridDim.x, gridDim.x);
}

// One workgroup per member.  row: the sample's rows, member k's at row + k * row_doubles: the eight statistics, then (u, v) of each probe.
// (blocks: the member's partial records; slots: records between two members)
template <typename Real>
__device__ __forceinline__ void observe_finish_body(const EnsembleMember *members, int src, const double *__restrict__ partials, int blocks, int slots, const ObserveProbes &pr,
                                                    int nx, double *__restrict__ row, int row_doubles)
{
	const int member = blockIdx.x, k = threadIdx.x;
	double *const out = row + (size_t)member * row_doubles;
	if (k < 8) {
		const double *const p = partials + (size_t)member * slots * 8 + k;
		auto fold = [&](double r, double o) { return (k & 3) == 0 ? nan_min(r, o) : (k & 3) == 1 ? nan_max(r, o) : r + o; };
		double r = p[0];
		int g = 1;
		for (; g + 8 <= blocks; g += 8) {  // index order; eight loads in flight, then their additions
			double o[8];
			for (int i = 0; i < 8; i++) o[i] = p[(size_t)(g + i) * 8];
			for (int i = 0; i < 8; i++) r = fold(r, o[i]);
		}
		for (; g < blocks; g++) r = fold(r, p[(size_t)g * 8]);
		out[k] = r;
	} else if (k < 8 + 2 * pr.n) {
		ConstMember *const mem = (ConstMember *)members + member;
		const int q = (k - 8) >> 1;
		const Real *const plane = static_cast<const Real *>((k & 1) ? mem->v[src] : mem->u[src]);
		out[k] = (double)plane[(size_t)pr.j[q] * nx + pr.i[q]];
	}
}

template <typename Real>
__global__ void __launch_bounds__(64) crd_observe_finish_kernel(const EnsembleMember *members, int src, const double *__restrict__ partials, int blocks, ObserveProbes pr,
                                                                int nx, double *__restrict__ row, int row_doubles)
{
	observe_finish_body<Real>(members, src, partials, blocks, blocks, pr, nx, row, row_doubles);
}

// ---- members of different shape: n_k = nx_k * ny_k from the shape table, G_k = observe_blocks(n_k) -- the member's partition, and with
// it every bit of its row, is what it is in any ensemble.  Further instantiations: the kernels above keep their code and registers. ----

__device__ __forceinline__ unsigned observe_blocks_of(size_t n)  // observe_blocks
{
	const size_t g = (n + kObservePointsPerBlock - 1) / kObservePointsPerBlock;
	return (unsigned)(g < 1 ? 1 : g > (size_t)kObserveMaxBlocks ? (size_t)kObserveMaxBlocks : g);
}

// grid (max_k G_k, members): blocks beyond the member's G_k return; member k's partials at partials + k * gridDim.x * 8
template <typename Real, bool MAPS>
__global__ void __launch_bounds__(kObserveThreads) crd_observe_sample_mixed_kernel(const EnsembleMember *members, const EnsembleShape *shapes, int src,
                                                                                   double *__restrict__ partials, double *__restrict__ maps, size_t map_plane, double threshold,
                                                                                   double t)
{
	ConstShape *const sh = (ConstShape *)shapes + blockIdx.y;
	const size_t n = (size_t)sh->nx * (size_t)sh->ny;
	const unsigned G = observe_blocks_of(n);
	if (blockIdx.x >= G) return;
	observe_sample_body<Real, MAPS, false>(members, src, n, partials, maps, map_plane, threshold, t, ObserveCycles{}, G, gridDim.x);
}

template <typename Real>
__global__ void __launch_bounds__(64) crd_observe_finish_mixed_kernel(const EnsembleMember *members, const EnsembleShape *shapes, int src, const double *__restrict__ partials,
                                                                      int slots, ObserveProbes pr, double *__restrict__ row, int row_doubles)
{
	ConstShape *const sh = (ConstShape *)shapes + blockIdx.x;
	const int nx = sh->nx;
	observe_finish_body<Real>(members, src, partials, (int)observe_blocks_of((size_t)nx * (size_t)sh->ny), slots, pr, nx, row, row_doubles);
}

__global__ void __launch_bounds__(256) crd_observe_fill_kernel(double *__restrict__ x, size_t n, double value)
{
	for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) x[q] = value;
}

// ---- sections ----

constexpr int kSectionThreads = 256;
constexpr int kSectionWaves = kSectionThreads / 64;

// The sums of one row of both fields, one wavefront: group c of V consecutive columns belongs to lane c mod 64, which takes its groups
// in rising order; element e of every group goes to the lane's accumulator e; the V accumulators are folded pairwise, the 64 lanes by a
// __shfl_down tree.  The 16-byte loads (where this row of both planes sits on 16 bytes: decided per row, the result does not depend on
// it) serve the same columns to the same lanes as the element-wise ones.  A column passes through at most
// ceil(ceil(nx / V) / 64) + log2 V + 6 additions.  Lane 0 holds the sums.
template <typename Real>
__device__ __forceinline__ void row_sums(const Real *__restrict__ u, const Real *__restrict__ v, int nx, int lane, double &sum_u, double &sum_v)
{
	constexpr int V = Wide<Real>::n;
	using Vec = typename Wide<Real>::type;
	double su[V], sv[V];
	for (int e = 0; e < V; e++) su[e] = sv[e] = 0.0;
	auto take_group = [&](const Real *xu, const Real *xv, int count) {
		for (int e = 0; e < V; e++)
			if (e < count) {
				su[e] += (double)xu[e];
				sv[e] += (double)xv[e];
			}
	};
	const bool wide = (((uintptr_t)u | (uintptr_t)v) & 15) == 0;
	const int groups = (nx + V - 1) / V;
	int c = lane;
	if (wide) {
		const int full = nx / V;
		constexpr int kAhead = 4;  // 16-byte loads in flight per lane and field
		for (; c + (kAhead - 1) * 64 < full; c += kAhead * 64) {
			Vec wu[kAhead], wv[kAhead];
			for (int i = 0; i < kAhead; i++) {
				wu[i] = *reinterpret_cast<const Vec *>(u + (size_t)(c + i * 64) * V);
				wv[i] = *reinterpret_cast<const Vec *>(v + (size_t)(c + i * 64) * V);
			}
			for (int i = 0; i < kAhead; i++) take_group(reinterpret_cast<const Real *>(&wu[i]), reinterpret_cast<const Real *>(&wv[i]), V);
		}
		for (; c < full; c += 64) {
			const Vec wu = *reinterpret_cast<const Vec *>(u + (size_t)c * V), wv = *reinterpret_cast<const Vec *>(v + (size_t)c * V);
			take_group(reinterpret_cast<const Real *>(&wu), reinterpret_cast<const Real *>(&wv), V);
		}
	}
	for (; c < groups; c += 64) {  // rows that do not sit on 16 bytes, and the last, short group of any row
		const int p0 = c * V, count = p0 + V <= nx ? V : nx - p0;
		Real xu[V] = {}, xv[V] = {};
		for (int e = 0; e < V; e++)
			if (e < count) {
				xu[e] = u[p0 + e];
				xv[e] = v[p0 + e];
			}
		take_group(xu, xv, count);
	}
	for (int w = 1; w < V; w *= 2)  // pairwise: (0 + 1) + (2 + 3)
		for (int e = 0; e + w < V; e += 2 * w) {
			su[e] += su[e + w];
			sv[e] += sv[e + w];
		}
	for (int off = 32; off > 0; off >>= 1) {
		su[0] += __shfl_down(su[0], off, 64);
		sv[0] += __shfl_down(sv[0], off, 64);
	}
	sum_u = su[0];
	sum_v = sv[0];
}

// grid (blocks of every section in turn, members), kSectionThreads lanes.  A block finds its section from the prefix of block counts
// (static indices: the argument stays in the kernel-argument segment) and writes into member k's line of it, sc.out[s] + 2 k length:
// (var0, var1) of each of the line's points.
//   ROW, COLUMN   a point per lane: the state's value widened to double
//   THETA_MEAN    a wavefront per row (row_sums), one division by nx
//   PHI_MEAN      a block per 64 columns (a row read is one coalesced access); wavefront w takes rows w, w + 4, ... in rising order,
//                 eight loads in flight per field; the four wavefronts are combined through LDS as (0 + 1) + (2 + 3); one division
//                 by ny.  A row passes through at most ceil(ny / 4) + 2 additions.
template <typename Real>
__global__ void __launch_bounds__(kSectionThreads) crd_observe_sections_kernel(const EnsembleMember *members, int src, int nx, int ny, ObserveSections sc)
{
	__shared__ double part[kSectionWaves][64][2];
	const int member = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	ConstMember *const mem = (ConstMember *)members + member;
	const Real *__restrict__ const u = static_cast<const Real *>(mem->u[src]);
	const Real *__restrict__ const v = static_cast<const Real *>(mem->v[src]);
	int kind = sc.kind[0], index = sc.index[0], first = 0, length = sc.length[0];
	double *line = sc.out[0];
#pragma unroll
	for (int q = 1; q < kObserveMaxSections; q++)
		if (q < sc.n && (int)blockIdx.x >= sc.first_block[q]) {
			kind = sc.kind[q];
			index = sc.index[q];
			first = sc.first_block[q];
			length = sc.length[q];
			line = sc.out[q];
		}
	const int b = (int)blockIdx.x - first;
	double2 *__restrict__ const out = reinterpret_cast<double2 *>(line) + (size_t)member * (size_t)length;
	if (kind == CRD_SECTION_ROW || kind == CRD_SECTION_COLUMN) {
		const int p = b * kSectionThreads + (int)threadIdx.x;
		if (p < length) {
			const size_t at = kind == CRD_SECTION_ROW ? (size_t)index * (size_t)nx + (size_t)p : (size_t)p * (size_t)nx + (size_t)index;
			out[p] = make_double2((double)u[at], (double)v[at]);
		}
	} else if (kind == CRD_SECTION_THETA_MEAN) {
		const int j = b * kSectionWaves + wave;
		if (j < ny) {
			double su, sv;
			row_sums<Real>(u + (size_t)j * (size_t)nx, v + (size_t)j * (size_t)nx, nx, lane, su, sv);
			if (lane == 0) out[j] = make_double2(su / (double)nx, sv / (double)nx);
		}
	} else {  // CRD_SECTION_PHI_MEAN
		const int col = b * 64 + lane;
		double su = 0.0, sv = 0.0;
		if (col < nx) {
			constexpr int kAhead = 8;
			const Real *const cu = u + col, *const cv = v + col;
			int j = wave;
			for (; j + (kAhead - 1) * kSectionWaves < ny; j += kAhead * kSectionWaves) {
				Real xu[kAhead], xv[kAhead];
				for (int i = 0; i < kAhead; i++) {
					xu[i] = cu[(size_t)(j + i * kSectionWaves) * (size_t)nx];
					xv[i] = cv[(size_t)(j + i * kSectionWaves) * (size_t)nx];
				}
				for (int i = 0; i < kAhead; i++) {
					su += (double)xu[i];
					sv += (double)xv[i];
				}
			}
			for (; j < ny; j += kSectionWaves) {
				su += (double)cu[(size_t)j * (size_t)nx];
				sv += (double)cv[(size_t)j * (size_t)nx];
			}
		}
		part[wave][lane][0] = su;
		part[wave][lane][1] = sv;
		__syncthreads();
		if (wave == 0 && col < nx)
			out[col] = make_double2(((part[0][lane][0] + part[1][lane][0]) + (part[2][lane][0] + part[3][lane][0])) / (double)ny,
			                        ((part[0][lane][1] + part[1][lane][1]) + (part[2][lane][1] + part[3][lane][1])) / (double)ny);
	}
}

}  // namespace

int observe_blocks(size_t n)
{
	const size_t g = (n + kObservePointsPerBlock - 1) / kObservePointsPerBlock;
	return (int)(g < 1 ? 1 : g > (size_t)kObserveMaxBlocks ? (size_t)kObserveMaxBlocks : g);
}

hipError_t launch_observe_sample(int precision, const EnsembleMember *table, int members, int src, size_t n, double *partials_dev, double *maps_dev, size_t map_plane,
                                 double threshold, double t, hipStream_t s)
{
	clear_launch_status();
	if (members < 1 || n == 0) return hipErrorInvalidValue;
	const dim3 grid((unsigned)observe_blocks(n), (unsigned)members);
	if (precision == CRD_PRECISION_F64) {
		if (maps_dev) crd_observe_sample_kernel<double, true><<<grid, kObserveThreads, 0, s>>>(table, src, n, partials_dev, maps_dev, map_plane, threshold, t);
		else crd_observe_sample_kernel<double, false><<<grid, kObserveThreads, 0, s>>>(table, src, n, partials_dev, nullptr, 0, threshold, t);
	} else {
		if (maps_dev) crd_observe_sample_kernel<float, true><<<grid, kObserveThreads, 0, s>>>(table, src, n, partials_dev, maps_dev, map_plane, threshold, t);
		else crd_observe_sample_kernel<float, false><<<grid, kObserveThreads, 0, s>>>(table, src, n, partials_dev, nullptr, 0, threshold, t);
	}
	return launch_status();
}

hipError_t launch_observe_sample_cycles(int precision, const EnsembleMember *table, int members, int src, size_t n, double *partials_dev, double *maps_dev, size_t map_plane,
                                        double threshold, double t, const ObserveCycles &cy, hipStream_t s)
{
	clear_launch_status();
	if (members < 1 || n == 0 || !cy.planes || cy.plane < n) return hipErrorInvalidValue;
	const dim3 grid((unsigned)observe_blocks(n), (unsigned)members);
	if (precision == CRD_PRECISION_F64) {
		if (maps_dev) crd_observe_sample_cycles_kernel<double, true><<<grid, kObserveThreads, 0, s>>>(table, src, n, partials_dev, maps_dev, map_plane, threshold, t, cy);
		else crd_observe_sample_cycles_kernel<double, false><<<grid, kObserveThreads, 0, s>>>(table, src, n, partials_dev, nullptr, 0, threshold, t, cy);
	} else {
		if (maps_dev) crd_observe_sample_cycles_kernel<float, true><<<grid, kObserveThreads, 0, s>>>(table, src, n, partials_dev, maps_dev, map_plane, threshold, t, cy);
		else crd_observe_sample_cycles_kernel<float, false><<<grid, kObserveThreads, 0, s>>>(table, src, n, partials_dev, nullptr, 0, threshold, t, cy);
	}
	return launch_status();
}

bool observe_section_shape(int precision, int kind, int nx, int ny, int *length, int *blocks, int64_t *additions)
{
	const int V = precision == CRD_PRECISION_F64 ? Wide<double>::n : Wide<float>::n, log2V = V == 2 ? 1 : 2;
	int len = 0, nb = 0;
	int64_t d = 0;
	switch (kind) {
	case CRD_SECTION_ROW:
		len = nx;
		nb = (nx + kSectionThreads - 1) / kSectionThreads;
		break;
	case CRD_SECTION_COLUMN:
		len = ny;
		nb = (ny + kSectionThreads - 1) / kSectionThreads;
		break;
	case CRD_SECTION_THETA_MEAN:  // row_sums: the lane's accumulator, the fold, the shuffle tree; + 3: crd.h
		len = ny;
		nb = (ny + kSectionWaves - 1) / kSectionWaves;
		d = ((nx + V - 1) / V + 63) / 64 + log2V + 6 + 3;
		break;
	case CRD_SECTION_PHI_MEAN:  // the wavefront's accumulator, the pairwise combination of four; + 3
		len = nx;
		nb = (nx + 63) / 64;
		d = (ny + kSectionWaves - 1) / kSectionWaves + 2 + 3;
		break;
	default:
		return false;
	}
	if (length) *length = len;
	if (blocks) *blocks = nb;
	if (additions) *additions = d;
	return true;
}

hipError_t launch_observe_sections(int precision, const EnsembleMember *table, int members, int src, int nx, int ny, const ObserveSections &sc, hipStream_t s)
{
	clear_launch_status();
	if (members < 1 || sc.n < 1 || sc.n > kObserveMaxSections || sc.first_block[sc.n] < 1) return hipErrorInvalidValue;
	const dim3 grid((unsigned)sc.first_block[sc.n], (unsigned)members);
	if (precision == CRD_PRECISION_F64) crd_observe_sections_kernel<double><<<grid, kSectionThreads, 0, s>>>(table, src, nx, ny, sc);
	else crd_observe_sections_kernel<float><<<grid, kSectionThreads, 0, s>>>(table, src, nx, ny, sc);
	return launch_status();
}

hipError_t launch_observe_finish(int precision, const EnsembleMember *table, int members, int src, size_t n, const double *partials_dev, const ObserveProbes &probes, int nx,
                                 double *row_dev, int row_doubles, hipStream_t s)
{
	clear_launch_status();
	if (members < 1 || probes.n < 0 || probes.n > kObserveMaxProbes || row_doubles < 8 + 2 * probes.n) return hipErrorInvalidValue;
	const int blocks = observe_blocks(n);
	if (precision == CRD_PRECISION_F64) crd_observe_finish_kernel<double><<<members, 64, 0, s>>>(table, src, partials_dev, blocks, probes, nx, row_dev, row_doubles);
	else crd_observe_finish_kernel<float><<<members, 64, 0, s>>>(table, src, partials_dev, blocks, probes, nx, row_dev, row_doubles);
	return launch_status();
}

hipError_t launch_observe_sample_mixed(int precision, const EnsembleMember *table, const EnsembleShape *shapes, int members, int src, int max_blocks, double *partials_dev,
                                       double *maps_dev, size_t map_plane, double threshold, double t, hipStream_t s)
{
	clear_launch_status();
	if (members < 1 || !shapes || max_blocks < 1 || max_blocks > kObserveMaxBlocks) return hipErrorInvalidValue;
	const dim3 grid((unsigned)max_blocks, (unsigned)members);
	if (precision == CRD_PRECISION_F64) {
		if (maps_dev) crd_observe_sample_mixed_kernel<double, true><<<grid, kObserveThreads, 0, s>>>(table, shapes, src, partials_dev, maps_dev, map_plane, threshold, t);
		else crd_observe_sample_mixed_kernel<double, false><<<grid, kObserveThreads, 0, s>>>(table, shapes, src, partials_dev, nullptr, 0, threshold, t);
	} else {
		if (maps_dev) crd_observe_sample_mixed_kernel<float, true><<<grid, kObserveThreads, 0, s>>>(table, shapes, src, partials_dev, maps_dev, map_plane, threshold, t);
		else crd_observe_sample_mixed_kernel<float, false><<<grid, kObserveThreads, 0, s>>>(table, shapes, src, partials_dev, nullptr, 0, threshold, t);
	}
	return launch_status();
}

hipError_t launch_observe_finish_mixed(int precision, const EnsembleMember *table, const EnsembleShape *shapes, int members, int src, int max_blocks,
                                       const double *partials_dev, const ObserveProbes &probes, double *row_dev, int row_doubles, hipStream_t s)
{
	clear_launch_status();
	if (members < 1 || !shapes || max_blocks < 1 || probes.n < 0 || probes.n > kObserveMaxProbes || row_doubles < 8 + 2 * probes.n) return hipErrorInvalidValue;
	if (precision == CRD_PRECISION_F64) crd_observe_finish_mixed_kernel<double><<<members, 64, 0, s>>>(table, shapes, src, partials_dev, max_blocks, probes, row_dev, row_doubles);
	else crd_observe_finish_mixed_kernel<float><<<members, 64, 0, s>>>(table, shapes, src, partials_dev, max_blocks, probes, row_dev, row_doubles);
	return launch_status();
}

hipError_t launch_observe_fill(double *x, size_t n, double value, hipStream_t s)
{
	clear_launch_status();
	if (n == 0) return hipSuccess;
	const size_t g = (n + 255) / 256;
	crd_observe_fill_kernel<<<(int)(g < 2048 ? g : 2048), 256, 0, s>>>(x, n, value);
	return launch_status();
}

}  // namespace crd
