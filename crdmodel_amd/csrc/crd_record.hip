// crd_record.hip -- the run recorder's kernels: statistics, probes, sections, maps and cycle maps of a context or of the slabs of a LOCAL
// group, recorded on the device while the state steps (crd_recorder.cpp drives them).  Per sample and slab two launches, then one on the
// lead slab's device:
//   rows     one wavefront per owned row reads the row of both planes ONCE and writes the row's record: min, max, sum and sum of squares
//            of each field (in fp64 whatever the state's precision) and the row's theta-mean; with maps or cycles on, the same pass folds
//            var0 into the slab's map and cycle planes.  Columns go to lanes and accumulators exactly as in the theta-mean section of
//            crd_observe.hip (row_sums): group c of V consecutive columns to lane c mod 64, element e into accumulator e in rising order,
//            accumulators folded pairwise, lanes by a __shfl_down tree -- whether the row sits on 16 bytes or not.
//   gather   the slab's exact values: the probes and `row:J` lines that fall into it, its part of every `column:I` line.
//   finish   one workgroup of 256 lanes: lane l folds the records of GLOBAL rows l, l + 256, ... in rising order, then a fixed LDS tree
//            128 ... 1; the probes and lines are put in place behind the statistics.
// A row belongs to one slab and rows are combined by global index, so every recorded bit is the same for one slab and for any cut into
// slabs.  No floating-point atomics.  DESIGN.md 4 (run recorder).
#include "crd_device.h"
#include "crd_record.h"

namespace crd {

using dev::clear_launch_status;
using dev::launch_status;

namespace {

constexpr int kRowThreads = 256;
constexpr int kRowWaves = kRowThreads / 64;

template <typename Real> struct Wide;
template <> struct Wide<double> { using type = double2; static constexpr int n = 2; };
template <> struct Wide<float> { using type = float4; static constexpr int n = 4; };

// NaN propagates through both (crd_observe.hip): once an operand is NaN the result is, whichever side it is on.
__device__ __forceinline__ double nan_min(double m, double x) { return (x < m || x != x) ? x : m; }
__device__ __forceinline__ double nan_max(double m, double x) { return (x > m || x != x) ? x : m; }
__device__ __forceinline__ double fold_stat(int k, double r, double o) { return (k & 3) == 0 ? nan_min(r, o) : (k & 3) == 1 ? nan_max(r, o) : r + o; }

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

// The maps' and the cycle maps' rules (crd.h), as crd_observe.hip applies them: an entry is rewritten only when it changes.
__device__ __forceinline__ void map_update(double *__restrict__ mmin, double *__restrict__ mmax, double *__restrict__ tact, size_t p, double x, double threshold,
                                           double t)
{
	const double lo = mmin[p], hi = mmax[p], ta = tact[p];
	if (x < lo || x != x) mmin[p] = x;
	if (x > hi || x != x) mmax[p] = x;
	if (ta != ta && x >= threshold) tact[p] = t;
}

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

// grid ceil(nyl / 4), 256 lanes: wavefront w of block b takes local row 4 b + w.
template <typename Real, bool MAPS, bool CYCLES>
__global__ void __launch_bounds__(kRowThreads) crd_record_rows_kernel(const Real *__restrict__ u0, const Real *__restrict__ v0, int nx, int nyl, double *__restrict__ rows,
                                                                      int stride, double *__restrict__ maps, size_t plane, double threshold, double t, ObserveCycles cy)
{
	constexpr int V = Wide<Real>::n;
	using Vec = typename Wide<Real>::type;
	const int lane = threadIdx.x & 63, j = (int)blockIdx.x * kRowWaves + (int)(threadIdx.x >> 6);
	if (j >= nyl) return;
	const size_t base = (size_t)j * (size_t)nx;
	const Real *__restrict__ const u = u0 + base;
	const Real *__restrict__ const v = v0 + base;
	double *const mmin = MAPS ? maps : nullptr;
	double *const mmax = MAPS ? mmin + plane : nullptr;
	double *const tact = MAPS ? mmax + plane : nullptr;
	double *const cprev = CYCLES ? cy.planes : nullptr;
	double *const cfirst = CYCLES ? cprev + cy.plane : nullptr;
	double *const clast = CYCLES ? cfirst + cy.plane : nullptr;
	int *const ccount = CYCLES ? reinterpret_cast<int *>(clast + cy.plane) : nullptr;

	FieldStats<V> a, b;
	a.clear();
	b.clear();
	auto take_group = [&](int p0, const Real *xu, const Real *xv, int count) {
		for (int e = 0; e < V; e++)
			if (e < count) {
				a.take(e, (double)xu[e]);
				b.take(e, (double)xv[e]);
				if constexpr (MAPS) map_update(mmin, mmax, tact, base + (size_t)(p0 + e), (double)xu[e], threshold, t);
				if constexpr (CYCLES) cycle_update(cprev, cfirst, clast, ccount, base + (size_t)(p0 + e), (double)xu[e], cy, t);
			}
	};
	// 16 bytes per lane and load where this row of both planes allows it (decided per row; the result does not depend on it)
	const bool wide = (((uintptr_t)u | (uintptr_t)v) & 15) == 0;
	const int groups = (nx + V - 1) / V;
	int c = lane;
	if (wide) {
		const int full = nx / V;  // groups that lie wholly inside the row
		constexpr int kAhead = 4;  // 16-byte loads in flight per lane and field
		for (; c + (kAhead - 1) * 64 < full; c += kAhead * 64) {
			Vec wu[kAhead], wv[kAhead];
			for (int i = 0; i < kAhead; i++) {
				wu[i] = *reinterpret_cast<const Vec *>(u + (size_t)(c + i * 64) * V);
				wv[i] = *reinterpret_cast<const Vec *>(v + (size_t)(c + i * 64) * V);
			}
			for (int i = 0; i < kAhead; i++) take_group((c + i * 64) * V, reinterpret_cast<const Real *>(&wu[i]), reinterpret_cast<const Real *>(&wv[i]), V);
		}
		for (; c < full; c += 64) {
			const Vec wu = *reinterpret_cast<const Vec *>(u + (size_t)c * V), wv = *reinterpret_cast<const Vec *>(v + (size_t)c * V);
			take_group(c * V, reinterpret_cast<const Real *>(&wu), reinterpret_cast<const Real *>(&wv), V);
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
		take_group(p0, xu, xv, count);
	}
	a.fold();
	b.fold();
	double r[8] = {a.mn, a.mx, a.s[0], a.q[0], b.mn, b.mx, b.s[0], b.q[0]};
	for (int off = 32; off > 0; off >>= 1)
		for (int k = 0; k < 8; k++) r[k] = fold_stat(k, r[k], __shfl_down(r[k], off, 64));
	if (lane == 0) {
		double *const out = rows + (size_t)j * (size_t)stride;
		for (int k = 0; k < 8; k++) out[k] = r[k];
		out[8] = r[2] / (double)nx;  // the row's theta-mean: one division
		out[9] = r[6] / (double)nx;
	}
}

// One flat index space: the probes, then the slab's rows of every column line, then the points of every row line.
template <typename Real>
__global__ void __launch_bounds__(256) crd_record_gather_kernel(const Real *__restrict__ u0, const Real *__restrict__ v0, int nx, int nyl, double *__restrict__ rows, int stride,
                                                                double *__restrict__ extras, RecordGather g)
{
	const long total = (long)g.n_probes + (long)g.n_columns * nyl + (long)g.n_rows * nx;
	for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
		if (q < g.n_probes) {
			int i = 0, j = -1;
#pragma unroll
			for (int k = 0; k < kObserveMaxProbes; k++)
				if (k == (int)q) {
					i = g.probe_i[k];
					j = g.probe_j[k];
				}
			if (j >= 0 && j < nyl && i >= 0 && i < nx) {
				const size_t at = (size_t)j * (size_t)nx + (size_t)i;
				extras[2 * q] = (double)u0[at];
				extras[2 * q + 1] = (double)v0[at];
			}
			continue;
		}
		long w = q - g.n_probes;
		if (w < (long)g.n_columns * nyl) {
			const int s = (int)(w / nyl), j = (int)(w - (long)s * nyl);
			int i = 0;
#pragma unroll
			for (int k = 0; k < kObserveMaxSections; k++)
				if (k == s) i = g.column_i[k];
			if (i >= 0 && i < nx) {
				const size_t at = (size_t)j * (size_t)nx + (size_t)i;
				double *const out = rows + (size_t)j * (size_t)stride + kRecordRowFixed + 2 * s;
				out[0] = (double)u0[at];
				out[1] = (double)v0[at];
			}
			continue;
		}
		w -= (long)g.n_columns * nyl;
		const int s = (int)(w / nx), i = (int)(w - (long)s * nx);
		int j = -1;
#pragma unroll
		for (int k = 0; k < kObserveMaxSections; k++)
			if (k == s) j = g.row_j[k];
		if (j >= 0 && j < nyl) {
			const size_t at = (size_t)j * (size_t)nx + (size_t)i;
			double *const out = extras + 2 * (size_t)g.n_probes + ((size_t)s * (size_t)nx + (size_t)i) * 2;
			out[0] = (double)u0[at];
			out[1] = (double)v0[at];
		}
	}
}

// One workgroup of 256 lanes on the lead slab's device.
__global__ void __launch_bounds__(kRecordFinishThreads) crd_record_finish_kernel(const double *__restrict__ rows, int stride, int nx, int ny, const double *__restrict__ extras,
                                                                                 size_t extras_doubles, RecordFinish f, double *__restrict__ row_out)
{
	__shared__ double part[kRecordFinishThreads][8];
	const int l = threadIdx.x;
	double r[8] = {INFINITY, -INFINITY, 0.0, 0.0, INFINITY, -INFINITY, 0.0, 0.0};
	if (l < ny) {
		for (int k = 0; k < 8; k++) r[k] = rows[(size_t)l * (size_t)stride + k];
		for (int j = l + kRecordFinishThreads; j < ny; j += kRecordFinishThreads) {  // global rows l, l + 256, ... in rising order
			double o[8];
			for (int k = 0; k < 8; k++) o[k] = rows[(size_t)j * (size_t)stride + k];
			for (int k = 0; k < 8; k++) r[k] = fold_stat(k, r[k], o[k]);
		}
	}
	for (int k = 0; k < 8; k++) part[l][k] = r[k];
	__syncthreads();
	for (int w = kRecordFinishThreads / 2; w > 0; w >>= 1) {  // the fixed tree 128 ... 1 (crd_sum_partials_kernel)
		if (l < w)
			for (int k = 0; k < 8; k++) part[l][k] = fold_stat(k, part[l][k], part[l + w][k]);
		__syncthreads();
	}
	if (l < 8) row_out[l] = part[0][l];
	if (l < f.n_probes) {
		int owner = 0;
#pragma unroll
		for (int k = 0; k < kObserveMaxProbes; k++)
			if (k == l) owner = f.probe_owner[k];
		const double *const src = extras + (size_t)owner * extras_doubles + 2 * (size_t)l;
		row_out[8 + 2 * l] = src[0];
		row_out[8 + 2 * l + 1] = src[1];
	}
#pragma unroll
	for (int s = 0; s < kObserveMaxSections; s++) {
		if (s >= f.n_sections) break;
		double *const out = f.out[s];
		const int kind = f.kind[s], slot = f.slot[s];
		if (kind == CRD_SECTION_ROW) {
			const double *const src = extras + (size_t)f.owner[s] * extras_doubles + 2 * (size_t)f.n_probes + (size_t)slot * (size_t)nx * 2;
			for (int p = l; p < 2 * nx; p += kRecordFinishThreads) out[p] = src[p];
		} else if (kind == CRD_SECTION_COLUMN || kind == CRD_SECTION_THETA_MEAN) {
			const int at = kind == CRD_SECTION_COLUMN ? kRecordRowFixed + 2 * slot : kRecordRowStats;
			for (int j = l; j < ny; j += kRecordFinishThreads) {
				out[2 * (size_t)j] = rows[(size_t)j * (size_t)stride + at];
				out[2 * (size_t)j + 1] = rows[(size_t)j * (size_t)stride + at + 1];
			}
		}
	}
}

// The phi-mean of crd_observe_sections_kernel: a block per 64 columns, wavefront w adds rows w, w + 4, ... in rising order, the four are
// combined (0 + 1) + (2 + 3), one division by ny.
template <typename Real>
__global__ void __launch_bounds__(256) crd_record_phi_mean_kernel(const Real *__restrict__ u, const Real *__restrict__ v, int nx, int ny, double2 *__restrict__ out)
{
	__shared__ double part[4][64][2];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = (int)blockIdx.x * 64 + lane;
	double su = 0.0, sv = 0.0;
	if (col < nx)
		for (int j = wave; j < ny; j += 4) {
			su += (double)u[(size_t)j * (size_t)nx + col];
			sv += (double)v[(size_t)j * (size_t)nx + col];
		}
	part[wave][lane][0] = su;
	part[wave][lane][1] = sv;
	__syncthreads();
	if (wave == 0 && col < nx)
		out[col] = make_double2(((part[0][lane][0] + part[1][lane][0]) + (part[2][lane][0] + part[3][lane][0])) / (double)ny,
		                        ((part[0][lane][1] + part[1][lane][1]) + (part[2][lane][1] + part[3][lane][1])) / (double)ny);
}

template <typename Real>
hipError_t rows_launch(const void *u, const void *v, int nx, int nyl, double *rows, int stride, double *maps, size_t plane, double threshold, double t, const ObserveCycles *cy,
                       hipStream_t s)
{
	const Real *const uu = static_cast<const Real *>(u), *const vv = static_cast<const Real *>(v);
	const int grid = (nyl + kRowWaves - 1) / kRowWaves;
	const ObserveCycles none{};
	if (maps && cy) crd_record_rows_kernel<Real, true, true><<<grid, kRowThreads, 0, s>>>(uu, vv, nx, nyl, rows, stride, maps, plane, threshold, t, *cy);
	else if (maps) crd_record_rows_kernel<Real, true, false><<<grid, kRowThreads, 0, s>>>(uu, vv, nx, nyl, rows, stride, maps, plane, threshold, t, none);
	else if (cy) crd_record_rows_kernel<Real, false, true><<<grid, kRowThreads, 0, s>>>(uu, vv, nx, nyl, rows, stride, nullptr, 0, threshold, t, *cy);
	else crd_record_rows_kernel<Real, false, false><<<grid, kRowThreads, 0, s>>>(uu, vv, nx, nyl, rows, stride, nullptr, 0, threshold, t, none);
	return launch_status();
}

}  // namespace

int64_t record_additions(int precision, int nx, int ny)
{
	const int V = precision == CRD_PRECISION_F64 ? Wide<double>::n : Wide<float>::n, log2V = V == 2 ? 1 : 2;
	return (int64_t)(((nx + V - 1) / V + 63) / 64) + log2V + 6 + (ny + kRecordFinishThreads - 1) / kRecordFinishThreads + 8;
}

hipError_t launch_record_rows(int precision, const void *u, const void *v, int nx, int nyl, double *rows, int stride, double *maps, size_t plane, double threshold, double t,
                              const ObserveCycles *cy, hipStream_t s)
{
	clear_launch_status();
	if (!u || !v || !rows || nx < 1 || nyl < 1 || stride < kRecordRowFixed) return hipErrorInvalidValue;
	if ((maps && plane < (size_t)nx * (size_t)nyl) || (cy && (!cy->planes || cy->plane < (size_t)nx * (size_t)nyl))) return hipErrorInvalidValue;
	if (precision == CRD_PRECISION_F64) return rows_launch<double>(u, v, nx, nyl, rows, stride, maps, plane, threshold, t, cy, s);
	return rows_launch<float>(u, v, nx, nyl, rows, stride, maps, plane, threshold, t, cy, s);
}

hipError_t launch_record_gather(int precision, const void *u, const void *v, int nx, int nyl, double *rows, int stride, double *extras, const RecordGather &g, hipStream_t s)
{
	clear_launch_status();
	if (!u || !v || !rows || nx < 1 || nyl < 1) return hipErrorInvalidValue;
	if (g.n_probes < 0 || g.n_probes > kObserveMaxProbes || g.n_columns < 0 || g.n_rows < 0 || g.n_columns + g.n_rows > kObserveMaxSections) return hipErrorInvalidValue;
	if (stride < kRecordRowFixed + 2 * g.n_columns || ((g.n_probes || g.n_rows) && !extras)) return hipErrorInvalidValue;
	const long total = (long)g.n_probes + (long)g.n_columns * nyl + (long)g.n_rows * nx;
	if (total == 0) return hipSuccess;
	const long blocks = (total + 255) / 256;
	const int grid = (int)(blocks < 256 ? blocks : 256);
	if (precision == CRD_PRECISION_F64) crd_record_gather_kernel<double><<<grid, 256, 0, s>>>(static_cast<const double *>(u), static_cast<const double *>(v), nx, nyl, rows, stride, extras, g);
	else crd_record_gather_kernel<float><<<grid, 256, 0, s>>>(static_cast<const float *>(u), static_cast<const float *>(v), nx, nyl, rows, stride, extras, g);
	return launch_status();
}

hipError_t launch_record_finish(const double *rows, int stride, int nx, int ny, const double *extras, size_t extras_doubles, const RecordFinish &f, double *row_out, hipStream_t s)
{
	clear_launch_status();
	if (!rows || !row_out || nx < 1 || ny < 1 || stride < kRecordRowFixed) return hipErrorInvalidValue;
	if (f.n_probes < 0 || f.n_probes > kObserveMaxProbes || f.n_sections < 0 || f.n_sections > kObserveMaxSections) return hipErrorInvalidValue;
	crd_record_finish_kernel<<<1, kRecordFinishThreads, 0, s>>>(rows, stride, nx, ny, extras, extras_doubles, f, row_out);
	return launch_status();
}

hipError_t launch_record_phi_mean(int precision, const void *u, const void *v, int nx, int ny, double *out, hipStream_t s)
{
	clear_launch_status();
	if (!u || !v || !out || nx < 1 || ny < 1) return hipErrorInvalidValue;
	const int grid = (nx + 63) / 64;
	if (precision == CRD_PRECISION_F64) crd_record_phi_mean_kernel<double><<<grid, 256, 0, s>>>(static_cast<const double *>(u), static_cast<const double *>(v), nx, ny, reinterpret_cast<double2 *>(out));
	else crd_record_phi_mean_kernel<float><<<grid, 256, 0, s>>>(static_cast<const float *>(u), static_cast<const float *>(v), nx, ny, reinterpret_cast<double2 *>(out));
	return launch_status();
}

}  // namespace crd
