// crd_record.h -- the run recorder's kernels (crd_record.hip) as crd_recorder.cpp launches them.  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include "crd_ensemble.h"  // ObserveCycles, kObserveMaxProbes, kObserveMaxSections

namespace crd {

// A row's record: kRecordRowStats doubles (min, max, sum, sum of squares of var0, then of var1), the row's theta-mean of both fields, then
// (var0, var1) of the row's point on each `column:I` line.  Rows of the GLOBAL grid lie one record after the other.
constexpr int kRecordRowStats = 8;
constexpr int kRecordRowFixed = kRecordRowStats + 2;
constexpr int kRecordFinishThreads = 256;

// What one slab gathers at a sample besides its rows: the probes and `row:J` lines that fall into it (local row, or -1 for another
// slab's) and its part of every `column:I` line.
struct RecordGather {
	int n_probes, n_columns, n_rows;
	int probe_i[kObserveMaxProbes], probe_j[kObserveMaxProbes];  // probe_j: local row, -1: not in this slab
	int column_i[kObserveMaxSections];
	int row_j[kObserveMaxSections];                              // local row, -1: not in this slab
};

// What the finishing launch assembles: the sample's row of the record buffer and its section lines.
struct RecordFinish {
	int n_probes, n_sections;
	int probe_owner[kObserveMaxProbes];        // slab whose block of extras holds the probe
	int kind[kObserveMaxSections];             // CRD_SECTION_*
	int slot[kObserveMaxSections];             // ROW: which of the row lines; COLUMN: which of the columns
	int owner[kObserveMaxSections];            // ROW: slab whose block of extras holds the line
	double *out[kObserveMaxSections];          // this sample's line, (var0, var1) per point; PHI_MEAN: written by its own launch
};

// The rounding bound's D of the statistics (crd.h): additions a value passes through at most.
int64_t record_additions(int precision, int nx, int ny);

// One wavefront per owned row: u / v point at local row 0 of the two planes.  rows: the slab's first row record, `stride` doubles apart.
// maps (or null): three planes of `plane` doubles (running minimum, maximum, activation time), nyl x nx each; cy (or null): the four
// cycle planes.
hipError_t launch_record_rows(int precision, const void *u, const void *v, int nx, int nyl, double *rows, int stride, double *maps, size_t plane, double threshold, double t,
                              const ObserveCycles *cy, hipStream_t s);
// The slab's exact values: column parts into its row records, probes and row lines into its block of extras (2 n_probes doubles, then
// 2 nx per row line).
hipError_t launch_record_gather(int precision, const void *u, const void *v, int nx, int nyl, double *rows, int stride, double *extras, const RecordGather &g, hipStream_t s);
// One workgroup: the ny row records folded by global row, the probes and lines put in place.  extras: n_slabs blocks of extras_doubles.
hipError_t launch_record_finish(const double *rows, int stride, int nx, int ny, const double *extras, size_t extras_doubles, const RecordFinish &f, double *row_out, hipStream_t s);
// The phi-mean line of a lone context, as crd_observe_sections_kernel forms it.
hipError_t launch_record_phi_mean(int precision, const void *u, const void *v, int nx, int ny, double *out, hipStream_t s);

}  // namespace crd
