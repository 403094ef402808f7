// crd_run_output.h -- what the driver (crd_run.cpp) writes besides the state files (those are crd_writer's and crd_npy_writer's): the
// files --observe leaves, in one statement of their names and formats, the .npy writer under them, and the copy between the slabs'
// frames and the file blocks' that --decomp needs.
#ifndef CRD_RUN_OUTPUT_H
#define CRD_RUN_OUTPUT_H

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "crd.h"
#include "crd_run_options.h"

// An array of the given element type (descr: '<f8', '<i4') and shape (two dimensions or more), row-major, as a NumPy .npy file (format 1.0).
inline bool write_npy(const std::string &path, const char *descr, const std::vector<int64_t> &shape, const void *data, size_t bytes)
{
	std::string dims;
	for (int64_t d : shape) dims += (dims.empty() ? "" : ", ") + std::to_string(d);
	std::string head = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (" + dims + "), }";
	while ((10 + head.size() + 1) % 64) head += ' ';
	head += '\n';
	FILE *f = std::fopen(path.c_str(), "wb");
	if (!f) return false;
	const unsigned char magic[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(head.size() & 0xff), (unsigned char)(head.size() >> 8)};
	bool ok = std::fwrite(magic, 1, 10, f) == 10 && std::fwrite(head.data(), 1, head.size(), f) == head.size() && std::fwrite(data, 1, bytes, f) == bytes;
	return std::fclose(f) == 0 && ok;
}

// The samples of one directory's observables.txt: n times, and per sample 8 statistics and the probes' 2 values each.  Read from an
// ensemble's observer they lie [sample][member]: sample s of this member is row s * members + member.
struct Samples {
	int64_t n;
	const double *t, *stats, *probes;
	int member, members;
};
// ... and where the rest comes from, asked for only when the options want it: section q's lines of this directory, [sample][length][2],
// the cycle planes and the map planes (crd_ensemble_observe_* of a member, or crd_recorder_*), each returning the library's status.
struct ObservationSource {
	std::function<int(int q, int64_t *length, std::vector<double> *lines)> section;
	std::function<int(int32_t *count, double *t_first, double *t_last)> cycles;
	std::function<int(double *min_u, double *max_u, double *t_act)> maps;
};

// observables.txt: one line per sample in the state files' number format, under comment lines that numpy.loadtxt skips.
inline int write_observables_txt(const Options &o, const std::string &path, const Samples &s)
{
	FILE *f = std::fopen(path.c_str(), "w");
	if (!f) return CRD_EIO;
	const size_t P = o.probes.size();
	std::fprintf(f, "# t min0 max0 sum0 sumsq0 min1 max1 sum1 sumsq1");
	for (const auto &q : o.probes) std::fprintf(f, " var0(%lld,%lld) var1(%lld,%lld)", q.first, q.second, q.first, q.second);
	std::fprintf(f, "\n");
	for (size_t q = 0; q < o.sections.size(); q++) {
		std::fprintf(f, "# section_%zu.npy: %s", q, section_name(o.sections[q].first));
		if (o.sections[q].first == CRD_SECTION_ROW || o.sections[q].first == CRD_SECTION_COLUMN) std::fprintf(f, " %lld", o.sections[q].second);
		std::fprintf(f, ", [sample, length, 2]; sample s at the time t of line s below\n");
	}
	if (!o.sections.empty()) {
		std::fprintf(f, "# sample times:");
		for (size_t i = 0; i < (size_t)s.n; i++) std::fprintf(f, " %.16e", s.t[i]);
		std::fprintf(f, "\n");
	}
	for (size_t i = 0; i < (size_t)s.n; i++) {
		const size_t row = i * (size_t)s.members + (size_t)s.member;
		std::fprintf(f, "%.16e", s.t[i]);
		for (size_t c = 0; c < 8; c++) std::fprintf(f, " %.16e", s.stats[row * 8 + c]);
		for (size_t c = 0; c < 2 * P; c++) std::fprintf(f, " %.16e", s.probes[row * 2 * P + c]);
		std::fprintf(f, "\n");
	}
	return std::fclose(f) == 0 ? CRD_OK : CRD_EIO;
}

// What --observe leaves in a directory -- <outdir>/member_<k> of an ensemble, <outdir> itself of a run without one: observables.txt;
// per --section, section_<n>.npy; with --observe-cycles activation_count.npy (upward crossings) and period_map.npy (mean time between
// them, NaN below two); with --observe-maps amplitude_map.npy (running maximum - running minimum of var0) and activation_time.npy.
// The planes are the grid's, [ny][nx].
inline int write_observations(const Options &o, const std::string &dir, const crd_grid &g, const Samples &s, const ObservationSource &from)
{
	int rc = write_observables_txt(o, dir + "/observables.txt", s);
	if (rc != CRD_OK) return rc;
	for (size_t q = 0; q < o.sections.size(); q++) {
		int64_t length = 0;
		std::vector<double> lines;
		if ((rc = from.section((int)q, &length, &lines)) != CRD_OK) return rc;
		if (!write_npy(dir + "/section_" + std::to_string(q) + ".npy", "<f8", {s.n, length, 2}, lines.data(), lines.size() * sizeof(double))) return CRD_EIO;
	}
	const size_t points = (size_t)(g.nx * g.ny);
	const std::vector<int64_t> plane = {g.ny, g.nx};
	if (o.observe_cycles) {
		std::vector<int32_t> count(points);
		std::vector<double> tf(points), tl(points), period(points, std::nan(""));
		if ((rc = from.cycles(count.data(), tf.data(), tl.data())) != CRD_OK) return rc;
		for (size_t q = 0; q < points; q++)
			if (count[q] >= 2) period[q] = (tl[q] - tf[q]) / (double)(count[q] - 1);
		if (!write_npy(dir + "/activation_count.npy", "<i4", plane, count.data(), points * sizeof(int32_t)) ||
		    !write_npy(dir + "/period_map.npy", "<f8", plane, period.data(), points * sizeof(double)))
			return CRD_EIO;
	}
	if (o.observe_maps) {
		std::vector<double> lo(points), hi(points), ta(points);
		if ((rc = from.maps(lo.data(), hi.data(), ta.data())) != CRD_OK) return rc;
		for (size_t q = 0; q < points; q++) hi[q] -= lo[q];
		if (!write_npy(dir + "/amplitude_map.npy", "<f8", plane, hi.data(), points * sizeof(double)) ||
		    !write_npy(dir + "/activation_time.npy", "<f8", plane, ta.data(), points * sizeof(double)))
			return CRD_EIO;
	}
	return CRD_OK;
}

// A context's or a file block's part of the grid: columns is .. ie of rows js .. je.
struct Rect {
	int64_t is, ie, js, je;
};
// Copy between the slabs' AoS frames (full width nx, the rows of slab_rect) and the file blocks' (block_rect), either way.
inline void recut_frames(const std::vector<Rect> &slab_rect, const std::vector<Rect> &block_rect, int64_t nx, std::vector<std::vector<double>> &slabs,
                         std::vector<std::vector<double>> &blocks, bool to_blocks)
{
	for (size_t f = 0; f < block_rect.size(); f++) {
		const Rect &b = block_rect[f];
		const int64_t nxl = b.ie - b.is + 1;
		for (int64_t j = b.js; j <= b.je; j++) {
			size_t c = 0;
			while (c + 1 < slab_rect.size() && j > slab_rect[c].je) c++;
			double *slab_row = slabs[c].data() + 2 * ((j - slab_rect[c].js) * nx + b.is), *block_row = blocks[f].data() + 2 * (j - b.js) * nxl;
			if (to_blocks) std::memcpy(block_row, slab_row, (size_t)(2 * nxl) * sizeof(double));
			else std::memcpy(slab_row, block_row, (size_t)(2 * nxl) * sizeof(double));
		}
	}
}

#endif
