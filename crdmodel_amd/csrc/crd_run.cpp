// crd_run.cpp -- command-line driver with the reference's surface: `<program> <ini file>` writes the per-subdomain
// text files the reference's Python plotting / torus-mapping utilities read.  It replaces main() of the four
// reference programs (src/FHNmodel_torus.cpp:148-497 and siblings); invoked through one of the alias names
// FHNmodel_torus / FHNmodel_flat / GoldbeterModel_torus / GoldbeterModel_flat it takes exactly one argument, like
// they do.  Time integration is fixed-step RK4 on the GPU (libcrd) by default; --adaptive runs the reference's integrator,
// ARKode's default explicit pair and controller restated (CRD_ADAPT_ARKODE), --adaptive-rk43 the RK4(3) pair of earlier rounds.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <filesystem>
#include <iostream>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "crd.h"

namespace {

struct Options {
	int model = -1, surface = -1;
	int gpus = 0;        // 0 = take [Solver] gpus from the ini (default 1)
	int devices = 0;     // number of physical devices to spread the slabs over (0 = as many as slabs)
	double dt = -1.0;
	int stepper = -1;
	int precision = -1;
	std::string outdir = ".";
	std::string ini;
	bool quiet = false;
	int adaptive = -1;
	bool binary = false;       // also write <Model>_<surface>_<var>.NNN.npy (crd_npy_writer)
	bool binary_only = false;  // ... and no text rows (the text files are created empty; only crdmodel_amd.post reads such a run)
	bool ref_steady_state = false;  // Goldbeter rest state as the reference reads it from its script's print (8 decimals)
	int d0 = 0, d1 = 0;  // --decomp d0xd1: the reference's 2-D block layout (theta x phi) instead of phi-slabs; "--decomp mpi" = MPI_Dims_create(gpus)
	bool block_contexts = false;  // --block-contexts: also COMPUTE on those blocks (staged kernels); default: files in that layout, computed on phi-slabs
	bool decomp_mpi = false;
	// --ensemble KEY=v1,v2,...: members that differ in one or more parameters, zipped over the lists (run_ensemble)
	std::vector<std::pair<std::string, std::vector<double>>> ensemble;
	int ensemble_steps = 0;  // --ensemble-steps 1|2: RK4 steps per launch of the ensemble (crd_ensemble_set_steps_per_launch); 0: not given
	bool ensemble_own_dt = false;  // --ensemble-own-dt: every member at its own dtSafety x stable dt (crd_ensemble_step_rk4_own)
	// --observe STRIDE [--probe i,j]... [--observe-maps THRESHOLD]: the ensemble's observer (crd_ensemble_observe_*)
	bool observe = false, observe_maps = false;
	long long observe_stride = 0;
	double observe_threshold = 0.0;
	std::vector<std::pair<long long, long long>> probes;
	// --section row:J|column:I|theta-mean|phi-mean (repeatable), --observe-cycles THRESHOLD: the observer's sections and cycle maps
	std::vector<std::pair<int, long long>> sections;  // (CRD_SECTION_*, index)
	bool observe_cycles = false;
	double cycle_threshold = 0.0;
};

[[noreturn]] void usage(const char *argv0, bool alias)
{
	if (alias) {
		std::cerr << "Usage: " << argv0 << " <Config file path>";  // src/FHNmodel_torus.cpp:153
	} else {
		std::cerr << "Usage: " << argv0
		          << " --model fhn|goldbeter --surface torus|flat [--gpus G] [--devices D] [--dt DT] [--stepper auto|staged|fused]\n"
		             "       [--precision 64|32] [--adaptive|--adaptive-rk43|--fixed] [--binary|--binary-only] [--ref-steady-state] [--decomp D0xD1|mpi [--block-contexts]]\n"
		             "       [--outdir DIR] [--quiet] [--ensemble beta|betaMin|betaMax|diffusion|tBoundary|surfaceLength|surfaceWidth|xMesh|surface=V1,V2,... (repeatable)]\n"
		             "       [--ensemble-steps 1|2] [--ensemble-own-dt]\n"
		             "       [--observe STRIDE [--probe I,J (repeatable)] [--observe-maps THRESHOLD]\n"
		             "                         [--section row:J|column:I|theta-mean|phi-mean (repeatable)] [--observe-cycles THRESHOLD]]\n"
		             "       <Config file path>\n"
		             "  --ensemble: fixed-step RK4, or error-controlled (each member its own ARKode-style steps) when the ini asks for [Solver] adaptive = 1\n"
		             "  --ensemble-steps: fixed steps one launch takes (2: pairs, the same bits as single steps; members of at least 9 rows; not with adaptive = 1)\n"
		             "  --ensemble-own-dt: every member steps at its own dtSafety x stable dt instead of the smallest member's (member files as a lone run of\n"
		             "             that member's ini writes them; one observer sample per output; not with adaptive = 1, a pinned [Solver] dt / --dt or --ensemble-steps 2)\n"
		             "  --observe without --ensemble (with at least one of --probe / --section / --observe-maps / --observe-cycles): the same files in the output\n"
		             "             directory itself, recorded while a lone run or its in-process phi-slabs step (not with --decomp / --block-contexts; phi-mean: one slab)\n"
		             "  --observe: with --ensemble, member_<k>/observables.txt -- time, min / max / sum / sum of squares of both fields and the probes' values\n"
		             "             after every STRIDE-th step (error-controlled: at every output), recorded on the GPU; --observe-maps: also\n"
		             "             amplitude_map.npy and activation_time.npy (first sample with var0 >= THRESHOLD); --section: also\n"
		             "             section_<n>.npy, [sample, length, 2]: both fields along a row or a column, or their mean over theta / over phi;\n"
		             "             --observe-cycles: also activation_count.npy (upward crossings of THRESHOLD by var0) and period_map.npy\n";
	}
	std::exit(EXIT_FAILURE);
}

bool preset_from_name(const std::string &base, Options *o)
{
	if (base == "FHNmodel_torus") { o->model = CRD_MODEL_FHN; o->surface = CRD_SURFACE_TORUS; return true; }
	if (base == "FHNmodel_flat") { o->model = CRD_MODEL_FHN; o->surface = CRD_SURFACE_FLAT; return true; }
	if (base == "GoldbeterModel_torus") { o->model = CRD_MODEL_GOLDBETER; o->surface = CRD_SURFACE_TORUS; return true; }
	if (base == "GoldbeterModel_flat") { o->model = CRD_MODEL_GOLDBETER; o->surface = CRD_SURFACE_FLAT; return true; }
	return false;
}

// Keys --ensemble takes: the parameters members of one ensemble may differ in (crd_ensemble_create), by their ini names.
double *ensemble_field(const std::string &key, crd_params *p)
{
	if (key == "beta") return &p->beta;
	if (key == "betaMin") return &p->beta_min;
	if (key == "betaMax") return &p->beta_max;
	if (key == "diffusion") return &p->diffusion;
	if (key == "tBoundary") return &p->t_boundary;
	if (key == "surfaceLength") return &p->surface_length;
	if (key == "surfaceWidth") return &p->surface_width;
	return nullptr;
}
// ... and the keys that make the members' geometry differ (crd_ensemble_create_mixed): the two lengths above, xMesh (nx) and surface
// (torus | flat, held as CRD_SURFACE_*).
bool ensemble_geometry_key(const std::string &key) { return key == "surfaceLength" || key == "surfaceWidth" || key == "xMesh" || key == "surface"; }
bool ensemble_key(const std::string &key)
{
	crd_params probe{};
	return ensemble_field(key, &probe) || key == "xMesh" || key == "surface";
}
void set_ensemble_value(const std::string &key, double value, crd_params *p)
{
	if (key == "xMesh") p->nx = (int64_t)value;
	else if (key == "surface") p->surface = (int)value;
	else *ensemble_field(key, p) = value;
}

[[noreturn]] void usage_error(const std::string &msg)
{
	std::cerr << "\nCRD_ERROR: " << msg << "\n\n";
	std::exit(EXIT_FAILURE);  // (the status of any bad option)
}

void parse_ensemble(const std::string &arg, Options *o)
{
	const size_t eq = arg.find('=');
	const std::string key = arg.substr(0, eq);
	if (eq == std::string::npos || !ensemble_key(key))
		usage_error("--ensemble takes KEY=V1,V2,... with KEY one of beta, betaMin, betaMax, diffusion, tBoundary, surfaceLength, surfaceWidth, xMesh, surface (got '" + arg + "')");
	std::vector<double> values;
	size_t at = eq + 1;
	while (true) {
		const size_t comma = arg.find(',', at);
		const std::string v = arg.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
		if (key == "surface") {
			if (v != "torus" && v != "flat") usage_error("--ensemble surface: '" + v + "' is neither torus nor flat");
			values.push_back(v == "torus" ? CRD_SURFACE_TORUS : CRD_SURFACE_FLAT);
		} else {
			char *end = nullptr;
			const double x = std::strtod(v.c_str(), &end);
			if (v.empty() || *end != '\0' || !std::isfinite(x)) usage_error("--ensemble " + key + ": '" + v + "' is not a number");
			if (key == "xMesh" && (x < 1 || x != std::floor(x) || x > 1e9)) usage_error("--ensemble xMesh: '" + v + "' is not a positive whole number");
			values.push_back(x);
		}
		if (comma == std::string::npos) break;
		at = comma + 1;
	}
	for (const auto &kv : o->ensemble)
		if (kv.first == key) usage_error("--ensemble " + key + " given twice");
	o->ensemble.emplace_back(key, values);
}

// What --ensemble cannot be combined with, and lists of unequal length: refused before the ini is read or any device touched.
void check_ensemble_options(const Options &o)
{
	if (o.ensemble.empty()) {
		if (o.ensemble_steps) usage_error("--ensemble-steps sets an ensemble's steps per launch: it needs --ensemble");
		if (o.ensemble_own_dt) usage_error("--ensemble-own-dt steps an ensemble's members at their own step sizes: it needs --ensemble");
		if (!o.observe) {
			if (!o.probes.empty()) usage_error("--probe belongs to --observe, which needs --ensemble");
			if (o.observe_maps) usage_error("--observe-maps belongs to --observe, which needs --ensemble");
			if (!o.sections.empty()) usage_error("--section belongs to --observe, which needs --ensemble");
			if (o.observe_cycles) usage_error("--observe-cycles belongs to --observe, which needs --ensemble");
			return;
		}
		// --observe without --ensemble: the run recorder (crd_recorder_*) of a lone run or of its in-process slabs.  A bare --observe
		// STRIDE, naming nothing to record, keeps the refusal it has always had here (tests/test_observe_host.py pins it).
		if (o.probes.empty() && !o.observe_maps && o.sections.empty() && !o.observe_cycles)
			usage_error("--observe records an ensemble's members: it needs --ensemble (a run without one names what to record besides the statistics: --probe, --section, --observe-maps or "
			            "--observe-cycles)");
		if (o.observe_stride < 1) usage_error("--observe takes a stride of at least 1 (got " + std::to_string(o.observe_stride) + ")");
		if ((int)o.sections.size() > CRD_OBSERVE_MAX_SECTIONS) usage_error("--section: at most " + std::to_string(CRD_OBSERVE_MAX_SECTIONS) + " sections");
		if ((int)o.probes.size() > CRD_OBSERVE_MAX_PROBES) usage_error("--probe: at most " + std::to_string(CRD_OBSERVE_MAX_PROBES) + " probes");
		if (o.d0 > 0 || o.decomp_mpi) usage_error("--observe records phi-slabs: not with --decomp (2-D block files and contexts are not recorded)");
		if (o.block_contexts) usage_error("--observe records phi-slabs: not with --block-contexts");
		return;
	}
	if (!o.observe && !o.sections.empty()) usage_error("--section belongs to --observe STRIDE");
	if (!o.observe && o.observe_cycles) usage_error("--observe-cycles belongs to --observe STRIDE");
	if ((int)o.sections.size() > CRD_OBSERVE_MAX_SECTIONS) usage_error("--section: at most " + std::to_string(CRD_OBSERVE_MAX_SECTIONS) + " sections");
	if (!o.observe && !o.probes.empty()) usage_error("--probe belongs to --observe STRIDE");
	if (!o.observe && o.observe_maps) usage_error("--observe-maps belongs to --observe STRIDE");
	if (o.observe && o.observe_stride < 1) usage_error("--observe takes a stride of at least 1 (got " + std::to_string(o.observe_stride) + ")");
	if ((int)o.probes.size() > CRD_OBSERVE_MAX_PROBES) usage_error("--probe: at most " + std::to_string(CRD_OBSERVE_MAX_PROBES) + " probes");
	if (o.adaptive == 1 || o.adaptive == 2) usage_error("--ensemble steps fixed-step RK4 only: not with --adaptive / --adaptive-rk43");
	if (o.ensemble_own_dt && o.ensemble_steps == 2) usage_error("--ensemble-own-dt takes single steps (pairs of own steps are not built): not with --ensemble-steps 2");
	if (o.ensemble_own_dt && o.dt > 0) usage_error("--ensemble-own-dt gives every member its own step size: not with --dt, which pins one for all");
	if (o.gpus > 1) usage_error("--ensemble runs on one GPU: not with --gpus " + std::to_string(o.gpus));
	if (o.d0 > 0 || o.decomp_mpi) usage_error("--ensemble members are single slabs: not with --decomp");
	if (o.block_contexts) usage_error("--ensemble members are single slabs: not with --block-contexts");
	if (o.binary) usage_error("--ensemble writes the text files only: not with --binary / --binary-only");
	const size_t n = o.ensemble[0].second.size();
	for (const auto &kv : o.ensemble)
		if (kv.second.size() != n) {
			std::string lens;
			for (const auto &x : o.ensemble) lens += (lens.empty() ? "" : ", ") + x.first + " has " + std::to_string(x.second.size());
			usage_error("--ensemble lists differ in length (" + lens + "): they are zipped into members");
		}
}

void banner(const crd_run_config &cfg, const crd_grid &g, int n_slabs, int64_t nxl0, int64_t nyl0, double s0, double s1, double dt, int64_t steps_per_output)
{
	// Same lines as src/FHNmodel_torus.cpp:249-275 (and the Goldbeter variant, src/GoldbeterModel_torus.cpp:266-303),
	// with rtol / atol replaced by the fixed step.
	const crd_params &p = cfg.params;
	const bool fhn = p.model == CRD_MODEL_FHN, torus = p.surface == CRD_SURFACE_TORUS;
	std::cout << (fhn ? "\n2D FHN model PDE problem on a " : "\n Goldbeter model PDE problem on a ") << (torus ? "torus" : "flat surface") << ":\n";
	std::cout << "   nprocs = " << n_slabs << "\n";
	std::cout << "   nx = " << g.nx << "\n";
	std::cout << "   ny = " << g.ny << "\n";
	std::cout << "   nxl = " << nxl0 << "\n";
	std::cout << "   nyl = " << nyl0 << "\n";
	std::cout << "   Diff = " << p.diffusion << "\n";
	std::cout << "   Tfinal = " << cfg.t_final << "\n";
	std::cout << "   Output timesteps = " << cfg.output_timestep << "\n";
	if (torus) {
		std::cout << "   Major circumference = " << p.surface_length << "\n";
		std::cout << "   Minor circumference = " << p.surface_width << "\n";
	} else {
		std::cout << "   Surface length = " << p.surface_length << "\n";
		std::cout << "   Surface width = " << p.surface_width << "\n";
	}
	if (fhn) std::cout << "   Absorbing boundary turn off time = " << p.t_boundary << "\n";
	std::cout << "   Wavelength = " << cfg.wave_length * 100 << "%\n";
	std::cout << "   Wavewidth = " << cfg.wave_width * 100 << "%\n";
	if (fhn && torus) std::cout << "   Wave inside = " << cfg.wave_inside << "\n";
	if (cfg.adaptive == 2) std::cout << "   integrator = adaptive RK4(3) on GPU\n   rtol = " << cfg.rtol << "\n   atol = " << cfg.atol << "\n";
	else if (cfg.adaptive) std::cout << "   integrator = ARKode-style ERK on GPU (Zonneveld 5(3)4, PID controller)\n   rtol = " << cfg.rtol << "\n   atol = " << cfg.atol << "\n";
	else std::cout << "   integrator = classical RK4 on GPU, dt = " << dt << " (" << steps_per_output << " steps per output)\n";
	if (!fhn && p.just_diffusion == 1) {
		std::cout << "   Diffusion Only\n\n";
		return;
	}
	std::cout << "   Include all variables in output = " << cfg.include_all_vars << "\n";
	if (!fhn) std::cout << "   Absorbing boundary turn off time = " << p.t_boundary << "\n";
	if (p.vary_beta == 0) {
		std::cout << "   Beta = " << p.beta << "\n";
		std::cout << "   Stable state values: " << (fhn ? "U = " : "Z = ") << s0 << (fhn ? ", V = " : ", Y = ") << s1 << "\n\n";
	} else {
		std::cout << "   Beta varied over " << (torus ? "torus" : "surface") << "\n";
		if (!fhn) {
			if (cfg.ic_type == 0) std::cout << "   Homogeneous ICs\n";
			if (cfg.ic_type == 1) std::cout << "   ICs: initial perturbation\n";
			if (cfg.ic_type == 2) std::cout << "   Random ICs\n";
		}
		std::cout << "\n";
	}
}

int die(const char *what, int rc, crd_ctx *ctx)
{
	std::cerr << "\nCRD_ERROR: " << what << " failed with flag = " << rc << " (" << crd_status_string(rc) << ")";
	const char *detail = crd_last_error(ctx);
	if (detail && *detail) std::cerr << ": " << detail;
	std::cerr << "\n\n";
	return 1;
}

const char *section_name(int kind)
{
	return kind == CRD_SECTION_ROW ? "row" : kind == CRD_SECTION_COLUMN ? "column" : kind == CRD_SECTION_THETA_MEAN ? "theta-mean" : "phi-mean";
}

// --section's argument: row:J, column:I, theta-mean or phi-mean.
void parse_section(const std::string &v, Options *o)
{
	if (v == "theta-mean") return (void)o->sections.emplace_back(CRD_SECTION_THETA_MEAN, 0);
	if (v == "phi-mean") return (void)o->sections.emplace_back(CRD_SECTION_PHI_MEAN, 0);
	const size_t colon = v.find(':');
	const std::string name = v.substr(0, colon), at = colon == std::string::npos ? "" : v.substr(colon + 1);
	char *end = nullptr;
	const long long index = std::strtoll(at.c_str(), &end, 10);
	if ((name != "row" && name != "column") || at.empty() || *end != '\0') usage_error("--section takes row:J, column:I, theta-mean or phi-mean (got '" + v + "')");
	o->sections.emplace_back(name == "row" ? CRD_SECTION_ROW : CRD_SECTION_COLUMN, index);
}

// An array of doubles or int32 of the given shape as a NumPy .npy file (format 1.0).
bool write_npy(const std::string &path, const void *data, size_t bytes, const char *descr, const std::string &shape)
{
	std::string head = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (" + shape + "), }";
	while ((10 + head.size() + 1) % 64) head += ' ';
	head += '\n';
	FILE *f = std::fopen(path.c_str(), "wb");
	if (!f) return false;
	const unsigned char magic[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(head.size() & 0xff), (unsigned char)(head.size() >> 8)};
	bool ok = std::fwrite(magic, 1, 10, f) == 10 && std::fwrite(head.data(), 1, head.size(), f) == head.size() && std::fwrite(data, 1, bytes, f) == bytes;
	return std::fclose(f) == 0 && ok;
}

// A [ny][nx] array of doubles as a NumPy .npy file (format 1.0).
bool write_npy_2d(const std::string &path, const std::vector<double> &a, long long ny, long long nx)
{
	std::string head = "{'descr': '<f8', 'fortran_order': False, 'shape': (" + std::to_string(ny) + ", " + std::to_string(nx) + "), }";
	while ((10 + head.size() + 1) % 64) head += ' ';
	head += '\n';
	FILE *f = std::fopen(path.c_str(), "wb");
	if (!f) return false;
	const unsigned char magic[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(head.size() & 0xff), (unsigned char)(head.size() >> 8)};
	bool ok = std::fwrite(magic, 1, 10, f) == 10 && std::fwrite(head.data(), 1, head.size(), f) == head.size() && std::fwrite(a.data(), sizeof(double), a.size(), f) == a.size();
	return std::fclose(f) == 0 && ok;
}

// What --observe leaves in <outdir>/member_<k>/: observables.txt, one line per sample in the state files' number format, and with
// --observe-maps amplitude_map.npy (running maximum - running minimum of var0) and activation_time.npy.
int write_observations(const Options &o, crd_ensemble *ens, int B)
{
	int64_t n = 0;
	int rc = crd_ensemble_observe_count(ens, &n);
	const size_t P = o.probes.size();
	std::vector<double> t((size_t)n), stats((size_t)n * (size_t)B * 8), pv((size_t)n * (size_t)B * P * 2);
	if (rc == CRD_OK) rc = crd_ensemble_observe_read(ens, 0, n, t.data(), stats.data(), pv.data());
	if (rc != CRD_OK) return rc;
	std::vector<std::vector<double>> section_values(o.sections.size());
	for (int k = 0; k < B; k++) {
		crd_grid g;  // the member's own
		if ((rc = crd_ensemble_member_grid(ens, k, &g)) != CRD_OK) return rc;
		const size_t points = (size_t)(g.nx * g.ny);
		std::vector<double> lo(points), hi(points), ta(points);
		const std::string dir = o.outdir + "/member_" + std::to_string(k);
		FILE *f = std::fopen((dir + "/observables.txt").c_str(), "w");
		if (!f) return CRD_EIO;
		std::fprintf(f, "# t min0 max0 sum0 sumsq0 min1 max1 sum1 sumsq1");
		for (const auto &q : o.probes) std::fprintf(f, " var0(%lld,%lld) var1(%lld,%lld)", q.first, q.second, q.first, q.second);
		std::fprintf(f, "\n");
		for (size_t q = 0; q < o.sections.size(); q++) {  // (further comment lines: numpy.loadtxt skips them)
			std::fprintf(f, "# section_%zu.npy: %s", q, section_name(o.sections[q].first));
			if (o.sections[q].first == CRD_SECTION_ROW || o.sections[q].first == CRD_SECTION_COLUMN) std::fprintf(f, " %lld", o.sections[q].second);
			std::fprintf(f, ", [sample, length, 2]; sample s at the time t of line s below\n");
		}
		if (!o.sections.empty()) {
			std::fprintf(f, "# sample times:");
			for (size_t s = 0; s < (size_t)n; s++) std::fprintf(f, " %.16e", t[s]);
			std::fprintf(f, "\n");
		}
		for (size_t s = 0; s < (size_t)n; s++) {
			std::fprintf(f, "%.16e", t[s]);
			for (int c = 0; c < 8; c++) std::fprintf(f, " %.16e", stats[(s * (size_t)B + (size_t)k) * 8 + (size_t)c]);
			for (size_t c = 0; c < 2 * P; c++) std::fprintf(f, " %.16e", pv[(s * (size_t)B + (size_t)k) * 2 * P + c]);
			std::fprintf(f, "\n");
		}
		if (std::fclose(f) != 0) return CRD_EIO;
		for (size_t q = 0; q < o.sections.size(); q++) {  // the member's lines out of the section's [sample][member][length][2]
			int64_t length = 0;
			if ((rc = crd_ensemble_observe_section_info(ens, (int)q, nullptr, nullptr, &length, nullptr)) != CRD_OK) return rc;
			const size_t line = (size_t)length * 2;
			if (k == 0) {
				section_values[q].resize((size_t)n * (size_t)B * line);
				if ((rc = crd_ensemble_observe_read_section(ens, (int)q, 0, n, section_values[q].data())) != CRD_OK) return rc;
			}
			std::vector<double> mine((size_t)n * line);
			for (size_t s = 0; s < (size_t)n; s++)
				std::copy(section_values[q].begin() + (ptrdiff_t)((s * (size_t)B + (size_t)k) * line), section_values[q].begin() + (ptrdiff_t)((s * (size_t)B + (size_t)k + 1) * line), mine.begin() + (ptrdiff_t)(s * line));
			if (!write_npy(dir + "/section_" + std::to_string(q) + ".npy", mine.data(), mine.size() * sizeof(double), "<f8", std::to_string(n) + ", " + std::to_string(length) + ", 2")) return CRD_EIO;
		}
		if (o.observe_cycles) {
			std::vector<int32_t> count(points);
			std::vector<double> tf(points), tl(points), period(points, std::nan(""));
			if ((rc = crd_ensemble_observe_cycles(ens, k, count.data(), tf.data(), tl.data())) != CRD_OK) return rc;
			for (size_t q = 0; q < points; q++)
				if (count[q] >= 2) period[q] = (tl[q] - tf[q]) / (double)(count[q] - 1);
			const std::string shape = std::to_string(g.ny) + ", " + std::to_string(g.nx);
			if (!write_npy(dir + "/activation_count.npy", count.data(), points * sizeof(int32_t), "<i4", shape) || !write_npy_2d(dir + "/period_map.npy", period, g.ny, g.nx)) return CRD_EIO;
		}
		if (!o.observe_maps) continue;
		if ((rc = crd_ensemble_observe_maps(ens, k, lo.data(), hi.data(), ta.data())) != CRD_OK) return rc;
		for (size_t q = 0; q < points; q++) hi[q] -= lo[q];
		if (!write_npy_2d(dir + "/amplitude_map.npy", hi, g.ny, g.nx) || !write_npy_2d(dir + "/activation_time.npy", ta, g.ny, g.nx)) return CRD_EIO;
	}
	return CRD_OK;
}

// What --observe leaves in <outdir> itself for a run without --ensemble: the files a member's directory gets, in the same formats, read
// from the run recorder (crd_recorder_*) -- whole-grid planes whatever the number of slabs.
int write_recording(const Options &o, crd_recorder *rec, const crd_grid &g)
{
	int64_t n = 0;
	int rc = crd_recorder_count(rec, &n);
	const size_t P = o.probes.size(), points = (size_t)(g.nx * g.ny);
	std::vector<double> t((size_t)n), stats((size_t)n * 8), pv((size_t)n * P * 2);
	if (rc == CRD_OK) rc = crd_recorder_read(rec, 0, n, t.data(), stats.data(), pv.data());
	if (rc != CRD_OK) return rc;
	FILE *f = std::fopen((o.outdir + "/observables.txt").c_str(), "w");
	if (!f) return CRD_EIO;
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
		for (size_t s = 0; s < (size_t)n; s++) std::fprintf(f, " %.16e", t[s]);
		std::fprintf(f, "\n");
	}
	for (size_t s = 0; s < (size_t)n; s++) {
		std::fprintf(f, "%.16e", t[s]);
		for (int c = 0; c < 8; c++) std::fprintf(f, " %.16e", stats[s * 8 + (size_t)c]);
		for (size_t c = 0; c < 2 * P; c++) std::fprintf(f, " %.16e", pv[s * 2 * P + c]);
		std::fprintf(f, "\n");
	}
	if (std::fclose(f) != 0) return CRD_EIO;
	for (size_t q = 0; q < o.sections.size(); q++) {
		int64_t length = 0;
		if ((rc = crd_recorder_section_info(rec, (int)q, nullptr, nullptr, &length, nullptr)) != CRD_OK) return rc;
		std::vector<double> lines((size_t)n * (size_t)length * 2);
		if (n > 0 && (rc = crd_recorder_read_section(rec, (int)q, 0, n, lines.data())) != CRD_OK) return rc;
		if (!write_npy(o.outdir + "/section_" + std::to_string(q) + ".npy", lines.data(), lines.size() * sizeof(double), "<f8", std::to_string(n) + ", " + std::to_string(length) + ", 2")) return CRD_EIO;
	}
	if (o.observe_cycles) {
		std::vector<int32_t> count(points);
		std::vector<double> tf(points), tl(points), period(points, std::nan(""));
		if ((rc = crd_recorder_cycles(rec, count.data(), tf.data(), tl.data())) != CRD_OK) return rc;
		for (size_t q = 0; q < points; q++)
			if (count[q] >= 2) period[q] = (tl[q] - tf[q]) / (double)(count[q] - 1);
		const std::string shape = std::to_string(g.ny) + ", " + std::to_string(g.nx);
		if (!write_npy(o.outdir + "/activation_count.npy", count.data(), points * sizeof(int32_t), "<i4", shape) || !write_npy_2d(o.outdir + "/period_map.npy", period, g.ny, g.nx)) return CRD_EIO;
	}
	if (o.observe_maps) {
		std::vector<double> lo(points), hi(points), ta(points);
		if ((rc = crd_recorder_maps(rec, lo.data(), hi.data(), ta.data())) != CRD_OK) return rc;
		for (size_t q = 0; q < points; q++) hi[q] -= lo[q];
		if (!write_npy_2d(o.outdir + "/amplitude_map.npy", hi, g.ny, g.nx) || !write_npy_2d(o.outdir + "/activation_time.npy", ta, g.ny, g.nx)) return CRD_EIO;
	}
	return CRD_OK;
}

}  // namespace

// --ensemble: the run of the ini once per member, the members' parameters zipped from the lists, all stepped together on one GPU
// (crd_ensemble_*).  Member k writes the reference's files of a single-rank run into <outdir>/member_<k>/, from its own initial
// conditions.  Fixed steps: all members take one step size, the ini's / --dt's, else the smallest member's dtSafety x crd_stable_dt.
// [Solver] adaptive = 1 in the ini: error-controlled, one crd_ensemble_integrate_adaptive call per output (a lone adaptive run's
// crd_group_integrate_adaptive call), each member with its own step sequence.  A member whose state goes non-finite, or whose
// integrator fails, is written no further from that output on, as a lone run stops there; the others run to tFinal, and the run then
// exits 1 naming it.
int run_ensemble(const Options &o, crd_run_config cfg)
{
	if (cfg.adaptive == 2)
		usage_error("--ensemble integrates error-controlled with ARKode's pair only: the ini asks for [Solver] adaptive = 2 (RK4(3); pass --fixed, or set adaptive = 1)");
	const bool adaptive = cfg.adaptive == 1;
	if (adaptive && o.ensemble_steps)
		usage_error("--ensemble-steps sets the steps of a fixed-step launch: the ini asks for [Solver] adaptive = 1, which takes attempts, not steps (pass --fixed)");
	const bool own_dt = o.ensemble_own_dt;
	if (own_dt && adaptive) usage_error("--ensemble-own-dt sets the steps of the fixed-step path: the ini asks for [Solver] adaptive = 1, where every member takes its own steps already (pass --fixed)");
	if (own_dt && cfg.dt > 0) usage_error("--ensemble-own-dt gives every member its own step size: the ini pins [Solver] dt = " + std::to_string(cfg.dt) + " for all (set dt = 0)");
	if (cfg.n_gpus > 1) usage_error("--ensemble runs on one GPU: the ini asks for [Solver] gpus = " + std::to_string(cfg.n_gpus) + " (pass --gpus 1)");
	const int B = (int)o.ensemble[0].second.size();
	std::vector<crd_run_config> mc((size_t)B, cfg);
	std::vector<crd_params> mp((size_t)B);
	for (int k = 0; k < B; k++) {
		for (const auto &kv : o.ensemble) set_ensemble_value(kv.first, kv.second[(size_t)k], &mc[(size_t)k].params);
		mp[(size_t)k] = mc[(size_t)k].params;
	}
	// With a geometry key the members may differ in surface and grid (crd_ensemble_create_mixed); where nx or ny truly differ, what
	// such an ensemble refuses is refused here, before any device is asked for, by the option's name.
	bool geometry = false;
	for (const auto &kv : o.ensemble) geometry = geometry || ensemble_geometry_key(kv.first);
	std::vector<crd_grid> mg((size_t)B);
	bool shapes_differ = false;
	for (int k = 0; k < B; k++) {
		if (crd_grid_from_params(&mp[(size_t)k], &mg[(size_t)k]) != CRD_OK) usage_error("member " + std::to_string(k) + ": bad geometry");
		shapes_differ = shapes_differ || mg[(size_t)k].nx != mg[0].nx || mg[(size_t)k].ny != mg[0].ny;
	}
	if (geometry && shapes_differ) {
		if (adaptive) usage_error("[Solver] adaptive = 1: members of different shape integrate with fixed steps only (pass --fixed)");
		if (!o.sections.empty()) usage_error("--section: members of different shape take no sections");
		if (o.observe_cycles) usage_error("--observe-cycles: members of different shape take no cycle maps");
	}
	const int Nt = cfg.output_timestep;
	const double dTout = cfg.t_final / Nt;
	double dt_cap = cfg.dt;
	int dt_member = -1;
	if (!(dt_cap > 0))
		for (int k = 0; k < B; k++) {
			const double c = cfg.dt_safety * crd_stable_dt(&mp[(size_t)k]);
			if (dt_member < 0 || c < dt_cap) dt_cap = c, dt_member = k;
		}
	const int64_t steps_per_output = (int64_t)std::ceil(dTout / dt_cap - 1e-12);
	const double dt = dTout / (double)steps_per_output;

	if (o.observe) {  // (refused before any device is asked for)
		const crd_grid &pg = mg[0];
		for (const auto &q : o.probes)
			for (int k = 0; k < B; k++) {
				const crd_grid &kg = mg[(size_t)k];
				if (q.first < 0 || q.first >= kg.nx || q.second < 0 || q.second >= kg.ny)
					usage_error("--probe " + std::to_string(q.first) + "," + std::to_string(q.second) + " is outside the " + std::to_string(kg.nx) + " x " + std::to_string(kg.ny) + " grid" +
					            (shapes_differ ? " of member " + std::to_string(k) : std::string()));
			}
		for (const auto &q : o.sections)
			if ((q.first == CRD_SECTION_ROW && (q.second < 0 || q.second >= pg.ny)) || (q.first == CRD_SECTION_COLUMN && (q.second < 0 || q.second >= pg.nx)))
				usage_error(std::string("--section ") + section_name(q.first) + ":" + std::to_string(q.second) + " is outside the " + std::to_string(pg.nx) + " x " + std::to_string(pg.ny) + " grid");
	}

	crd_ensemble *ens = nullptr;
	int rc = geometry ? crd_ensemble_create_mixed(mp.data(), B, 0, &ens) : crd_ensemble_create(mp.data(), B, 0, &ens);
	if (rc != CRD_OK) {
		std::cerr << "\nCRD_ERROR: " << (geometry ? "crd_ensemble_create_mixed" : "crd_ensemble_create") << " failed with flag = " << rc << " (" << crd_status_string(rc) << "): " << crd_ensemble_last_error(nullptr) << "\n\n";
		return 1;
	}
	if (o.ensemble_steps && (rc = crd_ensemble_set_steps_per_launch(ens, o.ensemble_steps)) != CRD_OK) {
		std::cerr << "\nCRD_ERROR: --ensemble-steps " << o.ensemble_steps << ": " << crd_ensemble_last_error(ens) << "\n\n";
		crd_ensemble_destroy(ens);
		return 1;
	}
	// --ensemble-own-dt: member k takes own_n[k] steps of dTout / own_n[k] per output, a lone run's count and step size for its ini.
	// The step sizes are handed over as formed here (crd_ensemble_step_rk4_own_dt): (t + dTout) - t need not be dTout.
	std::vector<int64_t> own_n((size_t)B, 0);
	std::vector<double> own_step((size_t)B, 0.0);
	if (own_dt) {
		if ((rc = crd_ensemble_own_steps(ens, 0.0, dTout, cfg.dt_safety, own_n.data())) != CRD_OK) {
			std::cerr << "\nCRD_ERROR: --ensemble-own-dt: " << crd_ensemble_last_error(ens) << "\n\n";
			crd_ensemble_destroy(ens);
			return 1;
		}
		for (int k = 0; k < B; k++) own_step[(size_t)k] = dTout / (double)own_n[(size_t)k];
	}
	crd_grid g;
	crd_ensemble_info(ens, nullptr, &g);
	if (!o.quiet) {
		std::cout << "\nEnsemble of " << B << " members on one GPU (" << (mp[0].model == CRD_MODEL_FHN ? "FHN" : "Goldbeter") << ", "
		          << (geometry ? std::string("each member's own surface and grid") : std::string(mp[0].surface == CRD_SURFACE_TORUS ? "torus" : "flat surface") + ", nx = " + std::to_string(g.nx) + ", ny = " + std::to_string(g.ny)) << "):\n";
		for (int k = 0; k < B; k++) {
			std::cout << "   member " << k << ":";
			for (const auto &kv : o.ensemble) std::cout << " " << kv.first << " = " << kv.second[(size_t)k];
			if (geometry) std::cout << "  (" << mg[(size_t)k].nx << " x " << mg[(size_t)k].ny << ")";
			std::cout << "  -> " << o.outdir << "/member_" << k << "\n";
		}
		std::cout << "   Tfinal = " << cfg.t_final << ", output timesteps = " << Nt << "\n";
		if (adaptive)
			std::cout << "   integrator = ARKode-style ERK on GPU (Zonneveld 5(3)4, PID controller), each member its own steps\n   rtol = " << cfg.rtol
			          << "\n   atol = " << cfg.atol << "\n";
		else if (own_dt) {
			std::cout << "   integrator = classical RK4 on GPU, every member at its own dtSafety x stable dt (single steps, one launch per round)\n";
			for (int k = 0; k < B; k++) std::cout << "   member " << k << ": dt = " << own_step[(size_t)k] << " (" << own_n[(size_t)k] << " steps per output)\n";
		} else
			std::cout << "   integrator = classical RK4 on GPU, dt = " << dt << " (" << steps_per_output << " steps per output; "
			          << (dt_member < 0 ? std::string("from [Solver] dt / --dt") : "the smallest member's dtSafety x stable dt: member " + std::to_string(dt_member)) << ")\n"
			          << (crd_ensemble_get_steps_per_launch(ens) == 2 ? "   two steps per launch\n" : "");
	}

	std::vector<crd_writer *> wr((size_t)B, nullptr);
	int64_t most_points = 0;
	for (const crd_grid &kg : mg) most_points = std::max(most_points, kg.nx * kg.ny);
	std::vector<double> buf((size_t)(2 * most_points));  // (the largest member's state; a member fills its own nx * ny pairs)
	auto cleanup = [&]() {
		for (auto *w : wr) crd_writer_close(w);
		crd_ensemble_destroy(ens);
	};
	for (int k = 0; k < B; k++) {
		const std::string dir = o.outdir + "/member_" + std::to_string(k);
		std::error_code ec;
		std::filesystem::create_directories(dir, ec);
		if ((rc = crd_initial_conditions(&mc[(size_t)k], 0, mg[(size_t)k].ny - 1, buf.data())) != CRD_OK) {
			die("crd_initial_conditions", rc, nullptr);
			cleanup();
			return 1;
		}
		if ((rc = crd_writer_open(&mc[(size_t)k], dir.c_str(), 0, 1, &wr[(size_t)k])) != CRD_OK || (rc = crd_writer_write_row(wr[(size_t)k], buf.data())) != CRD_OK) {
			die("crd_writer", rc, nullptr);
			cleanup();
			return 1;
		}
		if ((rc = crd_ensemble_upload(ens, k, buf.data(), 1)) != CRD_OK) {
			std::cerr << "\nCRD_ERROR: crd_ensemble_upload failed: " << crd_ensemble_last_error(ens) << "\n\n";
			cleanup();
			return 1;
		}
	}

	if (o.observe) {
		crd_observe_options oo{};
		oo.stride = o.observe_stride;
		oo.n_probes = (int32_t)o.probes.size();
		for (size_t q = 0; q < o.probes.size(); q++) {
			oo.probe_i[q] = (int32_t)o.probes[q].first;
			oo.probe_j[q] = (int32_t)o.probes[q].second;
		}
		oo.maps = o.observe_maps ? 1 : 0;
		oo.threshold = o.observe_threshold;
		// fixed steps: every stride-th step of the run -- floor(total steps / stride), the count the library itself reaches, since its
		// step count carries over the calls; error-controlled: one sample per output
		const int64_t capacity = (adaptive || own_dt) ? Nt : std::max<int64_t>(1, steps_per_output * Nt / oo.stride);
		crd_observe_extras ex{};
		ex.n_sections = (int32_t)o.sections.size();
		for (size_t q = 0; q < o.sections.size(); q++) {
			ex.kind[q] = o.sections[q].first;
			ex.index[q] = (int32_t)o.sections[q].second;
		}
		ex.cycles = o.observe_cycles ? 1 : 0;
		ex.cycle_threshold = o.cycle_threshold;
		const bool extras = ex.n_sections > 0 || ex.cycles;
		if ((rc = extras ? crd_ensemble_observe_begin_with(ens, &oo, &ex, capacity) : crd_ensemble_observe_begin(ens, &oo, capacity)) != CRD_OK) {
			std::cerr << "\nCRD_ERROR: crd_ensemble_observe_begin failed with flag = " << rc << " (" << crd_status_string(rc) << "): " << crd_ensemble_last_error(ens) << "\n\n";
			cleanup();
			return 1;
		}
	}

	std::vector<int> blown_at((size_t)B, 0);  // output (1-based) at which a member went non-finite; 0: never
	std::vector<int> failed_at((size_t)B, 0);  // ... at which its error-controlled integration failed
	std::vector<double> peak((size_t)B);
	std::vector<crd_adaptive_stats> as((size_t)B);
	std::vector<int32_t> member_status((size_t)B);
	std::vector<long long> accepted((size_t)B, 0), rejected((size_t)B, 0);
	crd_adaptive_options ao;
	crd_adaptive_defaults(&ao);
	ao.rtol = cfg.rtol;
	ao.atol = cfg.atol;
	ao.method = CRD_ADAPT_ARKODE;
	ao.h0 = 0.0;          // first step: arkHin; the controller's memory carries over in the ensemble
	ao.dense_output = 1;  // ARK_NORMAL: output times do not shorten steps, the row written is the interpolant at tout
	double stepping_s = 0.0;
	for (int iout = 0; iout < Nt; iout++) {
		const double t = iout * dTout;
		const auto step_t0 = std::chrono::steady_clock::now();
		if (adaptive) {
			// one ARKode(...) call per output interval for every member, src/FHNmodel_torus.cpp:423 (a failed member still takes part in
			// later calls, from the state it was left at, but is written no further)
			rc = crd_ensemble_integrate_adaptive(ens, t, (iout + 1 == Nt) ? cfg.t_final : (iout + 1) * dTout, &ao, as.data(), member_status.data());
			if (rc == CRD_ESTATE) {
				for (int k = 0; k < B; k++)
					if (member_status[(size_t)k] != CRD_OK && !failed_at[(size_t)k] && !blown_at[(size_t)k]) {
						failed_at[(size_t)k] = iout + 1;
						std::cerr << "\nSolver failure, stopping integration of member " << k << " (" << crd_ensemble_last_error(ens) << ")\n";  // src/FHNmodel_torus.cpp:433
					}
				rc = CRD_OK;
			}
			for (int k = 0; k < B && rc == CRD_OK; k++)
				if (!failed_at[(size_t)k] && !blown_at[(size_t)k]) accepted[(size_t)k] += as[(size_t)k].accepted, rejected[(size_t)k] += as[(size_t)k].rejected;
		} else if (own_dt) {
			// (the time given is the observer sample's alone: the output time as the error-controlled branch forms it)
			rc = crd_ensemble_step_rk4_own_dt(ens, t, (iout + 1 == Nt) ? cfg.t_final : (iout + 1) * dTout, own_step.data(), own_n.data());
		} else {
			rc = crd_ensemble_step_rk4(ens, t, dt, steps_per_output);
		}
		if (rc == CRD_OK) rc = crd_ensemble_synchronize(ens);
		stepping_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - step_t0).count();
		if (rc == CRD_OK) rc = crd_ensemble_max_abs(ens, peak.data());
		for (int k = 0; k < B && rc == CRD_OK; k++) {
			if (blown_at[(size_t)k] || failed_at[(size_t)k]) continue;
			if (!std::isfinite(peak[(size_t)k])) {
				blown_at[(size_t)k] = iout + 1;
				std::cerr << "\nSolver failure, stopping integration of member " << k << " (non-finite state at output " << iout + 1 << ")\n";  // src/FHNmodel_torus.cpp:433
				continue;
			}
			if ((rc = crd_ensemble_download(ens, k, buf.data(), 1)) == CRD_OK) rc = crd_writer_write_row(wr[(size_t)k], buf.data());
		}
		if (rc != CRD_OK) {
			std::cerr << "\nCRD_ERROR: ensemble stepping / output failed with flag = " << rc << " (" << crd_status_string(rc) << "): " << crd_ensemble_last_error(ens) << "\n\n";
			cleanup();
			return 1;
		}
		if (!o.quiet) {
			std::printf("%s   %3d %%", iout > 0 ? "\r" : "", 100 * (iout + 1) / Nt);
			std::fflush(stdout);
		}
	}
	if (o.observe && (rc = write_observations(o, ens, B)) != CRD_OK) {
		std::cerr << "\nCRD_ERROR: writing the observations failed with flag = " << rc << " (" << crd_status_string(rc) << "): " << crd_ensemble_last_error(ens) << "\n\n";
		cleanup();
		return 1;
	}
	int status = 0;
	for (int k = 0; k < B; k++)
		if (blown_at[(size_t)k]) {
			std::cerr << "member " << k << " blew up at output " << blown_at[(size_t)k] << " of " << Nt << "; its files stop there\n";
			status = 1;
		} else if (failed_at[(size_t)k]) {
			std::cerr << "member " << k << " failed its error-controlled integration at output " << failed_at[(size_t)k] << " of " << Nt << "; its files stop there\n";
			status = 1;
		}
	if (!o.quiet && adaptive) {
		std::cout << "\n";
		for (int k = 0; k < B; k++) std::cout << "   member " << k << ": steps = " << accepted[(size_t)k] << " (+" << rejected[(size_t)k] << " rejected)\n";
	}
	if (!o.quiet && adaptive && stepping_s > 0.0) {
		long long attempts = 0;
		for (int k = 0; k < B; k++) attempts += accepted[(size_t)k] + rejected[(size_t)k];
		std::printf("   rate: %d members, %lld attempts in %.6f s of stepping = %.1f attempts/s\n", B, attempts, stepping_s, (double)attempts / stepping_s);
		std::cout << "   ----------------------\n";
	} else if (!o.quiet && own_dt && stepping_s > 0.0) {
		double point_steps = 0.0;  // sum over the members of points x steps per output
		long long most = 0;
		for (int k = 0; k < B; k++) {
			point_steps += (double)mg[(size_t)k].nx * (double)mg[(size_t)k].ny * (double)own_n[(size_t)k];
			most = std::max(most, (long long)own_n[(size_t)k]);
		}
		std::printf("\n   rate: %d members at their own step sizes, %lld rounds in %.6f s of stepping = %.4g grid-point-steps/s\n", B, most * Nt, stepping_s, point_steps * Nt / stepping_s);
		std::cout << "   ----------------------\n";
	} else if (!o.quiet && stepping_s > 0.0) {
		double points = 0.0;  // (every member's own grid: they may differ in shape)
		for (const crd_grid &kg : mg) points += (double)kg.nx * (double)kg.ny;
		const double ps = points * (double)steps_per_output * Nt / stepping_s;
		std::printf("\n   rate: %d members x %lld steps in %.6f s of stepping = %.4g grid-point-steps/s\n", B, (long long)steps_per_output * Nt, stepping_s, ps);
		std::cout << "   ----------------------\n";
	}
	cleanup();
	return status;
}

// Rank and size an MPI launcher gave this process through its environment (no MPI library is linked).
struct Launcher {
	int rank = 0, size = 1;
	const char *kind = "";
};
static Launcher detect_launcher()
{
	static const struct {
		const char *rank, *size, *kind;
	} known[] = {{"OMPI_COMM_WORLD_RANK", "OMPI_COMM_WORLD_SIZE", "Open MPI"},
	             {"PMI_RANK", "PMI_SIZE", "MPICH / Hydra"},
	             {"MV2_COMM_WORLD_RANK", "MV2_COMM_WORLD_SIZE", "MVAPICH"}};
	Launcher l;
	for (const auto &k : known) {
		const char *r = std::getenv(k.rank), *n = std::getenv(k.size);
		if (r && n && std::atoi(n) >= 1 && std::atoi(r) >= 0 && std::atoi(r) < std::atoi(n)) {
			l.rank = std::atoi(r);
			l.size = std::atoi(n);
			l.kind = k.kind;
			break;
		}
	}
	return l;
}

int main(int argc, char *argv[])
{
	Options o;
	std::string base = argv[0];
	const size_t slash = base.find_last_of('/');
	if (slash != std::string::npos) base = base.substr(slash + 1);
	const bool alias = preset_from_name(base, &o);

	if (alias) {
		if (argc != 2) usage(argv[0], true);  // src/FHNmodel_torus.cpp:151-155
		o.ini = argv[1];
	} else {
		for (int a = 1; a < argc; a++) {
			const std::string s = argv[a];
			auto next = [&]() -> std::string {
				if (a + 1 >= argc) usage(argv[0], false);
				return argv[++a];
			};
			if (s == "--model") {
				const std::string v = next();
				o.model = v == "fhn" ? CRD_MODEL_FHN : v == "goldbeter" ? CRD_MODEL_GOLDBETER : -1;
			} else if (s == "--surface") {
				const std::string v = next();
				o.surface = v == "torus" ? CRD_SURFACE_TORUS : v == "flat" ? CRD_SURFACE_FLAT : -1;
			} else if (s == "--gpus") o.gpus = std::atoi(next().c_str());
			else if (s == "--devices") o.devices = std::atoi(next().c_str());
			else if (s == "--dt") o.dt = std::atof(next().c_str());
			else if (s == "--outdir") o.outdir = next();
			else if (s == "--quiet") o.quiet = true;
			else if (s == "--adaptive") o.adaptive = 1;
			else if (s == "--adaptive-rk43") o.adaptive = 2;
			else if (s == "--fixed") o.adaptive = 0;
			else if (s == "--binary") o.binary = true;
			else if (s == "--binary-only") o.binary = o.binary_only = true;
			else if (s == "--ref-steady-state") o.ref_steady_state = true;
			else if (s == "--block-contexts") o.block_contexts = true;
			else if (s == "--ensemble") parse_ensemble(next(), &o);
			else if (s == "--ensemble-own-dt") o.ensemble_own_dt = true;
			else if (s == "--ensemble-steps") {
				const std::string v = next();
				o.ensemble_steps = v == "1" ? 1 : v == "2" ? 2 : 0;
				if (!o.ensemble_steps) usage_error("--ensemble-steps takes 1 or 2 (got '" + v + "')");
			}
			else if (s == "--observe") {
				const std::string v = next();
				char *end = nullptr;
				o.observe = true;
				o.observe_stride = std::strtoll(v.c_str(), &end, 10);
				if (v.empty() || *end != '\0') usage_error("--observe takes a stride, a whole number of steps (got '" + v + "')");
			} else if (s == "--probe") {
				const std::string v = next();
				long long i = 0, j = 0;
				int used = 0;
				if (std::sscanf(v.c_str(), "%lld,%lld%n", &i, &j, &used) != 2 || used != (int)v.size()) usage_error("--probe takes I,J, a grid point's theta and phi index (got '" + v + "')");
				o.probes.emplace_back(i, j);
			} else if (s == "--observe-maps") {
				const std::string v = next();
				char *end = nullptr;
				o.observe_maps = true;
				o.observe_threshold = std::strtod(v.c_str(), &end);
				if (v.empty() || *end != '\0' || !std::isfinite(o.observe_threshold)) usage_error("--observe-maps takes a threshold, a number (got '" + v + "')");
			} else if (s == "--section") {
				parse_section(next(), &o);
			} else if (s == "--observe-cycles") {
				const std::string v = next();
				char *end = nullptr;
				o.observe_cycles = true;
				o.cycle_threshold = std::strtod(v.c_str(), &end);
				if (v.empty() || *end != '\0' || !std::isfinite(o.cycle_threshold)) usage_error("--observe-cycles takes a threshold, a number (got '" + v + "')");
			}
			else if (s == "--decomp") {
				const std::string v = next();
				if (v == "mpi") o.decomp_mpi = true;
				else if (std::sscanf(v.c_str(), "%dx%d", &o.d0, &o.d1) != 2 || o.d0 < 1 || o.d1 < 1) usage(argv[0], false);
			}
			else if (s == "--precision") {
				const std::string v = next();
				o.precision = v == "32" ? CRD_PRECISION_F32 : v == "64" ? CRD_PRECISION_F64 : -2;
			} else if (s == "--stepper") {
				const std::string v = next();
				o.stepper = v == "auto" ? CRD_STEPPER_AUTO : v == "staged" ? CRD_STEPPER_STAGED : v == "fused" ? CRD_STEPPER_FUSED : -2;
			} else if (!s.empty() && s[0] == '-') usage(argv[0], false);
			else if (o.ini.empty()) o.ini = s;
			else usage(argv[0], false);
		}
		if (o.model < 0 || o.surface < 0 || o.ini.empty() || o.precision == -2 || o.stepper == -2) usage(argv[0], false);
		check_ensemble_options(o);
	}

	// Started by an MPI launcher the way the reference is (`mpirun -np N <exe> <ini>`, util/ShellScripts/run*.sh)?  This
	// program needs one process only: rank 0 drives N phi-slabs, one per GPU, and writes the N subdomain file sets the N
	// reference ranks would; the other ranks have nothing to do.
	const Launcher launcher = detect_launcher();
	if (launcher.size > 1 && launcher.rank != 0) return 0;

	crd_run_config cfg;
	char err[512];
	int rc = crd_config_load_ini(o.ini.c_str(), o.model, o.surface, &cfg, err, sizeof err);
	if (rc != CRD_OK) {
		std::cerr << "\nCRD_ERROR: cannot use " << o.ini << ": " << err << "\n\n";
		return 1;
	}
	if (o.gpus > 0) cfg.n_gpus = o.gpus;
	else if (launcher.size > 1 && cfg.n_gpus == 1) {
		cfg.n_gpus = launcher.size;
		if (o.devices <= 0) o.devices = std::max(1, std::min(launcher.size, crd_device_count()));
		if (!o.quiet)
			std::cout << "\n" << launcher.kind << " started " << launcher.size << " ranks: rank 0 drives " << launcher.size << " phi-slabs on " << o.devices
			          << " GPU(s), the other ranks exit\n";
	}
	if (o.dt > 0) cfg.dt = o.dt;
	if (o.stepper >= 0) cfg.stepper = o.stepper;
	if (o.precision >= 0) cfg.params.precision = o.precision;
	if (o.adaptive >= 0) cfg.adaptive = o.adaptive;
	if (o.ref_steady_state) cfg.steady_state_decimals = 8;  // numpy's print precision, util/GoldbeterModel/SolveGoldbeterODE.py:111
	if (!o.ensemble.empty()) return run_ensemble(o, cfg);
	time_t start_t = 0, end_t = 0;
	double total_t = 0, eta = 0;
	time(&start_t);

	crd_grid g;
	if ((rc = crd_grid_from_params(&cfg.params, &g)) != CRD_OK) return die("crd_grid_from_params", rc, nullptr);
	// Two decompositions.  FILES: phi-slabs (1 x gpus) unless the reference's own 2-D blocks are asked for -- `--decomp 2x2`, or
	// `--decomp mpi` = what MPI_Dims_create makes of the slab count (src/FHNmodel_torus.cpp:724-728: `mpirun -np 4` is 2 x 2): the file
	// sets, subdomain headers and (for the rand() rule) initial conditions of that process grid.  COMPUTE: phi-slabs, one per GPU (the
	// layout for one node, and the one the one-launch stepper, the error-controlled integrators and the deep halo need) -- also
	// under --decomp (round 4): the blocks' rows are cut out of the slabs' frames at output time; `--block-contexts` computes on
	// the 2-D blocks themselves instead (staged kernels, fixed step, text files), bit-equal to the whole domain's staged run.
	int fd0 = 1, fd1 = cfg.n_gpus;  // the files' process grid
	if (o.decomp_mpi) crd_dims_create(cfg.n_gpus, &fd0, &fd1);
	else if (o.d0 > 0) {
		fd0 = o.d0;
		fd1 = o.d1;
	}
	const int F = fd0 * fd1;
	const bool recut = fd0 > 1 && !o.block_contexts;  // files in a layout the contexts do not have
	const int d0 = recut ? 1 : fd0, d1 = recut ? cfg.n_gpus : fd1;  // the contexts' decomposition
	const int G = d0 * d1;
	if (fd0 > 1 && o.binary) {
		std::cerr << "\nCRD_ERROR: the .npy side-channel holds phi-slab frames: not available with theta-blocks (--decomp with more than one theta-block)\n\n";
		return 1;
	}
	if (d0 > 1 && cfg.adaptive) {
		std::cerr << "\nCRD_ERROR: theta-block contexts (--block-contexts) step with the fixed-step staged RK4 and write text files only\n\n";
		return 1;
	}
	const int ndev = o.devices > 0 ? o.devices : G;
	if (o.observe) {  // (refused before any device is asked for)
		for (const auto &q : o.probes)
			if (q.first < 0 || q.first >= g.nx || q.second < 0 || q.second >= g.ny)
				usage_error("--probe " + std::to_string(q.first) + "," + std::to_string(q.second) + " is outside the " + std::to_string(g.nx) + " x " + std::to_string(g.ny) + " grid");
		for (const auto &q : o.sections) {
			if ((q.first == CRD_SECTION_ROW && (q.second < 0 || q.second >= g.ny)) || (q.first == CRD_SECTION_COLUMN && (q.second < 0 || q.second >= g.nx)))
				usage_error(std::string("--section ") + section_name(q.first) + ":" + std::to_string(q.second) + " is outside the " + std::to_string(g.nx) + " x " + std::to_string(g.ny) + " grid");
			if (q.first == CRD_SECTION_PHI_MEAN && G > 1)
				usage_error("--section phi-mean is not recorded on more than one slab (a column's sum crosses the slabs): this run has " + std::to_string(G) + " (pass --gpus 1)");
		}
	}

	double s0 = 0, s1 = 0;  // banner only, and only printed for a constant beta (src/FHNmodel_torus.cpp:268-271)
	if (cfg.params.vary_beta == 0 && (rc = crd_steady_state_as_printed(cfg.params.model, cfg.params.beta, cfg.steady_state_decimals, &s0, &s1)) != CRD_OK)
		return die("crd_steady_state", rc, nullptr);

	// Output cadence (src/FHNmodel_torus.cpp:415-429): Nt outputs dTout apart; every interval is an integer number of
	// equal RK4 steps no longer than the requested / stable step.
	const int Nt = cfg.output_timestep;
	const double dTout = cfg.t_final / Nt;
	const double dt_cap = cfg.dt > 0 ? cfg.dt : cfg.dt_safety * crd_stable_dt(&cfg.params);
	const int64_t steps_per_output = (int64_t)std::ceil(dTout / dt_cap - 1e-12);
	const double dt = dTout / (double)steps_per_output;

	std::vector<crd_ctx *> ctx((size_t)G, nullptr);
	std::vector<crd_writer *> wr((size_t)F, nullptr);
	// recut: the frames of the F file blocks, cut out of the G slabs' frames (two sets, like the slabs' own)
	std::vector<std::vector<double>> fhost((size_t)(recut ? F : 0)), fhost_b((size_t)(recut ? F : 0));
	struct Rect {
		int64_t is, ie, js, je;
	};
	std::vector<Rect> frect((size_t)F), crect((size_t)G);
	// copy between the slabs' AoS frames (full width, rows cjs .. cje) and the blocks' (columns is .. ie of rows js .. je)
	auto recut_frames = [&](std::vector<std::vector<double>> &slabs, std::vector<std::vector<double>> &blocks, bool to_blocks) {
		for (int f = 0; f < F; f++) {
			const Rect &b = frect[(size_t)f];
			const int64_t nxl = b.ie - b.is + 1;
			for (int64_t j = b.js; j <= b.je; j++) {
				int c = 0;
				while (c + 1 < G && j > crect[(size_t)c].je) c++;
				double *slab_row = slabs[(size_t)c].data() + 2 * ((j - crect[(size_t)c].js) * g.nx + b.is), *block_row = blocks[(size_t)f].data() + 2 * (j - b.js) * nxl;
				if (to_blocks) std::memcpy(block_row, slab_row, (size_t)(2 * nxl) * sizeof(double));
				else std::memcpy(slab_row, block_row, (size_t)(2 * nxl) * sizeof(double));
			}
		}
	};
	// Two host copies of every slab: while the writer thread formats output k from one, the GPU integrates towards
	// output k+1 and downloads into the other (text output of a large grid costs more than the steps between outputs).
	std::vector<std::vector<double>> host((size_t)G), host_b((size_t)G);
	std::thread writer;
	int writer_rc = CRD_OK;
	// Binary side-channel: the owned rows of a field plane ARE the (nyl, nxl) frame of the .npy file, so a frame is one
	// device-to-host copy into page-locked memory (two sets: one being written to disk, one being filled) -- no layout change,
	// no formatting.  [slab][var][set]
	const int nvars_out = 1 + (cfg.include_all_vars == 1 ? 1 : 0);
	const size_t value_bytes = cfg.params.precision == CRD_PRECISION_F64 ? 8 : 4;
	std::vector<crd_npy_writer *> npy((size_t)(2 * G), nullptr);
	std::vector<void *> frame((size_t)(4 * G), nullptr);
	auto cleanup = [&]() {
		if (writer.joinable()) writer.join();
		for (auto *w : wr) crd_writer_close(w);
		for (auto *w : npy) crd_npy_writer_close(w);
		for (void *f : frame) crd_host_free(f);
		for (auto *c : ctx) crd_destroy(c);
	};
	for (int k = 0; k < G; k++) {
		if ((rc = crd_create_block(&cfg.params, k / d1, d0, k % d1, d1, k % ndev, &ctx[(size_t)k])) != CRD_OK) {
			die("crd_create", rc, nullptr);
			cleanup();
			return 1;
		}
		crd_set_stepper(ctx[(size_t)k], cfg.stepper);
	}
	if ((rc = crd_comm_attach_local(ctx.data(), G)) != CRD_OK) {
		die("crd_comm_attach_local", rc, ctx[0]);
		cleanup();
		return 1;
	}
	if (G > 1 && d0 == 1 && cfg.exchange_period) {
		// exchange period of the one-launch stepper: the ini's; without one the contexts keep what crd_create chose (10 steps where every
		// slab has 256 rows or more, else 8: include/crd.h, crd_set_exchange_period)
		for (int k = 0; k < G; k++)
			if ((rc = crd_set_exchange_period(ctx[(size_t)k], cfg.exchange_period)) != CRD_OK) {
				die("crd_set_exchange_period", rc, ctx[(size_t)k]);
				cleanup();
				return 1;
			}
	}

	for (int k = 0; k < G; k++) crd_get_block(ctx[(size_t)k], &crect[(size_t)k].is, &crect[(size_t)k].ie, &crect[(size_t)k].js, &crect[(size_t)k].je);
	for (int f = 0; f < F; f++) {
		if (recut) crd_block_extents(g.nx, g.ny, f / fd1, fd0, f % fd1, fd1, &frect[(size_t)f].is, &frect[(size_t)f].ie, &frect[(size_t)f].js, &frect[(size_t)f].je);
		else frect[(size_t)f] = crect[(size_t)f];
	}
	if (!o.quiet) banner(cfg, g, F, frect[0].ie - frect[0].is + 1, frect[0].je - frect[0].js + 1, s0, s1, dt, steps_per_output);

	// Initial conditions, subdomain files, first output row (src/FHNmodel_torus.cpp:285-354,376-410).  The initial conditions are
	// those of the FILES' process grid (the rand() rule draws block by block, as every reference rank does); recut: the blocks'
	// frames are then laid into the slabs' for the upload.
	for (int k = 0; k < G; k++) {
		host[(size_t)k].resize((size_t)(2 * (crect[(size_t)k].ie - crect[(size_t)k].is + 1) * (crect[(size_t)k].je - crect[(size_t)k].js + 1)));
		host_b[(size_t)k].resize(host[(size_t)k].size());
	}
	for (int f = 0; f < F; f++) {
		const Rect &b = frect[(size_t)f];
		std::vector<double> &ic = recut ? fhost[(size_t)f] : host[(size_t)f];
		if (recut) {
			fhost[(size_t)f].resize((size_t)(2 * (b.ie - b.is + 1) * (b.je - b.js + 1)));
			fhost_b[(size_t)f].resize(fhost[(size_t)f].size());
		}
		if ((rc = crd_initial_conditions_block(&cfg, b.is, b.ie, b.js, b.je, ic.data())) != CRD_OK) {
			die("crd_initial_conditions", rc, nullptr);
			cleanup();
			return 1;
		}
		if ((rc = crd_writer_open_block(&cfg, o.outdir.c_str(), f, f / fd1, fd0, f % fd1, fd1, &wr[(size_t)f])) != CRD_OK ||
		    (!o.binary_only && (rc = crd_writer_write_row(wr[(size_t)f], ic.data())) != CRD_OK)) {
			die("crd_writer", rc, nullptr);
			cleanup();
			return 1;
		}
	}
	if (recut) recut_frames(host, fhost, false);
	for (int k = 0; k < G; k++) {
		const int64_t js = crect[(size_t)k].js, je = crect[(size_t)k].je;
		if ((rc = crd_state_upload(ctx[(size_t)k], host[(size_t)k].data(), 1)) != CRD_OK) {
			die("crd_state_upload", rc, ctx[(size_t)k]);
			cleanup();
			return 1;
		}
		if (o.binary) {
			const size_t frame_bytes = (size_t)(g.nx * (je - js + 1)) * value_bytes;
			for (int v = 0; v < nvars_out && rc == CRD_OK; v++) {
				rc = crd_npy_writer_open(&cfg, o.outdir.c_str(), k, G, v, (int)value_bytes, &npy[(size_t)(2 * k + v)]);
				for (int set = 0; set < 2 && rc == CRD_OK; set++)
					if (!(frame[(size_t)(4 * k + 2 * v + set)] = crd_host_alloc(frame_bytes))) rc = CRD_ENOMEM;
				if (rc == CRD_OK) rc = crd_state_download_rows(ctx[(size_t)k], v, 0, je - js + 1, frame[(size_t)(4 * k + 2 * v)]);
				if (rc == CRD_OK) rc = crd_npy_writer_append(npy[(size_t)(2 * k + v)], frame[(size_t)(4 * k + 2 * v)]);  // the initial state
			}
			if (rc != CRD_OK) {
				die("crd_npy_writer", rc, ctx[(size_t)k]);
				cleanup();
				return 1;
			}
		}
	}

	// The one-launch stepper measures its launch plan on a context's first full-size step (~0.7 s at 8192^2): done here, ahead of the
	// first output interval, so that the rate line below is the stepping's and nothing else's.  (The error-controlled integrators
	// measure theirs inside their first attempt.)
	if (!cfg.adaptive) {
		const auto plan_t0 = std::chrono::steady_clock::now();
		for (int k = 0; k < G; k++)
			if ((rc = crd_plan_launches(ctx[(size_t)k])) != CRD_OK) {
				die("crd_plan_launches", rc, ctx[(size_t)k]);
				cleanup();
				return 1;
			}
		const double plan_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - plan_t0).count();
		crd_launch_plan lp;
		if (!o.quiet && crd_get_launch_plan(ctx[0], &lp) == CRD_OK && lp.tuned)
			std::printf("   launch plan (measured in %.2f s): chunk mode %d, XCD mapping %d, %d column(s) per lane, %s stores, %d step(s) per launch\n", plan_s, lp.one_round,
			            lp.xcd_mapping, lp.columns_per_lane, lp.nontemporal_stores ? "non-temporal" : "plain", lp.steps_per_launch);
	}

	crd_recorder *rec = nullptr;  // (closed by crd_destroy of its contexts: cleanup)
	if (o.observe) {
		crd_observe_options oo{};
		oo.stride = o.observe_stride;
		oo.n_probes = (int32_t)o.probes.size();
		for (size_t q = 0; q < o.probes.size(); q++) {
			oo.probe_i[q] = (int32_t)o.probes[q].first;
			oo.probe_j[q] = (int32_t)o.probes[q].second;
		}
		oo.maps = o.observe_maps ? 1 : 0;
		oo.threshold = o.observe_threshold;
		crd_observe_extras ex{};
		ex.n_sections = (int32_t)o.sections.size();
		for (size_t q = 0; q < o.sections.size(); q++) {
			ex.kind[q] = o.sections[q].first;
			ex.index[q] = (int32_t)o.sections[q].second;
		}
		ex.cycles = o.observe_cycles ? 1 : 0;
		ex.cycle_threshold = o.cycle_threshold;
		// fixed steps: every stride-th step of the run; error-controlled: one sample per output
		const int64_t capacity = cfg.adaptive ? Nt : std::max<int64_t>(1, steps_per_output * Nt / oo.stride);
		if ((rc = crd_recorder_open(ctx.data(), G, &oo, &ex, capacity, &rec)) != CRD_OK) {
			die("crd_recorder_open", rc, ctx[0]);
			cleanup();
			return 1;
		}
	}

	int status = 0;
	double adaptive_h = 0.0;
	long long adaptive_steps = 0, adaptive_rejected = 0;
	// Rate summary ("keep banner; add steps/s, point-steps/s, GB/s"): wall time spent inside the stepping calls
	// (they block on the download that follows, so the device work of an interval is inside its bracket) and the steps taken.
	double stepping_s = 0.0;
	long long steps_taken = 0;
	for (int iout = 0; iout < Nt; iout++) {
		const double t = iout * dTout;
		char range_name[64];
		std::snprintf(range_name, sizeof range_name, "crd_run output interval %d/%d", iout + 1, Nt);
		crd_trace_range_push(range_name);
		const auto step_t0 = std::chrono::steady_clock::now();
		auto &buf = (iout & 1) ? host_b : host;  // the other set may still be in the writer's hands
		if (cfg.adaptive) {
			// one ARKode(...) call per output interval, src/FHNmodel_torus.cpp:423; the controller's step carries over
			crd_adaptive_options ao;
			crd_adaptive_defaults(&ao);
			ao.rtol = cfg.rtol;
			ao.atol = cfg.atol;
			ao.method = cfg.adaptive == 2 ? CRD_ADAPT_RK43 : CRD_ADAPT_ARKODE;
			ao.h0 = cfg.adaptive == 2 ? adaptive_h : 0.0;  // (the ARKode-style controller keeps its own memory in the contexts; first step: arkHin)
			ao.dense_output = 1;  // ARK_NORMAL: output times do not shorten steps, the row written is the interpolant at tout
			crd_adaptive_stats as;
			rc = crd_group_integrate_adaptive(ctx.data(), G, t, (iout + 1 == Nt) ? cfg.t_final : (iout + 1) * dTout, &ao, &as);
			adaptive_h = as.h_next;
			adaptive_steps += as.accepted;
			adaptive_rejected += as.rejected;
			steps_taken += as.accepted + as.rejected;
		} else {
			rc = crd_group_step_rk4(ctx.data(), G, t, dt, steps_per_output);
			steps_taken += steps_per_output;
		}
		for (int k = 0; k < G && rc == CRD_OK; k++) rc = crd_synchronize(ctx[(size_t)k]);
		stepping_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - step_t0).count();
		const int set = (iout + 1) & 1;  // the other set of frame buffers may still be in the writer's hands
		for (int k = 0; k < G && rc == CRD_OK; k++) {
			if (!o.binary_only) rc = crd_state_download(ctx[(size_t)k], buf[(size_t)k].data(), 1);
			int64_t js, je;
			crd_get_slab(ctx[(size_t)k], &js, &je);
			for (int v = 0; o.binary && v < nvars_out && rc == CRD_OK; v++)
				rc = crd_state_download_rows(ctx[(size_t)k], v, 0, je - js + 1, frame[(size_t)(4 * k + 2 * v + set)]);
		}
		// the reference stops at the first failing ARKode call on ANY rank (src/FHNmodel_torus.cpp:424-435): look at every slab
		bool blown = false;  // sticky: a NaN / Inf on ANY slab stops the run, whatever the later slabs hold
		for (int k = 0; k < G && rc == CRD_OK; k++) {
			double pk = 0;
			rc = crd_state_max_abs(ctx[(size_t)k], &pk);
			blown = blown || !std::isfinite(pk);
		}
		if (rc != CRD_OK || blown) {
			if (rc != CRD_OK) die("crd_group_step_rk4", rc, ctx[0]);
			std::cerr << "Solver failure, stopping integration\n";  // src/FHNmodel_torus.cpp:433
			status = 1;
			crd_trace_range_pop();
			break;
		}
		if (writer.joinable()) writer.join();
		if (writer_rc != CRD_OK) {
			die("crd_writer_write_row", writer_rc, nullptr);
			status = 1;
			crd_trace_range_pop();
			break;
		}
		auto &fbuf = (iout & 1) ? fhost_b : fhost;
		writer = std::thread([&wr, &buf, &fbuf, &writer_rc, &npy, &frame, &o, &recut_frames, G, F, recut, set, nvars_out]() {
			for (int k = 0; k < G && writer_rc == CRD_OK; k++)
				for (int v = 0; o.binary && v < nvars_out && writer_rc == CRD_OK; v++)
					writer_rc = crd_npy_writer_append(npy[(size_t)(2 * k + v)], frame[(size_t)(4 * k + 2 * v + set)]);
			if (recut && !o.binary_only) recut_frames(buf, fbuf, true);  // the file blocks' frames out of the slabs' (on the writer's time)
			for (int f = 0; f < F && !o.binary_only && writer_rc == CRD_OK; f++)
				writer_rc = crd_writer_write_row(wr[(size_t)f], (recut ? fbuf : buf)[(size_t)f].data());
		});

		// progress line, src/FHNmodel_torus.cpp:457-477
		time(&end_t);
		total_t += difftime(end_t, start_t);
		start_t = end_t;
		eta = (Nt - (iout + 1)) * (total_t / (iout + 1));
		if (!o.quiet) {
			if (iout > 0) std::printf("\r");
			std::printf("   %3d %% | %3d min %2d sec elapsed | %3d min %2d sec remaining", 100 * (iout + 1) / Nt, (int)(total_t / 60), ((int)total_t % 60),
			            (int)(eta / 60), ((int)eta % 60));
			std::fflush(stdout);
		}
		crd_trace_range_pop();
	}
	if (writer.joinable()) writer.join();
	if (writer_rc != CRD_OK && status == 0) status = die("crd_writer_write_row", writer_rc, nullptr);
	if (rec && (rc = write_recording(o, rec, g)) != CRD_OK && status == 0) status = die("writing the recording", rc, ctx[0]);
	if (!o.quiet && cfg.adaptive) std::cout << "\n   steps = " << adaptive_steps << " (+" << adaptive_rejected << " rejected)";
	if (!o.quiet && steps_taken > 0 && stepping_s > 0.0) {
		// compulsory-byte model of a step: both fields read once and written once (the one-launch stepper's traffic; the four
		// stage kernels move 8 x that)
		crd_launch_plan lp{};
		const bool pairs = !cfg.adaptive && crd_get_launch_plan(ctx[0], &lp) == CRD_OK && lp.tuned && lp.steps_per_launch == 2;
		const double points = (double)g.nx * (double)g.ny, bytes_per_point_step = 4.0 * (double)value_bytes / (pairs ? 2.0 : 1.0);  // (two steps per launch: the state crosses memory once per two)
		char line[256];
		std::snprintf(line, sizeof line, "\n   rate: %lld steps in %.6f s of stepping = %.1f steps/s, %.4g grid-point-steps/s, %.1f GB/s (%g B per point-step)",
		              steps_taken, stepping_s, (double)steps_taken / stepping_s, points * (double)steps_taken / stepping_s,
		              points * (double)steps_taken * bytes_per_point_step / stepping_s / 1e9, bytes_per_point_step);
		std::cout << line;
	}
	if (!o.quiet) std::cout << "\n   ----------------------\n";
	cleanup();
	return status;
}
