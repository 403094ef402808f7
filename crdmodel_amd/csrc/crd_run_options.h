// crd_run_options.h -- what the driver (crd_run.cpp) is asked for: its options, the usage text, the parsers, the checks across options
// that refuse a command line before any device is touched, and what the options make of a configuration for the library (output
// cadence, observe request, error-controlled stepping).  Plain C++17 over include/crd.h.
#ifndef CRD_RUN_OPTIONS_H
#define CRD_RUN_OPTIONS_H

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <utility>
#include <vector>

#include "crd.h"

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
	// --imex euler|ars222|ars443: a lone single-slab run stepped by crd_step_imex (CRD_IMEX_*) at the run's fixed dt; -1: not given.
	// (Not in the usage text, whose bytes the recorded refusals of tests/golden/driver_refusals.json pin: README.md and INTEGRATION.md name it.)
	int imex = -1;
	// --imex-solver gmres|bicgstab|bicgstab-warm: the linear solver of every stage (CRD_IMEX_SOLVER_*); valid only with --imex; -1: not
	// given, crd_imex_defaults' (GMRES).  Not in the usage text either, for the same reason.
	int imex_solver = -1;
	// --imex-adaptive: the IMEX run finds its own steps from the ini's rtol / atol (crd_integrate_imex); valid only with --imex ars443.
	// Not in the usage text either.
	bool imex_adaptive = false;
};

[[noreturn]] inline void usage(const char *argv0, bool alias)
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

[[noreturn]] inline void usage_error(const std::string &msg)
{
	std::cerr << "\nCRD_ERROR: " << msg << "\n\n";
	std::exit(EXIT_FAILURE);  // (the status of any bad option)
}

inline bool preset_from_name(const std::string &base, Options *o)
{
	if (base == "FHNmodel_torus") { o->model = CRD_MODEL_FHN; o->surface = CRD_SURFACE_TORUS; return true; }
	if (base == "FHNmodel_flat") { o->model = CRD_MODEL_FHN; o->surface = CRD_SURFACE_FLAT; return true; }
	if (base == "GoldbeterModel_torus") { o->model = CRD_MODEL_GOLDBETER; o->surface = CRD_SURFACE_TORUS; return true; }
	if (base == "GoldbeterModel_flat") { o->model = CRD_MODEL_GOLDBETER; o->surface = CRD_SURFACE_FLAT; return true; }
	return false;
}

// Keys --ensemble takes: the parameters members of one ensemble may differ in (crd_ensemble_create), by their ini names.
inline double *ensemble_field(const std::string &key, crd_params *p)
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
inline bool ensemble_geometry_key(const std::string &key) { return key == "surfaceLength" || key == "surfaceWidth" || key == "xMesh" || key == "surface"; }
inline bool ensemble_key(const std::string &key)
{
	crd_params probe{};
	return ensemble_field(key, &probe) || key == "xMesh" || key == "surface";
}
inline void set_ensemble_value(const std::string &key, double value, crd_params *p)
{
	if (key == "xMesh") p->nx = (int64_t)value;
	else if (key == "surface") p->surface = (int)value;
	else *ensemble_field(key, p) = value;
}

// The options that validate their number: the whole of v as one whole number, or as one finite number, else the option's refusal.
inline long long whole_number(const std::string &v, const std::string &refusal)
{
	char *end = nullptr;
	const long long x = std::strtoll(v.c_str(), &end, 10);
	if (v.empty() || *end != '\0') usage_error(refusal);
	return x;
}
inline double finite_number(const std::string &v, const std::string &refusal)
{
	char *end = nullptr;
	const double x = std::strtod(v.c_str(), &end);
	if (v.empty() || *end != '\0' || !std::isfinite(x)) usage_error(refusal);
	return x;
}

inline void parse_ensemble(const std::string &arg, Options *o)
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
			const double x = finite_number(v, "--ensemble " + key + ": '" + v + "' is not a number");
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

inline const char *section_name(int kind)
{
	return kind == CRD_SECTION_ROW ? "row" : kind == CRD_SECTION_COLUMN ? "column" : kind == CRD_SECTION_THETA_MEAN ? "theta-mean" : "phi-mean";
}

// --section's argument: row:J, column:I, theta-mean or phi-mean.
inline void parse_section(const std::string &v, Options *o)
{
	if (v == "theta-mean") return (void)o->sections.emplace_back(CRD_SECTION_THETA_MEAN, 0);
	if (v == "phi-mean") return (void)o->sections.emplace_back(CRD_SECTION_PHI_MEAN, 0);
	const size_t colon = v.find(':');
	const std::string name = v.substr(0, colon), at = colon == std::string::npos ? "" : v.substr(colon + 1);
	const std::string refusal = "--section takes row:J, column:I, theta-mean or phi-mean (got '" + v + "')";
	const long long index = whole_number(at, refusal);
	if (name != "row" && name != "column") usage_error(refusal);
	o->sections.emplace_back(name == "row" ? CRD_SECTION_ROW : CRD_SECTION_COLUMN, index);
}

// What --ensemble cannot be combined with, what belongs to --observe, and lists of unequal length: refused before the ini is read or
// any device touched.  Every refusal is written once; a run with --ensemble and one without look at them in different orders, and of
// two faults the first in that order is the one reported.
inline void check_ensemble_options(const Options &o)
{
	const bool lone = o.ensemble.empty();
	auto belongs_to_observe = [&](bool given, const char *option) {
		if (given && !o.observe) usage_error(std::string(option) + " belongs to --observe" + (lone ? ", which needs --ensemble" : " STRIDE"));
	};
	auto stride = [&]() {
		if (o.observe && o.observe_stride < 1) usage_error("--observe takes a stride of at least 1 (got " + std::to_string(o.observe_stride) + ")");
	};
	auto sections_limit = [&]() {
		if ((int)o.sections.size() > CRD_OBSERVE_MAX_SECTIONS) usage_error("--section: at most " + std::to_string(CRD_OBSERVE_MAX_SECTIONS) + " sections");
	};
	auto probes_limit = [&]() {
		if ((int)o.probes.size() > CRD_OBSERVE_MAX_PROBES) usage_error("--probe: at most " + std::to_string(CRD_OBSERVE_MAX_PROBES) + " probes");
	};
	if (lone) {
		if (o.ensemble_steps) usage_error("--ensemble-steps sets an ensemble's steps per launch: it needs --ensemble");
		if (o.ensemble_own_dt) usage_error("--ensemble-own-dt steps an ensemble's members at their own step sizes: it needs --ensemble");
		belongs_to_observe(!o.probes.empty(), "--probe");
		belongs_to_observe(o.observe_maps, "--observe-maps");
		belongs_to_observe(!o.sections.empty(), "--section");
		belongs_to_observe(o.observe_cycles, "--observe-cycles");
		if (!o.observe) return;
		// --observe without --ensemble: the run recorder (crd_recorder_*) of a lone run or of its in-process slabs.  A bare --observe
		// STRIDE, naming nothing to record, keeps the refusal it has always had here (tests/test_observe_host.py pins it).
		if (o.probes.empty() && !o.observe_maps && o.sections.empty() && !o.observe_cycles)
			usage_error("--observe records an ensemble's members: it needs --ensemble (a run without one names what to record besides the statistics: --probe, --section, --observe-maps or "
			            "--observe-cycles)");
		stride();
		sections_limit();
		probes_limit();
		if (o.d0 > 0 || o.decomp_mpi) usage_error("--observe records phi-slabs: not with --decomp (2-D block files and contexts are not recorded)");
		if (o.block_contexts) usage_error("--observe records phi-slabs: not with --block-contexts");
		return;
	}
	belongs_to_observe(!o.sections.empty(), "--section");
	belongs_to_observe(o.observe_cycles, "--observe-cycles");
	sections_limit();
	belongs_to_observe(!o.probes.empty(), "--probe");
	belongs_to_observe(o.observe_maps, "--observe-maps");
	stride();
	probes_limit();
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

// What --imex cannot be combined with on the command line, looked at after everything above: a command line without --imex is refused as
// ever.  What the ini adds is check_imex_config's (crd_run.cpp).
inline void check_imex_options(const Options &o)
{
	if (o.imex < 0 && o.imex_solver >= 0) usage_error("--imex-solver chooses the linear solver of an IMEX run: only with --imex");
	if (o.imex_adaptive && o.imex != CRD_IMEX_ARS443) usage_error("--imex-adaptive controls the error of ARS(4,4,3), the one scheme with an embedded solution: only with --imex ars443");
	if (o.imex < 0) return;
	if (!o.ensemble.empty()) usage_error("--imex steps a lone single-slab run: not with --ensemble");
	if (o.gpus > 1) usage_error("--imex steps a lone single-slab run: not with --gpus " + std::to_string(o.gpus));
	if (o.d0 > 0 || o.decomp_mpi || o.block_contexts) usage_error("--imex steps a lone single-slab run: not with --decomp / --block-contexts");
	if (o.observe) usage_error("--imex takes no recorder samples: not with --observe");
	if (o.adaptive == 1 || o.adaptive == 2) usage_error("--imex steps at the run's fixed dt: not with --adaptive / --adaptive-rk43");
}

// The command line of an invocation as crd_run (an alias takes the ini alone: main).  --gpus, --devices and --dt take whatever atoi /
// atof make of their value.
inline void parse_options(int argc, char *argv[], Options *out)
{
	Options &o = *out;
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
		} else if (s == "--observe") {
			const std::string v = next();
			o.observe = true;
			o.observe_stride = whole_number(v, "--observe takes a stride, a whole number of steps (got '" + v + "')");
		} else if (s == "--probe") {
			const std::string v = next();
			long long i = 0, j = 0;
			int used = 0;
			if (std::sscanf(v.c_str(), "%lld,%lld%n", &i, &j, &used) != 2 || used != (int)v.size()) usage_error("--probe takes I,J, a grid point's theta and phi index (got '" + v + "')");
			o.probes.emplace_back(i, j);
		} else if (s == "--observe-maps") {
			const std::string v = next();
			o.observe_maps = true;
			o.observe_threshold = finite_number(v, "--observe-maps takes a threshold, a number (got '" + v + "')");
		} else if (s == "--section") {
			parse_section(next(), &o);
		} else if (s == "--observe-cycles") {
			const std::string v = next();
			o.observe_cycles = true;
			o.cycle_threshold = finite_number(v, "--observe-cycles takes a threshold, a number (got '" + v + "')");
		} else if (s == "--imex") {
			const std::string v = next();
			o.imex = v == "euler" ? CRD_IMEX_EULER : v == "ars222" ? CRD_IMEX_ARS222 : v == "ars443" ? CRD_IMEX_ARS443 : -1;
			if (o.imex < 0) usage_error("--imex takes euler, ars222 or ars443 (got '" + v + "')");
		} else if (s == "--imex-adaptive") {
			o.imex_adaptive = true;
		} else if (s == "--imex-solver") {
			const std::string v = next();
			o.imex_solver = v == "gmres" ? CRD_IMEX_SOLVER_GMRES : v == "bicgstab" ? CRD_IMEX_SOLVER_BICGSTAB : v == "bicgstab-warm" ? CRD_IMEX_SOLVER_BICGSTAB_WARM : -1;
			if (o.imex_solver < 0) usage_error("--imex-solver takes gmres, bicgstab or bicgstab-warm (got '" + v + "')");
		} else if (s == "--decomp") {
			const std::string v = next();
			if (v == "mpi") o.decomp_mpi = true;
			else if (std::sscanf(v.c_str(), "%dx%d", &o.d0, &o.d1) != 2 || o.d0 < 1 || o.d1 < 1) usage(argv[0], false);
		} else if (s == "--precision") {
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
	check_imex_options(o);
}

// --probe I,J and --section row:J | column:I against the grid they are recorded on; `of` names the member (" of member k") where the
// members' grids differ.  Refused before any device is asked for.
inline void check_probe(const std::pair<long long, long long> &q, const crd_grid &g, const std::string &of)
{
	if (q.first < 0 || q.first >= g.nx || q.second < 0 || q.second >= g.ny)
		usage_error("--probe " + std::to_string(q.first) + "," + std::to_string(q.second) + " is outside the " + std::to_string(g.nx) + " x " + std::to_string(g.ny) + " grid" + of);
}
inline void check_section(const std::pair<int, long long> &q, const crd_grid &g)
{
	if ((q.first == CRD_SECTION_ROW && (q.second < 0 || q.second >= g.ny)) || (q.first == CRD_SECTION_COLUMN && (q.second < 0 || q.second >= g.nx)))
		usage_error(std::string("--section ") + section_name(q.first) + ":" + std::to_string(q.second) + " is outside the " + std::to_string(g.nx) + " x " + std::to_string(g.ny) + " grid");
}

// Output cadence (src/FHNmodel_torus.cpp:415-429): Nt outputs dTout apart; every interval is an integer number of equal RK4 steps no
// longer than the step cap -- the ini's / --dt's step, else the smallest dtSafety x crd_stable_dt among the B members (a lone run: its
// one set of parameters), whose index goes to *cap_member (-1: the pinned step).
struct Cadence {
	int Nt;
	double dTout;
	int64_t steps_per_output;
	double dt;
};
inline Cadence output_cadence(const crd_run_config &cfg, const crd_params *members, int B, int *cap_member)
{
	Cadence c;
	c.Nt = cfg.output_timestep;
	c.dTout = cfg.t_final / c.Nt;
	double dt_cap = cfg.dt;
	int from = -1;
	if (!(dt_cap > 0))
		for (int k = 0; k < B; k++) {
			const double cap = cfg.dt_safety * crd_stable_dt(&members[k]);
			if (from < 0 || cap < dt_cap) dt_cap = cap, from = k;
		}
	if (cap_member) *cap_member = from;
	c.steps_per_output = (int64_t)std::ceil(c.dTout / dt_cap - 1e-12);
	c.dt = c.dTout / (double)c.steps_per_output;
	return c;
}

// What --observe and its companions ask of an observer or a recorder, and the room for its samples.  Fixed steps: every stride-th
// step of the run -- floor(total steps / stride), the count the library itself reaches, since its step count carries over the calls;
// one sample per output (error-controlled stepping, members at their own step sizes): Nt.
struct ObserveRequest {
	crd_observe_options options{};
	crd_observe_extras extras{};
	int64_t capacity = 0;
};
inline ObserveRequest observe_request(const Options &o, const Cadence &c, bool sample_per_output)
{
	ObserveRequest r;
	r.options.stride = o.observe_stride;
	r.options.n_probes = (int32_t)o.probes.size();
	for (size_t q = 0; q < o.probes.size(); q++) {
		r.options.probe_i[q] = (int32_t)o.probes[q].first;
		r.options.probe_j[q] = (int32_t)o.probes[q].second;
	}
	r.options.maps = o.observe_maps ? 1 : 0;
	r.options.threshold = o.observe_threshold;
	r.extras.n_sections = (int32_t)o.sections.size();
	for (size_t q = 0; q < o.sections.size(); q++) {
		r.extras.kind[q] = o.sections[q].first;
		r.extras.index[q] = (int32_t)o.sections[q].second;
	}
	r.extras.cycles = o.observe_cycles ? 1 : 0;
	r.extras.cycle_threshold = o.cycle_threshold;
	r.capacity = sample_per_output ? c.Nt : std::max<int64_t>(1, c.steps_per_output * c.Nt / o.observe_stride);
	return r;
}

// The driver's error-controlled stepping: one ARKode(...) call per output interval (src/FHNmodel_torus.cpp:423), [Solver] adaptive = 2
// the RK4(3) pair, which is handed the step its last call proposed (h_next); the ARKode-style controller keeps its own memory in
// the contexts / the ensemble, and its first step is arkHin.
inline crd_adaptive_options adaptive_options(const crd_run_config &cfg, double h_next)
{
	crd_adaptive_options ao;
	crd_adaptive_defaults(&ao);
	ao.rtol = cfg.rtol;
	ao.atol = cfg.atol;
	ao.method = cfg.adaptive == 2 ? CRD_ADAPT_RK43 : CRD_ADAPT_ARKODE;
	ao.h0 = cfg.adaptive == 2 ? h_next : 0.0;
	ao.dense_output = 1;  // ARK_NORMAL: output times do not shorten steps, the row written is the interpolant at tout
	return ao;
}

// --imex ars443 --imex-adaptive: one crd_integrate_imex call per output interval with the ini's rtol / atol, as --adaptive takes them;
// the first call's h0 is the run's dt where that is positive (0: crd_stable_dt), every later one the previous call's h_next.
inline crd_imex_adaptive_options imex_adaptive_options(const Options &o, const crd_run_config &cfg, double h_next)
{
	crd_imex_adaptive_options ao;
	crd_imex_adaptive_defaults(&ao);
	if (o.imex_solver >= 0) ao.imex.solver = o.imex_solver;
	ao.rtol = cfg.rtol;
	ao.atol = cfg.atol;
	ao.h0 = h_next > 0.0 ? h_next : (cfg.dt > 0.0 ? cfg.dt : 0.0);
	return ao;
}

#endif
