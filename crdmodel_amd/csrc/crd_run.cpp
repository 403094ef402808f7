// crd_run.cpp -- command-line driver with the reference's surface: `<program> <ini file>` writes the per-subdomain
// text files the reference's Python plotting / torus-mapping utilities read.  It replaces main() of the four
// reference programs (src/FHNmodel_torus.cpp:148-497 and siblings); invoked through one of the alias names
// FHNmodel_torus / FHNmodel_flat / GoldbeterModel_torus / GoldbeterModel_flat it takes exactly one argument, like
// they do.  Time integration is fixed-step RK4 on the GPU (libcrd) by default; --adaptive runs the reference's integrator,
// ARKode's default explicit pair and controller restated (CRD_ADAPT_ARKODE), --adaptive-rk43 the RK4(3) pair of earlier rounds,
// --imex euler|ars222|ars443 IMEX steps with the diffusion part implicit at the run's fixed dt (crd_step_imex; a lone single slab).
// --imex-solver gmres|bicgstab|bicgstab-warm  the linear solver of its stages (CRD_IMEX_SOLVER_*; only with --imex).
// --imex-adaptive  with --imex ars443: error-controlled steps from the ini's rtol / atol, output interval by output interval
//                  (crd_integrate_imex); a positive dt is the first step.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <filesystem>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "crd.h"
#include "crd_run_options.h"
#include "crd_run_output.h"

namespace {

void banner(const crd_run_config &cfg, const crd_grid &g, int n_slabs, int64_t nxl0, int64_t nyl0, double s0, double s1, double dt, int64_t steps_per_output, int imex, bool imex_adaptive)
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
	else if (imex_adaptive)
		std::cout << "   integrator = IMEX ARS(4,4,3) on GPU (diffusion implicit), embedded order 2, PID controller\n   rtol = " << cfg.rtol << "\n   atol = " << cfg.atol << "\n";
	else if (imex >= 0)
		std::cout << "   integrator = IMEX " << (imex == CRD_IMEX_EULER ? "Euler" : imex == CRD_IMEX_ARS222 ? "ARS(2,2,2)" : "ARS(4,4,3)") << " on GPU (diffusion implicit), dt = " << dt << " ("
		          << steps_per_output << " steps per output)\n";
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

// The ensemble's failures carry its own error text; one that a library status comes with, and one that refuses an option.
int ensemble_failed(const std::string &what, int rc, const crd_ensemble *ens)
{
	std::cerr << "\nCRD_ERROR: " << what << " failed with flag = " << rc << " (" << crd_status_string(rc) << "): " << crd_ensemble_last_error(ens) << "\n\n";
	return 1;
}
int ensemble_refused(const std::string &what, const crd_ensemble *ens)
{
	std::cerr << "\nCRD_ERROR: " << what << ": " << crd_ensemble_last_error(ens) << "\n\n";
	return 1;
}

// What --ensemble cannot be combined with in the ini.
void check_ensemble_config(const Options &o, const crd_run_config &cfg)
{
	if (cfg.adaptive == 2)
		usage_error("--ensemble integrates error-controlled with ARKode's pair only: the ini asks for [Solver] adaptive = 2 (RK4(3); pass --fixed, or set adaptive = 1)");
	const bool adaptive = cfg.adaptive == 1;
	if (adaptive && o.ensemble_steps)
		usage_error("--ensemble-steps sets the steps of a fixed-step launch: the ini asks for [Solver] adaptive = 1, which takes attempts, not steps (pass --fixed)");
	if (o.ensemble_own_dt && adaptive) usage_error("--ensemble-own-dt sets the steps of the fixed-step path: the ini asks for [Solver] adaptive = 1, where every member takes its own steps already (pass --fixed)");
	if (o.ensemble_own_dt && cfg.dt > 0) usage_error("--ensemble-own-dt gives every member its own step size: the ini pins [Solver] dt = " + std::to_string(cfg.dt) + " for all (set dt = 0)");
	if (cfg.n_gpus > 1) usage_error("--ensemble runs on one GPU: the ini asks for [Solver] gpus = " + std::to_string(cfg.n_gpus) + " (pass --gpus 1)");
}

// The members of an ensemble: the run of the ini once per member, the members' parameters zipped from the lists.
struct Members {
	int B = 0;
	std::vector<crd_run_config> cfg;
	std::vector<crd_params> params;
	std::vector<crd_grid> grid;
	bool geometry = false;       // a geometry key is among the lists: the members may differ in surface and grid (crd_ensemble_create_mixed)
	bool shapes_differ = false;  // ... and nx or ny truly differ
};
Members ensemble_members(const Options &o, const crd_run_config &cfg)
{
	Members m;
	m.B = (int)o.ensemble[0].second.size();
	m.cfg.assign((size_t)m.B, cfg);
	m.params.resize((size_t)m.B);
	m.grid.resize((size_t)m.B);
	for (int k = 0; k < m.B; k++) {
		for (const auto &kv : o.ensemble) set_ensemble_value(kv.first, kv.second[(size_t)k], &m.cfg[(size_t)k].params);
		m.params[(size_t)k] = m.cfg[(size_t)k].params;
	}
	for (const auto &kv : o.ensemble) m.geometry = m.geometry || ensemble_geometry_key(kv.first);
	for (int k = 0; k < m.B; k++) {
		if (crd_grid_from_params(&m.params[(size_t)k], &m.grid[(size_t)k]) != CRD_OK) usage_error("member " + std::to_string(k) + ": bad geometry");
		m.shapes_differ = m.shapes_differ || m.grid[(size_t)k].nx != m.grid[0].nx || m.grid[(size_t)k].ny != m.grid[0].ny;
	}
	return m;
}

// What an ensemble of different shapes refuses, and probes and sections outside the members' grids: refused here, before any device is
// asked for, by the option's name.
void check_members(const Options &o, const Members &m, bool adaptive)
{
	if (m.geometry && m.shapes_differ) {
		if (adaptive) usage_error("[Solver] adaptive = 1: members of different shape integrate with fixed steps only (pass --fixed)");
		if (!o.sections.empty()) usage_error("--section: members of different shape take no sections");
		if (o.observe_cycles) usage_error("--observe-cycles: members of different shape take no cycle maps");
	}
	if (!o.observe) return;
	for (const auto &q : o.probes)
		for (int k = 0; k < m.B; k++) check_probe(q, m.grid[(size_t)k], m.shapes_differ ? " of member " + std::to_string(k) : std::string());
	for (const auto &q : o.sections) check_section(q, m.grid[0]);
}

// What an ensemble run holds: released in this order -- the members' writers, then the ensemble -- whichever way the run ends.
struct EnsembleRun {
	crd_ensemble *ens = nullptr;
	std::vector<crd_writer *> wr;
	// --ensemble-own-dt: member k takes own_n[k] steps of dTout / own_n[k] per output, a lone run's count and step size for its ini.
	// The step sizes are handed over as formed here (crd_ensemble_step_rk4_own_dt): (t + dTout) - t need not be dTout.
	std::vector<int64_t> own_n;
	std::vector<double> own_step;
	std::vector<double> buf;  // the largest member's state; a member fills its own nx * ny pairs
	~EnsembleRun()
	{
		for (auto *w : wr) crd_writer_close(w);
		if (ens) crd_ensemble_destroy(ens);
	}
};

int create_ensemble(const Options &o, const crd_run_config &cfg, const Members &m, double dTout, EnsembleRun *run)
{
	const char *create = m.geometry ? "crd_ensemble_create_mixed" : "crd_ensemble_create";
	int rc = m.geometry ? crd_ensemble_create_mixed(m.params.data(), m.B, 0, &run->ens) : crd_ensemble_create(m.params.data(), m.B, 0, &run->ens);
	if (rc != CRD_OK) return ensemble_failed(create, rc, nullptr);
	if (o.ensemble_steps && (rc = crd_ensemble_set_steps_per_launch(run->ens, o.ensemble_steps)) != CRD_OK)
		return ensemble_refused("--ensemble-steps " + std::to_string(o.ensemble_steps), run->ens);
	run->own_n.assign((size_t)m.B, 0);
	run->own_step.assign((size_t)m.B, 0.0);
	if (o.ensemble_own_dt) {
		if ((rc = crd_ensemble_own_steps(run->ens, 0.0, dTout, cfg.dt_safety, run->own_n.data())) != CRD_OK) return ensemble_refused("--ensemble-own-dt", run->ens);
		for (int k = 0; k < m.B; k++) run->own_step[(size_t)k] = dTout / (double)run->own_n[(size_t)k];
	}
	return 0;
}

void ensemble_banner(const Options &o, const crd_run_config &cfg, const Members &m, const Cadence &c, int dt_member, const EnsembleRun &run)
{
	crd_grid g;
	crd_ensemble_info(run.ens, nullptr, &g);
	const crd_params &p0 = m.params[0];
	std::cout << "\nEnsemble of " << m.B << " members on one GPU (" << (p0.model == CRD_MODEL_FHN ? "FHN" : "Goldbeter") << ", "
	          << (m.geometry ? std::string("each member's own surface and grid") : std::string(p0.surface == CRD_SURFACE_TORUS ? "torus" : "flat surface") + ", nx = " + std::to_string(g.nx) + ", ny = " + std::to_string(g.ny)) << "):\n";
	for (int k = 0; k < m.B; k++) {
		std::cout << "   member " << k << ":";
		for (const auto &kv : o.ensemble) std::cout << " " << kv.first << " = " << kv.second[(size_t)k];
		if (m.geometry) std::cout << "  (" << m.grid[(size_t)k].nx << " x " << m.grid[(size_t)k].ny << ")";
		std::cout << "  -> " << o.outdir << "/member_" << k << "\n";
	}
	std::cout << "   Tfinal = " << cfg.t_final << ", output timesteps = " << c.Nt << "\n";
	if (cfg.adaptive == 1)
		std::cout << "   integrator = ARKode-style ERK on GPU (Zonneveld 5(3)4, PID controller), each member its own steps\n   rtol = " << cfg.rtol
		          << "\n   atol = " << cfg.atol << "\n";
	else if (o.ensemble_own_dt) {
		std::cout << "   integrator = classical RK4 on GPU, every member at its own dtSafety x stable dt (single steps, one launch per round)\n";
		for (int k = 0; k < m.B; k++) std::cout << "   member " << k << ": dt = " << run.own_step[(size_t)k] << " (" << run.own_n[(size_t)k] << " steps per output)\n";
	} else
		std::cout << "   integrator = classical RK4 on GPU, dt = " << c.dt << " (" << c.steps_per_output << " steps per output; "
		          << (dt_member < 0 ? std::string("from [Solver] dt / --dt") : "the smallest member's dtSafety x stable dt: member " + std::to_string(dt_member)) << ")\n"
		          << (crd_ensemble_get_steps_per_launch(run.ens) == 2 ? "   two steps per launch\n" : "");
}

// Member k writes the reference's files of a single-rank run into <outdir>/member_<k>/, from its own initial conditions.
int open_member_files(const Options &o, const Members &m, EnsembleRun *run)
{
	run->wr.assign((size_t)m.B, nullptr);
	int64_t most_points = 0;
	for (const crd_grid &kg : m.grid) most_points = std::max(most_points, kg.nx * kg.ny);
	run->buf.resize((size_t)(2 * most_points));
	for (int k = 0; k < m.B; k++) {
		const std::string dir = o.outdir + "/member_" + std::to_string(k);
		std::error_code ec;
		std::filesystem::create_directories(dir, ec);
		int rc = crd_initial_conditions(&m.cfg[(size_t)k], 0, m.grid[(size_t)k].ny - 1, run->buf.data());
		if (rc != CRD_OK) return die("crd_initial_conditions", rc, nullptr);
		if ((rc = crd_writer_open(&m.cfg[(size_t)k], dir.c_str(), 0, 1, &run->wr[(size_t)k])) != CRD_OK || (rc = crd_writer_write_row(run->wr[(size_t)k], run->buf.data())) != CRD_OK)
			return die("crd_writer", rc, nullptr);
		if ((rc = crd_ensemble_upload(run->ens, k, run->buf.data(), 1)) != CRD_OK) return ensemble_refused("crd_ensemble_upload failed", run->ens);
	}
	return 0;
}

// Which members have stopped, and what the stepping has cost.
struct EnsembleTally {
	std::vector<int> blown_at;   // output (1-based) at which a member went non-finite; 0: never
	std::vector<int> failed_at;  // ... at which its error-controlled integration failed
	std::vector<long long> accepted, rejected;
	double stepping_s = 0.0;
	explicit EnsembleTally(int B) : blown_at((size_t)B, 0), failed_at((size_t)B, 0), accepted((size_t)B, 0), rejected((size_t)B, 0) {}
};

// One output interval of every member: step (error-controlled, at own step sizes, or at the common one), then write the row of every
// member still running.  Returns the library's status.
int ensemble_interval(const Options &o, const crd_run_config &cfg, const Cadence &c, int iout, EnsembleRun *run, EnsembleTally *tally)
{
	crd_ensemble *ens = run->ens;
	const int B = (int)run->wr.size();
	const double t = iout * c.dTout, t_out = (iout + 1 == c.Nt) ? cfg.t_final : (iout + 1) * c.dTout;
	std::vector<double> peak((size_t)B);
	int rc;
	const auto step_t0 = std::chrono::steady_clock::now();
	if (cfg.adaptive == 1) {
		// one ARKode(...) call per output interval for every member, src/FHNmodel_torus.cpp:423 (a failed member still takes part in
		// later calls, from the state it was left at, but is written no further)
		const crd_adaptive_options ao = adaptive_options(cfg, 0.0);
		std::vector<crd_adaptive_stats> as((size_t)B);
		std::vector<int32_t> member_status((size_t)B);
		rc = crd_ensemble_integrate_adaptive(ens, t, t_out, &ao, as.data(), member_status.data());
		if (rc == CRD_ESTATE) {
			for (int k = 0; k < B; k++)
				if (member_status[(size_t)k] != CRD_OK && !tally->failed_at[(size_t)k] && !tally->blown_at[(size_t)k]) {
					tally->failed_at[(size_t)k] = iout + 1;
					std::cerr << "\nSolver failure, stopping integration of member " << k << " (" << crd_ensemble_last_error(ens) << ")\n";  // src/FHNmodel_torus.cpp:433
				}
			rc = CRD_OK;
		}
		for (int k = 0; k < B && rc == CRD_OK; k++)
			if (!tally->failed_at[(size_t)k] && !tally->blown_at[(size_t)k]) tally->accepted[(size_t)k] += as[(size_t)k].accepted, tally->rejected[(size_t)k] += as[(size_t)k].rejected;
	} else if (o.ensemble_own_dt) {
		// (the time given is the observer sample's alone: the output time as the error-controlled branch forms it)
		rc = crd_ensemble_step_rk4_own_dt(ens, t, t_out, run->own_step.data(), run->own_n.data());
	} else {
		rc = crd_ensemble_step_rk4(ens, t, c.dt, c.steps_per_output);
	}
	if (rc == CRD_OK) rc = crd_ensemble_synchronize(ens);
	tally->stepping_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - step_t0).count();
	if (rc == CRD_OK) rc = crd_ensemble_max_abs(ens, peak.data());
	for (int k = 0; k < B && rc == CRD_OK; k++) {
		if (tally->blown_at[(size_t)k] || tally->failed_at[(size_t)k]) continue;
		if (!std::isfinite(peak[(size_t)k])) {
			tally->blown_at[(size_t)k] = iout + 1;
			std::cerr << "\nSolver failure, stopping integration of member " << k << " (non-finite state at output " << iout + 1 << ")\n";  // src/FHNmodel_torus.cpp:433
			continue;
		}
		if ((rc = crd_ensemble_download(ens, k, run->buf.data(), 1)) == CRD_OK) rc = crd_writer_write_row(run->wr[(size_t)k], run->buf.data());
	}
	return rc;
}

// What --observe leaves in <outdir>/member_<k>/ (write_observations), every member's samples out of the ensemble's observer.
int write_member_observations(const Options &o, crd_ensemble *ens, int B)
{
	int64_t n = 0;
	int rc = crd_ensemble_observe_count(ens, &n);
	const size_t P = o.probes.size();
	std::vector<double> t((size_t)n), stats((size_t)n * (size_t)B * 8), pv((size_t)n * (size_t)B * P * 2);
	if (rc == CRD_OK) rc = crd_ensemble_observe_read(ens, 0, n, t.data(), stats.data(), pv.data());
	if (rc != CRD_OK) return rc;
	std::vector<std::vector<double>> all(o.sections.size());  // a section's [sample][member][length][2], read when the first member asks
	for (int k = 0; k < B; k++) {
		crd_grid g;  // the member's own
		if ((rc = crd_ensemble_member_grid(ens, k, &g)) != CRD_OK) return rc;
		ObservationSource from;
		from.section = [&](int q, int64_t *length, std::vector<double> *lines) -> int {  // the member's lines out of the section's
			int rs = crd_ensemble_observe_section_info(ens, q, nullptr, nullptr, length, nullptr);
			if (rs != CRD_OK) return rs;
			const size_t line = (size_t)*length * 2;
			std::vector<double> &every = all[(size_t)q];
			if (k == 0) {
				every.resize((size_t)n * (size_t)B * line);
				if ((rs = crd_ensemble_observe_read_section(ens, q, 0, n, every.data())) != CRD_OK) return rs;
			}
			lines->resize((size_t)n * line);
			for (size_t s = 0; s < (size_t)n; s++)
				std::copy(every.begin() + (ptrdiff_t)((s * (size_t)B + (size_t)k) * line), every.begin() + (ptrdiff_t)((s * (size_t)B + (size_t)k + 1) * line), lines->begin() + (ptrdiff_t)(s * line));
			return CRD_OK;
		};
		from.cycles = [&](int32_t *count, double *t_first, double *t_last) -> int { return crd_ensemble_observe_cycles(ens, k, count, t_first, t_last); };
		from.maps = [&](double *min_u, double *max_u, double *t_act) -> int { return crd_ensemble_observe_maps(ens, k, min_u, max_u, t_act); };
		const Samples mine = {n, t.data(), stats.data(), pv.data(), k, B};
		if ((rc = write_observations(o, o.outdir + "/member_" + std::to_string(k), g, mine, from)) != CRD_OK) return rc;
	}
	return CRD_OK;
}

// The members that stopped, by name (the run then exits 1), and the rate of the stepping.
int ensemble_summary(const Options &o, const crd_run_config &cfg, const Members &m, const Cadence &c, const EnsembleRun &run, const EnsembleTally &tally)
{
	const int B = m.B, Nt = c.Nt;
	const bool adaptive = cfg.adaptive == 1;
	int status = 0;
	for (int k = 0; k < B; k++)
		if (tally.blown_at[(size_t)k]) {
			std::cerr << "member " << k << " blew up at output " << tally.blown_at[(size_t)k] << " of " << Nt << "; its files stop there\n";
			status = 1;
		} else if (tally.failed_at[(size_t)k]) {
			std::cerr << "member " << k << " failed its error-controlled integration at output " << tally.failed_at[(size_t)k] << " of " << Nt << "; its files stop there\n";
			status = 1;
		}
	if (o.quiet) return status;
	if (adaptive) {
		std::cout << "\n";
		for (int k = 0; k < B; k++) std::cout << "   member " << k << ": steps = " << tally.accepted[(size_t)k] << " (+" << tally.rejected[(size_t)k] << " rejected)\n";
	}
	const double stepping_s = tally.stepping_s;
	if (!(stepping_s > 0.0)) return status;
	if (adaptive) {
		long long attempts = 0;
		for (int k = 0; k < B; k++) attempts += tally.accepted[(size_t)k] + tally.rejected[(size_t)k];
		std::printf("   rate: %d members, %lld attempts in %.6f s of stepping = %.1f attempts/s\n", B, attempts, stepping_s, (double)attempts / stepping_s);
	} else if (o.ensemble_own_dt) {
		double point_steps = 0.0;  // sum over the members of points x steps per output
		long long most = 0;
		for (int k = 0; k < B; k++) {
			point_steps += (double)m.grid[(size_t)k].nx * (double)m.grid[(size_t)k].ny * (double)run.own_n[(size_t)k];
			most = std::max(most, (long long)run.own_n[(size_t)k]);
		}
		std::printf("\n   rate: %d members at their own step sizes, %lld rounds in %.6f s of stepping = %.4g grid-point-steps/s\n", B, most * Nt, stepping_s, point_steps * Nt / stepping_s);
	} else {
		double points = 0.0;  // (every member's own grid: they may differ in shape)
		for (const crd_grid &kg : m.grid) points += (double)kg.nx * (double)kg.ny;
		const double ps = points * (double)c.steps_per_output * Nt / stepping_s;
		std::printf("\n   rate: %d members x %lld steps in %.6f s of stepping = %.4g grid-point-steps/s\n", B, (long long)c.steps_per_output * Nt, stepping_s, ps);
	}
	std::cout << "   ----------------------\n";
	return status;
}

// --ensemble: the run of the ini once per member, the members' parameters zipped from the lists, all stepped together on one GPU
// (crd_ensemble_*).  Member k writes the reference's files of a single-rank run into <outdir>/member_<k>/, from its own initial
// conditions.  Fixed steps: all members take one step size, the ini's / --dt's, else the smallest member's dtSafety x crd_stable_dt.
// [Solver] adaptive = 1 in the ini: error-controlled, one crd_ensemble_integrate_adaptive call per output (a lone adaptive run's
// crd_group_integrate_adaptive call), each member with its own step sequence.  A member whose state goes non-finite, or whose
// integrator fails, is written no further from that output on, as a lone run stops there; the others run to tFinal, and the run then
// exits 1 naming it.
int run_ensemble(const Options &o, const crd_run_config &cfg)
{
	check_ensemble_config(o, cfg);
	const bool adaptive = cfg.adaptive == 1;
	const Members m = ensemble_members(o, cfg);
	check_members(o, m, adaptive);
	int dt_member = -1;
	const Cadence c = output_cadence(cfg, m.params.data(), m.B, &dt_member);

	EnsembleRun run;
	if (create_ensemble(o, cfg, m, c.dTout, &run)) return 1;
	if (!o.quiet) ensemble_banner(o, cfg, m, c, dt_member, run);
	if (open_member_files(o, m, &run)) return 1;
	int rc;
	if (o.observe) {
		const ObserveRequest r = observe_request(o, c, adaptive || o.ensemble_own_dt);
		const bool extras = r.extras.n_sections > 0 || r.extras.cycles;
		rc = extras ? crd_ensemble_observe_begin_with(run.ens, &r.options, &r.extras, r.capacity) : crd_ensemble_observe_begin(run.ens, &r.options, r.capacity);
		if (rc != CRD_OK) return ensemble_failed("crd_ensemble_observe_begin", rc, run.ens);
	}
	EnsembleTally tally(m.B);
	for (int iout = 0; iout < c.Nt; iout++) {
		if ((rc = ensemble_interval(o, cfg, c, iout, &run, &tally)) != CRD_OK) return ensemble_failed("ensemble stepping / output", rc, run.ens);
		if (!o.quiet) {
			std::printf("%s   %3d %%", iout > 0 ? "\r" : "", 100 * (iout + 1) / c.Nt);
			std::fflush(stdout);
		}
	}
	if (o.observe && (rc = write_member_observations(o, run.ens, m.B)) != CRD_OK) return ensemble_failed("writing the observations", rc, run.ens);
	return ensemble_summary(o, cfg, m, c, run, tally);
}

// What a lone run or its in-process slabs hold.  Released in this order whichever way the run ends: the writer thread is joined before
// anything it reads goes, then the text writers, the .npy writers, the page-locked frames and the contexts.
struct LoneRun {
	// Two decompositions.  FILES: phi-slabs (1 x gpus) unless the reference's own 2-D blocks are asked for -- `--decomp 2x2`, or
	// `--decomp mpi` = what MPI_Dims_create makes of the slab count (src/FHNmodel_torus.cpp:724-728: `mpirun -np 4` is 2 x 2): the file
	// sets, subdomain headers and (for the rand() rule) initial conditions of that process grid.  COMPUTE: phi-slabs, one per GPU (the
	// layout for one node, and the one the one-launch stepper, the error-controlled integrators and the deep halo need) -- also
	// under --decomp (round 4): the blocks' rows are cut out of the slabs' frames at output time; `--block-contexts` computes on
	// the 2-D blocks themselves instead (staged kernels, fixed step, text files), bit-equal to the whole domain's staged run.
	int fd0 = 1, fd1 = 1;  // the files' process grid
	int d0 = 1, d1 = 1;    // the contexts' decomposition
	int F = 1, G = 1;
	bool recut = false;  // files in a layout the contexts do not have
	std::vector<crd_ctx *> ctx;
	std::vector<crd_writer *> wr;
	std::vector<Rect> frect, crect;
	// Two host copies of every slab: while the writer thread formats output k from one, the GPU integrates towards
	// output k+1 and downloads into the other (text output of a large grid costs more than the steps between outputs).
	std::vector<std::vector<double>> host, host_b;
	// recut: the frames of the F file blocks, cut out of the G slabs' frames (two sets, like the slabs' own)
	std::vector<std::vector<double>> fhost, fhost_b;
	// Binary side-channel: the owned rows of a field plane ARE the (nyl, nxl) frame of the .npy file, so a frame is one
	// device-to-host copy into page-locked memory (two sets: one being written to disk, one being filled) -- no layout change,
	// no formatting.  [slab][var][set]
	int nvars_out = 1;
	size_t value_bytes = 8;
	std::vector<crd_npy_writer *> npy;
	std::vector<void *> frame;
	std::thread writer;
	int writer_rc = CRD_OK;
	crd_recorder *rec = nullptr;  // (closed by crd_destroy of its contexts)
	~LoneRun()
	{
		if (writer.joinable()) writer.join();
		for (auto *w : wr) crd_writer_close(w);
		for (auto *w : npy) crd_npy_writer_close(w);
		for (void *f : frame) crd_host_free(f);
		for (auto *c : ctx) crd_destroy(c);
	}
};

// The steps of a lone run return its exit status: 0, or 1 with the reason on stderr.
int decompose(const Options &o, const crd_run_config &cfg, LoneRun *run)
{
	run->fd1 = cfg.n_gpus;
	if (o.decomp_mpi) crd_dims_create(cfg.n_gpus, &run->fd0, &run->fd1);
	else if (o.d0 > 0) {
		run->fd0 = o.d0;
		run->fd1 = o.d1;
	}
	run->F = run->fd0 * run->fd1;
	run->recut = run->fd0 > 1 && !o.block_contexts;
	run->d0 = run->recut ? 1 : run->fd0;
	run->d1 = run->recut ? cfg.n_gpus : run->fd1;
	run->G = run->d0 * run->d1;
	if (run->fd0 > 1 && o.binary) {
		std::cerr << "\nCRD_ERROR: the .npy side-channel holds phi-slab frames: not available with theta-blocks (--decomp with more than one theta-block)\n\n";
		return 1;
	}
	if (run->d0 > 1 && cfg.adaptive) {
		std::cerr << "\nCRD_ERROR: theta-block contexts (--block-contexts) step with the fixed-step staged RK4 and write text files only\n\n";
		return 1;
	}
	const size_t F = (size_t)run->F, G = (size_t)run->G;
	run->ctx.assign(G, nullptr);
	run->wr.assign(F, nullptr);
	run->frect.resize(F);
	run->crect.resize(G);
	run->host.resize(G);
	run->host_b.resize(G);
	run->fhost.resize(run->recut ? F : 0);
	run->fhost_b.resize(run->recut ? F : 0);
	run->nvars_out = 1 + (cfg.include_all_vars == 1 ? 1 : 0);
	run->value_bytes = cfg.params.precision == CRD_PRECISION_F64 ? 8 : 4;
	run->npy.assign(2 * G, nullptr);
	run->frame.assign(4 * G, nullptr);
	return 0;
}

int create_contexts(const crd_run_config &cfg, int ndev, LoneRun *run)
{
	const int G = run->G, d0 = run->d0, d1 = run->d1;
	int rc;
	for (int k = 0; k < G; k++) {
		if ((rc = crd_create_block(&cfg.params, k / d1, d0, k % d1, d1, k % ndev, &run->ctx[(size_t)k])) != CRD_OK) return die("crd_create", rc, nullptr);
		crd_set_stepper(run->ctx[(size_t)k], cfg.stepper);
	}
	if ((rc = crd_comm_attach_local(run->ctx.data(), G)) != CRD_OK) return die("crd_comm_attach_local", rc, run->ctx[0]);
	if (G > 1 && d0 == 1 && cfg.exchange_period) {
		// exchange period of the one-launch stepper: the ini's; without one the contexts keep what crd_create chose (10 steps where every
		// slab has 256 rows or more, else 8: include/crd.h, crd_set_exchange_period)
		for (int k = 0; k < G; k++)
			if ((rc = crd_set_exchange_period(run->ctx[(size_t)k], cfg.exchange_period)) != CRD_OK) return die("crd_set_exchange_period", rc, run->ctx[(size_t)k]);
	}
	for (int k = 0; k < G; k++) crd_get_block(run->ctx[(size_t)k], &run->crect[(size_t)k].is, &run->crect[(size_t)k].ie, &run->crect[(size_t)k].js, &run->crect[(size_t)k].je);
	return 0;
}

// Initial conditions, subdomain files, first output row (src/FHNmodel_torus.cpp:285-354,376-410).  The initial conditions are
// those of the FILES' process grid (the rand() rule draws block by block, as every reference rank does); recut: the blocks'
// frames are then laid into the slabs' for the upload.
int open_files(const Options &o, const crd_run_config &cfg, const crd_grid &g, LoneRun *run)
{
	for (int k = 0; k < run->G; k++) {
		const Rect &c = run->crect[(size_t)k];
		run->host[(size_t)k].resize((size_t)(2 * (c.ie - c.is + 1) * (c.je - c.js + 1)));
		run->host_b[(size_t)k].resize(run->host[(size_t)k].size());
	}
	for (int f = 0; f < run->F; f++) {
		const Rect &b = run->frect[(size_t)f];
		std::vector<double> &ic = run->recut ? run->fhost[(size_t)f] : run->host[(size_t)f];
		if (run->recut) {
			run->fhost[(size_t)f].resize((size_t)(2 * (b.ie - b.is + 1) * (b.je - b.js + 1)));
			run->fhost_b[(size_t)f].resize(run->fhost[(size_t)f].size());
		}
		int rc = crd_initial_conditions_block(&cfg, b.is, b.ie, b.js, b.je, ic.data());
		if (rc != CRD_OK) return die("crd_initial_conditions", rc, nullptr);
		if ((rc = crd_writer_open_block(&cfg, o.outdir.c_str(), f, f / run->fd1, run->fd0, f % run->fd1, run->fd1, &run->wr[(size_t)f])) != CRD_OK ||
		    (!o.binary_only && (rc = crd_writer_write_row(run->wr[(size_t)f], ic.data())) != CRD_OK))
			return die("crd_writer", rc, nullptr);
	}
	if (run->recut) recut_frames(run->crect, run->frect, g.nx, run->host, run->fhost, false);
	return 0;
}

// The state onto the devices; --binary: the .npy files and their page-locked frames, and the initial state as their first frame.
int upload(const Options &o, const crd_run_config &cfg, const crd_grid &g, LoneRun *run)
{
	for (int k = 0; k < run->G; k++) {
		crd_ctx *ctx = run->ctx[(size_t)k];
		const int64_t rows = run->crect[(size_t)k].je - run->crect[(size_t)k].js + 1;
		int rc = crd_state_upload(ctx, run->host[(size_t)k].data(), 1);
		if (rc != CRD_OK) return die("crd_state_upload", rc, ctx);
		if (!o.binary) continue;
		const size_t frame_bytes = (size_t)(g.nx * rows) * run->value_bytes;
		for (int v = 0; v < run->nvars_out && rc == CRD_OK; v++) {
			crd_npy_writer *&npy = run->npy[(size_t)(2 * k + v)];
			void **frame = &run->frame[(size_t)(4 * k + 2 * v)];  // the variable's two sets
			rc = crd_npy_writer_open(&cfg, o.outdir.c_str(), k, run->G, v, (int)run->value_bytes, &npy);
			for (int set = 0; set < 2 && rc == CRD_OK; set++)
				if (!(frame[set] = crd_host_alloc(frame_bytes))) rc = CRD_ENOMEM;
			if (rc == CRD_OK) rc = crd_state_download_rows(ctx, v, 0, rows, frame[0]);
			if (rc == CRD_OK) rc = crd_npy_writer_append(npy, frame[0]);  // the initial state
		}
		if (rc != CRD_OK) return die("crd_npy_writer", rc, ctx);
	}
	return 0;
}

// The one-launch stepper measures its launch plan on a context's first full-size step (~0.7 s at 8192^2): done here, ahead of the
// first output interval, so that the rate line below is the stepping's and nothing else's.  (The error-controlled integrators
// measure theirs inside their first attempt.)
int plan_launches(const Options &o, LoneRun *run)
{
	const auto plan_t0 = std::chrono::steady_clock::now();
	for (crd_ctx *ctx : run->ctx) {
		const int rc = crd_plan_launches(ctx);
		if (rc != CRD_OK) return die("crd_plan_launches", rc, ctx);
	}
	const double plan_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - plan_t0).count();
	crd_launch_plan lp;
	if (!o.quiet && crd_get_launch_plan(run->ctx[0], &lp) == CRD_OK && lp.tuned)
		std::printf("   launch plan (measured in %.2f s): chunk mode %d, XCD mapping %d, %d column(s) per lane, %s stores, %d step(s) per launch\n", plan_s, lp.one_round,
		            lp.xcd_mapping, lp.columns_per_lane, lp.nontemporal_stores ? "non-temporal" : "plain", lp.steps_per_launch);
	return 0;
}

// What the stepping has taken and cost.  Rate summary ("keep banner; add steps/s, point-steps/s, GB/s"): wall time
// spent inside the stepping calls (they block on the download that follows, so the device work of an interval is inside its bracket)
// and the steps taken.
struct LoneTally {
	double adaptive_h = 0.0;  // the step the RK4(3) controller proposed last
	long long adaptive_steps = 0, adaptive_rejected = 0;
	double stepping_s = 0.0;
	long long steps_taken = 0;
	long long imex_solves = 0, imex_iterations = 0;  // --imex: linear solves and their GMRES iterations
};

// Step all contexts over output interval iout and wait for them.  Returns the library's status.
int step_interval(const Options &o, const crd_run_config &cfg, const Cadence &c, int iout, LoneRun *run, LoneTally *tally)
{
	const double t = iout * c.dTout;
	const auto step_t0 = std::chrono::steady_clock::now();
	int rc;
	if (cfg.adaptive) {
		const crd_adaptive_options ao = adaptive_options(cfg, tally->adaptive_h);
		crd_adaptive_stats as;
		rc = crd_group_integrate_adaptive(run->ctx.data(), run->G, t, (iout + 1 == c.Nt) ? cfg.t_final : (iout + 1) * c.dTout, &ao, &as);
		tally->adaptive_h = as.h_next;
		tally->adaptive_steps += as.accepted;
		tally->adaptive_rejected += as.rejected;
		tally->steps_taken += as.accepted + as.rejected;
	} else if (o.imex_adaptive) {
		const crd_imex_adaptive_options ao = imex_adaptive_options(o, cfg, tally->adaptive_h);
		crd_imex_adaptive_stats as{};
		rc = crd_integrate_imex(run->ctx[0], t, (iout + 1 == c.Nt) ? cfg.t_final : (iout + 1) * c.dTout, &ao, &as, nullptr, 0);
		tally->adaptive_h = as.h_next;
		tally->adaptive_steps += as.accepted;
		tally->adaptive_rejected += as.rejected;
		tally->steps_taken += as.attempts;
		tally->imex_solves += as.imex.solves;
		tally->imex_iterations += as.imex.iterations;
	} else if (o.imex >= 0) {
		crd_imex_options io;
		crd_imex_defaults(&io);
		io.scheme = o.imex;
		if (o.imex_solver >= 0) io.solver = o.imex_solver;
		crd_imex_stats is{};
		rc = crd_step_imex(run->ctx[0], t, c.dt, c.steps_per_output, &io, &is);
		tally->steps_taken += is.steps;
		tally->imex_solves += is.solves;
		tally->imex_iterations += is.iterations;
	} else {
		rc = crd_group_step_rk4(run->ctx.data(), run->G, t, c.dt, c.steps_per_output);
		tally->steps_taken += c.steps_per_output;
	}
	for (int k = 0; k < run->G && rc == CRD_OK; k++) rc = crd_synchronize(run->ctx[(size_t)k]);
	tally->stepping_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - step_t0).count();
	return rc;
}

// Output iout off the devices, into the sets of host frames the writer thread is not reading (the others may still be in its hands),
// and whether any slab has blown up.  Passes a failed status through.
int download_interval(const Options &o, int iout, int rc, LoneRun *run, bool *blown)
{
	auto &buf = (iout & 1) ? run->host_b : run->host;
	const int set = (iout + 1) & 1;
	for (int k = 0; k < run->G && rc == CRD_OK; k++) {
		if (!o.binary_only) rc = crd_state_download(run->ctx[(size_t)k], buf[(size_t)k].data(), 1);
		int64_t js, je;
		crd_get_slab(run->ctx[(size_t)k], &js, &je);
		for (int v = 0; o.binary && v < run->nvars_out && rc == CRD_OK; v++)
			rc = crd_state_download_rows(run->ctx[(size_t)k], v, 0, je - js + 1, run->frame[(size_t)(4 * k + 2 * v + set)]);
	}
	// the reference stops at the first failing ARKode call on ANY rank (src/FHNmodel_torus.cpp:424-435): look at every slab
	*blown = false;  // sticky: a NaN / Inf on ANY slab stops the run, whatever the later slabs hold
	for (int k = 0; k < run->G && rc == CRD_OK; k++) {
		double pk = 0;
		rc = crd_state_max_abs(run->ctx[(size_t)k], &pk);
		*blown = *blown || !std::isfinite(pk);
	}
	return rc;
}

// The writer thread's work: output iout from the sets download_interval filled, formatted while the GPU steps on.
void write_output(LoneRun *run, const Options *o, int64_t nx, int iout)
{
	auto &buf = (iout & 1) ? run->host_b : run->host;
	auto &fbuf = (iout & 1) ? run->fhost_b : run->fhost;
	const int set = (iout + 1) & 1;
	int &rc = run->writer_rc;
	for (int k = 0; k < run->G && rc == CRD_OK; k++)
		for (int v = 0; o->binary && v < run->nvars_out && rc == CRD_OK; v++)
			rc = crd_npy_writer_append(run->npy[(size_t)(2 * k + v)], run->frame[(size_t)(4 * k + 2 * v + set)]);
	if (run->recut && !o->binary_only) recut_frames(run->crect, run->frect, nx, buf, fbuf, true);  // the file blocks' frames out of the slabs' (on the writer's time)
	for (int f = 0; f < run->F && !o->binary_only && rc == CRD_OK; f++)
		rc = crd_writer_write_row(run->wr[(size_t)f], (run->recut ? fbuf : buf)[(size_t)f].data());
}

// progress line, src/FHNmodel_torus.cpp:457-477
struct Progress {
	time_t start_t = 0;
	double total_t = 0;
};
void progress_line(const Options &o, int iout, int Nt, Progress *p)
{
	time_t end_t = 0;
	time(&end_t);
	p->total_t += difftime(end_t, p->start_t);
	p->start_t = end_t;
	const double total_t = p->total_t, eta = (Nt - (iout + 1)) * (total_t / (iout + 1));
	if (o.quiet) return;
	if (iout > 0) std::printf("\r");
	std::printf("   %3d %% | %3d min %2d sec elapsed | %3d min %2d sec remaining", 100 * (iout + 1) / Nt, (int)(total_t / 60), ((int)total_t % 60), (int)(eta / 60),
	            ((int)eta % 60));
	std::fflush(stdout);
}

// One output: step an interval, download, check for blow-up, hand the frames to the writer thread, print the progress line.  Returns
// whether the run goes on; where it does not, *status is 1 and the reason is on stderr.
bool output_interval(const Options &o, const crd_run_config &cfg, const crd_grid &g, const Cadence &c, int iout, LoneRun *run, LoneTally *tally, Progress *progress, int *status)
{
	bool blown = false;
	int rc = step_interval(o, cfg, c, iout, run, tally);
	rc = download_interval(o, iout, rc, run, &blown);
	if (rc != CRD_OK || blown) {
		if (rc != CRD_OK) die(o.imex_adaptive ? "crd_integrate_imex" : o.imex >= 0 ? "crd_step_imex" : "crd_group_step_rk4", rc, run->ctx[0]);
		std::cerr << "Solver failure, stopping integration\n";  // src/FHNmodel_torus.cpp:433
		*status = 1;
		return false;
	}
	if (run->writer.joinable()) run->writer.join();
	if (run->writer_rc != CRD_OK) {
		*status = die("crd_writer_write_row", run->writer_rc, nullptr);
		return false;
	}
	run->writer = std::thread(write_output, run, &o, g.nx, iout);
	progress_line(o, iout, c.Nt, progress);
	return true;
}

// What --observe leaves in <outdir> itself for a run without --ensemble: the files a member's directory gets (write_observations), read
// from the run recorder (crd_recorder_*) -- whole-grid planes whatever the number of slabs.
int write_recording(const Options &o, crd_recorder *rec, const crd_grid &g)
{
	int64_t n = 0;
	int rc = crd_recorder_count(rec, &n);
	const size_t P = o.probes.size();
	std::vector<double> t((size_t)n), stats((size_t)n * 8), pv((size_t)n * P * 2);
	if (rc == CRD_OK) rc = crd_recorder_read(rec, 0, n, t.data(), stats.data(), pv.data());
	if (rc != CRD_OK) return rc;
	ObservationSource from;
	from.section = [&](int q, int64_t *length, std::vector<double> *lines) -> int {
		const int rs = crd_recorder_section_info(rec, q, nullptr, nullptr, length, nullptr);
		if (rs != CRD_OK) return rs;
		lines->resize((size_t)n * (size_t)*length * 2);
		return n > 0 ? crd_recorder_read_section(rec, q, 0, n, lines->data()) : CRD_OK;
	};
	from.cycles = [&](int32_t *count, double *t_first, double *t_last) -> int { return crd_recorder_cycles(rec, count, t_first, t_last); };
	from.maps = [&](double *min_u, double *max_u, double *t_act) -> int { return crd_recorder_maps(rec, min_u, max_u, t_act); };
	return write_observations(o, o.outdir, g, Samples{n, t.data(), stats.data(), pv.data(), 0, 1}, from);
}

void rate_summary(const Options &o, const crd_run_config &cfg, const crd_grid &g, const LoneRun &run, const LoneTally &tally)
{
	if (o.quiet) return;
	const long long steps_taken = tally.steps_taken;
	const double stepping_s = tally.stepping_s;
	if (cfg.adaptive || o.imex_adaptive) std::cout << "\n   steps = " << tally.adaptive_steps << " (+" << tally.adaptive_rejected << " rejected)";
	if (o.imex >= 0 && steps_taken > 0 && stepping_s > 0.0) {
		char line[256];
		std::snprintf(line, sizeof line, "\n   rate: %lld IMEX steps in %.6f s of stepping = %.1f steps/s; %lld linear solves, %lld %s iterations", steps_taken, stepping_s,
		              (double)steps_taken / stepping_s, tally.imex_solves, tally.imex_iterations, o.imex_solver > CRD_IMEX_SOLVER_GMRES ? "BiCGStab" : "GMRES");
		std::cout << line;
	} else if (steps_taken > 0 && stepping_s > 0.0) {
		// compulsory-byte model of a step: both fields read once and written once (the one-launch stepper's traffic; the four
		// stage kernels move 8 x that)
		crd_launch_plan lp{};
		const bool pairs = !cfg.adaptive && crd_get_launch_plan(run.ctx[0], &lp) == CRD_OK && lp.tuned && lp.steps_per_launch == 2;
		const double points = (double)g.nx * (double)g.ny, bytes_per_point_step = 4.0 * (double)run.value_bytes / (pairs ? 2.0 : 1.0);  // (two steps per launch: the state crosses memory once per two)
		char line[256];
		std::snprintf(line, sizeof line, "\n   rate: %lld steps in %.6f s of stepping = %.1f steps/s, %.4g grid-point-steps/s, %.1f GB/s (%g B per point-step)",
		              steps_taken, stepping_s, (double)steps_taken / stepping_s, points * (double)steps_taken / stepping_s,
		              points * (double)steps_taken * bytes_per_point_step / stepping_s / 1e9, bytes_per_point_step);
		std::cout << line;
	}
	std::cout << "\n   ----------------------\n";
}

// What --imex cannot be combined with in the ini, and the fixed step it needs: refused before any device is touched.
void check_imex_config(const Options &o, const crd_run_config &cfg)
{
	if (o.imex < 0) return;
	if (cfg.n_gpus > 1) usage_error("--imex steps a lone single-slab run: the ini asks for [Solver] gpus = " + std::to_string(cfg.n_gpus) + " (pass --gpus 1)");
	if (cfg.adaptive) usage_error("--imex steps at the run's fixed dt: the ini asks for [Solver] adaptive = " + std::to_string(cfg.adaptive) + " (pass --fixed)");
	if (!(cfg.dt > 0) && !o.imex_adaptive)
		usage_error("--imex needs the run's fixed step: give --dt DT or a positive [Solver] dt (dt = 0 asks for dtSafety x the stable step of RK4, which is what an IMEX run is there to exceed)");
}

// A lone run, or its phi-slabs (or theta x phi blocks) stepped together in this process.
int run_lone(const Options &o, const crd_run_config &cfg)
{
	Progress progress;
	time(&progress.start_t);
	crd_grid g;
	int rc;
	if ((rc = crd_grid_from_params(&cfg.params, &g)) != CRD_OK) return die("crd_grid_from_params", rc, nullptr);
	LoneRun run;
	if (decompose(o, cfg, &run)) return 1;
	const int ndev = o.devices > 0 ? o.devices : run.G;
	if (o.observe) {  // (refused before any device is asked for)
		for (const auto &q : o.probes) check_probe(q, g, "");
		for (const auto &q : o.sections) {
			check_section(q, g);
			if (q.first == CRD_SECTION_PHI_MEAN && run.G > 1)
				usage_error("--section phi-mean is not recorded on more than one slab (a column's sum crosses the slabs): this run has " + std::to_string(run.G) + " (pass --gpus 1)");
		}
	}
	double s0 = 0, s1 = 0;  // banner only, and only printed for a constant beta (src/FHNmodel_torus.cpp:268-271)
	if (cfg.params.vary_beta == 0 && (rc = crd_steady_state_as_printed(cfg.params.model, cfg.params.beta, cfg.steady_state_decimals, &s0, &s1)) != CRD_OK)
		return die("crd_steady_state", rc, nullptr);
	const Cadence c = output_cadence(cfg, &cfg.params, 1, nullptr);

	if (create_contexts(cfg, ndev, &run)) return 1;
	for (int f = 0; f < run.F; f++) {
		Rect &b = run.frect[(size_t)f];
		if (run.recut) crd_block_extents(g.nx, g.ny, f / run.fd1, run.fd0, f % run.fd1, run.fd1, &b.is, &b.ie, &b.js, &b.je);
		else b = run.crect[(size_t)f];
	}
	if (!o.quiet) banner(cfg, g, run.F, run.frect[0].ie - run.frect[0].is + 1, run.frect[0].je - run.frect[0].js + 1, s0, s1, c.dt, c.steps_per_output, o.imex, o.imex_adaptive);
	if (open_files(o, cfg, g, &run) || upload(o, cfg, g, &run)) return 1;
	if (!cfg.adaptive && o.imex < 0 && plan_launches(o, &run)) return 1;
	if (o.observe) {
		// fixed steps: every stride-th step of the run; error-controlled: one sample per output
		const ObserveRequest r = observe_request(o, c, cfg.adaptive != 0);
		if ((rc = crd_recorder_open(run.ctx.data(), run.G, &r.options, &r.extras, r.capacity, &run.rec)) != CRD_OK) return die("crd_recorder_open", rc, run.ctx[0]);
	}

	int status = 0;
	LoneTally tally;
	for (int iout = 0; iout < c.Nt; iout++) {
		char range_name[64];
		std::snprintf(range_name, sizeof range_name, "crd_run output interval %d/%d", iout + 1, c.Nt);
		crd_trace_range_push(range_name);
		const bool goes_on = output_interval(o, cfg, g, c, iout, &run, &tally, &progress, &status);
		crd_trace_range_pop();
		if (!goes_on) break;
	}
	if (run.writer.joinable()) run.writer.join();
	if (run.writer_rc != CRD_OK && status == 0) status = die("crd_writer_write_row", run.writer_rc, nullptr);
	if (run.rec && (rc = write_recording(o, run.rec, g)) != CRD_OK && status == 0) status = die("writing the recording", rc, run.ctx[0]);
	rate_summary(o, cfg, g, run, tally);
	return status;
}

// Rank and size an MPI launcher gave this process through its environment (no MPI library is linked).
struct Launcher {
	int rank = 0, size = 1;
	const char *kind = "";
};
Launcher detect_launcher()
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

// The ini, with what the command line and the launcher override in it.
int load_config(Options *o, const Launcher &launcher, crd_run_config *cfg)
{
	char err[512];
	if (crd_config_load_ini(o->ini.c_str(), o->model, o->surface, cfg, err, sizeof err) != CRD_OK) {
		std::cerr << "\nCRD_ERROR: cannot use " << o->ini << ": " << err << "\n\n";
		return 1;
	}
	if (o->gpus > 0) cfg->n_gpus = o->gpus;
	else if (launcher.size > 1 && cfg->n_gpus == 1) {
		cfg->n_gpus = launcher.size;
		if (o->devices <= 0) o->devices = std::max(1, std::min(launcher.size, crd_device_count()));
		if (!o->quiet)
			std::cout << "\n" << launcher.kind << " started " << launcher.size << " ranks: rank 0 drives " << launcher.size << " phi-slabs on " << o->devices
			          << " GPU(s), the other ranks exit\n";
	}
	if (o->dt > 0) cfg->dt = o->dt;
	if (o->stepper >= 0) cfg->stepper = o->stepper;
	if (o->precision >= 0) cfg->params.precision = o->precision;
	if (o->adaptive >= 0) cfg->adaptive = o->adaptive;
	if (o->ref_steady_state) cfg->steady_state_decimals = 8;  // numpy's print precision, util/GoldbeterModel/SolveGoldbeterODE.py:111
	return 0;
}

}  // namespace

int main(int argc, char *argv[])
{
	Options o;
	std::string base = argv[0];
	const size_t slash = base.find_last_of('/');
	if (slash != std::string::npos) base = base.substr(slash + 1);
	if (!preset_from_name(base, &o)) parse_options(argc, argv, &o);
	else if (argc != 2) usage(argv[0], true);  // src/FHNmodel_torus.cpp:151-155
	else o.ini = argv[1];

	// Started by an MPI launcher the way the reference is (`mpirun -np N <exe> <ini>`, util/ShellScripts/run*.sh)?  This
	// program needs one process only: rank 0 drives N phi-slabs, one per GPU, and writes the N subdomain file sets the N
	// reference ranks would; the other ranks have nothing to do.
	const Launcher launcher = detect_launcher();
	if (launcher.size > 1 && launcher.rank != 0) return 0;

	crd_run_config cfg;
	if (load_config(&o, launcher, &cfg)) return 1;
	check_imex_config(o, cfg);
	return o.ensemble.empty() ? run_lone(o, cfg) : run_ensemble(o, cfg);
}
