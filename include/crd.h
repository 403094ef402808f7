/*
 * crd.h -- C ABI of libcrd: the MI355X-native replacement for CRDModel's per-timestep RHS path.
 *
 * Everything here is plain C: POD structs, pointers and sizes, `int` status returns (0 = ok, negative =
 * crd_status), no exceptions cross the boundary, no torch/HIP types in any signature.  Each entry point names
 * the reference interface it replaces (paths under the reference tree, e.g. src/FHNmodel_torus.cpp).
 *
 * Field layout at the boundary is the reference's own: state vectors are AoS pairs [var0, var1] per grid point,
 * theta / x (index i) fastest, IDX(i,j) = 2 i + 2 j nxl (src/FHNmodel_torus.cpp:60); var0 is the diffusing
 * variable (FHN u, Goldbeter Z), var1 the local one (FHN v, Goldbeter Y).  A context owns one phi-slab
 * [js, je] x [0, nx-1] of the global grid (the reference's subdomain with dims = {1, G}).
 */
#ifndef CRD_H
#define CRD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRD_ABI_VERSION 8

typedef enum crd_status {
	CRD_OK = 0,
	CRD_EINVAL = -1,   /* bad argument / inconsistent parameters */
	CRD_ENOMEM = -2,   /* host or device allocation failed */
	CRD_EHIP = -3,     /* a HIP runtime call failed (no GPU, launch error, ...) */
	CRD_ERCCL = -4,    /* an RCCL call failed */
	CRD_EIO = -5,      /* file could not be read / written */
	CRD_EPARSE = -6,   /* malformed ini file or missing mandatory key */
	CRD_ESTATE = -7    /* call not valid in the context's current state */
} crd_status;

enum { CRD_MODEL_FHN = 0, CRD_MODEL_GOLDBETER = 1 };
enum { CRD_SURFACE_TORUS = 0, CRD_SURFACE_FLAT = 1 };
enum { CRD_PRECISION_F64 = 0, CRD_PRECISION_F32 = 1 };

/* Which RK4 implementation crd_step_rk4 runs (results agree to round-off). */
enum {
	CRD_STEPPER_AUTO = 0,
	CRD_STEPPER_STAGED = 1, /* four stage kernels per step, one halo row exchanged per stage */
	CRD_STEPPER_FUSED = 2   /* one kernel per step (all four stages on chip); multi-slab: 4 E halo rows every E steps (crd_set_exchange_period); slabs shorter than that use the staged kernels */
};

/* Halo transport between the slabs of one run. */
enum {
	CRD_HALO_SELF = 0,  /* single slab: periodic wrap inside the kernels */
	CRD_HALO_LOCAL = 1, /* several contexts in one process (any devices): device-to-device copies */
	CRD_HALO_RCCL = 2   /* one context per process / GPU: ncclSend / ncclRecv over xGMI */
};

/* ---------------------------------------------------------------------------------------------------------
 * Parameters of the hot path: what f() reads from UserData and from the file-scope globals
 * (src/FHNmodel_torus.cpp:80-94,97-122; src/GoldbeterModel_torus.cpp:91-106).
 * --------------------------------------------------------------------------------------------------------- */
typedef struct crd_params {
	int32_t model;          /* CRD_MODEL_* */
	int32_t surface;        /* CRD_SURFACE_* */
	int64_t nx;             /* thetaMesh / xMesh */
	int64_t ny;             /* 0 = derive as the reference does (:193 / flat :190-192); >0 = phiMesh override */
	double surface_length;  /* surfaceLength: major circumference / flat length */
	double surface_width;   /* surfaceWidth:  minor circumference / flat width */
	double diffusion;       /* DIFF */
	double beta;            /* BETA */
	double beta_min;        /* BETAMIN */
	double beta_max;        /* BETAMAX */
	int32_t vary_beta;      /* VARYBETA */
	int32_t just_diffusion; /* JUST_DIFFUSION (Goldbeter) */
	double t_boundary;      /* TBOUNDARY */
	int32_t precision;      /* CRD_PRECISION_*: arithmetic and storage type on the device */
	int32_t reserved;
} crd_params;

/* Derived geometry (src/FHNmodel_torus.cpp:186-193,233-234; src/FHNmodel_flat.cpp:172-175,190-192,230-231). */
typedef struct crd_grid {
	int64_t nx, ny;
	double dx, dy;
	double xmin, xmax, ymin, ymax;
	double R, r;            /* torus radii; 0 for flat */
} crd_grid;

/* Driver-level configuration: everything main() reads from the ini file (src/FHNmodel_torus.cpp:158-174,
 * src/FHNmodel_flat.cpp:157-170, src/GoldbeterModel_torus.cpp:174-187, src/GoldbeterModel_flat.cpp:169-184),
 * plus this build's extension keys. */
typedef struct crd_run_config {
	crd_params params;
	double wave_length;       /* waveLength */
	double wave_width;        /* waveWidth */
	int32_t wave_inside;      /* waveInside (torus) */
	int32_t output_timestep;  /* outputTimestep = Nt */
	double t_final;           /* tFinal */
	int32_t include_all_vars; /* includeAllVars */
	int32_t ic_type;          /* icType (Goldbeter flat) */
	/* extensions (absent keys take these defaults) */
	double dt;                /* [Solver] dt: fixed RK4 step; 0 = safety * crd_stable_dt */
	double dt_safety;         /* [Solver] dtSafety, default 0.8 */
	int32_t n_gpus;           /* [Solver] gpus, default 1 */
	int32_t stepper;          /* [Solver] stepper: CRD_STEPPER_* */
	int32_t adaptive;         /* [Solver] adaptive: 0 = fixed dt; 1 = error-controlled steps with ARKode's default explicit pair and controller
	                           * (CRD_ADAPT_ARKODE: the reference's integrator); 2 = the RK4(3) pair of earlier rounds (CRD_ADAPT_RK43) */
	int32_t steady_state_decimals; /* [Solver] steadyStateDigits (crd_run --ref-steady-state = 8): 0 = the exact Goldbeter fixed point;
	                                * n > 0 = that fixed point as the reference receives it, through numpy's print of a one-element
	                                * array (n digits behind the decimal point; numpy's default is 8) and fscanf
	                                * (crd_steady_state_as_printed) */
	double rtol, atol;        /* [Solver] rtol / atol, defaults 1e-5 / 1e-10 (src/FHNmodel_torus.cpp:197-198) */
	int32_t exchange_period;  /* [Solver] exchangePeriod: fused steps between two halo exchanges of a multi-slab run (crd_set_exchange_period, 3 .. 16);
	                           * 0 (default) = the driver chooses: 10 where every slab has at least 256 rows, else 8 */
	int32_t reserved;
} crd_run_config;

typedef struct crd_ctx crd_ctx;

/* ---------------------------------------------------------------------------------------------------------
 * Host-side helpers (no GPU needed).
 * --------------------------------------------------------------------------------------------------------- */

int crd_abi_version(void);
const char *crd_status_string(int status);
/* 16 hex digits over the step kernels of THIS build as the assembler printed them (template arguments, registers, occupancy, the
 * steady-state loop's instruction mix: tools/kernel_regs.py writes them into the library when it is built); "" for a build without the
 * table.  The profile tables a run quotes counters from (profiles/pmc_traffic.json, plan_stats.json) carry the digest of the build they
 * were measured on; bench.py quotes them only when it equals this one.  No reference counterpart. */
const char *crd_kernel_table_digest(void);

/* Replaces boost::property_tree::ini_parser::read_ini + the pt.get<T>() block of main()
 * (src/FHNmodel_torus.cpp:158-174 and the three siblings).  The program's own mesh key is preferred
 * (thetaMesh for FHN, xMesh for Goldbeter) but either is accepted; keys the reference program does not read
 * are optional; a missing mandatory key is CRD_EPARSE (the reference aborts on ptree_bad_path).  err (may be
 * NULL) receives a message. */
int crd_config_load_ini(const char *path, int model, int surface, crd_run_config *cfg, char *err, size_t err_len);

/* Geometry scalars a9: r, R, ny, dx, dy, domain bounds. */
int crd_grid_from_params(const crd_params *p, crd_grid *g);

/* phi-slab extents: SetupDecomp (src/FHNmodel_torus.cpp:750-755) with dims = {1, n_slabs}. */
int crd_slab_extents(int64_t ny, int slab, int n_slabs, int64_t *js, int64_t *je);

/* The reference's own 2-D (theta x phi) block decomposition: MPI_Dims_create(nprocs, 2, dims) as SetupDecomp
 * calls it (src/FHNmodel_torus.cpp:724-728: 4 -> {2, 2}, 8 -> {4, 2}, 2 -> {2, 1}), and the extents of block (c0, c1) of a d0 x d1
 * process grid (:750-753: is = nx c0 / d0, ie = nx (c0 + 1) / d0 - 1, likewise js, je).  The rank of a block is MPI's Cartesian
 * rank, c0 d1 + c1.  Blocks with d0 > 1 step with the staged kernels (one ghost row / column strip of var0 per stage, the four
 * strips of the reference's Exchange(), :775-950) in LOCAL groups; the one-launch stepper, the adaptive integrators and the RCCL
 * transport need phi-slabs (d0 = 1), which is the layout to use on one node -- the block layout exists so that `-np 4` of the
 * reference's scripts (util/ShellScripts/runFHNmodelTorus.sh:6) can be reproduced file for file. */
int crd_dims_create(int nprocs, int *d0, int *d1);
int crd_block_extents(int64_t nx, int64_t ny, int c0, int d0, int c1, int d1, int64_t *is, int64_t *ie, int64_t *js, int64_t *je);

/* Stable state used by the initial conditions and the banner: FHN analytic (src/FHNmodel_torus.cpp:242-244);
 * Goldbeter fixed point, computed natively instead of popen("SolveGoldbeterODE.py")
 * (src/GoldbeterModel_torus.cpp:254-261). */
int crd_steady_state(int model, double beta, double *s0, double *s1);

/* The same state the way the reference's Goldbeter programs receive it: `print Z[-1], Y[-1]` of one-element numpy arrays
 * (util/GoldbeterModel/SolveGoldbeterODE.py:111; numpy prints `decimals` = 8 digits behind the decimal point, e.g.
 * "[ 0.392] [ 1.64562147]") read back by fscanf("[%lf] [%lf]", ...) (src/GoldbeterModel_torus.cpp:254-261).  decimals = 0, or
 * the FHN model (computed in C++ by the reference, :242-244): no rounding.  What this cannot reproduce is the error of the
 * script's own BDF integration towards that point (scipy VODE at its default rtol 1e-6 over 50 time units): the reference's
 * printed digits agree with these to about that tolerance, not to the last of the eight. */
int crd_steady_state_as_printed(int model, double beta, int decimals, double *s0, double *s1);

/* Initial conditions of rows [js, je] in the boundary layout (AoS doubles, 2*nx*(je-js+1) values):
 * src/FHNmodel_torus.cpp:285-354, src/FHNmodel_flat.cpp:280-319, src/GoldbeterModel_torus.cpp:313-414,
 * src/GoldbeterModel_flat.cpp:309-379. */
int crd_initial_conditions(const crd_run_config *cfg, int64_t js, int64_t je, double *y_aos);
/* ... of the block [is, ie] x [js, je] (2 (ie-is+1) (je-js+1) values, IDX with nxl = ie-is+1).  The rand() rule draws row by row
 * through the block from the default seed, as every reference rank does. */
int crd_initial_conditions_block(const crd_run_config *cfg, int64_t is, int64_t ie, int64_t js, int64_t je, double *y_aos);

/* Largest step the classical RK4 scheme takes stably on this problem: 2.785 / lambda_max (2.785 = the extent of RK4's stability
 * region on the negative real axis), with
 *   lambda_max = 4 D (1/(r dx)^2 + 1/((R - r) dy)^2) + D / (r (R - r) dx)      torus: the second differences at theta = pi, where
 *                                                                              the phi spacing is smallest, plus the advective term
 *              = 4 D (1/dx^2 + 1/dy^2)                                         flat
 *              + a bound on the reaction Jacobian: 10 for FitzHugh-Nagumo (|3 - 3 u^2| <= 9 for |u| <= 2, which contains the
 *                limit cycle, + 1), 400 for Goldbeter (the spectral radius of the kinetics' Jacobian over 0 <= Z <= 1.5,
 *                0 <= Y <= 3 is 333, the VM3 Hill term's slope in Z reaching 410; rounded up).  On the BASELINE grids the reaction
 *                term is 0.05 % (FHN) / 2 % (Goldbeter at 4096^2) of lambda_max; it decides on coarse grids (the shipped 100 x 400
 *                Goldbeter run).
 * crd_run's default step is dtSafety (0.8) times this, and it is the default cap of crd_integrate_adaptive (h_max = 0).
 * No reference counterpart: ARKode finds its steps by error control (src/FHNmodel_torus.cpp:365). */
double crd_stable_dt(const crd_params *p);

/* Output files of one slab, byte-compatible with src/FHNmodel_torus.cpp:376-410,438-455:
 * <Model>_<surface>_subdomain.%03i.txt, <Model>_<surface>_<var0>.%03i.txt, <..>_<var1>.%03i.txt in `dir`. */
typedef struct crd_writer crd_writer;
int crd_writer_open(const crd_run_config *cfg, const char *dir, int slab, int n_slabs, crd_writer **out);
int crd_writer_open_block(const crd_run_config *cfg, const char *dir, int rank, int c0, int d0, int c1, int d1, crd_writer **out); /* block (c0, c1) of d0 x d1 */
int crd_writer_write_row(crd_writer *w, const double *y_aos); /* one output time: nyl*nxl values per file */
int crd_writer_close(crd_writer *w);

/* Binary side-channel next to the text files (no reference counterpart: src/FHNmodel_torus.cpp:438-455 writes 24 characters per
 * value, 1.6 GB per output time at 8192^2): <Model>_<surface>_<var>.%03i.npy, a NumPy array of shape (frames, nyl, nxl) in the
 * text file's own ordering (frame = output time, then j, then i), value_bytes = 8 or 4 per value, little endian.  `frame` is a
 * contiguous (nyl, nxl) block, e.g. what crd_state_download_rows(ctx, var, 0, nyl, frame) delivers. */
typedef struct crd_npy_writer crd_npy_writer;
int crd_npy_writer_open(const crd_run_config *cfg, const char *dir, int slab, int n_slabs, int var, int value_bytes, crd_npy_writer **out);
int crd_npy_writer_append(crd_npy_writer *w, const void *frame);
int crd_npy_writer_close(crd_npy_writer *w);

/* ---------------------------------------------------------------------------------------------------------
 * Device context: replaces UserData + InitUserData / SetupDecomp / FreeUserData
 * (src/FHNmodel_torus.cpp:97-122,708-772,953-997).  Not thread-safe; calls on one context must be serialised.
 * --------------------------------------------------------------------------------------------------------- */

/* HIP devices visible to this process (0 when there is none or the runtime cannot start). */
int crd_device_count(void);

/* slab / n_slabs: which phi-slab of the global grid this context owns; device: HIP device ordinal. */
int crd_create(const crd_params *p, int slab, int n_slabs, int device, crd_ctx **out);
/* Block (c0, c1) of a d0 x d1 decomposition (crd_create(p, slab, n, ...) = crd_create_block(p, 0, 1, slab, n, ...)); group arrays
 * (crd_comm_attach_local, crd_group_*) hold the blocks in rank order, c0 d1 + c1. */
int crd_create_block(const crd_params *p, int c0, int d0, int c1, int d1, int device, crd_ctx **out);
int crd_get_block(const crd_ctx *ctx, int64_t *is, int64_t *ie, int64_t *js, int64_t *je);
void crd_destroy(crd_ctx *ctx);
const char *crd_last_error(const crd_ctx *ctx); /* never NULL; ctx may be NULL (creation errors) */

int crd_get_grid(const crd_ctx *ctx, crd_grid *g);
int crd_get_slab(const crd_ctx *ctx, int64_t *js, int64_t *je);

/* Multi-slab wiring.  LOCAL: give every context of the run the full array (same process).
 * RCCL: rank r of n_slabs ranks calls crd_comm_init_rccl with the 128-byte id rank 0 obtained from
 * crd_comm_unique_id and distributed by any means (MPI_Bcast, torch.distributed, a file).  The RCCL entry points are bound at
 * first use from librccl.so.1 -- or from the file given to crd_comm_set_rccl_library before that first use (another RCCL
 * build; NULL or "" = the default again; CRD_ESTATE once bound). */
int crd_comm_attach_local(crd_ctx *const *ctxs, int n_slabs);
int crd_comm_set_rccl_library(const char *path);
int crd_comm_unique_id(void *id128);
int crd_comm_init_rccl(crd_ctx *ctx, const void *id128);

/* What the context's transport is and, for RCCL, what the communicator itself reports (ncclCommCount / ncclCommUserRank):
 * halo = CRD_HALO_* (-1 while a multi-slab context is not wired yet), ranks / rank of the ring.  Any pointer may be NULL. */
int crd_comm_info(const crd_ctx *ctx, int *halo, int *ranks, int *rank);

/* ONE halo exchange of the resident state, outside any step: fills ghost rows [-depth, 0) and [nyl, nyl+depth) of both
 * fields from the ring neighbours (the N/S half of Exchange(), src/FHNmodel_torus.cpp:775-950, at the depth the fused
 * stepper uses) and waits for it.  1 <= depth <= 64.  Every rank of an RCCL run must make the same call.  Together with
 * crd_state_download_rows it lets a host program verify the transport (ghost rows == the neighbours' owned rows). */
int crd_halo_exchange(crd_ctx *ctx, int depth);

/* Rows [row_begin, row_begin + row_count) of ONE field (var 0 / 1) of the resident state, ghost rows included
 * (-64 <= row_begin, row_begin + row_count <= nyl + 64), as contiguous rows of nx reals in the DEVICE precision. */
int crd_state_download_rows(crd_ctx *ctx, int var, int64_t row_begin, int64_t row_count, void *rows_host);

/* The ring protocol of one halo exchange, as data: the four point-to-point operations slab `slab` of `n_slabs` issues,
 * in issue order, to fill its ghost rows [-depth, 0) and [nyl, nyl+depth) from its periodic phi neighbours (replaces the
 * N/S half of Exchange(), src/FHNmodel_torus.cpp:775-950; the E/W half disappears because a slab spans all of theta).
 * Rows are local indices (ghost rows are negative or >= nyl).  The order matters when both neighbours are the same
 * rank (n_slabs <= 2): operations between one pair of ranks match in issue order, so the LAST rows are sent first and
 * the LOW ghost rows are received first.  The RCCL transport issues exactly this plan inside one ncclGroup; the CPU
 * tests drive it over gloo. */
typedef struct crd_halo_op {
	int32_t is_send;    /* 1 = send owned rows, 0 = receive into ghost rows */
	int32_t peer;       /* slab index of the other side */
	int64_t row_begin;  /* first local row */
	int64_t row_count;
} crd_halo_op;
int crd_halo_plan(int slab, int n_slabs, int64_t nyl, int depth, crd_halo_op ops[4]);

/* How the ranks of an RCCL ring agree, at the start of a stepping call, where in the deep-halo exchange cycle the ring stands --
 * as data, like crd_halo_plan, so that the rule can be driven over any transport (the CPU tests use gloo).  Each rank votes
 * crd_cycle_vote(pos): pos = steps its resident state has taken since its ghost rows were last exchanged (0 .. E - 1), or -1 for a
 * state whose ghost rows cannot be trusted (new upload, other stepper, failed call).  The element-wise MIN of the votes over
 * the ranks (ncclAllReduce in the library) goes to crd_cycle_agreed: the common position when every rank voted the same
 * non-negative one -- the call carries on there -- else -1: every rank starts with an exchange.  No reference counterpart: the
 * reference exchanges inside every f() (src/FHNmodel_torus.cpp:521). */
int crd_cycle_vote(int pos, double vote[2]);
int crd_cycle_agreed(const double reduced[2]);

/* State transfer in the boundary layout.  host_is_f64 = 1: host buffer holds doubles whatever the device
 * precision (converted on the device); 0: host buffer holds the device precision. */
int crd_state_upload(crd_ctx *ctx, const void *y_aos_host, int host_is_f64);
int crd_state_download(crd_ctx *ctx, void *y_aos_host, int host_is_f64);

/* Page-locked host memory for the vectors handed to crd_rhs_host (e.g. as the data array of N_VMake_Parallel).  With
 * pinned y and ydot a single-slab crd_rhs_host streams the slab band by band -- upload of band k+1, kernel on band k and
 * download of band k-1 overlap, both directions of the host link busy -- instead of copy, compute, copy; pageable
 * vectors work too, at the rate of a staged copy each way.  NULL when the allocation fails. */
void *crd_host_alloc(size_t bytes);
void crd_host_free(void *p);

/* One RHS evaluation, the ARKRhsFn `f(t, y, ydot, user_data)` of src/FHNmodel_torus.cpp:126,504-667 (and
 * siblings): halo exchange + diffusion + kinetics, writes every element of ydot, does not modify y.
 * y / ydot are this slab's AoS vectors in the device precision; *_host takes host pointers (staged through
 * device memory), *_device takes device pointers on the context's device.  Returns 0, or <0 like the
 * reference's f() returns -1 when Exchange fails (:522). */
int crd_rhs_host(crd_ctx *ctx, double t, const void *y_aos, void *ydot_aos);
int crd_rhs_device(crd_ctx *ctx, double t, const void *y_aos_dev, void *ydot_aos_dev);

/* The rest of what an integrator asks of a problem: f split into its diffusion and its reaction part, and the action of the
 * Jacobian on a vector -- ARKode's implicit slot `fi` and its Jacobian-times-vector callback, both of which the reference leaves
 * empty (ARKodeInit(arkode_mem, f, NULL, T0, y), src/FHNmodel_torus.cpp:362; arkode_pcg.h included at :51 and never used).
 * Vectors are in the layout of crd_rhs_*: AoS [var0, var1], theta fastest, the local slab only, the context's precision.
 *   f = f_D + f_R.  CRD_PART_FULL: f itself; crd_rhs_part_* then launches what crd_rhs_* launches and gives its bits.
 *   CRD_PART_DIFFUSION: the operator alone, dvar1 = +0.0 (the bits of a diffusion-only Goldbeter context's f on the same geometry).
 *   CRD_PART_REACTION: the kinetics alone (zeros for Goldbeter with just_diffusion); on a uniform state it has the bits of f.
 *   crd_jtimes_*: jv = J_part(t, y) v.  J_D does not depend on y: J_D v is f_D evaluated on v, bit for bit.  J_R is the pointwise
 *   2x2 block, FHN [[3 - 3u^2, -1], [EPSILON, 0]], Goldbeter [[-w_z - k, -w_y + kf], [w_z, w_y - kf]] with w = v2(z) - v3(z, y).
 * Absorbing rows: while t < t_boundary (strictly, as in f) global rows 0 and ny - 1 are zero in every part of f and are zero rows
 * of every part of J, on the slab that owns them.  A Goldbeter context with just_diffusion has no absorbing rows in f
 * (src/GoldbeterModel_torus.cpp:668 skips them with the kinetics), so it has none here either.
 * Halos: DIFFUSION and FULL of crd_rhs_part_* exchange var0 of y's edge rows as crd_rhs_* does; DIFFUSION and FULL of crd_jtimes_*
 * exchange var0 of V's edge rows and nothing of y.  Those calls are collective like crd_rhs_*: RCCL contexts through the plain entry
 * points, LOCAL groups through the crd_group_* ones.  REACTION exchanges nothing and is NOT collective: any context may call it alone,
 * through either entry point.  theta-block contexts (crd_create_block with d0 > 1) are refused with CRD_ESTATE; a part that is none
 * of the three returns CRD_EINVAL.  The *_host forms stage through device memory (no banded pipeline). */
enum { CRD_PART_FULL = 0, CRD_PART_DIFFUSION = 1, CRD_PART_REACTION = 2 };
int crd_rhs_part_device(crd_ctx *ctx, double t, int part, const void *y_aos_dev, void *ydot_aos_dev);
int crd_rhs_part_host(crd_ctx *ctx, double t, int part, const void *y_aos, void *ydot_aos);
int crd_jtimes_device(crd_ctx *ctx, double t, int part, const void *y_aos_dev, const void *v_aos_dev, void *jv_aos_dev);
int crd_jtimes_host(crd_ctx *ctx, double t, int part, const void *y_aos, const void *v_aos, void *jv_aos);

/* The preconditioner solve of an implicit stage's system (I - gamma J_D(t)) z = r: z = M r, M one geometric multigrid V-cycle on the
 * device.  Vectors are those of crd_jtimes_*: AoS, the context's precision.  P = I - gamma J_D acts on var0 only; z_var1 = r_var1 bit
 * for bit.  M is a fixed linear map of r (what a Krylov method asks of a preconditioner); gamma = 0 returns z = r exactly.
 *   Level l:  L_l x (j, i) = cE[i] (x[j, i+1] - x[j, i]) + cWn[i] (x[j, i] - x[j, i-1]) + cP[i] (x[j+1, i] - 2 x[j, i] + x[j-1, i]), periodic in
 *   theta and phi as crd_rhs_part_*(CRD_PART_DIFFUSION) takes its neighbours; A_l = I - gamma L_l; diagonal d_l[i] = 1 + gamma (2 cX_l + 2 cP_l[i]).
 *   Level 0 is the context's grid and tables.  Level l + 1 exists while nx_l and ny_l are both even and both halves are >= 4, up to
 *   max_levels; coarse point (J, I) is fine point (2 J, 2 I); the coarse tables are the same formulas at doubled spacing,
 *   cX / 4, cA[2 I] / 2, cP[2 I] / 4 (cE = cX + cA, cWn = cA - cX formed in double, rounded once).
 *   Held rows: when J has zero rows at t (t < t_boundary strictly, never with just_diffusion: the rule of crd_jtimes_*) level 0 holds
 *   rows 0 and ny - 1 and every coarser level row 0 only -- fine row ny - 1 has no coarse counterpart.  L_l has zero rows there.
 *   Sweep (damped Jacobi): z <- z + omega (r - (z - gamma L_l z)) / d_l from the old z everywhere, then z = r on held rows.
 *   Cycle on level l: the coarsest level takes `coarse` sweeps from z = 0; any other `pre` sweeps from z = 0, the residual
 *   r - A_l z restricted by full weighting (1/16 [1 2 1; 2 4 2; 1 2 1], periodic) and zeroed on the coarse held row, the cycle on
 *   level l + 1 for the correction, its bilinear prolongation (periodic) zeroed on this level's held rows and added, `post` sweeps.
 * Limit: with held rows and large gamma ONE cycle alone is not a contraction (||r - A z|| / ||r|| up to 13 was measured on a
 * prototype: the coarse levels hold a row shifted by one fine row); as a Krylov preconditioner that costs a few iterations.
 * opt == NULL: the defaults (pre = post = 2, coarse = 8, max_levels = 16, omega = 0.8).  CRD_EINVAL, before any device work: gamma
 * negative or not finite; pre or post negative or pre + post < 1; coarse < 1; max_levels outside 1 .. 16; omega outside (0, 1]; z == r.
 * CRD_ESTATE: a context that is one of several slabs (a LOCAL group member, an RCCL world > 1) and theta-block contexts.  The
 * workspace -- three var0 planes per level, every level the grid has -- is allocated by the first crd_psolve_device / _host call and freed
 * by crd_destroy (CRD_ENOMEM if it cannot be had); crd_psolve_info reports its size and the levels a call with `opt` uses (entries of
 * nx / ny beyond `levels` are 0; any output pointer may be NULL).  Launches go on the context's compute stream: _device returns
 * without waiting, like crd_jtimes_device; _host stages through device memory and waits. */
typedef struct crd_psolve_options {
	int32_t pre, post, coarse, max_levels;
	double omega;
} crd_psolve_options;
int crd_psolve_defaults(crd_psolve_options *opt);
int crd_psolve_info(crd_ctx *ctx, const crd_psolve_options *opt, int32_t *levels, int32_t nx[16], int32_t ny[16], int64_t *workspace_bytes);
int crd_psolve_device(crd_ctx *ctx, double t, double gamma, const crd_psolve_options *opt, const void *r_aos_dev, void *z_aos_dev);
int crd_psolve_host(crd_ctx *ctx, double t, double gamma, const crd_psolve_options *opt, const void *r_aos, void *z_aos);

/* The linear solve of an implicit stage: (I - gamma J_part(t, y)) z = r by restarted, right-preconditioned GMRES(restart) on the
 * device, from z = 0.  Vectors are those of crd_jtimes_*: AoS, the context's precision.  It solves A M u = r, z = M u, with
 * A v = v - gamma J_part v through the launch of crd_jtimes_device and M the cycle of crd_psolve_device for I - gamma J_D(t) with the
 * options `psolve` (precondition = 1), or the identity (precondition = 0).  With the preconditioner on the right the residual the
 * iteration carries is the residual of the system itself: it stops when ||r - A z|| <= rtol ||r|| + atol, 2-norms over the whole vector.
 *   A new Krylov vector w = A M V_j is orthogonalised against V_0 .. V_j by classical Gram-Schmidt applied twice, in four launches:
 *   multi-dot h = V^T w (one pass over w per 8 basis vectors, double accumulators, per-block partials summed in a fixed order),
 *   multi-axpy w -= V h with the partials of ||w||^2 from the same pass, and both again; the Hessenberg column is the sum of the two
 *   coefficient sets.  The host reads that column -- j + 2 doubles, the one device-to-host copy of an inner iteration -- keeps the
 *   Givens rotations and solves the small least-squares problem; a cycle ends with z += M (sum_i y_i V_i), one M for the cycle.
 *   Breakdown: when ||w|| after the orthogonalisation is at most 2 u ||A M V_j|| (u the unit roundoff of the precision, ||A M V_j|| taken
 *   as the 2-norm of the column), the column is final: the basis is not extended, nothing is divided by that norm, the solve has converged.
 *   CRD_PART_DIFFUSION: J_D acts on var0 alone, so the iteration runs on var0 (var1 of every Krylov vector is +0) and z_var1 = r_var1
 *   bit for bit; y is not read and may be NULL.  CRD_PART_FULL takes J(t, y) and needs y.
 * gamma == 0 returns z = r exactly without iterating; r == 0 returns z = 0 with 0 iterations.  Reaching max_iters (inner iterations
 * in total) is NOT an error: the call returns 0 with converged = 0 and z the last iterate.  Every loop is bounded by restart and max_iters.
 * opt == NULL: the defaults (DIFFUSION, preconditioned, restart 30, max_iters 200, rtol 1e-8, atol 0, crd_psolve_defaults).
 * CRD_EINVAL, before any device work: gamma negative or not finite; part CRD_PART_REACTION or none of the three; restart outside
 * 1 .. 64; max_iters < 1; rtol or atol negative or not finite; z aliasing r or y; y == NULL with CRD_PART_FULL; psolve options that
 * crd_psolve_* refuses.  CRD_ESTATE: a context that is one of several slabs and theta-block contexts, as for crd_psolve_*.
 * Workspace: restart + 1 basis vectors, two work vectors and the reductions' partials, allocated by the first call on the context
 * for the largest restart seen so far and freed by crd_destroy (CRD_ENOMEM if it cannot be had); crd_lsolve_info reports the device
 * bytes a call with `opt` needs (the preconditioner's own workspace is crd_psolve_info's).  Launches go on the context's compute
 * stream, and the call WAITS for it -- it reads scalars every inner iteration -- so _device too returns with z complete.
 * stats (may be NULL): r_norm = ||r||; res_norm = the iteration's own residual norm at exit; restarts = cycles begun after the first;
 * matvecs / psolves = launches of J v / of the cycle. */
typedef struct crd_lsolve_options {
	int32_t part;          /* CRD_PART_DIFFUSION (default) or CRD_PART_FULL */
	int32_t precondition;  /* 1 (default): M = the crd_psolve cycle for I - gamma J_D; 0: none */
	int32_t restart;       /* default 30; 1 .. 64 */
	int32_t max_iters;     /* default 200; inner iterations in total */
	double rtol, atol;     /* default 1e-8, 0 */
	crd_psolve_options psolve;
} crd_lsolve_options;
typedef struct crd_lsolve_stats {
	int32_t converged, iterations, restarts, matvecs, psolves, breakdown;
	double r_norm, res_norm;
} crd_lsolve_stats;
int crd_lsolve_defaults(crd_lsolve_options *opt);
int crd_lsolve_info(crd_ctx *ctx, const crd_lsolve_options *opt, int64_t *workspace_bytes);
int crd_lsolve_device(crd_ctx *ctx, double t, double gamma, const crd_lsolve_options *opt, const void *y_aos_dev, const void *r_aos_dev, void *z_aos_dev,
                      crd_lsolve_stats *stats);
int crd_lsolve_host(crd_ctx *ctx, double t, double gamma, const crd_lsolve_options *opt, const void *y_aos, const void *r_aos, void *z_aos, crd_lsolve_stats *stats);
/* For the test suite's gate on the reductions alone: out[i] = <V_i, w>, i < count (1 .. 65), as the solve's multi-dot forms it.
 * vectors: `count` AoS vectors back to back, w: one, all HOST memory in the context's precision; out: `count` doubles. */
int crd_krylov_probe_dots(crd_ctx *ctx, const void *vectors, int count, const void *w, double *out);

/* The same system by BiCGStab: (I - gamma J_part(t, y)) z = r, right-preconditioned, A and M those of crd_lsolve_*.  A short
 * recurrence: no basis, no orthogonalisation, eight work vectors whatever the iteration count; one iteration is TWO A and TWO M.
 * tol = rtol ||r|| + atol, ||r|| the 2-norm over the whole vector.  CRD_PART_DIFFUSION runs on var0: var1 of every work vector is +0
 * and z_var1 = r_var1 bit for bit.
 *   Start.  x = 0 and res = r (var1 masked), no matvec; with guess = 1: x = the caller's z (DIFFUSION: its var0) and
 *           res = r - fma(-gamma, J x, x) through one matvec.  rhat = res, rho = <rhat, res>, p = res.  ||res|| <= tol: 0 iterations,
 *           converged.
 *   Iteration i = 1 .. max_iters:
 *      1. phat = M p
 *      2. v = fma(-gamma, J phat, phat);  d = <rhat, v>
 *      3. alpha = rho / d
 *      4. s = fma(-alpha, v, res);  ||s||^2 of the stored s
 *      5. ||s|| <= tol:  x = fma(alpha, phat, x); half exit, converged
 *      6. shat = M s
 *      7. t = fma(-gamma, J shat, shat);  <t, s>, <t, t>
 *      8. omega = <t, s> / <t, t>
 *      9. x = fma(omega, shat, fma(alpha, phat, x))
 *     10. res = fma(-omega, t, s);  ||res||^2 and rho' = <rhat, res> of the stored res
 *     11. ||res|| <= tol: converged
 *     12. beta = (rho' / rho) (alpha / omega);  rho = rho'
 *     13. p = fma(beta, fma(-omega, v, p), res)
 *   Five fused kernels carry that (crd_bicgstab.hip): 2 and 7 in place over the J v buffer with their dots; 4; 9 - 10 in one pass; 13; 5.
 *   Scalars: alpha, omega, beta are formed in double on the host from the reductions the device leaves, rounded ONCE to the context's
 *   precision and passed by value; the same rounded alpha (omega) updates x and the residual.  Vector arithmetic is in the context's
 *   precision, every multiply-add fused; reductions are in double, per-block partials summed in a fixed order, no atomics: the bits
 *   repeat from run to run.
 *   Breakdown: the host looks at every scalar before the kernel that uses it is launched.  A zero or non-finite d (or alpha),
 *   <t, t>, omega, rho' (or a non-finite beta) ends the call with status 0, converged = 0 and breakdown = CRD_BICGSTAB_BREAKDOWN_*;
 *   z is the last consistent iterate -- at <t, t> or omega x = fma(alpha, phat, x) is applied first, since s is its residual
 *   (half_exit = 1, the iteration counts).  An iteration that breaks down at d does not count.
 * Reaching max_iters is NOT an error (converged = 0, z the last iterate); gamma == 0 returns z = r; r == 0 returns z = 0; a
 * non-finite ||r|| returns converged = 0 without an iteration.  No convergence is promised for CRD_PART_FULL where I - gamma J is
 * indefinite: the recurrences may then end in a breakdown.  Every loop is bounded by max_iters.
 * After the loop one more matvec forms ||r - A z|| (counted in matvecs): true_res_norm.  res_norm stays the recurrence's own, and
 * converged is judged on the recurrence.
 * opt == NULL: the defaults (DIFFUSION, preconditioned, max_iters 200, guess 0, rtol 1e-8, atol 0, crd_psolve_defaults).
 * Refusals and contexts: those of crd_lsolve_* (there is no restart), and guess outside {0, 1}.  Workspace: eight vectors (res, rhat,
 * p, v, s, t, phat, shat), the partials and a page-locked scalar block -- its own allocation, never that of crd_lsolve_*, made by the
 * first call, freed by crd_destroy; crd_bicgstab_info reports its device bytes.  The call WAITS for its work.
 * The device vectors of crd_bicgstab_device (y, r, z) must be 16-byte aligned, as hipMalloc returns them: the kernels move 16 bytes
 * per thread.
 * stats (may be NULL): iterations completed (each two matvecs, a half exit one); half_exit = 1 when z is the iterate of step 5;
 * matvecs / psolves = launches of J v / of the cycle. */
enum { CRD_BICGSTAB_BREAKDOWN_NONE = 0, CRD_BICGSTAB_BREAKDOWN_D = 1, CRD_BICGSTAB_BREAKDOWN_TT = 2, CRD_BICGSTAB_BREAKDOWN_OMEGA = 3, CRD_BICGSTAB_BREAKDOWN_RHO = 4 };
typedef struct crd_bicgstab_options {
	int32_t part;          /* CRD_PART_DIFFUSION (default) or CRD_PART_FULL */
	int32_t precondition;  /* 1 (default): M = the crd_psolve cycle for I - gamma J_D; 0: none */
	int32_t max_iters;     /* default 200 */
	int32_t guess;         /* 0 (default): from x = 0; 1: from the caller's z */
	double rtol, atol;     /* default 1e-8, 0 */
	crd_psolve_options psolve;
} crd_bicgstab_options;
typedef struct crd_bicgstab_stats {
	int32_t converged, iterations, half_exit, matvecs, psolves, breakdown;
	double r_norm, res_norm, true_res_norm;
} crd_bicgstab_stats;
int crd_bicgstab_defaults(crd_bicgstab_options *opt);
int crd_bicgstab_info(crd_ctx *ctx, const crd_bicgstab_options *opt, int64_t *workspace_bytes);
int crd_bicgstab_device(crd_ctx *ctx, double t, double gamma, const crd_bicgstab_options *opt, const void *y_aos_dev, const void *r_aos_dev, void *z_aos_dev,
                        crd_bicgstab_stats *stats);
int crd_bicgstab_host(crd_ctx *ctx, double t, double gamma, const crd_bicgstab_options *opt, const void *y_aos, const void *r_aos, void *z_aos, crd_bicgstab_stats *stats);
/* For the test suite's gate on each fused kernel alone: runs kernel `kernel` once on HOST vectors in the context's precision, given
 * back to back in `in`, with `scalars` rounded as the solve rounds them, and returns its output vectors back to back in `out` and its
 * reductions in `sums`:
 *   CRD_BICGSTAB_KERNEL_APPLY_DOT   in jv, x, b       scalars gamma         out fma(-gamma, jv, x)   sums <b, out>
 *   CRD_BICGSTAB_KERNEL_APPLY_DOT2  in jv, x, b       scalars gamma         out fma(-gamma, jv, x)   sums <out, b>, <out, out>
 *   CRD_BICGSTAB_KERNEL_S_UPDATE    in v, res         scalars alpha         out s                    sums ||s||^2
 *   CRD_BICGSTAB_KERNEL_XR_UPDATE   in x, phat, shat, t, s, rhat   scalars alpha, omega   out x, res sums ||res||^2, <rhat, res>
 *   CRD_BICGSTAB_KERNEL_P_UPDATE    in p, v, res      scalars beta, omega   out p                    no sums
 *   CRD_BICGSTAB_KERNEL_X_HALF      in x, phat        scalars alpha         out x                    no sums
 * var0_only (0 / 1) masks var1 of the two apply kernels' output as CRD_PART_DIFFUSION does. */
enum { CRD_BICGSTAB_KERNEL_APPLY_DOT = 0, CRD_BICGSTAB_KERNEL_APPLY_DOT2 = 1, CRD_BICGSTAB_KERNEL_S_UPDATE = 2, CRD_BICGSTAB_KERNEL_XR_UPDATE = 3,
       CRD_BICGSTAB_KERNEL_P_UPDATE = 4, CRD_BICGSTAB_KERNEL_X_HALF = 5 };
int crd_bicgstab_probe(crd_ctx *ctx, int kernel, int var0_only, const double *scalars, const void *in, void *out, double *sums);

/* Fast path that never leaves the GPU: nsteps classical RK4 steps of size dt on the context's resident state,
 * stage k of step n evaluated at t0 + n dt + c_k dt (replaces the ARKode(...) call, src/FHNmodel_torus.cpp:423).
 * Asynchronous; crd_synchronize() waits.  With several slabs every context of the run must make the same call: stepping is
 * COLLECTIVE (same t0, dt, nsteps, stepper on every rank, like the reference's ARKode call on every MPI rank).  Calls that only
 * change one rank's state need not be: crd_state_upload on one rank (a stimulus injected by its owner), or a call that failed
 * there.  The one-launch stepper carries its deep-halo exchange cycle across calls, so under RCCL every stepping call begins
 * with a two-value ncclAllReduce in which the ranks agree where in the cycle the ring stands; if any rank holds a new state,
 * all of them start afresh with an exchange (crd_step_timing.agreement_restarts counts those).  The reduction overlaps the
 * call's first step except when that step is the one that exchanges. */
int crd_set_stepper(crd_ctx *ctx, int stepper);
int crd_step_rk4(crd_ctx *ctx, double t0, double dt, int64_t nsteps);

/* IMEX stepping: nsteps steps of size dt of an additive Runge-Kutta scheme on the context's resident state, the diffusion part f_D
 * implicit and the kinetics f_R explicit, so that dt is not bound by crd_stable_dt's diffusion limit (the kinetics' own explicit
 * limit remains).  Step n starts at t_n = t0 + n dt, as crd_step_rk4 forms it.  Three built-in schemes of the Ascher-Ruuth-Spiteri
 * type -- stage 0 is Y_0 = y_n, the implicit matrix has a zero first column and ONE diagonal value gamma, y_{n+1} is the last stage,
 * c is shared:
 *   CRD_IMEX_EULER   s = 1, order 1: A^E = [1], A^I = [1]
 *   CRD_IMEX_ARS222  s = 2, order 2: gamma = 1 - 1/sqrt(2), delta = 1 - 1/(2 gamma), c = (0, gamma, 1),
 *                    A^E rows (gamma), (delta, 1 - delta); A^I rows (gamma), (1 - gamma, gamma)
 *   CRD_IMEX_ARS443  s = 4, order 3: gamma = 1/2, c = (0, 1/2, 2/3, 1/2, 1),
 *                    A^E rows (1/2), (11/18, 1/18), (5/6, -5/6, 1/2), (1/4, 7/4, 3/4, -7/4)
 *                    A^I rows (1/2), (1/6, 1/2), (-1/2, 1/2, 1/2), (3/2, -3/2, 1/2, 1/2)
 * (A^E columns 0 .. i - 1, A^I columns 1 .. i of stage i = 1 .. s).  f_D is linear, so no Newton iteration: with hE_ij = dt A^E_ij,
 * hI_ij = dt A^I_ij and dt gamma formed in double and rounded to the context's precision, one step is
 *   FR_0 = f_R(t_n, y_n);  R_1 = fma(hE_10, FR_0, y_n);  and for i = 1 .. s at t_i = t_n + c_i dt:
 *     r = f_D(t_i, R_i)                      crd_rhs_part_device(CRD_PART_DIFFUSION)
 *     k_i = (I - dt gamma J_D(t_i))^-1 r     crd_lsolve_device with `lsolve`, from z = 0: k_i = f_D(Y_i)
 *     Y_i = fma(dt gamma, k_i, R_i);  FR_i = f_R(t_i, Y_i), the bits of crd_rhs_part_*(CRD_PART_REACTION) on Y_i;
 *     R_{i+1} = y_n, then for j = 0 .. i ascending fma(hE_{i+1,j}, FR_j, .) and fma(hI_{i+1,j}, k_j, .), terms whose coefficient
 *     is exactly zero skipped -- one kernel, one pass (crd_imex.hip); at i = s it stores Y_s, the new state, and nothing else.
 * The operator and the held rows are those of each stage's own time (zero rows while t_i < tBoundary), as in crd_rhs_part_* and
 * crd_lsolve_*.  The call WAITS for its work, as crd_lsolve_* does.
 * A solve that does not converge within lsolve.max_iters, or a state whose max |var0| is not finite, ends the call with CRD_ESTATE:
 * the resident state is that of the last completed step and stats says where it stopped.
 * Refused before any device work -- CRD_EINVAL: an unknown scheme; lsolve.part other than CRD_PART_DIFFUSION; dt not positive or not
 * finite; t0 not finite; nsteps < 0; lsolve options crd_lsolve_* refuses.  CRD_ESTATE: a context that is one of several slabs,
 * theta-block contexts, and a context with a run recorder open on it.  opt == NULL: crd_imex_defaults.
 * Workspace: y_n, R, s vectors k_j and s + 1 vectors FR_j (the last one holds r) besides crd_lsolve_*'s own, allocated by the first
 * call, kept on the context, freed by crd_destroy; crd_imex_info reports the bytes of both together.
 * stats (may be NULL): steps completed; t = t0 + steps dt; solves and GMRES iterations in total; max_iterations of one solve;
 * failed_step / failed_stage (-1: none); worst_residual = the largest res_norm / r_norm of a solve; max_abs_u = max |var0| of the
 * final state (what crd_state_max_abs reports).
 * solver: CRD_IMEX_SOLVER_GMRES (the default) is everything above.  CRD_IMEX_SOLVER_BICGSTAB solves every stage with
 * crd_bicgstab_device instead, from x = 0: `lsolve` then gives part, precondition, max_iters, rtol, atol and psolve, and restart is
 * not read.  CRD_IMEX_SOLVER_BICGSTAB_WARM starts each stage's solve from the previous stage's k (guess = 1), stage 1 from the
 * previous step's last k once this call has taken a step, and from x = 0 otherwise.  With either, iterations and max_iterations count
 * BiCGStab iterations -- each is two matvecs and two cycles -- and worst_residual takes true_res_norm / r_norm.  Any other value:
 * CRD_EINVAL.  crd_imex_info reports the step's vectors and the chosen solver's workspace alone. */
enum { CRD_IMEX_EULER = 0, CRD_IMEX_ARS222 = 1, CRD_IMEX_ARS443 = 2 };
enum { CRD_IMEX_SOLVER_GMRES = 0, CRD_IMEX_SOLVER_BICGSTAB = 1, CRD_IMEX_SOLVER_BICGSTAB_WARM = 2 };
typedef struct crd_imex_options {
	int32_t scheme;    /* CRD_IMEX_*; default CRD_IMEX_ARS222 */
	int32_t solver;    /* CRD_IMEX_SOLVER_*; default CRD_IMEX_SOLVER_GMRES */
	crd_lsolve_options lsolve;  /* crd_lsolve_defaults; part must be CRD_PART_DIFFUSION */
} crd_imex_options;
typedef struct crd_imex_stats {
	int64_t steps, solves, iterations, failed_step;
	int32_t max_iterations, failed_stage;
	double t, worst_residual, max_abs_u;
} crd_imex_stats;
int crd_imex_defaults(crd_imex_options *opt);
int crd_imex_info(crd_ctx *ctx, const crd_imex_options *opt, int64_t *workspace_bytes);
int crd_step_imex(crd_ctx *ctx, double t0, double dt, int64_t nsteps, const crd_imex_options *opt, crd_imex_stats *stats);

/* Error-controlled IMEX integration from t0 to tout with CRD_IMEX_ARS443 and its embedded second-order solution: the caller gives rtol
 * and atol, the step sizes are found.  An error-controlled step costs no solve and no f_R beyond crd_step_imex's.
 * The pair.  One weight vector for both parts, bhat = (0, 5/2, 0, -3/2, 0):
 *   yhat = y_n + dt [ 5/2 (FR_1 + k_1) - 3/2 (FR_3 + k_3) ]
 * of order 2 (sum bhat = 1, bhat.c = 1/2; both matrices have row sums c), not of order 3 (bhat.c^2 = 1/4), damped at infinity
 * (1 - bhat_I^T A_I^-1 e = 0 on the implicit 4 x 4 block), and without FR_4.  The estimate is e = y_{n+1} - yhat
 *   e = dt sum_{j=0..3} dE_j FR_j + dt sum_{j=1..4} dI_j k_j,   dE = (1/4, -3/4, 3/4, -1/4),   dI = (-1, -3/2, 2, 1/2),
 * formed per real in the context's precision with dt dE_j and dt dI_j rounded as the step's coefficients are: the FIRST term one rounded
 * product, every further term one fma, in the order FR_0, FR_1, k_1, FR_2, k_2, FR_3, k_3, k_4 (j ascending, explicit before implicit;
 * a term whose coefficient is exactly zero is skipped).
 * CRD_IMEX_EULER and CRD_IMEX_ARS222 have no estimate and are refused: the only first-order implicit weights of ARS(2,2,2) that are
 * damped at infinity are b_I itself, and an estimate built on them is blind to the diffusion error (identically zero with justDiffusion).
 * The norm.  w = rtol |y_n| + atol per real of the step's START y_n (ARKode's ewt), q = ((double)e / w)^2, every operation in double
 * and rounded once; norm = sqrt(sum q / (2 nx ny)) over var0 and var1 of every point.  The sum is left by the kernel that closes the
 * last stage (crd_imex.hip), reduced in a fixed order without atomics: the bits repeat.  The host reads two doubles per attempt, the
 * sum and max |var0| of the new state.
 * An attempt from t_n of size h is crd_step_imex's own code and launches up to the last solve; an ACCEPTED step (norm <= 1) leaves the
 * bits crd_step_imex(ctx, t_n, h, 1, &opt->imex) leaves -- with CRD_IMEX_SOLVER_BICGSTAB_WARM too, every attempt starting its first
 * solve from x = 0 as a call of one step does.  A REJECTED attempt (norm > 1, or a norm or max |var0| that is not finite) leaves y_n
 * untouched and is repeated with a smaller step.
 * The controller is crd_integrate_adaptive's CRD_ADAPT_ARKODE controller (PID gains 0.58 / 0.21 / 0.1, no change of h for a suggested
 * growth within [1, 1.5], 0.3 from the second failure of a step on, CRD_ESTATE on the 7th) with the embedding order 2 in its exponents;
 * the controller sees bias x norm.  h0 > 0 is the first step; h0 = 0 starts from crd_stable_dt; either way the first step may grow by
 * 10000, later ones by `growth`.  h_max > 0 caps the step, h_max <= 0 means no cap: the diffusion bound means nothing here and the
 * explicit kinetics' limit is found by the error test.  The last step is shortened to land on tout (a step that would leave less than
 * 1e-12 |tout| is stretched to it); there is no dense output.  max_steps bounds the ATTEMPTS of a call, rejected ones included.
 * Steps are NOT clipped at tBoundary: the held rows are those of each stage's own time, and a step across it that is inaccurate is met
 * by rejecting it.  No controller memory is kept between calls: stats.h_next is what the caller passes as the next call's h0.
 * A solve that does not converge ends the call with CRD_ESTATE exactly as in crd_step_imex; so do max_steps attempts short of tout, a
 * step size below 1e-14 |t| and the 7th failure.  The resident state is then that of the last accepted step, and stats says where.
 * Refused before any device work: what crd_step_imex refuses; CRD_EINVAL for a scheme other than CRD_IMEX_ARS443, rtol or atol negative
 * or not finite or both zero, tout < t0 or either not finite, h0 < 0, h_max NaN, safety <= 0, bias <= 0, growth < 1, shrink outside
 * (0, 1), max_steps < 1, history_cap < 0 or history == NULL with history_cap > 0.  opt == NULL: crd_imex_adaptive_defaults.
 * Workspace: crd_step_imex's, as crd_imex_info reports it with opt->imex (the sum's partials lie in the vector of the solve's
 * right-hand side, free at the last close).
 * stats (may be NULL): imex = crd_step_imex's figures over every attempt (steps = accepted; failed_step counts attempts); accepted,
 * rejected, attempts; h_first = the first attempt's size; h_last, h_min, h_max = the last, smallest, largest accepted step; err_last = bias x norm of
 * the last attempt; t = the time reached (tout on success); h_next; recorded = records written to history.
 * history (may be NULL with history_cap 0): one record per attempt in order -- t_n, h, err = bias x norm, accepted 0 / 1, iterations
 * of the attempt's solves.  When history_cap runs out the call goes on; stats.attempts says how many there were. */
typedef struct crd_imex_adaptive_options {
	crd_imex_options imex;  /* crd_imex_defaults with scheme CRD_IMEX_ARS443 */
	double rtol, atol;      /* 1e-5, 1e-10 */
	double h0;              /* first step; 0 = crd_stable_dt */
	double h_max;           /* > 0: cap; <= 0 (default 0): none */
	double safety, bias, growth, shrink; /* 0.96, 1.5, 20, 0.1: crd_adaptive_options' */
	int64_t max_steps;      /* 200000 attempts */
} crd_imex_adaptive_options;
typedef struct crd_imex_adaptive_stats {
	crd_imex_stats imex;
	int64_t accepted, rejected, attempts, recorded;
	double h_first, h_last, h_next, h_min, h_max, err_last, t;
} crd_imex_adaptive_stats;
typedef struct crd_imex_attempt {
	double t, h, err;
	int32_t accepted, iterations;
} crd_imex_attempt;
int crd_imex_adaptive_defaults(crd_imex_adaptive_options *opt);
int crd_integrate_imex(crd_ctx *ctx, double t0, double tout, const crd_imex_adaptive_options *opt, crd_imex_adaptive_stats *stats, crd_imex_attempt *history,
                       int64_t history_cap);
/* For the test suite's gate on the estimating close alone: runs it once on HOST vectors in the context's precision given back to back in
 * `in` -- R_s, k_s, y_n, then the stored vectors in the estimate's order FR_0, FR_1, k_1, FR_2, k_2, FR_3, k_3 -- with
 * scalars = {hg, dt, rtol, atol}, hg rounded to the context's precision and the coefficients formed from dt as an attempt forms them.
 * out: the new state and e back to back; result: {sum of q, max |var0| of the new state}.  Uses crd_step_imex's workspace. */
int crd_imex_estimate_probe(crd_ctx *ctx, const double *scalars, const void *in, void *out, double *result);

/* The exchange period E of the one-launch stepper on several slabs: E steps between two halo exchanges, each of 4 E ghost rows
 * of both fields; in between every slab recomputes the shrinking ghost region redundantly (same kernel, same inputs: bit-identical
 * to what the owner computes).  3 <= E <= 16; default 10 where every slab of the run has 256 rows or more, else 8.  A property of the RUN: every context of a LOCAL group / every rank of a
 * ring must be given the same value before its next stepping call (which then starts with an exchange).  A longer period halves the
 * per-step share of a cycle's fixed cost (two small launches, two cross-stream waits) and of the exchange's latency for a few per
 * cent more redundant rows; bench.py rehearses 8 and 16 on the machine at hand.  Slabs shorter than 4 E rows step with the staged
 * kernels.  Replaces nothing in the reference: its Exchange() runs inside every f() (src/FHNmodel_torus.cpp:521). */
int crd_set_exchange_period(crd_ctx *ctx, int steps);
int crd_get_exchange_period(const crd_ctx *ctx);
int crd_synchronize(crd_ctx *ctx);

/* Error-controlled integration from t0 to exactly tout on the resident state: replaces what the reference gets from
 * ARKodeSStolerances(rtol, atol) + ARKode(..., tout, ..., ARK_NORMAL) (src/FHNmodel_torus.cpp:365,423).  The propagated
 * solution is classical RK4 (the same one-launch step kernel as crd_step_rk4); a fifth evaluation k5 = f(t+h, y_new) gives
 * the embedded third-order solution y + h (k1/6 + k2/3 + k3/3 + k5/6) and the local error estimate h (k4 - k5)/6, measured
 * in ARKode's WRMS norm with weights 1 / (rtol |y_n| + atol); a step is accepted when bias * norm <= 1 and the next step
 * is safety * h * (bias * norm)^(-1/4), growth-limited (constants in crd_adaptive_options; defaults are ARKode's).
 * Not ARKode's step sequence: its method table and controller are not in the reference tree.
 * Output times: with dense_output = 0 the last step is shortened to land on tout.  With dense_output = 1 the call does what
 * ARK_NORMAL does (src/FHNmodel_torus.cpp:423): steps are never shortened for an output time; the integrator steps until it has
 * reached or passed tout, the state handed back (crd_state_download, the writers) is the cubic Hermite interpolant of the last
 * step at tout, built from y_n, y_{n+1}, f(t_n, y_n), f(t_{n+1}, y_{n+1}) (ARKode's default dense output is of degree 3 too), and
 * the integrator's own state stays at its internal time (stats.t_internal >= tout): the next call with t0 equal to this call's
 * tout continues from there.  Any other call that changes the state (upload, fixed-step stepping, a different t0) drops it.
 * Multi-slab runs exchange 60 ghost rows of the state every twelve
 * accepted steps (each attempt also produces the ghost-region rows its input still covers: the fixed stepper's deep halo, by
 * attempts) and reduce the norm of the OWNED rows over the ring (ncclAllReduce; LOCAL groups add the slabs' sums on the host in
 * slab order), so every rank takes the same decisions.  h0 = 0 starts from the diffusion-stability step; by default steps are
 * also capped at that bound (h_max = 0), which removes the reject / regrow cycle of a stability-limited explicit method. */
/* Which embedded pair and controller crd_integrate_adaptive runs. */
enum {
	CRD_ADAPT_RK43 = 0,   /* rounds 1-2: classical RK4 + k5 = f(t+h, y_new) as third-order embedding, I-controller; steps may be shortened to
	                       * land on tout (dense_output = 0) */
	CRD_ADAPT_ARKODE = 1  /* the integrator the reference uses (src/FHNmodel_torus.cpp:356-372): SUNDIALS ARKode's default explicit
	                       * fourth-order table, Zonneveld 5(3)4 -- whose propagated solution is classical RK4 too -- with ARKode's PID
	                       * controller, its safeguards, its initial-step estimate and ARK_NORMAL output (dense_output is taken as 1).
	                       * Restated from ARKode's published documentation (the library is not in the reference tree): the algorithm
	                       * and every constant are written out in oracle/arkode_erk.py.  The controller's memory (step, error history)
	                       * lives in the context and carries from call to call like ARKode's does, until the state is replaced. */
};

typedef struct crd_adaptive_options {
	double rtol, atol;      /* 1e-5, 1e-10 in the reference (src/FHNmodel_torus.cpp:197-198) */
	double h0;              /* first step; 0 = automatic */
	double safety;          /* 0.96 */
	double bias;            /* 1.5 */
	double growth;          /* 20: largest h_new / h */
	double shrink;          /* 0.1: smallest h_new / h */
	int64_t max_steps;      /* 200000 attempts (ARKodeSetMaxNumSteps, :372) */
	double h_max;           /* largest step: > 0 explicit cap (ARKodeSetMaxStep); 0 = the classical-RK4 stability bound of the
	                         * diffusion operator, crd_stable_dt (what ARKodeSetStabilityFn is for: beyond it the error test
	                         * only finds out by failing); < 0 = no cap, error control alone (ARKode's default) */
	int32_t dense_output;   /* 0: shorten the last step to hit tout; 1: ARK_NORMAL -- overshoot and interpolate back (see above) */
	int32_t method;         /* CRD_ADAPT_*; crd_adaptive_defaults: CRD_ADAPT_ARKODE with dense_output = 1.  Under CRD_ADAPT_ARKODE h0 = 0 means
	                         * ARKode's own estimate (arkHin) on a fresh state, safety / bias / growth / shrink are ARKode's constants of the
	                         * same names (shrink = ETAMIN), and the remaining ones (PID gains 0.58 / 0.21 / 0.1 over the embedding order 3,
	                         * first-step growth 10000, 0.3 after repeated failures, at most 7 failures per step, no change of h for a
	                         * suggested growth within [1, 1.5]) are fixed */
} crd_adaptive_options;
typedef struct crd_adaptive_stats {
	int64_t accepted, rejected;
	double h_last;          /* size of the last accepted step that was not shortened to hit tout */
	double h_next;          /* controller's suggestion for the next call */
	double h_min, h_max;    /* over accepted steps */
	double err_last;        /* bias * WRMS norm of the last attempt */
	double t;               /* time of the state handed back (== tout on success) */
	double t_internal;      /* time the integrator itself has reached: == t without dense output, >= t with it */
	double h_first;         /* size of the first step this call attempted (on a fresh state under CRD_ADAPT_ARKODE: the arkHin estimate) */
	int64_t launched_ahead; /* attempts that were already running when their predecessor's error norm arrived (CRD_ADAPT_ARKODE launches the next
	                         * step ahead of the verdict, assuming "accepted, same size"; a wrong guess costs one discarded launch) */
} crd_adaptive_stats;
int crd_adaptive_defaults(crd_adaptive_options *opt);
int crd_integrate_adaptive(crd_ctx *ctx, double t0, double tout, const crd_adaptive_options *opt, crd_adaptive_stats *stats);
int crd_group_integrate_adaptive(crd_ctx *const *ctxs, int n, double t0, double tout, const crd_adaptive_options *opt,
                                 crd_adaptive_stats *stats); /* LOCAL groups */

/* LOCAL groups (several slabs driven by one host thread): the same two operations on every slab of the run in
 * lockstep; ctxs[k] must be slab k of n.  y[k] / ydot[k] are device pointers on ctxs[k]'s device. */
int crd_group_step_rk4(crd_ctx *const *ctxs, int n, double t0, double dt, int64_t nsteps);
/* ... with the clocks of crd_step_rk4_timed (below) on every slab: device time of the batch and the duration of one full-height
 * launch of the dominant kernel per context; crd_get_step_timing(ctxs[k]) returns slab k's figures.  Returns when every slab's last
 * step is done. */
int crd_group_step_rk4_timed(crd_ctx *const *ctxs, int n, double t0, double dt, int64_t nsteps);
/* Host threads that issue a group's work in crd_group_step_rk4: 0 (default) = one per device the group is spread over, k >= 1 =
 * exactly k (contiguous runs of slabs per thread; k = 1: the calling thread alone).  The threads meet at a host rendezvous around
 * every halo exchange; results do not depend on k. */
int crd_group_set_threads(crd_ctx *const *ctxs, int n, int threads);
int crd_group_rhs_device(crd_ctx *const *ctxs, int n, double t, const void *const *y_aos_dev, void *const *ydot_aos_dev);
int crd_group_rhs_host(crd_ctx *const *ctxs, int n, double t, const void *const *y_aos, void *const *ydot_aos); /* host vectors, device precision */
/* ... and the parts of f and J v (crd_rhs_part_* / crd_jtimes_* above) on every slab of a LOCAL group */
int crd_group_rhs_part_device(crd_ctx *const *ctxs, int n, double t, int part, const void *const *y_aos_dev, void *const *ydot_aos_dev);
int crd_group_rhs_part_host(crd_ctx *const *ctxs, int n, double t, int part, const void *const *y_aos, void *const *ydot_aos);
int crd_group_jtimes_device(crd_ctx *const *ctxs, int n, double t, int part, const void *const *y_aos_dev, const void *const *v_aos_dev,
                            void *const *jv_aos_dev);
int crd_group_jtimes_host(crd_ctx *const *ctxs, int n, double t, int part, const void *const *y_aos, const void *const *v_aos, void *const *jv_aos);

/* Same as crd_step_rk4 but bracketed by HIP events on the context's compute stream; blocks until done.
 * ms_total: device time of the whole batch; kernel_ms: average duration of one launch of the dominant kernel
 * (the fused step kernel, or the stage-2/3 kernel of the staged stepper), measured by per-launch events on a
 * subset of the steps; launches: how many launches of that kernel one step makes. */
int crd_step_rk4_timed(crd_ctx *ctx, double t0, double dt, int64_t nsteps, double *ms_total, double *kernel_ms,
                       int *launches_per_step);

/* What the last crd_step_rk4_timed call measured, plus -- after crd_set_diagnostics(ctx, 1), on an RCCL context stepping with the
 * one-launch kernel -- two figures per deep-halo exchange of that call: how long the compute stream stood at its wait for the
 * halo (event pair around the wait; a few microseconds of queue latency when the exchange hid under the sweeps it is given, the
 * exposed remainder when it did not), and how long the exchange itself took on the second stream (from "its rows are ready" to
 * "last byte landed").  Replaces nothing in the reference: its Exchange() is eight blocking MPI_Waits inside f()
 * (src/FHNmodel_torus.cpp:904-946), all of it exposed.  Diagnostics put event records between sweeps that otherwise run back to
 * back; leave them off in runs whose rate is being measured. */
typedef struct crd_step_timing {
	double ms_total;            /* device time of the batch */
	double kernel_ms;           /* average duration of the timed launches of the dominant kernel */
	double exposed_halo_ms;     /* sum over halo_waits */
	double exchange_ms;         /* sum over exchanges */
	int64_t steps;
	int32_t halo_slack;         /* crd_set_halo_slack at the time of the call */
	int32_t timed_steps_per_launch; /* RK4 steps one of the timed launches advanced: 1, or 2 (a two-steps-per-launch plan); 0: none timed */
	int32_t halo_waits;         /* waits measured (at most 64 per call) */
	int32_t exchanges;          /* exchanges measured */
	int64_t agreement_restarts; /* stepping calls of this context that started afresh with an exchange because the ring's ranks stood
	                             * at different positions of the exchange cycle (see crd_step_rk4) */
} crd_step_timing;
int crd_set_diagnostics(crd_ctx *ctx, int on);
/* How many sweeps of rows that read owned rows only the one-launch stepper puts between an exchange and its wait for the halo:
 * 1 (default) splits the first step of an exchange cycle, 2 the first two -- one more small launch per cycle for a third sweep
 * of cover, for links on which the exchange does not land within two (exposed_halo_ms says so).  A rank-local choice: it moves
 * the point where THIS rank consumes its halo, not the exchange; results are bit-identical either way. */
int crd_set_halo_slack(crd_ctx *ctx, int sweeps);
int crd_get_step_timing(const crd_ctx *ctx, crd_step_timing *out);

/* Rows of the slab one timed launch of the dominant kernel covers (all of them for a single slab; the interior, i.e. all
 * but the edge rows / bands that are launched separately ahead of the halo exchange, for a multi-slab context). */
int crd_dominant_kernel_rows(const crd_ctx *ctx, int64_t *rows);

/* Name of the dominant kernel as it appears in a rocprofv3 kernel trace (static string). */
const char *crd_dominant_kernel_name(const crd_ctx *ctx);

/* Launch plan of the one-launch step kernel.  How a slab is cut into work items (32-row chunks, or chunks stretched so that
 * every workgroup is resident at once), how the items are dealt to the 8 XCDs, how many columns a lane steps and how the new
 * state is stored is measured on the device at hand, on the
 * context's first full-size step (a handful of extra launches of that step; every plan computes bit-identical results), unless
 * autotuning is off (crd_set_autotune(ctx, 0) or CRD_AUTOTUNE=0 in the environment): launches then take 32-row chunks in dispatch
 * order, plain stores and the default columns per lane of their precision (fp32 on an even nx: two; crd_get_launch_plan reports
 * it).  crd_set_autotune(ctx, 2) / CRD_AUTOTUNE=2 also prints every candidate's timing to stderr.  No reference counterpart: a
 * property of this implementation. */
typedef struct crd_launch_plan {
	int32_t autotune;     /* measuring enabled (2: verbose) */
	int32_t tuned;        /* a measurement has been made (or a plan pinned) */
	int32_t one_round;    /* chunk mode: 0 = 32-row chunks, 1 = stretched so that all workgroups are resident at once, 2 = 64-row chunks,
	                       * 3 = as 1 with eight wavefronts per block strip (the three-step fp64 FHN kernel; reported as 1 where that kernel does not run) */
	int32_t xcd_mapping;  /* 0 theta-first dispatch order, 1 one contiguous band of the slab per XCD, 2 the same with succession in phi */
	int32_t rows;         /* height of the launch it was measured on */
	int32_t columns_per_lane; /* 1: a wavefront steps a strip of 64 columns (56 valid); 2: 128 columns (120 valid), two per lane -- packed
	                           * arithmetic in fp32 */
	int32_t nontemporal_stores; /* 1: the new state is written with the non-temporal hint (it is not read again by the launch, and
	                             * does not displace from L2 what neighbouring work items share) */
	int32_t steps_per_launch; /* 1; 2: one launch advances the state by TWO RK4 steps (the state crosses memory once per two steps, for twice
	                           * the pipeline registers and a 16-row / 16-column apron); crd_step_rk4 then issues pairs; 3 (FHN: in fp64 on a
	                           * single slab, a block's wavefronts running as one strip with one column per lane; in fp32 -- an even nx --
	                           * with two columns per lane and a strip per wavefront, single slabs and the slabs of a run inside their
	                           * exchange cycles; elsewhere taken as 2): THREE steps; triples, then a pair or a single step for what is
	                           * left (fp32: also for triples any stage of which has the absorbing rows on).  What crd_get_launch_plan
	                           * reports -- steps and columns -- is what a launch does. */
	double ms_default, ms_chosen; /* measured times PER STEP: plain plan, chosen plan */
} crd_launch_plan;
int crd_set_autotune(crd_ctx *ctx, int on);
int crd_get_launch_plan(const crd_ctx *ctx, crd_launch_plan *out);
/* What the context's full-height launch of the step kernel looks like under its current plan, and what the assembler printed about
 * the instantiation it runs (read off the device assembly when the library was built: tools/kernel_regs.py) -- enough to price the
 * launch's vector issue without a profiler: loop_valu x (wavefront_iterations / iterations_per_trip) x 4 cycles per wavefront
 * instruction over simds x clock (bench.py: roofline.issue_frac).  No reference counterpart. */
typedef struct crd_launch_geometry {
	int32_t rows;                      /* rows the launch produces (a multi-slab context: the launch the timed calls time) */
	int32_t strips, chunk_rows, chunks; /* work items: strips of columns (one per wavefront) x chunks of rows */
	int32_t workgroups, wavefronts_per_workgroup;
	int32_t fill_iterations;           /* pipeline iterations an item runs beyond its rows (the aprons in phi) */
	int32_t iterations_per_trip;       /* pipeline iterations one trip of the steady-state loop holds (its unroll factor) */
	int32_t lanes, lanes_valid;        /* lanes of a wavefront / lanes whose column is an output (kernels that put one apron around a
	                                    * workgroup's wavefronts -- Goldbeter fp64, two steps per launch -- : the workgroup's average, 60) */
	int32_t vgprs, sgprs, lds_bytes, scratch_bytes, wavefronts_per_simd; /* of the instantiation; 0: the build carries no kernel table */
	int32_t loop_valu, loop_salu, loop_vmem, loop_lds, loop_instructions; /* static instruction mix of one trip of that loop */
	int32_t simds, clock_khz;          /* of the device: 4 x compute units, hipDeviceProp_t::clockRate */
	int32_t exec_skipped_vmem;         /* vector-memory regions of that kernel a wavefront can skip on its execution mask (device assembly,
	                                    * tools/kernel_regs.py).  The multi-step kernels wait for their LDS-DMA row fills with hand-counted
	                                    * s_waitcnt vmcnt(N); N counts the iteration's stores, which therefore must issue whatever the mask:
	                                    * 0 for every such kernel, or the build stops */
	int64_t wavefront_iterations;      /* pipeline iterations all wavefronts of the launch run: strips x (rows + chunks x fill_iterations) */
	int64_t wavefront_iterations_effective; /* ... with an item's filling iterations at what they cost: stage k of the pipeline starts at
	                                    * iteration 2 k, so the fill runs fill_iterations / 2 - 1 iterations' worth of stages */
} crd_launch_geometry;
int crd_get_launch_geometry(crd_ctx *ctx, crd_launch_geometry *out);
/* The plans the measurement chooses among, index 0 .. (first index that returns CRD_EINVAL) - 1: one_round, xcd_mapping,
 * columns_per_lane, nontemporal_stores and steps_per_launch of *out are set, the rest zero.  (tools/plan_sweep.py profiles every one of them;
 * tests/test_profiles.py checks that profiles/pmc_traffic.json has an entry for each.) */
int crd_launch_plan_candidate(int index, crd_launch_plan *out);
/* Steps per launch a plan that asks for `steps_wanted` (1..3) gets on a slab of nx x nyl points -- what crd_get_launch_plan reports as
 * steps_per_launch for a context of that shape -- without a context or a device (single_slab: phi wraps inside the slab).  The
 * three-step fp64 kernel addresses a plane's rows by 32-bit byte offsets: crd_rows_addressable says whether `rows` rows of nx reals
 * (the slab's rows, and its ghost rows where it has them) fit -- rows x nx x real_bytes below 2^32 minus one row; beyond that such a
 * plan steps pairs.  crd_steps_per_launch_on: CRD_EINVAL (negative) for arguments out of range.  No reference counterpart. */
int crd_steps_per_launch_on(int model, int precision, int64_t nx, int64_t nyl, int single_slab, int steps_wanted);
int crd_rows_addressable(int64_t nx, int64_t rows, int real_bytes);
/* Use THIS plan (chunk mode 0..2, or 3 together with three steps per launch; mapping 0..2, columns per lane 1..2, non-temporal stores 0..1, steps per launch 1..3) for the fixed-step kernel instead of measuring one -- a plan
 * read back from an earlier context of the same shape on the same device (the measurement costs ~0.45 s per context at 8192^2), or
 * a profiling run in which every launch of the kernel should be the plan a previous run chose (`bench.py --launch-plan`).  A pinned
 * plan applies to launches of EVERY size (a measured one only to launches of the height it was measured on).  Where a choice cannot
 * be honoured (two columns per lane on an odd nx, mapping 2 on a launch too short for it) the launch falls back as it would for a
 * measured plan.  crd_get_launch_plan then reports tuned = 1 with both times 0.  CRD_EINVAL outside the ranges. */
int crd_set_launch_plan(crd_ctx *ctx, int chunk_mode, int xcd_mapping, int columns_per_lane, int nontemporal_stores, int steps_per_launch);
/* Measure the plan NOW (a step of the resident state into scratch planes, discarded; the state is not advanced) instead of
 * inside the first crd_step_rk4 -- for callers that time their first steps; also creates the events crd_step_rk4_timed uses.  The
 * measurement is skipped when a plan exists or autotuning is off. */
int crd_plan_launches(crd_ctx *ctx);

/* Named ranges for a profiler's timeline (roctx: `rocprofv3 --marker-trace`), SURVEY section 5.  libcrd puts its own around
 * step batches (crd_step_rk4 ...), halo exchanges, state transfers and output rows; a host program brackets its phases with
 * these two (crd_run: one range per output interval, where the reference prints its progress line, src/FHNmodel_torus.cpp:
 * 457-477).  No-ops unless a profiler is attached (ROCP_TOOL_LIBRARIES in the environment) or CRD_ROCTX=1; the marker library
 * is bound with dlopen on first use, never linked. */
void crd_trace_range_push(const char *name);
void crd_trace_range_pop(void);

/* max |var0| over the slab (blow-up guard; synchronises). */
int crd_state_max_abs(crd_ctx *ctx, double *out);

/* ---------------------------------------------------------------------------------------------------------
 * Ensembles: B independent single-slab problems stepped together, one launch per RK4 step for all of them -- what a parameter
 * scan of the reference does with B separate runs (`mpirun ... FHNmodel_torus <ini>` once per value, src/FHNmodel_torus.cpp:148-497),
 * each with its own ARKode stepping loop.  On the reference's own small grids (data/FHNmodelArgs.ini: 400 x 1600) one problem's step
 * is bound by the launch, not by the device; B members share that launch.  Members of crd_ensemble_create must agree on model,
 * surface, nx, the derived ny, surface length and width, precision and justDiffusion; they may differ in diffusion, beta, betaMin,
 * betaMax, varyBeta and tBoundary.  Members of crd_ensemble_create_mixed must agree on model, precision and justDiffusion only: the
 * reference's own scan -- torus 80/20 against torus 40/20 against the flat control (data/FHNmodelArgs.ini: surfaceLength "80 for
 * normal, 40 for more curved surface") -- in one ensemble; every size below is then the member's own.  One device.  Fixed-step classical RK4 (crd_ensemble_step_rk4): every member's result is bit-identical to a context
 * (crd_create) of the same parameters stepped alone with crd_step_rk4 and the one-launch stepper.  Error-controlled integration
 * (crd_ensemble_integrate_adaptive): every member takes its own step sequence, as a context of its parameters integrated alone with
 * crd_integrate_adaptive would.  Not thread-safe; calls on one ensemble must be serialised.
 * --------------------------------------------------------------------------------------------------------- */
typedef struct crd_ensemble crd_ensemble;
/* members[0 .. n_members): the members' parameters.  Refusals come before any HIP call: CRD_EINVAL for n_members < 1, invalid
 * parameters or members that disagree where they must agree (crd_ensemble_last_error(NULL) names the first such member and field);
 * CRD_EHIP without a device.  Each member owns two state buffers of its own (no ghost rows, none of a context's other planes); the
 * state starts at zero.  Replaces InitUserData + SetupDecomp of B single-rank runs (src/FHNmodel_torus.cpp:708-772). */
int crd_ensemble_create(const crd_params *members, int n_members, int device, crd_ensemble **out);
/* crd_ensemble_create for members that may also differ in surface, nx, ny, surface length and surface width (they must agree on model,
 * precision and justDiffusion).  Refused before any HIP call, crd_ensemble_last_error(NULL) naming the member and the field: such a
 * disagreement, a member of fewer than 8 rows, block ids of all members together overflowing 32 bits; CRD_EHIP without a device.
 * Members that all share nx and ny (torus and flat at one mesh, lengths with ny pinned) make an ordinary ensemble: it launches exactly
 * what crd_ensemble_create's launches and keeps every call below.  Members of different shape step with crd_ensemble_step_rk4 /
 * _timed at one or two steps per launch -- a block finds its member by a scalar search of a per-member table of shapes; one chunk height
 * and block size per launch, a fixed rule of the shapes, precision, model and member order -- and take the basic observer
 * (crd_ensemble_observe_begin: statistics, probes, maps); every member's state, statistics row, probe values and maps stay bit-identical
 * to the same problem alone.  They refuse, with CRD_EINVAL and "members of different shape" in crd_ensemble_last_error, and nothing
 * opened or allocated: crd_ensemble_integrate_adaptive, and crd_ensemble_observe_begin_with with any section or with cycles. */
int crd_ensemble_create_mixed(const crd_params *members, int n_members, int device, crd_ensemble **out);
void crd_ensemble_destroy(crd_ensemble *e);
const char *crd_ensemble_last_error(const crd_ensemble *e); /* never NULL; e may be NULL (creation errors) */
/* Member count and the members' common grid (crd_ensemble_create_mixed: member 0's).  Either pointer may be NULL. */
int crd_ensemble_info(const crd_ensemble *e, int *n_members, crd_grid *g);
/* Member `member`'s own grid.  CRD_EINVAL for a null pointer or an index out of range. */
int crd_ensemble_member_grid(const crd_ensemble *e, int member, crd_grid *g);
/* State of ONE member in the boundary layout (AoS, the member's ny * nx pairs; host_is_f64 as crd_state_upload).  Synchronous; other members'
 * states are not touched.  Stands in for the initial-condition upload of that member's run (src/FHNmodel_torus.cpp:285-354). */
int crd_ensemble_upload(crd_ensemble *e, int member, const void *y_aos_host, int host_is_f64);
int crd_ensemble_download(crd_ensemble *e, int member, void *y_aos_host, int host_is_f64);
/* nsteps classical RK4 steps of size dt on EVERY member, stage k of step n at t0 + n dt + c_k dt (the same times crd_step_rk4 forms);
 * each member's absorbing rows follow its own tBoundary.  One launch per step.  Asynchronous on the ensemble's own stream
 * (crd_ensemble_synchronize waits).  Replaces the members' ARKode(...) calls (src/FHNmodel_torus.cpp:423), one per member. */
int crd_ensemble_step_rk4(crd_ensemble *e, double t0, double dt, int64_t nsteps);
/* ... bracketed by events on the ensemble's stream; blocks until done; ms_total: device time of the batch. */
int crd_ensemble_step_rk4_timed(crd_ensemble *e, double t0, double dt, int64_t nsteps, double *ms_total);
int crd_ensemble_synchronize(crd_ensemble *e);
/* RK4 steps one launch of crd_ensemble_step_rk4 takes: 1 (the default) or 2.  With 2, a call steps PAIRS from its start -- both steps
 * of every member in one launch, the state across memory once per two steps -- and a single step for an odd remainder; with an observer
 * open a pair never straddles a sample (the step that completes a stride is taken alone).  Results, samples and sample times are those
 * of single steps bit for bit: a pair is the sequence of two single steps per point.  The two-step pipeline needs room in phi (an item
 * touches its rows and 16 apron rows, fewer than 2 ny in all): CRD_EINVAL for steps = 2 on members of fewer than
 * CRD_ENSEMBLE_PAIR_MIN_ROWS rows (members of different shape: any member, named), and for any steps other than 1 or 2 (crd_ensemble_last_error says which); the setting is then
 * unchanged.  The first call with 2 plans the pair launches (a fixed rule of grid, precision, model and member count).  A library built
 * without the build-time check of the pair kernels' assembly (make KERNEL_TABLE=0) carries no pair kernels and refuses 2 likewise.
 * crd_ensemble_integrate_adaptive takes attempts, not steps, and is not affected. */
#define CRD_ENSEMBLE_PAIR_MIN_ROWS 9
int crd_ensemble_set_steps_per_launch(crd_ensemble *e, int steps);
int crd_ensemble_get_steps_per_launch(const crd_ensemble *e); /* 1 or 2; CRD_EINVAL (negative) for NULL */
/* Every member at its OWN step size to a common time: member k goes from t0 to t1 in nsteps[k] classical RK4 steps of
 * dt_k = (t1 - t0) / nsteps[k] -- what crd_step_rk4(ctx_k, t0, dt_k, nsteps[k]) does to a lone one-launch context of member k's
 * parameters, bit for bit, stage q of its step s at (t0 + s dt_k) + c_q dt_k and its absorbing rows on while that time is < its own
 * tBoundary.  Rounds: round s is ONE launch for all members with nsteps[k] > s, so the launches shrink as members finish (the set
 * need not stay a prefix of the member list); which rounds a member steps in moves no bit.  A scan over diffusion, or of curved
 * against flat surfaces, then costs the sum of the members' own work instead of every member stepping at the smallest member's bound.
 * Serves ensembles of crd_ensemble_create and of crd_ensemble_create_mixed (members of different shape included).  Asynchronous on
 * the ensemble's stream.  Afterwards every call above and below finds each member's state where it expects it (a member that took an
 * odd number of steps has its two buffers re-labelled; nothing is copied); as crd_ensemble_step_rk4, the call ends every member's
 * error-controlled carry-over.
 *   Steps per launch: the call takes single steps whatever crd_ensemble_set_steps_per_launch says; the setting keeps governing
 *   crd_ensemble_step_rk4.
 *   Observer: with one open the call records ONE sample at its end, at time t1, of every member (crd_ensemble_integrate_adaptive's
 *   rule); the stride's count of fixed steps does not move.  A call for which there is no room is refused whole.
 * CRD_EINVAL, crd_ensemble_last_error naming the cause (and the member where there is one), nothing launched and the ensemble as it
 * was: a NULL argument, a non-finite t0 or t1, t1 <= t0, any nsteps[k] < 1.  A HIP failure while the rounds are being launched
 * (CRD_EHIP) leaves the members at different times: each has taken the steps of the rounds launched, its descriptor names that
 * state, and crd_ensemble_last_error says how many rounds those were; upload every member before stepping on. */
int crd_ensemble_step_rk4_own(crd_ensemble *e, double t0, double t1, const int64_t *nsteps);
/* ... with member k's step size GIVEN, dt[k], instead of formed from t1: what crd_step_rk4(ctx_k, t0, dt[k], nsteps[k]) does, bit for
 * bit; t1 is the time of the observer's sample and nothing else.  For a caller whose interval is not a machine number apart from t0
 * (the driver's t + dTout: (t + dTout) - t need not be dTout, and a lone run steps at dTout / n exactly).  Refusals as above, and for
 * a dt[k] that is not positive and finite. */
int crd_ensemble_step_rk4_own_dt(crd_ensemble *e, double t0, double t1, const double *dt, const int64_t *nsteps);
/* crd_ensemble_step_rk4_own bracketed by events on the ensemble's stream, as crd_ensemble_step_rk4_timed: blocks until done;
 * ms_total: device time of all rounds, the table copies between them and -- an observer open -- the sample. */
int crd_ensemble_step_rk4_own_timed(crd_ensemble *e, double t0, double t1, const int64_t *nsteps, double *ms_total);
/* The driver's rule for those counts, per member: nsteps[k] = ceil((t1 - t0) / (dt_safety * crd_stable_dt(member k)) - 1e-12), at
 * least 1 -- the steps a lone run of member k's ini takes over one output interval.  No device work.  CRD_EINVAL for a NULL argument,
 * a non-finite t0 or t1, t1 <= t0, or a dt_safety that is not positive and finite. */
int crd_ensemble_own_steps(const crd_ensemble *e, double t0, double t1, double dt_safety, int64_t *nsteps);
/* max |var0| of every member, per_member[0 .. n_members) (non-finite for a member that blew up; synchronises).  The blow-up guard of
 * each member's run (its ARKode call's failure, src/FHNmodel_torus.cpp:424-435). */
int crd_ensemble_max_abs(crd_ensemble *e, double *per_member);
/* Error-controlled integration of EVERY member from t0 to tout: member k integrates exactly as crd_integrate_adaptive would on a lone
 * single-slab context of member k's parameters and state -- CRD_ADAPT_ARKODE with ARK_NORMAL dense output, arkHin on a fresh state,
 * the PID controller and its safeguards, the 7-failure limit, max_steps and the step-size underflow check -- with its own step size,
 * accept / reject sequence, controller memory and stats.  With h_max = 0 each member is capped at its own crd_stable_dt.  Replaces
 * the members' ARKode(..., tout, ..., ARK_NORMAL) calls (src/FHNmodel_torus.cpp:423), one per member.
 *   Rounds: one launch runs one attempt of every member still short of tout, one wait brings back all their error norms, and each
 *   member's controller decides on its own.  A member's error norm is summed over the ensemble's fixed partition of work items (planned
 *   at the first call from the member count), not a context's: its step sizes agree with a lone context's to rounding (~1e-15), and a
 *   member's result does not depend on the other members or on when they finish.  Repeated calls are bit-identical.
 *   Resume: member k continues from its internal state when t0 is the tout its previous call handed back and nothing has replaced its
 *   state since; crd_ensemble_upload(e, k, ...) ends member k's carry-over only, crd_ensemble_step_rk4 every member's.
 *   Failures stay per member: a member that fails the error test 7 times on one step, takes max_steps steps or underflows its step
 *   size stops alone (status[k] = CRD_ESTATE; its state is left where crd_integrate_adaptive leaves a context), the others reach tout,
 *   and the call returns CRD_ESTATE with crd_ensemble_last_error naming the failed members.
 * stats and status: n_members entries each, or NULL.  CRD_EINVAL, before any device work, for CRD_ADAPT_RK43 and every option or
 * interval crd_integrate_adaptive refuses.  The first call allocates three more state buffers per member (the dense output's y_n,
 * y_{n+1} / f_n, f_{n+1} / interpolant), kept for later calls; an ensemble that only takes fixed steps never does.  Synchronous. */
int crd_ensemble_integrate_adaptive(crd_ensemble *e, double t0, double tout, const crd_adaptive_options *opt,
                                    crd_adaptive_stats *stats, int32_t *status);

/* Observers: while an ensemble steps, record for every member -- on the device, without a host synchronisation -- the field
 * statistics, the values at a few probe points and, optionally, per-point maps.  What a scan is read for (does member k oscillate,
 * with what amplitude and period, where, and when does the wave arrive) without downloading every member's state at every output
 * (the reference answers these from its output files, util/Plotting).  One sample is two small launches on the ensemble's stream
 * behind the step it samples: a sampling pass over the state (blocks_per_member workgroups per member, each writing one partial
 * record) and a finishing launch that adds a member's partials in index order.  No floating-point atomics: every addition has a
 * fixed place, blocks_per_member depends on the grid size alone, so a member's row is bit-identical from run to run and in an
 * ensemble of 1 and of 64.  Statistics accumulate in double whatever the ensemble's precision.  min and max are exact; a sum differs
 * from the exact sum of the n = nx ny values by at most D u sum|x| (sums of squares: (D + 1) u sum x^2), u = 2^-53,
 * D = ceil(n / (256 blocks_per_member)) + 8 + blocks_per_member: no value passes through more additions than that.  A field that
 * holds a NaN reports NaN for its min, max and both sums.  This observer serves ensembles; a single context and the slabs of a LOCAL
 * group are recorded by the run recorder (crd_recorder_open, below), whose partition is by rows and survives a cut into slabs. */
#define CRD_OBSERVE_MAX_PROBES 16
typedef struct crd_observe_options {
	int64_t stride;         /* >= 1: crd_ensemble_step_rk4 records a sample after every stride-th step since crd_ensemble_observe_begin */
	int32_t n_probes;       /* 0 .. CRD_OBSERVE_MAX_PROBES grid points, the same for every member */
	int32_t maps;           /* 1: also keep three planes per member, folded at every sample: running minimum and maximum of var0 (their
	                         * difference is the peak-to-peak amplitude map) and the activation time */
	int32_t probe_i[CRD_OBSERVE_MAX_PROBES]; /* theta index, 0 .. nx - 1 */
	int32_t probe_j[CRD_OBSERVE_MAX_PROBES]; /* phi index (row), 0 .. ny - 1 */
	double threshold;       /* maps: the activation time of a point is the time of the first sample at which var0 >= threshold */
} crd_observe_options;
/* Open the ensemble's observer with room for `capacity` samples: allocates the record buffer (capacity x n_members rows of
 * 8 + 2 n_probes doubles), the partial records and, with maps, three planes of doubles per member.  CRD_EINVAL before any device work
 * for a NULL opt, stride < 1, capacity < 1, n_probes outside 0 .. CRD_OBSERVE_MAX_PROBES, a probe outside the grid, a non-finite
 * threshold with maps on, or an observer already open.  While it is open:
 *   crd_ensemble_step_rk4 records a sample after every step whose count since this call is a multiple of stride (the count carries
 *   over calls), at time t0 + (s + 1) dt for step s of the call; the call stays asynchronous.  A call that would record more
 *   samples than there is room left is refused whole (CRD_EINVAL, nothing launched, state and sample count untouched);
 *   crd_ensemble_integrate_adaptive records one sample per call, at tout, of the states it hands back; a member whose status is not
 *   CRD_OK gets a row of NaNs (CRD_EINVAL, before any work, when no room is left) -- the sample is recorded and counted also when the call returns CRD_ESTATE -- and with maps on that
 *   member's state, NaNs included, is still folded into its map planes (they follow np.minimum / np.maximum: a NaN stays);
 *   crd_ensemble_upload does not disturb it.
 * With no observer open an ensemble launches exactly what it launches without this interface. */
int crd_ensemble_observe_begin(crd_ensemble *e, const crd_observe_options *opt, int64_t capacity);
/* Samples recorded (enqueued) so far. */
int crd_ensemble_observe_count(const crd_ensemble *e, int64_t *n_samples);
/* Samples first .. first + count - 1: synchronises, ONE device-to-host copy.  Any of the three outputs may be NULL.
 *   t[count]                                  sample times
 *   stats[count][n_members][8]                min, max, sum, sum of squares of var0, then the same four of var1
 *   probes[count][n_members][n_probes][2]     var0, var1 at each probe
 * CRD_EINVAL for a range outside the recorded samples.  Reading does not consume: samples stay until crd_ensemble_observe_end. */
int crd_ensemble_observe_read(crd_ensemble *e, int64_t first, int64_t count, double *t, double *stats, double *probes);
/* One member's maps as they stand, ny * nx doubles each (row-major, theta fastest), any of them NULL: running minimum and maximum of
 * var0 over the samples so far (+inf / -inf before the first) and the activation time (NaN where var0 was never >= threshold at a
 * sample).  Synchronises.  CRD_EINVAL without maps. */
int crd_ensemble_observe_maps(crd_ensemble *e, int member, double *min_u, double *max_u, double *t_act);
/* What states the rounding bound above: sampling blocks per member, values per field (nx ny), and the observer's options and
 * capacity.  Any pointer may be NULL.  CRD_EINVAL with no observer open. */
/* (members of different shape, crd_ensemble_create_mixed: blocks_per_member and values_per_field are member 0's, as crd_ensemble_info's
 * grid; member k's are those of its own nx * ny, crd_ensemble_member_grid) */
int crd_ensemble_observe_info(const crd_ensemble *e, int32_t *blocks_per_member, int64_t *values_per_field, crd_observe_options *opt, int64_t *capacity);
/* Close the observer and free what it holds (crd_ensemble_destroy does too).  CRD_EINVAL with no observer open. */
int crd_ensemble_observe_end(crd_ensemble *e);
/* The same eight statistics of a single-slab context's state, stats[8] as a row of crd_ensemble_observe_read: one synchronous call
 * on the same sampling kernel, bit-identical to the row of an ensemble of one holding that state.  Generalises crd_state_max_abs.
 * CRD_EINVAL for a context that is one of several slabs (no cross-rank reduction). */
int crd_state_observe(crd_ctx *ctx, double stats[8]);

/* Sections and cycle maps: what a scan's space-time plots and period maps are read from, recorded by the same observer.
 * A section is one line of values per sample and member, (var0, var1) per point, stored as doubles: recorded on the device by one
 * more launch per sample (only when sections are configured), on the ensemble's stream behind the finishing launch, with no host wait.
 *   CRD_SECTION_ROW, index j      nx values: both fields along theta at row j -- exact: the state's value widened to double
 *   CRD_SECTION_COLUMN, index i   ny values: both fields along phi at column i -- exact
 *   CRD_SECTION_THETA_MEAN        ny values: the mean over theta of each row (the axial profile)
 *   CRD_SECTION_PHI_MEAN          nx values: the mean over phi of each column (around the tube: inner against outer equator)
 * The means accumulate in double whatever the ensemble's precision, without atomics: which lane takes which point and the order of every
 * addition depend on nx, ny and the precision alone, so a line is bit-identical from run to run, in an ensemble of 1 and of 64 and from
 * crd_state_section.  theta-mean: a wavefront per row; group c of V consecutive columns (V = 2 in fp64, 4 in fp32: a 16-byte load)
 * belongs to lane c mod 64, element e of a lane's groups is added in rising order into its accumulator e, the V accumulators are
 * folded pairwise, the 64 lanes by a shuffle tree: ceil(ceil(nx / V) / 64) + log2 V + 6 additions at most.  phi-mean: a workgroup per
 * 64 columns; wavefront w adds rows w, w + 4, ... in rising order, the four are combined (0 + 1) + (2 + 3): ceil(ny / 4) + 2 additions.
 * With D that count + 3 (crd_ensemble_observe_section_info reports it) a mean of n values x satisfies
 *   |mean - exact| <= D u sum|x| / n, u = 2^-53, also with fsum(x) / n standing for the exact mean
 * (the + 3: the division by n, and the two roundings of fsum(x) / n; an accumulator's first addition, to zero, is exact and pays for
 * the terms of second order).  A NaN in a row (column) makes that row's theta-mean (that column's phi-mean) NaN and touches nothing else.
 * A field whose partial sums are all representable -- a uniform field of values with few significant bits, e.g. any uniform fp32
 * field on a grid of less than 2^29 points a side -- has means equal to its value exactly.
 *
 * Cycle maps (cycles = 1): four more planes per member -- the previous sample's var0, an int32 count, t_first and t_last -- folded at
 * every sample in the sampling pass itself (the state is read once for statistics, maps and cycles together).  At a point, in double,
 * every operation rounded once, with x_prev / t_prev the previous sample's value and time:
 *   d0 = x_prev - cycle_threshold, d1 = x - cycle_threshold; an upward crossing is d0 < 0 && d1 >= 0, at
 *   tc = t_prev + (t - t_prev) * (-d0 / (d1 - d0)); then count += 1, t_first = tc if it is the first, t_last = tc.
 * The first sample after begin only stores x_prev.  A NaN compares false: it makes no crossing and becomes the next x_prev.  The
 * period map is (t_last - t_first) / (count - 1) where count >= 2, formed by the caller. */
#define CRD_OBSERVE_MAX_SECTIONS 8
#define CRD_SECTION_ROW 0
#define CRD_SECTION_COLUMN 1
#define CRD_SECTION_THETA_MEAN 2
#define CRD_SECTION_PHI_MEAN 3
typedef struct crd_observe_extras {
	int32_t n_sections;                              /* 0 .. CRD_OBSERVE_MAX_SECTIONS, the same for every member */
	int32_t cycles;                                  /* 1: keep the cycle maps */
	int32_t kind[CRD_OBSERVE_MAX_SECTIONS];          /* CRD_SECTION_* */
	int32_t index[CRD_OBSERVE_MAX_SECTIONS];         /* row j or column i; ignored by the two means */
	double cycle_threshold;
} crd_observe_extras;
/* crd_ensemble_observe_begin with sections and cycle maps; extras == NULL is crd_ensemble_observe_begin itself, which launches exactly
 * what it launched without this interface.  Besides its refusals, CRD_EINVAL before any device work for n_sections outside
 * 0 .. CRD_OBSERVE_MAX_SECTIONS, an unknown kind, a row or column outside the grid, cycles other than 0 or 1, or a non-finite
 * cycle_threshold with cycles on.  The record buffer grows by capacity x n_members x (sum of the sections' lengths) x 2 doubles
 * (CRD_ENOMEM when it cannot be had; nothing is left open).  Everything said of sampling under crd_ensemble_observe_begin holds: the
 * stride's count over calls, the refusal of a whole call when the room runs out, one sample per crd_ensemble_integrate_adaptive call
 * at tout -- a failed member gets lines of NaNs, and its state is still folded into its cycle planes by the rule above. */
int crd_ensemble_observe_begin_with(crd_ensemble *e, const crd_observe_options *opt, const crd_observe_extras *extras, int64_t capacity);
/* Section `section` of the open observer: its kind and index, its values per field and D of the bound above (0 for the exact kinds).
 * Any pointer may be NULL.  CRD_EINVAL with no observer open or for a section that was not configured. */
int crd_ensemble_observe_section_info(const crd_ensemble *e, int section, int32_t *kind, int32_t *index, int64_t *length, int64_t *additions);
/* Samples first .. first + count - 1 of one section, values[count][n_members][length][2]: synchronises, ONE device-to-host copy.
 * CRD_EINVAL for a section that was not configured or a range outside the recorded samples. */
int crd_ensemble_observe_read_section(crd_ensemble *e, int section, int64_t first, int64_t count, double *values);
/* One member's cycle maps as they stand, ny * nx values each (row-major, theta fastest), any of them NULL: the count of upward
 * crossings, and the times of the first and of the last (NaN where count = 0).  Synchronises.  CRD_EINVAL when cycles are off. */
int crd_ensemble_observe_cycles(crd_ensemble *e, int member, int32_t *count, double *t_first, double *t_last);
/* One section of a single-slab context's state, values[length][2]: the single-slab counterpart of crd_state_observe.  One synchronous
 * call on the sections kernel with a one-entry descriptor over the context's owned rows, bit-identical to the line of an ensemble of
 * one holding that state: the axial profile of a large run without downloading it.  CRD_EINVAL for an unknown kind, a row or column
 * outside the grid, or a context that is one of several slabs. */
int crd_state_section(crd_ctx *ctx, int kind, int index, double *values);

/* ---------------------------------------------------------------------------------------------------------
 * Run recorder: the observer of a single-slab context or of ALL contexts of one LOCAL group (crd_comm_attach_local), sampling inside
 * the stepping calls.  What the ensemble observer gives a scan -- statistics, probes, sections, amplitude / activation maps, cycle maps,
 * read off the device without downloading the state -- for the runs a context exists for: one large grid, whole or cut into phi-slabs.
 * No reference counterpart (the reference writes every output time to text files, src/FHNmodel_torus.cpp:438-455, and reads them back
 * in util/Plotting).  crd_observe_options and crd_observe_extras keep their documented meaning; probes, rows and columns are indices
 * on the GLOBAL grid.
 *
 * One sample is, per slab, two launches on the slab's compute stream behind the step it samples -- a row pass that reads the state
 * ONCE whatever is recorded, and a small gather of the exact values -- and one finishing launch on slab 0's device behind an event of
 * every slab's stream (the other slabs' row records and line parts arrive by at most two peer copies per slab and sample).  No host wait.
 *   Row pass: one wavefront per owned row.  Group c of V consecutive columns (V = 2 in fp64, 4 in fp32: a 16-byte load, or the same
 *   columns element by element where the row does not sit on 16 bytes) belongs to lane c mod 64; element e of a lane's groups is added
 *   in rising order into its accumulator e (squares: fma(x, x, q)); the V accumulators are folded pairwise, the 64 lanes by a shuffle
 *   tree -- the theta-mean section's partition.  Per row: min, max, sum, sum of squares of both fields, and the row's theta-mean,
 *   sum / nx.  With maps / cycles on, the same pass folds var0 into the slab's map / cycle planes by the rules above.
 *   Finish: one workgroup of 256 lanes; lane l folds the records of GLOBAL rows l, l + 256, ... in rising order, then a fixed tree
 *   128 ... 1 in LDS.  No floating-point atomics.
 * A row belongs to exactly one slab and rows are combined by global index: statistics, theta-mean, rows, columns, probes, maps and cycle
 * maps are THE SAME BITS for one slab and for any cut into slabs, and from run to run.  This partition differs from crd_state_observe's
 * and the ensemble observer's on purpose (theirs is defined on the flat point index and cannot survive a cut): the sums agree with
 * theirs to the bounds, not to the bit.  The theta-mean line of a lone context is the bits of crd_state_section(CRD_SECTION_THETA_MEAN);
 * its phi-mean line those of crd_state_section(CRD_SECTION_PHI_MEAN).
 * Bounds: min, max, probes, rows, columns, maps and cycle planes are exact.  With u = 2^-53,
 *   |sum - exact| <= D u sum|x|,   |sumsq - exact| <= (D + 1) u sum x^2,
 *   D = ceil(ceil(nx / V) / 64) + log2 V + 6 + ceil(ny / 256) + 8        (crd_recorder_info reports it);
 * theta-mean and phi-mean: the bounds stated for the sections above.  A NaN in a row makes that field's four statistics and that row's
 * theta-mean NaN and touches nothing else.
 *
 * crd_recorder_open: ctxs[k] must be slab k of n_slabs, the whole group (n_slabs = 1: a single-slab context).  Allocates, on slab 0's
 * device, capacity rows of 8 + 2 n_probes doubles, capacity lines per section and one record of 10 + 2 (column sections) doubles per
 * grid row; per slab, with maps three and with cycles four planes of nyl x nx doubles.  extras may be NULL.  CRD_EINVAL before any
 * device work, crd_last_error(ctxs[0]) naming the reason: everything crd_ensemble_observe_begin_with refuses; CRD_SECTION_PHI_MEAN on
 * more than one slab (a column's sum crosses the slabs; allowed on a lone context); block contexts (crd_create_block with d0 > 1); a
 * context wired through RCCL with more than one rank; a context list that is not the whole LOCAL group; a second recorder on a context.
 * While it is open:
 *   crd_step_rk4 / crd_group_step_rk4 and their timed variants take a sample after every step whose count since open is a multiple of
 *   stride (the count carries over calls), at time t0 + (s + 1) dt for step s of the call.  A call that would overrun the capacity is
 *   refused whole (CRD_EINVAL, nothing launched, state and counts untouched).  Stage times are formed from the call's t0 and the step's
 *   index as without a recorder; only the grouping of steps into launches changes -- no pair, triple or split launch straddles a
 *   sample -- so the state is bit-identical to the same call without a recorder.  A recorded group is issued by one host thread.
 *   crd_integrate_adaptive / crd_group_integrate_adaptive record one sample per call, at tout, of the state handed back (CRD_EINVAL
 *   before any work when no room is left); the stride's count does not move.
 *   A stepping call on recorded contexts that does not cover the recorder's whole group returns CRD_ESTATE.
 * With no recorder open every call launches exactly what it launches without this interface. */
typedef struct crd_recorder crd_recorder;
int crd_recorder_open(crd_ctx *const *ctxs, int n_slabs, const crd_observe_options *opt, const crd_observe_extras *extras, int64_t capacity, crd_recorder **out);
/* Samples recorded (enqueued) so far. */
int crd_recorder_count(const crd_recorder *rec, int64_t *n_samples);
/* D of the bound above, values per field (nx ny), the slabs recorded, the options and the capacity.  Any pointer may be NULL. */
int crd_recorder_info(const crd_recorder *rec, int64_t *additions, int64_t *values_per_field, int32_t *n_slabs, crd_observe_options *opt, crd_observe_extras *extras,
                      int64_t *capacity);
/* Samples first .. first + count - 1: t[count], stats[count][8], probes[count][n_probes][2], any of them NULL.  Synchronises; one
 * device-to-host copy.  CRD_EINVAL for a range outside the recorded samples.  Reading does not consume. */
int crd_recorder_read(crd_recorder *rec, int64_t first, int64_t count, double *t, double *stats, double *probes);
/* As crd_ensemble_observe_section_info / _read_section: values[count][length][2]; one copy. */
int crd_recorder_section_info(const crd_recorder *rec, int section, int32_t *kind, int32_t *index, int64_t *length, int64_t *additions);
int crd_recorder_read_section(crd_recorder *rec, int section, int64_t first, int64_t count, double *values);
/* The maps / cycle maps as they stand, as whole-grid ny x nx planes gathered from the slabs (one copy per slab), any of them NULL;
 * meaning and initial values as crd_ensemble_observe_maps / _cycles.  CRD_EINVAL when maps / cycles are off. */
int crd_recorder_maps(crd_recorder *rec, double *min_u, double *max_u, double *t_act);
int crd_recorder_cycles(crd_recorder *rec, int32_t *count, double *t_first, double *t_last);
/* Close the recorder and free what it holds.  crd_destroy of a recorded context closes it too (do not close it again). */
int crd_recorder_close(crd_recorder *rec);

#ifdef __cplusplus
}
#endif
#endif /* CRD_H */
