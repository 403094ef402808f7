/*
 * crd_arkode_shim.h -- CRDModel's SUNDIALS callback bound to libcrd.
 *
 * For a maintainer who keeps the reference's adaptive ARKode loop (src/FHNmodel_torus.cpp:356-372,423) and only replaces the
 * right-hand side: compile crd_arkode_shim.c into the reference program with the SUNDIALS headers that program already uses
 * (2.6 / 2.7: `ARKRhsFn` = int (*)(realtype, N_Vector, N_Vector, void *)), then
 *
 *     crd_ctx *gpu;  crd_arkode_attach(&cfg, rank, nprocs, device, bcast, comm, &gpu);
 *     ARKodeInit(arkode_mem, crd_arkode_f, NULL, T0, y);          // was f           (:362)
 *     ARKodeSetUserData(arkode_mem, (void *) gpu);                // was udata       (:369)
 *
 * INTEGRATION.md section 1 has the surrounding lines.
 */
#ifndef CRD_ARKODE_SHIM_H
#define CRD_ARKODE_SHIM_H

#ifdef CRD_SHIM_NVECTOR_HEADER /* the self-test supplies its own N_Vector (tests/native/mock_nvector.h) */
#include CRD_SHIM_NVECTOR_HEADER
#else
#include <nvector/nvector_parallel.h>
#include <sundials/sundials_types.h>
#endif

#include "crd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The ARKRhsFn: replaces `static int f(realtype t, N_Vector y, N_Vector ydot, void *user_data)` (src/FHNmodel_torus.cpp:126,
 * 504-667 and the three siblings).  user_data is the crd_ctx.  y / ydot are the rank's NVECTOR_PARALLEL vectors in the
 * reference's layout (IDX, :60); halo exchange, diffusion and kinetics happen on the GPU; every element of ydot is written.
 * Returns 0, or -1 as the reference does when its Exchange fails (:522) -- unrecoverable for ARKode. */
int crd_arkode_f(realtype t, N_Vector y, N_Vector ydot, void *user_data);

/* The same right-hand side split for an IMEX or implicit ARKode: fe = the kinetics (crd_rhs_part_host, CRD_PART_REACTION), fi = the
 * diffusion operator (CRD_PART_DIFFUSION); fe + fi = f up to rounding.  The reference passes NULL for fi (src/FHNmodel_torus.cpp:362):
 *
 *     ARKodeInit(arkode_mem, crd_arkode_fe, crd_arkode_fi, T0, y);
 *     ARKSpgmr(arkode_mem, PREC_NONE, 0);
 *     ARKSpilsSetJacTimesVecFn(arkode_mem, crd_arkode_jtimes_fi);
 *
 * crd_arkode_jtimes_fi is J_fi(t, y) v, the Jacobian of the implicit part alone, which is what an IMEX ARKode's Newton iteration
 * linearises (it equals fi applied to v: the operator is linear); crd_arkode_jtimes is the whole f's, for a fully implicit run
 * (ARKodeInit(arkode_mem, NULL, crd_arkode_f, T0, y)).  Both take the arguments ARKode 1.x documents for ARKSpilsJacTimesVecFn,
 * (v, Jv, t, y, fy, user_data, tmp); fy and tmp are not used.  UNVERIFIED: the signature is taken from SUNDIALS' documentation, no
 * SUNDIALS build has compiled or called these callbacks (tests drive them through the test double's N_Vector).  Return 0 / -1 as
 * crd_arkode_f.  INTEGRATION.md section 1b has the surrounding lines and why GMRES, not the PCG solver the reference includes. */
int crd_arkode_fe(realtype t, N_Vector y, N_Vector ydot, void *user_data);
int crd_arkode_fi(realtype t, N_Vector y, N_Vector ydot, void *user_data);
int crd_arkode_jtimes_fi(N_Vector v, N_Vector Jv, realtype t, N_Vector y, N_Vector fy, void *user_data, N_Vector tmp);
int crd_arkode_jtimes(N_Vector v, N_Vector Jv, realtype t, N_Vector y, N_Vector fy, void *user_data, N_Vector tmp);

/* The preconditioner solve of the IMEX run's Newton system (I - gamma J_fi) z = r: one multigrid V-cycle on the GPU (crd_psolve_host
 * with the default options; single-slab contexts only).  With it the Krylov iteration count stays bounded where it otherwise grows
 * like the square root of gamma times the operator's largest eigenvalue:
 *
 *     ARKSpgmr(arkode_mem, PREC_LEFT, 0);                                   // or PREC_RIGHT
 *     ARKSpilsSetPreconditioner(arkode_mem, NULL, crd_arkode_psolve);       // no setup function: the cycle has nothing to factor
 *
 * The arguments are those ARKode 1.x documents for ARKSpilsPrecSolveFn, (t, y, fy, r, z, gamma, delta, lr, user_data, tmp); y, fy,
 * delta and tmp are not used and either lr is taken (the cycle is one fixed linear map).  UNVERIFIED against a SUNDIALS build like the
 * callbacks above.  Returns 0 / -1. */
int crd_arkode_psolve(realtype t, N_Vector y, N_Vector fy, N_Vector r, N_Vector z, realtype gamma, realtype delta, int lr, void *user_data, N_Vector tmp);

/* Creates the rank's context from the run configuration (crd_config_load_ini of the same ini file main() reads, :158-174) and,
 * for nprocs > 1, joins the RCCL ring: `bcast(buf, bytes, comm)` is any broadcast of `bytes` (129: a status byte + the 128-byte
 * id) from rank 0 -- with MPI, `MPI_Bcast(buf, bytes, MPI_BYTE, 0, comm)` wrapped in a two-line function.  Every rank always
 * takes part in that one broadcast, also a rank whose own set-up has failed, and a failure of rank 0 (context, RCCL library,
 * unique id) is returned by EVERY rank after it, so an error never turns into a hang in bcast.  A crd_create failure on another
 * rank is returned by that rank only: treat any non-zero return as fatal for the job (MPI_Abort), as the reference treats a
 * failing check_flag (src/FHNmodel_torus.cpp:681-705).  The reference's 2-D process grid becomes
 * phi-slabs: run it with dims = {1, nprocs} (:724-728).  Returns crd_status; *out is NULL on failure and crd_last_error(NULL)
 * has the text. */
typedef int (*crd_bcast_fn)(void *buf, int bytes, void *comm);
int crd_arkode_attach(const crd_run_config *cfg, int rank, int nprocs, int device, crd_bcast_fn bcast, void *comm, crd_ctx **out);

/* Page-locked storage for the N_Vector data (N_VMake_Parallel instead of N_VNew_Parallel, :281): with it a single-GPU
 * crd_arkode_f streams the slab band by band over the host link. */
realtype *crd_arkode_alloc(long local_length);
void crd_arkode_free(realtype *data);

#ifdef __cplusplus
}
#endif
#endif
