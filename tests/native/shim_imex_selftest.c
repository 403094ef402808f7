/* Drives the IMEX callbacks of integration/crd_arkode_shim.c on host vectors, as ARKodeInit(mem, fe, fi, T0, y) with a Krylov solver
 * would: fe, fi and f at one state, and the Jacobian-times-vector callbacks on one direction.  argv[1] = ini file, argv[2] = where
 * to write y, f, fe, fi (four runs of doubles, in that order, per time) for tests/test_gpu_jacobian.py, which holds fe + fi to the
 * rounding bounds of f's parts.  Checked here: jtimes_fi(v) is fi applied to v, bit for bit; the callbacks' error convention.
 * Built with gcc -DCRD_SHIM_NVECTOR_HEADER='"mock_nvector.h"'. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "crd_arkode_shim.h"

typedef int (*ARKRhsFn)(realtype t, N_Vector y, N_Vector ydot, void *user_data);                                              /* SUNDIALS 2.x arkode.h */
typedef int (*ARKSpilsJacTimesVecFn)(N_Vector v, N_Vector Jv, realtype t, N_Vector y, N_Vector fy, void *user_data, N_Vector tmp); /* arkode_spils.h */

static N_Vector make_vector(long n)
{
	N_Vector v = (N_Vector)malloc(sizeof *v);
	v->local_length = n;
	v->data = (realtype *)malloc((size_t)n * sizeof(realtype));
	return v;
}

int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	crd_run_config cfg;
	char err[256];
	if (crd_config_load_ini(argv[1], CRD_MODEL_FHN, CRD_SURFACE_TORUS, &cfg, err, sizeof err) != CRD_OK) {
		fprintf(stderr, "%s\n", err);
		return 3;
	}
	crd_ctx *gpu = NULL;
	if (crd_arkode_attach(&cfg, 0, 1, 0, NULL, NULL, &gpu) != CRD_OK) {
		fprintf(stderr, "%s\n", crd_last_error(NULL));
		return 4;
	}
	crd_grid g;
	crd_get_grid(gpu, &g);
	const long n = 2 * g.nx * g.ny;
	N_Vector y = make_vector(n), v = make_vector(n), f = make_vector(n), fe = make_vector(n), fi = make_vector(n), jv = make_vector(n), fiv = make_vector(n);
	if (crd_initial_conditions(&cfg, 0, g.ny - 1, y->data) != CRD_OK) return 5;
	unsigned long long s = 88172645463325252ull; /* xorshift: a direction with no structure */
	for (long q = 0; q < n; q++) {
		s ^= s << 13, s ^= s >> 7, s ^= s << 17;
		v->data[q] = (double)(s >> 11) / 9007199254740992.0 - 0.5;
		y->data[q] += 0.02 * v->data[q];
	}
	ARKRhsFn rhs = crd_arkode_f, rhs_e = crd_arkode_fe, rhs_i = crd_arkode_fi;
	ARKSpilsJacTimesVecFn jt_i = crd_arkode_jtimes_fi, jt = crd_arkode_jtimes;
	FILE *out = fopen(argv[2], "wb");
	if (!out) return 6;
	const double times[2] = {0.5 * cfg.params.t_boundary, 2.0 * cfg.params.t_boundary + 1.0}; /* absorbing rows on, and off */
	for (int k = 0; k < 2; k++) {
		const realtype t = times[k];
		if (rhs(t, y, f, gpu) != 0 || rhs_e(t, y, fe, gpu) != 0 || rhs_i(t, y, fi, gpu) != 0) {
			fprintf(stderr, "a right-hand side failed: %s\n", crd_last_error(gpu));
			return 7;
		}
		if (jt_i(v, jv, t, y, f, gpu, NULL) != 0 || rhs_i(t, v, fiv, gpu) != 0) return 8;
		if (memcmp(jv->data, fiv->data, (size_t)n * sizeof(realtype)) != 0) {
			fprintf(stderr, "jtimes_fi(v) is not fi(v) at t = %g\n", (double)t);
			return 9;
		}
		if (jt(v, jv, t, y, f, gpu, NULL) != 0) return 10;
		N_Vector dump[4] = {y, f, fe, fi};
		for (int i = 0; i < 4; i++)
			if (fwrite(dump[i]->data, sizeof(realtype), (size_t)n, out) != (size_t)n) return 11;
	}
	fclose(out);
	if (rhs_e(0.0, NULL, fe, gpu) != -1 || rhs_i(0.0, y, NULL, gpu) != -1 || jt_i(NULL, jv, 0.0, y, f, gpu, NULL) != -1 || jt(v, jv, 0.0, y, f, NULL, NULL) != -1) return 12;
	printf("shim imex selftest: %ld unknowns, %ld x %ld, tBoundary %.17g, times %.17g %.17g\n", n, (long)g.nx, (long)g.ny, cfg.params.t_boundary, times[0], times[1]);
	N_Vector all[7] = {y, v, f, fe, fi, jv, fiv};
	for (int i = 0; i < 7; i++) {
		free(all[i]->data);
		free(all[i]);
	}
	crd_destroy(gpu);
	return 0;
}
