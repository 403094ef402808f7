/* Drives crd_arkode_psolve of integration/crd_arkode_shim.c on host vectors through a SUNDIALS-typed function pointer, as
 * ARKSpilsSetPreconditioner(arkode_mem, NULL, crd_arkode_psolve) would.  argv[1] = ini file, argv[2] = where to write r and z (two runs
 * of doubles per time) for tests/test_gpu_multigrid.py, which holds z to the bits of crd_psolve_device.  Checked here: the callback
 * gives crd_psolve_host's bits with either lr, ignores y, fy, delta and tmp, copies var1, and follows the callbacks' error
 * convention.  Built with gcc -DCRD_SHIM_NVECTOR_HEADER='"mock_nvector.h"'. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "crd_arkode_shim.h"

/* ARKode 1.x, arkode_spils.h */
typedef int (*ARKSpilsPrecSolveFn)(realtype t, N_Vector y, N_Vector fy, N_Vector r, N_Vector z, realtype gamma, realtype delta, int lr, void *user_data, N_Vector tmp);

#define SELFTEST_GAMMA 0.0625

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
	N_Vector r = make_vector(n), z = make_vector(n), z2 = make_vector(n), zh = make_vector(n);
	unsigned long long s = 88172645463325252ull; /* xorshift: a right-hand side with no structure */
	for (long q = 0; q < n; q++) {
		s ^= s << 13, s ^= s >> 7, s ^= s << 17;
		r->data[q] = (double)(s >> 11) / 9007199254740992.0 - 0.5;
	}
	ARKSpilsPrecSolveFn psolve = crd_arkode_psolve;
	FILE *out = fopen(argv[2], "wb");
	if (!out) return 5;
	const double times[2] = {0.5 * cfg.params.t_boundary, 2.0 * cfg.params.t_boundary + 1.0}; /* rows held, and free */
	for (int k = 0; k < 2; k++) {
		const realtype t = times[k];
		if (psolve(t, NULL, NULL, r, z, SELFTEST_GAMMA, 1e-3, 1, gpu, NULL) != 0 || psolve(t, r, z, r, z2, SELFTEST_GAMMA, 0.0, 2, gpu, zh) != 0) {
			fprintf(stderr, "crd_arkode_psolve failed: %s\n", crd_last_error(gpu));
			return 6;
		}
		if (crd_psolve_host(gpu, t, SELFTEST_GAMMA, NULL, r->data, zh->data) != CRD_OK) return 7;
		if (memcmp(z->data, z2->data, (size_t)n * sizeof(realtype)) != 0 || memcmp(z->data, zh->data, (size_t)n * sizeof(realtype)) != 0) {
			fprintf(stderr, "crd_arkode_psolve is not crd_psolve_host at t = %g\n", (double)t);
			return 8;
		}
		for (long q = 1; q < n; q += 2)
			if (memcmp(&z->data[q], &r->data[q], sizeof(realtype)) != 0) return 9;
		if (fwrite(r->data, sizeof(realtype), (size_t)n, out) != (size_t)n || fwrite(z->data, sizeof(realtype), (size_t)n, out) != (size_t)n) return 10;
	}
	fclose(out);
	if (psolve(0.0, NULL, NULL, NULL, z, SELFTEST_GAMMA, 0.0, 1, gpu, NULL) != -1 || psolve(0.0, NULL, NULL, r, NULL, SELFTEST_GAMMA, 0.0, 1, gpu, NULL) != -1 ||
	    psolve(0.0, NULL, NULL, r, z, SELFTEST_GAMMA, 0.0, 1, NULL, NULL) != -1 || psolve(0.0, NULL, NULL, r, z, -1.0, 0.0, 1, gpu, NULL) != -1)
		return 11;
	printf("shim psolve selftest: %ld unknowns, %ld x %ld, tBoundary %.17g, gamma %.17g, times %.17g %.17g\n", n, (long)g.nx, (long)g.ny, cfg.params.t_boundary,
	       (double)SELFTEST_GAMMA, times[0], times[1]);
	N_Vector all[4] = {r, z, z2, zh};
	for (int i = 0; i < 4; i++) {
		free(all[i]->data);
		free(all[i]);
	}
	crd_destroy(gpu);
	return 0;
}
