/* Stand-in for <arkode/arkode.h>.  NOT an integrator with step-size control: it remembers the right-hand side the program hands
 * to ARKodeInit -- the reference's own static f(), which runs its own Exchange() -- and calls it in one of two modes, chosen by
 * the environment:
 *
 *   CRD_REF_PROBE=<file>   probe mode.  The file holds records of (t, state): one double, then as many doubles as the vector
 *                          has.  Call k of ARKode() reads record k into y, calls f(t_k, y, ydot), copies ydot over y and sets
 *                          *t = tout.  No arithmetic on field values happens here: what the program then writes is f()'s output.
 *   CRD_REF_RK4_DT=<dt>    fixed-step mode.  Classical RK4 steps of dt from *t to tout, stages through f at t + c dt.  The stage
 *                          states and the four-term update are formed in exactly the order of crd_oracle_rk4 (oracle/crd_oracle.c);
 *                          that combination is this file's arithmetic, every f() is the reference's.
 *
 * With neither set, or with a missing or short probe file, ARKode() returns a negative flag, which the programs report as a
 * solver failure after having written their subdomain file and initial row. */
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "nvector/nvector_parallel.h"

#define ARK_NORMAL 1
#define ARK_SUCCESS 0
#define ARK_ILL_INPUT (-22)

typedef int (*ARKRhsFn)(realtype t, N_Vector y, N_Vector ydot, void *user_data);

struct crd_standin_arkode {
	ARKRhsFn fe;
	void *user_data;
	long calls;
	realtype t;
};

static inline void *ARKodeCreate()
{
	crd_standin_arkode *m = new crd_standin_arkode;
	m->fe = NULL;
	m->user_data = NULL;
	m->calls = 0;
	m->t = 0;
	return m;
}

static inline int ARKodeInit(void *mem, ARKRhsFn fe, ARKRhsFn, realtype t0, N_Vector)
{
	if (!mem || !fe) return ARK_ILL_INPUT;
	((crd_standin_arkode *)mem)->fe = fe;
	((crd_standin_arkode *)mem)->t = t0;
	return ARK_SUCCESS;
}

static inline int ARKodeSStolerances(void *, realtype, realtype) { return ARK_SUCCESS; }

static inline int ARKodeSetUserData(void *mem, void *user_data)
{
	((crd_standin_arkode *)mem)->user_data = user_data;
	return ARK_SUCCESS;
}

static inline int ARKodeSetMaxNumSteps(void *, long) { return ARK_SUCCESS; }

static inline void ARKodeFree(void **mem)
{
	delete (crd_standin_arkode *)*mem;
	*mem = NULL;
}

static inline int crd_standin_arkode_probe(crd_standin_arkode *m, const char *path, N_Vector y)
{
	FILE *fp = fopen(path, "rb");
	if (!fp) return -1;
	const long n = y->length;
	double tk = 0;
	int ok = fseek(fp, m->calls * (n + 1) * (long)sizeof(double), SEEK_SET) == 0 && fread(&tk, sizeof(double), 1, fp) == 1;
	N_Vector state = ok ? N_VNew_Parallel(MPI_COMM_WORLD, n, n) : NULL;
	ok = ok && state && fread(state->data, sizeof(double), (size_t)n, fp) == (size_t)n;  /* a short record leaves y untouched */
	fclose(fp);
	N_Vector ydot = ok ? N_VNew_Parallel(MPI_COMM_WORLD, n, n) : NULL;
	int rc = -1;
	if (ok && ydot) {
		memcpy(y->data, state->data, sizeof(double) * (size_t)n);
		rc = m->fe(tk, y, ydot, m->user_data);
		memcpy(y->data, ydot->data, sizeof(double) * (size_t)n);
	}
	N_VDestroy_Parallel(state);
	N_VDestroy_Parallel(ydot);
	return rc < 0 ? -1 : ARK_SUCCESS;
}

static inline int crd_standin_arkode_rk4(crd_standin_arkode *m, double dt, realtype tout, N_Vector yv)
{
	if (!(dt > 0.0) || !(tout > m->t)) return -1;
	const long n = yv->length, nsteps = lrint((tout - m->t) / dt);
	if (nsteps < 1) return -1;
	N_Vector k1 = N_VNew_Parallel(0, n, n), k2 = N_VNew_Parallel(0, n, n), k3 = N_VNew_Parallel(0, n, n), k4 = N_VNew_Parallel(0, n, n);
	N_Vector ysv = N_VNew_Parallel(0, n, n);
	int rc = (k1 && k2 && k3 && k4 && ysv) ? 0 : -1;
	double *y = yv->data;
	const double t0 = m->t;
	for (long s = 0; s < nsteps && rc == 0; s++) {
		const double t = t0 + (double)s * dt;
		double *ys = ysv->data;
		long q;
		rc |= m->fe(t, yv, k1, m->user_data);
		for (q = 0; q < n; q++) ys[q] = y[q] + (0.5 * dt) * k1->data[q];
		rc |= m->fe(t + 0.5 * dt, ysv, k2, m->user_data);
		for (q = 0; q < n; q++) ys[q] = y[q] + (0.5 * dt) * k2->data[q];
		rc |= m->fe(t + 0.5 * dt, ysv, k3, m->user_data);
		for (q = 0; q < n; q++) ys[q] = y[q] + dt * k3->data[q];
		rc |= m->fe(t + dt, ysv, k4, m->user_data);
		for (q = 0; q < n; q++) y[q] = y[q] + (dt / 6.0) * (k1->data[q] + 2.0 * k2->data[q] + 2.0 * k3->data[q] + k4->data[q]);
	}
	N_VDestroy_Parallel(k1);
	N_VDestroy_Parallel(k2);
	N_VDestroy_Parallel(k3);
	N_VDestroy_Parallel(k4);
	N_VDestroy_Parallel(ysv);
	return rc != 0 ? -1 : ARK_SUCCESS;
}

static inline int ARKode(void *mem, realtype tout, N_Vector y, realtype *t, int)
{
	crd_standin_arkode *m = (crd_standin_arkode *)mem;
	if (!m || !m->fe || !y || !t) return ARK_ILL_INPUT;
	const char *probe = getenv("CRD_REF_PROBE"), *rk4_dt = getenv("CRD_REF_RK4_DT");
	int rc = -1;
	if (probe && *probe) rc = crd_standin_arkode_probe(m, probe, y);
	else if (rk4_dt && *rk4_dt) rc = crd_standin_arkode_rk4(m, strtod(rk4_dt, NULL), tout, y);
	if (rc < 0) return rc;
	m->calls++;
	m->t = tout;
	*t = tout;
	return ARK_SUCCESS;
}
