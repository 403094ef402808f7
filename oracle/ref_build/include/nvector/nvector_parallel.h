/* Stand-in for <nvector/nvector_parallel.h>: an N_Vector is a local length and a realtype array.  Plumbing only: the one
 * arithmetic-free fill (N_VConst) is the only operation on values. */
#pragma once
#include <stdlib.h>

#include "mpi.h"
#include "sundials/sundials_types.h"

struct crd_standin_nvector {
	long length;
	realtype *data;
};
typedef crd_standin_nvector *N_Vector;

#define NV_DATA_P(v) ((v)->data)

static inline N_Vector N_VNew_Parallel(MPI_Comm, long local_length, long)
{
	if (local_length < 0) return NULL;
	N_Vector v = new crd_standin_nvector;
	v->length = local_length;
	v->data = (realtype *)calloc(local_length > 0 ? (size_t)local_length : 1, sizeof(realtype));
	if (!v->data) {
		delete v;
		return NULL;
	}
	return v;
}

static inline realtype *N_VGetArrayPointer(N_Vector v) { return v->data; }

static inline void N_VConst(realtype c, N_Vector v)
{
	for (long i = 0; i < v->length; i++) v->data[i] = c;
}

static inline void N_VDestroy_Parallel(N_Vector v)
{
	if (!v) return;
	free(v->data);
	delete v;
}
