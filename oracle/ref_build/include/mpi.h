/* Stand-in for <mpi.h>: ONE rank, written from the calls the reference programs make.  Plumbing only -- no arithmetic on data.
 *
 * size 1, rank 0; MPI_Dims_create -> {1, 1}; the Cartesian grid is periodic, so MPI_Cart_shift names this rank as the neighbour
 * in both directions.  A message to self is matched as MPI matches it: posted receives and sends are paired in posting order, a
 * receive taking the earliest unmatched send whose tag it accepts (MPI_ANY_TAG accepts all); the bytes move when the later of the
 * pair is posted.  Anything that is not such a self-exchange aborts with a message: a peer other than rank 0, a pair whose byte
 * counts differ, a wait on a request that found no partner, and requests still unmatched at MPI_Finalize. */
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef int MPI_Comm;
typedef int MPI_Datatype; /* the value is the element size in bytes */
typedef int MPI_Request;  /* index into the table below */
typedef struct {
	int MPI_SOURCE, MPI_TAG, MPI_ERROR;
} MPI_Status;

#define MPI_SUCCESS 0
#define MPI_COMM_WORLD 0
#define MPI_ANY_TAG (-1)
#define MPI_FLOAT 4
#define MPI_DOUBLE 8
#define MPI_LONG_DOUBLE 16

struct crd_standin_mpi_request {
	void *buffer;
	size_t bytes;
	int tag;
	int is_send;
	int partner; /* -1 while unmatched */
};
enum { CRD_STANDIN_MPI_MAX_REQUESTS = 64 };
static crd_standin_mpi_request crd_standin_mpi_requests[CRD_STANDIN_MPI_MAX_REQUESTS];
static int crd_standin_mpi_count = 0;

static inline void crd_standin_mpi_abort(const char *what)
{
	fprintf(stderr, "one-rank MPI stand-in: %s\n", what);
	abort();
}

static inline int MPI_Init(int *, char ***) { return MPI_SUCCESS; }

static inline int MPI_Finalize()
{
	for (int k = 0; k < crd_standin_mpi_count; k++)
		if (crd_standin_mpi_requests[k].partner == -1) crd_standin_mpi_abort("a request was still unmatched at MPI_Finalize");
	return MPI_SUCCESS;
}

static inline int MPI_Comm_rank(MPI_Comm, int *rank)
{
	*rank = 0;
	return MPI_SUCCESS;
}

static inline int MPI_Comm_size(MPI_Comm, int *size)
{
	*size = 1;
	return MPI_SUCCESS;
}

static inline int MPI_Dims_create(int nnodes, int ndims, int *dims)
{
	if (nnodes != 1) crd_standin_mpi_abort("MPI_Dims_create for more than one rank");
	for (int k = 0; k < ndims; k++) dims[k] = 1;
	return MPI_SUCCESS;
}

static inline int MPI_Cart_create(MPI_Comm, int ndims, int *dims, int *periods, int, MPI_Comm *cart)
{
	for (int k = 0; k < ndims; k++)
		if (dims[k] != 1 || periods[k] != 1) crd_standin_mpi_abort("MPI_Cart_create: not a periodic 1 x 1 grid");
	*cart = MPI_COMM_WORLD;
	return MPI_SUCCESS;
}

static inline int MPI_Cart_get(MPI_Comm, int maxdims, int *dims, int *periods, int *coords)
{
	for (int k = 0; k < maxdims; k++) {
		dims[k] = 1;
		periods[k] = 1;
		coords[k] = 0;
	}
	return MPI_SUCCESS;
}

static inline int MPI_Cart_shift(MPI_Comm, int, int, int *rank_source, int *rank_dest)
{
	*rank_source = 0; /* periodic, one rank per direction: both neighbours are this rank */
	*rank_dest = 0;
	return MPI_SUCCESS;
}

static inline void crd_standin_mpi_post(void *buffer, int count, MPI_Datatype type, int peer, int tag, int is_send, MPI_Request *request)
{
	if (peer != 0) crd_standin_mpi_abort("a message to or from a rank other than 0");
	if (count < 0) crd_standin_mpi_abort("a negative count");
	/* every earlier request completed and waited for: start the table afresh */
	int all_done = 1;
	for (int k = 0; k < crd_standin_mpi_count; k++) all_done &= (crd_standin_mpi_requests[k].partner == -2);
	if (all_done) crd_standin_mpi_count = 0;
	if (crd_standin_mpi_count == CRD_STANDIN_MPI_MAX_REQUESTS) crd_standin_mpi_abort("too many requests in flight");
	const int me = crd_standin_mpi_count++;
	crd_standin_mpi_request &r = crd_standin_mpi_requests[me];
	r.buffer = buffer;
	r.bytes = (size_t)count * (size_t)type;
	r.tag = tag;
	r.is_send = is_send;
	r.partner = -1;
	*request = me;
	/* the earliest unmatched request of the other kind whose tag fits (MPI's non-overtaking order) */
	for (int k = 0; k < me; k++) {
		crd_standin_mpi_request &o = crd_standin_mpi_requests[k];
		if (o.partner != -1 || o.is_send == is_send) continue;
		const crd_standin_mpi_request &recv = is_send ? o : r, &send = is_send ? r : o;
		if (recv.tag != MPI_ANY_TAG && recv.tag != send.tag) continue;
		if (recv.bytes != send.bytes) crd_standin_mpi_abort("a matched send and receive differ in size");
		memcpy(recv.buffer, send.buffer, send.bytes);
		o.partner = me;
		r.partner = k;
		return;
	}
}

static inline int MPI_Irecv(void *buffer, int count, MPI_Datatype type, int source, int tag, MPI_Comm, MPI_Request *request)
{
	crd_standin_mpi_post(buffer, count, type, source, tag, 0, request);
	return MPI_SUCCESS;
}

static inline int MPI_Isend(void *buffer, int count, MPI_Datatype type, int dest, int tag, MPI_Comm, MPI_Request *request)
{
	if (tag < 0) crd_standin_mpi_abort("a send with a negative tag");
	crd_standin_mpi_post(buffer, count, type, dest, tag, 1, request);
	return MPI_SUCCESS;
}

static inline int MPI_Wait(MPI_Request *request, MPI_Status *)
{
	if (*request < 0 || *request >= crd_standin_mpi_count) crd_standin_mpi_abort("MPI_Wait on an unknown request");
	crd_standin_mpi_request &r = crd_standin_mpi_requests[*request];
	if (r.partner == -1) crd_standin_mpi_abort("MPI_Wait on a request that no send or receive matches (one rank: it would never complete)");
	if (r.partner == -2) crd_standin_mpi_abort("MPI_Wait twice on one request");
	r.partner = -2; /* completed and waited for */
	return MPI_SUCCESS;
}
