/* Stand-in for <mpi.h>, written from the eleven calls the reference programs make.  Plumbing only -- no arithmetic on data.
 *
 * ONE RANK (CRD_REF_MPI_SIZE unset, empty or 1): size 1, rank 0; MPI_Dims_create -> {1, 1}; the Cartesian grid is periodic, so
 * MPI_Cart_shift names this rank as the neighbour in both directions.  A message to self is matched as MPI matches it: posted
 * receives and sends are paired in posting order, a receive taking the earliest unmatched send whose tag it accepts (MPI_ANY_TAG
 * accepts all); the bytes move when the later of the pair is posted.  Anything that is not such a self-exchange aborts with a
 * message: a peer other than rank 0, a pair whose byte counts differ, a wait on a request that found no partner, and requests
 * still unmatched at MPI_Finalize.
 *
 * TWO OR FOUR RANKS (CRD_REF_MPI_SIZE = 2 or 4, CRD_REF_MPI_RANK = this process's rank, CRD_REF_MPI_DIR = a directory all ranks
 * share, empty at the start): every rank is a process of its own, started side by side in one working directory as mpirun would.
 *   MPI_Dims_create   {2, 1} for 2 ranks, {2, 2} for 4: the balanced, non-increasing factorisation.  Any other size aborts.
 *   MPI_Cart_create   reorder = 0: ranks are numbered row-major, rank = c0 dims[1] + c1.  Only a periodic grid of the dims above.
 *   MPI_Cart_shift    (direction, +1), periodic: source = the rank at coordinate - 1, dest = the rank at coordinate + 1.
 *   MPI_Isend         copies its buffer (behind the tag) into DIR/msg.<source>.<dest>.<n>, n counting this rank's sends to <dest>
 *                     from 0; the file is written under a temporary name and renamed, so a reader sees all of it or none.
 *   MPI_Irecv         takes the next sequence number of its source when it is POSTED: MPI's non-overtaking order.  With two ranks
 *                     in a direction both receives of a rank name the same source with MPI_ANY_TAG, and the order of posting alone
 *                     says which message is whose.  A receive with a tag of its own must meet that tag (no matching out of order).
 *   MPI_Wait          on a receive polls for its file until the deadline (CRD_REF_MPI_DEADLINE seconds, 60 unless set), requires the
 *                     posted byte count, copies the bytes and removes the file; on a send it only marks the request as waited for.
 *   MPI_Finalize      requires every request waited for and no message to this rank left in DIR.
 * Every way this can go wrong aborts with a message: a size or tag mismatch, a wait past its deadline (a lost rank ends the run
 * and does not hang it), a second wait on one request, requests or files left at MPI_Finalize, a peer outside the grid, a rank
 * outside the size, a directory that cannot be written.  No threads, no sockets. */
#pragma once
#include <dirent.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

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
	int partner; /* -1 while unmatched (several ranks: while not waited for), -2 once waited for */
	int peer;    /* several ranks: the other rank, and the message's sequence number between the two */
	long seq;
};
enum { CRD_STANDIN_MPI_MAX_REQUESTS = 64, CRD_STANDIN_MPI_MAX_RANKS = 4 };
static crd_standin_mpi_request crd_standin_mpi_requests[CRD_STANDIN_MPI_MAX_REQUESTS];
static int crd_standin_mpi_count = 0;

/* several ranks: what the environment said (size 0 = not read yet), the grid MPI_Cart_create made, the per-peer message counters */
static int crd_standin_mpi_size = 0, crd_standin_mpi_rank = 0;
static int crd_standin_mpi_dims[2] = {1, 1};
static long crd_standin_mpi_sent[CRD_STANDIN_MPI_MAX_RANKS], crd_standin_mpi_received[CRD_STANDIN_MPI_MAX_RANKS];
static const char *crd_standin_mpi_dir = NULL;
static double crd_standin_mpi_deadline = 60.0;

static inline void crd_standin_mpi_abort(const char *what)
{
	if (crd_standin_mpi_size > 1) fprintf(stderr, "MPI stand-in, rank %d of %d: %s\n", crd_standin_mpi_rank, crd_standin_mpi_size, what);
	else fprintf(stderr, "one-rank MPI stand-in: %s\n", what);
	abort();
}

/* The environment, read once.  Returns the number of ranks. */
static inline int crd_standin_mpi_ranks()
{
	if (crd_standin_mpi_size > 0) return crd_standin_mpi_size;
	const char *size = getenv("CRD_REF_MPI_SIZE");
	if (!size || !*size || strcmp(size, "1") == 0) return crd_standin_mpi_size = 1;
	const char *rank = getenv("CRD_REF_MPI_RANK"), *dir = getenv("CRD_REF_MPI_DIR"), *deadline = getenv("CRD_REF_MPI_DEADLINE");
	char *end = NULL;
	const long n = strtol(size, &end, 10);
	if (*end || (n != 2 && n != 4)) crd_standin_mpi_abort("CRD_REF_MPI_SIZE is not 1, 2 or 4 (the reference's exchange is the periodic halo for at most two ranks per direction)");
	crd_standin_mpi_size = (int)n;
	const long r = rank && *rank ? strtol(rank, &end, 10) : -1;
	if (r < 0 || r >= n || *end) {
		crd_standin_mpi_rank = -1;
		crd_standin_mpi_abort("CRD_REF_MPI_RANK is not a rank of CRD_REF_MPI_SIZE");
	}
	crd_standin_mpi_rank = (int)r;
	if (!dir || !*dir || access(dir, W_OK | X_OK) != 0) crd_standin_mpi_abort("CRD_REF_MPI_DIR is not a directory this rank can write to");
	crd_standin_mpi_dir = dir;
	if (deadline && *deadline) {
		crd_standin_mpi_deadline = strtod(deadline, &end);
		if (*end || !(crd_standin_mpi_deadline > 0.0)) crd_standin_mpi_abort("CRD_REF_MPI_DEADLINE is not a positive number of seconds");
	}
	return crd_standin_mpi_size;
}

static inline int MPI_Init(int *, char ***)
{
	crd_standin_mpi_ranks();
	return MPI_SUCCESS;
}

static inline int MPI_Finalize()
{
	for (int k = 0; k < crd_standin_mpi_count; k++)
		if (crd_standin_mpi_requests[k].partner == -1)
			crd_standin_mpi_abort(crd_standin_mpi_ranks() == 1 ? "a request was still unmatched at MPI_Finalize" : "a request was never waited for at MPI_Finalize");
	if (crd_standin_mpi_ranks() == 1) return MPI_SUCCESS;
	DIR *d = opendir(crd_standin_mpi_dir);
	if (!d) crd_standin_mpi_abort("MPI_Finalize: the message directory cannot be read");
	while (struct dirent *e = readdir(d)) {
		int src = -1, dst = -1;
		long seq = -1;
		if (sscanf(e->d_name, "msg.%d.%d.%ld", &src, &dst, &seq) == 3 && dst == crd_standin_mpi_rank)
			crd_standin_mpi_abort("a message to this rank was left unreceived at MPI_Finalize");
	}
	closedir(d);
	return MPI_SUCCESS;
}

static inline int MPI_Comm_rank(MPI_Comm, int *rank)
{
	*rank = crd_standin_mpi_ranks() == 1 ? 0 : crd_standin_mpi_rank;
	return MPI_SUCCESS;
}

static inline int MPI_Comm_size(MPI_Comm, int *size)
{
	*size = crd_standin_mpi_ranks();
	return MPI_SUCCESS;
}

static inline int MPI_Dims_create(int nnodes, int ndims, int *dims)
{
	if (nnodes != crd_standin_mpi_ranks()) crd_standin_mpi_abort(crd_standin_mpi_ranks() == 1 ? "MPI_Dims_create for more than one rank" : "MPI_Dims_create for another number of ranks than the run has");
	if (nnodes == 1) {
		for (int k = 0; k < ndims; k++) dims[k] = 1;
		return MPI_SUCCESS;
	}
	if (ndims != 2 || dims[0] != 0 || dims[1] != 0) crd_standin_mpi_abort("MPI_Dims_create: not two free dimensions");
	dims[0] = 2; /* 2 = 2 x 1, 4 = 2 x 2 */
	dims[1] = nnodes / 2;
	return MPI_SUCCESS;
}

static inline int MPI_Cart_create(MPI_Comm, int ndims, int *dims, int *periods, int reorder, MPI_Comm *cart)
{
	if (crd_standin_mpi_ranks() == 1) {
		for (int k = 0; k < ndims; k++)
			if (dims[k] != 1 || periods[k] != 1) crd_standin_mpi_abort("MPI_Cart_create: not a periodic 1 x 1 grid");
	} else {
		if (ndims != 2 || dims[0] != 2 || dims[0] * dims[1] != crd_standin_mpi_size || periods[0] != 1 || periods[1] != 1 || reorder != 0)
			crd_standin_mpi_abort("MPI_Cart_create: not the periodic 2 x (size / 2) grid of MPI_Dims_create with reorder = 0");
		crd_standin_mpi_dims[0] = dims[0];
		crd_standin_mpi_dims[1] = dims[1];
	}
	*cart = MPI_COMM_WORLD;
	return MPI_SUCCESS;
}

static inline int MPI_Cart_get(MPI_Comm, int maxdims, int *dims, int *periods, int *coords)
{
	if (crd_standin_mpi_ranks() == 1) {
		for (int k = 0; k < maxdims; k++) {
			dims[k] = 1;
			periods[k] = 1;
			coords[k] = 0;
		}
		return MPI_SUCCESS;
	}
	if (maxdims != 2) crd_standin_mpi_abort("MPI_Cart_get: not two dimensions");
	for (int k = 0; k < 2; k++) {
		dims[k] = crd_standin_mpi_dims[k];
		periods[k] = 1;
	}
	coords[0] = crd_standin_mpi_rank / crd_standin_mpi_dims[1]; /* row-major: rank = c0 dims[1] + c1 */
	coords[1] = crd_standin_mpi_rank % crd_standin_mpi_dims[1];
	return MPI_SUCCESS;
}

static inline int MPI_Cart_shift(MPI_Comm, int direction, int displacement, int *rank_source, int *rank_dest)
{
	if (crd_standin_mpi_ranks() == 1) {
		*rank_source = 0; /* periodic, one rank per direction: both neighbours are this rank */
		*rank_dest = 0;
		return MPI_SUCCESS;
	}
	if (direction < 0 || direction > 1 || displacement != 1) crd_standin_mpi_abort("MPI_Cart_shift: not a shift by +1 along dimension 0 or 1");
	const int *d = crd_standin_mpi_dims;
	int c[2] = {crd_standin_mpi_rank / d[1], crd_standin_mpi_rank % d[1]}, lo[2] = {c[0], c[1]}, hi[2] = {c[0], c[1]};
	lo[direction] = (c[direction] - 1 + d[direction]) % d[direction];
	hi[direction] = (c[direction] + 1) % d[direction];
	*rank_source = lo[0] * d[1] + lo[1];
	*rank_dest = hi[0] * d[1] + hi[1];
	return MPI_SUCCESS;
}

static inline void crd_standin_mpi_path(char *path, size_t size, const char *kind, int source, int dest, long seq)
{
	if (snprintf(path, size, "%s/%s.%d.%d.%ld", crd_standin_mpi_dir, kind, source, dest, seq) >= (int)size) crd_standin_mpi_abort("CRD_REF_MPI_DIR is too long a path");
}

/* Several ranks: the request's slot; a send also writes its message. */
static inline void crd_standin_mpi_post_ranks(void *buffer, size_t bytes, int peer, int tag, int is_send, MPI_Request *request)
{
	if (peer < 0 || peer >= crd_standin_mpi_size) crd_standin_mpi_abort("a message to or from a rank outside the grid");
	int all_done = 1;
	for (int k = 0; k < crd_standin_mpi_count; k++) all_done &= (crd_standin_mpi_requests[k].partner == -2);
	if (all_done) crd_standin_mpi_count = 0;
	if (crd_standin_mpi_count == CRD_STANDIN_MPI_MAX_REQUESTS) crd_standin_mpi_abort("too many requests in flight");
	const int me = crd_standin_mpi_count++;
	crd_standin_mpi_request &r = crd_standin_mpi_requests[me];
	r.buffer = buffer;
	r.bytes = bytes;
	r.tag = tag;
	r.is_send = is_send;
	r.partner = -1;
	r.peer = peer;
	r.seq = is_send ? crd_standin_mpi_sent[peer]++ : crd_standin_mpi_received[peer]++;
	*request = me;
	if (!is_send) return;
	char tmp[4096], path[4096];
	crd_standin_mpi_path(tmp, sizeof tmp, "tmp", crd_standin_mpi_rank, peer, r.seq);
	crd_standin_mpi_path(path, sizeof path, "msg", crd_standin_mpi_rank, peer, r.seq);
	FILE *fp = fopen(tmp, "wb");
	const int ok = fp && fwrite(&tag, sizeof tag, 1, fp) == 1 && (bytes == 0 || fwrite(buffer, 1, bytes, fp) == bytes);
	if ((fp && fclose(fp) != 0) || !ok || rename(tmp, path) != 0) crd_standin_mpi_abort("MPI_Isend could not write its message into CRD_REF_MPI_DIR");
}

static inline void crd_standin_mpi_post(void *buffer, int count, MPI_Datatype type, int peer, int tag, int is_send, MPI_Request *request)
{
	if (count < 0) crd_standin_mpi_abort("a negative count");
	if (crd_standin_mpi_ranks() > 1) {
		crd_standin_mpi_post_ranks(buffer, (size_t)count * (size_t)type, peer, tag, is_send, request);
		return;
	}
	if (peer != 0) crd_standin_mpi_abort("a message to or from a rank other than 0");
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

/* Several ranks, a receive: poll for the message's file until the deadline, check it, take the bytes, remove it. */
static inline void crd_standin_mpi_receive(crd_standin_mpi_request &r)
{
	char path[4096];
	crd_standin_mpi_path(path, sizeof path, "msg", r.peer, crd_standin_mpi_rank, r.seq);
	struct timespec t0, t;
	clock_gettime(CLOCK_MONOTONIC, &t0);
	FILE *fp;
	while (!(fp = fopen(path, "rb"))) {
		if (errno != ENOENT) crd_standin_mpi_abort("MPI_Wait could not open a message in CRD_REF_MPI_DIR");
		clock_gettime(CLOCK_MONOTONIC, &t);
		if ((double)(t.tv_sec - t0.tv_sec) + 1e-9 * (double)(t.tv_nsec - t0.tv_nsec) > crd_standin_mpi_deadline)
			crd_standin_mpi_abort("MPI_Wait: no message from the receive's source by the deadline (a lost rank, or a send that was never made)");
		usleep(200);
	}
	int tag = 0;
	if (fread(&tag, sizeof tag, 1, fp) != 1) crd_standin_mpi_abort("MPI_Wait: a message without its tag");
	if (r.tag != MPI_ANY_TAG && r.tag != tag) crd_standin_mpi_abort("the next message of the source carries another tag than the receive asks for");
	if (fseek(fp, 0, SEEK_END) != 0 || ftell(fp) < 0) crd_standin_mpi_abort("MPI_Wait: a message that cannot be measured");
	if ((size_t)ftell(fp) - sizeof tag != r.bytes) crd_standin_mpi_abort("a matched send and receive differ in size");
	if (fseek(fp, (long)sizeof tag, SEEK_SET) != 0 || (r.bytes > 0 && fread(r.buffer, 1, r.bytes, fp) != r.bytes)) crd_standin_mpi_abort("MPI_Wait: a message that cannot be read");
	fclose(fp);
	if (unlink(path) != 0) crd_standin_mpi_abort("MPI_Wait could not remove a received message");
}

static inline int MPI_Wait(MPI_Request *request, MPI_Status *)
{
	if (*request < 0 || *request >= crd_standin_mpi_count) crd_standin_mpi_abort("MPI_Wait on an unknown request");
	crd_standin_mpi_request &r = crd_standin_mpi_requests[*request];
	if (r.partner == -2) crd_standin_mpi_abort("MPI_Wait twice on one request");
	if (crd_standin_mpi_ranks() > 1) {
		if (!r.is_send) crd_standin_mpi_receive(r);
	} else if (r.partner == -1)
		crd_standin_mpi_abort("MPI_Wait on a request that no send or receive matches (one rank: it would never complete)");
	r.partner = -2; /* completed and waited for */
	return MPI_SUCCESS;
}
