// crd_jacobian.cpp -- entry points of the split right-hand side and of J(t, y) v (crd_rhs_part_* / crd_jtimes_*, include/crd.h):
// the halo exchange of the vector the stencil reads, then one launch of crd_jacobian.hip per slab.  Host code only.
#include <vector>

#include "crd_ctx.h"

using namespace crd;

namespace {

bool valid_part(int part) { return part == CRD_PART_FULL || part == CRD_PART_DIFFUSION || part == CRD_PART_REACTION; }

// A diffusion-only Goldbeter context has no absorbing rows in f (crd_device.h: kModelDiffusionOnly), so none in its parts or in J.
int absorb_flag(const crd_ctx *c, double t) { return absorbing(c, t) && !c->desc.just_diffusion ? 1 : 0; }

// What every entry point refuses, and what the collective parts refuse of a context on its own: the division of crd_rhs_device.
int check_ctx(crd_ctx *c, int part, const char *group_entry)
{
	if (!valid_part(part)) return fail(c, CRD_EINVAL, "part must be CRD_PART_FULL, CRD_PART_DIFFUSION or CRD_PART_REACTION");
	if (c->d0 > 1) return fail(c, CRD_ESTATE, "theta-blocks have neither the parts of f nor J v");
	if (part == CRD_PART_REACTION || !group_entry) return CRD_OK;  // pointwise: nothing to exchange, any context on its own
	if (c->halo < 0) return fail(c, CRD_ESTATE, "multi-slab context is not wired (crd_comm_attach_local / crd_comm_init_rccl)");
	if (c->halo == CRD_HALO_LOCAL) return fail(c, CRD_ESTATE, std::string("LOCAL groups evaluate this through ") + group_entry);
	return CRD_OK;
}

// Exchange() on an RCCL ring for the vector x (src/FHNmodel_torus.cpp:775-950): pack var0 of its first / last row, swap with the
// ring neighbours into the ghost strips -- the exchange of crd_rhs_device.
int exchange_rccl(crd_ctx *c, const void *x)
{
	const ncclDataType_t dt = c->p.precision == CRD_PRECISION_F64 ? ncclDouble : ncclFloat;
	crd_halo_op ops[4];
	if (crd_halo_plan(c->slab, c->n_slabs, c->nyl, 1, ops) != CRD_OK) return fail(c, CRD_EINVAL, "bad halo plan");
	HIP_TRY(c, launch_aos_row_extract(c->p.precision, x, c->edge_lo, c->nx, 0, c->compute));
	HIP_TRY(c, launch_aos_row_extract(c->p.precision, x, c->edge_hi, c->nx, c->nyl - 1, c->compute));
	NCCL_TRY(c, g_rccl.GroupStart());
	for (const crd_halo_op &op : ops) {
		if (op.is_send) NCCL_TRY(c, g_rccl.Send(op.row_begin == 0 ? c->edge_lo : c->edge_hi, (size_t)c->nx, dt, op.peer, c->nccl, c->compute));
		else NCCL_TRY(c, g_rccl.Recv(op.row_begin < 0 ? c->ghost_lo : c->ghost_hi, (size_t)c->nx, dt, op.peer, c->nccl, c->compute));
	}
	NCCL_TRY(c, g_rccl.GroupEnd());
	return CRD_OK;
}

// ... and in a LOCAL group of phi-slabs: every slab packs the edge rows of its x[k], then pulls its two neighbours' strips; the
// exchange of crd_group_rhs_device.  The caller launches on each compute stream behind it and synchronises every slab afterwards.
int exchange_local(crd_ctx *const *ctxs, int n, const void *const *x)
{
	for (int k = 0; k < n; k++) {
		crd_ctx *c = ctxs[k];
		if (int rc = set_device(c)) return rc;
		HIP_TRY(c, launch_aos_row_extract(c->p.precision, x[k], c->edge_lo, c->nx, 0, c->compute));
		HIP_TRY(c, launch_aos_row_extract(c->p.precision, x[k], c->edge_hi, c->nx, c->nyl - 1, c->compute));
		HIP_TRY(c, hipEventRecord(c->ev_edges, c->compute));
	}
	for (int k = 0; k < n; k++) {
		crd_ctx *c = ctxs[k];
		if (int rc = set_device(c)) return rc;
		crd_ctx *prev = c->neighbour(0, -1), *next = c->neighbour(0, +1);
		const size_t bytes = (size_t)c->nx * c->real_size;
		HIP_TRY(c, hipStreamWaitEvent(c->compute, prev->ev_edges, 0));
		HIP_TRY(c, hipStreamWaitEvent(c->compute, next->ev_edges, 0));
		HIP_TRY(c, hipMemcpyPeerAsync(c->ghost_lo, c->device, prev->edge_hi, prev->device, bytes, c->compute));
		HIP_TRY(c, hipMemcpyPeerAsync(c->ghost_hi, c->device, next->edge_lo, next->device, bytes, c->compute));
	}
	return CRD_OK;
}

// One slab's launch: v == nullptr, a part of f at y; else J(t, y) v.
int launch_one(crd_ctx *c, double t, int part, const void *y, const void *v, void *out)
{
	if (v) HIP_TRY(c, launch_jtimes_aos(c->p.precision, c->desc, part, absorb_flag(c, t), y, v, out, c->ghost_lo, c->ghost_hi, c->compute));
	else HIP_TRY(c, launch_rhs_part_aos(c->p.precision, c->desc, part, absorb_flag(c, t), y, out, c->ghost_lo, c->ghost_hi, c->compute));
	return CRD_OK;
}

int one_device(crd_ctx *c, double t, int part, const void *y, const void *v, void *out, const char *group_entry)
{
	if (int rc = check_ctx(c, part, group_entry)) return rc;
	if (int rc = set_device(c)) return rc;
	if (part != CRD_PART_REACTION && c->halo == CRD_HALO_RCCL)
		if (int rc = exchange_rccl(c, v ? v : y)) return rc;
	return launch_one(c, t, part, y, v, out);
}

int group_device(crd_ctx *const *ctxs, int n, double t, int part, const void *const *y, const void *const *v, void *const *out, const char *group_entry)
{
	if (int rc = check_group(ctxs, n)) return rc;
	if (!y || !out) return CRD_EINVAL;
	for (int k = 0; k < n; k++)
		if (!y[k] || !out[k] || (v && !v[k])) return CRD_EINVAL;
	if (n == 1) return one_device(ctxs[0], t, part, y[0], v ? v[0] : nullptr, out[0], group_entry);
	for (int k = 0; k < n; k++) {
		if (int rc = check_ctx(ctxs[k], part, nullptr)) return rc;
		if (part != CRD_PART_REACTION && ctxs[k]->halo != CRD_HALO_LOCAL) return fail(ctxs[0], CRD_ESTATE, "group is not attached");
	}
	if (part != CRD_PART_REACTION)
		if (int rc = exchange_local(ctxs, n, v ? v : y)) return rc;
	for (int k = 0; k < n; k++) {
		if (int rc = set_device(ctxs[k])) return rc;
		if (int rc = launch_one(ctxs[k], t, part, y[k], v ? v[k] : nullptr, out[k])) return rc;
	}
	// the edge buffers may be repacked by the next call only after every neighbour has copied them
	for (int k = 0; k < n; k++) {
		if (int rc = set_device(ctxs[k])) return rc;
		HIP_TRY(ctxs[k], hipStreamSynchronize(ctxs[k]->compute));
	}
	return CRD_OK;
}

size_t vector_bytes(const crd_ctx *c) { return 2 * (size_t)c->nx * (size_t)c->nyl * c->real_size; }

// y (and v) into the staging buffers of the context, on its compute stream
int stage_up(crd_ctx *c, const void *y, const void *v)
{
	if (int rc = set_device(c)) return rc;
	if (int rc = ensure_staging(c, 2 * (size_t)c->nx * (size_t)c->nyl * 8)) return rc;
	HIP_TRY(c, hipMemcpyAsync(c->stage_in, y, vector_bytes(c), hipMemcpyHostToDevice, c->compute));
	if (!v) return CRD_OK;
	if (c->stage_v_bytes < vector_bytes(c)) {
		if (c->stage_v) (void)hipFree(c->stage_v);
		c->stage_v = nullptr;
		c->stage_v_bytes = 0;
		HIP_TRY(c, hipMalloc(&c->stage_v, vector_bytes(c)));
		c->stage_v_bytes = vector_bytes(c);
	}
	HIP_TRY(c, hipMemcpyAsync(c->stage_v, v, vector_bytes(c), hipMemcpyHostToDevice, c->compute));
	return CRD_OK;
}

int stage_down(crd_ctx *c, void *out)
{
	if (int rc = set_device(c)) return rc;
	HIP_TRY(c, hipMemcpyAsync(out, c->stage_out, vector_bytes(c), hipMemcpyDeviceToHost, c->compute));
	HIP_TRY(c, hipStreamSynchronize(c->compute));
	return CRD_OK;
}

int one_host(crd_ctx *c, double t, int part, const void *y, const void *v, void *out, const char *group_entry)
{
	if (int rc = check_ctx(c, part, group_entry)) return rc;
	if (int rc = stage_up(c, y, v)) return rc;
	if (int rc = one_device(c, t, part, c->stage_in, v ? c->stage_v : nullptr, c->stage_out, group_entry)) return rc;
	return stage_down(c, out);
}

int group_host(crd_ctx *const *ctxs, int n, double t, int part, const void *const *y, const void *const *v, void *const *out, const char *group_entry)
{
	if (int rc = check_group(ctxs, n)) return rc;
	if (!y || !out) return CRD_EINVAL;
	std::vector<const void *> din((size_t)n), dv((size_t)n);
	std::vector<void *> dout((size_t)n);
	for (int k = 0; k < n; k++) {
		if (!y[k] || !out[k] || (v && !v[k])) return CRD_EINVAL;
		if (int rc = check_ctx(ctxs[k], part, nullptr)) return rc;
	}
	for (int k = 0; k < n; k++) {
		if (int rc = stage_up(ctxs[k], y[k], v ? v[k] : nullptr)) return rc;
		din[(size_t)k] = ctxs[k]->stage_in;
		dv[(size_t)k] = ctxs[k]->stage_v;
		dout[(size_t)k] = ctxs[k]->stage_out;
	}
	if (int rc = group_device(ctxs, n, t, part, din.data(), v ? dv.data() : nullptr, dout.data(), group_entry)) return rc;
	for (int k = 0; k < n; k++)
		if (int rc = stage_down(ctxs[k], out[k])) return rc;
	return CRD_OK;
}

}  // namespace

extern "C" {

int crd_rhs_part_device(crd_ctx *c, double t, int part, const void *y, void *ydot)
{
	if (!c || !y || !ydot) return CRD_EINVAL;
	return one_device(c, t, part, y, nullptr, ydot, "crd_group_rhs_part_device");
}

int crd_rhs_part_host(crd_ctx *c, double t, int part, const void *y, void *ydot)
{
	if (!c || !y || !ydot) return CRD_EINVAL;
	return one_host(c, t, part, y, nullptr, ydot, "crd_group_rhs_part_host");
}

int crd_jtimes_device(crd_ctx *c, double t, int part, const void *y, const void *v, void *jv)
{
	if (!c || !y || !v || !jv) return CRD_EINVAL;
	return one_device(c, t, part, y, v, jv, "crd_group_jtimes_device");
}

int crd_jtimes_host(crd_ctx *c, double t, int part, const void *y, const void *v, void *jv)
{
	if (!c || !y || !v || !jv) return CRD_EINVAL;
	return one_host(c, t, part, y, v, jv, "crd_group_jtimes_host");
}

int crd_group_rhs_part_device(crd_ctx *const *ctxs, int n, double t, int part, const void *const *y, void *const *ydot)
{
	return group_device(ctxs, n, t, part, y, nullptr, ydot, "crd_group_rhs_part_device");
}

int crd_group_rhs_part_host(crd_ctx *const *ctxs, int n, double t, int part, const void *const *y, void *const *ydot)
{
	return group_host(ctxs, n, t, part, y, nullptr, ydot, "crd_group_rhs_part_host");
}

int crd_group_jtimes_device(crd_ctx *const *ctxs, int n, double t, int part, const void *const *y, const void *const *v, void *const *jv)
{
	if (!v) return CRD_EINVAL;
	return group_device(ctxs, n, t, part, y, v, jv, "crd_group_jtimes_device");
}

int crd_group_jtimes_host(crd_ctx *const *ctxs, int n, double t, int part, const void *const *y, const void *const *v, void *const *jv)
{
	if (!v) return CRD_EINVAL;
	return group_host(ctxs, n, t, part, y, v, jv, "crd_group_jtimes_host");
}

}  // extern "C"
