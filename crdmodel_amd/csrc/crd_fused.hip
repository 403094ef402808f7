// crd_fused.hip -- the one-launch RK4 step kernels (crd_fused_launch.h): fp64 instantiations, the precision dispatch and the launch
// interface's small functions.  The fp32 instantiations live in crd_fused_f32.hip.
#include "crd_fused_launch.h"

namespace crd {

bool fused_step_supported(int, const SlabDesc &d) { return d.nyl >= 2 * kStepHalo; }

bool fused_two_steps_supported(const SlabDesc &d) { return d.nyl >= 4 * kStepHalo && kernel_model(d) != kModelDiffusionOnly; }

// What the plan arithmetic is told about the kernels of a precision and model (crd_fused_launch.h: kTraits).
static const plan::KernelTraits &kernel_traits(int precision, int model)
{
	const bool f64 = precision == CRD_PRECISION_F64;
	switch (model) {
	case CRD_MODEL_FHN: return f64 ? kTraits<double, CRD_MODEL_FHN> : kTraits<float, CRD_MODEL_FHN>;
	case CRD_MODEL_GOLDBETER: return f64 ? kTraits<double, CRD_MODEL_GOLDBETER> : kTraits<float, CRD_MODEL_GOLDBETER>;
	default: return f64 ? kTraits<double, kModelDiffusionOnly> : kTraits<float, kModelDiffusionOnly>;
	}
}

// Steps one launch of this slab takes when the plan asks for `want` (1 .. 3): crd_fused_plan.h has the rule, steps_per_launch -- the
// one the launcher holds its calls to.
int fused_steps_supported(int precision, const SlabDesc &d, int want)
{
	const plan::KernelTraits &k = kernel_traits(precision, kernel_model(d));
	return plan::steps_per_launch(k, {d.nx, d.nyl, d.wrap != 0, false, fused_scalar_rows_addressable(d.nx, fused_addressed_rows(d), k.real_bytes), false}, want);
}

long fused_addressed_rows(const SlabDesc &d) { return (long)d.nyl + (d.wrap ? 0L : 2L * kGhost); }

// Chunk mode 3 (eight wavefronts per block strip): where a launch of the plan is the three-step fp64 FHN kernel's (crd_fused_impl.h: kCanWide).
bool fused_wide_supported(int precision, const SlabDesc &d, int want_steps)
{
	return precision == CRD_PRECISION_F64 && kernel_model(d) == CRD_MODEL_FHN && fused_steps_supported(precision, d, want_steps) == 3;
}

int fused_max_items(const SlabDesc &d)
{
	// upper bound on the work items of any launch on this slab: the narrowest strips, the shortest chunks the heuristic uses
	// (4 rows: launches that leave most CUs idle, fused_chunk_rows)
	const int strips = (d.nx + (kValid - 2) - 1) / (kValid - 2);
	return strips * ((d.nyl + 2 * kGhost + 3) / 4 + 2);
}

int device_cus()
{
	// compute units of a device of this node (the GPUs of a node are alike); initialised once, also when several issuing threads of a
	// LOCAL group arrive together
	static const int cus = [] {
		int dev = 0;
		hipDeviceProp_t prop;
		const int n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
		(void)hipGetLastError();
		return n;
	}();
	return cus;
}

const char *fused_kernel_name(int, int) { return "crd_rk4_fused_step_kernel"; }

int fused_default_columns(int precision, int nx) { return (precision == CRD_PRECISION_F32 && nx % 2 == 0) ? 2 : 1; }

int fused_plan_candidates() { return plan::kNumPlanCandidates; }

bool fused_plan_candidate(int index, int *chunk_mode, int *mapping, int *cols, int *nt, int *steps)
{
	if (index < 0 || index >= plan::kNumPlanCandidates) return false;
	*steps = plan::kPlanCandidates[index].steps;
	*chunk_mode = plan::kPlanCandidates[index].one_round;
	*mapping = plan::kPlanCandidates[index].remap;
	*cols = plan::kPlanCandidates[index].cols;
	*nt = plan::kPlanCandidates[index].nt;
	return true;
}

hipError_t launch_sum_partials(const double *partials, int n, double *out, hipEvent_t done, hipStream_t s)
{
	clear_launch_status();
	if (done) hipExtLaunchKernelGGL(crd_sum_partials_kernel, dim3(1), dim3(256), 0, s, nullptr, done, 0, partials, n, out);
	else crd_sum_partials_kernel<<<1, 256, 0, s>>>(partials, n, out);
	return launch_status();
}

hipError_t launch_fused_step(int precision, const SlabDesc &d, const FusedCall &c, int row_begin, int row_end, int row_begin2, int row_end2,
                             hipStream_t s)
{
	static_assert(kApron == kStepHalo && kGhost >= kStepHalo, "the planes carry at least the ghost rows one fused step consumes");
	const int model = kernel_model(d);
	if (precision != CRD_PRECISION_F64) return launch_fused_step_f32(d, c, row_begin, row_end, row_begin2, row_end2, s);
	switch (model) {
	case CRD_MODEL_FHN: return launch_fused_t<double, CRD_MODEL_FHN>(d, c, row_begin, row_end, row_begin2, row_end2, d.js, d.ny, s);
	case CRD_MODEL_GOLDBETER: return launch_fused_t<double, CRD_MODEL_GOLDBETER>(d, c, row_begin, row_end, row_begin2, row_end2, d.js, d.ny, s);
	default: return launch_fused_t<double, kModelDiffusionOnly>(d, c, row_begin, row_end, row_begin2, row_end2, d.js, d.ny, s);
	}
}

}  // namespace crd
