// svdq_project_walk.hip -- pass 2 in the mask-walk mode for 16 < N <= 32 tasks (svdq_compress_masked).
// The two-wave kernels that serve N > 16 otherwise (svdq_project.hip) live on a one-block-ahead prefetch at 218-243
// registers; the walk keeps a chunk's overflow rows in registers across the block's compute phase and cannot share that
// budget.  So the walk takes the ONE-wave kernel here -- the form N <= 16 uses, the whole strip and
// both 16-column halves in one wavefront: 256 vector + 95-152 accumulation registers, one wave per SIMD, no scratch.
// Slower per byte than the two-wave kernels, but it reads the mask byte beside the rows instead of a 4-byte index per
// selected row, builds no index lists, and hands the batched consumers the same unit starts.  Which task counts the
// walk covers and what its artifacts are bit-identical to: include/svdq.h, svdq_compress_masked.  A translation unit
// of its own so that the build compiles it beside svdq_project.hip.
#include "svdq_project_unit.h"
#include "svdq_dispatch.h"

int svdq_launch_basis_project_walk32(const svdq_plan *pl, const SvdqInput &in, const float *W, const int32_t *k_dev,
                                     const int32_t *r_dev, uint8_t *basis, float *mean, double *cpart, int unit0,
                                     int nunits, int reverse, hipStream_t st) {
    const bool ok = svdq_dispatch_int<20, 24, 28, 32>(pl->ntp, [&](auto ntp_c) {
        constexpr int NTP = ntp_c;
        return svdq_dispatch_bool(pl->cfg.fp16 != 0, [&](auto f16_c) {
            constexpr bool F16 = f16_c;
            hipLaunchKernelGGL((k_basis_project<NTP, F16, 4, false>), dim3(nunits), dim3(64), 0, st, pl->d_params,
                               pl->d_units, in.tensors(), in.rows_dev, pl->n_tasks, pl->cfg.center, W, k_dev, r_dev, basis,
                               mean, cpart, unit0, reverse, in.aux(), in.aux2(), in.ustart);
            return true;
        });
    });
    return svdq_launch_status(ok, "k_basis_project (walk above 16 tasks)");
}
