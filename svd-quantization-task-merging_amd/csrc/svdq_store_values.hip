// svdq_store_values.hip -- what the four merges over every task's own value (svdq_store_values.h) need exactly once: the
// coefficient kernel and the argument check of their entry points.  Compiled with -ffp-contract=off like its users: the
// coefficients are rounded as k_task_coeff (svdq_merge.hip) rounds them.

#include "svdq_store_values.h"

// cbar [P][n_out][N]: slot j of parameter p holds the coefficients of plan task slot_task[p][j] exactly as k_task_coeff
// (svdq_merge.hip) leaves them (0 + c * 1, rounded as there); a slot whose task_map entry is < 0 holds zeros.
__global__ __launch_bounds__(64) void k_store_coeff(int NT, int stages, int n_out, const int32_t *__restrict__ slot_task,
                                                    const int32_t *__restrict__ task_map,
                                                    const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                                    const uint16_t *__restrict__ chigh, const uint8_t *__restrict__ codes,
                                                    const float *__restrict__ scale, const float *__restrict__ zp,
                                                    float *__restrict__ cbar) {
    const int p = blockIdx.x, i = threadIdx.x, n = NT;
    const int k = k_in[p], r = r_in[p];
    if (i >= n) return;
    for (int s = 0; s < n_out; ++s) {
        const int t = slot_task[(size_t)p * n_out + s];
        float acc = 0.f;
        if (i < r && task_map[(size_t)p * n_out + s] >= 0 && (unsigned)t < (unsigned)n)
            acc = __fadd_rn(acc, __fmul_rn(task_coeff(p, t, i, n, k, stages, chigh, codes, scale, zp), 1.f));
        cbar[((size_t)p * n_out + s) * n + i] = acc;
    }
}

void store_coeff_launch(const svdq_plan *pl, const SmallView &sv, const int32_t *slot_task, const int32_t *task_map,
                        int n_out, float *cbar, hipStream_t st) {
    hipLaunchKernelGGL(k_store_coeff, dim3(pl->n_params), dim3(64), 0, st, pl->n_tasks, pl->cfg.rtvq_stages, n_out,
                       slot_task, task_map, sv.k, sv.r, sv.chigh, sv.codes, sv.scale, sv.zp, cbar);
}

int store_args_ok(const char *who, const svdq_plan *pl, const void *small, const void *basis, const float *mean,
                  const int32_t *slot_task, const int32_t *task_map, int32_t n_out, int32_t n_tasks, const void *state,
                  const void *work) {
    if (!pl || !small || !basis || !slot_task || !task_map || !state || !work) {
        svdq_set_error("%s: plan, small, basis, slot_task, task_map, state and work are required", who);
        return SVDQ_EINVAL;
    }
    if (n_out < 1 || n_out > SVDQ_MAX_TASKS || n_tasks < 1 || n_tasks > SVDQ_MAX_TASKS) {
        svdq_set_error("%s: n_out and n_tasks must be in [1, %d], got %d and %d", who, SVDQ_MAX_TASKS, n_out, n_tasks);
        return SVDQ_EINVAL;
    }
    return svdq_refuse_no_mean(who, pl, mean) ? SVDQ_EINVAL : SVDQ_OK;
}
