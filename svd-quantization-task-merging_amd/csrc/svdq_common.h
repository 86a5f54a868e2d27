// svdq_common.h -- shared declarations of the gfx950 SVD-Hybrid compressor library.
//
// Work decomposition:
//   parameter p : D_p rows (elements) x N tasks; the N task deltas are N separate fp32 buffers.
//   block       : 256 consecutive rows of one parameter, staged (centred) in LDS as [task][row].
//   unit        : a run of blocks of one parameter handled by ONE wavefront (= one 64-thread
//                 workgroup).  Each unit emits one fp64 partial N x N matrix per "slot".
//   slot        : with row-set packing (N <= 8) a 16x16 MFMA tile carries two independent
//                 8-task row sets, so a unit has 2 slots; otherwise 1.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svdq.h"

#define SVDQ_BLK_ROWS 256
#define SVDQ_RC 16  // level-2 partial chunks per parameter (k_reduce)
#ifndef SVDQ_XS
#define SVDQ_XS 260  // LDS row stride (floats) of one task's 256-row strip: 256 + pad, multiple of 4 (16-B alignment)
#endif

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct SvdqParam {     // one per parameter (device table)
    int64_t rows;      // D_p (upper bound when rows_dev overrides)
    int64_t slab_off;  // byte offset of the U slab in the packed basis buffer (256-aligned)
    int64_t mean_off;  // float offset in the packed mean buffer (64-aligned)
    int32_t unit_begin;
    int32_t unit_count;
};

struct SvdqUnit {      // one per work unit (device table)
    int32_t param;
    int32_t nrows;     // rows covered by this unit (multiple of 256 except the last unit of a parameter)
    int64_t row0;
};

struct svdq_plan {
    int32_t n_tasks, n_params, n_units, n_slots, ntp, pack;
    svdq_config cfg;
    svdq_sizes sizes;
    svdq_small_layout small;
    // workspace offsets (bytes)
    int64_t ws_gram_off, ws_cpart_off, ws_w_off, ws_c0_off, ws_gram2_off, ws_cpart2_off, ws_flag_off;
    // host copies
    SvdqParam *h_params;
    SvdqUnit *h_units;
    // device tables
    SvdqParam *d_params;
    SvdqUnit *d_units;
    int32_t *d_bits;  // optional per-parameter low_bits (svdq_plan_set_low_bits), NULL = cfg.low_bits everywhere
    int32_t in_type;  // SVDQ_INPUT_*: element type of the task / fine-tuned / base tensors (svdq_plan_set_input_type)
    // task-Gram by-product (svdq_plan_set_task_gram): pass 1 also leaves the side sums a = Tc^T m, s = m^T m
    int32_t task_gram;
    int64_t ws_base_bytes;              // workspace_bytes without the by-product's regions
    int64_t ws_side_off, ws_side2_off;  // [n_units][N + 1] unit partials, [n_params * SVDQ_RC][N + 1] (k_reduce_side)
};

__host__ __device__ static inline int64_t svdq_align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// padded task count the streaming kernels are instantiated for (multiple of 4, <= 32)
static inline int svdq_ntp(int n) { return (n + 3) / 4 * 4; }

// svdq_config.reserved: the measurement switches (bit meanings: include/svdq.h)
enum {
    SVDQ_SW_REVERSE = 1,         // pass 2 walks the units in reverse order
    SVDQ_SW_GRAM_F32 = 2,        // fp32-product Gram for every N
    SVDQ_SW_XCD_CHUNKED = 4,     // XCD-chunked unit order in both passes
    SVDQ_SW_PASS2_TWO_WAVE = 8,  // N = 17..20: the two-wave pass 2
};

// What the streaming passes of one compress step read.  Which pointers are set selects the kernels' MODE.
struct SvdqInput {
    const void *ptrs;         // device table [n_params * n_tasks] of task (with base: fine-tuned) tensors
    const int64_t *rows_dev;  // NULL, or per-parameter row counts [n_params]
    const void *index;        // NULL, or device table [n_params] of int32 index lists (gather, svdq_compress_gather)
    const void *mask;         // NULL, or device table [n_params] of combined-mask byte tensors (walk, svdq_compress_masked)
    const int64_t *ustart;    // NULL, or the walk's per-unit source start positions [n_units] (svdq_maskset_*_starts)
    const void *base;         // NULL, or device table [n_params] of base tensors (minus-base, svdq_compress_from_base)

    // the kernels' MODE template value: 0 plain, 1 gather, 2 base, 3 gather + base, 4 walk, 6 walk + base
    int mode() const { return (ustart ? 4 : (index ? 1 : 0)) | (base ? 2 : 0); }
    // the streaming kernels' two `aux` tables: the walk reads its masks where the gather reads its index lists
    const void *const *aux() const { return static_cast<const void *const *>(mask ? mask : index); }
    const void *const *aux2() const { return static_cast<const void *const *>(base); }
    const float *const *tensors() const { return static_cast<const float *const *>(ptrs); }
};

void svdq_set_error(const char *fmt, ...);
// SVDQ_OK for an fp32-input plan; otherwise SVDQ_EUNSUPPORTED with the error text naming `who` (entry points whose
// kernels read task tensors as fp32 only)
int svdq_require_f32_input(const svdq_plan *pl, const char *who);
// what a launcher returns: `launched` is its dispatch's result (svdq_dispatch.h).  Which (mode, input type, task
// count) combinations have a kernel is svdq_check_input's business (svdq_api.hip), so false here is a library bug.
int svdq_launch_status(bool launched, const char *kernel);

// launchers (defined in the .hip files)
// only: NULL, or a device table [n_params] of int32 -- parameters whose entry is 0 are skipped (refinement pass)
// f64: accumulate the products with v_mfma_f64_16x16x4_f64 (exact) instead of fp32 MFMA
int svdq_launch_gram(const svdq_plan *pl, const SvdqInput &in, double *gram_part, int unit0, int nunits, int center,
                     int f64, const int32_t *only, hipStream_t st, double *side_part = nullptr);
int svdq_launch_gram_total(const svdq_plan *pl, const double *part2, double *out, hipStream_t st);
// task-Gram by-product: the unit side partials -> SVDQ_RC chunks per parameter (k_reduce's order), and
// out = total(part2) + a 1^T + 1 a^T + s 1 1^T with a, s the totals of side2
int svdq_launch_reduce_side(const svdq_plan *pl, const double *side, double *side2, hipStream_t st);
int svdq_launch_gram_total_side(const svdq_plan *pl, const double *part2, const double *side2, double *out,
                                hipStream_t st);
// reverse: the unit order switches (SVDQ_SW_REVERSE | SVDQ_SW_XCD_CHUNKED) of cfg.reserved
int svdq_launch_basis_project(const svdq_plan *pl, const SvdqInput &in, const float *W, const int32_t *k_dev,
                              const int32_t *r_dev, uint8_t *basis, float *mean, double *cpart, int unit0, int nunits,
                              int reverse, hipStream_t st);
// pass 2 of the mask-walk mode for 16 < N <= 32 (svdq_project_walk.hip)
int svdq_launch_basis_project_walk32(const svdq_plan *pl, const SvdqInput &in, const float *W, const int32_t *k_dev,
                                     const int32_t *r_dev, uint8_t *basis, float *mean, double *cpart, int unit0,
                                     int nunits, int reverse, hipStream_t st);
// refine_out: NULL, or a device table [n_params] that receives 1 where a singular value lies in the band the fp32-product
// Gram does not resolve (then the caller re-accumulates those parameters in fp64 and calls again with only = that table)
int svdq_launch_eig(const svdq_plan *pl, const SvdqInput &in, const double *gram_part, float *W, double *c0,
                    uint8_t *small, int param0, int nparams, const int32_t *only, int32_t *refine_out, hipStream_t st);
int svdq_launch_reduce(const svdq_plan *pl, const double *part, double *part2, int param0, int nparams,
                       const int32_t *only, hipStream_t st);
int svdq_launch_coeff(const svdq_plan *pl, const double *cpart, const double *c0, uint8_t *small, int param0,
                      int nparams, hipStream_t st);
