/*
 * include/svdq.h -- C ABI of libsvdq_hip.so: the MI355X (gfx950) SVD-Hybrid task-vector
 * compressor hot path.  extern "C", plain pointers and sizes, no framework types.
 *
 * The reference (mgradyn/SVD-Quantization-Task-Merging) is pure Python and has NO FFI /
 * operator interface for this path: its boundary is a set of
 * Python callables exchanging dicts.  Each entry point below states which of those
 * callables (reference file:line) it replaces; the Python host layer in
 * svd-quantization-task-merging_amd/ rebuilds the reference's exact signatures and dict
 * layouts on top of this ABI through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - Every pointer named *_dev is a DEVICE pointer (HBM).  Nothing here copies to or from
 *    the host except svdq_plan_create (tables, once) -- no entry point synchronises the
 *    stream or the device; all work is enqueued on `stream` (a hipStream_t passed as void*).
 *  - Return value: SVDQ_OK or a negative SVDQ_E* code; svdq_last_error() gives text.
 *  - Task delta buffers are fp32, contiguous, one buffer per (parameter, task), base
 *    address 16-byte aligned; the [D,N] stack of basis.py:103 is never materialised.
 *  - N (tasks) <= SVDQ_MAX_TASKS.
 */
#ifndef SVDQ_H
#define SVDQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVDQ_ABI_VERSION 1
#define SVDQ_MAX_TASKS 32
#define SVDQ_MAX_STAGES 8
#define SVDQ_MAX_BOOL_MASKS 255 /* bool-byte masks one combine call votes on (the bit-packed routes: SVDQ_MAX_TASKS) */

enum {
    SVDQ_OK = 0,
    SVDQ_EINVAL = -1,     /* bad argument (the reference raises ValueError) */
    SVDQ_EHIP = -2,       /* HIP runtime error */
    SVDQ_EUNSUPPORTED = -3
};

enum { SVDQ_MASK_UNION = 0, SVDQ_MASK_INTERSECTION = 1, SVDQ_MASK_MAJORITY = 2 };

/* Element type of the task / fine-tuned / base tensors a plan's streaming entry points read
 * (svdq_plan_set_input_type). */
enum { SVDQ_INPUT_F32 = 0, SVDQ_INPUT_F16 = 1, SVDQ_INPUT_BF16 = 2 };

/* Run-wide settings; field names follow SVDHybridConfig (reference src/svd_hybrid/config.py:157-205). */
typedef struct svdq_config {
    float   energy_threshold;  /* svd_energy_threshold, (0,1]                       */
    int32_t max_rank;          /* svd_max_rank, <= 0 means None                      */
    int32_t center;            /* svd_center                                         */
    int32_t fp16;              /* svd_fp16: basis stored (and projected with) fp16   */
    int32_t low_bits;          /* svd_low_bits 1..8                                  */
    int32_t rtvq_stages;       /* svd_rtvq_stages 1..SVDQ_MAX_STAGES                 */
    int32_t unit_rows;         /* 0 = auto; rows per work unit (multiple of 256)     */
    int32_t reserved;          /* measurement switches, 0 in production.  bit 0: reverse unit order in pass 2;
                                  bit 1: fp32-product Gram for every N (the round-1 kernel; sigma then only resolves
                                  down to ~3e-4 sigma_0 and smaller ones are treated as null directions);
                                  bit 2: XCD-chunked unit order (XCD x walks a contiguous eighth of the units; measured: no change);
                                  bit 3: N = 17..20: the two-wave pass 2 instead of the one-wave 4x4-block kernel. */
} svdq_config;

/* Byte sizes / strides the caller needs to allocate outputs (all device memory). */
typedef struct svdq_sizes {
    int64_t workspace_bytes;   /* scratch: Gram / projection partials, W, ranks               */
    int64_t basis_bytes;       /* packed U buffer (see svdq_plan_basis_layout)                 */
    int64_t mean_floats;       /* packed mean buffer, floats                                   */
    int64_t small_bytes;       /* packed small artifacts (see svdq_small_layout)               */
    int32_t n_units;           /* work units (one wavefront each) in passes 1 and 2            */
    int32_t n_slots;           /* partial-sum slots                                            */
} svdq_sizes;

/* Offsets (bytes) of the typed arrays inside the packed "small artifacts" buffer.
 * P = parameters, N = tasks, S = stages.  Everything a caller needs on the host after a
 * run is in this one buffer, so one D2H copy fetches it. */
typedef struct svdq_small_layout {
    int64_t sigma_off;      /* float   [P][N]       singular values, descending (first r valid)   */
    int64_t k_off;          /* int32   [P]          selected rank k                                */
    int64_t r_off;          /* int32   [P]          r = min(D, N) = number of singular values      */
    int64_t energy_off;     /* float   [P]          energy_retained = cum_energy[k-1]              */
    int64_t rows_off;       /* int64   [P]          rows actually processed (D, or mask.sum())     */
    int64_t chigh_off;      /* uint16  [P][N][N]    fp16 bits of c_high per task (first k valid)   */
    int64_t codes_off;      /* uint8   [P][N][S][N] RTVQ codes of c_low per task (first r-k valid) */
    int64_t scale_off;      /* float   [P][N][S]                                                   */
    int64_t zp_off;         /* float   [P][N][S]                                                   */
    int64_t rnorm_off;      /* float   [P][N][S]    residual norm before each stage                */
    int64_t coef_off;       /* float   [P][N][N]    fp32 coefficients c[t][i] before rounding      */
    int64_t status_off;     /* int32   [1]          written by svdq_compress: 0 = ok, 1 = fused schedule timed out */
    int64_t total_bytes;
} svdq_small_layout;

typedef struct svdq_plan svdq_plan;

/* ---- library ---------------------------------------------------------------------------- */
int         svdq_abi_version(void);
const char *svdq_last_error(void);

/* ---- plan: a ragged batch of P parameter tensors x N tasks -------------------------------
 * rows[p] = D_p, the element count of parameter p (upper bound when a mask is applied on
 * device).  Replaces the Python loop state of cli.py:317 (Step 4) / compress.py:187 (Step 5).
 * Allocates and fills small device tables (hipMalloc + hipMemcpy): call outside timed code. */
int  svdq_plan_create(svdq_plan **plan, int32_t n_tasks, int32_t n_params, const int64_t *rows,
                      const svdq_config *cfg);
void svdq_plan_destroy(svdq_plan *plan);
/* Per-parameter code width for the low-energy coefficients (host array [n_params], each in [1, 8]); NULL
 * restores cfg.low_bits for every parameter.  The reference builds ONE RTVQQuantizer(config.svd_low_bits, ...)
 * per run (compress.py:180-183); BASELINE config #5's "mixed 8-bit / 2-bit" run is two quantizer instances over
 * a partition of the parameters, which this expresses inside one plan. */
int  svdq_plan_set_low_bits(svdq_plan *plan, const int32_t *bits);
/* Element type of every tensor the plan's streaming entry points read as task, fine-tuned or base tensors:
 * SVDQ_INPUT_F32 (the default), SVDQ_INPUT_F16 or SVDQ_INPUT_BF16.  Half elements are converted to fp32 in
 * registers (exactly) and the fp32 arithmetic follows unchanged, so every output -- small artifacts, basis, mean,
 * task Gram, diagnostics -- is byte-identical to the same call on the tensors converted to fp32 first.  Half tensors
 * must start on an 8-byte boundary (fp32 ones, as always, on 16 bytes).  Covered: svdq_gram_center[_range],
 * svdq_eig_rank_select[_range], svdq_basis_project[_range], svdq_compress, svdq_compress_gather,
 * svdq_compress_from_base, svdq_compress_gather_from_base, svdq_task_gram, svdq_diagnostics (N <= 32).  The mask walk
 * (svdq_compress_masked[_from_base], svdq_diagnostics_masked), svdq_ingest and svdq_tvq_* read fp32 only and return
 * SVDQ_EUNSUPPORTED on a plan whose input type is not SVDQ_INPUT_F32.  Any other code: SVDQ_EINVAL. */
int  svdq_plan_set_input_type(svdq_plan *plan, int32_t type);
int  svdq_plan_sizes(const svdq_plan *plan, svdq_sizes *out);
int  svdq_plan_small_layout(const svdq_plan *plan, svdq_small_layout *out);
/* Per parameter: byte offset of its slab in the packed basis buffer and float offset of its
 * mean in the packed mean buffer.  Inside a slab (rows = rows processed, e = 2 or 4 bytes):
 *   U_high [rows, k]     row-major at slab + 0
 *   U_low  [rows, r-k]   row-major at slab + align256(rows * k * e)
 * i.e. the two .contiguous() tensors of basis.py:363-364, already cast per cli.py:354-361. */
int  svdq_plan_basis_layout(const svdq_plan *plan, int64_t *slab_off_bytes /*[P]*/,
                            int64_t *mean_off_floats /*[P]*/);

/* ---- pass 1: centred Gram  (stack_and_center basis.py:63-113 + first half of compute_svd
 *      basis.py:216-249).  G_p = Tc^T Tc accumulated by fp32 MFMA per 256-row block and fp64
 *      across blocks; one fp64 partial per work unit goes to the workspace.
 *      delta_ptrs_dev: device array [P*N] of const float* (parameter-major, task order =
 *      column order of basis.py:103).  rows_dev: optional device int64 [P] overriding rows
 *      (mask.sum() computed on device); NULL = plan rows. */
int svdq_gram_center(const svdq_plan *plan, const void *delta_ptrs_dev, const int64_t *rows_dev,
                     void *workspace_dev, void *stream);

/* ---- N x N eigen-solve + rank selection  (second half of compute_svd; compute_energy_spectrum
 *      basis.py:116-156; select_rank basis.py:159-213; energy_retained basis.py:367).
 *      Cyclic Jacobi in fp64, sigma = sqrt(lambda) -> fp32, fp32 cumsum rule of the reference.
 *      Writes sigma / k / r / energy / rows into small_dev and W = V Sigma^-1 into the workspace.
 *      Reads row 0 of every task (delta_ptrs_dev) to build the orthonormal completion column of the
 *      null direction that centring creates (LAPACK returns an arbitrary orthonormal vector there).
 *
 *      NON-FINITE INPUT (the one statement of the contract; the sources point here).  The reference stops on a task
 *      delta that holds NaN or +-Inf: torch.linalg.svd raises "input matrix contained non-finite values" (compute_svd,
 *      basis.py:216-249).  Errors of the data cannot be return codes of an asynchronous call, so they travel in the
 *      small buffer:
 *        what is flagged   a parameter with rows > 0 whose N x N Gram, right after the fixed-order sum of its partials,
 *                          has an entry that is NaN or +-Inf.  Every compress route (plain, gather, from-base, gather +
 *                          base, walk, walk + base) and the staged _range entry points end in this stage.  The Gram is
 *                          accumulated in fp64 from exact products, so a non-finite entry means a non-finite delta among
 *                          the rows processed (a centred Inf is a NaN; finetuned - base counts as formed in the passes).
 *                          Rows that a mask does not select and parameters with rows_dev[p] == 0 are never read.
 *        how it is seen    energy[p] is NaN.  energy[p] of every healthy parameter is finite, so isnan(energy[p]) IS the
 *                          flag; it is written by every eigen stage, so a later clean run on the same buffers clears it.
 *                          Also: sigma[p][0..N) = NaN; k[p] = min(1, r), r[p] and rows[p] as always (pass 2 and the
 *                          coefficient epilogue index as for a healthy parameter); W and the closed-form coefficients
 *                          are zero; the parameter's basis, mean and coefficient outputs are unspecified.  No Jacobi
 *                          sweep runs on it, nothing reads out of bounds.
 *        who raises        the calls here return SVDQ_OK and the torch operators stay asynchronous: a C or operator
 *                          caller tests isnan(energy[p]) in its host copy of the small buffer (Python:
 *                          pipeline.nonfinite_parameters).  CompressPlan.fetch_small raises NonFiniteInput, the
 *                          dictionary API a RuntimeError that names the parameters and regions.
 *        above 16 tasks    the first accumulation uses fp32 products, which overflow for finite deltas beyond ~1.8e19
 *                          that the reference accepts: a non-finite fp32-product Gram asks for the fp64 refinement
 *                          pass, and only a Gram that is still non-finite after it flags the parameter.
 *        exception         cfg.reserved bit 1 (fp32-product Gram for every N, a measurement switch) has no refinement
 *                          pass: there the fp32-product Gram flags directly, finite deltas beyond ~1.8e19 included.
 *      Healthy parameters with sigma_0 beyond ~1.8e19 (where the reference's fp32 sum of squares overflows and its
 *      energy reads inf / inf = NaN, k = 1): the same energy rule is evaluated in fp64, so their energy is finite. */
int svdq_eig_rank_select(const svdq_plan *plan, const void *delta_ptrs_dev, const int64_t *rows_dev,
                         void *workspace_dev, void *small_dev, void *stream);

/* ---- pass 2: basis + projection  (U = Tc W and the split of basis.py:363-364, the fp16 cast
 *      of cli.py:354-361, mean of basis.py:109, and project_to_basis compress.py:6-21 for all
 *      N tasks against the ROUNDED basis, fused in one streaming pass).
 *      Writes U_high/U_low slabs into basis_dev, means into mean_dev (NULL allowed when
 *      center == 0) and fp64 projection partials into the workspace. */
int svdq_basis_project(const svdq_plan *plan, const void *delta_ptrs_dev, const int64_t *rows_dev,
                       void *workspace_dev, const void *small_dev, void *basis_dev, float *mean_dev,
                       void *stream);

/* ---- coefficient epilogue  (compress_single_task compress.py:42-56: c_high -> fp16,
 *      c_low -> RTVQQuantizer.quantize rtvq.py:39-82, for every (parameter, task)). */
int svdq_coeff_quantize(const svdq_plan *plan, void *workspace_dev, void *small_dev, void *stream);

/* ---- the same four stages restricted to parameters [param0, param0 + nparams) of the plan.
 *      They let a caller pipeline groups of parameters (gram of group g+1 while the eigen-solve
 *      of group g runs on a second stream), which keeps a group's deltas resident in the 256 MiB
 *      Infinity Cache between its two streaming passes ("cache-resident pipeline"). */
int svdq_gram_center_range(const svdq_plan *plan, const void *delta_ptrs_dev, const int64_t *rows_dev,
                           void *workspace_dev, int32_t param0, int32_t nparams, void *stream);
int svdq_eig_rank_select_range(const svdq_plan *plan, const void *delta_ptrs_dev, const int64_t *rows_dev,
                               void *workspace_dev, void *small_dev, int32_t param0, int32_t nparams,
                               void *stream);
int svdq_basis_project_range(const svdq_plan *plan, const void *delta_ptrs_dev, const int64_t *rows_dev,
                             void *workspace_dev, const void *small_dev, void *basis_dev, float *mean_dev,
                             int32_t param0, int32_t nparams, void *stream);
int svdq_coeff_quantize_range(const svdq_plan *plan, void *workspace_dev, void *small_dev, int32_t param0,
                              int32_t nparams, void *stream);

/* Uncentred Gram of the CONCATENATED task vectors: out_gram[N*N] (device, fp64, row-major) =
 * sum over parameters of T_p^T T_p.  Replaces the [N, sum D] host feature matrix of
 * flatten_task_vectors (src/svd_hybrid/clustering.py:55-120): every quantity cluster_tasks (:198-245)
 * and compute_cluster_statistics (:263-316) need is a function of these N*N inner products.
 * Overwrites the pass-1 partials in `workspace`; multi-GPU callers all-reduce out_gram. */
int svdq_task_gram(const svdq_plan *plan, const void *delta_ptrs, const int64_t *rows_dev, void *workspace,
                   double *out_gram, void *stream);

/* The same Gram as a by-product of pass 1 (the one statement of the contract; the sources point here).  The
 * reference's clustering (flatten_task_vectors clustering.py:55-120, cluster_tasks :198-245,
 * compute_cluster_statistics :263-316) needs only the N x N inner products of the concatenated task vectors, and
 * pass 1 of the compressor reads every task vector anyway.
 *   svdq_plan_set_task_gram(plan, enable): call before svdq_plan_sizes.  It may enlarge workspace_bytes (N + 1 side
 *     sums per work unit and their reduced form) and changes nothing else: sizes, small layout, basis layout and the
 *     unit table stay, and every artifact of the plan (small buffer, basis, mean) is byte-identical to that of the
 *     same plan without the by-product.  A plan that does not enable it runs exactly the kernels it ran before.
 *   svdq_plan_task_gram(plan, workspace, out_gram, stream): valid once pass 1 and the eigen stage of ALL parameters
 *     of the plan have been enqueued on `workspace` -- after svdq_compress, svdq_compress_from_base, or
 *     svdq_gram_center[_range] + svdq_eig_rank_select[_range] covering every parameter; before or after pass 2.
 *     Writes out_gram[N*N] (device, fp64, row-major, plan task order) = sum over the plan's parameters of T_p^T T_p
 *     over the rows processed (rows_dev respected; from-base plans: T = finetuned - base), i.e. what svdq_task_gram
 *     returns for the same tensors, without reading them again.  Asynchronous on `stream`, no host copy, capturable.
 *     center == 0: the total of the Gram partials pass 1 left, the very sums of svdq_task_gram (bit-equal to it for
 *     N <= 16 with the default switches).  center == 1: with m the row mean that was subtracted and Tc the centred rows,
 *     T^T T = Tc^T Tc + a 1^T + 1 a^T + s 1 1^T, a = Tc^T m, s = m^T m; pass 1 sums a and s beside the Gram (fp32 over
 *     four rows, fp64 beyond) and the correction is applied on the device in fp64 in a fixed order.  The result is
 *     exactly symmetric and the same bits in every run.
 *   Covered: plain deltas and from-base plans, fp32 / fp16 / bf16 inputs, N = 1..32.  Not covered: the masked routes --
 *     on a plan with the by-product enabled svdq_compress_gather[_from_base] and svdq_compress_masked[_from_base]
 *     return SVDQ_EUNSUPPORTED (their Gram would be over the selected rows only; the reference clusters on the
 *     unmasked vectors).  svdq_plan_task_gram on a plan that did not enable it: SVDQ_EINVAL. */
int svdq_plan_set_task_gram(svdq_plan *plan, int32_t enable);
int svdq_plan_task_gram(const svdq_plan *plan, void *workspace_dev, double *out_gram_dev, void *stream);

/* svdq_compress for MASKED parameters without a compaction pass (replaces the 2*N boolean-index gathers per
 * parameter of cli.py:333 / compress.py:144, i.e. apply_mask_to_tensor mask_loader.py:651-679 feeding
 * construct_masked_basis and compress_masked_regions): delta_ptrs name the original full-size tensors,
 * index_ptrs is a device table [n_params] of int32 lists -- the ascending flat positions of the selected
 * elements of each parameter (svdq_maskset_indices) -- and rows_dev[p] their number (<= the plan's rows[p]).
 * Artifacts are those of svdq_compress on the compacted tensors, bit for bit. */
int svdq_compress_gather(const svdq_plan *plan, const void *delta_ptrs, const void *index_ptrs,
                         const int64_t *rows_dev, void *workspace_dev, void *small_dev, void *basis_dev,
                         float *mean_dev, void *stream);

/* svdq_compress straight from checkpoints: finetuned_ptrs [n_params * n_tasks] name the FINE-TUNED tensors,
 * base_ptrs [n_params] the base model's; delta = finetuned - base (compute_task_vector,
 * task_vector_loader.py:103-141) is formed in registers inside the streaming passes, so Step 1's task vectors
 * (cli.py:241-262) are never written to or read back from HBM.  Artifacts are those of svdq_ingest followed by
 * svdq_compress, bit for bit. */
int svdq_compress_from_base(const svdq_plan *plan, const void *finetuned_ptrs, const void *base_ptrs,
                            const int64_t *rows_dev, void *workspace_dev, void *small_dev, void *basis_dev,
                            float *mean_dev, void *stream);
/*      svdq_compress_gather_from_base: both at once -- masked parameters straight from checkpoints (cli.py Step 1 +
 *      the flat[mask] selections of Steps 4 and 5): finetuned[idx] - base[idx] is formed in registers.  Bit-identical to
 *      svdq_ingest followed by svdq_compress_gather. */
int svdq_compress_gather_from_base(const svdq_plan *plan, const void *finetuned_ptrs_dev, const void *base_ptrs_dev,
                                   const void *index_ptrs_dev, const int64_t *rows_dev, void *workspace, void *small,
                                   void *basis, float *mean, void *stream);

/* svdq_compress for MASKED parameters without index lists and without compacted copies (the default for dense masks;
 * the same reference calls as svdq_compress_gather: apply_mask_to_tensor / get_unmasked_portion mask_loader.py:651-709
 * inside the loops of cli.py:324-341 and compress.py:140-155).  delta_ptrs name the original full-size tensors,
 * mask_ptrs [n_params] the combined mask of each parameter as bool bytes (combine_masks mask_loader.py:488-648),
 * unit_start [n_units] the source position of every work unit's first row (svdq_maskset_unit_starts or
 * svdq_maskset_combine_starts; bit 62 set = the unit takes the CLEARED elements, i.e. the noise region), rows_dev[p] the
 * number of selected rows.  Both passes walk the source rows with contiguous loads, read the mask byte beside them and
 * compact the selected rows into the LDS strip: 4 N + 1 bytes per source row and pass against (4 N + 4) per selected row
 * through index lists.
 * Range of the walk (the one statement of it; the sources point here):
 *   svdq_compress_masked            N <= 32.  Artifacts bit-identical to svdq_compress_gather on the same masks (and so,
 *                                   up to 16 tasks, to svdq_compress on the compacted tensors).  Above 16 tasks both
 *                                   passes run their one-wave kernels (one wavefront per SIMD: measured 20-24 % slower
 *                                   than svdq_compress_gather, whose index lists feed the two-wave kernels) and repeat the
 *                                   two-wave kernels' sums; N = 17..20 is therefore bit-identical to svdq_compress_gather
 *                                   on a plan with bit 3 of svdq_config.reserved set (the default pass 2 of those N, the
 *                                   4x4-block kernel, associates the task sum differently).
 *   svdq_compress_masked_from_base  N <= 16; SVDQ_EUNSUPPORTED above: use svdq_compress_gather_from_base. */
int svdq_compress_masked(const svdq_plan *plan, const void *delta_ptrs, const void *mask_ptrs,
                         const int64_t *unit_start, const int64_t *rows_dev, void *workspace_dev, void *small_dev,
                         void *basis_dev, float *mean_dev, void *stream);
/*      svdq_compress_masked_from_base: the same straight from checkpoints (finetuned[row] - base[row] formed in
 *      registers, compute_task_vector task_vector_loader.py:103-141).  Bit-identical to svdq_ingest + svdq_compress_masked. */
int svdq_compress_masked_from_base(const svdq_plan *plan, const void *finetuned_ptrs_dev, const void *base_ptrs_dev,
                                   const void *mask_ptrs_dev, const int64_t *unit_start, const int64_t *rows_dev,
                                   void *workspace, void *small, void *basis, float *mean, void *stream);

/* ---- the step before the path: task-vector ingest and whole-tensor quantization ("TVQ"),
 * batched over a plan's parameters x tasks.  All pointer tables are DEVICE arrays of device addresses,
 * parameter-major ([p * n_tasks + t]); fp32 buffers 16-byte aligned, code buffers 4-byte aligned. ---- */

/* delta[p][t] = finetuned[p][t] - base[p] in one pass, base read once for the N tasks.
 * Replaces compute_task_vector (src/svd_hybrid/task_vector_loader.py:103-141) and the delta loop of
 * TaskVector.__init__ (task_vectors.py:98-, "delta = finetuned_param - pretrained_param").
 * base_ptrs: [n_params].  stats_work: NULL, or svdq_tvq_work_bytes() bytes that receive the per-unit
 * min/max of every delta so that svdq_tvq_quantize(..., stats_ready = 1) skips its statistics pass. */
int svdq_ingest(const svdq_plan *plan, const void *base_ptrs, const void *finetuned_ptrs, const void *delta_ptrs,
                void *stats_work, void *stream);

int64_t svdq_tvq_work_bytes(const svdq_plan *plan);

/* Whole-tensor quantization of every (parameter, task) tensor of the plan.
 * mode 0: asymmetric_quantization (quantization_utils.py:76-99) -> uint8 codes, scale, zero_point;
 * mode 1: absmax_quantization (quantization_utils.py:60-73)     -> int8 codes, scale.
 * As used by QuantizedFinetunedModel / QuantizedBaseAndTaskVector (task_vectors.py:764-1010).
 * scale / zero_point: device float [n_params * n_tasks].  bits in [1, 8] (absmax: [2, 8], or 16 -> int16 codes,
 * code buffers then 8-byte aligned; dequantize those with mode 2). */
int svdq_tvq_quantize(const svdq_plan *plan, const void *x_ptrs, int32_t mode, int32_t bits, const void *code_ptrs,
                      float *scale, float *zero_point, void *work, int32_t stats_ready, void *stream);

/* dequantize_asymmetric (quantization_utils.py:137-172) / dequantize_absmax (:102-134, which MULTIPLIES by
 * the scale -- kept as is), optionally fused with "+ add[p]" (QuantizedTaskVector.apply_to,
 * task_vectors.py:638-761; QuantizedBaseAndTaskVector.dequantize).  add_ptrs: NULL or [n_params]. */
int svdq_tvq_dequantize(const svdq_plan *plan, const void *code_ptrs, int32_t mode, const float *scale,
                        const float *zero_point, const void *add_ptrs, const void *out_ptrs, void *stream);

/* ---- all four stages back to back on one stream (cli.py Step 4 + Step 5 for the batch) ---- */
int svdq_compress(const svdq_plan *plan, const void *delta_ptrs_dev, const int64_t *rows_dev,
                  void *workspace_dev, void *small_dev, void *basis_dev, float *mean_dev, void *stream);

/* ---- standalone quantizer on one large tensor  (RTVQQuantizer.quantize / dequantize
 *      rtvq.py:106-139; asymmetric_quantization rtvq.py:4-27 == quantization_utils.py:76-99).
 *      codes_dev: uint8 [stages][code_stride] (code_stride % 4 == 0, >= n; first n of each
 *      row valid); scale/zp/rnorm_dev: float [stages];
 *      work_dev: svdq_rtvq_work_bytes(n) bytes of scratch. */
int64_t svdq_rtvq_work_bytes(int64_t n);
int svdq_rtvq_quantize(const float *x_dev, int64_t n, int32_t bits, int32_t stages,
                       uint8_t *codes_dev, int64_t code_stride, float *scale_dev, float *zp_dev,
                       float *rnorm_dev, void *work_dev, void *stream);
int svdq_rtvq_dequantize(const uint8_t *codes_dev, int64_t code_stride, int64_t n, int32_t stages,
                         const float *scale_dev, const float *zp_dev, float *out_dev, void *stream);

/*      qbit = 16 (asymmetric_quantization rtvq.py:22-25 only; SVDHybridConfig allows at most 8 bits): one stage, int16
 *      codes exactly as the reference's CPU cast leaves them (values above 32767 wrap negative), and the matching
 *      asymmetric_dequantization on int16 input.  work_dev: svdq_rtvq_work_bytes(n) bytes. */
int svdq_asym16_quantize(const float *x_dev, int64_t n, int16_t *codes_dev, float *scale_dev, float *zp_dev,
                         void *work_dev, void *stream);
int svdq_asym16_dequantize(const int16_t *codes_dev, int64_t n, const float *scale_dev, const float *zp_dev,
                           float *out_dev, void *stream);

/* ---- standalone projection for callers that bring their own basis
 *      (project_to_basis compress.py:6-21 with the mean subtraction of compress.py:35-37):
 *      c_out[i] = sum_d float(U[d][i]) * (delta[d] - mean[d]),  i < k from U_high [rows,k],
 *      then i < k+nl from U_low [rows,nl]; both row-major, fp16 (u_fp16 != 0) or fp32;
 *      mean may be NULL; k + nl <= 32.  work_dev: svdq_project_work_bytes(rows, k+nl) bytes. */
int64_t svdq_project_work_bytes(int64_t rows, int32_t ncols);
int svdq_project(const void *u_high_dev, const void *u_low_dev, int32_t u_fp16, int64_t rows,
                 int32_t k, int32_t nl, const float *delta_dev, const float *mean_dev,
                 float *c_out_dev, void *work_dev, void *stream);

/* ---- masks  (compute_union/intersection/majority_mask mask_loader.py:412-485;
 *      apply_mask_to_tensor / get_unmasked_portion mask_loader.py:651-709).
 *      mask_ptrs_dev: device array [n_masks] of const uint8_t* (torch.bool storage).
 *      svdq_mask_combine writes the combined mask (0/1 bytes) and its popcount.  strategy: SVDQ_MASK_*; for
 *      SVDQ_MASK_MAJORITY bits 8.. may carry (votes needed + 1) for compute_majority_mask(threshold != 0.5)
 *      (mask_loader.py:456-485: vote_sum >= threshold * len(masks), compared in fp32); 0 there = threshold 0.5.
 *      Every votes needed in 0..n_masks + 1 is accepted (0: every element passes, n_masks + 1: none does).
 *      n_masks <= SVDQ_MAX_BOOL_MASKS (255) for svdq_mask_combine, svdq_maskset_combine, svdq_maskset_combine_indices
 *      and svdq_maskset_combine_starts: the votes of an element are counted in one byte.  More is SVDQ_EINVAL before
 *      anything is launched, and svdq_last_error() names the limit.  The svdq_mask_* and svdq_maskset_* entry points take mask pointers of any alignment.
 *      svdq_mask_compact: order-preserving compaction of n_src fp32 buffers under one mask
 *      (invert != 0 selects the False positions); count_dev receives the selected count.
 *      work_dev: svdq_mask_work_bytes(numel) bytes. */
int64_t svdq_mask_work_bytes(int64_t numel);
int svdq_mask_combine(const void *mask_ptrs_dev, int32_t n_masks, int64_t numel, int32_t strategy,
                      uint8_t *out_dev, int64_t *count_dev, void *work_dev, void *stream);
int svdq_mask_compact(const void *src_ptrs_dev, const void *dst_ptrs_dev, int32_t n_src,
                      const uint8_t *mask_dev, int32_t invert, int64_t numel, int64_t *count_dev,
                      void *work_dev, void *stream);

/* ---- the mask operators over a ragged SET of parameters in a handful of launches (the reference runs
 *      them once per parameter and task: cli.py:324-341, compress.py:140-155).  numel[q] = elements of
 *      masked parameter q.  Tables are device arrays of device pointers:
 *        mask_ptrs [Q*n_masks] uint8 per-task masks (combine) / [Q] combined masks (compact)
 *        out_ptrs  [Q] combined mask outputs;  src/dst [Q*n_src] fp32 buffers (dst sized numel[q])
 *      counts stay on the device (int64 [Q]): mask.sum() and (~mask).sum(); they feed rows_dev.
 *      svdq_maskset_compact writes flat[mask] to dst_true and, when dst_false_ptrs != NULL,
 *      flat[~mask] to dst_false in the same pass.  work_dev: svdq_maskset_work_bytes() bytes. */
typedef struct svdq_maskset svdq_maskset;
int     svdq_maskset_create(svdq_maskset **ms, int32_t n_params, const int64_t *numel);
void    svdq_maskset_destroy(svdq_maskset *ms);
int64_t svdq_maskset_work_bytes(const svdq_maskset *ms);
int     svdq_maskset_combine(const svdq_maskset *ms, const void *mask_ptrs_dev, int32_t n_masks, int32_t strategy,
                             const void *out_ptrs_dev, int64_t *counts_dev, void *stream);
int     svdq_maskset_compact(const svdq_maskset *ms, const void *mask_ptrs_dev, const void *src_ptrs_dev,
                             const void *dst_true_ptrs_dev, const void *dst_false_ptrs_dev, int32_t n_src,
                             int64_t *count_true_dev, int64_t *count_false_dev, void *work_dev, void *stream);

/* Index lists instead of compacted copies: idx_true_ptrs[q] (int32, room for numel[q] entries, 16-byte aligned)
 * receives the ascending flat positions of the set elements of mask q, idx_false_ptrs[q] (NULL table = skip)
 * those of the cleared ones; counts as in svdq_maskset_compact.  This is what `flat[mask]` / `flat[~mask]`
 * (mask_loader.py:651-709) select; svdq_compress_gather reads the task deltas through these lists, so the
 * 2*N compacted copies per parameter never exist. */
int     svdq_maskset_indices(const svdq_maskset *ms, const void *mask_ptrs_dev, const void *idx_true_ptrs_dev,
                             const void *idx_false_ptrs_dev, int64_t *count_true_dev, int64_t *count_false_dev,
                             void *work_dev, void *stream);

/* svdq_maskset_combine followed by svdq_maskset_indices on the combined masks in 3 launches: the combine pass
 * already counts every tile, so the separate counting pass over the combined masks is skipped.
 * (combine_masks mask_loader.py:488-648 feeding the flat[mask] selections of cli.py:333 / compress.py:144.) */
int     svdq_maskset_combine_indices(const svdq_maskset *ms, const void *mask_ptrs_dev, int32_t n_masks,
                                     int32_t strategy, const void *out_ptrs_dev, const void *idx_true_ptrs_dev,
                                     const void *idx_false_ptrs_dev, int64_t *count_true_dev,
                                     int64_t *count_false_dev, void *work_dev, void *stream);

/* The same from BIT-PACKED tall masks, the form the reference's mask files have (load_tall_mask_file,
 * mask_loader.py:125-206: one numpy.packbits stream per task over the flattened state dict, first element = most
 * significant bit): stream_ptrs_dev [n_masks] device streams, stream_bytes_dev [n_masks] their lengths,
 * bit_offsets_dev [n_params] the bit position of each parameter's first element inside every stream.  Reads
 * n_masks / 8 bytes per element instead of n_masks; writes the combined bool masks, index lists and counts.
 * n_masks <= SVDQ_MAX_TASKS (32; the bool-byte routes above take SVDQ_MAX_BOOL_MASKS).  Every stream pointer is
 * 16-byte aligned: the kernel fetches a stream in 16-byte chunks counted from its first byte.  No byte at or past
 * stream_bytes_dev[m] is read, so a stream may end anywhere, also in the middle of a chunk.  The same holds for
 * svdq_maskset_combine_packed_starts. */
int     svdq_maskset_combine_packed_indices(const svdq_maskset *ms, const void *stream_ptrs_dev,
                                            const int64_t *stream_bytes_dev, const int64_t *bit_offsets_dev,
                                            int32_t n_masks, int32_t strategy, const void *out_ptrs_dev,
                                            const void *idx_true_ptrs_dev, const void *idx_false_ptrs_dev,
                                            int64_t *count_true_dev, int64_t *count_false_dev, void *work_dev,
                                            void *stream);

/* Unit starts for svdq_compress_masked instead of index lists (same reference calls: mask.sum() and flat[mask] of
 * cli.py:332-333 / compress.py:143-144, mask_loader.py:651-709).
 *   svdq_maskset_count_scan: per-tile counts + per-parameter exclusive scan of already combined masks (2 launches);
 *     counts as in svdq_maskset_compact; the tile offsets stay in work_dev for svdq_maskset_unit_starts.
 *   svdq_maskset_unit_starts: unit_start_dev[u] (int64 [plan n_units]) = source position of the element of rank
 *     unit.row0 among the selected elements of the unit's mask, numel when the unit lies past rows_dev[p].
 *     entry_map_dev: NULL (plan parameter p uses mask p; the plan's rows must equal the set's numel) or int32
 *     [plan n_params]: low 31 bits = index of the mask in the set, bit 31 = take the CLEARED elements (the noise
 *     region of cli.py:336-338).  rows_dev [plan n_params] as handed to svdq_compress_masked.
 *   svdq_maskset_combine_starts / _combine_packed_starts: combine (bool-byte / bit-packed per-task masks, as
 *     svdq_maskset_combine_indices / _combine_packed_indices) + scan + unit starts in 3 launches, identity map,
 *     rows = count_true. */
int     svdq_maskset_count_scan(const svdq_maskset *ms, const void *mask_ptrs_dev, int64_t *count_true_dev,
                                int64_t *count_false_dev, void *work_dev, void *stream);
int     svdq_maskset_unit_starts(const svdq_maskset *ms, const svdq_plan *plan, const void *mask_ptrs_dev,
                                 const int32_t *entry_map_dev, const int64_t *rows_dev, const void *work_dev,
                                 int64_t *unit_start_dev, void *stream);
int     svdq_maskset_combine_starts(const svdq_maskset *ms, const svdq_plan *plan, const void *mask_ptrs_dev,
                                    int32_t n_masks, int32_t strategy, const void *out_ptrs_dev,
                                    int64_t *count_true_dev, int64_t *count_false_dev, void *work_dev,
                                    int64_t *unit_start_dev, void *stream);
int     svdq_maskset_combine_packed_starts(const svdq_maskset *ms, const svdq_plan *plan, const void *stream_ptrs_dev,
                                           const int64_t *stream_bytes_dev, const int64_t *bit_offsets_dev,
                                           int32_t n_masks, int32_t strategy, const void *out_ptrs_dev,
                                           int64_t *count_true_dev, int64_t *count_false_dev, void *work_dev,
                                           int64_t *unit_start_dev, void *stream);

/* ---- merge consumers (the parity reconstruction of R14)
 *      svdq_reconstruct: reconstruct_from_coefficients (merge.py:144-194):
 *        out[d] = ((sum_i U_high[d][i] c[i] + sum_j U_low[d][j] c[k+j]) + mean[d]) * scale
 *        coef_dev: float [k+nl] on the device; mean_dev may be NULL; scale = noise_shrink or 1.
 *      svdq_mask_expand: reconstruct_from_masked (mask_loader.py:712-763): out = 0; out[mask] = signal;
 *        out[~mask] = noise (noise_dev may be NULL).  work_dev: svdq_mask_work_bytes(numel) bytes. */
int svdq_reconstruct(const void *u_high_dev, const void *u_low_dev, int32_t u_fp16, int64_t rows, int32_t k,
                     int32_t nl, const float *coef_dev, const float *mean_dev, float scale, float *out_dev,
                     void *stream);
int svdq_mask_expand(const float *signal_dev, const float *noise_dev, const uint8_t *mask_dev, int64_t numel,
                     float *out_dev, void *work_dev, void *stream);

/* ---- diagnostics: compute_reconstruction_error (diagnostics.py:72-117).
 *      recon_dev != NULL: metrics of (orig - recon) for two given vectors.
 *      recon_dev == NULL: the reconstruction U_high c_high + U_low c_low (+ mean_dev if not NULL; the
 *      reference's compute_parameter_diagnostics passes none: diagnostics.py:210-212) is formed
 *      on the fly and never stored.  out6_dev (double[6]) = absolute_error, relative_error,
 *      max_absolute_error, mean_absolute_error, original_norm, reconstructed_norm.
 *      work_dev: svdq_recon_error_work_bytes(rows) bytes. */
int64_t svdq_recon_error_work_bytes(int64_t rows);
int svdq_recon_error(const void *u_high_dev, const void *u_low_dev, int32_t u_fp16, int64_t rows, int32_t k,
                     int32_t nl, const float *coef_dev, const float *mean_dev, const float *recon_dev,
                     const float *orig_dev, double *out6_dev, void *work_dev, void *stream);

/* ---- the same consumers for a WHOLE PLAN, straight from the buffers the compressor left in HBM (no host copy of the
 *      payloads, no per-parameter / per-task launch): what cli.py Steps 7-9 do parameter by parameter --
 *      merge_all_parameters (merge.py:304-426) -> merge_parameter (:197-301) -> dequantize_and_average (:61-141, with
 *      RTVQQuantizer.dequantize rtvq.py:85-103) + reconstruct_from_coefficients (:144-194); merge_with_clustering
 *      (:555-626) + merge_cluster_results (clustering.py:374-425); apply_merged_deltas (merge.py:429-552);
 *      compute_parameter_diagnostics (diagnostics.py:120-231).
 *   A "set" is a group of tasks averaged together: one set of all tasks (merge_all_parameters), one per cluster
 *   (merge_with_clustering) or one per task (diagnostics).
 *   weights_dev: float [n_sets][N] (per_param = 0) or [P][n_sets][N] (per_param = 1): weight of task t in set s,
 *     renormalised over the set's present tasks as the reference does on the host (merge.py:123-124); < 0 = not in the set.
 *   order_dev:   NULL or int32 [N] / [P][N]: task indices in the order of the sorted task names (merge.py:89).
 *   svdq_merge_coeffs: cbar_dev float [P][n_sets][N] = averaged c_high (columns < k) and dequantized c_low (k..r-1).
 *   svdq_merge_reconstruct: one streaming launch over the plan's units,
 *       out[p][d] = sum_s share[s] * (((U_high c_s,high + U_low c_s,low)[d] + mean[d]) * scale[p])  (+ base[p][d])
 *     set_share_dev: NULL (n_sets = 1: no weighting) or float [n_sets] / [P][n_sets]: the clusters' shares as
 *     apply_weights_to_tensors leaves them (weighting.py:332-372: shares / shares.sum() over ALL clusters -- in
 *     merge_with_clustering a cluster none of whose members holds the parameter still contributes its zeros,
 *     merge.py:297-299,555-626); < 0 = the set does not hold the parameter: skipped, the others are NOT renormalised;
 *     n_sets <= 8.
 *     scale_dev: NULL or float [P] (noise_shrink of the noise regions, merge.py:284); base_ptrs_dev: NULL or [P] base
 *     tensors (then out = base + delta); out_ptrs_dev [P] fp32 outputs of rows[p] elements (compacted rows for masked
 *     parameters: svdq_mask_expand scatters them).  A parameter's rows are the bits svdq_reconstruct gives.
 *   svdq_merge = both; work_dev: svdq_merge_work_bytes(plan, n_sets).
 *   svdq_diagnostics: out_dev double [P][N][6], the six numbers of svdq_recon_error for every (parameter, task) from
 *     one pass over U and the N deltas (delta_ptrs_dev as for svdq_compress); add_mean = 0 reproduces the reference
 *     (SURVEY Q1).  The reconstruction U_high c_high + U_low c_low is formed in fp32 (matrix pipe), the sums in fp64: every
 *     number is within the fp32 forward-error bound of diagnostics.py:210-212 of the formula evaluated in fp64 on the same
 *     artifacts (tests/test_hip_diagnostics.py).  work_dev: svdq_diagnostics_work_bytes(plan). */
int64_t svdq_merge_work_bytes(const svdq_plan *plan, int32_t n_sets);
int svdq_merge_coeffs(const svdq_plan *plan, const void *small_dev, const float *weights_dev, const int32_t *order_dev,
                      int32_t n_sets, int32_t per_param, float *cbar_dev, void *stream);
int svdq_merge_reconstruct(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev, const void *basis_dev,
                           const float *mean_dev, const float *cbar_dev, int32_t n_sets, int32_t per_param,
                           const float *set_share_dev, const float *scale_dev, const void *base_ptrs_dev,
                           const void *out_ptrs_dev, void *stream);
int svdq_merge(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev, const void *basis_dev,
               const float *mean_dev, const float *weights_dev, const int32_t *order_dev, int32_t n_sets,
               int32_t per_param, const float *set_share_dev, const float *scale_dev, const void *base_ptrs_dev,
               const void *out_ptrs_dev, void *work_dev, void *stream);
int64_t svdq_diagnostics_work_bytes(const svdq_plan *plan);
int svdq_diagnostics(const svdq_plan *plan, const void *delta_ptrs_dev, const int64_t *rows_dev, const void *small_dev,
                     const void *basis_dev, const float *mean_dev, int32_t add_mean, double *out_dev, void *work_dev,
                     void *stream);

/* ---- every task's OWN reconstruction for a whole plan, in one pass over the basis: what the reference does per
 *      (parameter, task) with RTVQQuantizer.dequantize (rtvq.py:85-103) + reconstruct_from_coefficients
 *      (merge.py:144-194), and apply_merged_deltas (merge.py:429-552) when a base is given -- "give me task t's model
 *      back" for one task, several or all.  Two launches per plan: the selected tasks' coefficients straight from the
 *      small-artifact buffer (c_high, dequantized c_low), then ONE streaming launch over the plan's units that reads a
 *      block of U_high / U_low / mean (and base) rows once and writes every selected task's rows:
 *        out[p][j][d] = ((U_high c_j,high + U_low c_j,low)[d] + mean[d]) * scale[p]   (base[p][d] + that, given base)
 *      with c_j the coefficients of plan task task_dev[j].  Per-row arithmetic is svdq_reconstruct's and
 *      svdq_merge_reconstruct's (fp32 fma chains from 0 over the U_high columns in order, a separate chain over the U_low
 *      columns, hi + lo, + mean on a centred plan, * scale, base + res): out[p][j] is bit for bit svdq_reconstruct on
 *      that task's coefficients and bit for bit svdq_merge with the one-hot set {task_dev[j]: 1.0}.
 *   task_dev      int32 [n_out] plan task indices, 1 <= n_out <= SVDQ_MAX_TASKS; duplicates are allowed.  NULL or an
 *                 n_out outside the range is SVDQ_EINVAL before anything is launched.  The indices themselves live on the
 *                 device, where this call cannot see them (it copies nothing to the host): the caller that builds the
 *                 table checks them against [0, N) -- CompressPlan.reconstruct_tasks does, and refuses with the same
 *                 error -- and on the device an index outside [0, N) is skipped like a NULL output.
 *   out_ptrs_dev  [P][n_out] fp32 outputs of rows[p] elements (compacted rows for masked regions: svdq_mask_expand
 *                 scatters them); a NULL entry = that (parameter, task) is neither formed nor written (a task that lacks
 *                 the parameter).  Nothing is written past rows[p] elements of any output.
 *   rows_dev, scale_dev, base_ptrs_dev: as for svdq_merge_reconstruct; rows[p] == 0: nothing of p is read or written.
 *   work_dev      svdq_task_reconstruct_work_bytes(plan, n_out) bytes (0 for an n_out outside the range).
 *   Allocates nothing, copies nothing to the host, synchronises nothing: capturable like every other entry point.
 *   Works on plans filled by any compress route and on plans filled by svdq_plan_import. */
int64_t svdq_task_reconstruct_work_bytes(const svdq_plan *plan, int32_t n_out);
int svdq_task_reconstruct(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev, const void *basis_dev,
                          const float *mean_dev, const int32_t *task_dev /*[n_out] plan task indices*/, int32_t n_out,
                          const float *scale_dev /*NULL or [P]*/, const void *base_ptrs_dev /*NULL or [P]*/,
                          const void *out_ptrs_dev /*[P][n_out] fp32 outputs of rows[p] elements; NULL entry = skip*/,
                          void *work_dev, void *stream);

/* ---- the same for MASKED regions, with reconstruct_from_masked (mask_loader.py:712-763: zeros; result[mask] = signal;
 *      result[~mask] = noise) and apply_mask_to_tensor (:651-679, the "original" of the masked diagnostics,
 *      diagnostics.py:186-199) inside the streaming launch: the plan's artifacts describe the COMPACTED rows of every
 *      region; the launch walks the SOURCE rows with the combined mask byte beside them (mask_ptrs_dev [P], unit_start_dev
 *      [plan units] from svdq_maskset_unit_starts / *_starts; bit 62 of a start = the region is the CLEARED elements),
 *      finds each selected row's compacted row by wave ballots and reads the contiguous run of basis rows it needs.
 *   svdq_merge_masked: out_ptrs_dev [P] = FULL tensors (params[p].rows elements; NULL = leave this entry alone); every
 *     selected source row gets the merged value of its compacted row (+ base at the source row); fill_dev NULL or int32
 *     [P]: 1 = the entry also writes 0 (+ base) to the rows its region does not select -- for a signal region without a
 *     noise region; with one, the noise entry (its own plan entry, inverted polarity, scale = noise_shrink) writes
 *     them.  Same bits as svdq_merge + svdq_mask_expand (+ base).
 *   svdq_diagnostics_masked: delta_ptrs_dev = the N unmasked task deltas per entry. */
int svdq_merge_masked(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev, const void *basis_dev,
                      const float *mean_dev, const float *weights_dev, const int32_t *order_dev, int32_t n_sets,
                      int32_t per_param, const float *set_share_dev, const float *scale_dev, const void *mask_ptrs_dev,
                      const int64_t *unit_start_dev, const int32_t *fill_dev, const void *base_ptrs_dev,
                      const void *out_ptrs_dev, void *work_dev, void *stream);

/* ---- every task's OWN reconstruction of MASKED regions, inside the source walk (the one statement of the contract; the
 *      sources point here): what the reference does per (parameter, task) with RTVQQuantizer.dequantize (rtvq.py:85-103)
 *      + reconstruct_from_coefficients (merge.py:144-194) on the signal and the noise region, reconstruct_from_masked
 *      (mask_loader.py:712-763) to put both back at their source rows, and apply_merged_deltas (merge.py:429-552) when a
 *      base is given.  Two launches per plan: svdq_task_reconstruct's coefficient launch, unchanged, then ONE streaming
 *      launch that walks the SOURCE rows as svdq_merge_masked does (same mask_ptrs_dev, unit_start_dev, fill_dev, ranks
 *      by wave ballots clamped to the unit's compacted rows) and, from one staged run of U_high / U_low / mean rows,
 *      writes every selected task's value at the source row:
 *        out[p][j][s] = base[p][s] + ((U_high c_j,high + U_low c_j,low)[rank(s)] + mean[rank(s)]) * scale[p]
 *      for a selected source row s; base[p][s] + 0 for an unselected row when fill[p] is set; an unselected row is
 *      otherwise left untouched (the noise entry of the same parameter writes it).  Without base the value alone.
 *   The contract on bits: out[p][j] is bit for bit svdq_merge_masked with the one-hot set {task_dev[j]: 1.0} and the same
 *     scale, fill, base, masks and unit starts; and bit for bit svdq_task_reconstruct into compacted rows followed by
 *     svdq_mask_expand, plus base.
 *   task_dev, n_out, scale_dev, work_dev (svdq_task_reconstruct_work_bytes): as for svdq_task_reconstruct -- NULL
 *     task_dev, an n_out outside [1, SVDQ_MAX_TASKS] or a missing mean on a centred plan is SVDQ_EINVAL before anything
 *     is launched; a device index outside [0, N) is skipped like a NULL output.
 *   mask_ptrs_dev, unit_start_dev, rows_dev, fill_dev, base_ptrs_dev: as for svdq_merge_masked (the first three required:
 *     NULL is SVDQ_EINVAL).
 *   out_ptrs_dev  [P][n_out] FULL fp32 tensors (params[p].rows elements); a NULL entry = that (parameter, task) is neither
 *                 formed nor written; a parameter whose outputs are all skipped is not read at all.
 *   Allocates nothing, copies nothing to the host, synchronises nothing: capturable like every other entry point. */
int svdq_task_reconstruct_masked(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev,
                                 const void *basis_dev, const float *mean_dev, const int32_t *task_dev, int32_t n_out,
                                 const float *scale_dev, const void *mask_ptrs_dev, const int64_t *unit_start_dev,
                                 const int32_t *fill_dev, const void *base_ptrs_dev,
                                 const void *out_ptrs_dev /* [P][n_out] FULL tensors */, void *work_dev, void *stream);
int svdq_diagnostics_masked(const svdq_plan *plan, const void *delta_ptrs_dev, const void *mask_ptrs_dev,
                            const int64_t *unit_start_dev, const int64_t *rows_dev, const void *small_dev,
                            const void *basis_dev, const float *mean_dev, int32_t add_mean, double *out_dev,
                            void *work_dev, void *stream);

/* ---- the diagnostics straight from checkpoints (the one statement of the contract; the sources point here): what the
 *      reference does with compute_task_vector (task_vector_loader.py:103-141: delta = finetuned - base, per parameter)
 *      followed by the per-task loop of compute_parameter_diagnostics (diagnostics.py:186-215), without the N task
 *      vectors ever existing in memory.  finetuned_ptrs_dev [P*N] names the FINE-TUNED tensors (parameter-major, as
 *      delta_ptrs_dev of svdq_diagnostics), base_ptrs_dev [P] the base model's; inside the one pass over U every block's
 *      base row is loaded once beside its N task rows, widened to fp32 as they are, and each element becomes
 *      x = finetuned - base, a single fp32 subtraction; everything after it is svdq_diagnostics' own code.
 *   The contract on bits: out_dev is bit for bit what svdq_diagnostics gives on fp32 tensors holding
 *     (float)finetuned - (float)base; svdq_diagnostics_masked_from_base is bit for bit svdq_diagnostics_masked on such
 *     tensors.
 *   Element type: the plan's input type (svdq_plan_set_input_type) governs the fine-tuned and the base tensors alike,
 *     with the alignment of svdq_compress_from_base (16 bytes for fp32, 8 for fp16 / bf16).  The masked form reads fp32
 *     only (SVDQ_EUNSUPPORTED on a half plan, as svdq_diagnostics_masked).  Any N <= SVDQ_MAX_TASKS, masked form included.
 *   A NULL base_ptrs_dev is SVDQ_EINVAL before anything is launched; the masked form also requires mask_ptrs_dev,
 *     unit_start_dev and rows_dev, as svdq_diagnostics_masked.  work_dev: svdq_diagnostics_work_bytes(plan).
 *   Allocates nothing, copies nothing to the host, synchronises nothing: capturable like every other entry point.
 *   Works on plans filled by any compress route and on plans filled by svdq_plan_import. */
int svdq_diagnostics_from_base(const svdq_plan *plan, const void *finetuned_ptrs_dev /*[P*N]*/,
                               const void *base_ptrs_dev /*[P]*/, const int64_t *rows_dev, const void *small_dev,
                               const void *basis_dev, const float *mean_dev, int32_t add_mean, double *out_dev,
                               void *work_dev, void *stream);
int svdq_diagnostics_masked_from_base(const svdq_plan *plan, const void *finetuned_ptrs_dev, const void *base_ptrs_dev,
                                      const void *mask_ptrs_dev, const int64_t *unit_start_dev, const int64_t *rows_dev,
                                      const void *small_dev, const void *basis_dev, const float *mean_dev,
                                      int32_t add_mean, double *out_dev, void *work_dev, void *stream);

/* ---- adopt STORED artifacts into a plan (the one statement of the contract; the sources point here).  The reference
 *      writes its artifacts one file per parameter (save_basis / save_compressed_coefficients storage.py:52-174) and merges
 *      them again later, with other weights or another base model (load_all_artifacts storage.py:341-389 ->
 *      reconstruct_from_artifacts reload.py:142-238 -> merge_all_parameters merge.py:304-426).  svdq_plan_import puts such
 *      artifacts -- wherever they came from -- into the packed buffers of a plan, after which every plan-level consumer that
 *      needs only the artifacts works on them: svdq_merge, svdq_merge_coeffs, svdq_merge_reconstruct, svdq_task_reconstruct
 *      (and, given masks and unit starts of the caller's, the source walks svdq_merge_masked and
 *      svdq_task_reconstruct_masked -- on a plan created with rows[p] = the element count of the mask: a walk ends where
 *      the plan's rows end, so a plan created with rows[p] = D would stop at source row D; rows_dev carries D).
 *   the plan         svdq_plan_create with rows[p] = D of the stored basis, n_tasks = the tasks that hold the parameters,
 *                    cfg.fp16 = the stored basis is fp16 (else fp32), cfg.center = means are stored, cfg.rtvq_stages as
 *                    stored.  It needs no compress workspace.
 *   small_dev        the plan's small-artifact buffer, ALREADY FILLED by the caller in the published layout
 *                    (svdq_plan_small_layout; a host image + one hipMemcpyAsync): sigma[p][0..r), k, r, energy, rows (= D;
 *                    0 = skip the parameter), c_high[p][t][0..k), codes[p][t][s][0..r-k), scale, zero_point, residual_norm,
 *                    status = 0.  r <= min(rows, N), k <= r.  coef holds the fp32 coefficients before rounding; no stored
 *                    artifact has them: they are ZERO on an adopted plan (no consumer above reads them).
 *   u_high_ptrs_dev  device table [P] of U_high [rows, k]; u_low_ptrs_dev: [P] of U_low [rows, r - k]; mean_ptrs_dev: [P] of
 *                    mean [rows] fp32, NULL exactly when cfg.center == 0 (mean_dev may then be NULL too).  Element type of
 *                    U: fp16 / fp32 as cfg.fp16 says.  Every source is on the device, row-major and contiguous and starts
 *                    on a 16-byte boundary (the caller's contract: the addresses live on the device, the host cannot see
 *                    them; what it can see -- NULL tables or buffers, tables off 8 bytes, buffers off 16 -- is SVDQ_EINVAL).
 *                    A table entry whose tensor is empty (k = 0, r = k, rows = 0) is never dereferenced.
 *   what it does     ONE streaming launch over the plan's own work units: the unit (p, row0, nrows) copies rows
 *                    [row0, min(row0 + nrows, rows)) of U_high to slab_off[p], of U_low to slab_off[p] +
 *                    align256(rows * k * e), of mean to mean_off[p] (svdq_plan_basis_layout) -- each a contiguous byte
 *                    range of a row-major tensor, 16-byte aligned at both ends except a parameter's last bytes.  k, r and
 *                    rows are read from small_dev ON THE DEVICE (held to the slab: rows <= plan rows, r <= min(rows, N),
 *                    k <= r), so the call copies nothing to the host, synchronises nothing, allocates nothing and is
 *                    capturable like every other entry point.  rows[p] == 0: nothing of p is read or written.  Nothing is
 *                    written outside the three ranges of a parameter -- not the gap between U_high and U_low, not a slab's
 *                    or the buffers' tails.  small_dev is only read. */
int svdq_plan_import(const svdq_plan *plan, const void *u_high_ptrs_dev /*[P]*/, const void *u_low_ptrs_dev /*[P]*/,
                     const void *mean_ptrs_dev /*[P], NULL when center == 0*/, const void *small_dev, void *basis_dev,
                     float *mean_dev, void *stream);

/* ---- project NEW task tensors onto the basis a plan already holds (the one statement of the contract; the sources point
 *      here).  The reference's Step 5 on its own: compress_all_parameters (compress.py:173-207) -> compress_parameter ->
 *      compress_single_task -> project_to_basis (compress.py:6-56) with bases that were not made in this process -- loaded
 *      from disk, adopted, a caller's own U.  A new fine-tuned model is projected onto the stored bases, its coefficients
 *      are quantized, and it joins the store; no other task's checkpoint is read and no basis is recomputed.  Pass 2 of the
 *      compressor without pass 1: the basis, mean, k, r and rows in the plan's buffers are ONLY READ (they may come from
 *      any compress route or from svdq_plan_import), and the coefficient epilogue is the fused route's own code.
 *   task_ptrs_dev   [P*N], parameter-major: the tensor of task slot t of parameter p; a NULL entry = the slot is absent:
 *                   nothing of it is read and its fields in small_dev stay exactly as they were.  Element type: the plan's
 *                   input type (fp32 16-byte aligned, fp16 / bf16 8-byte aligned).
 *   base_ptrs_dev   NULL, or [P] base tensors of the same element type: the task tensors are then FINE-TUNED weights and
 *                   x[d] = finetuned[d] - base[d], one fp32 subtraction (compute_task_vector, task_vector_loader.py:103-141).
 *   index_ptrs_dev  NULL, or [P] int32 index lists (the ascending positions svdq_maskset_indices writes): row d of
 *                   parameter p is element index[p][d] of the full-size task (and base) tensors.  The mask walk is not
 *                   offered here.
 *   rows_dev        NULL (the plan's rows) or int64 [P]: rows of each parameter's basis, <= the plan's rows; 0 = nothing of
 *                   p is read or written.
 *   arithmetic      for every present slot: c[i] = sum_d float(U[d][i]) * xc[d] for i < r[p], columns < k[p] from U_high, the
 *                   rest from U_low; xc[d] = x[d] - mean[d] on a centred plan (one fp32 subtraction), x[d] otherwise.  Sums
 *                   are fp32 inside one block of at most 256 rows (the matrix pipe's chain over the block's rows) and fp64
 *                   across blocks and work units, in a fixed order without atomics: the same bits in every run.  Then
 *                   compress_single_task's tail: coef = the fp32 coefficients, c_high = coef[:k] as fp16, and codes, scale,
 *                   zero_point, residual_norm = RTVQQuantizer(bits[p], stages).quantize(coef[k:r]) bit for bit
 *                   (svdq_plan_set_low_bits is respected).
 *   launches        two: one streaming launch over the plan's own work units -- a block of basis, mean and base rows is
 *                   read once, and the rows of every present task once; one fp64 partial per unit goes to work_dev -- and
 *                   the fixed-order finish with the quantizer.
 *   never written   sigma, k, r, energy, rows, status, the basis and the mean; the fields of absent slots.
 *   errors          NULL plan, task_ptrs_dev, basis_dev, small_dev or work_dev, or a NULL mean_dev on a centred plan:
 *                   SVDQ_EINVAL before anything is launched.  (On an uncentred plan mean_dev is ignored.)
 *   work_dev        svdq_plan_project_work_bytes bytes (one N x N fp64 matrix per work unit).
 *   Allocates nothing, copies nothing to the host, synchronises nothing: capturable like every other entry point.  Any
 *   N <= SVDQ_MAX_TASKS, fp16 or fp32 basis. */
int64_t svdq_plan_project_work_bytes(const svdq_plan *plan);
int svdq_plan_project(const svdq_plan *plan, const void *task_ptrs_dev /*[P*N]; NULL entry = slot absent*/,
                      const void *base_ptrs_dev /*NULL or [P]*/, const void *index_ptrs_dev /*NULL or [P]*/,
                      const int64_t *rows_dev, const void *basis_dev, const float *mean_dev, void *small_dev,
                      void *work_dev, void *stream);

/* ---- extend the basis a plan holds by what NEW tasks add outside its span (the one statement of the contract; the
 *      sources point here).  No reference counterpart: the reference never adds a task to a store.  svdq_plan_project
 *      projects a new task onto the stored columns and drops what lies outside their span -- for a new fine-tuned model
 *      against r <= 32 stored directions that is nearly all of it.  These two entry points grow the stored U_high by the
 *      orthonormal directions of the new tasks' residuals, without any other task's checkpoint and without touching a
 *      stored column.  Call order per plan: svdq_plan_project (leaves the fp32 coefficients coef in small_dev) ->
 *      svdq_plan_residual_gram -> the host reads the m values (ONE small device-to-host copy of the extension buffer, to
 *      allocate the outputs) -> svdq_plan_extend_basis.  The two entry points themselves allocate nothing, copy nothing
 *      to the host and synchronise nothing.
 *   inputs          task_ptrs_dev, base_ptrs_dev, index_ptrs_dev, rows_dev, basis_dev, mean_dev: exactly as for
 *                   svdq_plan_project, and the same tensors.  small_dev is ONLY READ: k, r and coef[p][t][0..r), the fp32
 *                   coefficients svdq_plan_project has just left there (not the rounded or quantized ones).
 *   n_new           the new tasks sit in task slots [0, n_new), 1 <= n_new <= SVDQ_MAX_NEW_TASKS (8) and n_new <= N; a NULL
 *                   entry of task_ptrs_dev = the slot is absent for that parameter.  Slots >= n_new are never read.
 *   per entry p     with U = [U_high | U_low] [D, r] as stored, xc_j = x_j - mean (formed exactly as svdq_plan_project forms
 *                   it) and c_j = coef[p][j]:
 *     residual      e_j[d] = fma(-u[d][r-1], c_j[r-1], ... fma(-u[d][0], c_j[0], xc_j[d])), u = float(U[d][i]): one fp32 fma
 *                   chain in column order, U_high columns then U_low.  ONE device function serves both passes: the same
 *                   bits.  By construction xc_j = U c_j + e_j whether or not the rounded U is orthonormal.
 *     Gram          H = E^T E [n_new, n_new], n_j = |xc_j|^2 (and |e_j|^2 = H[j][j]).  fp32 inside one block of at most
 *                   256 rows (the matrix pipe's chain, v_mfma_f32_16x16x4f32; n_j: an fma chain over the lane's rows, then
 *                   the 64 lane sums in lane order), fp64 across blocks and work units in a fixed order, no atomics: the
 *                   same bits in every run.  H is NOT formed from Xc^T Xc - 2 C^T C + ...: that cancels exactly when a task
 *                   lies almost in the span, the case the threshold has to judge.
 *     eigen stage   H = W L W^T in fp64 (the Jacobi of the compressor's eigen stage) over the PRESENT slots, lambda
 *                   descending, each eigenvector's sign fixed so that its largest-magnitude component is positive.
 *                   Direction i is kept iff lambda_i > min_residual^2 * max_j n_j and i < min(present slots, D - r);
 *                   m = the number kept.  Z = W[:, :m] L^-1/2 [slot][column] and d_j = (L^1/2 W^T)[:m, j], task j's
 *                   coefficients on the new columns, both fp32 (absent slots: zeros).
 *     min_residual  relative to the largest |xc_j|.  Default 2^-12: the worst-case fp32 noise of the residual relative to
 *                   |xc| is about (r + 2) 2^-24 sqrt(r) <= 1.2e-5 at r = 32, 16 x or more below the threshold, and the
 *                   threshold is far below what a 4-bit c_low resolves.  Must be finite and >= 0.
 *   non-finite data a NaN or +-Inf among the rows of a present slot makes that slot's n_j NaN or +Inf (a sum of squares; so does
 *                   finite data whose squares overflow fp32).  The eigen stage then decomposes nothing: m = 0, lambda, Z
 *                   and d are zeros, the entry is not extended, and n_j in ext_dev is the flag -- every healthy n_j is finite.
 *                   CompressPlan.residual_gram raises NonFiniteInput on it, as the compress route does on a NaN energy.
 *   ext_dev         svdq_plan_extend_layout bytes, 16-byte aligned; every field of every parameter is written by
 *                   svdq_plan_residual_gram (rows = 0: zeros), so the buffer is the same bytes in every run.
 *   work_dev        svdq_plan_residual_gram_work_bytes bytes: per work unit one fp64 [8][8] partial of H and [8] of n.
 *   svdq_plan_extend_basis   the same walk again: e recomputed by the same device function, q[d][c] = sum_j e_j[d] Z[j][c]
 *                   as an fp32 fma chain from 0 over j in slot order, and row d of out_ptrs_dev[p] -- the caller's U_high'
 *                   [D, k + m] row-major in the basis element type -- = the k stored U_high elements of the row, copied bit
 *                   for bit, then the m new ones rounded to the element type (fp16: round to nearest even).  m is read from
 *                   ext_dev ON THE DEVICE.  A parameter with m = 0, rows = 0 or a NULL out_ptrs_dev[p] is not written at
 *                   all, and nothing is written past D (k + m) elements.  out tensors: 16-byte aligned (caller's contract).
 *   the extended entry   U_high' = [U_high | Q], U_low unchanged, k' = k + m.  Old tasks: c_high' = [c_high, 0 ... 0]
 *                   (fp16 holds their zeros exactly; an affine RTVQ code has no exact zero -- hence the high side), c_low
 *                   untouched.  New tasks: c_high' = fp16([coef[:k], d_j]), c_low as svdq_plan_project quantized it.
 *                   singular_values' = [sigma[:k], sqrt(lambda[:m]), sigma[k:]] -- no longer globally descending; its
 *                   first k' entries are still the high columns.  This bookkeeping is the host's (compress.extend_bases).
 *   launches        svdq_plan_residual_gram: the streaming launch over the plan's own work units (one wavefront each) and
 *                   the eigen launch (one workgroup per parameter).  svdq_plan_extend_basis: one streaming launch.
 *   errors          SVDQ_EINVAL before anything is launched: a NULL plan, task_ptrs_dev, basis_dev, small_dev, ext_dev,
 *                   work_dev or out_ptrs_dev; a NULL mean_dev on a centred plan; tables, rows or work off 8 bytes; small,
 *                   basis, mean or ext off 16; n_new outside [1, min(8, N)]; min_residual negative or not finite.
 *   Any N <= SVDQ_MAX_TASKS plan slots (the 8-, 16- and 32-slot instantiations), fp16 or fp32 basis, every input form of
 *   svdq_plan_project (from-base, index lists, fp16 / bf16 inputs). */
#define SVDQ_MAX_NEW_TASKS 8
typedef struct svdq_extend_layout {
    int64_t m_off;          /* int32  [P]        new columns kept                                          */
    int64_t lambda_off;     /* double [P][8]     eigenvalues of H over the present slots, descending       */
    int64_t z_off;          /* float  [P][8][8]  Z[slot][column], first m columns valid                    */
    int64_t d_off;          /* float  [P][8][8]  d[slot][column]: the slot's coefficients on the new columns */
    int64_t xnorm_off;      /* double [P][8]     n_j = |xc_j|^2                                            */
    int64_t enorm_off;      /* double [P][8]     |e_j|^2 = H[j][j]                                         */
    int64_t total_bytes;
} svdq_extend_layout;
int64_t svdq_plan_residual_gram_work_bytes(const svdq_plan *plan);
int svdq_plan_extend_layout(const svdq_plan *plan, svdq_extend_layout *out);
int svdq_plan_residual_gram(const svdq_plan *plan, const void *task_ptrs_dev /*[P*N]; NULL entry = slot absent*/,
                            const void *base_ptrs_dev /*NULL or [P]*/, const void *index_ptrs_dev /*NULL or [P]*/,
                            const int64_t *rows_dev, const void *basis_dev, const float *mean_dev, const void *small_dev,
                            int32_t n_new, float min_residual, void *ext_dev, void *work_dev, void *stream);
int svdq_plan_extend_basis(const svdq_plan *plan, const void *task_ptrs_dev, const void *base_ptrs_dev,
                           const void *index_ptrs_dev, const int64_t *rows_dev, const void *basis_dev,
                           const float *mean_dev, const void *small_dev, int32_t n_new, const void *ext_dev,
                           const void *out_ptrs_dev /*[P] U_high' [D, k + m]; NULL entry = not written*/, void *stream);

/* ---- the task Gram of a STORE: G[t][s] = <delta_t, delta_s> of the task vectors the stored artifacts reconstruct (the
 *      one statement of the contract; the sources point here).  What the reference's cluster weighting looks at --
 *      flatten_task_vectors (clustering.py:55-120) stacks the task vectors, cluster_tasks (clustering.py:198-245) clusters
 *      the unit-normalised rows, and k-means / Ward only ever see their inner products -- computed from a plan's basis,
 *      mean and small buffer alone: no fine-tuned checkpoint is read and no reconstructed model is written.
 *   the identity    per parameter p, with A = [U_high | U_low | mean] [D, r + 1] and c'_t = [c_t ; 1] (c_t = the fp16
 *                   c_high then the dequantized c_low of task slot t, exactly the values svdq_merge reconstructs from):
 *                   delta_t = A c'_t, so G_p[t][s] = c'_t^T (A^T A) c'_s.  On an uncentred plan A = U and c'_t = c_t.
 *                   U^T U is the real one, not I: stored columns are fp16 roundings, svdq_plan_extend_basis appends
 *                   columns, and svdq_plan_import accepts any caller's U.  No scale (noise_shrink) is applied: the
 *                   reference clusters raw task vectors.
 *   inputs          rows_dev, small_dev, basis_dev, mean_dev: exactly as for svdq_plan_project -- k, r (held to the slab:
 *                   r <= min(rows, N), k <= r) and, with rows_dev pointing at the small buffer's rows field, rows are read
 *                   ON THE DEVICE.  All of them are ONLY READ.  rows[p] == 0: nothing of p is read, zeros are written.
 *   arithmetic      A^T A: sums are fp32 inside one block of at most 256 rows (U^T U on the matrix pipe -- fp16 basis:
 *                   v_mfma_f32_16x16x32_f16, whose fp16 x fp16 products are exact in fp32; fp32 basis: v_mfma_f32_16x16x4_f32;
 *                   the mean column as fp32 fma chains over at most 4 rows per lane) and fp64 across blocks, lanes and work
 *                   units, in a fixed order without atomics: the same bits in every run.  The coefficients are fp32 as the
 *                   merge dequantizes them; C' (A^T A) C'^T is fp64, formed for t <= s and mirrored: exactly symmetric.
 *   launches        two: one streaming launch over the plan's own work units (one wavefront each; a block of basis rows is
 *                   staged once and is both operands of U^T U; one fp64 partial per unit goes to work_dev) and the
 *                   fixed-order finish, one workgroup per parameter.  Reads 2 r + 4 bytes per row with an fp16 basis.
 *   task_gram_dev   double [P][N][N], every entry written.  The per-parameter matrices are additive: the store's Gram is
 *                   their sum, scattered by task name on the host (a plan's slot t may be another task in another entry).
 *   basis_gram_dev  NULL, or double [P][33][33], every entry written: A^T A in rows / columns [0, r], row / column r = the
 *                   mean (absent on an uncentred plan), zeros elsewhere.  max |U^T U - I| over its leading r x r block is
 *                   the orthonormality of a stored or extended basis.
 *   work_dev        svdq_plan_store_gram_work_bytes bytes: per work unit one fp64 [N][N] and one [N + 1].
 *   errors          SVDQ_EINVAL before anything is launched: a NULL plan, small_dev, basis_dev, work_dev or task_gram_dev; a
 *                   NULL mean_dev on a centred plan (on an uncentred plan it is ignored); rows, work or an output off 8
 *                   bytes; small, basis or mean off 16.
 *   Allocates nothing, copies nothing to the host, synchronises nothing: capturable like every other entry point.  Any
 *   N <= SVDQ_MAX_TASKS, fp16 or fp32 basis, fused or adopted plans. */
int64_t svdq_plan_store_gram_work_bytes(const svdq_plan *plan);
int svdq_plan_store_gram(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev, const void *basis_dev,
                         const float *mean_dev, void *work_dev, double *task_gram_dev /*[P][N][N]*/,
                         double *basis_gram_dev /*NULL or [P][33][33]*/, void *stream);

/* ---- consolidate a STORE: bases, rank and mean re-derived from the artifacts alone (the one statement of the contract;
 *      the sources point here).  No reference counterpart.  svdq_plan_extend_basis appends columns (singular values no
 *      longer descending, the k + M <= 32 room used up), a task cannot be dropped from a store (its share stays in the
 *      mean), and a store cannot be taken to another energy threshold, max_rank, low_bits or stage count without the
 *      fine-tuned checkpoints.  These entry points return a store to the form a fresh compress run of the tasks it
 *      reconstructs would give it, without materialising a task model: per entry delta_t = A c'_t, so the SVD of the kept
 *      tasks is an N' x N' problem on top of A^T A, plus one linear map of the stored rows, U' = A W.
 *   call order      per source plan: svdq_plan_store_gram(src, ..., basis_gram_dev) -> svdq_plan_consolidate_eig ->
 *                   svdq_plan_rebase.  Four launches (the streaming Gram and its finish, the eigen stage, the streaming
 *                   rebase); none copies to the host, allocates or synchronises: capturable like every other entry point.
 *   the two plans   src: the plan that holds the store (any compress route or svdq_plan_import).  dst: a plan created with
 *                   the SAME rows per parameter and the same basis element type (cfg.fp16), N' task slots and the settings
 *                   the consolidated store is to have: cfg.center, energy_threshold, max_rank, low_bits (per parameter:
 *                   svdq_plan_set_low_bits) and rtvq_stages.  No conversion of the element type is offered.
 *   keep            int32 [P][N']: destination slot j of parameter p takes source slot keep[p][j]; -1 = the slot is absent
 *                   (this is how tasks are dropped).  keep_host is what the call validates (the device cannot refuse
 *                   before a launch), keep_dev holds the same values on the device and is what the kernel reads.
 *   per entry p     (one parameter region) with A = [U_high | U_low | mean] [D, r + 1] as stored (an uncentred source has
 *                   no mean column) and M = A^T A as svdq_plan_store_gram forms it (fp32 sums inside blocks of at most 256
 *                   rows, fp64 across blocks, a fixed order):
 *     coefficients  b_j = [c_j ; 1], c_j = the fp16 c_high then the dequantized c_low of source slot keep[p][j] -- the
 *                   merge's own dequantizing lines, exactly the values every consumer reconstructs from.
 *     centring      bbar = the mean of the kept b_j in task order (fp64) on a centred destination, else 0;
 *                   Bc = B - bbar 1^T.  A centred source going to an uncentred destination keeps the 1 row in B (the old
 *                   mean is folded into the data); the reverse direction is allowed too.
 *     eigen stage   K = Bc^T M Bc in fp64, the fp64 Jacobi of the compressor's eigen stage, lambda descending, each
 *                   eigenvector's sign fixed so that its largest-magnitude component is positive.
 *     keep rule     M carries a relative error gamma = (256 + r + 3) 2^-24 against |A|^T |A|, and |A|^T |A|[i][j] <=
 *                   sqrt(M_ii M_jj), so ||dK|| <= eta := gamma sum_j g_j^2 with g_j = sum_i sqrt(M_ii) |Bc[i][j]| (fp64, on
 *                   the device).  Direction i is kept iff lambda_i > max(4 eta, min_sigma^2 lambda_0), i < min(kept
 *                   tasks, D) and lambda_i > 0: above 4 eta the true eigenvalue is positive and within 25 % of the computed
 *                   one; below it the column A w_i / sigma_i is amplified rounding noise.  r' = the number kept.
 *                   Unresolved directions are DROPPED, not kept as zero or completion columns (svdq_plan_import accepts
 *                   r < min(rows, N)); dropped_energy = the sum of the dropped lambda_i, each clipped at 0.
 *                   min_sigma: finite and >= 0, 0 = the noise floor alone.
 *     rank rule     k' and energy_retained: the reference's fp32 cumulative rule (basis.py:147-156, :199-211) on
 *                   sigma' = sqrt(lambda[:r']), with svdq_eig_rank_select's fp64 form when the fp32 sum overflows.
 *     new artifacts W = Bc V_r' Sigma^-1 [r (+ 1)][r'], U' = A W split at k' into U_high' and U_low', mean' = A bbar on a
 *                   centred destination.  Coefficients: the closed form c'_j[i] = sgn_i sigma_i V[j][i], fp64 then fp32 --
 *                   the coefficients of the UNROUNDED U'.  By construction A W c'_j + A bbar = A b_j minus the dropped part,
 *                   whatever the accuracy of V; projecting onto the rounded columns instead would make the reconstruction
 *                   depend on how orthonormal they came out, so that is not done.  Then compress_single_task's tail
 *                   through the compressor's own epilogue: coef = the fp32 c', c_high = fp16(c'[:k']), c_low =
 *                   RTVQ(bits[p], stages)(c'[k':r']) bit for bit.  Absent destination slots: zeros in every field.
 *     non-finite    a non-finite entry of M or of a kept coefficient flags the entry as every eigen stage does
 *                   (svdq_eig_rank_select above): energy and sigma are NaN, k = min(1, r), r = min(D, kept tasks), rows = D,
 *                   W is zero, no Jacobi sweep runs, and svdq_plan_rebase writes nothing of the entry.
 *     nothing to do rows == 0 or no kept task: nothing of p is read, the destination's fields are zeros (rows = 0: every
 *                   consumer skips the entry), and no row is written.
 *   dst_small_dev   the destination plan's small buffer: sigma / k / r / energy / rows / c_high / codes / scale /
 *                   zero_point / residual_norm / coef / status of EVERY entry are written on every run.
 *   rebase_dev      svdq_plan_consolidate_layout bytes, 16-byte aligned; every field of every entry is written by
 *                   svdq_plan_consolidate_eig, so the buffer is the same bytes in every run.
 *   svdq_plan_rebase   one streaming launch over the SOURCE plan's work units, one wavefront each, the geometry and
 *                   staging of svdq_plan_store_gram (blocks of 256 rows up to 16 source slots, 128 above; the mean rows
 *                   beside the basis rows; the next block's loads in flight during compute).  Row d of [U' | mean'] =
 *                   row d of A times [W | bbar] on the matrix pipe (v_mfma_f32_16x16x4_f32, basis elements widened to fp32
 *                   exactly): fp32 sums over the source columns in one fixed order, four columns per instruction in column
 *                   order, U_high then U_low, the mean column last -- the same bits in every run (how the matrix pipe
 *                   orders the four products of one instruction is the hardware's; the error is that of r + 1 fp32 terms).  Results are rounded to the element type (fp16: nearest
 *                   even; mean': fp32) and go straight into the DESTINATION plan's buffers at svdq_plan_basis_layout's
 *                   offsets: U_high' at slab_off[p], U_low' at slab_off[p] + align256(rows k' e), mean' at mean_off[p].
 *                   k', r' and W are read from rebase_dev ON THE DEVICE.  Nothing is written outside the three ranges of a
 *                   parameter -- not the gap between U_high' and U_low', not a slab's or the buffers' tails.  The source's
 *                   buffers are only read.  Reads 2 r + 4 and writes 2 r' + 4 bytes per row with an fp16 basis.
 *   errors          SVDQ_EINVAL before anything is launched: a NULL plan or buffer; a NULL mean on a centred source (or
 *                   destination); tables off 8 bytes, buffers off 16; a destination plan whose parameter count, rows or
 *                   element type differ from the source's; N' > SVDQ_MAX_TASKS; a keep entry outside [-1, N);
 *                   min_sigma negative or not finite.
 *   Any N, N' <= SVDQ_MAX_TASKS (the 8-, 16- and 32-slot instantiations of the source), fp16 or fp32 basis, fused or
 *   adopted source plans. */
typedef struct svdq_consolidate_layout {
    int64_t w_off;          /* float  [P][33][32] W[source column][new column]; row r = the mean column of a centred source */
    int64_t bbar_off;       /* float  [P][33]     bbar over the source columns (zeros on an uncentred destination)        */
    int64_t r_off;          /* int32  [P]         r': directions kept                                                      */
    int64_t k_off;          /* int32  [P]         k'                                                                       */
    int64_t live_off;       /* int32  [P]         1 = svdq_plan_rebase writes the entry (rows > 0, a kept task, finite)    */
    int64_t dropped_off;    /* double [P]         dropped_energy                                                           */
    int64_t eta_off;        /* double [P]         eta, the bound on ||dK||                                                 */
    int64_t lambda_off;     /* double [P][32]     eigenvalues of K over the kept tasks, descending                         */
    int64_t total_bytes;
} svdq_consolidate_layout;
int svdq_plan_consolidate_layout(const svdq_plan *plan, svdq_consolidate_layout *out);
int svdq_plan_consolidate_eig(const svdq_plan *src_plan, const svdq_plan *dst_plan, const int32_t *keep_host /*[P][N']*/,
                              const int32_t *keep_dev /*[P][N']*/, const int64_t *rows_dev, const void *src_small_dev,
                              const double *basis_gram_dev /*[P][33][33]*/, float min_sigma, void *dst_small_dev,
                              void *rebase_dev, void *stream);
int svdq_plan_rebase(const svdq_plan *src_plan, const svdq_plan *dst_plan, const int64_t *rows_dev,
                     const void *src_small_dev, const void *src_basis_dev, const float *src_mean_dev,
                     const void *rebase_dev, void *dst_basis_dev, float *dst_mean_dev, void *stream);

/* ---- the sign-elected (TIES) merge of a store, in streaming passes over the basis.  The reference's dispatcher lists
 *      "ties" beside "svd_hybrid" and implements none (cli.py answers "not yet implemented"); the definition is Yadav et
 *      al. 2023 as published in the authors' code (topk_values_mask -> resolve_sign -> disjoint_merge), on what the store
 *      reconstructs: v_t[d] = the value svdq_task_reconstruct writes for task t at row d, bit for bit
 *      (RTVQQuantizer.dequantize rtvq.py:85-103 + reconstruct_from_coefficients merge.py:144-194), 0 on the rows of a
 *      parameter the task lacks.  With D the rows of ALL parameters of the store and T its tasks in sorted-name order:
 *        trim   tau_t = the j-th smallest |v_t[.]| over all D rows, j = max(D - int(D * density), 1); v_t[d] is kept iff
 *               |v_t[d]| >= tau_t (equal magnitudes at the threshold are all kept)
 *        elect  s[d] = the kept v_t[d] added in task order, each sum rounded in fp32; positive iff s[d] >= 0 (s == 0
 *               elects positive: the published code asks the sign majority of the whole model there)
 *        merge  a[d] = the kept values whose sign strictly agrees (v > 0 / v < 0) added in task order, c[d] their number;
 *               mean: a / max(c, 1) (one fp32 division), sum: a
 *        apply  out = base + scaling * merged (one product, one sum; without base the product)
 *      No buffer proportional to D * T exists at any point: the values are formed in registers, pass by pass, by the
 *      streaming structure of svdq_task_reconstruct (fma chains, hi + lo, + mean on a centred plan), so every pass sees
 *      the same bits.  tau_t is found EXACTLY by a radix selection on the magnitude bits (bits & 0x7fffffff, as unsigned
 *      integers ordered like the magnitudes), 8 bits per pass from the top, SVDQ_TIES_DIGITS passes:
 *        for digit in 0 .. SVDQ_TIES_DIGITS - 1:
 *            svdq_plan_ties_hist(plan, ..., digit, state, ...)      for every plan of the store
 *            svdq_ties_select_step(state, T, digit, j, zeros)       once
 *        svdq_plan_ties_merge(plan, ..., state, ...)                for every plan of the store
 *      state_dev: ONE table of svdq_ties_work_bytes(T) bytes shared by all plans of the store (thresholds are global),
 *      zeroed by the caller before digit 0; uint64 words: hist [T][256] | prefix [T] (after the last digit: the bit
 *      pattern of tau_t in the low 32 bits) | rank [T] | kept [T] (values kept per task, implicit zeros included) |
 *      rows with kept values of both signs | rows with nothing kept.  Counts are integers added by atomics, one flush per
 *      work unit: no result depends on the order the units run in.  State, histogram and thresholds stay on the device.
 *   slot_task_dev int32 [P][n_out]: the plan task index behind slot j of parameter p.
 *   task_map_dev  int32 [P][n_out]: the store task (0 .. T-1) behind slot j of parameter p, -1 = the slot is unused.  The
 *                 live slots of a parameter must name its store tasks in ASCENDING order: slot order is the order of the
 *                 sums.  Like svdq_task_reconstruct's table the entries live on the device and are the caller's to have
 *                 checked; a slot outside [0, T) or [0, N) is skipped.
 *   svdq_plan_ties_hist   counts, for every row of the plan and every live slot whose magnitude bits above `digit` equal
 *                 the task's prefix, the digit's value.  Reads the basis once (as svdq_task_reconstruct), writes nothing
 *                 but the table.
 *   svdq_ties_select_step  one small launch: per task the bin that holds the wanted rank (walked from the top), appended
 *                 to the prefix; the remaining rank; the histogram zeroed for the next digit.  rank: j, read at digit 0.
 *                 zeros_dev NULL or int64 [T]: the rows of the parameters task t lacks -- implicit zeros, counted in bin 0
 *                 while the prefix is all zero.
 *   svdq_plan_ties_merge  elect, merge, apply for every parameter with a non-NULL output: out_ptrs_dev [P] fp32 tensors of
 *                 rows[p] elements, base_ptrs_dev NULL or [P] (NULL entry = no base); merge_sum 0 = mean, else sum.  Adds
 *                 the by-products to the table.
 *   rows_dev, small_dev, basis_dev, mean_dev: as for svdq_task_reconstruct.  work_dev: svdq_task_reconstruct_work_bytes(
 *                 plan, n_out) bytes (the live tasks' coefficients).
 *   errors        SVDQ_EINVAL before anything is launched: a NULL plan, buffer or table; n_out or n_tasks outside
 *                 [1, SVDQ_MAX_TASKS]; a digit outside [0, SVDQ_TIES_DIGITS); a missing mean on a centred plan; rank < 1.
 *   Allocates nothing, copies nothing to the host, synchronises nothing: capturable like every other entry point.  Works
 *   on plans filled by any compress route and on plans filled by svdq_plan_import.  Non-finite values are outside the
 *   definition. */
#define SVDQ_TIES_DIGITS 4
int64_t svdq_ties_work_bytes(int32_t n_tasks);
int svdq_plan_ties_hist(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev, const void *basis_dev,
                        const float *mean_dev, const int32_t *slot_task_dev /*[P][n_out]*/,
                        const int32_t *task_map_dev /*[P][n_out]*/, int32_t n_out, int32_t n_tasks, int32_t digit,
                        void *state_dev, void *work_dev, void *stream);
int svdq_ties_select_step(void *state_dev, int32_t n_tasks, int32_t digit, int64_t rank,
                          const int64_t *zeros_dev /*NULL or [T]*/, void *stream);
int svdq_plan_ties_merge(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev, const void *basis_dev,
                         const float *mean_dev, const int32_t *slot_task_dev /*[P][n_out]*/,
                         const int32_t *task_map_dev /*[P][n_out]*/, int32_t n_out, int32_t n_tasks, int32_t merge_sum,
                         float scaling, const void *base_ptrs_dev /*NULL or [P]*/, const void *out_ptrs_dev /*[P]*/,
                         void *state_dev, void *work_dev, void *stream);

/* ---- the Model Breadcrumbs merge of a store (Davari & Belilovsky 2023: "Model Breadcrumbs: Scaling Multi-Task Model
 *      Merging with Sparse Masks"), and with it the per-tensor trim: a two-sided magnitude band per weight tensor and
 *      task, in streaming passes over the basis.  The definition, on what the store reconstructs:
 *        inputs   T tasks in sorted-name order.  For parameter p with D_p rows and a task t that has p: v_t[d] = the value
 *                 svdq_task_reconstruct writes for task t at row d, bit for bit (RTVQQuantizer.dequantize rtvq.py:85-103
 *                 + reconstruct_from_coefficients merge.py:144-194), m = |v_t[d]|.  A task that lacks p contributes
 *                 nothing to p: ranks are per tensor, so this operator has no implicit zeros.
 *        counts   Python integers per parameter, computed by the caller: n_keep = int(D_p * density), n_top = int(D_p *
 *                 gamma), n_bot = D_p - n_keep - n_top; if n_bot < 0: n_top += n_bot, n_bot = 0 (the outlier cut gives
 *                 way so the density is met).
 *        band     n_keep == 0: nothing of (p, t) is kept.  Otherwise lo = the (n_bot + 1)-th smallest magnitude of
 *                 (p, t), hi = the (D_p - n_top)-th smallest; a value is kept iff lo <= m <= hi.  Equal magnitudes at
 *                 either threshold are all kept, so kept >= n_keep.  density >= 1 keeps everything, whatever gamma is.
 *        combine  in task order over the kept values, every sum rounded in fp32.  sign_election 0: a = their sum, c =
 *                 their number.  sign_election != 0: s = their sum, positive iff s >= 0 (s == 0 elects positive, as for
 *                 svdq_plan_ties_merge); a and c run over the kept values whose sign strictly agrees (v > 0 / v < 0).
 *                 merge_sum != 0: a; else the mean a / max(c, 1), one fp32 division.
 *        apply    out = base + scaling * merged (one product, one sum, each rounded; without base the product)
 *      The paper's method is sign_election 0, sum, density = gamma_paper - beta_paper, gamma = 1 - gamma_paper; the
 *      per-tensor TIES trim is gamma = 0, sign_election 1, mean.  lo and hi are found EXACTLY by a radix selection on the
 *      magnitude bits (bits & 0x7fffffff), 8 bits per pass from the top, SVDQ_CRUMBS_DIGITS passes, per plan:
 *        for digit in 0 .. SVDQ_CRUMBS_DIGITS - 1:
 *            svdq_plan_crumbs_hist(plan, ..., digit, bounds, state, ...)   once with bounds 3 for n_out <= 16; above
 *                                                                          twice, bounds 1 then bounds 2
 *            svdq_plan_crumbs_select_step(plan, T, digit, ranks, state)    once
 *        svdq_plan_crumbs_merge(plan, ..., state, ...)
 *      state_dev: ONE table per plan (thresholds never cross parameters) of svdq_crumbs_work_bytes(P, T) bytes, zeroed by
 *      the caller before digit 0: hist uint32 [P][2][T][256], then uint64 words prefix [P][2][T] (bound 0 = lo, 1 = hi;
 *      after the last digit the bit pattern of the bound in the low 32 bits; a (p, t) that keeps nothing ends with the
 *      sentinel band lo = 0xffffffff, hi = 0) | rank [P][2][T] | kept [P][T] | rows with kept values of both signs | rows
 *      with nothing kept.  Counts are integers added by atomics, one flush per work unit: no result depends on the order
 *      the units run in, two calls give identical bits.  Histogram counts are 32-bit: a plan with a parameter of 2^32
 *      rows or more is refused.
 *   svdq_plan_crumbs_hist  counts, for every live slot and every bound named by `bounds` (1 = lo, 2 = hi, 3 = both), the
 *                 digit's value of the magnitudes whose bits above `digit` equal that bound's prefix.  Both bounds in one
 *                 pass need [2][16][256] counters in LDS: bounds 3 is refused for n_out > 16.
 *   svdq_plan_crumbs_select_step  one small launch, one thread per (parameter, task, bound): the bin that holds the
 *                 wanted rank (walked from the top), appended to the prefix; the remaining rank; the histograms it read
 *                 zeroed.  ranks_dev int64 [P][2], read at digit 0: n_bot + 1 and D_p - n_top, or 0 and 0 for a
 *                 parameter with n_keep == 0.  A (p, t) without counts at digit 0 is no live task of the parameter.
 *   svdq_plan_crumbs_merge  band, elect, combine, apply for every parameter with a non-NULL output; adds the by-products
 *                 to the table.
 *   slot_task_dev, task_map_dev, n_out, n_tasks, rows_dev, small_dev, basis_dev, mean_dev, base_ptrs_dev, out_ptrs_dev,
 *                 work_dev: as for svdq_plan_ties_merge (live slots in ASCENDING store order).
 *   errors        SVDQ_EINVAL before anything is launched: a NULL plan, buffer or table; n_out or n_tasks outside
 *                 [1, SVDQ_MAX_TASKS]; a digit outside [0, SVDQ_CRUMBS_DIGITS); bounds outside {1, 2, 3}; a missing mean
 *                 on a centred plan; a parameter of 2^32 rows or more.
 *   Allocates nothing, copies nothing to the host, synchronises nothing.  Works on plans filled by any compress route and
 *   on plans filled by svdq_plan_import.  Non-finite store values are outside the definition, as for TIES. */
#define SVDQ_CRUMBS_DIGITS 4
int64_t svdq_crumbs_work_bytes(int32_t n_params, int32_t n_tasks);
int svdq_plan_crumbs_hist(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev, const void *basis_dev,
                          const float *mean_dev, const int32_t *slot_task_dev /*[P][n_out]*/,
                          const int32_t *task_map_dev /*[P][n_out]*/, int32_t n_out, int32_t n_tasks, int32_t digit,
                          int32_t bounds /*1 lo, 2 hi, 3 both*/, void *state_dev, void *work_dev, void *stream);
int svdq_plan_crumbs_select_step(const svdq_plan *plan, int32_t n_tasks, int32_t digit,
                                 const int64_t *ranks_dev /*[P][2]*/, void *state_dev, void *stream);
int svdq_plan_crumbs_merge(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev, const void *basis_dev,
                           const float *mean_dev, const int32_t *slot_task_dev /*[P][n_out]*/,
                           const int32_t *task_map_dev /*[P][n_out]*/, int32_t n_out, int32_t n_tasks,
                           int32_t sign_election, int32_t merge_sum, float scaling,
                           const void *base_ptrs_dev /*NULL or [P]*/, const void *out_ptrs_dev /*[P]*/, void *state_dev,
                           void *work_dev, void *stream);

/* ---- the drop-and-rescale (DARE) merge of a store, and task arithmetic from a store, in ONE streaming pass over the
 *      basis.  The reference's dispatcher lists "dare" and "task_arithmetic" beside "svd_hybrid" and implements neither
 *      (cli.py answers "not yet implemented"; scripts/main.py keeps that answer); the definition is Yu et al. 2024
 *      ("Language Models are Super Mario": thin every task vector by a random mask with drop rate p, rescale the
 *      survivors by 1 / (1 - p), combine linearly), on what the store reconstructs:
 *        inputs   T tasks in sorted-name order, store task index g = 0 .. T-1; the parameters of the store in sorted-name
 *                 order, row_base[name] = the sum of the rows of the parameters before it, G = row_base + d (int64) the
 *                 GLOBAL row of row d; v_t[G] = the value svdq_task_reconstruct writes for task t, bit for bit
 *                 (RTVQQuantizer.dequantize rtvq.py:85-103 + reconstruct_from_coefficients merge.py:144-194).  A task that
 *                 lacks a parameter contributes nothing on its rows.
 *        draw     Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9,
 *                 0xBB67AE85), key (seed & 0xffffffff, seed >> 32), counter (G & 0xffffffff, G >> 32, g >> 2, 0); task g
 *                 uses output word g & 3 (one call serves four tasks of a row).  drop_threshold = min(int(drop_rate *
 *                 2^32), 2^32 - 1), computed by the caller in double; the value is DROPPED iff word < drop_threshold.
 *                 drop_threshold 0 drops nothing and the generator is skipped (wave-uniform): task arithmetic.
 *        rescale  q = float32(1.0 - drop_rate) (a double subtraction, rounded once) = keep_scale; a kept value becomes
 *                 v / q, ONE correctly rounded fp32 division; keep_scale 0 = no rescale, the kept value is v.
 *        combine  m[G] starts at +0; for the kept tasks in ascending g: m = m + w_g * x, the product rounded, then the sum
 *                 rounded.  Dropped and lacking tasks are skipped, not added as zeros.  w_g fp32 (weights_dev [T]).
 *        apply    out = base + scaling * m (one product, one sum, each rounded; without base the product)
 *      By-product: the values kept per task, uint64 kept [T] in state_dev (svdq_dare_work_bytes(T) bytes, zeroed by the
 *      caller, shared by all plans of the store), integer atomics, one flush per work unit.  No result depends on the order
 *      the units run in: two calls give identical bits.  Non-finite store values are outside the definition, as for TIES.
 *   slot_task_dev, task_map_dev, n_out, n_tasks, rows_dev, small_dev, basis_dev, mean_dev, base_ptrs_dev, out_ptrs_dev:
 *                 as for svdq_plan_ties_merge (live slots in ASCENDING store order: slot order is the order of the sums,
 *                 and what lets a quad's Philox block be computed once).  row_base_dev int64 [P]: row_base of every
 *                 parameter of the plan.  work_dev: svdq_task_reconstruct_work_bytes(plan, n_out) bytes.
 *   errors        SVDQ_EINVAL before anything is launched: a NULL plan, buffer or table (row_base_dev, weights_dev and
 *                 out_ptrs_dev included); n_out or n_tasks outside [1, SVDQ_MAX_TASKS]; a missing mean on a centred plan.
 *   Allocates nothing, copies nothing to the host, synchronises nothing.  Works on plans filled by any compress route and
 *   on plans filled by svdq_plan_import. */
int64_t svdq_dare_work_bytes(int32_t n_tasks);
int svdq_plan_dare_merge(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev, const void *basis_dev,
                         const float *mean_dev, const int32_t *slot_task_dev /*[P][n_out]*/,
                         const int32_t *task_map_dev /*[P][n_out]*/, int32_t n_out, int32_t n_tasks,
                         const int64_t *row_base_dev /*[P]*/, const float *weights_dev /*[T]*/, uint64_t seed,
                         uint32_t drop_threshold, float keep_scale /*q; 0 = no rescale*/, float scaling,
                         const void *base_ptrs_dev /*NULL or [P]*/, const void *out_ptrs_dev /*[P]*/, void *state_dev,
                         void *work_dev, void *stream);

/* ---- TALL masks and the consensus merge of a store (Wang et al. 2024: "Localizing Task Information for Improved Model
 *      Merging and Compression") in ONE streaming pass over the basis.  The package reads TALL_mask_{n}task files
 *      (load_tall_mask_file, combine_tall_masks_packed, --mask-dir) that were made from the fine-tuned checkpoints; this
 *      entry point makes them from what the store reconstructs, and merges by the consensus of the masks:
 *        inputs   T tasks in sorted-name order, store task index g = 0 .. T-1 (the index among the MERGED tasks where a
 *                 subset is merged); v_t[d] = the value svdq_task_reconstruct writes for task t at row d of a parameter,
 *                 bit for bit.  A task that lacks a parameter contributes nothing on its rows and its mask bits there
 *                 are 0.  lambda_g fp32, finite and >= 0 (lambdas_dev [T]); min_agree = k, an integer in [0, T].
 *        sum      S starts at +0; for the tasks that have the parameter, in ascending g: S = S + v_g, every sum rounded
 *                 in fp32.
 *        mask     R_g = S - v_g (one fp32 subtraction); m_g = |v_g| > lambda_g * |R_g|, the product rounded once, the
 *                 comparison STRICT.  The paper writes ">="; the comparison here is ">" by decision (to the best of our
 *                 knowledge what the authors' published code does -- not verified here), and strict makes a row where
 *                 every value is zero inactive.  Consequences: lambda_g = 0 marks every non-zero value; with T = 1 the
 *                 mask is v != 0.
 *        consensus  c = the number of set masks at the row; the row is kept iff c >= min_agree, so min_agree = 0 keeps
 *                 everything (plain task arithmetic); m = kept ? S : +0.
 *        apply    out = base + scaling * m (one product, one sum, each rounded; without base the product)
 *        streams  one per store task (mask_ptrs_dev [T]), in numpy.packbits order: stream bit i is bit 7 - (i & 7) of
 *                 byte i >> 3.  Row d of parameter p is stream bit bit_base[p] + d; bit_base_dev int64 [P] is the
 *                 caller's table of arbitrary non-negative bit offsets.  A stream is written in 32-bit words: it starts
 *                 on a 4-byte boundary and spans every word its bits touch (4 * ceil(bits / 32) bytes).  The caller
 *                 zeroes the streams before the first plan of the store; bits of rows the store does not cover stay 0.
 *                 Words wholly inside a block's bit range are stored, the partial first and last word of the range are
 *                 OR'ed in atomically: parameters, plans and work units may share words, in any order.
 *      By-products, uint64 words in state_dev (svdq_tall_work_bytes(T) bytes, zeroed by the caller, shared by all plans
 *      of the store): active [T] set bits per task | agree [T + 1] rows with c = 0 .. T.  Integer atomics, one flush per
 *      work unit.  No result depends on the order the units run in: two calls give identical bits.  Non-finite store
 *      values are outside the definition, as for TIES and DARE.
 *   out_ptrs_dev  NULL (masks only) or [P]; a NULL entry skips that parameter's output, never its mask bits or counts.
 *   mask_ptrs_dev NULL (merge only) or [T].
 *   slot_task_dev, task_map_dev, n_out, n_tasks, rows_dev, small_dev, basis_dev, mean_dev, base_ptrs_dev: as for
 *                 svdq_plan_ties_merge (live slots in ASCENDING store order: slot order is the order of the sum).
 *                 work_dev: svdq_task_reconstruct_work_bytes(plan, n_out) bytes.
 *   errors        SVDQ_EINVAL before anything is launched: a NULL plan, buffer or table (bit_base_dev and lambdas_dev
 *                 included); out_ptrs_dev and mask_ptrs_dev both NULL; n_out or n_tasks outside [1, SVDQ_MAX_TASKS];
 *                 min_agree outside [0, n_tasks]; a missing mean on a centred plan.
 *   Allocates nothing, copies nothing to the host, synchronises nothing.  Works on plans filled by any compress route and
 *   on plans filled by svdq_plan_import. */
int64_t svdq_tall_work_bytes(int32_t n_tasks);
int svdq_plan_tall_consensus(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev, const void *basis_dev,
                             const float *mean_dev, const int32_t *slot_task_dev /*[P][n_out]*/,
                             const int32_t *task_map_dev /*[P][n_out]*/, int32_t n_out, int32_t n_tasks,
                             const int64_t *bit_base_dev /*[P]*/, const float *lambdas_dev /*[T]*/, int32_t min_agree,
                             float scaling, const void *base_ptrs_dev /*NULL or [P]*/,
                             const void *out_ptrs_dev /*NULL or [P]*/,
                             const void *mask_ptrs_dev /*NULL or [T] uint32-aligned streams*/, void *state_dev,
                             void *work_dev, void *stream);

/* ---- the EMR merge of a store (Huang et al. 2024: "EMR-Merging: Tuning-Free High-Performance Model Merging"): Elect one
 *      task vector tau_uni, a 1-bit Mask per task and one Rescaler per task in ONE streaming pass over the basis
 *      (svdq_plan_emr_elect), and serve task t's model base + lambda_t * (M_t (.) tau_uni) in one streaming launch over
 *      the whole model (svdq_emr_apply).  No task model is written by the first; the second reads tau_uni, 1 bit per row
 *      and the base.  The definition follows the paper's equations; where the paper is silent the line says DECISION.
 *        inputs   T tasks in sorted-name order, store task index g = 0 .. T-1, as for svdq_plan_tall_consensus;
 *                 v_g[d] = the value svdq_task_reconstruct writes for task g at row d, bit for bit.  A task that lacks a
 *                 parameter contributes nothing on its rows and its mask bits there are 0.  Non-finite store values are
 *                 outside the definition, as for TIES, DARE and TALL.
 *        sum      S starts at +0; for the tasks that have the parameter, in ascending g: S = S + v_g, every sum rounded
 *                 in fp32 (the sum of svdq_plan_tall_consensus).
 *        elect    gamma = +1 if S > 0, -1 if S < 0, 0 if S == 0.  eps = the maximum of |v_g| over the tasks that have the
 *                 row and AGREE (v_g > 0 for gamma = +1, v_g < 0 for gamma = -1); eps = 0 with gamma = 0.  tau_uni = +0
 *                 when gamma = 0 (DECISION: a row whose values cancel exactly elects nothing), else copysign(eps, gamma).
 *                 A maximum is exact: tau_uni depends on no order.  fp32 addition is monotone, so S > 0 implies some
 *                 v_g > 0: eps > 0 whenever gamma != 0.
 *        mask     M_g[d] = the task has the row && v_g * gamma > 0 (the sign equals gamma and v_g != 0) -- the paper's
 *                 v_g (.) tau_uni > 0, since eps > 0 there.  A row with S == 0 is in no mask.
 *        rescale  over ALL rows of the store (every plan): A_g = sum |v_g[d]| over the rows the task has,
 *                 B_g = sum M_g[d] * eps[d]; every term a non-negative fp32 value converted to fp64 exactly, the sums
 *                 fp64.  lambda_g = A_g / B_g in fp64 (the caller's division); lambda_g = 1.0 when B_g == 0 (DECISION:
 *                 the mask then selects nothing that is non-zero, the value is immaterial).
 *        apply    out[d] = base[d] + lambda32 * (M_g[d] ? tau_uni[d] : +0), one product, one sum, each rounded in fp32;
 *                 without a base the product.  lambda32 is a float the CALLER passes (by default float32(lambda_g)).
 *        streams  one per store task (mask_ptrs_dev [T]), in exactly the layout of svdq_plan_tall_consensus: stream bit i
 *                 is bit 7 - (i & 7) of byte i >> 3; row d of parameter p is stream bit bit_base[p] + d; whole 32-bit
 *                 words are stored, the partial first and last word of a block's bit range are OR'ed in atomically; a
 *                 stream starts on a 4-byte boundary, spans 4 * ceil(bits / 32) bytes and is zeroed by the caller.
 *        sums     state_dev: double A [T] | double B [T] (svdq_emr_state_bytes(T) bytes, zeroed by the caller before the
 *                 first plan of the store, shared by all plans).  DETERMINISTIC, the sums included: no floating-point
 *                 atomics.  Every work unit adds its lanes' fp64 partials in a fixed order and STORES [2][T] doubles at
 *                 its own slot of a per-plan table in work_dev; a one-block kernel then adds the units in ascending
 *                 order -- as 1024 / 2T contiguous runs of units, the runs added in ascending order -- into state_dev.
 *                 Plans are added in call order on the one stream.  The same arguments give the same bits on every call.
 *   svdq_emr_state_bytes(T)                  [2][T] doubles, rounded up to 256 bytes; 0 for T outside [1, SVDQ_MAX_TASKS].
 *   svdq_emr_work_bytes(plan, n_out, T)      the coefficient scratch of svdq_task_reconstruct_work_bytes(plan, n_out)
 *                                            plus the per-unit table; 0 for a NULL plan or a count outside the range.
 *   svdq_plan_emr_elect   uni_ptrs_dev [P] fp32 outputs of rows[p] elements, the table required (a NULL entry skips that
 *                 parameter's tau_uni, never its mask bits or sums); mask_ptrs_dev [T] required.  One mode: there is no
 *                 mask-only or vector-only variant.  slot_task_dev, task_map_dev, n_out, n_tasks, rows_dev, small_dev,
 *                 basis_dev, mean_dev, bit_base_dev: as for svdq_plan_tall_consensus (live slots in ASCENDING store order).
 *   svdq_emr_apply        one task's model for the n_params parameters of the tables, in ONE launch: rows_dev int64 [P],
 *                 bit_base_dev int64 [P], uni_ptrs_dev [P] (what svdq_plan_emr_elect wrote), mask_stream_dev the task's
 *                 stream, base_ptrs_dev NULL or [P] with NULL entries allowed, out_ptrs_dev [P] fp32 outputs (a NULL
 *                 entry, or a NULL tau_uni, skips the parameter).  out may alias base.  16-byte loads and stores where a
 *                 parameter's pointers are 16-byte aligned, 4-byte ones otherwise.  n_params <= 7679 (the prefix table of
 *                 the rows lives in LDS).
 *   errors        SVDQ_EINVAL before anything is launched: a NULL plan, buffer or table; n_out or n_tasks outside
 *                 [1, SVDQ_MAX_TASKS]; a missing mean on a centred plan; n_params outside [1, 7679]; a non-finite lambda32.
 *   Allocate nothing, copy nothing to the host, synchronise nothing.  Work on plans filled by any compress route and on
 *   plans filled by svdq_plan_import. */
int64_t svdq_emr_state_bytes(int32_t n_tasks);
int64_t svdq_emr_work_bytes(const svdq_plan *plan, int32_t n_out, int32_t n_tasks);
int svdq_plan_emr_elect(const svdq_plan *plan, const int64_t *rows_dev, const void *small_dev, const void *basis_dev,
                        const float *mean_dev, const int32_t *slot_task_dev /*[P][n_out]*/,
                        const int32_t *task_map_dev /*[P][n_out]*/, int32_t n_out, int32_t n_tasks,
                        const int64_t *bit_base_dev /*[P]*/, const void *uni_ptrs_dev /*[P], required*/,
                        const void *mask_ptrs_dev /*[T] uint32-aligned streams, required*/, void *state_dev,
                        void *work_dev, void *stream);
int svdq_emr_apply(int32_t n_params, const int64_t *rows_dev /*[P]*/, const int64_t *bit_base_dev /*[P]*/,
                   const void *uni_ptrs_dev /*[P]*/, const void *mask_stream_dev, float lambda32,
                   const void *base_ptrs_dev /*NULL or [P]*/, const void *out_ptrs_dev /*[P]*/, void *stream);

/* ---- measurement aid (no reference counterpart; SURVEY.md section 8d asks for "a measured device-copy ceiling on
 *      the box" beside the 8 TB/s specification): plain streaming kernels with the access shape of the two passes.
 *      mode 0: read `bytes` from src_dev (dst_dev receives one float per 256 KiB read); mode 1: copy `bytes`;
 *      mode 2: read `bytes`, write 5/8 of that (pass 2's read : write mix at N = 8).  dst_dev must hold `bytes`. */
int svdq_hbm_probe(int32_t mode, const void *src_dev, void *dst_dev, int64_t bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SVDQ_H */
