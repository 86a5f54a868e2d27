// svdq_plan_project.hip -- svdq_plan_project: the projections of NEW task tensors onto the basis a plan already holds
// (contract: include/svdq.h).  Pass 2 of the compressor without pass 1: the basis, mean, k and r in the plan's buffers
// are only read -- they may come from any compress route or from svdq_plan_import -- and the coefficient epilogue is the
// fused route's own (svdq_coeff.h).  Replaces the per-(parameter, region, task) loop of compress_all_parameters
// (compress.py:173-207) -> compress_parameter (:114-170) -> compress_single_task (:24-56) -> project_to_basis (:6-21).
//
// Two launches.
//   k_plan_project         one wavefront per work unit of the plan.  A block of RB rows (256 up to 16 task slots, 128
//                          above): the block's U_high / U_low rows are staged row-major in LDS (svdq_merge_stream.h's
//                          staging), the rows of every PRESENT task slot are loaded once, x = finetuned - base and
//                          xc = x - mean are formed in registers (one fp32 subtraction each) and written to per-task
//                          LDS strips X[t][row].  The r x M products of a row go to the matrix pipe:
//                          v_mfma_f32_16x16x4f32 with A[i][kk] = U[row kk][column i], B[kk][j] = xc[task j][row kk];
//                          the contraction runs over the block's rows, four per instruction, so a block's sum is one
//                          fp32 accumulation chain of RB / 4 steps per (column, task) and the result tile holds
//                          c[task][column] directly.  After each block the tile is added to fp64 accumulators; a unit
//                          leaves one fp64 partial matrix [task][column] in work_dev.
//   k_plan_project_finish  per parameter: the unit partials summed in a fixed order (reduce_partials), then
//                          coeff_store_quantize for the present slots.
// No atomics: the same bits in every run.  Compiled with -ffp-contract=off (the quantizer's roundings).

#include "svdq_coeff.h"
#include "svdq_dispatch.h"
#include "svdq_input.h"
#include "svdq_merge_stream.h"
#include "svdq_plan_rows.h"
#include "svdq_small_view.h"
#include "svdq_store_pass.h"

// dynamic LDS: the staged basis rows | X [n][XS].  The launcher sizes it with bytes, the kernel carves it with the offset.
__host__ __device__ constexpr size_t pp_x_off(int rb, int n, int es) { return (size_t)stream_ubytes(rb, n, es); }
__host__ __device__ constexpr size_t pp_lds_bytes(int rb, int n, int es) {
    return pp_x_off(rb, n, es) + (size_t)n * plan_strip_stride(rb) * 4;
}

// NTP: the task slots the instantiation has registers for (8, 16 or 32 >= N): the prefetch registers of a block are
// NTP x RPL task values and the block's basis rows, and with them sized to the plan the kernel runs at three to four
// waves per SIMD up to 8 slots -- one wave per SIMD leaves the pass at a quarter of the read rate.
// TL = 16-slot tiles of the task (and column) dimension: 1 for N <= 16, 2 above.  GATHER: rows through int32 index lists.
// FB: the task tensors are fine-tuned weights, base_ptrs names the base tensors.
template <bool U16, typename TIN, int NTP, bool GATHER, bool FB>
__global__ __launch_bounds__(64) void k_plan_project(const SvdqParam *__restrict__ params,
                                                     const SvdqUnit *__restrict__ units,
                                                     const void *const *__restrict__ ptrs,
                                                     const void *const *__restrict__ base_ptrs,
                                                     const int32_t *const *__restrict__ idx_ptrs,
                                                     const int64_t *__restrict__ rows_dev, int NT,
                                                     const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                                     const uint8_t *__restrict__ basis, const float *__restrict__ meanbuf,
                                                     double *__restrict__ part /* [n_units][NT * NT] */) {
    using T = typename UElem<U16>::type;
    constexpr int ES = U16 ? 2 : 4;
    constexpr int TL = NTP > 16 ? 2 : 1;
    constexpr int RPL = store_rpl(NTP), RB = store_rb(NTP), XS = plan_strip_stride(RB), SV = store_sv(NTP, ES);
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int lane = threadIdx.x, n = NT, u = blockIdx.x;
    const int g = lane >> 4, col = lane & 15;
    uint8_t *Ubuf = lds_raw;
    float *X = reinterpret_cast<float *>(lds_raw + pp_x_off(RB, n, ES));      // [n][XS]
    const SvdqUnit ud = units[u];
    const int p = ud.param;
    const SvdqParam pd = params[p];
    const StoreUnit su = store_unit<ES>(pd, ud, p, plan_rows_of(pd, rows_dev, p), n, k_in, r_in, basis, meanbuf);
    const int64_t cend = su.cend;
    const int k = su.k, r = su.r, nl = su.nl;
    double accd[TL][TL][4];
#pragma unroll
    for (int ti = 0; ti < TL; ++ti)
#pragma unroll
        for (int tt = 0; tt < TL; ++tt)
#pragma unroll
            for (int v = 0; v < 4; ++v) accd[ti][tt][v] = 0.0;
    if (su.cpos < cend && r > 0) {      // wave-uniform
        const uint8_t *gUh = su.gUh, *gUl = su.gUl;
        mg_gfloat *gmean = su.gmean;
        gin<TIN> *dp[NTP];
#pragma unroll
        for (int t = 0; t < NTP; ++t) dp[t] = t < n ? (gin<TIN> *)ptrs[(size_t)p * n + t] : nullptr;
        gin<TIN> *bp = nullptr;
        if constexpr (FB) bp = (gin<TIN> *)base_ptrs[p];
        plan_gint *gidx = nullptr;
        if constexpr (GATHER) gidx = (plan_gint *)idx_ptrs[p];

        // ---- the loads of one block into registers; lane l owns rows c0 + RPL l .. + RPL - 1
        float xpf[NTP][RPL] = {}, mpf[RPL] = {}, bpf[RPL] = {};
        f32x4 ureg[SV];
        auto prefetch = [&](int64_t c0) {
            plan_rows_fetch<TIN, NTP, RPL, GATHER, FB>(xpf, mpf, bpf, dp, bp, gidx, gmean, c0, cend, lane);
            ustage_fetch(ureg, ustage_plan<ES>(c0, block_rows<RB>(c0, cend), k, nl), gUh, gUl, lane);
        };

        // ---- where the lane's A operand (basis column i = col + 16 ti, row 4 g of a 16-row step) sits in the staged image.
        // A column past r reads column 0 of a part that exists: a finite staged value whose result row is dropped.
        const int ntile_i = (r + 15) >> 4;
        auto compute = [&](const UStage &cur, int count, auto masked_c) {
            constexpr bool MASKED = decltype(masked_c)::value;
            int ua[TL], urow[TL];
#pragma unroll
            for (int ti = 0; ti < TL; ++ti) {
                int i = col + 16 * ti;
                if (i >= r) i = 0;
                // ustage_column's expression with the lane's row 4 g inside it, written out: through the shared function
                // the 32-slot fp32-input instantiations wait for the next block's loads inside the matrix loop (DESIGN.md
                // section 27)
                const bool hi = i < k;
                const int w = hi ? k : nl;
                urow[ti] = w * ES;
                ua[ti] = (hi ? cur.offh * ES : 16 * cur.nvh + cur.offl * ES) + (4 * g * w + (hi ? i : i - k)) * ES;
            }
            int xo[TL];
#pragma unroll
            for (int tt = 0; tt < TL; ++tt) {
                const int j = col + 16 * tt;
                xo[tt] = (j < n ? j : 0) * XS + 4 * g;
            }
            f32x4 acc[TL][TL];
#pragma unroll
            for (int ti = 0; ti < TL; ++ti)
#pragma unroll
                for (int tt = 0; tt < TL; ++tt) acc[ti][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int nsteps = (count + 15) >> 4;
            // two steps in flight: unrolled further (a full block's count is a constant) the LDS reads of all sixteen steps
            // are hoisted and hold 100 more vector registers, which costs the kernel half of its waves
#pragma unroll 2
            for (int s = 0; s < nsteps; ++s) {
                f32x4 xb[TL];
#pragma unroll
                for (int tt = 0; tt < TL; ++tt) xb[tt] = *reinterpret_cast<const f32x4 *>(X + xo[tt] + 16 * s);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    float a[TL];
#pragma unroll
                    for (int ti = 0; ti < TL; ++ti) {
                        a[ti] = 0.f;
                        if (ti < ntile_i) {      // wave-uniform
                            a[ti] = lds_u(Ubuf, ua[ti] + (16 * s + v) * urow[ti], T{});
                            // rows past the block's count were never staged: whatever sits there must not reach the
                            // matrix pipe (their x is an exact zero, but NaN * 0 is NaN)
                            if constexpr (MASKED) a[ti] = (16 * s + 4 * g + v < count) ? a[ti] : 0.f;
                        }
                    }
#pragma unroll
                    for (int ti = 0; ti < TL; ++ti)
                        if (ti < ntile_i) {
#pragma unroll
                            for (int tt = 0; tt < TL; ++tt)
                                acc[ti][tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ti], xb[tt][v], acc[ti][tt], 0, 0, 0);
                        }
                }
            }
#pragma unroll
            for (int ti = 0; ti < TL; ++ti)
#pragma unroll
                for (int tt = 0; tt < TL; ++tt)
#pragma unroll
                    for (int v = 0; v < 4; ++v) accd[ti][tt][v] += (double)acc[ti][tt][v];
        };

        stream_blocks<RB, ES>(
            su.cpos, cend, k, nl, prefetch,
            [&](const UStage &cur, int) {
                ustage_commit(Ubuf, ureg, cur, lane);
                plan_rows_commit<NTP, RPL, FB, false>(X, xpf, mpf, bpf, dp, gmean != nullptr, lane);
            },
            [&](const UStage &cur, int64_t, int nr, bool) {
                if (nr == RB) compute(cur, nr, std::false_type{});
                else compute(cur, nr, std::true_type{});
            });
    }
    // the unit's partial [task][column]: result register v of tile (ti, tt) is column 16 ti + 4 g + v of task 16 tt + col.
    // Columns past r and absent slots leave as zeros, so work_dev is the same bytes in every run.
    double *dst = part + (size_t)u * n * n;
#pragma unroll
    for (int tt = 0; tt < TL; ++tt) {
        const int t = col + 16 * tt;
        if (t >= n) continue;
        const bool present = ptrs[(size_t)p * n + t] != nullptr;
#pragma unroll
        for (int ti = 0; ti < TL; ++ti)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = 16 * ti + 4 * g + v;
                if (i < n) dst[(size_t)t * n + i] = (present && i < r) ? accd[ti][tt][v] : 0.0;
            }
    }
}

__global__ __launch_bounds__(EIG_THREADS) void k_plan_project_finish(
    const SvdqParam *__restrict__ params, const void *const *__restrict__ ptrs, const int64_t *__restrict__ rows_dev,
    int NT, int bits, int stages, const int32_t *__restrict__ bits_tab, const double *__restrict__ part,
    const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in, float *__restrict__ coef_out,
    uint16_t *__restrict__ chigh_out, uint8_t *__restrict__ codes_out, float *__restrict__ scale_out,
    float *__restrict__ zp_out, float *__restrict__ rnorm_out) {
    __shared__ double red[4 * 1024];
    __shared__ double C[1024];
    __shared__ float res[32 * LDN];
    const int p = blockIdx.x, n = NT;
    const SvdqParam pd = params[p];
    const int64_t D = plan_rows_of(pd, rows_dev, p);
    if (D <= 0) return;      // workgroup-uniform: nothing of p is written
    if (bits_tab) bits = bits_tab[p];
    reduce_partials(part, pd.unit_begin, pd.unit_begin + pd.unit_count, n * n, red, C);
    int k, r;
    plan_ranks(k_in, r_in, p, D, n, k, r);
    coeff_store_quantize(p, n, k, r, bits, stages, C, nullptr, ptrs + (size_t)p * n, res, coef_out, chigh_out, codes_out,
                         scale_out, zp_out, rnorm_out);
}

extern "C" int64_t svdq_plan_project_work_bytes(const svdq_plan *pl) {
    if (!pl) return 0;
    return svdq_align_up((int64_t)pl->n_units * pl->n_tasks * pl->n_tasks * 8, 256);
}

extern "C" int svdq_plan_project(const svdq_plan *pl, const void *task_ptrs, const void *base_ptrs, const void *index_ptrs,
                                 const int64_t *rows_dev, const void *basis, const float *mean, void *small, void *work,
                                 void *stream) {
    if (!pl || !task_ptrs || !basis || !small || !work) {
        svdq_set_error("svdq_plan_project: the plan, task_ptrs, basis, small and work are required");
        return SVDQ_EINVAL;
    }
    const char *who = "svdq_plan_project";
    if (svdq_refuse_no_mean(who, pl, mean)) return SVDQ_EINVAL;
    if (svdq_refuse_unaligned(who, svdq_addr_bits(task_ptrs, base_ptrs, index_ptrs, rows_dev, work), 8,
                              "pointer tables, rows and work"))
        return SVDQ_EINVAL;
    if (svdq_refuse_unaligned(who, svdq_addr_bits(small, basis, mean), 16, "small, basis and mean")) return SVDQ_EINVAL;
    const SmallViewMut sv = small_view_mut(pl->small, small);
    auto tp = reinterpret_cast<const void *const *>(task_ptrs), bp = reinterpret_cast<const void *const *>(base_ptrs);
    auto ip = reinterpret_cast<const int32_t *const *>(index_ptrs);
    auto bs = reinterpret_cast<const uint8_t *>(basis);
    const float *mn = pl->cfg.center ? mean : nullptr;      // an uncentred plan subtracts nothing
    double *part = reinterpret_cast<double *>(work);
    hipStream_t st = (hipStream_t)stream;
    const int n = pl->n_tasks;
    const bool ok = svdq_dispatch_input(pl->in_type, [&](auto tin_c) {
        using TIN = typename decltype(tin_c)::type;
        return svdq_dispatch_bool(pl->cfg.fp16 != 0, [&](auto f16_c) {
            constexpr bool U16 = f16_c;
            return svdq_dispatch_int<8, 16, 32>(svdq_slot_class(n), [&](auto ntp_c) {
                constexpr int NTP = ntp_c;
                return svdq_dispatch_bool(index_ptrs != nullptr, [&](auto gather_c) {
                    constexpr bool GATHER = gather_c;
                    return svdq_dispatch_bool(base_ptrs != nullptr, [&](auto fb_c) {
                        constexpr bool FB = fb_c;
                        const size_t lds = pp_lds_bytes(store_rb(NTP), n, U16 ? 2 : 4);
                        hipLaunchKernelGGL((k_plan_project<U16, TIN, NTP, GATHER, FB>), dim3(pl->n_units), dim3(64), lds, st,
                                           pl->d_params, pl->d_units, tp, bp, ip, rows_dev, n, sv.k, sv.r, bs, mn, part);
                        return true;
                    });
                });
            });
        });
    });
    if (!ok) return svdq_launch_status(false, "k_plan_project");
    if (hipGetLastError() != hipSuccess) return SVDQ_EHIP;
    hipLaunchKernelGGL(k_plan_project_finish, dim3(pl->n_params), dim3(EIG_THREADS), 0, st, pl->d_params, tp, rows_dev, n,
                       pl->cfg.low_bits, pl->cfg.rtvq_stages, pl->d_bits, part, sv.k, sv.r, sv.coef, sv.chigh, sv.codes,
                       sv.scale, sv.zp, sv.rnorm);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}
