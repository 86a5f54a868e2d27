// svdq_store_gram.hip -- svdq_plan_store_gram: the N x N Gram of the task vectors a plan's STORED artifacts reconstruct
// (contract: include/svdq.h).  What flatten_task_vectors + cluster_tasks (clustering.py:55-120, :198-245) need of a
// store, without the fine-tuned checkpoints and without writing one reconstructed model: with A = [U_high | U_low | mean]
// and c'_t = [c_t ; 1], delta_t = A c'_t and G[t][s] = c'_t^T (A^T A) c'_s.  One pass over the basis and the mean forms
// A^T A, the rest is (r + 1)^2 numbers per parameter.
//
// Two launches.
//   k_store_gram         one wavefront per work unit of the plan, the geometry of k_plan_project and the merge
//                        consumers: a block of RB rows (256 up to 16 task slots, 128 above) of U_high / U_low is staged
//                        row-major in LDS (svdq_merge_stream.h's staging) and is BOTH operands of U^T U on the matrix pipe --
//                        the lane that holds column i of the block's rows as the A operand holds column i as the B operand,
//                        so a diagonal tile is one register set used twice.  fp16 basis: v_mfma_f32_16x16x32_f16, 32 rows
//                        per instruction (fp16 x fp16 products are exact in fp32); fp32 basis: v_mfma_f32_16x16x4_f32.
//                        The mean column (fp32, absent on an uncentred plan) is formed on the vector ALU: each lane owns
//                        RPL rows of the block, u^T m and m^T m are fp32 fma chains over them, each row of 16 lanes sums
//                        its values with four DPP steps (still one block's fp32 sum) and adds them to fp64 totals; the
//                        four rows of lanes meet once per unit.
//                        After each block the result tiles are added to fp64 accumulators; a unit leaves one fp64 partial
//                        [N][N] (both triangles, zeros past r) and one [N + 1] (U^T m, then m^T m) in work_dev.
//   k_store_gram_finish  per parameter: the unit partials summed in a fixed order (reduce_partials), every task slot's
//                        coefficients through task_coeff (the merge's dequantizing lines), G = C' (A^T A) C'^T in fp64,
//                        formed for t <= s and mirrored: exactly symmetric.
// No atomics: the same bits in every run.  Nothing of the plan, the small buffer, the basis or the mean is written.

#include "svdq_coeff.h"
#include "svdq_dispatch.h"
#include "svdq_merge_stream.h"
#include "svdq_small_view.h"
#include "svdq_store_pass.h"

typedef _Float16 sg_f16x8 __attribute__((ext_vector_type(8)));

#define SG_BG 33      // rows / columns of one parameter's basis_gram_dev matrix: r <= 32 columns and the mean

// The lane's operand of one MFMA step: column `off`/`stride` (ustage_column) of the rows the instruction's k index gives the
// lane.  fp16: 8 rows 32 s + 8 g + j (v_mfma_f32_16x16x32_f16; the same register set serves as A and B, so any k
// assignment is consistent as long as both operands use it); fp32: row 4 s + g.  Rows past `count` were never staged:
// whatever sits there must not reach the matrix pipe.
template <bool MASKED>
__device__ __forceinline__ sg_f16x8 sg_operand(const uint8_t *lds, int off, int stride, int s, int g, int count, __half) {
    sg_f16x8 a;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int row = 32 * s + 8 * g + j;
        _Float16 v = *reinterpret_cast<const _Float16 *>(lds + off + row * stride);
        if constexpr (MASKED) v = row < count ? v : (_Float16)0.f;
        a[j] = v;
    }
    return a;
}
template <bool MASKED>
__device__ __forceinline__ float sg_operand(const uint8_t *lds, int off, int stride, int s, int g, int count, float) {
    const int row = 4 * s + g;
    float v = *reinterpret_cast<const float *>(lds + off + row * stride);
    if constexpr (MASKED) v = row < count ? v : 0.f;
    return v;
}
__device__ __forceinline__ f32x4 sg_mfma(const sg_f16x8 &a, const sg_f16x8 &b, const f32x4 &c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 sg_mfma(float a, float b, const f32x4 &c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// the sum of the 16 lanes of the lane's row (lanes 16 g .. 16 g + 15), in each of them: four DPP steps on the vector ALU
// (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror); every step adds the same two numbers in both
// partners, so the 16 lanes end with the same bits
template <int CTRL> __device__ __forceinline__ float sg_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float sg_row_sum(float v) {
    v = __fadd_rn(v, sg_dpp<0xB1>(v));
    v = __fadd_rn(v, sg_dpp<0x4E>(v));
    v = __fadd_rn(v, sg_dpp<0x141>(v));
    v = __fadd_rn(v, sg_dpp<0x140>(v));
    return v;
}
// the sum over the four rows of lanes, once per unit
__device__ __forceinline__ double sg_rows_sum(double v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// CMAX: the basis columns the instantiation has registers for (8, 16 or 32 >= N >= r).  TL = 16-column tiles: 1 up to 16
// columns, 2 above; of the TL x TL result tiles only those with ti <= tj are computed.
template <bool U16, int CMAX>
__global__ __launch_bounds__(64) void k_store_gram(const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units,
                                                   const int64_t *__restrict__ rows_dev, int NT,
                                                   const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                                   const uint8_t *__restrict__ basis, const float *__restrict__ meanbuf,
                                                   double *__restrict__ partU /* [n_units][NT * NT] */,
                                                   double *__restrict__ partM /* [n_units][NT + 1] */) {
    using T = typename UElem<U16>::type;
    constexpr int ES = U16 ? 2 : 4;
    constexpr int TL = CMAX > 16 ? 2 : 1;
    constexpr int RPL = store_rpl(CMAX), RB = store_rb(CMAX), SV = store_sv(CMAX, ES);
    constexpr int KS = U16 ? 32 : 4;      // rows one MFMA contracts
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int lane = threadIdx.x, n = NT, u = blockIdx.x;
    const int g = lane >> 4, col = lane & 15;
    uint8_t *Ubuf = lds_raw;      // sg_lds_bytes: the staged basis rows and nothing else
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
        for (int tj = 0; tj < TL; ++tj)
#pragma unroll
            for (int v = 0; v < 4; ++v) accd[ti][tj][v] = 0.0;
    double dm0 = 0.0, dm1 = 0.0, dmm = 0.0;      // lane (g, c): columns c and 16 + c of U^T m, and m^T m, of row g's rows
    mg_gfloat *gmean = su.gmean;
    if (su.cpos < cend && (r > 0 || gmean)) {      // wave-uniform
        const uint8_t *gUh = su.gUh, *gUl = su.gUl;

        // ---- the loads of one block into registers; lane l owns rows l, 64 + l, ... of the block for the mean column
        float mpf[RPL] = {}, bpf[RPL] = {}, mcur[RPL] = {};
        f32x4 ureg[SV];
        auto prefetch = [&](int64_t c0) {
            const int nr = block_rows<RB>(c0, cend);
            load_rows<RPL>(mpf, bpf, gmean, (mg_gfloat *)nullptr, c0, nr, lane);
            ustage_fetch(ureg, ustage_plan<ES>(c0, nr, k, nl), gUh, gUl, lane);
        };

        const int ntile = (r + 15) >> 4;
        auto compute = [&](const UStage &cur, int count, auto masked_c) {
            constexpr bool MASKED = decltype(masked_c)::value;
            // ---- U^T U on the matrix pipe.  A column past r reads column 0 of a part that exists: a finite staged value
            // whose result rows and columns are dropped.
            if (r > 0) {
                int uo[TL], us[TL];
#pragma unroll
                for (int ti = 0; ti < TL; ++ti) {
                    int i = col + 16 * ti;
                    if (i >= r) i = 0;
                    ustage_column(cur, i, k, nl, ES, uo[ti], us[ti]);
                }
                f32x4 acc[TL][TL];
#pragma unroll
                for (int ti = 0; ti < TL; ++ti)
#pragma unroll
                    for (int tj = 0; tj < TL; ++tj) acc[ti][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
                const int nsteps = (count + KS - 1) / KS;
#pragma unroll 2
                for (int s = 0; s < nsteps; ++s) {
                    decltype(sg_operand<MASKED>(Ubuf, 0, 0, 0, 0, 0, T{})) a[TL];
#pragma unroll
                    for (int ti = 0; ti < TL; ++ti)
                        if (ti < ntile) a[ti] = sg_operand<MASKED>(Ubuf, uo[ti], us[ti], s, g, count, T{});
#pragma unroll
                    for (int ti = 0; ti < TL; ++ti)
#pragma unroll
                        for (int tj = ti; tj < TL; ++tj)
                            if (tj < ntile) acc[ti][tj] = sg_mfma(a[ti], a[tj], acc[ti][tj]);
                }
#pragma unroll
                for (int ti = 0; ti < TL; ++ti)
#pragma unroll
                    for (int tj = ti; tj < TL; ++tj)
#pragma unroll
                        for (int v = 0; v < 4; ++v) accd[ti][tj][v] += (double)acc[ti][tj][v];
            }
            // ---- the mean column on the vector ALU: fp32 fma chains over the lane's rows of the block, then the sum of each
            // row of 16 lanes (64 rows of the block: still an fp32 sum inside one block); lane (g, c) keeps the fp64
            // total of column c (dm0) and 16 + c (dm1) over the rows its row of lanes owns, every lane that of m^T m
            if (gmean) {
                int rl[RPL];
                float mv[RPL];
#pragma unroll
                for (int m = 0; m < RPL; ++m) {
                    const int q = 64 * m + lane;
                    rl[m] = q < count ? q : 0;
                    mv[m] = q < count ? mcur[m] : 0.f;      // a row past the block's end adds u * 0 of a staged row
                }
                float mm = 0.f;
#pragma unroll
                for (int m = 0; m < RPL; ++m) mm = fmaf(mv[m], mv[m], mm);
                dmm += (double)sg_row_sum(mm);
#pragma unroll 4
                for (int c = 0; c < r; ++c) {
                    int off, stride;
                    ustage_column(cur, c, k, nl, ES, off, stride);
                    float um = 0.f;
#pragma unroll
                    for (int m = 0; m < RPL; ++m) um = fmaf(lds_u(Ubuf, off + rl[m] * stride, T{}), mv[m], um);
                    um = sg_row_sum(um);
                    if (col == (c & 15)) {
                        if (CMAX <= 16 || c < 16) dm0 += (double)um;
                        else dm1 += (double)um;
                    }
                }
            }
        };

        // the block loop written out: as stream_blocks (svdq_store_pass.h) <fp16, 32> measured 2 % slower (DESIGN.md
        // section 27)
        int64_t cpos = su.cpos;
        prefetch(cpos);
        while (true) {
            const int nr = block_rows<RB>(cpos, cend);
            const UStage cur = ustage_plan<ES>(cpos, nr, k, nl);
            ustage_commit(Ubuf, ureg, cur, lane);
#pragma unroll
            for (int m = 0; m < RPL; ++m) mcur[m] = mpf[m];      // out of the way of the next block's loads
            lds_fence();
            const bool more = cpos + RB < cend;
            if (more) prefetch(cpos + RB);
            if (nr == RB) compute(cur, nr, std::false_type{});
            else compute(cur, nr, std::true_type{});
            if (!more) break;
            cpos += RB;
            lds_fence();      // the basis rows are rewritten next
        }
    }
    // ---- the unit's partials.  Result register v of tile (ti, tj) is entry (16 ti + 4 g + v, 16 tj + col); an off-diagonal
    // tile also fills its mirror image.  Rows and columns past r leave as zeros: work_dev is the same bytes in every run.
    double *dst = partU + (size_t)u * n * n;
#pragma unroll
    for (int ti = 0; ti < TL; ++ti)
#pragma unroll
        for (int tj = ti; tj < TL; ++tj) {
            const int j = col + 16 * tj;
            if (j >= n) continue;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = 16 * ti + 4 * g + v;
                if (i >= n) continue;
                const double val = (i < r && j < r) ? accd[ti][tj][v] : 0.0;
                dst[(size_t)i * n + j] = val;
                if (ti != tj) dst[(size_t)j * n + i] = val;
            }
        }
    // the mean column: the four rows of lanes meet (the same association in every run); zeros on an uncentred plan
    dm0 = sg_rows_sum(dm0);
    dmm = sg_rows_sum(dmm);
    double *dstm = partM + (size_t)u * (n + 1);
    if (lane < 16 && lane < n) dstm[lane] = lane < r ? dm0 : 0.0;
    if constexpr (CMAX > 16) {
        dm1 = sg_rows_sum(dm1);
        if (lane < 16 && 16 + lane < n) dstm[16 + lane] = 16 + lane < r ? dm1 : 0.0;
    }
    if (lane == 0) dstm[n] = dmm;
}

__global__ __launch_bounds__(EIG_THREADS) void k_store_gram_finish(
    const SvdqParam *__restrict__ params, const int64_t *__restrict__ rows_dev, int NT, int stages, int centred,
    const double *__restrict__ partU, const double *__restrict__ partM, const int32_t *__restrict__ k_in,
    const int32_t *__restrict__ r_in, const uint16_t *__restrict__ chigh, const uint8_t *__restrict__ codes,
    const float *__restrict__ scale, const float *__restrict__ zp, double *__restrict__ task_gram /* [P][NT][NT] */,
    double *__restrict__ basis_gram /* NULL or [P][33][33] */) {
    __shared__ double red[4 * 1024];
    __shared__ double S[1024], Mv[SG_BG];
    __shared__ double Cc[32 * SG_BG], Tm[SG_BG * 32];
    const int p = blockIdx.x, n = NT, tid = threadIdx.x;
    const SvdqParam pd = params[p];
    const int64_t D = plan_rows_of(pd, rows_dev, p);
    double *G = task_gram + (size_t)p * n * n;
    double *B = basis_gram ? basis_gram + (size_t)p * SG_BG * SG_BG : nullptr;
    if (D <= 0) {      // workgroup-uniform: nothing of p is read, zeros are written
        for (int e = tid; e < n * n; e += EIG_THREADS) G[e] = 0.0;
        if (B)
            for (int e = tid; e < SG_BG * SG_BG; e += EIG_THREADS) B[e] = 0.0;
        return;
    }
    reduce_partials(partU, pd.unit_begin, pd.unit_begin + pd.unit_count, n * n, red, S);
    reduce_partials(partM, pd.unit_begin, pd.unit_begin + pd.unit_count, n + 1, red, Mv);
    int k, r;
    plan_ranks(k_in, r_in, p, D, n, k, r);
    const int ra = r + (centred ? 1 : 0);      // columns of A = [U | mean]
    // A^T A, read from the upper triangle of the totals: entry (a, b) and (b, a) are one number
    auto ata = [&](int a, int b) -> double {
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        if (b < r) return S[a * n + b];
        return a < r ? Mv[a] : Mv[n];
    };
    if (B)
        for (int e = tid; e < SG_BG * SG_BG; e += EIG_THREADS) {
            const int a = e / SG_BG, b = e % SG_BG;
            B[e] = (a < ra && b < ra) ? ata(a, b) : 0.0;
        }
    // C'[t] = [c_t ; 1]: the merge's own dequantizing lines
    for (int e = tid; e < n * SG_BG; e += EIG_THREADS) {
        const int t = e / SG_BG, i = e % SG_BG;
        double c = 0.0;
        if (i < r) c = (double)task_coeff(p, t, i, n, k, stages, chigh, codes, scale, zp);
        else if (i == r && centred) c = 1.0;
        Cc[e] = c;
    }
    __syncthreads();
    // Tm[a][s] = sum_b (A^T A)[a][b] C'[s][b]
    for (int e = tid; e < ra * n; e += EIG_THREADS) {
        const int a = e / n, s = e % n;
        double acc = 0.0;
        for (int b = 0; b < ra; ++b) acc += ata(a, b) * Cc[s * SG_BG + b];
        Tm[a * 32 + s] = acc;
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += EIG_THREADS) {
        const int t = e / n, s = e % n;
        if (t > s) continue;
        double acc = 0.0;
        for (int a = 0; a < ra; ++a) acc += Cc[t * SG_BG + a] * Tm[a * 32 + s];
        G[(size_t)t * n + s] = acc;
        G[(size_t)s * n + t] = acc;
    }
}

// dynamic LDS of k_store_gram
__host__ __device__ constexpr size_t sg_lds_bytes(int rb, int n, int es) { return (size_t)stream_ubytes(rb, n, es); }

extern "C" int64_t svdq_plan_store_gram_work_bytes(const svdq_plan *pl) {
    if (!pl) return 0;
    return svdq_align_up((int64_t)pl->n_units * ((int64_t)pl->n_tasks * pl->n_tasks + pl->n_tasks + 1) * 8, 256);
}

extern "C" int svdq_plan_store_gram(const svdq_plan *pl, const int64_t *rows_dev, const void *small, const void *basis,
                                    const float *mean, void *work, double *task_gram, double *basis_gram, void *stream) {
    if (!pl || !small || !basis || !work || !task_gram) {
        svdq_set_error("svdq_plan_store_gram: the plan, small, basis, work and task_gram are required");
        return SVDQ_EINVAL;
    }
    const char *who = "svdq_plan_store_gram";
    if (svdq_refuse_no_mean(who, pl, mean)) return SVDQ_EINVAL;
    if (svdq_refuse_unaligned(who, svdq_addr_bits(rows_dev, work, task_gram, basis_gram), 8, "rows, work and the outputs"))
        return SVDQ_EINVAL;
    if (svdq_refuse_unaligned(who, svdq_addr_bits(small, basis, mean), 16, "small, basis and mean")) return SVDQ_EINVAL;
    const SmallView sv = small_view(pl->small, small);
    auto bs = reinterpret_cast<const uint8_t *>(basis);
    const float *mn = pl->cfg.center ? mean : nullptr;      // an uncentred plan has A = U
    const int n = pl->n_tasks;
    double *partU = reinterpret_cast<double *>(work);
    double *partM = partU + (size_t)pl->n_units * n * n;
    hipStream_t st = (hipStream_t)stream;
    const bool ok = svdq_dispatch_bool(pl->cfg.fp16 != 0, [&](auto f16_c) {
        constexpr bool U16 = f16_c;
        return svdq_dispatch_int<8, 16, 32>(svdq_slot_class(n), [&](auto cmax_c) {
            constexpr int CMAX = cmax_c;
            const size_t lds = sg_lds_bytes(store_rb(CMAX), n, U16 ? 2 : 4);
            hipLaunchKernelGGL((k_store_gram<U16, CMAX>), dim3(pl->n_units), dim3(64), lds, st, pl->d_params, pl->d_units,
                               rows_dev, n, sv.k, sv.r, bs, mn, partU, partM);
            return true;
        });
    });
    if (!ok) return svdq_launch_status(false, "k_store_gram");
    if (hipGetLastError() != hipSuccess) return SVDQ_EHIP;
    hipLaunchKernelGGL(k_store_gram_finish, dim3(pl->n_params), dim3(EIG_THREADS), 0, st, pl->d_params, rows_dev, n,
                       pl->cfg.rtvq_stages, pl->cfg.center != 0, partU, partM, sv.k, sv.r, sv.chigh, sv.codes, sv.scale,
                       sv.zp, task_gram, basis_gram);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}
