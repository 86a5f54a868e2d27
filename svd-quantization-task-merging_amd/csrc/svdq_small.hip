// svdq_small.hip -- the two latency-bound kernels between / after the streaming passes.
// Compiled with -ffp-contract=off: the quantizer must round scale*x and +zero_point separately.
//
//   k_eig    per parameter: deterministic fp64 reduction of the Gram partials, cyclic Jacobi
//            eigen-solve of the N x N Gram in fp64, sigma = sqrt(lambda), the reference's fp32
//            energy / rank rule (basis.py:116-156, 159-213, :367), W = V Sigma^-1.
//   k_coeff  per parameter: deterministic fp64 reduction of the projection partials,
//            c_high -> fp16 (compress.py:44-47), multi-stage affine quantization of c_low
//            (rtvq.py:4-82) -- one lane per task, n = r-k <= 31 scalars each.

#include "svdq_common.h"
#include "svdq_dispatch.h"
#include "svdq_coeff.h"
#include "svdq_small_view.h"

// First-level reduction, spread over the chip: chunk c of parameter p sums its share of the unit slots into
// part2[(p*SVDQ_RC + c)][nn]; k_eig / k_coeff then only add SVDQ_RC partials per parameter.  Keeps the whole reduction
// deterministic and off one CU.  Latency-bound (a chunk of a 4 M-row tensor is 128 slots of N x N doubles, each thread
// adds its entry of every slot): 256 threads = G groups of >= nn threads; group g takes slots a + g, a + g + G, ...
// with eight loads in flight per thread, the G group sums meet in LDS in group order.  Fixed order, so the same bits
// in every run and every batch; 4 dependent memory round trips per chunk where the 64-thread version had 16.
#define RED_THREADS 256
__global__ __launch_bounds__(RED_THREADS) void k_reduce(const SvdqParam *__restrict__ params, int NT, int pack,
                                                        const double *__restrict__ part, double *__restrict__ part2,
                                                        int param0, const int32_t *__restrict__ only) {
#pragma clang fp contract(off)
    __shared__ double red[RED_THREADS];
    const int p = param0 + blockIdx.x, c = blockIdx.y, nn = NT * NT;
    if (only && !only[p]) return;
    const SvdqParam pd = params[p];
    const int per = (pd.unit_count + SVDQ_RC - 1) / SVDQ_RC;  // units per chunk
    int ua = c * per, ub = ua + per;
    if (ub > pd.unit_count) ub = pd.unit_count;
    if (ua > ub) ua = ub;
    const int a = (pd.unit_begin + ua) * pack, b = (pd.unit_begin + ub) * pack;
    const int width = nn <= 64 ? 64 : (nn <= 128 ? 128 : RED_THREADS);   // threads per group
    const int G = RED_THREADS / width;
    const int g = threadIdx.x / width, l = threadIdx.x % width;
    double *dst = part2 + ((size_t)p * SVDQ_RC + c) * nn;
    for (int e0 = 0; e0 < nn; e0 += width) {      // one round unless nn > 256
        const int e = e0 + l;
        double acc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = 0.0;
        if (e < nn) {
            int s = a + g;
            for (; s + 7 * G < b; s += 8 * G) {
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] += part[(size_t)(s + u * G) * nn + e];
            }
            for (; s < b; s += G) acc[0] += part[(size_t)s * nn + e];
        }
        const double mine = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
        if (G == 1) {
            if (e < nn) dst[e] = mine;
        } else {
            red[threadIdx.x] = mine;
            __syncthreads();
            if (g == 0 && e < nn) {
                double t = red[l];
                for (int j = 1; j < G; ++j) t += red[j * width + l];
                dst[e] = t;
            }
            __syncthreads();
        }
    }
}

int svdq_launch_reduce(const svdq_plan *pl, const double *part, double *part2, int param0, int nparams,
                       const int32_t *only, hipStream_t st) {
    hipLaunchKernelGGL(k_reduce, dim3(nparams, SVDQ_RC), dim3(RED_THREADS), 0, st, pl->d_params, pl->n_tasks, pl->pack,
                       part, part2, param0, only);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

// Sum of the level-2 partials over all parameters and chunks, fixed order: 256 threads, thread j of an
// entry's group takes partials j, j+G, ... (chunk_sum order within), then a fixed tree over the group.
__global__ __launch_bounds__(256) void k_gram_total(int nparams, int nn, const double *__restrict__ part2,
                                                    double *__restrict__ out) {
    __shared__ double red[256];
    const int total = nparams * SVDQ_RC;
    for (int e0 = 0; e0 < nn; e0 += 16) {   // 16 entries x 16 partial-sums per pass
        const int e = e0 + (threadIdx.x & 15), j = threadIdx.x >> 4;
        const int per = (total + 15) / 16;
        int a = j * per, b = a + per;
        if (b > total) b = total;
        if (a > b) a = b;
        red[threadIdx.x] = e < nn ? chunk_sum(part2, a, b, nn, e) : 0.0;
        __syncthreads();
        for (int off = 128; off >= 16; off >>= 1) {
            if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x < 16 && e < nn) out[e] = red[threadIdx.x];
        __syncthreads();
    }
}

int svdq_launch_gram_total(const svdq_plan *pl, const double *part2, double *out, hipStream_t st) {
    hipLaunchKernelGGL(k_gram_total, dim3(1), dim3(256), 0, st, pl->n_params, pl->n_tasks * pl->n_tasks, part2, out);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

// ------------------------------------------------------------------------------------ task-Gram by-product
// The side sums of k_gram_side (a[0..N-1] = Tc^T m and s = m^T m, N + 1 doubles per unit) take the same two steps as the
// Gram partials.  k_reduce_side: chunk c of parameter p -> side2[(p * SVDQ_RC + c)][N + 1]; 256 threads = four groups
// of 64, group g takes units a + g, a + g + 4, ... with eight loads in flight, the group sums meet in LDS in group
// order.  Fixed order: the same bits in every run, and per parameter in every batch.
__global__ __launch_bounds__(RED_THREADS) void k_reduce_side(const SvdqParam *__restrict__ params, int NT,
                                                             const double *__restrict__ side,
                                                             double *__restrict__ side2) {
#pragma clang fp contract(off)
    __shared__ double red[RED_THREADS];
    const int p = blockIdx.x, c = blockIdx.y, ns = NT + 1;
    const SvdqParam pd = params[p];
    const int per = (pd.unit_count + SVDQ_RC - 1) / SVDQ_RC;  // units per chunk, as in k_reduce
    int ua = c * per, ub = ua + per;
    if (ub > pd.unit_count) ub = pd.unit_count;
    if (ua > ub) ua = ub;
    const int a = pd.unit_begin + ua, b = pd.unit_begin + ub;
    const int g = threadIdx.x >> 6, l = threadIdx.x & 63;
    double acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = 0.0;
    if (l < ns) {
        int s = a + g;
        for (; s + 28 < b; s += 32) {
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += side[(size_t)(s + 4 * u) * ns + l];
        }
        for (; s < b; s += 4) acc[0] += side[(size_t)s * ns + l];
    }
    red[threadIdx.x] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    __syncthreads();
    if (g == 0 && l < ns)
        side2[((size_t)p * SVDQ_RC + c) * ns + l] = (red[l] + red[64 + l]) + (red[128 + l] + red[192 + l]);
}

int svdq_launch_reduce_side(const svdq_plan *pl, const double *side, double *side2, hipStream_t st) {
    hipLaunchKernelGGL(k_reduce_side, dim3(pl->n_params, SVDQ_RC), dim3(RED_THREADS), 0, st, pl->d_params, pl->n_tasks,
                       side, side2);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

// k_gram_total plus the correction.  First the totals of a and s over all parameters and chunks: 256 threads =
// G = 256 / (N + 1) groups, thread (group j, entry e) takes partials j, j + G, ... (eight in flight), entry e's group
// sums are added in group order.  Then every Gram entry is totalled exactly as k_gram_total does and leaves as
// G[i][j] + ((a[i] + a[j]) + s): symmetric partials in, an exactly symmetric matrix out.
__global__ __launch_bounds__(256) void k_gram_total_side(int nparams, int NT, const double *__restrict__ part2,
                                                         const double *__restrict__ side2, double *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[256];
    __shared__ double tot[SVDQ_MAX_TASKS + 1];
    const int total = nparams * SVDQ_RC, nn = NT * NT, ns = NT + 1;
    {
        const int G = 256 / ns, j = threadIdx.x / ns, e = threadIdx.x % ns;
        double acc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = 0.0;
        if (j < G) {
            int s = j;
            for (; s + 7 * G < total; s += 8 * G) {
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] += side2[(size_t)(s + u * G) * ns + e];
            }
            for (; s < total; s += G) acc[0] += side2[(size_t)s * ns + e];
        }
        red[threadIdx.x] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
        __syncthreads();
        if (threadIdx.x < ns) {
            double t = red[threadIdx.x];
            for (int q = 1; q < G; ++q) t += red[q * ns + threadIdx.x];
            tot[threadIdx.x] = t;
        }
        __syncthreads();
    }
    for (int e0 = 0; e0 < nn; e0 += 16) {   // k_gram_total's order
        const int e = e0 + (threadIdx.x & 15), j = threadIdx.x >> 4;
        const int per = (total + 15) / 16;
        int a = j * per, b = a + per;
        if (b > total) b = total;
        if (a > b) a = b;
        red[threadIdx.x] = e < nn ? chunk_sum(part2, a, b, nn, e) : 0.0;
        __syncthreads();
        for (int off = 128; off >= 16; off >>= 1) {
            if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x < 16 && e < nn) out[e] = red[threadIdx.x] + ((tot[e / NT] + tot[e % NT]) + tot[NT]);
        __syncthreads();
    }
}

int svdq_launch_gram_total_side(const svdq_plan *pl, const double *part2, const double *side2, double *out,
                                hipStream_t st) {
    hipLaunchKernelGGL(k_gram_total_side, dim3(1), dim3(256), 0, st, pl->n_params, pl->n_tasks, part2, side2, out);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

template <int THREADS, int NMAX, typename TIN>
__global__ __launch_bounds__(THREADS) void k_eig(const SvdqParam *__restrict__ params,
                                                 const float *const *__restrict__ ptrs,
                                                 const int64_t *__restrict__ rows_dev, int NT, int center, float thr,
                                                 int max_rank, const double *__restrict__ gram_part2,
                                                 float *__restrict__ Wtab, double *__restrict__ c0_out, int param0,
                                                 float *__restrict__ sigma_out, int32_t *__restrict__ k_out,
                                                 int32_t *__restrict__ r_out, float *__restrict__ energy_out,
                                                 int64_t *__restrict__ rows_out,
                                                 const int32_t *const *__restrict__ idx_ptrs,
                                                 const float *const *__restrict__ base_ptrs,
                                                 const int32_t *__restrict__ only, int32_t *__restrict__ refine_out,
                                                 float resolve, const int64_t *__restrict__ ustart) {
    __shared__ __attribute__((aligned(16))) double lds[SVDQ_EIG_LDS_BYTES(NMAX) / 8 + 1];
    const int p = param0 + blockIdx.x;
    if (only && !only[p]) return;
    const int64_t D = rows_dev ? rows_dev[p] : params[p].rows;
    // source position of the parameter's first row: 0, the first entry of its index list (gather mode), or the start
    // of its first work unit (walk mode; bit 62 is the mask polarity)
    int64_t row0 = 0;
    if (D > 0) {
        if (idx_ptrs) row0 = idx_ptrs[p][0];
        else if (ustart) row0 = ustart[params[p].unit_begin] & ((1ll << 62) - 1);
    }
    eig_param<THREADS, NMAX, TIN>(lds, p, threadIdx.x, D, ptrs, NT, center, thr, max_rank, gram_part2, Wtab, c0_out, sigma_out,
                             k_out, r_out, energy_out, rows_out, row0, base_ptrs, refine_out, (double)resolve);
}

// ------------------------------------------------------------------------------------ epilogue
__global__ __launch_bounds__(EIG_THREADS) void k_coeff(const SvdqParam *__restrict__ params, int NT, int pack,
                                                       int bits, int stages, const double *__restrict__ cpart,
                                                       const double *__restrict__ c0_in,
                                                       const int32_t *__restrict__ k_in,
                                                       const int32_t *__restrict__ r_in,
                                                       float *__restrict__ coef_out, uint16_t *__restrict__ chigh_out,
                                                       uint8_t *__restrict__ codes_out, float *__restrict__ scale_out,
                                                       float *__restrict__ zp_out, float *__restrict__ rnorm_out, int param0,
                                                       const int32_t *__restrict__ bits_tab) {
    __shared__ double red[4 * 1024];
    __shared__ double C[1024];
    __shared__ float res[32 * LDN];

    const int p = param0 + blockIdx.x, tid = threadIdx.x, n = NT;
    const SvdqParam pd = params[p];
    if (bits_tab) bits = bits_tab[p];   // per-parameter code width (config #5's mixed 8-bit / 2-bit run)
    (void)pack;
    (void)pd;
    reduce_partials(cpart, p * SVDQ_RC, (p + 1) * SVDQ_RC, n * n, red, C);  // level-2 partials of k_reduce

    coeff_store_quantize(p, n, k_in[p], r_in[p], bits, stages, C, c0_in, nullptr, res, coef_out, chigh_out, codes_out,
                         scale_out, zp_out, rnorm_out);
}

// ------------------------------------------------------------------------------------ launchers
int svdq_launch_eig(const svdq_plan *pl, const SvdqInput &in, const double *gram_part2, float *W, double *c0,
                    uint8_t *small, int param0, int nparams, const int32_t *only, int32_t *refine_out, hipStream_t st) {
    // smallest sigma / sigma_0 the Gram behind gram_part2 resolves: exact-product (fp64 MFMA) sums reach the fp32
    // resolution of the data; fp32-product sums (SVDQ_SW_GRAM_F32, and N > 16 before its refinement) do not
    const bool exact = (pl->ntp <= 16 && !(pl->cfg.reserved & SVDQ_SW_GRAM_F32)) || only != nullptr;
    const float resolve = exact ? 1e-6f : 3e-4f;
    const SmallViewMut sv = small_view_mut(pl->small, small);
    // the input type only changes how k_eig reads row 0 of every task (the completion column)
    const bool ok = svdq_dispatch_input(pl->in_type, [&](auto tin_c) {
        using TIN = typename decltype(tin_c)::type;
        return svdq_dispatch_bool(pl->n_tasks <= 8, [&](auto small_c) {
            constexpr int THREADS = small_c ? 64 : 256, NMAX = small_c ? 8 : 32;
            hipLaunchKernelGGL((k_eig<THREADS, NMAX, TIN>), dim3(nparams), dim3(THREADS), 0, st, pl->d_params, in.tensors(),
                               in.rows_dev, pl->n_tasks, pl->cfg.center, pl->cfg.energy_threshold, pl->cfg.max_rank,
                               gram_part2, W, c0, param0, sv.sigma, sv.k, sv.r, sv.energy, sv.rows,
                               static_cast<const int32_t *const *>(in.index), static_cast<const float *const *>(in.base), only,
                               refine_out, resolve, in.ustart);
            return true;
        });
    });
    return svdq_launch_status(ok, "k_eig");
}

int svdq_launch_coeff(const svdq_plan *pl, const double *cpart, const double *c0, uint8_t *small, int param0,
                      int nparams, hipStream_t st) {
    const SmallViewMut sv = small_view_mut(pl->small, small);
    hipLaunchKernelGGL(k_coeff, dim3(nparams), dim3(EIG_THREADS), 0, st, pl->d_params, pl->n_tasks, pl->pack,
                       pl->cfg.low_bits, pl->cfg.rtvq_stages, cpart, c0, sv.k, sv.r, sv.coef, sv.chigh, sv.codes, sv.scale,
                       sv.zp, sv.rnorm, param0, pl->d_bits);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}
