// svdq_plan_extend.hip -- svdq_plan_residual_gram / svdq_plan_extend_basis: the stored basis of a plan grown by the
// directions NEW tasks add outside its span (contract: include/svdq.h).  No reference counterpart.
//
// Three launches, the host reading the column counts m between the second and the third.
//   k_plan_residual_gram   one wavefront per work unit of the plan; k_plan_project's walk (svdq_plan_project.hip): the
//                          block's U_high / U_low rows staged row-major in LDS, the rows of the present new-task slots
//                          loaded once, xc formed in registers and written to per-task LDS strips X[t][row].  Then the
//                          residual e = xc - U c is formed IN PLACE in the strips (pe_residual: one fp32 fma chain per
//                          element, lane l owns rows l, 64 + l, ... of the block) and E^T E goes to the matrix pipe:
//                          v_mfma_f32_16x16x4f32 with BOTH operands read from the strips (A[i][kk] = e[task i][row kk],
//                          B[kk][j] = e[task j][row kk], the K map of k_plan_project).  n_j = |xc_j|^2 beside it.  After
//                          each block the tile is added to fp64 accumulators; a unit leaves one fp64 partial.
//   k_plan_extend_eig      per parameter: the unit partials summed in a fixed order (reduce_partials), the fp64 Jacobi of
//                          svdq_eig.h on the present slots, the keep and sign rules, m / lambda / Z / d / norms.
//   k_plan_extend_write    the same walk and the same pe_residual again; q = E Z as an fp32 fma chain over the slots, and
//                          the rows of U_high' = [stored U_high bits | q rounded].
// At most SVDQ_MAX_NEW_TASKS = 8 new tasks per call, in task slots [0, n_new): the strips, the load registers and the
// tile are sized by that, the plan's slot count N only sizes the staged basis rows (r <= N).  No atomics: the same bits
// in every run.  Compiled with -ffp-contract=off (every fma here is written as one).

#include "svdq_coeff.h"
#include "svdq_dispatch.h"
#include "svdq_input.h"
#include "svdq_merge_stream.h"
#include "svdq_plan_rows.h"
#include "svdq_small_view.h"
#include "svdq_store_pass.h"

#define PE_MT SVDQ_MAX_NEW_TASKS
#define PE_NS 68      // stride (floats) of one task's 64 lane sums of xc^2

// dynamic LDS: the staged basis rows | X [8][XS] | C [32][8] coefficient image | [8][PE_NS] lane sums (write pass: Z [8][8])
__host__ __device__ constexpr size_t pe_lds_bytes(int rb, int n, int es) {
    return (size_t)stream_ubytes(rb, n, es) + (size_t)PE_MT * plan_strip_stride(rb) * 4 + 32 * PE_MT * 4 + PE_MT * PE_NS * 4;
}

// THE residual: e[m][s] <- fma(-u[rl[m]][i], C[i][t0 + s], e[m][s]) over the columns in order, U_high then U_low; e holds
// xc on entry.  Both passes call this one function on the same staged bytes, so both see the same bits.
template <typename T, int RPL>
__device__ __forceinline__ void pe_residual(float (&e)[RPL][4], const T *Uh, const T *Ul, const int (&rl)[RPL], int k,
                                            int nl, const float *C, int t0) {
    for (int i = 0; i < k; ++i) {
        const f32x4 c = *reinterpret_cast<const f32x4 *>(C + i * PE_MT + t0);
#pragma unroll
        for (int m = 0; m < RPL; ++m) {
            const float u = -u_val(Uh, rl[m] * k + i);
#pragma unroll
            for (int s = 0; s < 4; ++s) e[m][s] = fmaf(u, c[s], e[m][s]);
        }
    }
    for (int j = 0; j < nl; ++j) {
        const f32x4 c = *reinterpret_cast<const f32x4 *>(C + (k + j) * PE_MT + t0);
#pragma unroll
        for (int m = 0; m < RPL; ++m) {
            const float u = -u_val(Ul, rl[m] * nl + j);
#pragma unroll
            for (int s = 0; s < 4; ++s) e[m][s] = fmaf(u, c[s], e[m][s]);
        }
    }
}

__device__ __forceinline__ void pe_store_q(__half *dst, float q) { *dst = __float2half_rn(q); }
__device__ __forceinline__ void pe_store_q(float *dst, float q) { *dst = q; }

// One work unit of either pass.  NTP: the plan's slot-count instantiation (8, 16 or 32 >= N): it sizes the block (256
// rows up to 16 slots, 128 above) and the registers of the staged basis rows.  GATHER: rows through int32 index lists.
// FB: the task tensors are fine-tuned weights, base_ptrs names the base tensors.  WRITE: the third launch.
template <bool U16, typename TIN, int NTP, bool GATHER, bool FB, bool WRITE>
__device__ __forceinline__ void pe_unit(const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units,
                                        const void *const *__restrict__ ptrs, const void *const *__restrict__ base_ptrs,
                                        const int32_t *const *__restrict__ idx_ptrs, const int64_t *__restrict__ rows_dev,
                                        int NT, int n_new, const int32_t *__restrict__ k_in,
                                        const int32_t *__restrict__ r_in, const float *__restrict__ coef,
                                        const uint8_t *__restrict__ basis, const float *__restrict__ meanbuf,
                                        double *__restrict__ partH /* [n_units][64] */,
                                        double *__restrict__ partN /* [n_units][8] */,
                                        const int32_t *__restrict__ ext_m, const float *__restrict__ ext_z,
                                        void *const *__restrict__ out_ptrs) {
    using T = typename UElem<U16>::type;
    constexpr int ES = U16 ? 2 : 4;
    constexpr int RPL = store_rpl(NTP), RB = store_rb(NTP), XS = plan_strip_stride(RB), SV = store_sv(NTP, ES);
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int lane = threadIdx.x, n = NT, u = blockIdx.x;
    const int g = lane >> 4, col = lane & 15;
    uint8_t *Ubuf = lds_raw;
    float *X = reinterpret_cast<float *>(lds_raw + stream_ubytes(RB, n, ES));      // [PE_MT][XS]
    float *C = X + PE_MT * XS;                                                     // [32][PE_MT]
    float *NS = C + 32 * PE_MT;                                                    // [PE_MT][PE_NS] / Z [PE_MT][PE_MT]
    const SvdqUnit ud = units[u];
    const int p = ud.param;
    const SvdqParam pd = params[p];
    // the unit's rows and, below, its view of the plan and the block loop, written out: as store_unit / stream_blocks
    // (svdq_store_pass.h) this kernel spills more scalar registers
    const int64_t D = plan_rows_of(pd, rows_dev, p);
    int64_t cpos = ud.row0;
    int64_t cend = ud.row0 + ud.nrows;
    if (cend > D) cend = D;
    double accd[4] = {0.0, 0.0, 0.0, 0.0}, nacc = 0.0;
    int mm = 0;
    T *outp = nullptr;
    if constexpr (WRITE) {
        mm = ext_m[p];
        mm = mm < 0 ? 0 : (mm > PE_MT ? PE_MT : mm);
        outp = reinterpret_cast<T *>(out_ptrs[p]);
        if (mm == 0 || !outp) return;      // wave-uniform: nothing of p is written
    }
    if (cpos < cend) {      // wave-uniform
        int k, r;
        plan_ranks(k_in, r_in, p, D, n, k, r);
        const int nl = r - k;
        const uint8_t *gUh = basis + pd.slab_off;
        const uint8_t *gUl = SVDQ_SLAB_LOW(gUh, D, k, ES);
        mg_gfloat *gmean = meanbuf ? (mg_gfloat *)(meanbuf + pd.mean_off) : nullptr;
        gin<TIN> *dp[PE_MT];
#pragma unroll
        for (int t = 0; t < PE_MT; ++t) dp[t] = t < n_new ? (gin<TIN> *)ptrs[(size_t)p * n + t] : nullptr;
        gin<TIN> *bp = nullptr;
        if constexpr (FB) bp = (gin<TIN> *)base_ptrs[p];
        plan_gint *gidx = nullptr;
        if constexpr (GATHER) gidx = (plan_gint *)idx_ptrs[p];

        // ---- once per unit: the coefficient image C[column][slot] of the present slots (absent: 0), zero strips for
        // the absent slots (both MFMA operands read every strip), and in the write pass Z[slot][column]
        for (int e = lane; e < 32 * PE_MT; e += 64) {
            const int i = e / PE_MT, t = e % PE_MT;
            C[e] = (i < r && t < n_new && ptrs[(size_t)p * n + t]) ? coef[((size_t)p * n + t) * n + i] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < PE_MT; ++t)
            if (!dp[t])
                for (int e = lane; e < XS; e += 64) X[t * XS + e] = 0.f;
        if constexpr (WRITE) NS[lane] = ext_z[(size_t)p * PE_MT * PE_MT + lane];

        // ---- the loads of one block into registers; lane l owns rows c0 + RPL l .. + RPL - 1 (k_plan_project's)
        float xpf[PE_MT][RPL] = {}, mpf[RPL] = {}, bpf[RPL] = {};
        f32x4 ureg[SV];
        auto prefetch = [&](int64_t c0) {
            plan_rows_fetch<TIN, PE_MT, RPL, GATHER, FB>(xpf, mpf, bpf, dp, bp, gidx, gmean, c0, cend, lane);
            ustage_fetch(ureg, ustage_plan<ES>(c0, block_rows<RB>(c0, cend), k, nl), gUh, gUl, lane);
        };

        auto stage = [&](const UStage &cur, int) {
            ustage_commit(Ubuf, ureg, cur, lane);
            plan_rows_commit<PE_MT, RPL, FB, !WRITE>(X, xpf, mpf, bpf, dp, gmean != nullptr, lane, NS, PE_NS);
        };
        prefetch(cpos);
        while (true) {
            const int nr = block_rows<RB>(cpos, cend);
            const UStage cur = ustage_plan<ES>(cpos, nr, k, nl);
            stage(cur, nr);
            lds_fence();
            const bool more = cpos + RB < cend;
            if (more) prefetch(cpos + RB);
            // ---- e in place: lane l takes rows l, 64 + l, ... of the block (conflict-free reads of the row-major basis
            // image).  A row past the block's count was never staged: its basis row is clamped into the block and its e
            // forced to the exact zero its xc is (NaN * 0 is NaN).
            int rl[RPL];
            block_rows_of_lane(rl, nr, lane);
            const T *Uh = ustage_high<T>(Ubuf, cur), *Ul = ustage_low<T>(Ubuf, cur);
            for (int t0 = 0; t0 < n_new; t0 += 4) {      // wave-uniform
                float e[RPL][4];
#pragma unroll
                for (int m = 0; m < RPL; ++m)
#pragma unroll
                    for (int s = 0; s < 4; ++s) e[m][s] = X[(t0 + s) * XS + 64 * m + lane];
                pe_residual<T, RPL>(e, Uh, Ul, rl, k, nl, C, t0);
#pragma unroll
                for (int m = 0; m < RPL; ++m)
#pragma unroll
                    for (int s = 0; s < 4; ++s) X[(t0 + s) * XS + 64 * m + lane] = (64 * m + lane < nr) ? e[m][s] : 0.f;
            }
            lds_fence();

            if constexpr (!WRITE) {
                // n_j of the block: the 64 lane sums in lane order, fp32; fp64 across blocks
                if (lane < PE_MT) {
                    bool present = false;
#pragma unroll
                    for (int t = 0; t < PE_MT; ++t) present = (lane == t && dp[t]) ? true : present;
                    if (present) {
                        float s = 0.f;
                        for (int l = 0; l < 64; ++l) s = __fadd_rn(s, NS[lane * PE_NS + l]);
                        nacc += (double)s;
                    }
                }
                // E^T E over the block's rows, four per instruction; rows past the count are exact zeros in every strip
                const float *xo = X + (col & (PE_MT - 1)) * XS + 4 * g;
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
                const int nsteps = (nr + 15) >> 4;
                for (int s = 0; s < nsteps; ++s) {
                    const f32x4 xb = *reinterpret_cast<const f32x4 *>(xo + 16 * s);
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[v], xb[v], acc, 0, 0, 0);
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) accd[v] += (double)acc[v];
            } else {
                // q[d][c] = sum_j e_j[d] Z[j][c], an fp32 fma chain from 0 over the slots in order; the row of U_high'
                const int kw = k + mm;
#pragma unroll
                for (int m = 0; m < RPL; ++m) {
                    const int q = 64 * m + lane;
                    if (q < nr) {
                        T *row = outp + (cpos + q) * (int64_t)kw;
                        for (int i = 0; i < k; ++i) row[i] = Uh[q * k + i];
                        for (int c = 0; c < mm; ++c) {
                            float qv = 0.f;
                            for (int t = 0; t < n_new; ++t) qv = fmaf(X[t * XS + q], NS[t * PE_MT + c], qv);
                            pe_store_q(row + k + c, qv);
                        }
                    }
                }
            }
            if (!more) break;
            cpos += RB;
            lds_fence();      // the strips and the basis rows are rewritten next
        }
    }
    if constexpr (!WRITE) {
        // the unit's partial: result register v is H[4 g + v][col].  Absent slots leave zeros, so work_dev is the same
        // bytes in every run.
        if (col < PE_MT && g < 2) {
            const bool pj = col < n_new && ptrs[(size_t)p * n + col] != nullptr;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = 4 * g + v;
                const bool pi = i < n_new && ptrs[(size_t)p * n + i] != nullptr;
                partH[(size_t)u * 64 + i * PE_MT + col] = (pi && pj) ? accd[v] : 0.0;
            }
        }
        if (lane < PE_MT) partN[(size_t)u * PE_MT + lane] = nacc;
    }
}

template <bool U16, typename TIN, int NTP, bool GATHER, bool FB>
__global__ __launch_bounds__(64) void k_plan_residual_gram(
    const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units, const void *const *__restrict__ ptrs,
    const void *const *__restrict__ base_ptrs, const int32_t *const *__restrict__ idx_ptrs,
    const int64_t *__restrict__ rows_dev, int NT, int n_new, const int32_t *__restrict__ k_in,
    const int32_t *__restrict__ r_in, const float *__restrict__ coef, const uint8_t *__restrict__ basis,
    const float *__restrict__ meanbuf, double *__restrict__ partH, double *__restrict__ partN) {
    pe_unit<U16, TIN, NTP, GATHER, FB, false>(params, units, ptrs, base_ptrs, idx_ptrs, rows_dev, NT, n_new, k_in, r_in, coef,
                                              basis, meanbuf, partH, partN, nullptr, nullptr, nullptr);
}

template <bool U16, typename TIN, int NTP, bool GATHER, bool FB>
__global__ __launch_bounds__(64) void k_plan_extend_write(
    const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units, const void *const *__restrict__ ptrs,
    const void *const *__restrict__ base_ptrs, const int32_t *const *__restrict__ idx_ptrs,
    const int64_t *__restrict__ rows_dev, int NT, int n_new, const int32_t *__restrict__ k_in,
    const int32_t *__restrict__ r_in, const float *__restrict__ coef, const uint8_t *__restrict__ basis,
    const float *__restrict__ meanbuf, const int32_t *__restrict__ ext_m, const float *__restrict__ ext_z,
    void *const *__restrict__ out_ptrs) {
    pe_unit<U16, TIN, NTP, GATHER, FB, true>(params, units, ptrs, base_ptrs, idx_ptrs, rows_dev, NT, n_new, k_in, r_in, coef,
                                             basis, meanbuf, nullptr, nullptr, ext_m, ext_z, out_ptrs);
}

// Per parameter: H and n summed over the units, the eigen-decomposition over the present slots, the keep rule.
__global__ __launch_bounds__(EIG_THREADS) void k_plan_extend_eig(
    const SvdqParam *__restrict__ params, const void *const *__restrict__ ptrs, const int64_t *__restrict__ rows_dev,
    int NT, int n_new, const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
    const double *__restrict__ partH, const double *__restrict__ partN, double min_residual, int32_t *__restrict__ m_out,
    double *__restrict__ lam_out, float *__restrict__ z_out, float *__restrict__ d_out, double *__restrict__ xn_out,
    double *__restrict__ en_out) {
#pragma clang fp contract(off)
    constexpr int LDX = PE_MT + 1;
    __shared__ double red[4 * 1024];
    __shared__ double Hs[PE_MT * PE_MT], Ns[PE_MT];
    __shared__ double A[PE_MT * LDX], V[PE_MT * LDX], rowoff[PE_MT], rowdg[PE_MT], lam[PE_MT], sgn[PE_MT];
    __shared__ int order[PE_MT], slot[PE_MT], s_m;
    const int p = blockIdx.x, n = NT, tid = threadIdx.x;
    const SvdqParam pd = params[p];
    const int64_t D = plan_rows_of(pd, rows_dev, p);
    // every field of the entry is written, whatever follows: the same bytes in every run
    if (tid < PE_MT * PE_MT) {
        z_out[(size_t)p * 64 + tid] = 0.f;
        d_out[(size_t)p * 64 + tid] = 0.f;
    }
    if (tid < PE_MT) {
        lam_out[(size_t)p * PE_MT + tid] = 0.0;
        xn_out[(size_t)p * PE_MT + tid] = 0.0;
        en_out[(size_t)p * PE_MT + tid] = 0.0;
    }
    if (tid == 0) m_out[p] = 0;
    if (D <= 0) return;      // workgroup-uniform
    reduce_partials(partH, pd.unit_begin, pd.unit_begin + pd.unit_count, PE_MT * PE_MT, red, Hs);
    reduce_partials(partN, pd.unit_begin, pd.unit_begin + pd.unit_count, PE_MT, red, Ns);
    // the present slots, in slot order (every thread derives the same list)
    int np = 0;
    for (int t = 0; t < n_new && t < PE_MT; ++t)
        if (ptrs[(size_t)p * n + t]) {
            if (tid == 0) slot[np] = t;
            ++np;
        }
    __syncthreads();
    if (np == 0) return;      // workgroup-uniform
    if (tid < np) {
        xn_out[(size_t)p * PE_MT + slot[tid]] = Ns[slot[tid]];
        en_out[(size_t)p * PE_MT + slot[tid]] = Hs[slot[tid] * PE_MT + slot[tid]];
    }
    // non-finite data (include/svdq.h): the norms just written are the flag, nothing is decomposed and m stays 0
    bool finite = true;
    for (int j = 0; j < np; ++j) finite = finite && isfinite(Ns[slot[j]]) && isfinite(Hs[slot[j] * PE_MT + slot[j]]);
    if (!finite) return;      // workgroup-uniform
    if (tid < PE_MT * PE_MT) {
        const int a = tid / PE_MT, b = tid % PE_MT;
        if (a < np && b < np) {
            A[a * LDX + b] = 0.5 * (Hs[slot[a] * PE_MT + slot[b]] + Hs[slot[b] * PE_MT + slot[a]]);
            V[a * LDX + b] = (a == b) ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    jacobi_parallel<EIG_THREADS, PE_MT>(A, V, rowoff, rowdg, np, tid);
    __syncthreads();
    // sort descending (stable on ties); sign: the largest-magnitude component positive (the first of equals)
    if (tid < np) lam[tid] = A[tid * LDX + tid];
    __syncthreads();
    if (tid < np) {
        int rank = 0;
        for (int i = 0; i < np; ++i)
            if (lam[i] > lam[tid] || (lam[i] == lam[tid] && i < tid)) ++rank;
        order[rank] = tid;
    }
    __syncthreads();
    if (tid < np) {
        const int c = order[tid];
        double best = 0.0, bv = 1.0;
        for (int j = 0; j < np; ++j) {
            const double x = V[j * LDX + c];
            if (fabs(x) > best) {
                best = fabs(x);
                bv = x;
            }
        }
        sgn[tid] = bv < 0.0 ? -1.0 : 1.0;
    }
    if (tid == 0) {
        int k, r;
        plan_ranks(k_in, r_in, p, D, n, k, r);
        double nmax = 0.0;
        for (int j = 0; j < np; ++j) nmax = Ns[slot[j]] > nmax ? Ns[slot[j]] : nmax;
        const double thr = min_residual * min_residual * nmax;
        const int64_t room = D - r;
        const int cap = (int)(room < np ? room : np);
        int m = 0;
        while (m < cap && lam[order[m]] > thr) ++m;      // lambda is descending: the kept directions are a prefix
        s_m = m;
        m_out[p] = m;
    }
    __syncthreads();
    const int m = s_m;
    if (tid < np) lam_out[(size_t)p * PE_MT + tid] = lam[order[tid]];
    if (tid < PE_MT * PE_MT) {
        const int j = tid / PE_MT, c = tid % PE_MT;
        if (j < np && c < m) {
            const double l = lam[order[c]], w = sgn[c] * V[j * LDX + order[c]], s = sqrt(l);
            z_out[(size_t)p * 64 + slot[j] * PE_MT + c] = (float)(w / s);
            d_out[(size_t)p * 64 + slot[j] * PE_MT + c] = (float)(s * w);
        }
    }
}

static svdq_extend_layout pe_layout(int P) {
    svdq_extend_layout L;
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = off;
        off = svdq_align_up(off + bytes, 256);
        return at;
    };
    L.m_off = take((int64_t)P * 4);
    L.lambda_off = take((int64_t)P * PE_MT * 8);
    L.z_off = take((int64_t)P * PE_MT * PE_MT * 4);
    L.d_off = take((int64_t)P * PE_MT * PE_MT * 4);
    L.xnorm_off = take((int64_t)P * PE_MT * 8);
    L.enorm_off = take((int64_t)P * PE_MT * 8);
    L.total_bytes = off > 0 ? off : 256;
    return L;
}

static int64_t pe_parth_bytes(const svdq_plan *pl) { return svdq_align_up((int64_t)pl->n_units * PE_MT * PE_MT * 8, 256); }

extern "C" int64_t svdq_plan_residual_gram_work_bytes(const svdq_plan *pl) {
    if (!pl) return 0;
    return pe_parth_bytes(pl) + svdq_align_up((int64_t)pl->n_units * PE_MT * 8, 256);
}

extern "C" int svdq_plan_extend_layout(const svdq_plan *pl, svdq_extend_layout *out) {
    if (!pl || !out) {
        svdq_set_error("svdq_plan_extend_layout: the plan and out are required");
        return SVDQ_EINVAL;
    }
    *out = pe_layout(pl->n_params);
    return SVDQ_OK;
}

// what both entry points refuse before anything is launched
static int pe_check(const char *who, const svdq_plan *pl, const void *task_ptrs, const void *base_ptrs,
                    const void *index_ptrs, const int64_t *rows_dev, const void *basis, const float *mean,
                    const void *small, int32_t n_new, const void *ext, const void *other, const char *other_name) {
    if (!pl || !task_ptrs || !basis || !small || !ext || !other) {
        svdq_set_error("%s: the plan, task_ptrs, basis, small, ext and %s are required", who, other_name);
        return SVDQ_EINVAL;
    }
    if (svdq_refuse_no_mean(who, pl, mean)) return SVDQ_EINVAL;
    if (svdq_refuse_unaligned(who, svdq_addr_bits(task_ptrs, base_ptrs, index_ptrs, rows_dev, other), 8,
                              "pointer tables, rows and ", other_name))
        return SVDQ_EINVAL;
    if (svdq_refuse_unaligned(who, svdq_addr_bits(small, basis, mean, ext), 16, "small, basis, mean and ext"))
        return SVDQ_EINVAL;
    if (n_new < 1 || n_new > PE_MT || n_new > pl->n_tasks) {
        svdq_set_error("%s: n_new = %d new tasks, need 1 <= n_new <= min(%d, the plan's %d slots)", who, (int)n_new, PE_MT,
                       (int)pl->n_tasks);
        return SVDQ_EINVAL;
    }
    return SVDQ_OK;
}

// the streaming launch of either pass
template <bool WRITE, typename... Tail>
static bool pe_launch(const svdq_plan *pl, const void *task_ptrs, const void *base_ptrs, const void *index_ptrs,
                      const int64_t *rows_dev, const void *basis, const float *mean, const void *small, int n_new,
                      hipStream_t st, Tail... tail) {
    const SmallView sv = small_view(pl->small, small);
    auto tp = reinterpret_cast<const void *const *>(task_ptrs), bp = reinterpret_cast<const void *const *>(base_ptrs);
    auto ip = reinterpret_cast<const int32_t *const *>(index_ptrs);
    auto bs = reinterpret_cast<const uint8_t *>(basis);
    const float *mn = pl->cfg.center ? mean : nullptr;      // an uncentred plan subtracts nothing
    const int n = pl->n_tasks;
    return svdq_dispatch_input(pl->in_type, [&](auto tin_c) {
        using TIN = typename decltype(tin_c)::type;
        return svdq_dispatch_bool(pl->cfg.fp16 != 0, [&](auto f16_c) {
            constexpr bool U16 = f16_c;
            return svdq_dispatch_int<8, 16, 32>(svdq_slot_class(n), [&](auto ntp_c) {
                constexpr int NTP = ntp_c;
                return svdq_dispatch_bool(index_ptrs != nullptr, [&](auto gather_c) {
                    constexpr bool GATHER = gather_c;
                    return svdq_dispatch_bool(base_ptrs != nullptr, [&](auto fb_c) {
                        constexpr bool FB = fb_c;
                        const size_t lds = pe_lds_bytes(store_rb(NTP), n, U16 ? 2 : 4);
                        if constexpr (WRITE)
                            hipLaunchKernelGGL((k_plan_extend_write<U16, TIN, NTP, GATHER, FB>), dim3(pl->n_units), dim3(64),
                                               lds, st, pl->d_params, pl->d_units, tp, bp, ip, rows_dev, n, n_new, sv.k, sv.r,
                                               sv.coef, bs, mn, tail...);
                        else
                            hipLaunchKernelGGL((k_plan_residual_gram<U16, TIN, NTP, GATHER, FB>), dim3(pl->n_units), dim3(64),
                                               lds, st, pl->d_params, pl->d_units, tp, bp, ip, rows_dev, n, n_new, sv.k, sv.r,
                                               sv.coef, bs, mn, tail...);
                        return true;
                    });
                });
            });
        });
    });
}

extern "C" int svdq_plan_residual_gram(const svdq_plan *pl, const void *task_ptrs, const void *base_ptrs,
                                       const void *index_ptrs, const int64_t *rows_dev, const void *basis,
                                       const float *mean, const void *small, int32_t n_new, float min_residual, void *ext,
                                       void *work, void *stream) {
    const char *who = "svdq_plan_residual_gram";
    const int rc = pe_check(who, pl, task_ptrs, base_ptrs, index_ptrs, rows_dev, basis, mean, small, n_new, ext, work, "work");
    if (rc != SVDQ_OK) return rc;
    if (!(min_residual >= 0.f) || !(min_residual <= 3.0e38f)) {
        svdq_set_error("%s: min_residual must be finite and >= 0", who);
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    double *partH = reinterpret_cast<double *>(work);
    double *partN = reinterpret_cast<double *>(reinterpret_cast<uint8_t *>(work) + pe_parth_bytes(pl));
    if (pl->n_units > 0) {
        const bool ok = pe_launch<false>(pl, task_ptrs, base_ptrs, index_ptrs, rows_dev, basis, mean, small, n_new, st, partH,
                                         partN);
        if (!ok) return svdq_launch_status(false, "k_plan_residual_gram");
        if (hipGetLastError() != hipSuccess) return SVDQ_EHIP;
    }
    if (pl->n_params <= 0) return SVDQ_OK;
    const svdq_extend_layout E = pe_layout(pl->n_params);
    const SmallView sv = small_view(pl->small, small);
    uint8_t *ex = reinterpret_cast<uint8_t *>(ext);
    hipLaunchKernelGGL(k_plan_extend_eig, dim3(pl->n_params), dim3(EIG_THREADS), 0, st, pl->d_params,
                       reinterpret_cast<const void *const *>(task_ptrs), rows_dev, pl->n_tasks, (int)n_new,
                       sv.k, sv.r, partH, partN, (double)min_residual, reinterpret_cast<int32_t *>(ex + E.m_off),
                       reinterpret_cast<double *>(ex + E.lambda_off), reinterpret_cast<float *>(ex + E.z_off),
                       reinterpret_cast<float *>(ex + E.d_off), reinterpret_cast<double *>(ex + E.xnorm_off),
                       reinterpret_cast<double *>(ex + E.enorm_off));
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

extern "C" int svdq_plan_extend_basis(const svdq_plan *pl, const void *task_ptrs, const void *base_ptrs,
                                      const void *index_ptrs, const int64_t *rows_dev, const void *basis, const float *mean,
                                      const void *small, int32_t n_new, const void *ext, const void *out_ptrs, void *stream) {
    const char *who = "svdq_plan_extend_basis";
    const int rc = pe_check(who, pl, task_ptrs, base_ptrs, index_ptrs, rows_dev, basis, mean, small, n_new, ext, out_ptrs,
                            "out_ptrs");
    if (rc != SVDQ_OK) return rc;
    if (pl->n_units <= 0) return SVDQ_OK;
    const svdq_extend_layout E = pe_layout(pl->n_params);
    const uint8_t *ex = reinterpret_cast<const uint8_t *>(ext);
    const bool ok = pe_launch<true>(pl, task_ptrs, base_ptrs, index_ptrs, rows_dev, basis, mean, small, n_new,
                                    (hipStream_t)stream, reinterpret_cast<const int32_t *>(ex + E.m_off),
                                    reinterpret_cast<const float *>(ex + E.z_off),
                                    reinterpret_cast<void *const *>(out_ptrs));
    if (!ok) return svdq_launch_status(false, "k_plan_extend_write");
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}
