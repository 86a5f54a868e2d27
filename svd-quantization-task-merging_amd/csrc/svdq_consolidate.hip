// svdq_consolidate.hip -- svdq_plan_consolidate_eig / svdq_plan_rebase: a plan's STORED artifacts brought back to the form
// a fresh compress run of the tasks they reconstruct would give them (contract: include/svdq.h).  No reference
// counterpart.  Per entry delta_t = A c'_t with A = [U_high | U_low | mean] and c'_t = [c_t ; 1], so the SVD of the kept
// tasks is an N' x N' problem on K = Bc^T (A^T A) Bc plus one linear map of the stored rows, U' = A W.
//
// Two launches here, behind svdq_plan_store_gram's (which leaves A^T A in basis_gram_dev):
//   k_plan_consolidate_eig   one workgroup per entry: the kept slots' coefficients through task_coeff (the merge's
//                            dequantizing lines), bbar, Bc, K and eta in fp64, the fp64 Jacobi of svdq_eig.h, the keep and
//                            rank rules, W = Bc V Sigma^-1, the closed-form coefficients and compress_single_task's tail
//                            (coeff_store_quantize of svdq_coeff.h) into the DESTINATION plan's small buffer, and the
//                            rebase table.
//   k_plan_rebase            one wavefront per work unit of the SOURCE plan, the geometry and staging of k_store_gram: a
//                            block of RB rows (256 up to 16 task slots, 128 above) of U_high / U_low is staged row-major
//                            in LDS, the mean rows beside it, the next block's loads in flight during compute.
//                            [rows] x [r + 1] . [r + 1] x [r' + 1] on the matrix pipe (v_mfma_f32_16x16x4_f32): a tile of 16
//                            rows x 16 new columns per accumulator, the source columns four per instruction in column
//                            order, the mean column last; bbar rides as output column r'.  The block's rows of U_high',
//                            U_low' and mean' are built in LDS and leave with 16-byte stores.
// No atomics: the same bits in every run.  Compiled with -ffp-contract=off.

#include "svdq_coeff.h"
#include "svdq_dispatch.h"
#include "svdq_merge_stream.h"
#include "svdq_small_view.h"
#include "svdq_store_pass.h"

#define CS_RA 33      // rows of W and of basis_gram_dev: r <= 32 source columns and the mean
#define CS_WC 32      // columns of W: r' <= 32
#define CS_KS 9       // MFMA steps over the source columns: ceil(33 / 4)
#define CS_WS 48      // floats per row of the staged B operand: r' + 1 <= 33 columns in three 16-column tiles

typedef __attribute__((address_space(1))) f32x4 cs_gf32x4_w;

// the destination's small buffer as k_plan_consolidate_eig takes it: the mutable SmallView under the name the kernel's
// symbol carries
struct CsSmall : SmallViewMut {};
struct CsTable {      // the typed arrays of the rebase table (svdq_consolidate_layout)
    float *w, *bbar;
    int32_t *r, *k, *live;
    double *dropped, *eta, *lambda;
};

// basis.py:147-156 and :199-211 on sig[0..r): the lines of eig_param (svdq_eig.h, which points back here), fp32 like
// the reference, with its fp64 form when the fp32 sum of squares overflows.  A second copy, not a shared function, so that
// no existing kernel is compiled from other source than before: keep the two in step.  One thread.
__device__ __forceinline__ void cs_rank_rule(const double *sig, int r, float thr, int max_rank, float *S, int &k_out,
                                             float &en_out) {
#pragma clang fp contract(off)
    float cum[32];
    float total = 0.f;
    for (int i = 0; i < r; ++i) {
        S[i] = (float)sig[i];
        total += S[i] * S[i];
    }
    if (total < 1e-10f) {
        for (int i = 0; i < r; ++i) cum[i] = 1.f;
    } else {
        float run = 0.f;
        for (int i = 0; i < r; ++i) {
            run += S[i] * S[i];
            cum[i] = run / total;
        }
    }
    int kk = 1;
    for (int i = 0; i < r; ++i)
        if (cum[i] < thr) ++kk;
    if (kk < 1) kk = 1;
    if (max_rank > 0 && kk > max_rank) kk = max_rank;
    if (kk > r) kk = r;
    float en = (kk > 0 && r > 0) ? cum[kk - 1] : 0.f;
    if (total > 3.4028234e38f) {
        double tot64 = 0.0, run64 = 0.0;
        for (int i = 0; i < r; ++i) tot64 += sig[i] * sig[i];
        kk = 1;
        for (int i = 0; i < r; ++i) {
            run64 += sig[i] * sig[i];
            if ((float)(run64 / tot64) < thr) ++kk;
        }
        if (max_rank > 0 && kk > max_rank) kk = max_rank;
        if (kk > r) kk = r;
        run64 = 0.0;
        for (int i = 0; i < kk; ++i) run64 += sig[i] * sig[i];
        en = (float)(run64 / tot64);
    }
    k_out = kk;
    en_out = en;
}

// Per entry: everything between A^T A and the destination's small buffer.  NS / ND: task slots of the source / the
// destination plan.
__global__ __launch_bounds__(EIG_THREADS) void k_plan_consolidate_eig(
    const SvdqParam *__restrict__ params, const int64_t *__restrict__ rows_dev, int NS, int ND, int src_stages,
    int src_centred, int dst_centred, float thr, int max_rank, int dst_bits, const int32_t *__restrict__ dst_bits_tab,
    int dst_stages, double min_sigma, const int32_t *__restrict__ keep /*[P][ND]*/,
    const double *__restrict__ basis_gram /*[P][33][33]*/, const int32_t *__restrict__ k_in,
    const int32_t *__restrict__ r_in, const uint16_t *__restrict__ chigh, const uint8_t *__restrict__ codes,
    const float *__restrict__ scale, const float *__restrict__ zp, CsSmall o, CsTable tb) {
#pragma clang fp contract(off)
    constexpr int LDX = 33, LDB = CS_RA;
    __shared__ double Ms[CS_RA * CS_RA], Bc[CS_RA * LDB], Tm[CS_RA * LDB], A[32 * LDX], V[32 * LDX];
    __shared__ double bb[CS_RA], rowoff[32], rowdg[32], lam[32], sgn[32], sig[32], gq[32];
    __shared__ float res[32 * LDN];
    __shared__ int order[32], slot[32], src[32], s_r, s_k;
    __shared__ const void *present[32];
    const int p = blockIdx.x, tid = threadIdx.x, nd = ND;
    const SvdqParam pd = params[p];
    const int64_t D = plan_rows_of(pd, rows_dev, p);

    // every field of the entry is written, whatever follows: the same bytes in every run
    for (int e = tid; e < nd * nd; e += EIG_THREADS) {
        o.coef[(size_t)p * nd * nd + e] = 0.f;
        o.chigh[(size_t)p * nd * nd + e] = 0;
    }
    for (int e = tid; e < nd * dst_stages * nd; e += EIG_THREADS) o.codes[(size_t)p * nd * dst_stages * nd + e] = 0;
    for (int e = tid; e < nd * dst_stages; e += EIG_THREADS) {
        o.scale[(size_t)p * nd * dst_stages + e] = 0.f;
        o.zp[(size_t)p * nd * dst_stages + e] = 0.f;
        o.rnorm[(size_t)p * nd * dst_stages + e] = 0.f;
    }
    for (int e = tid; e < CS_RA * CS_WC; e += EIG_THREADS) tb.w[(size_t)p * CS_RA * CS_WC + e] = 0.f;
    if (tid < CS_RA) tb.bbar[(size_t)p * CS_RA + tid] = 0.f;
    if (tid < 32) tb.lambda[(size_t)p * 32 + tid] = 0.0;
    if (tid < nd) o.sigma[(size_t)p * nd + tid] = 0.f;
    if (tid == 0) {
        o.k[p] = 0;
        o.r[p] = 0;
        o.energy[p] = 0.f;
        o.rows[p] = 0;
        tb.r[p] = 0;
        tb.k[p] = 0;
        tb.live[p] = 0;
        tb.dropped[p] = 0.0;
        tb.eta[p] = 0.0;
        if (p == 0) o.status[0] = 0;
    }
    __syncthreads();      // the defaults are in place before any thread writes a result over one
    if (D <= 0) return;   // workgroup-uniform: nothing of p is read

    // the kept slots, in destination slot order (every thread derives the same count)
    int nk = 0;
    for (int j = 0; j < nd; ++j) {
        const int s = keep[(size_t)p * nd + j];
        if (s >= 0 && s < NS) {
            if (tid == 0) {
                slot[nk] = j;
                src[nk] = s;
            }
            ++nk;
        }
    }
    if (tid < 32) present[tid] = nullptr;
    __syncthreads();
    if (nk == 0) return;      // workgroup-uniform
    if (tid < nk) present[slot[tid]] = params;      // any non-NULL value: coeff_store_quantize writes the slot

    int k, r;
    plan_ranks(k_in, r_in, p, D, NS, k, r);
    const int ra = r + (src_centred ? 1 : 0);      // columns of A = [U | mean]
    int bad = 0;
    const double *Mg = basis_gram + (size_t)p * CS_RA * CS_RA;
    for (int e = tid; e < ra * ra; e += EIG_THREADS) {
        const int a = e / ra, b = e % ra;
        const double v = Mg[a * CS_RA + b];
        Ms[a * CS_RA + b] = v;
        bad |= !isfinite(v);
    }
    // B = [c_j ; 1] of the kept slots: the merge's own dequantizing lines
    for (int e = tid; e < ra * nk; e += EIG_THREADS) {
        const int i = e / nk, j = e % nk;
        const double c = i < r ? (double)task_coeff(p, src[j], i, NS, k, src_stages, chigh, codes, scale, zp) : 1.0;
        Bc[i * LDB + j] = c;
        bad |= !isfinite(c);
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        // flagged (include/svdq.h, svdq_eig_rank_select): sigma and energy NaN, k / r / rows indexable, W zero, no sweep
        const int rf = (int)(D < (int64_t)nk ? D : (int64_t)nk);
        const float qnan = __builtin_nanf("");
        if (tid < nd) o.sigma[(size_t)p * nd + tid] = qnan;
        if (tid == 0) {
            o.k[p] = rf < 1 ? rf : 1;
            o.r[p] = rf;
            o.energy[p] = qnan;
            o.rows[p] = D;
        }
        return;
    }
    // bbar: the mean of the kept b_j in task order (centred destination), else 0; Bc = B - bbar 1^T
    if (tid < ra) {
        double s = 0.0;
        for (int j = 0; j < nk; ++j) s += Bc[tid * LDB + j];
        bb[tid] = dst_centred ? s / nk : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < ra * nk; e += EIG_THREADS) {
        const int i = e / nk, j = e % nk;
        Bc[i * LDB + j] -= bb[i];
    }
    __syncthreads();
    // Tm = (A^T A) Bc, K = Bc^T Tm formed for x <= y and mirrored
    for (int e = tid; e < ra * nk; e += EIG_THREADS) {
        const int a = e / nk, j = e % nk;
        double acc = 0.0;
        for (int b = 0; b < ra; ++b) acc += Ms[a * CS_RA + b] * Bc[b * LDB + j];
        Tm[a * LDB + j] = acc;
    }
    // g_j = sum_i sqrt(M_ii) |Bc[i][j]|
    if (tid < nk) {
        double g = 0.0;
        for (int i = 0; i < ra; ++i) {
            const double d = Ms[i * CS_RA + i];
            g += sqrt(d > 0.0 ? d : 0.0) * fabs(Bc[i * LDB + tid]);
        }
        gq[tid] = g * g;
    }
    __syncthreads();
    for (int e = tid; e < nk * nk; e += EIG_THREADS) {
        const int x = e / nk, y = e % nk;
        if (x > y) continue;
        double acc = 0.0;
        for (int a = 0; a < ra; ++a) acc += Bc[a * LDB + x] * Tm[a * LDB + y];
        A[x * LDX + y] = acc;
        A[y * LDX + x] = acc;
        V[x * LDX + y] = (x == y) ? 1.0 : 0.0;
        V[y * LDX + x] = (x == y) ? 1.0 : 0.0;
    }
    __syncthreads();
    double gsum = 0.0;
    for (int j = 0; j < nk; ++j) gsum += gq[j];
    const double eta = ((double)(256 + r + 3) * 5.9604644775390625e-08) * gsum;      // gamma = (256 + r + 3) 2^-24

    jacobi_parallel<EIG_THREADS, 32>(A, V, rowoff, rowdg, nk, tid);
    __syncthreads();
    // sort descending (stable on ties); sign: the largest-magnitude component positive (the first of equals)
    if (tid < nk) lam[tid] = A[tid * LDX + tid];
    __syncthreads();
    if (tid < nk) {
        int rank = 0;
        for (int i = 0; i < nk; ++i)
            if (lam[i] > lam[tid] || (lam[i] == lam[tid] && i < tid)) ++rank;
        order[rank] = tid;
    }
    __syncthreads();
    if (tid < nk) {
        const int c = order[tid];
        const double l = lam[c];
        sig[tid] = l > 0.0 ? sqrt(l) : 0.0;
        double best = 0.0, bv = 1.0;
        for (int j = 0; j < nk; ++j) {
            const double x = V[j * LDX + c];
            if (fabs(x) > best) {
                best = fabs(x);
                bv = x;
            }
        }
        sgn[tid] = bv < 0.0 ? -1.0 : 1.0;
        tb.lambda[(size_t)p * 32 + tid] = l;
    }
    __syncthreads();
    if (tid == 0) {
        // the keep rule: lambda is descending, so the kept directions are a prefix
        const double l0 = lam[order[0]];
        double floor_ = 4.0 * eta;
        const double rel = min_sigma * min_sigma * l0;
        if (rel > floor_) floor_ = rel;
        int cap = (int)(D < (int64_t)nk ? D : (int64_t)nk);
        if (cap > nd) cap = nd;
        int rn = 0;
        while (rn < cap && lam[order[rn]] > floor_ && lam[order[rn]] > 0.0) ++rn;
        double dropped = 0.0;
        for (int i = rn; i < nk; ++i) dropped += lam[order[i]] > 0.0 ? lam[order[i]] : 0.0;
        float S[32], en;
        int kn;
        cs_rank_rule(sig, rn, thr, max_rank, S, kn, en);
        for (int i = 0; i < rn; ++i) o.sigma[(size_t)p * nd + i] = S[i];
        o.k[p] = kn;
        o.r[p] = rn;
        o.energy[p] = en;
        o.rows[p] = D;
        tb.r[p] = rn;
        tb.k[p] = kn;
        tb.live[p] = 1;
        tb.dropped[p] = dropped;
        tb.eta[p] = eta;
        s_r = rn;
        s_k = kn;
    }
    __syncthreads();
    const int rn = s_r, kn = s_k;
    // W = Bc V Sigma^-1 (rows: the source columns, then the mean) and bbar, fp64 then fp32
    for (int e = tid; e < ra * rn; e += EIG_THREADS) {
        const int i = e / rn, c = e % rn;
        double acc = 0.0;
        for (int j = 0; j < nk; ++j) acc += Bc[i * LDB + j] * V[j * LDX + order[c]];
        tb.w[(size_t)p * CS_RA * CS_WC + i * CS_WC + c] = (float)(sgn[c] * acc / sig[c]);
    }
    if (tid < ra) tb.bbar[(size_t)p * CS_RA + tid] = (float)bb[tid];
    // the closed form c'_j[i] = sgn_i sigma_i V[j][i]: the coefficients of the UNROUNDED U' (Tm is free now)
    for (int e = tid; e < nd * nd; e += EIG_THREADS) Tm[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < nk * rn; e += EIG_THREADS) {
        const int j = e / rn, i = e % rn;
        Tm[slot[j] * nd + i] = sgn[i] * sig[i] * V[j * LDX + order[i]];
    }
    __syncthreads();
    const int bits = dst_bits_tab ? dst_bits_tab[p] : dst_bits;
    coeff_store_quantize(p, nd, kn, rn, bits, dst_stages, Tm, nullptr, present, res, o.coef, o.chigh, o.codes, o.scale,
                         o.zp, o.rnorm);
}

// ---------------------------------------------------------------------------------------------- the streaming pass
__host__ __device__ constexpr int cs_align16(int x) { return (x + 15) / 16 * 16; }
// dynamic LDS: the staged basis rows | the block's mean rows [RB] | the B operand [36][CS_WS] | the output image:
// U_high' rows, U_low' rows (each from a 16-byte boundary), mean' [RB]
__host__ __device__ constexpr size_t cs_lds_bytes(int rb, int ns, int nd, int es) {
    return (size_t)stream_ubytes(rb, ns, es) + (size_t)rb * 4 + (size_t)4 * CS_KS * CS_WS * 4 +
           (size_t)cs_align16(rb * nd * es) + 32 + (size_t)rb * 4;
}

__device__ __forceinline__ void cs_put(__half *dst, float v) { *dst = __float2half_rn(v); }
__device__ __forceinline__ void cs_put(float *dst, float v) { *dst = v; }

// nbytes of an LDS image (16-byte aligned) to a global range that starts on a 16-byte boundary: 16 bytes per lane and
// store, the last nbytes % 16 bytes element by element.  Nothing past nbytes is written.
template <typename E>
__device__ __forceinline__ void cs_store_range(uint8_t *gdst, const uint8_t *img, int nbytes, int lane) {
    const int nv = nbytes >> 4;
    for (int v = lane; v < nv; v += 64) *(cs_gf32x4_w *)(gdst + 16ll * v) = reinterpret_cast<const f32x4 *>(img)[v];
    const int e0 = (nv << 4) / (int)sizeof(E), e1 = nbytes / (int)sizeof(E);
    if (e0 + lane < e1) reinterpret_cast<E *>(gdst)[e0 + lane] = reinterpret_cast<const E *>(img)[e0 + lane];
}

// CMAX: the source columns the instantiation has registers for (8, 16 or 32 >= NS >= r).
template <bool U16, int CMAX>
__global__ __launch_bounds__(64) void k_plan_rebase(const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units,
                                                    const SvdqParam *__restrict__ dparams,
                                                    const int64_t *__restrict__ rows_dev, int NS, int ND, int dst_centred,
                                                    const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                                    const uint8_t *__restrict__ basis, const float *__restrict__ meanbuf,
                                                    const float *__restrict__ w_tab, const float *__restrict__ bbar_tab,
                                                    const int32_t *__restrict__ tr, const int32_t *__restrict__ tk,
                                                    const int32_t *__restrict__ live, uint8_t *__restrict__ obasis,
                                                    float *__restrict__ omean) {
    using T = typename UElem<U16>::type;
    constexpr int ES = U16 ? 2 : 4;
    constexpr int RPL = store_rpl(CMAX), RB = store_rb(CMAX), SV = store_sv(CMAX, ES);
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int lane = threadIdx.x, n = NS, u = blockIdx.x;
    const int g = lane >> 4, col = lane & 15;
    const SvdqUnit ud = units[u];
    const int p = ud.param;
    if (!live[p]) return;      // wave-uniform: nothing of p is written
    const SvdqParam pd = params[p];
    const SvdqParam dd = dparams[p];
    int64_t D = plan_rows_of(pd, rows_dev, p);
    if (D > dd.rows) D = dd.rows;      // and never more than the destination's slab has room for
    // the unit's view of the plan and the block loop written out: as store_unit / stream_blocks (svdq_store_pass.h) this
    // kernel spills more scalar registers
    int64_t cpos = ud.row0;
    int64_t cend = ud.row0 + ud.nrows;
    if (cend > D) cend = D;
    if (cpos >= cend) return;      // wave-uniform
    int k, r;
    plan_ranks(k_in, r_in, p, D, n, k, r);
    const int nl = r - k;
    mg_gfloat *gmean = meanbuf ? (mg_gfloat *)(meanbuf + pd.mean_off) : nullptr;
    const int ra = r + (gmean ? 1 : 0);
    // r' and k' as the eigen stage left them, held to what the destination's slab and the output image have room for
    int rn = tr[p], kn = tk[p];
    const int rcap = (int)(D < (int64_t)ND ? D : (int64_t)ND);
    rn = rn < 0 ? 0 : (rn > rcap ? rcap : rn);
    kn = kn < 0 ? 0 : (kn > rn ? rn : kn);
    const int nln = rn - kn;
    const bool wmean = dst_centred && omean;
    const int oc = rn + (wmean ? 1 : 0);      // output columns: U', then bbar's
    if (oc == 0) return;                      // wave-uniform
    const int ntile = (oc + 15) >> 4, nsteps = (ra + 3) >> 2;

    uint8_t *Ubuf = lds_raw;
    const int moff = stream_ubytes(RB, n, ES);
    float *Ms = reinterpret_cast<float *>(lds_raw + moff);                                   // [RB]
    float *Wl = Ms + RB;                                                                     // [36][CS_WS]
    uint8_t *Oh = reinterpret_cast<uint8_t *>(Wl + 4 * CS_KS * CS_WS);                       // [RB][k']
    uint8_t *Ol = Oh + cs_align16(RB * kn * ES);                                             // [RB][r' - k']
    float *Om = reinterpret_cast<float *>(Ol + cs_align16(RB * nln * ES));                   // [RB]

    // ---- once per unit: the B operand Wl[source column][output column], zeros past ra and past oc
    for (int e = lane; e < 4 * CS_KS * CS_WS; e += 64) {
        const int i = e / CS_WS, c = e % CS_WS;
        float v = 0.f;
        if (i < ra) {
            if (c < rn) v = w_tab[(size_t)p * CS_RA * CS_WC + i * CS_WC + c];
            else if (c == rn && wmean) v = bbar_tab[(size_t)p * CS_RA + i];
        }
        Wl[e] = v;
    }

    const uint8_t *gUh = basis + pd.slab_off;
    const uint8_t *gUl = SVDQ_SLAB_LOW(gUh, D, k, ES);
    uint8_t *goh = obasis + dd.slab_off;
    uint8_t *gol = SVDQ_SLAB_LOW(goh, D, kn, ES);
    float *gom = wmean ? omean + dd.mean_off : nullptr;

    float mpf[RPL] = {}, bpf[RPL] = {};
    f32x4 ureg[SV];
    auto prefetch = [&](int64_t c0) {
        const int nr = block_rows<RB>(c0, cend);
        load_rows<RPL>(mpf, bpf, gmean, (mg_gfloat *)nullptr, c0, nr, lane);
        ustage_fetch(ureg, ustage_plan<ES>(c0, nr, k, nl), gUh, gUl, lane);
    };

    auto stage = [&](const UStage &cur, int) {
        ustage_commit(Ubuf, ureg, cur, lane);
        if (gmean) {
#pragma unroll
            for (int m = 0; m < RPL; ++m) Ms[64 * m + lane] = mpf[m];
        }
    };
    prefetch(cpos);
    while (true) {
        const int nr = block_rows<RB>(cpos, cend);
        const UStage cur = ustage_plan<ES>(cpos, nr, k, nl);
        stage(cur, nr);
        lds_fence();
        const bool more = cpos + RB < cend;
        if (more) prefetch(cpos + RB);

        // ---- the lane's A operand of step s is source column 4 s + g of its row: where that column sits in the staged
        // image (byte offset of the block's row 0, byte stride from row to row); the mean column reads the fp32 strip, a
        // column past ra reads nothing
        int aoff[CS_KS], astr[CS_KS];
        unsigned mmask = 0, zmask = 0;
#pragma unroll
        for (int s = 0; s < CS_KS; ++s) {
            const int i = 4 * s + g;
            aoff[s] = 0;
            astr[s] = 0;
            if (i < r) {
                ustage_column(cur, i, k, nl, ES, aoff[s], astr[s]);
            } else if (i < ra) {
                aoff[s] = moff;
                astr[s] = 4;
                mmask |= 1u << s;
            } else {
                zmask |= 1u << s;
            }
        }
        auto a_operand = [&](int s, int row) -> float {
            const int ao = aoff[s] + row * astr[s];
            float a;
            if ((mmask >> s) & 1u) a = lds_u(lds_raw, ao, float{});
            else a = lds_u(lds_raw, ao, T{});
            return ((zmask >> s) & 1u) ? 0.f : a;
        };
        const int nrt = (nr + 15) >> 4;
        const int nfull = r >> 2;      // steps whose four columns are basis columns in every lane: no kinds to tell apart
        for (int ot = 0; ot < ntile; ++ot) {      // wave-uniform
            float b[CS_KS];
#pragma unroll
            for (int s = 0; s < CS_KS; ++s) b[s] = Wl[(4 * s + g) * CS_WS + 16 * ot + col];
            // where the lane's output column 16 ot + col goes in the image: element 0 of it, the byte stride from row
            // to row, and what it is (0 nothing, 1 a basis element, 2 the fp32 mean)
            const int c = 16 * ot + col;
            int okind = 0, ostr = 0;
            uint8_t *obase = Oh;
            if (c < kn) {
                okind = 1;
                obase = Oh + c * ES;
                ostr = kn * ES;
            } else if (c < rn) {
                okind = 1;
                obase = Ol + (c - kn) * ES;
                ostr = nln * ES;
            } else if (c == rn && wmean) {
                okind = 2;
                obase = reinterpret_cast<uint8_t *>(Om);
                ostr = 4;
            }
            for (int rt = 0; rt < nrt; rt += 2) {
                // two independent accumulators: rows 16 rt + col and 16 (rt + 1) + col, clamped into the block (a row
                // of A only reaches its own row of the result, and rows past nr are not stored)
                int row0 = 16 * rt + col, row1 = row0 + 16;
                row0 = row0 < nr ? row0 : nr - 1;
                row1 = row1 < nr ? row1 : nr - 1;
                f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < CS_KS; ++s)
                    if (s < nsteps) {      // wave-uniform, and so is s < nfull
                        float a0, a1;
                        if (s < nfull) {
                            a0 = lds_u(lds_raw, aoff[s] + row0 * astr[s], T{});
                            a1 = lds_u(lds_raw, aoff[s] + row1 * astr[s], T{});
                        } else {
                            a0 = a_operand(s, row0);
                            a1 = a_operand(s, row1);
                        }
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b[s], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b[s], acc1, 0, 0, 0);
                    }
                // result register v of accumulator h is (row 16 (rt + h) + 4 g + v, output column 16 ot + col)
                uint8_t *op = obase + (16 * rt + 4 * g) * ostr;
                auto emit = [&](auto guarded_c, auto put) {
                    constexpr bool GUARDED = decltype(guarded_c)::value;
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int v = 0; v < 4; ++v)
                            if (!GUARDED || 16 * (rt + h) + 4 * g + v < nr) put(op + (16 * h + v) * ostr, h ? acc1[v] : acc0[v]);
                };
                auto put_t = [](uint8_t *d, float x) { cs_put(reinterpret_cast<T *>(d), x); };
                auto put_f = [](uint8_t *d, float x) { *reinterpret_cast<float *>(d) = x; };
                const bool whole = 16 * (rt + 2) <= nr;      // wave-uniform: both tiles lie inside the block
                if (okind == 1) {
                    if (whole) emit(std::false_type{}, put_t);
                    else emit(std::true_type{}, put_t);
                } else if (okind == 2) {
                    if (whole) emit(std::false_type{}, put_f);
                    else emit(std::true_type{}, put_f);
                }
            }
        }
        lds_fence();
        // ---- the block's rows leave: a block starts at a multiple of 128 rows, so each range starts on 16 bytes
        if (kn > 0) cs_store_range<T>(goh + cpos * (int64_t)kn * ES, Oh, nr * kn * ES, lane);
        if (nln > 0) cs_store_range<T>(gol + cpos * (int64_t)nln * ES, Ol, nr * nln * ES, lane);
        if (wmean) cs_store_range<float>(reinterpret_cast<uint8_t *>(gom + cpos), reinterpret_cast<const uint8_t *>(Om), nr * 4, lane);
        if (!more) break;
        cpos += RB;
        lds_fence();      // the basis rows and the output image are rewritten next
    }
}

// ---------------------------------------------------------------------------------------------- host
static svdq_consolidate_layout cs_layout(int P) {
    svdq_consolidate_layout L;
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = off;
        off = svdq_align_up(off + bytes, 256);
        return at;
    };
    L.w_off = take((int64_t)P * CS_RA * CS_WC * 4);
    L.bbar_off = take((int64_t)P * CS_RA * 4);
    L.r_off = take((int64_t)P * 4);
    L.k_off = take((int64_t)P * 4);
    L.live_off = take((int64_t)P * 4);
    L.dropped_off = take((int64_t)P * 8);
    L.eta_off = take((int64_t)P * 8);
    L.lambda_off = take((int64_t)P * 32 * 8);
    L.total_bytes = off > 0 ? off : 256;
    return L;
}

static CsTable cs_table(void *rebase, int P) {
    const svdq_consolidate_layout L = cs_layout(P);
    uint8_t *b = reinterpret_cast<uint8_t *>(rebase);
    CsTable t;
    t.w = reinterpret_cast<float *>(b + L.w_off);
    t.bbar = reinterpret_cast<float *>(b + L.bbar_off);
    t.r = reinterpret_cast<int32_t *>(b + L.r_off);
    t.k = reinterpret_cast<int32_t *>(b + L.k_off);
    t.live = reinterpret_cast<int32_t *>(b + L.live_off);
    t.dropped = reinterpret_cast<double *>(b + L.dropped_off);
    t.eta = reinterpret_cast<double *>(b + L.eta_off);
    t.lambda = reinterpret_cast<double *>(b + L.lambda_off);
    return t;
}

extern "C" int svdq_plan_consolidate_layout(const svdq_plan *pl, svdq_consolidate_layout *out) {
    if (!pl || !out) {
        svdq_set_error("svdq_plan_consolidate_layout: the plan and out are required");
        return SVDQ_EINVAL;
    }
    *out = cs_layout(pl->n_params);
    return SVDQ_OK;
}

// what both entry points refuse of the two plans
static int cs_check_plans(const char *who, const svdq_plan *src, const svdq_plan *dst) {
    if (!src || !dst) {
        svdq_set_error("%s: the source and the destination plan are required", who);
        return SVDQ_EINVAL;
    }
    if (src->n_params != dst->n_params) {
        svdq_set_error("%s: the destination plan has %d parameters, the source %d", who, (int)dst->n_params,
                       (int)src->n_params);
        return SVDQ_EINVAL;
    }
    if ((src->cfg.fp16 != 0) != (dst->cfg.fp16 != 0)) {
        svdq_set_error("%s: the destination's basis element type differs from the source's", who);
        return SVDQ_EINVAL;
    }
    if (dst->n_tasks > SVDQ_MAX_TASKS || src->n_tasks > SVDQ_MAX_TASKS) {
        svdq_set_error("%s: at most %d task slots", who, SVDQ_MAX_TASKS);
        return SVDQ_EINVAL;
    }
    for (int p = 0; p < src->n_params; ++p)
        if (src->h_params[p].rows != dst->h_params[p].rows) {
            svdq_set_error("%s: parameter %d has %lld rows in the destination plan, %lld in the source", who, p,
                           (long long)dst->h_params[p].rows, (long long)src->h_params[p].rows);
            return SVDQ_EINVAL;
        }
    return SVDQ_OK;
}

extern "C" int svdq_plan_consolidate_eig(const svdq_plan *src, const svdq_plan *dst, const int32_t *keep_host,
                                         const int32_t *keep_dev, const int64_t *rows_dev, const void *src_small,
                                         const double *basis_gram, float min_sigma, void *dst_small, void *rebase,
                                         void *stream) {
    const char *who = "svdq_plan_consolidate_eig";
    const int rc = cs_check_plans(who, src, dst);
    if (rc != SVDQ_OK) return rc;
    if (!keep_host || !keep_dev || !src_small || !basis_gram || !dst_small || !rebase) {
        svdq_set_error("%s: keep (host and device), the two small buffers, basis_gram and rebase are required", who);
        return SVDQ_EINVAL;
    }
    if (svdq_refuse_unaligned(who, svdq_addr_bits(keep_dev, rows_dev, basis_gram), 8, "keep, rows and basis_gram"))
        return SVDQ_EINVAL;
    if (svdq_refuse_unaligned(who, svdq_addr_bits(src_small, dst_small, rebase), 16, "the small buffers and rebase"))
        return SVDQ_EINVAL;
    if (!(min_sigma >= 0.f) || !(min_sigma <= 3.0e38f)) {
        svdq_set_error("%s: min_sigma must be finite and >= 0", who);
        return SVDQ_EINVAL;
    }
    const int P = src->n_params, NS = src->n_tasks, ND = dst->n_tasks;
    for (int64_t e = 0; e < (int64_t)P * ND; ++e)
        if (keep_host[e] < -1 || keep_host[e] >= NS) {
            svdq_set_error("%s: keep[%lld][%lld] = %d, need -1 (absent) or a source slot in [0, %d)", who,
                           (long long)(e / ND), (long long)(e % ND), (int)keep_host[e], NS);
            return SVDQ_EINVAL;
        }
    const SmallView ss = small_view(src->small, src_small);
    const CsSmall o{small_view_mut(dst->small, dst_small)};
    hipLaunchKernelGGL(k_plan_consolidate_eig, dim3(P), dim3(EIG_THREADS), 0, (hipStream_t)stream, src->d_params, rows_dev,
                       NS, ND, src->cfg.rtvq_stages, src->cfg.center != 0, dst->cfg.center != 0,
                       dst->cfg.energy_threshold, dst->cfg.max_rank, dst->cfg.low_bits, dst->d_bits,
                       dst->cfg.rtvq_stages, (double)min_sigma, keep_dev, basis_gram, ss.k, ss.r, ss.chigh, ss.codes,
                       ss.scale, ss.zp, o, cs_table(rebase, P));
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

extern "C" int svdq_plan_rebase(const svdq_plan *src, const svdq_plan *dst, const int64_t *rows_dev,
                                const void *src_small, const void *src_basis, const float *src_mean, const void *rebase,
                                void *dst_basis, float *dst_mean, void *stream) {
    const char *who = "svdq_plan_rebase";
    const int rc = cs_check_plans(who, src, dst);
    if (rc != SVDQ_OK) return rc;
    if (!src_small || !src_basis || !rebase || !dst_basis) {
        svdq_set_error("%s: the source's small buffer and basis, rebase and the destination's basis are required", who);
        return SVDQ_EINVAL;
    }
    if (src->cfg.center && !src_mean) {
        svdq_set_error("%s: the source's mean is required on a centred source", who);
        return SVDQ_EINVAL;
    }
    if (dst->cfg.center && !dst_mean) {
        svdq_set_error("%s: the destination's mean is required on a centred destination", who);
        return SVDQ_EINVAL;
    }
    if (svdq_refuse_unaligned(who, svdq_addr_bits(rows_dev), 8, "rows")) return SVDQ_EINVAL;
    if (svdq_refuse_unaligned(who, svdq_addr_bits(src_small, src_basis, src_mean, rebase, dst_basis, dst_mean), 16,
                              "small, the basis and mean buffers and rebase"))
        return SVDQ_EINVAL;
    if (src->n_units <= 0) return SVDQ_OK;
    const SmallView ss = small_view(src->small, src_small);
    const CsTable t = cs_table(const_cast<void *>(rebase), src->n_params);
    const float *mn = src->cfg.center ? src_mean : nullptr;      // an uncentred source has A = U
    float *om = dst->cfg.center ? dst_mean : nullptr;
    const int n = src->n_tasks, nd = dst->n_tasks;
    const bool ok = svdq_dispatch_bool(src->cfg.fp16 != 0, [&](auto f16_c) {
        constexpr bool U16 = f16_c;
        return svdq_dispatch_int<8, 16, 32>(svdq_slot_class(n), [&](auto cmax_c) {
            constexpr int CMAX = cmax_c;
            const size_t lds = cs_lds_bytes(store_rb(CMAX), n, nd, U16 ? 2 : 4);
            hipLaunchKernelGGL((k_plan_rebase<U16, CMAX>), dim3(src->n_units), dim3(64), lds, (hipStream_t)stream,
                               src->d_params, src->d_units, dst->d_params, rows_dev, n, nd, dst->cfg.center != 0, ss.k, ss.r,
                               reinterpret_cast<const uint8_t *>(src_basis), mn, t.w, t.bbar, t.r, t.k, t.live,
                               reinterpret_cast<uint8_t *>(dst_basis), om);
            return true;
        });
    });
    if (!ok) return svdq_launch_status(false, "k_plan_rebase");
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}
