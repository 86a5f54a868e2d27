// svdq_merge_stream.h -- the device pieces the streaming consumers of svdq_merge.hip share.  k_merge_reconstruct,
// k_task_reconstruct and k_task_expand are the order in which they call these pieces plus their family's epilogue;
// k_diag takes the byte count, ustage_fetch and unit_source_range; k_merge_expand takes the types, ustage_plan,
// lds_fence and unit_source_range and carries its own copy of the other steps (its launch is sized by StreamLds; the
// comment at the kernel says why).  svdq_ties.hip builds its two streaming kernels from the same pieces, and the passes
// over a plan's stored artifacts (plan_project, plan_extend, store_gram, consolidate) take the staging from here and
// their own shared steps -- the clamped unit view, the staged image by column, the block loop -- from svdq_store_pass.h,
// which includes this file.  Included by files compiled with -ffp-contract=off alone (every product and sum is rounded
// where the reference's torch ops round).
#pragma once

#include "svdq_common.h"
#include <hip/hip_fp16.h>

// pointers read out of device tables are generic to the compiler: without the address space it emits flat_load /
// flat_store, which count on lgkmcnt as well and so make every LDS wait a wait for HBM
typedef const __attribute__((address_space(1))) float mg_gfloat;
typedef __attribute__((address_space(1))) float mg_gfloat_w;
typedef const __attribute__((address_space(1))) uint8_t mg_gbyte;
typedef const __attribute__((address_space(1))) f32x4 mg_gf32x4;

template <bool U16> struct UElem;
template <> struct UElem<true> { using type = __half; };
template <> struct UElem<false> { using type = float; };
__device__ __forceinline__ float u_val(const __half *u, int i) { return __half2float(u[i]); }
__device__ __forceinline__ float u_val(const float *u, int i) { return u[i]; }

__device__ __forceinline__ void lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------ geometry and the LDS carve
// bytes of the staged basis rows of one block of rb rows: both parts + the alignment slack of their 16-byte loads
__host__ __device__ constexpr int stream_ubytes(int rb, int n, int es) {
    return (int)(((int64_t)rb * n * es + 48 + 15) / 16 * 16);
}

// Blocks of RB = 64 RPL rows (256 for N <= 16, 128 above: the block's basis rows then fit 9 (fp16) / 17 (fp32) 16-byte
// registers per lane); lane l owns rows l, 64 + l, ... of a block (conflict-free row reads from the row-major LDS image).
template <bool U16, int RPL> struct StreamGeom {
    using T = typename UElem<U16>::type;
    static constexpr int ES = U16 ? 2 : 4;
    static constexpr int RB = 64 * RPL;
    static constexpr int NMAX = RPL == 4 ? 16 : 32;                     // tasks this block size is launched for
    static constexpr int SV = (RB * NMAX * ES / 16 + 2 + 63) / 64;     // 16-byte vectors of one block's basis rows per lane
    __host__ __device__ static constexpr int ubytes(int n) { return stream_ubytes(RB, n, ES); }
};

// dynamic LDS of a streaming kernel: the staged basis rows, the [RB] mean strip (source walk only), the coefficient
// image [column][stride], the share strip.  The launchers size the allocation with bytes(), the kernels carve it with
// the offsets: one formula.
template <bool U16, int RPL, bool WALK> struct StreamLds {
    using G = StreamGeom<U16, RPL>;
    __host__ __device__ static constexpr size_t mean_off(int n) { return (size_t)G::ubytes(n); }
    __host__ __device__ static constexpr size_t coeff_off(int n) { return mean_off(n) + (WALK ? (size_t)G::RB * 4 : 0); }
    __host__ __device__ static constexpr size_t share_off(int n, int stride) { return coeff_off(n) + (size_t)stride * n * 4; }
    __host__ __device__ static constexpr size_t bytes(int n, int stride, int n_share) {
        return share_off(n, stride) + (size_t)n_share * 4;
    }
};

template <int RB> __device__ __forceinline__ int block_rows(int64_t pos, int64_t end) {
    return (int)((end - pos < RB) ? (end - pos) : RB);
}

// ------------------------------------------------------------------------------------ a unit's view of the plan
// THE slab split: U_low [D][r - k] starts on the first 256-byte boundary behind U_high [D][k] (include/svdq.h).  A macro:
// as an inlined function the same expression reaches the scheduler in another order and the merge kernels move.
#define SVDQ_SLAB_LOW(gUh, D, k, ES) ((gUh) + svdq_align_up((D) * (int64_t)(k) * (ES), 256))

struct UnitView {
    int64_t D;                    // rows of the parameter (compacted rows of a masked region)
    int k, nl;                    // columns of U_high, of U_low
    const uint8_t *gUh, *gUl;     // the two parts of the parameter's slab
    mg_gfloat *gmean, *gbase;     // NULL = not centred / nothing to add
};
template <int ES>
__device__ __forceinline__ UnitView unit_view(const SvdqParam &pd, int p, const int64_t *__restrict__ rows_dev,
                                              const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                              const uint8_t *__restrict__ basis, const float *__restrict__ meanbuf,
                                              const float *const *__restrict__ base_ptrs) {
    UnitView v;
    v.D = rows_dev ? rows_dev[p] : pd.rows;
    v.k = k_in[p];
    v.nl = r_in[p] - v.k;
    v.gUh = basis + pd.slab_off;
    v.gUl = SVDQ_SLAB_LOW(v.gUh, v.D, v.k, ES);
    v.gmean = meanbuf ? (mg_gfloat *)(meanbuf + pd.mean_off) : nullptr;
    v.gbase = base_ptrs ? (mg_gfloat *)base_ptrs[p] : nullptr;
    return v;
}

// ------------------------------------------------------------------------------------ basis staging
// where a block's staged basis rows sit (wave-uniform): the two parts are fetched with aligned 16-byte loads and kept
// row-major, one after the other, in LDS
struct UStage {
    int nvh, nv;     // 16-byte vectors of the U_high part, of both parts
    int offh, offl;  // element offset of the block's first row inside each part
    int64_t a0h, a0l;
};
template <int ES>
__device__ __forceinline__ UStage ustage_plan(int64_t c0, int nr, int k, int nl) {
    UStage u;
    const int64_t b0h = c0 * k * ES, b1h = (c0 + nr) * (int64_t)k * ES;
    const int64_t b0l = c0 * nl * ES, b1l = (c0 + nr) * (int64_t)nl * ES;
    u.a0h = b0h & ~15ll;
    u.a0l = b0l & ~15ll;
    u.nvh = k > 0 ? (int)((b1h - u.a0h + 15) >> 4) : 0;
    u.nv = u.nvh + (nl > 0 ? (int)((b1l - u.a0l + 15) >> 4) : 0);
    u.offh = (int)(b0h - u.a0h) / ES;
    u.offl = (int)(b0l - u.a0l) / ES;
    return u;
}

// global -> registers: the block's run of basis rows, 16 bytes per lane and load
template <int SV>
__device__ __forceinline__ void ustage_fetch(f32x4 (&ureg)[SV], const UStage &us, const uint8_t *gUh, const uint8_t *gUl,
                                             int lane) {
#pragma unroll
    for (int s = 0; s < SV; ++s) {
        const int v = lane + 64 * s;
        if (v < us.nv) {
            const uint8_t *gp = (v < us.nvh) ? gUh + us.a0h + 16ll * v : gUl + us.a0l + 16ll * (v - us.nvh);
            ureg[s] = *(mg_gf32x4 *)gp;
        }
    }
}

// registers -> LDS (the staging layout is a function of the block's first row: recomputed by the caller, not kept)
template <int SV>
__device__ __forceinline__ void ustage_commit(uint8_t *lds, const f32x4 (&ureg)[SV], const UStage &cur, int lane) {
#pragma unroll
    for (int s = 0; s < SV; ++s) {
        const int v = lane + 64 * s;
        if (v < cur.nv) reinterpret_cast<f32x4 *>(lds)[v] = ureg[s];
    }
}

// row 0 of the block in each part of the LDS image
template <typename T> __device__ __forceinline__ const T *ustage_high(const uint8_t *lds, const UStage &cur) {
    return reinterpret_cast<const T *>(lds) + cur.offh;
}
template <typename T> __device__ __forceinline__ const T *ustage_low(const uint8_t *lds, const UStage &cur) {
    return reinterpret_cast<const T *>(lds + 16 * cur.nvh) + cur.offl;
}

// ------------------------------------------------------------------------------------ row loads
// plain form: the mean and base values of the lane's rows of the block [rb, rb + nr); rows past the block's end are
// clamped into it (their results are not stored)
template <int RPL>
__device__ __forceinline__ void load_rows(float (&mpf)[RPL], float (&bpf)[RPL], mg_gfloat *gmean, mg_gfloat *gbase,
                                          int64_t rb, int nr, int lane) {
#pragma unroll
    for (int m = 0; m < RPL; ++m) {
        const int q = 64 * m + lane;
        const int64_t row = rb + (q < nr ? q : nr - 1);
        if (gmean) mpf[m] = gmean[row];
        if (gbase) bpf[m] = gbase[row];
    }
}

// walk form: mask bytes and base values at the lane's SOURCE rows s0 + 64 e + lane (a full chunk without tests, the
// range's last chunk guarded), mean values at the compacted rows c0 + 64 e + lane of the nr rows that are fetched.
// mk = 0x100 past the end of the range: selected by neither polarity.
template <int RPL>
__device__ __forceinline__ void load_rows_walk(unsigned (&mk)[RPL], float (&bpf)[RPL], float (&mpf)[RPL], mg_gbyte *gmask,
                                               mg_gfloat *gbase, mg_gfloat *gmean, int64_t s0, int64_t src_hi, int64_t c0,
                                               int nr, int lane) {
    constexpr int RB = 64 * RPL;
    const int64_t r0 = s0 + lane;
    if (s0 + RB <= src_hi) {
#pragma unroll
        for (int e = 0; e < RPL; ++e) {
            mk[e] = (unsigned)gmask[r0 + 64 * e];
            if (gbase) bpf[e] = gbase[r0 + 64 * e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < RPL; ++e) {
            const bool in = r0 + 64 * e < src_hi;
            mk[e] = in ? (unsigned)gmask[r0 + 64 * e] : 0x100u;
            if (gbase) bpf[e] = in ? gbase[r0 + 64 * e] : 0.f;
        }
    }
    if (gmean) {
#pragma unroll
        for (int e = 0; e < RPL; ++e) mpf[e] = (64 * e + lane < nr) ? gmean[c0 + 64 * e + lane] : 0.f;
    }
}

// ------------------------------------------------------------------------------------ source walk
#define MRG_POS_MASK ((1ll << 62) - 1)      // ustart: bit 62 = the region takes the cleared mask elements

struct SrcRange {
    int64_t lo, hi;
    int inv;
};
__device__ __forceinline__ SrcRange unit_source_range(const SvdqParam &pd, int u, const int64_t *__restrict__ ustart) {
    const int64_t us = ustart[u];
    SrcRange s;
    s.inv = (int)((us >> 62) & 1);
    s.lo = (u == pd.unit_begin) ? 0 : (us & MRG_POS_MASK);
    s.hi = (u == pd.unit_begin + pd.unit_count - 1) ? pd.rows : (ustart[u + 1] & MRG_POS_MASK);
    return s;
}

// The chunk's selection from its mask bytes: RPL ballots give the rank of each of the lane's rows among the chunk's
// selected rows (no index list, no scan through memory) and their number, never past `room`, the compacted rows the
// unit has left, whatever the mask says.  The lane's own flags sit in ONE vector register: bit m = row m is selected,
// bit 4 + m = it is inside the range -- as lane masks (bool in[], sel[]) they hold sixteen scalar registers across the
// compute phase.
template <int RPL> struct WalkSel {
    int rank[RPL];
    int count;
    unsigned flags;
    __device__ __forceinline__ bool sel(int m) const { return (flags >> m) & 1u; }
    __device__ __forceinline__ bool in(int m) const { return (flags >> (4 + m)) & 1u; }
};
template <int RPL>
__device__ __forceinline__ WalkSel<RPL> walk_select(const unsigned (&mk)[RPL], int inv, int64_t room) {
    static_assert(RPL <= 4, "four flag bits per kind");
    WalkSel<RPL> w;
    w.flags = 0;
    int base = 0;
#pragma unroll
    for (int e = 0; e < RPL; ++e) {
        if (mk[e] != 0x100u) w.flags |= 16u << e;
        const bool sb = inv ? (mk[e] == 0u) : (mk[e] != 0u && mk[e] != 0x100u);
        const unsigned long long bal = __ballot(sb);
        w.rank[e] = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
        if (sb && w.rank[e] < room) w.flags |= 1u << e;
        base += (int)__popcll(bal);
    }
    w.count = base < room ? base : (int)room;
    return w;
}

// ------------------------------------------------------------------------------------ coefficients and fma chains
// coefficient i (< r) of task t of parameter p as the reference holds it in fp32: column i < k the fp16 c_high, else the
// dequantized c_low
__device__ __forceinline__ float task_coeff(int p, int t, int i, int n, int k, int stages,
                                            const uint16_t *__restrict__ chigh, const uint8_t *__restrict__ codes,
                                            const float *__restrict__ scale, const float *__restrict__ zp) {
    if (i < k) return __half2float(__ushort_as_half(chigh[((size_t)p * n + t) * n + i]));
    // zeros + sum over stages of (q - zero_point) / scale (rtvq.py:29-36, :85-103)
    float c = 0.f;
    const size_t sb = ((size_t)p * n + t) * stages;
    for (int st = 0; st < stages; ++st) {
        const float q = (float)codes[(sb + st) * n + (i - k)];
        c = __fadd_rn(c, __fdiv_rn(__fsub_rn(q, zp[sb + st]), scale[sb + st]));
    }
    return c;
}

// the transposed coefficient image C[column][stride]: the coefficients of a column side by side, one per set or task;
// slots past n_valid are 0.  cbar_p [n_valid][n]: the parameter's coefficient vectors.
__device__ __forceinline__ void stage_coeffs(float *C, const float *__restrict__ cbar_p, int n, int n_valid, int stride,
                                             int lane) {
    for (int e = lane; e < stride * n; e += 64) {
        const int i = e / stride, s = e % stride;
        C[e] = s < n_valid ? cbar_p[(size_t)s * n + i] : 0.f;
    }
}

// the lane's rows inside the LDS image.  Plain form: rows l, 64 + l, ... of the block, clamped into it
template <int RPL> __device__ __forceinline__ void block_rows_of_lane(int (&rl)[RPL], int rows_blk, int lane) {
#pragma unroll
    for (int m = 0; m < RPL; ++m) {
        const int q = 64 * m + lane;
        rl[m] = q < rows_blk ? q : rows_blk - 1;
    }
}
// walk form: a selected source row reads the basis row of its rank (and its mean value from the strip M), any other row 0
template <int RPL>
__device__ __forceinline__ void walk_rows_of_lane(int (&rl)[RPL], float (&mv)[RPL], const WalkSel<RPL> &w, const float *M,
                                                  bool has_mean) {
#pragma unroll
    for (int m = 0; m < RPL; ++m) {
        rl[m] = w.sel(m) ? w.rank[m] : 0;
        mv[m] = has_mean ? M[rl[m]] : 0.f;
    }
}

// hi[m][s] = sum_i Uh[rl[m]][i] C[i][c0 + s], lo likewise over the low part: fp32 fma chains from 0 over the columns in
// order -- the per-row arithmetic of k_reconstruct (svdq_basis_ops.hip), so every kernel built on this gives the per-parameter
// route's bits.  Columns outermost: one coefficient read serves the lane's rows, the G x RPL chains are independent.
template <typename T, int G, int RPL>
__device__ __forceinline__ void fma_chains(float (&hi)[RPL][G], float (&lo)[RPL][G], const T *Uh, const T *Ul,
                                           const int (&rl)[RPL], int k, int nl, const float *C, int cstride, int c0) {
#pragma unroll
    for (int m = 0; m < RPL; ++m)
#pragma unroll
        for (int s = 0; s < G; ++s) hi[m][s] = lo[m][s] = 0.f;
    for (int i = 0; i < k; ++i) {
        float c[G];
#pragma unroll
        for (int s = 0; s < G; ++s) c[s] = C[i * cstride + c0 + s];
#pragma unroll
        for (int m = 0; m < RPL; ++m) {
            const float u = u_val(Uh, rl[m] * k + i);
#pragma unroll
            for (int s = 0; s < G; ++s) hi[m][s] = fmaf(u, c[s], hi[m][s]);
        }
    }
    for (int j = 0; j < nl; ++j) {
        float c[G];
#pragma unroll
        for (int s = 0; s < G; ++s) c[s] = C[(k + j) * cstride + c0 + s];
#pragma unroll
        for (int m = 0; m < RPL; ++m) {
            const float u = u_val(Ul, rl[m] * nl + j);
#pragma unroll
            for (int s = 0; s < G; ++s) lo[m][s] = fmaf(u, c[s], lo[m][s]);
        }
    }
}

// ------------------------------------------------------------------------------------ epilogues
// (hi + lo), + mean, * scale: reconstruct_from_coefficients' row (merge.py:144-194)
__device__ __forceinline__ float row_value(float hi, float lo, bool has_mean, float mean, float scale) {
    float v = __fadd_rn(hi, lo);
    if (has_mean) v = __fadd_rn(v, mean);
    return __fmul_rn(v, scale);
}

// the merge kernels' share strip SH[NS]: the share of every set, -1 = the slot holds no set (or there is no share table)
template <int NS>
__device__ __forceinline__ void stage_shares(float *SH, const float *__restrict__ set_share, int per_param, int p,
                                             int n_sets, int lane) {
    if (lane < NS)
        SH[lane] = (set_share && lane < n_sets) ? set_share[(per_param ? (size_t)p * n_sets : 0) + lane] : -1.f;
}

// the merge kernels: the row's NS sets combined with their shares, (stack * w).sum(0) set by set over the sets with
// SH[s] >= 0; without a share table the row of set 0
template <int NS>
__device__ __forceinline__ float combine_sets(const float (&hi)[NS], const float (&lo)[NS], bool has_mean, float mean,
                                              float scale, bool shared, const float *SH) {
    float res = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const float v = row_value(hi[s], lo[s], has_mean, mean, scale);
        if (shared) {
            if (SH[s] >= 0.f) res = __fadd_rn(res, __fmul_rn(v, SH[s]));
        } else if (s == 0) {
            res = v;
        }
    }
    return res;
}

// the task kernels: one task's row; 0 where the source row is not selected; base + delta (merge.py:429-552)
__device__ __forceinline__ float task_value(float hi, float lo, bool has_mean, float mean, float scale, bool sel,
                                            bool has_base, float base) {
    float v = row_value(hi, lo, has_mean, mean, scale);
    v = sel ? v : 0.f;
    if (has_base) v = __fadd_rn(base, v);
    return v;
}
