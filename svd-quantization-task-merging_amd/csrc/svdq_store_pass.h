// svdq_store_pass.h -- the pieces the passes over a plan's STORED artifacts share: k_plan_project (svdq_plan_project.hip),
// the two streaming passes of svdq_plan_extend.hip, k_store_gram (svdq_store_gram.hip), k_plan_rebase
// (svdq_consolidate.hip), their per-parameter finish / eigen kernels and their launchers.  On top of
// svdq_merge_stream.h's staging: what of a stored plan a unit reads (k and r held to the slab, the rows held to the
// plan's), where a basis column sits in a block's staged image, the block loop, and the geometry the launcher and the
// kernel must agree on.  DESIGN.md section 27 lists who uses what, and what kept its own text.
#pragma once

#include "svdq_merge_stream.h"

// ------------------------------------------------------------------------------------ what a unit reads of the plan
// k and r as every consumer reads them, held to what the slab has room for (svdq_plan_import's rule)
__device__ __forceinline__ void plan_ranks(const int32_t *k_in, const int32_t *r_in, int p, int64_t rows, int n, int &k,
                                           int &r) {
    const int64_t rmax = rows < n ? rows : n;
    int64_t rr = r_in[p], kk = k_in[p];
    rr = rr < 0 ? 0 : (rr > rmax ? rmax : rr);
    kk = kk < 0 ? 0 : (kk > rr ? rr : kk);
    k = (int)kk;
    r = (int)rr;
}

// the rows of parameter p that were processed: rows_dev's count, never more than the plan laid the slab out for
__device__ __forceinline__ int64_t plan_rows_of(const SvdqParam &pd, const int64_t *__restrict__ rows_dev, int p) {
    const int64_t D = rows_dev ? rows_dev[p] : pd.rows;
    return D > pd.rows ? pd.rows : D;
}

// One work unit's view of a stored plan: rows [cpos, cend) of the D the parameter has; k, r (plan_ranks; 0 on a unit
// without rows, which then reads nothing of the small buffer) and nl = r - k; the two parts of the slab; the mean (NULL =
// not centred).  unit_view (svdq_merge_stream.h) is the same split without the clamps, for callers checked on the host.
struct StoreUnit {
    int64_t D, cpos, cend;
    int k, r, nl;
    const uint8_t *gUh, *gUl;
    mg_gfloat *gmean;
};
template <int ES>
__device__ __forceinline__ StoreUnit store_unit(const SvdqParam &pd, const SvdqUnit &ud, int p, int64_t D, int n,
                                                const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                                const uint8_t *__restrict__ basis, const float *__restrict__ meanbuf) {
    StoreUnit s;
    s.D = D;
    s.cpos = ud.row0;
    s.cend = ud.row0 + ud.nrows;
    if (s.cend > D) s.cend = D;
    s.k = s.r = 0;
    if (s.cpos < s.cend) plan_ranks(k_in, r_in, p, D, n, s.k, s.r);
    s.nl = s.r - s.k;
    s.gUh = basis + pd.slab_off;
    s.gUl = SVDQ_SLAB_LOW(s.gUh, D, s.k, ES);
    s.gmean = meanbuf ? (mg_gfloat *)(meanbuf + pd.mean_off) : nullptr;
    return s;
}

// ------------------------------------------------------------------------------------ the staged image, by column
// one element of the staged image as fp32
__device__ __forceinline__ float lds_u(const uint8_t *lds, int byte_off, __half) {
    return __half2float(*reinterpret_cast<const __half *>(lds + byte_off));
}
__device__ __forceinline__ float lds_u(const uint8_t *lds, int byte_off, float) {
    return *reinterpret_cast<const float *>(lds + byte_off);
}

// where column c (< r) of the basis sits in a block's staged image: byte offset of its element of the block's row 0, and
// the byte stride from row to row
__device__ __forceinline__ void ustage_column(const UStage &cur, int c, int k, int nl, int es, int &off, int &stride) {
    const bool hi = c < k;
    const int w = hi ? k : nl;
    stride = w * es;
    off = (hi ? cur.offh * es : 16 * cur.nvh + cur.offl * es) + (hi ? c : c - k) * es;
}

// ------------------------------------------------------------------------------------ the block loop
// The blocks of RB rows of [cpos, cend), cpos < cend, with the next block's loads in flight during compute.
//   prefetch(c0)              the loads of the block that starts at c0, into registers
//   stage(cur, nr)            registers -> LDS: ustage_commit and whatever the kernel parks in LDS or registers
//   body(cur, c0, nr, more)   the block's compute; the next block's loads have been issued
// The fence after a block (its LDS image is rewritten next) is skipped after the last one.
template <int RB, int ES, typename Prefetch, typename Stage, typename Body>
__device__ __forceinline__ void stream_blocks(int64_t cpos, int64_t cend, int k, int nl, Prefetch &&prefetch, Stage &&stage,
                                              Body &&body) {
    prefetch(cpos);
    while (true) {
        const int nr = block_rows<RB>(cpos, cend);
        const UStage cur = ustage_plan<ES>(cpos, nr, k, nl);
        stage(cur, nr);
        lds_fence();
        const bool more = cpos + RB < cend;
        if (more) prefetch(cpos + RB);
        body(cur, cpos, nr, more);
        if (!more) break;
        cpos += RB;
        lds_fence();
    }
}

// ------------------------------------------------------------------------------------ geometry: launcher == kernel
// the instantiation a slot count n is launched with: 8, 16 or 32 task slots / basis columns
__host__ __device__ constexpr int svdq_slot_class(int n) { return n <= 8 ? 8 : (n <= 16 ? 16 : 32); }
// rows per lane and per block of a slot class: 256 rows up to 16 slots, 128 above
__host__ __device__ constexpr int store_rpl(int cls) { return cls > 16 ? 2 : 4; }
__host__ __device__ constexpr int store_rb(int cls) { return 64 * store_rpl(cls); }
// 16-byte vectors of one block's basis rows per lane
__host__ __device__ constexpr int store_sv(int cls, int es) { return (store_rb(cls) * cls * es / 16 + 2 + 63) / 64; }

// ------------------------------------------------------------------------------------ refusals
// Each sets the error text and returns true when the call is to be refused with SVDQ_EINVAL.
static inline bool svdq_refuse_no_mean(const char *who, const svdq_plan *pl, const float *mean) {
    if (!pl->cfg.center || mean) return false;
    svdq_set_error("%s: mean is required on a centred plan", who);
    return true;
}
template <typename... P> static inline uintptr_t svdq_addr_bits(P... p) { return (uintptr_t(0) | ... | (uintptr_t)p); }
// bits: svdq_addr_bits of the pointers; `list` (+ `tail`) names them in the message
static inline bool svdq_refuse_unaligned(const char *who, uintptr_t bits, int align, const char *list,
                                         const char *tail = "") {
    if (!(bits & (uintptr_t)(align - 1))) return false;
    svdq_set_error("%s: %s%s must be %d-byte aligned", who, list, tail, align);
    return true;
}
