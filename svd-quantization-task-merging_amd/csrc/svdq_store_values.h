// svdq_store_values.h -- the pieces the merges that need every task's OWN value at every row share: the TIES, DARE,
// TALL / consensus and EMR merges of a store (svdq_ties.hip, svdq_dare.hip, svdq_tall.hip, svdq_emr.hip).  On top of
// svdq_store_pass.h: which slots of a parameter are live tasks, the packed mask stream a block writes (the bit image's
// geometry and the word writer of k_tall_consensus and k_emr_elect), and the host front of every entry point -- the
// argument check, the coefficient launch and the dispatch over (basis type, task group, rows per lane).  The text that
// must exist once (k_store_coeff, the check) is in svdq_store_values.hip.  The block loop, group_values and sweep A stay
// written out in each kernel.  DESIGN.md section 32 lists who uses what, and what kept its own text.
#pragma once

#include "svdq_common.h"
#include "svdq_dispatch.h"
#include "svdq_merge_stream.h"
#include "svdq_small_view.h"
#include "svdq_store_pass.h"

typedef unsigned long long store_u64;
typedef __attribute__((address_space(1))) uint32_t store_gu32;

// ------------------------------------------------------------------------------------ the live slots
// bit j: slot j of the parameter is a live task of the store (wave-uniform)
__device__ __forceinline__ unsigned store_live_mask(const int32_t *__restrict__ st, const int32_t *__restrict__ tm,
                                                    int n_out, int n, int T, int lane) {
    const int j = lane < n_out ? lane : 0;
    return (unsigned)__ballot(lane < n_out && (unsigned)tm[j] < (unsigned)T && (unsigned)st[j] < (unsigned)n);
}

// ------------------------------------------------------------------------------------ the packed mask stream
// A lane holds rows lane + 64 m of a block, so the ballot of (slot, m) is 64 consecutive stream bits.  They go to an LDS
// bit image per slot, IMG [nop][IW]: word 0 and word IW - 1 stay 0 (what the funnel shift reads before the block's first
// and behind its last row), words 1 .. RB / 32 hold rows 0 .. RB - 1, least significant bit first.
template <int RPL> struct MaskImage {
    static constexpr int IW = 2 * RPL + 2;      // words of one slot's image
    static constexpr int NW = 2 * RPL + 1;      // stream words a block's bit range can touch
};

// The block's stream words from its image (fenced by the caller: the image is read by other lanes): lanes build one
// 32-bit stream word each -- two image words, a funnel shift by the block's bit offset inside the word, __brev and a
// byte swap.  b0: the stream bit of the block's row 0.  Words wholly inside the block's bit range are stored; the partial
// first and last word -- the only ones another block, unit, parameter or plan can touch -- are atomicOr'ed.
template <int RPL>
__device__ __forceinline__ void store_mask_words(const unsigned *IMG, unsigned live, const int32_t *tm, int n_out, int nop,
                                                 uint32_t *const *__restrict__ mask_ptrs, int64_t b0, int rows_blk,
                                                 int lane) {
    constexpr int IW = MaskImage<RPL>::IW, NW = MaskImage<RPL>::NW;
    const int64_t b1 = b0 + rows_blk;      // the block's bit range [b0, b1)
    const int64_t w0 = b0 >> 5;
    const int sh = (int)(b0 & 31);
    const int nw = (int)(((b1 - 1) >> 5) - w0) + 1;      // <= NW
    for (int e = lane; e < nop * NW; e += 64) {
        const int j = e / NW, wi = e % NW;
        if (j >= n_out || !((live >> j) & 1u) || wi >= nw) continue;
        // stream bits 32 (w0 + wi) + i, i = 0 .. 31, are rows 32 wi + i - sh of the block
        const store_u64 pair = ((store_u64)IMG[j * IW + wi + 1] << 32) | IMG[j * IW + wi];
        const unsigned x = (unsigned)(pair >> (32 - sh));
        // bit i -> bit 7 - (i & 7) of byte i >> 3 of a little-endian word (numpy.packbits order)
        const unsigned word = __builtin_bswap32(__brev(x));
        // the address space named (the reason is at mg_gfloat in svdq_merge_stream.h): a flat store here would make the
        // caller's next fence wait for HBM once per block
        store_gu32 *dst = (store_gu32 *)mask_ptrs[tm[j]] + (w0 + wi);
        const bool whole = 32 * (w0 + wi) >= b0 && 32 * (w0 + wi) + 32 <= b1;
        if (whole)
            *dst = word;
        else if (word)
            __hip_atomic_fetch_or(dst, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------------------------ the host front of an entry point
// What every entry point checks first, in this order: the required pointers, the range of n_out and n_tasks, the mean of
// a centred plan.  SVDQ_OK, or SVDQ_EINVAL with the error text set.
int store_args_ok(const char *who, const svdq_plan *pl, const void *small, const void *basis, const float *mean,
                  const int32_t *slot_task, const int32_t *task_map, int32_t n_out, int32_t n_tasks, const void *state,
                  const void *work);

// cbar [P][n_out][N] on `st`: slot j of parameter p holds the coefficients of plan task slot_task[p][j] exactly as
// k_task_coeff (svdq_merge.hip) leaves them; a slot whose task_map entry is < 0 holds zeros
void store_coeff_launch(const svdq_plan *pl, const SmallView &sv, const int32_t *slot_task, const int32_t *task_map,
                        int n_out, float *cbar, hipStream_t st);

// the live tasks' coefficients, then `launch` with the compiled-in basis type, task group and rows per lane
template <typename F>
static int store_stream(const char *who, const svdq_plan *pl, const void *small, const int32_t *slot_task,
                        const int32_t *task_map, int n_out, float *cbar, hipStream_t st, F &&launch) {
    const SmallView sv = small_view(pl->small, small);
    store_coeff_launch(pl, sv, slot_task, task_map, n_out, cbar, st);
    const int tg = n_out == 1 ? 1 : (n_out <= 4 ? 4 : 8);      // tasks per pass over a block's LDS image
    const int rpl = pl->n_tasks <= 16 ? 4 : 2;
    const bool ok = svdq_dispatch_bool(pl->cfg.fp16 != 0, [&](auto f16_c) {
        return svdq_dispatch_int<1, 4, 8>(tg, [&](auto tg_c) {
            return svdq_dispatch_int<4, 2>(rpl, [&](auto rpl_c) {
                launch(f16_c, tg_c, rpl_c, sv, (n_out + tg - 1) / tg * tg);
                return true;
            });
        });
    });
    return svdq_launch_status(ok, who);
}
