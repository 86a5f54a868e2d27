// svdq_tall.hip -- TALL masks and the consensus merge of a store (Wang et al. 2024: "Localizing Task Information for
// Improved Model Merging and Compression") in ONE streaming pass over the basis.  Compiled with -ffp-contract=off like
// svdq_ties.hip and svdq_dare.hip: every product and sum is rounded where the definition (DESIGN.md section 30,
// include/svdq.h at svdq_plan_tall_consensus) rounds.
//
// A task's mask compares its OWN value with the sum of the others at every row, so like TIES and DARE the operation
// cannot be done in coefficient space.  k_tall_consensus is k_ties_merge's structure: one wave per work unit, the
// staging, the one-block prefetch, the LDS image and the fma chains of svdq_merge_stream.h, task groups of TG, RPL rows
// per lane, two sweeps over the task groups per block.  Sweep A adds the values task by task (S); sweep B forms them
// again from the staged rows, subtracts, multiplies, compares, counts per row and ballots.  The value of (row, task) is
// fma_chains + task_value unchanged -- the bits reconstruct_task_vectors writes.  No task model is written.
//
// Mask bits: a lane holds rows lane + 64 m of a block, so the ballot of (slot, m) is 64 consecutive stream bits.  They
// go to an LDS bit image per slot (row q of the block = bit q, least significant first); then lanes build one 32-bit
// stream word each: two image words, a funnel shift by the block's bit offset inside the word, __brev and a byte swap
// (numpy.packbits order inside a little-endian word).  Words wholly inside the block's bit range are stored; the partial
// first and last word -- the only ones another block, unit, parameter or plan can touch -- are atomicOr'ed.
//
// The state table (uint64 words; svdq_tall_work_bytes): active [T] set bits per store task | agree [T + 1] rows with
// c = 0 .. T set masks.  Integer counts added by atomics, one flush per unit: no result depends on the order the units
// arrive in.
//
// k_tall_coeff, tall_live_mask and tall_stream are COPIES of k_ties_coeff, ties_live_mask and ties_stream
// (svdq_ties.hip; svdq_dare.hip holds the second copy), kept here so that those two files are compiled from the text
// they had (the rule of DESIGN.md section 27: share through a header only when every instantiation keeps its resource
// usage; not tried here -- the kernels of a translation unit that is not touched cannot move).  A change to one of the
// three belongs in all three files.

#include "svdq_common.h"
#include "svdq_dispatch.h"
#include "svdq_merge_stream.h"
#include "svdq_small_view.h"
#include "svdq_store_pass.h"

typedef unsigned long long tall_u64;
typedef __attribute__((address_space(1))) uint32_t tall_gu32;

// ------------------------------------------------------------------------------------ coefficients (copy of k_ties_coeff)
// cbar [P][n_out][N]: slot j of parameter p holds the coefficients of plan task slot_task[p][j] exactly as k_task_coeff
// (svdq_merge.hip) leaves them (0 + c * 1, rounded as there); a slot whose task_map entry is < 0 holds zeros.
__global__ __launch_bounds__(64) void k_tall_coeff(int NT, int stages, int n_out, const int32_t *__restrict__ slot_task,
                                                   const int32_t *__restrict__ task_map,
                                                   const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                                   const uint16_t *__restrict__ chigh, const uint8_t *__restrict__ codes,
                                                   const float *__restrict__ scale, const float *__restrict__ zp,
                                                   float *__restrict__ cbar) {
    const int p = blockIdx.x, i = threadIdx.x, n = NT;
    const int k = k_in[p], r = r_in[p];
    if (i >= n) return;
    for (int s = 0; s < n_out; ++s) {
        const int t = slot_task[(size_t)p * n_out + s];
        float acc = 0.f;
        if (i < r && task_map[(size_t)p * n_out + s] >= 0 && (unsigned)t < (unsigned)n)
            acc = __fadd_rn(acc, __fmul_rn(task_coeff(p, t, i, n, k, stages, chigh, codes, scale, zp), 1.f));
        cbar[((size_t)p * n_out + s) * n + i] = acc;
    }
}

// bit j: slot j of the parameter is a live task of the store (wave-uniform; copy of ties_live_mask)
__device__ __forceinline__ unsigned tall_live_mask(const int32_t *__restrict__ st, const int32_t *__restrict__ tm,
                                                   int n_out, int n, int T, int lane) {
    const int j = lane < n_out ? lane : 0;
    return (unsigned)__ballot(lane < n_out && (unsigned)tm[j] < (unsigned)T && (unsigned)st[j] < (unsigned)n);
}

// ------------------------------------------------------------------------------------ the LDS beyond the streaming carve
// LAM [nop] the lambdas of the slots' store tasks | KC [nop] set bits per slot | AG [T + 1] rows by their count |
// IMG [nop][IW] the block's mask bits per slot: word 0 and word IW - 1 stay 0 (what the funnel shift reads before the
// block's first and behind its last row), words 1 .. RB / 32 hold rows 0 .. RB - 1, least significant bit first.
template <int RPL> struct TallLds {
    static constexpr int IW = 2 * RPL + 2;      // words of one slot's image
    static constexpr int NW = 2 * RPL + 1;      // stream words a block's bit range can touch
    __host__ __device__ static constexpr int words(int nop, int T) { return 2 * nop + (T + 1) + nop * IW; }
};

// ------------------------------------------------------------------------------------ sum, masks, consensus, apply
// masks: NULL or [T] streams of 32-bit words; outs: NULL (masks only) or [P] (a NULL entry: that parameter's masks only).
template <bool U16, int TG, int RPL>
__global__ __launch_bounds__(64) void k_tall_consensus(
    const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units, const int64_t *__restrict__ rows_dev, int NT,
    int n_out, int T, const int32_t *__restrict__ slot_task, const int32_t *__restrict__ task_map,
    const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in, const uint8_t *__restrict__ basis,
    const float *__restrict__ meanbuf, const float *__restrict__ cbar, const int64_t *__restrict__ bit_base,
    const float *__restrict__ lambdas, int min_agree, float scaling, const float *const *__restrict__ base_ptrs,
    float *const *__restrict__ out_ptrs, uint32_t *const *__restrict__ mask_ptrs, tall_u64 *__restrict__ state) {
    using Geo = StreamGeom<U16, RPL>;
    using L = StreamLds<U16, RPL, false>;
    using X = TallLds<RPL>;
    using TU = typename Geo::T;
    constexpr int ES = Geo::ES, RB = Geo::RB, IW = X::IW, NW = X::NW;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int lane = threadIdx.x, n = NT;
    const int nop = (n_out + TG - 1) / TG * TG;
    float *C = reinterpret_cast<float *>(lds_raw + L::coeff_off(n));           // [column][nop]
    float *LAM = reinterpret_cast<float *>(lds_raw + L::share_off(n, nop));
    unsigned *KC = reinterpret_cast<unsigned *>(LAM + nop);
    unsigned *AG = KC + nop;
    unsigned *IMG = AG + (T + 1);
    const SvdqUnit ud = units[blockIdx.x];
    const int p = ud.param;
    const UnitView uv = unit_view<ES>(params[p], p, rows_dev, k_in, r_in, basis, meanbuf, base_ptrs);
    const int64_t r_begin = ud.row0;
    int64_t r_end = r_begin + ud.nrows;
    if (r_end > uv.D) r_end = uv.D;
    if (r_begin >= r_end) return;
    mg_gfloat_w *gout = out_ptrs ? (mg_gfloat_w *)out_ptrs[p] : nullptr;      // NULL: the parameter's masks and counts only
    const int32_t *tm = task_map + (size_t)p * n_out;
    const unsigned live = tall_live_mask(slot_task + (size_t)p * n_out, tm, n_out, n, T, lane);
    const int k = uv.k, nl = uv.nl;
    const int64_t bit_first = mask_ptrs ? bit_base[p] : 0;      // the stream bit of the parameter's row 0
    stage_coeffs(C, cbar + (size_t)p * n_out * n, n, n_out, nop, lane);
    for (int j = lane; j < nop; j += 64) {
        LAM[j] = (j < n_out && ((live >> j) & 1u)) ? lambdas[tm[j]] : 0.f;
        KC[j] = 0u;
    }
    for (int j = lane; j < T + 1; j += 64) AG[j] = 0u;
    for (int j = lane; j < nop * IW; j += 64) IMG[j] = 0u;

    f32x4 ureg[Geo::SV];
    float mpf[RPL] = {}, bpf[RPL] = {};
    auto prefetch = [&](int64_t rb) {
        const int nr = block_rows<RB>(rb, r_end);
        ustage_fetch(ureg, ustage_plan<ES>(rb, nr, k, nl), uv.gUh, uv.gUl, lane);
        load_rows(mpf, bpf, uv.gmean, uv.gbase, rb, nr, lane);
    };
    // the block loop written out, as in k_ties_merge
    prefetch(r_begin);
    for (int64_t rb = r_begin; rb < r_end; rb += RB) {
        const int rows_blk = block_rows<RB>(rb, r_end);
        const UStage cur = ustage_plan<ES>(rb, rows_blk, k, nl);
        ustage_commit(lds_raw, ureg, cur, lane);
        float mv[RPL], bv[RPL];
        int rl[RPL];
        block_rows_of_lane(rl, rows_blk, lane);
#pragma unroll
        for (int m = 0; m < RPL; ++m) mv[m] = mpf[m], bv[m] = bpf[m];
        lds_fence();
        if (rb + RB < r_end) prefetch(rb + RB);
        const TU *Uh = ustage_high<TU>(lds_raw, cur), *Ul = ustage_low<TU>(lds_raw, cur);

        // the group's values: what svdq_task_reconstruct writes for the slots' tasks at the lane's rows
        float v[RPL][TG];
        auto group_values = [&](int g0) {
            float hi[RPL][TG], lo[RPL][TG];
            fma_chains<TU, TG, RPL>(hi, lo, Uh, Ul, rl, k, nl, C, nop, g0);
#pragma unroll
            for (int m = 0; m < RPL; ++m)
#pragma unroll
                for (int s = 0; s < TG; ++s)
                    v[m][s] = task_value(hi[m][s], lo[m][s], uv.gmean != nullptr, mv[m], 1.f, true, false, 0.f);
        };
        // ---- sweep A: S = the values of the tasks that have the parameter, added in ascending store order
        float ssum[RPL];
#pragma unroll
        for (int m = 0; m < RPL; ++m) ssum[m] = 0.f;
        for (int g0 = 0; g0 < n_out; g0 += TG) {
            const unsigned gm = (live >> g0) & ((1u << TG) - 1u);
            if (!gm) continue;
            group_values(g0);
#pragma unroll
            for (int s = 0; s < TG; ++s) {
                if (!((gm >> s) & 1u)) continue;      // wave-uniform: a slot that is no live task holds the mean alone
#pragma unroll
                for (int m = 0; m < RPL; ++m) ssum[m] = __fadd_rn(ssum[m], v[m][s]);
            }
        }
        // ---- sweep B: |v_g| > lambda_g * |S - v_g| per slot; the bits, their number per slot and per row
        unsigned cnt[RPL];
#pragma unroll
        for (int m = 0; m < RPL; ++m) cnt[m] = 0u;
        for (int g0 = 0; g0 < n_out; g0 += TG) {
            const unsigned gm = (live >> g0) & ((1u << TG) - 1u);
            if (!gm) continue;
            if (n_out > TG) group_values(g0);      // a single group is still in registers
#pragma unroll
            for (int s = 0; s < TG; ++s) {
                if (!((gm >> s) & 1u)) continue;      // wave-uniform
                const float lam = LAM[g0 + s];
                unsigned kc = 0u;
#pragma unroll
                for (int m = 0; m < RPL; ++m) {
                    const float rest = __fsub_rn(ssum[m], v[m][s]);
                    const bool set = fabsf(v[m][s]) > __fmul_rn(lam, fabsf(rest));
                    if (set) ++cnt[m];
                    const tall_u64 bal = __ballot(set && 64 * m + lane < rows_blk);
                    kc += (unsigned)__popcll(bal);
                    if (lane < 2) IMG[(g0 + s) * IW + 1 + 2 * m + lane] = (unsigned)(bal >> (32 * lane));
                }
                if (lane == 0) KC[g0 + s] += kc;
            }
        }
        // ---- consensus and apply
#pragma unroll
        for (int m = 0; m < RPL; ++m) {
            const bool in = 64 * m + lane < rows_blk;
            float res = __fmul_rn(scaling, (int)cnt[m] >= min_agree ? ssum[m] : 0.f);
            if (uv.gbase) res = __fadd_rn(bv[m], res);
            if (in && gout) gout[rb + 64 * m + lane] = res;
            // cnt <= live slots <= T where the slots name distinct tasks; a table that repeats one must not leave the strip
            if (in) atomicAdd(&AG[(int)cnt[m] < T ? (int)cnt[m] : T], 1u);
        }
        // ---- the block's stream words
        if (mask_ptrs) {
            lds_fence();      // the image is read by other lanes
            const int64_t b0 = bit_first + rb, b1 = b0 + rows_blk;      // the block's bit range [b0, b1)
            const int64_t w0 = b0 >> 5;
            const int sh = (int)(b0 & 31);
            const int nw = (int)(((b1 - 1) >> 5) - w0) + 1;      // <= NW
            for (int e = lane; e < nop * NW; e += 64) {
                const int j = e / NW, wi = e % NW;
                if (j >= n_out || !((live >> j) & 1u) || wi >= nw) continue;
                // stream bits 32 (w0 + wi) + i, i = 0 .. 31, are rows 32 wi + i - sh of the block
                const tall_u64 pair = ((tall_u64)IMG[j * IW + wi + 1] << 32) | IMG[j * IW + wi];
                const unsigned x = (unsigned)(pair >> (32 - sh));
                // bit i -> bit 7 - (i & 7) of byte i >> 3 of a little-endian word
                const unsigned word = __builtin_bswap32(__brev(x));
                // the address space named (the reason is at mg_gfloat in svdq_merge_stream.h): a flat store here would
                // make the fence below wait for HBM once per block
                tall_gu32 *dst = (tall_gu32 *)mask_ptrs[tm[j]] + (w0 + wi);
                const bool whole = 32 * (w0 + wi) >= b0 && 32 * (w0 + wi) + 32 <= b1;
                if (whole)
                    *dst = word;
                else if (word)
                    __hip_atomic_fetch_or(dst, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        lds_fence();      // the basis rows and the bit image are rewritten next
    }
    // ---- one flush per unit
    lds_fence();
    for (int j = lane; j < n_out; j += 64)
        if (((live >> j) & 1u) && KC[j]) atomicAdd(&state[tm[j]], (tall_u64)KC[j]);
    for (int j = lane; j < T + 1; j += 64)
        if (AG[j]) atomicAdd(&state[T + j], (tall_u64)AG[j]);
}

// ------------------------------------------------------------------------------------ entry points
extern "C" int64_t svdq_tall_work_bytes(int32_t n_tasks) {
    if (n_tasks < 1 || n_tasks > SVDQ_MAX_TASKS) return 0;
    return svdq_align_up(((int64_t)2 * n_tasks + 1) * 8, 256);
}

// the live tasks' coefficients, then `launch` with the compiled-in basis type, task group and rows per lane (copy of
// ties_stream)
template <typename F>
static int tall_stream(const char *who, const svdq_plan *pl, const void *small, const int32_t *slot_task,
                       const int32_t *task_map, int n_out, float *cbar, hipStream_t st, F &&launch) {
    const SmallView sv = small_view(pl->small, small);
    hipLaunchKernelGGL(k_tall_coeff, dim3(pl->n_params), dim3(64), 0, st, pl->n_tasks, pl->cfg.rtvq_stages, n_out,
                       slot_task, task_map, sv.k, sv.r, sv.chigh, sv.codes, sv.scale, sv.zp, cbar);
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

extern "C" int svdq_plan_tall_consensus(const svdq_plan *pl, const int64_t *rows_dev, const void *small, const void *basis,
                                        const float *mean, const int32_t *slot_task, const int32_t *task_map,
                                        int32_t n_out, int32_t n_tasks, const int64_t *bit_base, const float *lambdas,
                                        int32_t min_agree, float scaling, const void *base_ptrs, const void *out_ptrs,
                                        const void *mask_ptrs, void *state, void *work, void *stream) {
    const char *who = "svdq_plan_tall_consensus";
    if (!pl || !small || !basis || !slot_task || !task_map || !state || !work) {
        svdq_set_error("%s: plan, small, basis, slot_task, task_map, state and work are required", who);
        return SVDQ_EINVAL;
    }
    if (n_out < 1 || n_out > SVDQ_MAX_TASKS || n_tasks < 1 || n_tasks > SVDQ_MAX_TASKS) {
        svdq_set_error("%s: n_out and n_tasks must be in [1, %d], got %d and %d", who, SVDQ_MAX_TASKS, n_out, n_tasks);
        return SVDQ_EINVAL;
    }
    if (svdq_refuse_no_mean(who, pl, mean)) return SVDQ_EINVAL;
    if (!bit_base || !lambdas) {
        svdq_set_error("%s: bit_base and lambdas are required", who);
        return SVDQ_EINVAL;
    }
    if (!out_ptrs && !mask_ptrs) {
        svdq_set_error("%s: out_ptrs and mask_ptrs are both NULL: nothing to write", who);
        return SVDQ_EINVAL;
    }
    if (min_agree < 0 || min_agree > n_tasks) {
        svdq_set_error("%s: min_agree must be in [0, n_tasks = %d], got %d", who, n_tasks, min_agree);
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const int n = pl->n_tasks;
    const uint8_t *bs = reinterpret_cast<const uint8_t *>(basis);
    const float *mn = pl->cfg.center ? mean : nullptr;
    float *cbar = reinterpret_cast<float *>(work);
    auto bp = reinterpret_cast<const float *const *>(base_ptrs);
    auto op = reinterpret_cast<float *const *>(out_ptrs);
    auto mp = reinterpret_cast<uint32_t *const *>(mask_ptrs);
    return tall_stream(who, pl, small, slot_task, task_map, (int)n_out, cbar, st,
                       [&](auto f16_c, auto tg_c, auto rpl_c, const SmallView &sv, int nop) {
                           constexpr bool F16 = f16_c;
                           constexpr int TG = tg_c, RPL = rpl_c;
                           using Plain = StreamLds<F16, RPL, false>;
                           hipLaunchKernelGGL((k_tall_consensus<F16, TG, RPL>), dim3(pl->n_units), dim3(64),
                                              Plain::bytes(n, nop, TallLds<RPL>::words(nop, (int)n_tasks)), st,
                                              pl->d_params, pl->d_units, rows_dev, n, (int)n_out, (int)n_tasks, slot_task,
                                              task_map, sv.k, sv.r, bs, mn, cbar, bit_base, lambdas, (int)min_agree,
                                              scaling, bp, op, mp, reinterpret_cast<tall_u64 *>(state));
                       });
}
