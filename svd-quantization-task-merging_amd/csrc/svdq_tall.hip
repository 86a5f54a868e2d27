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
// Mask bits: the ballots of sweep B go to the LDS bit image of svdq_store_values.h (MaskImage), and store_mask_words
// there turns a block's image into the words of the packed streams.
//
// The state table (uint64 words; svdq_tall_work_bytes): active [T] set bits per store task | agree [T + 1] rows with
// c = 0 .. T set masks.  Integer counts added by atomics, one flush per unit: no result depends on the order the units
// arrive in.
//
// The coefficient kernel, the live mask, the argument check and the dispatcher are those of svdq_store_values.h too.

#include "svdq_store_values.h"

// ------------------------------------------------------------------------------------ the LDS beyond the streaming carve
// LAM [nop] the lambdas of the slots' store tasks | KC [nop] set bits per slot | AG [T + 1] rows by their count |
// IMG [nop][IW] the block's mask bits per slot (MaskImage).
template <int RPL> struct TallLds : MaskImage<RPL> {
    __host__ __device__ static constexpr int words(int nop, int T) {
        return 2 * nop + (T + 1) + nop * MaskImage<RPL>::IW;
    }
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
    float *const *__restrict__ out_ptrs, uint32_t *const *__restrict__ mask_ptrs, store_u64 *__restrict__ state) {
    using Geo = StreamGeom<U16, RPL>;
    using L = StreamLds<U16, RPL, false>;
    using X = TallLds<RPL>;
    using TU = typename Geo::T;
    constexpr int ES = Geo::ES, RB = Geo::RB, IW = X::IW;
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
    const unsigned live = store_live_mask(slot_task + (size_t)p * n_out, tm, n_out, n, T, lane);
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
                    const store_u64 bal = __ballot(set && 64 * m + lane < rows_blk);
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
            store_mask_words<RPL>(IMG, live, tm, n_out, nop, mask_ptrs, bit_first + rb, rows_blk, lane);
        }
        lds_fence();      // the basis rows and the bit image are rewritten next
    }
    // ---- one flush per unit
    lds_fence();
    for (int j = lane; j < n_out; j += 64)
        if (((live >> j) & 1u) && KC[j]) atomicAdd(&state[tm[j]], (store_u64)KC[j]);
    for (int j = lane; j < T + 1; j += 64)
        if (AG[j]) atomicAdd(&state[T + j], (store_u64)AG[j]);
}

// ------------------------------------------------------------------------------------ entry points
extern "C" int64_t svdq_tall_work_bytes(int32_t n_tasks) {
    if (n_tasks < 1 || n_tasks > SVDQ_MAX_TASKS) return 0;
    return svdq_align_up(((int64_t)2 * n_tasks + 1) * 8, 256);
}

extern "C" int svdq_plan_tall_consensus(const svdq_plan *pl, const int64_t *rows_dev, const void *small, const void *basis,
                                        const float *mean, const int32_t *slot_task, const int32_t *task_map,
                                        int32_t n_out, int32_t n_tasks, const int64_t *bit_base, const float *lambdas,
                                        int32_t min_agree, float scaling, const void *base_ptrs, const void *out_ptrs,
                                        const void *mask_ptrs, void *state, void *work, void *stream) {
    const char *who = "svdq_plan_tall_consensus";
    if (int rc = store_args_ok(who, pl, small, basis, mean, slot_task, task_map, n_out, n_tasks, state, work)) return rc;
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
    return store_stream(who, pl, small, slot_task, task_map, (int)n_out, cbar, st,
                       [&](auto f16_c, auto tg_c, auto rpl_c, const SmallView &sv, int nop) {
                           constexpr bool F16 = f16_c;
                           constexpr int TG = tg_c, RPL = rpl_c;
                           using Plain = StreamLds<F16, RPL, false>;
                           hipLaunchKernelGGL((k_tall_consensus<F16, TG, RPL>), dim3(pl->n_units), dim3(64),
                                              Plain::bytes(n, nop, TallLds<RPL>::words(nop, (int)n_tasks)), st,
                                              pl->d_params, pl->d_units, rows_dev, n, (int)n_out, (int)n_tasks, slot_task,
                                              task_map, sv.k, sv.r, bs, mn, cbar, bit_base, lambdas, (int)min_agree,
                                              scaling, bp, op, mp, reinterpret_cast<store_u64 *>(state));
                       });
}
