// svdq_dare.hip -- the drop-and-rescale (DARE, Yu et al. 2024: "Language Models are Super Mario") merge of a store in ONE
// streaming pass over the basis; with drop threshold 0 the same launch is plain task arithmetic.  Compiled with
// -ffp-contract=off like svdq_ties.hip: every product and sum is rounded where the definition (DESIGN.md section 28,
// include/svdq.h at svdq_plan_dare_merge) rounds.
//
// The mask acts on every task's OWN value at every row, so like TIES the merge cannot be done in coefficient space.
// k_dare_merge is k_ties_merge's structure with one sweep in place of two: one wave per work unit, the staging, the
// one-block prefetch, the LDS image and the fma chains of svdq_merge_stream.h, task groups of TG, RPL rows per lane.  The
// value of (row, task) is fma_chains + task_value unchanged -- the bits reconstruct_task_vectors writes -- and the
// epilogue is a counter-based draw (svdq_philox.h), a division, a product and a sum.  No task model is written.
//
// The state table (uint64 words; svdq_dare_work_bytes): kept [T], the values kept per store task.  Integer counts added
// by atomics, one flush per unit: no result depends on the order the units arrive in.
//
// The coefficient kernel, the live mask, the argument check and the dispatcher are those of svdq_store_values.h.

#include "svdq_philox.h"
#include "svdq_store_values.h"

// ------------------------------------------------------------------------------------ draw, rescale, combine, apply
// LDS beyond the streaming carve: W [nop] the weights of the slots' store tasks (0 on a slot that is no live task), KC [nop]
// kept counts.  key0 / key1: the two halves of the seed; thr: a value is dropped iff its Philox word < thr (0 = nothing is
// dropped and the generator is skipped: wave-uniform); keep_scale: q, 0 = kept values are not divided.
template <bool U16, int TG, int RPL>
__global__ __launch_bounds__(64) void k_dare_merge(const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units,
                                                   const int64_t *__restrict__ rows_dev, int NT, int n_out, int T,
                                                   const int32_t *__restrict__ slot_task,
                                                   const int32_t *__restrict__ task_map,
                                                   const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                                   const uint8_t *__restrict__ basis, const float *__restrict__ meanbuf,
                                                   const float *__restrict__ cbar, const int64_t *__restrict__ row_base,
                                                   const float *__restrict__ weights, uint32_t key0, uint32_t key1,
                                                   uint32_t thr, float keep_scale, float scaling,
                                                   const float *const *__restrict__ base_ptrs,
                                                   float *const *__restrict__ out_ptrs, store_u64 *__restrict__ state) {
    using Geo = StreamGeom<U16, RPL>;
    using L = StreamLds<U16, RPL, false>;
    using TU = typename Geo::T;
    constexpr int ES = Geo::ES, RB = Geo::RB;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int lane = threadIdx.x, n = NT;
    const int nop = (n_out + TG - 1) / TG * TG;
    float *C = reinterpret_cast<float *>(lds_raw + L::coeff_off(n));           // [column][nop]
    float *W = reinterpret_cast<float *>(lds_raw + L::share_off(n, nop));
    unsigned *KC = reinterpret_cast<unsigned *>(W + nop);
    const SvdqUnit ud = units[blockIdx.x];
    const int p = ud.param;
    const UnitView uv = unit_view<ES>(params[p], p, rows_dev, k_in, r_in, basis, meanbuf, base_ptrs);
    const int64_t r_begin = ud.row0;
    int64_t r_end = r_begin + ud.nrows;
    if (r_end > uv.D) r_end = uv.D;
    if (r_begin >= r_end) return;
    mg_gfloat_w *gout = (mg_gfloat_w *)out_ptrs[p];
    if (!gout) return;
    const int32_t *tm = task_map + (size_t)p * n_out;
    const unsigned live = store_live_mask(slot_task + (size_t)p * n_out, tm, n_out, n, T, lane);
    const int k = uv.k, nl = uv.nl;
    const int64_t g_first = row_base[p];      // the global row of the parameter's row 0
    const bool divide = keep_scale != 0.f && keep_scale != 1.f;      // v / 1 is v: task arithmetic divides nothing
    stage_coeffs(C, cbar + (size_t)p * n_out * n, n, n_out, nop, lane);
    for (int j = lane; j < nop; j += 64) {
        W[j] = (j < n_out && ((live >> j) & 1u)) ? weights[tm[j]] : 0.f;
        KC[j] = 0u;
    }

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

        float msum[RPL];
#pragma unroll
        for (int m = 0; m < RPL; ++m) msum[m] = 0.f;
        for (int g0 = 0; g0 < n_out; g0 += TG) {
            const unsigned gm = (live >> g0) & ((1u << TG) - 1u);
            if (!gm) continue;
            float hi[RPL][TG], lo[RPL][TG];
            fma_chains<TU, TG, RPL>(hi, lo, Uh, Ul, rl, k, nl, C, nop, g0);
            unsigned kc[TG];      // the group's kept counts of this block: wave-uniform, one LDS update per slot below
#pragma unroll
            for (int s = 0; s < TG; ++s) kc[s] = 0u;
#pragma unroll
            for (int m = 0; m < RPL; ++m) {
                const bool in = 64 * m + lane < rows_blk;
                const uint64_t grow = (uint64_t)(g_first + rb + 64 * m + lane);      // G; past the block's end: not used
                // the Philox block of (G, quad): live slots name store tasks in ascending order, so a quad's block is
                // computed once and kept while the following slots share it
                uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
                int quad = -1;      // wave-uniform
#pragma unroll
                for (int s = 0; s < TG; ++s) {
                    if (!((gm >> s) & 1u)) continue;      // wave-uniform
                    const float v = task_value(hi[m][s], lo[m][s], uv.gmean != nullptr, mv[m], 1.f, true, false, 0.f);
                    bool kept = true;
                    if (thr) {      // wave-uniform
                        const int g = tm[g0 + s];
                        if ((g >> 2) != quad) {
                            quad = g >> 2;
                            philox4x32_10((uint32_t)grow, (uint32_t)(grow >> 32), (uint32_t)quad, 0u, key0, key1, w0, w1, w2,
                                          w3);
                        }
                        const int j = g & 3;
                        const uint32_t word = j == 0 ? w0 : (j == 1 ? w1 : (j == 2 ? w2 : w3));
                        kept = word >= thr;
                    }
                    const float x = divide ? __fdiv_rn(v, keep_scale) : v;
                    if (kept) msum[m] = __fadd_rn(msum[m], __fmul_rn(W[g0 + s], x));
                    kc[s] += (unsigned)__popcll(__ballot(kept && in));
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int s = 0; s < TG; ++s)
                    if ((gm >> s) & 1u) KC[g0 + s] += kc[s];
            }
        }
        // ---- apply
#pragma unroll
        for (int m = 0; m < RPL; ++m) {
            float res = __fmul_rn(scaling, msum[m]);
            if (uv.gbase) res = __fadd_rn(bv[m], res);
            if (64 * m + lane < rows_blk) gout[rb + 64 * m + lane] = res;
        }
        lds_fence();      // the basis rows are rewritten next
    }
    // ---- one flush per unit
    lds_fence();
    for (int j = lane; j < n_out; j += 64)
        if (((live >> j) & 1u) && KC[j]) atomicAdd(&state[tm[j]], (store_u64)KC[j]);
}

// ------------------------------------------------------------------------------------ entry points
extern "C" int64_t svdq_dare_work_bytes(int32_t n_tasks) {
    if (n_tasks < 1 || n_tasks > SVDQ_MAX_TASKS) return 0;
    return svdq_align_up((int64_t)n_tasks * 8, 256);
}

extern "C" int svdq_plan_dare_merge(const svdq_plan *pl, const int64_t *rows_dev, const void *small, const void *basis,
                                    const float *mean, const int32_t *slot_task, const int32_t *task_map, int32_t n_out,
                                    int32_t n_tasks, const int64_t *row_base, const float *weights, uint64_t seed,
                                    uint32_t drop_threshold, float keep_scale, float scaling, const void *base_ptrs,
                                    const void *out_ptrs, void *state, void *work, void *stream) {
    const char *who = "svdq_plan_dare_merge";
    if (int rc = store_args_ok(who, pl, small, basis, mean, slot_task, task_map, n_out, n_tasks, state, work)) return rc;
    if (!row_base || !weights || !out_ptrs) {
        svdq_set_error("%s: row_base, weights and out_ptrs are required", who);
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const int n = pl->n_tasks;
    const uint8_t *bs = reinterpret_cast<const uint8_t *>(basis);
    const float *mn = pl->cfg.center ? mean : nullptr;
    float *cbar = reinterpret_cast<float *>(work);
    auto bp = reinterpret_cast<const float *const *>(base_ptrs);
    auto op = reinterpret_cast<float *const *>(out_ptrs);
    const uint32_t key0 = (uint32_t)(seed & 0xffffffffull), key1 = (uint32_t)(seed >> 32);
    return store_stream(who, pl, small, slot_task, task_map, (int)n_out, cbar, st,
                       [&](auto f16_c, auto tg_c, auto rpl_c, const SmallView &sv, int nop) {
                           constexpr bool F16 = f16_c;
                           constexpr int TG = tg_c, RPL = rpl_c;
                           using Plain = StreamLds<F16, RPL, false>;
                           hipLaunchKernelGGL((k_dare_merge<F16, TG, RPL>), dim3(pl->n_units), dim3(64),
                                              Plain::bytes(n, nop, 2 * nop), st, pl->d_params, pl->d_units, rows_dev, n,
                                              (int)n_out, (int)n_tasks, slot_task, task_map, sv.k, sv.r, bs, mn, cbar,
                                              row_base, weights, key0, key1, drop_threshold, keep_scale, scaling, bp, op,
                                              reinterpret_cast<store_u64 *>(state));
                       });
}
