// svdq_ties.hip -- the sign-elected (TIES, Yadav et al. 2023: topk_values_mask -> resolve_sign -> disjoint_merge) merge of
// a store, in streaming passes over the basis.  Compiled with -ffp-contract=off like svdq_merge.hip: every product and
// sum is rounded where the definition (include/svdq.h) rounds.
//
// Trim and sign election are element-wise and non-linear, so the merge needs every task's OWN value at every row --
// what k_task_reconstruct (svdq_merge.hip) forms in registers from one staged block of basis rows.  The two streaming
// kernels below are that kernel with another epilogue: one wave per work unit, the staging, one-block prefetch, LDS
// image and fma chains of svdq_merge_stream.h, task groups of TG, RPL rows per lane.  The value of (row, task) is
// fma_chains + task_value unchanged, so every pass sees the bits reconstruct_task_vectors writes -- and no task model is
// ever written.
//
//   k_store_coeff       the live tasks' coefficients per parameter, in the order of the store's task list
//                       (svdq_store_values.hip, launched by store_stream)
//   k_ties_hist         one digit of the radix selection of tau_t (the j-th smallest |v_t| over the whole store): the
//                       magnitudes whose upper bits equal the task's prefix so far are counted per digit value in an LDS
//                       histogram, flushed once per unit into the store's [T][256] table with integer atomics
//   k_ties_select_step  one small block: per task the bin that holds the wanted rank, appended to the prefix
//   k_ties_merge        elect (sweep A over the task groups), merge (sweep B, the staged rows read again from LDS), apply
//
// The state table (uint64 words, T tasks; svdq_ties_work_bytes): hist [T][256] | prefix [T] (after the last digit: the bit
// pattern of tau_t) | rank [T] (1-based from below among the candidates left) | kept [T] | rows with kept values of both
// signs | rows with nothing kept.  Integer counts only: no result depends on the order the units arrive in.

#include "svdq_store_values.h"

#define TIES_BINS 256
#define TIES_DIGIT_BITS 8
#define TIES_DIGITS SVDQ_TIES_DIGITS      // 4: 31 magnitude bits, 8 per pass from the top (the first digit's top bit is always 0)

__host__ __device__ constexpr int64_t ties_prefix_off(int T) { return (int64_t)T * TIES_BINS; }
__host__ __device__ constexpr int64_t ties_rank_off(int T) { return ties_prefix_off(T) + T; }
__host__ __device__ constexpr int64_t ties_kept_off(int T) { return ties_rank_off(T) + T; }
__host__ __device__ constexpr int64_t ties_conflict_off(int T) { return ties_kept_off(T) + T; }
__host__ __device__ constexpr int64_t ties_empty_off(int T) { return ties_conflict_off(T) + 1; }
__host__ __device__ constexpr int64_t ties_words(int T) { return ties_empty_off(T) + 1; }

// ------------------------------------------------------------------------------------ one digit of the selection
// LDS beyond the streaming carve: H [nop][256] uint32 (a unit has fewer than 2^31 rows).
template <bool U16, int TG, int RPL>
__global__ __launch_bounds__(64) void k_ties_hist(const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units,
                                                  const int64_t *__restrict__ rows_dev, int NT, int n_out, int T,
                                                  const int32_t *__restrict__ slot_task,
                                                  const int32_t *__restrict__ task_map,
                                                  const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                                  const uint8_t *__restrict__ basis, const float *__restrict__ meanbuf,
                                                  const float *__restrict__ cbar, int digit, store_u64 *__restrict__ state) {
    using G = StreamGeom<U16, RPL>;
    using L = StreamLds<U16, RPL, false>;
    using TU = typename G::T;
    constexpr int ES = G::ES, RB = G::RB;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int lane = threadIdx.x, n = NT;
    const int nop = (n_out + TG - 1) / TG * TG;
    float *C = reinterpret_cast<float *>(lds_raw + L::coeff_off(n));           // [column][nop]
    unsigned *H = reinterpret_cast<unsigned *>(lds_raw + L::share_off(n, nop));      // [nop][256]
    const SvdqUnit ud = units[blockIdx.x];
    const int p = ud.param;
    const UnitView uv = unit_view<ES>(params[p], p, rows_dev, k_in, r_in, basis, meanbuf, nullptr);
    const int64_t r_begin = ud.row0;
    int64_t r_end = r_begin + ud.nrows;
    if (r_end > uv.D) r_end = uv.D;
    if (r_begin >= r_end) return;
    const int32_t *tm = task_map + (size_t)p * n_out;
    const unsigned live = store_live_mask(slot_task + (size_t)p * n_out, tm, n_out, n, T, lane);
    if (!live) return;
    const int k = uv.k, nl = uv.nl;
    stage_coeffs(C, cbar + (size_t)p * n_out * n, n, n_out, nop, lane);
    for (int e = lane; e < nop * TIES_BINS; e += 64) H[e] = 0u;
    const int shift = 32 - TIES_DIGIT_BITS * (digit + 1);      // 24, 16, 8, 0
    const unsigned upper = digit ? 0xffffffffu << (shift + TIES_DIGIT_BITS) : 0u;      // the bits of the earlier digits

    f32x4 ureg[G::SV];
    float mpf[RPL] = {}, bpf[RPL] = {};
    auto prefetch = [&](int64_t rb) {
        const int nr = block_rows<RB>(rb, r_end);
        ustage_fetch(ureg, ustage_plan<ES>(rb, nr, k, nl), uv.gUh, uv.gUl, lane);
        load_rows(mpf, bpf, uv.gmean, uv.gbase, rb, nr, lane);
    };
    float mv[RPL];
    auto stage = [&](const UStage &cur, int) {
        ustage_commit(lds_raw, ureg, cur, lane);
#pragma unroll
        for (int m = 0; m < RPL; ++m) mv[m] = mpf[m];
    };
    stream_blocks<RB, ES>(r_begin, r_end, k, nl, prefetch, stage, [&](const UStage &cur, int64_t, int rows_blk, bool) {
        int rl[RPL];
        block_rows_of_lane(rl, rows_blk, lane);
        const TU *Uh = ustage_high<TU>(lds_raw, cur), *Ul = ustage_low<TU>(lds_raw, cur);
        for (int g0 = 0; g0 < n_out; g0 += TG) {
            const unsigned gm = (live >> g0) & ((1u << TG) - 1u);
            if (!gm) continue;
            float hi[RPL][TG], lo[RPL][TG];
            fma_chains<TU, TG, RPL>(hi, lo, Uh, Ul, rl, k, nl, C, nop, g0);
#pragma unroll
            for (int s = 0; s < TG; ++s) {
                if (!((gm >> s) & 1u)) continue;      // wave-uniform
                // the task's prefix so far: the magnitude bits above this digit (0 before the first digit)
                const unsigned prefix = digit ? (unsigned)state[ties_prefix_off(T) + tm[g0 + s]] : 0u;
                unsigned *Hs = H + (g0 + s) * TIES_BINS;
#pragma unroll
                for (int m = 0; m < RPL; ++m) {
                    const float v = task_value(hi[m][s], lo[m][s], uv.gmean != nullptr, mv[m], 1.f, true, false, 0.f);
                    const unsigned mag = __float_as_uint(v) & 0x7fffffffu;
                    const bool in = 64 * m + lane < rows_blk && ((mag ^ prefix) & upper) == 0u;
                    const unsigned d = (mag >> shift) & (TIES_BINS - 1);
                    // the rows of a wave mostly share the upper digits: one LDS add for the wave when they all do
                    const store_u64 act = __ballot(in);
                    if (!act) continue;      // wave-uniform
                    const unsigned dl = (unsigned)__shfl((int)d, (int)__ffsll((long long)act) - 1);
                    if (__ballot(in && d != dl) == 0) {
                        if (lane == 0) atomicAdd(&Hs[dl], (unsigned)__popcll(act));
                    } else if (in) {
                        atomicAdd(&Hs[d], 1u);
                    }
                }
            }
        }
    });
    // ---- one flush per unit
    lds_fence();
    for (int e = lane; e < nop * TIES_BINS; e += 64) {
        const int j = e / TIES_BINS;
        if (j < n_out && ((live >> j) & 1u) && H[e])
            atomicAdd(&state[(size_t)tm[j] * TIES_BINS + (e % TIES_BINS)], (store_u64)H[e]);
    }
}

// ------------------------------------------------------------------------------------ the digit's bin per task
// rank0: the wanted rank j (1-based from below) over all D rows, set at digit 0.  zeros [T]: the rows of the parameters
// a task lacks -- implicit values 0, in bin 0 of every digit while the prefix is all zero.
__global__ __launch_bounds__(64) void k_ties_select_step(store_u64 *__restrict__ state, int T, int digit, int64_t rank0,
                                                         const int64_t *__restrict__ zeros) {
    const int t = threadIdx.x;
    if (t >= T) return;
    store_u64 *h = state + (size_t)t * TIES_BINS;
    const unsigned prefix = digit ? (unsigned)state[ties_prefix_off(T) + t] : 0u;
    const store_u64 rank = digit ? state[ties_rank_off(T) + t] : (store_u64)rank0;
    const store_u64 z = (zeros && prefix == 0u) ? (store_u64)zeros[t] : 0ull;
    store_u64 total = z;
    for (int b = 0; b < TIES_BINS; ++b) total += h[b];
    // from the top: the rank counted from above among the candidates
    store_u64 rtop = total >= rank ? total - rank + 1 : 1, above = 0;
    int pick = 0;
    store_u64 inbin = h[0] + z;
    for (int b = TIES_BINS - 1; b >= 0; --b) {
        const store_u64 c = h[b] + (b == 0 ? z : 0ull);
        if (above + c >= rtop) {
            pick = b;
            inbin = c;
            break;
        }
        above += c;
    }
    const int shift = 32 - TIES_DIGIT_BITS * (digit + 1);
    state[ties_prefix_off(T) + t] = (store_u64)(prefix | ((unsigned)pick << shift));
    state[ties_rank_off(T) + t] = inbin - (rtop - above) + 1;      // from below inside the bin
    for (int b = 0; b < TIES_BINS; ++b) h[b] = 0ull;
}

// ------------------------------------------------------------------------------------ elect, merge, apply
// LDS beyond the streaming carve: TAU [nop] (0xffffffff on a slot that is no live task: never kept), KC [nop] kept counts.
template <bool U16, int TG, int RPL>
__global__ __launch_bounds__(64) void k_ties_merge(const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units,
                                                   const int64_t *__restrict__ rows_dev, int NT, int n_out, int T,
                                                   const int32_t *__restrict__ slot_task,
                                                   const int32_t *__restrict__ task_map,
                                                   const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                                   const uint8_t *__restrict__ basis, const float *__restrict__ meanbuf,
                                                   const float *__restrict__ cbar, int merge_sum, float scaling,
                                                   const float *const *__restrict__ base_ptrs,
                                                   float *const *__restrict__ out_ptrs, store_u64 *__restrict__ state) {
    using G = StreamGeom<U16, RPL>;
    using L = StreamLds<U16, RPL, false>;
    using TU = typename G::T;
    constexpr int ES = G::ES, RB = G::RB;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int lane = threadIdx.x, n = NT;
    const int nop = (n_out + TG - 1) / TG * TG;
    float *C = reinterpret_cast<float *>(lds_raw + L::coeff_off(n));           // [column][nop]
    unsigned *TAU = reinterpret_cast<unsigned *>(lds_raw + L::share_off(n, nop));
    unsigned *KC = TAU + nop;
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
    stage_coeffs(C, cbar + (size_t)p * n_out * n, n, n_out, nop, lane);
    for (int j = lane; j < nop; j += 64) {
        TAU[j] = (j < n_out && ((live >> j) & 1u)) ? (unsigned)state[ties_prefix_off(T) + tm[j]] : 0xffffffffu;
        KC[j] = 0u;
    }
    // the tasks of the store that lack this parameter: their rows are implicit zeros, kept iff tau_t == 0
    bool lacks = lane < T;
    for (int j = 0; j < n_out; ++j)
        if (((live >> j) & 1u) && tm[j] == lane) lacks = false;
    const bool zero_kept = lacks && (unsigned)state[ties_prefix_off(T) + (lane < T ? lane : 0)] == 0u;
    if (zero_kept) atomicAdd(&state[ties_kept_off(T) + lane], (store_u64)(r_end - r_begin));
    const bool any_zero_kept = __ballot(zero_kept) != 0;
    unsigned n_conflict = 0, n_empty = 0;      // wave-uniform

    f32x4 ureg[G::SV];
    float mpf[RPL] = {}, bpf[RPL] = {};
    auto prefetch = [&](int64_t rb) {
        const int nr = block_rows<RB>(rb, r_end);
        ustage_fetch(ureg, ustage_plan<ES>(rb, nr, k, nl), uv.gUh, uv.gUl, lane);
        load_rows(mpf, bpf, uv.gmean, uv.gbase, rb, nr, lane);
    };
    // the block loop written out: as stream_blocks (svdq_store_pass.h) two instantiations spill more scalar registers
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

        // the group's values and which of them the trim keeps (bit s of kb[m])
        float v[RPL][TG];
        unsigned kb[RPL];
        auto group_values = [&](int g0) {
            float hi[RPL][TG], lo[RPL][TG];
            fma_chains<TU, TG, RPL>(hi, lo, Uh, Ul, rl, k, nl, C, nop, g0);
#pragma unroll
            for (int m = 0; m < RPL; ++m) {
                kb[m] = 0u;
#pragma unroll
                for (int s = 0; s < TG; ++s) {
                    v[m][s] = task_value(hi[m][s], lo[m][s], uv.gmean != nullptr, mv[m], 1.f, true, false, 0.f);
                    if ((__float_as_uint(v[m][s]) & 0x7fffffffu) >= TAU[g0 + s]) kb[m] |= 1u << s;
                }
            }
        };
        // ---- sweep A: s[d] = the kept values added task by task
        float ssum[RPL];
        unsigned any_kept = 0u;      // bit m: the row has a kept value
#pragma unroll
        for (int m = 0; m < RPL; ++m) ssum[m] = 0.f;
        for (int g0 = 0; g0 < n_out; g0 += TG) {
            if (!((live >> g0) & ((1u << TG) - 1u))) continue;
            group_values(g0);
#pragma unroll
            for (int s = 0; s < TG; ++s) {
#pragma unroll
                for (int m = 0; m < RPL; ++m) {
                    const bool kept = (kb[m] >> s) & 1u;
                    if (kept) ssum[m] = __fadd_rn(ssum[m], v[m][s]);
                    const store_u64 bal = __ballot(kept && 64 * m + lane < rows_blk);
                    if (bal && lane == 0) KC[g0 + s] += (unsigned)__popcll(bal);
                }
            }
#pragma unroll
            for (int m = 0; m < RPL; ++m)
                if (kb[m]) any_kept |= 1u << m;
        }
        // ---- sweep B: the kept values whose sign agrees with the elected one, and their count
        float asum[RPL], cnt[RPL];
        unsigned sides = 0u;      // bit m: a kept value > 0, bit 4 + m: a kept value < 0
#pragma unroll
        for (int m = 0; m < RPL; ++m) asum[m] = cnt[m] = 0.f;
        for (int g0 = 0; g0 < n_out; g0 += TG) {
            if (!((live >> g0) & ((1u << TG) - 1u))) continue;
            if (n_out > TG) group_values(g0);      // a single group is still in registers
#pragma unroll
            for (int s = 0; s < TG; ++s) {
#pragma unroll
                for (int m = 0; m < RPL; ++m) {
                    const bool kept = (kb[m] >> s) & 1u;
                    const float x = v[m][s];
                    if (kept && x > 0.f) sides |= 1u << m;
                    if (kept && x < 0.f) sides |= 16u << m;
                    if (kept && (ssum[m] >= 0.f ? x > 0.f : x < 0.f)) {
                        asum[m] = __fadd_rn(asum[m], x);
                        cnt[m] = __fadd_rn(cnt[m], 1.f);
                    }
                }
            }
        }
        // ---- apply
#pragma unroll
        for (int m = 0; m < RPL; ++m) {
            const bool in = 64 * m + lane < rows_blk;
            float res = merge_sum ? asum[m] : __fdiv_rn(asum[m], cnt[m] > 1.f ? cnt[m] : 1.f);
            res = __fmul_rn(scaling, res);
            if (uv.gbase) res = __fadd_rn(bv[m], res);
            if (in) gout[rb + 64 * m + lane] = res;
            n_conflict += (unsigned)__popcll(__ballot(in && ((sides >> m) & 1u) && ((sides >> (4 + m)) & 1u)));
            n_empty += (unsigned)__popcll(__ballot(in && !((any_kept >> m) & 1u) && !any_zero_kept));
        }
        lds_fence();      // the basis rows are rewritten next
    }
    // ---- one flush per unit
    lds_fence();
    for (int j = lane; j < n_out; j += 64)
        if (((live >> j) & 1u) && KC[j]) atomicAdd(&state[ties_kept_off(T) + tm[j]], (store_u64)KC[j]);
    if (lane == 0) {
        if (n_conflict) atomicAdd(&state[ties_conflict_off(T)], (store_u64)n_conflict);
        if (n_empty) atomicAdd(&state[ties_empty_off(T)], (store_u64)n_empty);
    }
}

// ------------------------------------------------------------------------------------ entry points
extern "C" int64_t svdq_ties_work_bytes(int32_t n_tasks) {
    if (n_tasks < 1 || n_tasks > SVDQ_MAX_TASKS) return 0;
    return svdq_align_up(ties_words(n_tasks) * 8, 256);
}

extern "C" int svdq_plan_ties_hist(const svdq_plan *pl, const int64_t *rows_dev, const void *small, const void *basis,
                                   const float *mean, const int32_t *slot_task, const int32_t *task_map, int32_t n_out,
                                   int32_t n_tasks, int32_t digit, void *state, void *work, void *stream) {
    const char *who = "svdq_plan_ties_hist";
    if (int rc = store_args_ok(who, pl, small, basis, mean, slot_task, task_map, n_out, n_tasks, state, work)) return rc;
    if (digit < 0 || digit >= TIES_DIGITS) {
        svdq_set_error("%s: digit must be in [0, %d), got %d", who, TIES_DIGITS, digit);
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const int n = pl->n_tasks;
    const uint8_t *bs = reinterpret_cast<const uint8_t *>(basis);
    const float *mn = pl->cfg.center ? mean : nullptr;
    float *cbar = reinterpret_cast<float *>(work);
    return store_stream(who, pl, small, slot_task, task_map, (int)n_out, cbar, st,
                       [&](auto f16_c, auto tg_c, auto rpl_c, const SmallView &sv, int nop) {
                           constexpr bool F16 = f16_c;
                           constexpr int TG = tg_c, RPL = rpl_c;
                           using Plain = StreamLds<F16, RPL, false>;
                           hipLaunchKernelGGL((k_ties_hist<F16, TG, RPL>), dim3(pl->n_units), dim3(64),
                                              Plain::bytes(n, nop, nop * TIES_BINS), st, pl->d_params, pl->d_units,
                                              rows_dev, n, (int)n_out, (int)n_tasks, slot_task, task_map, sv.k, sv.r, bs,
                                              mn, cbar, (int)digit, reinterpret_cast<store_u64 *>(state));
                       });
}

extern "C" int svdq_ties_select_step(void *state, int32_t n_tasks, int32_t digit, int64_t rank,
                                     const int64_t *zeros_dev, void *stream) {
    const char *who = "svdq_ties_select_step";
    if (!state) {
        svdq_set_error("%s: state is required", who);
        return SVDQ_EINVAL;
    }
    if (n_tasks < 1 || n_tasks > SVDQ_MAX_TASKS) {
        svdq_set_error("%s: n_tasks must be in [1, %d], got %d", who, SVDQ_MAX_TASKS, n_tasks);
        return SVDQ_EINVAL;
    }
    if (digit < 0 || digit >= TIES_DIGITS) {
        svdq_set_error("%s: digit must be in [0, %d), got %d", who, TIES_DIGITS, digit);
        return SVDQ_EINVAL;
    }
    if (digit == 0 && rank < 1) {
        svdq_set_error("%s: rank must be >= 1, got %lld", who, (long long)rank);
        return SVDQ_EINVAL;
    }
    hipLaunchKernelGGL(k_ties_select_step, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<store_u64 *>(state),
                       (int)n_tasks, (int)digit, rank, zeros_dev);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

extern "C" int svdq_plan_ties_merge(const svdq_plan *pl, const int64_t *rows_dev, const void *small, const void *basis,
                                    const float *mean, const int32_t *slot_task, const int32_t *task_map, int32_t n_out,
                                    int32_t n_tasks, int32_t merge_sum, float scaling, const void *base_ptrs,
                                    const void *out_ptrs, void *state, void *work, void *stream) {
    const char *who = "svdq_plan_ties_merge";
    if (int rc = store_args_ok(who, pl, small, basis, mean, slot_task, task_map, n_out, n_tasks, state, work)) return rc;
    if (!out_ptrs) {
        svdq_set_error("%s: out_ptrs is required", who);
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const int n = pl->n_tasks;
    const uint8_t *bs = reinterpret_cast<const uint8_t *>(basis);
    const float *mn = pl->cfg.center ? mean : nullptr;
    float *cbar = reinterpret_cast<float *>(work);
    auto bp = reinterpret_cast<const float *const *>(base_ptrs);
    auto op = reinterpret_cast<float *const *>(out_ptrs);
    return store_stream(who, pl, small, slot_task, task_map, (int)n_out, cbar, st,
                       [&](auto f16_c, auto tg_c, auto rpl_c, const SmallView &sv, int nop) {
                           constexpr bool F16 = f16_c;
                           constexpr int TG = tg_c, RPL = rpl_c;
                           using Plain = StreamLds<F16, RPL, false>;
                           hipLaunchKernelGGL((k_ties_merge<F16, TG, RPL>), dim3(pl->n_units), dim3(64),
                                              Plain::bytes(n, nop, 2 * nop), st, pl->d_params, pl->d_units, rows_dev, n,
                                              (int)n_out, (int)n_tasks, slot_task, task_map, sv.k, sv.r, bs, mn, cbar,
                                              merge_sum ? 1 : 0, scaling, bp, op, reinterpret_cast<store_u64 *>(state));
                       });
}
