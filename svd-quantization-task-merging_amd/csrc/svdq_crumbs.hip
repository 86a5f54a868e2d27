// svdq_crumbs.hip -- the Model Breadcrumbs merge (Davari & Belilovsky 2023) of a store, and with it the per-tensor trim:
// per parameter and task a two-sided magnitude band -- the small bulk and the few largest outliers are dropped -- then an
// optional sign election and the sum or mean of what is left, in streaming passes over the basis.  Compiled with
// -ffp-contract=off like svdq_ties.hip: every product and sum is rounded where the definition (DESIGN.md section 35,
// include/svdq.h) rounds.
//
// The band needs two exact order statistics per (parameter, task).  The kernels below are the frame of k_ties_hist /
// k_ties_merge (one wave per work unit, the staging, one-block prefetch, LDS image and fma chains of
// svdq_merge_stream.h, task groups of TG, RPL rows per lane): the value of (row, task) is fma_chains + task_value
// unchanged, so every pass sees the bits reconstruct_task_vectors writes -- and no task model is ever written.
//
//   k_store_coeff         the live tasks' coefficients per parameter (svdq_store_values.hip, launched by store_stream)
//   k_crumbs_hist         one digit of the radix selection of lo and hi of every (parameter, task) of the plan: for each
//                         requested bound the magnitudes whose upper bits equal that bound's prefix are counted per digit
//                         value in an LDS histogram, flushed once per unit into the parameter's rows of the table
//   k_crumbs_select_step  one thread per (parameter, task, bound): the bin that holds the wanted rank, appended to the
//                         prefix; the histogram it read is zeroed
//   k_crumbs_merge        band test, elect (sweep A, only with sign election), combine (sweep B), apply
//
// The state table of ONE plan (svdq_crumbs_work_bytes(P, T) bytes; P parameters, T store tasks; bound b: 0 = lo, 1 = hi):
//   hist    uint32 [P][2][T][256]                     = P * T * 256 uint64 words
//   then uint64 words:
//   prefix  [P][2][T]    after the last digit the bit pattern of the bound in the low 32 bits; the sentinel band of a
//                        (p, t) that keeps nothing is lo = 0xffffffff, hi = 0: no magnitude passes
//   rank    [P][2][T]    1-based from below among the candidates left; 0 = the (p, t) keeps nothing (set at digit 0)
//   kept    [P][T]       values kept per (parameter, task)
//   rows with kept values of both signs | rows with nothing kept
// Integer counts only: no result depends on the order the units arrive in.  Counts are uint32, so a parameter of 2^32
// rows or more is refused by the entry points.

#include "svdq_store_values.h"

#define CRUMBS_BINS 256
#define CRUMBS_DIGIT_BITS 8
#define CRUMBS_DIGITS SVDQ_CRUMBS_DIGITS      // 4: 31 magnitude bits, 8 per pass from the top
#define CRUMBS_BOTH_MAX 16                    // task slots up to which both bounds are counted in one pass (32 KB of LDS)

__host__ __device__ constexpr int64_t crumbs_prefix_off(int64_t P, int T) { return P * T * CRUMBS_BINS; }
__host__ __device__ constexpr int64_t crumbs_rank_off(int64_t P, int T) { return crumbs_prefix_off(P, T) + 2 * P * T; }
__host__ __device__ constexpr int64_t crumbs_kept_off(int64_t P, int T) { return crumbs_rank_off(P, T) + 2 * P * T; }
__host__ __device__ constexpr int64_t crumbs_conflict_off(int64_t P, int T) { return crumbs_kept_off(P, T) + P * T; }
__host__ __device__ constexpr int64_t crumbs_empty_off(int64_t P, int T) { return crumbs_conflict_off(P, T) + 1; }
__host__ __device__ constexpr int64_t crumbs_words(int64_t P, int T) { return crumbs_empty_off(P, T) + 1; }
// word of (p, b, t) inside prefix / rank
__host__ __device__ constexpr int64_t crumbs_pbt(int p, int b, int t, int T) { return ((int64_t)p * 2 + b) * T + t; }

// ------------------------------------------------------------------------------------ one digit of the selection
// LDS beyond the streaming carve: PFX [2][nop] the two prefixes of every slot | H [nb][nop][256] uint32, nb = 2 with
// bounds == 3 (nop <= 16: 32 KB), else 1 (nop <= 32: 32 KB).  While the two prefixes of a slot are equal (always at digit
// 0) its magnitudes are counted once, into the lo histogram, and the flush adds that count to both tables.
template <bool U16, int TG, int RPL>
__global__ __launch_bounds__(64) void k_crumbs_hist(const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units,
                                                    const int64_t *__restrict__ rows_dev, int NT, int n_out, int T,
                                                    const int32_t *__restrict__ slot_task,
                                                    const int32_t *__restrict__ task_map,
                                                    const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                                    const uint8_t *__restrict__ basis, const float *__restrict__ meanbuf,
                                                    const float *__restrict__ cbar, int P, int digit, int bounds,
                                                    store_u64 *__restrict__ state) {
    using G = StreamGeom<U16, RPL>;
    using L = StreamLds<U16, RPL, false>;
    using TU = typename G::T;
    constexpr int ES = G::ES, RB = G::RB;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int lane = threadIdx.x, n = NT;
    const int nop = (n_out + TG - 1) / TG * TG;
    float *C = reinterpret_cast<float *>(lds_raw + L::coeff_off(n));           // [column][nop]
    unsigned *PFX = reinterpret_cast<unsigned *>(lds_raw + L::share_off(n, nop));      // [2][nop]
    unsigned *H = PFX + 2 * nop;                                                       // [nb][nop][256]
    const bool want_lo = bounds & 1, want_hi = bounds & 2, both = bounds == 3;
    const int nh = (both ? 2 : 1) * nop * CRUMBS_BINS;
    unsigned *Hhi = both ? H + nop * CRUMBS_BINS : H;
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
    for (int e = lane; e < nh; e += 64) H[e] = 0u;
    for (int e = lane; e < 2 * nop; e += 64) {
        const int b = e / nop, j = e % nop;
        const bool on = digit && j < n_out && ((live >> j) & 1u);
        PFX[e] = on ? (unsigned)state[crumbs_prefix_off(P, T) + crumbs_pbt(p, b, tm[j], T)] : 0u;
    }
    lds_fence();
    const int shift = 32 - CRUMBS_DIGIT_BITS * (digit + 1);      // 24, 16, 8, 0
    const unsigned upper = digit ? 0xffffffffu << (shift + CRUMBS_DIGIT_BITS) : 0u;      // the bits of the earlier digits

    // the rows of a wave mostly share the upper digits: one LDS add for the wave when they all do
    auto count = [&](unsigned *Hs, bool in, unsigned d) {
        const store_u64 act = __ballot(in);
        if (!act) return;      // wave-uniform
        const unsigned dl = (unsigned)__shfl((int)d, (int)__ffsll((long long)act) - 1);
        if (__ballot(in && d != dl) == 0) {
            if (lane == 0) atomicAdd(&Hs[dl], (unsigned)__popcll(act));
        } else if (in) {
            atomicAdd(&Hs[d], 1u);
        }
    };

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
                const unsigned plo = PFX[g0 + s], phi = PFX[nop + g0 + s];
                const bool same = both && plo == phi;      // wave-uniform: one count serves both bounds
                unsigned *Hl = H + (g0 + s) * CRUMBS_BINS, *Hh = Hhi + (g0 + s) * CRUMBS_BINS;
#pragma unroll
                for (int m = 0; m < RPL; ++m) {
                    const float v = task_value(hi[m][s], lo[m][s], uv.gmean != nullptr, mv[m], 1.f, true, false, 0.f);
                    const unsigned mag = __float_as_uint(v) & 0x7fffffffu;
                    const bool row = 64 * m + lane < rows_blk;
                    const unsigned d = (mag >> shift) & (CRUMBS_BINS - 1);
                    if (want_lo) count(Hl, row && ((mag ^ plo) & upper) == 0u, d);
                    if (want_hi && !same) count(Hh, row && ((mag ^ phi) & upper) == 0u, d);
                }
            }
        }
    });
    // ---- one flush per unit, into the parameter's rows of the table
    lds_fence();
    store_gu32 *hist = (store_gu32 *)reinterpret_cast<uint32_t *>(state);
    for (int e = lane; e < nop * CRUMBS_BINS; e += 64) {
        const int j = e / CRUMBS_BINS, b = e % CRUMBS_BINS;
        if (j >= n_out || !((live >> j) & 1u)) continue;
        const bool same = both && PFX[j] == PFX[nop + j];
        const unsigned cl = want_lo ? H[e] : 0u;
        const unsigned ch = want_hi ? (same ? H[e] : Hhi[e]) : 0u;
        if (cl)
            __hip_atomic_fetch_add(hist + crumbs_pbt(p, 0, tm[j], T) * CRUMBS_BINS + b, cl, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        if (ch)
            __hip_atomic_fetch_add(hist + crumbs_pbt(p, 1, tm[j], T) * CRUMBS_BINS + b, ch, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------------------------ the digit's bin per (p, t, bound)
// ranks int64 [P][2]: the wanted ranks (1-based from below) of lo and hi over the parameter's rows, read at digit 0;
// <= 0 = the parameter keeps nothing.  A (p, t) without counts at digit 0 is no live task of the parameter.  Both end
// with the sentinel band and rank 0, which the later digits leave alone.  The walk is k_ties_select_step's, without its
// implicit zeros.
__global__ __launch_bounds__(64) void k_crumbs_select_step(store_u64 *__restrict__ state, int P, int T, int digit,
                                                           const int64_t *__restrict__ ranks) {
    const int p = blockIdx.x, i = threadIdx.x;
    if (i >= 2 * T) return;
    const int b = i / T, t = i % T;
    const int64_t w = crumbs_pbt(p, b, t, T);
    uint32_t *h = reinterpret_cast<uint32_t *>(state) + w * CRUMBS_BINS;
    store_u64 *prefix_w = state + crumbs_prefix_off(P, T) + w, *rank_w = state + crumbs_rank_off(P, T) + w;
    store_u64 total = 0;
    for (int bin = 0; bin < CRUMBS_BINS; ++bin) total += h[bin];
    const int64_t r0 = digit ? 1 : ranks[2 * p + b];
    const store_u64 rank = digit ? *rank_w : (r0 > 0 && total ? (store_u64)r0 : 0ull);
    if (rank == 0ull) {
        if (!digit) {
            *prefix_w = b ? 0ull : 0xffffffffull;
            *rank_w = 0ull;
        }
    } else {
        const unsigned prefix = digit ? (unsigned)*prefix_w : 0u;
        // from the top: the rank counted from above among the candidates
        store_u64 rtop = total >= rank ? total - rank + 1 : 1, above = 0, inbin = h[0];
        int pick = 0;
        for (int bin = CRUMBS_BINS - 1; bin >= 0; --bin) {
            const store_u64 c = h[bin];
            if (above + c >= rtop) {
                pick = bin;
                inbin = c;
                break;
            }
            above += c;
        }
        const int shift = 32 - CRUMBS_DIGIT_BITS * (digit + 1);
        *prefix_w = (store_u64)(prefix | ((unsigned)pick << shift));
        *rank_w = inbin - (rtop - above) + 1;      // from below inside the bin
    }
    for (int bin = 0; bin < CRUMBS_BINS; ++bin) h[bin] = 0u;
}

// ------------------------------------------------------------------------------------ band, elect, combine, apply
// LDS beyond the streaming carve: LO [nop] | HI [nop] (the sentinel band on a slot that is no live task) | KC [nop] kept
// counts.
template <bool U16, int TG, int RPL>
__global__ __launch_bounds__(64) void k_crumbs_merge(const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units,
                                                     const int64_t *__restrict__ rows_dev, int NT, int n_out, int T,
                                                     const int32_t *__restrict__ slot_task,
                                                     const int32_t *__restrict__ task_map,
                                                     const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                                     const uint8_t *__restrict__ basis, const float *__restrict__ meanbuf,
                                                     const float *__restrict__ cbar, int P, int elect, int merge_sum,
                                                     float scaling, const float *const *__restrict__ base_ptrs,
                                                     float *const *__restrict__ out_ptrs, store_u64 *__restrict__ state) {
    using G = StreamGeom<U16, RPL>;
    using L = StreamLds<U16, RPL, false>;
    using TU = typename G::T;
    constexpr int ES = G::ES, RB = G::RB;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int lane = threadIdx.x, n = NT;
    const int nop = (n_out + TG - 1) / TG * TG;
    float *C = reinterpret_cast<float *>(lds_raw + L::coeff_off(n));           // [column][nop]
    unsigned *LO = reinterpret_cast<unsigned *>(lds_raw + L::share_off(n, nop));
    unsigned *HI = LO + nop, *KC = HI + nop;
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
        const bool on = j < n_out && ((live >> j) & 1u);
        LO[j] = on ? (unsigned)state[crumbs_prefix_off(P, T) + crumbs_pbt(p, 0, tm[j], T)] : 0xffffffffu;
        HI[j] = on ? (unsigned)state[crumbs_prefix_off(P, T) + crumbs_pbt(p, 1, tm[j], T)] : 0u;
        KC[j] = 0u;
    }
    unsigned n_conflict = 0, n_empty = 0;      // wave-uniform

    f32x4 ureg[G::SV];
    float mpf[RPL] = {}, bpf[RPL] = {};
    auto prefetch = [&](int64_t rb) {
        const int nr = block_rows<RB>(rb, r_end);
        ustage_fetch(ureg, ustage_plan<ES>(rb, nr, k, nl), uv.gUh, uv.gUl, lane);
        load_rows(mpf, bpf, uv.gmean, uv.gbase, rb, nr, lane);
    };
    // the block loop written out: as stream_blocks (svdq_store_pass.h) the instantiations spill more scalar registers
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

        // the group's values and which of them the band keeps (bit s of kb[m])
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
                    const unsigned mag = __float_as_uint(v[m][s]) & 0x7fffffffu;
                    if (mag >= LO[g0 + s] && mag <= HI[g0 + s]) kb[m] |= 1u << s;
                }
            }
        };
        // ---- sweep A (sign election only): s[d] = the kept values added task by task
        float ssum[RPL];
#pragma unroll
        for (int m = 0; m < RPL; ++m) ssum[m] = 0.f;
        if (elect) {
            for (int g0 = 0; g0 < n_out; g0 += TG) {
                if (!((live >> g0) & ((1u << TG) - 1u))) continue;
                group_values(g0);
#pragma unroll
                for (int s = 0; s < TG; ++s) {
#pragma unroll
                    for (int m = 0; m < RPL; ++m)
                        if ((kb[m] >> s) & 1u) ssum[m] = __fadd_rn(ssum[m], v[m][s]);
                }
            }
        }
        // ---- sweep B: the kept values (with election: whose sign agrees with the elected one), and their count
        float asum[RPL], cnt[RPL];
        unsigned sides = 0u;          // bit m: a kept value > 0, bit 4 + m: a kept value < 0
        unsigned any_kept = 0u;      // bit m: the row has a kept value
#pragma unroll
        for (int m = 0; m < RPL; ++m) asum[m] = cnt[m] = 0.f;
        for (int g0 = 0; g0 < n_out; g0 += TG) {
            if (!((live >> g0) & ((1u << TG) - 1u))) continue;
            if (n_out > TG || !elect) group_values(g0);      // a single elected group is still in registers
#pragma unroll
            for (int s = 0; s < TG; ++s) {
#pragma unroll
                for (int m = 0; m < RPL; ++m) {
                    const bool kept = (kb[m] >> s) & 1u;
                    const float x = v[m][s];
                    if (kept && x > 0.f) sides |= 1u << m;
                    if (kept && x < 0.f) sides |= 16u << m;
                    if (kept && (!elect || (ssum[m] >= 0.f ? x > 0.f : x < 0.f))) {
                        asum[m] = __fadd_rn(asum[m], x);
                        cnt[m] = __fadd_rn(cnt[m], 1.f);
                    }
                    const store_u64 bal = __ballot(kept && 64 * m + lane < rows_blk);
                    if (bal && lane == 0) KC[g0 + s] += (unsigned)__popcll(bal);
                }
            }
#pragma unroll
            for (int m = 0; m < RPL; ++m)
                if (kb[m]) any_kept |= 1u << m;
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
            n_empty += (unsigned)__popcll(__ballot(in && !((any_kept >> m) & 1u)));
        }
        lds_fence();      // the basis rows are rewritten next
    }
    // ---- one flush per unit
    lds_fence();
    for (int j = lane; j < n_out; j += 64)
        if (((live >> j) & 1u) && KC[j])
            atomicAdd(&state[crumbs_kept_off(P, T) + (int64_t)p * T + tm[j]], (store_u64)KC[j]);
    if (lane == 0) {
        if (n_conflict) atomicAdd(&state[crumbs_conflict_off(P, T)], (store_u64)n_conflict);
        if (n_empty) atomicAdd(&state[crumbs_empty_off(P, T)], (store_u64)n_empty);
    }
}

// ------------------------------------------------------------------------------------ entry points
extern "C" int64_t svdq_crumbs_work_bytes(int32_t n_params, int32_t n_tasks) {
    if (n_params < 1 || n_tasks < 1 || n_tasks > SVDQ_MAX_TASKS) return 0;
    return svdq_align_up(crumbs_words(n_params, n_tasks) * 8, 256);
}

// uint32 counts: the named refusal of a parameter with 2^32 rows or more
static bool crumbs_refuse_rows(const char *who, const svdq_plan *pl) {
    for (int p = 0; p < pl->n_params; ++p)
        if (pl->h_params[p].rows >= (int64_t)1 << 32) {
            svdq_set_error("%s: parameter %d has %lld rows; the histogram counts are 32-bit: fewer than 2^32 rows per "
                           "parameter", who, p, (long long)pl->h_params[p].rows);
            return true;
        }
    return false;
}

static bool crumbs_refuse_digit(const char *who, int digit) {
    if (digit >= 0 && digit < CRUMBS_DIGITS) return false;
    svdq_set_error("%s: digit must be in [0, %d), got %d", who, CRUMBS_DIGITS, digit);
    return true;
}

extern "C" int svdq_plan_crumbs_hist(const svdq_plan *pl, const int64_t *rows_dev, const void *small, const void *basis,
                                     const float *mean, const int32_t *slot_task, const int32_t *task_map, int32_t n_out,
                                     int32_t n_tasks, int32_t digit, int32_t bounds, void *state, void *work,
                                     void *stream) {
    const char *who = "svdq_plan_crumbs_hist";
    if (int rc = store_args_ok(who, pl, small, basis, mean, slot_task, task_map, n_out, n_tasks, state, work)) return rc;
    if (crumbs_refuse_digit(who, digit)) return SVDQ_EINVAL;
    if (bounds < 1 || bounds > 3) {
        svdq_set_error("%s: bounds must be 1 (lo), 2 (hi) or 3 (both), got %d", who, bounds);
        return SVDQ_EINVAL;
    }
    if (bounds == 3 && n_out > CRUMBS_BOTH_MAX) {
        svdq_set_error("%s: bounds 3 counts both histograms in one pass for n_out <= %d, got %d: one bound per call "
                       "above", who, CRUMBS_BOTH_MAX, n_out);
        return SVDQ_EINVAL;
    }
    if (crumbs_refuse_rows(who, pl)) return SVDQ_EINVAL;
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
                           const int nb = bounds == 3 ? 2 : 1;
                           hipLaunchKernelGGL((k_crumbs_hist<F16, TG, RPL>), dim3(pl->n_units), dim3(64),
                                              Plain::bytes(n, nop, 2 * nop + nb * nop * CRUMBS_BINS), st, pl->d_params,
                                              pl->d_units, rows_dev, n, (int)n_out, (int)n_tasks, slot_task, task_map,
                                              sv.k, sv.r, bs, mn, cbar, (int)pl->n_params, (int)digit, (int)bounds,
                                              reinterpret_cast<store_u64 *>(state));
                       });
}

extern "C" int svdq_plan_crumbs_select_step(const svdq_plan *pl, int32_t n_tasks, int32_t digit, const int64_t *ranks_dev,
                                            void *state, void *stream) {
    const char *who = "svdq_plan_crumbs_select_step";
    if (!pl || !ranks_dev || !state) {
        svdq_set_error("%s: plan, ranks and state are required", who);
        return SVDQ_EINVAL;
    }
    if (n_tasks < 1 || n_tasks > SVDQ_MAX_TASKS) {
        svdq_set_error("%s: n_tasks must be in [1, %d], got %d", who, SVDQ_MAX_TASKS, n_tasks);
        return SVDQ_EINVAL;
    }
    if (crumbs_refuse_digit(who, digit)) return SVDQ_EINVAL;
    hipLaunchKernelGGL(k_crumbs_select_step, dim3(pl->n_params), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<store_u64 *>(state), (int)pl->n_params, (int)n_tasks, (int)digit, ranks_dev);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

extern "C" int svdq_plan_crumbs_merge(const svdq_plan *pl, const int64_t *rows_dev, const void *small, const void *basis,
                                      const float *mean, const int32_t *slot_task, const int32_t *task_map, int32_t n_out,
                                      int32_t n_tasks, int32_t sign_election, int32_t merge_sum, float scaling,
                                      const void *base_ptrs, const void *out_ptrs, void *state, void *work, void *stream) {
    const char *who = "svdq_plan_crumbs_merge";
    if (int rc = store_args_ok(who, pl, small, basis, mean, slot_task, task_map, n_out, n_tasks, state, work)) return rc;
    if (!out_ptrs) {
        svdq_set_error("%s: out_ptrs is required", who);
        return SVDQ_EINVAL;
    }
    if (crumbs_refuse_rows(who, pl)) return SVDQ_EINVAL;
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
                           hipLaunchKernelGGL((k_crumbs_merge<F16, TG, RPL>), dim3(pl->n_units), dim3(64),
                                              Plain::bytes(n, nop, 3 * nop), st, pl->d_params, pl->d_units, rows_dev, n,
                                              (int)n_out, (int)n_tasks, slot_task, task_map, sv.k, sv.r, bs, mn, cbar,
                                              (int)pl->n_params, sign_election ? 1 : 0, merge_sum ? 1 : 0, scaling, bp, op,
                                              reinterpret_cast<store_u64 *>(state));
                       });
}
