// svdq_emr.hip -- the EMR merge of a store (Huang et al. 2024: "EMR-Merging: Tuning-Free High-Performance Model Merging"):
// Elect one task vector, a 1-bit Mask per task and one Rescaler per task in ONE streaming pass over the basis, and the
// streaming kernel that serves a task's model from the three.  Compiled with -ffp-contract=off like svdq_ties.hip,
// svdq_dare.hip and svdq_tall.hip: every product and sum is rounded where the definition (DESIGN.md section 31,
// include/svdq.h at svdq_plan_emr_elect) rounds.
//
// k_emr_elect is k_tall_consensus' frame (svdq_tall.hip): one wave per work unit, the staging, the one-block prefetch,
// the fma chains of svdq_merge_stream.h, task groups of TG, RPL rows per lane, two sweeps over the task groups per block.
// Sweep A adds the values task by task (S, whose sign is gamma); sweep B forms them again, tests each against gamma, keeps
// the largest agreeing magnitude per row (eps), ballots the agree bits into the LDS bit image and adds |v| into the
// slot's A partial.  After sweep B eps is final for the lane's rows: every slot's image bits are read back and eps is
// added into the slot's B partial where set.  The stream words are built as k_tall_consensus builds them.  The value of
// (row, task) is fma_chains + task_value unchanged -- the bits reconstruct_task_vectors writes.  No task model is written.
//
// The sums A_g = sum |v_g| and B_g = sum M_g eps are fp64 and DETERMINISTIC: no floating-point atomics.  Up to 8 slots
// every lane owns one fp64 cell per (sum, slot) in LDS ([2][nop][64], written by that lane alone: conflict-free, no
// fence), adds its rows block by block in ascending order, and at the end of the unit lane e < 2 T adds the 64 cells of
// its (sum, task) in a fixed order (starting at cell e, wrapping: the bank rotation).  Above 8 slots the cells would take
// the LDS that the waves per SIMD need (EmrLds): there the wave adds a block's 64 lane values by a butterfly of fixed
// order and lane 0 adds the sum to the slot's one cell, block by block.  Either way the unit STORES [2][T] doubles at
// its own slot of the plan's table [n_units][2][T].  k_emr_finish, one block, then adds the units in ascending order -- in 1024 / 2 T
// contiguous runs of units, one per thread, the runs added in ascending order -- into the store's state [2][T].
//
// The coefficient kernel, the live mask, the bit image and its word writer, the argument check and the dispatcher are
// those of svdq_store_values.h.

#include "svdq_store_values.h"

#include <cmath>

typedef const __attribute__((address_space(1))) uint32_t emr_gcu32;
typedef __attribute__((address_space(1))) f32x4 emr_gf32x4_w;

// ------------------------------------------------------------------------------------ the LDS beyond the streaming carve
// IMG [nop][IW] the block's agree bits per slot (MaskImage) | SLOT [T] the slot of every store task, -1 = the
// parameter has none | one word of alignment slack | AB, the fp64 partials of A (w = 0) and B (w = 1).  Up to CELLS slots:
// [2][nop][64], lane l's own cell of slot j at [(w * nop + j) * 64 + l] (8 KB at 8 slots: the VGPRs, not the LDS, bound
// the waves per SIMD).  Above: [2][nop], one cell per slot that lane 0 adds the wave's sum of a block to -- per-lane cells
// (24 KB at 24 slots) left one wave per SIMD where k_tall_consensus runs four, and the kernel took 2.7 times its time.
template <int RPL> struct EmrLds : MaskImage<RPL> {
    static constexpr int CELLS = 8;             // slots up to which every lane keeps its own cells
    __host__ __device__ static constexpr int ab_doubles(int nop) { return nop <= CELLS ? 2 * nop * 64 : 2 * nop; }
    __host__ __device__ static constexpr int words(int nop, int T) {
        return nop * MaskImage<RPL>::IW + T + 1 + 2 * ab_doubles(nop);
    }
};

// the sum of a wave's 64 values by the xor butterfly (32, 16, .. 1): both partners of a step add the same two numbers, so
// every lane ends with the same bits, and the order is fixed
__device__ __forceinline__ double emr_wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// ------------------------------------------------------------------------------------ elect, mask, rescale
template <bool U16, int TG, int RPL>
__global__ __launch_bounds__(64) void k_emr_elect(
    const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units, const int64_t *__restrict__ rows_dev, int NT,
    int n_out, int T, const int32_t *__restrict__ slot_task, const int32_t *__restrict__ task_map,
    const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in, const uint8_t *__restrict__ basis,
    const float *__restrict__ meanbuf, const float *__restrict__ cbar, const int64_t *__restrict__ bit_base,
    float *const *__restrict__ uni_ptrs, uint32_t *const *__restrict__ mask_ptrs, double *__restrict__ table) {
    using Geo = StreamGeom<U16, RPL>;
    using L = StreamLds<U16, RPL, false>;
    using X = EmrLds<RPL>;
    using TU = typename Geo::T;
    constexpr int ES = Geo::ES, RB = Geo::RB, IW = X::IW;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int lane = threadIdx.x, n = NT;
    const int nop = (n_out + TG - 1) / TG * TG;
    float *C = reinterpret_cast<float *>(lds_raw + L::coeff_off(n));           // [column][nop]
    unsigned *IMG = reinterpret_cast<unsigned *>(lds_raw + L::share_off(n, nop));
    int *SLOT = reinterpret_cast<int *>(IMG + nop * IW);
    double *AB = reinterpret_cast<double *>(lds_raw + ((L::share_off(n, nop) + 4 * (size_t)(nop * IW + T) + 7) & ~(size_t)7));
    double *mine = table + (size_t)blockIdx.x * 2 * T;      // the unit's own slot of the plan's table
    const SvdqUnit ud = units[blockIdx.x];
    const int p = ud.param;
    const UnitView uv = unit_view<ES>(params[p], p, rows_dev, k_in, r_in, basis, meanbuf, nullptr);
    const int64_t r_begin = ud.row0;
    int64_t r_end = r_begin + ud.nrows;
    if (r_end > uv.D) r_end = uv.D;
    if (r_begin >= r_end) {      // a unit without rows adds zeros: its slot is read by k_emr_finish all the same
        if (lane < 2 * T) mine[lane] = 0.0;
        return;
    }
    mg_gfloat_w *gout = (mg_gfloat_w *)uni_ptrs[p];      // NULL: the parameter's masks and sums only
    const int32_t *tm = task_map + (size_t)p * n_out;
    const unsigned live = store_live_mask(slot_task + (size_t)p * n_out, tm, n_out, n, T, lane);
    const int k = uv.k, nl = uv.nl;
    const int64_t bit_first = bit_base[p];      // the stream bit of the parameter's row 0
    stage_coeffs(C, cbar + (size_t)p * n_out * n, n, n_out, nop, lane);
    for (int j = lane; j < nop * IW; j += 64) IMG[j] = 0u;
    for (int j = lane; j < T; j += 64) SLOT[j] = -1;
    const bool cells = nop <= X::CELLS;      // wave-uniform: which form the partials have
    for (int j = lane; j < X::ab_doubles(nop); j += 64) AB[j] = 0.0;
    lds_fence();
    if (lane < n_out && ((live >> lane) & 1u)) SLOT[tm[lane]] = lane;

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
        float mv[RPL];
        int rl[RPL];
        block_rows_of_lane(rl, rows_blk, lane);
#pragma unroll
        for (int m = 0; m < RPL; ++m) mv[m] = mpf[m];
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
        // ---- sweep B: the agree test against gamma = sign(S), eps = the largest agreeing |v|, the bits, A += |v|
        float eps[RPL];
#pragma unroll
        for (int m = 0; m < RPL; ++m) eps[m] = 0.f;
        for (int g0 = 0; g0 < n_out; g0 += TG) {
            const unsigned gm = (live >> g0) & ((1u << TG) - 1u);
            if (!gm) continue;
            if (n_out > TG) group_values(g0);      // a single group is still in registers
#pragma unroll
            for (int s = 0; s < TG; ++s) {
                if (!((gm >> s) & 1u)) continue;      // wave-uniform
                double a = 0.0;
#pragma unroll
                for (int m = 0; m < RPL; ++m) {
                    const float x = v[m][s], ax = fabsf(x);
                    const bool in = 64 * m + lane < rows_blk;
                    const bool set = (ssum[m] > 0.f && x > 0.f) || (ssum[m] < 0.f && x < 0.f);
                    if (set && ax > eps[m]) eps[m] = ax;
                    const store_u64 bal = __ballot(set && in);
                    if (lane < 2) IMG[(g0 + s) * IW + 1 + 2 * m + lane] = (unsigned)(bal >> (32 * lane));
                    if (in) a += (double)ax;
                }
                if (cells) {
                    AB[(g0 + s) * 64 + lane] += a;      // the lane's own cell
                } else {
                    a = emr_wave_sum(a);
                    if (lane == 0) AB[g0 + s] += a;
                }
            }
        }
        lds_fence();      // the image is read by other lanes
        // ---- eps is final: B += eps where the slot's bit of the row is set
        for (int j = 0; j < n_out; ++j) {
            if (!((live >> j) & 1u)) continue;      // wave-uniform
            double b = 0.0;
#pragma unroll
            for (int m = 0; m < RPL; ++m) {
                const unsigned w = IMG[j * IW + 1 + 2 * m + (lane >> 5)];
                if ((w >> (lane & 31)) & 1u) b += (double)eps[m];
            }
            if (cells) {
                AB[(nop + j) * 64 + lane] += b;
            } else {
                b = emr_wave_sum(b);
                if (lane == 0) AB[nop + j] += b;
            }
        }
        // ---- tau_uni = copysign(eps, gamma); eps = +0 where gamma = 0
#pragma unroll
        for (int m = 0; m < RPL; ++m) {
            const float res = ssum[m] < 0.f ? -eps[m] : eps[m];
            if (64 * m + lane < rows_blk && gout) gout[rb + 64 * m + lane] = res;
        }
        // ---- the block's stream words
        store_mask_words<RPL>(IMG, live, tm, n_out, nop, mask_ptrs, bit_first + rb, rows_blk, lane);
        lds_fence();      // the basis rows and the bit image are rewritten next
    }
    // ---- the unit's sums: lane e = (sum w, store task g) adds the 64 cells of the task's slot, cell e first, or takes
    // the slot's one cell
    lds_fence();
    if (lane < 2 * T) {
        const int w = lane / T, g = lane % T, j = SLOT[g];
        double s = 0.0;
        if (j >= 0 && cells)
            for (int i = 0; i < 64; ++i) s += AB[(w * nop + j) * 64 + ((i + lane) & 63)];
        else if (j >= 0)
            s = AB[w * nop + j];
        mine[lane] = s;
    }
}

// state [2][T] += the plan's units in ascending order: thread (run c, column j) adds the units of run c, a contiguous
// 1 / nch of the table, in ascending order; then thread j adds the runs in ascending order.  One block: the order is a
// function of (n_units, T) alone.
__global__ __launch_bounds__(1024) void k_emr_finish(const double *__restrict__ table, int n_units, int T,
                                                     double *__restrict__ state) {
    __shared__ double part[1024];
    const int cols = 2 * T, nch = 1024 / cols;
    const int tid = threadIdx.x, j = tid % cols, c = tid / cols;
    if (c < nch) {
        const int per = (n_units + nch - 1) / nch;
        const int u0 = c * per, u1 = u0 + per < n_units ? u0 + per : n_units;
        double s = 0.0;
#pragma unroll 8
        for (int u = u0; u < u1; ++u) s += table[(size_t)u * cols + j];
        part[tid] = s;
    }
    __syncthreads();
    if (tid < cols) {
        double s = state[tid];
        for (int q = 0; q < nch; ++q) s += part[q * cols + tid];
        state[tid] = s;
    }
}

// ------------------------------------------------------------------------------------ the task model
// out[d] = base[d] + lambda * (M[d] ? tau_uni[d] : +0) over the whole model in one launch.  LDS: the prefix table
// PRE [P + 1] of the parameters' rows, built by every block.  The grid strides over chunks of EMR_CHUNK rows of the
// concatenated row space; a block finds its chunk's first parameter by bisection and walks on from there.  Inside a
// parameter a thread owns 4 consecutive rows that start at a multiple of 4 (16-byte loads and stores where the
// parameter's three pointers allow them and the 4 rows lie inside the block's range), a wave 256: lanes 0 .. 8 read the
// at most 9 stream words of the wave's rows once, turn them least-significant-bit-first, and every lane takes the two
// words its 4 bits can lie in from them by a shuffle.
#define EMR_CHUNK 4096
#define EMR_APPLY_THREADS 256
#define EMR_APPLY_MAX_PARAMS 7679      // (P + 1) int64 beside the 2 KB of run totals in 64 KB of LDS

__global__ __launch_bounds__(EMR_APPLY_THREADS) void k_emr_apply(int P, const int64_t *__restrict__ rows_dev,
                                                                 const int64_t *__restrict__ bit_base,
                                                                 const float *const *__restrict__ uni_ptrs,
                                                                 const uint32_t *__restrict__ stream, float lambda,
                                                                 const float *const *__restrict__ base_ptrs,
                                                                 float *const *__restrict__ out_ptrs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    __shared__ int64_t seg[EMR_APPLY_THREADS];
    int64_t *PRE = reinterpret_cast<int64_t *>(lds_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- the prefix table: a run of parameters per thread, the runs' totals, the runs' offsets
    const int per = (P + EMR_APPLY_THREADS - 1) / EMR_APPLY_THREADS;
    const int q0 = tid * per < P ? tid * per : P, q1 = q0 + per < P ? q0 + per : P;
    int64_t tot = 0;
    for (int q = q0; q < q1; ++q) tot += rows_dev[q] > 0 ? rows_dev[q] : 0;
    seg[tid] = tot;
    __syncthreads();
    int64_t at = 0;
    for (int t = 0; t < tid; ++t) at += seg[t];
    for (int q = q0; q < q1; ++q) {
        PRE[q] = at;
        at += rows_dev[q] > 0 ? rows_dev[q] : 0;
    }
    if (tid == EMR_APPLY_THREADS - 1) PRE[P] = at;
    __syncthreads();
    const int64_t total = PRE[P];
    emr_gcu32 *gs = (emr_gcu32 *)stream;
    for (int64_t c0 = (int64_t)blockIdx.x * EMR_CHUNK; c0 < total; c0 += (int64_t)gridDim.x * EMR_CHUNK) {
        const int64_t c1 = c0 + EMR_CHUNK < total ? c0 + EMR_CHUNK : total;
        int lo = 0, hi = P;      // the last parameter with PRE[p] <= c0: it has rows, since c0 < total
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (PRE[mid] <= c0) lo = mid; else hi = mid;
        }
        for (int p = lo; p < P && PRE[p] < c1; ++p) {
            const int64_t D = PRE[p + 1] - PRE[p];
            mg_gfloat *gu = (mg_gfloat *)uni_ptrs[p];
            mg_gfloat *gb = base_ptrs ? (mg_gfloat *)base_ptrs[p] : nullptr;
            mg_gfloat_w *go = (mg_gfloat_w *)out_ptrs[p];
            if (D <= 0 || !gu || !go) continue;
            const int64_t a = c0 > PRE[p] ? c0 - PRE[p] : 0;                 // the block's rows of the parameter: [a, b)
            const int64_t b = c1 - PRE[p] < D ? c1 - PRE[p] : D;
            const bool vec = (((uintptr_t)gu | (uintptr_t)gb | (uintptr_t)go) & 15u) == 0;
            const int64_t bitb = bit_base[p];
            const int64_t wlast = (bitb + D - 1) >> 5;      // the last stream word that holds a bit of the parameter
            for (int64_t g0 = a & ~(int64_t)3; g0 < b; g0 += 4 * EMR_APPLY_THREADS) {
                const int64_t rw = g0 + 256 * wave;      // the wave's first row
                if (rw >= b) continue;                   // wave-uniform
                const int64_t Bw = bitb + rw, w0 = Bw >> 5;
                unsigned word = 0u;
                if (lane < 9 && w0 + lane <= wlast) word = __brev(__builtin_bswap32(gs[w0 + lane]));
                const int bl = (int)(Bw & 31) + 4 * lane;      // the lane's first bit, counted from bit 0 of word w0
                const unsigned wl = (unsigned)__shfl((int)word, bl >> 5, 64);
                const unsigned wh = (unsigned)__shfl((int)word, (bl >> 5) + 1, 64);
                const unsigned bits = (unsigned)(((((store_u64)wh) << 32) | wl) >> (bl & 31)) & 15u;
                const int64_t r = rw + 4 * lane;
                if (r >= b) continue;
                if (vec && r >= a && r + 4 <= b) {
                    const f32x4 t4 = *(mg_gf32x4 *)(gu + r);
                    f32x4 o4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o4[e] = __fmul_rn(lambda, ((bits >> e) & 1u) ? t4[e] : 0.f);
                    if (gb) {
                        const f32x4 b4 = *(mg_gf32x4 *)(gb + r);
#pragma unroll
                        for (int e = 0; e < 4; ++e) o4[e] = __fadd_rn(b4[e], o4[e]);
                    }
                    *(emr_gf32x4_w *)(go + r) = o4;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (r + e < a || r + e >= b) continue;
                        float o = __fmul_rn(lambda, ((bits >> e) & 1u) ? gu[r + e] : 0.f);
                        if (gb) o = __fadd_rn(gb[r + e], o);
                        go[r + e] = o;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------ entry points
extern "C" int64_t svdq_emr_state_bytes(int32_t n_tasks) {
    if (n_tasks < 1 || n_tasks > SVDQ_MAX_TASKS) return 0;
    return svdq_align_up((int64_t)2 * n_tasks * 8, 256);
}

// the coefficient scratch of svdq_task_reconstruct_work_bytes, then the per-unit table [n_units][2][T] doubles
static int64_t emr_coeff_bytes(const svdq_plan *pl, int32_t n_out) {
    return svdq_align_up((int64_t)pl->n_params * n_out * pl->n_tasks * 4, 256);
}
extern "C" int64_t svdq_emr_work_bytes(const svdq_plan *pl, int32_t n_out, int32_t n_tasks) {
    if (!pl || n_out < 1 || n_out > SVDQ_MAX_TASKS || n_tasks < 1 || n_tasks > SVDQ_MAX_TASKS) return 0;
    return emr_coeff_bytes(pl, n_out) + svdq_align_up((int64_t)pl->n_units * 2 * n_tasks * 8, 256);
}

extern "C" int svdq_plan_emr_elect(const svdq_plan *pl, const int64_t *rows_dev, const void *small, const void *basis,
                                   const float *mean, const int32_t *slot_task, const int32_t *task_map, int32_t n_out,
                                   int32_t n_tasks, const int64_t *bit_base, const void *uni_ptrs, const void *mask_ptrs,
                                   void *state, void *work, void *stream) {
    const char *who = "svdq_plan_emr_elect";
    if (int rc = store_args_ok(who, pl, small, basis, mean, slot_task, task_map, n_out, n_tasks, state, work)) return rc;
    if (!bit_base || !uni_ptrs || !mask_ptrs) {
        svdq_set_error("%s: bit_base, uni_ptrs and mask_ptrs are required", who);
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const int n = pl->n_tasks;
    const uint8_t *bs = reinterpret_cast<const uint8_t *>(basis);
    const float *mn = pl->cfg.center ? mean : nullptr;
    float *cbar = reinterpret_cast<float *>(work);
    double *table = reinterpret_cast<double *>(reinterpret_cast<uint8_t *>(work) + emr_coeff_bytes(pl, n_out));
    auto up = reinterpret_cast<float *const *>(uni_ptrs);
    auto mp = reinterpret_cast<uint32_t *const *>(mask_ptrs);
    const int rc = store_stream(who, pl, small, slot_task, task_map, (int)n_out, cbar, st,
                              [&](auto f16_c, auto tg_c, auto rpl_c, const SmallView &sv, int nop) {
                                  constexpr bool F16 = f16_c;
                                  constexpr int TG = tg_c, RPL = rpl_c;
                                  using Plain = StreamLds<F16, RPL, false>;
                                  hipLaunchKernelGGL((k_emr_elect<F16, TG, RPL>), dim3(pl->n_units), dim3(64),
                                                     Plain::bytes(n, nop, EmrLds<RPL>::words(nop, (int)n_tasks)), st,
                                                     pl->d_params, pl->d_units, rows_dev, n, (int)n_out, (int)n_tasks,
                                                     slot_task, task_map, sv.k, sv.r, bs, mn, cbar, bit_base, up, mp, table);
                              });
    if (rc != SVDQ_OK) return rc;
    hipLaunchKernelGGL(k_emr_finish, dim3(1), dim3(1024), 0, st, table, (int)pl->n_units, (int)n_tasks,
                       reinterpret_cast<double *>(state));
    return svdq_launch_status(true, who);
}

extern "C" int svdq_emr_apply(int32_t n_params, const int64_t *rows_dev, const int64_t *bit_base, const void *uni_ptrs,
                              const void *mask_stream, float lambda32, const void *base_ptrs, const void *out_ptrs,
                              void *stream) {
    const char *who = "svdq_emr_apply";
    if (!rows_dev || !bit_base || !uni_ptrs || !mask_stream || !out_ptrs) {
        svdq_set_error("%s: rows, bit_base, uni_ptrs, mask_stream and out_ptrs are required", who);
        return SVDQ_EINVAL;
    }
    if (n_params < 1 || n_params > EMR_APPLY_MAX_PARAMS) {
        svdq_set_error("%s: n_params must be in [1, %d], got %d", who, EMR_APPLY_MAX_PARAMS, n_params);
        return SVDQ_EINVAL;
    }
    if (!std::isfinite(lambda32)) {
        svdq_set_error("%s: lambda32 is not finite", who);
        return SVDQ_EINVAL;
    }
    // the grid does not depend on the rows (they are on the device): 8 blocks per CU of a 256-CU device, striding
    hipLaunchKernelGGL(k_emr_apply, dim3(2048), dim3(EMR_APPLY_THREADS), (size_t)(n_params + 1) * 8, (hipStream_t)stream,
                       (int)n_params, rows_dev, bit_base, reinterpret_cast<const float *const *>(uni_ptrs),
                       reinterpret_cast<const uint32_t *>(mask_stream), lambda32,
                       reinterpret_cast<const float *const *>(base_ptrs), reinterpret_cast<float *const *>(out_ptrs));
    return svdq_launch_status(true, who);
}
