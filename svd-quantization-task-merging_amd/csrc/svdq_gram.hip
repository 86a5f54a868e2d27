// svdq_gram.hip -- pass 1 of the SVD-Hybrid compressor: G = Tc^T Tc (k_gram).  Helpers and the layout notes: svdq_stream.h.
#include "svdq_stream.h"
#include "svdq_dispatch.h"

// ------------------------------------------------------------------------------------ pass 1
// One work unit of pass 1 (a run of 256-row blocks of one parameter) by ONE wavefront.
// X: wave-private LDS, gram_lds_floats<NTP, F64>() floats: the strip of NTP*XS floats, and at N <= 8 with exact products
// room for a round of the end-of-unit reduction.
// MODE bit 0: gather through an index list (aux[p] = int32 list); bit 1: the task tensors are fine-tuned weights and a
// base tensor is subtracted in registers (aux2[p] = base).  0 = contiguous task vectors, 3 = both.
// F64: exact fp32 x fp32 products and fp64 running sums over the whole unit -- in registers with v_fma_f64 at N <= 8
// (the register form below), on the fp64 MFMA above (v_mfma_f64_4x4x4 at N = 9..12, v_mfma_f64_16x16x4 at 13..16) --
// which resolves singular values down to ~1e-6 sigma_0 like the reference's LAPACK path; the fp32 form (fp32 sums
// inside a 256-row block) only reaches ~1e-3..1e-4 sigma_0.  Pass 1 is HBM-bound for N <= 16, so the fp64 form is the
// default there; N > 16 would become MFMA-bound and keeps fp32 products.
// TIN: element type of the task / base tensors (svdq_input.h), widened to fp32 by the loaders; float for the walk.
// SIDE (MODE 0 / 2 only; the task-Gram by-product, svdq_plan_task_gram): beside the Gram of the centred rows Tc the
// unit sums a[t] = sum_rows Tc[row][t] m[row] and s = sum_rows m[row]^2 (m = the row mean that was subtracted), from
// which T^T T = Tc^T Tc + a 1^T + 1 a^T + s 1 1^T.  fp32 inside a block: an explicit fma chain over the lane's four
// rows (so every instantiation rounds alike), then the 64 lane values of one sum at a time meet in side_wave_sum
// (fixed order) and lane i keeps sum i, which it carries in fp64 across the blocks of the unit -- a handful of
// registers, where N + 1 fp64 lane accumulators, and a reduce-scatter of all N + 1 lane values at once, cost the
// N <= 8 and N <= 16 kernels their launch bounds (spills) and N = 20 its second wave.
// side_part[unit][NT + 1].  The Gram partials are those of the SIDE = false kernel, bit for bit (above 8 tasks the strip
// in LDS and the MFMA phase are; the register form takes the lane's rows for the side sums from its registers).
// Sum of x over the 64 lanes, the same bits in every lane: inside a row of 16 lanes four DPP adds (lane ^ 1, lane ^ 2,
// the mirror of the half row, the mirror of the row: both lanes of a pair add the same two numbers), across the four
// rows two shuffles.  In place: one value at a time needs one register.
template <int CTRL>
__device__ __forceinline__ float side_dpp_add(float x) {
    return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float side_wave_sum(float x) {
    x = side_dpp_add<0xB1>(x);    // quad_perm [1, 0, 3, 2]
    x = side_dpp_add<0x4E>(x);    // quad_perm [2, 3, 0, 1]
    x = side_dpp_add<0x141>(x);   // row_half_mirror
    x = side_dpp_add<0x140>(x);   // row_mirror
    x += __shfl_xor(x, 16);
    x += __shfl_xor(x, 32);
    return x;
}

// Register form (N <= 8, exact products).  The lane that loads a block holds rows 4l..4l+3 of every task, and the Gram
// is a sum of per-row outer products: per row the lane converts its NTP centred values to fp64 once and adds the
// NTP (NTP + 1) / 2 products on or above the diagonal to fp64 accumulators of its own with v_fma_f64 (a product of two
// fp32 values is exact in fp64, so an entry is the correctly rounded running sum of exact products, as on the fp64
// MFMA).  32 conversions and 144 FMAs per 256-row block at N = 8, where the v_mfma_f64_4x4x4 form this replaced paid
// 8 + 32 LDS instructions, 128 conversions (every 4x4x4 instruction wants two freshly converted operands per lane) and
// 64 MFMAs to re-shape the same registers.  v_fma_f64 issues at the rate of v_fma_f32 on gfx950, v_cvt_f64_f32 at 0.6
// of it (tools/probe/valu_f64_rate.hip).  Measured on ViT-L-14, pass 1 alone, MFMA form -> this: x 8 1.67 -> 1.60 ms
// (fp32 inputs), 1.23 -> 1.02 (half); x 5 1.39 -> 1.12; x 4 0.82 -> 0.83; x 2 0.52 -> 0.47.
// Summation order of one entry, which every mode keeps so that the routes stay bit-identical:
//   lane l: the rows 4l + e (e = 0..3) of block 0, then of block 1, ... of the unit, one running sum;
//   across lanes at the end of the unit, through LDS: the lanes q, PER + q, 2 PER + q, ... in turn (PER = 64 / (2 NTP)
//   lanes share an entry), then the PER partial sums in a butterfly (lane ^ 1, ^ 2, ^ 4);
//   the unit's first slot takes the sum, the second is zeros; k_reduce goes on from there.
// Plain and minus-base: two register sets, the block after the one being summed is in flight; no strip in LDS.  With
// 36 fp64 accumulators that is two waves per SIMD (about 200 VGPRs); three waves spill and run at half the speed, one
// set at three waves leaves too little in flight (1.90 ms), a third set at two waves measured the same as two.
// Gather and walk: the strip stays as a transposer -- rows are scattered into it as before and every lane reads rows
// 4l..4l+3 of each task back (NTP ds_read_b128), so a compacted row sits in the lane and the position of the sum where
// the plain kernel has it.
template <int NTP, bool F64>
__host__ __device__ constexpr bool gram_registers() {
    return F64 && NTP <= 8;
}
// LDS floats of k_gram: the strip, or the 2 NTP entries x (64 + PER) lane values (fp64) of one reduction round
template <int NTP, bool F64>
__host__ __device__ constexpr int gram_lds_floats() {
    constexpr int strip = NTP * XS, round = 2 * (2 * NTP) * (64 + 64 / (2 * NTP));
    return (gram_registers<NTP, F64>() && round > strip) ? round : strip;
}

template <int NTP, int MODE = 0, bool F64 = false, bool FULL = false, typename TIN = float, bool SIDE = false>
__device__ __forceinline__ void gram_unit(float *X, int uidx, const SvdqParam *__restrict__ params,
                                          const SvdqUnit *__restrict__ units,
                                          const float *const *__restrict__ ptrs,
                                          const int64_t *__restrict__ rows_dev, int NT_arg, int center,
                                          double *__restrict__ gram_part,
                                          const void *const *__restrict__ aux = nullptr,
                                          const int32_t *__restrict__ only = nullptr,
                                          const void *const *__restrict__ aux2 = nullptr,
                                          const int64_t *__restrict__ ustart = nullptr,
                                          double *__restrict__ side_part = nullptr) {
    static_assert(!SIDE || (MODE & ~2) == 0, "the side sums exist for plain deltas and minus-base only");
    constexpr bool GATHER = (MODE & 1) != 0, SUB = (MODE & 2) != 0, WALK = (MODE & 4) != 0;
    static_assert(!(GATHER && WALK), "index lists and the mask walk are alternatives");
    static_assert(!(MODE != 0 && SVDQ_PREFETCH2), "gather / minus-base support the one-block-ahead pipeline only");
    static_assert(!WALK || sizeof(TIN) == 4, "the mask walk reads fp32 tensors only");
    const int NT = FULL ? NTP : NT_arg;      // FULL: the plan has exactly NTP tasks, the "task t is real" tests fold away
    constexpr int PACK = (NTP <= 8) ? 2 : 1;
    constexpr int NB = (NTP + 15) / 16;
    // N = 17..20: of the 2x2-blocked Gram only AA is a full 16 x 16 tile; AB is 16 x 4 and BB 4 x 4.  A 16x16x4 MFMA per
    // k-step for each of them wastes 3/4 and 15/16 of the matrix pipe, and pass 1 at N = 20 is MFMA-issue-bound
    // (SQ_WAIT_INST_ANY 69 %, MFMA busy 58 %).  They are taken by v_mfma_f32_4x4x1_16b_f32 instead -- sixteen 4x4 outer
    // products per instruction, 8 cycles:  AB: block (mg, rg) = tasks 4mg..4mg+3 x tasks 16..19 on row 4rg + e of the
    // sub-tile (four instructions per 16 rows);  BB: block b = row b of the sub-tile (one instruction per 16 rows).
    // 2 688 matrix-pipe cycles per 256-row block instead of 4 096 plus the vector-ALU corner.
    constexpr bool VBB = (NTP == 20) && !F64;
    constexpr int NACC = (NB == 1 || VBB) ? 1 : 3;  // AA | AA, AB, BB
    // N = 9..12 with exact products: v_mfma_f64_4x4x4_4b_f64 (four independent 4 x 4 blocks, K = 4 rows, 16 cycles)
    // over the six 4 x 4 tiles on or above the diagonal, four per instruction, so two instructions per four rows: 32
    // matrix-pipe cycles against 64 for the 16x16x4 form (3.21 -> 2.98 ms at N = 12).  Layout probed on the device
    // (tools/probe/mfma_f64_layout.hip): lane l = (k = l >> 4, b = (l >> 2) & 3, x = l & 3) supplies A_b[x][k] and
    // B_b[k][x] and holds D_b[i = l >> 4][j = l & 3].  The lane's k selects rows 4k..4k+3 of a 16-row sub-tile (one
    // 16-byte LDS read per operand), the four instructions of a sub-tile take one of them each.  (Ten tiles in three
    // instructions at N = 13..16 were measured SLOWER than the 16x16x4 form -- 4.62 against 3.58 ms at ViT-L-14 x 16:
    // every 4x4x4 instruction needs two converted operands per lane, eight times the v_cvt_f64_f32 work per output.
    // N <= 8 ran on this instruction too, one or four tiles, until the register form took it over.)
    constexpr bool Q64 = F64 && NTP > 8 && NTP <= 12;
    constexpr int TQ = NTP / 4;
    constexpr int NTILE = TQ * (TQ + 1) / 2;
    constexpr int NSET = (NTILE + 3) / 4;
    // N <= 8 with exact products: no matrix pipe at all (REG, "register form" in the notes above gram_unit).
    constexpr bool REG = gram_registers<NTP, F64>();
    constexpr int NRACC = NTP * (NTP + 1) / 2;

    const int lane = threadIdx.x & 63;
    const SvdqUnit ud = units[uidx];
    const int p = ud.param;
    if (only && !only[p]) return;  // refinement pass (N > 16): only the parameters the eigen-stage flagged
    const int64_t D = rows_dev ? rows_dev[p] : params[p].rows;
    const int64_t r_begin = ud.row0;
    int64_t r_end = r_begin + ud.nrows;
    if (r_end > D) r_end = D;

    gin<TIN> *bp[NTP];
#pragma unroll
    for (int t = 0; t < NTP; ++t) bp[t] = (gin<TIN> *)ptrs[(size_t)p * NT + (t < NT ? t : NT - 1)];

    const int c = lane & 15, g = lane >> 4;
    double accd[NACC][4];
#pragma unroll
    for (int i = 0; i < NACC; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) accd[i][e] = 0.0;

#ifndef SVDQ_GRAM64_CHAINS
#define SVDQ_GRAM64_CHAINS 1
#endif
    constexpr int QC = (NB == 1) ? SVDQ_GRAM64_CHAINS : 1;  // F64: independent accumulation chains per block
    f64x4 accq[NACC * QC];
#pragma unroll
    for (int i = 0; i < NACC * QC; ++i) accq[i] = f64x4{0.0, 0.0, 0.0, 0.0};

    double q64[Q64 ? NSET : 1];   // Q64: this lane's Gram entries (one per instruction of a step), over the whole unit
#ifndef SVDQ_Q64_CHAINS
#define SVDQ_Q64_CHAINS 2   // independent accumulation chains per entry (even / odd k-steps), added at the end of the unit
#endif
    double q64b[(Q64 && SVDQ_Q64_CHAINS == 2) ? NSET : 1];
#pragma unroll
    for (int i = 0; i < (Q64 ? NSET : 1); ++i) q64[i] = 0.0;
#pragma unroll
    for (int i = 0; i < ((Q64 && SVDQ_Q64_CHAINS == 2) ? NSET : 1); ++i) q64b[i] = 0.0;
    // tile (ti <= tj) number q in row-major order of the upper triangle
    auto tile_of = [](int q, int &ti, int &tj) {
        ti = 0;
        int rowlen = TQ;
        while (q >= rowlen) {
            q -= rowlen;
            --rowlen;
            ++ti;
        }
        tj = ti + q;
    };
    double qd[2][4];  // VBB: AB and BB block partials of the 4x4x1 chains (fp32 inside a block, fp64 across)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) qd[i][e] = 0.0;
    const int b4 = lane >> 2, i4 = lane & 3, mg4 = b4 & 3, rg4 = b4 >> 2;
    double side = 0.0;   // SIDE: lane t < NT: a[t], lane NTP: s, over the whole unit
    double racc[REG ? NRACC : 1];   // REG: entries (i <= j) of this lane's rows in row-major order, over the whole unit
#pragma unroll
    for (int i = 0; i < (REG ? NRACC : 1); ++i) racc[i] = 0.0;
    // REG: the lane's four rows of a block (centred, zero in padded tasks and past the end), row after row
    auto accumulate = [&](const f32x4 (&xc)[NTP]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double d[NTP];
#pragma unroll
            for (int t = 0; t < NTP; ++t) d[t] = (double)xc[t][e];
            int q = 0;
#pragma unroll
            for (int i = 0; i < NTP; ++i)
#pragma unroll
                for (int j = i; j < NTP; ++j, ++q) racc[REG ? q : 0] = __builtin_fma(d[i], d[j], racc[REG ? q : 0]);
            __builtin_amdgcn_sched_barrier(0);   // one converted row at a time: converting ahead costs registers, not time
        }
    };
    // SIDE: a[t] and s of one block from the lane's centred rows xc(t) and the mean that was subtracted
    auto side_block = [&](const f32x4 &mean, auto xc) {
        float s = mean.x * mean.x;
        s = __builtin_fmaf(mean.y, mean.y, s);
        s = __builtin_fmaf(mean.z, mean.z, s);
        s = __builtin_fmaf(mean.w, mean.w, s);
        s = side_wave_sum(s);
        float mine = (lane == NTP) ? s : 0.f;
#pragma unroll
        for (int t = 0; t < NTP; ++t) {
            if (t < NT) {
                const f32x4 x = xc(t);
                float a = x.x * mean.x;
                a = __builtin_fmaf(x.y, mean.y, a);
                a = __builtin_fmaf(x.z, mean.z, a);
                a = __builtin_fmaf(x.w, mean.w, a);
                a = side_wave_sum(a);
                mine = (lane == t) ? a : mine;
            }
        }
        side += (double)mine;
    };

    // The loads of the next block (or next two, SVDQ_PREFETCH2) are in flight while a block is computed.
    constexpr int AHEAD = SVDQ_PREFETCH2 ? 2 : 1;
    f32x4 v0[NTP];
    gint *gidx = nullptr;
    i32x4 ixn = {-1, -1, -1, -1};  // indices of the block after the one whose data is in flight
    gin<TIN> *gbase = nullptr;
    f32x4 vb = zero4();  // base rows of the block whose fine-tuned rows sit in v
    if constexpr (SUB) gbase = (gin<TIN> *)aux2[p];
    if constexpr (WALK) {
        // loads are issued by the walk loop below
    } else if constexpr (GATHER) {
        gidx = (gint *)aux[p];
        if (r_begin < r_end) {
            const i32x4 ix0 = load_idx(gidx, r_begin, D, lane);
            load_block_gather<NTP, TIN>(v0, bp, ix0, r_begin + SVDQ_BLK_ROWS <= D);
            if constexpr (SUB) vb = load_base_gather<TIN>(gbase, ix0, r_begin + SVDQ_BLK_ROWS <= D);
            if (r_begin + SVDQ_BLK_ROWS < r_end) ixn = load_idx(gidx, r_begin + SVDQ_BLK_ROWS, D, lane);
        }
    } else {
        if (r_begin < r_end) load_block<NTP, TIN>(v0, bp, r_begin, D, lane);
        if constexpr (SUB) {
            if (r_begin < r_end) vb = load_base<TIN>(gbase, r_begin, D, lane);
        }
    }
#if SVDQ_PREFETCH2
    f32x4 v1[NTP];
    if (r_begin + SVDQ_BLK_ROWS < r_end) load_block<NTP, TIN>(v1, bp, r_begin + SVDQ_BLK_ROWS, D, lane);
#endif

    // the MFMA phase over the strip of one block (ends with the barrier that frees the strip)
    auto compute = [&]() {
        if constexpr (REG) {   // gather / walk: the strip only transposes, every lane takes rows 4l..4l+3 back
            f32x4 xr[NTP];
#pragma unroll
            for (int t = 0; t < NTP; ++t) xr[t] = *reinterpret_cast<const f32x4 *>(X + t * XS + 4 * lane);
            accumulate(xr);
            wave_sync();
            return;
        }
        f32x4 acc[NACC];
#pragma unroll
        for (int i = 0; i < NACC; ++i) acc[i] = zero4();
        f32x4 qab = zero4(), qbb = zero4();

        if constexpr (Q64) {
            const int kq = lane >> 4, bq = (lane >> 2) & 3, xq = lane & 3;
            const float *pa[NSET], *pb[NSET];
#pragma unroll
            for (int st = 0; st < NSET; ++st) {
                int ti, tj;
                const int q = 4 * st + bq;
                tile_of(q < NTILE ? q : NTILE - 1, ti, tj);   // spare blocks repeat the last tile, unused
                pa[st] = X + (4 * ti + xq) * XS + 4 * kq;
                pb[st] = X + (4 * tj + xq) * XS + 4 * kq;
            }
UNROLL_N(SVDQ_UNROLL_GRAM)
            for (int j = 0; j < 16; ++j) {
#pragma unroll
                for (int st = 0; st < NSET; ++st) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(pa[st] + 16 * j);
                    const f32x4 b = *reinterpret_cast<const f32x4 *>(pb[st] + 16 * j);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (SVDQ_Q64_CHAINS == 2 && (e & 1))
                            q64b[st] = __builtin_amdgcn_mfma_f64_4x4x4f64((double)a[e], (double)b[e], q64b[st], 0, 0, 0);
                        else
                            q64[st] = __builtin_amdgcn_mfma_f64_4x4x4f64((double)a[e], (double)b[e], q64[st], 0, 0, 0);
                    }
                }
            }
        } else if constexpr (PACK == 2) {
            const int t = c & 7;
            const bool valid = t < NTP;
            const float *xr = X + (valid ? t : 0) * XS + 16 * (c >> 3) + 4 * g;
UNROLL_N(SVDQ_UNROLL_GRAM)
            for (int j = 0; j < 8; ++j) {
                f32x4 a = *reinterpret_cast<const f32x4 *>(xr + 32 * j);
                if (!valid) a = zero4();
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[0] = mfma4(a[e], a[e], acc[0]);   // fp32 products only: F64 is REG here
            }
        } else {
            const bool v0ok = c < NTP;
            const bool v1ok = (NB == 2) && (16 + c < NTP);
            const float *x0 = X + (v0ok ? c : 0) * XS + 4 * g;
            const float *x1 = X + (v1ok ? 16 + c : 0) * XS + 4 * g;
UNROLL_N(SVDQ_UNROLL_GRAM_P1)
            for (int j = 0; j < 16; ++j) {
                f32x4 a0 = *reinterpret_cast<const f32x4 *>(x0 + 16 * j);
                if (!v0ok) a0 = zero4();
                if constexpr (F64 && NB == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double ad = (double)a0[e];
                        accq[e % QC] = mfma4d(ad, ad, accq[e % QC]);
                    }
                } else if constexpr (F64) {
                    f32x4 a1 = *reinterpret_cast<const f32x4 *>(x1 + 16 * j);
                    if (!v1ok) a1 = zero4();
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double d0 = (double)a0[e], d1 = (double)a1[e];
                        accq[0] = mfma4d(d0, d0, accq[0]);
                        accq[1] = mfma4d(d0, d1, accq[1]);
                        accq[2] = mfma4d(d1, d1, accq[2]);
                    }
                } else if constexpr (NB == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[0] = mfma4(a0[e], a0[e], acc[0]);
                } else if constexpr (VBB) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[0] = mfma4(a0[e], a0[e], acc[0]);
                    const f32x4 xa = *reinterpret_cast<const f32x4 *>(X + (4 * mg4 + i4) * XS + 16 * j + 4 * rg4);
                    const f32x4 xq = *reinterpret_cast<const f32x4 *>(X + (16 + i4) * XS + 16 * j + 4 * rg4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) qab = mfma_4x4x1(xa[e], xq[e], qab);
                    const float xr = X[(16 + i4) * XS + 16 * j + b4];
                    qbb = mfma_4x4x1(xr, xr, qbb);
                } else {
                    f32x4 a1 = *reinterpret_cast<const f32x4 *>(x1 + 16 * j);
                    if (!v1ok) a1 = zero4();
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[0] = mfma4(a0[e], a0[e], acc[0]);
                        acc[1] = mfma4(a0[e], a1[e], acc[1]);
                        acc[2] = mfma4(a1[e], a1[e], acc[2]);
                    }
                }
            }
        }
        if constexpr (!F64) {
#pragma unroll
            for (int i = 0; i < NACC; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) accd[i][e] += (double)acc[i][e];
            if constexpr (VBB) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    qd[0][e] += (double)qab[e];
                    qd[1][e] += (double)qbb[e];
                }
            }
        }
        wave_sync();
    };

    if constexpr (WALK) {
        // walk the source rows from this unit's first selected element (see "walk mode" above)
        gbyte *gmask = (gbyte *)aux[p];
        const int64_t Dsrc = params[p].rows;
        const int64_t us = ustart[uidx];
        const int inv = (us & SVDQ_WALK_INV) ? 1 : 0;
        int64_t src = us & (SVDQ_WALK_INV - 1);
        int64_t src_end = Dsrc;      // where the next unit's rows begin
        if (uidx + 1 < params[p].unit_begin + params[p].unit_count) src_end = ustart[uidx + 1] & (SVDQ_WALK_INV - 1);
        if (src_end > Dsrc) src_end = Dsrc;
        const int need = (r_begin < r_end) ? (int)(r_end - r_begin) : 0;
        int produced = 0, fill = 0;
        unsigned mk[4];
        bool have = need > 0 && src < src_end;
        if (have) walk_load<NTP, SUB>(v0, vb, mk, bp, gbase, gmask, src, src_end, lane);
        bool more = need > 0;
        while (more) {
            const int fill0 = fill;
            WalkSel w;
            w.total = SVDQ_BLK_ROWS;      // no chunk left: flush the partial block
            if (have) {
                w = walk_select(mk, inv, fill0);
                if constexpr (SUB) {
#pragma unroll
                    for (int t = 0; t < NTP; ++t) v0[t] = v0[t] - vb;
                }
                const f32x4 mean = row_mean<NTP>(v0, NT, center);
#pragma unroll
                for (int t = 0; t < NTP; ++t) v0[t] = (t < NT) ? (v0[t] - mean) : zero4();
                walk_scatter<NTP>(X, v0, w, 0);
            } else {
                walk_zero_tail<NTP>(X, fill0, lane);
            }
            if (w.total >= SVDQ_BLK_ROWS) {
                wave_sync();
                compute();
                if (have) walk_scatter<NTP>(X, v0, w, SVDQ_BLK_ROWS);
                fill = have ? w.total - SVDQ_BLK_ROWS : 0;
            } else {
                fill = w.total;
            }
            if (have) {
                produced += w.total - fill0;
                src += SVDQ_BLK_ROWS;
            }
            have = have && produced < need && src < src_end;
            if (have) walk_load<NTP, SUB>(v0, vb, mk, bp, gbase, gmask, src, src_end, lane);
            more = have || fill > 0;
        }
    } else if constexpr (REG && !GATHER) {
        // straight from the load registers; two sets, so that the next block is in flight while one is summed
        f32x4 v1[NTP];
        f32x4 vb1 = zero4();
        auto take = [&](f32x4 (&v)[NTP], const f32x4 &b) {
            if constexpr (SUB) {
#pragma unroll
                for (int t = 0; t < NTP; ++t) v[t] = v[t] - b;
            }
            const f32x4 mean = row_mean<NTP>(v, NT, center);
#pragma unroll
            for (int t = 0; t < NTP; ++t) v[t] = (t < NT) ? (v[t] - mean) : zero4();
            if constexpr (SIDE) side_block(mean, [&](int t) { return v[t]; });
            accumulate(v);
        };
        // the loads of a set are issued where they stand, after the last use of the set they refill: hoisted into the
        // sums before them they would need a third set of registers
        auto refill = [&](f32x4 (&v)[NTP], f32x4 &b, int64_t rb) {
            __builtin_amdgcn_sched_barrier(0);
            if (rb < r_end) {
                load_block<NTP, TIN>(v, bp, rb, D, lane);
                if constexpr (SUB) b = load_base<TIN>(gbase, rb, D, lane);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        // set 0 holds the even blocks of the unit, set 1 the odd ones: summed, then refilled at once two blocks on
        refill(v1, vb1, r_begin + SVDQ_BLK_ROWS);
#pragma nounroll
        for (int64_t rb = r_begin; rb < r_end; rb += 2 * SVDQ_BLK_ROWS) {
            take(v0, vb);
            refill(v0, vb, rb + 2 * SVDQ_BLK_ROWS);
            if (rb + SVDQ_BLK_ROWS < r_end) take(v1, vb1);
            refill(v1, vb1, rb + 3 * SVDQ_BLK_ROWS);
        }
    } else {
        auto do_block = [&](f32x4 (&v)[NTP], int64_t rb) {
            if constexpr (SUB) {
#pragma unroll
                for (int t = 0; t < NTP; ++t) v[t] = v[t] - vb;
            }
            const f32x4 mean = center_store<NTP, GATHER>(v, NT, center, X, lane);
            wave_sync();
            if (rb + AHEAD * SVDQ_BLK_ROWS < r_end) {
                if constexpr (GATHER) {
                    load_block_gather<NTP, TIN>(v, bp, ixn, rb + 2 * SVDQ_BLK_ROWS <= D);
                    if constexpr (SUB) vb = load_base_gather<TIN>(gbase, ixn, rb + 2 * SVDQ_BLK_ROWS <= D);
                    if (rb + 2 * SVDQ_BLK_ROWS < r_end) ixn = load_idx(gidx, rb + 2 * SVDQ_BLK_ROWS, D, lane);
                } else {
                    load_block<NTP, TIN>(v, bp, rb + AHEAD * SVDQ_BLK_ROWS, D, lane);
                    if constexpr (SUB) vb = load_base<TIN>(gbase, rb + AHEAD * SVDQ_BLK_ROWS, D, lane);
                }
            }
            if constexpr (SIDE) {   // the lane's own four rows of every task, back from the strip (v is being refilled)
                side_block(mean, [&](int t) { return *reinterpret_cast<const f32x4 *>(X + t * XS + 4 * lane); });
            }
            compute();
        };
        for (int64_t rb = r_begin; rb < r_end; rb += AHEAD * SVDQ_BLK_ROWS) {
            do_block(v0, rb);
#if SVDQ_PREFETCH2
            if (rb + SVDQ_BLK_ROWS < r_end) do_block(v1, rb + SVDQ_BLK_ROWS);
#endif
        }
    }
    if constexpr (F64) {
#pragma unroll
        for (int i = 0; i < NACC; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double t = accq[i * QC][e];
#pragma unroll
                for (int q = 1; q < QC; ++q) t += accq[i * QC + q][e];
                accd[i][e] = t;
            }
    }

    if constexpr (SIDE) {   // every unit writes its NT + 1 numbers, zeros included
        if (lane < NT || lane == NTP) side_part[(size_t)uidx * (NT + 1) + (lane < NT ? lane : NT)] = side;
    }

    // One fp64 partial per slot, dense [NT][NT].  Lane (c,g) holds D[4g+e][c] (fp32 MFMA) or D[g+4e][c] (fp64 MFMA).
    const int NN = NT * NT;
    if constexpr (REG) {
        // The 64 lane sums of an entry meet in LDS, R entries a round: lane (v, q) = (lane / PER, lane % PER) adds the
        // values of lanes q, PER + q, ... of entry v in turn, the PER partial sums meet in a butterfly.  Rows of
        // 64 + PER doubles: the lanes of one read touch different banks.
        constexpr int R = 2 * NTP, PER = 64 / R, S = 64 + PER;
        static_assert(2 * R * S <= gram_lds_floats<NTP, F64>(), "a reduction round must fit the kernel's LDS");
        double *red = reinterpret_cast<double *>(X);
        const int rv = lane / PER, rq = lane % PER;
        double *dst = gram_part + (size_t)uidx * PACK * NN;
#pragma unroll
        for (int r0 = 0; r0 < NRACC; r0 += R) {
            wave_sync();
#pragma unroll
            for (int i = 0; i < R; ++i)
                if (r0 + i < NRACC) red[i * S + lane] = racc[r0 + i];
            wave_sync();
            double x = red[rv * S + rq];
#pragma unroll
            for (int k = 1; k < R; ++k) x += red[rv * S + k * PER + rq];
#pragma unroll
            for (int off = 1; off < PER; off <<= 1) x += __shfl_xor(x, off);
            int ei = 0, ej = r0 + rv, rowlen = NTP;   // entry number -> (ei <= ej), row-major over the upper triangle
            while (ej >= rowlen && rowlen > 0) {
                ej -= rowlen;
                --rowlen;
                ++ei;
            }
            ej += ei;
            if (rq == 0 && r0 + rv < NRACC && ej < NT) {   // ei <= ej
                dst[ei * NT + ej] = x;
                dst[ej * NT + ei] = x;
                dst[NN + ei * NT + ej] = 0.0;
                dst[NN + ej * NT + ei] = 0.0;
            }
        }
        return;
    }
    if constexpr (Q64 && SVDQ_Q64_CHAINS == 2) {
#pragma unroll
        for (int st = 0; st < NSET; ++st) q64[st] += q64b[st];
    }
    if constexpr (Q64) {
        const int i = lane >> 4, bq = (lane >> 2) & 3, jq = lane & 3;
        double *dst = gram_part + (size_t)uidx * PACK * NN;
#pragma unroll
        for (int st = 0; st < NSET; ++st) {
            const int q = 4 * st + bq;
            if (q < NTILE) {
                int ti, tj;
                tile_of(q, ti, tj);
                const int m = 4 * ti + i, n = 4 * tj + jq;
                if (m < NT && n < NT) {
                    dst[m * NT + n] = q64[st];
                    if (ti != tj) dst[n * NT + m] = q64[st];
                }
            }
        }
    } else if constexpr (PACK == 2) {
        const int rs = c >> 3, n = c & 7;
        double *dst = gram_part + ((size_t)uidx * 2 + rs) * NN;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m = F64 ? g + 4 * e : 4 * g + e;
            if ((m >> 3) == rs && (m & 7) < NT && n < NT) dst[(m & 7) * NT + n] = accd[0][e];
        }
    } else {
        double *dst = gram_part + (size_t)uidx * NN;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m = F64 ? g + 4 * e : 4 * g + e;
            if (m < NT && c < NT) dst[m * NT + c] = accd[0][e];
            if constexpr (NB == 2 && !VBB) {
                if (m < NT && 16 + c < NT) {
                    dst[m * NT + 16 + c] = accd[1][e];
                    dst[(16 + c) * NT + m] = accd[1][e];
                }
                if (16 + m < NT && 16 + c < NT) dst[(16 + m) * NT + 16 + c] = accd[2][e];
            }
        }
        if constexpr (VBB) {   // block partials meet in fixed-order shuffles
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // AB: lane (block (mg, rg), j) register e = [task 4mg + e][task 16 + j] over the rows of row group rg
                double x = qd[0][e];
                x += __shfl_xor(x, 16);
                x += __shfl_xor(x, 32);
                const int m = 4 * mg4 + e;
                if (rg4 == 0 && m < NT && 16 + i4 < NT) {
                    dst[m * NT + 16 + i4] = x;
                    dst[(16 + i4) * NT + m] = x;
                }
                // BB: lane (block b, j) register e = [task 16 + e][task 16 + j] over the rows b mod 16
                double y = qd[1][e];
#pragma unroll
                for (int off = 4; off < 64; off <<= 1) y += __shfl_xor(y, off);
                if (b4 == 0 && 16 + e < NT && 16 + i4 < NT) dst[(16 + e) * NT + 16 + i4] = y;
            }
        }
    }
}

// second launch bound = waves per SIMD the register allocation must leave room for: the fp64 accumulators would
// otherwise cost the N <= 16 kernels one resident wave (measured: -9 % bandwidth)
#ifndef SVDQ_GRAM64_WAVES16
#define SVDQ_GRAM64_WAVES16 3
#endif
// the register form: 36 fp64 accumulators, one converted row and two sets of load registers need two waves' share of
// the register file at N = 5..8 (see the notes above gram_registers); the 10 accumulators of N <= 4 leave room for 4-5
#ifndef SVDQ_GRAM_REG_WAVES
#define SVDQ_GRAM_REG_WAVES 2
#endif
template <int NTP, int MODE, bool F64>
__host__ __device__ constexpr int gram_waves() {
    if (gram_registers<NTP, F64>()) return SVDQ_GRAM_REG_WAVES;
    if (F64 && (MODE == 0 || MODE == 4) && NTP <= 16) return SVDQ_GRAM64_WAVES16;
    return 1;
}
SVDQ_STAMP_DECL(svdq_stamps_gram)
template <int NTP, int MODE, bool F64, bool FULL, typename TIN>
__global__ __launch_bounds__(64, (gram_waves<NTP, MODE, F64>())) void k_gram(const SvdqParam *__restrict__ params,
                                             const SvdqUnit *__restrict__ units,
                                             const float *const *__restrict__ ptrs,
                                             const int64_t *__restrict__ rows_dev, int NT, int center,
                                             double *__restrict__ gram_part, int unit0,
                                             const void *const *__restrict__ aux,
                                             const int32_t *__restrict__ only,
                                             const void *const *__restrict__ aux2, int order,
                                             const int64_t *__restrict__ ustart) {
    __shared__ __attribute__((aligned(16))) float X[gram_lds_floats<NTP, F64>()];
    SVDQ_STAMP_BEGIN();
    const int uidx = unit0 + unit_of_block((int)blockIdx.x, (int)gridDim.x, order);
    gram_unit<NTP, MODE, F64, FULL, TIN>(X, uidx, params, units, ptrs, rows_dev, NT, center, gram_part, aux, only, aux2, ustart);
    SVDQ_STAMP_END(svdq_stamps_gram, uidx);
}

// k_gram with the side sums of the task-Gram by-product (gram_unit, SIDE).  A kernel of its own, so that k_gram's
// instantiations stay what they were; same launch bounds.
template <int NTP, int MODE, bool F64, bool FULL, typename TIN>
__global__ __launch_bounds__(64, (gram_waves<NTP, MODE, F64>())) void k_gram_side(const SvdqParam *__restrict__ params,
                                             const SvdqUnit *__restrict__ units,
                                             const float *const *__restrict__ ptrs,
                                             const int64_t *__restrict__ rows_dev, int NT, int center,
                                             double *__restrict__ gram_part, int unit0,
                                             const void *const *__restrict__ aux2, int order,
                                             double *__restrict__ side_part) {
    __shared__ __attribute__((aligned(16))) float X[gram_lds_floats<NTP, F64>()];
    const int uidx = unit0 + unit_of_block((int)blockIdx.x, (int)gridDim.x, order);
    gram_unit<NTP, MODE, F64, FULL, TIN, true>(X, uidx, params, units, ptrs, rows_dev, NT, center, gram_part, nullptr,
                                                nullptr, aux2, nullptr, side_part);
}

// ------------------------------------------------------------------------------------ launcher
// The by-product launch: plain deltas and minus-base only (MODE 0, 2), never with `only` (the refinement launch of
// N > 16 leaves the side partials of the first launch where they are).
static int launch_gram_side(const svdq_plan *pl, const SvdqInput &in, double *gram_part, int unit0, int nunits,
                            int center, int f64, hipStream_t st, double *side_part) {
    const bool ok = svdq_dispatch_input(pl->in_type, [&](auto tin_c) {
        using TIN = typename decltype(tin_c)::type;
        return svdq_dispatch_int<4, 8, 12, 16, 20, 24, 28, 32>(pl->ntp, [&](auto ntp_c) {
            constexpr int NTP = ntp_c;
            return svdq_dispatch_int<0, 2>(in.mode(), [&](auto mode_c) {
                constexpr int MODE = mode_c;
                return svdq_dispatch_bool(f64 != 0, [&](auto f64_c) {
                    constexpr bool F64 = f64_c;
                    return svdq_dispatch_bool(MODE == 0 && pl->n_tasks == NTP, [&](auto full_c) {
                        constexpr bool FULL = full_c;
                        if constexpr (FULL && MODE != 0) return false;
                        else {
                            hipLaunchKernelGGL((k_gram_side<NTP, MODE, F64, FULL, TIN>), dim3(nunits), dim3(64), 0, st,
                                               pl->d_params, pl->d_units, in.tensors(), in.rows_dev, pl->n_tasks, center,
                                               gram_part, unit0, in.aux2(), pl->cfg.reserved & SVDQ_SW_XCD_CHUNKED,
                                               side_part);
                            return true;
                        }
                    });
                });
            });
        });
    });
    return svdq_launch_status(ok, "k_gram_side");
}

// Variants: the walk (MODE 4, 6) reads fp32 tensors only, and above 16 tasks plain deltas only (MODE 4); the plain and
// the walk mode have a FULL variant for plans with exactly NTP tasks, the walk up to 16 tasks only.
int svdq_launch_gram(const svdq_plan *pl, const SvdqInput &in, double *gram_part, int unit0, int nunits, int center,
                     int f64, const int32_t *only, hipStream_t st, double *side_part) {
    if (side_part) return launch_gram_side(pl, in, gram_part, unit0, nunits, center, f64, st, side_part);
    const bool ok = svdq_dispatch_input(pl->in_type, [&](auto tin_c) {
        using TIN = typename decltype(tin_c)::type;
        return svdq_dispatch_int<4, 8, 12, 16, 20, 24, 28, 32>(pl->ntp, [&](auto ntp_c) {
            constexpr int NTP = ntp_c;
            return svdq_dispatch_int<0, 1, 2, 3, 4, 6>(in.mode(), [&](auto mode_c) {
                constexpr int MODE = mode_c;
                constexpr bool WALK = (MODE & 4) != 0;
                constexpr bool HAS_FULL = MODE == 0 || (MODE == 4 && NTP <= 16);
                if constexpr (WALK && (!std::is_same_v<TIN, float> || (NTP > 16 && MODE != 4))) return false;
                else return svdq_dispatch_bool(f64 != 0, [&](auto f64_c) {
                    constexpr bool F64 = f64_c;
                    return svdq_dispatch_bool(HAS_FULL && pl->n_tasks == NTP, [&](auto full_c) {
                        constexpr bool FULL = full_c;
                        if constexpr (FULL && !HAS_FULL) return false;
                        else {
                            hipLaunchKernelGGL((k_gram<NTP, MODE, F64, FULL, TIN>), dim3(nunits), dim3(64), 0, st,
                                               pl->d_params, pl->d_units, in.tensors(), in.rows_dev, pl->n_tasks, center,
                                               gram_part, unit0, in.aux(), only, in.aux2(),
                                               pl->cfg.reserved & SVDQ_SW_XCD_CHUNKED, in.ustart);
                            return true;
                        }
                    });
                });
            });
        });
    });
    return svdq_launch_status(ok, "k_gram");
}


#ifdef SVDQ_UNIT_STAMPS
extern "C" int svdq_debug_stamps_gram(unsigned long long *buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(svdq_stamps_gram), &buf, sizeof(buf)) == hipSuccess ? 0 : -1;
}
#endif
