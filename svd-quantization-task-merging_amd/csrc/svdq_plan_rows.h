// svdq_plan_rows.h -- the row loads of one block of a plan's work unit, shared by the kernels that form xc from new
// task tensors against a stored basis: k_plan_project (svdq_plan_project.hip) and the two streaming passes of
// svdq_plan_extend.hip.  "xc formed exactly as svdq_plan_project forms it" is part of the extension's contract
// (include/svdq.h), so both read their rows through plan_rows_fetch (the same loads, the same zeros past the block) and
// form xc and write its strips through plan_rows_commit (the same two subtractions in the same order).
#pragma once

#include "svdq_input.h"
#include "svdq_merge_stream.h"

typedef const __attribute__((address_space(1))) int32_t plan_gint;

// Lane l owns rows c0 + RPL l .. + RPL - 1 of the block that starts at c0 (RB = 64 RPL rows, the unit ends at cend).
// xpf[t][e]: the row of task slot t (absent slots, dp[t] == NULL, keep what they hold: zeros); bpf: the base tensor's row
// (FB: the task tensors are fine-tuned weights); mpf: the stored mean's (gmean != NULL).  Rows at or past cend read
// nothing and leave 0.  GATHER: rows through the int32 index list gidx; otherwise a full block takes one vector load per
// slot and a partial block element loads.
template <typename TIN, int NS, int RPL, bool GATHER, bool FB>
__device__ __forceinline__ void plan_rows_fetch(float (&xpf)[NS][RPL], float (&mpf)[RPL], float (&bpf)[RPL],
                                                gin<TIN> *const (&dp)[NS], gin<TIN> *bp, plan_gint *gidx,
                                                mg_gfloat *gmean, int64_t c0, int64_t cend, int lane) {
    constexpr int RB = 64 * RPL;
    const int64_t r0 = c0 + RPL * lane;
    const int nr = block_rows<RB>(c0, cend);
    if constexpr (GATHER) {
        int64_t src[RPL];
        bool in[RPL];
#pragma unroll
        for (int e = 0; e < RPL; ++e) {
            in[e] = r0 + e < cend;
            src[e] = in[e] ? (int64_t)gidx[r0 + e] : 0;
        }
        if constexpr (FB) {
#pragma unroll
            for (int e = 0; e < RPL; ++e) bpf[e] = in[e] ? in_load1<TIN>(bp + src[e]) : 0.f;
        }
#pragma unroll
        for (int t = 0; t < NS; ++t)
            if (dp[t]) {      // wave-uniform
#pragma unroll
                for (int e = 0; e < RPL; ++e) xpf[t][e] = in[e] ? in_load1<TIN>(dp[t] + src[e]) : 0.f;
            }
    } else if (nr == RB) {
        if constexpr (FB) {
            if constexpr (RPL == 4) {
                const f32x4 v = in_load4<TIN>(bp + r0);
                bpf[0] = v.x, bpf[1] = v.y, bpf[2] = v.z, bpf[3] = v.w;
            } else {
                const svdq_f32x2 v = in_load2<TIN>(bp + r0);
                bpf[0] = v.x, bpf[1] = v.y;
            }
        }
#pragma unroll
        for (int t = 0; t < NS; ++t)
            if (dp[t]) {
                if constexpr (RPL == 4) {
                    const f32x4 v = in_load4<TIN>(dp[t] + r0);
                    xpf[t][0] = v.x, xpf[t][1] = v.y, xpf[t][2] = v.z, xpf[t][3] = v.w;
                } else {
                    const svdq_f32x2 v = in_load2<TIN>(dp[t] + r0);
                    xpf[t][0] = v.x, xpf[t][1] = v.y;
                }
            }
    } else {
        if constexpr (FB) {
#pragma unroll
            for (int e = 0; e < RPL; ++e) bpf[e] = (r0 + e < cend) ? in_load1<TIN>(bp + (r0 + e)) : 0.f;
        }
#pragma unroll
        for (int t = 0; t < NS; ++t)
            if (dp[t]) {
#pragma unroll
                for (int e = 0; e < RPL; ++e) xpf[t][e] = (r0 + e < cend) ? in_load1<TIN>(dp[t] + (r0 + e)) : 0.f;
            }
    }
    if (gmean) {
#pragma unroll
        for (int e = 0; e < RPL; ++e) mpf[e] = (r0 + e < cend) ? gmean[r0 + e] : 0.f;
    }
}

// stride (floats) of one task slot's strip of a block of rb rows: rb + pad, a multiple of 4 (16-byte alignment)
__host__ __device__ constexpr int plan_strip_stride(int rb) { return rb + 4; }

// xc = (finetuned - base) - mean of what plan_rows_fetch left, each a single fp32 subtraction (rows past the block's end
// are 0 - 0 - 0), written to the strips X[t][RPL lane ..] of the present slots.  SQ: the lane's sum of xc^2 per slot, an
// fp32 fma chain over its rows, goes to sq[t * sq_stride + lane] (the extension's |xc|^2).
template <int NS, int RPL, bool FB, bool SQ, typename DP>
__device__ __forceinline__ void plan_rows_commit(float *X, const float (&xpf)[NS][RPL], const float (&mpf)[RPL],
                                                 const float (&bpf)[RPL], const DP (&dp)[NS], bool has_mean, int lane,
                                                 float *sq = nullptr, int sq_stride = 0) {
    constexpr int XS = plan_strip_stride(64 * RPL);
#pragma unroll
    for (int t = 0; t < NS; ++t)
        if (dp[t]) {
            float xc[RPL];
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < RPL; ++e) {
                float x = xpf[t][e];
                if constexpr (FB) x = __fsub_rn(x, bpf[e]);
                if (has_mean) x = __fsub_rn(x, mpf[e]);
                xc[e] = x;
                if constexpr (SQ) s = fmaf(x, x, s);
            }
            if constexpr (RPL == 4) {
                *reinterpret_cast<f32x4 *>(X + t * XS + 4 * lane) = f32x4{xc[0], xc[1], xc[2], xc[3]};
            } else {
                *reinterpret_cast<svdq_f32x2 *>(X + t * XS + 2 * lane) = svdq_f32x2{xc[0], xc[1]};
            }
            if constexpr (SQ) sq[t * sq_stride + lane] = s;
        }
}
