// svdq_quant.hip -- the standalone multi-stage quantizer on large tensors (RTVQQuantizer.quantize/dequantize,
// rtvq.py:39-139) and its 16-bit single-stage form.  Compiled with -ffp-contract=off.
//
// Quantizer on n elements, S stages, all on device, no host round trip:
//   k_rtvq_stats   x -> per-block {min, max, has_nan, sum of squares}        (read 4n)
//   per stage s:
//     k_rtvq_params  block partials -> scale_s, zero_point_s, residual_norm_s (fixed order)
//     k_rtvq_apply   residual -> codes_s (1 B/elem), next residual, next stage's partials
//                                                                            (read 4n, write 5n)
// Algorithmic bytes n*(4+S); this schedule moves n*(4 + S*9 - 4) because stage s+1's min/max
// depends on stage s's scale.  A one-launch form for tensors that fit the register file (x read
// once, grid-wide meetings between the stages) was built and measured in round 4: 3-8x SLOWER -- a meeting of 10^3
// workgroups across eight XCDs costs 15-80 us against ~2 us for a kernel boundary (profiles/r04_rtvq_one_launch_experiment.txt).

#include "svdq_common.h"
#include <hip/hip_fp16.h>
#include <stdlib.h>

#define ELT_THREADS 256
#define RTVQ_MAX_BLOCKS 2048

struct RtvqPartial {
    float mn, mx;
    int has_nan, pad;
    double ss;
};

typedef unsigned char u8x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void stat_acc(float x, float &mn, float &mx, int &has_nan, double &ss) {
    if (x != x) has_nan = 1;
    mn = x < mn ? x : mn;
    mx = x > mx ? x : mx;
    ss += (double)x * (double)x;
}

// block-level combine of per-thread stats, result written by thread 0
__device__ void stats_block_reduce(float mn, float mx, int has_nan, double ss, RtvqPartial *dst) {
    __shared__ float s_mn[ELT_THREADS], s_mx[ELT_THREADS];
    __shared__ int s_nan[ELT_THREADS];
    __shared__ double s_ss[ELT_THREADS];
    const int tid = threadIdx.x;
    s_mn[tid] = mn;
    s_mx[tid] = mx;
    s_nan[tid] = has_nan;
    s_ss[tid] = ss;
    __syncthreads();
    for (int off = ELT_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            s_mn[tid] = s_mn[tid + off] < s_mn[tid] ? s_mn[tid + off] : s_mn[tid];
            s_mx[tid] = s_mx[tid + off] > s_mx[tid] ? s_mx[tid + off] : s_mx[tid];
            s_nan[tid] |= s_nan[tid + off];
            s_ss[tid] += s_ss[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        dst->mn = s_mn[0];
        dst->mx = s_mx[0];
        dst->has_nan = s_nan[0];
        dst->pad = 0;
        dst->ss = s_ss[0];
    }
    __syncthreads();
}

__global__ __launch_bounds__(ELT_THREADS) void k_rtvq_stats(const float *__restrict__ x, int64_t n,
                                                            RtvqPartial *__restrict__ part) {
    const int64_t nvec = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * ELT_THREADS;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int has_nan = 0;
    double ss = 0.0;
    int64_t i = (int64_t)blockIdx.x * ELT_THREADS + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {  // four independent 16-byte loads in flight per thread
        f32x4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = reinterpret_cast<const f32x4 *>(x)[i + q * stride];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) stat_acc(v[q][e], mn, mx, has_nan, ss);
    }
    for (; i < nvec; i += stride) {
        const f32x4 v = reinterpret_cast<const f32x4 *>(x)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) stat_acc(v[e], mn, mx, has_nan, ss);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) stat_acc(x[(nvec << 2) + threadIdx.x], mn, mx, has_nan, ss);
    stats_block_reduce(mn, mx, has_nan, ss, part + blockIdx.x);
}

// rtvq.py:10-18 for one stage, from the block partials of the previous pass.  Every block of the apply
// kernel recomputes it (<= 2048 partials, L2-resident; fixed order => the same bits in every block and a
// deterministic norm), which removes a dependent single-block launch per stage.
__device__ void stage_params(const RtvqPartial *__restrict__ part, int nblk, int bits, float &scale, float &zp,
                             float &rnorm) {
    __shared__ RtvqPartial s_tot;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int has_nan = 0;
    double ss = 0.0;
    for (int b = threadIdx.x; b < nblk; b += ELT_THREADS) {
        const RtvqPartial q = part[b];
        mn = q.mn < mn ? q.mn : mn;
        mx = q.mx > mx ? q.mx : mx;
        has_nan |= q.has_nan;
        ss += q.ss;
    }
    stats_block_reduce(mn, mx, has_nan, ss, &s_tot);
    mn = s_tot.mn;
    mx = s_tot.mx;
    if (s_tot.has_nan) {  // torch min/max propagate NaN
        mn = __builtin_nanf("");
        mx = mn;
    }
    const float qmax = (float)((1 << bits) - 1);
    // python-int / Tensor == Tensor.reciprocal() * int: two roundings (tests/golden/rtvq_cases.npz)
    scale = __fmul_rn(__fdiv_rn(1.0f, __fsub_rn(mx, mn)), qmax);
    zp = __fmul_rn(-1.0f, rintf(__fmul_rn(scale, mn)));
    rnorm = (float)sqrt(s_tot.ss);
    __syncthreads();  // s_tot and the reduction scratch are reused by the caller's own reduction
}

__device__ __forceinline__ unsigned char quant_one(float x, float scale, float zp, float qmax, float &res) {
    float vq = rintf(__fadd_rn(__fmul_rn(scale, x), zp));   // rtvq.py:20, two roundings
    unsigned char q;
    if (vq != vq) {
        q = 0;                                               // NaN -> code 0 (reference CPU cast)
    } else {
        vq = vq < 0.f ? 0.f : (vq > qmax ? qmax : vq);
        q = (unsigned char)vq;
    }
    const float deq = __fdiv_rn(__fsub_rn((float)q, zp), scale);   // rtvq.py:35
    res = __fsub_rn(x, deq);                                       // rtvq.py:65
    return q;
}

template <bool LAST>
__global__ __launch_bounds__(ELT_THREADS) void k_rtvq_apply(const float *__restrict__ rin, float *__restrict__ rout,
                                                            int64_t n, const RtvqPartial *__restrict__ part_in,
                                                            int nblk_in, int stage, int bits,
                                                            uint8_t *__restrict__ codes,
                                                            RtvqPartial *__restrict__ part_out,
                                                            float *__restrict__ scale_out, float *__restrict__ zp_out,
                                                            float *__restrict__ rnorm_out) {
    float scale, zp, rnorm;
    stage_params(part_in, nblk_in, bits, scale, zp, rnorm);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        scale_out[stage] = scale;
        zp_out[stage] = zp;
        rnorm_out[stage] = rnorm;
    }
    const float qmax = (float)((1 << bits) - 1);
    const int64_t nvec = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * ELT_THREADS;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int has_nan = 0;
    double ss = 0.0;
    int64_t i = (int64_t)blockIdx.x * ELT_THREADS + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        f32x4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = reinterpret_cast<const f32x4 *>(rin)[i + q * stride];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 r;
            u8x4 c;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float re;
                c[e] = quant_one(v[q][e], scale, zp, qmax, re);
                r[e] = re;
                if (!LAST) stat_acc(re, mn, mx, has_nan, ss);
            }
            reinterpret_cast<u8x4 *>(codes)[i + q * stride] = c;
            if (!LAST) reinterpret_cast<f32x4 *>(rout)[i + q * stride] = r;
        }
    }
    for (; i < nvec; i += stride) {
        const f32x4 v = reinterpret_cast<const f32x4 *>(rin)[i];
        f32x4 r;
        u8x4 q;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float re;
            q[e] = quant_one(v[e], scale, zp, qmax, re);
            r[e] = re;
            if (!LAST) stat_acc(re, mn, mx, has_nan, ss);
        }
        reinterpret_cast<u8x4 *>(codes)[i] = q;
        if (!LAST) reinterpret_cast<f32x4 *>(rout)[i] = r;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t j = (nvec << 2) + threadIdx.x;
        float re;
        codes[j] = quant_one(rin[j], scale, zp, qmax, re);
        if (!LAST) {
            rout[j] = re;
            stat_acc(re, mn, mx, has_nan, ss);
        }
    }
    if (!LAST) stats_block_reduce(mn, mx, has_nan, ss, part_out + blockIdx.x);
}

// rtvq.py:85-103: ((0 + deq_0) + deq_1) + ...
__global__ __launch_bounds__(ELT_THREADS) void k_rtvq_dequant(const uint8_t *__restrict__ codes, int64_t cstride,
                                                              int64_t n, int stages,
                                                              const float *__restrict__ scale,
                                                              const float *__restrict__ zp, float *__restrict__ out) {
    const int64_t nvec = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * ELT_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * ELT_THREADS + threadIdx.x; i < nvec; i += stride) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < stages; ++s) {
            const u8x4 q = reinterpret_cast<const u8x4 *>(codes + (size_t)s * cstride)[i];
            const float sc = scale[s], z = zp[s];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(acc[e], __fdiv_rn(__fsub_rn((float)q[e], z), sc));
        }
        reinterpret_cast<f32x4 *>(out)[i] = acc;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (nvec << 2) + threadIdx.x;
        float acc = 0.f;
        for (int s = 0; s < stages; ++s)
            acc = __fadd_rn(acc, __fdiv_rn(__fsub_rn((float)codes[(size_t)s * cstride + i], zp[s]), scale[s]));
        out[i] = acc;
    }
}

static int rtvq_grid(int64_t n) {
    int64_t b = ((n >> 2) + ELT_THREADS * 4 - 1) / (ELT_THREADS * 4);
    if (b < 1) b = 1;
    if (b > RTVQ_MAX_BLOCKS) b = RTVQ_MAX_BLOCKS;
    return (int)b;
}

extern "C" int64_t svdq_rtvq_work_bytes(int64_t n) {
    return svdq_align_up(n * 4, 256) + 2 * (int64_t)RTVQ_MAX_BLOCKS * sizeof(RtvqPartial) + 256;  // residual + ping-pong partials
}

extern "C" int svdq_rtvq_quantize(const float *x, int64_t n, int32_t bits, int32_t stages, uint8_t *codes,
                                  int64_t code_stride, float *scale, float *zp, float *rnorm, void *work,
                                  void *stream) {
    if (n < 1 || !x || !codes || !scale || !zp || !rnorm || !work) {
        svdq_set_error("svdq_rtvq_quantize: bad argument (n must be >= 1; empty tensors are the caller's job)");
        return SVDQ_EINVAL;
    }
    if (bits < 1 || bits > 8 || stages < 1 || stages > SVDQ_MAX_STAGES) {
        svdq_set_error("svdq_rtvq_quantize: bits in [1,8], stages in [1,%d]", SVDQ_MAX_STAGES);
        return SVDQ_EINVAL;
    }
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(work) & 255) ||
        (reinterpret_cast<uintptr_t>(codes) & 3) || (code_stride & 3) || code_stride < n) {
        svdq_set_error("svdq_rtvq_quantize: x 16-byte, work 256-byte, codes 4-byte aligned; code_stride %% 4 == 0, >= n");
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    uint8_t *wb = reinterpret_cast<uint8_t *>(work);
    float *res = reinterpret_cast<float *>(wb);
    RtvqPartial *part[2];
    part[0] = reinterpret_cast<RtvqPartial *>(wb + svdq_align_up(n * 4, 256));
    part[1] = part[0] + RTVQ_MAX_BLOCKS;
    const int grid = rtvq_grid(n);
    // 1 + S launches: statistics of x, then per stage "parameters (recomputed per block) + codes + residual +
    // statistics of the residual"
    hipLaunchKernelGGL(k_rtvq_stats, dim3(grid), dim3(ELT_THREADS), 0, st, x, n, part[0]);
    for (int s = 0; s < stages; ++s) {
        const float *rin = (s == 0) ? x : res;
        if (s == stages - 1)
            hipLaunchKernelGGL((k_rtvq_apply<true>), dim3(grid), dim3(ELT_THREADS), 0, st, rin, res, n, part[s & 1], grid,
                               s, bits, codes + (size_t)s * code_stride, part[(s + 1) & 1], scale, zp, rnorm);
        else
            hipLaunchKernelGGL((k_rtvq_apply<false>), dim3(grid), dim3(ELT_THREADS), 0, st, rin, res, n, part[s & 1], grid,
                               s, bits, codes + (size_t)s * code_stride, part[(s + 1) & 1], scale, zp, rnorm);
    }
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

extern "C" int svdq_rtvq_dequantize(const uint8_t *codes, int64_t code_stride, int64_t n, int32_t stages,
                                    const float *scale, const float *zp, float *out, void *stream) {
    if (n < 1 || !codes || !scale || !zp || !out || stages < 1) {
        svdq_set_error("svdq_rtvq_dequantize: bad argument");
        return SVDQ_EINVAL;
    }
    if ((reinterpret_cast<uintptr_t>(codes) & 3) || (reinterpret_cast<uintptr_t>(out) & 15) || (code_stride & 3) ||
        code_stride < n) {
        svdq_set_error("svdq_rtvq_dequantize: codes 4-byte / out 16-byte aligned; code_stride %% 4 == 0, >= n");
        return SVDQ_EINVAL;
    }
    hipLaunchKernelGGL(k_rtvq_dequant, dim3(rtvq_grid(n)), dim3(ELT_THREADS), 0, (hipStream_t)stream, codes,
                       code_stride, n, stages, scale, zp, out);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

// ---- qbit = 16 (rtvq.py:22-25): single stage, int16 codes.  The reference casts the clamped fp32 value (0 .. 65535) to
// torch.int16; on the CPU that goes through a 32-bit integer and keeps the low 16 bits, so codes above 32767 come out
// negative -- reproduced as is (tests/golden/rtvq_cases.npz holds the reference's values).
__global__ __launch_bounds__(ELT_THREADS) void k_asym16_apply(const float *__restrict__ x, int64_t n,
                                                              const RtvqPartial *__restrict__ part, int nblk,
                                                              int16_t *__restrict__ codes, float *__restrict__ scale_out,
                                                              float *__restrict__ zp_out) {
    float scale, zp, rnorm;
    stage_params(part, nblk, 16, scale, zp, rnorm);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        scale_out[0] = scale;
        zp_out[0] = zp;
    }
    const int64_t stride = (int64_t)gridDim.x * ELT_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * ELT_THREADS + threadIdx.x; i < n; i += stride) {
        float vq = rintf(__fadd_rn(__fmul_rn(scale, x[i]), zp));
        int32_t q = 0;
        if (vq == vq) {
            vq = vq < 0.f ? 0.f : (vq > 65535.f ? 65535.f : vq);
            q = (int32_t)vq;
        }
        codes[i] = (int16_t)(uint16_t)q;
    }
}

__global__ __launch_bounds__(ELT_THREADS) void k_asym16_dequant(const int16_t *__restrict__ codes, int64_t n,
                                                                const float *__restrict__ scale,
                                                                const float *__restrict__ zp, float *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * ELT_THREADS;
    const float sc = scale[0], z = zp[0];
    for (int64_t i = (int64_t)blockIdx.x * ELT_THREADS + threadIdx.x; i < n; i += stride)
        out[i] = __fdiv_rn(__fsub_rn((float)codes[i], z), sc);   // rtvq.py:35 on the int16 values as they are
}

extern "C" int svdq_asym16_quantize(const float *x, int64_t n, int16_t *codes, float *scale, float *zp, void *work,
                                    void *stream) {
    if (n < 1 || !x || !codes || !scale || !zp || !work || (reinterpret_cast<uintptr_t>(x) & 15) ||
        (reinterpret_cast<uintptr_t>(work) & 255)) {
        svdq_set_error("svdq_asym16_quantize: bad argument (n >= 1, x 16-byte aligned, work 256-byte aligned)");
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    RtvqPartial *part = reinterpret_cast<RtvqPartial *>(reinterpret_cast<uint8_t *>(work) + svdq_align_up(n * 4, 256));
    const int grid = rtvq_grid(n);
    hipLaunchKernelGGL(k_rtvq_stats, dim3(grid), dim3(ELT_THREADS), 0, st, x, n, part);
    hipLaunchKernelGGL(k_asym16_apply, dim3(grid), dim3(ELT_THREADS), 0, st, x, n, part, grid, codes, scale, zp);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

extern "C" int svdq_asym16_dequantize(const int16_t *codes, int64_t n, const float *scale, const float *zp, float *out,
                                      void *stream) {
    if (n < 1 || !codes || !scale || !zp || !out) {
        svdq_set_error("svdq_asym16_dequantize: bad argument");
        return SVDQ_EINVAL;
    }
    hipLaunchKernelGGL(k_asym16_dequant, dim3(rtvq_grid(n)), dim3(ELT_THREADS), 0, (hipStream_t)stream, codes, n, scale,
                       zp, out);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}
