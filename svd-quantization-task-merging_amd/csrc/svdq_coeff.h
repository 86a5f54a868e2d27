// svdq_coeff.h -- the coefficient epilogue as device functions, shared by k_coeff (svdq_small.hip: the fused compress
// route) and k_plan_project_finish (svdq_plan_project.hip: projection onto a plan's stored basis): the fixed-order sum
// of fp64 partial matrices and compress_single_task's tail (compress.py:42-56: c_high -> fp16, c_low ->
// RTVQQuantizer.quantize rtvq.py:39-82), one lane per task.  Both files are compiled with -ffp-contract=off: the
// quantizer must round scale * x and + zero_point separately.
#pragma once

#include "svdq_common.h"
#include "svdq_eig.h"
#include <hip/hip_fp16.h>

#define EIG_THREADS 256

// Sum partial matrices [slot][nn] over slots [s0, s1) into out[nn] (LDS), fixed order:
// wave w takes slots s0+w, s0+w+4, ... ; the four wave sums are then added 0+1+2+3.
static __device__ void reduce_partials(const double *__restrict__ part, int s0, int s1, int nn, double *red /*[4][1024]*/,
                                       double *out /*[nn]*/) {
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    for (int e = l; e < nn; e += 64) {
        double a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = 0.0;
        int s = s0 + w;
        for (; s + 28 < s1; s += 32) {
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] += part[(size_t)(s + 4 * u) * nn + e];
        }
        for (; s < s1; s += 4) a[0] += part[(size_t)s * nn + e];
        red[w * 1024 + e] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    __syncthreads();
    for (int e = tid; e < nn; e += EIG_THREADS)
        out[e] = (red[e] + red[1024 + e]) + (red[2048 + e] + red[3072 + e]);
    __syncthreads();
}

__device__ __forceinline__ float f_min_nan(float a, float b) { return (a != a) ? a : ((b != b) ? b : (b < a ? b : a)); }
__device__ __forceinline__ float f_max_nan(float a, float b) { return (a != a) ? a : ((b != b) ? b : (b > a ? b : a)); }

// From the totals C[t * n + i] (fp64, LDS) of parameter p: coef, c_high and the quantized c_low of every task slot, by
// the EIG_THREADS threads of one workgroup.  c0_in: NULL, or the closed-form part the totals are added to (k_coeff).
// slot_ptrs: NULL (every slot is written), or the [n] pointers of the parameter's task slots -- a slot whose pointer is
// NULL is left exactly as it was.  res: LDS scratch [32 * LDN].
__device__ __forceinline__ void coeff_store_quantize(int p, int n, int k, int r, int bits, int stages,
                                                     const double *C, const double *__restrict__ c0_in,
                                                     const void *const *__restrict__ slot_ptrs, float *res,
                                                     float *__restrict__ coef_out, uint16_t *__restrict__ chigh_out,
                                                     uint8_t *__restrict__ codes_out, float *__restrict__ scale_out,
                                                     float *__restrict__ zp_out, float *__restrict__ rnorm_out) {
    const int tid = threadIdx.x;
    const int nl = r - k;
    // c[t][i] fp32, c_high fp16 (round-to-nearest-even), zero padding past the valid prefix
    for (int e = tid; e < n * n; e += EIG_THREADS) {
        const int t = e / n, i = e % n;
        if (slot_ptrs && !slot_ptrs[t]) continue;
        const float cv = c0_in ? (float)(c0_in[(size_t)p * n * n + e] + C[e]) : (float)C[e];
        coef_out[(size_t)p * n * n + e] = cv;
        chigh_out[(size_t)p * n * n + e] = (i < k) ? __half_as_ushort(__float2half_rn(cv)) : (uint16_t)0;
        if (i >= k && i < r) res[t * LDN + (i - k)] = cv;
    }
    __syncthreads();

    if (tid < n && !(slot_ptrs && !slot_ptrs[tid])) {
        const int t = tid;
        float *x = res + t * LDN;
        const float qmax = (float)((1 << bits) - 1);
        const size_t sbase = ((size_t)p * n + t) * stages;
        for (int s = 0; s < stages; ++s) {
            uint8_t *cdst = codes_out + (sbase + s) * n;
            if (nl <= 0) {
                for (int j = 0; j < n; ++j) cdst[j] = 0;
                scale_out[sbase + s] = 0.f;
                zp_out[sbase + s] = 0.f;
                rnorm_out[sbase + s] = 0.f;
                continue;
            }
            double ss = 0.0;
            float mn = x[0], mx = x[0];
            for (int j = 0; j < nl; ++j) {
                ss += (double)x[j] * (double)x[j];
                mn = f_min_nan(mn, x[j]);
                mx = f_max_nan(mx, x[j]);
            }
            // rtvq.py:17-18: python-int / Tensor == Tensor.reciprocal() * int -> two roundings
            const float range = __fsub_rn(mx, mn);
            const float recip = __fdiv_rn(1.0f, range);
            const float scale = __fmul_rn(recip, qmax);
            const float zp = __fmul_rn(-1.0f, rintf(__fmul_rn(scale, mn)));
            for (int j = 0; j < nl; ++j) {
                float vq = rintf(__fadd_rn(__fmul_rn(scale, x[j]), zp));
                uint8_t q;
                if (vq != vq) {
                    q = 0;
                } else {
                    vq = vq < 0.f ? 0.f : (vq > qmax ? qmax : vq);
                    q = (uint8_t)vq;
                }
                cdst[j] = q;
                const float deq = __fdiv_rn(__fsub_rn((float)q, zp), scale);
                x[j] = __fsub_rn(x[j], deq);
            }
            for (int j = nl; j < n; ++j) cdst[j] = 0;
            scale_out[sbase + s] = scale;
            zp_out[sbase + s] = zp;
            rnorm_out[sbase + s] = (float)sqrt(ss);
        }
    }
}
