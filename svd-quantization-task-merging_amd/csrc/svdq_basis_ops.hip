// svdq_basis_ops.hip -- the operators on one parameter's basis for callers that bring their own: projection
// (svdq_project), reconstruction (svdq_reconstruct) and the fused reconstruction error (svdq_recon_error).
// Thread per row, 256 threads per block, at most PROJ_BLOCKS blocks.  Compiled with -ffp-contract=off.

#include "svdq_common.h"
#include "svdq_dispatch.h"
#include <hip/hip_fp16.h>

#define ELT_THREADS 256

// the element type of a call's basis arrays, from svdq_dispatch_bool(u_fp16 != 0, ...)'s tag
template <bool F16> using BasisT = std::conditional_t<F16, __half, float>;

// ------------------------------------------------------------------------------------ projection
// project_to_basis (compress.py:6-21) with the mean subtraction of compress.py:35-37 folded in,
// for callers that bring their own basis: c[i] = sum_d float(U[d][i]) * (delta[d] - mean[d]).
// Thread per row (adjacent threads read adjacent rows of the row-major [D,k] / [D,nl] arrays),
// fp32 per thread, fp64 across threads and blocks, fixed-order final sum => deterministic.
#define PROJ_BLOCKS 1024

__device__ __forceinline__ float u_load(const __half *u, int64_t i) { return __half2float(u[i]); }
__device__ __forceinline__ float u_load(const float *u, int64_t i) { return u[i]; }

template <typename T>
__global__ __launch_bounds__(ELT_THREADS) void k_project(const T *__restrict__ uh, const T *__restrict__ ul,
                                                         int64_t rows, int k, int nl,
                                                         const float *__restrict__ delta,
                                                         const float *__restrict__ mean,
                                                         double *__restrict__ part /*[grid][32]*/) {
    float acc[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) acc[i] = 0.f;
    const int64_t stride = (int64_t)gridDim.x * ELT_THREADS;
    for (int64_t d = (int64_t)blockIdx.x * ELT_THREADS + threadIdx.x; d < rows; d += stride) {
        float x = delta[d];
        if (mean) x = __fsub_rn(x, mean[d]);
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            if (i < k)
                acc[i] = fmaf(u_load(uh, d * k + i), x, acc[i]);
            else if (i < k + nl)
                acc[i] = fmaf(u_load(ul, d * nl + (i - k)), x, acc[i]);
        }
    }
    __shared__ double red[ELT_THREADS];
    for (int i = 0; i < k + nl; ++i) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if (j == i) v = (double)acc[j];
        red[threadIdx.x] = v;
        __syncthreads();
        for (int off = ELT_THREADS / 2; off > 0; off >>= 1) {
            if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * 32 + i] = red[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_project_finish(const double *__restrict__ part, int nblk, int ncols,
                                                       float *__restrict__ c_out) {
    const int i = threadIdx.x;
    if (i >= ncols) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * 32 + i];
    c_out[i] = (float)s;
}

static int project_grid(int64_t rows) {
    int64_t b = (rows + ELT_THREADS * 8 - 1) / (ELT_THREADS * 8);
    if (b < 1) b = 1;
    if (b > PROJ_BLOCKS) b = PROJ_BLOCKS;
    return (int)b;
}

extern "C" int64_t svdq_project_work_bytes(int64_t rows, int32_t ncols) {
    (void)ncols;
    return (int64_t)project_grid(rows) * 32 * 8 + 256;
}

extern "C" int svdq_project(const void *u_high, const void *u_low, int32_t u_fp16, int64_t rows, int32_t k, int32_t nl,
                            const float *delta, const float *mean, float *c_out, void *work, void *stream) {
    if (rows < 1 || k < 0 || nl < 0 || k + nl < 1 || k + nl > 32 || !delta || !c_out || !work ||
        (k > 0 && !u_high) || (nl > 0 && !u_low)) {
        svdq_set_error("svdq_project: bad argument (1 <= k + nl <= 32)");
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const int grid = project_grid(rows);
    double *part = reinterpret_cast<double *>(work);
    svdq_dispatch_bool(u_fp16 != 0, [&](auto f16_c) {
        using T = BasisT<decltype(f16_c)::value>;
        hipLaunchKernelGGL((k_project<T>), dim3(grid), dim3(ELT_THREADS), 0, st, reinterpret_cast<const T *>(u_high),
                           reinterpret_cast<const T *>(u_low), rows, k, nl, delta, mean, part);
        return true;
    });
    hipLaunchKernelGGL(k_project_finish, dim3(1), dim3(64), 0, st, part, grid, k + nl, c_out);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

// ------------------------------------------------------------------------------------ merge consumers
// reconstruct_from_coefficients (merge.py:144-194): out = ((U_high c_high + U_low c_low) + mean) * scale.
// HBM-bound: reads the fp16 (or fp32) basis once (e*(k+nl) B/row) + mean, writes 4 B/row.
// Thread per row; adjacent threads read adjacent rows of the row-major [D,k] / [D,nl] arrays.
template <typename T>
__global__ __launch_bounds__(ELT_THREADS) void k_reconstruct(const T *__restrict__ uh, const T *__restrict__ ul,
                                                             int64_t rows, int k, int nl,
                                                             const float *__restrict__ coef,
                                                             const float *__restrict__ mean, float scale,
                                                             float *__restrict__ out) {
    __shared__ float c[32];
    if (threadIdx.x < k + nl) c[threadIdx.x] = coef[threadIdx.x];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * ELT_THREADS;
    for (int64_t d = (int64_t)blockIdx.x * ELT_THREADS + threadIdx.x; d < rows; d += stride) {
        float hi = 0.f, lo = 0.f;
        for (int i = 0; i < k; ++i) hi = fmaf(u_load(uh, d * k + i), c[i], hi);
        for (int j = 0; j < nl; ++j) lo = fmaf(u_load(ul, d * nl + j), c[k + j], lo);
        float v = __fadd_rn(hi, lo);
        if (mean) v = __fadd_rn(v, mean[d]);
        out[d] = __fmul_rn(v, scale);
    }
}

extern "C" int svdq_reconstruct(const void *u_high, const void *u_low, int32_t u_fp16, int64_t rows, int32_t k,
                                int32_t nl, const float *coef, const float *mean, float scale, float *out,
                                void *stream) {
    if (rows < 1 || k < 0 || nl < 0 || k + nl > 32 || !out || (k + nl > 0 && !coef) || (k > 0 && !u_high) ||
        (nl > 0 && !u_low)) {
        svdq_set_error("svdq_reconstruct: bad argument (k + nl <= 32)");
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const int grid = project_grid(rows);
    svdq_dispatch_bool(u_fp16 != 0, [&](auto f16_c) {
        using T = BasisT<decltype(f16_c)::value>;
        hipLaunchKernelGGL((k_reconstruct<T>), dim3(grid), dim3(ELT_THREADS), 0, st, reinterpret_cast<const T *>(u_high),
                           reinterpret_cast<const T *>(u_low), rows, k, nl, coef, mean, scale, out);
        return true;
    });
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}

// ------------------------------------------------------------------------------------ diagnostics
// compute_reconstruction_error (diagnostics.py:72-117) fused with the reconstruction it is applied to in
// compute_parameter_diagnostics (diagnostics.py:205-215): rec = U_high c_high + U_low c_low (+ mean when
// given -- the reference's diagnostics do NOT add it back) is never materialised.
// out[6] = {||x-rec||, ||x-rec||/||x|| (0 when ||x|| <= 1e-10), max|x-rec|, mean|x-rec|, ||x||, ||rec||}
struct ErrPart {
    double se, sx, sr, sa, mx;
};

template <typename T>
__global__ __launch_bounds__(ELT_THREADS) void k_recon_error(const T *__restrict__ uh, const T *__restrict__ ul,
                                                             int64_t rows, int k, int nl,
                                                             const float *__restrict__ coef,
                                                             const float *__restrict__ mean,
                                                             const float *__restrict__ recon_in,
                                                             const float *__restrict__ orig,
                                                             ErrPart *__restrict__ part) {
    __shared__ float c[32];
    if (threadIdx.x < k + nl) c[threadIdx.x] = coef[threadIdx.x];
    __syncthreads();
    double se = 0.0, sx = 0.0, sr = 0.0, sa = 0.0;
    float mx = 0.f;
    const int64_t stride = (int64_t)gridDim.x * ELT_THREADS;
    for (int64_t d = (int64_t)blockIdx.x * ELT_THREADS + threadIdx.x; d < rows; d += stride) {
        float rec;
        if (recon_in) {
            rec = recon_in[d];
        } else {
            float hi = 0.f, lo = 0.f;
            for (int i = 0; i < k; ++i) hi = fmaf(u_load(uh, d * k + i), c[i], hi);
            for (int j = 0; j < nl; ++j) lo = fmaf(u_load(ul, d * nl + j), c[k + j], lo);
            rec = __fadd_rn(hi, lo);
            if (mean) rec = __fadd_rn(rec, mean[d]);
        }
        const float x = orig[d];
        const float e = __fsub_rn(x, rec);
        se += (double)e * e;
        sx += (double)x * x;
        sr += (double)rec * rec;
        sa += fabs((double)e);
        mx = fmaxf(mx, fabsf(e));      // skips a NaN: the finish kernel puts it back from the sum of squares
    }
    __shared__ double r0[ELT_THREADS], r1[ELT_THREADS], r2[ELT_THREADS], r3[ELT_THREADS], r4[ELT_THREADS];
    const int tid = threadIdx.x;
    r0[tid] = se; r1[tid] = sx; r2[tid] = sr; r3[tid] = sa; r4[tid] = (double)mx;
    __syncthreads();
    for (int off = ELT_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            r0[tid] += r0[tid + off]; r1[tid] += r1[tid + off]; r2[tid] += r2[tid + off]; r3[tid] += r3[tid + off];
            const double a = r4[tid], b = r4[tid + off];
            r4[tid] = b > a ? b : a;
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[blockIdx.x].se = r0[0]; part[blockIdx.x].sx = r1[0]; part[blockIdx.x].sr = r2[0];
        part[blockIdx.x].sa = r3[0]; part[blockIdx.x].mx = r4[0];
    }
}

__global__ __launch_bounds__(64) void k_recon_error_finish(const ErrPart *__restrict__ part, int nblk, int64_t rows,
                                                           double *__restrict__ out) {
    if (threadIdx.x != 0) return;
    double se = 0.0, sx = 0.0, sr = 0.0, sa = 0.0, mx = 0.0;
    for (int b = 0; b < nblk; ++b) {
        se += part[b].se; sx += part[b].sx; sr += part[b].sr; sa += part[b].sa;
        const double v = part[b].mx;
        mx = v > mx ? v : mx;
    }
    // NaN propagates like torch.max: an error element is NaN exactly when the sum of the squares is (a square is
    // >= 0 or NaN, so the sum cannot cancel to one), whichever row, thread or block it sat in
    if (se != se) mx = se;
    // the reference works on fp32 tensors: norms are fp32 values
    const float en = (float)sqrt(se), on = (float)sqrt(sx);
    out[0] = (double)en;
    out[1] = on > 1e-10f ? (double)en / (double)on : 0.0;
    out[2] = mx;
    out[3] = (double)(float)(sa / (double)rows);
    out[4] = (double)on;
    out[5] = (double)(float)sqrt(sr);
}

extern "C" int64_t svdq_recon_error_work_bytes(int64_t rows) { return (int64_t)project_grid(rows) * sizeof(ErrPart) + 256; }

extern "C" int svdq_recon_error(const void *u_high, const void *u_low, int32_t u_fp16, int64_t rows, int32_t k,
                                int32_t nl, const float *coef, const float *mean, const float *recon,
                                const float *orig, double *out6, void *work, void *stream) {
    const bool fused = recon == nullptr;
    if (rows < 1 || !orig || !out6 || !work || (fused && (k < 0 || nl < 0 || k + nl > 32 || (k + nl > 0 && !coef) ||
                                                          (k > 0 && !u_high) || (nl > 0 && !u_low)))) {
        svdq_set_error("svdq_recon_error: bad argument");
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const int grid = project_grid(rows);
    ErrPart *part = reinterpret_cast<ErrPart *>(work);
    if (!fused) {
        k = 0;
        nl = 0;
    }
    svdq_dispatch_bool(u_fp16 && fused, [&](auto f16_c) {   // a given reconstruction: the basis is not read
        using T = BasisT<decltype(f16_c)::value>;
        hipLaunchKernelGGL((k_recon_error<T>), dim3(grid), dim3(ELT_THREADS), 0, st, reinterpret_cast<const T *>(u_high),
                           reinterpret_cast<const T *>(u_low), rows, k, nl, coef, mean, recon, orig, part);
        return true;
    });
    hipLaunchKernelGGL(k_recon_error_finish, dim3(1), dim3(64), 0, st, part, grid, rows, out6);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}
