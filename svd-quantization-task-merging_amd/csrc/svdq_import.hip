// svdq_import.hip -- svdq_plan_import: adopt stored artifacts into a plan's packed buffers (contract: include/svdq.h).
//
// The reference keeps its artifacts as one file per parameter (storage.py:52-202) and merges them again later
// (reload.py:142-238): U_high / U_low / mean come back as one tensor each.  The batched consumers (svdq_merge.hip) read
// them from the plan's packed basis and mean buffers, so this is a copy -- one streaming launch over the plan's own unit
// table, the shape of k_probe's copy mode (svdq_probe.hip): 16 B per lane, eight loads in flight per lane before the
// first store, sources read once (non-temporal), destinations stored plainly (the merge reads them next).
//
// k, r and rows are read from the small buffer ON THE DEVICE: the host never needs them, nothing is synchronised.

#include "svdq_common.h"

typedef const __attribute__((address_space(1))) f32x4 ig_f32x4;
typedef __attribute__((address_space(1))) f32x4 ig_f32x4_w;
typedef const __attribute__((address_space(1))) uint8_t ig_byte;
typedef __attribute__((address_space(1))) uint8_t ig_byte_w;

// bytes [b0, b1) of src -> the same bytes of dst, by one wavefront.  b0 is a multiple of 16 and src / dst are 16-byte
// aligned (row0 is a multiple of 256 rows); only a parameter's last unit has an end that is not.
__device__ __forceinline__ void import_range(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int64_t b0,
                                             int64_t b1, int lane) {
    constexpr int INFL = 8;
    if (b1 <= b0) return;
    ig_f32x4 *s = (ig_f32x4 *)(src + b0);
    ig_f32x4_w *d = (ig_f32x4_w *)(dst + b0);
    const int64_t nvec = (b1 - b0) >> 4;
    int64_t i = 0;
    for (; i + INFL * 64 <= nvec; i += INFL * 64) {
        f32x4 v[INFL];
#pragma unroll
        for (int u = 0; u < INFL; ++u) v[u] = __builtin_nontemporal_load(s + i + u * 64 + lane);
#pragma unroll
        for (int u = 0; u < INFL; ++u) d[i + u * 64 + lane] = v[u];
    }
    for (i += lane; i < nvec; i += 64) d[i] = __builtin_nontemporal_load(s + i);
    // the last < 16 bytes of a parameter, byte by byte: nothing past the range is written
    const int tail = (int)((b1 - b0) & 15);
    if (lane < tail) {
        const int64_t o = b0 + (nvec << 4) + lane;
        ((ig_byte_w *)dst)[o] = ((ig_byte *)src)[o];
    }
}

// One wavefront per work unit: rows [row0, row0 + nrows) of the unit's parameter, clipped to the rows the small buffer
// names.  ES: bytes per basis element.
template <int ES>
__global__ __launch_bounds__(64) void k_import(const SvdqParam *__restrict__ params, const SvdqUnit *__restrict__ units,
                                               int NT, const int32_t *__restrict__ k_in, const int32_t *__restrict__ r_in,
                                               const int64_t *__restrict__ rows_in,
                                               const uint8_t *const *__restrict__ uh_ptrs,
                                               const uint8_t *const *__restrict__ ul_ptrs,
                                               const uint8_t *const *__restrict__ mean_ptrs, uint8_t *__restrict__ basis,
                                               float *__restrict__ mean) {
    const int lane = threadIdx.x;
    const SvdqUnit un = units[blockIdx.x];
    const int p = un.param;
    const SvdqParam pd = params[p];
    int64_t rows = rows_in[p];
    if (rows > pd.rows) rows = pd.rows;      // the slab was sized for pd.rows: never past it, whatever the buffer says
    if (rows <= 0 || un.row0 >= rows) return;
    int64_t r1 = un.row0 + un.nrows;
    if (r1 > rows) r1 = rows;
    // the ranks as every consumer reads them, held to what the slab has room for: r <= min(rows, N), k <= r
    int64_t r = r_in[p], k = k_in[p];
    const int64_t rmax = rows < NT ? rows : NT;
    r = r < 0 ? 0 : (r > rmax ? rmax : r);
    k = k < 0 ? 0 : (k > r ? r : k);
    const int64_t nl = r - k;
    uint8_t *slab = basis + pd.slab_off;
    if (k > 0) import_range(uh_ptrs[p], slab, un.row0 * k * ES, r1 * k * ES, lane);
    if (nl > 0) import_range(ul_ptrs[p], slab + svdq_align_up(rows * k * ES, 256), un.row0 * nl * ES, r1 * nl * ES, lane);
    if (mean_ptrs) import_range(mean_ptrs[p], reinterpret_cast<uint8_t *>(mean + pd.mean_off), un.row0 * 4, r1 * 4, lane);
}

extern "C" int svdq_plan_import(const svdq_plan *pl, const void *u_high_ptrs, const void *u_low_ptrs,
                                const void *mean_ptrs, const void *small, void *basis, float *mean, void *stream) {
    if (!pl || !u_high_ptrs || !u_low_ptrs || !small || !basis) {
        svdq_set_error("svdq_plan_import: the plan, u_high_ptrs, u_low_ptrs, small and basis are required");
        return SVDQ_EINVAL;
    }
    if (pl->cfg.center ? (!mean_ptrs || !mean) : (mean_ptrs != nullptr)) {
        svdq_set_error("svdq_plan_import: mean_ptrs and mean are required on a centred plan (center = %d), and mean_ptrs "
                       "must be NULL on an uncentred one", pl->cfg.center);
        return SVDQ_EINVAL;
    }
    if (((uintptr_t)u_high_ptrs | (uintptr_t)u_low_ptrs | (uintptr_t)mean_ptrs) & 7) {
        svdq_set_error("svdq_plan_import: pointer tables must be 8-byte aligned");
        return SVDQ_EINVAL;
    }
    if (((uintptr_t)small | (uintptr_t)basis | (uintptr_t)mean) & 15) {
        svdq_set_error("svdq_plan_import: small, basis and mean must be 16-byte aligned");
        return SVDQ_EINVAL;
    }
    const svdq_small_layout &L = pl->small;
    const uint8_t *sm = reinterpret_cast<const uint8_t *>(small);
    auto kk = reinterpret_cast<const int32_t *>(sm + L.k_off), rr = reinterpret_cast<const int32_t *>(sm + L.r_off);
    auto rows = reinterpret_cast<const int64_t *>(sm + L.rows_off);
    auto uh = reinterpret_cast<const uint8_t *const *>(u_high_ptrs), ul = reinterpret_cast<const uint8_t *const *>(u_low_ptrs);
    auto mp = reinterpret_cast<const uint8_t *const *>(mean_ptrs);
    uint8_t *bs = reinterpret_cast<uint8_t *>(basis);
    hipStream_t st = (hipStream_t)stream;
    if (pl->cfg.fp16)
        hipLaunchKernelGGL(k_import<2>, dim3(pl->n_units), dim3(64), 0, st, pl->d_params, pl->d_units, pl->n_tasks, kk, rr,
                           rows, uh, ul, mp, bs, mean);
    else
        hipLaunchKernelGGL(k_import<4>, dim3(pl->n_units), dim3(64), 0, st, pl->d_params, pl->d_units, pl->n_tasks, kk, rr,
                           rows, uh, ul, mp, bs, mean);
    return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP;
}
