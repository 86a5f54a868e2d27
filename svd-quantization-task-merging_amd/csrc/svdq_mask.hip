// svdq_mask.hip -- the mask operators (mask_loader.py:412-485, 651-763): combine, count, compact, expand, index
// lists and unit starts, for one parameter and for a ragged set of parameters.  Compiled with -ffp-contract=off.
//
// A mask is processed in tiles of 2048 elements, one block of 256 threads per tile, 8 elements per thread.  Every
// step of a tile has ONE __device__ body; the __global__ kernels only resolve (parameter, tile, numel, mask) -- from
// their arguments in the single-parameter form, from the tile table of a svdq_maskset in the set form:
//   tile_select      8 mask bytes of a thread -> selected-bit field, count, valid elements
//   block_sum_u32 / block_scan_u32   sum / inclusive prefix sum over the block
//   combine_tile     vote of n bool masks; maskset_combine_packed_tile: the same from bit-packed streams
//   scan_tiles       exclusive scan of a parameter's tile counts
//   scatter_tile     order-preserving compaction;  maskset_index_tile: the index lists of the same partition
// The host side mirrors it: a source (masks as given: launch_count; a combine: launch_combine /
// launch_combine_packed) fills the tile counts, launch_scan turns them into offsets and totals, a back
// (scatter, launch_index, launch_unit_starts) consumes the offsets.

#include "svdq_common.h"
#include <stdlib.h>

#define ELT_THREADS 256
#define MASK_TILE 2048  // elements per block: 256 threads x 8
#define SCAN_THREADS 1024
// MASK_TPB consecutive tiles per block for the index and the packed-combine kernels: they do a few hundred bytes of
// work per thread and tile, so the block start-up dominates when every tile is its own block
#define MASK_TPB 4

// ------------------------------------------------------------------------------------ steps of a tile
// torch.bool storage is one byte per element holding 0 or 1, so 8 mask bytes can be voted on at once:
// byte lanes of a 64-bit word accumulate the per-element counts (n_masks <= SVDQ_MAX_BOOL_MASKS = 255: a lane holds
// every count, nothing carries into its neighbour; the host entry points refuse more, bool_mask_count_ok).
__device__ __forceinline__ unsigned long long load_mask8(const uint8_t *p, int lim) {
    unsigned long long w = 0;
    if (lim == 8 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) return *reinterpret_cast<const unsigned long long *>(p);
    for (int e = 0; e < lim; ++e) w |= (unsigned long long)(p[e] != 0) << (8 * e);
    return w;
}

// A thread's slice of a tile: elements base .. base + lim of `mask` (lim = 0 past the end), bit e of sel = element
// base + e is selected -- set, or with `invert` cleared -- and cnt = popcount(sel).  Any non-zero byte counts as set,
// in every kernel alike: a count and the scatter that trusts it cannot disagree.
struct TileSel {
    unsigned sel, cnt;
    int lim;
};

__device__ __forceinline__ TileSel tile_select(const uint8_t *mask, int64_t base, int64_t numel, int invert) {
    TileSel s = {0u, 0u, 0};
    if (base < numel) {
        s.lim = (int)((numel - base) < 8 ? (numel - base) : 8);
        const unsigned long long m7 = 0x7f7f7f7f7f7f7f7full;
        unsigned long long w = load_mask8(mask + base, s.lim);      // one 8-byte load; zero past lim
        w = (((w & m7) + m7) | w) & ~m7;                            // bit 7 of a byte: the byte is not zero
        s.cnt = (unsigned)__popcll(w);
        // bit 8e + 7 -> bit e: the partial products fall on distinct bits, so nothing carries into bits 56..63
        s.sel = (unsigned)(((w >> 7) * 0x0102040810204080ull) >> 56);
        if (invert) {
            s.cnt = (unsigned)s.lim - s.cnt;
            s.sel = ~s.sel & ((1u << s.lim) - 1u);
        }
    }
    return s;
}

// strategy: low byte = SVDQ_MASK_*; for the majority vote bits 8.. hold (votes needed + 1), 0 = the default threshold 0.5
__device__ __forceinline__ unsigned long long vote8(unsigned long long acc, int n_masks, int strategy) {
    unsigned long long out = 0;
    const int kind = strategy & 0xff, need1 = strategy >> 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int v = (int)((acc >> (8 * e)) & 0xff);
        int bit;
        if (kind == SVDQ_MASK_UNION)
            bit = v > 0;
        else if (kind == SVDQ_MASK_INTERSECTION)
            bit = v == n_masks;
        else
            bit = need1 ? (v >= need1 - 1) : (2 * v >= n_masks);  // vote_sum >= threshold * len(masks), mask_loader.py:483
        out |= (unsigned long long)bit << (8 * e);
    }
    return out;
}

// sum over the 256 threads of a block, valid in thread 0: wave shuffles, then one LDS hop for the 4 wave sums
__device__ __forceinline__ unsigned block_sum_u32(unsigned v) {
    __shared__ unsigned s_w[ELT_THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned tot = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < ELT_THREADS / 64; ++w) tot += s_w[w];
    }
    __syncthreads();
    return tot;
}

// inclusive prefix sum over the 256 threads of a block (wave shuffles + one LDS hop); *total = block sum.
// Two barriers, reached by every thread: the only in-block scan of this file.
__device__ __forceinline__ unsigned block_scan_u32(unsigned v, unsigned *total) {
    __shared__ unsigned s_w[ELT_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    unsigned add = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < ELT_THREADS / 64; ++i) {
        if (i < w) add += s_w[i];
        tot += s_w[i];
    }
    __syncthreads();
    *total = tot;
    return v + add;
}

// one 2048-element tile: combined mask out, number of selected elements returned by thread 0 via *cnt_out
__device__ void combine_tile(const uint8_t *const *masks, int n_masks, int strategy, int64_t tile, int64_t numel,
                             uint8_t *out, unsigned *cnt_out) {
    const int64_t base = tile * MASK_TILE + (int64_t)threadIdx.x * 8;
    unsigned cnt = 0;
    if (base < numel) {
        const int lim = (int)((numel - base) < 8 ? (numel - base) : 8);
        unsigned long long acc = 0;
        for (int m0 = 0; m0 < n_masks; m0 += 8) {   // 8 independent loads in flight per thread
            unsigned long long w[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = (m0 + j < n_masks) ? load_mask8(masks[m0 + j] + base, lim) : 0ull;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += w[j];
        }
        const unsigned long long res = vote8(acc, n_masks, strategy);
        if (lim == 8 && (reinterpret_cast<uintptr_t>(out + base) & 7) == 0) {
            *reinterpret_cast<unsigned long long *>(out + base) = res;
        } else {
            for (int e = 0; e < lim; ++e) out[base + e] = (uint8_t)((res >> (8 * e)) & 1);
        }
        cnt = (unsigned)__popcll(lim == 8 ? res : (res & ((1ull << (8 * lim)) - 1)));
    }
    const unsigned tot = block_sum_u32(cnt);
    if (threadIdx.x == 0) *cnt_out = tot;
}

// exclusive scan of the nt tile counts of one parameter (one block of 1024 threads, 1024 tiles per trip with a
// carry between the trips); returns the total to every thread
__device__ unsigned long long scan_tiles(const unsigned *__restrict__ tile_counts, int nt,
                                         unsigned long long *__restrict__ tile_offsets) {
    __shared__ unsigned long long s[SCAN_THREADS];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nt; base += SCAN_THREADS) {
        const int i = base + threadIdx.x;
        const unsigned long long v = i < nt ? tile_counts[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < SCAN_THREADS; off <<= 1) {
            unsigned long long add = threadIdx.x >= off ? s[threadIdx.x - off] : 0;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < nt) tile_offsets[i] = carry + s[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == SCAN_THREADS - 1) carry += s[SCAN_THREADS - 1];
        __syncthreads();
    }
    return carry;
}

// one tile of an order-preserving compaction for n_src buffers: every source tile is loaded with
// 16-B loads, compacted through LDS (selected -> one image, unselected -> a second one when asked)
// and written out as ONE contiguous, coalesced run per region.
__device__ void scatter_tile(const uint8_t *mask, int64_t tile, int64_t numel, const float *const *src,
                             float *const *dst_true, float *const *dst_false, int n_src,
                             unsigned long long tile_off) {
    __shared__ float lt[MASK_TILE], lf[MASK_TILE];
    const int tid = threadIdx.x;
    const int64_t tbase = tile * MASK_TILE;
    const int64_t base = tbase + (int64_t)tid * 8;
    const TileSel ts = tile_select(mask, base, numel, 0);
    const int lim = ts.lim;
    unsigned tot_true;
    const unsigned incl = block_scan_u32(ts.cnt, &tot_true);
    const int tile_n = (int)((numel - tbase) < MASK_TILE ? (numel - tbase) : MASK_TILE);
    const unsigned tot_false = (unsigned)tile_n - tot_true;
    const unsigned pt = incl - ts.cnt;                // rank of this thread's first selected element
    const unsigned pf = (unsigned)(tid * 8) - pt;     // ... and of its first unselected one
    const unsigned long long f_off = (unsigned long long)tbase - tile_off;
    for (int m = 0; m < n_src; ++m) {
        const float *sp = src[m] + base;
        float v[8];
        if (lim == 8 && (reinterpret_cast<uintptr_t>(sp) & 15) == 0) {
            const f32x4 a = reinterpret_cast<const f32x4 *>(sp)[0], b = reinterpret_cast<const f32x4 *>(sp)[1];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = e < lim ? sp[e] : 0.f;
        }
        unsigned jt = pt, jf = pf;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (e < lim) {
                if (ts.sel & (1u << e))
                    lt[jt++] = v[e];
                else
                    lf[jf++] = v[e];
            }
        }
        __syncthreads();
        if (dst_true) {
            float *dt = dst_true[m] + tile_off;
            for (unsigned i = tid; i < tot_true; i += ELT_THREADS) dt[i] = lt[i];
        }
        if (dst_false) {
            float *df = dst_false[m] + f_off;
            for (unsigned i = tid; i < tot_false; i += ELT_THREADS) df[i] = lf[i];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------ one parameter
// mask_loader.py:412-485.  torch.bool storage is one byte per element, 0 or 1.
__global__ __launch_bounds__(ELT_THREADS) void k_mask_combine(const uint8_t *const *__restrict__ masks, int n_masks,
                                                              int64_t numel, int strategy, uint8_t *__restrict__ out,
                                                              unsigned long long *__restrict__ count) {
    __shared__ unsigned cnt;
    combine_tile(masks, n_masks, strategy, blockIdx.x, numel, out, &cnt);
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(count, (unsigned long long)cnt);
}

__global__ __launch_bounds__(ELT_THREADS) void k_mask_count(const uint8_t *__restrict__ mask, int invert, int64_t numel,
                                                            unsigned *__restrict__ tile_counts) {
    const int64_t base = (int64_t)blockIdx.x * MASK_TILE + (int64_t)threadIdx.x * 8;
    const unsigned tot = block_sum_u32(tile_select(mask, base, numel, invert).cnt);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = tot;
}

// one block; total -> count_out
__global__ __launch_bounds__(SCAN_THREADS) void k_mask_scan(const unsigned *__restrict__ tile_counts, int ntiles,
                                                            unsigned long long *__restrict__ tile_offsets,
                                                            long long *__restrict__ count_out) {
    const unsigned long long total = scan_tiles(tile_counts, ntiles, tile_offsets);
    if (threadIdx.x == 0) *count_out = (long long)total;
}

// mask_loader.py:675-679 / :706-709: flat[mask] (or flat[~mask]) for n_src buffers sharing one mask
__global__ __launch_bounds__(ELT_THREADS) void k_mask_scatter(const float *const *__restrict__ src,
                                                              float *const *__restrict__ dst, int n_src,
                                                              const uint8_t *__restrict__ mask, int invert,
                                                              int64_t numel,
                                                              const unsigned long long *__restrict__ tile_offsets) {
    // tile_offsets were scanned over the SELECTED count (mask != invert); scatter_tile wants the offset of the
    // True elements, so for invert the roles of its two outputs are swapped
    const unsigned long long off = tile_offsets[blockIdx.x];
    if (!invert) {
        scatter_tile(mask, blockIdx.x, numel, src, dst, nullptr, n_src, off);
    } else {
        const unsigned long long true_off = (unsigned long long)blockIdx.x * MASK_TILE - off;
        scatter_tile(mask, blockIdx.x, numel, src, nullptr, dst, n_src, true_off);
    }
}

// reconstruct_from_masked (mask_loader.py:712-763): out = zeros; out[mask] = signal; out[~mask] = noise.
// Inverse of the compaction: same tile counts + scan, then a gather by rank.
__global__ __launch_bounds__(ELT_THREADS) void k_mask_expand(const float *__restrict__ sig,
                                                             const float *__restrict__ noise,
                                                             const uint8_t *__restrict__ mask, int64_t numel,
                                                             const unsigned long long *__restrict__ tile_offsets,
                                                             float *__restrict__ out) {
    // own text, not tile_select + block_scan_u32: with them the kernel was 11 % slower
    const int64_t base = (int64_t)blockIdx.x * MASK_TILE + (int64_t)threadIdx.x * 8;
    unsigned sel = 0, cnt = 0, n = 0;
    for (int e = 0; e < 8; ++e)
        if (base + e < numel) {
            ++n;
            if (mask[base + e] != 0) {
                sel |= 1u << e;
                ++cnt;
            }
        }
    __shared__ unsigned s[ELT_THREADS];
    s[threadIdx.x] = cnt;
    __syncthreads();
    for (int off = 1; off < ELT_THREADS; off <<= 1) {
        unsigned add = threadIdx.x >= off ? s[threadIdx.x - off] : 0;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    if (!n) return;
    const unsigned long long t0 = tile_offsets[blockIdx.x] + (s[threadIdx.x] - cnt);  // rank among True
    const unsigned long long f0 = (unsigned long long)base - t0;                       // rank among False
    unsigned jt = 0, jf = 0;
    for (unsigned e = 0; e < n; ++e) {
        float v;
        if (sel & (1u << e))
            v = sig[t0 + jt++];
        else
            v = noise ? noise[f0 + jf++] : 0.f;
        out[base + e] = v;
    }
}

// ------------------------------------------------------------------------------------ a set of parameters
// The same operators over a ragged SET of parameters in a handful of launches (cli.py runs them once
// per parameter and task): a tile table maps every 2048-element tile to (parameter,
// tile-in-parameter); per-parameter counts stay on the device and feed rows_dev of the plan.
struct svdq_maskset {
    int32_t n_params, n_tiles;
    int64_t *h_numel;
    int32_t *h_tile_begin;
    int64_t *d_numel;        // [Q]
    int32_t *d_tile_begin;   // [Q+1]
    int32_t *d_tile_param;   // [n_tiles]
};

__global__ __launch_bounds__(ELT_THREADS) void k_maskset_combine(const int32_t *__restrict__ tile_param,
                                                                 const int32_t *__restrict__ tile_begin,
                                                                 const int64_t *__restrict__ numel_tab,
                                                                 const uint8_t *const *__restrict__ masks, int n_masks,
                                                                 int strategy, uint8_t *const *__restrict__ outs,
                                                                 unsigned long long *__restrict__ counts,
                                                                 unsigned *__restrict__ tile_counts) {
    const int q = tile_param[blockIdx.x];
    __shared__ unsigned cnt;
    combine_tile(masks + (size_t)q * n_masks, n_masks, strategy, blockIdx.x - tile_begin[q], numel_tab[q], outs[q], &cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (tile_counts) tile_counts[blockIdx.x] = cnt;       // feeds the index build without a counting pass
        else if (cnt) atomicAdd(&counts[q], (unsigned long long)cnt);
    }
}

__global__ __launch_bounds__(ELT_THREADS) void k_maskset_count(const int32_t *__restrict__ tile_param,
                                                               const int32_t *__restrict__ tile_begin,
                                                               const int64_t *__restrict__ numel_tab,
                                                               const uint8_t *const *__restrict__ masks,
                                                               unsigned *__restrict__ tile_counts) {
    const int q = tile_param[blockIdx.x];
    const int64_t base = (int64_t)(blockIdx.x - tile_begin[q]) * MASK_TILE + (int64_t)threadIdx.x * 8;
    const unsigned tot = block_sum_u32(tile_select(masks[q], base, numel_tab[q], 0).cnt);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = tot;
}

// one block per parameter: exclusive scan of ITS tile counts; true / false totals out
__global__ __launch_bounds__(SCAN_THREADS) void k_maskset_scan(const int32_t *__restrict__ tile_begin,
                                                               const int64_t *__restrict__ numel_tab,
                                                               const unsigned *__restrict__ tile_counts,
                                                               unsigned long long *__restrict__ tile_offsets,
                                                               long long *__restrict__ count_true,
                                                               long long *__restrict__ count_false) {
    const int q = blockIdx.x, t0 = tile_begin[q];
    const unsigned long long total = scan_tiles(tile_counts + t0, tile_begin[q + 1] - t0, tile_offsets + t0);
    if (threadIdx.x == 0) {
        if (count_true) count_true[q] = (long long)total;
        if (count_false) count_false[q] = (long long)numel_tab[q] - (long long)total;
    }
}

// flat[mask] -> dst_true, flat[~mask] -> dst_false (optional), for n_src buffers per parameter, one pass
__global__ __launch_bounds__(ELT_THREADS) void k_maskset_scatter(const int32_t *__restrict__ tile_param,
                                                                 const int32_t *__restrict__ tile_begin,
                                                                 const int64_t *__restrict__ numel_tab,
                                                                 const uint8_t *const *__restrict__ masks,
                                                                 const float *const *__restrict__ src,
                                                                 float *const *__restrict__ dst_true,
                                                                 float *const *__restrict__ dst_false, int n_src,
                                                                 const unsigned long long *__restrict__ tile_offsets) {
    const int q = tile_param[blockIdx.x];
    scatter_tile(masks[q], blockIdx.x - tile_begin[q], numel_tab[q], src + (size_t)q * n_src,
                 dst_true + (size_t)q * n_src, dst_false ? dst_false + (size_t)q * n_src : nullptr, n_src,
                 tile_offsets[blockIdx.x]);
}

// Index lists for the gather mode of the streaming passes (svdq_compress_gather): the ascending flat positions
// of the selected (and, when asked, of the unselected) elements of every parameter.  Same tile scan as the
// compaction; 4 B written per element instead of 4 N B read + 4 N B written.
__device__ void maskset_index_tile(int gtile, const int32_t *__restrict__ tile_param,
                                   const int32_t *__restrict__ tile_begin, const int64_t *__restrict__ numel_tab,
                                   const uint8_t *const *__restrict__ masks, int32_t *const *__restrict__ idx_true,
                                   int32_t *const *__restrict__ idx_false,
                                   const unsigned long long *__restrict__ tile_offsets) {
    __shared__ int32_t lt[MASK_TILE], lf[MASK_TILE];
    const int q = tile_param[gtile];
    const int64_t tile = gtile - tile_begin[q], numel = numel_tab[q];
    const int tid = threadIdx.x;
    const int64_t tbase = tile * MASK_TILE;
    const int64_t base = tbase + (int64_t)tid * 8;
    const TileSel ts = tile_select(masks[q], base, numel, 0);
    unsigned tot_true;
    const unsigned incl = block_scan_u32(ts.cnt, &tot_true);
    const int tile_n = (int)((numel - tbase) < MASK_TILE ? (numel - tbase) : MASK_TILE);
    const unsigned tot_false = (unsigned)tile_n - tot_true;
    unsigned jt = incl - ts.cnt, jf = (unsigned)(tid * 8) - jt;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (e < ts.lim) {
            if (ts.sel & (1u << e))
                lt[jt++] = (int32_t)(base + e);
            else
                lf[jf++] = (int32_t)(base + e);
        }
    }
    __syncthreads();
    const unsigned long long t_off = tile_offsets[gtile];
    int32_t *dt = idx_true[q] + t_off;
    for (unsigned i = tid; i < tot_true; i += ELT_THREADS) dt[i] = lt[i];
    if (idx_false) {
        int32_t *df = idx_false[q] + ((unsigned long long)tbase - t_off);
        for (unsigned i = tid; i < tot_false; i += ELT_THREADS) df[i] = lf[i];
    }
    __syncthreads();   // the LDS images are reused by the block's next tile
}

__global__ __launch_bounds__(ELT_THREADS) void k_maskset_index(const int32_t *__restrict__ tile_param,
                                                               const int32_t *__restrict__ tile_begin,
                                                               const int64_t *__restrict__ numel_tab,
                                                               const uint8_t *const *__restrict__ masks,
                                                               int32_t *const *__restrict__ idx_true,
                                                               int32_t *const *__restrict__ idx_false,
                                                               const unsigned long long *__restrict__ tile_offsets,
                                                               int n_tiles) {
    for (int i = 0; i < MASK_TPB; ++i) {
        const int gtile = blockIdx.x * MASK_TPB + i;
        if (gtile >= n_tiles) break;
        maskset_index_tile(gtile, tile_param, tile_begin, numel_tab, masks, idx_true, idx_false, tile_offsets);
    }
}

// Tall masks as they are distributed (mask_loader.py:125-206): ONE bit per element of the flattened state dict,
// numpy.packbits order (first element = most significant bit), one stream per task.  Combining them from the
// packed form reads N/8 bytes per element instead of N: parameter q's elements are bits bit_off[q] + e of every
// stream.  Output: the combined mask as bool bytes (what the reference hands on), tile counts for the index build.
__device__ void maskset_combine_packed_tile(int gtile, const int32_t *__restrict__ tile_param,
                                                                        const int32_t *__restrict__ tile_begin,
                                                                        const int64_t *__restrict__ numel_tab,
                                                                        const uint8_t *const *__restrict__ streams,
                                                                        const int64_t *__restrict__ bit_off,
                                                                        const int64_t *__restrict__ stream_bytes,
                                                                        int n_masks, int strategy,
                                                                        uint8_t *const *__restrict__ outs,
                                                                        unsigned *__restrict__ tile_counts) {
    // the tile's packed bytes of every stream are fetched with 16-byte loads into LDS first (17 chunks cover the 257
    // bytes a 2048-element tile can touch at an arbitrary bit offset); byte loads per thread would waste the bus
    __shared__ __attribute__((aligned(16))) uint8_t S[SVDQ_MAX_TASKS][17 * 16];
    const int q = tile_param[gtile];
    const int64_t numel = numel_tab[q];
    const int64_t tile0 = (int64_t)(gtile - tile_begin[q]) * MASK_TILE;
    const int64_t base = tile0 + (int64_t)threadIdx.x * 8;
    const int64_t c0 = ((bit_off[q] + tile0) >> 3) & ~(int64_t)15;   // first 16-byte chunk of this tile in every stream
    for (int i = threadIdx.x; i < n_masks * 17; i += ELT_THREADS) {
        const int m = i / 17, c = i - m * 17;
        const int64_t b = c0 + 16 * c;
        const int64_t nb = stream_bytes[m];
        uint4 v = {0u, 0u, 0u, 0u};
        if (b + 16 <= nb) {
            v = *reinterpret_cast<const uint4 *>(streams[m] + b);
        } else if (b < nb) {
            uint8_t tmp[16];
            for (int k = 0; k < 16; ++k) tmp[k] = (b + k < nb) ? streams[m][b + k] : (uint8_t)0;
            v = *reinterpret_cast<const uint4 *>(tmp);
        }
        *reinterpret_cast<uint4 *>(&S[m][16 * c]) = v;
    }
    __syncthreads();
    unsigned cnt = 0;
    if (base < numel) {
        const int lim = (int)((numel - base) < 8 ? (numel - base) : 8);
        const int64_t pos = bit_off[q] + base;   // bit position of this thread's first element in every stream
        const int byte = (int)((pos >> 3) - c0);
        const int sh = (int)(pos & 7);
        unsigned char cnts[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) cnts[j] = 0;
        unsigned any = 0, all = 0xff;
        for (int m = 0; m < n_masks; ++m) {
            const unsigned w = ((unsigned)S[m][byte] << 8) | S[m][byte + 1];   // byte + 1 <= 16 * 17 - 1: in the image
            const unsigned bits = (w >> (8 - sh)) & 0xff;   // 8 elements, first element = bit 7
            any |= bits;
            all &= bits;
            if (strategy == SVDQ_MASK_MAJORITY) {
#pragma unroll
                for (int j = 0; j < 8; ++j) cnts[j] += (bits >> (7 - j)) & 1;
            }
        }
        unsigned long long res = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            unsigned bit;
            if (strategy == SVDQ_MASK_UNION)
                bit = (any >> (7 - j)) & 1;
            else if (strategy == SVDQ_MASK_INTERSECTION)
                bit = (all >> (7 - j)) & 1;
            else
                bit = 2 * cnts[j] >= n_masks;
            if (j < lim) res |= (unsigned long long)bit << (8 * j);
        }
        uint8_t *out = outs[q];
        if (lim == 8 && (reinterpret_cast<uintptr_t>(out + base) & 7) == 0) {
            *reinterpret_cast<unsigned long long *>(out + base) = res;
        } else {
            for (int j = 0; j < lim; ++j) out[base + j] = (uint8_t)((res >> (8 * j)) & 1);
        }
        cnt = (unsigned)__popcll(res);
    }
    const unsigned tot = block_sum_u32(cnt);
    if (threadIdx.x == 0) tile_counts[gtile] = tot;
    __syncthreads();   // the LDS image is reused by the block's next tile
}

__global__ __launch_bounds__(ELT_THREADS) void k_maskset_combine_packed(const int32_t *__restrict__ tile_param,
                                                                        const int32_t *__restrict__ tile_begin,
                                                                        const int64_t *__restrict__ numel_tab,
                                                                        const uint8_t *const *__restrict__ streams,
                                                                        const int64_t *__restrict__ bit_off,
                                                                        const int64_t *__restrict__ stream_bytes,
                                                                        int n_masks, int strategy,
                                                                        uint8_t *const *__restrict__ outs,
                                                                        unsigned *__restrict__ tile_counts, int n_tiles) {
    for (int i = 0; i < MASK_TPB; ++i) {
        const int gtile = blockIdx.x * MASK_TPB + i;
        if (gtile >= n_tiles) break;
        maskset_combine_packed_tile(gtile, tile_param, tile_begin, numel_tab, streams, bit_off, stream_bytes, n_masks,
                                    strategy, outs, tile_counts);
    }
}

// ------------------------------------------------------------------------------------ walk mode: unit starts
// The mask-walk mode of the streaming passes (svdq_compress_masked, svdq_stream.h "walk mode") needs, for every work
// unit of the plan, the SOURCE position of the unit's first row -- the element of rank unit.row0 among the selected
// (or, for the noise region, the cleared) elements of its mask.  One wavefront per unit: a 64-ary search over the
// exclusive tile offsets of the scan, then one pass over the 2048 mask bytes of the tile that holds the element.
// entry_map: NULL (plan parameter p uses mask p, selected elements) or [n_params] int32: low 31 bits = which mask of the
// set, bit 31 = the cleared elements.  Units past rows_dev[p] get numel (nothing to walk).  Bit 62 of every start
// carries the polarity to the streaming kernels.
#define SVDQ_WALK_INV (1ll << 62)
__global__ __launch_bounds__(64) void k_maskset_unit_starts(const SvdqParam *__restrict__ params,
                                                            const SvdqUnit *__restrict__ units,
                                                            const int64_t *__restrict__ rows_dev,
                                                            const int32_t *__restrict__ entry_map,
                                                            const int32_t *__restrict__ tile_begin,
                                                            const int64_t *__restrict__ numel_tab,
                                                            const uint8_t *const *__restrict__ masks,
                                                            const unsigned long long *__restrict__ tile_offsets,
                                                            int64_t *__restrict__ ustart) {
    const int u = blockIdx.x, lane = threadIdx.x;
    const SvdqUnit ud = units[u];
    const int p = ud.param;
    const unsigned em = entry_map ? (unsigned)entry_map[p] : (unsigned)p;
    const int q = (int)(em & 0x7fffffffu), inv = (int)(em >> 31);
    const int64_t numel = numel_tab[q];
    const int64_t tag = inv ? SVDQ_WALK_INV : 0;
    const int64_t D = rows_dev ? rows_dev[p] : params[p].rows;
    if (ud.row0 >= D) {
        if (lane == 0) ustart[u] = numel | tag;
        return;
    }
    const unsigned long long target = (unsigned long long)ud.row0;
    const int t0 = tile_begin[q], nt = tile_begin[q + 1] - t0;
    // off(i) = selected elements in front of tile i
    auto off = [&](int i) -> unsigned long long {
        const unsigned long long t = tile_offsets[t0 + i];
        return inv ? (unsigned long long)i * MASK_TILE - t : t;
    };
    int lo = 0, hi = nt;   // invariant: off(lo) <= target, the answer is the largest such tile in [lo, hi)
    while (hi - lo > 1) {
        const int step = (hi - lo + 63) / 64;
        const int i = lo + lane * step;
        const bool ok = i < hi && off(i) <= target;
        const int j = (int)__popcll(__ballot(ok)) - 1;   // off is monotone: lanes 0..j pass, lane 0 always does
        const int nlo = lo + (j < 0 ? 0 : j) * step;
        hi = (nlo + step < hi) ? nlo + step : hi;
        lo = nlo;
    }
    const unsigned rem = (unsigned)(target - off(lo));   // rank inside the tile
    const int64_t tb = (int64_t)lo * MASK_TILE;
    // 32 bytes per lane: a different shape from tile_select's 8 per thread, so this read keeps its own text
    const uint8_t *m = masks[q] + tb + 32 * lane;
    unsigned bits = 0;
    const int64_t left = numel - (tb + 32 * lane);
    if (left >= 32 && (reinterpret_cast<uintptr_t>(m) & 7) == 0) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned long long x = reinterpret_cast<const unsigned long long *>(m)[w];
#pragma unroll
            for (int e = 0; e < 8; ++e) bits |= (unsigned)(((x >> (8 * e)) & 0xff) != 0) << (8 * w + e);
        }
    } else {
        for (int e = 0; e < 32; ++e)
            if (e < left) bits |= (unsigned)(m[e] != 0) << e;
    }
    if (inv) {
        bits = ~bits;
        if (left < 32) bits &= left > 0 ? ((1u << left) - 1u) : 0u;
    }
    const unsigned cnt = __popc(bits);
    unsigned incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    const unsigned excl = incl - cnt;
    const bool mine = excl <= rem && rem < incl;
    if (mine) {
        unsigned b = bits;
        for (unsigned i = excl; i < rem; ++i) b &= b - 1;   // drop the set bits in front of ours
        ustart[u] = (tb + 32 * lane + (__ffs(b) - 1)) | tag;
    }
    if (__ballot(mine) == 0 && lane == 0) ustart[u] = numel | tag;   // counts and mask disagree: nothing to walk
}

// ------------------------------------------------------------------------------------ host: work buffer and checks
// The work buffer of every entry point, for ntiles tiles: [tile_counts: 4 B per tile][tile_offsets: 8 B per tile]
// [total: one int64 in the 256 spare bytes -- where svdq_mask_expand lets the scan put the count nobody asked for],
// each region 256-byte aligned.
struct MaskWork {
    unsigned *tile_counts;
    unsigned long long *tile_offsets;
    long long *total;
};

static int64_t mask_work_bytes(int64_t ntiles) {
    return svdq_align_up(ntiles * 4, 256) + svdq_align_up(ntiles * 8, 256) + 256;
}

static MaskWork mask_work(void *work, int64_t ntiles) {
    uint8_t *wb = reinterpret_cast<uint8_t *>(work);
    uint8_t *offs = wb + svdq_align_up(ntiles * 4, 256);
    return {reinterpret_cast<unsigned *>(wb), reinterpret_cast<unsigned long long *>(offs),
            reinterpret_cast<long long *>(offs + svdq_align_up(ntiles * 8, 256))};
}

static int mask_tiles(int64_t numel) { return (int)((numel + MASK_TILE - 1) / MASK_TILE); }

static int launch_result() { return hipGetLastError() == hipSuccess ? SVDQ_OK : SVDQ_EHIP; }

static bool bool_mask_count_ok(int n_masks, const char *who) {
    if (n_masks <= SVDQ_MAX_BOOL_MASKS) return true;
    svdq_set_error("%s: at most %d bool masks can be combined, got %d", who, SVDQ_MAX_BOOL_MASKS, n_masks);
    return false;
}

static bool packed_mask_count_ok(int n_masks) {
    if (n_masks <= SVDQ_MAX_TASKS) return true;
    svdq_set_error("at most %d packed mask streams are supported, got %d", SVDQ_MAX_TASKS, n_masks);
    return false;
}

// The first check of the fused combine entries.  An empty list is named as the reference names it
// (mask_loader.py:425) even when a pointer is missing as well.
static bool combine_args_ok(bool pointers_ok, int n_masks, const char *who) {
    if (pointers_ok && n_masks >= 1) return true;
    if (n_masks < 1)
        svdq_set_error("Empty mask list");
    else
        svdq_set_error("%s: bad argument", who);
    return false;
}

// strategy is a SVDQ_MASK_* value; with `votes` (svdq_mask_combine alone) bits 8.. may carry votes needed + 1 for the
// majority vote, votes needed in 0 .. n_masks + 1 (n_masks + 1: no element can pass)
static bool mask_strategy_ok(int strategy, int n_masks, bool votes) {
    const int kind = strategy & 0xff, need1 = strategy >> 8;
    const bool ok = strategy >= 0 && kind <= SVDQ_MASK_MAJORITY &&
                    (votes ? (need1 == 0 || kind == SVDQ_MASK_MAJORITY) && need1 <= n_masks + 2 : need1 == 0);
    if (!ok) svdq_set_error("Unknown mask strategy: %d", strategy);  // mask_loader.py:611
    return ok;
}

// index lists are int32
static bool maskset_index_ok(const svdq_maskset *ms, const char *who) {
    for (int q = 0; q < ms->n_params; ++q)
        if (ms->h_numel[q] > 0x7fffffffLL) {
            svdq_set_error("%s: parameter %d has more than 2^31-1 elements", who, q);
            return false;
        }
    return true;
}

static int maskset_check_plan(const svdq_maskset *ms, const svdq_plan *pl, const char *who, bool identity) {
    if (!ms || !pl) {
        svdq_set_error("%s: bad argument", who);
        return SVDQ_EINVAL;
    }
    if (identity) {
        if (pl->n_params != ms->n_params) {
            svdq_set_error("%s: the plan has %d parameters, the mask set %d", who, pl->n_params, ms->n_params);
            return SVDQ_EINVAL;
        }
        for (int q = 0; q < ms->n_params; ++q)
            if (pl->h_params[q].rows != ms->h_numel[q]) {
                svdq_set_error("Shape mismatch: parameter %d has %lld elements in the plan and %lld in the mask set", q,
                               (long long)pl->h_params[q].rows, (long long)ms->h_numel[q]);
                return SVDQ_EINVAL;
            }
    }
    return SVDQ_OK;
}

// ------------------------------------------------------------------------------------ host: one parameter
extern "C" int64_t svdq_mask_work_bytes(int64_t numel) { return mask_work_bytes(mask_tiles(numel)); }

extern "C" int svdq_mask_combine(const void *mask_ptrs, int32_t n_masks, int64_t numel, int32_t strategy, uint8_t *out,
                                 int64_t *count, void *work, void *stream) {
    (void)work;
    if (n_masks < 1) {
        svdq_set_error("Empty mask list");  // mask_loader.py:425
        return SVDQ_EINVAL;
    }
    if (!bool_mask_count_ok(n_masks, "svdq_mask_combine")) return SVDQ_EINVAL;
    if (!mask_strategy_ok(strategy, n_masks, true)) return SVDQ_EINVAL;
    if (!mask_ptrs || !out || !count || numel < 1) {
        svdq_set_error("svdq_mask_combine: bad argument");
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, 8, st) != hipSuccess) return SVDQ_EHIP;
    hipLaunchKernelGGL(k_mask_combine, dim3(mask_tiles(numel)), dim3(ELT_THREADS), 0, st,
                       reinterpret_cast<const uint8_t *const *>(mask_ptrs), n_masks, numel, strategy, out,
                       reinterpret_cast<unsigned long long *>(count));
    return launch_result();
}

// count + scan of one mask: tile offsets in w, the number of selected elements -> total
static void launch_count_scan1(const uint8_t *mask, int invert, int64_t numel, const MaskWork &w, long long *total,
                               hipStream_t st) {
    const int ntiles = mask_tiles(numel);
    hipLaunchKernelGGL(k_mask_count, dim3(ntiles), dim3(ELT_THREADS), 0, st, mask, invert, numel, w.tile_counts);
    hipLaunchKernelGGL(k_mask_scan, dim3(1), dim3(SCAN_THREADS), 0, st, w.tile_counts, ntiles, w.tile_offsets, total);
}

extern "C" int svdq_mask_compact(const void *src_ptrs, const void *dst_ptrs, int32_t n_src, const uint8_t *mask,
                                 int32_t invert, int64_t numel, int64_t *count, void *work, void *stream) {
    if (!src_ptrs || !dst_ptrs || !mask || !count || !work || n_src < 1 || numel < 1) {
        svdq_set_error("svdq_mask_compact: bad argument");
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const MaskWork w = mask_work(work, mask_tiles(numel));
    launch_count_scan1(mask, invert, numel, w, reinterpret_cast<long long *>(count), st);
    hipLaunchKernelGGL(k_mask_scatter, dim3(mask_tiles(numel)), dim3(ELT_THREADS), 0, st,
                       reinterpret_cast<const float *const *>(src_ptrs), reinterpret_cast<float *const *>(dst_ptrs),
                       n_src, mask, invert, numel, w.tile_offsets);
    return launch_result();
}

extern "C" int svdq_mask_expand(const float *signal, const float *noise, const uint8_t *mask, int64_t numel,
                                float *out, void *work, void *stream) {
    if (!signal || !mask || !out || !work || numel < 1) {
        svdq_set_error("svdq_mask_expand: bad argument");
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const MaskWork w = mask_work(work, mask_tiles(numel));
    launch_count_scan1(mask, 0, numel, w, w.total, st);
    hipLaunchKernelGGL(k_mask_expand, dim3(mask_tiles(numel)), dim3(ELT_THREADS), 0, st, signal, noise, mask, numel,
                       w.tile_offsets, out);
    return launch_result();
}

// ------------------------------------------------------------------------------------ host: a set of parameters
extern "C" int svdq_maskset_create(svdq_maskset **out, int32_t n_params, const int64_t *numel) {
    if (!out || !numel || n_params < 1) {
        svdq_set_error("svdq_maskset_create: bad argument");
        return SVDQ_EINVAL;
    }
    svdq_maskset *ms = (svdq_maskset *)calloc(1, sizeof(svdq_maskset));
    ms->n_params = n_params;
    ms->h_numel = (int64_t *)calloc(n_params, sizeof(int64_t));
    ms->h_tile_begin = (int32_t *)calloc(n_params + 1, sizeof(int32_t));
    int64_t tiles = 0;
    for (int q = 0; q < n_params; ++q) {
        if (numel[q] < 1) {
            svdq_set_error("svdq_maskset_create: parameter %d has %lld elements", q, (long long)numel[q]);
            free(ms->h_numel);
            free(ms->h_tile_begin);
            free(ms);
            return SVDQ_EINVAL;
        }
        ms->h_numel[q] = numel[q];
        ms->h_tile_begin[q] = (int32_t)tiles;
        tiles += (numel[q] + MASK_TILE - 1) / MASK_TILE;
    }
    ms->h_tile_begin[n_params] = (int32_t)tiles;
    ms->n_tiles = (int32_t)tiles;
    int32_t *tp = (int32_t *)malloc(sizeof(int32_t) * tiles);
    for (int q = 0; q < n_params; ++q)
        for (int t = ms->h_tile_begin[q]; t < ms->h_tile_begin[q + 1]; ++t) tp[t] = q;
    hipError_t e = hipMalloc((void **)&ms->d_numel, sizeof(int64_t) * n_params);
    if (e == hipSuccess) e = hipMalloc((void **)&ms->d_tile_begin, sizeof(int32_t) * (n_params + 1));
    if (e == hipSuccess) e = hipMalloc((void **)&ms->d_tile_param, sizeof(int32_t) * tiles);
    if (e == hipSuccess) e = hipMemcpy(ms->d_numel, ms->h_numel, sizeof(int64_t) * n_params, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(ms->d_tile_begin, ms->h_tile_begin, sizeof(int32_t) * (n_params + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ms->d_tile_param, tp, sizeof(int32_t) * tiles, hipMemcpyHostToDevice);
    free(tp);
    if (e != hipSuccess) {
        svdq_set_error("svdq_maskset_create: %s", hipGetErrorString(e));
        svdq_maskset_destroy(ms);
        return SVDQ_EHIP;
    }
    *out = ms;
    return SVDQ_OK;
}

extern "C" void svdq_maskset_destroy(svdq_maskset *ms) {
    if (!ms) return;
    if (ms->d_numel) (void)hipFree(ms->d_numel);
    if (ms->d_tile_begin) (void)hipFree(ms->d_tile_begin);
    if (ms->d_tile_param) (void)hipFree(ms->d_tile_param);
    free(ms->h_numel);
    free(ms->h_tile_begin);
    free(ms);
}

extern "C" int64_t svdq_maskset_work_bytes(const svdq_maskset *ms) { return ms ? mask_work_bytes(ms->n_tiles) : 0; }

// ---- sources: each fills the tile counts of the whole set (launch_combine: or, with tile_counts = NULL, adds to the
// per-parameter counts)
static dim3 tpb_grid(const svdq_maskset *ms) { return dim3((ms->n_tiles + MASK_TPB - 1) / MASK_TPB); }

static void launch_count(const svdq_maskset *ms, const void *mask_ptrs, unsigned *tile_counts, hipStream_t st) {
    hipLaunchKernelGGL(k_maskset_count, dim3(ms->n_tiles), dim3(ELT_THREADS), 0, st, ms->d_tile_param, ms->d_tile_begin,
                       ms->d_numel, reinterpret_cast<const uint8_t *const *>(mask_ptrs), tile_counts);
}

static void launch_combine(const svdq_maskset *ms, const void *mask_ptrs, int n_masks, int strategy,
                           const void *out_ptrs, int64_t *counts, unsigned *tile_counts, hipStream_t st) {
    hipLaunchKernelGGL(k_maskset_combine, dim3(ms->n_tiles), dim3(ELT_THREADS), 0, st, ms->d_tile_param,
                       ms->d_tile_begin, ms->d_numel, reinterpret_cast<const uint8_t *const *>(mask_ptrs), n_masks,
                       strategy, reinterpret_cast<uint8_t *const *>(out_ptrs),
                       reinterpret_cast<unsigned long long *>(counts), tile_counts);
}

static void launch_combine_packed(const svdq_maskset *ms, const void *stream_ptrs, const int64_t *stream_bytes,
                                  const int64_t *bit_offsets, int n_masks, int strategy, const void *out_ptrs,
                                  unsigned *tile_counts, hipStream_t st) {
    hipLaunchKernelGGL(k_maskset_combine_packed, tpb_grid(ms), dim3(ELT_THREADS), 0, st, ms->d_tile_param,
                       ms->d_tile_begin, ms->d_numel, reinterpret_cast<const uint8_t *const *>(stream_ptrs), bit_offsets,
                       stream_bytes, n_masks, strategy, reinterpret_cast<uint8_t *const *>(out_ptrs), tile_counts,
                       ms->n_tiles);
}

// ---- backs: the scan of every parameter's tile counts, then what reads the offsets
static void launch_scan(const svdq_maskset *ms, const MaskWork &w, int64_t *count_true, int64_t *count_false,
                        hipStream_t st) {
    hipLaunchKernelGGL(k_maskset_scan, dim3(ms->n_params), dim3(SCAN_THREADS), 0, st, ms->d_tile_begin, ms->d_numel,
                       w.tile_counts, w.tile_offsets, reinterpret_cast<long long *>(count_true),
                       reinterpret_cast<long long *>(count_false));
}

static void launch_index(const svdq_maskset *ms, const void *mask_ptrs, const void *idx_true_ptrs,
                         const void *idx_false_ptrs, const unsigned long long *tile_offsets, hipStream_t st) {
    hipLaunchKernelGGL(k_maskset_index, tpb_grid(ms), dim3(ELT_THREADS), 0, st, ms->d_tile_param, ms->d_tile_begin,
                       ms->d_numel, reinterpret_cast<const uint8_t *const *>(mask_ptrs),
                       reinterpret_cast<int32_t *const *>(idx_true_ptrs),
                       reinterpret_cast<int32_t *const *>(idx_false_ptrs), tile_offsets, ms->n_tiles);
}

static void launch_unit_starts(const svdq_maskset *ms, const svdq_plan *pl, const void *mask_ptrs,
                               const int32_t *entry_map, const int64_t *rows_dev,
                               const unsigned long long *tile_offsets, int64_t *unit_start, hipStream_t st) {
    hipLaunchKernelGGL(k_maskset_unit_starts, dim3(pl->n_units), dim3(64), 0, st, pl->d_params, pl->d_units, rows_dev,
                       entry_map, ms->d_tile_begin, ms->d_numel, reinterpret_cast<const uint8_t *const *>(mask_ptrs),
                       tile_offsets, unit_start);
}

// ---- entry points: checks, a source, the scan, a back
extern "C" int svdq_maskset_combine(const svdq_maskset *ms, const void *mask_ptrs, int32_t n_masks, int32_t strategy,
                                    const void *out_ptrs, int64_t *counts, void *stream) {
    if (!ms || !mask_ptrs || !out_ptrs || !counts) {
        svdq_set_error("svdq_maskset_combine: bad argument");
        return SVDQ_EINVAL;
    }
    if (n_masks < 1) {
        svdq_set_error("Empty mask list");
        return SVDQ_EINVAL;
    }
    if (!bool_mask_count_ok(n_masks, "svdq_maskset_combine")) return SVDQ_EINVAL;
    if (!mask_strategy_ok(strategy, n_masks, false)) return SVDQ_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(int64_t) * ms->n_params, st) != hipSuccess) return SVDQ_EHIP;
    launch_combine(ms, mask_ptrs, n_masks, strategy, out_ptrs, counts, nullptr, st);
    return launch_result();
}

extern "C" int svdq_maskset_compact(const svdq_maskset *ms, const void *mask_ptrs, const void *src_ptrs,
                                    const void *dst_true_ptrs, const void *dst_false_ptrs, int32_t n_src,
                                    int64_t *count_true, int64_t *count_false, void *work, void *stream) {
    if (!ms || !mask_ptrs || !src_ptrs || !dst_true_ptrs || !work || n_src < 1) {
        svdq_set_error("svdq_maskset_compact: bad argument");
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const MaskWork w = mask_work(work, ms->n_tiles);
    launch_count(ms, mask_ptrs, w.tile_counts, st);
    launch_scan(ms, w, count_true, count_false, st);
    hipLaunchKernelGGL(k_maskset_scatter, dim3(ms->n_tiles), dim3(ELT_THREADS), 0, st, ms->d_tile_param,
                       ms->d_tile_begin, ms->d_numel, reinterpret_cast<const uint8_t *const *>(mask_ptrs),
                       reinterpret_cast<const float *const *>(src_ptrs),
                       reinterpret_cast<float *const *>(dst_true_ptrs),
                       reinterpret_cast<float *const *>(dst_false_ptrs), n_src, w.tile_offsets);
    return launch_result();
}

extern "C" int svdq_maskset_indices(const svdq_maskset *ms, const void *mask_ptrs, const void *idx_true_ptrs,
                                    const void *idx_false_ptrs, int64_t *count_true, int64_t *count_false, void *work,
                                    void *stream) {
    if (!ms || !mask_ptrs || !idx_true_ptrs || !count_true || !work) {
        svdq_set_error("svdq_maskset_indices: bad argument");
        return SVDQ_EINVAL;
    }
    if (!maskset_index_ok(ms, "svdq_maskset_indices")) return SVDQ_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const MaskWork w = mask_work(work, ms->n_tiles);
    launch_count(ms, mask_ptrs, w.tile_counts, st);
    launch_scan(ms, w, count_true, count_false, st);
    launch_index(ms, mask_ptrs, idx_true_ptrs, idx_false_ptrs, w.tile_offsets, st);
    return launch_result();
}

extern "C" int svdq_maskset_combine_indices(const svdq_maskset *ms, const void *mask_ptrs, int32_t n_masks,
                                            int32_t strategy, const void *out_ptrs, const void *idx_true_ptrs,
                                            const void *idx_false_ptrs, int64_t *count_true, int64_t *count_false,
                                            void *work, void *stream) {
    const char *who = "svdq_maskset_combine_indices";
    if (!combine_args_ok(ms && mask_ptrs && out_ptrs && idx_true_ptrs && count_true && work, n_masks, who))
        return SVDQ_EINVAL;
    if (!bool_mask_count_ok(n_masks, who) || !mask_strategy_ok(strategy, n_masks, false)) return SVDQ_EINVAL;
    if (!maskset_index_ok(ms, who)) return SVDQ_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const MaskWork w = mask_work(work, ms->n_tiles);
    launch_combine(ms, mask_ptrs, n_masks, strategy, out_ptrs, nullptr, w.tile_counts, st);
    launch_scan(ms, w, count_true, count_false, st);
    launch_index(ms, out_ptrs, idx_true_ptrs, idx_false_ptrs, w.tile_offsets, st);
    return launch_result();
}

extern "C" int svdq_maskset_combine_packed_indices(const svdq_maskset *ms, const void *stream_ptrs,
                                                   const int64_t *stream_bytes, const int64_t *bit_offsets,
                                                   int32_t n_masks, int32_t strategy, const void *out_ptrs,
                                                   const void *idx_true_ptrs, const void *idx_false_ptrs,
                                                   int64_t *count_true, int64_t *count_false, void *work,
                                                   void *stream) {
    const char *who = "svdq_maskset_combine_packed_indices";
    if (!combine_args_ok(ms && stream_ptrs && stream_bytes && bit_offsets && out_ptrs && idx_true_ptrs && count_true &&
                             work, n_masks, who))
        return SVDQ_EINVAL;
    if (!packed_mask_count_ok(n_masks) || !mask_strategy_ok(strategy, n_masks, false)) return SVDQ_EINVAL;
    if (!maskset_index_ok(ms, who)) return SVDQ_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const MaskWork w = mask_work(work, ms->n_tiles);
    launch_combine_packed(ms, stream_ptrs, stream_bytes, bit_offsets, n_masks, strategy, out_ptrs, w.tile_counts, st);
    launch_scan(ms, w, count_true, count_false, st);
    launch_index(ms, out_ptrs, idx_true_ptrs, idx_false_ptrs, w.tile_offsets, st);
    return launch_result();
}

extern "C" int svdq_maskset_count_scan(const svdq_maskset *ms, const void *mask_ptrs, int64_t *count_true,
                                       int64_t *count_false, void *work, void *stream) {
    if (!ms || !mask_ptrs || !count_true || !work) {
        svdq_set_error("svdq_maskset_count_scan: bad argument");
        return SVDQ_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const MaskWork w = mask_work(work, ms->n_tiles);
    launch_count(ms, mask_ptrs, w.tile_counts, st);
    launch_scan(ms, w, count_true, count_false, st);
    return launch_result();
}

extern "C" int svdq_maskset_unit_starts(const svdq_maskset *ms, const svdq_plan *pl, const void *mask_ptrs,
                                        const int32_t *entry_map, const int64_t *rows_dev, const void *work,
                                        int64_t *unit_start, void *stream) {
    if (!mask_ptrs || !rows_dev || !work || !unit_start) {
        svdq_set_error("svdq_maskset_unit_starts: bad argument");
        return SVDQ_EINVAL;
    }
    if (int rc = maskset_check_plan(ms, pl, "svdq_maskset_unit_starts", entry_map == nullptr)) return rc;
    // the offsets a svdq_maskset_count_scan left in `work`; nothing is written to it here
    const MaskWork w = mask_work(const_cast<void *>(work), ms->n_tiles);
    launch_unit_starts(ms, pl, mask_ptrs, entry_map, rows_dev, w.tile_offsets, unit_start, (hipStream_t)stream);
    return launch_result();
}

extern "C" int svdq_maskset_combine_starts(const svdq_maskset *ms, const svdq_plan *pl, const void *mask_ptrs,
                                           int32_t n_masks, int32_t strategy, const void *out_ptrs, int64_t *count_true,
                                           int64_t *count_false, void *work, int64_t *unit_start, void *stream) {
    const char *who = "svdq_maskset_combine_starts";
    if (!combine_args_ok(mask_ptrs && out_ptrs && count_true && work && unit_start, n_masks, who)) return SVDQ_EINVAL;
    if (!bool_mask_count_ok(n_masks, who) || !mask_strategy_ok(strategy, n_masks, false)) return SVDQ_EINVAL;
    if (int rc = maskset_check_plan(ms, pl, who, true)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const MaskWork w = mask_work(work, ms->n_tiles);
    launch_combine(ms, mask_ptrs, n_masks, strategy, out_ptrs, nullptr, w.tile_counts, st);
    launch_scan(ms, w, count_true, count_false, st);
    launch_unit_starts(ms, pl, out_ptrs, nullptr, count_true, w.tile_offsets, unit_start, st);
    return launch_result();
}

extern "C" int svdq_maskset_combine_packed_starts(const svdq_maskset *ms, const svdq_plan *pl, const void *stream_ptrs,
                                                  const int64_t *stream_bytes, const int64_t *bit_offsets,
                                                  int32_t n_masks, int32_t strategy, const void *out_ptrs,
                                                  int64_t *count_true, int64_t *count_false, void *work,
                                                  int64_t *unit_start, void *stream) {
    const char *who = "svdq_maskset_combine_packed_starts";
    if (!combine_args_ok(stream_ptrs && stream_bytes && bit_offsets && out_ptrs && count_true && work && unit_start,
                         n_masks, who))
        return SVDQ_EINVAL;
    if (!packed_mask_count_ok(n_masks) || !mask_strategy_ok(strategy, n_masks, false)) return SVDQ_EINVAL;
    if (int rc = maskset_check_plan(ms, pl, who, true)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const MaskWork w = mask_work(work, ms->n_tiles);
    launch_combine_packed(ms, stream_ptrs, stream_bytes, bit_offsets, n_masks, strategy, out_ptrs, w.tile_counts, st);
    launch_scan(ms, w, count_true, count_false, st);
    launch_unit_starts(ms, pl, out_ptrs, nullptr, count_true, w.tile_offsets, unit_start, st);
    return launch_result();
}
