// svdq_small_view.h -- the packed small-artifact buffer of a plan: where its typed arrays sit (svdq_small_layout,
// include/svdq.h) and ONE typed view of them for the host-side launchers.  Plain C++: no device code, no HIP call.
#pragma once

#include <stdint.h>

#include <type_traits>

#include "../../include/svdq.h"

// P parameters, N task slots, S quantizer stages; every array starts on a 64-byte boundary
static inline svdq_small_layout svdq_small_layout_of(int64_t P, int64_t N, int64_t S) {
    svdq_small_layout L;
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = off;
        off += (bytes + 63) / 64 * 64;
        return at;
    };
    L.sigma_off = take(P * N * 4);
    L.k_off = take(P * 4);
    L.r_off = take(P * 4);
    L.energy_off = take(P * 4);
    L.rows_off = take(P * 8);
    L.chigh_off = take(P * N * N * 2);
    L.codes_off = take(P * N * S * N);
    L.scale_off = take(P * N * S * 4);
    L.zp_off = take(P * N * S * 4);
    L.rnorm_off = take(P * N * S * 4);
    L.coef_off = take(P * N * N * 4);
    L.status_off = take(64);
    L.total_bytes = off;
    return L;
}

// Every array of the layout, typed.  W: the buffer is written (the compressor's and the consolidation's outputs);
// otherwise every pointer is to const.
template <bool W> struct SmallViewT {
    template <typename T> using Ptr = std::conditional_t<W, T *, const T *>;
    Ptr<float> sigma;
    Ptr<int32_t> k, r;
    Ptr<float> energy;
    Ptr<int64_t> rows;
    Ptr<uint16_t> chigh;
    Ptr<uint8_t> codes;
    Ptr<float> scale, zp, rnorm, coef;
    Ptr<int32_t> status;
};
using SmallView = SmallViewT<false>;
using SmallViewMut = SmallViewT<true>;

template <bool W>
static inline SmallViewT<W> svdq_small_view_of(const svdq_small_layout &L, std::conditional_t<W, void *, const void *> small) {
    using B = std::conditional_t<W, uint8_t *, const uint8_t *>;
    const B sm = reinterpret_cast<B>(small);
    auto at = [&](int64_t off, auto tag) {
        return reinterpret_cast<typename SmallViewT<W>::template Ptr<decltype(tag)>>(sm + off);
    };
    SmallViewT<W> v;
    v.sigma = at(L.sigma_off, float{});
    v.k = at(L.k_off, int32_t{});
    v.r = at(L.r_off, int32_t{});
    v.energy = at(L.energy_off, float{});
    v.rows = at(L.rows_off, int64_t{});
    v.chigh = at(L.chigh_off, uint16_t{});
    v.codes = at(L.codes_off, uint8_t{});
    v.scale = at(L.scale_off, float{});
    v.zp = at(L.zp_off, float{});
    v.rnorm = at(L.rnorm_off, float{});
    v.coef = at(L.coef_off, float{});
    v.status = at(L.status_off, int32_t{});
    return v;
}
static inline SmallView small_view(const svdq_small_layout &L, const void *small) { return svdq_small_view_of<false>(L, small); }
static inline SmallViewMut small_view_mut(const svdq_small_layout &L, void *small) { return svdq_small_view_of<true>(L, small); }
