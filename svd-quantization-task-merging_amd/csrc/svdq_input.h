// svdq_input.h -- the element types the streaming kernels read task, fine-tuned and base tensors as
// (svdq_plan_set_input_type): float, __half, __hip_bfloat16.  A half element is widened to fp32 in registers right
// after the load; both conversions are exact, so everything after the load -- centring, the MFMA operands, the fp32
// block sums, the fp64 sums across blocks -- sees the same fp32 values as for the same tensor stored as fp32.
// Loads keep the lane -> row map of the fp32 kernels: four consecutive elements per lane are 16 B of fp32 or 8 B of
// half (hence the 8-byte alignment half tensors need), two are 8 B or 4 B.
#pragma once

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "svdq_common.h"

template <typename TIN> struct SvdqIn;
template <> struct SvdqIn<float> {
    typedef const __attribute__((address_space(1))) float g;   // one global element
    static __device__ __forceinline__ float cvt(float x) { return x; }
};
template <> struct SvdqIn<__half> {
    typedef const __attribute__((address_space(1))) uint16_t g;
    static __device__ __forceinline__ float cvt(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
};
template <> struct SvdqIn<__hip_bfloat16> {
    typedef const __attribute__((address_space(1))) uint16_t g;
    static __device__ __forceinline__ float cvt(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
};
template <typename TIN> using gin = typename SvdqIn<TIN>::g;

template <typename TIN> __device__ __forceinline__ float in_load1(gin<TIN> *p) { return SvdqIn<TIN>::cvt(*p); }

typedef float svdq_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned svdq_u32x2 __attribute__((ext_vector_type(2)));

// four consecutive elements (16 B of fp32 / 8 B of half), widened to fp32
template <typename TIN, bool NT_LOAD = false>
__device__ __forceinline__ f32x4 in_load4(gin<TIN> *p) {
    if constexpr (sizeof(*p) == 4) {
        typedef const __attribute__((address_space(1))) f32x4 g4;
        if constexpr (NT_LOAD) return __builtin_nontemporal_load(reinterpret_cast<g4 *>(p));
        else return *reinterpret_cast<g4 *>(p);
    } else {
        typedef const __attribute__((address_space(1))) svdq_u32x2 g2;
        svdq_u32x2 w;
        if constexpr (NT_LOAD) {
            w = __builtin_nontemporal_load(reinterpret_cast<g2 *>(p));
        } else {
            w = *reinterpret_cast<g2 *>(p);
        }
        f32x4 o;
        o.x = SvdqIn<TIN>::cvt((uint16_t)(w.x & 0xffffu));
        o.y = SvdqIn<TIN>::cvt((uint16_t)(w.x >> 16));
        o.z = SvdqIn<TIN>::cvt((uint16_t)(w.y & 0xffffu));
        o.w = SvdqIn<TIN>::cvt((uint16_t)(w.y >> 16));
        return o;
    }
}

// two half elements packed in one 32-bit word (the first in the low half), widened to fp32
template <typename TIN>
__device__ __forceinline__ svdq_f32x2 in_widen2(uint32_t w) {
    svdq_f32x2 o;
    o.x = SvdqIn<TIN>::cvt((uint16_t)(w & 0xffffu));
    o.y = SvdqIn<TIN>::cvt((uint16_t)(w >> 16));
    return o;
}

// two consecutive elements (8 B of fp32 / 4 B of half), widened to fp32
template <typename TIN>
__device__ __forceinline__ svdq_f32x2 in_load2(gin<TIN> *p) {
    if constexpr (sizeof(*p) == 4) {
        return *reinterpret_cast<const __attribute__((address_space(1))) svdq_f32x2 *>(p);
    } else {
        return in_widen2<TIN>(*reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(p));
    }
}
