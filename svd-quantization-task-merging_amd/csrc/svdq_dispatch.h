// svdq_dispatch.h -- runtime value -> template argument, for the host-side launchers.
//
// Each dispatcher compares a runtime value with its compile-time cases and calls `f` with the matching case as a
// tag object: std::bool_constant / std::integral_constant (read the value with `constexpr auto X = tag;`), or
// SvdqType<T> for the input element type (`using TIN = typename decltype(tag)::type;`).  `f` is a generic lambda
// that returns whether it launched a kernel; the dispatcher hands that back, and false when no case matches.  A
// combination that must not be instantiated is excluded with `if constexpr (...) return false;` on the tags' values
// inside the lambda, so that each kernel's launch is written once:
//
//     const bool ok = svdq_dispatch_int<4, 8, 12, 16>(pl->ntp, [&](auto ntp_c) {
//         constexpr int NTP = ntp_c;
//         return svdq_dispatch_bool(pl->cfg.fp16 != 0, [&](auto f16_c) {
//             constexpr bool F16 = f16_c;
//             hipLaunchKernelGGL((kernel<NTP, F16>), ...);
//             return true;
//         });
//     });
//     return svdq_launch_status(ok, "kernel");
#pragma once

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <type_traits>

#include "../../include/svdq.h"

template <typename F>
static inline bool svdq_dispatch_bool(bool v, F &&f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}

template <int... CASES, typename F>
static inline bool svdq_dispatch_int(int v, F &&f) {
    return ((v == CASES && f(std::integral_constant<int, CASES>{})) || ...);
}

template <typename T> struct SvdqType { using type = T; };

// in_type: a plan's SVDQ_INPUT_* (svdq_plan_set_input_type admits no other value)
template <typename F>
static inline bool svdq_dispatch_input(int in_type, F &&f) {
    switch (in_type) {
        case SVDQ_INPUT_F32: return f(SvdqType<float>{});
        case SVDQ_INPUT_F16: return f(SvdqType<__half>{});
        case SVDQ_INPUT_BF16: return f(SvdqType<__hip_bfloat16>{});
        default: return false;
    }
}
