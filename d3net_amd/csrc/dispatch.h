// dispatch.h -- host-side launch helpers: a kernel's dynamic-LDS limit, and run-time flags / counts as template arguments.
// A launch site names its kernel once, inside a generic lambda, with the argument list in plain code.  The selectors are
// inlined into their caller (no tables of function pointers, no std::function).  A selector instantiates the lambda for EVERY
// combination it lists: exclude what must not exist with `if constexpr` inside the lambda.
#pragma once
#include <type_traits>
#include "common.h"

// allow `bytes` of dynamic LDS for Kernel: set on the first call per device (and on every call while the device cannot be
// told).  The flag is written AFTER the attribute is set: the library is called from more than one host thread (the
// clustering helper, the input prefetch), and a thread that finds the flag set launches, or asks for the occupancy, at once.
// Returns 0 or the hipError_t.
template <auto Kernel>
static inline int d3_allow_lds(int bytes) {
    static bool done[64] = {false};
    int dev = 0;
    const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;
    if (known && done[dev]) return 0;
    const hipError_t e = hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && known) done[dev] = true;
    return (int)e;
}

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): 2^n instantiations of f
template <typename F, typename... B>
static __forceinline__ int d3_with_bools(F &&f, bool b0, B... rest) {
    if constexpr (sizeof...(rest) == 0) return b0 ? f(std::true_type{}) : f(std::false_type{});
    else return b0 ? d3_with_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
                   : d3_with_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// f(std::integral_constant<int, V>{}) for the V of the list that equals v; D3_ERR_ARG when none does (a site that wants a
// default clamps v to the list first)
template <int... Vs, typename F>
static __forceinline__ int d3_with_value(int v, F &&f) {
    int rc = D3_ERR_ARG;
    (void)((v == Vs ? (rc = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
    return rc;
}
