// lamellar_host.hpp — host helpers of the lamellar kernels shared between lamellar.hip, fused.hip and fused_step.hip
#pragma once

#include "lamellar_device.hpp"

#include <cassert>
#include <type_traits>

namespace mtd
{
constexpr unsigned int LAM_MAX_BLOCKS = 1024;

// validate a mtd_lamellar_set + box and expand it into the kernel-argument block
int fill_kargs(LamKArgs &k, const mtd_lamellar_set *set, const mtd_box *box);
unsigned int lam_cv_blocks(unsigned int N);
unsigned int lam_force_blocks(unsigned int N);
// hardware sine / cosine for this mode set? (the library setting AND phases inside the instructions' domain)
int lam_fast_trig(const LamKArgs &k);

// ---- run-time launch parameters -> template arguments -------------------------------------------------------------------------
// Each helper calls a generic lambda with the value as a TYPE (type_tag<S4>, std::integral_constant), so the lambda can name the
// kernel instantiation; nested, they replace the if / switch ladders around every launch.  All branches must return one type.
template<typename T> struct type_tag { using type = T; };

// (dtype, fast) -> f(type_tag<float4 | double4>{}, std::bool_constant<fast>{}); dtype is MTD_F32 or MTD_F64 (checked by the caller)
template<typename F> auto dispatch_s4_fast(int dtype, bool fast, F &&f)
    {
    if (dtype == MTD_F32)
        return fast ? f(type_tag<float4>{}, std::true_type{}) : f(type_tag<float4>{}, std::false_type{});
    return fast ? f(type_tag<double4>{}, std::true_type{}) : f(type_tag<double4>{}, std::false_type{});
    }

// a flag (ORTHO, COMM) -> f(std::bool_constant<b>{})
template<typename F> auto dispatch_bool(bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// a count 1 .. MAX (n_cv) -> f(std::integral_constant<int, n>{}).  The caller refuses every other count BEFORE it dispatches
// (each call site names its guard); one that slips through stops here instead of launching a neighbouring instantiation.
template<int MAX, typename F> auto dispatch_count(unsigned int n, F &&f)
    {
    assert(n >= 1 && n <= (unsigned int)MAX);
    if constexpr (MAX == 1)
        return f(std::integral_constant<int, 1>{});
    else
        return n >= (unsigned int)MAX ? f(std::integral_constant<int, MAX>{}) : dispatch_count<MAX - 1>(n, f);
    }
}
