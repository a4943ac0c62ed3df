// dispatch.hpp — run-time launch parameters -> template arguments (host only; shared by every unit that launches templated kernels)
// Each helper calls a generic lambda with the value as a TYPE (type_tag<S4>, std::integral_constant), so the lambda can name the
// kernel instantiation; nested, they replace the if / switch ladders around every launch.  All branches must return one type.
#pragma once

#include <hip/hip_runtime.h>

#include "mtd_abi.h"

#include <cassert>
#include <cstdint>
#include <type_traits>

namespace mtd
{
template<typename T> struct type_tag { using type = T; };

// dtype -> f(type_tag<float4 | double4>{}); dtype is MTD_F32 or MTD_F64 (checked by the caller)
template<typename F> auto dispatch_s4(int dtype, F &&f) { return dtype == MTD_F32 ? f(type_tag<float4>{}) : f(type_tag<double4>{}); }

// (dtype, fast) -> f(type_tag<float4 | double4>{}, std::bool_constant<fast>{}); dtype as above
template<typename F> auto dispatch_s4_fast(int dtype, bool fast, F &&f)
    {
    if (dtype == MTD_F32)
        return fast ? f(type_tag<float4>{}, std::true_type{}) : f(type_tag<float4>{}, std::false_type{});
    return fast ? f(type_tag<double4>{}, std::true_type{}) : f(type_tag<double4>{}, std::false_type{});
    }

// a flag (ORTHO, COMM, AVG) -> f(std::bool_constant<b>{})
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

// lmax of the Steinhardt variables -> f(std::integral_constant<int, LMAX>{}) with the smallest compiled bound 4 | 6 | 8 | 12 that
// holds it; the caller has refused lmax > 12
template<typename F> auto dispatch_lmax(unsigned int lmax, F &&f)
    {
    if (lmax <= 4) return f(std::integral_constant<int, 4>{});
    if (lmax <= 6) return f(std::integral_constant<int, 6>{});
    if (lmax <= 8) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, 12>{});
    }

// What every entry point that walks a neighbour list over an S4 array refuses before a device is touched: a missing array while there
// are particles (`pointers`: the caller's conjunction of the ones it needs), an unknown dtype, a scratch that is not 16-byte aligned, a
// virial array with a pitch below n_particles.  All four give MTD_ERR_INVALID_ARGUMENT, so their order among themselves cannot be seen
// from outside; WHERE the caller asks, before or after its own MTD_ERR_UNSUPPORTED refusals, can, and stays the caller's business.
inline int refuse_row_arrays(unsigned int n_particles, bool pointers, int dtype, const void *d_scratch, const void *d_virial,
                             unsigned int virial_pitch)
    {
    if (n_particles && !pointers) return MTD_ERR_INVALID_ARGUMENT;
    if (dtype != MTD_F32 && dtype != MTD_F64) return MTD_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)d_scratch & 15u) != 0) return MTD_ERR_INVALID_ARGUMENT;
    if (d_virial && virial_pitch < n_particles) return MTD_ERR_INVALID_ARGUMENT;
    return MTD_SUCCESS;
    }
}
