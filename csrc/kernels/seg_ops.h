// The operator of the segmented family (segreduce.hip, scanbykey.hip, ragged.hip; axis.hip takes combine and Vec4,
// reduce.hip Vec4): sum, min or max over float32 / int32, its identity, and the segmented-scan operator over
// (flag, value) pairs built from it.
#pragma once
#include <limits.h>

#include <type_traits>

#include "pcmx_common.h"
#include "pcmx_hip.h"

namespace pcmx {

// 4 elements of T as one native vector (f32x4 / i32x4 of pcmx_common.h are the same types)
template <class T>
struct Vec4 {
    typedef T type __attribute__((ext_vector_type(4)));
};

// The identity inside the kernels; a float sum starts from -0.0 (x + -0.0 == x for every x, -0.0 included).
template <class T, int OP>
__device__ __forceinline__ T identity() {
    if constexpr (std::is_same<T, float>::value)
        return OP == PCMX_OP_SUM ? -0.0f : (OP == PCMX_OP_MIN ? __builtin_inff() : -__builtin_inff());
    else
        return OP == PCMX_OP_SUM ? 0 : (OP == PCMX_OP_MIN ? INT_MAX : INT_MIN);
}

// What a result made of no element shows (the first element of a run in an exclusive scan, an empty segment): the
// identity, with +0.0 for a float sum.
template <class T, int OP>
__device__ __forceinline__ T positive_zero_identity() {
    if constexpr (std::is_same<T, float>::value && OP == PCMX_OP_SUM)
        return 0.0f;
    else
        return identity<T, OP>();
}

// a OP b; int32 sums wrap, float min / max hand on a NaN operand
template <class T, int OP>
__device__ __forceinline__ T combine(T a, T b) {
    if constexpr (std::is_same<T, float>::value) {
        if constexpr (OP == PCMX_OP_SUM) return a + b;
        if constexpr (OP == PCMX_OP_MIN) return (a < b || a != a) ? a : b;
        return (a > b || a != a) ? a : b;
    } else {
        if constexpr (OP == PCMX_OP_SUM) return (int)((unsigned)a + (unsigned)b);
        if constexpr (OP == PCMX_OP_MIN) return a < b ? a : b;
        return a > b ? a : b;
    }
}

template <class T>
__device__ __forceinline__ T combine_rt(int op, T a, T b) {  // kernel-uniform op
    return op == PCMX_OP_SUM ? combine<T, PCMX_OP_SUM>(a, b)
                             : (op == PCMX_OP_MIN ? combine<T, PCMX_OP_MIN>(a, b) : combine<T, PCMX_OP_MAX>(a, b));
}
template <class T>
__device__ __forceinline__ T identity_rt(int op) {
    return op == PCMX_OP_SUM ? identity<T, PCMX_OP_SUM>()
                             : (op == PCMX_OP_MIN ? identity<T, PCMX_OP_MIN>() : identity<T, PCMX_OP_MAX>());
}

// A segment summary is the pair (holds a segment border, aggregate behind the last border) under
// (f1, v1) . (f2, v2) = (f1 | f2, f2 ? v2 : v1 OP v2), whose neutral element is (0, identity).
// Inclusive scan of the lanes' pairs over the wave, in lane order.
template <class T, int OP>
__device__ __forceinline__ void wave_scan_pairs(unsigned& flag, T& value) {
    const int lane = lane_id();
    unsigned f = flag;  // local copies: the conditional updates below are on values, not through the references
    T v = value;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const T ov = __shfl_up(v, off, kWave);
        const unsigned of = __shfl_up(f, off, kWave);
        if (lane >= off) {
            v = f ? v : combine<T, OP>(ov, v);
            f |= of;
        }
    }
    flag = f, value = v;
}

// After wave_scan_pairs: the pair of the lanes below this one (the neutral element in lane 0).
template <class T, int OP>
__device__ __forceinline__ void pair_of_lanes_below(unsigned f, T v, unsigned& flag_below, T& value_below) {
    T ev = __shfl_up(v, 1, kWave);
    unsigned ef = __shfl_up(f, 1, kWave);
    if (lane_id() == 0) {
        ev = identity<T, OP>();
        ef = 0u;
    }
    flag_below = ef, value_below = ev;
}

}  // namespace pcmx
