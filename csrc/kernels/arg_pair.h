// The element of the arg-reductions (argreduce.hip): an (ordered key, position) pair packed into one 64-bit word,
// key in the high half and ~position in the low half, reduced with an unsigned max. "Better key wins, lower position
// wins a tie" is then one comparison; the operator is associative and commutative, so every tree shape, chunking and
// grid gives the same word. The key is radix_key.h's (-0.0 == +0.0, every NaN one key above +inf); for MIN it is
// flipped with the NaN key forced back to the top, so a NaN beats every number under both ops (torch's rule).
// The all-zero word is the identity: a real element never packs to it (its low half would be position 2^32 - 1), so
// it loses to everything, an all -inf or all INT32_MIN row included, and unpacks to position -1.
#pragma once
#include "pcmx_common.h"
#include "pcmx_hip.h"
#include "radix_key.h"

namespace pcmx {

typedef unsigned long long u64;

template <int KT, int OP>
__device__ __forceinline__ unsigned arg_key(unsigned bits) {
    unsigned k = to_key(bits, KT, 0u);
    if constexpr (OP == PCMX_OP_MIN) {
        k = ~k;
        // only the NaN key (all ones) flips to 0: no float packs to key 0 before the flip
        if constexpr (KT == PCMX_KEY_F32) k = k == 0u ? 0xffffffffu : k;
    }
    return k;
}

template <int KT, int OP>
__device__ __forceinline__ u64 arg_pack(unsigned bits, unsigned pos) {
    return ((u64)arg_key<KT, OP>(bits) << 32) | (u64)(unsigned)~pos;
}

__device__ __forceinline__ u64 arg_best(u64 a, u64 b) { return a > b ? a : b; }

// the position of a word; -1 for the identity
__device__ __forceinline__ int arg_pos(u64 w) { return (int)~(unsigned)w; }

// what a result made of no element shows as its value: -inf / INT32_MIN for MAX, +inf / INT32_MAX for MIN
template <int KT, int OP>
__device__ __forceinline__ unsigned arg_identity_bits() {
    if constexpr (KT == PCMX_KEY_F32) return OP == PCMX_OP_MIN ? 0x7f800000u : 0xff800000u;
    else return OP == PCMX_OP_MIN ? 0x7fffffffu : 0x80000000u;
}

__device__ __forceinline__ u64 arg_wave_best(u64 v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = arg_best(v, __shfl_xor(v, off, kWave));
    return v;
}

}  // namespace pcmx
