// The radix key transform shared by sort.hip and topk.hip: raw 32-bit patterns <-> keys whose unsigned order is the
// wanted order. Top-k is defined as a prefix of the stable sort, so both must compare keys through this one pair.
#pragma once
#include "pcmx_common.h"
#include "pcmx_hip.h"

namespace pcmx {

// Raw bits -> key whose unsigned order is the wanted order (flip = ~0 for descending).
__device__ __forceinline__ unsigned to_key(unsigned b, int type, unsigned flip) {
    unsigned k = b;
    if (type == PCMX_KEY_F32) {
        const unsigned a = b & 0x7fffffffu;
        k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
        if (a == 0u) k = 0x80000000u;          // -0.0 == +0.0
        if (a > 0x7f800000u) k = 0xffffffffu;  // every NaN: one key, above +inf
    } else if (type == PCMX_KEY_I32) {
        k = b ^ 0x80000000u;
    }
    return k ^ flip;
}

__device__ __forceinline__ unsigned from_key(unsigned k, int type, unsigned flip) {
    k ^= flip;
    if (type == PCMX_KEY_F32) return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    if (type == PCMX_KEY_I32) return k ^ 0x80000000u;
    return k;
}

}  // namespace pcmx
