// The in-wave digit ranking of the radix sorts (sort.hip's sort_pass_kernel, rowsort.hip's row_sort_kernel) and the
// 256-digit block prefix they share with rowsort.hip's row_select_kernel.
#pragma once
#include "pcmx_common.h"

namespace pcmx {

// A wave's 256 LDS digit counters are read and advanced with relaxed wavefront-scope atomics (plain ds_read / ds_write
// that the compiler neither forwards nor drops): one wave's LDS accesses execute in program order.
__device__ __forceinline__ unsigned cnt_load(const unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void cnt_store(unsigned* p, unsigned v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// Stable rank of one row of 64 keys (one per lane) on the wave's 256 counters: the equal digits this wave has ranked
// before the row plus the equal digits in the row's lower lanes; the counter of every digit in the row advances by its
// count. Match-any: the valid lanes of this row that hold digit d. Per digit bit one ballot m and, with x = 0 / ~0 for
// a clear / set bit, peers &= ~(m ^ x), which is m or ~m (one three-input bit operation per half). An invalid lane's
// rank is meaningless and it advances nothing.
__device__ __forceinline__ unsigned rank_row(unsigned d, bool valid, unsigned* wave_counters) {
    const unsigned long long vmask = __ballot(valid);
    unsigned plo = (unsigned)vmask, phi = (unsigned)(vmask >> 32);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const unsigned x = (unsigned)((int)(d << (31 - b)) >> 31);
        const unsigned long long m = __ballot(x != 0u);
        plo &= ~((unsigned)m ^ x);
        phi &= ~((unsigned)(m >> 32) ^ x);
    }
    const unsigned below = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
    const unsigned total = (unsigned)(__popc(plo) + __popc(phi));
    unsigned* counter = wave_counters + d;
    const unsigned old = cnt_load(counter);  // every peer reads the counter before the last peer advances it
    if (valid && below + 1u == total) cnt_store(counter, old + total);
    return old + below;
}

// Exclusive prefix of v over threads 0 .. 255 (waves 0 .. 3). Every thread of the block calls it (one barrier inside);
// the result of threads 256 .. 511 is meaningless.
__device__ __forceinline__ unsigned block_excl256(unsigned v, unsigned* s_wsum) {
    const int lane = lane_id(), wave = threadIdx.x / kWave;
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned o = __shfl_up(inc, off, kWave);
        if (lane >= off) inc += o;
    }
    if (wave < 4 && lane == kWave - 1) s_wsum[wave] = inc;
    __syncthreads();
    unsigned add = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) add += w < wave ? s_wsum[w] : 0u;
    return inc - v + add;
}

}  // namespace pcmx
