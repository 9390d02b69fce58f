// Pieces shared by the kernels that describe a 32768-element tile by one bit per element (select.hip: keep bits,
// segreduce.hip and scanbykey.hip: run heads). The tile is 8 waves x 16 rows x 64 lanes x 4 elements; a lane holds its
// 64 elements' bits in one 64-bit word, bit 4r+j = element j of row r.
#pragma once
#include "pcmx_common.h"

namespace pcmx {
namespace tile_bits {

constexpr int kRows = 16, kWaves = 8;            // 16 rows of 4 elements per lane, 8 waves
constexpr int kWaveItems = kRows * 4 * kWave;    // 4096 contiguous elements per wave
constexpr int kTileElems = kWaves * kWaveItems;  // 32768

// Clears the bits of the elements at or past n (only the last tile has any).
__device__ __forceinline__ unsigned long long drop_past_n(unsigned long long bits, long long n, long long tile) {
    if ((tile + 1) * kTileElems > n) {  // block-uniform
        const int lane = lane_id(), wave = threadIdx.x / kWave;
        const int rem = (int)(n - tile * kTileElems);  // elements of this tile below n (1 .. kTileElems - 1)
        const int base = wave * kWaveItems + lane * 4;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int left = rem - (base + r * 256);  // elements of this lane's row below n
            const unsigned ok = left >= 4 ? 0xfu : (left <= 0 ? 0u : ((1u << left) - 1u));
            bits &= ~((unsigned long long)(0xfu & ~ok) << (4 * r));
        }
    }
    return bits;
}

// Per row the integer wave prefix of the set bits, in input order (row, lane, element): lane_off[r] = set bits of the
// wave before this lane's row r; carry (wave-uniform) = the wave's total. No LDS: one ballot per element position,
// v_mbcnt of the four ballots for the lower lanes, scalar popcounts for the carry across rows.
__device__ __forceinline__ void rank_rows(unsigned long long bits, unsigned (&lane_off)[kRows], unsigned& carry) {
    carry = 0u;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const unsigned k = (unsigned)(bits >> (4 * r)) & 0xfu;
        const unsigned long long b0 = __ballot(k & 1u), b1 = __ballot(k & 2u), b2 = __ballot(k & 4u), b3 = __ballot(k & 8u);
        lane_off[r] = lanes_below(b3, lanes_below(b2, lanes_below(b1, lanes_below(b0, carry))));
        carry += (unsigned)(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3));
        // the offset is materialised here: left to the compiler it sinks to the staging loop and keeps all 64 ballots
        // (128 SGPRs) alive across the look-back
        asm volatile("" : "+v"(lane_off[r]));
    }
}

// The waves' totals (LDS, behind a barrier) -> the tile's total and the total of the waves below this one.
__device__ __forceinline__ void fold_wave_totals(const unsigned* s_wave_tot, unsigned& agg, unsigned& wexcl) {
    const int wave = threadIdx.x / kWave;
    agg = 0u, wexcl = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const unsigned c = s_wave_tot[w];
        wexcl += w < wave ? c : 0u;
        agg += c;
    }
}

}  // namespace tile_bits
}  // namespace pcmx
