// Pieces shared by the kernels that describe a 32768-element tile by one bit per element (select.hip: keep bits,
// segreduce.hip and scanbykey.hip: run heads). The tile is 8 waves x 16 rows x 64 lanes x 4 elements; a lane holds its
// 64 elements' bits in one 64-bit word, bit 4r+j = element j of row r.
//  * every user: the tile shape, drop_past_n, rank_rows, fold_wave_totals;
//  * the two by-key kernels: the key tile load with the wave's left-neighbour key, head_bits from the loaded keys, the
//    value sources and load_vals, and fold_wave_tails, the cross-wave step of their segmented scan. The per-row wave
//    scan between load and fold is NOT here: each of the two kernels keeps its own text of it (see the comment there).
#pragma once
#include "pcmx_common.h"
#include "seg_ops.h"

namespace pcmx {
namespace tile_bits {

constexpr int kRows = 16, kWaves = 8;            // 16 rows of 4 elements per lane, 8 waves
constexpr int kWaveItems = kRows * 4 * kWave;    // 4096 contiguous elements per wave
constexpr int kTileElems = kWaves * kWaveItems;  // 32768

// One tile's keys in registers, plus the key just before this wave's 4096 (the neighbour of its first key).
struct TileKeys {
    u32x4 k[kRows];
    unsigned prev;
};

// Keys at or past n are never read: they load as 0, and the caller drops their head bits (drop_past_n, or the mask of
// scanbykey.hip's valid_bits).
__device__ __forceinline__ void load_keys(const unsigned* __restrict__ x, long long n, long long tile, TileKeys& t) {
    const int lane = lane_id(), wave = threadIdx.x / kWave;
    const unsigned* xt = x + tile * kTileElems;
    const unsigned off = (unsigned)(wave * kWaveItems + lane * 4);
    const long long before = tile * kTileElems + (long long)wave * kWaveItems - 1;  // wave-uniform
    // element 0 of the stream is a head: its neighbour is made to differ
    t.prev = before < 0 ? ~x[0] : (before < n ? x[before] : 0u);
    if ((tile + 1) * kTileElems <= n) {  // block-uniform: full tiles take the branch-free path
#pragma unroll
        for (int r = 0; r < kRows; ++r)
            t.k[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(xt + r * 256 + off));
        return;
    }
    const unsigned rem = (unsigned)(n - tile * kTileElems);  // the last, partial tile (once per launch)
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const unsigned e = off + r * 256;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (e + 0 < rem) v.x = xt[e + 0];
        if (e + 1 < rem) v.y = xt[e + 1];
        if (e + 2 < rem) v.z = xt[e + 2];
        if (e + 3 < rem) v.w = xt[e + 3];
        t.k[r] = v;
    }
}

// Head bits of the lane's 64 elements: bit 4r+j = element j of row r starts a run (differs from its left neighbour,
// compared as bit patterns: the lane's own row, the lane below by DPP, the previous row's lane 63 by v_readlane).
__device__ __forceinline__ unsigned long long head_bits(const TileKeys& t) {
    const int lane = lane_id();
    unsigned long long bits = 0ull;
    unsigned before = t.prev;  // wave-uniform: the key left of this row's first
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const u32x4 k = t.k[r];
        const unsigned below = from_lane_below(k.w);
        const unsigned p = lane == 0 ? before : below;
        const unsigned h = (k.x != p ? 1u : 0u) | (k.y != k.x ? 2u : 0u) | (k.z != k.y ? 4u : 0u) | (k.w != k.z ? 8u : 0u);
        bits |= (unsigned long long)h << (4 * r);
        before = (unsigned)__builtin_amdgcn_readlane((int)k.w, 63);
    }
    return bits;
}

// Where a by-key kernel's values come from: the constant 1 (run lengths, run positions), an int32 or a float32 stream.
enum { kSrcOne = 0, kSrcI32 = 1, kSrcF32 = 2 };

// The tile's values; elements at or past n are never read and take the op's identity (0 for the constant-1 source:
// the tile's closing aggregate must not count them).
template <int SRC, class T, int OP>
__device__ __forceinline__ void load_vals(const T* __restrict__ vals, long long n, long long tile,
                                          typename Vec4<T>::type (&v)[kRows]) {
    typedef typename Vec4<T>::type V;
    const int lane = lane_id(), wave = threadIdx.x / kWave;
    if constexpr (SRC == kSrcOne) {
        if ((tile + 1) * kTileElems <= n) {  // block-uniform
#pragma unroll
            for (int r = 0; r < kRows; ++r) v[r] = V{1, 1, 1, 1};
            return;
        }
        const long long base = tile * kTileElems + wave * kWaveItems + lane * 4;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const long long e = base + r * 256;
            v[r] = V{e + 0 < n ? 1 : 0, e + 1 < n ? 1 : 0, e + 2 < n ? 1 : 0, e + 3 < n ? 1 : 0};
        }
    } else {
        const T* vt = vals + tile * kTileElems;
        const unsigned off = (unsigned)(wave * kWaveItems + lane * 4);
        if ((tile + 1) * kTileElems <= n) {
#pragma unroll
            for (int r = 0; r < kRows; ++r) v[r] = __builtin_nontemporal_load(reinterpret_cast<const V*>(vt + r * 256 + off));
            return;
        }
        const unsigned rem = (unsigned)(n - tile * kTileElems);
        const T id = identity<T, OP>();
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const unsigned e = off + r * 256;
            V q = {id, id, id, id};
            if (e + 0 < rem) q.x = vt[e + 0];
            if (e + 1 < rem) q.y = vt[e + 1];
            if (e + 2 < rem) q.z = vt[e + 2];
            if (e + 3 < rem) q.w = vt[e + 3];
            v[r] = q;
        }
    }
}

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

// The wave tails of a by-key kernel's segmented scan (LDS, behind a barrier) -> wc, the open run's aggregate on entry to
// this wave, and closing, the one on leaving the tile. has_head(w): wave w holds a head.
template <class T, int OP, class HasHead>
__device__ __forceinline__ void fold_wave_tails(const T* s_tail, HasHead has_head, T& wc, T& closing) {
    const int wave = threadIdx.x / kWave;
    T open = identity<T, OP>(), mine = open;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w == wave) mine = open;
        const T tw = s_tail[w];
        open = has_head(w) ? tw : combine<T, OP>(open, tw);
    }
    wc = mine, closing = open;
}

}  // namespace tile_bits
}  // namespace pcmx
