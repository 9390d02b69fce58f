// Single-pass stream compaction (select / nonzero / predicate select) on the scan's decoupled look-back.
// Ancestor: the pixel-stack frontier of the region programs (ref 2-mpi-region-growing/region.c:493-533 pushes the
// pixels that pass a test onto a stack); this is that "keep what passes, in order, and count it" as one kernel.
//
// Same protocol as scan.hip's persistent schedule (scan_persistent_kernel / finish_tile), with two differences: the
// granule value is the tile's KEPT COUNT as u32 (the look-back sums integers, so every output is exact), and the
// tile ends in a compacted store to out[p .. p+cnt) instead of a dense one.
//  * One 512-thread block per CU takes 128-KiB tiles (32768 elements) from the atomic ticket in the workspace and
//    keeps the next tile's loads in flight while wave 0 looks back.
//  * Three front ends share everything after the per-element keep bit: a byte mask with a 4-byte payload moved as
//    bits (select_b32), a byte mask alone (select_index, out[j] = i), and an IEEE comparison of an f32 payload with a
//    threshold (select_if, values or indices, no mask materialised).
//  * Lane offsets are an integer wave prefix with no LDS round trip: a row is 4 elements per lane, one ballot per
//    element position, and v_mbcnt of the four ballots counts the kept elements of the lower lanes. Row totals are
//    scalar popcounts, so the carry across the 16 rows never leaves the scalar unit.
//  * Store path: each wave stages its survivors in its 16-KiB slice of LDS (128 of the 160 KiB) at their wave-local
//    positions, then streams [0, count) out coalesced. The direct scattered store from registers was built first and
//    measured slower once half the elements are kept (0.48 -> 0.38 ms at keep 0.5, 0.63 -> 0.45 at 1.0 for 2^28 f32;
//    equal below; profiles/r7_select/store_path_ab.txt).
//  * Hand-off, workspace zeroing, bounded spins and the give-up report are lookback.h's: 8-byte {flag, count} granules,
//    one agent-scope relaxed atomic store, agent-scope relaxed polls, hipMemsetAsync before every launch, and a
//    look-back that gives up sets ws->timeout and ORs 1 into the caller's sticky error word.
#include "lookback.h"
#include "pcmx_common.h"
#include "pcmx_hip.h"
#include "tile_bits.h"

namespace {
using pcmx::at;
using pcmx::device_cus;
using pcmx::kFlagAgg;
using pcmx::kFlagIncl;
using pcmx::kWave;
using pcmx::u32x4;
using namespace pcmx::tile_bits;  // the tile shape (128 KiB of payload) and the per-element bit helpers
enum { kModeMask = 0, kModeIndex = 1, kModePred = 2 };

typedef pcmx::LookbackHeader SelectWs;  // followed by unsigned long long status[num_tiles]
typedef pcmx::GranuleU32 Granule;       // the tile's kept count

// One tile's inputs in registers: payload rows (kModeMask, kModePred) and/or the rows' four flag bytes.
template <int MODE>
struct TileRegs {
    u32x4 v[MODE == kModeIndex ? 1 : kRows];
    unsigned m[MODE == kModePred ? 1 : kRows];
};

// Elements and flag bytes at or past n are never read.
template <int MODE>
__device__ __forceinline__ void load_tile(const unsigned* __restrict__ x, const unsigned char* __restrict__ mask,
                                          long long n, long long tile, TileRegs<MODE>& t) {
    const int lane = pcmx::lane_id(), wave = threadIdx.x / kWave;
    // a block-uniform tile base and a 32-bit offset inside the tile: one scalar base + one VGPR offset per load
    const unsigned* xt = x + tile * kTileElems;
    const unsigned char* mt = mask + tile * kTileElems;
    const unsigned off = (unsigned)(wave * kWaveItems + lane * 4);
    if ((tile + 1) * kTileElems <= n) {  // block-uniform: full tiles take the branch-free path
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            // the row stride goes into the scalar base, the lane's offset stays one VGPR for all 16 rows
            if (MODE != kModeIndex) t.v[r] = __builtin_nontemporal_load(at<u32x4>(xt + r * 256, off * 4u));
            if (MODE != kModePred) t.m[r] = __builtin_nontemporal_load(at<unsigned>(mt + r * 256, off));
        }
        return;
    }
    // the last, partial tile (once per launch) keeps the full tile's register shape: rows wholly below n load as
    // usual, every other lane re-reads the last whole row (its data is dropped by keep_bits' bound), and the one
    // lane that owns the ragged row takes its 1..3 elements from three clamped, block-uniform loads. Nothing at
    // or past n is read.
    const unsigned rem = (unsigned)(n - tile * kTileElems);  // elements of this tile below n: 1 .. kTileElems - 1
    const unsigned part = rem & ~3u, last = rem - 1u;        // in-tile start of the ragged row, index of element n - 1
    const unsigned q0 = min(part, last), q1 = min(part + 1u, last), q2 = min(part + 2u, last);
    u32x4 pv = {0u, 0u, 0u, 0u};
    unsigned pm = 0u;
    if (MODE != kModeIndex) pv.x = xt[q0], pv.y = xt[q1], pv.z = xt[q2];
    if (MODE != kModePred) pm = (unsigned)mt[q0] | (unsigned)mt[q1] << 8 | (unsigned)mt[q2] << 16;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const unsigned e = off + r * 256;
        if (MODE != kModeIndex) t.v[r] = pv;
        if (MODE != kModePred) t.m[r] = pm;
        if (rem >= 4u) {  // block-uniform: a whole row exists
            const unsigned ev = min(e, part - 4u);
            if (MODE != kModeIndex) {
                const u32x4 v = __builtin_nontemporal_load(at<u32x4>(xt, ev * 4u));
                if (e != part) t.v[r] = v;
            }
            if (MODE != kModePred) {
                const unsigned m = __builtin_nontemporal_load(at<unsigned>(mt, ev));
                if (e != part) t.m[r] = m;
            }
        }
    }
}

// IEEE comparison x OP t; NaN (either side) is kept only by ne.
template <int OP>
__device__ __forceinline__ bool pred(unsigned bits, float t) {
    const float x = __uint_as_float(bits);
    switch (OP) {
        case PCMX_CMP_GT: return x > t;
        case PCMX_CMP_GE: return x >= t;
        case PCMX_CMP_LT: return x < t;
        case PCMX_CMP_LE: return x <= t;
        case PCMX_CMP_EQ: return x == t;
        default: return x != t;
    }
}

// Keep bits of the lane's 64 elements: bit 4r+j = element j of row r.
template <int OP>
__device__ __forceinline__ unsigned long long pred_bits(const u32x4 (&v)[kRows], float thr) {
    unsigned long long bits = 0ull;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const unsigned k = (pred<OP>(v[r].x, thr) ? 1u : 0u) | (pred<OP>(v[r].y, thr) ? 2u : 0u) |
                           (pred<OP>(v[r].z, thr) ? 4u : 0u) | (pred<OP>(v[r].w, thr) ? 8u : 0u);
        bits |= (unsigned long long)k << (4 * r);
    }
    return bits;
}

template <int MODE>
__device__ __forceinline__ unsigned long long keep_bits(const TileRegs<MODE>& t, int op, float thr, long long n,
                                                        long long tile) {
    unsigned long long bits = 0ull;
    if constexpr (MODE == kModePred) {
        switch (op) {  // kernel-uniform
            case PCMX_CMP_GT: bits = pred_bits<PCMX_CMP_GT>(t.v, thr); break;
            case PCMX_CMP_GE: bits = pred_bits<PCMX_CMP_GE>(t.v, thr); break;
            case PCMX_CMP_LT: bits = pred_bits<PCMX_CMP_LT>(t.v, thr); break;
            case PCMX_CMP_LE: bits = pred_bits<PCMX_CMP_LE>(t.v, thr); break;
            case PCMX_CMP_EQ: bits = pred_bits<PCMX_CMP_EQ>(t.v, thr); break;
            default: bits = pred_bits<PCMX_CMP_NE>(t.v, thr); break;
        }
    } else {
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const unsigned m = t.m[r];
            const unsigned k = ((m & 0xffu) ? 1u : 0u) | ((m & 0xff00u) ? 2u : 0u) | ((m & 0xff0000u) ? 4u : 0u) |
                               ((m & 0xff000000u) ? 8u : 0u);
            bits |= (unsigned long long)k << (4 * r);
        }
    }
    return drop_past_n(bits, n, tile);
}

// Counts tile `tile` held in t, publishes its count, issues the loads of `next` into tn, looks back, stores.
template <int MODE, bool kIndexOut>
__device__ __forceinline__ void finish_tile(const unsigned* __restrict__ x, const unsigned char* __restrict__ mask,
                                            unsigned* __restrict__ out, long long n, long long tile, TileRegs<MODE>& t,
                                            long long next, TileRegs<MODE>& tn, long long ntiles, int op, float thr,
                                            long long* count_dev, SelectWs* ws, unsigned* err_flag,
                                            unsigned* s_wave_tot, unsigned* s_prefix, unsigned* s_next, unsigned* s_stage) {
    unsigned long long* status = reinterpret_cast<unsigned long long*>(ws + 1);
    const int lane = pcmx::lane_id(), wave = threadIdx.x / kWave;
    // ---- keep bits, then per row the integer wave prefix of the kept elements (input order: row, lane, element)
    const unsigned long long bits = keep_bits<MODE>(t, op, thr, n, tile);
    unsigned carry;  // wave-uniform: the wave's kept elements
    unsigned lane_off[kRows];
    rank_rows(bits, lane_off, carry);
    if (lane == 0) s_wave_tot[wave] = carry;
    __syncthreads();
    unsigned agg, wexcl;
    fold_wave_totals(s_wave_tot, agg, wexcl);
    if (threadIdx.x == 0)
        __hip_atomic_store(&status[tile], Granule::pack(tile == 0 ? kFlagIncl : kFlagAgg, agg), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    // ---- the next tile's loads go out now and overlap the look-back below; in value mode this tile's payload stays
    //      in t until it is staged
    if (next < ntiles) load_tile<MODE>(x, mask, n, next, tn);
    // ---- the ticket for the tile after `next`, taken before this tile's stores (as in the scan)
    unsigned ticket = 0u;
    if (threadIdx.x == 0) ticket = atomicAdd(&ws->ticket, 1u);

    // ---- wave 0: decoupled look-back over the predecessors' {flag, count} granules
    if (wave == 0) {
        // (after a give-up the partial prefix is <= the true one: the stores stay inside out)
        const unsigned prefix = pcmx::lookback_publish<Granule>(ws, status, tile, agg, err_flag);
        if (lane == 0) {
            *s_prefix = prefix;
            if (tile == ntiles - 1) *count_dev = (long long)(prefix + agg);  // the owner of the last tile
        }
    }
    if (threadIdx.x == 0) *s_next = ticket;
    __syncthreads();
    if (agg == 0u) return;  // block-uniform: nothing kept in this tile

    // ---- stage: each wave writes its kept elements to its own LDS slice at their wave-local positions, in input order
    // (the keep bits are re-read from their two registers here: an opaque copy, or the compiler keeps all 64 of the
    // count phase's extracted bits alive in a VGPR each across the look-back)
    unsigned bits_lo = (unsigned)bits, bits_hi = (unsigned)(bits >> 32);
    asm volatile("" : "+v"(bits_lo), "+v"(bits_hi));
    const unsigned long long sbits = ((unsigned long long)bits_hi << 32) | bits_lo;
    const unsigned first = (unsigned)(tile * kTileElems) + (unsigned)(wave * kWaveItems + lane * 4);  // n < 2^31
    unsigned* st = s_stage + wave * kWaveItems;  // lane_off[r] + 3 < the wave's count <= kWaveItems
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const unsigned k = (unsigned)(sbits >> (4 * r)) & 0xfu;
        unsigned pos = lane_off[r];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (k & (1u << j)) {
                st[pos] = kIndexOut ? first + (unsigned)(r * 256 + j) : t.v[MODE == kModeIndex ? 0 : r][j];
                ++pos;
            }
        }
    }
    // ---- stream: the wave's [0, count) goes out coalesced to out[p + wave offset ...). A wave reads only its own
    // slice; the barrier orders its lanes' LDS writes before the other lanes' reads, and the next tile's staging by
    // this wave follows these reads in program order.
    __syncthreads();
    // block prefix + wave offset are wave-uniform: a scalar base, the lane's 32-bit position as the only VGPR address
    unsigned* dst = out + __builtin_amdgcn_readfirstlane(*s_prefix + wexcl);
    const unsigned wcnt = __builtin_amdgcn_readfirstlane(carry);
#pragma unroll 4
    for (unsigned i = lane; i < wcnt; i += kWave) dst[i] = st[i];
}

template <int MODE, bool kIndexOut>
__global__ __launch_bounds__(kWaves * kWave) void select_kernel(const unsigned* __restrict__ x,
                                                                const unsigned char* __restrict__ mask,
                                                                unsigned* __restrict__ out, long long n, long long ntiles,
                                                                int op, float thr, long long* count_dev, SelectWs* ws,
                                                                unsigned* err_flag) {
    // two LDS slots so consecutive tiles never race on the broadcast values: a slot is rewritten two tiles later,
    // with the other tile's two barriers in between
    __shared__ unsigned s_wave_tot[2][kWaves];
    __shared__ unsigned s_prefix[2];
    __shared__ unsigned s_tile[2];
    __shared__ unsigned s_stage[kTileElems];  // 128 KiB: wave w stages its survivors in [w * 4096, (w + 1) * 4096)
    TileRegs<MODE> ta_regs, tb_regs;
    if (threadIdx.x == 0) {
        s_tile[0] = atomicAdd(&ws->ticket, 1u);
        s_tile[1] = atomicAdd(&ws->ticket, 1u);
    }
    __syncthreads();
    // (tile numbers come out of LDS: readfirstlane tells the compiler they are wave-uniform, so tile bases stay scalar)
    long long ta = __builtin_amdgcn_readfirstlane(s_tile[0]), tb = __builtin_amdgcn_readfirstlane(s_tile[1]);
    if (ta >= ntiles) return;
    load_tile<MODE>(x, mask, n, ta, ta_regs);
    // unrolled by two so both register buffers are statically named (every exit is block-uniform); each finish_tile
    // takes the ticket two tiles ahead and publishes it in s_tile[slot] by its last barrier
    while (true) {
        finish_tile<MODE, kIndexOut>(x, mask, out, n, ta, ta_regs, tb, tb_regs, ntiles, op, thr, count_dev, ws, err_flag,
                                     s_wave_tot[0], &s_prefix[0], &s_tile[0], s_stage);
        if (tb >= ntiles) break;
        ta = __builtin_amdgcn_readfirstlane(s_tile[0]);
        finish_tile<MODE, kIndexOut>(x, mask, out, n, tb, tb_regs, ta, ta_regs, ntiles, op, thr, count_dev, ws, err_flag,
                                     s_wave_tot[1], &s_prefix[1], &s_tile[1], s_stage);
        if (ta >= ntiles) break;
        tb = __builtin_amdgcn_readfirstlane(s_tile[1]);
    }
}

inline long long num_tiles(long long n) { return (n + kTileElems - 1) / kTileElems; }
// header + one granule per tile, padded to a multiple of 16 bytes (the whole block is zeroed before every launch)
inline size_t ws_bytes(long long tiles) { return sizeof(SelectWs) + (size_t)pcmx::pad2(tiles) * 8; }

template <int MODE, bool kIndexOut>
int launch(const void* x, const void* mask, void* out, long long n, int op, float thr, long long* count_dev,
           void* workspace, unsigned* err_flag, hipStream_t s) {
    if (!count_dev) return PCMX_ERR_ARG;
    if (n <= 0) {
        PCMX_HIP_RET(hipMemsetAsync(count_dev, 0, sizeof(long long), s));
        return 0;
    }
    if (n >= (1LL << 31)) return PCMX_ERR_ARG;  // indices and granule counts are 32-bit
    if (MODE != kModeIndex && (!x || (((uintptr_t)x) & 15u))) return PCMX_ERR_ARG;
    if (MODE != kModePred && (!mask || (((uintptr_t)mask) & 3u))) return PCMX_ERR_ARG;
    if (!out || (((uintptr_t)out) & 15u) || !workspace) return PCMX_ERR_ARG;
    const long long tiles = num_tiles(n);
    PCMX_HIP_RET(hipMemsetAsync(workspace, 0, ws_bytes(tiles), s));
    const unsigned grid = (unsigned)(tiles < device_cus() ? tiles : device_cus());  // one resident block per CU
    select_kernel<MODE, kIndexOut><<<grid, kWaves * kWave, 0, s>>>(
        static_cast<const unsigned*>(x), static_cast<const unsigned char*>(mask), static_cast<unsigned*>(out), n, tiles, op,
        thr, count_dev, reinterpret_cast<SelectWs*>(workspace), err_flag);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" long long pcmx_select_workspace_bytes(long long n) { return (long long)ws_bytes(n > 0 ? num_tiles(n) : 0); }

extern "C" int pcmx_select_b32(const void* x, const unsigned char* mask, void* out, long long n, long long* count_dev,
                               void* workspace, unsigned* err_flag, hipStream_t s) {
    return launch<kModeMask, false>(x, mask, out, n, 0, 0.f, count_dev, workspace, err_flag, s);
}

extern "C" int pcmx_select_index(const unsigned char* mask, int* out_idx, long long n, long long* count_dev, void* workspace,
                                 unsigned* err_flag, hipStream_t s) {
    return launch<kModeIndex, true>(nullptr, mask, out_idx, n, 0, 0.f, count_dev, workspace, err_flag, s);
}

extern "C" int pcmx_select_if_f32(const float* x, int op, float threshold, void* out_or_idx, int want_index, long long n,
                                  long long* count_dev, void* workspace, unsigned* err_flag, hipStream_t s) {
    if (op < PCMX_CMP_GT || op > PCMX_CMP_NE) return PCMX_ERR_ARG;
    return want_index ? launch<kModePred, true>(x, nullptr, out_or_idx, n, op, threshold, count_dev, workspace, err_flag, s)
                      : launch<kModePred, false>(x, nullptr, out_or_idx, n, op, threshold, count_dev, workspace, err_flag, s);
}
