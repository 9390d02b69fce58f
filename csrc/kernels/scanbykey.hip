// Scan-by-key (segmented prefix scan): the running sum, min or max of a value stream (int32, float32, or the constant 1
// for run positions) inside every run of equal neighbouring 32-bit keys, or inside the runs a byte stream of head
// flags marks. The sibling of segreduce.hip, which writes one aggregate per run; this one writes every element. No
// counterpart in the reference programs.
//
// Shared with segreduce.hip through tile_bits.h: the tile shape, the key and value loads, the head bits from the
// neighbouring key bits (the lane's own row, DPP wave_shr:1, v_readlane of the previous row's lane 63, one extra load per
// wave; the keys are read once) and the fold of the 8 wave tails; the operator is seg_ops.h's. Also the same, but
// written out in both files: the persistent schedule (one 512-thread block per CU, 32768-element tiles from an atomic
// ticket) and the per-row wave scan (a lane's 4 elements, 64 lanes by shuffles, 16 rows by a wave-uniform carry). What
// differs:
//  * Nothing is compacted, so no output position depends on another tile: there is NO look-back. No block ever waits
//    for another block: no spin loop, no status granule, no timeout word, and nothing to report afterwards.
//  * Values never travel between blocks while they run (a float carried through a look-back would make the result
//    depend on timing). Three launches on the caller's stream instead:
//      1. tile kernel: scans the tile with the identity as carry-in and writes EVERY output of the tile; records per
//         tile whether it has a head, its lead length (offset of the first head, or the tile's valid length) and its
//         closing aggregate (the elements after its last head, or the whole tile);
//      2. carry kernel: one block runs a segmented scan over the at most 65536 tile summaries in a fixed order:
//         carry[t] = the closings from the nearest earlier tile with a head (or tile 0) up to tile t - 1;
//      3. lead kernel: out[i] = op(carry[t], out[i]) for the lead of every tile t >= 1 (16-byte accesses, clipped
//         tail). A tile that starts with a head exits at once, so short runs touch almost nothing.
//    A float32 sum is op(carry, op(wave carry, in-wave prefix)): a fixed tree over exactly the elements of the run
//    prefix, so the same input gives the same bits on every call and a NaN or inf never leaves its run.
//  * The identity of a float sum is -0.0 inside the kernels (x + -0.0 == x for every x); the first element of a run
//    in exclusive mode gets +0.0 / +inf / -inf (int: 0 / INT_MAX / INT_MIN).
//  * When all keys are equal the lead kernel re-reads and re-writes the whole output: 20 instead of 12 bytes per
//    element. Accepted; a single-pass variant would have to carry {flag, has-head, value} through a look-back, which
//    is exactly associative only for ints and min / max.
// Measured at 2^28 int32 keys on one MI355X (profiles/r11_scanbykey/README.md), mean run 1 / 4 / 100 / 10^5 / all equal:
// float32 sum by key 0.63 / 0.63 / 0.62 / 0.97 / 1.02 ms (the torch composition, unique_consecutive + cumsum minus the
// gathered base: 8.9 / 5.9 / 4.9 / 4.8 / 4.7), run positions 0.50 / 0.51 / 0.50 / 0.87 / 0.92 ms (8.5 / 6.0 / 5.3 / 5.3 /
// 5.2); 1.26-1.30x the time of a copy of the same bytes while runs are shorter than a tile, 2.1x with all keys equal,
// where the lead kernel takes 0.39 of 1.0 ms. The carry kernel takes 0.020 ms.
#include "pcmx_common.h"
#include "pcmx_hip.h"
#include "seg_ops.h"
#include "tile_bits.h"

namespace {
using pcmx::combine;
using pcmx::device_cus;
using pcmx::from_lane_below;
using pcmx::identity;
using pcmx::kWave;
using pcmx::misaligned;
using pcmx::pad4;
using pcmx::u32x4;
using pcmx::Vec4;
using namespace pcmx::tile_bits;         // the tile shape
constexpr unsigned kHasHead = 1u << 31;  // tile_meta: the tile holds a run head; low bits: lead length

struct SbkWs {
    unsigned ticket;  // zeroed before every launch
    unsigned pad[3];
    // followed by unsigned tile_meta[tiles4], 4-byte tile_closing[tiles4], 4-byte tile_carry[tiles4]
    // (tiles4 = tiles padded to a multiple of 4); every entry below `tiles` is written before it is read
};

struct SideArrays {
    unsigned* tile_meta;  // lead length | kHasHead
    void* tile_closing;   // aggregate of the elements after the tile's last head (the whole tile when it has none)
    void* tile_carry;     // aggregate of the open run on entry to the tile
};

__host__ __device__ inline SideArrays side_arrays(void* ws, long long tiles) {
    SideArrays s;
    s.tile_meta = reinterpret_cast<unsigned*>(static_cast<SbkWs*>(ws) + 1);
    s.tile_closing = s.tile_meta + pad4(tiles);
    s.tile_carry = s.tile_meta + 2 * pad4(tiles);
    return s;
}

// Bit 4r+j of the result: element j of row r of this lane lies below n (all ones for a full tile). (The same bound
// as tile_bits.h's drop_past_n, built as a mask: switching to that form changes this kernel's generated code.)
__device__ __forceinline__ unsigned long long valid_bits(long long n, long long tile) {
    if ((tile + 1) * kTileElems <= n) return ~0ull;  // block-uniform
    const int lane = pcmx::lane_id(), wave = threadIdx.x / kWave;
    const int rem = (int)(n - tile * kTileElems);
    const int base = wave * kWaveItems + lane * 4;
    unsigned long long ok = 0ull;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int left = rem - (base + r * 256);
        const unsigned m = left >= 4 ? 0xfu : (left <= 0 ? 0u : ((1u << left) - 1u));
        ok |= (unsigned long long)m << (4 * r);
    }
    return ok;
}

// Head bits from the keys: bit 4r+j = element j of row r differs from its left neighbour (compared as bit patterns).
// Keys at or past n are never read. Element 0 of the stream is a head: its neighbour is made to differ.
__device__ __forceinline__ unsigned long long head_bits_from_keys(const unsigned* __restrict__ x, long long n, long long tile) {
    TileKeys t;  // dropped again: only the bits are kept
    load_keys(x, n, tile, t);
    return head_bits(t) & valid_bits(n, tile);
}

// Head bits from a byte stream of flags (4-byte aligned): a non-zero byte starts a run, and so does element 0.
__device__ __forceinline__ unsigned long long head_bits_from_flags(const unsigned char* __restrict__ f, long long n,
                                                                   long long tile) {
    const int lane = pcmx::lane_id(), wave = threadIdx.x / kWave;
    const unsigned char* ft = f + tile * kTileElems;
    const unsigned off = (unsigned)(wave * kWaveItems + lane * 4);
    unsigned long long bits = 0ull;
    if ((tile + 1) * kTileElems <= n) {  // block-uniform
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const unsigned w = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(ft + r * 256 + off));
            const unsigned h = ((w & 0xffu) ? 1u : 0u) | ((w & 0xff00u) ? 2u : 0u) | ((w & 0xff0000u) ? 4u : 0u) |
                               ((w & 0xff000000u) ? 8u : 0u);
            bits |= (unsigned long long)h << (4 * r);
        }
    } else {
        const unsigned rem = (unsigned)(n - tile * kTileElems);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const unsigned e = off + r * 256;
            unsigned h = 0u;
            if (e + 0 < rem && ft[e + 0]) h |= 1u;
            if (e + 1 < rem && ft[e + 1]) h |= 2u;
            if (e + 2 < rem && ft[e + 2]) h |= 4u;
            if (e + 3 < rem && ft[e + 3]) h |= 8u;
            bits |= (unsigned long long)h << (4 * r);
        }
    }
    if (tile == 0 && threadIdx.x == 0) bits |= 1ull;
    return bits;
}

// One tile: loads its head bits and values (all of them before the first store: out may be the value stream), scans
// it with the identity as carry-in, writes every output below n and the tile's summary. Returns with the next ticket
// in *s_next.
template <int FLAGS, int SRC, class T, int OP>
__device__ __forceinline__ void process_tile(const void* __restrict__ keys_or_heads, const T* vals, T* out, long long n,
                                             long long tile, int exclusive, SbkWs* ws, const SideArrays& side,
                                             unsigned* s_next, T* s_tail, int* s_first) {
    typedef typename Vec4<T>::type V;
    const int lane = pcmx::lane_id(), wave = threadIdx.x / kWave;
    const T id = identity<T, OP>();
    const T hv = pcmx::positive_zero_identity<T, OP>();  // what a run's first element gets in exclusive mode
    V v[kRows];
    unsigned long long bits;
    if constexpr (FLAGS)
        bits = head_bits_from_flags(static_cast<const unsigned char*>(keys_or_heads), n, tile);
    else
        bits = head_bits_from_keys(static_cast<const unsigned*>(keys_or_heads), n, tile);
    load_vals<SRC, T, OP>(vals, n, tile, v);
    if (threadIdx.x == 0) *s_next = atomicAdd(&ws->ticket, 1u);  // the ticket of this block's next tile

    // ---- segmented scan, wave-local, in input order: per row the lane's 4 elements serially, then the 64 lanes by
    //      shuffles; rcur carries the open run's aggregate from row to row. v[r] becomes the row's outputs, still
    //      without what the earlier waves hold of the run that is open at this wave's first element.
    //      (The row's wave scan up to `acc` is segreduce.hip's text; shared as a function it moves both kernels'
    //      registers and spills, see the comment there.)
    T rcur = id;
    int first = kWaveItems;  // wave-uniform: the wave's first head, in elements from the wave's start
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const unsigned k = (unsigned)(bits >> (4 * r)) & 0xfu;
        T a = v[r].x;
        a = (k & 2u) ? v[r].y : combine<T, OP>(a, v[r].y);
        a = (k & 4u) ? v[r].z : combine<T, OP>(a, v[r].z);
        a = (k & 8u) ? v[r].w : combine<T, OP>(a, v[r].w);  // the lane's tail: everything after its last head
        const unsigned long long fmask = __ballot(k != 0u);
        const unsigned long long upto = fmask & ((2ull << lane) - 1ull);  // lanes <= this one that hold a head
        const int d = upto ? lane - (63 - __builtin_clzll(upto)) : 64;     // distance to the nearest of them
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const T o = __shfl_up(a, off, kWave);
            if (lane >= off && d >= off) a = combine<T, OP>(o, a);
        }
        const T up = __shfl_up(a, 1, kWave);
        const T tail = __shfl(a, 63, kWave);
        const bool low_head = (fmask & ((1ull << lane) - 1ull)) != 0ull;  // a lower lane of this row holds a head
        T acc = lane == 0 ? rcur : (low_head ? up : combine<T, OP>(rcur, up));
        V o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool head = (k & (1u << j)) != 0u;
            const T before = head ? hv : acc;
            acc = head ? v[r][j] : combine<T, OP>(acc, v[r][j]);
            o[j] = exclusive ? before : acc;
        }
        v[r] = o;
        if (first == kWaveItems && fmask != 0ull) {  // wave-uniform
            const int l0 = __builtin_ctzll(fmask);
            const unsigned k0 = (unsigned)__builtin_amdgcn_readlane((int)k, l0);
            first = r * 256 + l0 * 4 + __builtin_ctz(k0);
        }
        rcur = fmask ? tail : combine<T, OP>(rcur, tail);
    }
    if (lane == 0) {
        s_tail[wave] = rcur;
        s_first[wave] = first;
    }
    __syncthreads();
    // ---- the open run's aggregate on entry to this wave and on leaving the tile, and the tile's first head
    T wc, closing;
    fold_wave_tails<T, OP>(s_tail, [&](int w) { return s_first[w] < kWaveItems; }, wc, closing);
    int lead = -1;  // the tile's first head: that of the lowest wave with one
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int fw = s_first[w];
        if (lead < 0 && fw < kWaveItems) lead = w * kWaveItems + fw;
    }
    const bool full = (tile + 1) * kTileElems <= n;  // block-uniform
    const int valid = full ? kTileElems : (int)(n - tile * kTileElems);
    if (threadIdx.x == 0) {
        side.tile_meta[tile] = lead >= 0 ? ((unsigned)lead | kHasHead) : (unsigned)valid;
        static_cast<T*>(side.tile_closing)[tile] = closing;
    }
    // ---- the elements before the wave's first head continue the run of the earlier waves
    if (wave != 0) {
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            if (r * 256 < first) {  // wave-uniform
                const int e = r * 256 + lane * 4;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e + j < first) v[r][j] = combine<T, OP>(wc, v[r][j]);
            }
        }
    }
    // ---- every output of the tile
    const int off = wave * kWaveItems + lane * 4;
    T* ot = out + tile * kTileElems;
    if (full) {
#pragma unroll
        for (int r = 0; r < kRows; ++r) __builtin_nontemporal_store(v[r], reinterpret_cast<V*>(ot + r * 256 + off));
    } else {
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int e = off + r * 256;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e + j < valid) ot[e + j] = v[r][j];
        }
    }
}

template <int FLAGS, int SRC, class T, int OP>
__global__ __launch_bounds__(kWaves * kWave) void scanbykey_tile_kernel(const void* __restrict__ keys_or_heads, const T* vals,
                                                                        T* out, long long n, long long ntiles,
                                                                        int exclusive, SbkWs* ws) {
    // two LDS slots for the broadcast values: a slot is rewritten two tiles later, with the other tile's barrier in
    // between
    __shared__ T s_tail[2][kWaves];
    __shared__ int s_first[2][kWaves];
    __shared__ unsigned s_tile[2];
    const SideArrays side = side_arrays(ws, ntiles);
    if (threadIdx.x == 0) s_tile[0] = atomicAdd(&ws->ticket, 1u);
    __syncthreads();
    for (int slot = 0;; slot ^= 1) {
        // (the tile number comes out of LDS: readfirstlane tells the compiler it is wave-uniform)
        const long long tile = __builtin_amdgcn_readfirstlane(s_tile[slot]);
        if (tile >= ntiles) break;
        process_tile<FLAGS, SRC, T, OP>(keys_or_heads, vals, out, n, tile, exclusive, ws, side, &s_tile[slot ^ 1],
                                        s_tail[slot], s_first[slot]);
    }
}

// carry[t] for every tile: a segmented scan over the tile summaries in one block, in a fixed order. Thread i owns the
// tiles [i * per, (i + 1) * per); a summary is the pair (has head, closing) under (f1, v1) . (f2, v2) = (f1 | f2,
// f2 ? v2 : v1 OP v2), whose neutral element is (0, identity).
constexpr int kCarryThreads = 512;
template <class T, int OP>
__global__ __launch_bounds__(kCarryThreads) void scanbykey_carry_kernel(const unsigned* __restrict__ tile_meta,
                                                                        const T* __restrict__ tile_closing,
                                                                        T* __restrict__ tile_carry, int ntiles) {
    __shared__ T s_v[kCarryThreads / kWave];
    __shared__ unsigned s_f[kCarryThreads / kWave];
    const int lane = pcmx::lane_id(), wave = threadIdx.x / kWave;
    const T id = identity<T, OP>();
    const int per = (ntiles + kCarryThreads - 1) / kCarryThreads;
    const int t0 = min((int)threadIdx.x * per, ntiles), t1 = min(t0 + per, ntiles);
    unsigned f = 0u;
    T v = id;
    for (int t = t0; t < t1; ++t) {  // this thread's tiles, in order
        const bool h = (tile_meta[t] & kHasHead) != 0u;
        v = h ? tile_closing[t] : combine<T, OP>(v, tile_closing[t]);
        f |= h ? 1u : 0u;
    }
    // inclusive scan of the pairs over the wave's 64 threads (seg_ops.h), then over the 8 waves
    pcmx::wave_scan_pairs<T, OP>(f, v);
    if (lane == kWave - 1) {
        s_v[wave] = v;
        s_f[wave] = f;
    }
    T ev;  // the pair of the threads below this one in the wave
    unsigned ef;
    pcmx::pair_of_lanes_below<T, OP>(f, v, ef, ev);
    __syncthreads();
    T pv = id;
    unsigned pf = 0u;
    for (int w = 0; w < wave; ++w) {  // the waves below this one
        pv = s_f[w] ? s_v[w] : combine<T, OP>(pv, s_v[w]);
        pf |= s_f[w];
    }
    T c = ef ? ev : combine<T, OP>(pv, ev);  // the open run's aggregate on entry to tile t0
    for (int t = t0; t < t1; ++t) {
        tile_carry[t] = c;
        const bool h = (tile_meta[t] & kHasHead) != 0u;
        c = h ? tile_closing[t] : combine<T, OP>(c, tile_closing[t]);
    }
}

// out[i] = carry[t] OP out[i] over the lead of tile t = blockIdx.x + 1: the elements before its first head, which
// continue the run that is open at the end of tile t - 1.
constexpr int kLeadThreads = 256;
template <class T, int OP>
__global__ __launch_bounds__(kLeadThreads) void scanbykey_lead_kernel(T* __restrict__ out, const unsigned* __restrict__ tile_meta,
                                                                      const T* __restrict__ tile_carry) {
    typedef typename Vec4<T>::type V;
    const long long tile = (long long)blockIdx.x + 1;
    const int len = (int)(tile_meta[tile] & ~kHasHead);  // <= the tile's valid length
    if (len == 0) return;
    const T c = tile_carry[tile];
    T* ot = out + tile * kTileElems;
    const int len4 = len >> 2;
    for (int i = threadIdx.x; i < len4; i += kLeadThreads) {
        V q = reinterpret_cast<const V*>(ot)[i];
        q.x = combine<T, OP>(c, q.x);
        q.y = combine<T, OP>(c, q.y);
        q.z = combine<T, OP>(c, q.z);
        q.w = combine<T, OP>(c, q.w);
        reinterpret_cast<V*>(ot)[i] = q;
    }
    const int i = len4 * 4 + (int)threadIdx.x;  // the clipped tail: at most 3 elements
    if (i < len) ot[i] = combine<T, OP>(c, ot[i]);
}

inline long long num_tiles(long long n) { return (n + kTileElems - 1) / kTileElems; }
inline size_t ws_bytes(long long tiles) { return sizeof(SbkWs) + (size_t)pad4(tiles) * 12; }

template <int FLAGS, int SRC, class T, int OP>
int launch_op(const void* keys_or_heads, const T* vals, T* out, long long n, int exclusive, void* workspace, hipStream_t s) {
    const long long tiles = num_tiles(n);
    PCMX_HIP_RET(hipMemsetAsync(workspace, 0, sizeof(SbkWs), s));  // the ticket
    const unsigned grid = (unsigned)(tiles < device_cus() ? tiles : device_cus());  // one resident block per CU
    scanbykey_tile_kernel<FLAGS, SRC, T, OP><<<grid, kWaves * kWave, 0, s>>>(keys_or_heads, vals, out, n, tiles, exclusive,
                                                                             static_cast<SbkWs*>(workspace));
    PCMX_HIP_RET(hipGetLastError());
    if (tiles > 1) {
        const SideArrays side = side_arrays(workspace, tiles);
        scanbykey_carry_kernel<T, OP><<<1, kCarryThreads, 0, s>>>(side.tile_meta, static_cast<const T*>(side.tile_closing),
                                                                 static_cast<T*>(side.tile_carry), (int)tiles);
        PCMX_HIP_RET(hipGetLastError());
        scanbykey_lead_kernel<T, OP><<<(unsigned)(tiles - 1), kLeadThreads, 0, s>>>(out, side.tile_meta,
                                                                                   static_cast<const T*>(side.tile_carry));
    }
    return (int)hipGetLastError();
}

template <int FLAGS, int SRC, class T>
int launch_mode(const void* keys_or_heads, const T* vals, T* out, long long n, int op, int exclusive, void* workspace,
                hipStream_t s) {
    switch (op) {
        case PCMX_OP_SUM:
            return launch_op<FLAGS, SRC, T, PCMX_OP_SUM>(keys_or_heads, vals, out, n, exclusive, workspace, s);
        case PCMX_OP_MIN:
            return launch_op<FLAGS, SRC, T, PCMX_OP_MIN>(keys_or_heads, vals, out, n, exclusive, workspace, s);
        default:
            return launch_op<FLAGS, SRC, T, PCMX_OP_MAX>(keys_or_heads, vals, out, n, exclusive, workspace, s);
    }
}

template <int SRC, class T>
int launch(const void* keys_or_heads, int head_mode, const T* vals, T* out, long long n, int op, int exclusive,
           void* workspace, hipStream_t s) {
    if (op < PCMX_OP_SUM || op > PCMX_OP_MAX) return PCMX_ERR_ARG;
    if (head_mode != PCMX_HEADS_FROM_KEYS && head_mode != PCMX_HEADS_FROM_FLAGS) return PCMX_ERR_ARG;
    if (n <= 0) return 0;
    if (n >= (1LL << 31)) return PCMX_ERR_ARG;  // lead lengths and the tile count of the carry kernel are 32-bit
    if (!keys_or_heads || misaligned(keys_or_heads, head_mode == PCMX_HEADS_FROM_FLAGS ? 3u : 15u)) return PCMX_ERR_ARG;
    if (!out || misaligned(out) || !workspace || misaligned(workspace)) return PCMX_ERR_ARG;
    if (SRC != kSrcOne && (!vals || misaligned(vals))) return PCMX_ERR_ARG;
    if constexpr (SRC == kSrcOne) {
        return launch_op<0, SRC, T, PCMX_OP_SUM>(keys_or_heads, vals, out, n, 1, workspace, s);
    } else {
        if (head_mode == PCMX_HEADS_FROM_FLAGS)
            return launch_mode<1, SRC, T>(keys_or_heads, vals, out, n, op, exclusive != 0, workspace, s);
        return launch_mode<0, SRC, T>(keys_or_heads, vals, out, n, op, exclusive != 0, workspace, s);
    }
}
}  // namespace

extern "C" long long pcmx_scanbykey_workspace_bytes(long long n) { return (long long)ws_bytes(n > 0 ? num_tiles(n) : 0); }

extern "C" int pcmx_scan_by_key_f32(const void* keys_or_heads, int head_mode, const float* vals, float* out, long long n,
                                    int op, int exclusive, void* workspace, hipStream_t s) {
    return launch<kSrcF32, float>(keys_or_heads, head_mode, vals, out, n, op, exclusive, workspace, s);
}

extern "C" int pcmx_scan_by_key_i32(const void* keys_or_heads, int head_mode, const int32_t* vals, int32_t* out,
                                    long long n, int op, int exclusive, void* workspace, hipStream_t s) {
    return launch<kSrcI32, int>(keys_or_heads, head_mode, vals, out, n, op, exclusive, workspace, s);
}

extern "C" int pcmx_run_positions_b32(const void* keys, int32_t* out, long long n, void* workspace, hipStream_t s) {
    return launch<kSrcOne, int>(keys, PCMX_HEADS_FROM_KEYS, nullptr, out, n, PCMX_OP_SUM, 1, workspace, s);
}
