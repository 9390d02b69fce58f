// Single-pass run-length encode / reduce-by-key on the scan's decoupled look-back: collapses runs of equal neighbouring
// 32-bit keys and reduces a value stream (the constant 1, int32 or float32; sum, min or max) per run. No counterpart
// in the reference programs; the by-key member of the scan / select / sort family.
//
// Shared with select.hip: the persistent schedule (one 512-thread block per CU, 32768-key tiles from the atomic
// ticket), the look-back (lookback.h: 8-byte {flag, count} granules, bounded spins, ws->timeout plus the caller's
// sticky error word, the header that pcmx_scan_check reads), hipMemsetAsync of the workspace per launch, and the
// ballot / v_mbcnt lane offsets (tile_bits.h). The keep bit is the run head, key[i] != key[i-1] compared
// as bit patterns; the look-back carries only the integer count of heads, so every output position is exact.
// Shared with scanbykey.hip through tile_bits.h: the key and value loads of a tile, the head bits and the fold of the
// wave tails; the operator (identity, combine) is seg_ops.h's.
// What differs:
//  * The neighbour key comes from the lane's own row (4 keys), the lane below (DPP wave_shr:1), the previous row's
//    lane 63 (v_readlane) or, for a wave's first key, one extra load per wave; the keys are read once.
//  * Values never enter the granules: a float carried through the look-back would make the result depend on which
//    predecessor happened to be inclusive. The tile reduces its values with a segmented scan in a fixed order (4
//    elements per lane, 64 lanes per row by shuffles, 16 rows by v_readlane, 8 wave tails through LDS), overlapped
//    with wave 0's look-back. A run's in-tile aggregate is emitted by the head that closes it (or by the end of the
//    tile) into LDS at the run's in-tile rank h, and the tile streams [0, heads) out coalesced to out[P + h], P the
//    exclusive head count from the look-back. Run keys and start offsets go through the same LDS stage, one pass each.
//  * Runs that cross tiles: each tile records the aggregate of the elements before its first head (its lead), its P
//    and its head count in side arrays of the workspace. A second kernel on the same stream, one wave per tile that
//    begins a chain of leads, folds the leads of the tiles the run crosses in ascending order, 64 tiles per step with
//    a fixed butterfly, and combines the total into out[P - 1]. No float atomics anywhere: the same input gives the
//    same bits whatever the timing, and integer results are exact (int32 sums wrap).
//  * float min / max propagate a NaN value (like torch's amin / amax); which NaN's payload comes out is unspecified.
//  * No second tile in flight: keys (64 VGPRs), values (64) and the lane offsets (16) leave no room for select.hip's
//    second register buffer in the 256 VGPRs of a 512-thread block (built first with it: 850 B per lane of scratch).
//    A tile's keys and values are loaded together at its top; the look-back of wave 0 overlaps the other waves'
//    segmented scan instead.
// Measured at 2^28 int32 keys on one MI355X (profiles/r9_segreduce/README.md), mean run 1 / 4 / 100 / 10^5 / all equal:
// run-length encode 0.94 / 0.70 / 0.60 / 0.53 / 0.59 ms (torch.unique_consecutive with counts: 1.24 / 0.75 / 0.64 /
// 0.60 / 0.60), float32 sum by key 1.02 / 0.87 / 0.77 / 0.74 / 0.77 ms (unique_consecutive + index_add_: 3.5 to 79 ms);
// 1.5-3.5x the time of a copy of the same bytes (not bandwidth-bound). The fix-up kernel takes 0.106 ms for a run that
// crosses all 8192 tiles.
#include "lookback.h"
#include "pcmx_common.h"
#include "pcmx_hip.h"
#include "seg_ops.h"
#include "tile_bits.h"

namespace {
using pcmx::combine;
using pcmx::combine_rt;
using pcmx::device_cus;
using pcmx::from_lane_below;
using pcmx::identity;
using pcmx::identity_rt;
using pcmx::kFlagAgg;
using pcmx::kFlagIncl;
using pcmx::kWave;
using pcmx::misaligned;
using pcmx::pad2;
using pcmx::pad4;
using pcmx::u32x4;
using pcmx::Vec4;
using namespace pcmx::tile_bits;             // the tile shape (128 KiB of keys) and the per-element bit helpers
constexpr unsigned kFirstIsHead = 1u << 31;  // tile_meta: the tile's first element starts a run

// followed by unsigned long long status[tiles, padded to even], unsigned tile_p[tiles4], unsigned tile_meta[tiles4],
// 4-byte tile_lead[tiles4] (tiles4 = tiles padded to a multiple of 4)
typedef pcmx::LookbackHeader SegWs;
typedef pcmx::GranuleU32 Granule;  // the tile's count of run heads

__device__ __forceinline__ unsigned to_bits(float v) { return __float_as_uint(v); }
__device__ __forceinline__ unsigned to_bits(int v) { return (unsigned)v; }

// The side arrays behind the granules.
struct SideArrays {
    unsigned* tile_p;     // exclusive head count before the tile (from the look-back)
    unsigned* tile_meta;  // heads in the tile | kFirstIsHead
    void* tile_lead;      // aggregate of the elements before the tile's first head (the whole tile when it has none)
};

__host__ __device__ inline SideArrays side_arrays(void* ws, long long tiles) {
    unsigned long long* status = reinterpret_cast<unsigned long long*>(static_cast<SegWs*>(ws) + 1);
    SideArrays s;
    s.tile_p = reinterpret_cast<unsigned*>(status + pad2(tiles));
    s.tile_meta = s.tile_p + pad4(tiles);
    s.tile_lead = s.tile_meta + pad4(tiles);
    return s;
}

// Stream the stage's [0, cnt) out coalesced to dst[0 .. cnt).
__device__ __forceinline__ void stream_out(unsigned* __restrict__ dst, const unsigned* s_stage, unsigned cnt) {
#pragma unroll 4
    for (unsigned i = threadIdx.x; i < cnt; i += kWaves * kWave) dst[i] = s_stage[i];
}

// One tile: loads its keys and values, counts the heads, publishes the count, looks back (wave 0) while the other
// waves run the segmented scan of the values, then stores the tile's runs. Returns with the next ticket in *s_next.
template <int SRC, class T, int OP>
__device__ __forceinline__ void process_tile(const unsigned* __restrict__ keys, const T* __restrict__ vals,
                                             unsigned* __restrict__ run_keys, T* __restrict__ agg_out,
                                             int* __restrict__ starts, long long n, long long tile, long long ntiles,
                                             long long* num_runs_dev, SegWs* ws, unsigned* err_flag, const SideArrays& side,
                                             unsigned* s_wave_tot, unsigned* s_prefix, unsigned* s_next, T* s_tail,
                                             T* s_first, unsigned* s_stage) {
    typedef typename Vec4<T>::type V;
    unsigned long long* status = reinterpret_cast<unsigned long long*>(ws + 1);
    T* tile_lead = static_cast<T*>(side.tile_lead);
    const int lane = pcmx::lane_id(), wave = threadIdx.x / kWave;
    const T id = identity<T, OP>();
    TileKeys t;
    V v[kRows];
    load_keys(keys, n, tile, t);
    load_vals<SRC, T, OP>(vals, n, tile, v);
    // ---- head bits, then per row the integer wave prefix of the heads (input order: row, lane, element)
    const unsigned long long bits = drop_past_n(head_bits(t), n, tile);
    unsigned carry;  // wave-uniform: the wave's heads
    unsigned lane_off[kRows];
    rank_rows(bits, lane_off, carry);
    if (lane == 0) s_wave_tot[wave] = carry;
    __syncthreads();
    unsigned agg, wexcl;
    fold_wave_totals(s_wave_tot, agg, wexcl);
    const bool tile_starts_run = ((unsigned)bits & 1u) != 0u;  // meaningful in thread 0: it holds the tile's element 0
    if (threadIdx.x == 0) {
        __hip_atomic_store(&status[tile], Granule::pack(tile == 0 ? kFlagIncl : kFlagAgg, agg), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        side.tile_meta[tile] = agg | (tile_starts_run ? kFirstIsHead : 0u);
        *s_next = atomicAdd(&ws->ticket, 1u);  // the ticket of this block's next tile
    }

    // ---- wave 0: decoupled look-back over the predecessors' {flag, head count} granules
    if (wave == 0) {
        // (after a give-up the partial prefix is <= the true one: the stores stay inside out)
        const unsigned prefix = pcmx::lookback_publish<Granule>(ws, status, tile, agg, err_flag);
        if (lane == 0) {
            *s_prefix = prefix;
            side.tile_p[tile] = prefix;
            if (tile == ntiles - 1) *num_runs_dev = (long long)(prefix + agg);  // the owner of the last tile
        }
    }

    // ---- segmented scan of the values, wave-local, in input order (the other waves run this during the look-back):
    //      per row the lane's 4 elements serially, then the 64 lanes by shuffles; rcur carries the open run's aggregate
    //      from row to row. A head closes the run before it and sends that run's aggregate to the stage at its in-tile
    //      rank. Only the wave's FIRST head closes a run that may reach into earlier waves: its aggregate waits in
    //      s_first for the wave tails.
    //      (The row's wave scan up to `acc` has the same text in scanbykey.hip. As one __forceinline__ function of
    //      tile_bits.h, returning acc / fmask / tail as a struct or through references, with the lane's 4 elements
    //      inside or outside, it compiles differently: here 141 -> 143 SGPR spills in three kernels and 16 -> 0 bytes of
    //      scratch in float min / max, there 129-169 -> 128-168 VGPRs and 68-116 -> 29-70 SGPR spills. Kept written out.)
    T rcur = id;
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
        unsigned c = lane_off[r];  // heads of this wave before this lane's row
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (k & (1u << j)) {
                if (c != 0u)
                    s_stage[wexcl + c - 1u] = to_bits(acc);
                else
                    s_first[wave] = acc;
                ++c;
                acc = v[r][j];
            } else {
                acc = combine<T, OP>(acc, v[r][j]);
            }
        }
        rcur = fmask ? tail : combine<T, OP>(rcur, tail);
    }
    if (lane == 0) s_tail[wave] = rcur;
    __syncthreads();
    // ---- the open run's aggregate on entry to this wave, and on leaving the tile
    T wc, closing;
    fold_wave_tails<T, OP>(s_tail, [&](int w) { return s_wave_tot[w] != 0u; }, wc, closing);
    if (agg == 0u) {  // block-uniform: no head, the whole tile is the lead of a run that began earlier
        if (threadIdx.x == 0) tile_lead[tile] = closing;
        return;
    }
    if (lane == 0 && carry != 0u) {  // the run this wave's first head closes
        const T first = combine<T, OP>(wc, s_first[wave]);
        if (wexcl != 0u)
            s_stage[wexcl - 1u] = to_bits(first);
        else if (!(wave == 0 && tile_starts_run))
            tile_lead[tile] = first;  // the elements before the tile's first head
    }
    if (threadIdx.x == 0) s_stage[agg - 1u] = to_bits(closing);  // the tile's last run, closed by the end of the tile
    __syncthreads();
    const unsigned p = __builtin_amdgcn_readfirstlane(*s_prefix);
    stream_out(reinterpret_cast<unsigned*>(agg_out) + p, s_stage, agg);
    // ---- run keys, then start offsets, through the same stage: a head's entry goes to its run's in-tile rank
    if (run_keys) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const unsigned k = (unsigned)(bits >> (4 * r)) & 0xfu;
            unsigned pos = wexcl + lane_off[r];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k & (1u << j)) {
                    s_stage[pos] = t.k[r][j];
                    ++pos;
                }
            }
        }
        __syncthreads();
        stream_out(run_keys + p, s_stage, agg);
    }
    if (starts) {
        const unsigned first = (unsigned)(tile * kTileElems) + (unsigned)(wave * kWaveItems + lane * 4);  // n < 2^31
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const unsigned k = (unsigned)(bits >> (4 * r)) & 0xfu;
            unsigned pos = wexcl + lane_off[r];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k & (1u << j)) {
                    s_stage[pos] = first + (unsigned)(r * 256 + j);
                    ++pos;
                }
            }
        }
        __syncthreads();
        stream_out(reinterpret_cast<unsigned*>(starts) + p, s_stage, agg);
    }
    // (the next tile's first stage write follows its first barrier, which every wave reaches after these reads)
}

template <int SRC, class T, int OP>
__global__ __launch_bounds__(kWaves * kWave) void segreduce_kernel(const unsigned* __restrict__ keys,
                                                                   const T* __restrict__ vals,
                                                                   unsigned* __restrict__ run_keys, T* __restrict__ agg_out,
                                                                   int* __restrict__ starts, long long n, long long ntiles,
                                                                   long long* num_runs_dev, SegWs* ws, unsigned* err_flag) {
    // two LDS slots for the broadcast values, as in select.hip: a slot is rewritten two tiles later, with the other
    // tile's barriers in between
    __shared__ unsigned s_wave_tot[2][kWaves];
    __shared__ T s_tail[2][kWaves];
    __shared__ T s_first[2][kWaves];
    __shared__ unsigned s_prefix[2];
    __shared__ unsigned s_tile[2];
    __shared__ unsigned s_stage[kTileElems];  // 128 KiB: one entry per run of the tile, at its in-tile rank
    const SideArrays side = side_arrays(ws, ntiles);
    if (threadIdx.x == 0) s_tile[0] = atomicAdd(&ws->ticket, 1u);
    __syncthreads();
    for (int slot = 0;; slot ^= 1) {
        // (the tile number comes out of LDS: readfirstlane tells the compiler it is wave-uniform)
        const long long tile = __builtin_amdgcn_readfirstlane(s_tile[slot]);
        if (tile >= ntiles) break;
        process_tile<SRC, T, OP>(keys, vals, run_keys, agg_out, starts, n, tile, ntiles, num_runs_dev, ws, err_flag, side,
                                 s_wave_tot[slot], &s_prefix[slot], &s_tile[slot ^ 1], s_tail[slot], s_first[slot], s_stage);
    }
}

// Joins the runs that cross tile borders: one wave per tile s >= 1. Tile s begins a chain when the run open at its
// first element began in tile s - 1 (that tile has a head, and s does not start with one). The chain is s and every
// following tile reached without passing a head; their leads are folded in ascending tile order, 64 per step with a
// fixed butterfly, and combined into the run's aggregate at out[P_s - 1].
constexpr int kFixWaves = 4;
template <class T>
__global__ __launch_bounds__(kFixWaves * kWave) void lead_fixup_kernel(T* __restrict__ out, const unsigned* __restrict__ tile_p,
                                                                       const unsigned* __restrict__ tile_meta,
                                                                       const T* __restrict__ tile_lead, long long ntiles,
                                                                       int op) {
    const int lane = pcmx::lane_id();
    const long long s = (long long)blockIdx.x * kFixWaves + threadIdx.x / kWave + 1;  // wave-uniform
    if (s >= ntiles) return;
    if ((tile_meta[s] & kFirstIsHead) || (tile_meta[s - 1] & ~kFirstIsHead) == 0u) return;
    const unsigned p = tile_p[s];
    if (p == 0u || (long long)p > s * kTileElems) return;  // only after a look-back that gave up (already reported)
    const T id = identity_rt<T>(op);
    T acc = id;
    for (long long base = s; base < ntiles; base += kWave) {
        const long long u = base + lane;
        const bool in = u < ntiles;
        const unsigned mu = in ? tile_meta[u] : kFirstIsHead;
        const unsigned mprev = in ? tile_meta[u - 1] : 1u;
        const bool member = in && (u == s || ((mprev & ~kFirstIsHead) == 0u && !(mu & kFirstIsHead)));
        T v = in ? tile_lead[u] : id;
        const unsigned long long bad = __ballot(!member);
        const int cnt = bad ? __builtin_ctzll(bad) : kWave;
        v = lane < cnt ? v : id;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = combine_rt<T>(op, v, __shfl_xor(v, off, kWave));
        acc = combine_rt<T>(op, acc, v);
        if (cnt < kWave) break;
    }
    if (lane == 0) out[p - 1u] = combine_rt<T>(op, out[p - 1u], acc);
}

inline long long num_tiles(long long n) { return (n + kTileElems - 1) / kTileElems; }
// header + one granule per tile + three 4-byte side arrays, each padded to 16 bytes (zeroed before every launch)
inline size_t ws_bytes(long long tiles) { return sizeof(SegWs) + (size_t)pad2(tiles) * 8 + (size_t)pad4(tiles) * 12; }

template <int SRC, class T, int OP>
int launch_op(const void* keys, const T* vals, long long n, void* run_keys, T* agg, int* starts, long long* num_runs_dev,
              void* workspace, unsigned* err_flag, hipStream_t s) {
    const long long tiles = num_tiles(n);
    PCMX_HIP_RET(hipMemsetAsync(workspace, 0, ws_bytes(tiles), s));
    const unsigned grid = (unsigned)(tiles < device_cus() ? tiles : device_cus());  // one resident block per CU
    segreduce_kernel<SRC, T, OP><<<grid, kWaves * kWave, 0, s>>>(static_cast<const unsigned*>(keys), vals,
                                                                 static_cast<unsigned*>(run_keys), agg, starts, n, tiles,
                                                                 num_runs_dev, reinterpret_cast<SegWs*>(workspace), err_flag);
    PCMX_HIP_RET(hipGetLastError());
    if (tiles > 1) {
        const SideArrays side = side_arrays(workspace, tiles);
        const unsigned fgrid = (unsigned)((tiles - 1 + kFixWaves - 1) / kFixWaves);
        lead_fixup_kernel<T><<<fgrid, kFixWaves * kWave, 0, s>>>(agg, side.tile_p, side.tile_meta,
                                                                static_cast<const T*>(side.tile_lead), tiles, OP);
    }
    return (int)hipGetLastError();
}

template <int SRC, class T>
int launch(const void* keys, const T* vals, long long n, int op, void* run_keys, T* agg, int* starts,
           long long* num_runs_dev, void* workspace, unsigned* err_flag, hipStream_t s) {
    if (!num_runs_dev) return PCMX_ERR_ARG;
    if (op < PCMX_OP_SUM || op > PCMX_OP_MAX) return PCMX_ERR_ARG;
    if (n <= 0) {
        PCMX_HIP_RET(hipMemsetAsync(num_runs_dev, 0, sizeof(long long), s));
        return 0;
    }
    if (n >= (1LL << 31)) return PCMX_ERR_ARG;  // offsets and granule counts are 32-bit
    if (!keys || misaligned(keys) || !agg || misaligned(agg) || !workspace) return PCMX_ERR_ARG;
    if (SRC != kSrcOne && (!vals || misaligned(vals))) return PCMX_ERR_ARG;
    if (misaligned(run_keys) || misaligned(starts)) return PCMX_ERR_ARG;  // both may be NULL
    if constexpr (SRC == kSrcOne) {
        return launch_op<SRC, T, PCMX_OP_SUM>(keys, vals, n, run_keys, agg, starts, num_runs_dev, workspace, err_flag, s);
    } else {
        switch (op) {
            case PCMX_OP_SUM:
                return launch_op<SRC, T, PCMX_OP_SUM>(keys, vals, n, run_keys, agg, starts, num_runs_dev, workspace, err_flag, s);
            case PCMX_OP_MIN:
                return launch_op<SRC, T, PCMX_OP_MIN>(keys, vals, n, run_keys, agg, starts, num_runs_dev, workspace, err_flag, s);
            default:
                return launch_op<SRC, T, PCMX_OP_MAX>(keys, vals, n, run_keys, agg, starts, num_runs_dev, workspace, err_flag, s);
        }
    }
}
}  // namespace

extern "C" long long pcmx_segreduce_workspace_bytes(long long n) { return (long long)ws_bytes(n > 0 ? num_tiles(n) : 0); }

extern "C" int pcmx_run_length_encode_b32(const void* keys, long long n, void* run_keys, int* counts, int* starts,
                                          long long* num_runs_dev, void* workspace, unsigned* err_flag, hipStream_t s) {
    if (n > 0 && !run_keys) return PCMX_ERR_ARG;
    return launch<kSrcOne, int>(keys, nullptr, n, PCMX_OP_SUM, run_keys, counts, starts, num_runs_dev, workspace, err_flag, s);
}

extern "C" int pcmx_reduce_by_key_f32(const void* keys, const float* vals, long long n, int op, void* run_keys, float* agg,
                                      long long* num_runs_dev, void* workspace, unsigned* err_flag, hipStream_t s) {
    return launch<kSrcF32, float>(keys, vals, n, op, run_keys, agg, nullptr, num_runs_dev, workspace, err_flag, s);
}

extern "C" int pcmx_reduce_by_key_i32(const void* keys, const int32_t* vals, long long n, int op, void* run_keys,
                                      int32_t* agg, long long* num_runs_dev, void* workspace, unsigned* err_flag,
                                      hipStream_t s) {
    return launch<kSrcI32, int>(keys, vals, n, op, run_keys, agg, nullptr, num_runs_dev, workspace, err_flag, s);
}
