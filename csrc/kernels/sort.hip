// Stable LSD radix sort (keys, key-value pairs, argsort) of 32-bit keys: 8-bit digits, one upfront histogram kernel and
// one "one-sweep" kernel per digit (Adinets & Merrill, "Onesweep"), on the look-back machinery of scan.hip / select.hip.
// No counterpart in the reference programs: a library addition (the SpMV planners sort row / slice ids).
//
// A pass is select.hip's persistent schedule run over 256 digit counters instead of one kept count:
//  * One 512-thread block per CU claims 64-KiB tiles (16384 keys) from the pass's atomic ticket in the workspace, so
//    every predecessor of a claimed tile has itself been claimed by a resident block.
//  * Tile order is (wave, row, lane): wave w owns keys [2048 w, 2048 (w + 1)) of the tile as 32 rows of 64 lanes. A row
//    is ranked by match-any (radix_rank.h's rank_row: one ballot per digit bit, v_mbcnt of the peer mask) on top of the
//    wave's 256 LDS digit counters, so a key's rank counts exactly the equal digits before it in that order: the pass
//    is stable. cnt_load / cnt_store and block_excl256 are radix_rank.h's too, shared with rowsort.hip.
//  * Thread d publishes digit d's granule of the tile: one 4-byte word {flag (2 bits), count (30 bits)}, one relaxed
//    agent-scope store. Counts and prefixes stay below 2^30, which is why n is limited to 2^30 - 1.
//  * The tile is scattered into LDS at its sorted positions and the NEXT tile's loads are issued (the registers of this
//    tile are dead by then) before thread d looks back over its digit's column of granules, 32 predecessors per poll.
//  * The sorted tile streams out of LDS: position p of digit d goes to base[d] + prefix[d] + (p - start of d's run),
//    so the stores of a run are contiguous. Values travel with their keys through a second LDS array.
//  * Flag state: every pass has its own ticket and its own granule array; one hipMemsetAsync in front of the histogram
//    kernel zeroes the header, the histograms and the granules of all passes that run (1 KiB per tile and pass).
//  * The spin bound and the give-up report are lookback.h's (ws->head.timeout and the caller's sticky error word); the
//    per-digit loop and its 4-byte granules are this file's own.
// Keys live in the ping-pong buffers TRANSFORMED (u32 order = wanted order): the transform is applied in registers to
// what the first pass loads, and inverted in what the last pass stores.
#include "lookback.h"
#include "pcmx_common.h"
#include "pcmx_hip.h"
#include "radix_key.h"
#include "radix_rank.h"

namespace {
using pcmx::align16;
using pcmx::block_excl256;
using pcmx::cnt_store;
using pcmx::device_cus;
using pcmx::from_key;
using pcmx::kFlagAgg;
using pcmx::kFlagIncl;
using pcmx::kSpinLimit;
using pcmx::kWave;
using pcmx::misaligned;
using pcmx::rank_row;
using pcmx::report_timeout;
using pcmx::to_key;
using pcmx::u32x4;

// this file's granules are 4-byte words {flag: 2, count: 30}, one per digit and tile
constexpr unsigned kFlagShift = 30, kCountMask = (1u << kFlagShift) - 1u;
constexpr int kWaves = 8, kThreads = kWaves * kWave;  // 512
constexpr int kRows = 32;                             // keys per lane
constexpr int kWaveItems = kRows * kWave;             // 2048 contiguous keys per wave
constexpr int kTileElems = kWaves * kWaveItems;       // 16384 (64 KiB of keys)
constexpr int kDigits = 256, kMaxPasses = 4;
constexpr int kLook = 32;                             // predecessors per look-back poll and digit
constexpr long long kMaxN = (1LL << kFlagShift) - 1;  // a granule's count field carries an inclusive prefix <= n

struct SortWs {
    pcmx::LookbackHeader head;  // its `ticket` is unused here: every pass has its own
    unsigned pass_ticket[kMaxPasses];
    unsigned hist[kMaxPasses][kDigits];
    // followed by unsigned status[passes][num_tiles][256], then the ping-pong buffers
};
static_assert(offsetof(SortWs, head) == 0 && offsetof(SortWs, pass_ticket) == 16 && offsetof(SortWs, hist) == 32 &&
                  sizeof(SortWs) == 32 + kMaxPasses * kDigits * 4,
              "the workspace layout is part of the C interface (pcmx_sort_workspace_bytes)");

// ---------------------------------------------------------------- upfront histogram of every pass
// Reads the keys once. LDS counters per block, then one global atomic add per non-empty bin and block. A wave whose 64
// keys agree in every compared bit (all-equal or sorted input) adds 64 with one lane instead of 64 colliding atomics.
__global__ __launch_bounds__(kThreads) void sort_hist_kernel(const unsigned* __restrict__ keys, unsigned n,
                                                             unsigned* __restrict__ hist, int passes, int begin_bit,
                                                             int end_bit, int key_type, unsigned flip) {
    __shared__ unsigned s_h[kMaxPasses * kDigits];
    const int tid = threadIdx.x, lane = pcmx::lane_id();
    s_h[tid] = 0u, s_h[tid + kThreads] = 0u;
    __syncthreads();
    const int width = end_bit - begin_bit;
    const unsigned cmask = (width >= 32 ? ~0u : ((1u << width) - 1u)) << begin_bit;
    const unsigned nq = (n + 3u) / 4u;                                    // 16-byte quads, the last may be ragged
    const unsigned nq_round = (nq + (unsigned)kWave - 1u) & ~((unsigned)kWave - 1u);  // whole waves stay in the loop
    for (unsigned q = blockIdx.x * kThreads + tid; q < nq_round; q += gridDim.x * kThreads) {
        u32x4 v = {0u, 0u, 0u, 0u};
        unsigned cnt = 0u;  // keys of this quad below n; nothing at or past n is read
        if (q < nq) {
            const unsigned j = 4u * q;
            if (j + 4u <= n) {
                v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(keys + j));
                cnt = 4u;
            } else {
                cnt = n - j;
                v.x = keys[j];
                if (cnt > 1u) v.y = keys[j + 1u];
                if (cnt > 2u) v.z = keys[j + 2u];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool valid = (unsigned)e < cnt;
            const unsigned k = to_key(v[e], key_type, flip);
            const unsigned k0 = (unsigned)__builtin_amdgcn_readfirstlane((int)k);
            const bool uniform = __all(valid && ((k ^ k0) & cmask) == 0u);  // wave-uniform
            if (uniform ? lane == 0 : valid) {
                for (int p = 0; p < passes; ++p) {
                    const int shift = begin_bit + 8 * p, bits = min(8, end_bit - shift);
                    atomicAdd(&s_h[p * kDigits + ((k >> shift) & ((1u << bits) - 1u))], uniform ? (unsigned)kWave : 1u);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int b = tid + i * kThreads;
        if (b < passes * kDigits && s_h[b] != 0u) atomicAdd(&hist[b], s_h[b]);
    }
}

// ---------------------------------------------------------------- one pass
// The pointers are kernel parameters of their own (global address space, no flat accesses):
//   kin    keys read by this pass (the caller's raw keys in the first pass)
//   kout   keys written; NULL: this pass writes no keys (last pass of an argsort)
//   vin    values read; unused when iota
//   hist   this pass's 256 global digit counts
//   status this pass's granules [ntiles][256], zeroed
//   ticket this pass's tile ticket, zeroed
struct PassArgs {
    unsigned n, ntiles;
    int shift;             // first bit of the digit
    unsigned mask;         // (1 << digit width) - 1
    int key_type;
    unsigned flip;
    int first, last;       // transform on load / invert on store
    int iota;              // values of this pass are the global indices (first pass of an argsort)
};

// Issues the loads of one tile: key[r] / val[r] = element tile * 16384 + wave * 2048 + r * 64 + lane. Nothing at or
// past n is read (those registers hold 0 and are never ranked or staged).
template <bool VALS>
__device__ __forceinline__ void load_tile(const unsigned* __restrict__ kin, const unsigned* __restrict__ vin,
                                          const PassArgs& a, unsigned tile, unsigned (&key)[kRows],
                                          unsigned (&val)[VALS ? kRows : 1]) {
    const unsigned i0 = tile * kTileElems + (threadIdx.x / kWave) * kWaveItems + pcmx::lane_id();  // < 2^30
    const bool full = (tile + 1u) * kTileElems <= a.n;  // block-uniform
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const unsigned i = i0 + r * kWave;
        if (full) {
            key[r] = __builtin_nontemporal_load(kin + i);
            if (VALS && !a.iota) val[r] = __builtin_nontemporal_load(vin + i);
        } else {
            key[r] = i < a.n ? kin[i] : 0u;
            if (VALS && !a.iota) val[r] = i < a.n ? vin[i] : 0u;
        }
        if (VALS && a.iota) val[r] = i;
    }
}

template <bool VALS>
__global__ __launch_bounds__(kThreads) void sort_pass_kernel(const unsigned* __restrict__ kin, unsigned* __restrict__ kout,
                                                             const unsigned* __restrict__ vin, unsigned* __restrict__ vout,
                                                             const unsigned* __restrict__ hist, unsigned* status,
                                                             unsigned* ticket, SortWs* ws, unsigned* err_flag,
                                                             const PassArgs a) {
    __shared__ unsigned s_keys[kTileElems];             // the tile in sorted order
    __shared__ unsigned s_vals[VALS ? kTileElems : 1];
    __shared__ unsigned s_cnt[kWaves][kDigits];         // per wave: running digit counters, then exclusive wave offsets
    __shared__ unsigned s_base[kDigits];                // exclusive digit bases of the whole input (from the histogram)
    __shared__ unsigned s_toff[kDigits];                // start of each digit's run inside the sorted tile
    __shared__ unsigned s_gbase[kDigits];               // base + prefix - toff: global position = s_gbase[d] + p
    __shared__ unsigned s_wsum[4];
    __shared__ unsigned s_tick[2];
    const int tid = threadIdx.x, lane = pcmx::lane_id(), wave = tid / kWave;
    if (tid == 0) {
        s_tick[0] = atomicAdd(ticket, 1u);
        s_tick[1] = atomicAdd(ticket, 1u);
    }
    {   // the histogram kernel ran before this launch: its counts are complete
        const unsigned b = block_excl256(tid < kDigits ? hist[tid] : 0u, s_wsum);
        if (tid < kDigits) s_base[tid] = b;
    }
    unsigned cur = (unsigned)__builtin_amdgcn_readfirstlane((int)s_tick[0]);
    unsigned next = (unsigned)__builtin_amdgcn_readfirstlane((int)s_tick[1]);
    if (cur >= a.ntiles) return;  // block-uniform
    unsigned key[kRows], val[VALS ? kRows : 1];
    load_tile<VALS>(kin, vin, a, cur, key, val);
    while (true) {
        const bool full = (cur + 1u) * kTileElems <= a.n;                          // block-uniform
        const unsigned tile_n = full ? (unsigned)kTileElems : a.n - cur * kTileElems;  // 1 .. 16384
        const unsigned i0 = cur * kTileElems + wave * kWaveItems + lane;
        // ---- (b) stable ranks inside the wave. The wave zeroes its own counters: their last readers (the staging of
        //      the previous tile) are behind that tile's last barrier.
#pragma unroll
        for (int i = 0; i < kDigits / kWave; ++i) cnt_store(&s_cnt[wave][lane + i * kWave], 0u);
        unsigned rank[kRows];
        if (a.first) {  // kernel-uniform: the key transform, applied in registers to what the first pass loaded
            if (a.key_type == PCMX_KEY_F32) {
#pragma unroll
                for (int r = 0; r < kRows; ++r) key[r] = to_key(key[r], PCMX_KEY_F32, a.flip);
            } else {
                const unsigned x = (a.key_type == PCMX_KEY_I32 ? 0x80000000u : 0u) ^ a.flip;
#pragma unroll
                for (int r = 0; r < kRows; ++r) key[r] ^= x;
            }
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const bool valid = full || i0 + r * kWave < a.n;
            const unsigned d = (key[r] >> a.shift) & a.mask;
            rank[r] = rank_row(d, valid, s_cnt[wave]);  // match-any on the wave's counters (radix_rank.h)
        }
        __syncthreads();
        // ---- (c) thread d: digit d's count of the tile, the waves' exclusive offsets, and the tile's granule
        unsigned total = 0u;
        if (tid < kDigits) {
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const unsigned c = s_cnt[w][tid];
                s_cnt[w][tid] = total;
                total += c;
            }
            __hip_atomic_store(&status[cur * kDigits + tid], ((cur == 0u ? kFlagIncl : kFlagAgg) << kFlagShift) | total,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const unsigned toff = block_excl256(total, s_wsum);
        if (tid < kDigits) s_toff[tid] = toff;
        __syncthreads();
        // ---- the tile goes to LDS in sorted order: run start of the digit + equal digits of the lower waves + rank
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const bool valid = full || i0 + r * kWave < a.n;
            if (valid) {
                const unsigned d = (key[r] >> a.shift) & a.mask;
                const unsigned pos = s_toff[d] + s_cnt[wave][d] + rank[r];  // < tile_n
                s_keys[pos] = key[r];
                if (VALS) s_vals[pos] = val[r];
            }
        }
        // ---- (d) the next tile's loads go out now (this tile's registers are dead) and overlap the look-back and the
        //      stores; the ticket for the tile after `next` is taken here too
        if (next < a.ntiles) load_tile<VALS>(kin, vin, a, next, key, val);
        if (tid == 0) s_tick[0] = atomicAdd(ticket, 1u);
        // ---- (e) thread d: look back over digit d's granules of the predecessors, kLook of them per poll
        if (tid < kDigits) {
            unsigned prefix = 0u;
            if (cur != 0u) {
                int look = (int)cur - 1;  // newest predecessor still to account for
                unsigned spins = 0u;
                bool done = false;
                while (!done) {
                    unsigned g[kLook];
#pragma unroll
                    for (int i = 0; i < kLook; ++i) {
                        const int idx = look - i;
                        g[i] = idx >= 0 ? __hip_atomic_load(&status[(unsigned)idx * kDigits + tid], __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT)
                                        : (kFlagIncl << kFlagShift);
                    }
                    bool stalled = false;
#pragma unroll
                    for (int i = 0; i < kLook; ++i) {
                        const unsigned f = g[i] >> kFlagShift;
                        if (!done && !stalled) {
                            if (f == 0u) {
                                stalled = true;  // not published yet: poll again from here
                            } else {
                                prefix += g[i] & kCountMask;  // an aggregate never changes: it is taken once
                                --look;
                                done = f == kFlagIncl;
                            }
                        }
                    }
                    if (stalled) {
                        // bounded spin: report (workspace + sticky caller word) and go on with the partial prefix. A
                        // partial prefix is never larger than the true one, and base[d] comes from the complete
                        // histogram, so every store below stays inside [0, n) of the output buffers.
                        if (++spins > kSpinLimit) {
                            report_timeout(&ws->head, err_flag);  // from whichever thread gave up
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                }
                __hip_atomic_store(&status[cur * kDigits + tid], (kFlagIncl << kFlagShift) | (prefix + total),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            s_gbase[tid] = s_base[tid] + prefix - toff;  // mod 2^32; s_gbase[d] + p is in [0, n) for p in d's run
        }
        __syncthreads();
        const unsigned after = (unsigned)__builtin_amdgcn_readfirstlane((int)s_tick[0]);
        // ---- (f) stream the sorted tile out: consecutive p of one digit are consecutive in the output
#pragma unroll 8
        for (int i = 0; i < kRows; ++i) {
            const unsigned p = (unsigned)tid + (unsigned)i * kThreads;
            if (p < tile_n) {
                const unsigned k = s_keys[p];
                const unsigned g = s_gbase[(k >> a.shift) & a.mask] + p;
                if (kout) kout[g] = a.last ? from_key(k, a.key_type, a.flip) : k;
                if (VALS) vout[g] = s_vals[p];
            }
        }
        if (next >= a.ntiles) break;  // block-uniform
        // the next tile's first LDS writes that other waves read (s_cnt of other waves, s_toff, s_keys) all sit behind
        // its first barrier, which every wave reaches only after the reads above
        cur = next;
        next = after;
    }
}

inline long long num_tiles(long long n) { return (n + kTileElems - 1) / kTileElems; }
// One ping-pong buffer of n words plus an odd number of 256-byte lines, so that the keys and values a tile reads and
// writes together do not sit a power of two apart in the workspace.
inline size_t buf_bytes(long long n) { return align16((size_t)n * 4u) + 273u * 256u; }
inline size_t status_bytes(long long tiles) { return (size_t)tiles * kDigits * sizeof(unsigned); }
}  // namespace

// header | granules of 4 passes | key buffer A | key buffer B (index mode: the keys may never touch a caller buffer) |
// value buffer (pairs and index mode)
extern "C" long long pcmx_sort_workspace_bytes(long long n, int mode) {
    if (n <= 0) return (long long)sizeof(SortWs);
    const size_t buf = buf_bytes(n);
    const int bufs = mode == PCMX_SORT_KEYS ? 1 : (mode == PCMX_SORT_PAIRS ? 2 : 3);
    return (long long)(sizeof(SortWs) + kMaxPasses * status_bytes(num_tiles(n)) + bufs * buf);
}

extern "C" int pcmx_radix_sort(const void* keys_in, void* keys_out, const void* vals_in, void* vals_out, long long n,
                               int key_type, int mode, int descending, int begin_bit, int end_bit, void* workspace,
                               unsigned* err_flag, hipStream_t s) {
    if (n <= 0) return 0;
    if (n > kMaxN) return PCMX_ERR_ARG;  // indices and granule counts: 30 bits
    if (key_type < PCMX_KEY_U32 || key_type > PCMX_KEY_F32 || mode < PCMX_SORT_KEYS || mode > PCMX_SORT_INDEX)
        return PCMX_ERR_ARG;
    if (begin_bit < 0 || end_bit > 32 || begin_bit >= end_bit) return PCMX_ERR_ARG;
    if (!keys_in || misaligned(keys_in) || !workspace || misaligned(workspace)) return PCMX_ERR_ARG;
    if (misaligned(keys_out) || (!keys_out && mode != PCMX_SORT_INDEX)) return PCMX_ERR_ARG;
    if (mode == PCMX_SORT_PAIRS && (!vals_in || misaligned(vals_in))) return PCMX_ERR_ARG;
    if (mode != PCMX_SORT_KEYS && (!vals_out || misaligned(vals_out))) return PCMX_ERR_ARG;

    const int passes = (end_bit - begin_bit + 7) / 8;
    const long long tiles = num_tiles(n);
    char* w = static_cast<char*>(workspace);
    SortWs* ws = reinterpret_cast<SortWs*>(w);
    unsigned* status = reinterpret_cast<unsigned*>(w + sizeof(SortWs));
    const size_t buf = buf_bytes(n);
    char* bufs = w + sizeof(SortWs) + kMaxPasses * status_bytes(tiles);
    unsigned* key_a = reinterpret_cast<unsigned*>(bufs);
    unsigned* key_b = reinterpret_cast<unsigned*>(bufs + buf);                              // index mode only
    unsigned* val_a = reinterpret_cast<unsigned*>(bufs + (mode == PCMX_SORT_INDEX ? 2 : 1) * buf);  // pairs / index

    // flag reset: header, histograms, and the tickets + granules of every pass that runs, in one memset
    PCMX_HIP_RET(hipMemsetAsync(workspace, 0, sizeof(SortWs) + passes * status_bytes(tiles), s));
    const unsigned flip = descending ? ~0u : 0u;
    {
        const long long quads = (n + 3) / 4, want = (quads + kThreads - 1) / kThreads, cap = 4LL * device_cus();
        sort_hist_kernel<<<(unsigned)(want < cap ? want : cap), kThreads, 0, s>>>(
            static_cast<const unsigned*>(keys_in), (unsigned)n, &ws->hist[0][0], passes, begin_bit, end_bit, key_type, flip);
        PCMX_HIP_RET(hipGetLastError());
    }
    const unsigned grid = (unsigned)(tiles < device_cus() ? tiles : device_cus());  // one resident block per CU
    const unsigned* ksrc = static_cast<const unsigned*>(keys_in);
    const unsigned* vsrc = static_cast<const unsigned*>(vals_in);
    for (int p = 0; p < passes; ++p) {
        // ping-pong so that the LAST pass lands in the caller's output: passes from the end, even -> output, odd ->
        // workspace. The caller's input is only ever a source.
        const int from_end = passes - 1 - p;
        unsigned* kout;
        if (keys_out) kout = (from_end & 1) ? key_a : static_cast<unsigned*>(keys_out);
        else kout = from_end == 0 ? nullptr : ((from_end & 1) ? key_a : key_b);
        unsigned* vout = mode == PCMX_SORT_KEYS ? nullptr : ((from_end & 1) ? val_a : static_cast<unsigned*>(vals_out));
        unsigned* pass_status = status + (size_t)p * tiles * kDigits;
        PassArgs a;
        a.n = (unsigned)n, a.ntiles = (unsigned)tiles;
        a.shift = begin_bit + 8 * p;
        const int bits = end_bit - a.shift < 8 ? end_bit - a.shift : 8;
        a.mask = (1u << bits) - 1u;
        a.key_type = key_type, a.flip = flip;
        a.first = p == 0, a.last = p == passes - 1;
        a.iota = mode == PCMX_SORT_INDEX && p == 0;
        if (mode == PCMX_SORT_KEYS)
            sort_pass_kernel<false><<<grid, kThreads, 0, s>>>(ksrc, kout, vsrc, vout, ws->hist[p], pass_status,
                                                              &ws->pass_ticket[p], ws, err_flag, a);
        else
            sort_pass_kernel<true><<<grid, kThreads, 0, s>>>(ksrc, kout, vsrc, vout, ws->hist[p], pass_status,
                                                             &ws->pass_ticket[p], ws, err_flag, a);
        PCMX_HIP_RET(hipGetLastError());
        ksrc = kout, vsrc = vout;
    }
    return 0;
}
