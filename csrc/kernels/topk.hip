// Top-k and k-th value of 32-bit keys by a most-significant-digit radix select, beside the radix sort of sort.hip.
// No counterpart in the reference programs: a library addition, the next member of the scan / select / sort family.
//
// The result is the first k entries of sort.hip's stable sort (values and int32 flat indices), found without moving
// the data: keys are compared TRANSFORMED exactly as in sort.hip (radix_key.h's to_key, shared; flip = ~0 when the
// largest are wanted), so "better" always means "smaller transformed key" and the k best are the k smallest.
//  * Step A, the k-th key T: four passes over the keys, 8 bits per digit from the top. A pass histograms the current
//    digit of the keys whose higher digits equal the prefix chosen so far (256 LDS counters per block, sort.hip's
//    wave-uniform shortcut, one global atomic add per non-empty bin and block). Between passes a one-block kernel walks
//    the 256 bins from the best, finds the bin that holds the k-th key, subtracts what lies before it from the
//    remaining k and extends the prefix. Prefix, remaining k and the count of keys strictly better than the prefix
//    live in the workspace; the choice never goes through the host and kernel boundaries alone order the passes: no
//    inter-block waiting in step A. After the last pass the workspace holds T, c_beyond (keys better than T, < k) and
//    need_eq = k - c_beyond (>= 1). The k-th value is this step plus one store of from_key(T).
//  * Step B, the ordered gather: one pass on select.hip's schedule and lookback.h's look-back: one 512-thread block per
//    CU, 32768-key tiles claimed from the atomic ticket, the next tile's loads in flight during the look-back, 8-byte
//    granules written with one relaxed agent-scope store, bounded spins, hipMemsetAsync of the flags before the launch.
//    The granule carries TWO counts, {flag: 2 bits, keys better than T: 31, keys equal to T: 31}, because which ties are
//    taken must not depend on timing: an element is kept if it is better than T, or equals T with a global rank below
//    need_eq among the equal ones (the lowest flat indices). With exclusive ranks (gb, ge) of an element its output
//    position is gb + min(ge, need_eq); kept elements go straight from registers to vals[pos] (canonical bits,
//    from_key(to_key(bits))) and idx[pos]. Tiles that keep nothing (nearly all, when k << n) skip the store phase.
//    Every store is guarded by pos < k, so a look-back that gave up (a prefix too small) cannot write outside.
//  * Step C (sorted output): the k survivors, in ascending index order, are sorted as (value, index) pairs by sort.hip's
//    stable pcmx_radix_sort, which yields exactly the prefix of the full stable sort.
// The workspace begins with pcmx::LookbackHeader, so pcmx_scan_check reads a top-k workspace too; a give-up sets
// ws->timeout and ORs 1 into the caller's sticky error word.
#include "lookback.h"
#include "pcmx_common.h"
#include "pcmx_hip.h"
#include "radix_key.h"

namespace {
using pcmx::align16;
using pcmx::at;
using pcmx::device_cus;
using pcmx::from_key;
using pcmx::kFlagAgg;
using pcmx::kFlagIncl;
using pcmx::kWave;
using pcmx::lanes_below;
using pcmx::misaligned;
using pcmx::to_key;
using pcmx::u32x4;
typedef unsigned long long u64;
typedef pcmx::GranuleU31x2 Granule;  // {keys better than T, keys equal to T}

constexpr int kRows = 16, kWaves = 8, kThreads = kWaves * kWave;  // 16 rows of 4 keys per lane, 8 waves
constexpr int kWaveItems = kRows * 4 * kWave;                     // 4096 contiguous keys per wave
constexpr int kTileElems = kWaves * kWaveItems;                   // 32768 (128 KiB of keys)
constexpr int kDigits = 256, kPasses = 4;
constexpr long long kMaxN = (1LL << 30) - 1;                      // the sort's limit; granule counts have 31 bits

// The whole struct and the granules behind it are zeroed by one hipMemsetAsync in front of the first kernel.
struct TopkWs {
    pcmx::LookbackHeader head;
    unsigned prefix;    // the digits of T chosen so far (lower bits 0); T itself after the last pass
    unsigned k_rem;     // 1-based rank of the k-th key among the keys that match the prefix; need_eq after the last pass
    unsigned c_beyond;  // keys strictly better than every key that matches the prefix
    unsigned pad2;
    unsigned hist[kPasses][kDigits];
    // followed by u64 status[num_tiles]
};
static_assert(offsetof(TopkWs, head) == 0 && offsetof(TopkWs, prefix) == 16 && offsetof(TopkWs, k_rem) == 20 &&
                  offsetof(TopkWs, c_beyond) == 24 && offsetof(TopkWs, hist) == 32 &&
                  sizeof(TopkWs) == 32 + kPasses * kDigits * 4,
              "the workspace layout is part of the C interface (pcmx_topk_workspace_bytes)");

// ---------------------------------------------------------------- step A: one histogram pass
// Digit `pass` (0 = bits 31..24) of the keys whose higher digits equal ws->prefix. Reads the keys once and writes
// nothing but the 256 counters. A wave whose 64 keys all match and agree in the digit (all-equal or sorted input) adds
// 64 with one lane instead of 64 colliding atomics; keys that do not match the prefix touch no LDS.
__global__ __launch_bounds__(kThreads) void topk_hist_kernel(const unsigned* __restrict__ keys, unsigned n, TopkWs* ws,
                                                             int pass, int key_type, unsigned flip) {
    __shared__ unsigned s_h[kDigits];
    const int tid = threadIdx.x, lane = pcmx::lane_id();
    if (tid < kDigits) s_h[tid] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : ~0u << (shift + 8);
    const unsigned prefix = ws->prefix;  // written by the choose kernel of the previous pass
    const unsigned nq = (n + 3u) / 4u;   // 16-byte quads, the last may be ragged
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
            const unsigned k = to_key(v[e], key_type, flip);
            const bool match = (unsigned)e < cnt && ((k ^ prefix) & himask) == 0u;
            const unsigned d = (k >> shift) & 0xffu;
            const unsigned d0 = (unsigned)__builtin_amdgcn_readfirstlane((int)d);
            const bool uniform = __all(match && d == d0);  // wave-uniform
            if (uniform ? lane == 0 : match) atomicAdd(&s_h[d], uniform ? (unsigned)kWave : 1u);
        }
    }
    __syncthreads();
    if (tid < kDigits && s_h[tid] != 0u) atomicAdd(&ws->hist[pass][tid], s_h[tid]);
}

// ---------------------------------------------------------------- step A: the choice of one digit (one block)
// Thread d holds bin d of the finished histogram; the bin whose exclusive prefix is below the remaining k and whose
// inclusive prefix reaches it holds the k-th key. After the last pass ws->prefix is T and ws->k_rem is need_eq, and
// the k-th value goes to *out_kth when it is wanted.
__global__ __launch_bounds__(kDigits) void topk_choose_kernel(TopkWs* ws, int pass, unsigned k, int key_type, unsigned flip,
                                                              unsigned* out_kth) {
    __shared__ unsigned s_wsum[kDigits / kWave];
    const int tid = threadIdx.x, lane = pcmx::lane_id(), wave = tid / kWave;
    const unsigned k_rem = pass == 0 ? k : ws->k_rem;  // every thread reads it before the barrier, the winner writes after
    const unsigned prefix = ws->prefix, c_beyond = ws->c_beyond;
    const unsigned c = ws->hist[pass][tid];
    unsigned inc = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned o = __shfl_up(inc, off, kWave);
        if (lane >= off) inc += o;
    }
    if (lane == kWave - 1) s_wsum[wave] = inc;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kDigits / kWave; ++w) inc += w < wave ? s_wsum[w] : 0u;
    const unsigned excl = inc - c;
    if (excl < k_rem && k_rem <= inc) {  // exactly one bin (c != 0 follows)
        const unsigned t = prefix | ((unsigned)tid << (24 - 8 * pass));
        ws->prefix = t;
        ws->k_rem = k_rem - excl;
        ws->c_beyond = c_beyond + excl;
        if (pass == kPasses - 1 && out_kth) *out_kth = from_key(t, key_type, flip);
    }
}

// ---------------------------------------------------------------- step B: the ordered gather
struct TileRegs {
    u32x4 v[kRows];
};

// Element (r, j) of a lane is key tile * 32768 + wave * 4096 + r * 256 + lane * 4 + j. Nothing at or past n is read
// (those registers hold 0 and are dropped by the bound in classify).
__device__ __forceinline__ void load_tile(const unsigned* __restrict__ x, unsigned n, unsigned tile, TileRegs& t) {
    const int lane = pcmx::lane_id(), wave = threadIdx.x / kWave;
    const unsigned* xt = x + (size_t)tile * kTileElems;  // block-uniform base, 32-bit offsets inside the tile
    const unsigned off = (unsigned)(wave * kWaveItems + lane * 4);
    if ((tile + 1u) * (unsigned)kTileElems <= n) {  // block-uniform: full tiles take the branch-free path
#pragma unroll
        for (int r = 0; r < kRows; ++r) t.v[r] = __builtin_nontemporal_load(at<u32x4>(xt + r * 256, off * 4u));
        return;
    }
    const unsigned rem = n - tile * (unsigned)kTileElems;  // the last tile, once per launch: 1 .. 32767 keys, one by one
    unsigned o = off;
    asm volatile("" : "+v"(o));  // opaque: the 64 element offsets are formed here, not hoisted out of the tile loop
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned e = o + (unsigned)(r * 256 + j);
            t.v[r][j] = e < rem ? xt[e] : 0u;
        }
    }
}

// bit j: element j of the row is better than T (lo nibble) / equal to T (hi nibble); keys are returned transformed
template <int TYPE>
__device__ __forceinline__ unsigned classify(const u32x4& v, unsigned flip, unsigned T, unsigned left, unsigned (&key)[4]) {
    unsigned m = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        key[j] = to_key(v[j], TYPE, flip);
        const bool valid = (unsigned)j < left;
        m |= (valid && key[j] < T ? 1u : 0u) << j;
        m |= (valid && key[j] == T ? 16u : 0u) << j;
    }
    return m;
}

// Counts tile `tile` held in t, publishes its two counts, issues the loads of `next` into tn, looks back, stores.
template <int TYPE>
__device__ __forceinline__ void finish_tile(const unsigned* __restrict__ x, unsigned* __restrict__ vals,
                                            unsigned* __restrict__ idx, unsigned n, unsigned k, unsigned flip, unsigned T,
                                            unsigned need_eq, unsigned tile, TileRegs& t, unsigned next, TileRegs& tn,
                                            unsigned ntiles, TopkWs* ws, unsigned* err_flag, unsigned* s_wave_tot,
                                            unsigned* s_prefix, unsigned* s_next) {
    u64* status = reinterpret_cast<u64*>(ws + 1);
    const int lane = pcmx::lane_id(), wave = threadIdx.x / kWave;
    const unsigned base = (unsigned)(wave * kWaveItems + lane * 4);                 // in-tile index of (row 0, element 0)
    const unsigned rem = min(n - tile * (unsigned)kTileElems, (unsigned)kTileElems);  // keys of this tile below n
    // ---- the lane's counts of better and equal keys, then the wave's and the tile's
    unsigned cb = 0u, ce = 0u;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const unsigned e = base + (unsigned)(r * 256);
        unsigned key[4];
        const unsigned m = classify<TYPE>(t.v[r], flip, T, e < rem ? rem - e : 0u, key);
        cb += (unsigned)__popc(m & 0xfu);
        ce += (unsigned)__popc(m >> 4);
    }
    cb = pcmx::wave_reduce<unsigned, 0>(cb);
    ce = pcmx::wave_reduce<unsigned, 0>(ce);
    if (lane == 0) s_wave_tot[2 * wave] = cb, s_wave_tot[2 * wave + 1] = ce;
    __syncthreads();
    unsigned aggb = 0u, agge = 0u, wexb = 0u, wexe = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const unsigned b = s_wave_tot[2 * w], e = s_wave_tot[2 * w + 1];
        wexb += w < wave ? b : 0u, wexe += w < wave ? e : 0u;
        aggb += b, agge += e;
    }
    const pcmx::Count2 agg = {aggb, agge};
    if (threadIdx.x == 0)
        __hip_atomic_store(&status[tile], Granule::pack(tile == 0u ? kFlagIncl : kFlagAgg, agg), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    // ---- the next tile's loads go out now and overlap the look-back below; this tile's keys stay in t
    if (next < ntiles) load_tile(x, n, next, tn);
    // ---- the ticket for the tile after `next`, taken before this tile's stores (as in the scan)
    unsigned ticket = 0u;
    if (threadIdx.x == 0) ticket = atomicAdd(&ws->head.ticket, 1u);

    // ---- wave 0: decoupled look-back over the predecessors' {flag, better, equal} granules
    if (wave == 0) {
        // (after a give-up the partial prefixes are <= the true ones; stores are guarded by pos < k)
        const pcmx::Count2 p = pcmx::lookback_publish<Granule>(&ws->head, status, tile, agg, err_flag);
        if (lane == 0) s_prefix[0] = p.x, s_prefix[1] = p.y;
    }
    if (threadIdx.x == 0) *s_next = ticket;
    __syncthreads();
    const unsigned pb = (unsigned)__builtin_amdgcn_readfirstlane((int)s_prefix[0]);
    const unsigned pe = (unsigned)__builtin_amdgcn_readfirstlane((int)s_prefix[1]);
    // block-uniform: nothing of this tile is kept (no better key, and the equal ones are all past need_eq)
    if (aggb == 0u && (agge == 0u || pe >= need_eq)) return;

    // ---- store: exclusive global ranks (gb, ge) of every element in input order (wave, row, lane, element); the row
    //      ranks are a ballot per element position and class, the carry across rows is a scalar popcount
    unsigned rb = (unsigned)__builtin_amdgcn_readfirstlane((int)(pb + wexb));
    unsigned re = (unsigned)__builtin_amdgcn_readfirstlane((int)(pe + wexe));
    const unsigned first = tile * (unsigned)kTileElems + base;  // < 2^30
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const unsigned e = base + (unsigned)(r * 256);
        unsigned key[4];
        // (an opaque copy of the row: classified again here, or the compiler keeps the count phase's 64 transformed keys
        // and 16 class masks alive across the look-back and spills)
        u32x4 v = t.v[r];
        asm volatile("" : "+v"(v));
        const unsigned m = classify<TYPE>(v, flip, T, e < rem ? rem - e : 0u, key);
        const u64 b0 = __ballot(m & 1u), b1 = __ballot(m & 2u), b2 = __ballot(m & 4u), b3 = __ballot(m & 8u);
        const u64 e0 = __ballot(m & 16u), e1 = __ballot(m & 32u), e2 = __ballot(m & 64u), e3 = __ballot(m & 128u);
        if ((b0 | b1 | b2 | b3 | e0 | e1 | e2 | e3) == 0ull) continue;  // wave-uniform
        unsigned gb = lanes_below(b3, lanes_below(b2, lanes_below(b1, lanes_below(b0, rb))));
        unsigned ge = lanes_below(e3, lanes_below(e2, lanes_below(e1, lanes_below(e0, re))));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool better = (m >> j) & 1u, equal = (m >> (4 + j)) & 1u;
            if (better || (equal && ge < need_eq)) {
                const unsigned pos = gb + min(ge, need_eq);
                if (pos < k) {  // always true unless a look-back gave up
                    vals[pos] = from_key(key[j], TYPE, flip);
                    idx[pos] = first + (unsigned)(r * 256 + j);
                }
            }
            gb += better ? 1u : 0u;
            ge += equal ? 1u : 0u;
        }
        rb += (unsigned)(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3));
        re += (unsigned)(__popcll(e0) + __popcll(e1) + __popcll(e2) + __popcll(e3));
        __builtin_amdgcn_sched_barrier(0);  // one row at a time: 8 ballots are 16 SGPRs, 16 rows of them are not
    }
}

template <int TYPE>
__global__ __launch_bounds__(kThreads) void topk_gather_kernel(const unsigned* __restrict__ x, unsigned* __restrict__ vals,
                                                               unsigned* __restrict__ idx, unsigned n, unsigned k,
                                                               unsigned flip, unsigned ntiles, TopkWs* ws,
                                                               unsigned* err_flag) {
    // two LDS slots so consecutive tiles never race on the broadcast values: a slot is rewritten two tiles later,
    // with the other tile's two barriers in between
    __shared__ unsigned s_wave_tot[2][2 * kWaves];
    __shared__ unsigned s_prefix[2][2];
    __shared__ unsigned s_tile[2];
    TileRegs ta_regs, tb_regs;
    if (threadIdx.x == 0) {
        s_tile[0] = atomicAdd(&ws->head.ticket, 1u);
        s_tile[1] = atomicAdd(&ws->head.ticket, 1u);
    }
    __syncthreads();
    const unsigned T = ws->prefix, need_eq = ws->k_rem;  // step A's result (earlier kernels of this stream)
    unsigned ta = (unsigned)__builtin_amdgcn_readfirstlane((int)s_tile[0]);
    unsigned tb = (unsigned)__builtin_amdgcn_readfirstlane((int)s_tile[1]);
    if (ta >= ntiles) return;
    load_tile(x, n, ta, ta_regs);
    // unrolled by two so both register buffers are statically named (every exit is block-uniform); each finish_tile
    // takes the ticket two tiles ahead and publishes it in s_tile[slot] by its last barrier
    while (true) {
        finish_tile<TYPE>(x, vals, idx, n, k, flip, T, need_eq, ta, ta_regs, tb, tb_regs, ntiles, ws, err_flag,
                          s_wave_tot[0], s_prefix[0], &s_tile[0]);
        if (tb >= ntiles) break;
        ta = (unsigned)__builtin_amdgcn_readfirstlane((int)s_tile[0]);
        finish_tile<TYPE>(x, vals, idx, n, k, flip, T, need_eq, tb, tb_regs, ta, ta_regs, ntiles, ws, err_flag,
                          s_wave_tot[1], s_prefix[1], &s_tile[1]);
        if (ta >= ntiles) break;
        tb = (unsigned)__builtin_amdgcn_readfirstlane((int)s_tile[1]);
    }
}

inline long long num_tiles(long long n) { return (n + kTileElems - 1) / kTileElems; }
// header, histograms and one granule per tile, padded to a multiple of 16 bytes: the block zeroed before every call
inline size_t flag_bytes(long long tiles) { return sizeof(TopkWs) + (size_t)pcmx::pad2(tiles) * 8; }

int check_args(const void* keys, long long n, long long k, long long k_min, int key_type, const void* workspace) {
    if (n <= 0 || n > kMaxN || k < k_min || k > n) return PCMX_ERR_ARG;
    if (key_type < PCMX_KEY_U32 || key_type > PCMX_KEY_F32) return PCMX_ERR_ARG;
    if (!keys || misaligned(keys) || !workspace || misaligned(workspace)) return PCMX_ERR_ARG;
    return 0;
}

// Step A: zeroes the flag block, then four histogram passes with the one-block choice after each.
int select_kth(const void* keys, long long n, long long k, int key_type, unsigned flip, unsigned* out_kth, TopkWs* ws,
               hipStream_t s) {
    PCMX_HIP_RET(hipMemsetAsync(ws, 0, flag_bytes(num_tiles(n)), s));
    const long long quads = (n + 3) / 4, want = (quads + kThreads - 1) / kThreads, cap = 4LL * device_cus();
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    for (int p = 0; p < kPasses; ++p) {
        topk_hist_kernel<<<grid, kThreads, 0, s>>>(static_cast<const unsigned*>(keys), (unsigned)n, ws, p, key_type, flip);
        PCMX_HIP_RET(hipGetLastError());
        topk_choose_kernel<<<1, kDigits, 0, s>>>(ws, p, (unsigned)k, key_type, flip, out_kth);
        PCMX_HIP_RET(hipGetLastError());
    }
    return 0;
}
}  // namespace

// flag block | (sorted, k > 1) survivor values | survivor indices | the pair sort's workspace
extern "C" long long pcmx_topk_workspace_bytes(long long n, long long k, int sorted) {
    size_t b = flag_bytes(n > 0 ? num_tiles(n) : 0);
    if (sorted && k > 1) b += 2 * align16((size_t)k * 4u) + (size_t)pcmx_sort_workspace_bytes(k, PCMX_SORT_PAIRS);
    return (long long)b;
}

extern "C" int pcmx_kth_key_b32(const void* keys, long long n, long long k, int key_type, int largest, void* out_dev,
                                void* workspace, unsigned* err_flag, hipStream_t s) {
    (void)err_flag;  // step A has no look-back; the parameter keeps the family's signature
    if (const int rc = check_args(keys, n, k, 1, key_type, workspace)) return rc;
    if (!out_dev || (((uintptr_t)out_dev) & 3u)) return PCMX_ERR_ARG;
    return select_kth(keys, n, k, key_type, largest ? ~0u : 0u, static_cast<unsigned*>(out_dev),
                      reinterpret_cast<TopkWs*>(workspace), s);
}

extern "C" int pcmx_topk_b32(const void* keys, long long n, long long k, int key_type, int largest, int sorted,
                             void* out_vals, void* out_idx, void* workspace, unsigned* err_flag, hipStream_t s) {
    if (n == 0 && k == 0) return 0;
    if (n > 0 && k == 0) return n > kMaxN ? PCMX_ERR_ARG : 0;
    if (const int rc = check_args(keys, n, k, 1, key_type, workspace)) return rc;
    if (!out_vals || misaligned(out_vals) || !out_idx || misaligned(out_idx)) return PCMX_ERR_ARG;
    const unsigned flip = largest ? ~0u : 0u;
    const long long tiles = num_tiles(n);
    TopkWs* ws = reinterpret_cast<TopkWs*>(workspace);
    if (const int rc = select_kth(keys, n, k, key_type, flip, nullptr, ws, s)) return rc;
    // the survivors go to the outputs directly, or to the workspace when the pair sort follows
    const bool sort_after = sorted && k > 1;
    char* w = static_cast<char*>(workspace) + flag_bytes(tiles);
    unsigned* gv = sort_after ? reinterpret_cast<unsigned*>(w) : static_cast<unsigned*>(out_vals);
    unsigned* gi = sort_after ? reinterpret_cast<unsigned*>(w + align16((size_t)k * 4u)) : static_cast<unsigned*>(out_idx);
    const unsigned grid = (unsigned)(tiles < device_cus() ? tiles : device_cus());  // one resident block per CU
    const unsigned* x = static_cast<const unsigned*>(keys);
    if (key_type == PCMX_KEY_F32)
        topk_gather_kernel<PCMX_KEY_F32><<<grid, kThreads, 0, s>>>(x, gv, gi, (unsigned)n, (unsigned)k, flip, (unsigned)tiles, ws, err_flag);
    else if (key_type == PCMX_KEY_I32)
        topk_gather_kernel<PCMX_KEY_I32><<<grid, kThreads, 0, s>>>(x, gv, gi, (unsigned)n, (unsigned)k, flip, (unsigned)tiles, ws, err_flag);
    else
        topk_gather_kernel<PCMX_KEY_U32><<<grid, kThreads, 0, s>>>(x, gv, gi, (unsigned)n, (unsigned)k, flip, (unsigned)tiles, ws, err_flag);
    PCMX_HIP_RET(hipGetLastError());
    if (!sort_after) return 0;
    // canonical values transform to the same keys again, the survivors are in ascending index order and the sort is
    // stable: the result is the first k entries of the full stable sort
    return pcmx_radix_sort(gv, out_vals, gi, out_idx, k, key_type, PCMX_SORT_PAIRS, largest ? 1 : 0, 0, 32,
                           w + 2 * align16((size_t)k * 4u), err_flag, s);
}
