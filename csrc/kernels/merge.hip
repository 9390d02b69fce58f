// Merge of two sorted sequences and sorted search (searchsorted / bucketize) of 32-bit keys, on the merge-path diagonal
// partition (Odeh, Green, Mwassi, Shmueli, Birk, "Merge Path"; Green, McColl, Bader, "GPU Merge Path"). No counterpart
// in the reference programs: a library addition beside the radix sort, for data that is already sorted.
//
// Keys are compared only through to_key() of radix_key.h (the sort's order: F32 -0.0 == +0.0, every NaN one key above
// +inf; flip = ~0 for descending) and are MOVED as their raw 32 bits: the transform is never inverted, so payloads and
// the sign of zero survive. "Sorted" means non-decreasing in that order; it is a precondition and is not checked. With
// unsorted input the result is unspecified but every load and store stays inside the given buffers: every index below
// is bounded by counts, never by what a comparison returned (the arguments stand at the clamps).
//
//  * partition_kernel: one thread per output tile border. Tile t covers outputs [t * T, (t + 1) * T), T = kTile; the
//    thread binary-searches the diagonal d = min(t * T, na + nb) for a_begin[t], the number of keys of `a` among the
//    first d outputs (b_begin[t] = d - a_begin[t]). ntiles + 1 int32 values in the caller's workspace.
//  * merge_kernel: one block per tile. Its a range and its b range (together T keys, fewer in the last tile) go to LDS
//    side by side; lane l binary-searches the diagonal l * kItems of the tile in LDS and merges its kItems outputs
//    serially from LDS; the results go back through LDS so that the global stores are coalesced. kItems = 17 is odd on
//    purpose: the lanes' private read and write positions are then spread over the 32 banks of ds_read_b32 /
//    ds_write_b32 where a power of two would put them on two banks.
//  * A tie goes to `a` (an element of a precedes an equal element of b), which makes the merge the stable sort of the
//    concatenation. The sorted-needle search runs the same two kernels with needles as `a` and the haystack as `b` and
//    writes no keys: each needle's output is the number of haystack keys merged in front of it. For right != 0 the tie
//    goes to `b` instead, so equal haystack keys are counted.
//  * search_kernel (needles in any order): a block stages kSamples evenly spaced haystack keys in LDS (the whole
//    haystack when it fits), each lane bounds its needle among the samples and finishes in the one global interval
//    that is left, with the same predicate at both levels.
// No block waits for another, there are no atomics and no error word; outputs are the same on every call.
#include "pcmx_common.h"
#include "pcmx_hip.h"
#include "radix_key.h"

namespace {
using pcmx::misaligned;
using pcmx::to_key;

constexpr int kThreads = 256;
constexpr int kItems = 17;                 // outputs per lane (odd: see above)
constexpr int kTile = kThreads * kItems;   // 4352 outputs per block
constexpr int kModeSearch = 3;             // internal: PCMX_MERGE_* plus the sorted-needle search
constexpr long long kMaxN = (1LL << 31) - 1;

constexpr int kSamples = 8192;             // haystack samples per block of search_kernel (32 KiB of LDS)
constexpr int kNeedles = 4;                // needles a lane searches side by side (independent loads in flight)
constexpr int kSearchChunk = kThreads * kNeedles;
constexpr int kSearchMinChunks = 4;        // a block takes at least this many chunks when there are enough needles

// `x` precedes `y` when x comes from a and y from b: ties go to a unless tie_b
__device__ __forceinline__ bool a_first(unsigned ka, unsigned kb, bool tie_b) { return tie_b ? ka < kb : ka <= kb; }

// ---------------------------------------------------------------- partition
__global__ __launch_bounds__(kThreads) void partition_kernel(const unsigned* __restrict__ a, unsigned na,
                                                             const unsigned* __restrict__ b, unsigned nb,
                                                             unsigned ntiles, int* __restrict__ part, int key_type,
                                                             unsigned flip, int tie_b) {
    const unsigned t = blockIdx.x * kThreads + threadIdx.x;
    if (t > ntiles) return;
    const unsigned n = na + nb;  // < 2^31
    const unsigned long long d64 = (unsigned long long)t * kTile;
    const unsigned d = d64 < n ? (unsigned)d64 : n;
    // Clamp: the a-count of diagonal d lies in [max(0, d - nb), min(d, na)]. The search never leaves that interval
    // whatever the comparisons return, so 0 <= part[t] <= na and 0 <= d - part[t] <= nb. Inside the loop
    // lo <= mid < hi gives mid < na and 0 <= d - 1 - mid < nb: both loads are inside their arrays.
    unsigned lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        const unsigned ka = to_key(a[mid], key_type, flip), kb = to_key(b[d - 1u - mid], key_type, flip);
        if (a_first(ka, kb, tie_b != 0)) lo = mid + 1u;
        else hi = mid;
    }
    part[t] = (int)lo;
}

// ---------------------------------------------------------------- merge of one tile
struct MergeArgs {
    const unsigned* a;   // keys of a (MODE search: the needles)
    const unsigned* b;   // keys of b (MODE search: the haystack)
    const unsigned* va;  // values (pairs)
    const unsigned* vb;
    unsigned* keys_out;  // may be NULL in index mode; unused in search mode
    unsigned* aux_out;   // values (pairs), int32 indices (index), int32 counts per needle (search)
    const int* part;
    unsigned na, nb;
    int key_type;
    unsigned flip;
    int tie_b;
};

template <int MODE>
__global__ __launch_bounds__(kThreads) void merge_kernel(const MergeArgs g) {
    constexpr bool kVals = MODE == PCMX_MERGE_PAIRS;
    __shared__ unsigned s_keys[kTile + 1];  // a range, then b range (raw bits); one spare word for the read-ahead
    __shared__ unsigned s_out[kTile];       // keys mode: merged raw keys; else the LDS position each output came from
    __shared__ unsigned s_vals[kVals ? kTile : 1];
    const unsigned tid = threadIdx.x;
    const unsigned n = g.na + g.nb;
    const unsigned d0 = blockIdx.x * (unsigned)kTile;  // < n: the grid has ceil(n / kTile) blocks
    const unsigned tile_n = n - d0 < (unsigned)kTile ? n - d0 : (unsigned)kTile;
    // Clamp: with d1 = d0 + tile_n the partition kernel guarantees max(0, d0 - nb) <= a0 <= min(d0, na) and
    // max(0, d1 - nb) <= a1 <= min(d1, na). Unsorted input can still make a1 < a0 or a1 > a0 + tile_n, so a1 is forced
    // into [a0, a0 + tile_n]: then 0 <= na_t <= tile_n and nb_t = tile_n - na_t >= 0. a1 stays <= na (it is the old
    // a1, a0, or something below the old a1), b0 = d0 - a0 >= 0, and the b range ends at b0 + nb_t = d1 - a1 <= nb
    // because a1 >= d1 - nb (the old a1 is, a0 above it is, and a0 + tile_n >= d0 - nb + tile_n = d1 - nb). Every global
    // load below is therefore inside a[0, na) or b[0, nb).
    const unsigned a0 = (unsigned)g.part[blockIdx.x];
    unsigned a1 = (unsigned)g.part[blockIdx.x + 1];
    a1 = a1 < a0 ? a0 : (a1 > a0 + tile_n ? a0 + tile_n : a1);
    const unsigned na_t = a1 - a0, nb_t = tile_n - na_t, b0 = d0 - a0;

#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const unsigned i = tid + (unsigned)k * kThreads;
        if (i < tile_n) {
            const bool from_a = i < na_t;
            const unsigned* src = from_a ? g.a + a0 + i : g.b + b0 + (i - na_t);
            s_keys[i] = __builtin_nontemporal_load(src);
            if constexpr (kVals) {
                const unsigned* vsrc = from_a ? g.va + a0 + i : g.vb + b0 + (i - na_t);
                s_vals[i] = __builtin_nontemporal_load(vsrc);
            }
        }
    }
    __syncthreads();

    // ---- the lane's diagonal inside the tile. Same clamp as in partition_kernel, over the tile's two LDS ranges:
    // ai in [max(0, dl - nb_t), min(dl, na_t)], so ai <= na_t and bi = dl - ai <= nb_t.
    const unsigned dl = tid * kItems < tile_n ? tid * kItems : tile_n;
    const unsigned cnt = tile_n - dl < (unsigned)kItems ? tile_n - dl : (unsigned)kItems;  // outputs of this lane
    unsigned lo = dl > nb_t ? dl - nb_t : 0u, hi = dl < na_t ? dl : na_t;
    const bool tie_b = g.tie_b != 0;
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        const unsigned ka = to_key(s_keys[mid], g.key_type, g.flip);
        const unsigned kb = to_key(s_keys[na_t + dl - 1u - mid], g.key_type, g.flip);
        if (a_first(ka, kb, tie_b)) lo = mid + 1u;
        else hi = mid;
    }
    // ---- serial merge of cnt outputs from LDS positions ai in [0, na_t) and bi in [na_t, tile_n). The keys left from
    // the lane's start are (na_t - ai) + (tile_n - bi) = tile_n - dl >= cnt, and one is consumed per step from a range
    // that is not exhausted (take_a is forced by the range checks before any key is compared), so ai < na_t or
    // bi < tile_n holds for the side taken: positions stay inside the tile whatever the keys are. The read-ahead
    // s_keys[ai + 1] / s_keys[bi + 1] reaches index tile_n <= kTile at most, the spare word; its value is never used.
    unsigned ai = lo, bi = na_t + (dl - lo);
    unsigned ra = s_keys[ai], rb = s_keys[bi];  // ai <= na_t <= kTile, bi <= tile_n <= kTile
    unsigned ka = to_key(ra, g.key_type, g.flip), kb = to_key(rb, g.key_type, g.flip);
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        if ((unsigned)i < cnt) {
            const bool take_a = bi >= tile_n || (ai < na_t && a_first(ka, kb, tie_b));
            if constexpr (MODE == kModeSearch) {
                if (take_a) s_out[ai] = b0 + (bi - na_t);  // haystack keys merged in front of needle a0 + ai
            } else if constexpr (MODE == PCMX_MERGE_KEYS) {
                s_out[dl + i] = take_a ? ra : rb;
            } else {
                s_out[dl + i] = take_a ? ai : bi;
            }
            if (take_a) {
                ra = s_keys[++ai];
                ka = to_key(ra, g.key_type, g.flip);
            } else {
                rb = s_keys[++bi];
                kb = to_key(rb, g.key_type, g.flip);
            }
        }
    }
    __syncthreads();

    // ---- coalesced stores
    if constexpr (MODE == kModeSearch) {
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const unsigned i = tid + (unsigned)k * kThreads;
            if (i < na_t) g.aux_out[a0 + i] = s_out[i];  // a0 + na_t <= na: inside the needles' output
        }
    } else {
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const unsigned i = tid + (unsigned)k * kThreads;
            if (i < tile_n) {  // d0 + i < n
                if constexpr (MODE == PCMX_MERGE_KEYS) {
                    g.keys_out[d0 + i] = s_out[i];
                } else {
                    const unsigned p = s_out[i];  // < tile_n (above)
                    if (g.keys_out) g.keys_out[d0 + i] = s_keys[p];
                    if constexpr (kVals) g.aux_out[d0 + i] = s_vals[p];
                    else g.aux_out[d0 + i] = p < na_t ? a0 + p : g.na + b0 + (p - na_t);
                }
            }
        }
    }
}

// ---------------------------------------------------------------- sorted search, needles in any order
// lower bound (right == 0: keys < k) or upper bound (keys <= k) of k in keys[base, base + len), `steps` halvings
// (2^steps > the largest len of any lane, so the loop count is uniform and kNeedles searches run side by side).
// Invariant: base + len never grows past its initial value and a probe base + len / 2 is read only while len > 0,
// so every read is inside [base, base + len) of the initial interval.
template <class Load>
__device__ __forceinline__ void bound_search(unsigned (&base)[kNeedles], unsigned (&len)[kNeedles],
                                             const unsigned (&k)[kNeedles], int steps, bool right, Load load) {
    for (int s = 0; s < steps; ++s) {
#pragma unroll
        for (int j = 0; j < kNeedles; ++j) {
            const unsigned half = len[j] >> 1;
            if (len[j] != 0u) {
                const unsigned v = load(base[j] + half);
                const bool before = right ? v <= k[j] : v < k[j];
                base[j] = before ? base[j] + half + 1u : base[j];
                len[j] = before ? len[j] - half - 1u : half;
            }
        }
    }
}

__device__ __forceinline__ int steps_for(unsigned len) { return 32 - __clz((int)len); }  // 2^steps > len

__global__ __launch_bounds__(kThreads) void search_kernel(const unsigned* __restrict__ hay, unsigned n,
                                                          const unsigned* __restrict__ needles, unsigned m,
                                                          int* __restrict__ out, int key_type, unsigned flip, int right_,
                                                          unsigned stride, unsigned ns, unsigned chunks_per_block) {
    __shared__ unsigned s_samp[kSamples];  // transformed keys of hay[j * stride], j < ns <= kSamples
    const unsigned tid = threadIdx.x;
    const bool right = right_ != 0;
    for (unsigned j = tid; j < ns; j += kThreads) {
        const unsigned long long p = (unsigned long long)j * stride;  // < n: ns = ceil(n / stride)
        s_samp[j] = to_key(hay[p], key_type, flip);
    }
    __syncthreads();
    const int lds_steps = steps_for(ns), glob_steps = steps_for(stride);
    const unsigned long long first = (unsigned long long)blockIdx.x * chunks_per_block * kSearchChunk;
    for (unsigned c = 0; c < chunks_per_block; ++c) {
        const unsigned long long i0 = first + (unsigned long long)c * kSearchChunk + tid;
        if (i0 - tid >= m) break;  // block-uniform
        unsigned k[kNeedles], base[kNeedles], len[kNeedles];
#pragma unroll
        for (int j = 0; j < kNeedles; ++j) {
            const unsigned long long i = i0 + (unsigned long long)j * kThreads;
            k[j] = i < m ? to_key(__builtin_nontemporal_load(needles + i), key_type, flip) : 0u;
            base[j] = 0u, len[j] = i < m ? ns : 0u;
        }
        bound_search(base, len, k, lds_steps, right, [&](unsigned p) { return s_samp[p]; });
        // base[j] = c samples precede the needle (in the sense of `right`): hay[(c - 1) * stride] precedes it and
        // hay[c * stride] does not, so the answer lies in ((c - 1) * stride, min(c * stride, n)], and the same
        // predicate over that interval finds it. c == 0 leaves the empty interval at 0.
#pragma unroll
        for (int j = 0; j < kNeedles; ++j) {
            const unsigned cs = base[j];  // <= ns
            const unsigned long long top = (unsigned long long)cs * stride;
            const unsigned end = top < n ? (unsigned)top : n;
            base[j] = cs == 0u ? 0u : (cs - 1u) * stride + 1u;  // <= end: (cs - 1) * stride < n
            len[j] = i0 + (unsigned long long)j * kThreads < m ? end - base[j] : 0u;
        }
        bound_search(base, len, k, glob_steps, right, [&](unsigned p) { return to_key(hay[p], key_type, flip); });
#pragma unroll
        for (int j = 0; j < kNeedles; ++j) {
            const unsigned long long i = i0 + (unsigned long long)j * kThreads;
            if (i < m) out[i] = (int)base[j];
        }
    }
}

inline long long num_tiles(long long n) { return (n + kTile - 1) / kTile; }
inline bool key_type_ok(int t) { return t >= PCMX_KEY_U32 && t <= PCMX_KEY_F32; }

// partition + merge of (a, na) and (b, nb); part holds num_tiles + 1 ints
template <int MODE>
int launch_merge(MergeArgs g, int* part, hipStream_t s) {
    const long long tiles = num_tiles((long long)g.na + g.nb);
    g.part = part;
    partition_kernel<<<(unsigned)((tiles + 1 + kThreads - 1) / kThreads), kThreads, 0, s>>>(
        g.a, g.na, g.b, g.nb, (unsigned)tiles, part, g.key_type, g.flip, g.tie_b);
    PCMX_HIP_RET(hipGetLastError());
    merge_kernel<MODE><<<(unsigned)tiles, kThreads, 0, s>>>(g);
    return (int)hipGetLastError();
}

// The sorted-needle route merges m + n keys and needs m + n < 2^31; a larger pair takes the general route. So do few
// needles in a long haystack, where reading the whole haystack costs more than a search per needle: measured at
// n = 2^28, the merge route took 0.86 ms for m = 2^20 and 2.18 ms for m = 2^28, the general route on the same sorted
// needles 0.18 and 8.2 ms (profiles/r14_merge/README.md); a straight line through each pair crosses near m = n / 10.
// Both routes give the same result, so the rule only picks the faster one.
constexpr long long kMergeRouteRatio = 8;
inline bool merge_route(long long n, long long m, int needles_sorted) {
    return needles_sorted && n + m <= kMaxN && kMergeRouteRatio * m >= n;
}
}  // namespace

extern "C" long long pcmx_merge_workspace_bytes(long long na, long long nb) {
    const long long n = (na > 0 ? na : 0) + (nb > 0 ? nb : 0);
    return (long long)pcmx::align16((size_t)(num_tiles(n) + 1) * sizeof(int));
}

extern "C" int pcmx_merge_b32(const void* keys_a, const void* vals_a, long long na, const void* keys_b,
                              const void* vals_b, long long nb, void* keys_out, void* vals_or_idx_out, int key_type,
                              int mode, int descending, void* workspace, hipStream_t s) {
    if (na < 0 || nb < 0 || na + nb > kMaxN) return PCMX_ERR_ARG;
    if (!key_type_ok(key_type) || mode < PCMX_MERGE_KEYS || mode > PCMX_MERGE_INDEX) return PCMX_ERR_ARG;
    if (na + nb == 0) return 0;
    if ((na && (!keys_a || misaligned(keys_a, 3u))) || (nb && (!keys_b || misaligned(keys_b, 3u)))) return PCMX_ERR_ARG;
    if (!workspace || misaligned(workspace) || misaligned(keys_out) || misaligned(vals_or_idx_out)) return PCMX_ERR_ARG;
    if (!keys_out && mode != PCMX_MERGE_INDEX) return PCMX_ERR_ARG;
    if (mode != PCMX_MERGE_KEYS && !vals_or_idx_out) return PCMX_ERR_ARG;
    if (mode == PCMX_MERGE_PAIRS &&
        ((na && (!vals_a || misaligned(vals_a, 3u))) || (nb && (!vals_b || misaligned(vals_b, 3u)))))
        return PCMX_ERR_ARG;
    MergeArgs g = {};
    g.a = static_cast<const unsigned*>(keys_a), g.b = static_cast<const unsigned*>(keys_b);
    g.va = static_cast<const unsigned*>(vals_a), g.vb = static_cast<const unsigned*>(vals_b);
    g.keys_out = static_cast<unsigned*>(keys_out), g.aux_out = static_cast<unsigned*>(vals_or_idx_out);
    g.na = (unsigned)na, g.nb = (unsigned)nb;
    g.key_type = key_type, g.flip = descending ? ~0u : 0u, g.tie_b = 0;
    int* part = static_cast<int*>(workspace);
    if (mode == PCMX_MERGE_KEYS) return launch_merge<PCMX_MERGE_KEYS>(g, part, s);
    if (mode == PCMX_MERGE_PAIRS) return launch_merge<PCMX_MERGE_PAIRS>(g, part, s);
    return launch_merge<PCMX_MERGE_INDEX>(g, part, s);
}

extern "C" long long pcmx_searchsorted_workspace_bytes(long long n, long long m, int needles_sorted) {
    if (n < 0 || m < 0 || !merge_route(n, m, needles_sorted)) return 16;
    return pcmx_merge_workspace_bytes(m, n);
}

extern "C" int pcmx_searchsorted_b32(const void* sorted_keys, long long n, const void* needles, long long m,
                                     int32_t* out, int key_type, int right, int descending, int needles_sorted,
                                     void* workspace, hipStream_t s) {
    if (n < 0 || m < 0 || n > kMaxN || m > kMaxN || !key_type_ok(key_type)) return PCMX_ERR_ARG;
    if (m == 0) return 0;
    if (!needles || misaligned(needles, 3u) || !out || misaligned(out)) return PCMX_ERR_ARG;
    if (n && (!sorted_keys || misaligned(sorted_keys, 3u))) return PCMX_ERR_ARG;
    if (!workspace || misaligned(workspace)) return PCMX_ERR_ARG;
    const unsigned flip = descending ? ~0u : 0u;
    if (merge_route(n, m, needles_sorted)) {
        MergeArgs g = {};
        g.a = static_cast<const unsigned*>(needles), g.b = static_cast<const unsigned*>(sorted_keys);
        g.aux_out = reinterpret_cast<unsigned*>(out);
        g.na = (unsigned)m, g.nb = (unsigned)n;
        g.key_type = key_type, g.flip = flip, g.tie_b = right ? 1 : 0;
        return launch_merge<kModeSearch>(g, static_cast<int*>(workspace), s);
    }
    // samples hay[j * stride], j < ns: the whole haystack (stride 1) when it fits
    const unsigned stride = (unsigned)((n + kSamples - 1) / kSamples > 1 ? (n + kSamples - 1) / kSamples : 1);
    const unsigned ns = (unsigned)((n + stride - 1) / stride);  // <= kSamples
    const long long chunks = (m + kSearchChunk - 1) / kSearchChunk;
    // enough needles per block to pay for its samples; about 8 blocks per CU when there are many
    long long per_block = (chunks + 8LL * pcmx::device_cus() - 1) / (8LL * pcmx::device_cus());
    if (per_block < kSearchMinChunks) per_block = kSearchMinChunks;
    const long long blocks = (chunks + per_block - 1) / per_block;
    search_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(static_cast<const unsigned*>(sorted_keys), (unsigned)n,
                                                        static_cast<const unsigned*>(needles), (unsigned)m, out, key_type,
                                                        flip, right ? 1 : 0, stride, ns, (unsigned)per_block);
    return (int)hipGetLastError();
}
