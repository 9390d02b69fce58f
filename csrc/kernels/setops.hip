// Set operations on two sorted sequences of 32-bit keys (intersection, union, difference, symmetric difference; the
// multiset rule of std::set_*), fused into one pass: the merge-path tiles of merge.hip decide per element whether it is
// kept, and the kept elements leave through select.hip's compacted store at an exact position from the decoupled
// look-back of lookback.h. No counterpart in the reference programs: a library addition beside the merge.
//
// Keys are compared only through to_key() of radix_key.h (F32 -0.0 == +0.0, every NaN one key above +inf; flip = ~0
// for descending) and are MOVED as their raw 32 bits. "Sorted" is a precondition and is not checked: with unsorted
// input the result is unspecified, but every load and store stays inside the given buffers (the arguments stand at
// the clamps).
//
// The rule. A key occurs m times in a and n times in b; the i-th occurrence in a is PAIRED with the i-th in b for
// i < min(m, n). intersection keeps the paired elements of a, difference the unpaired elements of a, union all of a
// and the unpaired elements of b, symmetric difference the unpaired elements of both. The output is the kept elements
// in the order of the merge (a tie goes to a), so inside a run of one key the merged order is: the m elements of a,
// then the n of b.
//
//  * partition_kernel: one thread per tile border t (tile t covers merged positions [t * T, (t + 1) * T)). It finds
//    the diagonal split as merge.hip does and, beside it, the counts a tile needs for the runs it sees only part of:
//    for the key kf of the first output of the tile that starts here, how many elements of a and of b BEFORE the
//    border equal kf; for the key kl of the last output of the tile that ends here, how many elements of b AFTER the
//    border equal kl. With ties going to a only a tile's first and last key can have partners outside it. Elements of
//    a after the border are never needed: an element of b has all its partners in front of it, and an element of a
//    needs the length of b's run only. So there are three bounded binary searches per border, not four. 16 bytes per
//    border in the workspace.
//  * tile_kernel: one 256-thread block per tile, claimed from the workspace's ticket (the look-back needs claim order,
//    not launch order). The tile's a and b ranges go to LDS, each lane finds its diagonal and merges its 17 positions
//    serially, as the merge does. The merge loop itself supplies what the keep bit needs. When a[i] is taken, the b
//    cursor stands on b's first element that is not below it, so with r = the rank of a[i] in its run, a[i] is paired
//    exactly when b[cursor + r] exists and has the same key: ONE LDS read per element. When b[j] is taken, the a cursor
//    stands behind a's last element that is not above it, so b[j] with rank r is paired exactly when a[cursor - 1 - r]
//    has the same key. A partner position outside the tile's range is answered by the border counts. The rank is the
//    distance to the start of the element's run, which a lane carries along its serial merge and finds for its first
//    element of each side by one binary search in LDS.
//    Which was built: neither the forward / backward segmented counts across lanes nor a search per element. The
//    partner read replaces both: it needs no traffic between lanes, no second LDS pass, and two binary searches per
//    LANE (not per element); the per-element cost over the merge is one LDS read and a compare.
//  * Compacted store: the lane's keep bits give its count, a block scan gives its place in the tile and the tile's
//    kept count, which is the tile's aggregate in the look-back (GranuleU32, lookback_publish; the workspace header and
//    granules are zeroed by hipMemsetAsync before every launch; bounded spins and the give-up report are lookback.h's;
//    a given-up look-back leaves a prefix that is never too large). Waves 1 to 3 replay their merge decisions from two
//    17-bit masks and write the LDS positions of their kept elements, compacted, while wave 0 looks back; then the
//    block streams keys (and values or indices) to out[prefix + i], coalesced. The tile that owns the last merged
//    position writes the total to count_out.
//  * Every output store is bounded by the op's capacity (min(na, nb), na, na + nb, na + nb), which sorted input never
//    exceeds, and not only by the counts the comparisons produced.
//  * The op is a kernel-uniform runtime argument (a 4-bit truth table over (from a, paired)); the mode is a template
//    parameter because the pairs mode owns a third LDS array.
#include "lookback.h"
#include "pcmx_common.h"
#include "pcmx_hip.h"
#include "radix_key.h"

namespace {
using pcmx::kFlagAgg;
using pcmx::kFlagIncl;
using pcmx::kWave;
using pcmx::misaligned;
using pcmx::to_key;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kItems = 17;                // merged positions per lane (odd: the merge's bank argument)
constexpr int kTile = kThreads * kItems;  // 4352 merged positions per block, the merge's shape
constexpr long long kMaxN = (1LL << 31) - 1;

typedef pcmx::GranuleU32 Granule;  // the tile's kept count

// What partition_kernel leaves per tile border (one 16-byte store)
struct Border {
    int a_split;    // elements of a among the first min(t * T, na + nb) merged positions
    int a_before;   // elements of a in front of the border that equal the first key of the tile starting here
    int b_before;   // elements of b in front of the border that equal it
    int b_after;    // elements of b behind the border that equal the last key of the tile ending here
};
static_assert(sizeof(Border) == 16, "one 16-byte record per border");

// keep = bit ((from_a << 1) | paired) of the op's truth table
__host__ __device__ constexpr unsigned truth_table(int op) {
    return op == PCMX_SET_INTERSECTION ? 0x8u    // a and paired
           : op == PCMX_SET_UNION      ? 0xdu    // a, or b and unpaired
           : op == PCMX_SET_DIFFERENCE ? 0x4u    // a and unpaired
                                       : 0x5u;   // unpaired
}

// First index in [lo, hi) of p whose key is not below k (hi when there is none). lo <= mid < hi in every step: the
// result and every read stay inside the interval given, whatever the comparisons return.
__device__ __forceinline__ unsigned lower_bound(const unsigned* p, unsigned lo, unsigned hi, unsigned k, int key_type,
                                                unsigned flip) {
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;  // lo + hi < 2^32: both are below 2^31
        if (to_key(p[mid], key_type, flip) < k) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// First index in [lo, hi) of p whose key is above k; same bounds
__device__ __forceinline__ unsigned upper_bound(const unsigned* p, unsigned lo, unsigned hi, unsigned k, int key_type,
                                                unsigned flip) {
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        if (to_key(p[mid], key_type, flip) <= k) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------- partition
__global__ __launch_bounds__(kThreads) void partition_kernel(const unsigned* __restrict__ a, unsigned na,
                                                             const unsigned* __restrict__ b, unsigned nb,
                                                             unsigned ntiles, Border* __restrict__ border, int key_type,
                                                             unsigned flip) {
    const unsigned t = blockIdx.x * kThreads + threadIdx.x;
    if (t > ntiles) return;
    const unsigned n = na + nb;  // < 2^31
    const unsigned long long d64 = (unsigned long long)t * kTile;
    const unsigned d = d64 < n ? (unsigned)d64 : n;
    // Clamp (merge.hip's): the a-count of diagonal d lies in [max(0, d - nb), min(d, na)] and the search never leaves
    // that interval, so 0 <= A <= na and 0 <= B = d - A <= nb. Inside the loop lo <= mid < hi gives mid < na and
    // 0 <= d - 1 - mid < nb.
    unsigned lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        const unsigned ka = to_key(a[mid], key_type, flip), kb = to_key(b[d - 1u - mid], key_type, flip);
        if (ka <= kb) lo = mid + 1u;  // a tie goes to a
        else hi = mid;
    }
    const unsigned A = lo, B = d - lo;
    Border r = {(int)A, 0, 0, 0};
    if (d < n) {  // a tile starts here; A < na or B < nb. Its first output is the smaller head, a's on a tie.
        const bool has_a = A < na, has_b = B < nb;
        const unsigned ka = has_a ? to_key(a[A], key_type, flip) : 0u, kb = has_b ? to_key(b[B], key_type, flip) : 0u;
        const unsigned kf = !has_b || (has_a && ka <= kb) ? ka : kb;
        // sorted input: everything in front of the border is <= kf, so its elements equal to kf are the tail behind
        // the lower bound. The searches stay in a[0, A) and b[0, B): both counts lie in [0, A] and [0, B].
        r.a_before = (int)(A - lower_bound(a, 0u, A, kf, key_type, flip));
        r.b_before = (int)(B - lower_bound(b, 0u, B, kf, key_type, flip));
    }
    if (d > 0u) {  // a tile ends here; A > 0 or B > 0. Its last output is the larger tail, b's on a tie.
        const bool has_a = A > 0u, has_b = B > 0u;
        const unsigned ka = has_a ? to_key(a[A - 1u], key_type, flip) : 0u;
        const unsigned kb = has_b ? to_key(b[B - 1u], key_type, flip) : 0u;
        const unsigned kl = !has_a || (has_b && kb >= ka) ? kb : ka;
        // everything behind the border is >= kl: the search stays in b[B, nb), the count lies in [0, nb - B]
        r.b_after = (int)(upper_bound(b, B, nb, kl, key_type, flip) - B);
    }
    border[t] = r;
}

// ---------------------------------------------------------------- one tile
struct SetArgs {
    const unsigned* a;   // keys
    const unsigned* b;
    const unsigned* va;  // values (pairs)
    const unsigned* vb;
    unsigned* keys_out;  // may be NULL in index mode
    unsigned* aux_out;   // values (pairs) or int32 indices into the concatenation (index)
    long long* count_out;
    pcmx::LookbackHeader* ws;  // header, then ntiles granules
    const Border* border;      // ntiles + 1 records
    unsigned* err_flag;
    unsigned na, nb, ntiles;
    unsigned cap;        // the op's capacity: no store at or past it
    int key_type;
    unsigned flip;
    unsigned truth;      // truth_table(op)
};

template <int MODE>
__global__ __launch_bounds__(kThreads) void tile_kernel(const SetArgs g) {
    constexpr bool kVals = MODE == PCMX_MERGE_PAIRS;
    __shared__ unsigned s_keys[kTile + 1];  // a range, then b range (raw bits); one spare word for the read-ahead
    __shared__ unsigned s_out[kTile];       // the LDS positions of the kept elements, compacted
    __shared__ unsigned s_vals[kVals ? kTile : 1];
    __shared__ unsigned s_wave[kWaves];
    __shared__ unsigned s_tile, s_prefix;
    const unsigned tid = threadIdx.x;
    const int lane = pcmx::lane_id(), wave = (int)(tid / kWave);
    if (tid == 0) s_tile = atomicAdd(&g.ws->ticket, 1u);
    __syncthreads();
    const unsigned tile = __builtin_amdgcn_readfirstlane(s_tile);
    if (tile >= g.ntiles) return;  // block-uniform; never taken: ntiles blocks claim from a zeroed ticket
    unsigned long long* status = reinterpret_cast<unsigned long long*>(g.ws + 1);

    const unsigned n = g.na + g.nb;
    const unsigned d0 = tile * (unsigned)kTile;  // < n
    const unsigned tile_n = n - d0 < (unsigned)kTile ? n - d0 : (unsigned)kTile;
    // Clamp (merge.hip's): partition_kernel guarantees max(0, d - nb) <= a_split <= min(d, na) at both borders.
    // Unsorted input can still make a1 < a0 or a1 > a0 + tile_n, so a1 is forced into [a0, a0 + tile_n]: then
    // 0 <= na_t <= tile_n, nb_t = tile_n - na_t >= 0, a1 <= na, b0 = d0 - a0 >= 0 and b0 + nb_t = d1 - a1 <= nb.
    // Every global load below is inside a[0, na) or b[0, nb).
    const Border bd0 = g.border[tile], bd1 = g.border[tile + 1u];
    const unsigned a0 = (unsigned)bd0.a_split;
    unsigned a1 = (unsigned)bd1.a_split;
    a1 = a1 < a0 ? a0 : (a1 > a0 + tile_n ? a0 + tile_n : a1);
    const unsigned na_t = a1 - a0, nb_t = tile_n - na_t, b0 = d0 - a0;
    const unsigned a_before = (unsigned)bd0.a_before, b_before = (unsigned)bd0.b_before, b_after = (unsigned)bd1.b_after;

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

    // ---- the keys of the tile's first and last output, as partition_kernel chose them (tile_n >= 1: one side has
    // an element; the indices read are 0, na_t <= kTile, and the last element of a non-empty range)
    const unsigned kfa = to_key(s_keys[0], g.key_type, g.flip), kfb = to_key(s_keys[na_t], g.key_type, g.flip);
    const unsigned kf = nb_t == 0u || (na_t != 0u && kfa <= kfb) ? kfa : kfb;
    const unsigned kla = to_key(s_keys[na_t ? na_t - 1u : 0u], g.key_type, g.flip);
    const unsigned klb = to_key(s_keys[tile_n - 1u], g.key_type, g.flip);
    const unsigned kl = na_t == 0u || (nb_t != 0u && klb >= kla) ? klb : kla;

    // ---- the lane's diagonal inside the tile: ai in [max(0, dl - nb_t), min(dl, na_t)] (merge.hip's clamp)
    const unsigned dl = tid * kItems < tile_n ? tid * kItems : tile_n;
    const unsigned cnt = tile_n - dl < (unsigned)kItems ? tile_n - dl : (unsigned)kItems;  // outputs of this lane
    unsigned lo = dl > nb_t ? dl - nb_t : 0u, hi = dl < na_t ? dl : na_t;
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        const unsigned ka = to_key(s_keys[mid], g.key_type, g.flip);
        const unsigned kb = to_key(s_keys[na_t + dl - 1u - mid], g.key_type, g.flip);
        if (ka <= kb) lo = mid + 1u;
        else hi = mid;
    }
    // ---- serial merge of cnt outputs from LDS positions ai in [0, na_t) and bi in [na_t, tile_n). As in merge.hip
    // take_a is forced by the range checks before any key is compared, so ai < na_t or bi < tile_n holds for the side
    // taken; the read-ahead reaches index tile_n <= kTile at most (the spare word) and its value is never used.
    const unsigned ai0 = lo, bi0 = na_t + (dl - lo);
    unsigned ai = ai0, bi = bi0;
    unsigned ka = to_key(s_keys[ai], g.key_type, g.flip), kb = to_key(s_keys[bi], g.key_type, g.flip);
    // the start of the run each head belongs to, inside the tile's range: searched in [0, ai) and [na_t, bi), and
    // only when the head exists (else the value is never used)
    unsigned a_rs = lower_bound(s_keys, 0u, ai < na_t ? ai : 0u, ka, g.key_type, g.flip);
    unsigned b_rs = lower_bound(s_keys, na_t, bi < tile_n ? bi : na_t, kb, g.key_type, g.flip);
    unsigned side = 0u, keep = 0u;  // bit i: output i came from a / is kept
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        if ((unsigned)i < cnt) {
            const bool take_a = bi >= tile_n || (ai < na_t && ka <= kb);
            bool paired;
            if (take_a) {
                // rank in a's run: a run that starts the tile's a range AND has the tile's first key goes on in front
                // of the tile. Every b below ka is taken, no b equal to it is (ties go to a), and none lies in front
                // of the tile: the partner is b's element r places behind the b cursor. Inside the tile's b range
                // (j < nb_t, LDS index na_t + j < tile_n) it is read; behind it, b continues with keys >= kl, so only
                // ka == kl can find a partner there, b_after of them.
                const unsigned r = ai - a_rs + (ka == kf ? a_before : 0u);  // < 2^31 + kTile
                const unsigned j = (bi - na_t) + r;
                paired = j < nb_t ? to_key(s_keys[na_t + j], g.key_type, g.flip) == ka : (ka == kl && j - nb_t < b_after);
            } else {
                // every a not above kb is taken: the partner is a's element r places in front of the last one taken.
                // Inside the tile's a range (r < ai, LDS index ai - 1 - r in [0, na_t)) it is read; in front of it, a
                // holds keys <= kf, so only kb == kf can find a partner there, a_before of them.
                const unsigned r = bi - b_rs + (kb == kf ? b_before : 0u);
                paired = r < ai ? to_key(s_keys[ai - 1u - r], g.key_type, g.flip) == kb : (kb == kf && r - ai < a_before);
            }
            const unsigned k = (g.truth >> ((take_a ? 2u : 0u) | (paired ? 1u : 0u))) & 1u;
            side |= (take_a ? 1u : 0u) << i;
            keep |= k << i;
            if (take_a) {
                const unsigned next = to_key(s_keys[++ai], g.key_type, g.flip);
                if (next != ka) a_rs = ai;
                ka = next;
            } else {
                const unsigned next = to_key(s_keys[++bi], g.key_type, g.flip);
                if (next != kb) b_rs = bi;
                kb = next;
            }
        }
    }

    // ---- the lane's place among the tile's kept elements, and the tile's kept count
    const unsigned mine = (unsigned)__builtin_popcount(keep);  // <= cnt
    unsigned incl = mine;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned o = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += o;
    }
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    unsigned agg = 0u, wexcl = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const unsigned c = s_wave[w];
        wexcl += w < wave ? c : 0u;
        agg += c;
    }
    agg = __builtin_amdgcn_readfirstlane(agg);  // <= tile_n: the sum of the lanes' popcounts

    // ---- publish the aggregate; wave 0 looks back while the other waves compact
    if (tid == 0)
        __hip_atomic_store(&status[tile], Granule::pack(tile == 0u ? kFlagIncl : kFlagAgg, agg), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    if (wave == 0) {
        // (after a give-up the partial prefix is <= the true one: the stores stay in front of where they belong)
        const unsigned prefix = pcmx::lookback_publish<Granule>(g.ws, status, (long long)tile, agg, g.err_flag);
        if (lane == 0) {
            s_prefix = prefix;
            if (tile == g.ntiles - 1u) {  // the owner of the last merged position
                const unsigned total = prefix + agg;  // <= na + nb < 2^31
                *g.count_out = (long long)(total < g.cap ? total : g.cap);
            }
        }
    }
    // ---- replay the merge from the two masks: kept elements' LDS positions to s_out[place ...), place + mine <= agg
    {
        unsigned pos = wexcl + incl - mine, pa = ai0, pb = bi0;
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            const unsigned p = (side >> i) & 1u ? pa++ : pb++;  // bits at or past cnt are clear in keep
            if ((keep >> i) & 1u) s_out[pos++] = p;             // p < tile_n: a position the merge loop read
        }
    }
    __syncthreads();

    // ---- coalesced stores of [0, agg) to out[prefix ...), bounded by the capacity whatever the counts say
    const unsigned prefix = __builtin_amdgcn_readfirstlane(s_prefix);
    for (unsigned i = tid; i < agg; i += kThreads) {
        const unsigned o = prefix + i;  // < 2^32: both below 2^31
        if (o < g.cap) {
            const unsigned p = s_out[i];  // < tile_n
            if (g.keys_out) g.keys_out[o] = s_keys[p];
            if constexpr (kVals) g.aux_out[o] = s_vals[p];
            else if constexpr (MODE == PCMX_MERGE_INDEX) g.aux_out[o] = p < na_t ? a0 + p : g.na + b0 + (p - na_t);
        }
    }
}

inline long long num_tiles(long long n) { return (n + kTile - 1) / kTile; }
// header + one granule per tile, padded to a multiple of 16 bytes: the block that is zeroed before every launch
inline size_t head_bytes(long long tiles) { return sizeof(pcmx::LookbackHeader) + (size_t)pcmx::pad2(tiles) * 8; }
inline size_t ws_bytes(long long tiles) { return head_bytes(tiles) + (size_t)(tiles + 1) * sizeof(Border); }

template <int MODE>
int launch(SetArgs g, Border* border, hipStream_t s) {
    partition_kernel<<<(g.ntiles + 1u + kThreads - 1u) / kThreads, kThreads, 0, s>>>(g.a, g.na, g.b, g.nb, g.ntiles,
                                                                                      border, g.key_type, g.flip);
    PCMX_HIP_RET(hipGetLastError());
    tile_kernel<MODE><<<g.ntiles, kThreads, 0, s>>>(g);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" long long pcmx_set_op_workspace_bytes(long long na, long long nb) {
    const long long n = (na > 0 ? na : 0) + (nb > 0 ? nb : 0);
    return (long long)ws_bytes(num_tiles(n));
}

extern "C" int pcmx_set_op_b32(const void* keys_a, const void* vals_a, long long na, const void* keys_b,
                               const void* vals_b, long long nb, void* keys_out, void* vals_or_idx_out,
                               long long* count_out, int op, int mode, int key_type, int descending, void* workspace,
                               long long workspace_bytes, unsigned* err_flag, hipStream_t s) {
    if (na < 0 || nb < 0 || na + nb > kMaxN) return PCMX_ERR_ARG;
    if (key_type < PCMX_KEY_U32 || key_type > PCMX_KEY_F32 || mode < PCMX_MERGE_KEYS || mode > PCMX_MERGE_INDEX)
        return PCMX_ERR_ARG;
    if (op < PCMX_SET_INTERSECTION || op > PCMX_SET_SYMDIFF) return PCMX_ERR_ARG;
    if (!count_out || misaligned(count_out, 7u)) return PCMX_ERR_ARG;
    const long long cap = op == PCMX_SET_INTERSECTION ? (na < nb ? na : nb) : (op == PCMX_SET_DIFFERENCE ? na : na + nb);
    if (cap == 0) {  // nothing can be kept: only the count is written
        PCMX_HIP_RET(hipMemsetAsync(count_out, 0, sizeof(long long), s));
        return 0;
    }
    if ((na && (!keys_a || misaligned(keys_a, 3u))) || (nb && (!keys_b || misaligned(keys_b, 3u)))) return PCMX_ERR_ARG;
    if (!workspace || misaligned(workspace) || misaligned(keys_out) || misaligned(vals_or_idx_out)) return PCMX_ERR_ARG;
    if (workspace_bytes < pcmx_set_op_workspace_bytes(na, nb)) return PCMX_ERR_ARG;
    if (!keys_out && mode != PCMX_MERGE_INDEX) return PCMX_ERR_ARG;
    if (mode != PCMX_MERGE_KEYS && !vals_or_idx_out) return PCMX_ERR_ARG;
    if (mode == PCMX_MERGE_PAIRS &&
        ((na && (!vals_a || misaligned(vals_a, 3u))) || (nb && (!vals_b || misaligned(vals_b, 3u)))))
        return PCMX_ERR_ARG;
    const long long tiles = num_tiles(na + nb);
    SetArgs g = {};
    g.a = static_cast<const unsigned*>(keys_a), g.b = static_cast<const unsigned*>(keys_b);
    g.va = static_cast<const unsigned*>(vals_a), g.vb = static_cast<const unsigned*>(vals_b);
    g.keys_out = static_cast<unsigned*>(keys_out), g.aux_out = static_cast<unsigned*>(vals_or_idx_out);
    g.count_out = count_out;
    g.ws = static_cast<pcmx::LookbackHeader*>(workspace);
    Border* border = reinterpret_cast<Border*>(static_cast<char*>(workspace) + head_bytes(tiles));
    g.border = border;
    g.err_flag = err_flag;
    g.na = (unsigned)na, g.nb = (unsigned)nb, g.ntiles = (unsigned)tiles, g.cap = (unsigned)cap;
    g.key_type = key_type, g.flip = descending ? ~0u : 0u, g.truth = truth_table(op);
    PCMX_HIP_RET(hipMemsetAsync(workspace, 0, head_bytes(tiles), s));
    if (mode == PCMX_MERGE_KEYS) return launch<PCMX_MERGE_KEYS>(g, border, s);
    if (mode == PCMX_MERGE_PAIRS) return launch<PCMX_MERGE_PAIRS>(g, border, s);
    return launch<PCMX_MERGE_INDEX>(g, border, s);
}
