// Reduction over ragged segments given by offsets (CSR row_ptr form): out[j] = op over x[offsets[j], offsets[j+1]),
// j < S, for float32 / int32 and sum / min / max; and the head flags of the same offsets for the segmented scan of
// scanbykey.hip. Merge-based segmented reduction (Merrill, Garland, "Merge-based parallel sparse matrix-vector
// multiplication", SC16) on the merge-path partition of merge.hip and the carry scheme of scanbykey.hip. No counterpart
// in the reference programs. The operator (identity, combine) and the wave scan of (flag, value) pairs that both carry
// schemes use are seg_ops.h's.
//
// With base = offsets[0], ends e_j = offsets[j+1] - base (j < S) and m = e_{S-1}, the list of ends is merged with the
// natural numbers 0 .. m-1: a path of m + S steps on which end j sits at position e_j + j and element i behind every
// end with e_j <= i. The number of ends among the first d steps is #{j : e_j + j < d}; e_j + j is strictly increasing,
// so that is one binary search. Every block takes kTile steps of the path, whatever the segment lengths are: one
// segment of 2^28, 2^28 segments of one, power-law rows and mostly empty segments all give every block the same work.
// base and m are read on the device; the host sizes the grids from the upper bound n + S.
//
//  0. partition_kernel: one thread per tile border, as in merge.hip: part[t] = ends among the first min(t * kTile,
//     m + S) steps (ntiles + 1 int32 values in the workspace).
//  1. tile_kernel: one block per tile. The tile's offsets [s0, s0 + ns] and values [v0, v0 + nv) go to LDS (ns + nv <=
//     kTile); lane l binary-searches the diagonal l * kItems of the tile in LDS and walks its kItems steps serially:
//     an element is folded into the lane's accumulator, an end closes a segment (its partial goes to LDS) and resets
//     the accumulator. A segmented scan over the 256 lanes in a fixed order (shuffles inside a wave, wave tails through
//     LDS) gives each lane's first closed segment what the lanes below hold of it. The ns results go from LDS to
//     out[s0, s0 + ns) coalesced; an empty segment gets the identity with +0.0 for a float sum. Per tile the workspace
//     gets: whether it closed a segment, and its open partial (everything after its last end, or the whole tile).
//     The first segment it closed is part[t].
//  2. carry_kernel: ONE block runs a segmented scan over the tile summaries in a fixed order: carry[t] = the open
//     partials from the nearest earlier closing tile (or tile 0) up to tile t - 1. Not hierarchical: the block walks the
//     summaries in rounds of 4096 with the running partial in a register, whatever their number (n + S < 2^31 gives at
//     most 493448 tiles, 121 rounds), so no size is refused.
//  3. fixup_kernel: out[part[t]] = op(carry[t], out[part[t]]) for every tile t >= 1 that closed a segment, one thread
//     per tile (kept apart from launch 2: there a thread would make its read-modify-writes one after another).
// No look-back, no spin loop, no float atomics, no block waits for another, no error word. A float32 sum is
// op(carry, op(lanes below, lane partial)): a fixed tree whose shape depends only on where the segment lies relative to
// the tiles, so the same input gives the same bits on every call, and a NaN or inf never leaves its segment. The
// identity of a float sum is -0.0 inside the kernels (x + -0.0 == x for every x).
//
// The precondition 0 <= offsets[0] <= ... <= offsets[S] <= n is NOT checked. Offsets that break it give an unspecified
// result, but every load and store stays inside x[0, n), offsets[0, S], out[0, S) and the workspace: every index below
// is bounded by counts, never by what an offset or a comparison returned (the arguments stand at the clamps).
//
// Measured at 2^28 float32 elements on one MI355X (profiles/r18_ragged/README.md): 0.38-0.44 ms from one segment to mean
// length 100 (equal, uniform, power-law), 0.65 / 1.13 ms at length 4 / 1 and 3.0 ms at S = 4 n, 2.1x-2.6x the time of a
// copy of the same bytes: bound by each lane's chain of 17 dependent LDS steps, not by memory. torch.segment_reduce:
// 1.75 ms at length 100, 90 ms at one segment, FASTER at 2684 segments of 10^5 (0.196 against 0.378 ms).
// kThreads x kItems = 256 x 17 is merge.hip's tile (odd item count: the lanes' private LDS positions spread over the
// banks); the tile, the item count and kCarryThreads are starting values, NOT MEASURED against alternatives.
#include "pcmx_common.h"
#include "pcmx_hip.h"
#include "seg_ops.h"

namespace {
using pcmx::combine;
using pcmx::identity;
using pcmx::kWave;
using pcmx::misaligned;
using pcmx::pad4;
using pcmx::ranges_overlap;
using pcmx::Vec4;

constexpr int kThreads = 256;
constexpr int kItems = 17;                // path steps per lane (odd: see above)
constexpr int kTile = kThreads * kItems;  // 4352 path steps per block
constexpr int kWaves = kThreads / kWave;
constexpr int kCarryThreads = 1024;
constexpr long long kMaxPath = (1LL << 31) - 1;

// base = offsets[0] forced into [0, n] and m = offsets[S] - base forced into [0, n - base]: whatever the offsets hold,
// base + m <= n, so a value index base + v with v < m is inside x[0, n).
struct Span {
    unsigned base, m;
};
__device__ __forceinline__ Span span_of(const int* __restrict__ offsets, unsigned S, unsigned n) {
    const long long b = offsets[0], last = offsets[S];
    Span sp;
    sp.base = b < 0 ? 0u : (b > (long long)n ? n : (unsigned)b);
    const long long len = last - (long long)sp.base, room = (long long)n - sp.base;
    sp.m = len < 0 ? 0u : (len > room ? (unsigned)room : (unsigned)len);
    return sp;
}
// offsets[j] - base forced into [0, m], j <= S (the caller bounds j)
__device__ __forceinline__ unsigned end_of(int raw, Span sp) {
    const long long e = (long long)raw - (long long)sp.base;
    return e < 0 ? 0u : (e > (long long)sp.m ? sp.m : (unsigned)e);
}

struct Side {
    int* part;       // ntiles + 1: ends in front of every tile border
    unsigned* flag;  // ntiles: the tile closed a segment
    void* open;      // ntiles: the tile's open partial at its end
    void* carry;     // ntiles: the open segment's partial on entry to the tile
};
__host__ __device__ inline Side side_arrays(void* ws, long long tiles) {
    Side s;
    s.part = static_cast<int*>(ws);
    s.flag = reinterpret_cast<unsigned*>(s.part + pad4(tiles + 1));
    s.open = s.flag + pad4(tiles);
    s.carry = s.flag + 2 * pad4(tiles);
    return s;
}

// ---------------------------------------------------------------- launch 0: tile borders
__global__ __launch_bounds__(kThreads) void partition_kernel(const int* __restrict__ offsets, unsigned S, unsigned n,
                                                             unsigned ntiles, int* __restrict__ part) {
    const unsigned t = blockIdx.x * kThreads + threadIdx.x;
    if (t > ntiles) return;
    const Span sp = span_of(offsets, S, n);
    const unsigned len = sp.m + S;  // <= n + S < 2^31
    const unsigned long long d64 = (unsigned long long)t * kTile;
    const unsigned d = d64 < len ? (unsigned)d64 : len;
    // Clamp: the end count of diagonal d lies in [max(0, d - m), min(d, S)]. The search never leaves that interval
    // whatever the offsets hold, so 0 <= part[t] <= S and 0 <= d - part[t] <= m. Inside the loop lo <= mid < hi <= S,
    // so offsets[mid + 1] is inside offsets[0, S].
    unsigned lo = d > sp.m ? d - sp.m : 0u, hi = d < S ? d : S;
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        if (end_of(offsets[mid + 1u], sp) + mid < d) lo = mid + 1u;  // both terms < 2^31: no wrap
        else hi = mid;
    }
    part[t] = (int)lo;
}

// ---------------------------------------------------------------- launch 1: one tile of the path
template <class T, int OP>
__global__ __launch_bounds__(kThreads) void tile_kernel(const T* __restrict__ x, unsigned n, const int* __restrict__ offsets,
                                                        unsigned S, T* __restrict__ out, const int* __restrict__ part,
                                                        unsigned* __restrict__ flag, T* __restrict__ open) {
    // s_in: the tile's ns + 1 end values e(s0 - 1) .. e(s0 + ns - 1) (offsets minus base; entry 0 is the end in front
    // of the tile, 0 for s0 == 0), then its nv values as raw bits; ns + 1 + nv <= kTile + 1, one spare word for the
    // read-ahead
    __shared__ unsigned s_in[kTile + 2];
    __shared__ T s_out[kTile];  // the partial of every end closed in the tile
    __shared__ T s_wv[kWaves];
    __shared__ unsigned s_wf[kWaves];
    const unsigned tid = threadIdx.x;
    const int lane = pcmx::lane_id(), wave = (int)(tid / kWave);
    const T id = identity<T, OP>();
    const Span sp = span_of(offsets, S, n);
    const unsigned len = sp.m + S;
    const unsigned long long d64 = (unsigned long long)blockIdx.x * kTile;
    if (d64 >= len) {  // block-uniform: the grid is sized from n + S; a tile past the path is neutral for launch 2
        if (tid == 0) {
            flag[blockIdx.x] = 0u;
            open[blockIdx.x] = id;
        }
        return;
    }
    const unsigned d0 = (unsigned)d64;
    const unsigned tile_n = len - d0 < (unsigned)kTile ? len - d0 : (unsigned)kTile;
    // Clamp: with d1 = d0 + tile_n the partition kernel guarantees max(0, d0 - m) <= s0 <= min(d0, S) and
    // max(0, d1 - m) <= s1 <= min(d1, S). Offsets out of order can still make s1 < s0 or s1 > s0 + tile_n, so s1 is
    // forced into [s0, s0 + tile_n]: then 0 <= ns <= tile_n and nv = tile_n - ns >= 0. s1 stays <= S (it is the old
    // s1, s0, or something below the old s1), v0 = d0 - s0 >= 0, and the value range ends at v0 + nv = d1 - s1 <= m
    // because s1 >= d1 - m (the old s1 is, s0 above it is, and s0 + tile_n >= d0 - m + tile_n = d1 - m). So every load
    // below is inside offsets[0, S] or x[base, base + m), which span_of keeps inside x[0, n), and every store to out
    // is inside out[s0, s1), a part of out[0, S).
    const unsigned s0 = (unsigned)part[blockIdx.x];
    unsigned s1 = (unsigned)part[blockIdx.x + 1];
    s1 = s1 < s0 ? s0 : (s1 > s0 + tile_n ? s0 + tile_n : s1);
    const unsigned ns = s1 - s0, nv = tile_n - ns, v0 = d0 - s0;

    unsigned* s_val = s_in + ns + 1u;
    const unsigned* xt = reinterpret_cast<const unsigned*>(x) + sp.base + v0;
    const unsigned* ot = reinterpret_cast<const unsigned*>(offsets);
    // All loads of the tile are issued before the first LDS store (a load behind a store in the same branch would wait
    // for memory once per round). A lane with no word in a round reads offsets[0] and drops it, so every address is
    // valid: s0 + i <= s1 <= S for an end, v0 + (i - ns - 1) < v0 + nv <= m for a value.
    unsigned w[kItems + 1];
#pragma unroll
    for (int k = 0; k <= kItems; ++k) {  // tile_n + 1 <= kTile + 1 words: one round more than kItems
        const unsigned i = tid + (unsigned)k * kThreads;
        const unsigned* src = i <= ns ? ot + s0 + i : (i <= tile_n ? xt + (i - ns - 1u) : ot);
        w[k] = __builtin_nontemporal_load(src);
    }
#pragma unroll
    for (int k = 0; k <= kItems; ++k) {
        const unsigned i = tid + (unsigned)k * kThreads;
        if (i <= tile_n) s_in[i] = i <= ns ? end_of((int)w[k], sp) : w[k];
    }
    __syncthreads();

    // ---- the lane's diagonal inside the tile: local end i closes at local value index s_in[i + 1] - v0 and sits at
    // local path position s_in[i + 1] - v0 + i. Same clamp as in partition_kernel over the tile's two ranges: ai in
    // [max(0, dl - nv), min(dl, ns)], so ai <= ns and vi = dl - ai <= nv; mid < hi <= ns keeps s_in[mid + 1] inside
    // the staged ends.
    const unsigned dl = tid * kItems < tile_n ? tid * kItems : tile_n;
    const unsigned cnt = tile_n - dl < (unsigned)kItems ? tile_n - dl : (unsigned)kItems;  // steps of this lane
    unsigned lo = dl > nv ? dl - nv : 0u, hi = dl < ns ? dl : ns;
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        // (signed: an end out of order may lie below v0; all terms are below 2^31)
        if ((long long)s_in[mid + 1u] - (long long)v0 + (long long)mid < (long long)dl) lo = mid + 1u;
        else hi = mid;
    }
    // ---- serial walk of cnt steps over ends ai in [0, ns) and values vi in [0, nv). The steps left from the lane's
    // start are (ns - ai) + (nv - vi) = tile_n - dl >= cnt, and one is consumed per step from a range that is not
    // exhausted (take_end is forced by the range checks before any end is compared), so ai < ns or vi < nv holds for
    // the side taken: positions stay inside the tile whatever the offsets are. The read-ahead s_in[ai + 1] /
    // s_val[vi] reaches word tile_n + 1 <= kTile + 1 at most, the spare word; its value is never used.
    unsigned ai = lo, vi = dl - lo;
    unsigned e = s_in[ai + 1u];                      // ai + 1 <= ns + 1 <= kTile + 1
    T v = __builtin_bit_cast(T, s_val[vi]);          // ns + 1 + vi <= tile_n + 1
    T acc = id, firstval = id;
    unsigned first = ~0u;  // the first end this lane closed
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        if ((unsigned)i < cnt) {
            const bool take_end = vi >= nv || (ai < ns && e <= v0 + vi);
            if (take_end) {
                if (first == ~0u) first = ai, firstval = acc;
                else s_out[ai] = acc;  // ai < ns <= kTile
                acc = id;
                e = s_in[++ai + 1u];
            } else {
                acc = combine<T, OP>(acc, v);
                v = __builtin_bit_cast(T, s_val[++vi]);
            }
        }
    }
    // ---- segmented scan over the lanes in a fixed order: a lane's item is (closed an end, its tail) under
    // (f1, v1) . (f2, v2) = (f1 | f2, f2 ? v2 : v1 OP v2)
    // (seg_ops.h's wave_scan_pairs / pair_of_lanes_below, kept written out in this kernel: with the two calls the
    // registers and spills stay equal but the schedule moves (4-5 s_nop fewer in four of the six kernels, one s_xor_b64
    // more in the other two), and the float32 sum over power-law rows of mean length 100 at 2^28 elements measured
    // 0.432-0.436 against 0.428-0.431 ms, and 0.427 against 0.426 ms with the run order swapped. carry_kernel below
    // takes the calls.)
    unsigned f = first != ~0u ? 1u : 0u;
    T a = acc;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const T ov = __shfl_up(a, off, kWave);
        const unsigned of = __shfl_up(f, off, kWave);
        if (lane >= off) {
            a = f ? a : combine<T, OP>(ov, a);
            f |= of;
        }
    }
    if (lane == kWave - 1) {
        s_wv[wave] = a;
        s_wf[wave] = f;
    }
    T ev = __shfl_up(a, 1, kWave);  // the item of the lanes below this one in the wave
    unsigned ef = __shfl_up(f, 1, kWave);
    if (lane == 0) {
        ev = id;
        ef = 0u;
    }
    __syncthreads();
    T pv = id;
    for (int w = 0; w < wave; ++w) pv = s_wf[w] ? s_wv[w] : combine<T, OP>(pv, s_wv[w]);  // the waves below
    const T c = ef ? ev : combine<T, OP>(pv, ev);  // what the lanes below hold of the segment open at this lane
    if (first != ~0u) s_out[first] = combine<T, OP>(c, firstval);  // first < ns
    if (tid == kThreads - 1) {
        flag[blockIdx.x] = ns != 0u ? 1u : 0u;
        open[blockIdx.x] = first != ~0u ? acc : combine<T, OP>(c, acc);
    }
    __syncthreads();

    // ---- coalesced stores: every end of the tile was consumed by exactly one lane when the offsets are in order;
    // when they are not, a word of s_out may be stale, which is an unspecified result and no fault
    const T ev0 = pcmx::positive_zero_identity<T, OP>();  // what an empty segment gets
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const unsigned i = tid + (unsigned)k * kThreads;
        if (i < ns) out[s0 + i] = s_in[i + 1u] == s_in[i] ? ev0 : s_out[i];  // s0 + i < s1 <= S
    }
}

// ---------------------------------------------------------------- launch 2: carries, one block
// A summary is the pair (closed, open partial) under the operator above, whose neutral element is (0, identity). The
// block walks the summaries in rounds of kCarryThreads x 4: a thread takes 4 neighbouring tiles with one 16-byte load
// per array (coalesced; the next round's loads are issued before this round's scan), the pairs are scanned over the
// wave by shuffles and over the waves through LDS, and `run`, the open partial on entry to the round, is carried in a
// register. The order is fixed by the tile numbers alone. The arrays are padded to a multiple of 4 entries, so the
// vector accesses stay inside the workspace; entries from ntiles on are masked to the neutral element.
template <class T, int OP>
__global__ __launch_bounds__(kCarryThreads) void carry_kernel(const unsigned* __restrict__ flag, const T* __restrict__ open,
                                                              T* __restrict__ carry, int ntiles) {
    typedef typename Vec4<T>::type V;
    constexpr int kCarryWaves = kCarryThreads / kWave;
    __shared__ T s_v[2][kCarryWaves];  // two slots: a slot is rewritten two rounds later, behind the other round's barrier
    __shared__ unsigned s_f[2][kCarryWaves];
    const int lane = pcmx::lane_id(), wave = threadIdx.x / kWave;
    const T id = identity<T, OP>();
    const int quads = (ntiles + 3) / 4, rounds = (quads + kCarryThreads - 1) / kCarryThreads;
    const pcmx::u32x4* fq = reinterpret_cast<const pcmx::u32x4*>(flag);
    const V* vq = reinterpret_cast<const V*>(open);
    T run = id;
    int q = (int)threadIdx.x;
    pcmx::u32x4 fn = {0u, 0u, 0u, 0u};
    V vn = {id, id, id, id};
    if (q < quads) fn = fq[q], vn = vq[q];
    for (int r = 0; r < rounds; ++r, q += kCarryThreads) {
        pcmx::u32x4 f4 = fn;
        V v4 = vn;
        const int qn = q + kCarryThreads;
        if (qn < quads) fn = fq[qn], vn = vq[qn];  // the next round's summaries
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q >= quads || 4 * q + j >= ntiles) f4[j] = 0u, v4[j] = id;
        unsigned f = 0u;
        T v = id;
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // this thread's 4 tiles, in order
            v = f4[j] ? v4[j] : combine<T, OP>(v, v4[j]);
            f |= f4[j];
        }
        pcmx::wave_scan_pairs<T, OP>(f, v);
        if (lane == kWave - 1) {
            s_v[r & 1][wave] = v;
            s_f[r & 1][wave] = f;
        }
        T ev;  // the pair of the threads below this one in the wave
        unsigned ef;
        pcmx::pair_of_lanes_below<T, OP>(f, v, ef, ev);
        __syncthreads();
        T pv = run, total = run;
#pragma unroll
        for (int w = 0; w < kCarryWaves; ++w) {
            if (w == wave) pv = total;  // the waves below this one, behind `run`
            total = s_f[r & 1][w] ? s_v[r & 1][w] : combine<T, OP>(total, s_v[r & 1][w]);
        }
        run = total;
        T c = ef ? ev : combine<T, OP>(pv, ev);  // the open segment's partial on entry to tile 4 q
        V c4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c4[j] = c;
            c = f4[j] ? v4[j] : combine<T, OP>(c, v4[j]);
        }
        if (q < quads) reinterpret_cast<V*>(carry)[q] = c4;  // 4 q + 3 < pad4(ntiles): inside the workspace
    }
}

// ---------------------------------------------------------------- launch 3: the first segment every tile closed
// part[t] of a tile that closed a segment is below S (tile_kernel's clamp: s0 < s1 <= S). Two closing tiles have
// different part[t] when the offsets are in order; when they are not, two threads may meet in one word of out, which
// is an unspecified result and no fault.
template <class T, int OP>
__global__ __launch_bounds__(kThreads) void fixup_kernel(T* __restrict__ out, const int* __restrict__ part,
                                                         const unsigned* __restrict__ flag, const T* __restrict__ carry,
                                                         unsigned ntiles) {
    const unsigned t = blockIdx.x * kThreads + threadIdx.x + 1u;
    if (t >= ntiles || !flag[t]) return;
    const unsigned j = (unsigned)part[t];
    out[j] = combine<T, OP>(carry[t], out[j]);
}

// ---------------------------------------------------------------- head flags of the offsets
// heads[offsets[j]] = 1 for every j <= S with 0 <= offsets[j] < n; the caller zeroed heads[0, n). Equal offsets store
// the same byte. The store is bounded by n itself, whatever the offsets hold.
__global__ __launch_bounds__(kThreads) void heads_kernel(const int* __restrict__ offsets, long long S, long long n,
                                                         unsigned char* __restrict__ heads) {
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (j > S) return;
    const long long o = offsets[j];
    if (o >= 0 && o < n) heads[o] = 1;
}

inline long long num_tiles(long long path) { return (path + kTile - 1) / kTile; }
inline size_t ws_bytes(long long tiles) { return (size_t)(pad4(tiles + 1) + 3 * pad4(tiles)) * 4; }

template <class T, int OP>
int launch_op(const T* x, long long n, const int* offsets, long long S, T* out, void* workspace, hipStream_t s) {
    const long long tiles = num_tiles(n + S);  // >= 1: S > 0
    const Side side = side_arrays(workspace, tiles);
    partition_kernel<<<(unsigned)((tiles + 1 + kThreads - 1) / kThreads), kThreads, 0, s>>>(offsets, (unsigned)S, (unsigned)n,
                                                                                           (unsigned)tiles, side.part);
    PCMX_HIP_RET(hipGetLastError());
    tile_kernel<T, OP><<<(unsigned)tiles, kThreads, 0, s>>>(x, (unsigned)n, offsets, (unsigned)S, out, side.part, side.flag,
                                                            static_cast<T*>(side.open));
    PCMX_HIP_RET(hipGetLastError());
    if (tiles > 1) {
        carry_kernel<T, OP><<<1, kCarryThreads, 0, s>>>(side.flag, static_cast<const T*>(side.open),
                                                        static_cast<T*>(side.carry), (int)tiles);
        PCMX_HIP_RET(hipGetLastError());
        fixup_kernel<T, OP><<<(unsigned)((tiles - 1 + kThreads - 1) / kThreads), kThreads, 0, s>>>(
            out, side.part, side.flag, static_cast<const T*>(side.carry), (unsigned)tiles);
    }
    return (int)hipGetLastError();
}

template <class T>
int launch(const T* x, long long n, const int32_t* offsets, long long S, int op, T* out, void* workspace, hipStream_t s) {
    if (op < PCMX_OP_SUM || op > PCMX_OP_MAX) return PCMX_ERR_ARG;
    if (n < 0 || S < 0 || n + S > kMaxPath) return PCMX_ERR_ARG;
    if (!offsets || misaligned(offsets, 3u)) return PCMX_ERR_ARG;
    if (S == 0) return 0;
    if ((n && (!x || misaligned(x, 3u))) || !out || misaligned(out) || !workspace || misaligned(workspace)) return PCMX_ERR_ARG;
    const size_t out_b = (size_t)S * 4;  // 4-byte elements throughout
    if (ranges_overlap(out, out_b, x, (size_t)n * 4) || ranges_overlap(out, out_b, offsets, (size_t)(S + 1) * 4))
        return PCMX_ERR_ARG;
    switch (op) {
        case PCMX_OP_SUM: return launch_op<T, PCMX_OP_SUM>(x, n, offsets, S, out, workspace, s);
        case PCMX_OP_MIN: return launch_op<T, PCMX_OP_MIN>(x, n, offsets, S, out, workspace, s);
        default: return launch_op<T, PCMX_OP_MAX>(x, n, offsets, S, out, workspace, s);
    }
}
}  // namespace

extern "C" long long pcmx_segment_workspace_bytes(long long n, long long S) {
    const long long path = (n > 0 ? n : 0) + (S > 0 ? S : 0);
    return (long long)pcmx::align16(ws_bytes(num_tiles(path)));
}

extern "C" int pcmx_segment_reduce_f32(const float* x, long long n, const int32_t* offsets, long long S, int op, float* out,
                                       void* workspace, hipStream_t s) {
    return launch<float>(x, n, offsets, S, op, out, workspace, s);
}

extern "C" int pcmx_segment_reduce_i32(const int32_t* x, long long n, const int32_t* offsets, long long S, int op,
                                       int32_t* out, void* workspace, hipStream_t s) {
    return launch<int>(x, n, offsets, S, op, out, workspace, s);
}

extern "C" int pcmx_segment_heads(const int32_t* offsets, long long S, long long n, unsigned char* heads, hipStream_t s) {
    if (S < 0 || n < 0 || n > kMaxPath || S > kMaxPath) return PCMX_ERR_ARG;
    if (!offsets || misaligned(offsets, 3u)) return PCMX_ERR_ARG;
    if (n == 0) return 0;
    if (!heads) return PCMX_ERR_ARG;
    PCMX_HIP_RET(hipMemsetAsync(heads, 0, (size_t)n, s));
    heads_kernel<<<(unsigned)((S + 1 + kThreads - 1) / kThreads), kThreads, 0, s>>>(offsets, S, n, heads);
    return (int)hipGetLastError();
}
