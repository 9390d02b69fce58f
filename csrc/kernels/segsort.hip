// Stable sort INSIDE ragged segments given by offsets (CSR row_ptr form): for every j < S the keys x[offsets[j],
// offsets[j+1]) are sorted on their own (keys, keys + a payload, keys + their flat int32 input index). The cell between
// rowsort.hip (equal-length rows) and ragged.hip (reductions over offsets): rowsort.hip's in-CU passes with (begin,
// length) read per group from the offsets, behind a front end that routes every segment by its length. No counterpart
// in the reference programs: a library addition like its neighbours. Keys are compared TRANSFORMED (radix_key.h), ranks
// are radix_rank.h's, so a segment's result equals the 1-D op (sort.hip) applied to that slice, bit for bit.
//
// Launches of one call, all on the caller's stream, none waiting for another block, no spin, no flag, no look-back:
//  0. a memset of the 256-byte workspace header (class counts, list cursors, the 16-byte summary).
//  1. count_kernel: one thread per segment: its length class, counted per wave by ballots, per block in LDS and with one
//     integer atomic per class and block on the header. It also writes the SUMMARY {segments longer than
//     PCMX_SEGSORT_MAX_LEN, the keys in them, the longest length, 0} that the host may read (16 bytes).
//  2. fill_kernel: one thread per segment again: the class lists are laid out back to back in ONE array of S ids (list
//     c starts at the sum of the counts below it, known after launch 1); a block reserves its range of a list with one
//     atomic per class on the list's cursor. The order of a list depends on the atomics' order and influences no output
//     bit: every segment is sorted on its own. A ONE-KEY segment is finished here by its thread (the key canonical as
//     from a sort, its payload); an EMPTY one needs nothing: neither spends a wave.
//     DEVIATION from "one pass over the S lengths": with one pass every class would need a list of S entries (36 S
//     bytes of workspace instead of 4 S; S may reach 2^30 - 1). The second pass re-reads 4 (S + 1) bytes.
//  3. seg_sort_kernel<G, R, NW, VALS>, one launch per class: rowsort.hip's row_sort_kernel (the same passes, the same
//     barriers, rank_row written out as there and for the reason given there) with the row taken from the class list.
//     Classes = the row sort's instantiations under its own borders: a wave per segment with R = 1, 2, 4, 8 (up to 64,
//     128, 256, 512 = PCMX_ROWSORT_WAVE_COLS keys, 4 segments per 256-thread block), a 512-thread block per segment with
//     R = 2, 4, 8, 16, 32 (up to 1024 .. 16384 = PCMX_ROWSORT_MAX_COLS keys). The launch cannot know a class's
//     population without a host sync, so each class runs a FIXED grid of kGridMult blocks per CU that strides over its
//     list up to the count launch 1 stored, read once. The loop bound is block-uniform: every thread of a block reaches
//     every barrier of every round; a group without a segment (the last round) ranks zero keys. An empty class costs a
//     launch whose blocks read one count and leave.
//  4. copy_kernel: the keys before offsets[0] and from offsets[S] on belong to no segment: they are copied through
//     with their bits unchanged, their index is their own position. The two offsets are read on the device.
//  * Every access to x and the outputs is a 4-byte access at lane-consecutive addresses: a segment starts at byte
//    4 offsets[j]. Nothing before a segment's first key or past its last is touched.
//  * Segments LONGER than PCMX_SEGSORT_MAX_LEN are counted in the summary and otherwise left alone: their part of the
//    outputs is not written. The torch layer sorts them with the device-wide kernels (ops/vector.py).
//  * The precondition 0 <= offsets[0] <= ... <= offsets[S] <= n is NOT checked. Every offset is clamped to [0, n] where
//    it is read and a negative length counts as 0, so every load and store stays inside x[0, n), the outputs [0, n),
//    offsets[0, S] and the workspace whatever the offsets hold (segments that overlap then race for their outputs: an
//    unspecified result). A list position is bounded by S and a listed length by the class capacity once more where
//    they are used, so this holds even for offsets that change between the launches.
//
// Out of scope here: packing several very short segments into one wave, a multi-block merge sort for long segments,
// ragged top-k, 64-bit keys, out= / in-place.
//
// Footprint of the instantiations (compiler metadata for gfx950) and the measurements: profiles/r20_segsort/README.md.
// The class borders are the row sort's (measured there for equal rows); kGridMult is a starting value.
#include "pcmx_common.h"
#include "pcmx_hip.h"
#include "radix_key.h"
#include "radix_rank.h"

namespace {
using pcmx::cnt_load;
using pcmx::cnt_store;
using pcmx::from_key;
using pcmx::kWave;
using pcmx::misaligned;
using pcmx::ranges_overlap;
using pcmx::to_key;

constexpr int kDigits = 256;
constexpr int kWaveSegWaves = 4;   // wave-per-segment: 4 segments per 256-thread block
constexpr int kBlockSegWaves = 8;  // block-per-segment: 512 threads
constexpr int kClasses = 9;        // capacities 64 << c, c = 0 .. 8
constexpr unsigned kMaxLen = PCMX_SEGSORT_MAX_LEN;
constexpr long long kMaxN = (1LL << 30) - 1;  // the sort family's limit (int32 positions, 30-bit counts)
constexpr int kFrontThreads = 256;
constexpr int kGridMult = 8;       // blocks per CU of a class launch (NOT MEASURED against alternatives)
constexpr int kMaxGridMult = 64;

// workspace header, in 32-bit words; the lists follow at word kHdrWords
constexpr int kCount = 0, kCursor = 16, kSummary = 32, kHdrWords = 64;
// categories of count_kernel beside the classes
constexpr int kCatLong = kClasses, kCatNone = kClasses + 1;

struct SegSortArgs {
    unsigned n, S;
    int begin_bit, end_bit;
    int key_type;
    unsigned flip;
    int iota;  // the payload is the flat position of the key (PCMX_SORT_INDEX)
};

struct Seg {
    unsigned begin, len;  // begin + len <= n
};
__device__ __forceinline__ unsigned clamp_off(int raw, unsigned n) {
    return raw < 0 ? 0u : ((unsigned)raw > n ? n : (unsigned)raw);
}
// segment j < S (the caller bounds j): both ends forced into [0, n], a negative length is 0
__device__ __forceinline__ Seg seg_of(const int* __restrict__ offsets, unsigned j, unsigned n) {
    const unsigned b = clamp_off(offsets[j], n), e = clamp_off(offsets[j + 1u], n);
    Seg s;
    s.begin = b, s.len = e > b ? e - b : 0u;
    return s;
}
// the smallest c with len <= 64 << c for 2 <= len <= kMaxLen
__device__ __forceinline__ int class_of(unsigned len) {
    const int bits = 32 - __clz((int)(len - 1u));
    return bits > 6 ? bits - 6 : 0;
}
__device__ __forceinline__ int category_of(unsigned len) {
    return len < 2u ? kCatNone : (len > kMaxLen ? kCatLong : class_of(len));
}

// ---------------------------------------------------------------- launch 1: class counts and the summary
__global__ __launch_bounds__(kFrontThreads) void count_kernel(const int* __restrict__ offsets, unsigned S, unsigned n,
                                                              unsigned* __restrict__ hdr) {
    __shared__ unsigned s_c[kClasses + 3];  // the classes, long segments, the keys in them, the longest length
    const int tid = threadIdx.x, lane = pcmx::lane_id();
    if (tid < kClasses + 3) s_c[tid] = 0u;
    __syncthreads();
    const unsigned j = blockIdx.x * (unsigned)kFrontThreads + (unsigned)tid;
    const unsigned len = j < S ? seg_of(offsets, j, n).len : 0u;
    const int cat = category_of(len);
#pragma unroll
    for (int c = 0; c <= kClasses; ++c) {
        const unsigned long long m = __ballot(cat == c);
        if (lane == 0 && m) atomicAdd(&s_c[c], (unsigned)__popcll(m));
    }
    const unsigned long_keys = pcmx::wave_reduce<unsigned, 0>(cat == kCatLong ? len : 0u);  // <= n < 2^30
    const unsigned longest = pcmx::wave_reduce<unsigned, 2>(len);
    if (lane == 0) {
        if (long_keys) atomicAdd(&s_c[kClasses + 1], long_keys);
        atomicMax(&s_c[kClasses + 2], longest);
    }
    __syncthreads();
    if (tid < kClasses + 3 && s_c[tid]) {
        if (tid < kClasses) atomicAdd(&hdr[kCount + tid], s_c[tid]);
        else if (tid == kClasses + 2) atomicMax(&hdr[kSummary + 2], s_c[tid]);
        else atomicAdd(&hdr[kSummary + (tid - kClasses)], s_c[tid]);
    }
}

// ---------------------------------------------------------------- launch 2: the class lists; one-key segments
__global__ __launch_bounds__(kFrontThreads) void fill_kernel(const unsigned* __restrict__ kin, unsigned* __restrict__ kout,
                                                             const unsigned* __restrict__ vin, unsigned* __restrict__ vout,
                                                             const int* __restrict__ offsets, unsigned* __restrict__ hdr,
                                                             unsigned* __restrict__ list, const SegSortArgs a) {
    __shared__ unsigned s_c[kClasses], s_base[kClasses];
    const int tid = threadIdx.x, lane = pcmx::lane_id();
    if (tid < kClasses) s_c[tid] = 0u;
    __syncthreads();
    const unsigned j = blockIdx.x * (unsigned)kFrontThreads + (unsigned)tid;
    Seg sg;
    sg.begin = 0u, sg.len = 0u;
    if (j < a.S) sg = seg_of(offsets, j, a.n);
    const int cat = category_of(sg.len);
    unsigned rank = 0u;  // among the block's segments of this thread's class
#pragma unroll
    for (int c = 0; c < kClasses; ++c) {
        const unsigned long long m = __ballot(cat == c);
        unsigned wbase = 0u;
        if (lane == 0 && m) wbase = atomicAdd(&s_c[c], (unsigned)__popcll(m));
        wbase = (unsigned)__builtin_amdgcn_readfirstlane((int)wbase);
        if (cat == c) rank = pcmx::lanes_below(m, wbase);
    }
    __syncthreads();
    if (tid < kClasses) {
        unsigned start = 0u;  // list tid begins behind the lists of the classes below
        for (int c = 0; c < tid; ++c) start += hdr[kCount + c];
        s_base[tid] = start + (s_c[tid] ? atomicAdd(&hdr[kCursor + tid], s_c[tid]) : 0u);
    }
    __syncthreads();
    if (cat < kClasses) {
        const unsigned pos = s_base[cat] + rank;
        if (pos < a.S) list[pos] = j;  // always true while the offsets are what launch 1 read
    } else if (sg.len == 1u) {  // sorted as it stands: the key canonical, as the sort's last store leaves it
        const unsigned b = sg.begin;  // < n
        if (kout) kout[b] = from_key(to_key(kin[b], a.key_type, a.flip), a.key_type, a.flip);
        if (vout) vout[b] = a.iota ? b : vin[b];
    }
}

// ---------------------------------------------------------------- launch 3: one class, G waves per segment
template <int G, int R, int NW, bool VALS>
__global__ __launch_bounds__(NW * kWave) void seg_sort_kernel(const unsigned* __restrict__ kin, unsigned* __restrict__ kout,
                                                              const unsigned* __restrict__ vin, unsigned* __restrict__ vout,
                                                              const int* __restrict__ offsets,
                                                              const unsigned* __restrict__ hdr,
                                                              const unsigned* __restrict__ list, const int cls,
                                                              const SegSortArgs a) {
    constexpr int kSpb = NW / G, kGroupThreads = G * kWave, kWaveItems = R * kWave, kCap = kGroupThreads * R;
    __shared__ unsigned s_keys[kSpb][kCap];                           // the segment in the order of the last pass
    __shared__ unsigned s_vals[VALS ? kSpb : 1][VALS ? kCap : 1];
    __shared__ unsigned s_cnt[NW][kDigits];    // per wave: running digit counters, then exclusive offsets in the group
    __shared__ unsigned s_toff[kSpb][kDigits];  // per segment: digit totals, then the start of each digit's run
    const int tid = threadIdx.x, lane = pcmx::lane_id(), wave = tid / kWave;
    const int grp = wave / G, gw = wave % G, gt = tid - grp * kGroupThreads;
    // this class's list and its population, stored by launches 1 and 2; read once, block-uniform
    unsigned first = 0u;
    for (int c = 0; c < cls; ++c) first += hdr[kCount + c];
    unsigned count = hdr[kCount + cls];
    first = first < a.S ? first : a.S;
    count = count < a.S - first ? count : a.S - first;  // first + count <= S: every list read is inside the list
    const unsigned lane0 = (unsigned)(gw * kWaveItems + lane);
    const int passes = (a.end_bit - a.begin_bit + 7) / 8;
    for (unsigned it = blockIdx.x * (unsigned)kSpb; it < count; it += gridDim.x * (unsigned)kSpb) {
        // the lane's first position, opaque per round: hoisted out of this loop, the R positions derived from it and
        // their LDS addresses would stay live across the whole round (R more vector registers)
        unsigned i0 = lane0;
        asm volatile("" : "+v"(i0));
        const unsigned idx = it + (unsigned)grp;
        unsigned len = 0u, begin = 0u;  // a group without a segment ranks nothing but reaches every barrier
        if (idx < count) {
            const unsigned j = list[first + idx];
            if (j < a.S) {
                const Seg sg = seg_of(offsets, j, a.n);
                len = sg.len <= (unsigned)kCap ? sg.len : 0u;  // always the length while the offsets are what launch 1 read
                begin = sg.begin;
            }
        }
        // one segment per group of whole waves: both are wave-uniform, and as scalars they cost no vector register
        const unsigned n = (unsigned)__builtin_amdgcn_readfirstlane((int)len);
        const size_t rbase = (unsigned)__builtin_amdgcn_readfirstlane((int)begin);  // only dereferenced below n
        unsigned key[R], val[VALS ? R : 1];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const unsigned i = i0 + (unsigned)(r * kWave);
            key[r] = i < n ? to_key(kin[rbase + i], a.key_type, a.flip) : 0u;
            if (VALS) val[r] = a.iota ? (unsigned)rbase + i : (i < n ? vin[rbase + i] : 0u);
        }
        for (int p = 0; p < passes; ++p) {
            const int shift = a.begin_bit + 8 * p;
            const unsigned mask = (1u << min(8, a.end_bit - shift)) - 1u;
            // ---- stable ranks inside the wave (sort.hip's ranking). The wave zeroes its own counters: their last
            //      readers (the previous pass's or round's offsets and scatter) are behind that pass's last barrier.
#pragma unroll
            for (int i = 0; i < kDigits / kWave; ++i) cnt_store(&s_cnt[wave][lane + i * kWave], 0u);
            unsigned rank[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool valid = i0 + (unsigned)(r * kWave) < n;
                const unsigned d = (key[r] >> shift) & mask;
                // radix_rank.h's rank_row, kept written out as in rowsort.hip (as a call the compiler orders the row's
                // ballots differently and the R == 1 kernels there grow by 5-7 VGPRs)
                const unsigned long long vmask = __ballot(valid);
                unsigned plo = (unsigned)vmask, phi = (unsigned)(vmask >> 32);
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const unsigned x = (unsigned)((int)(d << (31 - b)) >> 31);
                    const unsigned long long m = __ballot(x != 0u);
                    plo &= ~((unsigned)m ^ x);
                    phi &= ~((unsigned)(m >> 32) ^ x);
                }
                const unsigned below = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
                const unsigned total = (unsigned)(__popc(plo) + __popc(phi));
                const unsigned old = cnt_load(&s_cnt[wave][d]);  // every peer reads the counter before the last peer advances it
                rank[r] = old + below;
                if (valid && below + 1u == total) cnt_store(&s_cnt[wave][d], old + total);
            }
            __syncthreads();
            // ---- digit d of the segment: its count over the group's waves, and each wave's exclusive offset
            for (int d = gt; d < kDigits; d += kGroupThreads) {
                unsigned total = 0u;
#pragma unroll
                for (int w = 0; w < G; ++w) {
                    const unsigned c = s_cnt[grp * G + w][d];
                    s_cnt[grp * G + w][d] = total;
                    total += c;
                }
                s_toff[grp][d] = total;
            }
            __syncthreads();
            // ---- the segment's 256 totals scanned in place by the group's first wave (4 digits per lane)
            if (gw == 0) {
                unsigned t[4], sum = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = s_toff[grp][4 * lane + j], sum += t[j];
                unsigned inc = sum;
#pragma unroll
                for (int off = 1; off < kWave; off <<= 1) {
                    const unsigned o = __shfl_up(inc, off, kWave);
                    if (lane >= off) inc += o;
                }
                unsigned ex = inc - sum;
#pragma unroll
                for (int j = 0; j < 4; ++j) s_toff[grp][4 * lane + j] = ex, ex += t[j];
            }
            __syncthreads();
            // ---- scatter: run start of the digit + equal digits of the group's lower waves + rank in the wave (< n)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (i0 + (unsigned)(r * kWave) < n) {
                    const unsigned d = (key[r] >> shift) & mask;
                    const unsigned pos = s_toff[grp][d] + s_cnt[wave][d] + rank[r];
                    s_keys[grp][pos] = key[r];
                    if (VALS) s_vals[grp][pos] = val[r];
                }
            }
            __syncthreads();
            if (p + 1 < passes) {  // back to registers in (wave, row, lane) order; the next scatter is two barriers away
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const unsigned i = i0 + (unsigned)(r * kWave);
                    if (i < n) {
                        key[r] = s_keys[grp][i];
                        if (VALS) val[r] = s_vals[grp][i];
                    }
                }
            }
        }
        // ---- the sorted segment, transform inverted; 4-byte stores at consecutive addresses. The next round's first
        //      scatter into s_keys is three barriers away, behind every read of this loop.
        for (unsigned q = (unsigned)gt; q < n; q += (unsigned)kGroupThreads) {
            if (kout) kout[rbase + q] = from_key(s_keys[grp][q], a.key_type, a.flip);
            if (VALS) vout[rbase + q] = s_vals[grp][q];
        }
    }
}

template <int G, int R, int NW>
int launch_class(const unsigned* kin, unsigned* kout, const unsigned* vin, unsigned* vout, const int* offsets,
                 const unsigned* hdr, const unsigned* list, int cls, const SegSortArgs& a, bool vals, unsigned grid,
                 hipStream_t s) {
    if (vals) seg_sort_kernel<G, R, NW, true><<<grid, NW * kWave, 0, s>>>(kin, kout, vin, vout, offsets, hdr, list, cls, a);
    else seg_sort_kernel<G, R, NW, false><<<grid, NW * kWave, 0, s>>>(kin, kout, vin, vout, offsets, hdr, list, cls, a);
    PCMX_HIP_RET(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- launch 4: the keys outside every segment
__global__ __launch_bounds__(kFrontThreads) void copy_kernel(const unsigned* __restrict__ kin, unsigned* __restrict__ kout,
                                                             const unsigned* __restrict__ vin, unsigned* __restrict__ vout,
                                                             const int* __restrict__ offsets, const SegSortArgs a) {
    const unsigned lo = clamp_off(offsets[0], a.n);
    unsigned hi = clamp_off(offsets[a.S], a.n);
    hi = hi < lo ? lo : hi;
    const unsigned outside = lo + (a.n - hi);  // [0, lo) and [hi, n)
    const unsigned stride = gridDim.x * (unsigned)kFrontThreads;
    for (unsigned t = blockIdx.x * (unsigned)kFrontThreads + threadIdx.x; t < outside; t += stride) {
        const unsigned i = t < lo ? t : hi + (t - lo);  // < n
        if (kout) kout[i] = kin[i];
        if (vout) vout[i] = a.iota ? i : vin[i];
    }
}
}  // namespace

extern "C" long long pcmx_segment_sort_workspace_bytes(long long n, long long S) {
    (void)n;
    return (long long)pcmx::align16(((size_t)kHdrWords + (size_t)(S > 0 ? S : 0)) * 4u);
}

extern "C" int pcmx_segment_sort_b32(const void* keys_in, void* keys_out, const void* vals_in, void* vals_out, long long n,
                                     const int32_t* offsets, long long S, int key_type, int mode, int descending,
                                     int begin_bit, int end_bit, void* workspace, hipStream_t s) {
    const int mult = (mode >> 8) & 0xff;  // PCMX_SEGSORT_GRID(m): the lab's blocks per CU; 0 = kGridMult
    mode &= 0xff;
    if (n < 0 || S < 0 || n > kMaxN || S > kMaxN || mult > kMaxGridMult) return PCMX_ERR_ARG;
    if (key_type < PCMX_KEY_U32 || key_type > PCMX_KEY_F32 || mode < PCMX_SORT_KEYS || mode > PCMX_SORT_INDEX)
        return PCMX_ERR_ARG;
    if (begin_bit < 0 || end_bit > 32 || begin_bit >= end_bit) return PCMX_ERR_ARG;
    if (!offsets || misaligned(offsets, 3u) || !workspace || misaligned(workspace)) return PCMX_ERR_ARG;
    if (!keys_in || misaligned(keys_in) || misaligned(keys_out) || (!keys_out && mode != PCMX_SORT_INDEX)) return PCMX_ERR_ARG;
    if (mode == PCMX_SORT_PAIRS && (!vals_in || misaligned(vals_in))) return PCMX_ERR_ARG;
    if (mode != PCMX_SORT_KEYS && (!vals_out || misaligned(vals_out))) return PCMX_ERR_ARG;
    const size_t nb = (size_t)n * 4u, ob = (size_t)(S + 1) * 4u;
    const size_t wb = (size_t)pcmx_segment_sort_workspace_bytes(n, S);
    const bool pairs = mode == PCMX_SORT_PAIRS, has_v = mode != PCMX_SORT_KEYS;
    if (ranges_overlap(keys_out, nb, keys_in, nb) || (has_v && ranges_overlap(vals_out, nb, keys_in, nb)) ||
        (pairs && (ranges_overlap(keys_out, nb, vals_in, nb) || ranges_overlap(vals_out, nb, vals_in, nb))) ||
        (has_v && ranges_overlap(keys_out, nb, vals_out, nb)))
        return PCMX_ERR_ARG;
    if (ranges_overlap(keys_out, nb, offsets, ob) || (has_v && ranges_overlap(vals_out, nb, offsets, ob)) ||
        ranges_overlap(workspace, wb, offsets, ob) || ranges_overlap(workspace, wb, keys_in, nb) ||
        ranges_overlap(workspace, wb, keys_out, nb) || (pairs && ranges_overlap(workspace, wb, vals_in, nb)) ||
        (has_v && ranges_overlap(workspace, wb, vals_out, nb)))
        return PCMX_ERR_ARG;
    unsigned* hdr = static_cast<unsigned*>(workspace);
    PCMX_HIP_RET(hipMemsetAsync(hdr, 0, (size_t)kHdrWords * 4u, s));  // the summary is valid after every accepted call
    if (n == 0) return 0;
    SegSortArgs a;
    a.n = (unsigned)n, a.S = (unsigned)S;
    a.begin_bit = begin_bit, a.end_bit = end_bit, a.key_type = key_type, a.flip = descending ? ~0u : 0u;
    a.iota = mode == PCMX_SORT_INDEX;
    const unsigned* ki = static_cast<const unsigned*>(keys_in);
    const unsigned* vi = static_cast<const unsigned*>(vals_in);
    unsigned* ko = static_cast<unsigned*>(keys_out);
    unsigned* vo = has_v ? static_cast<unsigned*>(vals_out) : nullptr;
    const unsigned* list = hdr + kHdrWords;
    const unsigned cus = (unsigned)pcmx::device_cus();
    if (S > 0) {
        const unsigned front = (unsigned)((S + kFrontThreads - 1) / kFrontThreads);
        count_kernel<<<front, kFrontThreads, 0, s>>>(offsets, a.S, a.n, hdr);
        PCMX_HIP_RET(hipGetLastError());
        fill_kernel<<<front, kFrontThreads, 0, s>>>(ki, ko, vi, vo, offsets, hdr, hdr + kHdrWords, a);
        PCMX_HIP_RET(hipGetLastError());
        const unsigned grid = cus * (unsigned)(mult ? mult : kGridMult);
        constexpr int W = kWaveSegWaves, B = kBlockSegWaves;
        int rc = launch_class<1, 1, W>(ki, ko, vi, vo, offsets, hdr, list, 0, a, has_v, grid, s);
        if (!rc) rc = launch_class<1, 2, W>(ki, ko, vi, vo, offsets, hdr, list, 1, a, has_v, grid, s);
        if (!rc) rc = launch_class<1, 4, W>(ki, ko, vi, vo, offsets, hdr, list, 2, a, has_v, grid, s);
        if (!rc) rc = launch_class<1, 8, W>(ki, ko, vi, vo, offsets, hdr, list, 3, a, has_v, grid, s);
        if (!rc) rc = launch_class<B, 2, B>(ki, ko, vi, vo, offsets, hdr, list, 4, a, has_v, grid, s);
        if (!rc) rc = launch_class<B, 4, B>(ki, ko, vi, vo, offsets, hdr, list, 5, a, has_v, grid, s);
        if (!rc) rc = launch_class<B, 8, B>(ki, ko, vi, vo, offsets, hdr, list, 6, a, has_v, grid, s);
        if (!rc) rc = launch_class<B, 16, B>(ki, ko, vi, vo, offsets, hdr, list, 7, a, has_v, grid, s);
        if (!rc) rc = launch_class<B, 32, B>(ki, ko, vi, vo, offsets, hdr, list, 8, a, has_v, grid, s);
        if (rc) return rc;
    }
    const unsigned need = (unsigned)((n + kFrontThreads - 1) / kFrontThreads), cap = cus * 8u;
    copy_kernel<<<need < cap ? need : cap, kFrontThreads, 0, s>>>(ki, ko, vi, vo, offsets, a);
    return (int)hipGetLastError();
}
