// Row-wise stable sort, top-k and k-th key of a [rows, cols] matrix of 32-bit keys: sort.hip's in-tile digit ranking
// and topk.hip's most-significant-digit select done INSIDE one wave or one block per row. No counterpart in the
// reference programs: a library addition, the batched members of the scan / select / sort family.
//
// Nothing here talks to another block: no workspace, no flags, no look-back, no error word. A row's 256 digit counters
// are scanned where they were counted, so no block waits for another and nothing can time out. The only atomics are
// integer adds on LDS counters. Keys are compared TRANSFORMED (radix_key.h, shared with sort.hip and topk.hip), so every
// row's result equals the 1-D op applied to that row, bit for bit.
//  * row_sort_kernel<G, R, NW, VALS>: a GROUP of G waves sorts one row of up to G * R * 64 keys, NW / G rows per block.
//    G = 1 is the wave-per-row sort of short rows (4 rows per 256-thread block), G = 8 the block-per-row sort up to
//    sort.hip's 16384-key tile; the host takes the smallest R that holds the row. The row is loaded once in (wave, row,
//    lane) order, transformed, and runs ceil(bits / 8) least-significant-digit passes without leaving the CU: ranks by
//    match-any ballots on the wave's 256 LDS counters exactly as sort.hip's (radix_rank.h's rank_row, written out here;
//    cnt_load / cnt_store are that header's), the counters of the group's waves summed and scanned by the group, the
//    keys (and a payload) scattered through LDS and read back in (wave, row, lane) order.
//    After the last pass the first `keep` entries stream out of LDS with the transform inverted.
//  * Every access to global memory is a 4-byte access at lane-consecutive addresses: row r starts at byte 4 r cols,
//    which is 16-byte aligned only when cols % 4 == 0, and nothing before a row's first key or past its last is touched.
//  * A group without a row (the last block of a `rows` that does not divide) and the waves past the end of a short row
//    run the same passes on zero valid keys: every thread of the block reaches every barrier.
//  * row_select_kernel<GATHER>: one 512-thread block per row. Four most-significant-digit histogram passes over the row
//    (256 LDS counters, the digit chosen in the block behind radix_rank.h's block_excl256) give the k-th key T and
//    need_eq, the number of ties to take. For top-k one more sweep in position order follows, 512 keys per step,
//    carrying two running counts (better than T, equal to T) from step to step: the k survivors leave in ascending
//    position, values canonical, positions int32. The sweep stops at the step that stores the k-th survivor. Counters,
//    threshold and counts are per block = per row.
#include "pcmx_common.h"
#include "pcmx_hip.h"
#include "radix_key.h"
#include "radix_rank.h"

namespace {
using pcmx::block_excl256;
using pcmx::cnt_load;
using pcmx::cnt_store;
using pcmx::from_key;
using pcmx::kWave;
using pcmx::lanes_below;
using pcmx::misaligned;
using pcmx::ranges_overlap;
using pcmx::to_key;

constexpr int kDigits = 256;
constexpr int kWaveRowWaves = 4;   // wave-per-row: 4 rows per 256-thread block
constexpr int kBlockRowWaves = 8;  // block-per-row: 512 threads
constexpr long long kMaxN = (1LL << 30) - 1;  // the family's limit on rows * cols (int32 positions, 30-bit counts)

struct RowSortArgs {
    unsigned rows, cols, keep;
    int begin_bit, end_bit;
    int key_type;
    unsigned flip;
    int iota;  // the payload is the position within the row (PCMX_SORT_INDEX)
};

// ---------------------------------------------------------------- sort: G waves per row, NW / G rows per block
template <int G, int R, int NW, bool VALS>
__global__ __launch_bounds__(NW * kWave) void row_sort_kernel(const unsigned* __restrict__ kin, unsigned* __restrict__ kout,
                                                              const unsigned* __restrict__ vin, unsigned* __restrict__ vout,
                                                              const RowSortArgs a) {
    constexpr int kRpb = NW / G, kGroupThreads = G * kWave, kWaveItems = R * kWave, kCap = kGroupThreads * R;
    __shared__ unsigned s_keys[kRpb][kCap];                           // the row in the order of the last pass
    __shared__ unsigned s_vals[VALS ? kRpb : 1][VALS ? kCap : 1];
    __shared__ unsigned s_cnt[NW][kDigits];    // per wave: running digit counters, then exclusive offsets in the group
    __shared__ unsigned s_toff[kRpb][kDigits];  // per row: digit totals, then the start of each digit's run
    const int tid = threadIdx.x, lane = pcmx::lane_id(), wave = tid / kWave;
    const int grp = wave / G, gw = wave % G, gt = tid - grp * kGroupThreads;
    const unsigned row = blockIdx.x * (unsigned)kRpb + (unsigned)grp;
    const unsigned n = row < a.rows ? a.cols : 0u;  // a group without a row ranks nothing but reaches every barrier
    const size_t rbase = (size_t)row * a.cols;      // only dereferenced below n
    const unsigned i0 = (unsigned)(gw * kWaveItems + lane);
    unsigned key[R], val[VALS ? R : 1];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const unsigned i = i0 + (unsigned)(r * kWave);
        key[r] = i < n ? to_key(kin[rbase + i], a.key_type, a.flip) : 0u;
        if (VALS) val[r] = a.iota ? i : (i < n ? vin[rbase + i] : 0u);
    }
    const int passes = (a.end_bit - a.begin_bit + 7) / 8;
    for (int p = 0; p < passes; ++p) {
        const int shift = a.begin_bit + 8 * p;
        const unsigned mask = (1u << min(8, a.end_bit - shift)) - 1u;
        // ---- stable ranks inside the wave (sort.hip's ranking). The wave zeroes its own counters: their last readers
        //      (the previous pass's offsets and scatter) are behind that pass's last barrier.
#pragma unroll
        for (int i = 0; i < kDigits / kWave; ++i) cnt_store(&s_cnt[wave][lane + i * kWave], 0u);
        unsigned rank[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool valid = i0 + (unsigned)(r * kWave) < n;
            const unsigned d = (key[r] >> shift) & mask;
            // radix_rank.h's rank_row, kept written out: as a call (counters by pointer or by array reference, the
            // counter read before or after the ballots) the compiler orders the row's ballots differently and the four
            // R == 1 kernels grow by 5-7 VGPRs (34 -> 39, 36 -> 42, 40 -> 45, 40 -> 46)
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
        // ---- digit d of the row: its count over the group's waves, and each wave's exclusive offset
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
        // ---- the row's 256 totals scanned in place by the group's first wave (4 digits per lane): this is what the
        //      look-back does between tiles in sort.hip
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
    // ---- the first `keep` entries of the sorted row, transform inverted; 4-byte stores at consecutive addresses
    const unsigned m = n < a.keep ? n : a.keep;
    const size_t obase = (size_t)row * a.keep;
    for (unsigned q = (unsigned)gt; q < m; q += (unsigned)kGroupThreads) {
        if (kout) kout[obase + q] = from_key(s_keys[grp][q], a.key_type, a.flip);
        if (VALS) vout[obase + q] = s_vals[grp][q];
    }
}

template <int G, int R, int NW>
int launch_sort(const unsigned* kin, unsigned* kout, const unsigned* vin, unsigned* vout, const RowSortArgs& a, bool vals,
                hipStream_t s) {
    const unsigned grid = (a.rows + (unsigned)(NW / G) - 1u) / (unsigned)(NW / G);
    if (vals) row_sort_kernel<G, R, NW, true><<<grid, NW * kWave, 0, s>>>(kin, kout, vin, vout, a);
    else row_sort_kernel<G, R, NW, false><<<grid, NW * kWave, 0, s>>>(kin, kout, vin, vout, a);
    PCMX_HIP_RET(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- select: one block per row
constexpr int kSelWaves = 8, kSelThreads = kSelWaves * kWave;  // 512
constexpr int kSelUnroll = 4;                                  // keys per thread and histogram step

struct RowSelArgs {
    unsigned rows, cols, k;
    int key_type;
    unsigned flip;
};

template <bool GATHER>
__global__ __launch_bounds__(kSelThreads) void row_select_kernel(const unsigned* __restrict__ x, unsigned* __restrict__ out_vals,
                                                                 unsigned* __restrict__ out_idx, const RowSelArgs a) {
    __shared__ unsigned s_h[kDigits];
    __shared__ unsigned s_wsum[4];
    __shared__ unsigned s_state[2];               // {prefix, remaining k} after the pass
    __shared__ unsigned s_tot[2][2 * kSelWaves];  // two slots: a slot is rewritten two steps later, a barrier in between
    const int tid = threadIdx.x, lane = pcmx::lane_id(), wave = tid / kWave;
    const unsigned row = blockIdx.x, cols = a.cols;
    const unsigned* xr = x + (size_t)row * cols;
    // ---- the k-th key: four histogram passes, most significant digit first; every loop bound is block-uniform
    unsigned prefix = 0u, k_rem = a.k;
    for (int pass = 0; pass < 4; ++pass) {
        if (tid < kDigits) s_h[tid] = 0u;
        __syncthreads();
        const int shift = 24 - 8 * pass;
        const unsigned himask = pass == 0 ? 0u : ~0u << (shift + 8);
        for (unsigned base = 0u; base < cols; base += kSelUnroll * kSelThreads) {
            unsigned v[kSelUnroll];
#pragma unroll
            for (int j = 0; j < kSelUnroll; ++j) {
                const unsigned i = base + (unsigned)(j * kSelThreads + tid);
                v[j] = i < cols ? xr[i] : 0u;
            }
#pragma unroll
            for (int j = 0; j < kSelUnroll; ++j) {
                const unsigned i = base + (unsigned)(j * kSelThreads + tid);
                const unsigned key = to_key(v[j], a.key_type, a.flip);
                const bool match = i < cols && ((key ^ prefix) & himask) == 0u;
                const unsigned d = (key >> shift) & 0xffu;
                const unsigned d0 = (unsigned)__builtin_amdgcn_readfirstlane((int)d);
                const bool uniform = __all(match && d == d0);  // wave-uniform: one add of 64 instead of 64 collisions
                if (uniform ? lane == 0 : match) atomicAdd(&s_h[d], uniform ? (unsigned)kWave : 1u);
            }
        }
        __syncthreads();
        const unsigned c = tid < kDigits ? s_h[tid] : 0u;
        const unsigned excl = block_excl256(c, s_wsum);
        if (tid < kDigits && excl < k_rem && k_rem <= excl + c) {  // exactly one bin
            s_state[0] = prefix | ((unsigned)tid << shift);
            s_state[1] = k_rem - excl;
        }
        __syncthreads();
        prefix = s_state[0], k_rem = s_state[1];
    }
    const unsigned T = prefix, need_eq = k_rem;  // need_eq >= 1 keys equal to T are taken, by lowest position
    if (!GATHER) {
        if (tid == 0) out_vals[row] = from_key(T, a.key_type, a.flip);
        return;
    }
    // ---- the survivors in position order: exclusive ranks (gb, ge) among the better and the equal keys
    unsigned run_b = 0u, run_e = 0u;
    const size_t obase = (size_t)row * a.k;
    int slot = 0;
    for (unsigned base = 0u; base < cols; base += kSelThreads, slot ^= 1) {
        const unsigned i = base + (unsigned)tid;
        const unsigned key = to_key(i < cols ? xr[i] : 0u, a.key_type, a.flip);
        const bool better = i < cols && key < T, equal = i < cols && key == T;
        const unsigned long long bb = __ballot(better), be = __ballot(equal);
        if (lane == 0) s_tot[slot][2 * wave] = (unsigned)__popcll(bb), s_tot[slot][2 * wave + 1] = (unsigned)__popcll(be);
        __syncthreads();
        unsigned wb = 0u, we = 0u, tb = 0u, te = 0u;
#pragma unroll
        for (int w = 0; w < kSelWaves; ++w) {
            const unsigned b = s_tot[slot][2 * w], e = s_tot[slot][2 * w + 1];
            wb += w < wave ? b : 0u, we += w < wave ? e : 0u;
            tb += b, te += e;
        }
        const unsigned gb = lanes_below(bb, run_b + wb), ge = lanes_below(be, run_e + we);
        if (better || (equal && ge < need_eq)) {
            const unsigned pos = gb + min(ge, need_eq);
            if (pos < a.k) {  // always true: gb < keys better than T, and that count + need_eq == k
                out_vals[obase + pos] = from_key(key, a.key_type, a.flip);
                out_idx[obase + pos] = i;
            }
        }
        run_b += tb, run_e += te;
        if (run_b + min(run_e, need_eq) >= a.k) break;  // block-uniform: the k-th survivor is stored
    }
}

int check_shape(long long rows, long long cols) {
    if (rows < 0 || cols < 0) return PCMX_ERR_ARG;
    if (rows > 0 && cols > 0 && (rows > kMaxN || cols > kMaxN || rows * cols > kMaxN)) return PCMX_ERR_ARG;
    return 0;
}
}  // namespace

extern "C" int pcmx_row_sort_b32(const void* keys_in, void* keys_out, const void* vals_in, void* vals_out, long long rows,
                                 long long cols, long long keep, int key_type, int mode, int descending, int begin_bit,
                                 int end_bit, hipStream_t s) {
    const int route = mode & (PCMX_ROWSORT_WAVE | PCMX_ROWSORT_BLOCK);
    mode &= ~(PCMX_ROWSORT_WAVE | PCMX_ROWSORT_BLOCK);
    if (check_shape(rows, cols) || keep < 0 || keep > cols || cols > PCMX_ROWSORT_MAX_COLS) return PCMX_ERR_ARG;
    if (key_type < PCMX_KEY_U32 || key_type > PCMX_KEY_F32 || mode < PCMX_SORT_KEYS || mode > PCMX_SORT_INDEX)
        return PCMX_ERR_ARG;
    if (route == (PCMX_ROWSORT_WAVE | PCMX_ROWSORT_BLOCK)) return PCMX_ERR_ARG;
    if (route == PCMX_ROWSORT_WAVE && cols > PCMX_ROWSORT_WAVE_MAX_COLS) return PCMX_ERR_ARG;
    if (begin_bit < 0 || end_bit > 32 || begin_bit >= end_bit) return PCMX_ERR_ARG;
    if (!keys_in || misaligned(keys_in) || misaligned(keys_out) || (!keys_out && mode != PCMX_SORT_INDEX)) return PCMX_ERR_ARG;
    if (mode == PCMX_SORT_PAIRS && (!vals_in || misaligned(vals_in))) return PCMX_ERR_ARG;
    if (mode != PCMX_SORT_KEYS && (!vals_out || misaligned(vals_out))) return PCMX_ERR_ARG;
    const size_t in_b = (size_t)rows * cols * 4u, out_b = (size_t)rows * keep * 4u;
    const bool pairs = mode == PCMX_SORT_PAIRS, has_v = mode != PCMX_SORT_KEYS;
    if (ranges_overlap(keys_out, out_b, keys_in, in_b) || (has_v && ranges_overlap(vals_out, out_b, keys_in, in_b)) ||
        (pairs && (ranges_overlap(keys_out, out_b, vals_in, in_b) || ranges_overlap(vals_out, out_b, vals_in, in_b))) ||
        (has_v && ranges_overlap(keys_out, out_b, vals_out, out_b)))
        return PCMX_ERR_ARG;
    if (rows == 0 || cols == 0 || keep == 0) return 0;
    RowSortArgs a;
    a.rows = (unsigned)rows, a.cols = (unsigned)cols, a.keep = (unsigned)keep;
    a.begin_bit = begin_bit, a.end_bit = end_bit, a.key_type = key_type, a.flip = descending ? ~0u : 0u;
    a.iota = mode == PCMX_SORT_INDEX;
    const unsigned* ki = static_cast<const unsigned*>(keys_in);
    const unsigned* vi = static_cast<const unsigned*>(vals_in);
    unsigned* ko = static_cast<unsigned*>(keys_out);
    unsigned* vo = static_cast<unsigned*>(vals_out);
    const bool wave = route ? route == PCMX_ROWSORT_WAVE : cols <= PCMX_ROWSORT_WAVE_COLS;
    if (wave) {  // the smallest R with 64 R >= cols
        constexpr int W = kWaveRowWaves;
        if (cols <= 64) return launch_sort<1, 1, W>(ki, ko, vi, vo, a, has_v, s);
        if (cols <= 128) return launch_sort<1, 2, W>(ki, ko, vi, vo, a, has_v, s);
        if (cols <= 256) return launch_sort<1, 4, W>(ki, ko, vi, vo, a, has_v, s);
        if (cols <= 512) return launch_sort<1, 8, W>(ki, ko, vi, vo, a, has_v, s);
        return launch_sort<1, 16, W>(ki, ko, vi, vo, a, has_v, s);
    }
    constexpr int B = kBlockRowWaves;  // the smallest R with 512 R >= cols
    if (cols <= 512) return launch_sort<B, 1, B>(ki, ko, vi, vo, a, has_v, s);
    if (cols <= 1024) return launch_sort<B, 2, B>(ki, ko, vi, vo, a, has_v, s);
    if (cols <= 2048) return launch_sort<B, 4, B>(ki, ko, vi, vo, a, has_v, s);
    if (cols <= 4096) return launch_sort<B, 8, B>(ki, ko, vi, vo, a, has_v, s);
    if (cols <= 8192) return launch_sort<B, 16, B>(ki, ko, vi, vo, a, has_v, s);
    return launch_sort<B, 32, B>(ki, ko, vi, vo, a, has_v, s);
}

namespace {
int check_select(const void* keys, long long rows, long long cols, long long k, int key_type) {
    if (check_shape(rows, cols) || k < 0 || k > cols) return PCMX_ERR_ARG;
    if (key_type < PCMX_KEY_U32 || key_type > PCMX_KEY_F32) return PCMX_ERR_ARG;
    if (!keys || misaligned(keys)) return PCMX_ERR_ARG;
    return 0;
}
}  // namespace

extern "C" int pcmx_row_topk_b32(const void* keys, long long rows, long long cols, long long k, int key_type, int largest,
                                 void* out_vals, void* out_idx, hipStream_t s) {
    if (const int rc = check_select(keys, rows, cols, k, key_type)) return rc;
    if (!out_vals || misaligned(out_vals) || !out_idx || misaligned(out_idx)) return PCMX_ERR_ARG;
    const size_t in_b = (size_t)rows * cols * 4u, out_b = (size_t)rows * k * 4u;
    if (ranges_overlap(out_vals, out_b, keys, in_b) || ranges_overlap(out_idx, out_b, keys, in_b) ||
        ranges_overlap(out_vals, out_b, out_idx, out_b))
        return PCMX_ERR_ARG;
    if (rows == 0 || cols == 0 || k == 0) return 0;
    RowSelArgs a;
    a.rows = (unsigned)rows, a.cols = (unsigned)cols, a.k = (unsigned)k, a.key_type = key_type, a.flip = largest ? ~0u : 0u;
    row_select_kernel<true><<<(unsigned)rows, kSelThreads, 0, s>>>(static_cast<const unsigned*>(keys),
                                                                  static_cast<unsigned*>(out_vals),
                                                                  static_cast<unsigned*>(out_idx), a);
    PCMX_HIP_RET(hipGetLastError());
    return 0;
}

extern "C" int pcmx_row_kth_key_b32(const void* keys, long long rows, long long cols, long long k, int key_type, int largest,
                                    void* out, hipStream_t s) {
    if (const int rc = check_select(keys, rows, cols, k, key_type)) return rc;
    if (!out || misaligned(out)) return PCMX_ERR_ARG;
    if (ranges_overlap(out, (size_t)rows * 4u, keys, (size_t)rows * cols * 4u)) return PCMX_ERR_ARG;
    if (rows == 0 || cols == 0 || k == 0) return 0;
    RowSelArgs a;
    a.rows = (unsigned)rows, a.cols = (unsigned)cols, a.k = (unsigned)k, a.key_type = key_type, a.flip = largest ? ~0u : 0u;
    row_select_kernel<false><<<(unsigned)rows, kSelThreads, 0, s>>>(static_cast<const unsigned*>(keys),
                                                                   static_cast<unsigned*>(out), nullptr, a);
    PCMX_HIP_RET(hipGetLastError());
    return 0;
}
