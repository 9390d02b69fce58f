// Device-wide histograms of a flat sample stream: bincount (int32 or uint8 samples, the value is the bin, optional
// int32 weights), hist_even (float32 samples into equal-width bins of [lo, hi]) and hist_range (float32 samples into
// the bins of an ascending edge array). Generalises the 256-bin image histogram of program 4 of the reference
// (4-histogram-equalization-openmp-pthreads), which histeq.hip keeps fused with its LUT; no direct counterpart there.
//
// One persistent kernel per form, one 512-thread block per CU, no block ever waits for another: the only traffic
// between blocks is non-returning integer atomicAdd into the counts, which commutes, so every count is exact and the
// same on every call. The launcher zeroes the counts first (hipMemsetAsync) unless the call accumulates.
//  * Loads: the histeq count loop. Lane t of input slice s takes the 16-byte vectors s*512 + t + k*slices*512; a stage of
//    kLaneSamples samples per lane (8 vectors of int32 / float32, 2 of uint8) is in flight while the stage before it is
//    counted. The trip count is the block's thread 0's, so the loop is wave-uniform; a slot past the end re-reads the
//    last vector and counts nothing. The samples may start at any element: slice 0 counts the up to 15 bytes before
//    the first 16-byte boundary and the tail after the last whole vector one by one.
//  * Every sample becomes a bin number or kNoBin (0xffffffff). A negative int32 is a value >= 2^31 as unsigned. A
//    float is compared with the range IN FLOAT first (NaN fails both comparisons), and only a sample inside it is
//    converted; the result is clamped to the last bin. The edge search clamps every index it reads or returns. Then
//    EVERY add, in LDS and in global memory, is guarded by `bin < bins` once more, whatever produced the bin.
//  * Up to kLdsBins bins the block counts in LDS (96 KiB of u32 counters; below 2^31 samples they cannot overflow) and
//    merges its non-zero bins into the output at the end. The counters are replicated R times, R the largest power of
//    two <= 64 with R * (bins | 1) <= kLdsBins, else 1 (layout_of): lane l counts in copy l % R, copy c starts at word
//    c * (bins | 1). The odd stride rotates the copies over the banks, so 64 lanes that hit ONE bin hit 32 different
//    banks in each half-wave and R different addresses: 256 bins get a copy per lane, as histeq's per-lane counters.
//    The fold reads copy after copy with consecutive threads on consecutive words (conflict-free).
//  * Above kLdsBins and up to kMaxRanges * kLdsBins (1572864) bins the LDS regime goes on with the bins cut into
//    ceil(bins / kLdsBins) equal ranges: block b counts range b % ranges over input slice b / ranges and ignores every
//    other bin, so the input is read `ranges` times (about 0.12-0.16 ms per range at 2^28 int32 samples). Measured,
//    64 ranges (7.6 ms, whatever the distribution) still beat scattered global atomics (9.9 ms at 2^28 uniform samples
//    whatever the bin count, 216 ms on a zipf-like skew, whose hot bins serialise at the memory side).
//  * Above that the adds go straight to the output, one non-returning atomicAdd per live lane. A wave whose live lanes
//    all hold the same bin sends one add of the wave's total from one lane (ballot, lane read, wave sum).
//  * In both regimes a lane merges equal bins among its own consecutive samples first (Run): a sample that repeats
//    the lane's previous bin joins an open run, a new bin closes the run with one add. All samples in one bin cost one
//    add per lane in the whole kernel; the number of add instructions is the same as without merging. uint8 samples
//    close their runs inside 4 bytes (their at most 256 bins always have a counter copy per lane).
//  * hist_range keeps the edges in LDS beside the counters (at most kMaxEdgeBins + 1 floats) and finds the bin by a
//    branch-free binary search: the number of steps depends only on the number of bins.
// Measured numbers, the rejected variants and the per-kernel resources: profiles/r12_bincount/README.md.
#include "pcmx_common.h"
#include "pcmx_hip.h"

namespace {
using pcmx::device_cus;
using pcmx::kWave;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 512;         // 8 waves, one block per CU
constexpr int kLdsBins = 24576;       // u32 counter words in LDS (96 KiB): all bins of a call fit one block up to here
constexpr int kMaxRanges = 64;        // the LDS regime reaches kMaxRanges * kLdsBins bins by splitting them into ranges
constexpr int kMaxCopies = 64;        // counter copies: at most one per lane
constexpr int kMaxEdgeBins = 8192;    // hist_range: the edges (32 KiB + 4 B) sit beside the counters
constexpr int kLaneSamples = 32;      // samples per lane and pipeline stage (unweighted)
constexpr unsigned kNoBin = 0xffffffffu;
enum { kSrcI32 = 0, kSrcU8 = 1, kSrcEven = 2, kSrcRange = 3 };

struct Layout {
    int copies, stride;
};
inline Layout layout_of(int bins) {
    const int s = bins | 1;
    int r = kMaxCopies;
    while (r > 1 && r * s > kLdsBins) r >>= 1;
    return r > 1 ? Layout{r, s} : Layout{1, bins};
}

struct Args {
    const void* x;         // the samples, element-aligned
    const unsigned* w;     // int32 weights or null (then x and w are 16-byte aligned)
    unsigned* out;         // the counts
    long long n;           // samples
    long long nvec;        // whole 16-byte vectors after the head
    int head;              // samples before the first 16-byte boundary (counted by slice 0)
    unsigned bins;         // bins that can receive a sample
    int copies, stride;    // LDS layout (layout_of) of one bin range
    int ranges;            // LDS regime: bin ranges (block b counts range b % ranges of input slice b / ranges)
    unsigned span;         // bins per range
    float lo, hi, scale, fbins;  // hist_even
    const float* edges;    // hist_range: bins + 1 ascending values
    unsigned top_step;     // hist_range: the largest power of two <= bins
};

// hist_range: K samples searched side by side (K independent chains of LDS reads per step). pos is the largest index
// in [0, B] whose edge is <= v; every index read is clamped to B, the result to B - 1.
template <int K>
__device__ __forceinline__ void bins_of_range(const unsigned (&raw)[K], const Args& a, const float* s_edges, unsigned (&bin)[K]) {
    const unsigned B = a.bins;
    const float e0 = s_edges[0], eB = s_edges[B];
    unsigned pos[K];
#pragma unroll
    for (int j = 0; j < K; ++j) pos[j] = 0u;
    for (unsigned step = a.top_step; step; step >>= 1) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const unsigned c = pos[j] + step;
            const float e = s_edges[c < B ? c : B];
            pos[j] = (c <= B && e <= __uint_as_float(raw[j])) ? c : pos[j];
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float v = __uint_as_float(raw[j]);
        const unsigned p = pos[j] < B ? pos[j] : B - 1u;  // v == edges[B] belongs to the last bin
        bin[j] = (v >= e0 && v <= eB) ? p : kNoBin;       // NaN fails both comparisons
    }
}

template <int SRC>
__device__ __forceinline__ unsigned bin_of(unsigned raw, const Args& a, const float* s_edges) {
    if constexpr (SRC == kSrcI32 || SRC == kSrcU8) {
        return raw;  // a negative int32 reads as >= 2^31: never below a.bins
    } else if constexpr (SRC == kSrcEven) {
        const float v = __uint_as_float(raw);
        const float t = __fmul_rn(__fsub_rn(v, a.lo), a.scale);  // two separately rounded steps, no contraction
        const bool in = v >= a.lo && v <= a.hi && t >= 0.0f;     // NaN and +-inf fail here, before any conversion
        const float ts = in ? t : 0.0f;
        unsigned b = ts >= a.fbins ? a.bins - 1u : (unsigned)(int)ts;
        b = b < a.bins ? b : a.bins - 1u;
        return in ? b : kNoBin;
    } else {
        unsigned b[1];
        const unsigned r[1] = {raw};
        bins_of_range<1>(r, a, s_edges, b);
        return b[0];
    }
}

// One guarded add of c into bin b. The global form must be reached by all lanes of the wave together.
template <bool LDS>
__device__ __forceinline__ void add_bin(unsigned* base, unsigned bins, unsigned b, unsigned c) {
    const bool live = c != 0u && b < bins;
    if constexpr (LDS) {
        if (live) atomicAdd(base + b, c);
    } else {
        const unsigned long long act = __ballot(live);
        if (act == 0ull) return;
        const int lead = __builtin_amdgcn_readfirstlane(__builtin_ctzll(act));
        const unsigned b0 = (unsigned)__builtin_amdgcn_readlane((int)b, lead);
        if ((act & (act - 1ull)) != 0ull && __ballot(live && b == b0) == act) {  // wave-uniform
            const unsigned total = pcmx::wave_reduce<unsigned, 0>(live ? c : 0u);
            if (pcmx::lane_id() == lead) atomicAdd(base + b0, total);  // b0 < bins: the lead lane is live
        } else if (live) {
            atomicAdd(base + b, c);
        }
    }
}

// The open run of a lane: the bin of its latest sample and what it has collected for it, not yet added.
struct Run {
    unsigned bin, cnt;
};

// Four more samples of a lane, in order: a sample that repeats the bin before it joins the open run, a new bin closes
// the run with one add. Four adds per call, as without merging; the last run stays open for the next call.
template <bool LDS>
__device__ __forceinline__ void add4(unsigned* base, unsigned bins, Run& run, unsigned b0, unsigned b1, unsigned b2,
                                     unsigned b3, unsigned w0, unsigned w1, unsigned w2, unsigned w3) {
    const bool m0 = b0 == run.bin, m1 = b1 == b0, m2 = b2 == b1, m3 = b3 == b2;
    const unsigned c0 = w0 + (m0 ? run.cnt : 0u), ec = m0 ? 0u : run.cnt;
    const unsigned c1 = w1 + (m1 ? c0 : 0u), e0 = m1 ? 0u : c0;
    const unsigned c2 = w2 + (m2 ? c1 : 0u), e1 = m2 ? 0u : c1;
    const unsigned c3 = w3 + (m3 ? c2 : 0u), e2 = m3 ? 0u : c2;
    add_bin<LDS>(base, bins, run.bin, ec);
    add_bin<LDS>(base, bins, b0, e0);
    add_bin<LDS>(base, bins, b1, e1);
    add_bin<LDS>(base, bins, b2, e2);
    run.bin = b3, run.cnt = c3;
}

template <int SRC>
constexpr int vec_samples() { return SRC == kSrcU8 ? 16 : 4; }
// 16-byte sample vectors per lane and stage: kLaneSamples samples unweighted, half of that with weights (a uint8
// vector brings four weight vectors with it)
template <int SRC, bool W>
constexpr int depth_of() { return SRC == kSrcU8 ? (W ? 1 : kLaneSamples / 16) : (W ? kLaneSamples / 8 : kLaneSamples / 4); }

template <int SRC, bool W>
struct Stage {
    static constexpr int D = depth_of<SRC, W>();
    static constexpr int WV = W ? vec_samples<SRC>() / 4 : 1;  // weight vectors per sample vector
    u32x4 x[D];
    u32x4 w[D][WV];
};

template <int SRC, bool W, bool LDS>
__device__ __forceinline__ void count_vec(const u32x4& x, const u32x4 (&w)[Stage<SRC, W>::WV], bool valid, const Args& a,
                                          unsigned* base, unsigned bin0, unsigned bins, Run& run, const float* s_edges) {
    if constexpr (SRC == kSrcU8) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned word = x[q];
            const unsigned b0 = valid ? __builtin_amdgcn_ubfe(word, 0, 8) : kNoBin;
            const unsigned b1 = valid ? __builtin_amdgcn_ubfe(word, 8, 8) : kNoBin;
            const unsigned b2 = valid ? __builtin_amdgcn_ubfe(word, 16, 8) : kNoBin;
            const unsigned b3 = valid ? (word >> 24) : kNoBin;
            // bytes reach at most 256 bins, which always get a counter copy per lane: no two lanes ever meet on an
            // address, so a run is closed inside its 4 bytes (carrying it on cost 16% at 2^28 samples)
            Run r4 = {kNoBin, 0u};
            if constexpr (W)
                add4<LDS>(base, bins, r4, b0, b1, b2, b3, w[q].x, w[q].y, w[q].z, w[q].w);
            else
                add4<LDS>(base, bins, r4, b0, b1, b2, b3, 1u, 1u, 1u, 1u);
            add_bin<LDS>(base, bins, r4.bin, r4.cnt);
        }
    } else {
        // bin - bin0 wraps to a value >= bins for a bin below the block's range, and so does kNoBin
        unsigned b[4];
        if constexpr (SRC == kSrcRange) {
            const unsigned raw[4] = {x.x, x.y, x.z, x.w};
            bins_of_range<4>(raw, a, s_edges, b);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = bin_of<SRC>(x[j], a, s_edges);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = valid ? b[j] - bin0 : kNoBin;
        if constexpr (W)
            add4<LDS>(base, bins, run, b[0], b[1], b[2], b[3], w[0].x, w[0].y, w[0].z, w[0].w);
        else
            add4<LDS>(base, bins, run, b[0], b[1], b[2], b[3], 1u, 1u, 1u, 1u);
    }
}

template <int SRC, bool W, bool LDS>
__global__ __launch_bounds__(kThreads) void bincount_kernel(const Args a) {
    typedef Stage<SRC, W> S;
    constexpr int D = S::D, WV = S::WV, E = vec_samples<SRC>();
    __shared__ unsigned s_cnt[LDS ? kLdsBins : 1];
    __shared__ float s_edges[SRC == kSrcRange ? kMaxEdgeBins + 1 : 1];
    const int lane = pcmx::lane_id();
    // the block's bin range [bin0, bin0 + bins) and its slice of the input (one range and every block a slice of its
    // own unless the LDS regime is split into ranges)
    const int range = LDS ? (int)(blockIdx.x % a.ranges) : 0;
    const long long slice = LDS ? blockIdx.x / a.ranges : blockIdx.x, slices = LDS ? gridDim.x / a.ranges : gridDim.x;
    const unsigned bin0 = (unsigned)range * a.span;
    const unsigned bins = LDS ? (a.bins - bin0 < a.span ? a.bins - bin0 : a.span) : a.bins;
    unsigned* base = a.out;
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < a.copies * a.stride; i += kThreads) s_cnt[i] = 0u;
        base = s_cnt + (lane & (a.copies - 1)) * a.stride;
    }
    if constexpr (SRC == kSrcRange)
        for (unsigned i = threadIdx.x; i <= a.bins; i += kThreads) s_edges[i] = a.edges[i];
    if constexpr (LDS || SRC == kSrcRange) __syncthreads();

    const unsigned char* xb = static_cast<const unsigned char*>(a.x) + (size_t)a.head * (16 / E);
    const u32x4* xv = reinterpret_cast<const u32x4*>(xb);
    const u32x4* wv = reinterpret_cast<const u32x4*>(a.w);  // weighted: head == 0
    const long long stride = slices * kThreads;
    const long long first = slice * kThreads;  // the block's thread 0
    const long long i0 = first + threadIdx.x;
    if (first < a.nvec) {
        // vectors i0 + k * stride, k = 0 .. n-1 with n taken from the block's thread 0 (wave-uniform loop), in stages
        // of D: the next stage's loads are issued before the current one is counted
        const int n = (int)((a.nvec - 1 - first) / stride) + 1;
        Run run = {kNoBin, 0u};
        auto load =[&](S& r, int k0) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                long long idx = i0 + (long long)(k0 + d) * stride;
                idx = idx < a.nvec ? idx : a.nvec - 1;  // always a valid vector
                r.x[d] = __builtin_nontemporal_load(xv + idx);
                if constexpr (W) {
#pragma unroll
                    for (int j = 0; j < WV; ++j) r.w[d][j] = __builtin_nontemporal_load(wv + idx * WV + j);
                }
            }
        };
        auto count = [&](const S& r, int k0) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const bool valid = i0 + (long long)(k0 + d) * stride < a.nvec;
                count_vec<SRC, W, LDS>(r.x[d], r.w[d], valid, a, base, bin0, bins, run, s_edges);
            }
        };
        S ra, rb;
        load(ra, 0);
        int k = 0;
        for (;;) {
            if (k + D < n) load(rb, k + D);
            count(ra, k);
            k += D;
            if (k >= n) break;
            if (k + D < n) load(ra, k + D);
            count(rb, k);
            k += D;
            if (k >= n) break;
        }
        add_bin<LDS>(base, bins, run.bin, run.cnt);  // the lane's last open run
    }
    if (slice == 0) {
        // the samples before the first and after the last whole vector, one by one (plain guarded adds)
        const long long tail0 = a.head + a.nvec * E;
        const long long rest = a.head + (a.n - tail0);
        for (long long j = threadIdx.x; j < rest; j += kThreads) {
            const long long i = j < a.head ? j : tail0 + (j - a.head);
            unsigned raw;
            if constexpr (SRC == kSrcU8)
                raw = static_cast<const unsigned char*>(a.x)[i];
            else
                raw = static_cast<const unsigned*>(a.x)[i];
            const unsigned b = bin_of<SRC>(raw, a, s_edges) - bin0;
            const unsigned c = W ? a.w[i] : 1u;
            if (c != 0u && b < bins) atomicAdd(base + b, c);
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        // fold the copies and merge the block's non-zero bins
        for (unsigned b = threadIdx.x; b < bins; b += kThreads) {
            unsigned sum = 0u;
            for (int c = 0; c < a.copies; ++c) sum += s_cnt[c * a.stride + b];
            if (sum != 0u) atomicAdd(a.out + bin0 + b, sum);
        }
    }
}

// out_bins: entries of out (all zeroed unless accumulate); a.bins: the bins a sample can reach
template <int SRC, bool W>
int launch(Args a, long long out_bins, int accumulate, hipStream_t s) {
    constexpr int E = vec_samples<SRC>(), kElem = 16 / E;
    if (out_bins < 1 || out_bins >= (1LL << 31) || a.n >= (1LL << 31)) return PCMX_ERR_ARG;
    if (!a.out || ((uintptr_t)a.out & 3u)) return PCMX_ERR_ARG;
    if (!accumulate) PCMX_HIP_RET(hipMemsetAsync(a.out, 0, (size_t)out_bins * 4, s));
    if (a.n <= 0) return 0;
    if (!a.x || ((uintptr_t)a.x & (uintptr_t)(kElem - 1))) return PCMX_ERR_ARG;
    if (W && (((uintptr_t)a.x | (uintptr_t)a.w) & 15u)) return PCMX_ERR_ARG;
    const long long to_boundary = (long long)((16u - ((uintptr_t)a.x & 15u)) & 15u) / kElem;
    a.head = (int)(to_boundary < a.n ? to_boundary : a.n);
    a.nvec = (a.n - a.head) / E;
    const bool lds = a.bins <= (unsigned)kLdsBins * kMaxRanges;
    a.ranges = lds ? (int)((a.bins + kLdsBins - 1) / kLdsBins) : 1;
    a.span = lds ? (a.bins + a.ranges - 1) / a.ranges : a.bins;
    const Layout lay = layout_of(lds ? (int)a.span : 1);
    a.copies = lay.copies, a.stride = lay.stride;
    // one block per CU; with several bin ranges the CUs are dealt to ranges x input slices
    long long slices = (a.nvec + kThreads - 1) / kThreads;
    const int per_range = device_cus() / a.ranges > 0 ? device_cus() / a.ranges : 1;
    slices = slices < 1 ? 1 : (slices > per_range ? per_range : slices);
    const unsigned blocks = (unsigned)(slices * a.ranges);
    if (lds) {
        bincount_kernel<SRC, W, true><<<blocks, kThreads, 0, s>>>(a);
    } else {
        if constexpr (SRC == kSrcI32 || SRC == kSrcEven)
            bincount_kernel<SRC, W, false><<<blocks, kThreads, 0, s>>>(a);
        else
            return PCMX_ERR_ARG;  // uint8 samples reach 256 bins, hist_range has at most kMaxEdgeBins
    }
    return (int)hipGetLastError();
}

template <int SRC>
int launch_w(Args a, long long out_bins, int accumulate, hipStream_t s) {
    return a.w ? launch<SRC, true>(a, out_bins, accumulate, s) : launch<SRC, false>(a, out_bins, accumulate, s);
}
}  // namespace

extern "C" int pcmx_bincount_i32(const int32_t* x, const int32_t* weights, long long n, long long num_bins, int32_t* out,
                                 int accumulate, hipStream_t s) {
    Args a = {};
    a.x = x, a.w = reinterpret_cast<const unsigned*>(weights), a.out = reinterpret_cast<unsigned*>(out), a.n = n;
    a.bins = (unsigned)(num_bins > 0 && num_bins < (1LL << 31) ? num_bins : 0);
    return launch_w<kSrcI32>(a, num_bins, accumulate, s);
}

extern "C" int pcmx_bincount_u8(const unsigned char* x, const int32_t* weights, long long n, long long num_bins,
                                int32_t* out, int accumulate, hipStream_t s) {
    Args a = {};
    a.x = x, a.w = reinterpret_cast<const unsigned*>(weights), a.out = reinterpret_cast<unsigned*>(out), a.n = n;
    a.bins = (unsigned)(num_bins > 256 ? 256 : (num_bins > 0 ? num_bins : 0));  // a byte reaches no bin above 255
    return launch_w<kSrcU8>(a, num_bins, accumulate, s);
}

extern "C" int pcmx_hist_even_f32(const float* x, long long n, long long num_bins, float lo, float hi, float scale,
                                  int32_t* out, int accumulate, hipStream_t s) {
    if (!(lo < hi) || !(scale >= 0.0f) || !(scale <= 3.402823466e38f)) return PCMX_ERR_ARG;
    Args a = {};
    a.x = x, a.out = reinterpret_cast<unsigned*>(out), a.n = n;
    a.bins = (unsigned)(num_bins > 0 && num_bins < (1LL << 31) ? num_bins : 0);
    a.lo = lo, a.hi = hi, a.scale = scale, a.fbins = (float)a.bins;
    return launch<kSrcEven, false>(a, num_bins, accumulate, s);
}

extern "C" int pcmx_hist_range_f32(const float* x, long long n, const float* edges, long long num_bins, int32_t* out,
                                   int accumulate, hipStream_t s) {
    if (num_bins < 1 || num_bins > kMaxEdgeBins || !edges || ((uintptr_t)edges & 3u)) return PCMX_ERR_ARG;
    Args a = {};
    a.x = x, a.out = reinterpret_cast<unsigned*>(out), a.n = n, a.edges = edges;
    a.bins = (unsigned)num_bins;
    a.top_step = 1u;
    while (a.top_step * 2u <= a.bins) a.top_step *= 2u;
    return launch<kSrcRange, false>(a, num_bins, accumulate, s);
}
