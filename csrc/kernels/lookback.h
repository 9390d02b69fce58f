// The decoupled look-back shared by scan.hip, select.hip, segreduce.hip, topk.hip and sort.hip: the workspace
// header, the granule flags, the bounded spin and its give-up report, and the wave-wide look-back loop itself.
//
// Protocol: tile t publishes {kFlagAgg, its own aggregate} (tile 0: kFlagIncl), sums its predecessors' granules back
// to the first kFlagIncl one, then republishes {kFlagIncl, prefix + aggregate}. A granule is data + flag in ONE relaxed
// agent-scope atomic store and is polled with relaxed agent-scope loads; flag 0 is "not published yet" (the
// workspace is zeroed by a hipMemsetAsync before every launch). Spins are bounded by kSpinLimit; a look-back that
// gives up reports through report_timeout and goes on with its partial prefix.
//
// The payload of the 8-byte granules is a codec (GranuleF32, GranuleU32, GranuleU31x2): wave_lookback is the one
// loop, instantiated per codec. Two look-backs are NOT this loop and stay with their one user, taking only the header,
// the constants and the report from here:
//  * scan.hip's parked look-back polls eight 64-tile windows with all loads in flight and classifies them in one
//    unrolled pass with a lane-partial accumulator (no reduction per window). A per-window classification shared
//    with wave_lookback (flag -> stall / whole window / ends at lane `first`) was built and changed the spill counts
//    of both scan schedules' 16-wave variants and of segreduce, so the two classifications stay written out;
//  * sort.hip's look-back is one THREAD per digit over 4-byte granules (flag at bit 30), kLook loads per poll.
#pragma once
#include <stddef.h>

#include "pcmx_common.h"

namespace pcmx {

// The first 16 bytes of every look-back workspace; pcmx_scan_check reads `timeout` of any of them.
struct LookbackHeader {
    unsigned ticket;   // next tile to claim
    unsigned timeout;  // set to 1 by a look-back that gave up
    unsigned pad[2];
    // followed by the granules: unsigned long long status[num_tiles] behind the struct that ends the header
};
static_assert(sizeof(LookbackHeader) == 16 && offsetof(LookbackHeader, ticket) == 0 &&
                  offsetof(LookbackHeader, timeout) == 4 && offsetof(LookbackHeader, pad) == 8,
              "pcmx_scan_check reads the timeout word at byte 4 of every workspace");

constexpr unsigned kFlagAgg = 1u, kFlagIncl = 2u;
#ifdef PCMX_FAULT_INJECT
// test-only build (libpcmx_faultinj.so): the look-back of tile 1 never sees its predecessors and gives up fast
constexpr unsigned kSpinLimit = 64u;
constexpr long long kFaultTile = 1;
#else
constexpr unsigned kSpinLimit = 1u << 26;
#endif

// A look-back that ran out of spins: marks the result invalid in the workspace and in the caller's sticky word
// (system scope: it may live in host-mapped pinned memory). No lane guard: the wave-wide look-back calls it from
// lane 0, the sort from whichever thread gave up.
__device__ __forceinline__ void report_timeout(LookbackHeader* ws, unsigned* err_flag) {
    atomicExch(&ws->timeout, 1u);
    if (err_flag) __hip_atomic_fetch_or(err_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- granule codecs: Value, pack(flag, value), flag(granule), value(granule), zero(), wave_sum(value); Value has +
struct GranuleF32 {  // {flag: 32, f32 value: 32}; the scan
    typedef float Value;
    static __device__ __forceinline__ unsigned long long pack(unsigned flag, float v) {
        return ((unsigned long long)flag << 32) | (unsigned long long)__float_as_uint(v);
    }
    static __device__ __forceinline__ unsigned flag(unsigned long long g) { return (unsigned)(g >> 32); }
    static __device__ __forceinline__ float value(unsigned long long g) { return __uint_as_float((unsigned)g); }
    static __device__ __forceinline__ float zero() { return 0.f; }
    static __device__ __forceinline__ float wave_sum(float v) { return wave_reduce<float, 0>(v); }
};

struct GranuleU32 {  // {flag: 32, u32 count: 32}; select and reduce-by-key
    typedef unsigned Value;
    static __device__ __forceinline__ unsigned long long pack(unsigned flag, unsigned v) {
        return ((unsigned long long)flag << 32) | (unsigned long long)v;
    }
    static __device__ __forceinline__ unsigned flag(unsigned long long g) { return (unsigned)(g >> 32); }
    static __device__ __forceinline__ unsigned value(unsigned long long g) { return (unsigned)g; }
    static __device__ __forceinline__ unsigned zero() { return 0u; }
    static __device__ __forceinline__ unsigned wave_sum(unsigned v) { return wave_reduce<unsigned, 0>(v); }
};

struct Count2 {  // two counts below 2^31 that travel together
    unsigned x, y;
};
__device__ __forceinline__ Count2 operator+(Count2 a, Count2 b) { return Count2{a.x + b.x, a.y + b.y}; }

struct GranuleU31x2 {  // {flag: 2, count x: 31, count y: 31}; top-k
    typedef Count2 Value;
    static constexpr unsigned long long kCountMask = (1ull << 31) - 1ull;
    static __device__ __forceinline__ unsigned long long pack(unsigned flag, Count2 v) {
        return ((unsigned long long)flag << 62) | ((unsigned long long)v.x << 31) | (unsigned long long)v.y;
    }
    static __device__ __forceinline__ unsigned flag(unsigned long long g) { return (unsigned)(g >> 62); }
    static __device__ __forceinline__ Count2 value(unsigned long long g) {
        return Count2{(unsigned)((g >> 31) & kCountMask), (unsigned)(g & kCountMask)};
    }
    static __device__ __forceinline__ Count2 zero() { return Count2{0u, 0u}; }
    static __device__ __forceinline__ Count2 wave_sum(Count2 v) {
        return Count2{wave_reduce<unsigned, 0>(v.x), wave_reduce<unsigned, 0>(v.y)};
    }
};

// The look-back of tile `tile` (>= 1), run by all 64 lanes of one wave: adds the granule values of the predecessors
// back to the first inclusive one to `prefix` (the same in every lane), 64 predecessors per poll. When it runs out of
// spins it reports and leaves a partial sum in prefix, which is never larger than the true one. The report sits
// inside the loop, where every kernel had it, and both exits are breaks: handed to the caller as a returned flag, the
// give-up cost scan_persistent_kernel<16, 8> a VGPR and the top-k gather 12 SGPR spills (profiles/r13_lookback/README.md).
template <class Codec>
__device__ __forceinline__ void wave_lookback(LookbackHeader* ws, const unsigned long long* status, long long tile,
                                              typename Codec::Value& prefix, unsigned* err_flag) {
    const int lane = lane_id();
    long long look = tile - 1;  // newest predecessor still to account for
    unsigned spins = 0;
    while (true) {
        const long long idx = look - lane;
        unsigned long long sv = idx >= 0 ? __hip_atomic_load(&status[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                         : Codec::pack(kFlagIncl, Codec::zero());
#ifdef PCMX_FAULT_INJECT
        if (tile == kFaultTile) sv = 0ull;  // fault injection: this tile never sees its predecessors
#endif
        const unsigned flag = Codec::flag(sv);
        const typename Codec::Value val = Codec::value(sv);
        const unsigned long long m_incl = __ballot(flag == kFlagIncl);
        const unsigned long long m_zero = __ballot(flag == 0u);
        if (m_incl != 0ull) {
            const int first = __builtin_ctzll(m_incl);
            const unsigned long long need = (first == 63) ? ~0ull : ((1ull << (first + 1)) - 1ull);
            if ((m_zero & need) == 0ull) {
                prefix = prefix + Codec::wave_sum(lane <= first ? val : Codec::zero());
                break;
            }
        } else if (m_zero == 0ull) {
            prefix = prefix + Codec::wave_sum(val);
            look -= kWave;
            continue;
        }
        if (++spins > kSpinLimit) {  // bounded spin: report (workspace + sticky caller word), keep the partial prefix
            if (lane == 0) report_timeout(ws, err_flag);
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// wave_lookback and the republication, for wave 0 of the block that owns `tile` and holds its aggregate `agg`: the
// tile becomes inclusive (also after a give-up, as before). Returns the exclusive prefix; zero for tile 0, which
// published itself as inclusive.
template <class Codec>
__device__ __forceinline__ typename Codec::Value lookback_publish(LookbackHeader* ws, unsigned long long* status,
                                                                  long long tile, typename Codec::Value agg,
                                                                  unsigned* err_flag) {
    typename Codec::Value prefix = Codec::zero();
    if (tile != 0) {
        wave_lookback<Codec>(ws, status, tile, prefix, err_flag);
        if (lane_id() == 0)
            __hip_atomic_store(&status[tile], Codec::pack(kFlagIncl, prefix + agg), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    return prefix;
}

}  // namespace pcmx
