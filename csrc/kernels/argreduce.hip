// argmin / argmax (float32 and int32): flat, along one dimension of a contiguous [outer, n, inner] view, and over
// ragged segments given by int32 offsets. No counterpart in the reference programs: the "where is the extremum?" members
// of the reduce family (torch.argmax, torch.max(dim), the arg outputs of segment reductions).
//
// One rule for all three forms: a NaN beats every number under both ops, otherwise the numerically largest (smallest)
// element wins with -0.0 == +0.0, and among equal winners (and among NaNs) the lowest position wins. The element of the
// reduction is arg_pair.h's packed (key, ~position) word under an unsigned 64-bit max, whose identity is 0. The
// operator is associative and commutative, so the result depends on the data only, never on the route, the chunk, the
// grid or timing. The value returned is read from x at the winning position by the last launch, bit for bit.
//
// Nothing here talks to another block inside a launch: no flags, no look-back, no spinning, no atomics. Blocks meet
// through a workspace of 8-byte partials BETWEEN launches, as in reduce.hip, axis.hip and ragged.hip, whose shapes the
// three forms follow (those files are left as they are; the host-side planning and the merge-path partition they
// would share are kept as copies here so that what they compile to does not move):
//  * flat: pass 1 is reduce.hip's reduce_pass1 (grid capped at 16384 blocks, grid-stride, four 16-byte non-temporal
//    loads in flight per lane, every element read once), each thread keeping its best word per load slot; pass 2 is one
//    block over the <= 16384 block partials, which also fetches the value.
//  * along a dimension: the reduce halves of axis.hip's routes under the same names. group: G lanes per row, butterfly.
//    block: one block per row. split: a block per chunk of a row into partials [outer, chunks], folded by a block per
//    row. column: a block TX column quads wide and 256 / TX rows deep, folded through LDS. column_split: the same per
//    chunk of n into partials [outer, chunks, inner], folded by `column` up to 4096 chunks and by another column_split
//    above. The position packed is the position along n. The default route is axis.hip's rule for a reduce: its borders
//    were measured for 4-byte reductions and are NOT MEASURED for 8-byte pairs.
//  * ragged segments: ragged.hip's merge-based scheme with the lane accumulator a (key, flat index) word: a partition
//    launch, one block per 4352 path steps, a one-block carry scan of the tile summaries, and a fix-up of the first
//    segment every tile closed. The tile kernel writes final results from its staged values in LDS; the fix-up combines
//    the carry with the tile's own partial of that segment (kept in the workspace) and reads x once per tile. An empty
//    segment gives position -1 and the identity as its value. The precondition on the offsets is NOT checked: offsets
//    that break it give an unspecified result, but every load and store stays inside x[0, n), offsets[0, S], the
//    outputs' [0, S) and the workspace (ragged.hip's clamps, plus a bound on every position that is dereferenced).
#include <limits.h>

#include "arg_pair.h"
#include "pcmx_common.h"
#include "pcmx_hip.h"

namespace {
using pcmx::arg_best;
using pcmx::arg_identity_bits;
using pcmx::arg_pack;
using pcmx::arg_pos;
using pcmx::arg_wave_best;
using pcmx::kWave;
using pcmx::lane_id;
using pcmx::misaligned;
using pcmx::pad4;
using pcmx::ranges_overlap;
using pcmx::u32x4;
using pcmx::u64;

constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr long long kLimit = 1LL << 31;  // element counts and positions stay below

#define PCMX_ARG_SWITCH(fn, ...)                                                                           \
    (key_type == PCMX_KEY_F32 ? (op == PCMX_OP_MIN ? fn<PCMX_KEY_F32, PCMX_OP_MIN>(__VA_ARGS__)           \
                                                   : fn<PCMX_KEY_F32, PCMX_OP_MAX>(__VA_ARGS__))           \
                              : (op == PCMX_OP_MIN ? fn<PCMX_KEY_I32, PCMX_OP_MIN>(__VA_ARGS__)           \
                                                   : fn<PCMX_KEY_I32, PCMX_OP_MAX>(__VA_ARGS__)))

inline bool bad_kind(int key_type, int op) {
    return (key_type != PCMX_KEY_F32 && key_type != PCMX_KEY_I32) || (op != PCMX_OP_MIN && op != PCMX_OP_MAX);
}

__device__ __forceinline__ u64 block_best(u64 v, u64* lds) {  // the result in thread 0
    v = arg_wave_best(v);
    if (lane_id() == 0) lds[threadIdx.x / kWave] = v;
    __syncthreads();
    u64 r = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kWaves; ++i) r = arg_best(r, lds[i]);
    }
    return r;
}

// The winner w of the elements src[0], src[stride], ... of one row: position to idx[o], the element's bits to vals[o].
// w is never the identity for a row of at least one element; should it be, nothing is dereferenced.
template <int KT, int OP>
__device__ __forceinline__ void emit(u64 w, const unsigned* __restrict__ src, long long stride, unsigned* __restrict__ vals,
                                     int* __restrict__ idx, long long o) {
    const int pos = arg_pos(w);
    if (idx) idx[o] = pos;
    if (vals) vals[o] = pos >= 0 ? src[(long long)pos * stride] : arg_identity_bits<KT, OP>();
}

// ================================================================================================ flat
constexpr int kUnroll = 4;  // 16-byte loads in flight per lane: 4 x 16 B x 256 threads = 16 KiB per block
constexpr int kMaxBlocks = 16384;

template <int KT, int OP>
__device__ __forceinline__ u64 fold4(u64 acc, const u32x4& v, unsigned pos) {
    const u64 a = arg_best(arg_pack<KT, OP>(v.x, pos), arg_pack<KT, OP>(v.y, pos + 1u));
    const u64 b = arg_best(arg_pack<KT, OP>(v.z, pos + 2u), arg_pack<KT, OP>(v.w, pos + 3u));
    return arg_best(acc, arg_best(a, b));
}

template <int KT, int OP>
__global__ __launch_bounds__(kThreads) void arg_pass1(const unsigned* __restrict__ x, long long n, u64* __restrict__ partials) {
    __shared__ u64 lds[kWaves];
    const long long n4 = n >> 2;
    const u32x4* x4 = reinterpret_cast<const u32x4*>(x);
    u64 acc[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) acc[u] = 0;
    const long long step = (long long)gridDim.x * kThreads * kUnroll;
    long long i = (long long)blockIdx.x * kThreads * kUnroll + threadIdx.x;
    for (; i + (kUnroll - 1) * kThreads < n4; i += step) {
        u32x4 v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) v[u] = __builtin_nontemporal_load(x4 + i + u * kThreads);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) acc[u] = fold4<KT, OP>(acc[u], v[u], (unsigned)((i + u * kThreads) << 2));
    }
    for (; i < n4; i += kThreads) acc[0] = fold4<KT, OP>(acc[0], x4[i], (unsigned)(i << 2));
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long long t = (n4 << 2) + threadIdx.x;
        acc[1] = arg_best(acc[1], arg_pack<KT, OP>(x[t], (unsigned)t));
    }
    const u64 r = block_best(arg_best(arg_best(acc[0], acc[1]), arg_best(acc[2], acc[3])), lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// One block folds the <= 16384 partials, 16 8-byte loads per thread in flight at a time, and reads the value.
template <int KT, int OP>
__global__ __launch_bounds__(kThreads) void arg_pass2(const u64* __restrict__ partials, int np, const unsigned* __restrict__ x,
                                                      unsigned* __restrict__ vals, int* __restrict__ idx) {
    __shared__ u64 lds[kWaves];
    constexpr int kV = 16;
    u64 acc = 0;
    for (int base = 0; base < np; base += kThreads * kV) {
        u64 v[kV];
#pragma unroll
        for (int u = 0; u < kV; ++u) {
            const int i = base + u * kThreads + (int)threadIdx.x;
            v[u] = i < np ? partials[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < kV; ++u) acc = arg_best(acc, v[u]);
    }
    const u64 r = block_best(acc, lds);
    if (threadIdx.x == 0) emit<KT, OP>(r, x, 1, vals, idx, 0);
}

inline int pass1_blocks(long long n, int cap) {
    long long b = ((n >> 2) + (long long)kThreads * kUnroll - 1) / ((long long)kThreads * kUnroll);
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

template <int KT, int OP>
int flat_launch(const unsigned* x, long long n, unsigned* vals, int* idx, u64* ws, int nb, hipStream_t s) {
    arg_pass1<KT, OP><<<nb, kThreads, 0, s>>>(x, n, ws);
    PCMX_HIP_RET(hipGetLastError());
    arg_pass2<KT, OP><<<1, kThreads, 0, s>>>(ws, nb, x, vals, idx);
    return (int)hipGetLastError();
}

// ================================================================================================ along a dimension
constexpr int kTile = kThreads * 4;
constexpr int kGridCap = 2048;                 // 256 CUs x 8 blocks, then grid-stride (axis.hip's)
constexpr long long kReduceFoldDirect = 4096;  // column partials folded by one `column` launch up to here

// elements e .. e + 3 of the `len` elements at p as words with positions pos0 + e ..; the identity past the end
template <int KT, int OP>
__device__ __forceinline__ void load4p(const unsigned* p, long long e, long long len, bool vec, unsigned pos0, u64 w[4]) {
    const unsigned pos = pos0 + (unsigned)e;
    if (vec && e + 4 <= len) {
        const u32x4 q = pcmx::ld_nt(reinterpret_cast<const u32x4*>(p + e));
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = arg_pack<KT, OP>(q[k], pos + k);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = e + k < len ? arg_pack<KT, OP>(__builtin_nontemporal_load(p + e + k), pos + k) : 0;
    }
}

__device__ __forceinline__ u64 quad_best(const u64 w[4]) { return arg_best(arg_best(w[0], w[1]), arg_best(w[2], w[3])); }

// ---------------------------------------------------------------- group: G lanes per row, 64 / G rows per wave
template <int KT, int OP>
__global__ __launch_bounds__(kThreads) void arg_group_kernel(const unsigned* __restrict__ x, unsigned* __restrict__ vals,
                                                             int* __restrict__ idx, long long rows, long long n, int G, int vec) {
    const int lane = lane_id(), j = lane & (G - 1), rpw = kWave / G;
    const long long steps = (((n + 3) >> 2) + G - 1) / G, wave_rows = (rows + rpw - 1) / rpw;
    for (long long w = (long long)blockIdx.x * kWaves + threadIdx.x / kWave; w < wave_rows; w += (long long)gridDim.x * kWaves) {
        const long long row = w * rpw + lane / G;
        const long long len = row < rows ? n : 0;  // a group without a row folds identities and stores nothing
        const unsigned* p = x + row * n;           // only dereferenced below len
        u64 acc = 0;
        for (long long i = 0; i < steps; ++i) {
            u64 q[4];
            load4p<KT, OP>(p, 4 * (j + G * i), len, vec != 0, 0u, q);
            acc = arg_best(acc, quad_best(q));
        }
        for (int off = G >> 1; off > 0; off >>= 1) acc = arg_best(acc, __shfl_xor(acc, off, kWave));
        if (j == 0 && row < rows) emit<KT, OP>(acc, p, 1, vals, idx, row);
    }
}

// ---------------------------------------------------------------- block / split: one block per row or per chunk of a row
// segment s = (row, c): the entries [c * chunk, min(n, (c + 1) * chunk)) of row s / chunks of src. PACKED false: src is
// x, the entries are elements and are packed with their position in the row. PACKED true: src holds words (the partials
// of a split, n of them per row). part_out: the segment's word goes to part_out[s]; NULL: chunks == 1 and the row's
// result is written from x, whose rows are xn elements long.
template <int KT, int OP, bool PACKED>
__global__ __launch_bounds__(kThreads) void arg_seg_kernel(const void* __restrict__ src, const unsigned* __restrict__ x,
                                                           long long xn, u64* __restrict__ part_out, unsigned* __restrict__ vals,
                                                           int* __restrict__ idx, long long segs, long long chunks, long long n,
                                                           long long chunk, int vec) {
    __shared__ u64 s_w[2][kWaves];  // two sets: one barrier per segment is enough
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
    int buf = 0;
    for (long long s = blockIdx.x; s < segs; s += gridDim.x, buf ^= 1) {
        const long long row = s / chunks, start = (s - row * chunks) * chunk;
        const long long len = min(chunk, n - start);
        u64 acc = 0;
        if constexpr (PACKED) {
            const u64* p = static_cast<const u64*>(src) + row * n + start;
#pragma unroll 4
            for (long long i = tid; i < len; i += kThreads) acc = arg_best(acc, p[i]);
        } else {
            const unsigned* p = static_cast<const unsigned*>(src) + row * n + start;
            const long long tiles = (len + kTile - 1) / kTile;
#pragma unroll 4
            for (long long t = 0; t < tiles; ++t) {
                u64 q[4];
                load4p<KT, OP>(p, (t * kThreads + tid) * 4, len, vec != 0, (unsigned)start, q);
                acc = arg_best(acc, quad_best(q));
            }
        }
        acc = arg_wave_best(acc);
        if (lane == 0) s_w[buf][wave] = acc;
        __syncthreads();
        if (tid == 0) {
            const u64 w = arg_best(arg_best(s_w[buf][0], s_w[buf][1]), arg_best(s_w[buf][2], s_w[buf][3]));
            if (part_out) part_out[s] = w;
            else emit<KT, OP>(w, x + row * xn, 1, vals, idx, row);
        }
    }
}

// ---------------------------------------------------------------- column / column_split: a thread owns 4 adjacent columns
// chunk c of outer slice o: rows [c * chunk, min(n, (c + 1) * chunk)) of src [outer, n, inner]; a block is TX column
// quads wide and TY = 256 / TX rows deep, thread (ty, tx) folds rows r0 + ty, r0 + ty + TY, ... of its 4 columns, then
// the TY partials of a column fold through LDS by halving. PACKED false: src is x and an element is packed with its row
// r; PACKED true: src holds words (the partials [outer, chunks, inner] of the level before). part_out: partial layout
// [outer, chunks, inner]; NULL: chunks == 1 and the results are written from x [outer, xn, inner].
template <int KT, int OP, bool PACKED>
__global__ __launch_bounds__(kThreads) void arg_col_kernel(const void* __restrict__ src, const unsigned* __restrict__ x,
                                                           long long xn, u64* __restrict__ part_out, unsigned* __restrict__ vals,
                                                           int* __restrict__ idx, long long outer, long long n, long long inner,
                                                           long long chunk, long long chunks, int TX, int vec) {
    __shared__ u64 s_p[4][kThreads];
    const int tid = threadIdx.x, TY = kThreads / TX, tx = tid & (TX - 1), ty = tid / TX;
    const long long cq = (inner + 3) >> 2, tiles = (cq + TX - 1) / TX, units = outer * chunks * tiles;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long oc = u / tiles, col = ((u - oc * tiles) * TX + tx) * 4, o = oc / chunks, c = oc - o * chunks;
        const long long r0 = c * chunk, r1 = min(n, r0 + chunk);
        u64 acc[4] = {0, 0, 0, 0};  // columns past inner fold identities and store nothing
        if constexpr (PACKED) {
            const u64* p = static_cast<const u64*>(src) + (o * n + r0 + ty) * inner;
#pragma unroll 4
            for (long long r = r0 + ty; r < r1; r += TY, p += (long long)TY * inner) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (col + k < inner) acc[k] = arg_best(acc[k], p[col + k]);
            }
        } else {
            const unsigned* p = static_cast<const unsigned*>(src) + (o * n + r0 + ty) * inner;
#pragma unroll 4
            for (long long r = r0 + ty; r < r1; r += TY, p += (long long)TY * inner) {
                if (vec && col + 4 <= inner) {
                    const u32x4 q = pcmx::ld_nt(reinterpret_cast<const u32x4*>(p + col));
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = arg_best(acc[k], arg_pack<KT, OP>(q[k], (unsigned)r));
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (col + k < inner)
                            acc[k] = arg_best(acc[k], arg_pack<KT, OP>(__builtin_nontemporal_load(p + col + k), (unsigned)r));
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s_p[k][tid] = acc[k];
        __syncthreads();
        for (int h = TY >> 1; h > 0; h >>= 1) {
            if (ty < h) {
#pragma unroll
                for (int k = 0; k < 4; ++k) s_p[k][tid] = arg_best(s_p[k][tid], s_p[k][tid + h * TX]);
            }
            __syncthreads();
        }
        if (ty == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (col + k >= inner) continue;
                if (part_out) part_out[oc * inner + col + k] = s_p[k][tid];
                else emit<KT, OP>(s_p[k][tid], x + o * xn * inner + col + k, inner, vals, idx, o * inner + col + k);
            }
        }
        __syncthreads();  // the next unit's partials overwrite s_p
    }
}

// ---------------------------------------------------------------- host side (the planning of axis.hip's reduce, copied)
unsigned grid_for(long long blocks) { return (unsigned)(blocks < 1 ? 1 : (blocks > kGridCap ? kGridCap : blocks)); }
long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

int group_lanes(long long n) {
    int g = 1;
    while (g < kWave && g < (n + 3) / 4) g <<= 1;
    return g;
}
int col_lanes(long long inner) {
    int tx = 1;
    while (tx < kWave && tx < (inner + 3) / 4) tx <<= 1;
    return tx;
}
long long col_tiles(long long inner) { return cdiv((inner + 3) / 4, col_lanes(inner)); }

long long default_col_chunk(long long n, long long inner) {
    const long long chunk = cdiv(n, cdiv(PCMX_AXIS_COLUMN_REDUCE_BLOCKS, col_tiles(inner)));
    const long long least = 16LL * (kThreads / col_lanes(inner));
    return chunk < least ? least : chunk;
}

// axis.hip's default for a reduce, unchanged: borders measured for 4-byte reductions, NOT MEASURED for 8-byte pairs
int default_route(long long outer, long long n, long long inner) {
    if (inner == 1) {
        if (n <= PCMX_AXIS_GROUP_N) return PCMX_AXIS_GROUP;
        if (n > PCMX_AXIS_BLOCK_MAX_N || (outer < PCMX_AXIS_SPLIT_ROWS && n >= PCMX_AXIS_SPLIT_MIN_N)) return PCMX_AXIS_SPLIT;
        return PCMX_AXIS_BLOCK;
    }
    const bool fills = outer * col_tiles(inner) >= PCMX_AXIS_COLUMN_MIN_BLOCKS;
    return fills || n < PCMX_AXIS_COLUMN_SPLIT_MIN_N ? PCMX_AXIS_COLUMN : PCMX_AXIS_COLUMN_SPLIT;
}

struct Plan {
    int route;
    long long chunk, chunks;
};

int make_plan(long long outer, long long n, long long inner, int route, long long chunk, Plan* pl) {
    if (route < 0 || route > PCMX_AXIS_COLUMN_SPLIT || chunk < 0) return PCMX_ERR_ARG;
    if (route == 0) route = default_route(outer, n, inner);
    if ((route <= PCMX_AXIS_SPLIT) != (inner == 1)) return PCMX_ERR_ARG;
    if (route == PCMX_AXIS_GROUP && n > PCMX_AXIS_GROUP_MAX_N) return PCMX_ERR_ARG;
    if (route == PCMX_AXIS_BLOCK && n > PCMX_AXIS_BLOCK_MAX_N) return PCMX_ERR_ARG;
    if (route == PCMX_AXIS_SPLIT) {
        if (chunk % kTile) return PCMX_ERR_ARG;
        if (!chunk) chunk = PCMX_AXIS_SPLIT_CHUNK;
    } else if (route == PCMX_AXIS_COLUMN_SPLIT) {
        if (chunk && chunk < PCMX_AXIS_COLUMN_MIN_CHUNK) return PCMX_ERR_ARG;
        if (!chunk) chunk = default_col_chunk(n, inner);
    } else {
        if (chunk) return PCMX_ERR_ARG;
        chunk = n;
    }
    pl->route = route, pl->chunk = chunk, pl->chunks = cdiv(n, chunk);
    return 0;
}

// src [outer, n, inner] (x, or the words of the level before) reduced along n in chunks of `chunk`; the partials
// [outer, chunks, inner] of more than one chunk are a column problem of their own, behind them in the workspace
template <int KT, int OP, bool PACKED>
int col_reduce(const void* src, const unsigned* x, long long xn, unsigned* vals, int* idx, long long outer, long long n,
               long long inner, long long chunk, u64* ws, hipStream_t s) {
    const long long chunks = cdiv(n, chunk);
    arg_col_kernel<KT, OP, PACKED><<<grid_for(outer * chunks * col_tiles(inner)), kThreads, 0, s>>>(
        src, x, xn, chunks == 1 ? nullptr : ws, vals, idx, outer, n, inner, chunk, chunks, col_lanes(inner), inner % 4 == 0);
    PCMX_HIP_RET(hipGetLastError());
    if (chunks == 1) return 0;
    const long long sub = chunks <= kReduceFoldDirect ? chunks : default_col_chunk(chunks, inner);
    return col_reduce<KT, OP, true>(ws, x, xn, vals, idx, outer, chunks, inner, sub, ws + pad4(outer * chunks * inner), s);
}

template <int KT, int OP>
int axis_launch(const unsigned* x, unsigned* vals, int* idx, long long outer, long long n, long long inner, const Plan& pl,
                u64* ws, hipStream_t s) {
    const int vec = n % 4 == 0;
    if (pl.route == PCMX_AXIS_GROUP) {
        const int G = group_lanes(n);
        const long long wave_rows = cdiv(outer, kWave / G);
        arg_group_kernel<KT, OP><<<grid_for(cdiv(wave_rows, kWaves)), kThreads, 0, s>>>(x, vals, idx, outer, n, G, vec);
    } else if (pl.route == PCMX_AXIS_BLOCK) {
        arg_seg_kernel<KT, OP, false><<<grid_for(outer), kThreads, 0, s>>>(x, x, n, nullptr, vals, idx, outer, 1, n, n, vec);
    } else if (pl.route == PCMX_AXIS_SPLIT) {
        const long long segs = outer * pl.chunks;
        arg_seg_kernel<KT, OP, false><<<grid_for(segs), kThreads, 0, s>>>(x, x, n, ws, nullptr, nullptr, segs, pl.chunks, n,
                                                                          pl.chunk, vec);
        PCMX_HIP_RET(hipGetLastError());
        arg_seg_kernel<KT, OP, true><<<grid_for(outer), kThreads, 0, s>>>(ws, x, n, nullptr, vals, idx, outer, 1, pl.chunks,
                                                                         pl.chunks, 0);
    } else {
        return col_reduce<KT, OP, false>(x, x, n, vals, idx, outer, n, inner, pl.chunk, ws, s);
    }
    return (int)hipGetLastError();
}

// ================================================================================================ ragged segments
// ragged.hip's path: with base = offsets[0], ends e_j = offsets[j+1] - base and m = e_{S-1}, the ends are merged with
// 0 .. m-1 into a path of m + S steps, end j at position e_j + j; every block takes kSegTile steps.
constexpr int kItems = 17;                   // path steps per lane (ragged.hip's)
constexpr int kSegTile = kThreads * kItems;  // 4352 path steps per block
constexpr int kCarryThreads = 1024;
constexpr long long kMaxPath = (1LL << 31) - 1;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// base = offsets[0] forced into [0, n] and m = offsets[S] - base forced into [0, n - base]: base + m <= n
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
    u64* open;       // ntiles: the tile's open partial at its end
    u64* carry;      // ntiles: the open segment's partial on entry to the tile
    u64* first;      // ntiles: the tile's own partial of the first segment it closed
};
inline Side side_arrays(void* ws, long long tiles) {
    Side s;
    s.part = static_cast<int*>(ws);
    s.flag = reinterpret_cast<unsigned*>(s.part + pad4(tiles + 1));
    s.open = reinterpret_cast<u64*>(s.flag + pad4(tiles));
    s.carry = s.open + pad4(tiles);
    s.first = s.carry + pad4(tiles);
    return s;
}
inline long long num_tiles(long long path) { return (path + kSegTile - 1) / kSegTile; }
inline size_t seg_ws_bytes(long long tiles) { return (size_t)(pad4(tiles + 1) + pad4(tiles)) * 4 + (size_t)pad4(tiles) * 24; }

// ---------------------------------------------------------------- launch 0: tile borders (ragged.hip's, a copy)
__global__ __launch_bounds__(kThreads) void seg_partition_kernel(const int* __restrict__ offsets, unsigned S, unsigned n,
                                                                 unsigned ntiles, int* __restrict__ part) {
    const unsigned t = blockIdx.x * kThreads + threadIdx.x;
    if (t > ntiles) return;
    const Span sp = span_of(offsets, S, n);
    const unsigned len = sp.m + S;  // <= n + S < 2^31
    const unsigned long long d64 = (unsigned long long)t * kSegTile;
    const unsigned d = d64 < len ? (unsigned)d64 : len;
    // The end count of diagonal d lies in [max(0, d - m), min(d, S)] and the search never leaves that interval, so
    // 0 <= part[t] <= S and 0 <= d - part[t] <= m; lo <= mid < hi <= S keeps offsets[mid + 1] inside offsets[0, S].
    unsigned lo = d > sp.m ? d - sp.m : 0u, hi = d < S ? d : S;
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        if (end_of(offsets[mid + 1u], sp) + mid < d) lo = mid + 1u;
        else hi = mid;
    }
    part[t] = (int)lo;
}

constexpr unsigned kNone = ~0u;
// a word of the tile whose values start at flat index flat0 -> the element's index among them; kNone for the identity
__device__ __forceinline__ unsigned local_of(u64 w, unsigned flat0) { return w ? (unsigned)arg_pos(w) - flat0 : kNone; }

// A segment's word to the outputs. pos is bounded before it is used: a word made from stale LDS or workspace (offsets
// out of order) gives an unspecified result and no fault.
template <int KT, int OP>
__device__ __forceinline__ void emit_bits(u64 w, bool ok, unsigned bits, unsigned* __restrict__ vals, int* __restrict__ idx,
                                          unsigned j) {
    if (idx) idx[j] = ok ? arg_pos(w) : -1;
    if (vals) vals[j] = ok ? bits : arg_identity_bits<KT, OP>();
}

// ---------------------------------------------------------------- launch 1: one tile of the path
template <int KT, int OP>
__global__ __launch_bounds__(kThreads) void seg_tile_kernel(const unsigned* __restrict__ x, unsigned n,
                                                            const int* __restrict__ offsets, unsigned S,
                                                            unsigned* __restrict__ vals, int* __restrict__ idx,
                                                            const int* __restrict__ part, unsigned* __restrict__ flag,
                                                            u64* __restrict__ open, u64* __restrict__ firstw) {
    // s_in: the tile's ns + 1 end values (offsets minus base; entry 0 is the end in front of the tile), then its nv
    // values as raw bits; ns + 1 + nv <= kSegTile + 1, one spare word for the read-ahead
    __shared__ unsigned s_in[kSegTile + 2];
    // the winner of every end closed in the tile as its index among the tile's staged values (kNone: no element); the
    // key is recomputed from s_val on the way out, which keeps the block at ragged.hip's 35 KiB of LDS (4 blocks a CU)
    __shared__ unsigned s_out[kSegTile];
    __shared__ u64 s_wv[kWaves];
    __shared__ unsigned s_wf[kWaves];
    const unsigned tid = threadIdx.x;
    const int lane = lane_id(), wave = (int)(tid / kWave);
    const Span sp = span_of(offsets, S, n);
    const unsigned len = sp.m + S;
    const unsigned long long d64 = (unsigned long long)blockIdx.x * kSegTile;
    if (d64 >= len) {  // block-uniform: a tile past the path is neutral for launch 2
        if (tid == 0) {
            flag[blockIdx.x] = 0u;
            open[blockIdx.x] = 0;
        }
        return;
    }
    const unsigned d0 = (unsigned)d64;
    const unsigned tile_n = len - d0 < (unsigned)kSegTile ? len - d0 : (unsigned)kSegTile;
    // ragged.hip's clamp: s1 forced into [s0, s0 + tile_n], so 0 <= ns <= tile_n, nv = tile_n - ns >= 0, s1 <= S,
    // v0 = d0 - s0 >= 0 and v0 + nv <= m: every load below is inside offsets[0, S] or x[base, base + m), and every
    // store to the outputs inside [s0, s1), a part of [0, S).
    const unsigned s0 = (unsigned)part[blockIdx.x];
    unsigned s1 = (unsigned)part[blockIdx.x + 1];
    s1 = s1 < s0 ? s0 : (s1 > s0 + tile_n ? s0 + tile_n : s1);
    const unsigned ns = s1 - s0, nv = tile_n - ns, v0 = d0 - s0;

    unsigned* s_val = s_in + ns + 1u;
    const unsigned* xt = x + sp.base + v0;
    const unsigned* ot = reinterpret_cast<const unsigned*>(offsets);
    // every address is valid: s0 + i <= s1 <= S for an end, v0 + (i - ns - 1) < v0 + nv <= m for a value; a lane with
    // no word in a round reads offsets[0] and drops it
    unsigned w[kItems + 1];
#pragma unroll
    for (int k = 0; k <= kItems; ++k) {
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

    // the lane's diagonal inside the tile (ragged.hip's search: ai in [max(0, dl - nv), min(dl, ns)])
    const unsigned dl = tid * kItems < tile_n ? tid * kItems : tile_n;
    const unsigned cnt = tile_n - dl < (unsigned)kItems ? tile_n - dl : (unsigned)kItems;
    unsigned lo = dl > nv ? dl - nv : 0u, hi = dl < ns ? dl : ns;
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        if ((long long)s_in[mid + 1u] - (long long)v0 + (long long)mid < (long long)dl) lo = mid + 1u;
        else hi = mid;
    }
    const unsigned flat0 = sp.base + v0;
    // serial walk of cnt steps over ends ai in [0, ns) and values vi in [0, nv); positions stay inside the tile
    // whatever the offsets are, the read-ahead reaches the spare word at most. A value's flat index is flat0 + vi,
    // below base + m <= n.
    unsigned ai = lo, vi = dl - lo;
    unsigned e = s_in[ai + 1u];
    unsigned v = s_val[vi];
    u64 acc = 0, firstval = 0;
    unsigned first = ~0u;  // the first end this lane closed
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        if ((unsigned)i < cnt) {
            const bool take_end = vi >= nv || (ai < ns && e <= v0 + vi);
            if (take_end) {
                if (first == ~0u) first = ai, firstval = acc;
                else s_out[ai] = local_of(acc, flat0);  // ai < ns <= kSegTile
                acc = 0;
                e = s_in[++ai + 1u];
            } else {
                acc = arg_best(acc, arg_pack<KT, OP>(v, flat0 + vi));
                v = s_val[++vi];
            }
        }
    }
    // segmented scan over the lanes in a fixed order: (f1, w1) . (f2, w2) = (f1 | f2, f2 ? w2 : best(w1, w2))
    unsigned f = first != ~0u ? 1u : 0u;
    u64 a = acc;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const u64 ov = __shfl_up(a, off, kWave);
        const unsigned of = __shfl_up(f, off, kWave);
        if (lane >= off) {
            a = f ? a : arg_best(ov, a);
            f |= of;
        }
    }
    if (lane == kWave - 1) {
        s_wv[wave] = a;
        s_wf[wave] = f;
    }
    u64 ev = __shfl_up(a, 1, kWave);  // the item of the lanes below this one in the wave
    unsigned ef = __shfl_up(f, 1, kWave);
    if (lane == 0) {
        ev = 0;
        ef = 0u;
    }
    __syncthreads();
    u64 pv = 0;
    for (int k = 0; k < wave; ++k) pv = s_wf[k] ? s_wv[k] : arg_best(pv, s_wv[k]);  // the waves below
    const u64 c = ef ? ev : arg_best(pv, ev);  // what the lanes below hold of the segment open at this lane
    if (first != ~0u) {
        const u64 fw = arg_best(c, firstval);
        s_out[first] = local_of(fw, flat0);        // first < ns
        if (first == 0u) firstw[blockIdx.x] = fw;  // the tile's own partial of the first segment it closed (launch 3)
    }
    if (tid == kThreads - 1) {
        flag[blockIdx.x] = ns != 0u ? 1u : 0u;
        open[blockIdx.x] = first != ~0u ? acc : arg_best(c, acc);
    }
    __syncthreads();

    // coalesced stores: the winner of a segment closed here is an element of this tile, still staged in s_val. When the
    // offsets are out of order a word of s_out may be stale: the index is bounded before it is used.
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const unsigned i = tid + (unsigned)k * kThreads;
        if (i < ns) {
            const unsigned local = s_in[i + 1u] == s_in[i] ? kNone : s_out[i];
            const bool ok = local < nv;
            if (idx) idx[s0 + i] = ok ? (int)(flat0 + local) : -1;  // s0 + i < s1 <= S
            if (vals) vals[s0 + i] = ok ? s_val[local] : arg_identity_bits<KT, OP>();
        }
    }
}

// ---------------------------------------------------------------- launch 2: carries, one block (ragged.hip's scheme)
// carry[t] = the open partials from the nearest earlier closing tile (or tile 0) up to tile t - 1. The block walks the
// summaries in rounds of kCarryThreads x 4 with the running word in a register; the arrays are padded to a multiple of
// 4 entries, entries from ntiles on are masked to the neutral element.
__global__ __launch_bounds__(kCarryThreads) void seg_carry_kernel(const unsigned* __restrict__ flag, const u64* __restrict__ open,
                                                                  u64* __restrict__ carry, int ntiles) {
    constexpr int kCarryWaves = kCarryThreads / kWave;
    __shared__ u64 s_v[2][kCarryWaves];
    __shared__ unsigned s_f[2][kCarryWaves];
    const int lane = lane_id(), wave = threadIdx.x / kWave;
    const int quads = (ntiles + 3) / 4, rounds = (quads + kCarryThreads - 1) / kCarryThreads;
    const u32x4* fq = reinterpret_cast<const u32x4*>(flag);
    const u64x2* vq = reinterpret_cast<const u64x2*>(open);
    u64 run = 0;
    int q = (int)threadIdx.x;
    for (int r = 0; r < rounds; ++r, q += kCarryThreads) {
        u32x4 f4 = {0u, 0u, 0u, 0u};
        u64 v4[4] = {0, 0, 0, 0};
        if (q < quads) {
            f4 = fq[q];
            const u64x2 lo2 = vq[2 * q], hi2 = vq[2 * q + 1];
            v4[0] = lo2[0], v4[1] = lo2[1], v4[2] = hi2[0], v4[3] = hi2[1];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q >= quads || 4 * q + j >= ntiles) f4[j] = 0u, v4[j] = 0;
        unsigned f = 0u;
        u64 v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // this thread's 4 tiles, in order
            v = f4[j] ? v4[j] : arg_best(v, v4[j]);
            f |= f4[j];
        }
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const u64 ov = __shfl_up(v, off, kWave);
            const unsigned of = __shfl_up(f, off, kWave);
            if (lane >= off) {
                v = f ? v : arg_best(ov, v);
                f |= of;
            }
        }
        if (lane == kWave - 1) {
            s_v[r & 1][wave] = v;
            s_f[r & 1][wave] = f;
        }
        u64 ev = __shfl_up(v, 1, kWave);  // the pair of the threads below this one in the wave
        unsigned ef = __shfl_up(f, 1, kWave);
        if (lane == 0) ev = 0, ef = 0u;
        __syncthreads();
        u64 pv = run, total = run;
#pragma unroll
        for (int k = 0; k < kCarryWaves; ++k) {
            if (k == wave) pv = total;  // the waves below this one, behind `run`
            total = s_f[r & 1][k] ? s_v[r & 1][k] : arg_best(total, s_v[r & 1][k]);
        }
        run = total;
        u64 c = ef ? ev : arg_best(pv, ev);  // the open segment's word on entry to tile 4 q
        u64 c4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c4[j] = c;
            c = f4[j] ? v4[j] : arg_best(c, v4[j]);
        }
        if (q < quads) {  // 4 q + 3 < pad4(ntiles): inside the workspace
            u64x2* cq = reinterpret_cast<u64x2*>(carry);
            cq[2 * q] = u64x2{c4[0], c4[1]};
            cq[2 * q + 1] = u64x2{c4[2], c4[3]};
        }
    }
}

// ---------------------------------------------------------------- launch 3: the first segment every tile closed
// part[t] of a tile that closed a segment is below S. The result is the better of the carry and the tile's own partial
// (a tie goes to the carry: its position is lower), written over what launch 1 stored; x is read once per tile, at a
// position bounded by n.
template <int KT, int OP>
__global__ __launch_bounds__(kThreads) void seg_fixup_kernel(const unsigned* __restrict__ x, unsigned n,
                                                             unsigned* __restrict__ vals, int* __restrict__ idx,
                                                             const int* __restrict__ part, const unsigned* __restrict__ flag,
                                                             const u64* __restrict__ carry, const u64* __restrict__ firstw,
                                                             unsigned ntiles) {
    const unsigned t = blockIdx.x * kThreads + threadIdx.x + 1u;
    if (t >= ntiles || !flag[t]) return;
    const u64 c = carry[t];
    if (c == 0) return;  // nothing of the segment lies in front of the tile
    const u64 w = arg_best(c, firstw[t]);
    const unsigned pos = (unsigned)arg_pos(w);
    const bool ok = pos < n;
    emit_bits<KT, OP>(w, ok, ok ? x[pos] : 0u, vals, idx, (unsigned)part[t]);
}

template <int KT, int OP>
int seg_launch(const unsigned* x, long long n, const int* offsets, long long S, unsigned* vals, int* idx, void* workspace,
               hipStream_t s) {
    const long long tiles = num_tiles(n + S);  // >= 1: S > 0
    const Side side = side_arrays(workspace, tiles);
    seg_partition_kernel<<<(unsigned)((tiles + 1 + kThreads - 1) / kThreads), kThreads, 0, s>>>(offsets, (unsigned)S, (unsigned)n,
                                                                                               (unsigned)tiles, side.part);
    PCMX_HIP_RET(hipGetLastError());
    seg_tile_kernel<KT, OP><<<(unsigned)tiles, kThreads, 0, s>>>(x, (unsigned)n, offsets, (unsigned)S, vals, idx, side.part,
                                                                 side.flag, side.open, side.first);
    PCMX_HIP_RET(hipGetLastError());
    if (tiles > 1) {
        seg_carry_kernel<<<1, kCarryThreads, 0, s>>>(side.flag, side.open, side.carry, (int)tiles);
        PCMX_HIP_RET(hipGetLastError());
        seg_fixup_kernel<KT, OP><<<(unsigned)((tiles - 1 + kThreads - 1) / kThreads), kThreads, 0, s>>>(
            x, (unsigned)n, vals, idx, side.part, side.flag, side.carry, side.first, (unsigned)tiles);
    }
    return (int)hipGetLastError();
}
}  // namespace

// ================================================================================================ C entries
extern "C" long long pcmx_arg_reduce_workspace_bytes(long long n) {
    return (long long)pass1_blocks(n > 0 ? n : 0, kMaxBlocks) * 8;
}

extern "C" int pcmx_arg_reduce_b32_grid(const void* x, long long n, int key_type, int op, void* value_out, int32_t* index_out,
                                        void* workspace, int max_blocks, hipStream_t s) {
    if (bad_kind(key_type, op) || n < 0 || n >= kLimit || max_blocks < 1 || max_blocks > kMaxBlocks) return PCMX_ERR_ARG;
    if ((n && !x) || misaligned(x) || !workspace || misaligned(workspace)) return PCMX_ERR_ARG;
    if ((!value_out && !index_out) || misaligned(value_out, 3u) || misaligned(index_out, 3u)) return PCMX_ERR_ARG;
    return PCMX_ARG_SWITCH(flat_launch, static_cast<const unsigned*>(x), n, static_cast<unsigned*>(value_out), index_out,
                           static_cast<u64*>(workspace), pass1_blocks(n, max_blocks), s);
}

extern "C" int pcmx_arg_reduce_b32(const void* x, long long n, int key_type, int op, void* value_out, int32_t* index_out,
                                   void* workspace, hipStream_t s) {
    return pcmx_arg_reduce_b32_grid(x, n, key_type, op, value_out, index_out, workspace, kMaxBlocks, s);
}

extern "C" long long pcmx_axis_arg_workspace_bytes(long long outer, long long n, long long inner) {
    if (outer <= 0 || n <= 0 || inner <= 0) return 16;
    // pcmx_axis_workspace_bytes' count of partials (split: one per 1024-element tile at the smallest chunk;
    // column_split: a partial row per 16 rows, every further level at most 1/16 of the one before), 8 bytes each
    const long long first = cdiv(n, inner == 1 ? (long long)kTile : (long long)PCMX_AXIS_COLUMN_MIN_CHUNK);
    const long long per_column = inner == 1 ? first : first + first / 8 + 8;
    return (long long)pcmx::align16((size_t)(outer * inner * per_column + 64) * 8u);
}

extern "C" int pcmx_axis_arg_reduce_b32(const void* x, void* value_out, int32_t* index_out, long long outer, long long n,
                                        long long inner, int key_type, int op, int route, long long chunk, void* workspace,
                                        hipStream_t s) {
    if (bad_kind(key_type, op) || outer < 0 || n < 0 || inner < 0) return PCMX_ERR_ARG;
    if (outer >= kLimit || n >= kLimit || inner >= kLimit) return PCMX_ERR_ARG;
    if (route < 0 || route > PCMX_AXIS_COLUMN_SPLIT || chunk < 0) return PCMX_ERR_ARG;
    if (!x || misaligned(x) || misaligned(workspace)) return PCMX_ERR_ARG;
    if ((!value_out && !index_out) || misaligned(value_out, 3u) || misaligned(index_out, 3u)) return PCMX_ERR_ARG;
    if (outer == 0 || inner == 0) return 0;
    if (n == 0 || outer * n >= kLimit || outer * n * inner >= kLimit) return PCMX_ERR_ARG;  // no extremum of nothing
    const size_t out_b = (size_t)outer * inner * 4, x_b = (size_t)outer * n * inner * 4;
    if (ranges_overlap(value_out, out_b, x, x_b) || ranges_overlap(index_out, out_b, x, x_b) ||
        ranges_overlap(value_out, out_b, index_out, out_b))
        return PCMX_ERR_ARG;
    Plan pl;
    if (const int rc = make_plan(outer, n, inner, route, chunk, &pl)) return rc;
    if ((pl.route == PCMX_AXIS_SPLIT || pl.route == PCMX_AXIS_COLUMN_SPLIT) && !workspace) return PCMX_ERR_ARG;
    return PCMX_ARG_SWITCH(axis_launch, static_cast<const unsigned*>(x), static_cast<unsigned*>(value_out), index_out, outer, n,
                           inner, pl, static_cast<u64*>(workspace), s);
}

extern "C" long long pcmx_segment_arg_workspace_bytes(long long n, long long S) {
    const long long path = (n > 0 ? n : 0) + (S > 0 ? S : 0);
    return (long long)pcmx::align16(seg_ws_bytes(num_tiles(path)));
}

extern "C" int pcmx_segment_arg_reduce_b32(const void* x, long long n, const int32_t* offsets, long long S, int key_type, int op,
                                           void* value_out, int32_t* index_out, void* workspace, hipStream_t s) {
    if (bad_kind(key_type, op) || n < 0 || S < 0 || n + S > kMaxPath) return PCMX_ERR_ARG;
    if (!offsets || misaligned(offsets, 3u)) return PCMX_ERR_ARG;
    if ((!value_out && !index_out) || misaligned(value_out, 3u) || misaligned(index_out, 3u)) return PCMX_ERR_ARG;
    if (S == 0) return 0;
    if ((n && (!x || misaligned(x, 3u))) || !workspace || misaligned(workspace)) return PCMX_ERR_ARG;
    const size_t out_b = (size_t)S * 4, x_b = (size_t)n * 4, off_b = (size_t)(S + 1) * 4;
    if (ranges_overlap(value_out, out_b, x, x_b) || ranges_overlap(value_out, out_b, offsets, off_b) ||
        ranges_overlap(index_out, out_b, x, x_b) || ranges_overlap(index_out, out_b, offsets, off_b) ||
        ranges_overlap(value_out, out_b, index_out, out_b))
        return PCMX_ERR_ARG;
    return PCMX_ARG_SWITCH(seg_launch, static_cast<const unsigned*>(x), n, offsets, S, static_cast<unsigned*>(value_out),
                           index_out, workspace, s);
}
