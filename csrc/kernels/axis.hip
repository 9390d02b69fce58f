// Reduce and scan (sum, min, max; float32 and int32) along one dimension of a contiguous tensor viewed as
// [outer, n, inner], the work running along n. No counterpart in the reference programs: a library addition, the
// batched members of the reduce / scan family (what torch.sum(dim), amax(dim), cumsum(dim), cummax(dim) are used for).
//
// Nothing here talks to another block inside a launch: no flags, no look-back, no ticket, no atomics, no error word.
// Where several blocks share a row they meet through a workspace of partials BETWEEN launches on the stream. The input
// is read where it lies for every dim (nothing is transposed or copied) and is never written, except by a scan whose
// output is the input (each thread reads its elements before it writes them, and nobody else reads them afterwards).
//
// A row (inner == 1) or a column (inner > 1) is `n` elements, `inner` elements apart. Elements past the end of a row
// read as the identity of the op (0, +inf / INT32_MAX, -inf / INT32_MIN), so rows never mix: a NaN, an inf or an
// overflow stays in its row. A QUAD is 4 consecutive elements v0..v3 of a row; its value is (v0 op v1) op (v2 op v3)
// for a reduce and the running v0, v0 op v1, (v0 op v1) op v2, ((v0 op v1) op v2) op v3 for a scan. Quads are loaded
// with one 16-B access when the row starts allow it (n % 4 == 0, and chunk % 4 == 0 under split) and with 4-B accesses
// otherwise; both forms combine in the same order.
//
// Routes for inner == 1:
//  * group: G lanes per row, G the smallest power of two with 4 G >= n, at most 64; 64 / G rows share a wave, 4 waves a
//    block, the grid strides over the rows. Lane j takes quads j, j + G, j + 2 G, ... Reduce: the lane folds its quads
//    in that order into one accumulator that starts as the identity, then the G lanes fold by a butterfly (partner at
//    distance G/2, G/4, ..., 1). Scan: step i covers quads i G .. i G + G - 1: a Hillis-Steele scan of the G quad totals
//    (distance 1, 2, ..., G/2), element = (carry op lanes-before) op running value, carry = carry op step total.
//  * block: one 256-thread block per row, the grid strides over the rows. A TILE is 256 quads; thread t takes quad t of
//    every tile. Reduce: thread accumulator over the tiles in order, 64-lane butterfly (32, 16, ..., 1), then the four
//    wave results as (w0 op w1) op (w2 op w3). Scan: per tile a 64-lane Hillis-Steele scan of the quad totals, wave
//    totals w0..w3 through LDS, element = ((carry op waves-before) op lanes-before) op running value, waves-before =
//    identity, w0, w0 op w1, (w0 op w1) op w2; carry = carry op (((w0 op w1) op w2) op w3).
//  * split: a row is cut into chunks of `chunk` elements (a multiple of 1024). Launch 1 reduces every chunk as the
//    block route reduces a row, into partials [outer, chunks]. Reduce: launch 2 folds the partials of a row as the
//    block route reduces a row. Scan: launch 2 exclusive-scans them in place as the block route scans a row, launch 3
//    scans every chunk as the block route scans a row with the chunk's partial as the starting carry. The input is read
//    twice and the output written once (12 B per element); the other form, local scans fixed up by a last pass, moves
//    16 B per element. Any number of partials per row is handled: the block route loops.
// Routes for inner > 1:
//  * column, scan: a thread owns 4 adjacent columns of one outer slice (one 16-B access per row when inner % 4 == 0)
//    and walks down n in input order holding 4 running values that start as the identity: a plain left-to-right scan.
//    Lanes run across inner, so a wave reads 1 KiB of one row at a time; outer * ceil(inner / 4) threads in all.
//  * column, reduce: a 256-thread block is TX column quads wide, TX the smallest power of two that covers
//    ceil(inner / 4), at most 64, and TY = 256 / TX rows deep. Thread (ty, tx) folds rows ty, ty + TY, ty + 2 TY, ... of
//    its 4 columns in that order from the identity; the TY partials of a column then fold by halving (ty with
//    ty + TY/2, then TY/4, ..., 1). One launch, no workspace.
//  * column_split: n is cut into chunks of `chunk` rows (at least 16). Launch 1 reduces every chunk as `column` reduces
//    a column, into partials [outer, chunks, inner]; the partials of a column are then a column problem of their own.
//    Reduce: they are reduced by `column` up to 4096 chunks and by another column_split (default chunk) above. Scan:
//    they are exclusive-scanned in place by `column` up to 1024 chunks and by another column_split above, and the last
//    launch scans every chunk as `column` does, starting from its partial. Default chunk, reduce: the smallest that
//    gives 1024 blocks, at least 16 TY rows; scan: the smallest that gives a column 65536 / ceil(inner / 4) chunks.
// The association order of a float32 sum is what is written above: it depends on n, inner, the route and the chunk
// only, never on the row's position, on outer or on timing. That is the "same bits" claim.
// combine and Vec4 are seg_ops.h's; the identity (`ident`) is this file's own.
#include "pcmx_common.h"
#include "pcmx_hip.h"
#include "seg_ops.h"

namespace {
using pcmx::combine;  // seg_ops.h: int32 sums wrap; float min / max hand on a NaN from either side (torch's rule)
using pcmx::kWave;
using pcmx::lane_id;
using pcmx::misaligned;
using pcmx::ranges_overlap;
using pcmx::Vec4;

constexpr int kThreads = 256, kWaves = kThreads / kWave, kTile = kThreads * 4;
constexpr int kGridCap = 2048;             // 256 CUs x 8 blocks, then grid-stride
constexpr long long kReduceFoldDirect = 4096;  // column partials reduced by one `column` launch up to here
constexpr long long kScanFoldDirect = 1024;    // ... and scanned by one up to here
constexpr long long kLimit = 1LL << 31;    // outer * n * inner must stay below

// Not seg_ops.h's identity: a float sum starts from +0.0 here and from -0.0 there, which differ on a row of -0.0s.
template <class T, int OP>
__device__ __forceinline__ T ident() {
    if constexpr (OP == PCMX_OP_SUM) return T(0);
    else if constexpr (std::is_same<T, float>::value) return OP == PCMX_OP_MIN ? __builtin_inff() : -__builtin_inff();
    else return OP == PCMX_OP_MIN ? INT_MAX : INT_MIN;
}

// elements e .. e + 3 of the `len` elements at p; the identity past the end
template <class T>
__device__ __forceinline__ void load4(const T* p, long long e, long long len, bool vec, T id, T v[4]) {
    if (vec && e + 4 <= len) {
        const typename Vec4<T>::type q = pcmx::ld_nt(reinterpret_cast<const typename Vec4<T>::type*>(p + e));
        v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = e + k < len ? __builtin_nontemporal_load(p + e + k) : id;
    }
}

template <class T>
__device__ __forceinline__ void store4(T* p, long long e, long long len, bool vec, const T v[4]) {
    if (vec && e + 4 <= len) {
        typename Vec4<T>::type q;
        q[0] = v[0], q[1] = v[1], q[2] = v[2], q[3] = v[3];
        pcmx::st_nt(reinterpret_cast<typename Vec4<T>::type*>(p + e), q);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e + k < len) p[e + k] = v[k];
    }
}

template <class T, int OP>
__device__ __forceinline__ T quad_fold(const T v[4]) {
    return combine<T, OP>(combine<T, OP>(v[0], v[1]), combine<T, OP>(v[2], v[3]));
}

// v becomes the running values of the quad; returns its total
template <class T, int OP>
__device__ __forceinline__ T quad_scan(T v[4]) {
    v[1] = combine<T, OP>(v[0], v[1]);
    v[2] = combine<T, OP>(v[1], v[2]);
    v[3] = combine<T, OP>(v[2], v[3]);
    return v[3];
}

// the 4 outputs of a quad from `base` (everything before the quad) and its running values r
template <class T, int OP>
__device__ __forceinline__ void quad_out(T base, const T r[4], bool exclusive, T o[4]) {
    if (exclusive) {
        o[0] = base;
#pragma unroll
        for (int k = 1; k < 4; ++k) o[k] = combine<T, OP>(base, r[k - 1]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = combine<T, OP>(base, r[k]);
    }
}

// inclusive Hillis-Steele scan over the G-lane group of this lane (j = lane % G)
template <class T, int OP>
__device__ __forceinline__ T group_scan(T s, int j, int G) {
    for (int off = 1; off < G; off <<= 1) {
        const T o = __shfl_up(s, off, kWave);
        if (j >= off) s = combine<T, OP>(o, s);
    }
    return s;
}

// ---------------------------------------------------------------- group: G lanes per row, 64 / G rows per wave
template <class T, int OP>
__global__ __launch_bounds__(kThreads) void axis_group_reduce_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                                     long long rows, long long n, int G, int vec) {
    const int lane = lane_id(), j = lane & (G - 1), rpw = kWave / G;
    const long long steps = (((n + 3) >> 2) + G - 1) / G, wave_rows = (rows + rpw - 1) / rpw;
    const T id = ident<T, OP>();
    for (long long w = (long long)blockIdx.x * kWaves + threadIdx.x / kWave; w < wave_rows; w += (long long)gridDim.x * kWaves) {
        const long long row = w * rpw + lane / G;
        const long long len = row < rows ? n : 0;  // a group without a row folds identities and stores nothing
        const T* p = x + row * n;                  // only dereferenced below len
        T acc = id;
        for (long long i = 0; i < steps; ++i) {
            T v[4];
            load4(p, 4 * (j + G * i), len, vec != 0, id, v);
            acc = combine<T, OP>(acc, quad_fold<T, OP>(v));
        }
        for (int off = G >> 1; off > 0; off >>= 1) acc = combine<T, OP>(acc, __shfl_xor(acc, off, kWave));
        if (j == 0 && row < rows) out[row] = acc;
    }
}

template <class T, int OP>
__global__ __launch_bounds__(kThreads) void axis_group_scan_kernel(const T* x, T* out, long long rows, long long n, int G,
                                                                   int vec, int exclusive) {
    const int lane = lane_id(), j = lane & (G - 1), rpw = kWave / G;
    const long long steps = (((n + 3) >> 2) + G - 1) / G, wave_rows = (rows + rpw - 1) / rpw;
    const T id = ident<T, OP>();
    for (long long w = (long long)blockIdx.x * kWaves + threadIdx.x / kWave; w < wave_rows; w += (long long)gridDim.x * kWaves) {
        const long long row = w * rpw + lane / G;
        const long long len = row < rows ? n : 0;
        const T* p = x + row * n;
        T* q = out + row * n;
        T carry = id;
        for (long long i = 0; i < steps; ++i) {
            const long long e = 4 * (j + G * i);
            T v[4], o[4];
            load4(p, e, len, vec != 0, id, v);
            const T incl = group_scan<T, OP>(quad_scan<T, OP>(v), j, G);
            const T before = __shfl_up(incl, 1, kWave);
            const T total = __shfl(incl, (lane & ~(G - 1)) + G - 1, kWave);
            quad_out<T, OP>(combine<T, OP>(carry, j ? before : id), v, exclusive != 0, o);
            store4(q, e, len, vec != 0, o);
            carry = combine<T, OP>(carry, total);
        }
    }
}

// ---------------------------------------------------------------- block / split: one block per row or per chunk of a row
// segment s = (row, c): the elements [c * chunk, min(n, (c + 1) * chunk)) of row s / chunks; block: chunks == 1, chunk == n
template <class T, int OP>
__global__ __launch_bounds__(kThreads) void axis_seg_reduce_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                                   long long segs, long long chunks, long long n,
                                                                   long long chunk, int vec) {
    __shared__ T s_w[2][kWaves];  // two sets: one barrier per segment is enough
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
    const T id = ident<T, OP>();
    int buf = 0;
    for (long long s = blockIdx.x; s < segs; s += gridDim.x, buf ^= 1) {
        const long long row = s / chunks, start = (s - row * chunks) * chunk;
        const long long len = min(chunk, n - start), tiles = (len + kTile - 1) / kTile;
        const T* p = x + row * n + start;
        T acc = id;
#pragma unroll 4
        for (long long t = 0; t < tiles; ++t) {
            T v[4];
            load4(p, (t * kThreads + tid) * 4, len, vec != 0, id, v);
            acc = combine<T, OP>(acc, quad_fold<T, OP>(v));
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) acc = combine<T, OP>(acc, __shfl_xor(acc, off, kWave));
        if (lane == 0) s_w[buf][wave] = acc;
        __syncthreads();
        if (tid == 0)
            out[s] = combine<T, OP>(combine<T, OP>(s_w[buf][0], s_w[buf][1]), combine<T, OP>(s_w[buf][2], s_w[buf][3]));
    }
}

// carry_in (or NULL): the starting carry of every segment
template <class T, int OP>
__global__ __launch_bounds__(kThreads) void axis_seg_scan_kernel(const T* x, T* out, const T* __restrict__ carry_in,
                                                                 long long segs, long long chunks, long long n,
                                                                 long long chunk, int vec, int exclusive) {
    __shared__ T s_w[2][kWaves];  // two sets: one barrier per tile is enough
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
    const T id = ident<T, OP>();
    int buf = 0;
    for (long long s = blockIdx.x; s < segs; s += gridDim.x) {
        const long long row = s / chunks, start = (s - row * chunks) * chunk;
        const long long len = min(chunk, n - start), tiles = (len + kTile - 1) / kTile;
        const T* p = x + row * n + start;
        T* q = out + row * n + start;
        T carry = carry_in ? carry_in[s] : id;
        for (long long t = 0; t < tiles; ++t, buf ^= 1) {
            const long long e = (t * kThreads + tid) * 4;
            T v[4], o[4];
            load4(p, e, len, vec != 0, id, v);
            const T incl = group_scan<T, OP>(quad_scan<T, OP>(v), lane, kWave);
            const T before = __shfl_up(incl, 1, kWave);
            if (lane == kWave - 1) s_w[buf][wave] = incl;
            __syncthreads();
            T waves_before = id, total = s_w[buf][0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) {
                if (w == wave) waves_before = total;
                total = combine<T, OP>(total, s_w[buf][w]);
            }
            const T base = combine<T, OP>(combine<T, OP>(carry, waves_before), lane ? before : id);
            quad_out<T, OP>(base, v, exclusive != 0, o);
            store4(q, e, len, vec != 0, o);
            carry = combine<T, OP>(carry, total);
        }
    }
}

// ---------------------------------------------------------------- column / column_split: a thread owns 4 adjacent columns
// chunk c of outer slice o: rows [c * chunk, min(n, (c + 1) * chunk)); partial layout [outer, chunks, inner]; column:
// chunks == 1, chunk == n. scan: unit u = ((o * chunks + c) * cq + g), one thread on columns 4 g .. 4 g + 3.
// reduce: a block is TX column quads wide (TX = col_lanes(inner), a power of two up to 64) and TY = 256 / TX rows deep:
// thread (ty, tx) folds rows r0 + ty, r0 + ty + TY, ... of its 4 columns in that order, then the TY partials of a column
// fold through LDS by halving (ty with ty + TY/2, then TY/4, ..., 1). unit u = ((o * chunks + c) * tiles + t), tile t =
// column quads t TX .. t TX + TX - 1.
template <class T, int OP>
__global__ __launch_bounds__(kThreads) void axis_col_reduce_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                                   long long outer, long long n, long long inner,
                                                                   long long chunk, long long chunks, int TX, int vec) {
    __shared__ T s_p[4][kThreads];
    const int tid = threadIdx.x, TY = kThreads / TX, tx = tid & (TX - 1), ty = tid / TX;
    const long long cq = (inner + 3) >> 2, tiles = (cq + TX - 1) / TX, units = outer * chunks * tiles;
    const T id = ident<T, OP>();
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long oc = u / tiles, col = ((u - oc * tiles) * TX + tx) * 4, o = oc / chunks, c = oc - o * chunks;
        const long long r0 = c * chunk, r1 = min(n, r0 + chunk);
        const T* p = x + (o * n + r0 + ty) * inner;
        T acc[4] = {id, id, id, id};  // columns past inner fold identities and store nothing
#pragma unroll 4
        for (long long r = r0 + ty; r < r1; r += TY, p += (long long)TY * inner) {
            T v[4];
            load4(p, col, inner, vec != 0, id, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = combine<T, OP>(acc[k], v[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s_p[k][tid] = acc[k];
        __syncthreads();
        for (int h = TY >> 1; h > 0; h >>= 1) {
            if (ty < h) {
#pragma unroll
                for (int k = 0; k < 4; ++k) s_p[k][tid] = combine<T, OP>(s_p[k][tid], s_p[k][tid + h * TX]);
            }
            __syncthreads();
        }
        if (ty == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = s_p[k][tid];
            store4(out + oc * inner, col, inner, vec != 0, acc);
        }
        __syncthreads();  // the next unit's partials overwrite s_p
    }
}

template <class T, int OP>
__global__ __launch_bounds__(kThreads) void axis_col_scan_kernel(const T* x, T* out, const T* __restrict__ carry_in,
                                                                 long long outer, long long n, long long inner,
                                                                 long long chunk, long long chunks, int vec, int exclusive) {
    const long long cq = (inner + 3) >> 2, units = outer * chunks * cq;
    const T id = ident<T, OP>();
    for (long long u = (long long)blockIdx.x * kThreads + threadIdx.x; u < units; u += (long long)gridDim.x * kThreads) {
        const long long oc = u / cq, col = (u - oc * cq) * 4, o = oc / chunks, c = oc - o * chunks;
        const long long r0 = c * chunk, r1 = min(n, r0 + chunk);
        const T* p = x + (o * n + r0) * inner;
        T* q = out + (o * n + r0) * inner;
        T acc[4] = {id, id, id, id};
        if (carry_in) load4(carry_in + oc * inner, col, inner, vec != 0, id, acc);
#pragma unroll 4
        for (long long r = r0; r < r1; ++r, p += inner, q += inner) {
            T v[4], nxt[4];
            load4(p, col, inner, vec != 0, id, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) nxt[k] = combine<T, OP>(acc[k], v[k]);
            store4(q, col, inner, vec != 0, exclusive ? acc : nxt);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = nxt[k];
        }
    }
}

// ---------------------------------------------------------------- host side
unsigned grid_for(long long blocks) { return (unsigned)(blocks < 1 ? 1 : (blocks > kGridCap ? kGridCap : blocks)); }
long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

int group_lanes(long long n) {
    int g = 1;
    while (g < kWave && g < (n + 3) / 4) g <<= 1;
    return g;
}

// reduce: the column quads a block is wide, and how many such tiles a row of `inner` columns is
int col_lanes(long long inner) {
    int tx = 1;
    while (tx < kWave && tx < (inner + 3) / 4) tx <<= 1;
    return tx;
}
long long col_tiles(long long inner) { return cdiv((inner + 3) / 4, col_lanes(inner)); }

enum Kind { kReduce, kScan };

// scan: the smallest chunk that gives a column PCMX_AXIS_COLUMN_MIN_UNITS / ceil(inner / 4) chunks (a thread each).
// reduce: the smallest chunk that gives PCMX_AXIS_COLUMN_REDUCE_BLOCKS blocks, and at least 16 rows per thread.
long long default_col_chunk(Kind kind, long long n, long long inner) {
    if (kind == kScan) {
        const long long chunk = cdiv(n, cdiv(PCMX_AXIS_COLUMN_MIN_UNITS, (inner + 3) / 4));
        return chunk < PCMX_AXIS_COLUMN_MIN_CHUNK ? PCMX_AXIS_COLUMN_MIN_CHUNK : chunk;
    }
    const long long chunk = cdiv(n, cdiv(PCMX_AXIS_COLUMN_REDUCE_BLOCKS, col_tiles(inner)));
    const long long least = 16LL * (kThreads / col_lanes(inner));
    return chunk < least ? least : chunk;
}

int default_route(Kind kind, long long outer, long long n, long long inner) {
    if (inner == 1) {
        if (n <= (kind == kScan ? PCMX_AXIS_GROUP_SCAN_N : PCMX_AXIS_GROUP_N)) return PCMX_AXIS_GROUP;
        if (n > PCMX_AXIS_BLOCK_MAX_N || (outer < PCMX_AXIS_SPLIT_ROWS && n >= PCMX_AXIS_SPLIT_MIN_N)) return PCMX_AXIS_SPLIT;
        return PCMX_AXIS_BLOCK;
    }
    const bool fills = kind == kReduce ? outer * col_tiles(inner) >= PCMX_AXIS_COLUMN_MIN_BLOCKS
                                       : outer * ((inner + 3) / 4) >= PCMX_AXIS_COLUMN_MIN_UNITS;
    return fills || n < PCMX_AXIS_COLUMN_SPLIT_MIN_N ? PCMX_AXIS_COLUMN : PCMX_AXIS_COLUMN_SPLIT;
}

struct Plan {
    int route;
    long long chunk, chunks;
};

// route and chunk validated against the shape and resolved; every extent > 0 here
int make_plan(Kind kind, long long outer, long long n, long long inner, int route, long long chunk, Plan* pl) {
    if (route < 0 || route > PCMX_AXIS_COLUMN_SPLIT || chunk < 0) return PCMX_ERR_ARG;
    if (route == 0) route = default_route(kind, outer, n, inner);
    if ((route <= PCMX_AXIS_SPLIT) != (inner == 1)) return PCMX_ERR_ARG;
    if (route == PCMX_AXIS_GROUP && n > PCMX_AXIS_GROUP_MAX_N) return PCMX_ERR_ARG;
    if (route == PCMX_AXIS_BLOCK && n > PCMX_AXIS_BLOCK_MAX_N) return PCMX_ERR_ARG;
    if (route == PCMX_AXIS_SPLIT) {
        if (chunk % kTile) return PCMX_ERR_ARG;
        if (!chunk) chunk = PCMX_AXIS_SPLIT_CHUNK;
    } else if (route == PCMX_AXIS_COLUMN_SPLIT) {
        if (chunk && chunk < PCMX_AXIS_COLUMN_MIN_CHUNK) return PCMX_ERR_ARG;
        if (!chunk) chunk = default_col_chunk(kind, n, inner);
    } else {
        if (chunk) return PCMX_ERR_ARG;
        chunk = n;
    }
    pl->route = route, pl->chunk = chunk, pl->chunks = cdiv(n, chunk);
    return 0;
}

// extents in range: 0 and *total = the product, or PCMX_ERR_ARG for a negative extent or a product of 2^31 or more
int check_extents(long long outer, long long n, long long inner, long long* total) {
    if (outer < 0 || n < 0 || inner < 0) return PCMX_ERR_ARG;
    *total = 0;
    if (outer == 0 || n == 0 || inner == 0) return (outer < kLimit && n < kLimit && inner < kLimit) ? 0 : PCMX_ERR_ARG;
    if (outer >= kLimit || n >= kLimit || inner >= kLimit || outer * n >= kLimit || outer * n * inner >= kLimit)
        return PCMX_ERR_ARG;
    *total = outer * n * inner;
    return 0;
}

template <class T, int OP>
int col_reduce(const T* x, T* out, long long outer, long long n, long long inner, long long chunk, T* ws, hipStream_t s);

// the partials [outer, chunks, inner] of a column_split folded into out [outer, inner]
template <class T, int OP>
int col_fold(const T* part, T* out, long long outer, long long chunks, long long inner, T* ws, hipStream_t s) {
    return col_reduce<T, OP>(part, out, outer, chunks, inner,
                             chunks <= kReduceFoldDirect ? chunks : default_col_chunk(kReduce, chunks, inner), ws, s);
}

template <class T, int OP>
int col_reduce(const T* x, T* out, long long outer, long long n, long long inner, long long chunk, T* ws, hipStream_t s) {
    const long long chunks = cdiv(n, chunk);
    const int vec = inner % 4 == 0;
    T* dst = chunks == 1 ? out : ws;
    axis_col_reduce_kernel<T, OP><<<grid_for(outer * chunks * col_tiles(inner)), kThreads, 0, s>>>(x, dst, outer, n, inner, chunk, chunks,
                                                                                                 col_lanes(inner), vec);
    PCMX_HIP_RET(hipGetLastError());
    if (chunks == 1) return 0;
    return col_fold<T, OP>(ws, out, outer, chunks, inner, ws + pcmx::pad4(outer * chunks * inner), s);
}

template <class T, int OP>
int col_scan(const T* x, T* out, long long outer, long long n, long long inner, long long chunk, int exclusive, T* ws, hipStream_t s) {
    const long long chunks = cdiv(n, chunk), cq = (inner + 3) / 4;
    const int vec = inner % 4 == 0;
    const unsigned grid = grid_for(cdiv(outer * chunks * cq, kThreads));
    if (chunks > 1) {
        axis_col_reduce_kernel<T, OP><<<grid_for(outer * chunks * col_tiles(inner)), kThreads, 0, s>>>(x, ws, outer, n, inner, chunk, chunks,
                                                                                                     col_lanes(inner), vec);
        PCMX_HIP_RET(hipGetLastError());
        const long long sub = chunks <= kScanFoldDirect ? chunks : default_col_chunk(kScan, chunks, inner);
        if (const int rc = col_scan<T, OP>(ws, ws, outer, chunks, inner, sub, 1, ws + pcmx::pad4(outer * chunks * inner), s)) return rc;
    }
    axis_col_scan_kernel<T, OP><<<grid, kThreads, 0, s>>>(x, out, chunks > 1 ? ws : nullptr, outer, n, inner, chunk, chunks, vec, exclusive);
    PCMX_HIP_RET(hipGetLastError());
    return 0;
}

template <class T, int OP>
int reduce_op(const T* x, T* out, long long outer, long long n, long long inner, const Plan& pl, T* ws, hipStream_t s) {
    if (pl.route == PCMX_AXIS_GROUP) {
        const int G = group_lanes(n);
        const long long wave_rows = cdiv(outer, kWave / G);
        axis_group_reduce_kernel<T, OP><<<grid_for(cdiv(wave_rows, kWaves)), kThreads, 0, s>>>(x, out, outer, n, G, n % 4 == 0);
    } else if (pl.route == PCMX_AXIS_BLOCK) {
        axis_seg_reduce_kernel<T, OP><<<grid_for(outer), kThreads, 0, s>>>(x, out, outer, 1, n, n, n % 4 == 0);
    } else if (pl.route == PCMX_AXIS_SPLIT) {
        const long long segs = outer * pl.chunks;
        axis_seg_reduce_kernel<T, OP><<<grid_for(segs), kThreads, 0, s>>>(x, ws, segs, pl.chunks, n, pl.chunk, n % 4 == 0);
        PCMX_HIP_RET(hipGetLastError());
        axis_seg_reduce_kernel<T, OP><<<grid_for(outer), kThreads, 0, s>>>(ws, out, outer, 1, pl.chunks, pl.chunks, 0);
    } else {
        return col_reduce<T, OP>(x, out, outer, n, inner, pl.chunk, ws, s);
    }
    PCMX_HIP_RET(hipGetLastError());
    return 0;
}

template <class T, int OP>
int scan_op(const T* x, T* out, long long outer, long long n, long long inner, const Plan& pl, int exclusive, T* ws, hipStream_t s) {
    if (pl.route == PCMX_AXIS_GROUP) {
        const int G = group_lanes(n);
        const long long wave_rows = cdiv(outer, kWave / G);
        axis_group_scan_kernel<T, OP><<<grid_for(cdiv(wave_rows, kWaves)), kThreads, 0, s>>>(x, out, outer, n, G, n % 4 == 0, exclusive);
    } else if (pl.route == PCMX_AXIS_BLOCK) {
        axis_seg_scan_kernel<T, OP><<<grid_for(outer), kThreads, 0, s>>>(x, out, nullptr, outer, 1, n, n, n % 4 == 0, exclusive);
    } else if (pl.route == PCMX_AXIS_SPLIT) {
        const long long segs = outer * pl.chunks;
        axis_seg_reduce_kernel<T, OP><<<grid_for(segs), kThreads, 0, s>>>(x, ws, segs, pl.chunks, n, pl.chunk, n % 4 == 0);
        PCMX_HIP_RET(hipGetLastError());
        axis_seg_scan_kernel<T, OP><<<grid_for(outer), kThreads, 0, s>>>(ws, ws, nullptr, outer, 1, pl.chunks, pl.chunks, 0, 1);
        PCMX_HIP_RET(hipGetLastError());
        axis_seg_scan_kernel<T, OP><<<grid_for(segs), kThreads, 0, s>>>(x, out, ws, segs, pl.chunks, n, pl.chunk, n % 4 == 0, exclusive);
    } else {
        return col_scan<T, OP>(x, out, outer, n, inner, pl.chunk, exclusive, ws, s);
    }
    PCMX_HIP_RET(hipGetLastError());
    return 0;
}

template <class T>
int axis_reduce(const T* x, T* out, long long outer, long long n, long long inner, int op, int route, long long chunk,
                void* workspace, hipStream_t s) {
    long long total = 0;
    if (!x || !out || misaligned(x) || misaligned(out) || misaligned(workspace)) return PCMX_ERR_ARG;
    if (op < PCMX_OP_SUM || op > PCMX_OP_MAX || check_extents(outer, n, inner, &total)) return PCMX_ERR_ARG;
    if (route < 0 || route > PCMX_AXIS_COLUMN_SPLIT || chunk < 0) return PCMX_ERR_ARG;
    const size_t out_b = (size_t)outer * inner * sizeof(T);
    if (ranges_overlap(out, out_b, x, total ? (size_t)total * sizeof(T) : 1)) return PCMX_ERR_ARG;
    if (outer == 0 || inner == 0) return 0;
    if (n == 0) {
        if (op == PCMX_OP_SUM) PCMX_HIP_RET(hipMemsetAsync(out, 0, out_b, s));
        return 0;
    }
    Plan pl;
    if (const int rc = make_plan(kReduce, outer, n, inner, route, chunk, &pl)) return rc;
    if ((pl.route == PCMX_AXIS_SPLIT || pl.route == PCMX_AXIS_COLUMN_SPLIT) && !workspace) return PCMX_ERR_ARG;
    T* ws = static_cast<T*>(workspace);
    if (op == PCMX_OP_SUM) return reduce_op<T, PCMX_OP_SUM>(x, out, outer, n, inner, pl, ws, s);
    if (op == PCMX_OP_MIN) return reduce_op<T, PCMX_OP_MIN>(x, out, outer, n, inner, pl, ws, s);
    return reduce_op<T, PCMX_OP_MAX>(x, out, outer, n, inner, pl, ws, s);
}

template <class T>
int axis_scan(const T* x, T* out, long long outer, long long n, long long inner, int op, int exclusive, int route,
              long long chunk, void* workspace, hipStream_t s) {
    long long total = 0;
    if (!x || !out || misaligned(x) || misaligned(out) || misaligned(workspace)) return PCMX_ERR_ARG;
    if (op < PCMX_OP_SUM || op > PCMX_OP_MAX || check_extents(outer, n, inner, &total)) return PCMX_ERR_ARG;
    if (route < 0 || route > PCMX_AXIS_COLUMN_SPLIT || chunk < 0) return PCMX_ERR_ARG;
    if (x != out && ranges_overlap(out, (size_t)total * sizeof(T), x, (size_t)total * sizeof(T))) return PCMX_ERR_ARG;
    if (total == 0) return 0;
    Plan pl;
    if (const int rc = make_plan(kScan, outer, n, inner, route, chunk, &pl)) return rc;
    if ((pl.route == PCMX_AXIS_SPLIT || pl.route == PCMX_AXIS_COLUMN_SPLIT) && !workspace) return PCMX_ERR_ARG;
    T* ws = static_cast<T*>(workspace);
    if (op == PCMX_OP_SUM) return scan_op<T, PCMX_OP_SUM>(x, out, outer, n, inner, pl, exclusive, ws, s);
    if (op == PCMX_OP_MIN) return scan_op<T, PCMX_OP_MIN>(x, out, outer, n, inner, pl, exclusive, ws, s);
    return scan_op<T, PCMX_OP_MAX>(x, out, outer, n, inner, pl, exclusive, ws, s);
}
}  // namespace

extern "C" long long pcmx_axis_workspace_bytes(long long outer, long long n, long long inner) {
    if (outer <= 0 || n <= 0 || inner <= 0) return 16;
    // split: a partial per 1024-element tile at the smallest chunk. column_split: a partial row per 16 rows at the
    // smallest chunk, every further level at most 1/16 of the one before (each padded to 4 entries)
    const long long first = cdiv(n, inner == 1 ? (long long)kTile : (long long)PCMX_AXIS_COLUMN_MIN_CHUNK);
    const long long per_column = inner == 1 ? first : first + first / 8 + 8;
    return (long long)pcmx::align16((size_t)(outer * inner * per_column + 64) * 4u);
}

extern "C" int pcmx_axis_reduce_f32(const float* x, float* out, long long outer, long long n, long long inner, int op,
                                    int route, long long chunk, void* workspace, hipStream_t s) {
    return axis_reduce<float>(x, out, outer, n, inner, op, route, chunk, workspace, s);
}
extern "C" int pcmx_axis_reduce_i32(const int32_t* x, int32_t* out, long long outer, long long n, long long inner, int op,
                                    int route, long long chunk, void* workspace, hipStream_t s) {
    return axis_reduce<int>(x, out, outer, n, inner, op, route, chunk, workspace, s);
}
extern "C" int pcmx_axis_scan_f32(const float* x, float* out, long long outer, long long n, long long inner, int op,
                                  int exclusive, int route, long long chunk, void* workspace, hipStream_t s) {
    return axis_scan<float>(x, out, outer, n, inner, op, exclusive, route, chunk, workspace, s);
}
extern "C" int pcmx_axis_scan_i32(const int32_t* x, int32_t* out, long long outer, long long n, long long inner, int op,
                                  int exclusive, int route, long long chunk, void* workspace, hipStream_t s) {
    return axis_scan<int>(x, out, outer, n, inner, op, exclusive, route, chunk, workspace, s);
}
