// Sparse matrix-vector products on MI355X (ref 3-serial-optimization/spmv.c: multiply_naive :170-177,
// banded SSE multiply :212-329) — and the north-star 1e8-nnz power-law CSR SpMV.
//
// CSR (any sparsity, power-law safe): CSR-adaptive with nnz-balanced work items. An analysis pass
// (pcmx_spmv_csr_plan, once per matrix) cuts the rows into items of <= kItemNnz nonzeros: runs of short
// rows are packed into one item, a long row is split into several items. One wave per item:
//   * multi-row item: the wave streams the item's values/columns coalesced, multiplies by the gathered x,
//     parks the products in LDS, then reduces rows with L = 64/rows lanes per row;
//   * long-row piece: straight wave reduction, one float atomic per piece into y (y zeroed first).
// Every wave does about the same number of nonzeros whatever the degree distribution, so the heavy rows
// of a power-law graph do not produce a tail.
//
// XCD-sliced CSR (SlicedCSR in ops/sparse.py): the plain kernel's x gathers miss the 4-MiB per-XCD L2 ~85%
// of the time at 1e7 columns (x = 40 MB) and run at the Infinity-Cache gather rate (~60 G gathers/s
// measured chip-wide by scripts/gather_lab.hip, vs ~270 G/s when each XCD gathers from its own <= 4 MiB).
// So the columns are cut into S = 8 * phases slices (a small, hot head of columns is dealt by rows instead,
// so every XCD keeps its own copy of it); workgroups are dealt round-robin over the 8 XCDs, so block b runs
// slice (b % 8) + 8 * phase and all of a slice's gathers stay inside ONE L2. Each slice writes a COMPACT
// partial y: one value per row the slice touches (36% of the S x n_rows pairs on the 1e8-nnz power-law graph;
// the dense S x n_rows partials cost 640 MB of writes + 640 MB of combine reads per product). A combine pass
// sums every row's partials (per-row slice mask + per-64-row-chunk base offsets, each lane's rank among the
// lanes touching a slice from one byte-packed DPP wave scan), a fix-up adds the later pieces of split long rows.
//
// Banded (implicit column indices): one wave per row; the 5 bands are contiguous slices of x and of the
// value array, so all loads are unit-stride and no column index is ever read.
#include "pcmx_common.h"
#include "pcmx_hip.h"

#include <map>
#include <mutex>
#include <vector>

namespace {
using pcmx::kWave;
constexpr int kItemNnz = 1024;
constexpr int kWavesPerBlock = 4;

struct Item {
    int row0, row1;        // rows [row0, row1) (row1 == row0 + 1 for a long-row piece)
    long long nz0, nz1;    // nonzeros [nz0, nz1)
};

constexpr int kItemRows = 1023;           // rows per multi-row item (bounds the row-pointer LDS stage)
constexpr int kRpPerLane = (kItemRows + 1 + 63) / 64;  // row pointers per lane (kItemRows + 1 per item)
constexpr int kPerLane = kItemNnz / kWave;  // nonzeros per lane
constexpr int kMaxSlices = PCMX_SPMV_MAX_SLICES;
constexpr int kPersistBlocks = 3;  // sliced kernel: resident blocks (of 4 waves) per CU (161 VGPRs -> 3 waves/SIMD)
constexpr int kBandedRows = 16;    // banded kernels: rows per block

// ------------------------------------------------------------------------------------------ plain CSR
// One wave per item. All column/value loads of the item AND its row pointers are issued up front, then all
// x gathers, so a lane keeps ~3 x kPerLane loads in flight instead of a dependent chain. Products are parked
// in LDS with the row pointers; the row reduction (L lanes per row) then reads LDS only.
__global__ __launch_bounds__(kWavesPerBlock * kWave) void spmv_csr_items_kernel(
    const long long* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ val,
    const float* __restrict__ x, float* __restrict__ y, const Item* __restrict__ items, long long n_items) {
    __shared__ float prod[kWavesPerBlock][kItemNnz];
    __shared__ int rps[kWavesPerBlock][kItemRows + 1];
    const int w = threadIdx.x / kWave, lane = pcmx::lane_id();
    const long long it = (long long)blockIdx.x * kWavesPerBlock + w;
    if (it >= n_items) return;
    const Item item = items[it];
    const long long nz0 = item.nz0;
    const int n = (int)(item.nz1 - nz0);
    const int nrows = item.row1 - item.row0;
    int cj[kPerLane];
    float vj[kPerLane];
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const int i = j * kWave + lane;
        cj[j] = i < n ? __builtin_nontemporal_load(col + nz0 + i) : 0;
        vj[j] = i < n ? __builtin_nontemporal_load(val + nz0 + i) : 0.f;
    }
    if (nrows == 1) {  // single row (whole short row, or one piece of a long row)
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) acc += vj[j] * x[cj[j]];
        acc = pcmx::wave_reduce<float, 0>(acc);
        if (lane == 0) {
            if (nz0 == row_ptr[item.row0] && item.nz1 == row_ptr[item.row0 + 1])
                y[item.row0] = acc;
            else
                atomicAdd(&y[item.row0], acc);
        }
        return;
    }
    long long rj[kRpPerLane];
#pragma unroll
    for (int j = 0; j < kRpPerLane; ++j) {
        const int i = j * kWave + lane;
        rj[j] = i <= nrows ? __builtin_nontemporal_load(row_ptr + item.row0 + i) : 0;
    }
    float* pr = prod[w];
    int* rp = rps[w];
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) pr[j * kWave + lane] = vj[j] * x[cj[j]];
#pragma unroll
    for (int j = 0; j < kRpPerLane; ++j) {
        const int i = j * kWave + lane;
        if (i <= nrows) rp[i] = (int)(rj[j] - nz0);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    // L lanes per row: about avg-row-length / 4 lanes, power of two, at most 64 / (rows per pass)
    const int avg = n / nrows;
    int L = 1;
    while (L < 64 && L * 4 < avg) L <<= 1;
    const int sub = lane & (L - 1), grp = lane / L, ngrp = kWave / L;
    for (int r = grp; r < nrows; r += ngrp) {
        const int b = rp[r], e = rp[r + 1];
        float acc = 0.f;
        for (int i = b + sub; i < e; i += L) acc += pr[i];
        for (int off = L >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);
        if (sub == 0) y[item.row0 + r] = acc;
    }
}

// ------------------------------------------------------------------------------------------ XCD-sliced CSR
// Layout per slice: col/val of its nonzeros (slice-major, row order kept), lrow = the u16 row offset of each
// nonzero inside its item, and nnz-balanced items (a later piece of a split long row has row1 == row0).
// A slice averages ~1 nonzero per row, so rows are not reduced from row pointers: an item's nonzeros are sorted
// by row and the wave sums each row with a segmented scan over its lanes (sliced_step), in a fixed order, so the
// sums are reproducible run to run. (An LDS-scatter form of the row sums lost to it in round 2, profiles/r2_spmv.)
//
// Persistent waves with a one-item software pipeline: a wave issues item k's gathers as soon as its columns
// are in registers, then item k+1's stream loads, and only then waits for the gathers, so the next item's
// HBM latency hides behind the current item's gathers and LDS work (measured: one item per wave 1.07 ms,
// pipelined 0.99 ms at 8 slices). Every load and store of the loop is a buffer instruction whose descriptor
// covers exactly the item's bytes: lanes past the end read 0 / drop their store in hardware, so no memory
// instruction sits under a branch and the compiler's vmcnt bookkeeping stays exact across the loop.
// The arrays of a second matrix in a PAIRED launch (pcmx_spmv_sliced_pair): slices with part[s] = 1 read these instead
// of the kernel arguments (the two row chunks of a distributed column-split step multiply their chunk-0 columns in ONE
// launch, profiles/r5_spmv/).
struct SlicePart {
    const int* col;
    const float* val;
    const unsigned short* lrow;
    const Item* items;
    float* ypart;
    float* extra;
};
struct SliceMeta {
    long long nz0[kMaxSlices];    // first nonzero of slice s in the slice-major col/val/lrow
    long long item0[kMaxSlices + 1];
    long long item1[kMaxSlices];  // items of slice s: [item0[s], item1[s])
    long long out0[kMaxSlices];   // first compact partial of slice s
    int colbase[kMaxSlices];      // packed layout: first tail column of slice s
    unsigned char part[kMaxSlices];  // 1: slice s belongs to the paired matrix `b`
    SlicePart b;
};
// Packed layout (kPacked): ONE 32-bit word per nonzero instead of a 4-B column + a 2-B row offset —
//   bits 0-20 column - colbase[s] (tail) or the column itself (head, bit 21 set), bits 22-31 the row offset in
//   the item (< 1023) — 6 -> 4 B of index stream per nonzero and one stream load instruction fewer per element.
constexpr unsigned kPackColMask = 0x1FFFFFu, kPackHead = 0x200000u;
constexpr int kPackRowShift = 22;

template <int kPL>
struct StreamRegs {
    int c[kPL];
    float v[kPL];
    unsigned short r[kPL];
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}

template <int kPL, bool kPacked>
__device__ __forceinline__ void load_item_stream(const int* __restrict__ col, const float* __restrict__ val,
                                                 const unsigned short* __restrict__ lrow, const Item& it,
                                                 StreamRegs<kPL>& q, int lane) {
    const unsigned n = (unsigned)(it.nz1 - it.nz0);
    const auto rc = rsrc(col + it.nz0, n * 4), rv = rsrc(val + it.nz0, n * 4), rr = rsrc(lrow + it.nz0, n * 2);
#pragma unroll
    for (int j = 0; j < kPL; ++j) {  // aux 2 = nt: streamed once
        const unsigned i = j * kWave + lane;
        q.c[j] = __builtin_amdgcn_raw_buffer_load_b32(rc, i * 4, 0, 2);
        q.v[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rv, i * 4, 0, 2));
    }
    if constexpr (!kPacked) {
#pragma unroll
        for (int j = 0; j < kPL; ++j) q.r[j] = __builtin_amdgcn_raw_buffer_load_b16(rr, (j * kWave + lane) * 2, 0, 2);
    }
}

struct SlicedCtx {
    const int* col;
    const float* val;
    const unsigned short* lrow;
    __amdgpu_buffer_rsrc_t rx;
    const Item* items;
    float* yp;
    float* extra;
    long long i1, stride;
    int lane;
    int colbase;  // packed layout: first tail column of the slice
};

// One step of a segmented inclusive scan over the wave (Hillis-Steele on DPP): (v, f) = (running sum, "a segment
// starts at or after the combined range"); a lane without a source in this pattern keeps its value (old = 0).
template <int kCtrl, int kRowMask>
__device__ __forceinline__ void seg_scan_step(float& v, int& f) {
    const float vp = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, kRowMask, 0xf, false));
    const int fp = __builtin_amdgcn_update_dpp(0, f, kCtrl, kRowMask, 0xf, false);
    v = f ? v : v + vp;
    f |= fp;
}
__device__ __forceinline__ void seg_scan_wave(float& v, int& f) {
    seg_scan_step<0x111, 0xf>(v, f);  // row_shr:1 .. row_shr:8: within rows of 16 lanes
    seg_scan_step<0x112, 0xf>(v, f);
    seg_scan_step<0x114, 0xf>(v, f);
    seg_scan_step<0x118, 0xf>(v, f);
    seg_scan_step<0x142, 0xa>(v, f);  // row_bcast:15 into rows 1 and 3
    seg_scan_step<0x143, 0xc>(v, f);  // row_bcast:31 into rows 2 and 3
}

// One pipeline step: gathers of the current item, stream loads of the next item, then the current item's row
// sums and stores. Called alternately with the two register sets swapped (a register copy would make the
// compiler wait for the prefetch).
// Row sums by a segmented DPP scan per 64-element stripe — an item's nonzeros are sorted by row, so element
// i = j * 64 + lane continues the row of element i - 1 unless its lrow differs; the lane holding a row's LAST
// element stores the row sum straight to the compact partials (a row running past a stripe carries its partial
// sum into the next stripe). No LDS, no barriers.
// Partial stores: temporal on the packed layout (the ~340 MB of compact partials are re-read by the combine right
// after the product, and non-temporal stores evicted them early: 0.633-0.652 -> 0.628 ms per step at 1e8 nnz,
// bit-identical; profiles/r4_spmv/store_temporal_partials.txt), non-temporal on the unpacked one. The policy follows
// the layout because that round-4 A/B was run on the packed layout only; the unpacked kernels keep the stores they had.
template <bool kPacked, int kPL>
__device__ __forceinline__ bool sliced_step(const SlicedCtx& k, long long& it, const Item& cur, const StreamRegs<kPL>& q,
                                            Item& nitem, StreamRegs<kPL>& nq) {
    constexpr int kStAux = kPacked ? 0 : 2;  // 0: temporal (may stay in L2 / MALL for the combine), 2: nt
    const int lane = k.lane;
    float g[kPL];
#pragma unroll
    for (int j = 0; j < kPL; ++j) {
        const unsigned w = (unsigned)q.c[j];
        const unsigned c = kPacked ? (w & kPackColMask) + ((w & kPackHead) ? 0u : (unsigned)k.colbase) : w;
        g[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(k.rx, c * 4, 0, 0));
    }
    // the row offset of element j (packed: the word's top bits; read before nq may reuse q's registers)
    auto lrow_of = [&](int j) __attribute__((always_inline)) {
        return kPacked ? (int)((unsigned)q.c[j] >> kPackRowShift) : (int)q.r[j];
    };
    const long long nxt = it + k.stride;
    const bool more = nxt < k.i1;
    nitem = k.items[more ? nxt : it];
    load_item_stream<kPL, kPacked>(k.col, k.val, k.lrow, nitem, nq, lane);  // (a harmless re-read of the last item)
    const int n = (int)(cur.nz1 - cur.nz0);
    const int nrows = cur.row1 - cur.row0;
    if (nrows <= 1) {  // whole short row or a piece of a long row (later piece: row1 == row0 -> extra[it])
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < kPL; ++j) acc += q.v[j] * g[j];
        acc = pcmx::wave_reduce<float, 0>(acc);
        const auto r1 = rsrc(nrows == 1 ? k.yp + cur.row0 : k.extra + it, 4u);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc), r1, lane == 0 ? 0u : 0x80000000u, 0, kStAux);
    } else {
        const auto ry = rsrc(k.yp + cur.row0, (unsigned)nrows * 4);
        float carry = 0.f;
        int rprev = -1;  // row of the element before this stripe (wave-uniform)
#pragma unroll
        for (int j = 0; j < kPL; ++j) {
            const bool valid = j * kWave + lane < n;
            const int r = valid ? lrow_of(j) : 0x10000;  // past the item: one trailing non-row segment
            float v = valid ? q.v[j] * g[j] : 0.f;
            const int rp = __builtin_amdgcn_update_dpp(rprev, r, 0x138, 0xf, 0xf, false);  // wave_shr:1
            int f = r != rp;
            seg_scan_wave(v, f);
            v = f ? v : v + carry;  // lanes still in the row carried in from the previous stripe
            const int rnext0 = (j + 1 < kPL && (j + 1) * kWave < n)
                                   ? __builtin_amdgcn_readlane(lrow_of(j + 1 < kPL ? j + 1 : j), 0)
                                   : 0x10000;
            const int rn = __builtin_amdgcn_update_dpp(rnext0, r, 0x130, 0xf, 0xf, false);  // wave_shl:1
            const bool tail = valid && r != rn;
            // predicated: only a row's last lane issues its store (an out-of-range offset on the other lanes
            // still cost them address slots: 0.706 -> 0.693 ms per product, profiles/r2_spmv/store_ab.txt)
            if (tail) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ry, (unsigned)r * 4u, 0, kStAux);
            const int r63 = __builtin_amdgcn_readlane(r, 63);
            carry = r63 == rnext0 ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)) : 0.f;
            rprev = r63;
        }
    }
    it = nxt;
    return more;
}

// The item loop of one wave over slice s (items [it, i1), stride apart) of ONE matrix, its arrays as __restrict__
// parameters (after inlining they keep their no-alias scopes).
template <bool kPacked, int kPL>
__device__ __forceinline__ void sliced_wave(const unsigned short* __restrict__ lrow, const int* __restrict__ col,
                                            const float* __restrict__ val, const float* __restrict__ x, int n_cols,
                                            float* __restrict__ ypart, float* __restrict__ extra,
                                            const Item* __restrict__ items, const SliceMeta& meta, int s, long long it,
                                            long long i1, long long stride) {
    SlicedCtx k;
    k.i1 = i1;
    k.stride = stride;
    const long long base = meta.nz0[s];
    k.col = col + base, k.val = val + base, k.lrow = lrow + base;
    k.colbase = meta.colbase[s];
    k.rx = rsrc(x, (unsigned)n_cols * 4);
    k.items = items, k.extra = extra, k.yp = ypart + meta.out0[s];
    k.lane = pcmx::lane_id();
    Item ia = items[it], ib;
    StreamRegs<kPL> qa, qb;
    load_item_stream<kPL, kPacked>(k.col, k.val, k.lrow, ia, qa, k.lane);
    while (sliced_step<kPacked, kPL>(k, it, ia, qa, ib, qb) && sliced_step<kPacked, kPL>(k, it, ib, qb, ia, qa)) {
    }
}

// kPaired: a paired launch (pcmx_spmv_sliced_pair), whose slices may belong to the second matrix (meta.b). The item
// loop is instantiated once per matrix with that matrix's arrays as its own __restrict__ parameters: selecting the
// pointers per slice in front of ONE loop cost the 1e8-nnz single-matrix product 8% (0.639 -> 0.691 ms in the round-5
// A/B of scripts/spmv_step_time.py: ~400 more instructions in the item loop).
template <bool kPacked, int kPL, bool kPaired = false>
__global__ __launch_bounds__(kWavesPerBlock * kWave) void spmv_sliced_kernel(
    const unsigned short* __restrict__ lrow, const int* __restrict__ col, const float* __restrict__ val,
    const float* __restrict__ x, int n_cols, float* __restrict__ ypart, float* __restrict__ extra,
    const Item* __restrict__ items, SliceMeta meta, int blocks_per_slice, int phase_lo) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int b = blockIdx.x;
    const int phase = phase_lo + b / (8 * blocks_per_slice);
    const int s = phase * 8 + (b & 7);
    const long long i1 = kPaired ? meta.item1[s] : meta.item0[s + 1];
    const long long stride = (long long)blocks_per_slice * kWavesPerBlock;
    const long long it = meta.item0[s] + (long long)((b >> 3) % blocks_per_slice) * kWavesPerBlock + w;
    if (it >= i1) return;
    if (kPaired && meta.part[s])  // (wave-uniform) a slice of the paired matrix
        sliced_wave<kPacked, kPL>(meta.b.lrow, meta.b.col, meta.b.val, x, n_cols, meta.b.ypart, meta.b.extra,
                                  meta.b.items, meta, s, it, i1, stride);
    else
        sliced_wave<kPacked, kPL>(lrow, col, val, x, n_cols, ypart, extra, items, meta, s, it, i1, stride);
}

// y[r] = sum over the slices touching row r (bit k of mask[r]) of that slice's compact partial, in slice order.
// One wave per 64-row chunk c: the partial of slice k for lane l sits at out0[k] + base[c][k] + (number of lower
// lanes whose row slice k also touches) — a ballot + popcount; base[c][*] is wave-uniform (scalar loads).
struct SliceOut {
    long long out0[kMaxSlices + 1];
};
template <int S>
__global__ __launch_bounds__(256) void spmv_combine_kernel(const float* __restrict__ comp, const unsigned* __restrict__ mask,
                                                           const int* __restrict__ base, SliceOut so, float* __restrict__ y,
                                                           int n_rows) {
    // XCD-aware chunk order: workgroups are dealt round-robin over the 8 XCDs, so block b takes chunk group
    // (b % 8) * (gridDim.x / 8) + b / 8 and each XCD walks ONE contiguous row range (a slice's partial runs of
    // neighbouring chunks share cache lines in that XCD's L2 instead of being fetched by two XCDs). One 64-row
    // chunk per wave: 2, 4 or 8 chunks per wave (more loads in flight per round trip) measured the same
    // (profiles/r2_spmv/combine_chunks_ab.txt).
    const int g = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    const int c = __builtin_amdgcn_readfirstlane(g * 4 + (int)threadIdx.x / kWave);
    const int lane = pcmx::lane_id();
    const int r = c * kWave + lane;
    if (c * kWave >= n_rows) return;
    const unsigned m = r < n_rows ? __builtin_nontemporal_load(mask + r) : 0u;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int* bc = base + (size_t)c * S;
    // predicated loads: only the lanes whose row slice k touches issue a load (~36% of them). The S loads still
    // overlap (no wait inside the loop), and inactive lanes cost the address unit nothing — issuing every lane
    // with an out-of-range buffer offset instead made the pass address-rate bound: 113 -> ~73 us per product
    // (profiles/r2_spmv/combine_variants_ab.txt; a cooperative 16-B-load + LDS variant measured in between)
    float v[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const bool bit = (m >> k) & 1u;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(bit);
        v[k] = 0.f;
        if (bit) v[k] = comp[so.out0[k] + bc[k] + (long long)__popcll(bal & below)];
    }
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < S; ++k) acc += v[k];  // slice order; untouched slices add +0
    if (r < n_rows) y[r] = acc;
}

// Production combine (same partials, same slice-order sums, so bit-identical to spmv_combine_kernel): the per-slice
// ranks "lanes below me whose row slice k touches" come from ONE byte-packed wave scan instead of S ballots + S
// popcounts. Slices 4j..4j+3 of a lane's mask become the bytes of word j (x * 0x00204081 spreads 4 bits to 4 bytes,
// no carries), a 6-step DPP inclusive scan of the S/4 words sums them over the lanes (each byte <= 64, so bytes
// never carry into each other), and inclusive - own is the exclusive rank. The pass is VALU-issue bound (~280 VALU
// per 64 rows at S = 24 with ballots, profiles/r3_spmv/combine_scan_ab.txt); this form issues ~40% fewer.
template <int kCtrl, int kRowMask>
__device__ __forceinline__ unsigned scan_step_u32(unsigned v) {
    return v + (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, kRowMask, 0xf, false);
}
// The combine of one 64-row chunk c for this lane's row r (the value it stores; 0 past n_rows).
template <int S>
__device__ __forceinline__ float combine_scan_row(const float* __restrict__ comp, const unsigned* __restrict__ mask,
                                                  const int* __restrict__ base, const SliceOut& so, int n_rows, int c,
                                                  int lane, int r) {
    static_assert(S % 4 == 0 && S <= 32, "byte-packed slice counters");
    constexpr int D = S / 4;
    const unsigned m = r < n_rows ? __builtin_nontemporal_load(mask + r) : 0u;
    const int* bc = base + (size_t)c * S;
    unsigned own[D], inc[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        own[j] = (((m >> (4 * j)) & 0xfu) * 0x00204081u) & 0x01010101u;
        inc[j] = own[j];
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
        inc[j] = scan_step_u32<0x111, 0xf>(inc[j]);  // row_shr:1 .. row_shr:8 within rows of 16 lanes
        inc[j] = scan_step_u32<0x112, 0xf>(inc[j]);
        inc[j] = scan_step_u32<0x114, 0xf>(inc[j]);
        inc[j] = scan_step_u32<0x118, 0xf>(inc[j]);
        inc[j] = scan_step_u32<0x142, 0xa>(inc[j]);  // row_bcast:15 into rows 1 and 3
        inc[j] = scan_step_u32<0x143, 0xc>(inc[j]);  // row_bcast:31 into rows 2 and 3
    }
    // the S wave-uniform partial bases (32-bit byte offsets: the host keeps the partials < 4 GiB), all in SGPRs
    // BEFORE the predicated loads: left to itself the compiler sinks each scalar load into its slice's branch and
    // waits on it there (S serial scalar round trips)
    unsigned off[S];
#pragma unroll
    for (int k = 0; k < S; ++k) off[k] = (unsigned)(so.out0[k] + bc[k]) * 4u;
#pragma unroll
    for (int k = 0; k < S; ++k) asm volatile("" ::"s"(off[k]));
    // exclusive ranks are < 64, so the byte offsets 4 * rank (< 256) still fit their bytes: one shift per word,
    // then one bit-field extract per slice
    unsigned ex4[D];
#pragma unroll
    for (int j = 0; j < D; ++j) ex4[j] = (inc[j] - own[j]) << 2;
    const auto rc = rsrc(comp, 0xffffffffu);
    float v[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const unsigned boff = (ex4[k / 4] >> (8 * (k % 4))) & 0xffu;
        v[k] = 0.f;
        if ((own[k / 4] >> (8 * (k % 4))) & 0xffu) v[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rc, boff, off[k], 0));
    }
    // the sum starts from an OPAQUE +0 (same value, same bits): from a literal 0 the compiler folds 0 + v[0] into the
    // first predicated load's branch and waits for that load there, a serial round trip per wave (round 5, with the
    // SGPR cap below: 93 -> 77 us per 1e8-nnz fused combine, profiles/r5_spmv/n1_step_regression_ab.txt)
    float acc = 0.f;
    asm volatile("" : "+v"(acc));
#pragma unroll
    for (int k = 0; k < S; ++k) acc += v[k];
    return acc;
}

// amdgpu_num_sgpr(76): the combine is latency-bound, so residency is its speed. 256-thread blocks are admitted per CU
// up to floor(800 / (ceil(sgpr / 16) * 16 + 16)): <= 80 SGPRs 8 blocks, 81-96 only 7. Left alone the compiler gives
// these kernels 90 SGPRs at S = 24 (106 at 32) without needing them (capped: 74, no spills).
#define PCMX_COMBINE_SGPRS __attribute__((amdgpu_num_sgpr(76)))
template <int S>
__global__ __launch_bounds__(256) PCMX_COMBINE_SGPRS void spmv_combine_scan_kernel(const float* __restrict__ comp,
                                                                const unsigned* __restrict__ mask,
                                                                const int* __restrict__ base, SliceOut so,
                                                                float* __restrict__ y, int n_rows) {
    const int g = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);  // as above
    const int c = __builtin_amdgcn_readfirstlane(g * 4 + (int)threadIdx.x / kWave);
    const int lane = pcmx::lane_id();
    const int r = c * kWave + lane;
    if (c * kWave >= n_rows) return;
    const float acc = combine_scan_row<S>(comp, mask, base, so, n_rows, c, lane, r);
    if (r < n_rows) y[r] = acc;
}

// Round 5: the combine with the split-row fix-up and the send-buffer pack in its epilogue — ONE launch per row chunk of
// a distributed step instead of three (combine, fix-up, pack; profiles/r5_spmv/).
//  * fix-up: fix_chunk0[c] .. fix_chunk0[c + 1] are the fix entries (item, row; sorted by row) of the wave's 64 rows; each
//    run of one row is summed exactly as spmv_fixup_kernel sums it (lane-strided from the run's first entry, then the
//    same wave reduction) and added to the row's combined value: bit-identical to combine + fix-up.
//  * pack: send_ptr[r] .. send_ptr[r + 1] index the send-buffer slots (send_slot) that carry row r to the peers that
//    reference it (built once at set-up from the same send lists the gather used): the wave writes its rows' values
//    straight into the send buffer, so no gather pass re-reads y after the combine (send_ptr == nullptr: no pack).
template <int S>
__global__ __launch_bounds__(256) PCMX_COMBINE_SGPRS void spmv_combine_fused_kernel(const float* __restrict__ comp,
                                                                 const unsigned* __restrict__ mask,
                                                                 const int* __restrict__ base, SliceOut so,
                                                                 float* __restrict__ y, int n_rows,
                                                                 const float* __restrict__ extra,
                                                                 const int2* __restrict__ fix,
                                                                 const int* __restrict__ fix_chunk0,
                                                                 const int* __restrict__ send_ptr,
                                                                 const int* __restrict__ send_slot,
                                                                 float* __restrict__ sendbuf) {
    const int g = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);  // as above
    const int c = __builtin_amdgcn_readfirstlane(g * 4 + (int)threadIdx.x / kWave);
    const int lane = pcmx::lane_id();
    const int r = c * kWave + lane;
    if (c * kWave >= n_rows) return;
    // the chunk's fix range [fix_chunk0[c], fix_chunk0[c + 1]) (lanes 0 / 1) and the row's send range as VECTOR loads
    // issued next to the mask load, so one wait covers them all (loaded after the combine, each was one more dependent
    // round trip per wave)
    const int fv = fix_chunk0 ? __builtin_nontemporal_load(fix_chunk0 + c + (lane & 1)) : 0;
    int p0 = 0, p1 = 0;
    if (send_ptr && r < n_rows) p0 = send_ptr[r], p1 = send_ptr[r + 1];
    float acc = combine_scan_row<S>(comp, mask, base, so, n_rows, c, lane, r);
    if (fix_chunk0) {
        const int f1 = __builtin_amdgcn_readlane(fv, 1);
        for (int k = __builtin_amdgcn_readlane(fv, 0); k < f1;) {  // wave-uniform: one run (one row) per iteration
            const int row = __builtin_amdgcn_readfirstlane(fix[k].y);
            float part = 0.f;
            int len = 0;
            for (int j0 = k;; j0 += kWave) {  // a row's entries are contiguous: the run ends in the first stripe with a gap
                const int j = j0 + lane;
                const bool in = j < f1 && fix[j].y == row;
                if (in) part += extra[fix[j].x];
                const unsigned long long bin = __builtin_amdgcn_ballot_w64(in);
                len += __popcll(bin);
                if (__builtin_amdgcn_ballot_w64(!in) != 0) break;
            }
            part = pcmx::wave_reduce<float, 0>(part);
            if (r == row) acc += part;
            k += len;
        }
    }
    if (r < n_rows) {
        y[r] = acc;
        for (int p = p0; p < p1; ++p) sendbuf[send_slot[p]] = acc;
    }
}

// later pieces of split long rows: fix[k] = {item index, row}, sorted by row (item order kept within a row). The
// wave of the first entry of each row's run sums the run's extras (lane-strided, then a fixed-order wave
// reduction) and adds them once: deterministic, unlike one float atomic per piece (whose order, and so whose
// rounding, varied run to run), and parallel (a hub row of the power-law graph has hundreds of pieces).
__global__ __launch_bounds__(256) void spmv_fixup_kernel(const float* __restrict__ extra, const int2* __restrict__ fix,
                                                         int n_fix, float* __restrict__ y) {
    const int k = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)threadIdx.x / kWave);  // one wave per entry
    const int lane = pcmx::lane_id();
    if (k >= n_fix) return;
    const int row = fix[k].y;
    if (k > 0 && fix[k - 1].y == row) return;
    float acc = 0.f;
    for (int j0 = k;; j0 += kWave) {  // a row's entries are contiguous: the run ends in the first stripe with a gap
        const int j = j0 + lane;
        const bool in = j < n_fix && fix[j].y == row;
        if (in) acc += extra[fix[j].x];
        if (__builtin_amdgcn_ballot_w64(!in) != 0) break;
    }
    acc = pcmx::wave_reduce<float, 0>(acc);
    if (lane == 0) y[row] += acc;
}

// Band limits of one row: left outer, left inner, centre, right inner, right outer (ref create_csr_matrix,
// spmv.c:91-107; clipped to [0, n), empty bands have hi == lo). Non-decreasing in `row`.
__device__ __forceinline__ void band_limits(int n, int a, int b, int c, int d, int e, int row, int (&lo)[5], int (&hi)[5]) {
    const int ah = a / 2;
    const int r5 = ah, r6 = ah + b, r7 = ah + b + c, r8 = ah + b + c + d, r9 = ah + b + c + d + e;
    lo[0] = max(0, row - r9), hi[0] = max(0, row - r8);
    lo[1] = max(0, row - r7), hi[1] = max(0, row - r6);
    lo[2] = max(0, row - r5), hi[2] = min(row + r5 + 1, n);
    lo[3] = min(n, row + r6 + 1), hi[3] = min(n, row + r7 + 1);
    lo[4] = min(n, row + r8 + 1), hi[4] = min(n, row + r9 + 1);
#pragma unroll
    for (int k = 0; k < 5; ++k) hi[k] = max(hi[k], lo[k]);
}

// Banded SpMV with implicit column indices (ref s_matrix `multiply`, spmv.c:212-329), one block per R = kBandedRows
// rows; a wave keeps U of its rows in flight (2 in the LDS-window kernel, 1 for the clipped blocks of the stream kernel).
//  * x: band k of rows r0..r0+R-1 reads the contiguous window [lo_k(r0), hi_k(r0+R-1)) — one row's band shifted
//    by up to R-1 — so the block stages the 5 windows in LDS once (coalesced) and every nonzero reads x there.
//  * values: row i's nonzeros are contiguous; a wave takes whole rows, lane j reads value j + 64m (coalesced
//    256-B wave loads, all ceil(nnz/64) <= NL of a row issued before use, two rows in flight per wave).
//  * no per-row metadata: the rows' nonzero counts and band limits are computed in registers (a wave prefix
//    scan of the R counts gives each row's offset from the block's first row); row_off is read ONCE per block.
template <int NL, int U>
__device__ __forceinline__ void banded_rows_body(const float* __restrict__ vals, const long long* __restrict__ row_off,
                                                 int n, int a, int b, int c, int d, int e, const float* __restrict__ x,
                                                 float* __restrict__ y, float* xw, int r0) {
    constexpr int R = kBandedRows;
    static_assert(R <= kWave && R % 4 == 0, "rows per block");
    const int lane = pcmx::lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const int nr = min(R, n - r0);
    int wlo[5], wbase[5], total = 0;
    {
        int lo0[5], hi0[5], lo1[5], hi1[5];
        band_limits(n, a, b, c, d, e, r0, lo0, hi0);
        band_limits(n, a, b, c, d, e, r0 + nr - 1, lo1, hi1);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            wlo[k] = lo0[k], wbase[k] = total;
            total += max(0, hi1[k] - lo0[k]);
        }
    }
    for (int i = (int)threadIdx.x; i < total; i += 256) {
        const int k = (i >= wbase[1]) + (i >= wbase[2]) + (i >= wbase[3]) + (i >= wbase[4]);
        int wl = wlo[0], wb = wbase[0];
#pragma unroll
        for (int q = 1; q < 5; ++q)
            if (k == q) wl = wlo[q], wb = wbase[q];
        xw[i] = x[wl + i - wb];
    }
    // nonzeros of the block's rows (lane l = row r0 + l) and their exclusive prefix
    int my = 0;
    if (lane < nr) {
        int lo[5], hi[5];
        band_limits(n, a, b, c, d, e, r0 + lane, lo, hi);
#pragma unroll
        for (int k = 0; k < 5; ++k) my += hi[k] - lo[k];
    }
    int incl = my;
#pragma unroll
    for (int off = 1; off < R; off <<= 1) {
        const int o = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += o;
    }
    const long long boff = row_off[r0];
    __syncthreads();

    for (int rr = wave; rr < nr; rr += 4 * U) {  // rows rr, rr + 4, ... (U rows of the wave in flight)
        float v[U][NL];
        int off[U][5], cum[U][4], nnz[U];
        const int cnt = min(U, (nr - rr + 3) / 4);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u >= cnt) break;
            const int row = rr + 4 * u;
            const int row_nnz = __builtin_amdgcn_readlane(my, row);
            const long long start = boff + (long long)__builtin_amdgcn_readlane(incl - my, row);
            const float* vr = vals + start;
#pragma unroll
            for (int m = 0; m < NL; ++m) {
                const int j = lane + 64 * m;
                v[u][m] = (64 * m < row_nnz && j < row_nnz) ? vr[j] : 0.f;
            }
            int lo[5], hi[5];
            band_limits(n, a, b, c, d, e, r0 + row, lo, hi);
            int cs = 0;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                off[u][k] = wbase[k] + lo[k] - wlo[k] - cs;  // LDS index of nonzero j of band k = j + off
                cs += hi[k] - lo[k];
                if (k < 4) cum[u][k] = cs;
            }
            nnz[u] = row_nnz;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u >= cnt) break;
            float acc = 0.f;
#pragma unroll
            for (int m = 0; m < NL; ++m) {
                if (64 * m >= nnz[u]) break;
                // lanes past the row's end read a valid slot (their value is 0): branch-free, a chain of
                // selects over the row's 5 scalar band offsets (no indexed register array)
                const int j = min(lane + 64 * m, nnz[u] - 1);
                const int o = off[u][0] + (j >= cum[u][0] ? off[u][1] - off[u][0] : 0) +
                              (j >= cum[u][1] ? off[u][2] - off[u][1] : 0) + (j >= cum[u][2] ? off[u][3] - off[u][2] : 0) +
                              (j >= cum[u][3] ? off[u][4] - off[u][3] : 0);
                acc = fmaf(v[u][m], xw[j + o], acc);
            }
            acc = pcmx::wave_reduce<float, 0>(acc);
            if (lane == 0) y[r0 + rr + 4 * u] = acc;
        }
    }
}
template <int NL>
__global__ __launch_bounds__(256) void spmv_banded_lds_kernel(const float* __restrict__ vals,
                                                              const long long* __restrict__ row_off, int n, int a, int b,
                                                              int c, int d, int e, const float* __restrict__ x,
                                                              float* __restrict__ y) {
    extern __shared__ float xw[];
    banded_rows_body<NL, 2>(vals, row_off, n, a, b, c, d, e, x, y, xw, (int)blockIdx.x * kBandedRows);
}

// Variant 8 (block stream): a block of R = kBandedRows rows reads its values — ONE contiguous CSR range — as one aligned 16-B
// stream through a buffer descriptor over exactly that range's float4s, instead of row by row with 4-B loads.
// Valid for blocks of UNCLIPPED rows (every band inside [0, n)): all such rows hold L nonzeros in the same band
// layout, and band k's window of a block starting at row r0 begins at column r0 + delta[k], so every block's five
// concatenated x windows have the same layout. Element e of a block (from its first value) is row rr = floor(e / L),
// position j = e - rr L, and its x slot is s(e) = e - rr (L - 1) + lut(j), lut(j) = window base of j's band minus the
// band's first position. Per float4 (elements e0 .. e0 + 3) ONE 16-B LDS read of lut4[j0] gives the four slot
// offsets (lut4[j][kk] = kk + lut(j + kk), or, past the row end, kk - (L - 1) + lut(j + kk - L): the next row), so
// the slots cost one add each and no per-element band search.
// Row sums: one wave iteration's 256 elements span at most two rows (L >= 256, checked by the launcher); lanes add
// their products to acc (the wave's current row `cur`) or accn, and when row cur has ended the wave sums acc on the
// DPP path into lane 63, which adds it to the block's row sums in LDS (ds_add_f32: a row split between two waves
// gets two commutative adds, the same result whichever lands first).
struct BandGeo {
    int L, W, n;     // row length, window floats per block (L + 5 (R - 1)), rows
    int delta[5];    // window k of a block starting at row r0 begins at column r0 + delta[k]
    int wbase[6];    // window k occupies LDS [wbase[k], wbase[k + 1])
    int cum[5];      // first position of band k in a row
};

// The slot table lut4 is the same for every block of a geometry: the launcher builds it once on the host (cached in
// device memory per geometry, banded_lut_table) and each block copies it into LDS with kLutPer 16-B loads per thread
// issued with the window loads (building it per block cost ~1/3 of the kernel's VALU work: profiles/r4_spmv).
constexpr int kLutPer = 4;  // table entries per thread: 4 * ql <= 1024, checked by the launcher
constexpr int kStreamNV = 10;  // value float4s per lane: a wave's quarter of 16 rows of up to 1024 nonzeros
constexpr int kStreamXW = 3;   // x-window floats per thread (256 * kStreamXW >= W + 3, checked by the launcher)
__device__ __forceinline__ void banded_stream_block(const float* __restrict__ vals, long long off0, const BandGeo& g,
                                                    const pcmx::i32x4* __restrict__ lut_g, int rb_begin, int sb_idx,
                                                    const float* __restrict__ x, float* __restrict__ y, float* sm) {
    constexpr int R = kBandedRows, NV = kStreamNV, XW = kStreamXW;
    const int L = g.L;
    // four copies of the x windows, copy q shifted by q (xq[q][i] = window[i + q]), each 16-B aligned: the four x
    // values of a float4 whose slots s .. s + 3 are consecutive are ONE aligned ds_read_b128 from copy s & 3
    // (conflict-free across the wave) instead of four ds_read_b32 at a 16-B lane stride (4-way bank conflicts)
    const int wq = 256 * XW;                                       // floats per copy (>= W + 3, checked by the launcher)
    float* xq = sm;                                                // [4][wq]
    float* ysum = sm + 4 * wq;                                     // [R]
    pcmx::i32x4* lut4 = reinterpret_cast<pcmx::i32x4*>(sm + 4 * wq + ((R + 3) & ~3));  // [L + 3], 16-B aligned
    const int lane = pcmx::lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const int r0 = (rb_begin + sb_idx) * R;
    // first value of the block: unclipped rows all hold L values, so no row_off load sits before the stream loads
    const long long boff = off0 + (long long)sb_idx * R * L;
    const long long a0 = boff & ~3LL;
    const int lead = (int)(boff - a0);
    const int nf4 = (lead + R * L + 3) >> 2;           // float4s of the block's aligned span
    const int qw = (nf4 + 3) >> 2;                     // per wave
    const int f0 = wave * qw, f1 = min(nf4, f0 + qw);  // this wave's float4s [f0, f1)
    const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), (short)0, g.n * 4, 0x00020000);
    float xv[XW];  // the x windows, loaded BEFORE the value stream: the LDS writes below wait for them with vmcnt, which counts in
                   // issue order, so they do not wait for the 40 KB of values behind them
#pragma unroll
    for (int t = 0; t < XW; ++t) {
        const int i = (int)threadIdx.x + 256 * t;
        const int k = (i >= g.wbase[1]) + (i >= g.wbase[2]) + (i >= g.wbase[3]) + (i >= g.wbase[4]);
        int dl = g.delta[0] - g.wbase[0];
#pragma unroll
        for (int p = 1; p < 5; ++p)
            if (k == p) dl = g.delta[p] - g.wbase[p];
        const unsigned off = i < g.W ? (unsigned)(r0 + dl + i) * 4u : 0x80000000u;  // (past the windows: reads 0)
        xv[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, off, 0, 0));
    }
    const int ql = (L + 3 + 3) >> 2, nlut = 4 * ql;
    const auto rl = __builtin_amdgcn_make_buffer_rsrc(const_cast<pcmx::i32x4*>(lut_g), (short)0, nlut * 16, 0x00020000);
    pcmx::i32x4 lv[kLutPer];
#pragma unroll
    for (int t = 0; t < kLutPer; ++t)
        lv[t] = __builtin_bit_cast(pcmx::i32x4,
                                   __builtin_amdgcn_raw_buffer_load_b128(rl, ((int)threadIdx.x + 256 * t) * 16, 0, 0));
    __builtin_amdgcn_sched_barrier(0);  // (keep every window / table load ahead of the value stream in issue order)
    // the span's last float4 ends at most 3 values past the block, inside the array: clipped rows always follow
    const auto rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(vals + a0), (short)0, nf4 * 16, 0x00020000);
    pcmx::f32x4 v[NV];
#pragma unroll
    for (int m = 0; m < NV; ++m) {
        const int f = f0 + lane + 64 * m;
        const unsigned off = f < f1 ? (unsigned)f * 16u : 0x80000000u;  // past this wave's quarter: reads 0
        v[m] = __builtin_bit_cast(pcmx::f32x4, __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 2));
    }
    // (unconditional writes: slots past W land in the copy's padding, i - cq < 0 in the previous copy's padding, so
    // no branch keeps a window load from issuing ahead of the value stream)
#pragma unroll
    for (int t = 0; t < XW; ++t) {
        const int i = (int)threadIdx.x + 256 * t;
#pragma unroll
        for (int cq = 0; cq < 4; ++cq) xq[max(cq * wq + i - cq, 0)] = xv[t];
    }
#pragma unroll
    for (int t = 0; t < kLutPer; ++t)
        if ((int)threadIdx.x + 256 * t < nlut) lut4[threadIdx.x + 256 * t] = lv[t];
    if (threadIdx.x < R) ysum[threadIdx.x] = 0.f;
    // the block's first / last value: elements before / past them in the first / last float4 are other rows' values
    if (f0 < f1) {
        if (f0 == 0 && lane == 0) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                if (kk < lead) v[0][kk] = 0.f;
        }
        const int last = nf4 - 1 - f0;  // this wave's index of the block's last float4 (if it holds it)
        if (f1 == nf4 && (last & 63) == lane) {
            const int tail = 4 * nf4 - lead - R * L;  // values past the block in its last float4 (0..3)
#pragma unroll
            for (int m = 0; m < NV; ++m)
                if (m == (last >> 6)) {
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
                        if (kk >= 4 - tail) v[m][kk] = 0.f;
                }
        }
    }
    __syncthreads();
    if (f0 < f1) {
        const float invL = 1.0f / (float)L;
        int cur = max(0, 4 * f0 - lead) / L;  // wave-uniform current row
        float acc = 0.f, accn = 0.f;
        const int elast = min(4 * f1 - lead, R * L) - 1;  // last element of this wave
#pragma unroll
        for (int m = 0; m < NV; ++m) {
            const int ebase = 4 * (f0 + 64 * m) - lead;  // wave-uniform
            if (ebase > elast) break;
            const int e0 = ebase + 4 * lane;  // >= -3 (the block's first float4: its lead values are zeroed)
            const int eend = min(ebase + 255, elast);
            if ((cur + 1) * L - 1 > eend) {
                // fast path (wave-uniform, ~60% of the iterations at L = 620): every element of the iteration is in row
                // cur, so no per-lane row and no per-element row select
                // (lanes past the wave's last element hold zero values; the clamp keeps their slot reads in the table)
                const int j0 = min(e0 - cur * L, L - 1);
                const pcmx::i32x4 lo = lut4[((j0 + 3) & 3) * ql + ((j0 + 3) >> 2)];
                const int sb = e0 - cur * (L - 1);
                const int s0 = sb + lo[0];
                pcmx::f32x4 xs = *reinterpret_cast<const pcmx::f32x4*>(xq + (s0 & 3) * wq + (s0 & ~3));
                if (lo[3] - lo[0] != 3) {  // a band boundary inside the float4
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) xs[kk] = xq[sb + lo[kk]];
                }
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc += v[m][kk] * xs[kk];
                continue;
            }
            // rr0 = floor(e0 / L): (e0 + 0.5) / L is at least 0.5 / L away from an integer, far above the f32 error
            // (e0 in [-3, 0): the product is in (-1, 0) and truncates to row 0)
            const int rr0 = (int)__builtin_fmaf((float)e0, invL, 0.5f * invL);
            const int j0 = e0 - rr0 * L;
            const pcmx::i32x4 lo = lut4[((j0 + 3) & 3) * ql + ((j0 + 3) >> 2)];
            const int sb = e0 - rr0 * (L - 1);
            const int s0 = sb + lo[0];
            pcmx::f32x4 xs = *reinterpret_cast<const pcmx::f32x4*>(xq + (s0 & 3) * wq + (s0 & ~3));
            if (lo[3] - lo[0] != 3) {  // a band or row boundary inside the float4 (a few lanes per iteration)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) xs[kk] = xq[sb + lo[kk]];
            }
            // row cur ends inside this iteration: this lane's elements kk < nc are in row cur, the rest in row cur + 1
            // (the iteration spans at most two rows); one lane-wide total and one masked partial per float4
            const int nc = (cur + 1) * L - e0;
            float pall = 0.f, pcur = 0.f;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                pall = __builtin_fmaf(v[m][kk], xs[kk], pall);
                pcur = __builtin_fmaf(v[m][kk], kk < nc ? xs[kk] : 0.f, pcur);
            }
            acc += pcur;
            accn += pall - pcur;
            // the current row ended inside this iteration (its last element is at or below the iteration's last)
            {
                const float s = pcmx::wave_sum_to_lane63(acc);
                if (lane == 63) atomicAdd(&ysum[cur], s);
                acc = accn, accn = 0.f, ++cur;
            }
        }
        if (cur < R) {  // the wave's range ends inside row cur (its other part belongs to the next wave)
            const float s = pcmx::wave_sum_to_lane63(acc);
            if (lane == 63) atomicAdd(&ysum[cur], s);
        }
    }
    __syncthreads();
    if (threadIdx.x < R) y[r0 + threadIdx.x] = ysum[threadIdx.x];
}

// Variant 8 launch: ONE grid; its first nclip blocks take the clipped first / last row blocks (row blocks [0, nfront)
// and [back0, ...)) with variant 1's row body, the rest stream. Dispatched first, the few clipped blocks (whose cost
// is latency: ~10 us as a launch of their own) overlap the streaming blocks instead of adding to them.
__global__ __launch_bounds__(256) void spmv_banded_stream_kernel(const float* __restrict__ vals,
                                                                 const long long* __restrict__ row_off, int n, int a,
                                                                 int b, int c, int d, int e, int nfront, int back0,
                                                                 int nclip, long long off0, BandGeo g,
                                                                 const pcmx::i32x4* __restrict__ lut_g, int rb_begin,
                                                                 const float* __restrict__ x, float* __restrict__ y) {
    extern __shared__ float sm[];
    const int bid = (int)blockIdx.x;
    if (bid < nclip) {
        const int rb = bid < nfront ? bid : back0 + (bid - nfront);
        banded_rows_body<16, 1>(vals, row_off, n, a, b, c, d, e, x, y, sm, rb * kBandedRows);
        return;
    }
    banded_stream_block(vals, off0, g, lut_g, rb_begin, bid - nclip, x, y, sm);
}

// fallback for rows longer than 16 x 64 nonzeros: one wave per row, strided band loops
__global__ __launch_bounds__(256) void spmv_banded_kernel(const float* __restrict__ vals,
                                                          const long long* __restrict__ row_off, int n, int a, int b,
                                                          int c, int d, int e, const float* __restrict__ x,
                                                          float* __restrict__ y) {
    const int lane = pcmx::lane_id();
    const int row = blockIdx.x * 4 + threadIdx.x / kWave;
    if (row >= n) return;
    int lo[5], hi[5];
    band_limits(n, a, b, c, d, e, row, lo, hi);
    const float* v = vals + row_off[row];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int len = hi[k] - lo[k];
        for (int j = lane; j < len; j += kWave) acc += v[j] * x[lo[k] + j];
        v += len;
    }
    acc = pcmx::wave_reduce<float, 0>(acc);
    if (lane == 0) y[row] = acc;
}
}  // namespace

// Host-side analysis: row_ptr is a HOST array (n_rows+1, int64). Writes up to max_items items into
// `items_host` (4 x int64 words each: row0, row1, nz0, nz1 packed as in Item) and returns the count, or
// -1 if max_items is too small. pcmx_spmv_csr_plan_count() gives the exact count first.
extern "C" long long pcmx_spmv_csr_plan_nnz(const long long* row_ptr, int n_rows, void* items_host,
                                           long long max_items, int item_nnz) {
    if (item_nnz < 64 || item_nnz > kItemNnz || item_nnz % 64) return -1;
    Item* items = reinterpret_cast<Item*>(items_host);
    long long k = 0;
    int r = 0;
    while (r < n_rows) {
        const long long len = row_ptr[r + 1] - row_ptr[r];
        if (len > item_nnz) {  // long row: split into pieces
            for (long long p = row_ptr[r]; p < row_ptr[r + 1]; p += item_nnz) {
                if (items && k < max_items) items[k] = Item{r, r + 1, p, p + item_nnz < row_ptr[r + 1] ? p + item_nnz : row_ptr[r + 1]};
                ++k;
            }
            ++r;
            continue;
        }
        int r1 = r + 1;
        while (r1 < n_rows && row_ptr[r1 + 1] - row_ptr[r] <= item_nnz && r1 - r < kItemRows) ++r1;
        if (items && k < max_items) items[k] = Item{r, r1, row_ptr[r], row_ptr[r1]};
        ++k;
        r = r1;
    }
    if (items && k > max_items) return -1;
    return k;
}

extern "C" long long pcmx_spmv_csr_plan(const long long* row_ptr, int n_rows, void* items_host, long long max_items) {
    return pcmx_spmv_csr_plan_nnz(row_ptr, n_rows, items_host, max_items, kItemNnz);
}

extern "C" int pcmx_spmv_csr(const long long* row_ptr, const int* col, const float* val, const float* x, float* y,
                             int n_rows, const void* items, long long n_items, hipStream_t s) {
    if (n_rows <= 0) return 0;
    PCMX_HIP_RET(hipMemsetAsync(y, 0, sizeof(float) * (size_t)n_rows, s));
    if (n_items <= 0) return 0;
    const long long blocks = (n_items + kWavesPerBlock - 1) / kWavesPerBlock;
    if (blocks > 0x7fffffffLL) return -1;
    spmv_csr_items_kernel<<<(unsigned)blocks, kWavesPerBlock * kWave, 0, s>>>(row_ptr, col, val, x, y,
                                                                               reinterpret_cast<const Item*>(items), n_items);
    return (int)hipGetLastError();
}

namespace {
// Items of 1024 / 512 nonzeros (16 / 8 per lane) exist in both layouts; 384 / 256 (6 / 4 per lane) in the packed one
// only — the short launches of a distributed rank's column-split step give each wave only a few items, so shorter
// items spread the same work over more of them.
bool sliced_item_ok(int item_nnz, bool packed) {
    return item_nnz == 1024 || item_nnz == 512 || (packed && (item_nnz == 384 || item_nnz == 256));
}
bool sliced_blocks_ok(int blocks_per_cu) { return blocks_per_cu >= 0 && blocks_per_cu <= 255; }
}  // namespace

extern "C" int pcmx_spmv_sliced(const unsigned short* lrow, const int* col, const float* val, const float* x,
                                float* ypart, float* extra, float* y, int n_rows, int n_cols, int n_slices,
                                const long long* slice_nz0, const long long* slice_item0, const long long* slice_out0,
                                const void* items, const unsigned* row_mask, const int* chunk_base, const void* fix,
                                int n_fix, int item_nnz, int stage, int ballot_combine, int blocks_per_cu, int phase_lo,
                                int phase_n, const int* slice_colbase, hipStream_t s) {
    if (!sliced_item_ok(item_nnz, slice_colbase != nullptr) || !sliced_blocks_ok(blocks_per_cu) ||
        (stage != PCMX_SPMV_ALL && stage != PCMX_SPMV_PRODUCTS && stage != PCMX_SPMV_COMBINE) ||
        (ballot_combine != 0 && ballot_combine != 1) || phase_lo < 0 || phase_n < 0)
        return PCMX_ERR_ARG;
    if (n_rows <= 0) return 0;
    if (n_slices <= 0 || n_slices % 8 || n_slices > kMaxSlices) return (int)hipErrorInvalidValue;
    const int persist_blocks = blocks_per_cu ? blocks_per_cu : kPersistBlocks;
    // the product launch covers phases [ph_lo, ph_lo + ph_n) (8 slices, one per XCD, per phase): a column-split
    // caller multiplies the slices of the columns it already holds first
    const int ph_all = n_slices / 8, ph_lo = phase_lo, ph_n = phase_n ? phase_n : ph_all - ph_lo;
    if (ph_lo + ph_n > ph_all || ph_n <= 0) return (int)hipErrorInvalidValue;
    SliceMeta meta{};
    SliceOut so{};
    long long most = 0;
    for (int k = 0; k < n_slices; ++k) {
        meta.nz0[k] = slice_nz0[k];
        meta.item0[k] = slice_item0[k];
        meta.out0[k] = so.out0[k] = slice_out0[k];
        if (slice_item0[k + 1] < slice_item0[k]) return (int)hipErrorInvalidValue;
        if (k >= 8 * ph_lo && k < 8 * (ph_lo + ph_n))
            most = slice_item0[k + 1] - slice_item0[k] > most ? slice_item0[k + 1] - slice_item0[k] : most;
    }
    meta.item0[n_slices] = slice_item0[n_slices];
    for (int k = 0; k < n_slices; ++k) {
        meta.colbase[k] = slice_colbase ? slice_colbase[k] : 0;
        meta.item1[k] = slice_item0[k + 1];
    }
    so.out0[n_slices] = slice_out0[n_slices];
    // PCMX_SPMV_PRODUCTS: no combine / fix-up, PCMX_SPMV_COMBINE: combine + fix-up only — a row-chunked caller runs
    // chunk q's combine on a second stream while chunk q + 1's products run
    if (most > 0 && stage != PCMX_SPMV_COMBINE) {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            cus = 256;
        const long long need = (most + kWavesPerBlock - 1) / kWavesPerBlock;
        const long long per = (long long)(cus / 8) * persist_blocks;  // resident blocks per XCD
        const int bp = (int)(need < per ? need : per);
        const unsigned nb = (unsigned)(bp * 8 * ph_n);
        const Item* it = reinterpret_cast<const Item*>(items);
        const dim3 blk(kWavesPerBlock * kWave);
#define PCMX_SLICED(PACKED, PL) \
    spmv_sliced_kernel<PACKED, PL><<<nb, blk, 0, s>>>(lrow, col, val, x, n_cols, ypart, extra, it, meta, bp, ph_lo)
        // slice_colbase != NULL: col holds the packed words (production layout when every slice is < 2^21 columns)
        if (slice_colbase) {
            switch (item_nnz) {
                case 256: PCMX_SLICED(true, 4); break;
                case 384: PCMX_SLICED(true, 6); break;
                case 512: PCMX_SLICED(true, 8); break;
                default: PCMX_SLICED(true, 16); break;
            }
        } else if (item_nnz == 512) {
            PCMX_SLICED(false, 8);
        } else {
            PCMX_SLICED(false, 16);
        }
#undef PCMX_SLICED
    }
    if (stage == PCMX_SPMV_PRODUCTS) return (int)hipGetLastError();
    const unsigned cb = (unsigned)((n_rows + 2047) / 2048) * 8;  // 4 waves of 64 rows per block, 8k blocks
    // ballot_combine: the ballot-rank combine instead of the byte-packed scan (bit-identical results; the tests'
    // oracle of the scan). The scan form addresses the partials with 32-bit byte offsets, so 2^30 partials or more
    // take the ballot form whatever the caller asked for.
    const bool ballot = ballot_combine || so.out0[n_slices] >= (1ll << 30);
#define PCMX_COMBINE(K)                                                                                            \
    do {                                                                                                           \
        if (ballot) spmv_combine_kernel<K><<<cb, 256, 0, s>>>(ypart, row_mask, chunk_base, so, y, n_rows);         \
        else spmv_combine_scan_kernel<K><<<cb, 256, 0, s>>>(ypart, row_mask, chunk_base, so, y, n_rows);           \
    } while (0)
    switch (n_slices) {
        case 8: PCMX_COMBINE(8); break;
        case 16: PCMX_COMBINE(16); break;
        case 24: PCMX_COMBINE(24); break;
        case 32: PCMX_COMBINE(32); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef PCMX_COMBINE
    if (n_fix > 0)
        spmv_fixup_kernel<<<(n_fix + 3) / 4, 256, 0, s>>>(extra, reinterpret_cast<const int2*>(fix), n_fix, y);
    return (int)hipGetLastError();
}

// Round 5: the products (no combine) of phases [a_lo, a_lo + a_n) of sliced matrix A and [b_lo, b_lo + b_n) of sliced
// matrix B — two matrices over the SAME x, e.g. the two row chunks of a distributed column-split step multiplying their
// chunk-0 columns — in ONE launch: a launch of a few items per wave pays its ramp and tail once instead of twice.
// Production layout only (packed index stream); item_nnz 256 / 384 / 512 / 1024, the same for both matrices.
// meta_*: host arrays nz0 (S), item0 (S + 1), out0 (S + 1), colbase (S) of each matrix.
extern "C" int pcmx_spmv_sliced_pair(const float* x, int n_cols, int item_nnz, int blocks_per_cu, const int* col_a,
                                     const float* val_a, const void* items_a, float* ypart_a, float* extra_a, int s_a,
                                     const long long* nz0_a, const long long* item0_a, const long long* out0_a,
                                     const int* colbase_a, int a_lo, int a_n, const int* col_b, const float* val_b,
                                     const void* items_b, float* ypart_b, float* extra_b, int s_b,
                                     const long long* nz0_b, const long long* item0_b, const long long* out0_b,
                                     const int* colbase_b, int b_lo, int b_n, hipStream_t s) {
    if (!sliced_item_ok(item_nnz, true) || !sliced_blocks_ok(blocks_per_cu)) return PCMX_ERR_ARG;
    if (s_a % 8 || s_b % 8 || a_lo < 0 || b_lo < 0 || a_n < 0 || b_n < 0 || 8 * (a_lo + a_n) > s_a ||
        8 * (b_lo + b_n) > s_b || 8 * (a_n + b_n) > kMaxSlices)
        return (int)hipErrorInvalidValue;
    if (a_n + b_n == 0) return 0;
    SliceMeta meta{};
    long long most = 0;
    int m = 0;
    auto add = [&](int k, const long long* nz0, const long long* item0, const long long* out0, const int* colbase,
                   int part) {
        meta.nz0[m] = nz0[k], meta.item0[m] = item0[k], meta.item1[m] = item0[k + 1], meta.out0[m] = out0[k];
        meta.colbase[m] = colbase[k], meta.part[m] = (unsigned char)part;
        most = std::max(most, item0[k + 1] - item0[k]);
        return item0[k + 1] >= item0[k];
    };
    for (int k = 8 * a_lo; k < 8 * (a_lo + a_n); ++k, ++m)
        if (!add(k, nz0_a, item0_a, out0_a, colbase_a, 0)) return (int)hipErrorInvalidValue;
    for (int k = 8 * b_lo; k < 8 * (b_lo + b_n); ++k, ++m)
        if (!add(k, nz0_b, item0_b, out0_b, colbase_b, 1)) return (int)hipErrorInvalidValue;
    meta.b = SlicePart{col_b, val_b, nullptr, reinterpret_cast<const Item*>(items_b), ypart_b, extra_b};
    if (most <= 0) return 0;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        cus = 256;
    const int persist_blocks = blocks_per_cu ? blocks_per_cu : kPersistBlocks;
    const long long need = (most + kWavesPerBlock - 1) / kWavesPerBlock;
    const long long per = (long long)(cus / 8) * persist_blocks;
    const int bp = (int)(need < per ? need : per);
    const unsigned nb = (unsigned)(bp * (m / 8) * 8);
    const Item* ia = reinterpret_cast<const Item*>(items_a);
    const dim3 blk(kWavesPerBlock * kWave);
#define PCMX_PAIR(PL) \
    spmv_sliced_kernel<true, PL, true><<<nb, blk, 0, s>>>(nullptr, col_a, val_a, x, n_cols, ypart_a, extra_a, ia, meta, bp, 0)
    switch (item_nnz) {
        case 256: PCMX_PAIR(4); break;
        case 384: PCMX_PAIR(6); break;
        case 512: PCMX_PAIR(8); break;
        default: PCMX_PAIR(16); break;
    }
#undef PCMX_PAIR
    return (int)hipGetLastError();
}

// Round 5: the combine + fix-up (+ send-buffer pack) of a sliced product in ONE launch (spmv_combine_fused_kernel), for
// a caller that ran the products alone (pcmx_spmv_sliced with stage PCMX_SPMV_PRODUCTS). slice_out0: n_slices + 1 partial offsets;
// fix_chunk0: n_rows / 64 + 2 entries (or null: no split rows); send_ptr / send_slot / sendbuf: the pack (or null).
extern "C" int pcmx_spmv_sliced_combine(const float* ypart, const unsigned* row_mask, const int* chunk_base,
                                        const long long* slice_out0, int n_slices, float* y, int n_rows,
                                        const float* extra, const void* fix, const int* fix_chunk0, const int* send_ptr,
                                        const int* send_slot, float* sendbuf, hipStream_t s) {
    if (n_rows <= 0) return 0;
    if (n_slices <= 0 || n_slices % 8 || n_slices > kMaxSlices || (fix_chunk0 && !fix) ||
        (send_ptr && (!send_slot || !sendbuf)) || slice_out0[n_slices] >= (1ll << 30))
        return (int)hipErrorInvalidValue;
    SliceOut so{};
    for (int k = 0; k <= n_slices; ++k) so.out0[k] = slice_out0[k];
    const unsigned cb = (unsigned)((n_rows + 2047) / 2048) * 8;  // 4 waves of 64 rows per block, XCD-contiguous order
    const int2* fx = reinterpret_cast<const int2*>(fix);
#define PCMX_FUSED(K)                                                                                              \
    spmv_combine_fused_kernel<K><<<cb, 256, 0, s>>>(ypart, row_mask, chunk_base, so, y, n_rows, extra, fx, fix_chunk0, \
                                                    send_ptr, send_slot, sendbuf)
    switch (n_slices) {
        case 8: PCMX_FUSED(8); break;
        case 16: PCMX_FUSED(16); break;
        case 24: PCMX_FUSED(24); break;
        case 32: PCMX_FUSED(32); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef PCMX_FUSED
    return (int)hipGetLastError();
}

namespace {
// host twin of band_limits (the launcher derives variant 8's window geometry from one unclipped row)
void band_limits_host(int n, int a, int b, int c, int d, int e, int row, int (&lo)[5], int (&hi)[5]) {
    const int ah = a / 2;
    const int r5 = ah, r6 = ah + b, r7 = ah + b + c, r8 = ah + b + c + d, r9 = ah + b + c + d + e;
    lo[0] = std::max(0, row - r9), hi[0] = std::max(0, row - r8);
    lo[1] = std::max(0, row - r7), hi[1] = std::max(0, row - r6);
    lo[2] = std::max(0, row - r5), hi[2] = std::min(row + r5 + 1, n);
    lo[3] = std::min(n, row + r6 + 1), hi[3] = std::min(n, row + r7 + 1);
    lo[4] = std::min(n, row + r8 + 1), hi[4] = std::min(n, row + r9 + 1);
    for (int k = 0; k < 5; ++k) hi[k] = std::max(hi[k], lo[k]);
}
}  // namespace

namespace {
constexpr int kStreamNotApplicable = -1000;

// Variant 8's slot table for one geometry (see banded_stream_block): lut4[j + 3] for j in [-3, L), entry jj = j + 3
// stored phase-major at (jj & 3) * ql + (jj >> 2) (the lanes of one row read positions 4 apart, i.e. consecutive entries
// of one phase table: 16-B lane stride, no bank conflicts). lut4[j][kk] = kk + lut(j + kk), or past the row end
// kk - (L - 1) + lut(j + kk - L) (the next row); the block's first float4 starts up to 3 values before its first element
// (j < 0, row 0): those (zeroed) values read slot 0. Built on the host once per (device, geometry) and kept in device
// memory for the life of the process (a few KB per geometry). The first call per geometry allocates and copies on
// stream s (stream-ordered: the copy lands before the launch that reads it; the host table stays cached so the async
// copy never reads freed memory). Inside a stream capture no HIP allocation may run: an uncached table returns nullptr
// there and the caller launches variant 1 instead.
const pcmx::i32x4* banded_lut_table(const BandGeo& g, hipStream_t s) {
    static std::mutex mu;
    static std::map<std::vector<int>, std::pair<void*, std::vector<int>>> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::vector<int> key{dev, g.L};
    key.insert(key.end(), g.wbase, g.wbase + 6);
    key.insert(key.end(), g.cum, g.cum + 5);
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return reinterpret_cast<const pcmx::i32x4*>(it->second.first);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (cap != hipStreamCaptureStatusNone) return nullptr;
    const int L = g.L, ql = (L + 6) >> 2;
    auto lut = [&](int j) {  // window base - first position of j's band
        const int k = (j >= g.cum[1]) + (j >= g.cum[2]) + (j >= g.cum[3]) + (j >= g.cum[4]);
        return g.wbase[k] - g.cum[k];
    };
    std::vector<int> tab((size_t)16 * ql, 0);  // 4 * ql entries of 4 ints
    for (int j = -3; j < L; ++j) {
        const int jj = j + 3, ent = (jj & 3) * ql + (jj >> 2);
        for (int kk = 0; kk < 4; ++kk)
            tab[4 * ent + kk] = j + kk < 0 ? -j : j + kk < L ? kk + lut(j + kk) : kk - (L - 1) + lut(j + kk - L);
    }
    void* d = nullptr;
    if (hipMalloc(&d, tab.size() * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();  // (clear it: the caller falls back to variant 1 and reports that launch's status)
        return nullptr;
    }
    auto& ent = cache[key];
    ent.second = std::move(tab);
    // the upload completes before the pointer is cached and returned (once per geometry; never inside a capture,
    // see above): a later caller on ANOTHER stream finds the cached table and must not read it before the copy on s
    // has landed
    if (hipMemcpyAsync(d, ent.second.data(), ent.second.size() * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        cache.erase(key);
        (void)hipFree(d);
        (void)hipGetLastError();
        return nullptr;
    }
    ent.first = d;
    return reinterpret_cast<const pcmx::i32x4*>(d);
}
// Which banded kernel a call takes, decided from the geometry alone: the ONE place the dispatch conditions live (the
// launcher below and the pcmx_spmv_banded_path query both read it). path 0: one wave per row; 1: the LDS-window kernel
// spmv_banded_lds_kernel<nl>; 8: the block stream, which the launcher may still turn into 1 (a stream capture or a failed
// table allocation, banded_lut_table); PCMX_ERR_ARG: refused. The other fields are what the launches need.
struct BandedPlan {
    int path, nl;             // nl: the LDS kernel's instantiation (also the fallback of path 8; 0 for path 0)
    int L, W;                 // nonzeros of an unclipped row, variant 8's window floats per block
    int rb_lo, rb_hi, nrb;    // row blocks [rb_lo, rb_hi) hold unclipped rows only; nrb row blocks in all
    size_t lds, lds8;         // dynamic LDS of the row body (variant 1, variant 8's clipped blocks) / of a stream block
};
BandedPlan banded_plan(int n, int a, int b, int c, int d, int e, int variant, bool vals_aligned) {
    constexpr int RS = kBandedRows, NV = kStreamNV, XW = kStreamXW;
    BandedPlan p{};
    p.path = PCMX_ERR_ARG;
    // 0: one wave per row; 1: LDS-staged x windows, 16 rows per block, 2 rows per wave in flight; 8: block stream
    // (16-B loads over each 16-row block's contiguous value range, spmv_banded_stream_kernel), the production path
    if (a < 1 || b < 0 || c < 0 || d < 0 || e < 0 || (variant != 0 && variant != 1 && variant != 8)) return p;
    const long long maxrow = 2LL * (a / 2) + 1 + 2LL * c + 2LL * e;  // nonzeros of an unclipped row
    const long long nl = (maxrow + 63) / 64;
    p.lds = (size_t)(maxrow + 5 * (RS - 1)) * sizeof(float);
    if (variant == 0 || nl > 16 || p.lds > 64 * 1024) {  // rows longer than 16 x 64 nonzeros: the wave-per-row kernel
        p.path = 0;
        return p;
    }
    p.path = 1;
    p.nl = nl <= 2 ? 2 : nl <= 4 ? 4 : nl <= 6 ? 6 : nl <= 8 ? 8 : nl <= 10 ? 10 : nl <= 12 ? 12 : 16;
    if (variant != 8) return p;
    // rows [rlo, rhi) are unclipped (every band inside [0, n)) and all hold L nonzeros
    const int ah = a / 2, r9 = ah + b + c + d + e;
    const int L = (int)maxrow;
    const int rlo = r9, rhi = n - r9;
    p.L = L, p.W = L + 5 * (RS - 1);
    p.rb_lo = (rlo + RS - 1) / RS, p.rb_hi = rhi >= 0 ? rhi / RS : 0, p.nrb = (n + RS - 1) / RS;
    const long long q = ((long long)L * RS + 6) / 16;  // float4s per wave quarter (lead <= 3)
    p.lds8 = (size_t)(4 * 256 * XW + ((RS + 3) & ~3) + 16 * ((L + 6) / 4)) * sizeof(float);
    // the wave-iteration rule needs rows of >= 256 nonzeros, the float4 stream a 16-B aligned vals; the register
    // sets hold NV float4s per lane and XW window floats per thread; the clipped body NL = 16 chunks of 64
    // (short rows or unaligned values: variant 1 runs instead)
    const bool ok = L >= 256 && L <= 16 * 64 && 4 * ((L + 6) / 4) <= 256 * kLutPer && q <= 64 * NV &&
                    p.W + 3 <= XW * 256 && p.rb_hi > p.rb_lo && vals_aligned && p.lds8 <= 64 * 1024;
    if (ok) p.path = 8;
    return p;
}

// Variant 8 launch (block stream over the unclipped rows, the clipped row blocks folded into the same grid) of a plan
// whose path is 8; kStreamNotApplicable when the slot table cannot be had (the caller launches variant 1 instead).
int launch_banded_stream(const BandedPlan& p, const float* vals, const long long* row_off, int n, int a, int b, int c,
                         int d, int e, const float* x, float* y, hipStream_t s) {
    constexpr int RS = kBandedRows;
    const int rlo = a / 2 + b + c + d + e, rb_lo = p.rb_lo, rb_hi = p.rb_hi;
    BandGeo g{};
    g.L = p.L, g.W = p.W, g.n = n;
    {
        int lo[5], hi[5], wb = 0, cs = 0;
        band_limits_host(n, a, b, c, d, e, rlo, lo, hi);
        for (int k = 0; k < 5; ++k) {
            g.delta[k] = lo[k] - rlo, g.wbase[k] = wb, g.cum[k] = cs;
            wb += hi[k] - lo[k] + RS - 1;
            cs += hi[k] - lo[k];
        }
        g.wbase[5] = wb;
    }
    // (the first call per geometry allocates the table and copies it on s; inside a stream capture, or if that fails,
    // variant 1 runs instead)
    const pcmx::i32x4* lut_g = banded_lut_table(g, s);
    if (!lut_g) return kStreamNotApplicable;
    const int nfront = rb_lo, back0 = rb_hi, nback = p.nrb - rb_hi;
    // first value of row rb_lo * RS: the nonzeros of the clipped rows before it (host sum of row lengths)
    long long off0 = 0;
    for (int r = 0; r < rb_lo * RS; ++r) {
        int lo[5], hi[5];
        band_limits_host(n, a, b, c, d, e, r, lo, hi);
        for (int k = 0; k < 5; ++k) off0 += hi[k] - lo[k];
    }
    spmv_banded_stream_kernel<<<nfront + nback + rb_hi - rb_lo, 256, std::max(p.lds, p.lds8), s>>>(
        vals, row_off, n, a, b, c, d, e, nfront, back0, nfront + nback, off0, g, lut_g, rb_lo, x, y);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" int pcmx_spmv_banded_path(int n, int a, int b, int c, int d, int e, int variant, int vals_aligned, int* nl) {
    const BandedPlan p = banded_plan(n, a, b, c, d, e, variant, vals_aligned != 0);
    if (nl) *nl = p.nl;
    return p.path;
}

extern "C" int pcmx_spmv_banded_variant(const float* vals, const long long* row_off, int n, int a, int b, int c, int d,
                                        int e, const float* x, float* y, int variant, hipStream_t s) {
    if (n <= 0) return 0;
    const BandedPlan p = banded_plan(n, a, b, c, d, e, variant, !((uintptr_t)vals & 15));
    if (p.path < 0) return p.path;
    if (p.path == 0) {
        spmv_banded_kernel<<<(n + 3) / 4, 256, 0, s>>>(vals, row_off, n, a, b, c, d, e, x, y);
        return (int)hipGetLastError();
    }
    if (p.path == 8) {
        // (a stream capture or a failed table allocation: variant 1 runs instead)
        const int rc = launch_banded_stream(p, vals, row_off, n, a, b, c, d, e, x, y, s);
        if (rc != kStreamNotApplicable) return rc;
    }
    const int grid = (n + kBandedRows - 1) / kBandedRows;
#define PCMX_BANDED(NL) \
    case NL: spmv_banded_lds_kernel<NL><<<grid, 256, p.lds, s>>>(vals, row_off, n, a, b, c, d, e, x, y); break
    switch (p.nl) {
        PCMX_BANDED(2);
        PCMX_BANDED(4);
        PCMX_BANDED(6);
        PCMX_BANDED(8);
        PCMX_BANDED(10);
        PCMX_BANDED(12);
        default: PCMX_BANDED(16);
    }
#undef PCMX_BANDED
    return (int)hipGetLastError();
}

extern "C" int pcmx_spmv_banded(const float* vals, const long long* row_off, int n, int a, int b, int c, int d, int e,
                                const float* x, float* y, hipStream_t s) {
    return pcmx_spmv_banded_variant(vals, row_off, n, a, b, c, d, e, x, y, 8, s);  // (falls back to 1 when needed)
}
