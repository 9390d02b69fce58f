// SpMM on MI355X: Y[n_rows, k] = A · X[n_cols, k], A in CSR (int64 row_ptr, int32 col, f32 val), X and Y row-major
// f32 with leading dimensions ldx, ldy >= k.
//
// Work items are the nnz-balanced items of the SpMV planner (pcmx_spmv_csr_plan_nnz: runs of short rows packed into
// one item, a row longer than the item size split into pieces), one wave per item and column tile, 4 waves per block.
//
// Wide classes (k > 32): the LANES RUN ACROSS THE DENSE COLUMNS, so a nonzero's gather of X[col, tile] is one
// coalesced wave load of 64 C floats, C = 1, 2 or 4 floats per lane (tiles of 64, 128, 256 columns). k > 256 runs as
// tiles of 256 on grid.y; the last, partial tile takes the smallest 64 C that covers it in a launch of its own, the
// lanes at or past k masked (their loads and stores are predicated off). With X, Y and both leading dimensions aligned
// to the vector, a lane owns C adjacent columns and moves them as one float2 / float4; otherwise it owns columns
// lane + 64 j and moves dwords (same class, "dword form"). A wave walks its item's nonzeros flat in ascending order:
// 64 columns / values at a time sit in one register per lane (the next 64 are prefetched), each nonzero's column and
// value reach the whole wave by a v_readlane, the loads of a group of kGroup nonzeros are issued first and their FMAs
// follow in nonzero order. The item's row pointers are staged in LDS; the row border is wave-uniform: store the
// accumulator, reset it. No partial sum ever crosses lanes, so column c of Y depends on column c of X only.
//
// Narrow classes (whole k <= 32): KP = 4, 8, 16 or 32 lanes per group (the smallest KP >= k), 64 / KP groups per wave
// (k = 33 .. 63 has no such KP and runs as one masked 64-column tile of the wide kernel).
// T groups share a row (T a power of two from the item's average row length, the plain CSR kernel's lanes-per-row
// rule), the 64 / (KP T) teams take the item's rows round-robin; group t of a team sums the row's nonzeros t, t + T,
// ... in ascending order and the T partial sums are combined by an xor butterfly (fixed order).
//
// Split rows without atomics or a memset: a piece writes its k-wide partial row into workspace slot slot[item]
// (row stride k rounded up to 4), and spmm_fixup_kernel sums each split row's pieces in ascending piece order into Y.
// Every other row of Y is written by exactly one wave (an empty row as +0.0), so the bits of Y depend only on the
// matrix, the item size, k and the data.
//
// All row addressing (col * ldx, row * ldy, slot * ldw) is 64-bit; plain global loads and stores, no buffer
// descriptors, no inline assembly, no block waits for another.
#include "pcmx_common.h"
#include "pcmx_hip.h"

namespace {
using pcmx::kWave;
constexpr int kWavesPerBlock = 4;
constexpr int kItemNnzMax = 1024;
constexpr int kNarrowMax = 32;  // widest k of the narrow classes (33 .. 63 columns take the 64-column tile, masked)
constexpr int kItemRows = 1023;  // the planner's rows-per-item cap (spmv.hip): bounds the row-pointer LDS stage

struct Item {              // as written by pcmx_spmv_csr_plan_nnz
    int row0, row1;        // rows [row0, row1) (row1 == row0 + 1 for a piece of a split row)
    long long nz0, nz1;    // nonzeros [nz0, nz1)
};

template <int C>
struct VecOf;
template <>
struct VecOf<2> {
    using type = float2;
};
template <>
struct VecOf<4> {
    using type = float4;
};

// One lane's C columns of a tile row at p (the tile's first column), kt valid columns in the tile.
// VEC: columns C lane .. C lane + C - 1 as one vector (a lane the mask cuts falls back to dwords); else lane + 64 j.
template <int C, bool VEC>
__device__ __forceinline__ void load_cols(const float* __restrict__ p, int lane, int kt, float (&r)[C]) {
    if constexpr (VEC) {
        const int nv = kt - C * lane;
        if (nv >= C) {
            const auto v = *reinterpret_cast<const typename VecOf<C>::type*>(p + C * lane);
            const float* f = reinterpret_cast<const float*>(&v);
#pragma unroll
            for (int j = 0; j < C; ++j) r[j] = f[j];
        } else {
#pragma unroll
            for (int j = 0; j < C; ++j) r[j] = j < nv ? p[C * lane + j] : 0.f;
        }
    } else {
#pragma unroll
        for (int j = 0; j < C; ++j) r[j] = lane + kWave * j < kt ? p[lane + kWave * j] : 0.f;
    }
}

template <int C, bool VEC>
__device__ __forceinline__ void store_cols(float* __restrict__ p, int lane, int kt, const float (&r)[C]) {
    if constexpr (VEC) {
        const int nv = kt - C * lane;
        if (nv >= C) {
            typename VecOf<C>::type v;
            float* f = reinterpret_cast<float*>(&v);
#pragma unroll
            for (int j = 0; j < C; ++j) f[j] = r[j];
            *reinterpret_cast<typename VecOf<C>::type*>(p + C * lane) = v;
        } else {
#pragma unroll
            for (int j = 0; j < C; ++j)
                if (j < nv) p[C * lane + j] = r[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < C; ++j)
            if (lane + kWave * j < kt) p[lane + kWave * j] = r[j];
    }
}

// ------------------------------------------------------------------------------------------ wide classes
template <int C, bool VEC, int kGroup>
__global__ __launch_bounds__(kWavesPerBlock * kWave) void spmm_wide_kernel(
    const long long* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ val,
    const float* __restrict__ x, long long ldx, float* __restrict__ y, long long ldy, float* __restrict__ ws,
    long long ldw, const Item* __restrict__ items, long long n_items, const int* __restrict__ slot, int col_base,
    int k) {
    __shared__ int rps[kWavesPerBlock][kItemRows + 1];
    const int w = threadIdx.x / kWave, lane = pcmx::lane_id();
    const long long it = (long long)blockIdx.x * kWavesPerBlock + w;
    if (it >= n_items) return;
    const int c0 = col_base + (int)blockIdx.y * (kWave * C);  // the tile's first column
    const int kt = min(k - c0, kWave * C);                    // its valid columns
    const Item item = items[it];
    const long long nz0 = item.nz0;
    const int n = (int)(item.nz1 - nz0);
    const int nrows = item.row1 - item.row0;
    const int sl = slot[it];
    // where the item's row r goes: a piece of a split row (one row) into its workspace slot
    float* const dst = sl >= 0 ? ws + (long long)sl * ldw + c0 : y + (long long)item.row0 * ldy + c0;
    int* rp = rps[w];
    if (nrows > 1) {
        for (int i = lane; i <= nrows; i += kWave) rp[i] = (int)(row_ptr[item.row0 + i] - nz0);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
    const float* const xt = x + c0;
    float acc[C];
#pragma unroll
    for (int j = 0; j < C; ++j) acc[j] = 0.f;
    int r = 0;                                                              // current row of the item
    int rend = nrows > 1 ? __builtin_amdgcn_readfirstlane(rp[1]) : n;      // its end, relative to nz0
    int cj = lane < n ? col[nz0 + lane] : 0;
    float vj = lane < n ? val[nz0 + lane] : 0.f;
    for (int base = 0; base < n; base += kWave) {
        const int nb = base + kWave + lane;  // prefetch the next 64 columns / values
        const int cn = nb < n ? col[nz0 + nb] : 0;
        const float vn = nb < n ? val[nz0 + nb] : 0.f;
        const int m = min(kWave, n - base);
        for (int l0 = 0; l0 < m; l0 += kGroup) {
            float xr[kGroup][C];
#pragma unroll
            for (int g = 0; g < kGroup; ++g)
                if (l0 + g < m) {
                    const int c = __builtin_amdgcn_readlane(cj, l0 + g);
                    load_cols<C, VEC>(xt + (long long)c * ldx, lane, kt, xr[g]);
                }
#pragma unroll
            for (int g = 0; g < kGroup; ++g)
                if (l0 + g < m) {
                    const int i = base + l0 + g;
                    while (i == rend) {  // row border (wave-uniform); an empty row stores +0.0
                        store_cols<C, VEC>(dst + (long long)r * ldy, lane, kt, acc);
#pragma unroll
                        for (int j = 0; j < C; ++j) acc[j] = 0.f;
                        ++r;
                        rend = __builtin_amdgcn_readfirstlane(rp[r + 1]);
                    }
                    const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vj), l0 + g));
#pragma unroll
                    for (int j = 0; j < C; ++j) acc[j] = fmaf(v, xr[g][j], acc[j]);
                }
        }
        cj = cn, vj = vn;
    }
    for (; r < nrows; ++r) {  // the last row with nonzeros and the empty rows behind it
        store_cols<C, VEC>(dst + (long long)r * ldy, lane, kt, acc);
#pragma unroll
        for (int j = 0; j < C; ++j) acc[j] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------ narrow classes (k <= 32)
template <int KP>
__global__ __launch_bounds__(kWavesPerBlock * kWave) void spmm_narrow_kernel(
    const long long* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ val,
    const float* __restrict__ x, long long ldx, float* __restrict__ y, long long ldy, float* __restrict__ ws,
    long long ldw, const Item* __restrict__ items, long long n_items, const int* __restrict__ slot, int k) {
    constexpr int NG = kWave / KP;  // groups per wave
    const int w = threadIdx.x / kWave, lane = pcmx::lane_id();
    const long long it = (long long)blockIdx.x * kWavesPerBlock + w;
    if (it >= n_items) return;
    const Item item = items[it];
    const int n = (int)(item.nz1 - item.nz0);
    const int nrows = item.row1 - item.row0;
    const int sl = slot[it];
    // T groups per row: about avg-row-length / 4, a power of two (the plain CSR kernel's lanes-per-row rule)
    const int avg = n / nrows;
    int T = 1;
    while (T < NG && T * 4 < avg) T <<= 1;
    const int c = lane % KP, g = lane / KP, t = g & (T - 1), team = g / T, nteams = NG / T;
    const bool on = c < k;
    const float* const xc = x + c;
    for (int r = team; r < nrows; r += nteams) {
        const long long b = nrows == 1 ? item.nz0 : row_ptr[item.row0 + r];
        const long long e = nrows == 1 ? item.nz1 : row_ptr[item.row0 + r + 1];
        float acc = 0.f;
        long long p = b + t;
        for (; p + 3 * T < e; p += 4 * T) {  // 4 X rows in flight per group
            const int c0 = col[p], c1 = col[p + T], c2 = col[p + 2 * T], c3 = col[p + 3 * T];
            const float v0 = val[p], v1 = val[p + T], v2 = val[p + 2 * T], v3 = val[p + 3 * T];
            const float x0 = on ? xc[(long long)c0 * ldx] : 0.f, x1 = on ? xc[(long long)c1 * ldx] : 0.f;
            const float x2 = on ? xc[(long long)c2 * ldx] : 0.f, x3 = on ? xc[(long long)c3 * ldx] : 0.f;
            acc = fmaf(v0, x0, acc), acc = fmaf(v1, x1, acc), acc = fmaf(v2, x2, acc), acc = fmaf(v3, x3, acc);
        }
        for (; p < e; p += T) {
            const float xv = on ? xc[(long long)col[p] * ldx] : 0.f;
            acc = fmaf(val[p], xv, acc);
        }
        for (int off = T >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off * KP, kWave);
        if (t == 0 && on) {
            float* const d = sl >= 0 ? ws + (long long)sl * ldw : y + (long long)(item.row0 + r) * ldy;
            d[c] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------ split-row fix-up
// split[s] = {row, first slot, pieces}: Y[row, :] = the pieces' partial rows summed in ascending piece order.
__global__ __launch_bounds__(256) void spmm_fixup_kernel(const float* __restrict__ ws, long long ldw,
                                                         const int* __restrict__ split, float* __restrict__ y,
                                                         long long ldy, int k) {
    const int row = split[3 * (long long)blockIdx.x], first = split[3 * (long long)blockIdx.x + 1];
    const int pieces = split[3 * (long long)blockIdx.x + 2];
    const float* const w0 = ws + (long long)first * ldw;
    for (int c = threadIdx.x; c < k; c += blockDim.x) {
        float acc = w0[c];
        for (int p = 1; p < pieces; ++p) acc += w0[(long long)p * ldw + c];
        y[(long long)row * ldy + c] = acc;
    }
}

struct Path {
    int cls, tail, vec;  // first tile's class (lanes per group, or tile columns), the partial last tile's, vector bits
};

bool aligned(unsigned long long xa, long long ldx, unsigned long long ya, long long ldy, int C) {
    return C > 1 && xa % (4u * C) == 0 && ya % (4u * C) == 0 && ldx % C == 0 && ldy % C == 0;
}

// the one predicate the launcher dispatches on and pcmx_spmm_path reports
bool spmm_path(int k, unsigned long long xa, long long ldx, unsigned long long ya, long long ldy, Path* p) {
    if (k < 0 || ldx < k || ldy < k) return false;
    *p = Path{0, 0, 0};
    if (k == 0) return true;
    if (k <= kNarrowMax) {
        p->cls = k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32;
        return true;
    }
    const int rem = k % 256;
    const int rc = rem == 0 ? 0 : rem <= 64 ? 64 : rem <= 128 ? 128 : 256;
    if (k >= 256) {
        p->cls = 256, p->tail = rc;
    } else {
        p->cls = rc;
    }
    if (aligned(xa, ldx, ya, ldy, p->cls / kWave)) p->vec |= 1;
    if (p->tail && aligned(xa, ldx, ya, ldy, p->tail / kWave)) p->vec |= 2;
    return true;
}

template <int C, bool VEC>
void launch_wide(dim3 grid, hipStream_t s, const long long* row_ptr, const int* col, const float* val, const float* x,
                 long long ldx, float* y, long long ldy, float* ws, long long ldw, const void* items, long long n_items,
                 const int* slot, int col_base, int k) {
    constexpr int kGroup = C == 4 ? 4 : 8;  // X-row loads in flight per wave
    spmm_wide_kernel<C, VEC, kGroup><<<grid, kWavesPerBlock * kWave, 0, s>>>(
        row_ptr, col, val, x, ldx, y, ldy, ws, ldw, reinterpret_cast<const Item*>(items), n_items, slot, col_base, k);
}
}  // namespace

extern "C" int pcmx_spmm_path(int k, unsigned long long x_addr, long long ldx, unsigned long long y_addr,
                              long long ldy, int* tail_class, int* vec) {
    Path p;
    if (!spmm_path(k, x_addr, ldx, y_addr, ldy, &p)) return PCMX_ERR_ARG;
    if (tail_class) *tail_class = p.tail;
    if (vec) *vec = p.vec;
    return p.cls;
}

extern "C" int pcmx_spmm_csr(const long long* row_ptr, const int* col, const float* val, const float* x,
                             long long ldx, float* y, long long ldy, int n_rows, int k, const void* items,
                             long long n_items, const int* slot, const int* split, int n_split, long long n_pieces,
                             int item_nnz, float* ws, long long ws_floats, hipStream_t s) {
    Path p;
    if (n_rows < 0 || !spmm_path(k, (unsigned long long)x, ldx, (unsigned long long)y, ldy, &p)) return PCMX_ERR_ARG;
    if (item_nnz < 64 || item_nnz > kItemNnzMax || item_nnz % 64) return PCMX_ERR_ARG;
    const long long ldw = ((long long)k + 3) & ~3LL;
    if (n_split < 0 || n_pieces < 0 || n_pieces > 0x7fffffffLL || ws_floats < n_pieces * ldw) return PCMX_ERR_ARG;
    if (n_pieces > 0 && (ws == nullptr || (unsigned long long)ws % 16)) return PCMX_ERR_ARG;
    if (n_rows == 0 || k == 0) return 0;
    const long long blocks = (n_items + kWavesPerBlock - 1) / kWavesPerBlock;
    if (n_items <= 0 || blocks > 0x7fffffffLL || k / 256 > 65535) return PCMX_ERR_ARG;
    const unsigned bx = (unsigned)blocks;
#define PCMX_SPMM_ARGS row_ptr, col, val, x, ldx, y, ldy, ws, ldw
    if (k <= kNarrowMax) {
        const Item* its = reinterpret_cast<const Item*>(items);
        switch (p.cls) {
            case 4: spmm_narrow_kernel<4><<<bx, kWavesPerBlock * kWave, 0, s>>>(PCMX_SPMM_ARGS, its, n_items, slot, k); break;
            case 8: spmm_narrow_kernel<8><<<bx, kWavesPerBlock * kWave, 0, s>>>(PCMX_SPMM_ARGS, its, n_items, slot, k); break;
            case 16: spmm_narrow_kernel<16><<<bx, kWavesPerBlock * kWave, 0, s>>>(PCMX_SPMM_ARGS, its, n_items, slot, k); break;
            default: spmm_narrow_kernel<32><<<bx, kWavesPerBlock * kWave, 0, s>>>(PCMX_SPMM_ARGS, its, n_items, slot, k); break;
        }
    } else {
        // the full 256-column tiles on grid.y, then the partial last tile (or the whole of a k < 256) in its own class
        for (int part = 0; part < 2; ++part) {
            const int full = k / 256;
            const int cls = part == 0 ? (full ? 256 : 0) : (full ? p.tail : p.cls);
            if (cls == 0) continue;
            const dim3 grid(bx, part == 0 ? full : 1);
            const int base = part == 0 ? 0 : full * 256;
            const bool vec = p.vec & (part == 0 || !full ? 1 : 2);
            if (cls == 64)
                launch_wide<1, false>(grid, s, PCMX_SPMM_ARGS, items, n_items, slot, base, k);
            else if (cls == 128 && vec)
                launch_wide<2, true>(grid, s, PCMX_SPMM_ARGS, items, n_items, slot, base, k);
            else if (cls == 128)
                launch_wide<2, false>(grid, s, PCMX_SPMM_ARGS, items, n_items, slot, base, k);
            else if (vec)
                launch_wide<4, true>(grid, s, PCMX_SPMM_ARGS, items, n_items, slot, base, k);
            else
                launch_wide<4, false>(grid, s, PCMX_SPMM_ARGS, items, n_items, slot, base, k);
        }
    }
#undef PCMX_SPMM_ARGS
    PCMX_HIP_RET(hipGetLastError());
    if (n_split > 0) {
        spmm_fixup_kernel<<<(unsigned)n_split, 256, 0, s>>>(ws, ldw, split, y, ldy, k);
        PCMX_HIP_RET(hipGetLastError());
    }
    return 0;
}
