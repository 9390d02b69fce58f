/*
 * pcmx_hip.h — C ABI of libpcmx_hip.so: every MI355X (gfx950) kernel of the framework.
 *
 * Conventions
 *  - All pointers are DEVICE pointers unless the name says host. Every launcher is asynchronous on the
 *    given stream, allocates nothing and never synchronises, so a caller may capture it into a hipGraph.
 *    Workspaces are caller-provided; pcmx_*_workspace_bytes() says how much.
 *  - Return value: 0 on success, a hipError_t (> 0), or one of the PCMX_ERR_* codes below (< 0).
 *  - No launcher keeps process-global tuning state: every knob is a per-call argument.
 *  - Element counts are 64-bit: 1e9-element arrays (4 GB) are first-class on a 288 GB MI355X.
 *
 * Reference parity (file:line in anonyomous4/parallel-c-programs):
 *  vmul            6-opencl-region-growing/multiply_opencl.cl:1-4
 *  sgemm           1-introduction/matrix.c:63-81 (matrix_multiply) — fp32 MFMA on gfx950
 *  histeq          4-histogram-equalization-openmp-pthreads/histogram_serial.c:11-42
 *  region2d        2-mpi-region-growing/region.c:493-533 (flood fill, tile + 1-px halo)
 *  region3d_*      5-cuda-region-growing/raycast.cu:534-699 (naive + shared-memory kernels)
 *  raycast_*       5-cuda-region-growing/raycast.cu:321-433 (global-memory + texture kernels)
 *  volume_gen      5-cuda-region-growing/raycast.cu:114-158
 *  spmv_*          3-serial-optimization/spmv.c:170-329
 */
#ifndef PCMX_HIP_H
#define PCMX_HIP_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#include "pcmx_errors.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- error codes: pcmx_errors.h */

/* ---------------------------------------------------------------- runtime / device info */
int pcmx_device_count(void);
/* Prints count, name, gcnArchName, CUs, LDS/CU, L2, HBM size, clock (replaces print_properties /
 * printDeviceInfo, ref raycast.cu:99-110, clutil.c:63-122). */
void pcmx_print_device_info(int device);
const char* pcmx_error_string(int err);
/* registers the MFMA SGEMM as matrix_multiply()'s backend (host matrices, copies in/out). */
void pcmx_register_gemm_backend(long long min_flops);
int pcmx_sgemm_host_arrays(const float* a, const float* b, float* c, int m, int n, int k);

/* ---------------------------------------------------------------- element-wise (HBM-bound) */
int pcmx_vmul_f32(const float* a, const float* b, float* r, long long n, hipStream_t s);
int pcmx_vadd_f32(const float* a, const float* b, float* r, long long n, hipStream_t s);
int pcmx_axpy_f32(float alpha, const float* x, float* y, long long n, hipStream_t s);
int pcmx_copy_f32(const float* a, float* r, long long n, hipStream_t s);
// dst[i] = src[idx[i]] (32-bit indices; an index outside [0, n_src) reads 0); idx, dst 16-B aligned
int pcmx_gather_f32(const float* src, long long n_src, const int* idx, float* dst, long long n, hipStream_t s);
int pcmx_fill_f32(float* x, float v, long long n, hipStream_t s);
/* x[i] = uniform[lo,hi) from a counter-based hash of (seed, i): on-device synthetic data */
int pcmx_rand_uniform_f32(float* x, long long n, unsigned long long seed, float lo, float hi, hipStream_t s);

/* ---------------------------------------------------------------- reductions */
enum { PCMX_OP_SUM = 0, PCMX_OP_MIN = 1, PCMX_OP_MAX = 2 };
/* number of first-pass partials the reduce launchers use (workspace = that many elements * 8 B) */
long long pcmx_reduce_workspace_bytes(long long n);
/* out[0] = op(x[0..n)) ; two passes, deterministic (fixed grid, fixed combine order) */
int pcmx_reduce_f32(const float* x, long long n, int op, float* out, void* workspace, hipStream_t s);
int pcmx_reduce_i32(const int32_t* x, long long n, int op, int32_t* out, void* workspace, hipStream_t s);
/* out[0] = sum a*b */
int pcmx_dot_f32(const float* a, const float* b, long long n, float* out, void* workspace, hipStream_t s);
/* The same launches with the first pass's grid capped at max_blocks instead of 16384 (csrc/kernels/reduce.hip): the
 * blocks then grid-stride, so a cap of 3 or 7 takes the second and third trip of that loop at a few hundred thousand
 * elements (the production grid needs more than 2^26). The entries above are these with 16384. max_blocks outside
 * 1..16384, n < 0, an unknown op, a NULL or misaligned workspace or a misaligned x / a / b: PCMX_ERR_ARG, nothing
 * launched, out not written. The workspace is pcmx_reduce_workspace_bytes(n) whatever the cap.
 * A float sum starts from +0.0 (a sum of -0.0 alone is +0.0) and hands on NaN and inf; float min / max skip NaNs (all
 * NaN, or n == 0: the identity, +inf / -inf); int32 sums wrap mod 2^32; n == 0 gives the identity (0, INT32_MAX,
 * INT32_MIN). */
int pcmx_reduce_f32_grid(const float* x, long long n, int op, float* out, void* workspace, int max_blocks, hipStream_t s);
int pcmx_reduce_i32_grid(const int32_t* x, long long n, int op, int32_t* out, void* workspace, int max_blocks, hipStream_t s);
int pcmx_dot_f32_grid(const float* a, const float* b, long long n, float* out, void* workspace, int max_blocks, hipStream_t s);

/* ---------------------------------------------------------------- prefix scan */
long long pcmx_scan_workspace_bytes(long long n);
/* out[i] = init + sum_{j<=i} x[j] (inclusive) or init + sum_{j<i} x[j] (exclusive), single pass with
 * decoupled look-back; init is read from device memory (init_dev may be NULL => 0) so a multi-GPU
 * offset can be fed without a host round trip. In-place (out == x) is allowed.
 * A look-back that exceeds its bounded spin (a stalled predecessor) leaves an INVALID result: it is recorded in
 * the workspace (pcmx_scan_check) and OR-ed into *err_flag when err_flag != NULL (device or host-mapped word,
 * sticky: the caller clears it). */
int pcmx_scan_f32(const float* x, float* out, long long n, int exclusive, const float* init_dev, void* workspace,
                  unsigned* err_flag, hipStream_t s);
/* same with an explicit tile shape: rows = f32x4 rows per lane, 16 (8 waves, the default) or 8 (16 waves) */
int pcmx_scan_f32_rows(const float* x, float* out, long long n, int exclusive, const float* init_dev, void* workspace,
                       unsigned* err_flag, int rows, hipStream_t s);
/* schedule A/B entry (csrc/kernels/scan.hip): 0 persistent R16xW8, 1 persistent R8xW16, 2 parked-tile R16xW8,
 * 3 parked-tile R8xW16, 4 parked-tile R16xW8 with early polls (pcmx_scan_f32); any other variant: PCMX_ERR_ARG */
int pcmx_scan_f32_variant(const float* x, float* out, long long n, int exclusive, const float* init_dev,
                          void* workspace, unsigned* err_flag, int variant, hipStream_t s);
/* synchronises s; PCMX_ERR_TIMEOUT if the last scan on this workspace gave up a look-back, else 0 */
int pcmx_scan_check(const void* workspace, hipStream_t s);

/* ---------------------------------------------------------------- stream compaction (select / nonzero) */
/* Keeps the selected elements of a length-n stream in input order and stores how many were kept to *count_dev
 * (int64, device memory) without a host sync: one pass on the scan's decoupled look-back, carrying the exact u32
 * kept count per tile (csrc/kernels/select.hip). out needs room for n elements (count is not known on the host);
 * elements of out at or past the count are not written. x and out 16-B aligned, mask 4-B aligned, n < 2^31 (else
 * PCMX_ERR_ARG); n <= 0 stores count 0 and returns 0. out must not overlap x or mask. A look-back that gives up is
 * reported as for pcmx_scan_f32: in the workspace (pcmx_scan_check reads a select workspace too) and in *err_flag. */
enum { PCMX_CMP_GT = 0, PCMX_CMP_GE = 1, PCMX_CMP_LT = 2, PCMX_CMP_LE = 3, PCMX_CMP_EQ = 4, PCMX_CMP_NE = 5 };
long long pcmx_select_workspace_bytes(long long n);
/* out[j] = x[i] for the j-th i with mask[i] != 0; x is any 4-byte payload moved as bits (f32 NaN payloads survive) */
int pcmx_select_b32(const void* x, const unsigned char* mask, void* out, long long n, long long* count_dev,
                    void* workspace, unsigned* err_flag, hipStream_t s);
/* out_idx[j] = i (int32) for the j-th i with mask[i] != 0: a flattened nonzero */
int pcmx_select_index(const unsigned char* mask, int* out_idx, long long n, long long* count_dev, void* workspace,
                      unsigned* err_flag, hipStream_t s);
/* keeps x[i] OP threshold (PCMX_CMP_*, IEEE: NaN is kept only by NE); writes the kept f32 values, or with
 * want_index != 0 their int32 indices; no mask is materialised */
int pcmx_select_if_f32(const float* x, int op, float threshold, void* out_or_idx, int want_index, long long n,
                       long long* count_dev, void* workspace, unsigned* err_flag, hipStream_t s);

/* ---------------------------------------------------------------- radix sort (keys, pairs, argsort) */
/* Stable LSD radix sort of n 32-bit keys, ascending (or descending != 0), by bits [begin_bit, end_bit) of the
 * TRANSFORMED key; ceil((end_bit - begin_bit) / 8) one-sweep passes on the scan's look-back plus one histogram kernel
 * (csrc/kernels/sort.hip). Bits outside the range are ignored; keys equal in the compared bits keep input order.
 * Transformed key: U32 identity; I32 k ^ 0x80000000; F32 the order of torch.sort: ~b for a set sign bit, else
 * b | 0x80000000, with -0.0 taking +0.0's key and every NaN (either sign, any payload) the key 0xffffffff, so NaNs
 * sort last ascending, first descending, and signed zeros / NaNs tie. The transform is inverted on the last store:
 * sorted F32 keys come out with +0.0 for both zeros and 0x7fffffff for every NaN (payloads are not preserved; gather
 * with the indices to get the original bits). Values are 4 bytes moved as bits.
 *   PCMX_SORT_KEYS   keys_out = sorted keys; vals_in / vals_out unused
 *   PCMX_SORT_PAIRS  keys_out, vals_out = keys and their values
 *   PCMX_SORT_INDEX  vals_out[j] = int32 input index of the j-th key (no iota array is read); keys_out may be NULL
 *                    (the keys then ping-pong inside the workspace only)
 * keys_in is never written and must not overlap an output; all pointers 16-B aligned; 0 < n < 2^30 (indices and the
 * 30-bit granule counts; else PCMX_ERR_ARG); n <= 0 returns 0 and touches nothing. The workspace (16-B aligned,
 * pcmx_sort_workspace_bytes) holds the flags, histograms and ping-pong buffers; one call in flight per workspace. Its
 * header has the scan's layout: a look-back that gives up is reported as for pcmx_scan_f32 (pcmx_scan_check,
 * *err_flag), and its result is invalid but every store stays inside the output buffers. */
enum { PCMX_KEY_U32 = 0, PCMX_KEY_I32 = 1, PCMX_KEY_F32 = 2 };
enum { PCMX_SORT_KEYS = 0, PCMX_SORT_PAIRS = 1, PCMX_SORT_INDEX = 2 };
long long pcmx_sort_workspace_bytes(long long n, int mode);
int pcmx_radix_sort(const void* keys_in, void* keys_out, const void* vals_in, void* vals_out, long long n,
                    int key_type, int mode, int descending, int begin_bit, int end_bit,
                    void* workspace, unsigned* err_flag, hipStream_t s);

/* ---------------------------------------------------------------- top-k / k-th value (radix select) */
/* The k best of n 32-bit keys, largest != 0: the largest, else the smallest, in the order of pcmx_radix_sort's
 * transformed keys (F32: -0.0 == +0.0, every NaN one key above +inf). The result is DEFINED as the first k entries of
 * the stable PCMX_SORT_INDEX sort with descending = largest: among keys that tie with the k-th key the lowest indices
 * are taken, ties come out in ascending index order, F32 values come out canonical (+0.0, NaN bits 0x7fffffff).
 * out_vals[j] / out_idx[j] (int32 flat index), j < k. sorted == 0: the same k elements in ascending index order (no
 * survivor sort runs). The keys are never written and must not overlap an output. Four histogram passes find the k-th
 * key (most significant digit first, the digit chosen on the device; no inter-block waiting), one pass on the scan's
 * look-back gathers the k survivors in index order, pcmx_radix_sort orders them (csrc/kernels/topk.hip). No host sync.
 * keys, outputs and workspace 16-B aligned, 0 < n < 2^30, 0 <= k <= n, a valid key type (else PCMX_ERR_ARG, nothing
 * launched); n == 0 or k == 0 returns 0 without a launch. The workspace header has the scan's layout: a look-back that
 * gives up is reported as for pcmx_scan_f32 (pcmx_scan_check, *err_flag); its result is invalid but every store stays
 * inside the k-element outputs. One call in flight per workspace. */
long long pcmx_topk_workspace_bytes(long long n, long long k, int sorted);
int pcmx_topk_b32(const void* keys, long long n, long long k, int key_type, int largest, int sorted, void* out_vals,
                  void* out_idx, void* workspace, unsigned* err_flag, hipStream_t s);
/* out_dev[0] = the k-th key (1 <= k <= n, 1-based; the k-th largest when largest != 0), canonical as above: the
 * histogram passes alone. Workspace: pcmx_topk_workspace_bytes(n, k, 0). err_flag is unused (no look-back runs). */
int pcmx_kth_key_b32(const void* keys, long long n, long long k, int key_type, int largest, void* out_dev,
                     void* workspace, unsigned* err_flag, hipStream_t s);

/* ---------------------------------------------------------------- row-wise sort / top-k / k-th value */
/* The same three operations on every row of a contiguous [rows, cols] matrix of 32-bit keys, one wave or one block per
 * row (csrc/kernels/rowsort.hip): row r's result equals pcmx_radix_sort / pcmx_topk_b32 / pcmx_kth_key_b32 applied to
 * keys + r * cols, bit for bit (same transformed keys, stable, F32 keys canonical on output, values moved as bits),
 * except that PCMX_SORT_INDEX and the top-k indices are int32 positions WITHIN the row. No workspace, no error word, no
 * communication between blocks, no host sync; the inputs are never written. rows * cols < 2^30.
 *
 * pcmx_row_sort_b32: cols <= PCMX_ROWSORT_MAX_COLS. Only the first `keep` (0 <= keep <= cols) entries of each sorted
 * row are stored: keys_out / vals_out are [rows, keep], so keep = k is the row-wise top-k of a short row. mode is
 * PCMX_SORT_KEYS / PAIRS / INDEX as for pcmx_radix_sort (keys_out may be NULL in INDEX mode), optionally OR-ed with
 * PCMX_ROWSORT_WAVE (one wave per row, cols <= PCMX_ROWSORT_WAVE_MAX_COLS) or PCMX_ROWSORT_BLOCK (one 512-thread block
 * per row) to force a kernel; with neither, rows of at most PCMX_ROWSORT_WAVE_COLS keys take the wave kernel. Rows
 * start at byte 4 * r * cols, so only the base pointers need alignment: every access is a 4-byte access.
 * pcmx_row_topk_b32: out_vals / out_idx are [rows, k], the k survivors of each row in ascending position (what
 * pcmx_topk_b32 gives for sorted == 0); any cols. pcmx_row_sort_b32 in PAIRS mode on them gives the sorted form.
 * pcmx_row_kth_key_b32: out[r] = the k-th key of row r (1-based, the k-th largest when largest != 0).
 * All three: a bad key type or mode, sizes out of range (k or keep > cols, rows * cols >= 2^30, cols over the limit), a
 * NULL or not 16-B aligned base pointer, or an output that overlaps an input or another output: PCMX_ERR_ARG, nothing
 * launched. rows == 0, cols == 0 or k (keep) == 0: returns 0, nothing launched. */
#define PCMX_ROWSORT_MAX_COLS 16384
#define PCMX_ROWSORT_WAVE_MAX_COLS 1024
#define PCMX_ROWSORT_WAVE_COLS 512
enum { PCMX_ROWSORT_WAVE = 0x100, PCMX_ROWSORT_BLOCK = 0x200 };
int pcmx_row_sort_b32(const void* keys_in, void* keys_out, const void* vals_in, void* vals_out, long long rows,
                      long long cols, long long keep, int key_type, int mode, int descending, int begin_bit, int end_bit,
                      hipStream_t s);
int pcmx_row_topk_b32(const void* keys, long long rows, long long cols, long long k, int key_type, int largest,
                      void* out_vals, void* out_idx, hipStream_t s);
int pcmx_row_kth_key_b32(const void* keys, long long rows, long long cols, long long k, int key_type, int largest,
                         void* out, hipStream_t s);

/* ---------------------------------------------------------------- reduce / scan along a dimension */
/* op (PCMX_OP_SUM / MIN / MAX) along the middle extent of a contiguous [outer, n, inner] tensor, read where it lies
 * (csrc/kernels/axis.hip): reduce writes out [outer, inner], scan writes out [outer, n, inner] (exclusive != 0: the
 * first element along n gets the identity, +0.0 / 0, +inf / INT32_MAX, -inf / INT32_MIN). int32 sums wrap mod 2^32 and
 * int32 results are exact; float32 min / max are exact and hand on a NaN (a scan: to the end of that row only); a
 * float32 sum uses the fixed association order written down in axis.hip's header, which depends on n, inner, the route
 * and the chunk only: the same row gives the same bits wherever it stands and on every call. Rows never mix. No block
 * waits for another, nothing can time out, there is no err_flag and no host sync; the split routes meet through the
 * workspace between their two or three launches on the stream.
 * route: 0 picks by the PCMX_AXIS_* borders below; PCMX_AXIS_GROUP (inner == 1, n <= PCMX_AXIS_GROUP_MAX_N: G lanes
 * per row), PCMX_AXIS_BLOCK (inner == 1, n <= PCMX_AXIS_BLOCK_MAX_N: one block per row), PCMX_AXIS_SPLIT (inner == 1:
 * chunks of a row over blocks), PCMX_AXIS_COLUMN (inner > 1: a thread walks down 4 adjacent columns) and
 * PCMX_AXIS_COLUMN_SPLIT (inner > 1: chunks of n over threads) force a route. chunk: 0 for the default, else the
 * elements along n per chunk of a split route: a multiple of 1024 for SPLIT, at least PCMX_AXIS_COLUMN_MIN_CHUNK for
 * COLUMN_SPLIT; non-zero with any other route is refused.
 * x, out and the workspace 16-B aligned (rows start wherever n and inner put them: only the bases need alignment).
 * The input is never written, except that a scan's out may be x itself (in place). The workspace
 * (pcmx_axis_workspace_bytes, one call in flight per workspace) may be NULL for the routes that are not split.
 * PCMX_ERR_ARG with nothing launched: a NULL or misaligned x or out (a NULL workspace on a split route), an out that
 * partly overlaps x, an unknown op or route, a route that cannot take the shape, a bad chunk, a negative extent, or
 * outer * n * inner >= 2^31. Any zero extent returns 0 and launches nothing, except a SUM reduce with n == 0 and
 * outer * inner > 0, which fills out with zeros. */
#define PCMX_AXIS_GROUP_MAX_N 4096        /* the group kernel's limit when forced: 16 quads per lane */
#define PCMX_AXIS_GROUP_N 2048            /* default, reduce: rows up to here take group, longer ones block */
#define PCMX_AXIS_GROUP_SCAN_N 512        /* default, scan: the same border */
#define PCMX_AXIS_BLOCK_MAX_N (1 << 20)   /* rows longer than this always take split */
#define PCMX_AXIS_SPLIT_ROWS 512          /* default: with fewer rows than this ... */
#define PCMX_AXIS_SPLIT_MIN_N (1 << 17)   /* ... rows from this length take split */
#define PCMX_AXIS_SPLIT_CHUNK 32768       /* default chunk of split */
#define PCMX_AXIS_COLUMN_MIN_UNITS 65536  /* default, scan: column when outer * ceil(inner / 4) threads reach this ... */
#define PCMX_AXIS_COLUMN_MIN_BLOCKS 1024  /* default, reduce: column when outer * (64-quad tiles of inner) reach this ... */
#define PCMX_AXIS_COLUMN_SPLIT_MIN_N 64   /* ... or n is below this; column_split otherwise */
#define PCMX_AXIS_COLUMN_REDUCE_BLOCKS 1024 /* the blocks the default chunk of a column_split reduce aims for */
#define PCMX_AXIS_COLUMN_MIN_CHUNK 16     /* smallest chunk of column_split */
enum { PCMX_AXIS_GROUP = 1, PCMX_AXIS_BLOCK = 2, PCMX_AXIS_SPLIT = 3, PCMX_AXIS_COLUMN = 4, PCMX_AXIS_COLUMN_SPLIT = 5 };
long long pcmx_axis_workspace_bytes(long long outer, long long n, long long inner);
int pcmx_axis_reduce_f32(const float* x, float* out, long long outer, long long n, long long inner, int op, int route,
                         long long chunk, void* workspace, hipStream_t s);
int pcmx_axis_reduce_i32(const int32_t* x, int32_t* out, long long outer, long long n, long long inner, int op, int route,
                         long long chunk, void* workspace, hipStream_t s);
int pcmx_axis_scan_f32(const float* x, float* out, long long outer, long long n, long long inner, int op, int exclusive,
                       int route, long long chunk, void* workspace, hipStream_t s);
int pcmx_axis_scan_i32(const int32_t* x, int32_t* out, long long outer, long long n, long long inner, int op, int exclusive,
                       int route, long long chunk, void* workspace, hipStream_t s);

/* ---------------------------------------------------------------- run-length encode / reduce by key */
/* Collapses runs of equal neighbouring 32-bit keys of a length-n stream and reduces a value stream per run, in one pass
 * on the scan's decoupled look-back plus a small kernel that joins the runs crossing tile borders
 * (csrc/kernels/segreduce.hip). Keys are compared as BIT PATTERNS: -0.0 and +0.0 are different keys, two NaNs with
 * the same bits are the same key (torch.unique_consecutive on the int32 view, not on the float view; the sorted float
 * keys of pcmx_radix_sort are canonical, so they collapse as values). A run is a maximal block of equal neighbours;
 * element 0 starts one. The number of runs goes to *num_runs_dev (int64, device memory) without a host sync; every
 * per-run array needs room for n entries and only [0, num_runs) is written. Run keys keep their exact bits; counts
 * and start offsets are int32. op is PCMX_OP_SUM / MIN / MAX: int32 sums wrap mod 2^32 and int32 results are exact;
 * float32 results depend only on the input, never on timing (fixed association order, no float atomics); float
 * min / max hand on a NaN value (which NaN's payload is unspecified). keys, vals and every output 16-B aligned,
 * 0 < n < 2^31 and a valid op (else PCMX_ERR_ARG, nothing launched); n <= 0 stores 0 runs and launches nothing else.
 * No output may overlap an input. The workspace header has the scan's layout: a look-back that gives up is reported
 * as for pcmx_scan_f32 (pcmx_scan_check, *err_flag); its result is invalid but every store stays inside the outputs. */
long long pcmx_segreduce_workspace_bytes(long long n);
/* run_keys[j], counts[j] (and starts[j], the offset of the run's first element, when starts != NULL) of the j-th run */
int pcmx_run_length_encode_b32(const void* keys, long long n, void* run_keys, int* counts, int* starts,
                               long long* num_runs_dev, void* workspace, unsigned* err_flag, hipStream_t s);
/* agg[j] = op over the values of the j-th run; run_keys may be NULL (the keys of the runs are then not written) */
int pcmx_reduce_by_key_f32(const void* keys, const float* vals, long long n, int op, void* run_keys, float* agg,
                           long long* num_runs_dev, void* workspace, unsigned* err_flag, hipStream_t s);
int pcmx_reduce_by_key_i32(const void* keys, const int32_t* vals, long long n, int op, void* run_keys, int32_t* agg,
                           long long* num_runs_dev, void* workspace, unsigned* err_flag, hipStream_t s);

/* ---------------------------------------------------------------- scan by key (segmented prefix scan) */
/* The running aggregate inside every run of a length-n stream: out[i] = op over vals[s .. i] (inclusive) or
 * vals[s .. i-1] (exclusive != 0), s the first element of i's run (csrc/kernels/scanbykey.hip). The runs come from
 * keys_or_heads: with PCMX_HEADS_FROM_KEYS it holds n 32-bit keys and a run is a maximal block of equal neighbours,
 * compared as BIT PATTERNS exactly as for pcmx_reduce_by_key_* (-0.0 != +0.0, NaNs equal only with equal bits); with
 * PCMX_HEADS_FROM_FLAGS it holds n bytes and a non-zero byte starts a run. Element 0 starts a run in either mode,
 * whatever its flag says. op is PCMX_OP_SUM / MIN / MAX. In exclusive mode the first element of every run gets the
 * identity: +0.0 / 0 for SUM, +inf / INT32_MAX for MIN, -inf / INT32_MIN for MAX. int32 sums wrap mod 2^32 and int32
 * results are exact; float32 min / max are exact and hand on a NaN value to the end of its run only; a float32 sum
 * uses a fixed association order (not input order), so the same input gives the same bits on every call, and a NaN
 * or inf in one run never reaches another run. Three launches on the stream (tile scan with every output written,
 * one-block scan of the tile summaries, carry added to the lead of every tile that continues a run); no block waits
 * for another, so nothing can time out and there is no err_flag. out may be vals itself (in place); it must not
 * overlap keys_or_heads. keys, vals, out and the workspace (pcmx_scanbykey_workspace_bytes, one call in flight per
 * workspace) 16-B aligned, the flag bytes 4-B aligned, 0 < n < 2^31, a valid op and head mode, no NULL pointer (else
 * PCMX_ERR_ARG, nothing launched); n <= 0 returns 0 and touches nothing. */
enum { PCMX_HEADS_FROM_KEYS = 0, PCMX_HEADS_FROM_FLAGS = 1 };
long long pcmx_scanbykey_workspace_bytes(long long n);
int pcmx_scan_by_key_f32(const void* keys_or_heads, int head_mode, const float* vals, float* out, long long n, int op,
                         int exclusive, void* workspace, hipStream_t s);
int pcmx_scan_by_key_i32(const void* keys_or_heads, int head_mode, const int32_t* vals, int32_t* out, long long n, int op,
                         int exclusive, void* workspace, hipStream_t s);
/* out[i] = int32 index of element i inside its run (0, 1, 2, ...): the exclusive sum-scan by key of the constant 1;
 * no value stream is read */
int pcmx_run_positions_b32(const void* keys, int32_t* out, long long n, void* workspace, hipStream_t s);

/* ---------------------------------------------------------------- histograms (bincount / even bins / explicit edges) */
/* Counts of a length-n sample stream in out[0 .. num_bins) (int32; csrc/kernels/bincount.hip). A sample that falls in
 * no bin is ignored: never an error, never an access outside out. accumulate == 0 zeroes out first (on the stream),
 * accumulate != 0 adds to what it holds. The samples are never written. One persistent kernel, no block waits for
 * another, the only traffic between blocks is integer atomic adds: counts are exact and the same on every call; there
 * is no workspace and no err_flag. Up to 24576 bins are counted in LDS per block and merged at the end; up to 64 * 24576
 * bins (bincount_i32 and hist_even) the blocks share the bins out in ranges and each reads its input slice for its
 * range; more bins are added straight into out.
 *  bincount: the bin of a sample is its value; values < 0 or >= num_bins are ignored. weights (may be NULL) are n
 *   int32 values: out[b] += weights[i] instead of 1, sums wrap mod 2^32.
 *  hist_even: bin = min((int)((v - lo) * scale), num_bins - 1) in float32 with each step rounded separately, counted
 *   only when lo <= v <= hi (compared in float before any conversion: NaN and +-inf are ignored). The caller passes
 *   scale = (float)num_bins / (hi - lo), computed once in float32.
 *  hist_range: edges holds num_bins + 1 ascending float32 values in device memory, 1 <= num_bins <= 8192; bin i holds
 *   edges[i] <= v < edges[i+1], the last bin also v == edges[num_bins]; NaN and values outside are ignored. Edges that
 *   do not ascend give unspecified counts, but every index is clamped: nothing outside out or edges is touched.
 * Alignment: x to its element size (any element-aligned start works: the kernel peels the bytes before the first and
 * after the last whole 16-byte vector), out and edges 4-B; with weights, x and weights both 16-B. 1 <= num_bins < 2^31,
 * n < 2^31, lo < hi and a finite scale >= 0 (else PCMX_ERR_ARG, nothing launched); n <= 0 only zeroes out (or leaves
 * it, when accumulating). */
int pcmx_bincount_i32(const int32_t* x, const int32_t* weights, long long n, long long num_bins, int32_t* out,
                      int accumulate, hipStream_t s);
int pcmx_bincount_u8(const unsigned char* x, const int32_t* weights, long long n, long long num_bins, int32_t* out,
                     int accumulate, hipStream_t s);
int pcmx_hist_even_f32(const float* x, long long n, long long num_bins, float lo, float hi, float scale, int32_t* out,
                       int accumulate, hipStream_t s);
int pcmx_hist_range_f32(const float* x, long long n, const float* edges, long long num_bins, int32_t* out,
                        int accumulate, hipStream_t s);

/* ---------------------------------------------------------------- merge of sorted sequences / sorted search */
/* Merges two SORTED sequences of 32-bit keys (na and nb keys, either may be empty) into one of na + nb keys, and
 * searches sorted keys, on the merge-path diagonal partition (csrc/kernels/merge.hip). Keys are compared only through
 * pcmx_radix_sort's TRANSFORMED key (U32 identity; I32 k ^ 0x80000000; F32 -0.0 == +0.0 and every NaN one key above
 * +inf), reversed for descending != 0, and are moved as their raw 32 bits: the transform is never inverted, so NaN
 * payloads and the sign of zero come out as they went in. "Sorted" means non-decreasing in that order. It is a
 * precondition and is not checked: with unsorted input the result is unspecified, but every load and store stays
 * inside the given buffers. A tie goes to a: an element of a precedes an equal element of b, so the result is the
 * stable sort of the concatenation a ++ b. Values are 4 bytes moved as bits.
 *   PCMX_MERGE_KEYS   keys_out = merged keys; vals_a / vals_b / vals_or_idx_out unused
 *   PCMX_MERGE_PAIRS  keys_out, vals_or_idx_out = keys and their values
 *   PCMX_MERGE_INDEX  vals_or_idx_out[j] = int32 index into the concatenation of the j-th key (i for a[i], na + i for
 *                     b[i]); keys_out may be NULL (no keys are written)
 * Two launches: a partition kernel (one thread per output tile writes where the tile starts in a: ntiles + 1 int32
 * values in the workspace) and a merge kernel (one block per tile, through LDS). No block waits for another, there are
 * no atomics and no err_flag; the outputs are the same on every call. The inputs are never written and need only 4-B
 * alignment; outputs and the workspace (pcmx_merge_workspace_bytes, one call in flight per workspace) are 16-B
 * aligned; no output may overlap an input; na + nb < 2^31. A bad key type, mode, alignment or size, or a missing
 * pointer, returns PCMX_ERR_ARG and launches nothing; na + nb == 0 returns 0 and touches nothing. */
enum { PCMX_MERGE_KEYS = 0, PCMX_MERGE_PAIRS = 1, PCMX_MERGE_INDEX = 2 };
long long pcmx_merge_workspace_bytes(long long na, long long nb);
int pcmx_merge_b32(const void* keys_a, const void* vals_a, long long na, const void* keys_b, const void* vals_b,
                   long long nb, void* keys_out, void* vals_or_idx_out, int key_type, int mode, int descending,
                   void* workspace, hipStream_t s);
/* out[i] (int32, i < m) = the number of the n sorted keys that precede needles[i] (right == 0: a lower bound), or
 * that precede or equal it (right != 0: an upper bound), in the order above: torch.searchsorted, except that a NaN
 * needle ties with the NaNs at the end of the keys. Needles may be in any order: a block stages evenly spaced keys in
 * LDS (all of them up to 8192), a lane bounds its needle among those and finishes in the one interval left in global
 * memory, with the same predicate at both levels. needles_sorted != 0 is the caller's promise that the needles are
 * sorted in the same order: with n + m < 2^31 and 8 m >= n (fewer needles are cheaper to search one by one than the
 * keys are to read) the search then runs as a merge of needles and keys that writes no keys (the partition and merge
 * kernels above; right != 0 gives ties to the keys), bandwidth-bound and load-balanced, with results bit-identical to
 * the general route when the promise holds and unspecified (but in bounds) when it does not.
 * n == 0 writes zeros. sorted_keys and needles 4-B aligned, out and the workspace
 * (pcmx_searchsorted_workspace_bytes, one call in flight per workspace) 16-B aligned, n and m < 2^31, out must not
 * overlap an input (else PCMX_ERR_ARG, nothing launched); m == 0 returns 0 and touches nothing. */
long long pcmx_searchsorted_workspace_bytes(long long n, long long m, int needles_sorted);
int pcmx_searchsorted_b32(const void* sorted_keys, long long n, const void* needles, long long m, int32_t* out,
                          int key_type, int right, int descending, int needles_sorted, void* workspace, hipStream_t s);

/* ---------------------------------------------------------------- set operations on sorted sequences */
/* Intersection, union, difference and symmetric difference of two SORTED sequences of 32-bit keys, with the multiset
 * rule of std::set_* (csrc/kernels/setops.hip). Order, key transform, the sortedness precondition (not checked:
 * unspecified result, but every load and store inside the given buffers) and the modes are pcmx_merge_b32's. Keys are
 * equal when their transformed keys are. For a key that occurs m times in a and n times in b, the i-th occurrence in
 * a is paired with the i-th in b, i < min(m, n):
 *   PCMX_SET_INTERSECTION  keeps the paired elements of a                           capacity min(na, nb)
 *   PCMX_SET_UNION         keeps all of a and the unpaired elements of b            capacity na + nb
 *   PCMX_SET_DIFFERENCE    keeps the unpaired elements of a                         capacity na
 *   PCMX_SET_SYMDIFF       keeps the unpaired elements of both                      capacity na + nb
 * The output is the kept elements in the order of the merge (a tie goes to a): pcmx_merge_b32's result filtered by
 * a keep mask, keys moved as raw bits, values (PCMX_MERGE_PAIRS) and indices into the concatenation
 * (PCMX_MERGE_INDEX, keys_out may be NULL) travelling with their element. *count_out (int64 in device memory, 8-B
 * aligned) receives the number of kept elements; the outputs have room for the op's capacity and nothing at or past
 * the count is written. Two launches on the stream behind a hipMemsetAsync of the workspace's head: a partition
 * kernel (the tile borders and the run counts that cross them) and one block per tile that merges, decides, and
 * stores compacted at an exact position from the decoupled look-back of the scan (bounded spins; a look-back that
 * gives up sets the workspace's timeout word, which pcmx_scan_check reads, and ORs 1 into *err_flag, which may be
 * NULL). Inputs 4-B aligned and never written; outputs and the workspace (pcmx_set_op_workspace_bytes, one call in
 * flight per workspace) 16-B aligned; no output may overlap an input; na + nb < 2^31. A bad key type, op, mode,
 * alignment or size, a missing pointer or a workspace_bytes below pcmx_set_op_workspace_bytes returns PCMX_ERR_ARG
 * and launches nothing. A capacity of 0 writes *count_out = 0 and nothing else. */
enum { PCMX_SET_INTERSECTION = 0, PCMX_SET_UNION = 1, PCMX_SET_DIFFERENCE = 2, PCMX_SET_SYMDIFF = 3 };
long long pcmx_set_op_workspace_bytes(long long na, long long nb);
int pcmx_set_op_b32(const void* keys_a, const void* vals_a, long long na, const void* keys_b, const void* vals_b,
                    long long nb, void* keys_out, void* vals_or_idx_out, long long* count_out, int op, int mode,
                    int key_type, int descending, void* workspace, long long workspace_bytes, unsigned* err_flag,
                    hipStream_t s);

/* ---------------------------------------------------------------- reduction over ragged segments (offsets) */
/* out[j] = op over x[offsets[j], offsets[j+1]) for j < S: the segments of a CSR row_ptr, torch.segment_reduce with
 * offsets= (csrc/kernels/ragged.hip). offsets holds S + 1 int32 values in device memory with the PRECONDITION
 * 0 <= offsets[0] <= ... <= offsets[S] <= n; elements before offsets[0] and from offsets[S] on are not read. op is
 * PCMX_OP_SUM / MIN / MAX. An empty segment gives the identity: +0.0 / 0 for SUM, +inf / INT32_MAX for MIN, -inf /
 * INT32_MIN for MAX. int32 sums wrap mod 2^32 and int32 results are exact; float32 min / max are exact and hand on a
 * NaN inside its segment only; a float32 sum uses a fixed association order that may depend on where the segment lies
 * relative to the tiles and never on timing: the same input gives the same bits on every call, and a NaN or inf in one
 * segment never reaches another. The list of segment ends is merged with the element indices and every block takes
 * the same number of steps of that path, whatever the segment lengths are. Four launches on the stream (tile borders,
 * tiles, a one-block scan of the tile summaries, the carry into the first segment every tile closed); no block waits
 * for another, there are no float atomics and no err_flag. The precondition is not checked: offsets that break it
 * give an unspecified result, but every load and store stays inside x[0, n), offsets[0, S], out[0, S) and the
 * workspace. x and offsets 4-B aligned, out and the workspace (pcmx_segment_workspace_bytes, one call in flight per
 * workspace) 16-B aligned, out must not overlap an input, n >= 0, S >= 0, n + S < 2^31, a valid op, no NULL pointer
 * (x may be NULL when n == 0) (else PCMX_ERR_ARG, nothing launched); S == 0 returns 0 and touches nothing; n == 0
 * with S > 0 writes S identities. */
long long pcmx_segment_workspace_bytes(long long n, long long S);
int pcmx_segment_reduce_f32(const float* x, long long n, const int32_t* offsets, long long S, int op, float* out,
                            void* workspace, hipStream_t s);
int pcmx_segment_reduce_i32(const int32_t* x, long long n, const int32_t* offsets, long long S, int op, int32_t* out,
                            void* workspace, hipStream_t s);
/* The head flags of the same offsets for pcmx_scan_by_key_* with PCMX_HEADS_FROM_FLAGS: heads[0, n) is zeroed, then
 * heads[offsets[j]] = 1 for every j <= S with 0 <= offsets[j] < n (the store is bounded by n itself, so offsets that
 * break the precondition touch nothing outside heads). offsets 4-B aligned, n and S < 2^31, no NULL pointer (else
 * PCMX_ERR_ARG, nothing launched); n == 0 returns 0 and touches nothing. */
int pcmx_segment_heads(const int32_t* offsets, long long S, long long n, unsigned char* heads, hipStream_t s);

/* ---------------------------------------------------------------- sort inside ragged segments (offsets) */
/* Every segment [offsets[j], offsets[j+1]) of n 32-bit keys, j < S, sorted on its own: restricted to a segment the
 * outputs equal pcmx_radix_sort applied to that slice, bit for bit (same transformed keys, stable, F32 keys canonical
 * on output, values moved as bits), except that PCMX_SORT_INDEX gives FLAT int32 indices into keys_in (the position
 * within the segment plus offsets[j]). keys_out / vals_out hold n entries, laid out as keys_in. offsets as for
 * pcmx_segment_reduce_*: S + 1 int32 values in device memory with the PRECONDITION 0 <= offsets[0] <= ... <=
 * offsets[S] <= n, not checked: every offset is clamped to [0, n] where it is read and a negative length counts as 0,
 * so offsets that break it give an unspecified result but every load and store stays inside the buffers. Keys before
 * offsets[0] and from offsets[S] on belong to no segment: they are copied through with their bits unchanged
 * (PCMX_SORT_INDEX: their own position); the two offsets are read on the device.
 * A segment of at most PCMX_SEGSORT_MAX_LEN keys is sorted inside one CU by one wave or one 512-thread block
 * (csrc/kernels/segsort.hip: segments are listed by length class on the device, every class runs a fixed grid over its
 * list). A LONGER segment is not sorted here: its part of the outputs is NOT WRITTEN, and it is reported in the
 * summary, 4 uint32 at byte PCMX_SEGSORT_SUMMARY_OFFSET of the workspace, valid once the stream has run the call:
 * {segments longer than PCMX_SEGSORT_MAX_LEN, the keys in them, the longest length of any segment, 0}.
 * mode is PCMX_SORT_KEYS / PAIRS / INDEX as for pcmx_radix_sort (keys_out may be NULL in INDEX mode), optionally OR-ed
 * with PCMX_SEGSORT_GRID(m), 1 <= m <= 64: m blocks per compute unit in every class launch (the lab's knob).
 * No error word, no block waits for another, no host sync; the inputs are never written. The workspace
 * (pcmx_segment_sort_workspace_bytes, 256 + 4 S bytes rounded up; one call in flight per workspace) and the key / value
 * buffers 16-B aligned, offsets 4-B aligned. PCMX_ERR_ARG with nothing launched and nothing written: a NULL or
 * misaligned pointer, an output that overlaps an input, the offsets or another output, a workspace that overlaps any
 * of them, a bad key type, mode or bit range, n or S negative or above 2^30 - 1. n == 0 clears the summary and
 * launches nothing else; S == 0 copies everything through. */
#define PCMX_SEGSORT_MAX_LEN 16384
#define PCMX_SEGSORT_SUMMARY_OFFSET 128
#define PCMX_SEGSORT_GRID(m) ((m) << 8)
long long pcmx_segment_sort_workspace_bytes(long long n, long long S);
int pcmx_segment_sort_b32(const void* keys_in, void* keys_out, const void* vals_in, void* vals_out, long long n,
                          const int32_t* offsets, long long S, int key_type, int mode, int descending, int begin_bit,
                          int end_bit, void* workspace, hipStream_t s);

/* ---------------------------------------------------------------- argmin / argmax (flat, along a dimension, ragged) */
/* Where the extremum is, and its value (csrc/kernels/argreduce.hip). key_type is PCMX_KEY_F32 or PCMX_KEY_I32, op is
 * PCMX_OP_MIN or PCMX_OP_MAX. One rule for the three forms: a NaN beats every number under both ops (torch's rule for
 * argmax / argmin / max(dim) / min(dim), NOT the NaN-skipping rule of pcmx_reduce_*); otherwise the numerically largest
 * (smallest) element wins with -0.0 == +0.0; among equal winners and among NaNs the lowest position wins; the value
 * written is the input element at that position, bit for bit. Positions are int32. The result depends on the data
 * only, never on the route, the chunk, the grid or timing. value_out or index_out may be NULL (not both): that output
 * is not written. x and the workspace 16-B aligned (the segment form: x and offsets 4-B), the outputs 4-B aligned and
 * overlapping neither an input nor each other. PCMX_ERR_ARG with nothing launched: another key type or op
 * (PCMX_OP_SUM), a NULL or misaligned required pointer, a negative extent, 2^31 elements or more, a route or chunk
 * that does not fit the shape, max_blocks outside 1..16384.
 *
 * Flat: two launches, reduce.hip's shape (the first pass's grid capped at max_blocks, 16384 for the plain entry; the
 * blocks then grid-stride; one block folds the 8-byte block partials and reads the value). index_out[0] is the position
 * in x[0, n); n == 0 gives -1 and the identity (-inf / INT32_MIN for MAX, +inf / INT32_MAX for MIN). The workspace is
 * pcmx_arg_reduce_workspace_bytes(n) whatever the cap. */
long long pcmx_arg_reduce_workspace_bytes(long long n);
int pcmx_arg_reduce_b32(const void* x, long long n, int key_type, int op, void* value_out, int32_t* index_out, void* workspace,
                        hipStream_t s);
int pcmx_arg_reduce_b32_grid(const void* x, long long n, int key_type, int op, void* value_out, int32_t* index_out,
                             void* workspace, int max_blocks, hipStream_t s);
/* Along the middle extent of a contiguous [outer, n, inner] tensor, read where it lies: value_out / index_out are
 * [outer, inner], the position is the position along n. route and chunk as for pcmx_axis_reduce_* (the reduce halves of
 * the same routes; 0 picks by the PCMX_AXIS_* borders of a reduce, which were measured for 4-byte reductions and are
 * not measured for the 8-byte partials used here). n == 0 with outer and inner above 0 is PCMX_ERR_ARG; outer == 0 or
 * inner == 0 returns 0 and touches nothing. outer * n * inner < 2^31. The workspace (pcmx_axis_arg_workspace_bytes, one
 * call in flight per workspace) may be NULL for the routes that are not split. */
long long pcmx_axis_arg_workspace_bytes(long long outer, long long n, long long inner);
int pcmx_axis_arg_reduce_b32(const void* x, void* value_out, int32_t* index_out, long long outer, long long n, long long inner,
                             int key_type, int op, int route, long long chunk, void* workspace, hipStream_t s);
/* Over the segments [offsets[j], offsets[j+1]) of x, j < S, offsets as for pcmx_segment_reduce_* (same PRECONDITION,
 * not checked: offsets that break it give an unspecified result, but every load and store stays inside x[0, n),
 * offsets[0, S], the outputs' [0, S) and the workspace). index_out[j] is the FLAT position in x (offsets[j] <=
 * index_out[j] < offsets[j+1]); an empty segment gives -1 and the identity as its value. The merge-based scheme of
 * ragged.hip with (key, flat index) words: four launches, no block waits for another. n + S < 2^31; S == 0 returns 0
 * and touches nothing; x may be NULL when n == 0. Workspace: pcmx_segment_arg_workspace_bytes(n, S), one call in
 * flight per workspace. */
long long pcmx_segment_arg_workspace_bytes(long long n, long long S);
int pcmx_segment_arg_reduce_b32(const void* x, long long n, const int32_t* offsets, long long S, int key_type, int op,
                                void* value_out, int32_t* index_out, void* workspace, hipStream_t s);

/* ---------------------------------------------------------------- SGEMM (fp32 MFMA) */
/* C = alpha*A*B + beta*C, row-major. Fast path needs M%256==0, N%256==0 (or %128 for the small-tile
 * kernel), K%32==0, 16-B aligned rows; anything else returns -1 (the torch layer pads). */
int pcmx_sgemm_f32(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                   float alpha, float beta, hipStream_t s);
/* explicit kernel: 16 = register-staged 256x256x32 / 8 waves (large problems), 0 = LDS-DMA 256x256x32 / 8 waves,
 * 1 = LDS-DMA 128x128x32 / 4 waves (the lab variants live in scripts/sgemm_lab.hip) */
int pcmx_sgemm_f32_variant(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb,
                           int ldc, float alpha, float beta, int variant, hipStream_t s);
/* fp32 GEMM on the bf16 matrix cores, operands split exactly into 3 bf16 pieces, 6 piece products (fp32
 * accuracy; sgemm_x6.hip). M, N % 256 == 0, K % 32 == 0. Also reachable as pcmx_sgemm_f32_variant(..., 20). */
int pcmx_sgemm_f32_x6(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                      float alpha, float beta, hipStream_t s);
/* Reference-style f32 VALU GEMM (one thread per output, LDS tiles) for A/B comparisons. */
int pcmx_sgemm_f32_simt(const float* A, const float* B, float* C, int M, int N, int K, hipStream_t s);

/* ---------------------------------------------------------------- histogram equalisation */
/* out = tf[img] (bit-identical to the serial reference). ws: pcmx_histeq_workspace_bytes(), 16-B aligned, ZEROED
 * before the first call and left zeroed by every call (self-cleaning ticket); one call in flight per workspace. */
long long pcmx_histeq_workspace_bytes(void);
int pcmx_histeq_u8(const unsigned char* img, unsigned char* out, long long npix, void* ws, hipStream_t s);

/* ---------------------------------------------------------------- region growing */
long long pcmx_region2d_workspace_bytes(int H, int W);
/* padded (H+2) x ld arrays, interior 1..H x 1..W; halo cells are read-only seeds. Blocks once per batch. */
int pcmx_region2d_grow(const unsigned char* img, unsigned char* region, int H, int W, int ld, int thr, void* ws,
                       int batch, int max_launches, hipStream_t s, int* launches_out);
long long pcmx_region3d_workspace_bytes(int dim);
int pcmx_region3d_grow_tiled(const unsigned char* data, unsigned char* region, int dim, int thr, void* ws, int batch,
                             int max_launches, hipStream_t s, int* launches_out);
/* z-slab of a distributed volume: dim x dim x nz planes at data/region (plane 0 = first owned plane); halos bit 0 /
 * bit 1 = plane -1 / plane nz are readable halo planes (read-only seeds, never grown); dim % 16 == 0 */
long long pcmx_region3d_slab_workspace_bytes(int dim, int nz);
int pcmx_region3d_grow_slab(const unsigned char* data, unsigned char* region, int dim, int nz, int halos, int thr,
                            void* ws, int batch, int max_launches, hipStream_t s, int* launches_out);
/* reference 0/1/2 frontier semantics, one launch per BFS level; flag_ws: 4 device ints (the pipelined fixpoint check's
 * flag ring); region 16-B aligned */
int pcmx_region3d_grow_naive(const unsigned char* data, unsigned char* region, int dim, int thr, int* flag_ws,
                             int max_launches, hipStream_t s, int* launches_out);

/* ---------------------------------------------------------------- volume + ray casting */
int pcmx_volume_gen_u8(unsigned char* data, int dim, unsigned seed, hipStream_t s);
/* planes [z_first, z_first + nplanes) of the same volume (zeros outside 0..dim-1): a z-slab with halo planes */
int pcmx_volume_gen_slab_u8(unsigned char* data, int dim, int z_first, int nplanes, unsigned seed, hipStream_t s);
/* z-slab stage of the distributed reference caster (bit-identical to pcmx_raycast_global with f64 colour):
 * data/region start at global plane z0 - 1 and hold plane z1 when the slab has one above; state = 6 ints per pixel
 * {pos xyz, colour (f32 bits), steps, flags}, initialised by the first (top) slab when init != 0; the bottom slab
 * (bottom != 0) marches to the end and writes the image. */
int pcmx_raycast_slab(const unsigned char* data, const unsigned char* region, int dim, int z0, int* state, int init,
                      int bottom, unsigned char* image, int image_dim, const float* cam12, float pixel_width,
                      float step, int max_steps, hipStream_t s);
int pcmx_raycast_global(const unsigned char* data, const unsigned char* region, int dim, unsigned char* image,
                        int image_dim, const float* cam12, float pixel_width, float step, int max_steps, int f64_color,
                        hipStream_t s);
/* the same with an explicit caster variant (0 = production; 1 = one step in flight, 16x16 tiles; 2 / 3 = 4 / 16 steps
 * in flight): identical images, the lab's A/B (scripts/raycast_global_lab.py) */
int pcmx_raycast_global_variant(const unsigned char* data, const unsigned char* region, int dim, unsigned char* image,
                                int image_dim, const float* cam12, float pixel_width, float step, int max_steps,
                                int f64_color, int variant, hipStream_t s);
long long pcmx_raycast_dr16_bytes(int dim);
int pcmx_raycast_dr16_pack(const unsigned char* data, const unsigned char* region, int dim, void* dr, hipStream_t s);
int pcmx_raycast_global_dr(const void* dr, int dim, unsigned char* image, int image_dim, const float* cam12,
                           float pixel_width, float step, int max_steps, int f64_color, int variant, hipStream_t s);
/* texture path: tex holds dim^3 * 16 + 16 bytes: per-voxel texels with the 2x2x2 footprint of data and region
 * (8-byte texels when every data value < 128, else 16-byte; the format flag is stored behind the texels),
 * dim <= 2048 */
int pcmx_brick_pack(const unsigned char* data, const unsigned char* region, int dim, void* tex, hipStream_t s);
/* texture ray caster; batch = steps per prefetch batch (1, 4, 8, 16; 0 = 16, the measured best); segments = waves
 * marching one ray patch, each a contiguous share of the step range (1, 2, 4; 0 = the measured best) */
int pcmx_raycast_bricked(const void* tex, int dim, unsigned char* image, int image_dim,
                         const float* cam12, float pixel_width, float step, int max_steps, int batch, int segments,
                         hipStream_t s);

/* ---------------------------------------------------------------- stencil */
int pcmx_stencil5_bf16(const void* u, void* out, int rows, int cols, int ld, int r0, int r1, long long global_row0,
                       long long global_rows, float k, hipStream_t s);
/* `steps` (2, 3, 4, 6, 8) fused updates (temporal blocking, bit-identical to single steps) over local rows
 * [r0, r1) of a (rows + 2*halo) x ld slab; cols % 8 == 0; rows within `steps` of a non-global slab edge need
 * halo >= steps. pcmx_stencil5x2_bf16 = steps 2. */
int pcmx_stencil5xT_bf16(const void* u, void* out, int rows, int cols, int ld, int halo, int steps, int r0, int r1,
                         long long global_row0, long long global_rows, float k, hipStream_t s);
/* the same over two row spans [r0a, r1a) and [r0b, r1b) (disjoint, either may be empty) in ONE launch: the
 * distributed step updates both rank-edge bands with one kernel once the halo rows have arrived */
int pcmx_stencil5xT_bf16_spans(const void* u, void* out, int rows, int cols, int ld, int halo, int steps, int r0a,
                               int r1a, int r0b, int r1b, long long global_row0, long long global_rows, float k,
                               hipStream_t s);
/* the same with an explicit launch shape of this launch (0 = production rule; bits 0-7 columns per lane 4 / 8, 8-15 rows
 * per wave, 16-23 prefetch ring depth 3 / 6 / 9; bits 24 and above must be 0, else -1): the lab sweeps, no state kept
 * in the library */
int pcmx_stencil5xT_bf16_spans_shape(const void* u, void* out, int rows, int cols, int ld, int halo, int steps, int r0a,
                                     int r1a, int r0b, int r1b, long long global_row0, long long global_rows, float k,
                                     int shape, hipStream_t s);
int pcmx_stencil5x2_bf16(const void* u, void* out, int rows, int cols, int ld, int halo, int r0, int r1,
                         long long global_row0, long long global_rows, float k, hipStream_t s);

/* ---------------------------------------------------------------- SpMV */
/* CSR-adaptive analysis: cuts the rows of a HOST row_ptr (n_rows + 1 entries) into work items of at most 1024
 * nonzeros (4 x int64 words each, written to items_host); returns the item count, or -1 when max_items is too small
 * (items_host == NULL: count only). */
long long pcmx_spmv_csr_plan(const long long* row_ptr_host, int n_rows, void* items_host, long long max_items);
/* the same cut with items of at most item_nnz (64..1024, multiple of 64) nonzeros */
long long pcmx_spmv_csr_plan_nnz(const long long* row_ptr_host, int n_rows, void* items_host, long long max_items,
                                 int item_nnz);
/* y = A x for a CSR matrix of any sparsity, one wave per item of pcmx_spmv_csr_plan (device arrays). */
int pcmx_spmv_csr(const long long* row_ptr, const int* col, const float* val, const float* x, float* y, int n_rows,
                  const void* items, long long n_items, hipStream_t s);

#define PCMX_SPMV_MAX_SLICES 32
/* which part of a sliced product one pcmx_spmv_sliced call runs */
enum {
    PCMX_SPMV_ALL = 0,      /* products, combine and fix-up */
    PCMX_SPMV_PRODUCTS = 1, /* the compact partials (ypart, extra) only */
    PCMX_SPMV_COMBINE = 2   /* combine + fix-up of the partials a PCMX_SPMV_PRODUCTS call wrote */
};
/* XCD-sliced CSR (ops/sparse.py SlicedCSR): n_slices = 8 * phases <= PCMX_SPMV_MAX_SLICES; per nonzero col, val
 * and lrow (u16 offset of its row inside its item, rows counted among the rows the slice touches); per slice
 * nnz-balanced items over the slice's touched rows (a later piece of a split long row has row1 == row0).
 * Slice s runs on the blocks b with b % 8 == s % 8 (one XCD) and writes one compact partial per touched row to
 * ypart[slice_out0[s] + touched-row index]; a combine pass sums each row's partials into y (row_mask[r] bit s:
 * slice s touches row r; chunk_base[c * n_slices + s]: touched rows of slice s before row 64c) and a fix-up adds
 * extra[fix[k].item] to y[fix[k].row]. slice_nz0 / slice_item0 / slice_out0 are HOST arrays (n_slices,
 * n_slices + 1 and n_slices + 1 entries).
 *  slice_colbase  HOST array of n_slices first tail columns: col holds the packed words (column offset | head flag |
 *                 row offset << 22) and lrow is not read; NULL: the unpacked col + lrow arrays.
 *  item_nnz       the size the items were planned with: 1024 or 512; 384 or 256 with slice_colbase only.
 *  stage          PCMX_SPMV_ALL, PCMX_SPMV_PRODUCTS or PCMX_SPMV_COMBINE.
 *  ballot_combine 1: the ballot-rank combine instead of the byte-packed scan (same bits; taken anyway when the
 *                 partials reach 2^30, which the scan's 32-bit offsets cannot address); 0: the scan.
 *  blocks_per_cu  resident product blocks per CU, 1..255; 0: the library default, 3.
 *  phase_lo, phase_n  the products cover slices [8 phase_lo, 8 (phase_lo + phase_n)); phase_n 0: all from phase_lo.
 * A value outside these sets returns PCMX_ERR_ARG before anything is launched. */
int pcmx_spmv_sliced(const unsigned short* lrow, const int* col, const float* val, const float* x, float* ypart,
                     float* extra, float* y, int n_rows, int n_cols, int n_slices, const long long* slice_nz0,
                     const long long* slice_item0, const long long* slice_out0, const void* items,
                     const unsigned* row_mask, const int* chunk_base, const void* fix, int n_fix, int item_nnz,
                     int stage, int ballot_combine, int blocks_per_cu, int phase_lo, int phase_n,
                     const int* slice_colbase, hipStream_t s);
/* products only of phases [a_lo, a_lo + a_n) of sliced matrix A and [b_lo, b_lo + b_n) of B (same x) in ONE launch.
 * Packed layout only; item_nnz (256, 384, 512 or 1024) is the item size of both matrices, blocks_per_cu as above;
 * nz0 / item0 / out0 / colbase: host arrays per matrix. Each matrix then combines its own partials. */
int pcmx_spmv_sliced_pair(const float* x, int n_cols, int item_nnz, int blocks_per_cu, const int* col_a,
                          const float* val_a, const void* items_a, float* ypart_a, float* extra_a, int s_a,
                          const long long* nz0_a, const long long* item0_a, const long long* out0_a,
                          const int* colbase_a, int a_lo, int a_n, const int* col_b, const float* val_b,
                          const void* items_b, float* ypart_b, float* extra_b, int s_b, const long long* nz0_b,
                          const long long* item0_b, const long long* out0_b, const int* colbase_b, int b_lo, int b_n,
                          hipStream_t s);
/* the combine + split-row fix-up (+ send-buffer pack: sendbuf[send_slot[p]] = y[r] for p in send_ptr[r] ..
 * send_ptr[r + 1]) of the partials a products-only call (PCMX_SPMV_PRODUCTS, or pcmx_spmv_sliced_pair) wrote, in ONE
 * launch. slice_out0: host array of n_slices + 1 partial offsets (fewer than 2^30 partials); fix: int2 {item, row}
 * sorted by row; fix_chunk0: the fix range of every 64-row chunk (n_rows / 64 + 2 ints, or NULL: no split rows);
 * send_ptr (n_rows + 1) / send_slot / sendbuf may be NULL (no pack). Same bits as combine + fix-up. */
int pcmx_spmv_sliced_combine(const float* ypart, const unsigned* row_mask, const int* chunk_base,
                             const long long* slice_out0, int n_slices, float* y, int n_rows, const float* extra,
                             const void* fix, const int* fix_chunk0, const int* send_ptr, const int* send_slot,
                             float* sendbuf, hipStream_t s);
/* banded product with implicit column indices (bands a .. e as in the reference's create_csr_matrix): variant 8 of
 * pcmx_spmv_banded_variant */
int pcmx_spmv_banded(const float* vals, const long long* row_off, int n, int a, int b, int c, int d, int e,
                     const float* x, float* y, hipStream_t s);
/* variant 0: one wave per row (strided band loops, global x); 1: LDS-staged x windows, 16 rows per block, 2 rows per
 * wave in flight, 4-B value loads; 8: each 16-row block's values as one aligned 16-B stream (falls back to 1 for rows
 * under 256 nonzeros, values not 16-B aligned, a stream capture before the geometry's table exists, or a failed table
 * allocation). 1 and 8 fall back to 0 for rows above 16 x 64 nonzeros. Any other variant: PCMX_ERR_ARG. */
int pcmx_spmv_banded_variant(const float* vals, const long long* row_off, int n, int a, int b, int c, int d, int e,
                             const float* x, float* y, int variant, hipStream_t s);
/* Which kernel pcmx_spmv_banded_variant takes for this geometry and variant, from the same host predicate the launcher
 * dispatches on; launches nothing and reads no device memory. vals_aligned: whether the value array is 16-B aligned.
 * Returns 0 (one wave per row), 1 (the LDS-window kernel) or 8 (the block stream), or PCMX_ERR_ARG for the geometries
 * and variants the launcher refuses. *nl (may be NULL): the LDS kernel's instantiation (2, 4, 6, 8, 10, 12 or 16
 * chunks of 64 nonzeros per row) for 1, and for 8 the one a fall-back would take; 0 otherwise. Geometry only: a stream
 * capture before the geometry's table exists, or a failed table allocation, still turns 8 into 1 at launch, and a call
 * with n <= 0 launches nothing. */
int pcmx_spmv_banded_path(int n, int a, int b, int c, int d, int e, int variant, int vals_aligned, int* nl);

/* ---------------------------------------------------------------- SpMM (kernels/spmm.hip) */
/* Y[n_rows, k] = A X for a CSR matrix and row-major f32 X (leading dimension ldx >= k) and Y (ldy >= k); device
 * arrays. items / n_items: the work items of pcmx_spmv_csr_plan_nnz(item_nnz). slot[item]: the workspace slot of a
 * piece of a split row (the pieces of one row take consecutive slots in piece order), -1 for every other item.
 * split: n_split x {row, first slot, pieces} (int32). ws: n_pieces rows of ((k + 3) & ~3) floats, 16-B aligned;
 * ws_floats its size. One wave per item and column tile; a fix-up launch sums each split row's pieces in piece order:
 * no atomics, no memset, the same bits on every call. Every row of Y is written once (an empty row as +0.0), columns
 * k .. ldy - 1 are not touched. Returns PCMX_ERR_ARG, before anything is launched, for k < 0, n_rows < 0, ldx < k,
 * ldy < k, an item_nnz that is no multiple of 64 in 64..1024, a workspace smaller than n_pieces rows (or misaligned),
 * and n_rows > 0 without items. */
int pcmx_spmm_csr(const long long* row_ptr, const int* col, const float* val, const float* x, long long ldx, float* y,
                  long long ldy, int n_rows, int k, const void* items, long long n_items, const int* slot,
                  const int* split, int n_split, long long n_pieces, int item_nnz, float* ws, long long ws_floats,
                  hipStream_t s);
/* Which kernels pcmx_spmm_csr takes for these operands, from the predicate the launcher dispatches on; launches
 * nothing and reads no memory (x_addr / y_addr: the operands' addresses). Returns the class of the first column tile:
 * 4, 8, 16 or 32 lanes per group (k <= 32), or a tile of 64 (from k = 33), 128 or 256 columns (256 for every
 * k >= 256); 0 for k == 0;
 * PCMX_ERR_ARG for k < 0, ldx < k or ldy < k. *tail_class (may be NULL): the class of the partial last tile of a
 * k > 256 (0: none). *vec (may be NULL): bit 0: the first class moves float2 / float4 (both addresses and both leading
 * dimensions aligned to its vector), bit 1: so does the tail class; a clear bit on a 128 / 256 class means dword form. */
int pcmx_spmm_path(int k, unsigned long long x_addr, long long ldx, unsigned long long y_addr, long long ldy,
                   int* tail_class, int* vec);

/* ---------------------------------------------------------------- halo pack/unpack */
int pcmx_pack_edges(const void* tile, int elem_bytes, int H, int W, int ld, void* buf, hipStream_t s);
int pcmx_unpack_halo(void* tile, int elem_bytes, int H, int W, int ld, const void* buf, int mask, hipStream_t s);
/* as pcmx_unpack_halo, and *changed (device int) is set to 1 when any halo cell takes a new value */
int pcmx_unpack_halo_changed(void* tile, int elem_bytes, int H, int W, int ld, const void* buf, int mask, int* changed,
                             hipStream_t s);

/* ---------------------------------------------------------------- grouped exchange on a dedicated RCCL communicator
 * (comm/exchange_rccl.hip): per-peer byte segments send[soff[q] .. + scnt[q]) -> peer q, recv[roff[q] .. + rcnt[q])
 * <- peer q, on the communicator's stream, ordered after `compute` (event) and waited for by pcmx_xcomm_wait. */
int pcmx_xcomm_id_bytes(void);
int pcmx_xcomm_unique_id(void* out);
int pcmx_xcomm_create(const void* id, int world, int rank, int device, void** out);
int pcmx_xcomm_exchange(void* handle, int slot, const void* send, const long long* soff, const long long* scnt,
                        void* recv, const long long* roff, const long long* rcnt, hipStream_t compute);
int pcmx_xcomm_wait(void* handle, int slot, hipStream_t compute);
int pcmx_xcomm_probe(void* handle, int timeout_ms);
int pcmx_xcomm_async_error(void* handle);
int pcmx_xcomm_destroy(void* handle);

#ifdef __cplusplus
}
#endif
#endif /* PCMX_HIP_H */
