"""Element-wise, reduction and scan ops.

GPU tensors run the hand-written gfx950 kernels (``torch.ops.pcmx.*``); CPU tensors run the host C library
(OpenMP) or, where the reference has no host routine, an exact torch reference. The CPU path exists so the
distributed algorithms can be exercised with the gloo backend on a GPU-less machine.

Reference parity: vmul = 6-opencl-region-growing/multiply_opencl.cl:1-4 (host check multiply_opencl.c:10-14);
reduce MIN/SUM = the MPI_Allreduce of 2-mpi-region-growing/region.c:437; scan = the histogram CDF
(4-histogram-equalization-openmp-pthreads/histogram_serial.c:29-34) generalised.
"""
from __future__ import annotations

import torch

from .._native import cpu_lib, ops

OP_CODES = {"sum": 0, "min": 1, "max": 2}


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def vmul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """r[i] = a[i] * b[i]."""
    if a.is_cuda:
        return ops().vmul(a, b).view(a.shape)
    a, b = _f32(a, "a"), _f32(b, "b")
    r = torch.empty_like(a)
    cpu_lib().pcmx_vmul_host(a.data_ptr(), b.data_ptr(), r.data_ptr(), a.numel())
    return r


def vadd(a: torch.Tensor, b: torch.Tensor, n_threads: int = 0) -> torch.Tensor:
    """r[i] = a[i] + b[i] (OpenMP on the host, float4 streaming kernel on the GPU)."""
    if a.is_cuda:
        return ops().vadd(a, b).view(a.shape)
    a, b = _f32(a, "a"), _f32(b, "b")
    r = torch.empty_like(a)
    cpu_lib().pcmx_vadd_omp(a.data_ptr(), b.data_ptr(), r.data_ptr(), a.numel(), n_threads)
    return r


def gather_(src: torch.Tensor, idx: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[i] = src[idx[i]] (int32 indices): the HIP gather kernel on the GPU (the SpMV send-buffer pack),
    torch.index_select on the host. The kernel addresses src with 32-bit byte offsets: a src of 2^29 or more floats
    takes torch.index_select on the GPU too."""
    if src.is_cuda and src.numel() < (1 << 29):
        return ops().gather_(src, idx, out)
    return torch.index_select(src, 0, idx.long(), out=out)


def axpy_(y: torch.Tensor, alpha: float, x: torch.Tensor, n_threads: int = 0) -> torch.Tensor:
    """y <- alpha * x + y in place."""
    if y.is_cuda:
        return ops().axpy_(y, float(alpha), x)
    x = _f32(x, "x")
    assert y.is_contiguous() and y.dtype == torch.float32
    cpu_lib().pcmx_axpy_omp(float(alpha), x.data_ptr(), y.data_ptr(), y.numel(), n_threads)
    return y


def copy_(dst: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """dst <- src (f32): the ticket-ordered streaming kernel on the GPU, torch's copy on the host."""
    if dst.is_cuda:
        return ops().copy_(dst, src)
    return dst.copy_(src)


def dot(a: torch.Tensor, b: torch.Tensor, n_threads: int = 0) -> torch.Tensor:
    """sum(a*b) as a 0-d float32 tensor (f64 host accumulation / f64 final fold on the GPU).

    On the GPU the products are summed as ``reduce`` sums float32: from +0.0 (a dot of -0.0 products is +0.0), NaN and
    inf are handed on, the same bits on every call and stream; empty operands give +0.0. Any view is accepted
    (strided or not 16-byte aligned operands are copied first; the inputs are never written)."""
    if a.is_cuda:
        return ops().dot(a, b)
    a, b = _f32(a, "a"), _f32(b, "b")
    return torch.tensor(cpu_lib().pcmx_dot_omp(a.data_ptr(), b.data_ptr(), a.numel(), n_threads), dtype=torch.float32)


def reduce(x: torch.Tensor, op: str = "sum", dim: int | None = None, keepdim: bool = False, route: str | None = None,
           chunk: int | None = None) -> torch.Tensor:
    """Global reduction of a float32/int32 tensor to a 0-d tensor (op in sum/min/max). dim=int: the reduction of every
    row along dim, torch's shape (dim removed, or kept with size 1 under keepdim); keepdim, route and chunk go with dim
    (the along-a-dimension section below).

    The global reduction on the GPU (two passes, the second folds the block partials in f64 / int64 in a fixed order:
    the same bits on every call and stream):
      * a float32 sum starts from +0.0, so a sum of -0.0 alone is +0.0; it hands on NaN and inf, and +inf with -inf
        gives NaN;
      * float32 min and max skip NaNs wherever they stand; an all-NaN input gives the identity, +inf for min and -inf
        for max (torch.min / max hand the NaN on);
      * int32 sums wrap mod 2^32 (the block partials wrap in int32, their int64 fold is cast back; the CPU path casts
        an int64 sum back and agrees); int32 min and max are exact, INT32_MIN / INT32_MAX inputs included;
      * numel() == 0 gives the identity: +0.0, +inf, -inf (int32: 0, INT32_MAX, INT32_MIN);
      * any view is accepted (strided or not 16-byte aligned input is copied first; the input is never written)."""
    if dim is not None:
        return _axis_reduce(x, op, dim, keepdim, route, chunk)
    if keepdim or route is not None or chunk is not None:
        raise ValueError("reduce: keepdim, route and chunk are for the reduction along a dimension: they need dim=")
    code = OP_CODES[op]
    if x.is_cuda:
        return ops().reduce(x, code)
    if op == "sum":
        if x.dtype == torch.float32:
            xc = x.contiguous()
            return torch.tensor(cpu_lib().pcmx_sum_omp(xc.data_ptr(), xc.numel(), 0), dtype=torch.float32)
        return x.sum(dtype=torch.int64).to(x.dtype)
    return x.min() if op == "min" else x.max()


def scan(x: torch.Tensor, exclusive: bool = False, init: torch.Tensor | None = None,
         check: bool = False, dim: int | None = None, op: str = "sum", out: torch.Tensor | None = None,
         route: str | None = None, chunk: int | None = None) -> torch.Tensor:
    """Prefix sum over the flattened tensor (decoupled look-back single pass on the GPU).

    ``init`` (a 1-element float32 tensor on the same device) is added to every output; the multi-GPU
    scan feeds its rank offset through it without a host round trip. ``check=True`` waits for the current
    stream and raises if this (or an earlier unchecked) scan on it gave up a look-back (scan_check).
    ``dim=int``: the running op (sum, min, max; float32 or int32) of every row along dim, x's shape; op, out, route
    and chunk go with dim (the along-a-dimension section below).
    A multi-dimensional or strided x is scanned in its logical (row-major flattened) order and the result has x's
    shape; numel() == 0 returns an empty tensor. A NaN or inf at position p reaches every output from p on (exclusive:
    after p) and leaves the outputs before it as they are without it; +inf and a later -inf give NaN from the second on.
    """
    if dim is not None:
        return _axis_scan(x, op, exclusive, init, check, dim, out, route, chunk)
    if op != "sum" or out is not None or route is not None or chunk is not None:
        raise ValueError("scan: op, out, route and chunk are for the scan along a dimension: they need dim=")
    if x.is_cuda:
        y = ops().scan(x, exclusive, init)
        if check:
            scan_check(x.device)
        return y
    xf = _f32(x, "x").view(-1)
    out = torch.cumsum(xf.double(), 0)
    if exclusive:
        out = torch.cat([out.new_zeros(1), out[:-1]])
    if init is not None:
        out = out + init.double().view(-1)[0]
    return out.float().view(x.shape)


def scan_check(device=None) -> None:
    """Synchronise the current stream of `device` and raise if a scan on it timed out in its look-back."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    ops().scan_check(dev.index if dev.index is not None else torch.cuda.current_device())


def fill_(x: torch.Tensor, value: float) -> torch.Tensor:
    if x.is_cuda:
        return ops().fill_(x, float(value))
    return x.fill_(value)


def rand_uniform_(x: torch.Tensor, seed: int = 0, lo: float = -1.0, hi: float = 1.0) -> torch.Tensor:
    """Counter-based uniform fill generated on the device (no host staging for 1e9-element inputs)."""
    if x.is_cuda:
        return ops().rand_uniform_(x, int(seed), float(lo), float(hi))
    g = torch.Generator().manual_seed(int(seed))
    return x.uniform_(lo, hi, generator=g)


# ---------------------------------------------------------------- stream compaction (select / nonzero)
# Keep the elements a mask or a predicate selects, in input order, and report how many were kept. On the GPU this is
# one pass on the scan's decoupled look-back carrying the exact integer kept count (csrc/kernels/select.hip); the
# ancestor is the pixel-stack frontier of the region programs (ref 2-mpi-region-growing/region.c:493-533). The
# compact* forms return (out, count) with count a 0-d int64 tensor on x's device and never synchronise: out has room
# for every element and only out[:count] is written. select / select_indices cut out to the exact size (one host sync).
CMP_CODES = {"gt": 0, "ge": 1, "lt": 2, "le": 3, "eq": 4, "ne": 5}
_CMP_TORCH = {"gt": torch.gt, "ge": torch.ge, "lt": torch.lt, "le": torch.le, "eq": torch.eq, "ne": torch.ne}


def _check_mask(mask: torch.Tensor, n: int | None) -> None:
    if mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"mask must be bool or uint8, got {mask.dtype}")
    if n is not None and mask.numel() != n:
        raise ValueError(f"mask has {mask.numel()} elements, x has {n}")


def _check_out(out: torch.Tensor | None, dtype: torch.dtype, n: int, like: torch.Tensor) -> None:
    if out is None:
        return
    if out.dtype != dtype:
        raise TypeError(f"out must be {dtype}, got {out.dtype}")
    if out.device != like.device:
        raise ValueError(f"out is on {out.device}, the input on {like.device}")
    if out.dim() != 1 or not out.is_contiguous() or out.numel() < n:
        raise ValueError(f"out must be 1-D, contiguous, with room for all {n} elements (the count is not known "
                         f"before the kernel ran), got shape {tuple(out.shape)}")


def _host_result(kept: torch.Tensor, n: int, out: torch.Tensor | None):
    """The CPU paths' (out, count): the kept elements at the front of an n-element (or the caller's) tensor."""
    if out is None:
        out = kept.new_empty(n)
    out[:kept.numel()] = kept
    return out, torch.tensor(kept.numel(), dtype=torch.int64)


def compact(x: torch.Tensor, mask: torch.Tensor, out: torch.Tensor | None = None):
    """(out, count): out[j] = x.flatten()[i] for the j-th i with mask.flatten()[i] != 0, count of them as a 0-d int64
    tensor on x's device. x float32 or int32 (moved as bits: NaN payloads survive), mask bool or uint8 of the same
    numel (any nonzero byte keeps). out (optional, 1-D, >= x.numel() elements) is left untouched past count. Does not
    synchronise."""
    if x.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"x must be float32 or int32, got {x.dtype}")
    _check_mask(mask, x.numel())
    _check_out(out, x.dtype, x.numel(), x)
    if x.is_cuda:
        return tuple(ops().select(x, mask, out))
    return _host_result(x.reshape(-1)[mask.reshape(-1) != 0], x.numel(), out)


def select(x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """x.flatten()[mask.flatten()] as a tensor of exactly count elements (one host sync for the count)."""
    out, count = compact(x, mask)
    return out[:int(count.item())]


def compact_indices(mask: torch.Tensor, out: torch.Tensor | None = None):
    """(idx, count): the int32 flat indices of the nonzero mask elements, ascending (a flattened nonzero), and their
    count as a 0-d int64 tensor on the mask's device. Does not synchronise."""
    _check_mask(mask, None)
    if mask.numel() >= 1 << 31:
        raise ValueError("compact_indices: indices are int32, the mask must have fewer than 2^31 elements")
    _check_out(out, torch.int32, mask.numel(), mask)
    if mask.is_cuda:
        return tuple(ops().select_index(mask, out))
    return _host_result(torch.nonzero(mask.reshape(-1)).reshape(-1).int(), mask.numel(), out)


def select_indices(mask: torch.Tensor) -> torch.Tensor:
    """torch.nonzero(mask.flatten()).flatten().int(), exact size (one host sync for the count)."""
    idx, count = compact_indices(mask)
    return idx[:int(count.item())]


def compact_where(x: torch.Tensor, op: str, threshold: float, indices: bool = False, out: torch.Tensor | None = None):
    """(out, count) of the elements of float32 x with x OP threshold, op in gt/ge/lt/le/eq/ne with IEEE semantics (NaN
    is kept only by ne; the threshold is compared as float32). indices=True writes their int32 flat indices instead
    of the values. No mask is materialised on the GPU. Does not synchronise."""
    if op not in CMP_CODES:
        raise ValueError(f"op must be one of {sorted(CMP_CODES)}, got {op!r}")
    if x.dtype != torch.float32:
        raise TypeError(f"x must be float32, got {x.dtype}")
    _check_out(out, torch.int32 if indices else torch.float32, x.numel(), x)
    if x.is_cuda:
        return tuple(ops().select_if(x, CMP_CODES[op], float(threshold), bool(indices), out))
    xf = x.reshape(-1)
    keep = _CMP_TORCH[op](xf, torch.tensor(float(threshold), dtype=torch.float32))
    kept = torch.nonzero(keep).reshape(-1).int() if indices else xf[keep]
    return _host_result(kept, x.numel(), out)


# ---------------------------------------------------------------- radix sort (keys, pairs, argsort)
# Stable sort of float32 / int32 keys, flattened, in torch.sort(stable=True)'s order with int32 indices. On the GPU a
# least-significant-digit radix sort, 8 bits per pass, each pass one kernel on the scan's decoupled look-back run over
# 256 digit counters (csrc/kernels/sort.hip); no counterpart in the reference programs. Nothing synchronises; a
# look-back that gave up is reported by scan_check(), as for scan and select.
#  * float32 order: -inf < ... < -0.0 == +0.0 < ... < +inf < NaN. Signed zeros tie, all NaNs tie (either sign, any
#    payload), ties keep input order. Sorted float32 KEYS come out canonical: both zeros as +0.0, every NaN as the one
#    NaN with bits 0x7fffffff. A caller who needs the original bits gathers with the indices. Values (sort_by_key) are
#    moved as bits and keep theirs.
#  * descending reverses the order of the keys, not of ties: equal keys stay in input order, as in torch.
#  * bits=B (int32 keys only): the caller promises 0 <= key < 2**B and only ceil(B / 8) passes run. The defined
#    semantics for any input are "stable sort by the low B bits"; the keys themselves come out unchanged.
#  * Measured against torch.sort on one MI355X at 2^28 keys (profiles/r8_sort/README.md): sort_keys 1.5-2.4x faster,
#    argsort(bits=20) 1.4-1.6x faster, sort on int32 1.27x faster. sort (values + indices) on float32 is SLOWER than
#    torch.sort(stable=True): 10.16 ms against 9.73 ms on uniform keys, 9.46 against 7.85 ms when all keys are equal.
_NAN_BITS = 0x7FFFFFFF
SORT_MAX_N = (1 << 30) - 1


def _check_sort_keys(x: torch.Tensor, bits, name: str = "x") -> int:
    """Validates keys / bits and returns the number of compared bits."""
    if x.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"{name} must be float32 or int32, got {x.dtype}")
    if x.numel() > SORT_MAX_N:
        raise ValueError(f"{name} has {x.numel()} elements; indices and digit counts are 30-bit (at most 2^30 - 1)")
    if bits is None:
        return 32
    if isinstance(bits, bool) or not isinstance(bits, int):
        raise TypeError(f"bits must be an int, got {type(bits).__name__}")
    if x.dtype != torch.int32:
        raise TypeError(f"bits is for int32 keys only, {name} is {x.dtype}")
    if not 1 <= bits <= 32:
        raise ValueError(f"bits must be in 1..32, got {bits}")
    return bits


def _host_order(x: torch.Tensor, descending: bool, nbits: int) -> torch.Tensor:
    """int64 indices of the stable sort of flat x by its low nbits bits (all of x when nbits == 32)."""
    key = x if nbits == 32 else x.long() & ((1 << nbits) - 1)
    return torch.sort(key, stable=True, descending=descending).indices


def _canonical_f32(v: torch.Tensor) -> torch.Tensor:
    """What the kernel's inverse key transform yields: +0.0 for both zeros, bits 0x7fffffff for every NaN."""
    if v.dtype != torch.float32:
        return v
    v = torch.where(v == 0, torch.zeros_like(v), v)
    return torch.where(torch.isnan(v), torch.full_like(v.view(torch.int32), _NAN_BITS).view(torch.float32), v)


def sort_keys(x: torch.Tensor, descending: bool = False, bits: int | None = None, dim: int | None = None,
              route: str | None = None) -> torch.Tensor:
    """The sorted values of x.flatten() (float32 or int32), 1-D. float32 zeros and NaNs come out canonical (above).
    dim=int: every row along dim is sorted on its own, the result has x's shape (the row-wise section below)."""
    if dim is not None:
        return _row_sort(x, None, "keys", descending, bits, dim, route)[0]
    _no_route(route)
    nbits = _check_sort_keys(x, bits)
    if x.is_cuda:
        return ops().sort_keys(x, bool(descending), 0, nbits)
    xf = x.reshape(-1)
    return _canonical_f32(xf[_host_order(xf, bool(descending), nbits)])


def sort(x: torch.Tensor, descending: bool = False, bits: int | None = None, dim: int | None = None,
         route: str | None = None):
    """(values, indices) of the stable sort of x.flatten(): torch.sort(x.flatten(), stable=True) with int32 indices.
    On float32 this is slower than torch on an MI355X (2^28 keys: 10.16 ms against 9.73 ms; faster on int32).
    dim=int: torch.sort(x, dim, stable=True) with int32 positions along dim (the row-wise section below)."""
    if dim is not None:
        return _row_sort(x, None, "index", descending, bits, dim, route)
    _no_route(route)
    nbits = _check_sort_keys(x, bits)
    if x.is_cuda:
        return tuple(ops().sort_index(x, bool(descending), 0, nbits, True))
    xf = x.reshape(-1)
    order = _host_order(xf, bool(descending), nbits)
    return _canonical_f32(xf[order]), order.int()


def argsort(x: torch.Tensor, descending: bool = False, bits: int | None = None, dim: int | None = None,
            route: str | None = None) -> torch.Tensor:
    """The int32 indices of the stable sort of x.flatten(); no sorted-keys tensor is written. dim=int: the int32
    positions along dim of every row's stable sort, x's shape (the row-wise section below)."""
    if dim is not None:
        return _row_sort(x, None, "argsort", descending, bits, dim, route)[1]
    _no_route(route)
    nbits = _check_sort_keys(x, bits)
    if x.is_cuda:
        return ops().sort_index(x, bool(descending), 0, nbits, False)[1]
    return _host_order(x.reshape(-1), bool(descending), nbits).int()


def sort_by_key(keys: torch.Tensor, values: torch.Tensor, descending: bool = False, bits: int | None = None,
                dim: int | None = None, route: str | None = None):
    """(keys_sorted, values_sorted): values (float32 or int32, same numel, moved as bits) reordered with their keys.
    dim=int: row by row along dim; values must then have the shape of keys (the row-wise section below)."""
    if dim is not None:
        return _row_sort(keys, values, "pairs", descending, bits, dim, route)
    _no_route(route)
    nbits = _check_sort_keys(keys, bits, "keys")
    if values.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"values must be float32 or int32, got {values.dtype}")
    if values.numel() != keys.numel():
        raise ValueError(f"{values.numel()} values for {keys.numel()} keys")
    if values.device != keys.device:
        raise ValueError(f"values are on {values.device}, the keys on {keys.device}")
    if keys.is_cuda:
        return tuple(ops().sort_pairs(keys, values, bool(descending), 0, nbits))
    kf = keys.reshape(-1)
    order = _host_order(kf, bool(descending), nbits)
    # (indexing an int32 view: a float gather would be free to quieten a signalling NaN payload)
    vbits = values.reshape(-1).view(torch.int32)[order]
    return _canonical_f32(kf[order]), vbits.view(values.dtype)


# ---------------------------------------------------------------- top-k / k-th value (radix select)
# The k best elements of the flattened input and the k-th value, in sort's order (above) and DEFINED by it:
#     topk(x, k, largest) == tuple(t[:k] for t in sort(x, descending=largest)), bit for bit.
# On the GPU nothing is sorted but the k survivors (csrc/kernels/topk.hip; no counterpart in the reference programs):
# a most-significant-digit radix select finds the k-th key from four histogram passes over the keys (reads, no writes,
# the digit chosen on the device, no inter-block waiting), one pass on the scan's decoupled look-back gathers the k
# survivors in index order, and the stable pair sort orders them. Nothing synchronises with the host; the output size
# is k, known on the host, so there is no exact-size form; a look-back that gave up is reported by scan_check().
#  * Indices are int32 flat indices. Among elements that tie with the k-th key the LOWEST flat indices are taken, and
#    ties come out in ascending index order. This is stricter than torch.topk, which leaves the choice among ties open.
#  * float32 values come out canonical, as from sort_keys: +0.0 for both zeros, bits 0x7fffffff for every NaN. NaNs are
#    the largest keys: they lead for largest=True.
#  * sorted=False: the same k elements in ascending flat-index order (no survivor sort runs).
#  * method (tests and the lab): "select" runs the radix-select kernels, "sort" runs sort and slices, None picks by the
#    measured rule: the sort route when sorted and k > TOPK_SORT_FRACTION * numel, select otherwise (sorted=False is
#    select for every k: 5.6x to 12x faster than sort, slice and re-order at every measured k).
#  * Measured on one MI355X at 2^28 keys, uniform / all equal / already sorted, largest=True
#    (profiles/r10_topk/README.md): select is 4.1x-13.4x faster than torch.topk and 4.4x-12.2x faster than sort and
#    slice for k <= 2^24, and 1.26x-2.0x / 1.4x-1.6x at k = numel / 2 with sorted=True. The survivor sort grows with
#    k: on uniform keys select is level with sort and slice at k = 3/4 numel (f32 9.88 against 10.07 ms, i32 9.50
#    against 9.94) and slower at 7/8 numel (f32 11.14 against 10.09 ms, i32 10.64 against 9.95), hence the constant.
#    method="select" on float32 with sorted=True and k >= 7/8 numel is SLOWER than torch.topk (11.14 against 10.86 ms
#    at 7/8 numel, 12.72 against 11.03 ms at k = numel); the default rule takes the sort route there (10.09 ms). The
#    sort route inherits sort's standing on float32: on all-equal keys it is slower than torch.topk (9.49 against
#    8.52 ms at k = numel / 2).
TOPK_SORT_FRACTION = 0.75
_TOPK_METHODS = (None, "select", "sort")


def _check_topk(x: torch.Tensor, k, k_min: int, name: str) -> None:
    if x.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"{name}: x must be float32 or int32, got {x.dtype}")
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"{name}: k must be an int, got {type(k).__name__}")
    if x.numel() > SORT_MAX_N:
        raise ValueError(f"{name}: x has {x.numel()} elements; indices and digit counts are 30-bit (at most 2^30 - 1)")
    if not k_min <= k <= x.numel():
        raise ValueError(f"{name}: k must be in {k_min}..{x.numel()} (the number of elements), got {k}")


def topk(x: torch.Tensor, k: int, largest: bool = True, sorted: bool = True, method: str | None = None,
         dim: int | None = None, route: str | None = None):
    """(values, indices): the k largest (or smallest) elements of x.flatten() (float32 or int32, at most SORT_MAX_N
    elements, never written) and their int32 flat indices; exactly the first k entries of sort(x, descending=largest).
    Stricter than torch.topk, which leaves the choice among ties open: elements that tie with the k-th key are taken by
    lowest flat index and ties come out in ascending index order. float32 zeros and NaNs come out canonical (+0.0, bits
    0x7fffffff); NaNs are the largest. sorted=False gives the same k elements in ascending index order. 0 <= k <=
    x.numel(), a Python int. Does not synchronise; scan_check() reports a look-back that gave up. method: "select" (the
    radix-select kernels), "sort" (sort and slice) or None: sort and slice when sorted and k > TOPK_SORT_FRACTION *
    numel (0.75: on an MI355X at 2^28 uniform keys select is level there, f32 9.88 against 10.07 ms, and slower at 7/8
    numel, 11.14 against 10.09 ms), select otherwise. At 2^28 keys select is 4.1x-13.4x faster than torch.topk for k <=
    2^24 (f32 k = 1024: 1.53 against 9.72 ms) and 1.26x-2.0x at numel / 2; method="select" with sorted=True on float32
    is slower than torch.topk from k = 7/8 numel (11.14 against 10.86 ms; 12.72 against 11.03 ms at k = numel), where
    the default rule takes the sort route (10.09 ms). dim=int: the top-k of every row along dim, shape of x with dim
    replaced by k, int32 positions along dim; method is for dim=None, route for dim=int (the row-wise section below)."""
    if dim is not None:
        if method is not None:
            raise ValueError("topk: method is for dim=None; with dim use route")
        return _row_topk(x, k, largest, sorted, dim, route)
    _no_route(route)
    _check_topk(x, k, 0, "topk")
    if method not in _TOPK_METHODS:
        raise ValueError(f"topk: method must be one of {_TOPK_METHODS}, got {method!r}")
    largest, n = bool(largest), x.numel()
    if not x.is_cuda:
        xf = x.reshape(-1)
        order = torch.sort(xf, stable=True, descending=largest).indices[:k]
        if not sorted:
            order = torch.sort(order).values
        return _canonical_f32(xf[order]), order.int()
    if method is None:
        method = "sort" if sorted and k > TOPK_SORT_FRACTION * n else "select"
    if method == "select":
        return tuple(ops().topk(x, k, largest, bool(sorted)))
    v, i = (t[:k] for t in ops().sort_index(x, largest, 0, 32, True))
    if not sorted and k > 1:
        i, v = ops().sort_pairs(i, v, False, 0, 32)  # back to index order: indices are distinct, the values ride along
    return v, i


def kth_value(x: torch.Tensor, k: int, largest: bool = False, dim: int | None = None) -> torch.Tensor:
    """The k-th smallest (largest=True: k-th largest) element of x.flatten() as a 0-d tensor on x's device: 1-based
    like torch.kthvalue, equal to sort_keys(x, descending=largest)[k - 1] (float32 canonical). On the GPU the
    threshold of the radix-select passes alone: four read passes, nothing moved, no host synchronisation. dim=int: the
    k-th value of every row along dim, shape of x without dim (the row-wise section below)."""
    if dim is not None:
        return _row_kth(x, k, largest, dim)
    _check_topk(x, k, 1, "kth_value")
    if x.is_cuda:
        return ops().kth_value(x, k, bool(largest))
    xf = x.reshape(-1)
    return _canonical_f32(xf[torch.sort(xf, stable=True, descending=bool(largest)).indices[k - 1:k]]).reshape(())


# ---------------------------------------------------------------- row-wise sort / top-k / k-th value (dim=)
# sort_keys, sort, argsort, sort_by_key, topk and kth_value with dim=int work on every row along dim on its own, with
# torch's output shapes, and are DEFINED by the 1-D ops above: every row's result equals the 1-D op applied to that row,
# bit for bit (same key order, stable, float32 keys canonical, payloads moved as bits). Indices are int32 positions
# along dim. A dim that is not the last is moved last and made contiguous, and the result is moved back, as torch
# does. On the GPU rows of up to ROWSORT_MAX_COLS keys are sorted inside one wave or one block per row
# (csrc/kernels/rowsort.hip; no counterpart in the reference programs): no workspace, no look-back, nothing that could
# time out, so scan_check() has nothing to report for them. Nothing synchronises with the host.
#  * route (tests and the lab) forces a GPU route and raises ValueError when it cannot take the shape; it is validated
#    on CPU tensors too, which otherwise ignore it. Sort routes: "wave" (one wave per row, cols <=
#    ROWSORT_WAVE_MAX_COLS), "block" (one 512-thread block per row, cols <= ROWSORT_MAX_COLS), "loop" (the 1-D sort per
#    row) and "global" (one 1-D stable index sort of all keys, then a stable sort by row id with bits = ceil(log2 rows):
#    any row length at about twice a flat sort). Top-k routes: "sortkeep" (the row sort storing only the first k
#    columns, cols <= ROWSORT_MAX_COLS), "select" (one block per row: four histogram passes and one ordered sweep, then
#    the row sort of the [rows, k] survivors) and "loop" (the 1-D topk per row). kth_value is the select kernel's
#    histogram passes alone.
#  * route=None picks by the constants below, each set from the lab's A/B of the two routes it separates on one MI355X
#    (scripts/rowsort_lab.py, profiles/r16_rowsort/README.md; float32, median ms of 5 interleaved runs):
#    - ROWSORT_WAVE_COLS: 2^24 keys, keys + indices: wave against block 0.152 / 0.203 at cols = 512, 0.184 / 0.167 at
#      1024 (keys alone 0.147 / 0.197 and 0.157 / 0.160); wave is 2.2x-5.4x faster from 256 down to 32.
#    - ROWSORT_LOOP_MIN_COLS: the border is in cols, not in rows: the loop pays launches per row, "global" pays the
#      row-id passes per key. Loop against global, keys + indices, rows = 2 / 8: 0.523 / 0.435 and 2.096 / 0.669 at
#      cols = 2^20; 0.632 / 0.663 and 2.524 / 2.230 at 2^22; 0.833 / 1.122 and 3.362 / 4.335 at 2^23. At 2^22 the loop
#      wins three of the four measured cases (keys alone 0.448 / 0.525 and 1.745 / 1.840) and loses [8, 2^22] with
#      indices by 12%; at 32768-key rows "global" wins from two rows (0.282 / 0.228) to 64 (9.306 / 0.474). One row is
#      the loop: the same work.
#    - ROW_TOPK_SORT_FRACTION: select against sortkeep at [8192, 2048]: 0.136 / 0.143 at k = cols / 8, 0.152 / 0.143 at
#      cols / 4, 0.190 / 0.145 at cols / 2; at [1024, 16384]: 0.159 / 0.238 at cols / 4, 0.246 / 0.244 at cols / 2,
#      0.360 / 0.245 at 3/4 cols. k = cols / 4 itself is select: 6% slower than sortkeep at cols = 2048, 1.5x faster at
#      16384.
#    - ROW_TOPK_LOOP_COLS_PER_ROW: the select kernel puts one block on a row and takes about 3.1 ns per key of a row
#      whatever the number of rows (up to the CUs); the loop takes about 0.12 ms per row. Select against loop, k = 64:
#      one row 0.097 / 0.123 at cols = 32768, 0.336 / 0.125 at 131072; eight rows 0.344 / 0.925 at 131072 (16384 per
#      row), 1.308 / 1.026 at 524288 (65536 per row).
#  * Measured against torch on one MI355X (profiles/r16_rowsort/README.md): sort 2.6x-3.2x faster than torch.sort(dim=-1,
#    stable=True) for rows of 32 to 16384 keys with indices (1.9x at [16384, 4096]); top-k 1.5x-2.1x faster than
#    torch.topk at [4096, 4096] and [65536, 512], 1.02x-1.10x at [512, 131072]. SLOWER than torch: the "global" sort
#    route ([1024, 32768]: 2.29 ms keys, 3.17 ms with indices against 1.64 ms, 0.52x-0.77x), float32 sort with indices
#    of [8, 2^24] by the loop (5.92 against 4.43 ms, 0.75x; keys alone 1.06x, int32 1.07x-1.65x), top-k of one row of
#    131072 keys for k >= 8 (0.13 against 0.07 ms, 0.53x-0.57x; k = 1 1.2x) and of [64, 32768] (0.095-0.118 against
#    0.089-0.110 ms on the minimum of 5, 0.85x-0.95x).
ROWSORT_MAX_COLS = 16384       # csrc/include/pcmx_hip.h PCMX_ROWSORT_MAX_COLS: sort.hip's tile, one block's LDS
ROWSORT_WAVE_MAX_COLS = 1024   # PCMX_ROWSORT_WAVE_MAX_COLS: 16 keys per lane
ROWSORT_WAVE_COLS = 512        # W: rows up to here take the wave kernel, longer ones the block kernel
ROWSORT_LOOP_MIN_COLS = 1 << 22  # rows longer than ROWSORT_MAX_COLS: "loop" from this many keys per row (or one row)
ROW_TOPK_SORT_FRACTION = 0.25  # cols <= ROWSORT_MAX_COLS: "sortkeep" when k > this * cols, "select" otherwise
ROW_TOPK_LOOP_COLS_PER_ROW = 65536  # "loop" (the device-wide topk per row) when cols >= this * rows
_ROW_SORT_ROUTES = (None, "wave", "block", "loop", "global")
_ROW_TOPK_ROUTES = (None, "sortkeep", "select", "loop")
_MODE_KEYS, _MODE_PAIRS, _MODE_INDEX = 0, 1, 2          # PCMX_SORT_*
_ROUTE_FLAG = {"wave": 0x100, "block": 0x200}           # PCMX_ROWSORT_WAVE / PCMX_ROWSORT_BLOCK


def _no_route(route) -> None:
    if route is not None:
        raise ValueError("route selects a row-wise kernel: it needs dim")


def _rows_of(x: torch.Tensor, dim, name: str):
    """(x as contiguous [rows, cols] with dim last, the dim-last shape, dim normalised)."""
    if isinstance(dim, bool) or not isinstance(dim, int):
        raise TypeError(f"{name}: dim must be an int or None, got {type(dim).__name__}")
    if x.dim() < 1 or not -x.dim() <= dim < x.dim():
        raise IndexError(f"{name}: dim {dim} is out of range for a tensor with {x.dim()} dimensions")
    d = dim % x.dim()
    xm = x.movedim(d, -1)
    cols = xm.shape[-1]
    rows = xm.numel() // cols if cols else int(torch.Size(xm.shape[:-1]).numel())
    return xm.reshape(rows, cols).contiguous(), tuple(xm.shape), d


def _rows_back(t: torch.Tensor, shape, d: int) -> torch.Tensor:
    return t.reshape(*shape[:-1], t.shape[-1]).movedim(-1, d)


def _sort_route(route, rows: int, cols: int, name: str) -> str:
    if route not in _ROW_SORT_ROUTES:
        raise ValueError(f"{name}: route must be one of {_ROW_SORT_ROUTES}, got {route!r}")
    if route is None:
        if cols <= ROWSORT_WAVE_COLS:
            return "wave"
        if cols <= ROWSORT_MAX_COLS:
            return "block"
        return "loop" if rows == 1 or cols >= ROWSORT_LOOP_MIN_COLS else "global"
    limit = {"wave": ROWSORT_WAVE_MAX_COLS, "block": ROWSORT_MAX_COLS}.get(route)
    if limit is not None and cols > limit:
        raise ValueError(f"{name}: route {route!r} takes rows of at most {limit} keys, got {cols}")
    return route


def _gather_bits(src2: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """src2[r, order[r, j]] moved as bits (a float gather would be free to quieten a signalling NaN payload)."""
    return torch.gather(src2.view(torch.int32), 1, order.long()).view(src2.dtype)


def _row_sort_global(k2: torch.Tensor, v2, descending: bool, nbits: int, want_keys: bool, want_pos: bool):
    """(sorted keys, int32 positions, sorted values), each None when not wanted, of every row of k2 with the device-wide
    kernels: one stable index sort of all keys, then a stable pair sort by row id per wanted stream: keys of one row
    stay in their sorted order."""
    rows, cols = k2.shape
    want_pos = want_pos or v2 is not None
    ks, fi = ops().sort_index(k2.reshape(-1), descending, 0, nbits, True)
    if rows > 1:
        rid = torch.div(fi, cols, rounding_mode="floor")
        rbits = (rows - 1).bit_length()
        if want_keys:
            ks = ops().sort_pairs(rid, ks, False, 0, rbits)[1]
        if want_pos:
            fi = ops().sort_pairs(rid, fi, False, 0, rbits)[1]
    pos = None
    if want_pos:
        pos = fi.view(rows, cols) - (torch.arange(rows, device=k2.device, dtype=torch.int32) * cols)[:, None]
    vs = None if v2 is None else _gather_bits(v2, pos)
    return (ks.view(rows, cols) if want_keys else None), pos, vs


def _row_sort_gpu(k2: torch.Tensor, v2, mode: str, keep: int, descending: bool, nbits: int, route: str):
    """(keys or None, payload or None), each [rows, keep], of the row sort of k2 on the GPU by `route`."""
    rows, cols = k2.shape
    want_keys = mode != "argsort"
    if route in _ROUTE_FLAG:
        code = {"keys": _MODE_KEYS, "pairs": _MODE_PAIRS}.get(mode, _MODE_INDEX) | _ROUTE_FLAG[route]
        ko, vo = ops().row_sort(k2, v2, keep, code, descending, 0, nbits, want_keys)
        return (ko if want_keys else None), (None if mode == "keys" else vo)
    if route == "global":
        ks, pos, vs = _row_sort_global(k2, v2, descending, nbits, want_keys, mode not in ("keys", "pairs"))
    else:  # "loop": the device-wide sort, row by row
        ks = pos = vs = None
        if mode == "keys":
            ks = torch.stack([ops().sort_keys(r, descending, 0, nbits) for r in k2])
        elif mode == "pairs":
            ks, vs = (torch.stack(t) for t in zip(*(ops().sort_pairs(r, v, descending, 0, nbits) for r, v in zip(k2, v2))))
        else:
            ks, pos = (torch.stack(t) for t in zip(*(ops().sort_index(r, descending, 0, nbits, True) for r in k2)))
    payload = vs if mode == "pairs" else pos
    return (ks[:, :keep] if want_keys else None), (None if mode == "keys" else payload[:, :keep])


def _row_sort(keys: torch.Tensor, values, mode: str, descending, bits, dim, route):
    """The row-wise form of sort_keys / sort / argsort / sort_by_key: (keys or None, payload or None) in x's shape."""
    nbits = _check_sort_keys(keys, bits, "keys" if mode == "pairs" else "x")
    descending = bool(descending)
    if mode == "pairs":
        if values.dtype not in (torch.float32, torch.int32):
            raise TypeError(f"values must be float32 or int32, got {values.dtype}")
        if values.shape != keys.shape:
            raise ValueError(f"with dim the values must have the keys' shape {tuple(keys.shape)}, got {tuple(values.shape)}")
        if values.device != keys.device:
            raise ValueError(f"values are on {values.device}, the keys on {keys.device}")
    k2, shape, d = _rows_of(keys, dim, "sort")
    v2 = _rows_of(values, dim, "sort")[0] if mode == "pairs" else None
    rows, cols = k2.shape
    route = _sort_route(route, rows, cols, "sort")
    if k2.numel() == 0:
        ko, po = k2.clone(), (v2.clone() if mode == "pairs" else k2.new_empty(k2.shape, dtype=torch.int32))
    elif keys.is_cuda:
        ko, po = _row_sort_gpu(k2, v2, mode, cols, descending, nbits, route)
    else:
        key = k2 if nbits == 32 else k2.long() & ((1 << nbits) - 1)
        order = torch.sort(key, dim=-1, stable=True, descending=descending).indices
        ko = _canonical_f32(_gather_bits(k2, order))
        po = _gather_bits(v2, order) if mode == "pairs" else order.int()
    return (None if mode == "argsort" else _rows_back(ko, shape, d)), (None if mode == "keys" else _rows_back(po, shape, d))


def _check_row_k(x: torch.Tensor, k, k_min: int, cols: int, name: str) -> None:
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"{name}: k must be an int, got {type(k).__name__}")
    if not k_min <= k <= cols:
        raise ValueError(f"{name}: k must be in {k_min}..{cols} (the size of dim), got {k}")


def _topk_route(route, rows: int, cols: int, k: int, name: str) -> str:
    if route not in _ROW_TOPK_ROUTES:
        raise ValueError(f"{name}: route must be one of {_ROW_TOPK_ROUTES}, got {route!r}")
    if route is None:
        if cols >= ROW_TOPK_LOOP_COLS_PER_ROW * rows:
            return "loop"
        return "sortkeep" if cols <= ROWSORT_MAX_COLS and k > ROW_TOPK_SORT_FRACTION * cols else "select"
    if route == "sortkeep" and cols > ROWSORT_MAX_COLS:
        raise ValueError(f"{name}: route 'sortkeep' takes rows of at most {ROWSORT_MAX_COLS} keys, got {cols}")
    return route


def _small_sort_route(cols: int) -> str:
    return "wave" if cols <= ROWSORT_WAVE_COLS else ("block" if cols <= ROWSORT_MAX_COLS else "global")


def _row_topk(x: torch.Tensor, k, largest, sorted, dim, route):
    _check_topk(x, 0, 0, "topk")  # dtype and the element limit; k is checked against the size of dim
    largest = bool(largest)
    x2, shape, d = _rows_of(x, dim, "topk")
    rows, cols = x2.shape
    _check_row_k(x, k, 0, cols, "topk")
    route = _topk_route(route, rows, cols, k, "topk")
    if rows == 0 or k == 0:
        v, i = x2.new_empty((rows, k)), x2.new_empty((rows, k), dtype=torch.int32)
    elif not x.is_cuda:
        order = torch.sort(x2, dim=-1, stable=True, descending=largest).indices[:, :k]
        if not sorted:
            order = torch.sort(order, dim=-1).values
        v, i = _canonical_f32(_gather_bits(x2, order)), order.int()
    elif route == "loop":
        v, i = (torch.stack(t) for t in zip(*(tuple(ops().topk(r, k, largest, bool(sorted))) for r in x2)))
    elif route == "sortkeep":
        v, i = _row_sort_gpu(x2, None, "index", k, largest, 32, _small_sort_route(cols))
        if not sorted and k > 1:  # back to position order: positions are distinct, the values ride along
            i, v = _row_sort_gpu(i, v, "pairs", k, False, 32, _small_sort_route(k))
    else:
        v, i = ops().row_topk(x2, k, largest)
        if sorted and k > 1:  # canonical values transform to the same keys again and the sort is stable
            v, i = _row_sort_gpu(v, i, "pairs", k, largest, 32, _small_sort_route(k))
    return _rows_back(v, shape, d), _rows_back(i, shape, d)


def _row_kth(x: torch.Tensor, k, largest, dim):
    _check_topk(x, 0, 0, "kth_value")  # dtype and the element limit; k is checked against the size of dim
    x2, shape, d = _rows_of(x, dim, "kth_value")
    rows, cols = x2.shape
    _check_row_k(x, k, 1, cols, "kth_value")
    if rows == 0:
        out = x2.new_empty((0,))
    elif x.is_cuda:
        out = ops().row_kth(x2, k, bool(largest))
    else:
        order = torch.sort(x2, dim=-1, stable=True, descending=bool(largest)).indices[:, k - 1:k]
        out = _canonical_f32(_gather_bits(x2, order))
    return out.reshape(shape[:-1])


# ---------------------------------------------------------------- run-length encode / reduce by key / unique
# Collapse runs of equal neighbouring keys of the flattened input and reduce a value stream per run. On the GPU one
# pass on the scan's decoupled look-back carrying the exact integer count of run heads, a segmented reduction inside
# each 32768-key tile, and a small second kernel that joins the runs crossing tile borders in a fixed order
# (csrc/kernels/segreduce.hip); no counterpart in the reference programs. The by-key members of the scan / select /
# sort family: unique and sum_by_key are "sort, then collapse".
#  * KEY RULE: keys (float32 or int32) are compared as 32-bit PATTERNS. -0.0 and +0.0 are different keys; two NaNs with
#    the same bits are the same key, NaNs with different payloads are different keys. This is torch.unique_consecutive
#    on the int32 view, not on the float view. sort_keys output is canonical (one zero, one NaN), so sorted float keys
#    collapse as values.
#  * A run is a maximal block of equal neighbours; element 0 starts one; an empty input has 0 runs.
#  * run_length_encode / reduce_by_key follow compact's (out, count) contract: per-run outputs have room for every
#    element, only [:num_runs] is written, num_runs is a 0-d int64 tensor on the input's device, nothing synchronises;
#    a look-back that gave up is reported by scan_check(). Run keys keep their exact bits; counts and starts are int32.
#  * int32 sums wrap mod 2^32 and int32 results are exact. A float32 result depends only on the input, never on
#    timing: the same call gives the same bits (fixed association order, no float atomics).
#  * Measured against torch on one MI355X at 2^28 int32 keys, mean run length 1 to 10^5 and all equal
#    (profiles/r9_segreduce/README.md): run_length_encode 1.01-1.33x faster than torch.unique_consecutive with counts,
#    reduce_by_key sums 3.4x-108x faster than unique_consecutive + index_add_. unique(return_counts=True) is SLOWER
#    than torch.unique: 6.22-7.39 ms against 6.15-6.21 ms (0.83-0.99x), level only when all keys are equal.
def _check_seg_keys(keys: torch.Tensor, name: str = "keys") -> None:
    if keys.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"{name} must be float32 or int32, got {keys.dtype}")
    if keys.numel() >= 1 << 31:
        raise ValueError(f"{name} has {keys.numel()} elements; run offsets are int32 (fewer than 2^31)")


def _host_runs(keys: torch.Tensor):
    """(run key bits, int64 run index of every element, int64 run lengths) of flat keys compared as bit patterns."""
    bits = keys.reshape(-1).contiguous().view(torch.int32)
    return torch.unique_consecutive(bits, return_inverse=True, return_counts=True)


def run_length_encode(keys: torch.Tensor, starts: bool = False, out_keys: torch.Tensor | None = None,
                      out_counts: torch.Tensor | None = None, out_starts: torch.Tensor | None = None):
    """(run_keys, counts, num_runs), or (run_keys, counts, starts, num_runs) with starts=True: the key, the int32
    length and the int32 offset of the first element of every run of equal neighbouring keys of keys.flatten(). Keys
    (float32 or int32) are compared as bit patterns: -0.0 != +0.0, NaNs are equal only with equal bits. num_runs is a
    0-d int64 tensor on the keys' device; the per-run tensors (or the optional caller tensors out_*, 1-D with room for
    keys.numel() entries) are written only in [:num_runs]. Does not synchronise."""
    _check_seg_keys(keys)
    n = keys.numel()
    _check_out(out_keys, keys.dtype, n, keys)
    _check_out(out_counts, torch.int32, n, keys)
    if starts:
        _check_out(out_starts, torch.int32, n, keys)
    if keys.is_cuda:
        rk, rc, rs, num = ops().run_length_encode(keys, bool(starts), out_keys, out_counts, out_starts if starts else None)
        return (rk, rc, rs, num) if starts else (rk, rc, num)
    kbits, _, counts = _host_runs(keys)
    rk, num = _host_result(kbits.view(keys.dtype), n, out_keys)
    rc, _ = _host_result(counts.int(), n, out_counts)
    if not starts:
        return rk, rc, num
    rs, _ = _host_result((torch.cumsum(counts, 0) - counts).int(), n, out_starts)
    return rk, rc, rs, num


def _check_seg_values(keys: torch.Tensor, values: torch.Tensor) -> None:
    if values.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"values must be float32 or int32, got {values.dtype}")
    if values.numel() != keys.numel():
        raise ValueError(f"{values.numel()} values for {keys.numel()} keys")
    if values.device != keys.device:
        raise ValueError(f"values are on {values.device}, the keys on {keys.device}")


def reduce_by_key(keys: torch.Tensor, values: torch.Tensor, op: str = "sum", out_keys: torch.Tensor | None = None,
                  out: torch.Tensor | None = None):
    """(run_keys, aggregates, num_runs): values (float32 or int32, same numel) reduced with op (sum, min, max) over
    every run of equal neighbouring keys of keys.flatten(); keys compared as bit patterns (-0.0 != +0.0, NaNs equal only
    with equal bits). int32 sums wrap mod 2^32; int32 results are exact. A float32 sum uses a fixed association order
    (not input order): the same input gives the same bits on every call, whatever the timing. float32 min / max
    propagate a NaN value (like torch's amin / amax; which NaN's payload comes out is unspecified). Outputs follow
    run_length_encode's contract; does not synchronise."""
    _check_seg_keys(keys)
    if op not in OP_CODES:
        raise ValueError(f"op must be one of {sorted(OP_CODES)}, got {op!r}")
    _check_seg_values(keys, values)
    n = keys.numel()
    _check_out(out_keys, keys.dtype, n, keys)
    _check_out(out, values.dtype, n, keys)
    if keys.is_cuda:
        return tuple(ops().reduce_by_key(keys, values, OP_CODES[op], out_keys, out))
    kbits, inv, _ = _host_runs(keys)
    k, vf = kbits.numel(), values.reshape(-1)
    if op == "sum" and values.dtype == torch.int32:
        s = torch.zeros(k, dtype=torch.int64).index_add_(0, inv, vf.long())
        agg = (((s + (1 << 31)) % (1 << 32)) - (1 << 31)).int()
    elif op == "sum":
        agg = torch.zeros(k, dtype=torch.float32).index_add_(0, inv, vf)
    else:
        agg = torch.zeros(k, dtype=values.dtype).scatter_reduce_(0, inv, vf, "amin" if op == "min" else "amax",
                                                                 include_self=False)
    rk, num = _host_result(kbits.view(keys.dtype), n, out_keys)
    ra, _ = _host_result(agg, n, out)
    return rk, ra, num


def unique_consecutive(keys: torch.Tensor, return_counts: bool = False):
    """The key of every run of equal neighbouring keys of keys.flatten() at exact size (one host sync for the count),
    with the int32 run lengths when return_counts. Keys are compared as bit patterns: torch.unique_consecutive on the
    int32 view (-0.0 and +0.0 stay apart, NaNs collapse only with equal bits)."""
    rk, rc, num = run_length_encode(keys)
    k = int(num.item())
    return (rk[:k], rc[:k]) if return_counts else rk[:k]


def unique(x: torch.Tensor, return_counts: bool = False):
    """The sorted distinct values of x.flatten() (float32 or int32, at most SORT_MAX_N elements) at exact size, with
    their int32 counts when return_counts: sort_keys, then run_length_encode (one host sync). For float32 the two
    zeros are ONE value (+0.0) and all NaNs are ONE value (bits 0x7fffffff, last), because sort_keys output is
    canonical; torch.unique keeps every NaN as a value of its own. On an MI355X this is slower than torch.unique
    (2^28 int32 keys: 6.22-7.39 ms against 6.15-6.21 ms; the sort dominates)."""
    rk, rc, num = run_length_encode(sort_keys(x))
    k = int(num.item())
    return (rk[:k], rc[:k]) if return_counts else rk[:k]


def sum_by_key(keys: torch.Tensor, values: torch.Tensor):
    """(unique_keys, sums) at exact size: the unsorted group-by sum, sort_by_key followed by reduce_by_key (one host
    sync). Keys as in unique (float32 zeros and NaNs are one group each). The sort is stable, so the values of equal
    keys meet the reduction in input order; a float32 sum is then reduce_by_key's fixed association over that
    sequence (deterministic, not a left-to-right sum). int32 sums wrap."""
    _check_seg_values(keys, values)
    ks, vs = sort_by_key(keys, values)
    rk, ra, num = reduce_by_key(ks, vs, "sum")
    k = int(num.item())
    return rk[:k], ra[:k]


# ---------------------------------------------------------------- scan by key (segmented prefix scan)
# The running aggregate INSIDE every run, where reduce_by_key gives one aggregate per run: out[i] = op(values[s..i])
# (inclusive) or op(values[s..i-1]) (exclusive), s the first element of i's run. The runs are those of the KEY RULE
# above (scan_by_key, run_positions) or start at the non-zero entries of a bool / uint8 tensor (segmented_scan);
# element 0 always starts one. On the GPU three launches with no waiting between blocks (csrc/kernels/scanbykey.hip):
# every 32768-element tile is scanned and written with the identity as carry-in, one block scans the tile summaries in
# a fixed order, and the carry is combined into the lead of every tile that continues a run.
#  * The result has the values' dtype and shape; `out` (contiguous, same numel and dtype) may be the values tensor
#    itself (in place); keys or heads that overlap out are cloned first. Nothing synchronises; n == 0 launches nothing.
#  * Exclusive mode gives the first element of every run the identity: +0.0 / 0 for sum, +inf / INT32_MAX for min,
#    -inf / INT32_MIN for max.
#  * int32 sums wrap mod 2^32 and int32 results are exact; float32 min / max are exact and hand on a NaN to the end
#    of that run only; a float32 sum uses a fixed association order (not input order): the same input gives the same
#    bits on every call. A NaN or inf in one run never reaches another run.
#  * Measured against the torch composition (unique_consecutive + cumsum minus the gathered per-run base) on one
#    MI355X at 2^28 int32 keys, mean run length 1 to 10^5 and all equal (profiles/r11_scanbykey/README.md): sums
#    14.2x-4.7x faster (0.61-1.02 ms), run_positions 16.9x-5.7x (0.50-0.92 ms); the slow end is all keys equal, where
#    the lead of every tile is the whole tile and the output is written twice.
_SCAN_IDENTITY = {"sum": (0.0, 0), "min": (float("inf"), 2**31 - 1), "max": (float("-inf"), -2**31)}
_SCAN_COMBINE = {"sum": torch.add, "min": torch.minimum, "max": torch.maximum}


def _check_scan_out(out: torch.Tensor | None, values: torch.Tensor) -> None:
    if out is None:
        return
    if out.dtype != values.dtype:
        raise TypeError(f"out must be {values.dtype}, got {out.dtype}")
    if out.device != values.device:
        raise ValueError(f"out is on {out.device}, the values on {values.device}")
    if not out.is_contiguous() or out.numel() != values.numel():
        raise ValueError(f"out must be contiguous with the values' {values.numel()} elements, got shape "
                         f"{tuple(out.shape)}")


def _host_segmented_scan(head: torch.Tensor, values: torch.Tensor, op: str, exclusive: bool,
                         out: torch.Tensor | None) -> torch.Tensor:
    """The CPU path of the three ops: head is a flat bool tensor with head[0] set. Integer sums through an int64 cumsum
    (exact, wrapped); everything else by doubling steps inside the runs (x[i] = op(x[i - d], x[i]) while i - d is in
    i's run, d = 1, 2, 4, ...), which keeps a NaN or inf inside its run and is a fixed order for float32 sums."""
    v = values.reshape(-1)
    n = v.numel()
    if n == 0:
        return out if out is not None else torch.empty_like(values)
    pos = torch.arange(n) - torch.cummax(torch.where(head, torch.arange(n), 0), 0).values  # index inside the run
    ident = _SCAN_IDENTITY[op][0 if v.dtype == torch.float32 else 1]
    if op == "sum" and v.dtype == torch.int32:
        c = torch.cumsum(v.long(), 0)
        incl = c - (c - v)[torch.arange(n) - pos]
        incl = (((incl + (1 << 31)) % (1 << 32)) - (1 << 31)).int()
    else:
        incl, d, longest = v.clone(), 1, int(pos.max())
        while d <= longest:
            joined = _SCAN_COMBINE[op](incl[:-d], incl[d:])
            incl[d:] = torch.where(pos[d:] >= d, joined, incl[d:])
            d *= 2
    res = incl
    if exclusive:
        res = torch.full_like(incl, ident)
        res[1:] = torch.where(head[1:], res[1:], incl[:-1])
    if out is None:
        return res.reshape(values.shape)
    out.view(-1).copy_(res)
    return out


def _check_scan_op(op: str) -> None:
    if op not in OP_CODES:
        raise ValueError(f"op must be one of {sorted(OP_CODES)}, got {op!r}")


def _key_heads(keys: torch.Tensor) -> torch.Tensor:
    bits = keys.reshape(-1).contiguous().view(torch.int32)
    head = torch.ones(bits.numel(), dtype=torch.bool)
    head[1:] = bits[1:] != bits[:-1]
    return head


def scan_by_key(keys: torch.Tensor, values: torch.Tensor, op: str = "sum", exclusive: bool = False,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """The running op (sum, min, max) of values (float32 or int32) inside every run of equal neighbouring keys of
    keys.flatten() (float32 or int32, same numel, compared as bit patterns: -0.0 != +0.0, NaNs equal only with equal
    bits), with the values' dtype and shape: out[i] = op(values[s..i]), or op(values[s..i-1]) when exclusive (the first
    element of a run then gets the identity: 0, +inf / INT32_MAX, -inf / INT32_MIN), s the first element of i's run.
    int32 sums wrap mod 2^32; int32 results are exact; float32 min / max are exact and hand on a NaN to the end of its
    run only; a float32 sum uses a fixed association order (not input order): the same input gives the same bits on
    every call. out (contiguous, same dtype and numel) may be values itself. Does not synchronise."""
    _check_seg_keys(keys)
    _check_scan_op(op)
    _check_seg_values(keys, values)
    _check_scan_out(out, values)
    if keys.is_cuda:
        return ops().scan_by_key(keys, values, OP_CODES[op], bool(exclusive), out)
    return _host_segmented_scan(_key_heads(keys), values, op, bool(exclusive), out)


def segmented_scan(values: torch.Tensor, heads: torch.Tensor, op: str = "sum", exclusive: bool = False,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """scan_by_key with the runs given by flags: a non-zero entry of heads.flatten() (bool or uint8, same numel) starts
    a run, and element 0 starts one whatever heads[0] says. segmented_scan(v, h) equals scan_by_key(k, v) when h[i] =
    (bits of k[i] != bits of k[i-1])."""
    if values.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"values must be float32 or int32, got {values.dtype}")
    if values.numel() >= 1 << 31:
        raise ValueError(f"values have {values.numel()} elements; tile offsets are int32 (fewer than 2^31)")
    if heads.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"heads must be bool or uint8, got {heads.dtype}")
    if heads.numel() != values.numel():
        raise ValueError(f"{heads.numel()} heads for {values.numel()} values")
    if heads.device != values.device:
        raise ValueError(f"heads are on {heads.device}, the values on {values.device}")
    _check_scan_op(op)
    _check_scan_out(out, values)
    if values.is_cuda:
        return ops().segmented_scan(values, heads, OP_CODES[op], bool(exclusive), out)
    head = heads.reshape(-1) != 0
    if head.numel():
        head[0] = True
    return _host_segmented_scan(head, values, op, bool(exclusive), out)


def run_positions(keys: torch.Tensor) -> torch.Tensor:
    """int32 index of every element inside its run of equal neighbouring keys (0, 1, 2, ... from each run's first
    element), with the keys' shape: the exclusive sum-scan by key of the constant 1; no value stream is read. Keys as
    in scan_by_key. Does not synchronise."""
    _check_seg_keys(keys)
    if keys.is_cuda:
        return ops().run_positions(keys)
    n = keys.numel()
    head = _key_heads(keys)
    start = torch.cummax(torch.where(head, torch.arange(n), 0), 0).values if n else torch.arange(0)
    return (torch.arange(n) - start).int().reshape(keys.shape)


# ---------------------------------------------------------------- reduce / scan along a dimension (dim=)
# reduce(x, op, dim) and scan(x, dim=dim, op=op) work on every row along dim on its own: torch.sum / amin / amax (dim)
# and torch.cumsum / cummin / cummax (dim).values, float32 or int32, with torch's shapes. The contiguous tensor is
# viewed as [outer, n, inner] with the work along n and read where it lies for every dim (csrc/kernels/axis.hip; no
# counterpart in the reference programs); a non-contiguous input is gathered first. No look-back, no block waits for
# another, nothing can time out, so scan_check() has nothing of these calls to report. Nothing synchronises.
#  * int32 sums wrap mod 2^32 and int32 results are exact; float32 min / max are exact where a row holds no NaN; a row
#    (for scan: a prefix) that holds a NaN gives a NaN (which NaN is unspecified, as is the sign of a zero min / max);
#    a float32 sum uses a fixed association order (axis.hip's header) that depends on size(dim), the inner extent and
#    the route only: the same row gives the same bits wherever it stands. Rows never mix. Fewer than 2^31 elements.
#  * A 1-D tensor with dim=0 is one long row: the int32 and min / max scans of a flat tensor. reduce(x) and scan(x)
#    without dim stay the flat kernels (the look-back scan, the two-pass reduce).
#  * route (tests and the lab) forces a GPU route and raises ValueError when it cannot take the shape; it is validated
#    on CPU tensors too, which otherwise ignore it. inner == 1: "group" (G lanes per row, n <= AXIS_GROUP_MAX_N),
#    "block" (one block per row, n <= AXIS_BLOCK_MAX_N), "split" (chunks of `chunk` elements of a row over blocks, a
#    multiple of 1024, then a fold / carry pass). inner > 1: "column" (a thread walks down 4 adjacent columns),
#    "column_split" (chunks of `chunk` >= AXIS_COLUMN_MIN_CHUNK rows over threads, then a fold / carry pass).
#  * route=None picks by the constants below (_axis_route), each set from the lab's A/B of the two routes it separates
#    on one MI355X (scripts/axis_lab.py, profiles/r17_axis/README.md; float32 sums, median ms of 5 interleaved runs,
#    reduce / scan):
#    - AXIS_GROUP_N, AXIS_GROUP_SCAN_N: 2^24 elements, group against block: 0.017 / 0.152 and 0.029 / 0.146 at n = 128;
#      0.017 / 0.040 and 0.028 / 0.038 at 512; 0.016 / 0.024 and 0.030 / 0.028 at 1024; 0.017 / 0.020 and 0.032 / 0.029 at
#      2048; 0.020 / 0.018 and 0.031 / 0.031 at 4096 (a second run: scans 0.031 / 0.044, 0.036 / 0.032, 0.034 / 0.031,
#      0.036 / 0.031). The reduce keeps group to 2048, the scan to 512: block scans are 7%-12% faster from 1024.
#    - AXIS_SPLIT_MIN_N, AXIS_SPLIT_ROWS: block against split at 1 / 8 / 64 / 256 / 1024 rows: n = 32768 block at every
#      row count (0.010 / 0.013 to 0.027 / 0.031 reduce, 0.025 / 0.030 to 0.056 / 0.083 scan); n = 131072 split up to 256
#      rows (reduce 0.023 / 0.012, 0.037 / 0.021, 0.052 / 0.023, 0.053 / 0.031; scan 0.088 / 0.032 to 0.140 / 0.085) and
#      block at 1024 rows (0.085 / 0.105 and 0.205 / 0.310). 512 lies between the two measured row counts and is itself
#      NOT MEASURED; 65536-element rows are not measured either.
#    - AXIS_BLOCK_MAX_N: at 2^20 elements per row split wins at every measured row count (64 rows 0.378 / 0.058 and
#      0.945 / 0.160); [1024, 2^20] is not measured: the border above 256 rows is a guess.
#    - AXIS_SPLIT_CHUNK: 8192 / 32768 / 131072 at [8, 2^24] 0.108 / 0.105 / 0.088 and 0.293 / 0.308 / 0.287, at [1, 2^26]
#      0.060 / 0.056 / 0.063 and 0.160 / 0.163 / 0.216, at [64, 2^20] 0.057 / 0.058 / 0.068 and 0.155 / 0.161 / 0.222: no
#      chunk wins everywhere, 32768 is never more than 7% (reduce: 19%) behind the best.
#    - AXIS_COLUMN_MIN_BLOCKS (reduce), column against column_split along dim 0: [1024, 16384] (64 blocks) 0.094 / 0.026,
#      [1024, 65536] and [64, 1024, 1024] along dim 1 (256 blocks) 0.105 / 0.052 and 0.110 / 0.051, [256, 262144] (1024
#      blocks) 0.044 / 0.044. Level at 1024, twice as slow at 256; 512 is NOT MEASURED.
#    - AXIS_COLUMN_MIN_UNITS (scan): [1024, 65536] (16384 threads) 0.541 / 0.237, [256, 262144] (65536) 0.179 / 0.176.
#    - AXIS_COLUMN_SPLIT_MIN_N is a guess and NOT MEASURED ([32, 262144]: 0.011 / 0.012 and 0.029 / 0.030, level).
#  * Measured against torch on one MI355X (profiles/r17_axis/README.md; float32, torch.sum / amax / cumsum /
#    cummax(dim)): along the last dim [2^20, 32] 5.3x / 5.5x / 53x / 59x, [2^16, 512] 1.2x-2.6x, [1024, 32768] 1.3x and
#    6.7x, [8, 2^24] 37x-164x, at 0.79x-1.31x the time of ops.copy_ of the same bytes for rows that fit a group or a
#    block; along dim 0 [4096, 4096] 1.0x / 1.2x / 16x / 17x, [2^20, 64] 1.3x / 1.3x / 1060x, [64, 2^20] 1.0x-1.9x, [64,
#    1024, 1024] along dim 1 1.1x-3.1x; 1.5x-18x faster than movedim().contiguous() and the row route in every cell.
#    SLOWER than torch: sum / amax of [16384, 4096] (0.053 against 0.051 ms, 0.96x-0.97x). A scan on a split route reads
#    the input twice: 1.8x the copy floor. SLOWER than the flat ops on one row of 2^28: reduce 0.206 against ops.reduce
#    0.157 ms, scan 0.625 against ops.scan 0.355 ms (torch 0.274 / 0.708): flat float32 sums keep reduce(x) / scan(x);
#    dim=0 of a flat tensor is for int32 and min / max.
AXIS_GROUP_MAX_N = 4096          # PCMX_AXIS_GROUP_MAX_N: the group kernel's limit when forced
AXIS_GROUP_N = 2048              # PCMX_AXIS_GROUP_N: reduce: rows up to here take group, longer ones block
AXIS_GROUP_SCAN_N = 512          # PCMX_AXIS_GROUP_SCAN_N: scan: the same border
AXIS_BLOCK_MAX_N = 1 << 20       # PCMX_AXIS_BLOCK_MAX_N: longer rows always take split
AXIS_SPLIT_ROWS = 512            # PCMX_AXIS_SPLIT_ROWS: with fewer rows than this ...
AXIS_SPLIT_MIN_N = 1 << 17       # PCMX_AXIS_SPLIT_MIN_N: ... rows from this length take split
AXIS_SPLIT_CHUNK = 32768         # PCMX_AXIS_SPLIT_CHUNK: the default chunk of split
AXIS_COLUMN_MIN_UNITS = 65536    # PCMX_AXIS_COLUMN_MIN_UNITS: scan: column from this many threads (outer * ceil(inner / 4))
AXIS_COLUMN_MIN_BLOCKS = 1024    # PCMX_AXIS_COLUMN_MIN_BLOCKS: reduce: column from this many blocks (outer * 64-quad tiles)
AXIS_COLUMN_SPLIT_MIN_N = 64     # PCMX_AXIS_COLUMN_SPLIT_MIN_N (guess, NOT MEASURED): ... or when n is below this
AXIS_COLUMN_MIN_CHUNK = 16       # PCMX_AXIS_COLUMN_MIN_CHUNK: the smallest chunk of column_split
AXIS_GROUP, AXIS_BLOCK, AXIS_SPLIT, AXIS_COLUMN, AXIS_COLUMN_SPLIT = 1, 2, 3, 4, 5  # PCMX_AXIS_*
_AXIS_ROUTE_CODE = {"group": AXIS_GROUP, "block": AXIS_BLOCK, "split": AXIS_SPLIT, "column": AXIS_COLUMN,
                    "column_split": AXIS_COLUMN_SPLIT}
_AXIS_TILE = 1024                # split chunks are whole tiles of the block kernel


def _axis_route(kind: str, outer: int, n: int, inner: int) -> str:
    """The default route of reduce / scan along a dimension for the [outer, n, inner] view (kind: "reduce" or "scan":
    the column reduce is a block-cooperative kernel, the column scan a thread per 4 columns, so their borders differ)."""
    if kind not in ("reduce", "scan"):
        raise ValueError(f"kind must be 'reduce' or 'scan', got {kind!r}")
    if inner == 1:
        if n <= (AXIS_GROUP_SCAN_N if kind == "scan" else AXIS_GROUP_N):
            return "group"
        if n > AXIS_BLOCK_MAX_N or (outer < AXIS_SPLIT_ROWS and n >= AXIS_SPLIT_MIN_N):
            return "split"
        return "block"
    quads = (inner + 3) // 4
    if kind == "reduce":  # a block is min(64, quads rounded up to a power of two) quads wide (axis.hip: col_lanes)
        fills = outer * -(-quads // min(64, 1 << (quads - 1).bit_length())) >= AXIS_COLUMN_MIN_BLOCKS
    else:
        fills = outer * quads >= AXIS_COLUMN_MIN_UNITS
    return "column" if fills or n < AXIS_COLUMN_SPLIT_MIN_N else "column_split"


def _axis_plan(kind: str, route, chunk, outer: int, n: int, inner: int, name: str):
    """(route code, chunk) for the kernels after validating route and chunk against the shape; 0 = the default."""
    if route is not None and route not in _AXIS_ROUTE_CODE:
        raise ValueError(f"{name}: route must be None or one of {sorted(_AXIS_ROUTE_CODE)}, got {route!r}")
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int)):
        raise TypeError(f"{name}: chunk must be an int or None, got {type(chunk).__name__}")
    resolved = route if route is not None else _axis_route(kind, outer, n, inner)
    if (resolved in ("group", "block", "split")) != (inner == 1):
        raise ValueError(f"{name}: route {route!r} is for {'the last dimension (inner extent 1)' if inner != 1 else 'an inner extent above 1'}, "
                         f"the view is [{outer}, {n}, {inner}]")
    limit = {"group": AXIS_GROUP_MAX_N, "block": AXIS_BLOCK_MAX_N}.get(resolved)
    if limit is not None and n > limit:
        raise ValueError(f"{name}: route {route!r} takes rows of at most {limit} elements, got {n}")
    if chunk is not None:
        if resolved == "split":
            if chunk < _AXIS_TILE or chunk % _AXIS_TILE:
                raise ValueError(f"{name}: the chunk of route 'split' is a positive multiple of {_AXIS_TILE}, got {chunk}")
        elif resolved == "column_split":
            if chunk < AXIS_COLUMN_MIN_CHUNK:
                raise ValueError(f"{name}: the chunk of route 'column_split' is at least {AXIS_COLUMN_MIN_CHUNK}, got {chunk}")
        else:
            raise ValueError(f"{name}: chunk is for the split routes, the route here is {resolved!r}")
    return (0 if route is None else _AXIS_ROUTE_CODE[route]), (0 if chunk is None else chunk)


def _axis_view(x: torch.Tensor, dim, op, name: str):
    """(outer, n, inner, dim normalised) of the [outer, n, inner] view along dim, after the checks of x, op and dim."""
    if isinstance(dim, bool) or not isinstance(dim, int):
        raise TypeError(f"{name}: dim must be an int or None, got {type(dim).__name__}")
    if x.dim() < 1 or not -x.dim() <= dim < x.dim():
        raise IndexError(f"{name}: dim {dim} is out of range for a tensor with {x.dim()} dimensions")
    if x.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"{name}: x must be float32 or int32, got {x.dtype}")
    if op not in OP_CODES:
        raise ValueError(f"{name}: op must be one of {sorted(OP_CODES)}, got {op!r}")
    if x.numel() >= 1 << 31:
        raise ValueError(f"{name}: x has {x.numel()} elements; offsets are 31-bit (fewer than 2^31)")
    d = dim % x.dim()
    return int(torch.Size(x.shape[:d]).numel()), x.shape[d], int(torch.Size(x.shape[d + 1:]).numel()), d


def _wrap_i32(t: torch.Tensor) -> torch.Tensor:
    return (((t + (1 << 31)) % (1 << 32)) - (1 << 31)).int()


def _axis_reduce(x: torch.Tensor, op, dim, keepdim, route, chunk) -> torch.Tensor:
    outer, n, inner, d = _axis_view(x, dim, op, "reduce")
    code, chunk = _axis_plan("reduce", route, chunk, outer, n, inner, "reduce")
    if n == 0 and op != "sum":
        raise ValueError(f"reduce: {op} along a dimension of size 0 has no identity")
    x3 = x.contiguous().view(outer, n, inner)
    if x.is_cuda:
        res = ops().axis_reduce(x3, OP_CODES[op], code, chunk)
    elif op == "sum":
        res = _wrap_i32(x3.long().sum(1)) if x.dtype == torch.int32 else x3.double().sum(1).float()
    else:
        res = torch.amin(x3, 1) if op == "min" else torch.amax(x3, 1)
    shape = list(x.shape)
    shape[d:d + 1] = [1] if keepdim else []
    return res.reshape(shape)


def _axis_scan(x: torch.Tensor, op, exclusive, init, check, dim, out, route, chunk) -> torch.Tensor:
    if init is not None:
        raise ValueError("scan: init is the single offset of the flat multi-GPU scan; with dim it must be None")
    outer, n, inner, d = _axis_view(x, dim, op, "scan")
    code, chunk = _axis_plan("scan", route, chunk, outer, n, inner, "scan")
    _check_scan_out(out, x)
    exclusive = bool(exclusive)
    x3 = x.contiguous().view(outer, n, inner)
    if x.is_cuda:
        res = ops().axis_scan(x3, OP_CODES[op], exclusive, code, chunk, out)
        if check:
            scan_check(x.device)
        return out if out is not None else res.view(x.shape)
    if x3.numel() == 0:
        res = x3.clone()
    else:
        if op == "sum":
            incl = torch.cumsum(x3.long() if x.dtype == torch.int32 else x3.double(), 1)
        else:
            incl = (torch.cummin if op == "min" else torch.cummax)(x3, 1).values
        if exclusive:
            ident = 0 if op == "sum" else _SCAN_IDENTITY[op][0 if x.dtype == torch.float32 else 1]
            incl = torch.cat([torch.full_like(incl[:, :1], ident), incl[:, :-1]], 1)
        res = incl if op != "sum" else (_wrap_i32(incl) if x.dtype == torch.int32 else incl.float())
    if out is None:
        return res.view(x.shape)
    out.view(-1).copy_(res.reshape(-1))
    return out


# ---------------------------------------------------------------- histograms (bincount / histc / explicit edges)
# int32 counts of x.flatten() per bin: bincount (the value of an int32 / uint8 sample is its bin), histc (equal-width
# float32 bins of [lo, hi]) and histogram (float32 bins between ascending edges). The generalisation of program 4's
# 256-bin image histogram; on the GPU one persistent kernel per form (csrc/kernels/bincount.hip): counters in LDS up to
# HIST_LDS_BINS bins (replicated and bank-rotated while they fit several times), in LDS with the bins cut into ranges
# and the input read once per range up to HIST_RANGED_BINS, straight integer atomics above, no block waits for
# another. Common rules:
#  * Counts are int32 (as unique / run_length_encode give), exact, and the same on every call. Fewer than 2^31 samples.
#  * A sample that falls in no bin is IGNORED (never an error): a negative or too large int, a float outside the range,
#    NaN, +-inf.
#  * out (optional): 1-D, exactly num_bins entries, int32 (float32 with float32 weights), on x's device; overwritten.
#    accumulate=True adds into out instead (a histogram over chunks). x is never written. An empty x gives zeros, or
#    leaves an accumulated out as it is.
#  * Nothing synchronises, except bincount(num_bins=None), which reads the largest sample (one sync).
#  * Measured on one MI355X at 2^28 samples (profiles/r12_bincount/README.md): int32 bincount 0.18 ms up to 24576 bins
#    for uniform, all-in-one-bin, sorted and zipf samples alike (1.06-1.10x a copy of the same bytes; torch.bincount
#    1.0-11.8 ms; unique with counts 5.8-8.2 ms), 0.34 ms at 24577 bins, 7.6 ms at 1572864, 9.9 ms above (torch 11.9);
#    uint8 0.093 ms; histc 0.27 ms at 256 bins (torch.histc 1.34); histogram 1.35 ms at 64 bins, 3.1 at 8192. The
#    weakest case is a zipf-like skew above HIST_RANGED_BINS: 216 ms (torch 237). float32 weights are SLOWER than
#    torch.bincount: 16.8 against 1.95 ms at 256 bins (the sort).
HIST_LDS_BINS = 24576     # csrc/kernels/bincount.hip kLdsBins: the counters of all bins fit one block's LDS up to here
HIST_RANGED_BINS = 64 * HIST_LDS_BINS  # kMaxRanges * kLdsBins: LDS counting over bin ranges up to here, global atomics above
HIST_MAX_EDGE_BINS = 8192  # histogram(): the edges live in LDS beside the counters


def _check_hist_common(x: torch.Tensor, num_bins: int, out, accumulate: bool, out_dtype: torch.dtype, name: str) -> None:
    if x.numel() >= 1 << 31:
        raise ValueError(f"{name}: x has {x.numel()} elements; counts are int32 (fewer than 2^31)")
    if accumulate and out is None:
        raise ValueError(f"{name}: accumulate=True needs out")
    if out is None:
        return
    if out.dtype != out_dtype:
        raise TypeError(f"{name}: out must be {out_dtype}, got {out.dtype}")
    if out.device != x.device:
        raise ValueError(f"{name}: out is on {out.device}, x on {x.device}")
    if out.dim() != 1 or out.numel() != num_bins:
        raise ValueError(f"{name}: out must be 1-D with exactly {num_bins} entries, got shape {tuple(out.shape)}")


def _wrap_i32(s: torch.Tensor) -> torch.Tensor:
    return (((s + (1 << 31)) % (1 << 32)) - (1 << 31)).int()


def _host_counts(bins_of_kept: torch.Tensor, num_bins: int, amounts: torch.Tensor | None, out, accumulate: bool):
    """The CPU paths' result: int64 sums per bin over the kept samples (1 each, or amounts), wrapped to int32."""
    add = torch.ones_like(bins_of_kept) if amounts is None else amounts.long()
    c = _wrap_i32(torch.zeros(num_bins, dtype=torch.int64).index_add_(0, bins_of_kept, add))
    if out is None:
        return c
    if accumulate:
        c = _wrap_i32(out.long() + c.long())
    out.copy_(c)
    return out


def _bincount_f32_weights(keys: torch.Tensor, weights: torch.Tensor, num_bins: int, out, accumulate: bool):
    """sum of float32 weights per bin without float atomics: stable sort by key, fixed-order sum per run, scatter of
    the run sums. Runs whose key is no bin, and the unwritten tail past num_runs, go to a discarded extra slot, so
    nothing has to be read back."""
    n = keys.numel()
    if n == 0:
        return out if out is not None and accumulate else (
            out.zero_() if out is not None else torch.zeros(num_bins, dtype=torch.float32, device=keys.device))
    ks, vs = sort_by_key(keys, weights.reshape(-1))
    rk, ra, num = reduce_by_key(ks, vs, "sum")
    live = (torch.arange(n, device=keys.device) < num) & (rk >= 0) & (rk < num_bins)
    slot = torch.where(live, rk.long(), num_bins)
    dense = torch.zeros(num_bins + 1, dtype=torch.float32, device=keys.device).scatter_(0, slot, ra)[:num_bins]
    if out is None:
        return dense
    if accumulate:
        out.add_(dense)
    else:
        out.copy_(dense)
    return out


def bincount(x: torch.Tensor, num_bins: int | None = None, weights: torch.Tensor | None = None,
             out: torch.Tensor | None = None, accumulate: bool = False) -> torch.Tensor:
    """out[b] = how many samples of x.flatten() (int32 or uint8) equal b, for b in [0, num_bins), as int32; samples
    below 0 or at or above num_bins are ignored. num_bins=None sizes the result like torch.bincount, max + 1 (0 bins
    for an empty x): ONE host sync, and ValueError on a negative sample. weights (same numel and device): int32 weights
    are summed per bin in the same kernel, int32 result, sums wrap mod 2^32 and are exact. float32 weights give a
    float32 result with the same bits on every call (no float atomics): that route COSTS A SORT (sort_by_key, then
    reduce_by_key's fixed-order sums, then a scatter; at most SORT_MAX_N samples) and is far slower than the integer
    forms. out / accumulate: see the rules above. Does not synchronise when num_bins is given."""
    if x.dtype not in (torch.int32, torch.uint8):
        raise TypeError(f"bincount: x must be int32 or uint8, got {x.dtype}")
    if weights is not None:
        if weights.dtype not in (torch.int32, torch.float32):
            raise TypeError(f"bincount: weights must be int32 or float32, got {weights.dtype}")
        if weights.numel() != x.numel():
            raise ValueError(f"bincount: {weights.numel()} weights for {x.numel()} samples")
        if weights.device != x.device:
            raise ValueError(f"bincount: weights are on {weights.device}, x on {x.device}")
    if num_bins is None:
        if x.numel() == 0:
            num_bins = 0
        else:
            lo, hi = torch.stack(torch.aminmax(x)).tolist()  # the one host sync
            if lo < 0:
                raise ValueError(f"bincount: num_bins=None needs non-negative samples, the smallest is {lo}")
            num_bins = int(hi) + 1
    elif isinstance(num_bins, bool) or not isinstance(num_bins, int):
        raise TypeError(f"bincount: num_bins must be an int or None, got {type(num_bins).__name__}")
    elif not 1 <= num_bins < 1 << 31:
        raise ValueError(f"bincount: num_bins must be in 1..2^31 - 1, got {num_bins}")
    fw = weights is not None and weights.dtype == torch.float32
    _check_hist_common(x, num_bins, out, accumulate, torch.float32 if fw else torch.int32, "bincount")
    if num_bins == 0:
        return out if out is not None else torch.zeros(0, dtype=torch.float32 if fw else torch.int32, device=x.device)
    if fw:
        return _bincount_f32_weights(x.reshape(-1).int(), weights, num_bins, out, bool(accumulate))
    if x.is_cuda:
        return ops().bincount(x, num_bins, weights, out, bool(accumulate))
    v = x.reshape(-1).long()
    keep = (v >= 0) & (v < num_bins)
    return _host_counts(v[keep], num_bins, None if weights is None else weights.reshape(-1)[keep], out, bool(accumulate))


def _histc_scale(bins: int, lo: float, hi: float):
    """(lo, hi, scale) as the float32 values the definition uses; ValueError for a range that is empty, reversed, not
    finite, or no longer a finite positive width in float32."""
    if isinstance(bins, bool) or not isinstance(bins, int):
        raise TypeError(f"histc: bins must be an int, got {type(bins).__name__}")
    if not 1 <= bins < 1 << 31:
        raise ValueError(f"histc: bins must be in 1..2^31 - 1, got {bins}")
    lo32, hi32 = torch.tensor(float(lo), dtype=torch.float32), torch.tensor(float(hi), dtype=torch.float32)
    width = hi32 - lo32
    if not (torch.isfinite(lo32) and torch.isfinite(hi32) and torch.isfinite(width) and lo32 < hi32):
        raise ValueError(f"histc: lo < hi, both finite in float32 with a finite width, got lo={lo}, hi={hi}")
    scale = torch.tensor(float(bins), dtype=torch.float32) / width
    if not torch.isfinite(scale):
        raise ValueError(f"histc: {bins} bins over [{lo}, {hi}] have no finite float32 scale")
    return lo32, hi32, scale


def histc(x: torch.Tensor, bins: int, lo: float, hi: float, out: torch.Tensor | None = None,
          accumulate: bool = False) -> torch.Tensor:
    """int32 counts of the float32 samples of x.flatten() in `bins` equal-width bins of [lo, hi] (bins >= 1, lo < hi,
    both finite; else ValueError). The bin is DEFINED by this float32 sequence, every step rounded on its own (no FMA):
        scale = float32(bins) / (float32(hi) - float32(lo))        once, on the host
        bin   = min(int((v - lo) * scale), bins - 1)                counted only when lo <= v <= hi
    so v == hi falls in the last bin and NaN, +-inf and samples outside the range are ignored (the range is compared
    in float before anything is converted). The definition is ours: torch.histc returns floats, and its CPU and GPU
    builds place samples that lie within rounding distance of a bin border differently (they compute the bin by other,
    mutually different formulas). All of them agree with this one wherever the arithmetic is exact, e.g. a
    power-of-two range with samples on a dyadic grid, and everywhere away from the borders. out / accumulate: see the
    rules above. Does not synchronise."""
    if x.dtype != torch.float32:
        raise TypeError(f"histc: x must be float32, got {x.dtype}")
    lo32, hi32, scale = _histc_scale(bins, lo, hi)
    _check_hist_common(x, bins, out, accumulate, torch.int32, "histc")
    if x.is_cuda:
        return ops().hist_even(x, bins, lo32.item(), hi32.item(), scale.item(), out, bool(accumulate))
    v = x.reshape(-1)
    v = v[(v >= lo32) & (v <= hi32)]
    b = ((v - lo32) * scale).to(torch.int64).clamp(max=bins - 1)
    return _host_counts(b, bins, None, out, bool(accumulate))


def histogram(x: torch.Tensor, edges: torch.Tensor, out: torch.Tensor | None = None,
              accumulate: bool = False) -> torch.Tensor:
    """int32 counts of the float32 samples of x.flatten() in the B bins between the B + 1 ascending float32 values of
    the 1-D tensor edges (on x's device, 1 <= B <= HIST_MAX_EDGE_BINS = 8192): bin i holds edges[i] <= v < edges[i+1],
    the last bin also v == edges[B] (the numpy / torch.histogram rule; repeated edges give empty bins). NaN and samples
    outside [edges[0], edges[B]] are ignored. Ascending order is the caller's duty: unsorted edges give unspecified
    counts, but every index of the search is clamped, so nothing outside the tensors is touched. out / accumulate: see
    the rules above. Does not synchronise."""
    if x.dtype != torch.float32:
        raise TypeError(f"histogram: x must be float32, got {x.dtype}")
    if edges.dtype != torch.float32:
        raise TypeError(f"histogram: edges must be float32, got {edges.dtype}")
    if edges.device != x.device:
        raise ValueError(f"histogram: edges are on {edges.device}, x on {x.device}")
    if edges.dim() != 1 or edges.numel() < 2:
        raise ValueError(f"histogram: edges must be 1-D with at least 2 values, got shape {tuple(edges.shape)}")
    nb = edges.numel() - 1
    if nb > HIST_MAX_EDGE_BINS:
        raise ValueError(f"histogram: {nb} bins; the limit is {HIST_MAX_EDGE_BINS} (the edges are kept in LDS)")
    _check_hist_common(x, nb, out, accumulate, torch.int32, "histogram")
    if x.is_cuda:
        return ops().hist_range(x, edges, out, bool(accumulate))
    v = x.reshape(-1)
    v = v[(v >= edges[0]) & (v <= edges[nb])]
    b = (torch.searchsorted(edges.contiguous(), v, right=True) - 1).clamp(0, nb - 1)
    return _host_counts(b, nb, None, out, bool(accumulate))


# ---------------------------------------------------------------- merge of sorted sequences / sorted search
# For data that is ALREADY sorted: merge two sorted sequences in one pass, and find where values fall in a sorted
# sequence (searchsorted / bucketize). float32 or int32 keys, flattened, in sort's order (above): float32 -0.0 == +0.0,
# every NaN one key above +inf; descending reverses the order of the keys, not of ties. On the GPU the merge-path
# diagonal partition (csrc/kernels/merge.hip; no counterpart in the reference programs): one thread per output tile of
# MERGE_TILE keys finds where the tile starts in a and in b, one block per tile merges its two ranges through LDS. No
# block waits for another, nothing can time out (scan_check() has nothing to report), nothing synchronises and the
# outputs are the same on every call.
#  * "Sorted" means non-decreasing in that order (non-increasing keys for descending=True). It is the caller's duty and
#    is not checked: unsorted input gives an unspecified result, but nothing outside the tensors is touched.
#  * DEFINITION of the merge: with cat = torch.cat([a.flatten(), b.flatten()]),
#        merge(a, b, d)[1] == argsort(cat, descending=d)       and       merge(a, b, d)[0] == cat[indices], bit for bit.
#    A tie goes to a: an element of a precedes an equal element of b. Unlike sort, nothing is transformed, so NaN
#    payloads and the sign of zero come out as they went in.
#  * searchsorted equals torch.searchsorted except for NaN: here a NaN value ties with the NaNs at the end of the
#    sequence (right=False gives the index of the first NaN), where torch sends it to len(sequence) on both sides.
#    Results are int32. values_sorted=True is the caller's promise that the values are sorted in the same order: with
#    at least an eighth as many values as keys the search then runs as a merge of values and sequence that writes no
#    keys (it reads both once, bandwidth-bound and load-balanced) instead of one two-level binary search per value
#    (SEARCH_LDS_KEYS evenly spaced keys of the sequence in LDS, then the one interval left in global memory;
#    latency-bound). Same result when the promise holds.
#  * An input that is not contiguous is gathered first; a slice such as x[1:] is read where it lies.
#  * Measured on one MI355X (profiles/r14_merge/README.md): merge_keys of 2^27 + 2^27 float32 keys 1.26 ms (0.93 when
#    the sides do not interleave) against 8.14 ms for sort_keys(cat) and 9.5 for torch.sort(cat); merge_by_key 1.79 ms,
#    merge 1.37 ms; 2.5-3.9x the time of a copy_ of the same bytes. searchsorted in 2^28 keys: 2^28 sorted values with
#    values_sorted=True 2.18 ms against torch.searchsorted 7.40; 2^20 random values 0.27 against 0.32 ms. SLOWER than
#    torch.searchsorted: 2^28 random values (72.2 against 69.5 ms) and sorted values that take the binary search, i.e.
#    without the promise or fewer than an eighth of the keys (2^28: 8.2 against 7.4 ms; 2^20: 0.18 against 0.12 ms; the
#    merge route would read the whole sequence for them: 0.86 ms).
MERGE_TILE = 4352          # csrc/kernels/merge.hip kTile: output keys per block (256 lanes x 17 keys)
SEARCH_LDS_KEYS = 8192     # csrc/kernels/merge.hip kSamples: a sequence up to here is searched in LDS alone
MERGE_MAX_N = (1 << 31) - 1


def _check_merge_keys(a: torch.Tensor, b: torch.Tensor, name: str, na: str = "a", nb: str = "b") -> None:
    if a.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"{name}: {na} must be float32 or int32, got {a.dtype}")
    if b.dtype != a.dtype:
        raise TypeError(f"{name}: {nb} is {b.dtype}, {na} is {a.dtype}")
    if b.device != a.device:
        raise ValueError(f"{name}: {nb} is on {b.device}, {na} on {a.device}")


def _check_merge(a: torch.Tensor, b: torch.Tensor, name: str) -> None:
    _check_merge_keys(a, b, name)
    if a.numel() + b.numel() > MERGE_MAX_N:
        raise ValueError(f"{name}: {a.numel()} + {b.numel()} elements; indices are int32 (at most 2^31 - 1 together)")


def _check_merge_pairs(keys_a, values_a, keys_b, values_b, name: str) -> None:
    _check_merge_keys(keys_a, keys_b, name, "keys_a", "keys_b")
    if values_a.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"{name}: values must be float32 or int32, got {values_a.dtype}")
    if values_b.dtype != values_a.dtype:
        raise TypeError(f"{name}: values_b is {values_b.dtype}, values_a is {values_a.dtype}")
    for k, v, side in ((keys_a, values_a, "a"), (keys_b, values_b, "b")):
        if v.numel() != k.numel():
            raise ValueError(f"{name}: {v.numel()} values for {k.numel()} keys on side {side}")
        if v.device != keys_a.device:
            raise ValueError(f"{name}: values_{side} are on {v.device}, the keys on {keys_a.device}")
    _check_merge(keys_a, keys_b, name)


def _order_key64(x: torch.Tensor, descending: bool) -> torch.Tensor:
    """int64 keys of flat x whose ascending order is the wanted order: radix_key.h's to_key, computed with torch."""
    b = x.reshape(-1).contiguous().view(torch.int32).long() & 0xFFFFFFFF
    if x.dtype == torch.float32:
        mag = b & 0x7FFFFFFF
        k = torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)
        k = torch.where(mag == 0, torch.full_like(k, 0x80000000), k)
        k = torch.where(mag > 0x7F800000, torch.full_like(k, 0xFFFFFFFF), k)
    else:
        k = b ^ 0x80000000
    return 0xFFFFFFFF - k if descending else k


def _host_merge(a: torch.Tensor, b: torch.Tensor, descending: bool):
    """(int32 view of the concatenation, int64 order of its stable sort)"""
    cat = torch.cat([a.reshape(-1), b.reshape(-1)])
    return cat.view(torch.int32), _host_order(cat, descending, 32)


def merge_keys(a: torch.Tensor, b: torch.Tensor, descending: bool = False) -> torch.Tensor:
    """The keys of two sorted tensors (float32 or int32, same dtype and device, either may be empty) merged into one
    sorted 1-D tensor: sort_keys(cat(a, b)) for sorted inputs, with every key's bits kept (rules above)."""
    _check_merge(a, b, "merge_keys")
    if a.is_cuda:
        return ops().merge_keys(a, b, bool(descending), None)
    bits, order = _host_merge(a, b, bool(descending))
    return bits[order].view(a.dtype)


def merge(a: torch.Tensor, b: torch.Tensor, descending: bool = False):
    """(keys, indices) of the merge of two sorted tensors: indices are int32 positions in cat(a.flatten(), b.flatten())
    (i for a[i], a.numel() + i for b[i]) and equal argsort(cat, descending); keys == cat[indices] bit for bit. A tie
    goes to a."""
    _check_merge(a, b, "merge")
    if a.is_cuda:
        return tuple(ops().merge_index(a, b, bool(descending), True, None, None))
    bits, order = _host_merge(a, b, bool(descending))
    return bits[order].view(a.dtype), order.int()


def merge_by_key(keys_a: torch.Tensor, values_a: torch.Tensor, keys_b: torch.Tensor, values_b: torch.Tensor,
                 descending: bool = False):
    """(keys, values): the merge of two sorted key tensors with their values (float32 or int32, the same dtype on both
    sides, one per key, moved as bits) carried along. A tie goes to a."""
    _check_merge_pairs(keys_a, values_a, keys_b, values_b, "merge_by_key")
    if keys_a.is_cuda:
        return tuple(ops().merge_pairs(keys_a, values_a, keys_b, values_b, bool(descending), None, None))
    bits, order = _host_merge(keys_a, keys_b, bool(descending))
    # (indexing an int32 view: a float gather would be free to quieten a signalling NaN payload)
    vbits = torch.cat([values_a.reshape(-1), values_b.reshape(-1)]).view(torch.int32)[order]
    return bits[order].view(keys_a.dtype), vbits.view(values_a.dtype)


def searchsorted(sorted_sequence: torch.Tensor, values: torch.Tensor, right: bool = False, descending: bool = False,
                 values_sorted: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
    """int32 tensor in the shape of values: for each value the number of keys of the flattened sorted_sequence that
    precede it (right=False: the first position where it could be inserted) or that precede or equal it (right=True:
    the last such position), in sort's order; descending=True for a sequence sorted descending. float32 or int32, both
    tensors the same dtype and device, fewer than 2^31 elements each. Equal to torch.searchsorted EXCEPT for NaN: a NaN
    value ties with the NaNs at the end of the sequence (with one trailing NaN in 7 keys, right=False gives 6 where
    torch gives 7), and -0.0 ties with +0.0 as in torch. values_sorted=True promises that the values are sorted in the
    same order and picks the merge route (rules above); the result is the same. out (optional): int32, values' shape
    and device, overwritten. Sortedness is not checked. Does not synchronise."""
    _check_merge_keys(sorted_sequence, values, "searchsorted", "sorted_sequence", "values")
    if sorted_sequence.numel() > MERGE_MAX_N or values.numel() > MERGE_MAX_N:
        raise ValueError(f"searchsorted: {sorted_sequence.numel()} keys and {values.numel()} values; results are int32 "
                         "(at most 2^31 - 1 each)")
    if out is not None:
        if out.dtype != torch.int32:
            raise TypeError(f"searchsorted: out must be int32, got {out.dtype}")
        if out.device != values.device:
            raise ValueError(f"searchsorted: out is on {out.device}, values on {values.device}")
        if out.shape != values.shape:
            raise ValueError(f"searchsorted: out must have shape {tuple(values.shape)}, got {tuple(out.shape)}")
    if values.is_cuda:
        direct = out is None or out.is_contiguous()
        r = ops().searchsorted(sorted_sequence, values, bool(right), bool(descending), bool(values_sorted),
                               out if direct else None)
    else:
        r = torch.searchsorted(_order_key64(sorted_sequence, bool(descending)), _order_key64(values, bool(descending)),
                               right=bool(right)).int().reshape(values.shape)
        direct = out is None
    if direct:
        return r
    out.copy_(r)
    return out


def bucketize(values: torch.Tensor, boundaries: torch.Tensor, right: bool = False) -> torch.Tensor:
    """torch.bucketize with int32 results: searchsorted(boundaries, values, right) for ascending boundaries."""
    return searchsorted(boundaries, values, right=right)


# ---------------------------------------------------------------- set operations on sorted sequences
# Intersection, union, difference and symmetric difference of two SORTED tensors (thrust::set_*, std::set_*): what one
# does with sorted id lists. float32 or int32, same dtype and device, flattened, sorted in the merge's order (above;
# descending=True for descending input); sortedness is the caller's duty and is not checked (unsorted input gives an
# unspecified result, but nothing outside the tensors is touched); a.numel() + b.numel() < 2^31. On the GPU one fused
# pass on the merge-path tiles (csrc/kernels/setops.hip; no counterpart in the reference programs): a partition kernel,
# then one block per SETOP_TILE merged positions that merges in LDS, decides per element, and stores compacted at an
# exact position from the decoupled look-back (scan_check() reports a look-back that gave up, as for select).
#  * Two elements are EQUAL when their transformed keys are: -0.0 == +0.0, every NaN equals every NaN.
#  * MULTISETS, by position. For a key that occurs m times in a and n times in b, the i-th occurrence in a is paired
#    with the i-th in b for i < min(m, n). Then
#        intersection          keeps the paired elements of a (the first min(m, n))         capacity min(na, nb)
#        difference            keeps the unpaired elements of a (the last max(m - n, 0))    capacity na
#        union                 keeps all of a and the unpaired elements of b (the last max(n - m, 0))   na + nb
#        symmetric_difference  keeps the unpaired elements of both                          capacity na + nb
#  * The result is the kept elements IN THE ORDER OF merge(a, b) (a tie goes to a): the merge filtered by a keep mask.
#    Keys are moved as their raw bits and nothing is transformed: the intersection of [-0.0] and [+0.0] is [-0.0], and
#    NaN payloads survive. Indices, where asked for, are int32 positions in cat(a.flatten(), b.flatten()), as in merge;
#    in the by-key forms a value travels with its kept element.
#  * set_compact / set_compact_by_key follow compact: the outputs have the op's capacity, only [:count] is written,
#    count is a 0-d int64 tensor on the inputs' device, nothing synchronises. set_intersection / set_union /
#    set_difference / set_symmetric_difference / set_op_by_key cut to the exact size (one host sync for the count).
#    intersect1d / union1d / setdiff1d / setxor1d are numpy's: unsorted input of any shape, unique() on each side (so
#    both zeros are +0.0 and all NaNs are one canonical NaN, last), then the set op.
#  * An input that is not contiguous is gathered first; a slice such as x[1:] is read where it lies.
SETOP_TILE = 4352          # csrc/kernels/setops.hip kTile: merged positions per block (the merge's tile)
SET_OP_CODES = {"intersection": 0, "union": 1, "difference": 2, "symmetric_difference": 3}   # PCMX_SET_*


def _set_capacity(op: str, na: int, nb: int, name: str) -> int:
    if op not in SET_OP_CODES:
        raise ValueError(f"{name}: op must be one of {sorted(SET_OP_CODES)}, got {op!r}")
    return min(na, nb) if op == "intersection" else (na if op == "difference" else na + nb)


def _host_set(a: torch.Tensor, b: torch.Tensor, op: str, descending: bool):
    """(int32 view of the concatenation, int64 positions in it of the kept elements, in merge order): the definition
    above with torch ops."""
    af, bf = a.reshape(-1), b.reshape(-1)
    ka, kb = _order_key64(af, descending), _order_key64(bf, descending)

    def paired(own, other):  # rank in the element's own run < length of the other side's run of its key
        lower = torch.searchsorted(own, own)
        upper = torch.searchsorted(other, own, right=True)
        return torch.arange(own.numel(), device=own.device) - lower < upper - torch.searchsorted(other, own)

    pa, pb = paired(ka, kb), paired(kb, ka)
    keep = {"intersection": (pa, torch.zeros_like(pb)), "union": (torch.ones_like(pa), ~pb),
            "difference": (~pa, torch.zeros_like(pb)), "symmetric_difference": (~pa, ~pb)}[op]
    order = torch.sort(torch.cat([ka, kb]), stable=True).indices  # a tie goes to a
    return torch.cat([af, bf]).view(torch.int32), order[torch.cat(keep)[order]]


def set_compact(a: torch.Tensor, b: torch.Tensor, op: str, descending: bool = False, indices: bool = False,
                out_keys: torch.Tensor | None = None, out_indices: torch.Tensor | None = None):
    """(keys, count), or (keys, idx, count) with indices=True: the set operation `op` (a key of SET_OP_CODES) on two
    sorted tensors, rules above. keys (a's dtype) and idx (int32 positions in cat(a.flatten(), b.flatten())) have the
    op's capacity and are written in [:count] only; count is a 0-d int64 tensor on a's device. out_keys / out_indices
    (optional, 1-D, contiguous, at least the capacity) are left untouched from count on. Does not synchronise."""
    _check_merge(a, b, "set_compact")
    cap = _set_capacity(op, a.numel(), b.numel(), "set_compact")
    if out_indices is not None and not indices:
        raise ValueError("set_compact: out_indices needs indices=True")
    _check_out(out_keys, a.dtype, cap, a)
    _check_out(out_indices, torch.int32, cap, a)
    if a.is_cuda:
        keys, idx, count = ops().set_op(a, b, SET_OP_CODES[op], bool(descending), bool(indices), out_keys, out_indices)
        return (keys, idx, count) if indices else (keys, count)
    bits, kept = _host_set(a, b, op, bool(descending))
    keys, count = _host_result(bits[kept].view(a.dtype), cap, out_keys)
    return (keys, _host_result(kept.int(), cap, out_indices)[0], count) if indices else (keys, count)


def set_compact_by_key(keys_a: torch.Tensor, values_a: torch.Tensor, keys_b: torch.Tensor, values_b: torch.Tensor,
                       op: str, descending: bool = False):
    """(keys, values, count): set_compact with a value per key (float32 or int32, the same dtype on both sides, moved
    as bits) that travels with its kept element. Does not synchronise."""
    _check_merge_pairs(keys_a, values_a, keys_b, values_b, "set_compact_by_key")
    cap = _set_capacity(op, keys_a.numel(), keys_b.numel(), "set_compact_by_key")
    if keys_a.is_cuda:
        return tuple(ops().set_op_pairs(keys_a, values_a, keys_b, values_b, SET_OP_CODES[op], bool(descending)))
    bits, kept = _host_set(keys_a, keys_b, op, bool(descending))
    # (indexing an int32 view: a float gather would be free to quieten a signalling NaN payload)
    vbits = torch.cat([values_a.reshape(-1), values_b.reshape(-1)]).view(torch.int32)[kept]
    keys, count = _host_result(bits[kept].view(keys_a.dtype), cap, None)
    return keys, _host_result(vbits.view(values_a.dtype), cap, None)[0], count


def _set_exact(a, b, op: str, descending: bool, return_indices: bool):
    r = set_compact(a, b, op, descending, indices=return_indices)
    k = int(r[-1].item())
    return (r[0][:k], r[1][:k]) if return_indices else r[0][:k]


def set_intersection(a: torch.Tensor, b: torch.Tensor, descending: bool = False, return_indices: bool = False):
    """The elements of sorted a that have a partner in sorted b (multiset rule above), at exact size (one host sync);
    with return_indices (keys, int32 positions in cat(a.flatten(), b.flatten()))."""
    return _set_exact(a, b, "intersection", descending, return_indices)


def set_union(a: torch.Tensor, b: torch.Tensor, descending: bool = False, return_indices: bool = False):
    """All of sorted a and the elements of sorted b without a partner in a, in merge order, at exact size."""
    return _set_exact(a, b, "union", descending, return_indices)


def set_difference(a: torch.Tensor, b: torch.Tensor, descending: bool = False, return_indices: bool = False):
    """The elements of sorted a without a partner in sorted b, at exact size."""
    return _set_exact(a, b, "difference", descending, return_indices)


def set_symmetric_difference(a: torch.Tensor, b: torch.Tensor, descending: bool = False, return_indices: bool = False):
    """The elements of either sorted tensor without a partner in the other, in merge order, at exact size."""
    return _set_exact(a, b, "symmetric_difference", descending, return_indices)


def set_op_by_key(keys_a: torch.Tensor, values_a: torch.Tensor, keys_b: torch.Tensor, values_b: torch.Tensor, op: str,
                  descending: bool = False):
    """(keys, values) of set_compact_by_key at exact size (one host sync for the count)."""
    keys, values, count = set_compact_by_key(keys_a, values_a, keys_b, values_b, op, descending)
    k = int(count.item())
    return keys[:k], values[:k]


def intersect1d(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """np.intersect1d: the sorted distinct values present in both x and y (any shape, any order)."""
    return set_intersection(unique(x), unique(y))


def union1d(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """np.union1d: the sorted distinct values present in x or in y."""
    return set_union(unique(x), unique(y))


def setdiff1d(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """np.setdiff1d: the sorted distinct values of x that are not in y."""
    return set_difference(unique(x), unique(y))


def setxor1d(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """np.setxor1d: the sorted distinct values present in exactly one of x and y."""
    return set_symmetric_difference(unique(x), unique(y))


# ---------------------------------------------------------------- reduction / scan over ragged segments (offsets)
# The third way of reducing in pieces, beside runs of equal keys (reduce_by_key, scan_by_key) and equal-length rows
# (dim=): ragged segments given by an offsets tensor, the form of CSR.row_ptr, powerlaw_row_ptr and the starts of
# run_length_encode, and of torch.segment_reduce(data, reduce, offsets=...). Segment j is
# x.flatten()[offsets[j] : offsets[j+1]]; result j belongs to segment j, empty segments included. On the GPU the list
# of segment ends is merged with the element indices and every block takes RAGGED_TILE steps of that path, so one
# segment of 2^28, 2^28 segments of one, power-law rows and mostly empty segments all load the blocks evenly
# (csrc/kernels/ragged.hip; no counterpart in the reference programs). No look-back, no block waits for another,
# nothing synchronises.
#  * PRECONDITION: 0 <= offsets[0] <= ... <= offsets[S] <= n. Elements before offsets[0] and from offsets[S] on belong
#    to no segment and are not read. It is not checked unless validate=True (one host sync); offsets that break it
#    give an unspecified result, but nothing outside the tensors is touched.
#  * An empty segment gives the identity: +0.0 / 0 for sum, +inf / INT32_MAX for min, -inf / INT32_MIN for max (for
#    floats the values of torch.segment_reduce).
#  * int32 sums wrap mod 2^32; int32 results and float32 min / max are exact; float32 min / max hand on a NaN inside
#    its segment only; a float32 sum uses a fixed association order that may depend on where the segment lies relative
#    to the tiles, never on timing: the same input gives the same bits on every call. A NaN or inf in one segment never
#    reaches another.
#  * Measured on one MI355X at 2^28 float32 elements (profiles/r18_ragged/README.md; ours / torch.segment_reduce /
#    reduce_by_key on expanded ids, ms): equal segments of 100 0.44 / 1.75 / 0.73, one segment 0.39 / 90.3 / 0.73,
#    power-law rows of mean 100 0.43 / 1.79 / n/a, S = 4 n 3.01 (torch raises from 2^26 segments); 2.1x-2.6x the time
#    of ops.copy_ of the same bytes in every case. SLOWER than torch at 2684 segments of 10^5 (0.378 against 0.196 ms)
#    and than the reduce_by_key route at length 1 (1.132 against 1.062 ms, its id expansion not counted).
RAGGED_TILE = 4352        # csrc/kernels/ragged.hip kTile: path steps (elements + segment ends) per block; not measured
RAGGED_LANE_ITEMS = 17    # kItems: path steps per lane (256 lanes per block); not measured
RAGGED_MAX_PATH = (1 << 31) - 1


def _check_segments(x: torch.Tensor, offsets: torch.Tensor, op: str, name: str) -> int:
    """The number of segments after the argument checks the two ops share."""
    if x.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"{name}: x must be float32 or int32, got {x.dtype}")
    if offsets.dtype != torch.int32:
        raise TypeError(f"{name}: offsets must be int32, got {offsets.dtype}")
    if op not in OP_CODES:
        raise ValueError(f"op must be one of {sorted(OP_CODES)}, got {op!r}")
    if offsets.device != x.device:
        raise ValueError(f"{name}: offsets are on {offsets.device}, x on {x.device}")
    if offsets.dim() != 1 or not offsets.is_contiguous() or offsets.numel() < 1:
        raise ValueError(f"{name}: offsets must be 1-D and contiguous with S + 1 >= 1 entries, got shape "
                         f"{tuple(offsets.shape)}")
    if not x.is_contiguous():
        raise ValueError(f"{name}: x must be contiguous")
    s = offsets.numel() - 1
    if x.numel() + s > RAGGED_MAX_PATH:
        raise ValueError(f"{name}: {x.numel()} elements and {s} segments; path positions are int32 (fewer than 2^31 "
                         "together)")
    return s


def _validate_offsets(offsets: torch.Tensor, n: int) -> None:
    """Raises ValueError naming the first entry that breaks 0 <= offsets[0] <= ... <= offsets[S] <= n (one host sync)."""
    o = offsets.long()
    lower = torch.cat([o.new_zeros(1), o[:-1]])  # what entry k must not lie below
    bad = (o < lower) | (o > n)
    k = int(torch.argmax(bad.int())) if bool(bad.any()) else -1
    if k < 0:
        return
    v = int(offsets[k])
    if v > n:
        raise ValueError(f"offsets[{k}] = {v} lies above the {n} elements of x")
    if k == 0 or v < 0:
        raise ValueError(f"offsets[{k}] = {v} is negative")
    raise ValueError(f"offsets[{k}] = {v} lies below offsets[{k - 1}] = {int(offsets[k - 1])}")


def _host_segment_reduce(x: torch.Tensor, offsets: torch.Tensor, op: str) -> torch.Tensor:
    """The CPU path: int32 sums through int64 prefix differences (exact, wrapped); everything else through
    torch.segment_reduce, int32 min / max on a float64 copy (exact) with the int32 identities for empty segments."""
    xf, s = x.reshape(-1), offsets.numel() - 1
    ident = _SCAN_IDENTITY[op][0 if x.dtype == torch.float32 else 1]
    if s == 0 or xf.numel() == 0:
        return torch.full((s,), ident, dtype=x.dtype)
    o = offsets.long()
    if x.dtype == torch.float32:
        return torch.segment_reduce(xf, op, offsets=o)
    if op == "sum":
        c = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(xf.long(), 0)])
        return _wrap_i32(c[o[1:]] - c[o[:-1]])
    r = torch.segment_reduce(xf.double(), op, offsets=o)
    return torch.where(o[1:] == o[:-1], torch.full_like(r, float(ident)), r).int()


def segment_reduce(x: torch.Tensor, offsets: torch.Tensor, op: str = "sum", out: torch.Tensor | None = None,
                   validate: bool = False) -> torch.Tensor:
    """[S] tensor of x's dtype: op (sum, min, max) over x.flatten()[offsets[j] : offsets[j+1]] for every j < S, S =
    offsets.numel() - 1: torch.segment_reduce(x, op, offsets=offsets) for float32 and int32 (rules above). x is
    contiguous, offsets int32, 1-D, contiguous, on x's device, with 0 <= offsets[0] <= ... <= offsets[S] <= x.numel();
    x.numel() + S < 2^31. An empty segment gives the identity (+0.0 / 0, +inf / INT32_MAX, -inf / INT32_MIN). out
    (optional: 1-D, contiguous, x's dtype, at least S elements, not overlapping an input) is written in [:S] only and
    returned as out[:S]. validate=True checks the offsets first (one host sync) and raises ValueError naming the first
    offending entry; without it offsets that break the precondition give an unspecified result (nothing outside the
    tensors is touched). S == 0 returns an empty tensor. Does not synchronise."""
    s = _check_segments(x, offsets, op, "segment_reduce")
    n = x.numel()
    if out is not None:
        if out.dtype != x.dtype:
            raise TypeError(f"out must be {x.dtype}, got {out.dtype}")
        if out.device != x.device:
            raise ValueError(f"out is on {out.device}, the input on {x.device}")
        if out.dim() != 1 or not out.is_contiguous() or out.numel() < s:
            raise ValueError(f"out must be 1-D, contiguous, with room for all {s} segments, got shape {tuple(out.shape)}")
        if _overlap(out, x) or _overlap(out, offsets):
            raise ValueError("out must not overlap x or offsets")
    if validate:
        _validate_offsets(offsets, n)
    if x.is_cuda:
        return ops().segment_reduce(x, offsets, OP_CODES[op], out)
    r = _host_segment_reduce(x, offsets, op)
    if out is None:
        return r
    out[:s] = r
    return out[:s]


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.numel() == 0 or b.numel() == 0 or a.device != b.device:
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def segment_scan(x: torch.Tensor, offsets: torch.Tensor, op: str = "sum", exclusive: bool = False,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """The running op (sum, min, max) inside every segment x.flatten()[offsets[j] : offsets[j+1]], with x's dtype and
    shape: segmented_scan with a head at every offsets[j] < x.numel(), for callers who hold offsets and not head flags
    (x, offsets and the limits as in segment_reduce; exclusive, out and the number rules as in segmented_scan). The
    positions before offsets[0] form one run of their own, and so do the positions from offsets[S] on. There is no
    validate: a head is stored only where 0 <= offsets[j] < x.numel(), so offsets out of order still touch nothing
    outside the tensors. Does not synchronise."""
    _check_segments(x, offsets, op, "segment_scan")
    n = x.numel()
    if x.is_cuda:
        heads = ops().segment_heads(offsets, n, x)
    else:
        heads = torch.zeros(n, dtype=torch.uint8)
        o = offsets.long()
        heads[o[(o >= 0) & (o < n)]] = 1
    return segmented_scan(x, heads, op, exclusive, out)


# ---------------------------------------------------------------- sort inside ragged segments (offsets)
# The sorting member of the offsets family: every segment x.flatten()[offsets[j] : offsets[j+1]] sorted on its own, the
# column indices of each CSR row, the candidates of each query, the tokens of each sequence of a packed batch. Restricted
# to a segment every output equals the 1-D op (sort_keys / sort / argsort / sort_by_key with the same descending and
# bits) on that slice, BIT FOR BIT: stable, ties by lowest position, float32 keys canonical, values moved as bits.
#  * offsets as for segment_reduce: int32, 1-D, contiguous, on x's device, S + 1 >= 1 entries, PRECONDITION
#    0 <= offsets[0] <= ... <= offsets[S] <= n, checked only with validate=True (one host sync, ValueError naming the
#    first bad entry). Offsets that break it give an unspecified result; every offset is clamped to [0, n] and a
#    negative length counts as 0, so nothing outside the tensors is read or written. n and S are at most 2^30 - 1.
#  * indices are FLAT int32 indices into x.flatten(): values.flatten() == x.flatten()[indices.flatten()] as bits for
#    int32 keys (float32 values are canonical), and indices[b:e] - b is the 1-D argsort of the slice.
#  * Elements before offsets[0] and from offsets[S] on belong to no segment: they come through with their bits unchanged
#    (NOT canonical) and their index is their own position; the two offsets are read on the device.
#  * On the GPU (csrc/kernels/segsort.hip; no counterpart in the reference programs) the segments are listed by length
#    class on the device and every class runs the row sort's in-CU passes over its list: one wave per segment up to
#    SEGSORT_CLASS_LIMITS[3] keys, one 512-thread block up to SEGSORT_MAX_LEN. A class launch is a FIXED grid of
#    SEGSORT_GRID_MULT blocks per compute unit striding over the list, so the launch needs no count on the host.
#    Segments LONGER than SEGSORT_MAX_LEN take the device-wide kernels: their keys are gathered into a packed buffer,
#    sorted by one stable index sort, then by long-segment rank (bits = ceil(log2 count); skipped for a single long
#    segment) and scattered back.
#  * HOST SYNCS: the host learns whether the long route is needed from a 16-byte summary: ONE host sync per call, and
#    none after it when no segment is that long (the long route itself synchronises again to size its buffers).
#    max_len=M is the caller's promise that no segment is longer than M: with M <= SEGSORT_MAX_LEN the call does not
#    synchronise at all. A segment that breaks the promise gets an unspecified result inside its own range (with M <=
#    SEGSORT_MAX_LEN: one longer than SEGSORT_MAX_LEN is left unwritten). validate=True also checks max_len.
#  * route: None is the rule above; "classes" never takes the long route and raises ValueError when the summary shows
#    a segment above SEGSORT_MAX_LEN (with max_len <= SEGSORT_MAX_LEN nothing is read back, so nothing is raised);
#    "global" sorts ALL keys with the device-wide kernels: a stable index sort, then a stable sort by segment id with
#    bits = ceil(log2(S + 2)), any lengths at about twice a flat sort: the route callers had before, the A/B partner and
#    the tests' cross-check. route is validated on CPU tensors too; "classes" refuses long segments there as well.
#  * CPU tensors: two stable torch.sort on the host (by key, then by segment id).
#  * The class borders are the row sort's instantiations under its measured border ROWSORT_WAVE_COLS (wave against block
#    at equal rows, above); they and SEGSORT_GRID_MULT are NOT MEASURED for ragged lengths
#    (profiles/r20_segsort/README.md holds the footprint of every instantiation and the lab's method).
#  * Measured on one MI355X (scripts/segsort_lab.py, profiles/r20_segsort/README.md): 2^28 keys NOT MEASURED yet. The
#    lab's launch-bound dry run at 2^21 float32 keys, ours / route="global" / the same composition in torch, ms with
#    indices: equal segments of 32 0.18 / 0.84 / 0.51, of 100 0.15 / 0.73 / 0.51, of 4096 0.16 / 0.70 / 0.50, of 16384
#    0.17 / 0.57 / 0.51, uniform borders of mean 100 0.16 / 0.70 / 0.50 (3.3x-4.8x global, 2.8x-3.4x torch). SLOWER at
#    that size: segments of 4 keys, keys alone 0.72 / 0.65 / 0.50 (one wave per 4 keys); power-law rows of mean 100
#    0.62-0.69 against torch 0.50-0.51 and one segment 1.41-1.48 against 0.46-0.59 (both take the long route); and
#    against ops.sort(dim=-1) on the same equal-length data the front end costs 1.5x-3.7x (eleven more launches and the
#    read-back on a 0.04-0.08 ms sort).
SEGSORT_MAX_LEN = ROWSORT_MAX_COLS    # csrc/include/pcmx_hip.h PCMX_SEGSORT_MAX_LEN: one block's LDS
SEGSORT_CLASS_LIMITS = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)  # segsort.hip: the capacity of every class
SEGSORT_WAVE_CLASSES = 4              # the first four classes put 4 segments into a block (one wave each), the rest one
SEGSORT_GRID_MULT = 8                 # segsort.hip kGridMult: blocks per compute unit of a class launch; not measured
SEGSORT_MAX_S = (1 << 30) - 1
_SEGSORT_ROUTES = (None, "classes", "global")


def _segment_ids(offsets: torch.Tensor, n: int) -> torch.Tensor:
    """int64 [n]: 0 before offsets[0], j + 1 inside segment j, S + 1 from offsets[S] on (offsets clamped to [0, n])."""
    o = offsets.long().clamp(0, n)
    return torch.searchsorted(o, torch.arange(n, device=offsets.device), right=True)


def _check_segsort(keys, values, offsets, mode, bits, validate, max_len, route, name: str):
    """(compared bits, S) after every argument check of the four ops."""
    nbits = _check_sort_keys(keys, bits, "keys" if mode == "pairs" else "x")
    if offsets.numel() - 1 > SEGSORT_MAX_S:
        raise ValueError(f"{name}: {offsets.numel() - 1} segments; at most 2^30 - 1")
    s = _check_segments(keys, offsets, "sum", name)
    if mode == "pairs":
        if values.dtype not in (torch.float32, torch.int32):
            raise TypeError(f"{name}: values must be float32 or int32, got {values.dtype}")
        if values.shape != keys.shape:
            raise ValueError(f"{name}: values must have the keys' shape {tuple(keys.shape)}, got {tuple(values.shape)}")
        if values.device != keys.device:
            raise ValueError(f"{name}: values are on {values.device}, the keys on {keys.device}")
        if not values.is_contiguous():
            raise ValueError(f"{name}: values must be contiguous")
    if route not in _SEGSORT_ROUTES:
        raise ValueError(f"{name}: route must be one of {_SEGSORT_ROUTES}, got {route!r}")
    if max_len is not None:
        if isinstance(max_len, bool) or not isinstance(max_len, int):
            raise TypeError(f"{name}: max_len must be an int or None, got {type(max_len).__name__}")
        if max_len < 0:
            raise ValueError(f"{name}: max_len must not be negative, got {max_len}")
    if validate:
        _validate_offsets(offsets, keys.numel())
        if max_len is not None and s > 0:
            lens = offsets[1:].long() - offsets[:-1].long()
            j = int(torch.argmax(lens))
            if int(lens[j]) > max_len:
                raise ValueError(f"{name}: segment {j} has {int(lens[j])} keys, more than max_len = {max_len}")
    return nbits, s


def _segsort_by_ids(pk: torch.Tensor, sid: torch.Tensor, groups: int, descending: bool, nbits: int, want_keys: bool,
                    want_perm: bool):
    """(sorted keys or None, int32 permutation or None) of the packed keys pk sorted inside the groups that the
    non-decreasing int32 ids sid (< groups) give, with the device-wide kernels: one stable index sort of all keys, then
    a stable pair sort by group id per wanted stream (skipped for one group)."""
    ks, perm = ops().sort_index(pk, descending, 0, nbits, True)
    if groups > 1:
        gid = sid[perm.long()]
        gbits = (groups - 1).bit_length()
        if want_keys:
            ks = ops().sort_pairs(gid, ks, False, 0, gbits)[1]
        if want_perm:
            perm = ops().sort_pairs(gid, perm, False, 0, gbits)[1]
    return (ks if want_keys else None), (perm if want_perm else None)


def _segsort_long(xf, vf, offsets, ko, po, mode: str, descending: bool, nbits: int, n_long: int, long_keys: int) -> None:
    """Sorts the n_long segments above SEGSORT_MAX_LEN (long_keys keys together, both from the kernel's summary) into
    the outputs ko / po, which the class kernels left unwritten there."""
    n, dev = xf.numel(), xf.device
    o = offsets.long().clamp(0, n)
    lens = (o[1:] - o[:-1]).clamp(min=0)
    ids = torch.nonzero(lens > SEGSORT_MAX_LEN).view(-1)[:n_long]
    ll, starts = lens[ids], o[:-1][ids]
    rank = torch.repeat_interleave(torch.arange(ids.numel(), device=dev), ll, output_size=long_keys)
    src = starts[rank] + (torch.arange(long_keys, device=dev) - (torch.cumsum(ll, 0) - ll)[rank])  # < n
    pk = xf.view(torch.int32)[src].view(xf.dtype)
    ks, perm = _segsort_by_ids(pk, rank.int(), n_long, descending, nbits, ko is not None, po is not None)
    if ko is not None:
        ko.view(torch.int32)[src] = ks.view(torch.int32)
    if po is not None:
        flat = src[perm.long()]
        po.view(torch.int32)[src] = vf.view(torch.int32)[flat] if mode == "pairs" else flat.int()


def _segsort_gpu(xf, vf, offsets, mode: str, descending: bool, nbits: int, max_len, route, grid_mult: int = 0):
    """(keys or None, payload or None), flat, of the segment sort of xf on the GPU."""
    n, s = xf.numel(), offsets.numel() - 1
    want_keys, want_payload = mode != "argsort", mode != "keys"
    if route == "global":
        sid = _segment_ids(offsets, n)
        inside = (sid >= 1) & (sid <= s)
        ks, perm = _segsort_by_ids(xf, sid.int(), s + 2, descending, nbits, want_keys, want_payload)
        ko = po = None
        if want_keys:  # the groups 0 and S + 1 lie where they were: put their elements back as they came
            ko = torch.where(inside, ks.view(torch.int32), xf.view(torch.int32)).view(xf.dtype)
        if want_payload:
            perm = torch.where(inside, perm, torch.arange(n, device=xf.device, dtype=torch.int32))
            po = vf.view(torch.int32)[perm.long()].view(vf.dtype) if mode == "pairs" else perm
        return ko, po
    code = {"keys": _MODE_KEYS, "pairs": _MODE_PAIRS}.get(mode, _MODE_INDEX) | (int(grid_mult) << 8)
    ko, po, summary = ops().segment_sort(xf, vf, offsets, code, descending, 0, nbits, want_keys)
    ko, po = (ko if want_keys else None), (po if want_payload else None)
    if max_len is not None and max_len <= SEGSORT_MAX_LEN:
        return ko, po
    n_long, long_keys, longest, _ = summary.tolist()  # the one host sync: 16 bytes
    if n_long:
        if route == "classes":
            raise ValueError(f"segment sort: route 'classes' takes segments of at most {SEGSORT_MAX_LEN} keys; {n_long} "
                             f"are longer, the longest has {longest}")
        _segsort_long(xf, vf, offsets, ko, po, mode, descending, nbits, n_long, long_keys)
    return ko, po


def _segsort_host(xf, vf, offsets, mode: str, descending: bool, nbits: int, route):
    n, s = xf.numel(), offsets.numel() - 1
    if route == "classes" and s > 0:
        o = offsets.long().clamp(0, n)
        longest = int((o[1:] - o[:-1]).max())
        if longest > SEGSORT_MAX_LEN:
            raise ValueError(f"segment sort: route 'classes' takes segments of at most {SEGSORT_MAX_LEN} keys; the longest "
                             f"has {longest}")
    sid = _segment_ids(offsets, n)
    inside = (sid >= 1) & (sid <= s)
    order = _host_order(xf, descending, nbits)
    order = order[torch.sort(sid[order], stable=True).indices]
    order = torch.where(inside, order, torch.arange(n))
    xb = xf.view(torch.int32)
    ko = None if mode == "argsort" else torch.where(inside, _canonical_f32(xb[order].view(xf.dtype)).view(torch.int32),
                                                    xb).view(xf.dtype)
    po = None if mode == "keys" else (vf.view(torch.int32)[order].view(vf.dtype) if mode == "pairs" else order.int())
    return ko, po


def _segment_sort(keys, values, offsets, mode, descending, bits, validate, max_len, route, name, grid_mult=0):
    nbits, _ = _check_segsort(keys, values, offsets, mode, bits, validate, max_len, route, name)
    xf = keys.view(-1)
    vf = values.view(-1) if mode == "pairs" else None
    if xf.numel() == 0:
        ko = None if mode == "argsort" else xf.clone()
        po = None if mode == "keys" else (vf.clone() if mode == "pairs" else xf.new_empty(0, dtype=torch.int32))
    elif keys.is_cuda:
        ko, po = _segsort_gpu(xf, vf, offsets, mode, bool(descending), nbits, max_len, route, grid_mult)
    else:
        ko, po = _segsort_host(xf, vf, offsets, mode, bool(descending), nbits, route)
    return (None if ko is None else ko.view(keys.shape)), (None if po is None else po.view(keys.shape))


def segment_sort_keys(x: torch.Tensor, offsets: torch.Tensor, descending: bool = False, bits: int | None = None,
                      validate: bool = False, max_len: int | None = None, route: str | None = None) -> torch.Tensor:
    """x (float32 or int32, contiguous, read flattened) with every segment x.flatten()[offsets[j] : offsets[j+1]] sorted
    on its own, in x's shape: each segment equals sort_keys of that slice bit for bit (rules above). Elements outside
    [offsets[0], offsets[S]) come through unchanged. x is never modified. One host sync of 16 bytes (is any segment
    above SEGSORT_MAX_LEN?) unless max_len <= SEGSORT_MAX_LEN promises there is none: then the call does not
    synchronise, and a segment that breaks the promise gets an unspecified result inside its own range."""
    return _segment_sort(x, None, offsets, "keys", descending, bits, validate, max_len, route, "segment_sort_keys")[0]


def segment_sort(x: torch.Tensor, offsets: torch.Tensor, descending: bool = False, bits: int | None = None,
                 validate: bool = False, max_len: int | None = None, route: str | None = None):
    """(values, indices) in x's shape: segment_sort_keys(x, offsets) and the FLAT int32 index into x.flatten() of every
    output element, so indices[b:e] - b is the stable argsort of the slice; outside [offsets[0], offsets[S]) the index
    is the element's own position. Host syncs and max_len as for segment_sort_keys (one sync of 16 bytes; none with
    max_len <= SEGSORT_MAX_LEN, a broken promise giving an unspecified result in bounds)."""
    return _segment_sort(x, None, offsets, "index", descending, bits, validate, max_len, route, "segment_sort")


def segment_argsort(x: torch.Tensor, offsets: torch.Tensor, descending: bool = False, bits: int | None = None,
                    validate: bool = False, max_len: int | None = None, route: str | None = None) -> torch.Tensor:
    """The indices of segment_sort alone; no sorted-keys tensor is written. Host syncs and max_len as for
    segment_sort_keys (one sync of 16 bytes; none with max_len <= SEGSORT_MAX_LEN, a broken promise giving an
    unspecified result in bounds)."""
    return _segment_sort(x, None, offsets, "argsort", descending, bits, validate, max_len, route, "segment_argsort")[1]


def segment_sort_by_key(keys: torch.Tensor, values: torch.Tensor, offsets: torch.Tensor, descending: bool = False,
                        bits: int | None = None, validate: bool = False, max_len: int | None = None,
                        route: str | None = None):
    """(keys_sorted, values_sorted) in the keys' shape: values (float32 or int32, the keys' shape and device, contiguous,
    moved as bits) reordered with their keys inside every segment; sort_by_key of every slice, bit for bit. Host syncs
    and max_len as for segment_sort_keys (one sync of 16 bytes; none with max_len <= SEGSORT_MAX_LEN, a broken promise
    giving an unspecified result in bounds)."""
    return _segment_sort(keys, values, offsets, "pairs", descending, bits, validate, max_len, route, "segment_sort_by_key")


# ---------------------------------------------------------------------------------------------------------------------
# argmin / argmax: flat, along a dimension and over ragged segments (csrc/kernels/argreduce.hip; no counterpart in the
# reference programs). One rule for all forms, float32 and int32:
#  1. a NaN beats every number, for max AND min: torch's rule for argmax / argmin / max(dim) / min(dim) and the rule of
#     reduce(dim=). It is NOT the rule of the flat reduce(x, "max"), which skips NaNs;
#  2. otherwise the numerically largest (smallest) element wins; -0.0 and +0.0 are equal;
#  3. among equal winners, and among several NaNs, the lowest position wins;
#  4. the value returned is the input element at the returned position, bit for bit (the sign of a zero, a NaN's
#     payload).
# Indices are int32. On the GPU the element of the reduction is the (ordered key, ~position) pair packed into 64 bits
# under an unsigned max: associative and commutative, so the result depends on the data only, never on the route, the
# chunk, the grid, the row's place in the tensor or timing, and every result can be tested for equality.
#  * flat: two launches, each element read once (ARG_BLOCK elements per block and trip, at most ARG_MAX_BLOCKS blocks).
#  * dim=: the reduce halves of the routes of reduce(dim=) under the same names, with 8-byte partials. The default
#    route is _axis_route("reduce", ...) unchanged: those borders were measured for 4-byte reductions and are NOT
#    MEASURED for pairs.
#  * segments: the merge-path tiles, carry scan and fix-up of segment_reduce (RAGGED_TILE path steps per block).
# Nothing synchronises.
#  * Measured on one MI355X (scripts/argreduce_lab.py, profiles/r23_argreduce/README.md; op max, median ms). Flat at 2^28
#    float32: 0.181 against torch.argmax 0.423, topk(x, 1) 1.325 (the route until now), reduce(x, "max") 0.163 and copy_
#    of the same bytes 0.175. Along a dimension, ours / torch.max(x, dim): [2^20, 32] 0.053 / 0.203, [8, 2^24] 0.120 /
#    5.90, [2^20, 64] along dim 0 0.102 / 0.228; 0.57x-0.97x of reduce(dim=). SLOWER than torch on the block route:
#    [16384, 4096] 0.071 against 0.055 ms, [1024, 32768] 0.036 against 0.031, int32 [64, 1024, 1024] along dim 1 0.078
#    against 0.065. Segments at 2^28: 0.46-0.55 ms from one segment to mean length 100, 0.81 / 1.45 ms at length 4 / 1:
#    SLOWER than segment_reduce(x, offsets, "max") in every case (0.81x-0.87x), 2.2x-3.1x the copy floor.
ARG_OPS = ("min", "max")
ARG_BLOCK = 4096          # csrc/kernels/argreduce.hip: elements per block and grid-stride trip of the flat first pass
ARG_MAX_BLOCKS = 16384    # ... and the cap of its grid


def _check_arg(x: torch.Tensor, op, name: str) -> None:
    if op not in ARG_OPS:
        raise ValueError(f"{name}: op must be 'min' or 'max', got {op!r}")
    if x.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"{name}: x must be float32 or int32, got {x.dtype}")
    if x.numel() >= 1 << 31:
        raise ValueError(f"{name}: x has {x.numel()} elements; indices are int32 (fewer than 2^31)")


def _arg_key(x: torch.Tensor, op: str) -> torch.Tensor:
    """int64 keys whose order is the rule's: radix_key.h's ordered key (-0.0 == +0.0, every NaN one key above +inf),
    flipped for min with the NaN key kept on top. The host path's statement of rules 1 and 2."""
    b = x.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    nan = None
    if x.dtype == torch.float32:
        a = b & 0x7FFFFFFF
        nan = a > 0x7F800000
        k = torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)
        k = torch.where(a == 0, torch.full_like(k, 0x80000000), k)
        k = torch.where(nan, torch.full_like(k, 0xFFFFFFFF), k)
    else:
        k = b ^ 0x80000000
    if op == "min":
        k = 0xFFFFFFFF - k
        if nan is not None:
            k = torch.where(nan, torch.full_like(k, 0xFFFFFFFF), k)
    return k


def _arg_identity(dtype: torch.dtype, op: str):
    return _SCAN_IDENTITY[op][0 if dtype == torch.float32 else 1]


def _host_axis_arg(x3: torch.Tensor, op: str):
    """(values, int32 positions along n) of the [outer, n, inner] tensor on the host: the first position of the extreme
    key, the value gathered as bits."""
    n = x3.shape[1]
    key = _arg_key(x3, op)
    pos = torch.arange(n).view(1, n, 1)
    idx = torch.where(key == key.amax(1, keepdim=True), pos, n).amin(1)
    vals = x3.contiguous().view(torch.int32).gather(1, idx.unsqueeze(1)).squeeze(1).view(x3.dtype)
    return vals, idx.int()


def _host_segment_arg(xf: torch.Tensor, offsets: torch.Tensor, op: str):
    n, s = xf.numel(), offsets.numel() - 1
    vals = torch.full((s,), _arg_identity(xf.dtype, op), dtype=xf.dtype)
    idx = torch.full((s,), -1, dtype=torch.int32)
    if s == 0 or n == 0:
        return vals, idx
    o = offsets.long()
    lo, hi = int(o[0]), int(o[-1])
    if hi <= lo:
        return vals, idx
    pos = torch.arange(lo, hi)
    ids = torch.searchsorted(o[1:].contiguous(), pos, right=True)
    key = _arg_key(xf[lo:hi], op)
    top = torch.full((s,), -1, dtype=torch.int64).scatter_reduce(0, ids, key, "amax", include_self=True)
    first = torch.full((s,), n, dtype=torch.int64).scatter_reduce(0, ids, torch.where(key == top[ids], pos, n), "amin",
                                                                  include_self=True)
    hit = first < n
    idx[hit] = first[hit].int()
    vb = vals.view(torch.int32)
    vb[hit] = xf.view(torch.int32)[first[hit]]
    return vals, idx


def _arg_reduce(x: torch.Tensor, op, dim, keepdim, route, chunk, want_values: bool, want_indices: bool, name: str):
    _check_arg(x, op, name)
    if dim is None:
        if keepdim or route is not None or chunk is not None:
            raise ValueError(f"{name}: keepdim, route and chunk are for the form along a dimension: they need dim=")
        if x.numel() == 0:
            raise ValueError(f"{name}: an empty tensor has no extremum")
        if x.is_cuda:
            v, i = ops().arg_reduce(x, OP_CODES[op], want_values, want_indices)
        else:
            v, i = _host_axis_arg(x.reshape(1, -1, 1), op)
            v, i = v.reshape(()), i.reshape(())
        return (v if want_values else None), (i if want_indices else None)
    outer, n, inner, d = _axis_view(x, dim, op, name)
    if n == 0:
        raise ValueError(f"{name}: dimension {d} has size 0: no extremum")
    code, chunk = _axis_plan("reduce", route, chunk, outer, n, inner, name)  # borders NOT MEASURED for 8-byte pairs
    x3 = x.contiguous().view(outer, n, inner)
    if x.is_cuda:
        v, i = ops().axis_arg_reduce(x3, OP_CODES[op], code, chunk, want_values, want_indices)
    else:
        v, i = _host_axis_arg(x3, op)
    shape = list(x.shape)
    shape[d:d + 1] = [1] if keepdim else []
    return (v.reshape(shape) if want_values else None), (i.reshape(shape) if want_indices else None)


def arg_reduce(x: torch.Tensor, op: str, dim: int | None = None, keepdim: bool = False, route: str | None = None,
               chunk: int | None = None):
    """(values, indices) of the extremum of a float32 / int32 tensor, op "max" or "min"; indices are int32.
    dim=None: 0-d tensors, the index into the row-major flattened tensor. dim=int: torch.max(x, dim, keepdim)'s shapes,
    the position along dim; route and chunk as for reduce(dim=) (the default route is that of a reduce: its borders are
    not measured for the 8-byte partials used here).

    A NaN beats every number under BOTH ops (torch.argmax / argmin / max(dim) / min(dim), and reduce(dim=); not the
    NaN-skipping rule of the flat reduce(x, "max")); -0.0 == +0.0; among equal winners and among NaNs the lowest
    position wins; the value is the input element at that position, bit for bit. The result depends on the data only,
    never on the route, the chunk or timing. Any view is accepted (strided or misaligned input is copied first; the
    input is never written). ValueError: another op, an empty tensor or dimension, keepdim / route / chunk without
    dim, a route or chunk that does not fit; TypeError: another dtype. Does not synchronise."""
    return _arg_reduce(x, op, dim, keepdim, route, chunk, True, True, "arg_reduce")


def argmax(x: torch.Tensor, dim: int | None = None, keepdim: bool = False) -> torch.Tensor:
    """The indices of arg_reduce(x, "max", dim, keepdim) alone (int32; torch.argmax's positions, NaN first); no value
    is written."""
    return _arg_reduce(x, "max", dim, keepdim, None, None, False, True, "argmax")[1]


def argmin(x: torch.Tensor, dim: int | None = None, keepdim: bool = False) -> torch.Tensor:
    """The indices of arg_reduce(x, "min", dim, keepdim) alone (int32; torch.argmin's positions: a NaN beats every
    number here too); no value is written."""
    return _arg_reduce(x, "min", dim, keepdim, None, None, False, True, "argmin")[1]


def _segment_arg(x: torch.Tensor, offsets: torch.Tensor, op, validate, want_values: bool, want_indices: bool, name: str):
    _check_arg(x, op, name)
    xc = x.contiguous()
    _check_segments(xc, offsets, op, name)
    if validate:
        _validate_offsets(offsets, xc.numel())
    if x.is_cuda:
        v, i = ops().segment_arg_reduce(xc, offsets, OP_CODES[op], want_values, want_indices, None, None)
    else:
        v, i = _host_segment_arg(xc.reshape(-1), offsets, op)
    return (v if want_values else None), (i if want_indices else None)


def segment_arg_reduce(x: torch.Tensor, offsets: torch.Tensor, op: str, validate: bool = False):
    """(values, indices), both [S]: the extremum (op "max" or "min", the rule of arg_reduce: NaN beats every number,
    -0.0 == +0.0, the lowest position wins ties, the value bit for bit) of every segment x.flatten()[offsets[j] :
    offsets[j+1]], S = offsets.numel() - 1. indices are int32 FLAT positions in x.flatten() (the convention of
    segment_sort: offsets[j] <= indices[j] < offsets[j+1]); an empty segment gives -1 and the identity as its value
    (-inf / INT32_MIN for max, +inf / INT32_MAX for min, as segment_reduce). offsets as for segment_reduce: int32, 1-D,
    contiguous, on x's device, 0 <= offsets[0] <= ... <= offsets[S] <= x.numel(), not checked unless validate=True (one
    host sync; ValueError naming the first offending entry); offsets that break it give an unspecified result and
    touch nothing outside the tensors. Any view of x is accepted; x is never written. Does not synchronise."""
    return _segment_arg(x, offsets, op, validate, True, True, "segment_arg_reduce")


def segment_argmax(x: torch.Tensor, offsets: torch.Tensor, validate: bool = False) -> torch.Tensor:
    """The indices of segment_arg_reduce(x, offsets, "max") alone; no value is written."""
    return _segment_arg(x, offsets, "max", validate, False, True, "segment_argmax")[1]


def segment_argmin(x: torch.Tensor, offsets: torch.Tensor, validate: bool = False) -> torch.Tensor:
    """The indices of segment_arg_reduce(x, offsets, "min") alone; no value is written."""
    return _segment_arg(x, offsets, "min", validate, False, True, "segment_argmin")[1]
