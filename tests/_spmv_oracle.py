"""Operand families, matrix builders, a CPU model of the sliced layout and assertion functions for the SpMV tests
(torch only, no GPU).

The GPU tests (test_gpu_spmv.py) call the assertion functions on kernel output; test_spmv_oracle_cpu.py calls the same
functions on `layout_product` (a CPU walk over the arrays the gfx950 kernels read) and on eleven mutants of it, which
is the proof that they discriminate.

Operand families
  integer_operands       val in +-{1, 2, 3}, x in +-{1..7}: every product is a nonzero integer of magnitude <= 21, and
                         while a row's sum|v x| < 2^24 every partial sum in every summation order is exact in fp32
                         (rows up to ~798k nonzeros). `exact_product` asserts the condition per matrix. One dropped,
                         doubled or mis-slotted product changes an integer: `assert_exact` leaves no slack.
  full_mantissa_operands signed values with all 24 mantissa bits in use, for `assert_within_any_order_bound`: the fp64
                         product and the bound k u / (1 - k u) * sum|v x| (u = 2^-24, k the row's length) — one
                         rounding per product plus at most k - 1 additions on any path through any summation tree,
                         fused multiply-add or not, partials + combine + fix-up alike.

Every generator is seeded and returns CPU tensors; the GPU tests move them with `.to(device)`.
"""
from __future__ import annotations

import functools

import torch

from parallel_c_programs_amd import ops

U = 2.0 ** -24  # unit roundoff of f32
PACK_COL_MASK, PACK_HEAD_BIT, PACK_ROW_SHIFT = 0x1FFFFF, 21, 22  # spmv.hip: kPackColMask, kPackHead, kPackRowShift
STRIPE_PATTERN = (63, 1, 64, 64, 1, 127, 129, 150, 2, 62)


# ------------------------------------------------------------------------------------------ operands
def _signs(shape, g):
    return torch.randint(0, 2, shape, generator=g) * 2 - 1


def integer_operands(nnz: int, n_cols: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    val = (torch.randint(1, 4, (nnz,), generator=g) * _signs((nnz,), g)).float()
    x = (torch.randint(1, 8, (n_cols,), generator=g) * _signs((n_cols,), g)).float()
    return val, x


def full_mantissa_operands(nnz: int, n_cols: int, seed: int):
    """Signed floats of magnitude in [0.5, 1.5) drawn at full f32 resolution (the low mantissa bits are in use)."""
    g = torch.Generator().manual_seed(seed)
    val = ((torch.rand(nnz, dtype=torch.float64, generator=g) + 0.5) * _signs((nnz,), g)).float()
    x = ((torch.rand(n_cols, dtype=torch.float64, generator=g) + 0.5) * _signs((n_cols,), g)).float()
    return val, x


def with_values(m: ops.CSR, val: torch.Tensor) -> ops.CSR:
    assert val.shape == m.val.shape and val.dtype == torch.float32
    return ops.CSR(m.row_ptr, m.col, val, m.n_cols)


def row_lengths(m: ops.CSR) -> torch.Tensor:
    return (m.row_ptr[1:] - m.row_ptr[:-1]).cpu()


def rows_of(m: ops.CSR) -> torch.Tensor:
    return torch.repeat_interleave(torch.arange(m.n_rows), row_lengths(m))


# ------------------------------------------------------------------------------------------ references and assertions
def exact_product(m: ops.CSR, x: torch.Tensor) -> torch.Tensor:
    """The int64 row sums of an integer-valued matrix and vector (index_add_ on the CPU)."""
    val, x = m.val.cpu(), x.cpu()
    assert torch.equal(val, val.round()) and torch.equal(x, x.round()), "integer family only"
    rows = rows_of(m)
    prod = val.long() * x.long()[m.col.cpu().long()]
    absrow = torch.zeros(m.n_rows, dtype=torch.int64).index_add_(0, rows, prod.abs())
    # every partial sum of every summation order is an integer of magnitude < 2^24: exact in fp32
    assert m.n_rows == 0 or int(absrow.max()) < 2 ** 24, "a row's sum|v x| reaches 2^24: fp32 sums are no longer exact"
    return torch.zeros(m.n_rows, dtype=torch.int64).index_add_(0, rows, prod)


def assert_exact(out: torch.Tensor, m: ops.CSR, x: torch.Tensor) -> None:
    exact = exact_product(m, x).double()
    got = out.detach().cpu().double()
    assert got.shape == exact.shape, (tuple(got.shape), tuple(exact.shape))
    if torch.equal(got, exact):
        return
    bad = torch.nonzero(~(got == exact)).flatten()  # (~(==): a NaN is wrong too)
    r = int(bad[0])
    msg = (f"{bad.numel()} of {m.n_rows} rows wrong; first row {r} ({int(row_lengths(m)[r])} nonzeros): got {got[r].item()}, "
           f"exact {exact[r].item()}, difference {(got[r] - exact[r]).item()}")
    print(msg)
    raise AssertionError(msg)


def any_order_bound(m: ops.CSR, x: torch.Tensor):
    """(fp64 product, per-row bound k u / (1 - k u) * sum|v x|)."""
    rows = rows_of(m)
    prod = m.val.cpu().double() * x.cpu().double()[m.col.cpu().long()]  # (exact: 24 x 24 bits)
    ref = torch.zeros(m.n_rows, dtype=torch.float64).index_add_(0, rows, prod)
    absrow = torch.zeros(m.n_rows, dtype=torch.float64).index_add_(0, rows, prod.abs())
    ku = row_lengths(m).double() * U
    return ref, ku / (1 - ku) * absrow


def assert_within_any_order_bound(out: torch.Tensor, m: ops.CSR, x: torch.Tensor) -> float:
    """Every row within the any-order bound of the fp64 product (an empty row must be exactly 0). Returns the worst
    err / bound, which the caller prints."""
    ref, bound = any_order_bound(m, x)
    got = out.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    ok = err <= bound  # (a NaN compares false)
    if not bool(ok.all()):
        r = int(torch.nonzero(~ok).flatten()[0])
        msg = (f"{int((~ok).sum())} of {m.n_rows} rows outside the any-order bound; first row {r} "
               f"({int(row_lengths(m)[r])} nonzeros): got {got[r].item()!r}, fp64 {ref[r].item()!r}, error "
               f"{err[r].item():.3e}, bound {bound[r].item():.3e}; worst err / bound {worst:.3f}")
        print(msg)
        raise AssertionError(msg)
    return worst


def worst_ratio(out: torch.Tensor, m: ops.CSR, x: torch.Tensor, min_len: int) -> float:
    """Worst err / bound over the rows of at least min_len nonzeros (a figure to print: on a one-nonzero row the bound
    is the product's own rounding, so the overall worst sits near 1 whatever the kernel does)."""
    ref, bound = any_order_bound(m, x)
    sel = (row_lengths(m) >= min_len) & (bound > 0)
    err = (out.detach().cpu().double() - ref).abs()
    return float((err[sel] / bound[sel]).max()) if bool(sel.any()) else 0.0


def probe_columns(s) -> list:
    """The columns at which a SlicedCSR's column decode changes: the first and last column, both sides of every slice's
    first tail column, of the head boundary and of the column split."""
    cols = {0, s.n_cols - 1, s.head_cols - 1, s.head_cols, s.col_split - 1, s.col_split}
    for b in s.colbase:
        cols |= {int(b), int(b) - 1}
    return sorted(c for c in cols if 0 <= c < s.n_cols)


# ------------------------------------------------------------------------------------------ matrix builders
def _csr(n_rows: int, n_cols: int, rows: torch.Tensor, cols: torch.Tensor, seed: int) -> ops.CSR:
    """CSR of the (row, column) pairs, the rows' entries kept in the given order; integer-family values."""
    order = torch.sort(rows, stable=True).indices
    rp = torch.zeros(n_rows + 1, dtype=torch.int64)
    rp[1:] = torch.bincount(rows, minlength=n_rows).cumsum(0)
    val, _ = integer_operands(rows.numel(), 1, seed)
    return ops.CSR(rp, cols[order].to(torch.int32).contiguous(), val, n_cols)


def _draw(lens, lo: int, hi: int, g, unique: bool = True):
    """One (rows, cols) pair list: row i gets lens[i] columns of [lo, hi), distinct unless `unique` is off."""
    rows, cols = [], []
    for i, k in enumerate(lens):
        if k == 0:
            continue
        c = (torch.randperm(hi - lo, generator=g)[:k] if unique else torch.randint(0, hi - lo, (k,), generator=g)) + lo
        assert c.numel() == k
        rows.append(torch.full((k,), i, dtype=torch.int64))
        cols.append(c)
    return torch.cat(rows), torch.cat(cols)


@functools.lru_cache(maxsize=None)
def csr_item_edges() -> ops.CSR:
    """Aimed at the plain-CSR planner's cuts (pcmx_spmv_csr_plan_nnz) and the kernel's lanes-per-row rule: rows of
    exactly / one past the item size and its multiples, a run of empty rows and a run of one-nonzero rows that each
    cross the 1023-rows-per-item cap, empty first and last rows, and blocks of equal rows of length 2, 6, 12, 24, 48, 96,
    200 and 500 (40 rows, or as many as fill three items: 40 rows of 6 nonzeros would share one item with their
    neighbours) whose items' average row length falls in every class of L = 1, 2, 4, ..., 64. About 58k nonzeros,
    columns distinct inside a row."""
    lens = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3073] + [0] * 1100 + [1] * 1100
    for k in (2, 6, 12, 24, 48, 96, 200, 500):
        lens += [k] * max(40, 3 * 1024 // k)  # at least one 1024-nonzero item of these rows alone
    lens += [0]
    g = torch.Generator().manual_seed(101)
    rows, cols = _draw(lens, 0, 5003, g)
    m = _csr(len(lens), 5003, rows, cols, 102)
    assert m.nnz < 150_000
    return m


@functools.lru_cache(maxsize=None)
def sliced_stripe_edges(item_nnz: int) -> ops.CSR:
    """Aimed at sliced_step's stripe logic and the combine (2517 rows: not a multiple of 64, more than one 2048-row
    combine block group; 4100 columns). In row order:
      * 10 empty rows;
      * 1100 rows with one nonzero each, all in the LAST column (one column is never cut, so one slice holds the run
        and, being the first rows that slice touches, its first item starts on the run: an item of min(item_nnz, 1023)
        rows, row offsets up to that minus one);
      * 24 column windows of 160 columns, each with its own 50 consecutive rows of lengths STRIPE_PATTERN x 5 inside
        the window: a slice that holds a whole window (more windows than most slice counts have cuts there) sees
        consecutive touched rows of exactly these lengths — a row ending on lane 63, rows starting on lane 0, rows
        over two and three stripes, inside multi-row items. 663 nonzeros per repeat, so each repeat meets the stripes
        at another phase;
      * empty rows, then, past row 2048, rows of item_nnz + 1, 2 item_nnz and 2 item_nnz + 1 nonzeros in 250 columns
        (REPEATED columns: the one builder whose rows hold a column more than once), so a slice holds more than
        item_nnz nonzeros of one row and there are fix-up entries;
      * 6 rows with a nonzero in every 4th column (all slices touch them), and empty rows to the end."""
    assert item_nnz in (256, 384, 512, 1024)
    g = torch.Generator().manual_seed(200 + item_nnz)
    n_cols, n_rows = 4100, 2517
    R, C, r = [], [], 10
    R.append(torch.arange(r, r + 1100)), C.append(torch.full((1100,), n_cols - 1, dtype=torch.int64))
    r += 1100
    for w in range(24):
        a, b = _draw(STRIPE_PATTERN * 5, 160 * w, 160 * w + 160, g)
        R.append(a + r), C.append(b)
        r += 50
    assert r == 2310
    r = 2440
    a, b = _draw((item_nnz + 1, 2 * item_nnz, 2 * item_nnz + 1), 3840, 4090, g, unique=False)
    R.append(a + r), C.append(b)
    r += 3
    for i in range(6):
        c = torch.arange(i % 4, n_cols, 4)
        R.append(torch.full((c.numel(),), r + i, dtype=torch.int64)), C.append(c)
    return _csr(n_rows, n_cols, torch.cat(R), torch.cat(C), 300 + item_nnz)


@functools.lru_cache(maxsize=None)
def few_columns() -> ops.CSR:
    """All nonzeros in 3 of 1000 columns: most slices are empty (their waves take the `it >= i1` early return)."""
    g = torch.Generator().manual_seed(401)
    n_rows, picks = 333, torch.tensor([5, 500, 999])
    on = torch.rand(n_rows, 3, generator=g) < 0.6
    rc = torch.nonzero(on)
    return _csr(n_rows, 1000, rc[:, 0], picks[rc[:, 1]], 402)


@functools.lru_cache(maxsize=None)
def empty_matrix() -> ops.CSR:
    return _csr(130, 70, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 403)


@functools.lru_cache(maxsize=None)
def one_row() -> ops.CSR:
    """One row of 9000 nonzeros over 12000 columns: with 8 slices every slice holds more than 1024 of them, so the row
    is split into several items per slice (fix entries at every item size)."""
    g = torch.Generator().manual_seed(404)
    rows, cols = _draw([9000], 0, 12000, g)
    return _csr(1, 12000, rows, cols, 405)


WIDE_COLS = 4_200_000


@functools.lru_cache(maxsize=None)
def wide_matrix() -> ops.CSR:
    """2000 rows over 4.2e6 columns, columns distinct inside a row: ~92% of the ~200k nonzeros in the first 2.7e6
    columns, the rest spread thinly over the last 1.5e6, so with 8 slices the last one is wider than 2^20 columns (and
    under the packed word's 2^21): bit 20 of the column offset, next to the head flag, is in use."""
    g = torch.Generator().manual_seed(501)
    n_rows, nnz = 2000, 200_000
    rows = torch.randint(0, n_rows, (nnz,), generator=g)
    low = torch.rand(nnz, generator=g) < 0.92
    cols = torch.where(low, torch.randint(0, 2_700_000, (nnz,), generator=g),
                       torch.randint(2_700_000, WIDE_COLS, (nnz,), generator=g))
    key = torch.unique(rows * WIDE_COLS + cols)  # sorted: row-major, columns ascending and distinct in a row
    return _csr(n_rows, WIDE_COLS, key // WIDE_COLS, key % WIDE_COLS, 502)


# Banded geometries (a, b, c, d, e) by the nonzeros of an unclipped row, L = 2 (a // 2) + 1 + 2 c + 2 e, with the path
# pcmx_spmv_banded_variant must take for variants 1 and 8 on aligned values and enough unclipped rows: (path, NL) with
# path 0 the wave-per-row kernel, 1 spmv_banded_lds_kernel<NL>, 8 the block stream. The stream kernel applies for odd
# L from 257 (L >= 256) to 639 ((16 L + 6) / 16 <= 640 float4s per wave quarter); NL is the next of 2, 4, 6, 8, 10,
# 12, 16 at or above ceil(L / 64), and rows above 16 x 64 nonzeros take the wave-per-row kernel.
BANDED_GEOMETRIES = {
    25: ((9, 3, 5, 2, 3), (1, 2), (1, 2)),
    201: ((101, 5, 40, 5, 10), (1, 4), (1, 4)),
    255: ((201, 5, 20, 5, 7), (1, 4), (1, 4)),        # variant 8 must fall back
    257: ((201, 5, 20, 5, 8), (1, 6), (8, 6)),        # variant 8's lower end
    351: ((201, 5, 60, 5, 15), (1, 6), (8, 6)),
    407: ((301, 10, 50, 10, 3), (1, 8), (8, 8)),
    621: ((401, 200, 100, 200, 10), (1, 10), (8, 10)),
    639: ((401, 5, 100, 5, 19), (1, 10), (8, 10)),    # variant 8's upper end
    641: ((401, 5, 100, 5, 20), (1, 12), (1, 12)),    # ceil(641 / 64) = 11 -> NL 12; variant 8 falls back
    721: ((401, 5, 150, 5, 10), (1, 12), (1, 12)),
    1001: ((601, 5, 150, 5, 50), (1, 16), (1, 16)),
    1801: ((1301, 10, 200, 10, 50), (0, 0), (0, 0)),  # wave per row
}
ALL_BANDED_PATHS = {(0, 0), (8, 6), (8, 8), (8, 10)} | {(1, nl) for nl in (2, 4, 6, 8, 10, 12, 16)}


def banded_reach(a, b, c, d, e) -> int:
    return a // 2 + b + c + d + e


def banded_sizes(geo) -> list:
    """n for a geometry: a few unclipped 16-row blocks between clipped ones with the last block full, one row over
    and one row short, and one n below the reach, where every row is clipped (variant 8 has no block to stream)."""
    reach = banded_reach(*geo)
    return [2 * reach + 48 + r for r in (0, 1, 15)] + [max(1, reach - 3)]


def banded_path(lib, n, geo, variant, aligned=True):
    """(path, NL) from pcmx_spmv_banded_path of the loaded HIP library."""
    import ctypes

    nl = ctypes.c_int(-1)
    path = lib.pcmx_spmv_banded_path(int(n), *map(int, geo), int(variant), int(aligned), ctypes.byref(nl))
    return path, nl.value


# ------------------------------------------------------------------------------------------ CPU model of the layout
def decode(s, head_flag: bool = True, colbase_shift: int = 0, sign_extend_row: bool = False):
    """Per stored nonzero, what the product kernel derives from the arrays it READS: (column, row offset in the item,
    slice). Packed layout: the words s.cr and the colbase entries of s._meta_packed — c = w & 0x1FFFFF, plus
    colbase[slice] unless bit 21 is set; row offset = (w as u32) >> 22. Unpacked: s.col / s.lrow (u16).
    The keyword arguments are the decode mutants of the CPU tests."""
    S = s.n_slices
    slice_nnz = torch.diff(torch.cat([s.meta[:S], torch.tensor([s.nnz])]))
    sid = torch.repeat_interleave(torch.arange(S), slice_nnz)
    if s.cr is None:
        return s.col.cpu().long(), s.lrow.cpu().long() & 0xFFFF, sid
    mp = s._meta_packed
    assert mp.numel() == 4 * S + 2 and torch.equal(mp[:3 * S + 2], s.meta)
    colbase = mp[3 * S + 2:]
    w32 = s.cr.cpu().long()                     # the word as a signed int
    w = w32 & 0xFFFFFFFF                        # ... as the u32 the kernel decodes
    is_head = ((w >> PACK_HEAD_BIT) & 1).bool() if head_flag else torch.zeros_like(w, dtype=torch.bool)
    col = (w & PACK_COL_MASK) + torch.where(is_head, torch.zeros_like(w), colbase[(sid + colbase_shift) % S])
    lrow = (w32 if sign_extend_row else w) >> PACK_ROW_SHIFT
    return col, lrow, sid


def item_index(s):
    """Per stored nonzero: its item and its position inside the item (slice-major storage, items in order)."""
    it = s.items.cpu()
    n = it[:, 2] - it[:, 1]
    item_of = torch.repeat_interleave(torch.arange(it.shape[0]), n)
    S = s.n_slices
    # the items' nonzero ranges are relative to their slice's first nonzero
    start = torch.repeat_interleave(s.meta[:S], torch.diff(s.meta[S:2 * S + 1]))[item_of] + it[item_of, 1]
    pos = torch.arange(s.nnz) - start
    assert s.nnz == 0 or (int(pos.min()) >= 0 and bool((pos < n[item_of]).all()))
    return item_of, pos


def products(s, x: torch.Tensor, col: torch.Tensor) -> torch.Tensor:
    """int64 product of every stored nonzero with the x entry at `col`; a column outside x reads 0, as the gather's
    buffer descriptor does."""
    xi = torch.cat([x.cpu().long(), torch.zeros(1, dtype=torch.int64)])
    inside = (col >= 0) & (col < s.n_cols)
    return s.val.cpu().long() * xi[torch.where(inside, col, torch.full_like(col, s.n_cols))]


def layout_partials(s, x: torch.Tensor, col=None, lrow=None, prod=None):
    """int64 model of spmv_sliced_kernel on integer operands: (comp, extra). Per item the compact partials at
    out0[slice] + r0 + row offset (rows counted among the slice's touched rows); a later piece of a split row
    (row1 == row0) sums into extra[item]. A partial outside the item's rows is dropped, as the store's buffer
    descriptor does. col / lrow / prod replace the decoded arrays (the mutants of the CPU tests)."""
    S, it = s.n_slices, s.items.cpu()
    out0 = s.meta[2 * S + 1:3 * S + 2]
    dcol, dlrow, sid = decode(s)
    lrow = dlrow if lrow is None else lrow
    if prod is None:
        prod = products(s, x, dcol if col is None else col)
    comp = torch.zeros(int(out0[-1]), dtype=torch.int64)
    extra = torch.zeros(it.shape[0], dtype=torch.int64)
    if s.nnz:
        item_of, _ = item_index(s)
        r0, r1 = it[:, 0] & 0xFFFFFFFF, it[:, 0] >> 32
        later = r1[item_of] == r0[item_of]
        nrows = (r1 - r0)[item_of]
        ok = ~later & ((nrows == 1) | ((lrow >= 0) & (lrow < nrows)))  # (a one-row item ignores the row offset)
        tgt = out0[sid] + r0[item_of] + torch.where(nrows == 1, torch.zeros_like(lrow), lrow)
        comp.index_add_(0, tgt[ok], prod[ok])
        extra.index_add_(0, item_of[later], prod[later])
    return comp, extra


def layout_combine(s, comp: torch.Tensor, extra: torch.Tensor, mask=None, chunk_base=None, fix=None) -> torch.Tensor:
    """int64 model of the combine and the fix-up: per row the partials of the slices in its mask (read as u32), slice
    k's at out0[k] + chunk_base[chunk][k] + the row's rank among the chunk's lower rows that slice k touches; then
    y[row] += extra[item] for every fix entry. mask / chunk_base / fix replace the layout's (the mutants)."""
    S, n = s.n_slices, s.n_rows
    out0 = s.meta[2 * S + 1:3 * S + 2]
    n_chunks = (n + 63) // 64
    mask = (s.row_mask.cpu().long() & 0xFFFFFFFF) if mask is None else mask
    cb = s.chunk_base.cpu().long() if chunk_base is None else chunk_base
    assert cb.shape == (n_chunks, S)
    y = torch.zeros(n, dtype=torch.int64)
    padded = torch.cat([comp, torch.zeros(1, dtype=torch.int64)])  # (index numel: an address outside the partials)
    for k in range(S):
        bit = torch.zeros(n_chunks * 64, dtype=torch.int64)
        bit[:n] = (mask >> k) & 1
        rank = (bit.view(n_chunks, 64).cumsum(1) - bit.view(n_chunks, 64) + cb[:, k:k + 1]).flatten()[:n]
        on = bit[:n].bool()
        idx = int(out0[k]) + rank[on]
        y[on] += padded[torch.where((idx >= 0) & (idx < comp.numel()), idx, torch.full_like(idx, comp.numel()))]
    fix = s.fix.cpu().long() if fix is None else fix
    y.index_add_(0, fix[:, 1], extra[fix[:, 0]])
    return y


def layout_product(s, x: torch.Tensor) -> torch.Tensor:
    """The product as the kernels compute it from the arrays they read (int64, integer operands)."""
    return layout_combine(s, *layout_partials(s, x))


def stripe_features(s) -> dict:
    """What of sliced_step's stripe logic a layout exercises, read from the arrays the kernel reads (multi-row items
    only): the largest row offset and rows per item, and the number of rows that end exactly on lane 63 with more of
    the item behind them, start on lane 0 after another row, run over a stripe boundary (a carry), and touch three
    stripes or more."""
    _, lrow, _ = decode(s)
    item_of, pos = item_index(s)
    it = s.items.cpu()
    nrows = ((it[:, 0] >> 32) - (it[:, 0] & 0xFFFFFFFF))
    n = it[:, 2] - it[:, 1]
    multi = nrows[item_of] > 1
    f = dict(max_row_offset=0, max_item_rows=int(nrows.max()) if nrows.numel() else 0, ends_on_lane_63=0,
             starts_on_lane_0=0, carries=0, three_stripes=0, fix_entries=int(s.fix.shape[0]),
             all_slice_rows=int(((s.row_mask.cpu().long() & 0xFFFFFFFF) == (1 << s.n_slices) - 1).sum()))
    if not bool(multi.any()):
        return f
    io, po, lr = item_of[multi], pos[multi], lrow[multi]
    f["max_row_offset"] = int(lr.max())
    key = io * 65536 + lr  # (item, row): constant along a row, rising along the storage order
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = key[1:] != key[:-1]
    last = torch.ones_like(key, dtype=torch.bool)
    last[:-1] = first[1:]
    p_first, p_last = po[first], po[last]
    f["ends_on_lane_63"] = int(((p_last % 64 == 63) & (p_last + 1 < n[io[last]])).sum())
    f["starts_on_lane_0"] = int(((p_first % 64 == 0) & (p_first > 0)).sum())
    f["carries"] = int((p_last // 64 > p_first // 64).sum())
    f["three_stripes"] = int((p_last // 64 - p_first // 64 >= 2).sum())
    return f
