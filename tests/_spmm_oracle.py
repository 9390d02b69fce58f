"""Operand families, references, assertion functions and a CPU model of the kernels' walk for the SpMM tests (torch
only, no GPU). The matrix builders, the value families and U come from tests/_spmv_oracle.py.

The GPU tests (test_gpu_spmm.py) call the assertion functions on kernel output; test_spmm_cpu.py calls the same
functions on `model_product` (a CPU walk over the plan arrays the gfx950 kernels read: items, pieces and their slots,
column tiles, the tail mask, the groups of a narrow class, the fix-up in piece order) and on single-fault mutants of
it, which is the proof that they discriminate.

Operand families for X [n_cols, k]
  integer_x       entries +-{1..7} drawn independently per element: columns differ, so a column mix-up changes an
                  integer. With the matrices' +-{1, 2, 3} values every partial sum of every order is exact in fp32
                  while a row's sum|v x| < 2^24, which `exact_product_mm` asserts per matrix and X.
  full_mantissa_x signed values of magnitude in [0.5, 1.5) with all 24 mantissa bits in use, for
                  `assert_within_any_order_bound_mm`: the bound len u / (1 - len u) * sum|v x| of _spmv_oracle, per
                  entry of Y.
"""
from __future__ import annotations

import torch

from _spmv_oracle import (U, _csr, _draw, _signs, csr_item_edges, empty_matrix, few_columns,  # noqa: F401
                          full_mantissa_operands, integer_operands, one_row, row_lengths, rows_of, with_values)
from parallel_c_programs_amd import ops

SENTINEL = -7777777  # what the model's Y and workspace hold where nothing was written
JUNK = 977           # what the model reads outside X's k columns (a real buffer holds a neighbour's data there)
CHUNK = 128          # columns per pass of the references (bounds their memory)


# ------------------------------------------------------------------------------------------ operands
def integer_x(n_cols: int, k: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(1, 8, (n_cols, k), generator=g) * _signs((n_cols, k), g)).float()


def full_mantissa_x(n_cols: int, k: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n_cols, k, dtype=torch.float64, generator=g) + 0.5) * _signs((n_cols, k), g)).float()


def full_mantissa_values(m: ops.CSR, seed: int) -> ops.CSR:
    return with_values(m, full_mantissa_operands(m.nnz, 1, seed)[0])


# ------------------------------------------------------------------------------------------ references and assertions
def _row_sums(m: ops.CSR, prod_of_chunk, k: int, dtype) -> torch.Tensor:
    rows, out = rows_of(m), torch.zeros(m.n_rows, k, dtype=dtype)
    for c0 in range(0, k, CHUNK):
        out[:, c0:c0 + CHUNK].index_add_(0, rows, prod_of_chunk(c0, min(k, c0 + CHUNK)))
    return out


def exact_product_mm(m: ops.CSR, x: torch.Tensor) -> torch.Tensor:
    """The int64 product of an integer-valued matrix and block X [n_cols, k] (index_add_ on the CPU)."""
    val, x, col = m.val.cpu(), x.cpu(), m.col.cpu().long()
    assert torch.equal(val, val.round()) and torch.equal(x, x.round()), "integer family only"
    vl, xl = val.long()[:, None], x.long()
    absrow = _row_sums(m, lambda a, b: (vl * xl[col, a:b]).abs(), x.shape[1], torch.int64)
    # every partial sum of every summation order is an integer of magnitude < 2^24: exact in fp32
    assert absrow.numel() == 0 or int(absrow.max()) < 2 ** 24, "a row's sum|v x| reaches 2^24: fp32 sums are not exact"
    return _row_sums(m, lambda a, b: vl * xl[col, a:b], x.shape[1], torch.int64)


def assert_equals_exact(out: torch.Tensor, exact: torch.Tensor, m: ops.CSR) -> None:
    """`out` against an int64 product computed before (exact_product_mm, or columns of one); names the first wrong
    (row, column)."""
    got, want = out.detach().cpu().double(), exact.double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = torch.nonzero(~(got == want))  # (~(==): a NaN is wrong too)
    r, c = int(bad[0, 0]), int(bad[0, 1])
    msg = (f"{bad.shape[0]} of {want.numel()} entries wrong in {torch.unique(bad[:, 0]).numel()} rows and "
           f"{torch.unique(bad[:, 1]).numel()} columns; first (row {r}, column {c}) ({int(row_lengths(m)[r])} nonzeros): "
           f"got {got[r, c].item()}, exact {want[r, c].item()}, difference {(got[r, c] - want[r, c]).item()}")
    print(msg)
    raise AssertionError(msg)


def assert_exact_mm(out: torch.Tensor, m: ops.CSR, x: torch.Tensor) -> None:
    assert_equals_exact(out, exact_product_mm(m, x), m)


def any_order_bound_mm(m: ops.CSR, x: torch.Tensor):
    """(fp64 product, per-entry bound len_r u / (1 - len_r u) * sum|v x|)."""
    vd, xd, col = m.val.cpu().double()[:, None], x.cpu().double(), m.col.cpu().long()
    ref = _row_sums(m, lambda a, b: vd * xd[col, a:b], x.shape[1], torch.float64)  # (products exact: 24 x 24 bits)
    absrow = _row_sums(m, lambda a, b: (vd * xd[col, a:b]).abs(), x.shape[1], torch.float64)
    ku = (row_lengths(m).double() * U)[:, None]
    return ref, ku / (1 - ku) * absrow


def assert_within_any_order_bound_mm(out: torch.Tensor, m: ops.CSR, x: torch.Tensor) -> float:
    """Every entry within the any-order bound of the fp64 product (an empty row must be exactly 0). Returns the worst
    err / bound, which the caller prints."""
    ref, bound = any_order_bound_mm(m, x)
    got = out.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    ok = err <= bound  # (a NaN compares false; an empty row has bound 0 and ref 0)
    if not bool(ok.all()):
        bad = torch.nonzero(~ok)
        r, c = int(bad[0, 0]), int(bad[0, 1])
        msg = (f"{bad.shape[0]} of {ref.numel()} entries outside the any-order bound; first (row {r}, column {c}) "
               f"({int(row_lengths(m)[r])} nonzeros): got {got[r, c].item()!r}, fp64 {ref[r, c].item()!r}, error "
               f"{err[r, c].item():.3e}, bound {bound[r, c].item():.3e}; worst err / bound {worst:.3f}")
        print(msg)
        raise AssertionError(msg)
    return worst


# ------------------------------------------------------------------------------------------ more builders
def split_last_row() -> ops.CSR:
    """First row empty, short rows, and a LAST row of 2500 nonzeros (split at every item size)."""
    g = torch.Generator().manual_seed(601)
    rows, cols = _draw([0, 3, 70, 1, 0, 2500], 0, 4000, g)
    return _csr(6, 4000, rows, cols, 602)


def dense_3x3() -> ops.CSR:
    rows = torch.arange(3).repeat_interleave(3)
    return _csr(3, 3, rows, torch.arange(3).repeat(3), 603)


def one_by_one() -> ops.CSR:
    return _csr(1, 1, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 604)


def no_rows() -> ops.CSR:
    return _csr(0, 17, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 605)


# ------------------------------------------------------------------------------------------ CPU model of the walk
def width_classes(k: int):
    """The launches of pcmx_spmm_csr for a k: a list of (first column, class, tiles). class 4 / 8 / 16 / 32: lanes per
    group of the narrow kernel (k <= 32); 64 / 128 / 256: columns per tile of the wide kernel — the full 256-column
    tiles first, then the partial last tile (or the whole of a k < 256) in the smallest class that covers it."""
    if k == 0:
        return []
    if k <= 32:
        return [(0, next(kp for kp in (4, 8, 16, 32) if kp >= k), 1)]
    full, rem = divmod(k, 256)
    out = [(0, 256, full)] if full else []
    if rem:
        out.append((256 * full, 64 if rem <= 64 else 128 if rem <= 128 else 256, 1))
    return out


def plan_features(p) -> dict:
    """What a plan exercises: whole-row one-row items, multi-row items, pieces of split rows, split rows."""
    it = p.items.cpu()
    nrows = (it[:, 0] >> 32) - (it[:, 0] & 0xFFFFFFFF)
    piece = p.slot.cpu() >= 0
    return dict(items=int(it.shape[0]), whole_row=int(((nrows == 1) & ~piece).sum()), multi_row=int((nrows > 1).sum()),
                pieces=int(piece.sum()), split_rows=int(p.split.shape[0]), max_rows=int(nrows.max()) if nrows.numel() else 0)


def model_product(m: ops.CSR, p, x: torch.Tensor, pad: int = 5, mutant: str | None = None):
    """int64 model of pcmx_spmm_csr on integer operands, walking the plan arrays the kernels read.
    Returns (Y [n_rows, k + pad], writes [n_rows, k + pad]): Y starts as SENTINEL, `writes` counts the stores to every
    element (the fix-up's included). Reads outside X's k columns give JUNK.

    Per launch of width_classes(k), per item and column tile: the tile's first column c0 and its valid columns
    kt = min(k - c0, tile); wide: the nonzeros flat in order, the row border (from row_ptr relative to the item's first
    nonzero) stores the accumulator to Y[row0 + r] or, for a piece (slot >= 0), to workspace row slot; rows behind the
    last nonzero are stored at the item's end. Narrow: T groups per row from the item's average row length, teams of T
    groups take rows r = team, team + teams, ...; group t sums the row's nonzeros t, t + T, ...; the partial sums of
    a team's groups are added and stored. Then the fix-up: Y[row] = sum of workspace rows first .. first + pieces - 1.

    mutant: one of MUTANTS (a single fault each), None for the kernels as written."""
    assert mutant is None or mutant in MUTANTS, mutant
    n_rows, k = m.n_rows, x.shape[1]
    rp, col, val = m.row_ptr.cpu(), m.col.cpu().long(), m.val.cpu().long()
    xp = torch.cat([x.cpu().long(), torch.full((m.n_cols, 512), JUNK, dtype=torch.int64)], 1)
    items, slot, split = p.items.cpu(), p.slot.cpu().long(), p.split.cpu().long()
    ldw = (k + 3) & ~3
    Y = torch.full((n_rows, k + pad), SENTINEL, dtype=torch.int64)
    W = torch.zeros((n_rows, k + pad), dtype=torch.int64)
    ws = torch.full((p.n_pieces + 1, ldw + 1), SENTINEL, dtype=torch.int64)
    hit = mutant is None  # a mutant strikes once, at the first place it applies
    if n_rows == 0 or k == 0:
        return Y, W
    for c_base, cls, tiles in width_classes(k):
        for i in range(items.shape[0]):
            row0, row1 = int(items[i, 0] & 0xFFFFFFFF), int(items[i, 0] >> 32)
            nz0, nz1 = int(items[i, 1]), int(items[i, 2])
            n, nrows, sl = nz1 - nz0, row1 - row0, int(slot[i])
            rel = (rp[row0:row1 + 1] - nz0) if nrows > 1 else torch.tensor([0, n])
            pos = torch.arange(n)
            lrow = torch.searchsorted(rel[1:].contiguous(), pos, right=True)  # the row border walk
            if cls <= 32:  # ------------------------------------------------ narrow
                NG = 64 // cls
                T = 1
                while T < NG and T * 4 < n // nrows:
                    T <<= 1
                teams = NG // T
                passes = (nrows + teams - 1) // teams
                inrow = pos - rel[lrow]
                grp = (lrow % teams) * T + inrow % T  # the physical group of every nonzero
                prod = val[nz0:nz1, None] * xp[col[nz0:nz1], :k]
                if mutant == "dropped_nonzero" and not hit and n:
                    prod[n // 2, k // 2] = 0
                    hit = True
                acc = torch.zeros(passes * NG, k, dtype=torch.int64).index_add_(0, (lrow // teams) * NG + grp, prod)
                acc = acc.view(passes, NG, k)
                if mutant == "groups_swapped" and not hit and T < NG and bool((acc[:, 0] != acc[:, NG - 1]).any()):
                    acc = acc.clone()
                    acc[:, [0, NG - 1]] = acc[:, [NG - 1, 0]]
                    hit = True
                tot = acc.view(passes, teams, T, k).sum(2).reshape(passes * teams, k)[:nrows]  # row r = pass * teams + team
                kt_store = k
                if mutant == "mask_le" and not hit:
                    tot = torch.cat([tot, (val[nz0:nz1, None] * xp[col[nz0:nz1], k:k + 1]).sum(0).expand(nrows, 1)], 1)
                    kt_store, hit = k + 1, True
                stored = nrows
                if mutant == "border_missed" and not hit and nrows > 1:
                    stored, hit = nrows - 1, True
                if sl >= 0:
                    s = sl + 1 if mutant == "slot_off" else sl
                    ws[s, :kt_store] = tot[0]
                else:
                    Y[row0:row0 + stored, :kt_store] = tot[:stored]
                    W[row0:row0 + stored, :kt_store] += 1
                continue
            for ty in range(tiles):  # -------------------------------------------- wide
                c0 = c_base + ty * cls
                kt = min(k - c0, cls)
                if mutant == "mask_le" and not hit and kt < cls:
                    kt, hit = kt + 1, True
                cx = c0
                if mutant == "tile_off" and not hit:
                    cx, hit = c0 + cls, True
                prod = val[nz0:nz1, None] * xp[col[nz0:nz1], cx:cx + kt]
                if mutant == "dropped_nonzero" and not hit and n:
                    prod[n // 2, kt // 2] = 0
                    hit = True
                acc = torch.zeros(nrows, kt, dtype=torch.int64).index_add_(0, lrow, prod)
                if mutant == "swap_64" and not hit and kt > 64:
                    w = min(64, kt - 64)  # the dword form's registers 0 and 1: columns lane and lane + 64
                    acc[:, :w], acc[:, 64:64 + w] = acc[:, 64:64 + w].clone(), acc[:, :w].clone()
                    hit = True
                stored = nrows
                if mutant == "border_missed" and not hit and nrows > 1:
                    stored, hit = nrows - 1, True  # the rows behind the last border are never stored
                if sl >= 0:
                    s = sl + 1 if mutant == "slot_off" else sl
                    ws[s, c0:c0 + kt] = acc[0]
                else:
                    Y[row0:row0 + stored, c0:c0 + kt] = acc[:stored]
                    W[row0:row0 + stored, c0:c0 + kt] += 1
    for s in range(split.shape[0]):
        row, first, pieces = (int(v) for v in split[s])
        if mutant == "fixup_short" and not hit:
            pieces, hit = pieces - 1, True
        Y[row, :k] = ws[first:first + pieces, :k].sum(0)
        W[row, :k] += 1
    assert hit or mutant == "slot_off", f"mutant {mutant} found no place to strike"
    return Y, W


MUTANTS = ("dropped_nonzero", "fixup_short", "slot_off", "tile_off", "mask_le", "groups_swapped", "border_missed",
           "swap_64")


def assert_model(Y: torch.Tensor, W: torch.Tensor, m: ops.CSR, x: torch.Tensor, exact: torch.Tensor | None = None):
    """The model's (or a mutant's) output: the exact product in columns < k, every such element written exactly once,
    the padding untouched."""
    k = x.shape[1]
    assert bool((W[:, :k] == 1).all()), f"{int((W[:, :k] != 1).sum())} elements of Y not written exactly once"
    assert bool((W[:, k:] == 0).all()) and bool((Y[:, k:] == SENTINEL).all()), "the padding of Y was written"
    assert_equals_exact(Y[:, :k], exact_product_mm(m, x) if exact is None else exact, m)
