"""The SpMV oracle checked on the CPU: the model of the kernels' walk over the sliced layout (which reads the packed
words the GPU reads) equals the exact integer product for every builder and layout; eleven mutants of it are each
rejected by `assert_exact`; the any-order bound accepts three fp32 summation orders and rejects one dropped product;
and the banded path query names every kernel over the geometry table the GPU tests run."""
import functools
from types import SimpleNamespace

import pytest
import torch

import _spmv_oracle as so
from parallel_c_programs_amd import ops
from parallel_c_programs_amd.ops.sparse import PackedLayoutUnavailable

LAYOUTS = [(True, 256), (True, 384), (True, 512), (True, 1024), (False, 512), (False, 1024)]
BUILDERS = ["csr_item_edges", "sliced_stripe_edges", "few_columns", "empty_matrix", "one_row"]


def _build(name, item_nnz):
    return so.sliced_stripe_edges(item_nnz) if name == "sliced_stripe_edges" else getattr(so, name)()


def _x(m, seed=7):
    return so.integer_operands(1, m.n_cols, seed)[1]


# ------------------------------------------------------------------------------------------ operand families
def test_integer_operands_are_what_they_claim():
    val, x = so.integer_operands(100_000, 5000, 3)
    assert val.dtype == x.dtype == torch.float32
    assert set(val.tolist()) == {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
    assert set(x.tolist()) == {float(s * k) for s in (-1, 1) for k in range(1, 8)}
    v2, x2 = so.full_mantissa_operands(100_000, 5000, 3)
    assert bool((v2.abs() >= 0.5).all()) and bool((v2.abs() < 1.5 + 1e-6).all()) and bool((v2 < 0).any())
    # full mantissa: most values are not representable with fewer bits
    assert (v2.view(torch.int32) & 1).float().mean().item() > 0.2 and (x2.view(torch.int32) & 1).float().mean().item() > 0.2


def test_exact_product_refuses_rows_that_fp32_cannot_sum_exactly():
    n = 1 << 20  # sum|v x| = 21 * 2^20 > 2^24
    m = ops.CSR(torch.tensor([0, n]), torch.zeros(n, dtype=torch.int32), torch.full((n,), 3.0), 1)
    with pytest.raises(AssertionError, match="2\\^24"):
        so.exact_product(m, torch.tensor([7.0]))
    with pytest.raises(AssertionError, match="integer family"):
        so.exact_product(ops.CSR(torch.tensor([0, 1]), torch.zeros(1, dtype=torch.int32), torch.tensor([0.5]), 1),
                         torch.tensor([1.0]))


def test_builders_hold_the_cases_they_name():
    m = so.csr_item_edges()
    lens = so.row_lengths(m)
    assert m.nnz < 150_000 and lens[0] == 0 and lens[-1] == 0
    assert {0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3073} <= set(lens.tolist())
    for name in ("csr_item_edges", "few_columns", "one_row", "wide_matrix"):  # columns distinct inside a row
        b = getattr(so, name)()
        key = so.rows_of(b) * b.n_cols + b.col.long()
        assert torch.unique(key).numel() == b.nnz, name
    for item in (256, 384, 512, 1024):
        s = so.sliced_stripe_edges(item)
        lens = so.row_lengths(s)
        assert s.n_rows % 64 != 0 and s.n_rows > 2048 and lens[0] == 0 and lens[-1] == 0
        assert {item + 1, 2 * item, 2 * item + 1} <= set(lens[2048:].tolist())
        assert int((lens == 1).sum()) >= 1100
    assert so.empty_matrix().nnz == 0 and so.one_row().n_rows == 1
    assert torch.unique(so.few_columns().col).numel() == 3


# ------------------------------------------------------------------------------------------ the layout model
@pytest.mark.parametrize("name", BUILDERS)
@pytest.mark.parametrize("pack,item_nnz", LAYOUTS)
def test_layout_model_equals_exact_product(name, pack, item_nnz):
    """The walk over what the GPU reads (packed words + colbase, or col + lrow; items; row_mask as u32; chunk_base;
    fix) gives the exact integer product: every builder, S in {8, 16, 24, 32}, head 0 and 0.2, col_split on and off.
    The first CPU test of SlicedCSR._pack."""
    m = _build(name, item_nnz)
    x = _x(m)
    exact = so.exact_product(m, x)
    cases = [(S, head, 0) for S in (8, 16, 24, 32) for head in (0.0, 0.2)]
    cases += [(S, head, m.n_cols * 2 // 5) for S in (16, 32) for head in (0.0, 0.2)]
    for S, head, split in cases:
        if m.nnz == 0 and item_nnz in (256, 384):  # these items exist in the packed stream only: nothing to pack
            with pytest.raises(PackedLayoutUnavailable):
                ops.SlicedCSR(m, S, head=head, item_nnz=item_nnz, pack=pack, col_split=split)
            continue
        s = ops.SlicedCSR(m, S, head=head, item_nnz=item_nnz, pack=pack, col_split=split)
        assert (s.cr is not None) == (pack and m.nnz > 0), (S, head, split)
        y = so.layout_product(s, x)
        assert torch.equal(y, exact), (S, head, split, int((y != exact).sum()))
        so.assert_exact(y, m, x)
        it = s.items
        assert it.shape[0] == 0 or int((it[:, 2] - it[:, 1]).max()) <= item_nnz


@pytest.mark.parametrize("pack", [True, False])
def test_layout_model_on_wide_slices(pack):
    """4.2e6 columns in 8 slices with a head: one slice is wider than 2^20 columns, so bit 20 of the packed column
    offset, next to the head flag at bit 21, is in use; the model still gives the exact product."""
    m = so.wide_matrix()
    x = _x(m)
    s = ops.SlicedCSR(m, 8, head=0.1, pack=pack)
    widths = [h - l for l, h in zip(s.colbase, s.colbase[1:] + [m.n_cols])]
    assert (1 << 20) < max(widths) < (1 << 21) and s.head_cols > 0
    if pack:
        w = s.cr.long() & 0xFFFFFFFF
        tail = ((w >> so.PACK_HEAD_BIT) & 1) == 0
        assert bool(tail.any()) and bool((~tail).any())
        assert bool(((w[tail] >> 20) & 1).any())  # bit 20 of a tail offset
    else:
        assert s.cr is None
    so.assert_exact(so.layout_product(s, x), m, x)


def test_stripe_builder_reaches_the_stripe_cases():
    """At the layouts the GPU tests run, the stripe builder gives what it is for (read from the packed words): rows
    ending on lane 63 / starting on lane 0 inside multi-row items, carries, rows over three stripes, fix entries, rows
    touched by every slice, and the largest row offset an item size allows (a slice touches only rows with a nonzero in
    it, so an item holds at most item_nnz rows: offsets of 512 and more, bit 31 of the word, and 1023-row items exist
    at 1024-nonzero items only)."""
    for pack, item in LAYOUTS:
        s = ops.SlicedCSR(so.sliced_stripe_edges(item), 16, head=0.2, item_nnz=item, pack=pack)
        f = so.stripe_features(s)
        assert f["max_item_rows"] == min(item, 1023) and f["max_row_offset"] == min(item, 1023) - 1, (item, f)
        assert min(f["ends_on_lane_63"], f["starts_on_lane_0"], f["carries"], f["three_stripes"], f["fix_entries"],
                   f["all_slice_rows"]) > 0, (item, f)
        if pack and item == 1024:
            assert bool((s.cr < 0).any())  # the word is negative as an int


# ------------------------------------------------------------------------------------------ mutants
@functools.lru_cache(maxsize=None)
def _mutant_setup(item_nnz=512):
    """sliced_stripe_edges(512) in 32 slices with a head (bit 31 of row_mask and the head flag in use), 512-nonzero
    items; the row-offset sign mutant needs offsets >= 512 and takes the same matrix in 1024-nonzero items."""
    m = so.sliced_stripe_edges(512)
    x = _x(m, 11)
    s = ops.SlicedCSR(m, 32, head=0.2, item_nnz=item_nnz)
    assert s.cr is not None and s.head_cols > 0
    col, lrow, sid = so.decode(s)
    return m, x, s, col, lrow, sid, so.products(s, x, col)


def _row_runs(s, lrow):
    """(item, position in item, first-of-row, last-of-row) per stored nonzero."""
    item_of, pos = so.item_index(s)
    key = item_of * 65536 + lrow
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = key[1:] != key[:-1]
    last = torch.ones_like(key, dtype=torch.bool)
    last[:-1] = first[1:]
    return item_of, pos, first, last


def _nrows(s):
    it = s.items
    return (it[:, 0] >> 32) - (it[:, 0] & 0xFFFFFFFF)


def _mut_dropped():
    m, x, s, col, lrow, sid, prod = _mutant_setup()
    i = s.nnz // 2
    assert prod[i] != 0
    p = prod.clone()
    p[i] = 0
    return so.layout_combine(s, *so.layout_partials(s, x, prod=p))


def _mut_twice():
    m, x, s, col, lrow, sid, prod = _mutant_setup()
    i = s.nnz // 3
    assert prod[i] != 0
    p = prod.clone()
    p[i] *= 2
    return so.layout_combine(s, *so.layout_partials(s, x, prod=p))


def _mut_column_off_by_one():
    m, x, s, col, lrow, sid, prod = _mutant_setup()
    xl = x.long()
    ok = (col + 1 < s.n_cols) & (xl[(col + 1).clamp(max=s.n_cols - 1)] != xl[col])
    i = int(torch.nonzero(ok)[0])
    c = col.clone()
    c[i] += 1
    assert so.products(s, x, c)[i] != prod[i]
    return so.layout_combine(s, *so.layout_partials(s, x, col=c))


def _mut_next_row():
    m, x, s, col, lrow, sid, prod = _mutant_setup()
    item_of, pos, first, last = _row_runs(s, lrow)
    ok = last & (lrow + 1 < _nrows(s)[item_of])  # a row's last nonzero, another row of the item behind it
    i = int(torch.nonzero(ok)[0])
    lr = lrow.clone()
    lr[i] += 1
    assert prod[i] != 0
    return so.layout_combine(s, *so.layout_partials(s, x, lrow=lr))


def _mut_head_flag_ignored():
    m, x, s, col, lrow, sid, prod = _mutant_setup()
    c, _, _ = so.decode(s, head_flag=False)
    changed = so.products(s, x, c) != prod
    assert bool((c != col).any()) and bool(changed.any())  # a head column in a slice whose colbase is not 0
    return so.layout_combine(s, *so.layout_partials(s, x, col=c))


def _mut_neighbour_colbase():
    m, x, s, col, lrow, sid, prod = _mutant_setup()
    c, _, _ = so.decode(s, colbase_shift=1)
    assert bool((so.products(s, x, c) != prod).any())
    return so.layout_combine(s, *so.layout_partials(s, x, col=c))


def _mut_row_offset_sign_extended():
    m, x, s, col, lrow, sid, prod = _mutant_setup(1024)
    _, lr, _ = so.decode(s, sign_extend_row=True)
    neg = lr < 0
    assert bool(neg.any()) and bool((lrow[neg] >= 512).all()) and bool((prod[neg] != 0).all())
    return so.layout_combine(s, *so.layout_partials(s, x, lrow=lr))


def _mut_fix_entry_skipped():
    m, x, s, col, lrow, sid, prod = _mutant_setup()
    comp, extra = so.layout_partials(s, x)
    fix = s.fix.long()
    assert fix.shape[0] > 0
    j = int(torch.nonzero(extra[fix[:, 0]] != 0)[0])
    return so.layout_combine(s, comp, extra, fix=torch.cat([fix[:j], fix[j + 1:]]))


def _mut_chunk_base_off_by_one():
    m, x, s, col, lrow, sid, prod = _mutant_setup()
    comp, extra = so.layout_partials(s, x)
    S = s.n_slices
    out0 = s.meta[2 * S + 1:3 * S + 2]
    cb = s.chunk_base.long().clone()
    mask = s.row_mask.long() & 0xFFFFFFFF
    for c in range(cb.shape[0]):  # the first (chunk, slice) whose first touched row would read a different partial
        for k in range(S):
            if not bool(((mask[64 * c:64 * c + 64] >> k) & 1).any()):
                continue
            a = int(out0[k] + cb[c, k])
            if a + 1 < int(out0[k + 1]) and comp[a] != comp[a + 1]:
                cb[c, k] += 1
                return so.layout_combine(s, comp, extra, chunk_base=cb)
    raise AssertionError("no chunk where the shifted base reads another value")


def _mut_mask_bit_31_dropped():
    m, x, s, col, lrow, sid, prod = _mutant_setup()
    comp, extra = so.layout_partials(s, x)
    mask = s.row_mask.long() & 0xFFFFFFFF
    out0 = s.meta[2 * 32 + 1:]
    assert bool(((mask >> 31) & 1).any()) and bool((s.row_mask < 0).any())
    assert bool((comp[int(out0[31]):int(out0[32])] != 0).any())
    return so.layout_combine(s, comp, extra, mask=mask & 0x7FFFFFFF)


def _mut_carry_dropped():
    m, x, s, col, lrow, sid, prod = _mutant_setup()
    item_of, pos, first, last = _row_runs(s, lrow)
    multi = _nrows(s)[item_of] > 1
    run = torch.cumsum(first.long(), 0) - 1  # index of the row run of every nonzero
    p_first = pos[first][run]
    p_last = pos[last][run]
    # a row of a multi-row item that crosses a 64-element stripe: what it summed before its last stripe is the carry
    before = multi & (pos // 64 < p_last // 64)
    for r in torch.unique(run[before]).tolist():
        sel = before & (run == r)
        if int(prod[sel].sum()) != 0:
            assert int(p_first[sel][0]) // 64 < int(p_last[sel][0]) // 64
            p = prod.clone()
            p[sel] = 0
            return so.layout_combine(s, *so.layout_partials(s, x, prod=p))
    raise AssertionError("no row with a nonzero carry")


MUTANTS = {
    "one_nonzero_dropped": _mut_dropped,
    "one_nonzero_counted_twice": _mut_twice,
    "one_column_off_by_one": _mut_column_off_by_one,
    "one_nonzero_credited_to_the_next_row": _mut_next_row,
    "head_flag_ignored": _mut_head_flag_ignored,
    "colbase_of_the_neighbouring_slice": _mut_neighbour_colbase,
    "row_offset_sign_extended_from_bit_31": _mut_row_offset_sign_extended,
    "one_fix_entry_skipped": _mut_fix_entry_skipped,
    "chunk_base_of_one_chunk_off_by_one": _mut_chunk_base_off_by_one,
    "row_mask_bit_31_dropped": _mut_mask_bit_31_dropped,
    "carry_across_a_stripe_dropped_for_one_row": _mut_carry_dropped,
}


def test_unmutated_model_passes_on_the_mutant_layouts():
    for item in (512, 1024):
        m, x, s, *_ = _mutant_setup(item)
        so.assert_exact(so.layout_product(s, x), m, x)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_assert_exact_rejects_mutant(name, capsys):
    assert len(MUTANTS) == 11
    y = MUTANTS[name]()  # (asserts its own placement: the change alters an integer product)
    m, x = _mutant_setup()[:2]
    with pytest.raises(AssertionError, match="rows wrong; first row"):
        so.assert_exact(y, m, x)
    assert "difference" in capsys.readouterr().out  # the first wrong row, its length and the difference are printed


# ------------------------------------------------------------------------------------------ the any-order bound
def _padded_products(m, x):
    """fp32 products v * x[col], one row per matrix row, zero-padded to a power of two (adding +0 is exact)."""
    lens = so.row_lengths(m)
    width = 1 << int(lens.max() - 1).bit_length()
    p = torch.zeros(m.n_rows, width, dtype=torch.float32)
    pos = torch.arange(m.nnz) - m.row_ptr[:-1][so.rows_of(m)]
    p[so.rows_of(m), pos] = m.val * x[m.col.long()]
    return p


def _three_orders(p):
    fwd = torch.zeros(p.shape[0], dtype=torch.float32)
    rev = torch.zeros(p.shape[0], dtype=torch.float32)
    for j in range(p.shape[1]):
        fwd = fwd + p[:, j]
        rev = rev + p[:, p.shape[1] - 1 - j]
    pair = p.clone()
    while pair.shape[1] > 1:
        h = pair.shape[1] // 2
        pair = pair[:, :h] + pair[:, h:]
    return {"forward": fwd, "reversed": rev, "pairwise": pair[:, 0]}


def test_any_order_bound_accepts_three_orders_and_rejects_a_dropped_product(capsys):
    base = so.csr_item_edges()
    val, x = so.full_mantissa_operands(base.nnz, base.n_cols, 21)
    m = so.with_values(base, val)
    p = _padded_products(m, x)
    good = _three_orders(p)
    assert not torch.equal(good["forward"], good["reversed"]) and not torch.equal(good["forward"], good["pairwise"])
    for name, y in good.items():
        worst = so.assert_within_any_order_bound(y, m, x)
        print(f"{name}: worst err / bound = {worst:.4f}")
        assert 0 < worst <= 1
    # one product dropped from a row of at least 64 nonzeros, the product larger than that row's bound
    _, bound = so.any_order_bound(m, x)
    lens = so.row_lengths(m)
    r = int(torch.nonzero(lens >= 64)[0])
    assert lens[r] >= 64 and abs(p[r, 5].item()) > bound[r].item() * 2
    q = p.clone()
    q[r, 5] = 0
    for name, y in _three_orders(q).items():
        assert torch.equal(torch.cat([y[:r], y[r + 1:]]), torch.cat([good[name][:r], good[name][r + 1:]]))
        with pytest.raises(AssertionError, match="outside the any-order bound"):
            so.assert_within_any_order_bound(y, m, x)
    # an empty row must be exactly zero, and a NaN is outside every bound
    bad = good["forward"].clone()
    bad[0] = 1e-30
    with pytest.raises(AssertionError):
        so.assert_within_any_order_bound(bad, m, x)
    bad[0] = float("nan")
    with pytest.raises(AssertionError):
        so.assert_within_any_order_bound(bad, m, x)


def test_probe_columns_on_a_hand_built_layout():
    s = SimpleNamespace(n_cols=100, head_cols=7, col_split=50, colbase=[0, 7, 20, 50, 50, 80, 99, 100])
    assert so.probe_columns(s) == [0, 6, 7, 19, 20, 49, 50, 79, 80, 98, 99]
    s = SimpleNamespace(n_cols=10, head_cols=0, col_split=0, colbase=[0] * 8)
    assert so.probe_columns(s) == [0, 9]
    real = ops.SlicedCSR(so.few_columns(), 16, head=0.2, col_split=400)
    pc = so.probe_columns(real)
    assert pc == sorted(set(pc)) and {0, 999, 399, 400, real.head_cols} <= set(pc)
    assert all(b in pc for b in real.colbase if b < 1000)


# ------------------------------------------------------------------------------------------ the banded path query
def test_banded_path_query_names_every_kernel():
    """pcmx_spmv_banded_path (host code: nothing is launched) over the geometry table of the GPU tests: every path is
    reached — the wave-per-row kernel, all seven LDS instantiations, the stream kernel at both ends of its range
    (L = 257 and 639) with the fall-backs next to them (255 and 641)."""
    import re
    from pathlib import Path

    from parallel_c_programs_amd._native import hip_lib

    lib = hip_lib()
    header = Path(__file__).resolve().parents[1] / "csrc" / "include" / "pcmx_errors.h"
    err_arg = int(re.search(r"PCMX_ERR_ARG\s*=\s*(-?\d+)", header.read_text()).group(1))
    seen = set()
    for L, (geo, want1, want8) in so.BANDED_GEOMETRIES.items():
        a, b, c, d, e = geo
        assert 2 * (a // 2) + 1 + 2 * c + 2 * e == L
        *full, clipped = so.banded_sizes(geo)
        assert clipped < so.banded_reach(*geo)
        for n in full:
            assert so.banded_path(lib, n, geo, 0) == (0, 0), (L, n)
            assert so.banded_path(lib, n, geo, 1) == want1, (L, n)
            assert so.banded_path(lib, n, geo, 8) == want8, (L, n)
            assert so.banded_path(lib, n, geo, 8, aligned=False) == want1, (L, n)  # unaligned values: no stream
            seen |= {(0, 0), want1, want8}
        assert so.banded_path(lib, clipped, geo, 8) == want1, L  # every row clipped: no block to stream
    assert seen == so.ALL_BANDED_PATHS
    # what the launcher refuses
    for geo, variant in (((0, 1, 1, 1, 1), 8), ((3, -1, 1, 1, 1), 1), ((3, 1, 1, 1, -1), 0), ((3, 1, 1, 1, 1), 2),
                         ((3, 1, 1, 1, 1), 7), ((3, 1, 1, 1, 1), -1)):
        assert so.banded_path(lib, 100, geo, variant)[0] == err_arg, (geo, variant)
    assert lib.pcmx_spmv_banded_path(100, 9, 3, 5, 2, 3, 1, 1, None) == 1  # nl may be NULL
