"""SpMV on the GPU against references that leave no slack (tests/_spmv_oracle.py): the integer operand family, on
which every fp32 summation order is exact, so one dropped, doubled or mis-slotted product fails `assert_exact`; and
full-mantissa operands against the fp64 product within the any-order rounding bound. Every kernel path is run and the
tests prove from the work items, the layout and pcmx_spmv_banded_path that they reached it: the plain CSR kernel's
seven lanes-per-row classes and the planner's cuts, the six sliced product instantiations with both combines and the
fused one, the stripe cases of sliced_step, degenerate layouts, the packed column decode at every slice boundary, and
the banded wave-per-row kernel, all seven LDS instantiations and the stream kernel at both ends of its range."""
import ctypes
import functools

import pytest
import torch

import _spmv_oracle as so
from parallel_c_programs_amd import ops
from parallel_c_programs_amd.ops.sparse import PackedLayoutUnavailable

pytestmark = pytest.mark.gpu

SENT = -7.25  # no integer, no product of the families
PAD = 64
LAYOUTS = [(True, 256), (True, 384), (True, 512), (True, 1024), (False, 512), (False, 1024)]
ITEM_NNZ = 1024  # spmv.hip: kItemNnz


def _guarded(n, gpu):
    """(buffer, view of n floats inside it with PAD sentinels on both sides)."""
    buf = torch.full((n + 2 * PAD,), SENT, device=gpu)
    return buf, buf[PAD:PAD + n]


def _guards_intact(buf, n):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n:] == SENT).all())


def _lib():
    from parallel_c_programs_amd._native import hip_lib

    return hip_lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------ plain CSR
def _csr_into(mg, x, y):
    """pcmx_spmv_csr into a caller's y (ops.spmv allocates its own)."""
    rc = _lib().pcmx_spmv_csr(_p(mg.row_ptr), _p(mg.col), _p(mg.val), _p(x), _p(y), mg.n_rows, _p(mg.items),
                              ctypes.c_longlong(mg.items.shape[0]), _stream())
    assert rc == 0
    torch.cuda.synchronize()


def test_csr_item_edges_exact_and_reaches_every_class(gpu):
    """spmv_csr_items_kernel on the planner's cuts, integer operands: exact (split rows add with float atomics, and
    integer sums are exact in any order). The work items of the call prove what ran: all seven lanes-per-row classes,
    an item of exactly 1023 rows, an item of exactly kItemNnz nonzeros, whole-row and split-row single-row items."""
    m = so.csr_item_edges()
    _, x = so.integer_operands(1, m.n_cols, 31)
    mg = m.to(gpu)
    out = ops.spmv(mg, x.to(gpu))
    so.assert_exact(out, m, x)
    it = mg.items.cpu()
    nrows = (it[:, 0] >> 32) - (it[:, 0] & 0xFFFFFFFF)
    nnz = it[:, 2] - it[:, 1]
    classes = set()
    for r, n in zip(nrows[nrows > 1].tolist(), nnz[nrows > 1].tolist()):
        avg, L = n // r, 1
        while L < 64 and L * 4 < avg:  # the kernel's rule
            L <<= 1
        classes.add(L)
    assert classes == {1, 2, 4, 8, 16, 32, 64}
    assert 1023 in nrows.tolist() and int(nrows.max()) == 1023
    assert ITEM_NNZ in nnz.tolist() and int(nnz.max()) == ITEM_NNZ
    lens = so.row_lengths(m)
    single = nrows == 1
    whole = nnz[single] == lens[(it[:, 0] & 0xFFFFFFFF)[single]]
    assert bool(whole.any()) and bool((~whole).any())
    # y inside a sentinel-filled buffer
    buf, y = _guarded(m.n_rows, gpu)
    _csr_into(mg, x.to(gpu), y)
    so.assert_exact(y, m, x)
    assert _guards_intact(buf, m.n_rows)


def test_csr_item_edges_full_mantissa_within_any_order_bound(gpu):
    base = so.csr_item_edges()
    val, x = so.full_mantissa_operands(base.nnz, base.n_cols, 32)
    m = so.with_values(base, val)
    mg = m.to(gpu)
    buf, y = _guarded(m.n_rows, gpu)
    mg.plan()
    _csr_into(mg, x.to(gpu), y)
    worst = so.assert_within_any_order_bound(y, m, x)
    print(f"plain CSR, item edges: worst err / bound = {worst:.4f} (rows of >= 64 nonzeros: "
          f"{so.worst_ratio(y, m, x, 64):.4f})")
    assert _guards_intact(buf, m.n_rows)
    assert so.assert_within_any_order_bound(ops.spmv(mg, x.to(gpu)), m, x) <= 1


# ------------------------------------------------------------------------------------------ sliced
def _sliced_runs(s, xg, gpu, blocks=(0, 1)):
    """Every way one SlicedCSR multiplies: both combines, 0 and 1 resident blocks per CU, and on the packed layout the
    fused combine; each into a sentinel-guarded y. Yields (what, y)."""
    for fused in ((False, True) if s.cr is not None else (False,)):
        s.fused_combine = fused
        for combine in (("scan",) if fused else ("scan", "ballot")):
            for b in blocks:
                buf, y = _guarded(s.n_rows, gpu)
                got = s.spmv(xg, y, combine=combine, blocks_per_cu=b)
                assert got.data_ptr() == y.data_ptr()
                yield (f"fused={fused} combine={combine} blocks_per_cu={b}", y)
                assert _guards_intact(buf, s.n_rows)
    s.fused_combine = False


@pytest.mark.parametrize("pack,item_nnz", LAYOUTS)
def test_sliced_every_product_instantiation_exact(gpu, pack, item_nnz):
    """spmv_sliced_kernel<packed, 4 / 6 / 8 / 16> and <unpacked, 8 / 16> on the stripe builder, integer operands:
    exact, for both combines, the fused combine (packed) and 0 / 1 resident blocks per CU. The layout proves what ran:
    rows ending on lane 63, rows starting on lane 0, carries, rows over three stripes, fix entries, rows whose mask
    has every slice bit, and the largest row offset the item size allows — a slice touches only rows with a nonzero
    in it, so an item holds at most item_nnz rows: a row offset of at least 512 (bit 31 of the packed word) and an
    item of 1023 rows are asserted at the 1024-nonzero items, which alone can hold them."""
    m = so.sliced_stripe_edges(item_nnz)
    _, x = so.integer_operands(1, m.n_cols, 41)
    s = ops.SlicedCSR(m.to(gpu), 16, head=0.2, item_nnz=item_nnz, pack=pack)
    assert (s.cr is not None) == pack
    f = so.stripe_features(s)
    assert f["max_item_rows"] == min(item_nnz, 1023) and f["max_row_offset"] == min(item_nnz, 1023) - 1, f
    if item_nnz == 1024:
        assert f["max_row_offset"] >= 512 and f["max_item_rows"] == 1023
        assert not pack or bool((s.cr < 0).any())
    assert min(f["ends_on_lane_63"], f["starts_on_lane_0"], f["carries"], f["three_stripes"], f["fix_entries"],
               f["all_slice_rows"]) > 0, f
    so.assert_exact(so.layout_product(s, x), m, x)  # the layout itself, as the kernels read it
    xg = x.to(gpu)
    for what, y in _sliced_runs(s, xg, gpu):
        try:
            so.assert_exact(y, m, x)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None


@pytest.mark.parametrize("slices,item_nnz", [(8, 1024), (16, 512), (24, 384), (32, 256)])
@pytest.mark.parametrize("head", [0.0, 0.2])
def test_sliced_slice_counts_and_head_exact(gpu, slices, item_nnz, head):
    m = so.sliced_stripe_edges(item_nnz)
    _, x = so.integer_operands(1, m.n_cols, 42)
    s = ops.SlicedCSR(m.to(gpu), slices, head=head, item_nnz=item_nnz)
    assert (s.head_cols > 0) == (head > 0) and s.cr is not None
    f = so.stripe_features(s)
    assert f["all_slice_rows"] > 0 and f["fix_entries"] > 0, f
    if slices == 32:
        assert bool((s.row_mask < 0).any())  # bit 31 of the mask
    for what, y in _sliced_runs(s, x.to(gpu), gpu, blocks=(0,)):
        so.assert_exact(y, m, x)


@pytest.mark.parametrize("slices,pack,item_nnz", [(16, True, 512), (32, True, 256), (16, False, 1024), (32, True, 1024)])
def test_sliced_col_split_staged_exact(gpu, slices, pack, item_nnz):
    """A column-split matrix multiplied in stages — products of phases (0, S/16), then (S/16, S/16), then the
    combine — with the partials poisoned with NaN before the products: exact, and exact in one call."""
    m = so.sliced_stripe_edges(item_nnz)
    _, x = so.integer_operands(1, m.n_cols, 43)
    xg = x.to(gpu)
    for head in (0.0, 0.2):
        s = ops.SlicedCSR(m.to(gpu), slices, head=head, item_nnz=item_nnz, pack=pack, col_split=1640)
        assert s.col_split == 1640 and slices // 2 * [True] == [b <= 1640 for b in s.colbase[:slices // 2]]
        ph = slices // 16
        for combine in ("scan", "ballot"):
            s.ypart.fill_(float("nan")), s.extra.fill_(float("nan"))
            buf, y = _guarded(m.n_rows, gpu)
            s.spmv(xg, stage="products", phases=(0, ph))
            s.spmv(xg, stage="products", phases=(ph, ph))
            assert bool((y == SENT).all())
            s.spmv(xg, y, stage="combine", combine=combine)
            so.assert_exact(y, m, x)
            assert _guards_intact(buf, m.n_rows)
        for what, y in _sliced_runs(s, xg, gpu, blocks=(0,)):
            so.assert_exact(y, m, x)


@pytest.mark.parametrize("name", ["few_columns", "empty_matrix", "one_row"])
def test_sliced_degenerate_layouts_exact(gpu, name):
    """Nonzeros in 3 columns (most slices empty: their waves return at once), no nonzeros at all (all zeros, nothing
    faults) and a single row (split over several items): every layout that applies, 8 and 32 slices."""
    m = getattr(so, name)()
    _, x = so.integer_operands(1, m.n_cols, 44)
    xg = x.to(gpu)
    built = 0
    for pack, item_nnz in LAYOUTS:
        for slices, head in ((8, 0.0), (32, 0.2)):
            if m.nnz == 0 and item_nnz in (256, 384):
                with pytest.raises(PackedLayoutUnavailable):
                    ops.SlicedCSR(m.to(gpu), slices, head=head, item_nnz=item_nnz, pack=pack)
                continue
            s = ops.SlicedCSR(m.to(gpu), slices, head=head, item_nnz=item_nnz, pack=pack)
            assert (s.cr is not None) == (pack and m.nnz > 0)
            built += 1
            if name == "few_columns":
                per_slice = torch.diff(s.meta[slices:2 * slices + 1])
                assert int((per_slice == 0).sum()) >= slices - 3  # empty slices
            if name == "one_row" and slices == 8:
                assert s.fix.shape[0] > 0  # more than 1024 of the row's nonzeros in every slice
            for what, y in _sliced_runs(s, xg, gpu, blocks=(0,)):
                so.assert_exact(y, m, x)
    assert built == (8 if m.nnz == 0 else 12)


@functools.lru_cache(maxsize=None)
def _wide_full_mantissa():
    base = so.wide_matrix()
    val, _ = so.full_mantissa_operands(base.nnz, 1, 51)
    return so.with_values(base, val)


@pytest.mark.parametrize("pack", [True, False])
def test_sliced_column_probes_bit_exact(gpu, pack):
    """The column decode pinned without any summation: on the wide matrix (one slice wider than 2^20 columns, a head)
    x = t e_c for every probe column c (both sides of every slice's first column, of the head boundary, first and
    last column). Every row holding column c must give fl(val * t) bit for bit and every other row zero — a column
    decoded one off, a wrong colbase or an ignored head flag reads another x entry. (Columns are distinct inside a
    row, so a row adds one product to zeros: exact. A row none of whose nonzeros is at c sums signed zeros.)"""
    m = _wide_full_mantissa()
    s = ops.SlicedCSR(m.to(gpu), 8, head=0.1, pack=pack)
    assert (s.cr is not None) == pack and s.head_cols > 0
    widths = [h - l for l, h in zip(s.colbase, s.colbase[1:] + [m.n_cols])]
    assert (1 << 20) < max(widths) < (1 << 21)
    probes = so.probe_columns(s)
    assert len(probes) >= 2 * 7 + 2
    rows = so.rows_of(m)
    t = torch.tensor(1.2345678806304932, dtype=torch.float32)
    xg = torch.zeros(m.n_cols, device=gpu)
    hit = 0
    for c in probes:
        xg[c] = t
        y = s.spmv(xg).cpu()
        xg[c] = 0.0
        at = m.col == c
        want = torch.zeros(m.n_rows, dtype=torch.float32)
        want[rows[at]] = m.val[at] * t  # fp32 on the CPU
        hit += int(at.sum()) > 0
        assert torch.equal(y, want), (c, int((y != want).sum()))
        assert torch.equal(y[rows[at]].view(torch.int32), want[rows[at]].view(torch.int32)), c
    assert hit >= 7  # a slice's first tail column always holds a nonzero
    print(f"column probes pack={pack}: {len(probes)} probes, {hit} on columns with nonzeros")


@functools.lru_cache(maxsize=None)
def _powerlaw_full_mantissa():
    base = ops.powerlaw_csr(30000, 600_000, alpha=2.2, seed=5)
    val, x = so.full_mantissa_operands(base.nnz, base.n_cols, 52)
    return so.with_values(base, val), x


@pytest.mark.parametrize("data", ["powerlaw", "stripe_edges"])
def test_sliced_full_mantissa_within_any_order_bound(gpu, data):
    if data == "powerlaw":
        m, x = _powerlaw_full_mantissa()
    else:
        base = so.sliced_stripe_edges(1024)
        val, x = so.full_mantissa_operands(base.nnz, base.n_cols, 53)
        m = so.with_values(base, val)
    xg = x.to(gpu)
    for pack in (True, False):
        s = ops.SlicedCSR(m.to(gpu), 16, head=0.0625, pack=pack)
        first = None
        for what, y in _sliced_runs(s, xg, gpu, blocks=(0,)):
            worst = so.assert_within_any_order_bound(y, m, x)
            print(f"sliced, {data}, pack={pack}, {what}: worst err / bound = {worst:.4f} (rows of >= 64 nonzeros: "
                  f"{so.worst_ratio(y, m, x, 64):.4f})")
            first = y.clone() if first is None else first
            assert torch.equal(y.view(torch.int32), first.view(torch.int32)), what  # same bits, every form
        assert torch.equal(s.spmv(xg).view(torch.int32), first.view(torch.int32))  # and call to call


# ------------------------------------------------------------------------------------------ banded
def _banded_into(vals, ro, n, geo, xg, y, variant):
    rc = _lib().pcmx_spmv_banded_variant(_p(vals), _p(ro), int(n), *map(int, geo), _p(xg), _p(y), int(variant), _stream())
    assert rc == 0, (rc, n, geo, variant)
    torch.cuda.synchronize()


def _banded_exact_and_bound(gpu, n, geo, label, variants=(0, 1, 8)):
    """One (n, geometry): integer values exact into a guarded y for every variant, then full-mantissa signed values
    within the any-order bound through ops.spmv_banded. Returns the worst err / bound."""
    base = ops.banded_csr(n, *geo)  # row_ptr and the explicit columns, for the reference
    ival, x = so.integer_operands(base.nnz, n, 61)
    m = so.with_values(base, ival)
    ro, xg, vals = m.row_ptr.to(gpu), x.to(gpu), ival.to(gpu)
    assert vals.data_ptr() % 16 == 0
    for v in variants:
        buf, y = _guarded(n, gpu)
        _banded_into(vals, ro, n, geo, xg, y, v)
        try:
            so.assert_exact(y, m, x)
        except AssertionError as e:
            raise AssertionError(f"{label} n={n} variant {v}: {e}") from None
        assert _guards_intact(buf, n), (label, n, v)
    fval, fx = so.full_mantissa_operands(base.nnz, n, 62)
    mf = so.with_values(base, fval)
    worst = 0.0
    for v in variants:
        out = ops.spmv_banded(fval.to(gpu), ro, n, *geo, fx.to(gpu), variant=v)
        worst = max(worst, so.assert_within_any_order_bound(out, mf, fx))
    return worst


@pytest.mark.parametrize("L", sorted(so.BANDED_GEOMETRIES))
def test_banded_every_path_exact(gpu, L):
    """Variants 0, 1 and 8 on every kernel path: n gives unclipped row blocks between clipped ones with a full, a
    one-row and a 15-row last block, and one n below the band reach (every row clipped). pcmx_spmv_banded_path must
    name the expected kernel for each call before it runs."""
    geo, want1, want8 = so.BANDED_GEOMETRIES[L]
    lib = _lib()
    *full, clipped = so.banded_sizes(geo)
    worst = 0.0
    for n in full + [clipped]:
        assert so.banded_path(lib, n, geo, 0) == (0, 0)
        assert so.banded_path(lib, n, geo, 1) == want1
        assert so.banded_path(lib, n, geo, 8) == (want8 if n != clipped else want1)
        worst = max(worst, _banded_exact_and_bound(gpu, n, geo, f"L={L}"))
    print(f"banded L={L} paths variant 1 {want1} variant 8 {want8}: worst err / bound = {worst:.4f}")


def test_banded_geometries_cover_every_path(gpu):
    lib = _lib()
    seen = set()
    for L, (geo, want1, want8) in so.BANDED_GEOMETRIES.items():
        n = so.banded_sizes(geo)[0]
        seen |= {so.banded_path(lib, n, geo, v) for v in (0, 1, 8)}
        assert so.banded_path(lib, n, geo, 1) == want1 and so.banded_path(lib, n, geo, 8) == want8, L
    assert seen == so.ALL_BANDED_PATHS
    assert so.BANDED_GEOMETRIES[257][2][0] == 8 and so.BANDED_GEOMETRIES[639][2][0] == 8  # both ends of the stream
    assert so.BANDED_GEOMETRIES[255][2][0] == 1 and so.BANDED_GEOMETRIES[641][2][0] == 1  # and the fall-backs


@pytest.mark.parametrize("geo", [(41, 20, 0, 20, 5), (41, 20, 10, 20, 0), (41, 0, 10, 0, 5), (1, 3, 5, 2, 3),
                                 (301, 10, 0, 10, 3), (301, 10, 50, 10, 0), (301, 0, 50, 0, 3), (1, 5, 100, 5, 30)])
def test_banded_degenerate_bands_exact(gpu, geo):
    """An empty inner band (c = 0), an empty outer band (e = 0), no gaps (b = d = 0) and a one-column centre (a = 1),
    each short (LDS kernel) and at stream length (variant 8 runs the stream kernel)."""
    a, b, c, d, e = geo
    L = 2 * (a // 2) + 1 + 2 * c + 2 * e
    n = 2 * so.banded_reach(*geo) + 49
    assert so.banded_path(_lib(), n, geo, 8)[0] == (8 if L >= 257 else 1)
    _banded_exact_and_bound(gpu, n, geo, f"degenerate {geo}")


def test_banded_stream_unaligned_values_exact(gpu):
    """Variant 8 on a value view one float into its buffer: the path query says the LDS kernel, and the result is
    exact with nothing written outside y."""
    geo = so.BANDED_GEOMETRIES[621][0]
    n = so.banded_sizes(geo)[1]
    base = ops.banded_csr(n, *geo)
    ival, x = so.integer_operands(base.nnz, n, 63)
    m = so.with_values(base, ival)
    store = torch.zeros(base.nnz + 1, device=gpu)
    store[1:] = ival.to(gpu)
    vals = store[1:]
    aligned = vals.data_ptr() % 16 == 0
    assert not aligned
    assert so.banded_path(_lib(), n, geo, 8, aligned=True) == (8, 10)
    assert so.banded_path(_lib(), n, geo, 8, aligned=aligned) == (1, 10)
    buf, y = _guarded(n, gpu)
    _banded_into(vals, m.row_ptr.to(gpu), n, geo, x.to(gpu), y, 8)
    so.assert_exact(y, m, x)
    assert _guards_intact(buf, n)
    out = ops.spmv_banded(vals, m.row_ptr.to(gpu), n, *geo, x.to(gpu), variant=8)
    so.assert_exact(out, m, x)
