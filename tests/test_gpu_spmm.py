"""ops.spmm on the GPU (csrc/kernels/spmm.hip) against references that leave no slack (tests/_spmm_oracle.py): the
integer families on every k and item size at the planner's cuts, the any-order bound on full-mantissa data, the contract
of the docstring (reproducibility, column independence, empty rows and buffers, operand forms), addresses past 2^31
elements, and the C entry's refusals. Every output lies in a sentinel-filled buffer: ldy = k + 5, 64 sentinels before
the first row and after the last, all checked intact."""
import ctypes
import functools

import pytest
import torch

import _spmm_oracle as mo
from conftest import run_cli
from parallel_c_programs_amd import ops

pytestmark = pytest.mark.gpu

SENT = -12345.0
GUARD = 64
ALL_K = (1, 2, 3, 4, 5, 8, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 513)


def _lib():
    from parallel_c_programs_amd._native import hip_lib

    lib = hip_lib()
    lib.pcmx_spmm_path.restype = ctypes.c_int
    lib.pcmx_spmm_path.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_ulonglong,
                                   ctypes.c_longlong, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    return lib


def path_of(x: torch.Tensor, out: torch.Tensor):
    """(first class, tail class, vector bits) the launcher takes for these operands."""
    k = x.shape[1]
    tail, vec = ctypes.c_int(-1), ctypes.c_int(-1)
    cls = _lib().pcmx_spmm_path(k, x.data_ptr(), max(x.stride(0), k), out.data_ptr(), max(out.stride(0), k),
                                ctypes.byref(tail), ctypes.byref(vec))
    return cls, tail.value, vec.value


class Guarded:
    """An [n_rows, k] output inside a sentinel-filled buffer: `pad` sentinel columns per row, GUARD sentinels before
    the first row and after the last (`shift` more before, to misalign the base)."""

    def __init__(self, n_rows, k, dev, pad=5, shift=0):
        self.ld, self.n, self.k, self.o = k + pad, n_rows, k, GUARD + shift
        self.buf = torch.full((self.o + n_rows * self.ld + GUARD,), SENT, device=dev)
        self.out = self.buf[self.o:self.o + n_rows * self.ld].view(n_rows, self.ld)[:, :k]

    def intact(self):
        body = self.buf[self.o:self.o + self.n * self.ld].view(self.n, self.ld)
        assert bool((self.buf[:self.o] == SENT).all()), "sentinels before the first row overwritten"
        assert bool((self.buf[self.o + self.n * self.ld:] == SENT).all()), "sentinels after the last row overwritten"
        assert bool((body[:, self.k:] == SENT).all()), "padding between k and the row stride overwritten"

    def untouched(self):
        assert bool((self.buf == SENT).all()), "a refused call wrote into Y"


def padded_x(x: torch.Tensor, dev, pad=5):
    """x on the device as a view with leading dimension k + pad; the padding holds NaN (nothing may read it into Y)."""
    n, k = x.shape
    buf = torch.full((n, k + pad), float("nan"), device=dev)
    buf[:, :k] = x.to(dev)
    return buf[:, :k]


def spmm_guarded(m, x, item_nnz=None, pad=5, shift=0):
    g = Guarded(m.n_rows, x.shape[1], x.device, pad, shift)
    r = ops.spmm(m, x, out=g.out, item_nnz=item_nnz)
    assert r is g.out
    g.intact()
    return g.out


@functools.lru_cache(maxsize=None)
def edges_exact():
    """The planner's edge matrix, an integer X of 513 columns and their exact product (column c of the product depends
    on column c of X only, so the first k columns serve every k)."""
    m = mo.csr_item_edges()
    xb = mo.integer_x(m.n_cols, max(ALL_K), 800)
    return m, xb, mo.exact_product_mm(m, xb)


@functools.lru_cache(maxsize=None)
def edges_full_mantissa():
    m = mo.full_mantissa_values(mo.csr_item_edges(), 801)
    return m, mo.full_mantissa_x(m.n_cols, 320, 802)


# ------------------------------------------------------------------------------------------ every k on the planner's cuts
@pytest.mark.parametrize("item_nnz", [1024, 64])
def test_every_k_on_the_planner_cuts(gpu, item_nnz):
    m, xb, exact = edges_exact()
    md = m.to(gpu)
    f = mo.plan_features(md.spmm_plan(item_nnz))
    print(f"item_nnz {item_nnz}: {f}")
    assert f["whole_row"] > 0 and f["multi_row"] > 0 and f["pieces"] > 0 and f["max_rows"] > 1, f
    seen = set()
    for k in ALL_K:
        x = padded_x(xb[:, :k], gpu)
        g = Guarded(m.n_rows, k, gpu)
        cls, tail, vec = path_of(x, g.out)
        assert [c for _, c, _ in mo.width_classes(k)] == [c for c in (cls, tail) if c], (k, cls, tail)
        seen |= {(cls, bool(vec & 1))} | ({(tail, bool(vec & 2))} if tail else set())
        ops.spmm(md, x, out=g.out, item_nnz=item_nnz)
        g.intact()
        try:
            mo.assert_equals_exact(g.out, exact[:, :k], m)
        except AssertionError as e:
            raise AssertionError(f"k = {k}, item_nnz = {item_nnz}, class {cls} tail {tail} vec {vec}: {e}") from None
    want = {(4, False), (8, False), (16, False), (32, False), (64, False), (128, False), (128, True), (256, False),
            (256, True)}
    assert seen == want, f"classes / access forms reached: {sorted(seen)}"


@pytest.mark.parametrize("k", [4, 64, 257])
def test_full_mantissa_within_any_order_bound(gpu, k):
    m, xb = edges_full_mantissa()
    x = xb[:, :k].contiguous()
    for item_nnz in (1024, 64):
        out = spmm_guarded(m.to(gpu), padded_x(x, gpu), item_nnz)
        worst = mo.assert_within_any_order_bound_mm(out, m, x)
        print(f"spmm k={k} item_nnz={item_nnz}: worst err / bound {worst:.3f}")
        empty = torch.nonzero(mo.row_lengths(m) == 0).flatten().to(gpu)
        assert bool((out[empty] == 0).all()) and not bool(torch.signbit(out[empty]).any())  # +0.0


# ------------------------------------------------------------------------------------------ more shapes
SHAPES = {"one_row": mo.one_row, "empty": mo.empty_matrix, "few_columns": mo.few_columns, "one_by_one": mo.one_by_one,
          "no_rows": mo.no_rows, "split_last_row_empty_first": mo.split_last_row}


@pytest.mark.parametrize("item_nnz", [1024, 64])
@pytest.mark.parametrize("name", list(SHAPES))
def test_more_shapes(gpu, name, item_nnz):
    m = SHAPES[name]()
    md = m.to(gpu)
    p = md.spmm_plan(item_nnz)
    if name == "one_row":
        assert p.n_pieces >= 9 and p.split.shape[0] == 1
    if name == "split_last_row_empty_first":
        assert int(p.split[-1, 0]) == m.n_rows - 1 and int(m.row_ptr[1]) == 0
    for k in (0, 3, 40, 130, 257):
        x = mo.integer_x(m.n_cols, k, 810 + k)
        out = spmm_guarded(md, padded_x(x, gpu), item_nnz)
        assert out.shape == (m.n_rows, k)
        mo.assert_exact_mm(out, m, x)


# ------------------------------------------------------------------------------------------ column independence
@pytest.mark.parametrize("k", [4, 64, 257, 320])
def test_hot_column(gpu, k):
    m, xb, exact = edges_exact()
    md = m.to(gpu)
    for c0 in sorted({c for c in (0, 3, 63, 64, 255, 256, k - 1) if c < k}):
        x = torch.zeros(m.n_cols, k)
        x[:, c0] = xb[:, c0]
        out = spmm_guarded(md, padded_x(x, gpu))
        want = torch.zeros(m.n_rows, k, dtype=torch.int64)
        want[:, c0] = exact[:, c0]
        mo.assert_equals_exact(out, want, m)
        assert not bool(torch.signbit(out[:, [c for c in range(k) if c != c0]]).any()), f"-0.0 beside column {c0}"


@pytest.mark.parametrize("k", [16, 320])
def test_column_permutation_bitwise(gpu, k):
    m, xb = edges_full_mantissa()
    md, x = m.to(gpu), xb[:, :k].contiguous().to(gpu)
    perm = torch.randperm(k, generator=torch.Generator().manual_seed(820 + k)).to(gpu)
    a = ops.spmm(md, x)
    b = ops.spmm(md, x[:, perm].contiguous())
    assert torch.equal(b.view(torch.int32), a[:, perm].view(torch.int32))


@pytest.mark.parametrize("k", [5, 257])
def test_nan_inf_reach_exactly_their_entries(gpu, k):
    m, xb = edges_full_mantissa()
    md, x = m.to(gpu), xb[:, :k].contiguous().to(gpu)
    base = spmm_guarded(md, x).clone()
    col, rows = m.col.long(), mo.rows_of(m)
    j = int(torch.bincount(col, minlength=m.n_cols).argmax())
    hit_rows = torch.unique(rows[col == j])
    assert hit_rows.numel() >= 2
    for c, bad in ((0, float("nan")), (k - 1, float("inf")), (k // 2, float("-inf")), (k - 1, float("nan"))):
        xn = x.clone()
        xn[j, c] = bad
        out = spmm_guarded(md, xn)
        pred = torch.zeros(m.n_rows, k, dtype=torch.bool)
        pred[hit_rows, c] = True
        pred = pred.to(gpu)
        special = torch.isnan(out) if bad != bad else torch.isinf(out)
        assert torch.equal(special, pred), f"{bad} at X[{j}, {c}]: {int((special != pred).sum())} entries differ"
        assert torch.equal(out.view(torch.int32)[~pred], base.view(torch.int32)[~pred]), "other entries changed bits"


def test_reproducible_across_calls_and_streams(gpu):
    m, xb = edges_full_mantissa()
    md, x = m.to(gpu), xb.to(gpu)
    for item_nnz in (None, 64):
        first = ops.spmm(md, x, item_nnz=item_nnz)
        torch.cuda.synchronize()
        for s in (torch.cuda.Stream(gpu), torch.cuda.Stream(gpu), torch.cuda.current_stream(gpu)):
            with torch.cuda.stream(s):
                again = ops.spmm(md, x, item_nnz=item_nnz)
            s.synchronize()
            assert torch.equal(again.view(torch.int32), first.view(torch.int32))


# ------------------------------------------------------------------------------------------ operand forms
def test_views(gpu):
    m, xb, exact = edges_exact()
    md = m.to(gpu)
    wide = xb[:, :384].to(gpu)
    # X as a column slice of a wider tensor, read where it lies
    xs = wide[:, 100:228]
    assert xs.stride() == (384, 1) and path_of(xs, torch.empty(m.n_rows, 128, device=gpu))[2] == 1  # float2 form
    mo.assert_equals_exact(ops.spmm(md, xs), exact[:, 100:228], m)
    # a storage offset of 1 and an odd leading dimension at k = 128: dword form
    flat = torch.full((1 + m.n_cols * 131,), float("nan"), device=gpu)
    xo = flat[1:].view(m.n_cols, 131)[:, :128]
    xo.copy_(wide[:, :128])
    g = Guarded(m.n_rows, 128, gpu)
    assert path_of(xo, g.out) == (128, 0, 0)
    ops.spmm(md, xo, out=g.out)
    g.intact()
    mo.assert_equals_exact(g.out, exact[:, :128], m)
    # a non-unit column stride gets the contiguous copy
    mo.assert_equals_exact(ops.spmm(md, wide[:, ::3]), exact[:, :384:3], m)
    mo.assert_equals_exact(ops.spmm(md, wide.t().contiguous().t()[:, :70]), exact[:, :70], m)
    # out= aligned (vector form) and misaligned (dword form), same values
    for k, cls in ((128, 128), (256, 256)):
        x = wide[:, :k].contiguous()
        ga, gm = Guarded(m.n_rows, k, gpu, pad=8), Guarded(m.n_rows, k, gpu, pad=8, shift=1)
        assert path_of(x, ga.out) == (cls, 0, 1) and path_of(x, gm.out) == (cls, 0, 0)
        for g in (ga, gm):
            ops.spmm(md, x, out=g.out)
            g.intact()
            mo.assert_equals_exact(g.out, exact[:, :k], m)


def test_refusals_on_gpu_operands(gpu):
    m = mo.few_columns()
    md = m.to(gpu)
    x = mo.integer_x(m.n_cols, 4, 830).to(gpu)
    g = Guarded(m.n_rows, 4, gpu)
    with pytest.raises(ValueError):
        ops.spmm(md, x[:, 0], out=g.out)
    with pytest.raises(TypeError):
        ops.spmm(md, x.double(), out=g.out)
    with pytest.raises(ValueError):
        ops.spmm(md, x[:-1], out=g.out)
    with pytest.raises(ValueError):
        ops.spmm(md, x.cpu(), out=g.out)  # device mismatch
    with pytest.raises(ValueError):
        ops.spmm(m, x)                    # matrix on the host, X on the GPU
    big = torch.full((m.n_cols + m.n_rows, 4), SENT, device=gpu)
    with pytest.raises(ValueError):
        ops.spmm(md, big[:m.n_cols], out=big[m.n_cols:])
    assert bool((big == SENT).all())
    torch.cuda.synchronize()
    g.untouched()


# ------------------------------------------------------------------------------------------ far offsets
@pytest.mark.parametrize("k", [4, 64, 256])
def test_far_offsets(gpu, k):
    """Rows 2^30 + 64 elements apart from element 2^31 of a zero-filled buffer of 2^32 + 192 + k floats: row 1 starts
    past 2^32 bytes and row 2 past 2^31 elements of the view, and an address that wraps at 32 bits (signed or unsigned,
    in elements or in bytes) still lands inside the zeroed buffer, where it gives a wrong integer."""
    free = torch.cuda.mem_get_info(gpu)[0]
    if free < 48e9:
        print(f"far offsets skipped: {free / 1e9:.1f} GB free, 48 GB needed")
        pytest.skip(f"{free / 1e9:.1f} GB free on the GPU, 48 GB needed")
    ld, base, total = 2 ** 30 + 64, 2 ** 31, 2 ** 32 + 192 + k
    m = mo.dense_3x3()
    x = mo.integer_x(3, k, 840 + k)
    exact = mo.exact_product_mm(m, x)
    bx, by = torch.zeros(total, device=gpu), torch.zeros(total, device=gpu)
    xv, yv = bx.as_strided((3, k), (ld, 1), base), by.as_strided((3, k), (ld, 1), base)
    xv.copy_(x.to(gpu))
    ops.spmm(m.to(gpu), xv, out=yv)
    mo.assert_equals_exact(yv, exact, m)
    starts = [base + r * ld for r in range(3)]
    for buf, vals in ((bx, x), (by, exact.float())):
        assert int(buf.count_nonzero()) == int(vals.count_nonzero()), "stray writes in the buffer"
        # windows around the wrap targets of every row start: modulo 2^32 and 2^31 elements, 2^32 bytes (2^30 elements)
        for s in starts:
            for t in {s % 2 ** 32, s % 2 ** 31, s % 2 ** 30, (4 * s % 2 ** 32) // 4}:
                if t not in starts:
                    assert not bool(buf[max(0, t - 512):t + 512 + k].any()), f"nonzero near wrap target {t}"
    del bx, by, xv, yv
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ C entry and CLI
def test_c_entry_refusals(gpu):
    lib = _lib()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.pcmx_spmm_csr.restype = I
    lib.pcmx_spmm_csr.argtypes = [P, P, P, P, LL, P, LL, I, I, P, LL, P, P, I, LL, I, P, LL, P]
    m = mo.split_last_row().to(gpu)
    k, item = 6, 64
    p = m.spmm_plan(item)
    assert p.n_pieces > 0
    x = mo.integer_x(m.n_cols, k, 850).to(gpu)
    g = Guarded(m.n_rows, k, gpu)
    ws_floats = p.n_pieces * 8
    ws = torch.full((ws_floats + 1,), SENT, device=gpu)

    def call(k=k, ldx=k, ldy=g.ld, item_nnz=item, ws_ptr=ws.data_ptr(), ws_n=ws_floats, n_rows=m.n_rows):
        rc = lib.pcmx_spmm_csr(m.row_ptr.data_ptr(), m.col.data_ptr(), m.val.data_ptr(), x.data_ptr(), ldx,
                               g.out.data_ptr(), ldy, n_rows, k, p.items.data_ptr(), p.items.shape[0],
                               p.slot.data_ptr(), p.split.data_ptr(), p.split.shape[0], p.n_pieces, item_nnz, ws_ptr,
                               ws_n, None)
        torch.cuda.synchronize()
        return rc

    for name, kw in (("k < 0", dict(k=-1)), ("ldx < k", dict(ldx=k - 1)), ("ldy < k", dict(ldy=k - 1)),
                     ("item size 0", dict(item_nnz=0)), ("item size 96 + 4", dict(item_nnz=100)),
                     ("item size 2048", dict(item_nnz=2048)), ("workspace one float short", dict(ws_n=ws_floats - 1)),
                     ("no workspace", dict(ws_ptr=None, ws_n=0)), ("misaligned workspace", dict(ws_ptr=ws.data_ptr() + 4)),
                     ("n_rows < 0", dict(n_rows=-1))):
        assert call(**kw) == -1, name  # PCMX_ERR_ARG
        g.untouched()
        assert bool((ws == SENT).all()), name
    assert call() == 0  # and the same arguments unmodified run
    g.intact()
    mo.assert_exact_mm(g.out, m, x)


def test_cli(gpu):
    r = run_cli("run_spmm", 3000, 40000, "--k", 48, "--matrix", "powerlaw", "--item-nnz", 256)
    assert r.returncode == 0 and "checks_passed" in r.stdout, r.stdout + r.stderr
