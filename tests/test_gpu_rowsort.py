"""Row-wise sort / top-k / k-th value on the GPU (csrc/kernels/rowsort.hip) against torch.sort(dim=-1, stable=True) of a
HOST copy, canonicalised as in tests/test_gpu_sort.py; every comparison is exact (torch.equal on int32 views). Routes
are forced with route= so the default rule cannot hide a kernel; one test runs the default rule over the same shapes.
Shapes: the row lengths at which a kernel changes its keys-per-lane count or its path, every residue of cols % 4 (rows
start at all four misalignments), a partial last block, more blocks than CUs, an odd prime number of rows."""
import ctypes

import pytest
import torch

from conftest import run_cli
from parallel_c_programs_amd import ops
from parallel_c_programs_amd.ops import vector as V

pytestmark = pytest.mark.gpu

W = V.ROWSORT_WAVE_COLS
WAVE_COLS = [1, 2, 3, 63, 64, 65, W - 1, W]
BLOCK_COLS = [W + 1, 1000, 4095, 4097, 16383, 16384]
ROWS = [1, 2, 3, 9, 257, 3001]
MAX_KEYS = 1 << 22
NAN_BITS = 0x7fffffff
SPECIAL = [0x7fc00000, 0x7fc00001, 0x7f800001, 0xffc12345 - (1 << 32), 0x7fffffff, 0xffffffff - (1 << 32), 0, -2**31,
           0x7f800000, 0xff800000 - (1 << 32), 1, 0x80000001 - (1 << 32), 0, -2**31]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    assert torch.equal(_bits(got), _bits(ref.to(got.device)))


def _canonical(v):
    if v.dtype != torch.float32:
        return v
    v = torch.where(v == 0, torch.zeros_like(v), v)
    return torch.where(torch.isnan(v), torch.full_like(_bits(v), NAN_BITS).view(torch.float32), v)


def _oracle(x, descending=False, bits=None):
    """(canonical sorted values, int32 positions) of every row of a host copy of x, both back on x's device."""
    xh = x.cpu()
    key = xh if bits is None else xh.long() & ((1 << bits) - 1)
    idx = torch.sort(key, dim=-1, stable=True, descending=descending).indices
    vals = _canonical(torch.gather(_bits(xh), -1, idx).view(xh.dtype))
    return vals.to(x.device), idx.int().to(x.device)


def _ties(rows, cols, gpu, seed=0):
    g = torch.Generator(device=gpu).manual_seed(seed)
    return torch.round(torch.randn(rows, cols, device=gpu, generator=g) * 64) / 64


def _ints(rows, cols, gpu, seed=0):
    g = torch.Generator(device=gpu).manual_seed(seed)
    return torch.randint(-(1 << 31), 1 << 31, (rows, cols), device=gpu, generator=g, dtype=torch.int64).to(torch.int32)


def _check_sort(x, route, descending=False, bits=None, modes=("keys", "sort", "argsort", "pairs")):
    keep = x.clone()
    rv, ri = _oracle(x, descending, bits)
    if "keys" in modes:
        _same(ops.sort_keys(x, descending, bits, dim=-1, route=route), rv)
    if "sort" in modes:
        v, i = ops.sort(x, descending, bits, dim=-1, route=route)
        _same(v, rv)
        _same(i, ri)
    if "argsort" in modes:
        _same(ops.argsort(x, descending, bits, dim=-1, route=route), ri)
    if "pairs" in modes:
        pay = _bits(_ints(x.shape[0], x.shape[1], x.device, seed=77)).view(torch.float32)  # arbitrary bits, NaNs included
        k, v = ops.sort_by_key(x, pay, descending, bits, dim=-1, route=route)
        _same(k, rv)
        _same(v, torch.gather(_bits(pay), -1, ri.long()).view(torch.float32))
    _same(x, keep)  # the input is never written


def _rows_for(cols):
    return [r for r in ROWS if r * cols <= MAX_KEYS]


@pytest.mark.parametrize("cols", WAVE_COLS)
def test_wave_sort(gpu, cols):
    for rows in _rows_for(cols):
        _check_sort(_ties(rows, cols, gpu, seed=rows), "wave", modes=("keys", "sort") if rows > 9 else ("keys", "sort", "argsort", "pairs"))
    _check_sort(_ints(257, cols, gpu, seed=cols), "wave", descending=True, modes=("sort",))


@pytest.mark.parametrize("cols", BLOCK_COLS)
def test_block_sort(gpu, cols):
    for rows in _rows_for(cols):
        _check_sort(_ties(rows, cols, gpu, seed=rows), "block", modes=("sort",) if rows > 9 else ("keys", "sort", "argsort", "pairs"))
    _check_sort(_ints(9, cols, gpu, seed=cols), "block", descending=True, modes=("sort",))


@pytest.mark.parametrize("cols", [1, 65, W])
def test_block_kernel_takes_short_rows_too(gpu, cols):
    """The forced block route below W (the lab's A/B partner of the wave route)."""
    _check_sort(_ties(9, cols, gpu), "block", modes=("sort", "pairs"))


def test_wave_kernel_up_to_its_own_limit(gpu):
    for cols in (V.ROWSORT_WAVE_MAX_COLS - 1, V.ROWSORT_WAVE_MAX_COLS):
        _check_sort(_ties(9, cols, gpu), "wave", modes=("sort", "pairs"))


@pytest.mark.parametrize("route,cols", [("wave", 65), ("wave", W - 1), ("block", W + 1), ("block", 4097), ("block", 16384)])
def test_sort_properties(gpu, route, cols):
    rows = 9
    # int32 over the full range, both directions
    xi = _ints(rows, cols, gpu, seed=3)
    _check_sort(xi, route)
    _check_sort(xi, route, descending=True)
    # all-equal rows: every key ties, the order is the input order
    _check_sort(torch.full((rows, cols), 0.5, device=gpu), route, modes=("sort",))
    _check_sort(torch.full((rows, cols), -7, device=gpu, dtype=torch.int32), route, descending=True, modes=("sort",))
    # already sorted and reversed rows
    s = torch.sort(_ties(rows, cols, gpu, seed=4), dim=-1).values
    _check_sort(s, route, modes=("sort",))
    _check_sort(s.flip(-1).contiguous(), route, modes=("sort",))
    _check_sort(s, route, descending=True, modes=("sort",))
    # bits: stable by the low bits only, the keys come out unchanged
    xb = _ints(rows, cols, gpu, seed=5) & ((1 << 20) - 1)
    for bits in (1, 8, 9, 20):
        _check_sort(xb, route, bits=bits, modes=("sort", "pairs"))
    _check_sort(xb, route, descending=True, bits=9, modes=("sort",))
    # a signalling-NaN payload keeps its bits
    x = _ties(rows, cols, gpu, seed=6)
    pay = torch.full((rows, cols), 0x7f800001, device=gpu, dtype=torch.int32)
    pay[:, ::2] = 0xffc12345 - (1 << 32)
    _, v = ops.sort_by_key(x, pay.view(torch.float32), dim=-1, route=route)
    _same(v, torch.gather(pay, -1, _oracle(x)[1].long()).view(torch.float32))


def test_float_specials(gpu):
    for route, cols in (("wave", 100), ("block", 1000)):
        x = _ties(3, cols, gpu, seed=8)
        _bits(x)[1, 5:5 + len(SPECIAL)] = torch.tensor(SPECIAL, dtype=torch.int32, device=gpu)
        assert torch.isnan(x[1]).sum().item() == 6
        for descending in (False, True):
            _check_sort(x, route, descending)
            vals = ops.sort_keys(x, descending, dim=-1, route=route)
            nan_at = slice(0, 6) if descending else slice(cols - 6, cols)
            assert bool((_bits(vals)[1, nan_at] == NAN_BITS).all())
            assert not bool((_bits(vals) == -2**31).any())  # both zeros come out as +0.0


# ---------------------------------------------------------------- the C entry points directly: keep, guards, refusals
def _lib():
    from parallel_c_programs_amd._native import hip_lib

    lib = hip_lib()
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    lib.pcmx_row_sort_b32.argtypes = [P, P, P, P, LL, LL, LL, I, I, I, I, I, P]
    lib.pcmx_row_topk_b32.argtypes = [P, LL, LL, LL, I, I, P, P, P]
    lib.pcmx_row_kth_key_b32.argtypes = [P, LL, LL, LL, I, I, P, P]
    for f in (lib.pcmx_row_sort_b32, lib.pcmx_row_topk_b32, lib.pcmx_row_kth_key_b32):
        f.restype = I
    return lib


KEY_I32, KEY_F32, KEYS, PAIRS, INDEX, WAVE, BLOCK = 1, 2, 0, 1, 2, 0x100, 0x200
SENTINEL, GUARD = 0x5a5a5a5a, 16


@pytest.mark.parametrize("route,cols,keep", [(WAVE, 65, 7), (WAVE, W, 1), (BLOCK, W + 1, 129), (BLOCK, 4097, 4096),
                                             (BLOCK, 16383, 33)])
def test_keep_writes_nothing_else(gpu, route, cols, keep):
    """keep < cols into sentinel-filled [rows, keep] outputs with guard words on both sides: the outputs equal the first
    keep columns of the oracle (a store past keep would land in the next row) and the guards are intact."""
    lib, rows = _lib(), 11
    x = _ties(rows, cols, gpu, seed=9)
    x_before = x.clone()
    rv, ri = _oracle(x)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    ko = torch.full((GUARD + rows * keep + GUARD,), SENTINEL, device=gpu, dtype=torch.int32)
    vo = ko.clone()
    rc = lib.pcmx_row_sort_b32(x.data_ptr(), ko.data_ptr() + 4 * GUARD, None, vo.data_ptr() + 4 * GUARD, rows, cols, keep,
                               KEY_F32, INDEX | route, 0, 0, 32, stream)
    assert rc == 0
    torch.cuda.synchronize(gpu)
    for buf in (ko, vo):
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
    _same(ko[GUARD:-GUARD].view(rows, keep), _bits(rv[:, :keep].contiguous()))
    _same(vo[GUARD:-GUARD].view(rows, keep), ri[:, :keep].contiguous())
    _same(x, x_before)


def test_c_abi_refusals(gpu):
    lib = _lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    x = _ties(4, 100, gpu)
    out = torch.full((4, 100), SENTINEL, device=gpu, dtype=torch.int32)
    out2 = out.clone()
    xp, op, o2 = x.data_ptr(), out.data_ptr(), out2.data_ptr()
    sort = lib.pcmx_row_sort_b32
    ok_args = dict(ki=xp, ko=op, vi=None, vo=None, rows=4, cols=100, keep=100, kt=KEY_F32, mode=KEYS, desc=0, b=0, e=32)

    def call(**kw):
        a = {**ok_args, **kw}
        return sort(a["ki"], a["ko"], a["vi"], a["vo"], a["rows"], a["cols"], a["keep"], a["kt"], a["mode"], a["desc"], a["b"],
                    a["e"], stream)

    bad = [dict(kt=3), dict(kt=-1), dict(mode=3), dict(mode=KEYS | WAVE | BLOCK), dict(ki=None), dict(ko=None),
           dict(ki=xp + 4), dict(ko=op + 4), dict(keep=101), dict(keep=-1), dict(rows=-1), dict(cols=-1),
           dict(cols=V.ROWSORT_MAX_COLS + 1, rows=1), dict(rows=1 << 20, cols=1 << 10), dict(b=-1), dict(e=33), dict(b=8, e=8),
           dict(ko=xp), dict(ko=xp + 16), dict(mode=PAIRS), dict(mode=PAIRS, vi=xp, vo=None), dict(mode=INDEX, vo=None),
           dict(mode=INDEX, vo=op), dict(mode=PAIRS, vi=o2, vo=o2), dict(mode=INDEX, vo=o2 + 4),
           dict(mode=KEYS | WAVE, cols=V.ROWSORT_WAVE_MAX_COLS + 1, rows=1, keep=1)]
    for kw in bad:
        assert call(**kw) != 0, kw
    for kw in (dict(rows=0), dict(cols=0, keep=0), dict(keep=0)):
        assert call(**kw) == 0, kw
    topk, kth = lib.pcmx_row_topk_b32, lib.pcmx_row_kth_key_b32
    assert topk(xp, 4, 100, 101, KEY_F32, 1, op, o2, stream) != 0
    assert topk(xp, 4, 100, 5, 7, 1, op, o2, stream) != 0
    assert topk(None, 4, 100, 5, KEY_F32, 1, op, o2, stream) != 0
    assert topk(xp, 4, 100, 5, KEY_F32, 1, None, o2, stream) != 0
    assert topk(xp, 4, 100, 5, KEY_F32, 1, op, None, stream) != 0
    assert topk(xp, 4, 100, 5, KEY_F32, 1, op, op, stream) != 0
    assert topk(xp, 4, 100, 5, KEY_F32, 1, xp, o2, stream) != 0
    assert topk(xp, 4, 100, 5, KEY_F32, 1, op + 4, o2, stream) != 0
    assert topk(xp, 1 << 20, 1 << 10, 5, KEY_F32, 1, op, o2, stream) != 0
    assert topk(xp, 4, 100, 0, KEY_F32, 1, op, o2, stream) == 0
    assert topk(xp, 0, 100, 0, KEY_F32, 1, op, o2, stream) == 0
    assert kth(xp, 4, 100, 101, KEY_F32, 0, op, stream) != 0
    assert kth(xp, 4, 100, 5, 3, 0, op, stream) != 0
    assert kth(xp, 4, 100, 5, KEY_F32, 0, None, stream) != 0
    assert kth(xp, 4, 100, 5, KEY_F32, 0, xp, stream) != 0
    assert kth(xp, 4, 100, 5, KEY_F32, 0, op + 8, stream) != 0
    assert kth(xp, 0, 100, 5, KEY_F32, 0, op, stream) == 0
    torch.cuda.synchronize(gpu)
    assert bool((out == SENTINEL).all()) and bool((out2 == SENTINEL).all())  # nothing was launched
    # and through the op layer
    t = torch.ops.pcmx
    for f in (lambda: t.row_sort(x, None, 101, KEYS, False, 0, 32, True), lambda: t.row_sort(x, None, 100, 3, False, 0, 32, True),
              lambda: t.row_sort(x, None, 100, KEYS, False, 0, 33, True), lambda: t.row_topk(x, 101, True),
              lambda: t.row_kth(x, 101, False),
              lambda: t.row_sort(torch.zeros(1, V.ROWSORT_MAX_COLS + 1, device=gpu), None, 1, KEYS, False, 0, 32, True),
              lambda: t.row_sort(torch.zeros(1, V.ROWSORT_WAVE_MAX_COLS + 1, device=gpu), None, 1, KEYS | WAVE, False, 0, 32, True)):
        with pytest.raises(RuntimeError, match="failed"):
            f()
    with pytest.raises(RuntimeError):
        t.row_sort(x.reshape(-1), None, 1, KEYS, False, 0, 32, True)  # not 2-D


# ---------------------------------------------------------------- select (top-k, k-th value)
def _select_rows(rows, cols, gpu, seed):
    """Rows with a different threshold and a different need_eq each: small integers (heavy ties) shifted and scaled per
    row. With three or more rows the last row is all-equal, and row 1 is all 1.0 but 37 scattered keys of 2.0 and 37 of
    0.0 (37 better keys for either direction, the tie cut wherever k - 37 falls: mid-chunk for most k)."""
    g = torch.Generator(device=gpu).manual_seed(seed)
    span = torch.arange(rows, device=gpu)[:, None] % 7 + 3
    x = (torch.randint(0, 1 << 30, (rows, cols), device=gpu, generator=g) % span + torch.arange(rows, device=gpu)[:, None]).float()
    if rows >= 3:
        x[-1] = 4.0
    if rows >= 3 and cols > 200:
        x[1] = 1.0
        at = (torch.arange(37, device=gpu) * (cols // 37 - 1) + 3)
        x[1, at] = 2.0
        x[1, at + 1] = 0.0
    return x


def _ks(cols):
    return sorted({k for k in (1, 2, 64, 65, cols // 2, cols - 1, cols) if 1 <= k <= cols})


@pytest.mark.parametrize("cols", [5, 513, 16385, 40000, 131075])
def test_select(gpu, cols):
    for rows in (1, 3, 70):
        x = _select_rows(rows, cols, gpu, seed=cols + rows)
        before = x.clone()
        for largest in (True, False):
            rv, ri = _oracle(x, descending=largest)
            for k in _ks(cols):
                v, i = ops.topk(x, k, largest, True, dim=-1, route="select")
                _same(v, rv[:, :k].contiguous())
                _same(i, ri[:, :k].contiguous())
                ui, o = torch.sort(ri[:, :k], dim=-1)  # sorted=False: the same elements in ascending position
                v, i = ops.topk(x, k, largest, False, dim=-1, route="select")
                _same(i, ui.contiguous())
                _same(v, torch.gather(rv[:, :k], -1, o))
                _same(ops.kth_value(x, k, largest, dim=-1), rv[:, k - 1].contiguous())
        _same(x, before)


@pytest.mark.parametrize("dtype", ["i32", "f32-specials"])
def test_select_other_keys(gpu, dtype):
    cols = 1541
    if dtype == "i32":
        x = _ints(5, cols, gpu, seed=1)
        x[2] = x[2] >> 24  # ties
    else:
        x = _ties(5, cols, gpu, seed=2)
        _bits(x)[1, 700:700 + len(SPECIAL)] = torch.tensor(SPECIAL, dtype=torch.int32, device=gpu)
        _bits(x)[3, ::3] = 0x7fc00001  # a third of a row NaN: the NaNs tie, lowest positions first
    for largest in (True, False):
        rv, ri = _oracle(x, descending=largest)
        for k in (1, 5, 6, 7, 600, cols):
            for route in ("select", "sortkeep"):
                v, i = ops.topk(x, k, largest, True, dim=-1, route=route)
                _same(v, rv[:, :k].contiguous())
                _same(i, ri[:, :k].contiguous())
            _same(ops.kth_value(x, k, largest, dim=-1), rv[:, k - 1].contiguous())


@pytest.mark.parametrize("cols", [3, 65, W, W + 1, 4097, 16384])
def test_topk_sortkeep(gpu, cols):
    x = _ties(9, cols, gpu, seed=cols)
    for largest in (True, False):
        rv, ri = _oracle(x, descending=largest)
        for k in _ks(cols):
            v, i = ops.topk(x, k, largest, True, dim=-1, route="sortkeep")
            _same(v, rv[:, :k].contiguous())
            _same(i, ri[:, :k].contiguous())
            ui, o = torch.sort(ri[:, :k], dim=-1)
            v, i = ops.topk(x, k, largest, False, dim=-1, route="sortkeep")
            _same(i, ui.contiguous())
            _same(v, torch.gather(rv[:, :k], -1, o))


def test_topk_loop_route(gpu):
    x = _ties(2, 50000, gpu)
    rv, ri = _oracle(x, descending=True)
    v, i = ops.topk(x, 100, dim=-1, route="loop")
    _same(v, rv[:, :100].contiguous())
    _same(i, ri[:, :100].contiguous())


# ---------------------------------------------------------------- long rows, default routes, layouts
@pytest.mark.parametrize("rows,cols,route", [(3, 16385, "global"), (40, 20000, "global"), (2, 50000, "loop")])
def test_long_sort_routes(gpu, rows, cols, route):
    _check_sort(_ties(rows, cols, gpu, seed=rows), route)
    _check_sort(_ints(rows, cols, gpu, seed=rows), route, descending=True, modes=("sort",))
    xb = _ints(rows, cols, gpu, seed=5) & ((1 << 20) - 1)
    _check_sort(xb, route, bits=9, modes=("sort", "pairs"))


def test_default_routes(gpu):
    for cols in WAVE_COLS + BLOCK_COLS + [16385]:
        for rows in (3, 257):
            if rows * cols <= MAX_KEYS:
                x = _ties(rows, cols, gpu, seed=cols)
                _check_sort(x, None, modes=("sort",))
                rv, ri = _oracle(x, descending=True)
                for k in {1, min(cols, 64), cols}:
                    v, i = ops.topk(x, k, dim=-1)
                    _same(v, rv[:, :k].contiguous())
                    _same(i, ri[:, :k].contiguous())


def test_dims_and_layouts(gpu):
    x = _ties(300, 70, gpu, seed=1)
    rv, ri = _oracle(x.t().contiguous())
    v, i = ops.sort(x, dim=0)  # dim=0 of a 2-D tensor
    _same(v, rv.t())
    _same(i, ri.t())
    _same(ops.topk(x, 5, False, dim=0)[1], ri.t()[:5])
    _same(ops.kth_value(x, 5, dim=0), rv[:, 4].contiguous())
    y = _ties(6 * 5, 700, gpu, seed=2).view(6, 5, 700)  # 3-D, last and middle dims
    rv, ri = _oracle(y.view(30, 700))
    _same(ops.sort(y, dim=-1)[1], ri.view(6, 5, 700))
    _same(ops.sort_keys(y, dim=2), rv.view(6, 5, 700))
    rv, ri = _oracle(y.movedim(1, -1).reshape(-1, 5))
    _same(ops.argsort(y, dim=1), ri.view(6, 700, 5).movedim(-1, 1))
    z = _ties(40, 2000, gpu, seed=3)[::3, 5:1500:2]  # a sliced, non-contiguous view (and a misaligned first key)
    assert not z.is_contiguous()
    rv, ri = _oracle(z.contiguous())
    v, i = ops.sort(z, dim=-1)
    _same(v, rv)
    _same(i, ri)
    _same(ops.topk(z, 9, dim=-1, route="select")[1], _oracle(z.contiguous(), True)[1][:, :9].contiguous())


def test_same_bits_on_every_call(gpu):
    x = _ties(257, 1000, gpu, seed=4)
    for f in (lambda: ops.sort(x, dim=-1), lambda: ops.topk(x, 65, dim=-1, route="select"),
              lambda: ops.topk(x, 65, dim=-1, route="sortkeep"), lambda: ops.sort(x[:, :100], dim=-1)):
        a, b = f(), f()
        for s, t in zip(a, b):
            _same(s, t)


def test_run_rowsort_cli(gpu):
    r = run_cli("run_rowsort", 300, 1000, "--mode", "topk", "--k", 33, "--descending", "--dtype", "i32", "--steps", 2,
                "--warmup", 1, check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.endswith("Gkeys/s") for ln in lines)
    assert any(ln.endswith("GB/s") for ln in lines)
    assert '"check_passed": true' in r.stdout and '"elements_checked": 300000' in r.stdout
