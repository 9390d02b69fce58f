"""Row-wise sort / argsort / top-k / k-th value (dim=) on the host path: every row's result equals the 1-D op applied to
that row, bit for bit, with torch's output shapes; the refusals; dim=None unchanged; the workload. No GPU needed."""
import itertools

import pytest
import torch

from parallel_c_programs_amd import ops
from parallel_c_programs_amd.models import WORKLOADS, build_workload
from parallel_c_programs_amd.ops import vector as V
from parallel_c_programs_amd.parallel.dist import Context

# the float specials of tests/test_gpu_topk.py: six NaNs (quiet, signalling, negative, all-ones), both zeros twice,
# both infinities, the smallest denormals of either sign
SPECIAL = [0x7fc00000, 0x7fc00001, 0x7f800001, 0xffc12345 - (1 << 32), 0x7fffffff, 0xffffffff - (1 << 32), 0, -2**31,
           0x7f800000, 0xff800000 - (1 << 32), 1, 0x80000001 - (1 << 32), 0, -2**31]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(_bits(a), _bits(b))


def _keys(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        return torch.round(torch.randn(shape, generator=g) * 8) / 8  # ties in every row
    return torch.randint(-(1 << 31), 1 << 31, shape, generator=g, dtype=torch.int64).to(torch.int32)


def _per_row(x, dim, f, out_cols):
    """f applied to every 1-D row of x along dim, stacked back into torch's output shape (out_cols along dim; None
    removes dim)."""
    xm = x.movedim(dim, -1)
    rows = [f(r) for r in xm.reshape(-1, xm.shape[-1])]
    if out_cols is None:
        return torch.stack(rows).reshape(xm.shape[:-1])
    return torch.stack(rows).reshape(*xm.shape[:-1], out_cols).movedim(-1, dim)


SHAPES_DIMS = [((7,), 0), ((7,), -1), ((5, 9), 0), ((5, 9), 1), ((5, 9), -1), ((5, 9), -2), ((3, 4, 6), 0), ((3, 4, 6), 1),
               ((3, 4, 6), -1), ((3, 4, 6), -2)]


@pytest.mark.parametrize("shape,dim", SHAPES_DIMS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
@pytest.mark.parametrize("descending", [False, True])
def test_sort_family_equals_the_1d_op_per_row(shape, dim, dtype, descending):
    x = _keys(shape, dtype, seed=len(shape) * 10 + dim % len(shape))
    v = _keys(shape, torch.int32, seed=99)
    keep = x.clone()
    n = x.shape[dim]
    _same(ops.sort_keys(x, descending, dim=dim), _per_row(x, dim, lambda r: ops.sort_keys(r, descending), n))
    sv, si = ops.sort(x, descending, dim=dim)
    _same(sv, _per_row(x, dim, lambda r: ops.sort(r, descending)[0], n))
    _same(si, _per_row(x, dim, lambda r: ops.sort(r, descending)[1], n))
    _same(ops.argsort(x, descending, dim=dim), si)
    kk, vv = ops.sort_by_key(x, v, descending, dim=dim)
    _same(kk, sv)
    _same(vv, torch.gather(v, dim % x.dim(), si.long()))
    assert sv.shape == x.shape and si.dtype == torch.int32
    _same(x, keep)


@pytest.mark.parametrize("shape,dim", SHAPES_DIMS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
@pytest.mark.parametrize("largest", [False, True])
def test_topk_and_kth_equal_the_1d_op_per_row(shape, dim, dtype, largest):
    x = _keys(shape, dtype, seed=7)
    n = x.shape[dim]
    for k in sorted({0, 1, 2, n // 2, n - 1, n}):
        for srt in (True, False):
            v, i = ops.topk(x, k, largest, srt, dim=dim)
            if k == 0:
                assert v.shape == i.shape and v.shape[dim] == 0 and v.numel() == 0
                continue
            _same(v, _per_row(x, dim, lambda r: ops.topk(r, k, largest, srt)[0], k))
            _same(i, _per_row(x, dim, lambda r: ops.topk(r, k, largest, srt)[1], k))
        if k >= 1:
            _same(ops.kth_value(x, k, largest, dim=dim), _per_row(x, dim, lambda r: ops.kth_value(r, k, largest), None))


def test_non_contiguous_input():
    base = _keys((6, 20), torch.float32, seed=3)
    x = base[::2, 1::3]
    assert not x.is_contiguous()
    _same(ops.sort(x, dim=1)[1], ops.sort(x.contiguous(), dim=1)[1])
    _same(ops.sort(x.t(), dim=0)[0], ops.sort(x.contiguous(), dim=1)[0].t())
    _same(ops.topk(x, 3, dim=-1)[1], ops.topk(x.contiguous(), 3, dim=-1)[1])


@pytest.mark.parametrize("bits", [1, 8, 9, 20])
def test_bits_sorts_by_the_low_bits(bits):
    x = torch.randint(0, 1 << 20, (4, 50), generator=torch.Generator().manual_seed(bits), dtype=torch.int32)
    sv, si = ops.sort(x, bits=bits, dim=1)
    _same(sv, _per_row(x, 1, lambda r: ops.sort(r, bits=bits)[0], 50))
    _same(si, _per_row(x, 1, lambda r: ops.sort(r, bits=bits)[1], 50))
    with pytest.raises(TypeError):
        ops.sort(x.float(), bits=bits, dim=1)


@pytest.mark.parametrize("descending", [False, True])
def test_float_specials(descending):
    x = _keys((3, 40), torch.float32, seed=5)
    _bits(x)[1, 2:2 + len(SPECIAL)] = torch.tensor(SPECIAL, dtype=torch.int32)
    x = _bits(x).view(torch.float32)
    _bits(x)[1, 2:2 + len(SPECIAL)] = torch.tensor(SPECIAL, dtype=torch.int32)
    assert torch.isnan(x[1]).sum().item() == 6
    sv, si = ops.sort(x, descending, dim=-1)
    _same(sv, _per_row(x, 1, lambda r: ops.sort(r, descending)[0], 40))
    _same(si, _per_row(x, 1, lambda r: ops.sort(r, descending)[1], 40))
    nan_at = slice(0, 6) if descending else slice(34, 40)
    assert bool((_bits(sv)[1, nan_at] == 0x7fffffff).all())
    assert not bool((_bits(sv) == -2**31).any())  # both zeros come out as +0.0
    ks, vs = ops.sort_by_key(x, x, descending, dim=-1)  # payloads are moved as bits: the NaN payloads survive
    assert sorted(_bits(vs)[1][torch.isnan(vs[1])].tolist()) == sorted(SPECIAL[:6])
    v, i = ops.topk(x, 7, largest=descending, dim=-1)
    _same(v, sv[:, :7])
    _same(i, si[:, :7])
    _same(ops.kth_value(x, 7, largest=descending, dim=-1), sv[:, 6])


def test_empty_shapes_and_k_edges():
    for shape in ((0, 5), (4, 0)):
        x = torch.zeros(shape)
        for dim in (0, 1):
            sv, si = ops.sort(x, dim=dim)
            assert sv.shape == x.shape and si.shape == x.shape and si.dtype == torch.int32
            assert ops.sort_keys(x, dim=dim).shape == x.shape and ops.argsort(x, dim=dim).shape == x.shape
            v, i = ops.topk(x, 0, dim=dim)
            want = list(shape)
            want[dim] = 0
            assert list(v.shape) == want and list(i.shape) == want
    assert ops.kth_value(torch.zeros(0, 5), 2, dim=1).shape == (0,)
    x = _keys((3, 6), torch.int32, seed=1)
    v, i = ops.topk(x, 6, dim=1)  # k == cols: the whole sort
    _same(v, ops.sort(x, True, dim=1)[0])
    _same(i, ops.sort(x, True, dim=1)[1])


def test_refusals():
    x = _keys((3, 6), torch.float32)
    for dim in (2, -3):
        for call in (lambda: ops.sort(x, dim=dim), lambda: ops.sort_keys(x, dim=dim), lambda: ops.argsort(x, dim=dim),
                     lambda: ops.sort_by_key(x, x, dim=dim), lambda: ops.topk(x, 1, dim=dim),
                     lambda: ops.kth_value(x, 1, dim=dim)):
            with pytest.raises(IndexError):
                call()
    with pytest.raises(IndexError):
        ops.sort(torch.tensor(1.0), dim=0)
    with pytest.raises(TypeError):
        ops.sort(x, dim=1.0)
    with pytest.raises(ValueError):
        ops.topk(x, 7, dim=1)       # k > size(dim)
    with pytest.raises(ValueError):
        ops.topk(x, 4, dim=0)
    with pytest.raises(ValueError):
        ops.kth_value(x, 0, dim=1)
    with pytest.raises(ValueError):
        ops.kth_value(x, 7, dim=1)
    with pytest.raises(ValueError):
        ops.sort(x, dim=1, route="fast")          # bad route
    with pytest.raises(ValueError):
        ops.topk(x, 2, dim=1, route="wave")       # a sort route is no top-k route
    with pytest.raises(ValueError):
        ops.sort(x, route="wave")                 # route needs dim
    with pytest.raises(ValueError):
        ops.topk(x, 2, dim=1, method="select")    # method is for dim=None
    with pytest.raises(ValueError):
        ops.sort_by_key(x, x[:, :3], dim=1)
    with pytest.raises(TypeError):
        ops.sort(x.double(), dim=1)
    # a route that cannot take the shape
    long_row = torch.zeros(2, V.ROWSORT_MAX_COLS + 1)
    with pytest.raises(ValueError):
        ops.sort(long_row, dim=1, route="block")
    with pytest.raises(ValueError):
        ops.sort(long_row, dim=1, route="wave")
    with pytest.raises(ValueError):
        ops.sort(torch.zeros(2, V.ROWSORT_WAVE_MAX_COLS + 1), dim=1, route="wave")
    with pytest.raises(ValueError):
        ops.topk(long_row, 3, dim=1, route="sortkeep")
    # routes that can take it are accepted (and ignored) on the host
    for route in ("loop", "global"):
        assert ops.sort_keys(long_row, dim=1, route=route).shape == long_row.shape
    assert ops.topk(long_row, 3, dim=1, route="select")[0].shape == (2, 3)


def test_default_route_rule():
    W, M = V.ROWSORT_WAVE_COLS, V.ROWSORT_MAX_COLS
    assert W <= V.ROWSORT_WAVE_MAX_COLS < M
    assert V._sort_route(None, 10, W, "t") == "wave" and V._sort_route(None, 10, W + 1, "t") == "block"
    assert V._sort_route(None, 10, M, "t") == "block"
    assert V._sort_route(None, 1, M + 1, "t") == "loop" and V._sort_route(None, 2, M + 1, "t") == "global"
    assert V._sort_route(None, 2, V.ROWSORT_LOOP_MIN_COLS, "t") == "loop"
    assert V._sort_route(None, 2, V.ROWSORT_LOOP_MIN_COLS - 1, "t") == "global"
    assert V._topk_route(None, 10, M, M, "t") == "sortkeep" and V._topk_route(None, 10, M, 1, "t") == "select"
    assert V._topk_route(None, 10, M + 1, M + 1, "t") == "select"
    assert V._topk_route(None, 3, 3 * V.ROW_TOPK_LOOP_COLS_PER_ROW, 5, "t") == "loop"
    assert V._topk_route(None, 3, 3 * V.ROW_TOPK_LOOP_COLS_PER_ROW - 1, 5, "t") == "select"


def test_dim_none_is_unchanged():
    x = _keys((4, 9), torch.float32, seed=2)
    v = _keys((4, 9), torch.int32, seed=3)
    _same(ops.sort_keys(x, dim=None), ops.sort_keys(x))
    for a, b in zip(ops.sort(x, True, dim=None), ops.sort(x, True)):
        _same(a, b)
    _same(ops.argsort(x, dim=None), ops.argsort(x))
    for a, b in zip(ops.sort_by_key(x, v, dim=None), ops.sort_by_key(x, v)):
        _same(a, b)
    for a, b in zip(ops.topk(x, 5, dim=None), ops.topk(x, 5)):
        _same(a, b)
    _same(ops.kth_value(x, 5, dim=None), ops.kth_value(x, 5))
    assert ops.sort_keys(x).shape == (36,)  # still flattened


@pytest.mark.parametrize("mode,dtype,descending", list(itertools.product(["keys", "index", "pairs", "topk", "kth"],
                                                                           ["f32", "i32"], [False, True])))
def test_workload_on_cpu(mode, dtype, descending):
    assert "rowsort" in WORKLOADS
    w = build_workload("rowsort", Context(device=torch.device("cpu")), rows=13, cols=70, k=9, mode=mode, dtype=dtype,
                       descending=descending)
    w.step()
    r = w.check()
    assert r["check_passed"] and r["elements_checked"] == 13 * 70
    w.torch_step()
    assert w.work_per_step() > 0
    # the check has power: one changed output element fails it
    w.out[0].view(-1)[3] += 1
    assert not w.check()["check_passed"]
    with pytest.raises(ValueError):
        build_workload("rowsort", Context(device=torch.device("cpu")), rows=2, cols=5, k=6, mode="topk")
    with pytest.raises(ValueError):
        build_workload("rowsort", Context(device=torch.device("cpu")), mode="sideways")
