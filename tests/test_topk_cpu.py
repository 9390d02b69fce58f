"""ops.topk / ops.kth_value on CPU tensors (the exact torch path) and their argument errors; the TopK workload on the
CPU. The oracle is the first k entries of torch.sort(stable=True), which is also the definition of the ops."""
import pytest
import torch

from parallel_c_programs_amd import ops
from parallel_c_programs_amd.models import WORKLOADS, build_workload
from parallel_c_programs_amd.ops.vector import SORT_MAX_N
from parallel_c_programs_amd.parallel.dist import Context

# NaNs of both signs and several payloads (quiet and signalling), +-0 interleaved, +-inf, a denormal
SPECIAL = [0x7fc00000, 0x7fc00001, 0x7f800001, 0xffc12345 - (1 << 32), 0x7fffffff, 0xffffffff - (1 << 32), 0, -2**31,
           0x7f800000, 0xff800000 - (1 << 32), 1, 0x80000001 - (1 << 32), 0, -2**31]
NAN_BITS = 0x7fffffff


def _bits(t):
    return t.view(torch.int32)


def _canonical(v):
    if v.dtype != torch.float32:
        return v
    v = torch.where(v == 0, torch.zeros_like(v), v)
    return torch.where(torch.isnan(v), torch.full_like(_bits(v), NAN_BITS).view(torch.float32), v)


def _oracle(x, k, largest, sorted_):
    """(value bits, int32 indices) of the first k entries of the stable sort; in index order when not sorted_."""
    xf = x.reshape(-1)
    idx = torch.sort(xf, stable=True, descending=largest).indices[:k]
    if not sorted_:
        idx = torch.sort(idx).values
    return _bits(_canonical(xf[idx])), idx.int()


def _check(x, k, largest, sorted_):
    keep = x.clone()
    vals, idx = ops.topk(x, k, largest=largest, sorted=sorted_)
    rv, ri = _oracle(x, k, largest, sorted_)
    assert vals.dtype == x.dtype and idx.dtype == torch.int32 and vals.shape == idx.shape == (k,)
    assert torch.equal(idx, ri) and torch.equal(_bits(vals), rv)
    assert torch.equal(_bits(x), _bits(keep))  # the input is never written


def _keys(n, dtype):
    g = torch.Generator().manual_seed(100 + n)
    if dtype == torch.float32:
        return (torch.randn(n, generator=g) * 4).round() / 4  # many ties
    x = torch.randint(-2**31, 2**31, (n,), generator=g, dtype=torch.int64)
    x[:4] = torch.tensor([-2**31, 2**31 - 1, 0, -1])[:n]
    return x.to(torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
@pytest.mark.parametrize("n", [1, 2, 257, 5000])
def test_topk_matches_stable_sort_prefix(n, dtype):
    x = _keys(n, dtype)
    for k in sorted({0, 1, 2, n // 2, n - 1, n}):
        if not 0 <= k <= n:
            continue
        for largest in (True, False):
            for sorted_ in (True, False):
                _check(x, k, largest, sorted_)


def test_topk_is_the_sort_prefix():
    x = _keys(5000, torch.float32)
    for largest in (True, False):
        vals, idx = ops.topk(x, 777, largest=largest)
        sv, si = ops.sort(x, descending=largest)
        assert torch.equal(_bits(vals), _bits(sv[:777])) and torch.equal(idx, si[:777])


def test_f32_specials():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, generator=g)
    pos = torch.arange(len(SPECIAL)) * 17 + 2
    _bits(x)[pos] = torch.tensor(SPECIAL, dtype=torch.int32)
    assert torch.isnan(x).sum().item() == 6
    for k in (1, 4, 6, 7, 150, 300):
        for largest in (True, False):
            for sorted_ in (True, False):
                _check(x, k, largest, sorted_)
    vals, idx = ops.topk(x, 8, largest=True)
    assert bool((_bits(vals[:6]) == NAN_BITS).all())  # NaNs lead, canonical
    assert torch.equal(idx[:6], pos[:6].int())  # tied NaNs in index order
    assert _bits(vals[6]).item() == 0x7f800000  # then +inf
    # +-0 tie by index: with the zeros the best remaining keys of a non-negative array
    z = torch.full((64,), -1.0)
    _bits(z)[torch.tensor([5, 9, 30, 41])] = torch.tensor([-2**31, 0, -2**31, 0], dtype=torch.int32)
    vals, idx = ops.topk(z, 3, largest=True)
    assert idx.tolist() == [5, 9, 30] and bool((_bits(vals) == 0).all())  # both zeros come out as +0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_kth_value(dtype):
    x = _keys(5000, dtype)
    for largest in (False, True):
        s = ops.sort_keys(x, descending=largest)
        for k in (1, 2, 2500, 4999, 5000):
            v = ops.kth_value(x, k, largest=largest)
            assert v.dtype == x.dtype and v.shape == () and _bits(v).item() == _bits(s[k - 1]).item()
    assert _bits(ops.kth_value(x, 3)).item() == _bits(ops.sort_keys(x)[2]).item()  # smallest by default
    if dtype == torch.float32:
        y = torch.tensor([1.0, float("nan"), -0.0, 2.0])
        assert _bits(ops.kth_value(y, 1, largest=True)).item() == NAN_BITS
        assert _bits(ops.kth_value(y, 1)).item() == 0  # -0.0 comes out as +0.0


def test_noncontiguous_2d_is_flattened():
    g = torch.Generator().manual_seed(9)
    x = torch.randint(-99, 99, (30, 41), generator=g, dtype=torch.int32).t()
    assert not x.is_contiguous()
    _check(x, 100, True, True)
    _check(x, 100, False, False)


def test_empty_input():
    for dtype in (torch.float32, torch.int32):
        vals, idx = ops.topk(torch.empty(0, dtype=dtype), 0)
        assert vals.dtype == dtype and idx.dtype == torch.int32 and vals.shape == idx.shape == (0,)


def test_argument_errors():
    x = torch.zeros(10)
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.float16)):
        with pytest.raises(TypeError):
            ops.topk(bad, 1)
        with pytest.raises(TypeError):
            ops.kth_value(bad, 1)
    for k in (1.0, True, "3", None):
        with pytest.raises(TypeError):
            ops.topk(x, k)
        with pytest.raises(TypeError):
            ops.kth_value(x, k)
    for k in (-1, 11):
        with pytest.raises(ValueError):
            ops.topk(x, k)
        with pytest.raises(ValueError):
            ops.kth_value(x, k)
    with pytest.raises(ValueError):
        ops.kth_value(x, 0)  # 1-based
    with pytest.raises(ValueError):
        ops.kth_value(torch.empty(0), 1)
    with pytest.raises(ValueError):
        ops.topk(x, 1, method="heap")
    big = torch.zeros(1, dtype=torch.int32).expand(SORT_MAX_N + 1)  # no memory behind it
    with pytest.raises(ValueError):
        ops.topk(big, 1)
    with pytest.raises(ValueError):
        ops.kth_value(big, 1)


@pytest.mark.parametrize("dist", ["uniform", "equal", "sorted"])
def test_workload_on_cpu(dist):
    assert "topk" in WORKLOADS
    for dtype, largest, sorted_ in (("f32", True, True), ("i32", False, False)):
        w = build_workload("topk", Context(device=torch.device("cpu")), n=5000, k=37, dtype=dtype, largest=largest,
                           sorted=sorted_, dist=dist)
        w.step()
        chk = w.check()
        assert chk["check_passed"] and chk["k"] == 37
        assert w.work_per_step() >= 5 * 4 * 5000
        vals, idx = w.torch_step()
        assert vals.shape == (37,)
