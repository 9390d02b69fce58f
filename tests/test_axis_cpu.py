"""Reduce and scan along a dimension (dim= on ops.reduce and ops.scan) on the host path: the per-row definition with
torch's shapes, int32 wraparound, NaN isolation, empty extents, the refusals, dim=None unchanged, the default route rule
and the workload. No GPU needed."""
import itertools

import pytest
import torch

from parallel_c_programs_amd import ops
from parallel_c_programs_amd.models import WORKLOADS, build_workload
from parallel_c_programs_amd.ops import vector as V
from parallel_c_programs_amd.parallel.dist import Context

from test_rowsort_cpu import SHAPES_DIMS

OPS = ("sum", "min", "max")
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def _bits(t):
    return t.contiguous().view(torch.int32)


def _data(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        return torch.round(torch.randn(shape, generator=g) * 8) / 8  # ties in every row, sums exact in any order
    return torch.randint(I32_MIN, I32_MAX + 1, shape, generator=g, dtype=torch.int64).to(torch.int32)


def _wrap(t):
    return (((t + 2**31) % 2**32) - 2**31).int()


def _row_reduce(r, op):
    if op == "sum":
        return _wrap(r.long().sum()) if r.dtype == torch.int32 else r.double().sum().float()
    return r.min() if op == "min" else r.max()


def _row_scan(r, op, exclusive):
    """The definition, element by element: out[i] = op(r[0..i]) or op(r[0..i-1]), the identity for an empty prefix."""
    ident = {"sum": 0, "min": float("inf") if r.dtype == torch.float32 else I32_MAX,
             "max": float("-inf") if r.dtype == torch.float32 else I32_MIN}[op]
    out = []
    for i in range(r.numel()):
        pre = r[:i] if exclusive else r[:i + 1]
        out.append(torch.tensor(ident, dtype=r.dtype) if pre.numel() == 0 else _row_reduce(pre, op))
    return torch.stack(out) if out else r.clone()


def _per_row(x, dim, f, keep):
    xm = x.movedim(dim, -1)
    rows = [f(r) for r in xm.reshape(-1, xm.shape[-1])]
    if not keep:
        return torch.stack(rows).reshape(xm.shape[:-1])
    return torch.stack(rows).reshape(xm.shape).movedim(-1, dim)


@pytest.mark.parametrize("shape,dim", SHAPES_DIMS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
@pytest.mark.parametrize("op", OPS)
def test_reduce_equals_the_per_row_oracle(shape, dim, dtype, op):
    x = _data(shape, dtype, seed=len(shape) * 10 + dim % len(shape))
    keep = x.clone()
    want = _per_row(x, dim, lambda r: _row_reduce(r, op), False)
    got = ops.reduce(x, op, dim)
    assert got.dtype == dtype and got.shape == want.shape and torch.equal(got, want)
    kd = ops.reduce(x, op, dim=dim, keepdim=True)
    assert kd.shape == want.unsqueeze(dim % x.dim()).shape and torch.equal(kd.squeeze(dim % x.dim()), want)
    assert torch.equal(_bits(x), _bits(keep))


@pytest.mark.parametrize("shape,dim", SHAPES_DIMS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("exclusive", [False, True])
def test_scan_equals_the_per_row_oracle(shape, dim, dtype, op, exclusive):
    x = _data(shape, dtype, seed=len(shape) * 10 + dim % len(shape) + 1)
    keep = x.clone()
    want = _per_row(x, dim, lambda r: _row_scan(r, op, exclusive), True)
    got = ops.scan(x, exclusive, dim=dim, op=op)
    assert got.dtype == dtype and got.shape == x.shape and torch.equal(got, want)
    assert torch.equal(_bits(x), _bits(keep))
    out = torch.empty_like(x)
    assert ops.scan(x, exclusive, dim=dim, op=op, out=out) is out and torch.equal(out, want)
    y = x.clone()
    assert ops.scan(y, exclusive, dim=dim, op=op, out=y) is y and torch.equal(y, want)  # in place


def test_int32_wraparound_and_exclusive_identities():
    x = torch.full((2, 5), I32_MAX, dtype=torch.int32)
    assert ops.reduce(x, "sum", dim=1).tolist() == [_wrap(torch.tensor(5 * I32_MAX)).item()] * 2
    assert ops.scan(x, dim=1)[0].tolist() == [_wrap(torch.tensor((i + 1) * I32_MAX)).item() for i in range(5)]
    assert ops.scan(x, True, dim=1, op="sum")[:, 0].tolist() == [0, 0]
    assert ops.scan(x, True, dim=1, op="min")[:, 0].tolist() == [I32_MAX] * 2
    assert ops.scan(x, True, dim=1, op="max")[:, 0].tolist() == [I32_MIN] * 2
    xf = x.float()
    assert ops.scan(xf, True, dim=0, op="min")[0].tolist() == [float("inf")] * 5
    assert ops.scan(xf, True, dim=0, op="max")[0].tolist() == [float("-inf")] * 5
    assert ops.scan(xf, True, dim=0, op="sum")[0].tolist() == [0.0] * 5


@pytest.mark.parametrize("dim", [0, 1])
def test_nan_stays_in_its_row(dim):
    clean = _data((5, 9), torch.float32, seed=4)
    clean[2, 4] = 0.0
    x = clean.clone()
    x[2, 4] = float("nan")
    row = 2 if dim == 1 else 4       # the row along dim that holds the NaN, and its position inside it
    pos = 4 if dim == 1 else 2
    others = [i for i in range(x.shape[1 - dim]) if i != row]
    for op in OPS:
        r, rc = ops.reduce(x, op, dim=dim), ops.reduce(clean, op, dim=dim)
        assert torch.isnan(r[row]) and torch.equal(_bits(r[others]), _bits(rc[others]))
        for exclusive in (False, True):
            s = ops.scan(x, exclusive, dim=dim, op=op).movedim(dim, -1)
            sc = ops.scan(clean, exclusive, dim=dim, op=op).movedim(dim, -1)
            first = pos + 1 if exclusive else pos
            assert torch.isnan(s[row, first:]).all() and not torch.isnan(s[row, :first]).any()
            assert torch.equal(_bits(s[row, :first]), _bits(sc[row, :first]))
            assert torch.equal(_bits(s[others]), _bits(sc[others]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_empty_extents(dtype):
    x = torch.zeros((3, 0, 4), dtype=dtype)
    assert torch.equal(ops.reduce(x, "sum", dim=1), torch.zeros((3, 4), dtype=dtype))
    assert ops.reduce(x, "sum", dim=1, keepdim=True).shape == (3, 1, 4)
    for op in ("min", "max"):
        with pytest.raises(ValueError):
            ops.reduce(x, op, dim=1)
        assert ops.scan(x, dim=1, op=op).shape == x.shape
    assert ops.scan(x, True, dim=1).shape == x.shape
    for dim in (0, 2):  # outer == 0 or inner == 0 along the other dims of the same tensor
        for op in OPS:
            got = ops.reduce(x, op, dim=dim)
            assert got.numel() == 0 and got.shape == tuple(s for i, s in enumerate(x.shape) if i != dim)
            assert ops.scan(x, dim=dim, op=op).shape == x.shape
    assert ops.reduce(torch.zeros((0, 5), dtype=dtype), "max", dim=1).shape == (0,)
    assert ops.reduce(torch.zeros((5, 0), dtype=dtype), "max", dim=0).shape == (0,)


def test_refusals():
    x = _data((3, 6), torch.float32)
    for dim in (2, -3):
        with pytest.raises(IndexError):
            ops.reduce(x, "sum", dim=dim)
        with pytest.raises(IndexError):
            ops.scan(x, dim=dim)
    for call in (lambda: ops.reduce(torch.tensor(1.0), "sum", dim=0), lambda: ops.scan(torch.tensor(1.0), dim=0)):
        with pytest.raises(IndexError):
            call()
    for dim in (1.0, True):
        with pytest.raises(TypeError):
            ops.reduce(x, "sum", dim=dim)
        with pytest.raises(TypeError):
            ops.scan(x, dim=dim)
    with pytest.raises(TypeError):
        ops.reduce(x.double(), "sum", dim=1)
    with pytest.raises(TypeError):
        ops.scan(x.double(), dim=1)
    with pytest.raises(ValueError):
        ops.reduce(x, "prod", dim=1)
    with pytest.raises(ValueError):
        ops.scan(x, dim=1, op="prod")
    with pytest.raises(ValueError):
        ops.scan(x, False, torch.zeros(1), dim=1)      # init is the flat multi-GPU scan's offset
    # without dim the new arguments are refused, and the message points at dim=
    for call in (lambda: ops.reduce(x, "sum", keepdim=True), lambda: ops.reduce(x, "sum", route="group"),
                 lambda: ops.reduce(x, "sum", chunk=1024), lambda: ops.scan(x, op="max"),
                 lambda: ops.scan(x, out=torch.empty_like(x)), lambda: ops.scan(x, route="group"),
                 lambda: ops.scan(x, chunk=1024)):
        with pytest.raises(ValueError, match="dim="):
            call()
    # out follows _check_scan_out
    with pytest.raises(TypeError):
        ops.scan(x, dim=1, out=torch.empty(3, 6, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.scan(x, dim=1, out=torch.empty(3, 5))
    with pytest.raises(ValueError):
        ops.scan(x, dim=1, out=torch.empty(6, 3).t())
    # routes
    for call in (lambda r: ops.reduce(x, "sum", dim=1, route=r), lambda r: ops.scan(x, dim=1, route=r)):
        with pytest.raises(ValueError):
            call("fast")
        with pytest.raises(ValueError):
            call("column")                               # inner == 1
        with pytest.raises(ValueError):
            call("column_split")
    for route in ("group", "block", "split"):
        with pytest.raises(ValueError):
            ops.reduce(x, "sum", dim=0, route=route)     # inner > 1
        with pytest.raises(ValueError):
            ops.scan(x, dim=0, route=route)
    with pytest.raises(ValueError):
        ops.reduce(torch.zeros(2, V.AXIS_GROUP_MAX_N + 1), "sum", dim=1, route="group")
    with pytest.raises(ValueError):
        ops.scan(torch.zeros(V.AXIS_BLOCK_MAX_N + 1), dim=0, route="block")
    # chunks
    long_row = torch.zeros(2, 5000)
    for chunk in (0, 1000, -1024):
        with pytest.raises(ValueError):
            ops.reduce(long_row, "sum", dim=1, route="split", chunk=chunk)
    with pytest.raises(ValueError):
        ops.scan(long_row, dim=0, route="column_split", chunk=V.AXIS_COLUMN_MIN_CHUNK - 1)
    with pytest.raises(ValueError):
        ops.reduce(long_row, "sum", dim=1, route="block", chunk=1024)   # chunk is for the split routes
    with pytest.raises(TypeError):
        ops.reduce(long_row, "sum", dim=1, route="split", chunk=1024.0)
    # routes that can take the shape are accepted (and ignored) on the host
    want = long_row.sum(1)
    assert torch.equal(ops.reduce(torch.zeros(2, V.AXIS_GROUP_MAX_N), "sum", dim=1, route="group"), torch.zeros(2))
    for route, chunk in (("block", None), ("split", None), ("split", 2048)):
        assert torch.equal(ops.reduce(long_row, "sum", dim=1, route=route, chunk=chunk), want)
        assert torch.equal(ops.scan(long_row, dim=1, route=route, chunk=chunk), long_row)
    for route, chunk in (("column", None), ("column_split", None), ("column_split", 16)):
        assert ops.reduce(long_row, "max", dim=0, route=route, chunk=chunk).shape == (5000,)
        assert ops.scan(long_row, dim=0, op="max", route=route, chunk=chunk).shape == long_row.shape


def test_dim_none_is_unchanged():
    m = _data((4, 9), torch.float32, seed=2)
    assert ops.reduce(m).dim() == 0 and ops.reduce(m, "max").item() == m.max().item()
    assert ops.reduce(m, "sum", None).item() == pytest.approx(m.sum().item())
    flat = ops.scan(m.reshape(-1))
    assert torch.equal(ops.scan(m), flat.view(4, 9)) and torch.equal(ops.scan(m, dim=None), flat.view(4, 9))
    assert torch.allclose(flat, torch.cumsum(m.reshape(-1).double(), 0).float())
    ex = ops.scan(m, True)                                  # exclusive is still the second positional argument
    assert ex.view(-1)[0].item() == 0.0 and torch.equal(ex.view(-1)[1:], flat[:-1])
    init = torch.tensor([2.0])
    assert torch.equal(ops.scan(m, False, init), ops.scan(m, init=init))
    assert torch.equal(ops.scan(m, False, init, False), (torch.cumsum(m.reshape(-1).double(), 0) + 2.0).float().view(4, 9))
    with pytest.raises(TypeError):
        ops.scan(m.int())                                   # the flat scan still takes float32 only


@pytest.mark.parametrize("kind", ["reduce", "scan"])
def test_default_route_rule(kind):
    r = lambda outer, n, inner: V._axis_route(kind, outer, n, inner)  # noqa: E731
    assert V.AXIS_GROUP_N <= V.AXIS_GROUP_MAX_N < V.AXIS_BLOCK_MAX_N and V.AXIS_SPLIT_MIN_N <= V.AXIS_BLOCK_MAX_N
    g = V.AXIS_GROUP_SCAN_N if kind == "scan" else V.AXIS_GROUP_N
    assert V.AXIS_GROUP_SCAN_N <= V.AXIS_GROUP_MAX_N
    assert r(10, 1, 1) == "group" and r(10, g, 1) == "group" and r(10, g + 1, 1) == "block"
    big = V.AXIS_SPLIT_ROWS
    assert r(big, V.AXIS_BLOCK_MAX_N, 1) == "block" and r(big, V.AXIS_BLOCK_MAX_N + 1, 1) == "split"
    assert r(big - 1, V.AXIS_SPLIT_MIN_N, 1) == "split" and r(big - 1, V.AXIS_SPLIT_MIN_N - 1, 1) == "block"
    assert r(big, V.AXIS_SPLIT_MIN_N, 1) == "block" and r(1, V.AXIS_SPLIT_MIN_N, 1) == "split"
    n = V.AXIS_COLUMN_SPLIT_MIN_N
    if kind == "scan":  # a thread per 4 columns: outer * ceil(inner / 4) threads
        units = V.AXIS_COLUMN_MIN_UNITS
        assert r(1, n, 4 * units) == "column" and r(1, n, 4 * units - 4) == "column_split"
        assert r(units, n, 2) == "column" and r(units - 1, n, 3) == "column_split"
    else:               # a block per 64 column quads (fewer when inner is smaller): outer * tiles blocks
        blocks = V.AXIS_COLUMN_MIN_BLOCKS
        assert r(1, n, 256 * blocks) == "column" and r(1, n, 256 * blocks - 256) == "column_split"
        assert r(1, n, 256 * (blocks - 1) + 1) == "column"      # a ragged last tile counts
        assert r(blocks, n, 2) == "column" and r(blocks - 1, n, 5) == "column_split"
    assert r(1, n - 1, 8) == "column" and r(1, n, 8) == "column_split"
    with pytest.raises(ValueError):
        V._axis_route("sort", 1, 1, 1)
    codes = [V.AXIS_GROUP, V.AXIS_BLOCK, V.AXIS_SPLIT, V.AXIS_COLUMN, V.AXIS_COLUMN_SPLIT]
    assert codes == [1, 2, 3, 4, 5] and V.AXIS_SPLIT_CHUNK % 1024 == 0


@pytest.mark.parametrize("mode,op,dtype", list(itertools.product(["reduce", "scan"], OPS, ["f32", "i32"])))
def test_workload_on_cpu(mode, op, dtype):
    assert "axis" in WORKLOADS
    cpu = Context(device=torch.device("cpu"))
    for inner, exclusive in ((1, False), (5, True)):
        w = build_workload("axis", cpu, outer=5, n=70, inner=inner, mode=mode, op=op, dtype=dtype, exclusive=exclusive)
        w.step()
        r = w.check()
        assert r["check_passed"] and r["elements_checked"] == 5 * inner * (70 if mode == "scan" else 1)
        w.torch_step()
        assert w.work_per_step() > 0
        # the check has power: one changed output element fails it (the last one: never an exclusive scan's identity)
        w.out.view(-1)[-1] += 1
        assert not w.check()["check_passed"]
    with pytest.raises(ValueError):
        build_workload("axis", cpu, mode="sideways")
    with pytest.raises(ValueError):
        build_workload("axis", cpu, op="prod")
    with pytest.raises(ValueError):
        build_workload("axis", cpu, dtype="f64")
    with pytest.raises(ValueError):
        build_workload("axis", cpu, outer=2, n=8, inner=1, route="column")
    with pytest.raises(ValueError):
        build_workload("axis", cpu, outer=2, n=0, inner=1)
