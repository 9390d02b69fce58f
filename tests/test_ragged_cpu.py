"""ops.segment_reduce / ops.segment_scan on CPU tensors (the host path of parallel_c_programs_amd/ops/vector.py), their
argument checks, and the "ragged" workload. No GPU. The oracles are torch.segment_reduce (floating types only: int32
data goes through a float64 copy, which holds every int32 exactly) and int64 prefix differences wrapped mod 2^32."""
import pytest
import torch

from parallel_c_programs_amd import ops
from parallel_c_programs_amd.models.workloads import WORKLOADS, build_workload
from parallel_c_programs_amd.parallel.dist import Context

OPS = ("sum", "min", "max")
INT_IDENT = {"sum": 0, "min": 2**31 - 1, "max": -2**31}
F32_IDENT = {"sum": 0.0, "min": float("inf"), "max": float("-inf")}


def _offsets(n, s, seed, lo=0, hi=None):
    hi = n if hi is None else hi
    g = torch.Generator().manual_seed(seed)
    cuts = torch.sort(torch.randint(lo, hi + 1, (s - 1,), generator=g)).values
    return torch.cat([torch.tensor([lo]), cuts, torch.tensor([hi])]).int()


CASES = [(1000, 50, 0, None), (1000, 700, 0, None), (1000, 50, 9, 990), (37, 1, 5, 30), (64, 300, 0, None)]


@pytest.mark.parametrize("n,s,lo,hi", CASES)
def test_float32_against_torch_segment_reduce(n, s, lo, hi):
    g = torch.Generator().manual_seed(n + s)
    off = _offsets(n, s, s, lo, hi)
    ties = torch.round(torch.randn(n, generator=g) * 64) / 64
    whole = torch.randint(-8, 9, (n,), generator=g).float()
    for op in ("min", "max"):
        assert torch.equal(ops.segment_reduce(ties, off, op), torch.segment_reduce(ties, op, offsets=off.long()))
    got = ops.segment_reduce(whole, off)
    assert got.dtype == torch.float32 and got.shape == (s,)
    assert torch.equal(got, torch.segment_reduce(whole, "sum", offsets=off.long()))
    assert (off[1:] == off[:-1]).any() or s == 1  # the cases hold empty segments


@pytest.mark.parametrize("n,s,lo,hi", CASES)
def test_int32_against_float64_copy_and_prefix_differences(n, s, lo, hi):
    g = torch.Generator().manual_seed(n * s)
    off = _offsets(n, s, s + 1, lo, hi)
    x = torch.randint(-(1 << 31), 1 << 31, (n,), generator=g, dtype=torch.int64).int()
    empty = off[1:] == off[:-1]
    for op in ("min", "max"):
        ref = torch.segment_reduce(x.double(), op, offsets=off.long())
        ref = torch.where(empty, torch.full_like(ref, float(INT_IDENT[op])), ref).int()
        got = ops.segment_reduce(x, off, op)
        assert got.dtype == torch.int32 and torch.equal(got, ref), op
    c = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(x.long(), 0)])
    d = c[off.long()[1:]] - c[off.long()[:-1]]
    assert torch.equal(ops.segment_reduce(x, off), (((d + 2**31) % 2**32) - 2**31).int())
    assert bool((d.abs() >= 2**31).any()) or n < 100  # the sums do wrap


def test_empty_segments_give_the_identity():
    off = torch.tensor([2, 2, 2, 5, 5], dtype=torch.int32)
    for op in OPS:
        r = ops.segment_reduce(torch.arange(8, dtype=torch.int32), off, op)
        assert r.tolist() == [INT_IDENT[op], INT_IDENT[op], {"sum": 9, "min": 2, "max": 4}[op], INT_IDENT[op]]
        f = ops.segment_reduce(torch.arange(8.0), off, op)
        assert f.tolist() == [F32_IDENT[op], F32_IDENT[op], {"sum": 9.0, "min": 2.0, "max": 4.0}[op], F32_IDENT[op]]
        assert not bool(torch.signbit(f[0])) or op == "max"


def test_no_segments_no_elements_and_out():
    x = torch.arange(10.0)
    one = torch.tensor([4], dtype=torch.int32)
    for t in (x, x.int()):
        r = ops.segment_reduce(t, one)
        assert r.shape == (0,) and r.dtype == t.dtype
        for op in OPS:
            z = ops.segment_reduce(t[:0], torch.zeros(4, dtype=torch.int32), op)
            ident = (F32_IDENT if t.dtype == torch.float32 else INT_IDENT)[op]
            assert z.dtype == t.dtype and z.tolist() == [ident] * 3
    off = torch.tensor([1, 3, 3, 10], dtype=torch.int32)
    out = torch.full((6,), -7.0)
    r = ops.segment_reduce(x.view(2, 5), off, out=out)  # flattened
    assert r.data_ptr() == out.data_ptr() and r.tolist() == [3.0, 0.0, 42.0] and out[3:].tolist() == [-7.0] * 3
    # elements outside [offsets[0], offsets[S]) are not read
    y = x.clone()
    y[0] = float("nan")
    assert ops.segment_reduce(y, off).tolist() == [3.0, 0.0, 42.0]
    # a NaN stays in its segment
    y[4] = float("nan")
    for op in OPS:
        r = ops.segment_reduce(y, off, op)
        assert bool(torch.isnan(r[2])) and not bool(torch.isnan(r[:2]).any())


def test_validate():
    x = torch.ones(100)
    for bad, index in (([0, 50, 40, 100], 2), ([-1, 50, 60, 100], 0), ([0, 50, 60, 101], 3), ([0, -3, 60, 100], 1),
                       ([101, 101], 0)):
        with pytest.raises(ValueError, match=rf"offsets\[{index}\]"):
            ops.segment_reduce(x, torch.tensor(bad, dtype=torch.int32), validate=True)
    good = torch.tensor([0, 50, 50, 100], dtype=torch.int32)
    assert ops.segment_reduce(x, good, validate=True).tolist() == [50.0, 0.0, 50.0]


def test_wrong_arguments():
    x = torch.ones(10)
    o = torch.tensor([0, 4, 10], dtype=torch.int32)
    for fn in (ops.segment_reduce, ops.segment_scan):
        with pytest.raises(TypeError):
            fn(x.double(), o)
        with pytest.raises(TypeError):
            fn(x.long(), o)
        with pytest.raises(TypeError):
            fn(x, o.long())
        with pytest.raises(TypeError):
            fn(x, o, out=torch.empty(10, dtype=torch.int32))
        with pytest.raises(ValueError):
            fn(x, o, "prod")
        for xx, oo in ((x, o.view(3, 1)), (x, o[::2]), (x, o[:0]), (torch.ones(4, 10)[:, ::2], o),
                       (x, o.to("meta"))):
            with pytest.raises(ValueError):
                fn(xx, oo)
    for out in (torch.empty(1), torch.empty(4)[::2], torch.empty(2, 2), x[2:6], torch.empty(4, device="meta")):
        with pytest.raises(ValueError):
            ops.segment_reduce(x, o, out=out)
    with pytest.raises(ValueError):
        ops.segment_scan(x, o, out=torch.empty(9))
    big = torch.empty((1 << 31) - 2, device="meta")  # no memory behind it: n + S = 2^31 breaks the size limit
    with pytest.raises(ValueError, match="2\\^31"):
        ops.segment_reduce(big, o.to("meta"))


@pytest.mark.parametrize("exclusive", [False, True])
def test_segment_scan_equals_segmented_scan_with_hand_built_heads(exclusive):
    n = 500
    off = _offsets(n, 60, 3, 6, 480)
    heads = torch.zeros(n, dtype=torch.bool)
    for o in off.tolist():
        heads[o] = True
    g = torch.Generator().manual_seed(4)
    for x in (torch.randint(-(1 << 31), 1 << 31, (n,), generator=g, dtype=torch.int64).int(),
              torch.randint(-8, 9, (n,), generator=g).float()):
        for op in OPS:
            got = ops.segment_scan(x.view(50, 10), off, op, exclusive)
            assert got.shape == (50, 10)
            assert torch.equal(got, ops.segmented_scan(x.view(50, 10), heads, op, exclusive)), (x.dtype, op)
    out = torch.empty(n)
    assert ops.segment_scan(x, off, out=out).data_ptr() == out.data_ptr()
    # offsets[S] == n stores no head; the positions before offsets[0] are one run
    r = ops.segment_scan(torch.ones(6), torch.tensor([2, 4, 6], dtype=torch.int32))
    assert r.tolist() == [1.0, 2.0, 1.0, 2.0, 1.0, 2.0]


@pytest.mark.parametrize("dist", ["uniform", "equal", "powerlaw", "empty"])
def test_ragged_workload_on_the_cpu(dist):
    assert "ragged" in WORKLOADS
    for dtype, op in (("f32", "sum"), ("i32", "sum"), ("f32", "min"), ("i32", "max")):
        w = build_workload("ragged", Context(device=torch.device("cpu")), n=3000, mean_len=7, dist=dist, op=op, dtype=dtype)
        w.step()
        c = w.check(reduce=False)
        assert c["check_passed"] and c["elements_checked"] == w.segments() == (12000 if dist == "empty" else 428)
        assert w.work_per_step() == 4.0 * (3000 + 2 * w.segments() + 1)
        off = w.offsets.long()
        assert int(off[0]) == 0 and int(off[-1]) <= 3000 and bool((off[1:] >= off[:-1]).all())
    w.out = w.out + 1
    assert not w.check(reduce=False)["check_passed"]
    with pytest.raises(ValueError):
        build_workload("ragged", Context(device=torch.device("cpu")), n=10, dist="sideways")


def test_exports():
    assert "segment_reduce" in ops.__all__ and "segment_scan" in ops.__all__
    from parallel_c_programs_amd.ops import vector as V

    assert V.RAGGED_TILE == 256 * V.RAGGED_LANE_ITEMS and V.RAGGED_LANE_ITEMS % 2 == 1
