"""Stream compaction on CPU tensors (no GPU): ops.compact / select / compact_indices / select_indices / compact_where
take an exact torch path with the same return shapes as the GPU kernel: (out, count) with out of capacity n and count
a 0-d int64 tensor. Values and counts against plain torch indexing; dtype and size errors raise."""
import pytest
import torch

from parallel_c_programs_amd import ops

SIZES = [0, 1, 5, 1000]
OPS = {"gt": torch.gt, "ge": torch.ge, "lt": torch.lt, "le": torch.le, "eq": torch.eq, "ne": torch.ne}


def _payload(n, dtype, seed=0):
    g = torch.Generator().manual_seed(100 + seed + n)
    if dtype == torch.float32:
        return torch.randn(n, generator=g)
    return torch.randint(-2**31, 2**31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)


def _mask(n, dtype, seed=0):
    g = torch.Generator().manual_seed(200 + seed + n)
    m = torch.rand(n, generator=g) < 0.5
    return m if dtype == torch.bool else m.to(torch.uint8)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
@pytest.mark.parametrize("mdtype", [torch.bool, torch.uint8])
def test_compact_and_select(n, dtype, mdtype):
    x, m = _payload(n, dtype), _mask(n, mdtype)
    ref = x[m.bool()]
    out, count = ops.compact(x, m)
    assert out.shape == (n,) and out.dtype == dtype
    assert count.dtype == torch.int64 and count.dim() == 0 and count.item() == ref.numel()
    assert torch.equal(_bits(out[:ref.numel()]), _bits(ref))
    sel = ops.select(x, m)
    assert sel.shape == ref.shape and torch.equal(_bits(sel), _bits(ref))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mdtype", [torch.bool, torch.uint8])
def test_compact_indices_and_select_indices(n, mdtype):
    m = _mask(n, mdtype)
    ref = torch.nonzero(m.flatten()).flatten().int()
    idx, count = ops.compact_indices(m)
    assert idx.shape == (n,) and idx.dtype == torch.int32
    assert count.dtype == torch.int64 and count.dim() == 0 and count.item() == ref.numel()
    assert torch.equal(idx[:ref.numel()], ref)
    got = ops.select_indices(m)
    assert got.dtype == torch.int32 and torch.equal(got, ref)


def test_uint8_mask_any_nonzero_byte_keeps():
    x = torch.arange(8, dtype=torch.int32)
    m = torch.tensor([0, 1, 2, 0, 255, 128, 0, 7], dtype=torch.uint8)
    assert ops.select(x, m).tolist() == [1, 2, 4, 5, 7]
    assert ops.select_indices(m).tolist() == [1, 2, 4, 5, 7]


def test_multi_dimensional_inputs_are_flattened():
    x = _payload(24, torch.float32).reshape(2, 3, 4)
    m = _mask(24, torch.bool).reshape(2, 3, 4)
    assert torch.equal(ops.select(x, m), x.flatten()[m.flatten()])
    assert torch.equal(ops.select(x.transpose(0, 2), m.transpose(0, 2)), x.transpose(0, 2).flatten()[m.transpose(0, 2).flatten()])
    assert torch.equal(ops.select_indices(m), torch.nonzero(m.flatten()).flatten().int())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("indices", [False, True])
def test_compact_where_with_nan(n, op, indices):
    x = _payload(n, torch.float32)
    if n >= 5:
        x[1], x[n - 1] = float("nan"), float("nan")
        x[3] = x[0]  # the threshold occurs more than once
    t = x[0].item() if n else 0.25
    keep = OPS[op](x, t)
    ref = torch.nonzero(keep).flatten().int() if indices else x[keep]
    out, count = ops.compact_where(x, op, t, indices=indices)
    assert out.shape == (n,) and out.dtype == (torch.int32 if indices else torch.float32)
    assert count.dtype == torch.int64 and count.dim() == 0 and count.item() == ref.numel()
    assert torch.equal(_bits(out[:ref.numel()]), _bits(ref))


def test_nan_is_kept_only_by_ne():
    x = torch.tensor([float("nan"), 1.0, float("nan")])
    for op in OPS:
        _, count = ops.compact_where(x, op, float("nan"))
        assert count.item() == (3 if op == "ne" else 0), op
    _, count = ops.compact_where(x, "ne", 1.0)
    assert count.item() == 2


def test_out_is_used_and_left_untouched_past_count():
    x = torch.arange(10, dtype=torch.float32)
    m = x < 4
    out = torch.full((16,), -7.0)
    got, count = ops.compact(x, m, out=out)
    assert got is out and count.item() == 4
    assert out[:4].tolist() == [0, 1, 2, 3] and bool((out[4:] == -7.0).all())
    idx = torch.full((10,), -7, dtype=torch.int32)
    got, count = ops.compact_indices(m, out=idx)
    assert got is idx and idx[:4].tolist() == [0, 1, 2, 3] and bool((idx[4:] == -7).all())


def test_dtype_and_size_errors():
    x, m = torch.zeros(8), torch.ones(8, dtype=torch.bool)
    with pytest.raises(TypeError):
        ops.compact(x.double(), m)
    with pytest.raises(TypeError):
        ops.compact(x, m.int())
    with pytest.raises(ValueError):
        ops.compact(x, m[:7])
    with pytest.raises(TypeError):
        ops.compact_indices(m.float())
    with pytest.raises(TypeError):
        ops.compact_where(x.int(), "gt", 0.0)
    with pytest.raises(ValueError):
        ops.compact_where(x, "between", 0.0)
    with pytest.raises(TypeError):
        ops.compact(x, m, out=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.compact(x, m, out=torch.zeros(7))
    with pytest.raises(TypeError):
        ops.compact_where(x, "gt", 0.0, indices=True, out=torch.zeros(8))


def test_select_workload_on_cpu():
    from parallel_c_programs_amd.models import build_workload
    from parallel_c_programs_amd.parallel.dist import Context

    for mode in ("mask", "index", "where"):
        w = build_workload("select", Context(), n=5000, keep=0.3, mode=mode)
        w.step()
        r = w.check()
        assert r["check_passed"] and r["kept"] == r["kept_torch"], (mode, r)
        n, k = 5000, r["kept"]
        assert 0 < k < n and w.work_per_step() == {"mask": 5 * n, "index": n, "where": 4 * n}[mode] + 4 * k
