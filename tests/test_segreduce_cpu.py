"""Run-length encode, reduce-by-key, unique and sum_by_key on CPU tensors (the exact torch path of ops/vector.py)
against plain torch: return shapes, dtypes, the 0-d int64 count, caller outputs untouched past the count, the
bit-pattern key rule, the error cases, and the SegReduce workload in its three modes. No GPU needed."""
import pytest
import torch

from parallel_c_programs_amd import ops

SIZES = [0, 1, 5, 1000]
KEY_DTYPES = [torch.float32, torch.int32]
VAL_DTYPES = [torch.float32, torch.int32]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _keys(n, dtype, seed=0, mean_run=3.0):
    g = torch.Generator().manual_seed(100 + seed)
    ids = torch.cumsum(torch.rand(n, generator=g) < 1.0 / mean_run, 0)
    return (ids * 7 - 11).to(dtype)  # distinct neighbouring runs, exact in float32


def _ref_runs(keys):
    """(run key bits, int64 run index per element, int64 counts) by a plain loop-free torch formulation."""
    kb = _bits(keys.reshape(-1))
    n = kb.numel()
    if n == 0:
        return kb, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    head = torch.ones(n, dtype=torch.bool)
    head[1:] = kb[1:] != kb[:-1]
    inv = torch.cumsum(head, 0) - 1
    return kb[head], inv, torch.bincount(inv, minlength=int(inv[-1]) + 1)


def _ref_reduce(inv, k, values, op):
    v = values.reshape(-1)
    if op == "sum":
        if v.dtype == torch.int32:
            s = torch.zeros(k, dtype=torch.int64).index_add_(0, inv, v.long())
            return (((s + 2**31) % 2**32) - 2**31).int()
        return torch.zeros(k, dtype=torch.float32).index_add_(0, inv, v)
    return torch.zeros(k, dtype=v.dtype).scatter_reduce_(0, inv, v, "amin" if op == "min" else "amax", include_self=False)


def _check_count(num, k):
    assert num.dtype == torch.int64 and num.dim() == 0 and num.item() == k


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kdt", KEY_DTYPES)
def test_run_length_encode(n, kdt):
    keys = _keys(n, kdt, seed=n)
    rk_ref, _, cnt_ref = _ref_runs(keys)
    k = rk_ref.numel()
    assert k == (0 if n == 0 else k) and (n == 0) == (k == 0)
    rk, rc, num = ops.run_length_encode(keys)
    _check_count(num, k)
    assert rk.dtype == kdt and rc.dtype == torch.int32 and rk.shape == (n,) and rc.shape == (n,)
    assert torch.equal(_bits(rk[:k]), rk_ref) and torch.equal(rc[:k].long(), cnt_ref)
    rk, rc, rs, num = ops.run_length_encode(keys, starts=True)
    _check_count(num, k)
    assert rs.dtype == torch.int32 and rs.shape == (n,)
    assert torch.equal(rs[:k].long(), torch.cumsum(cnt_ref, 0) - cnt_ref)
    # caller outputs larger than needed stay untouched past the count
    ok, oc, os_ = (torch.full((n + 3,), -7, dtype=d) for d in (kdt, torch.int32, torch.int32))
    rk, rc, rs, num = ops.run_length_encode(keys, starts=True, out_keys=ok, out_counts=oc, out_starts=os_)
    assert rk.data_ptr() == ok.data_ptr() and rc.data_ptr() == oc.data_ptr() and rs.data_ptr() == os_.data_ptr()
    assert torch.equal(_bits(ok[:k]), rk_ref) and torch.equal(oc[:k].long(), cnt_ref)
    assert bool((ok[k:] == -7).all()) and bool((oc[k:] == -7).all()) and bool((os_[k:] == -7).all())
    # the exact-size form
    uk, uc = ops.unique_consecutive(keys, return_counts=True)
    assert uk.shape == (k,) and uc.shape == (k,) and uc.dtype == torch.int32
    assert torch.equal(_bits(uk), rk_ref) and torch.equal(uc.long(), cnt_ref)
    assert torch.equal(_bits(ops.unique_consecutive(keys)), rk_ref)
    tk, tcnt = torch.unique_consecutive(_bits(keys), return_counts=True)
    assert torch.equal(_bits(uk), tk) and torch.equal(uc.long(), tcnt)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kdt", KEY_DTYPES)
@pytest.mark.parametrize("vdt", VAL_DTYPES)
@pytest.mark.parametrize("op", ["sum", "min", "max"])
def test_reduce_by_key(n, kdt, vdt, op):
    keys = _keys(n, kdt, seed=n + 1)
    g = torch.Generator().manual_seed(n)
    values = torch.randint(-50, 50, (n,), generator=g).to(vdt)  # integer-valued: float sums are exact in any order
    rk_ref, inv, _ = _ref_runs(keys)
    k = rk_ref.numel()
    ref = _ref_reduce(inv, k, values, op)
    rk, ra, num = ops.reduce_by_key(keys, values, op)
    _check_count(num, k)
    assert rk.dtype == kdt and ra.dtype == vdt and rk.shape == (n,) and ra.shape == (n,)
    assert torch.equal(_bits(rk[:k]), rk_ref) and torch.equal(ra[:k], ref)
    ok, oa = torch.full((n + 2,), -7, dtype=kdt), torch.full((n + 2,), -7, dtype=vdt)
    rk, ra, num = ops.reduce_by_key(keys, values, op, out_keys=ok, out=oa)
    assert rk.data_ptr() == ok.data_ptr() and ra.data_ptr() == oa.data_ptr()
    assert torch.equal(oa[:k], ref) and bool((oa[k:] == -7).all()) and bool((ok[k:] == -7).all())


def test_int32_sum_wraps():
    keys = torch.tensor([1, 1, 1, 2], dtype=torch.int32)
    values = torch.tensor([2**31 - 1, 2**31 - 1, 5, -3], dtype=torch.int32)
    _, ra, num = ops.reduce_by_key(keys, values, "sum")
    assert num.item() == 2 and ra[:2].tolist() == [3, -3]  # 2 * (2^31 - 1) + 5 = 2^32 + 3


def test_keys_are_compared_as_bit_patterns():
    bits = torch.tensor([0, -2**31, 0x7fc00000, 0x7fc00000, 0x7fc00001], dtype=torch.int32)  # 0.0 -0.0 nan nan nan'
    keys = bits.view(torch.float32)
    rk, rc, num = ops.run_length_encode(keys)
    assert num.item() == 4 and rc[:4].tolist() == [1, 1, 2, 1]
    assert torch.equal(_bits(rk[:4]), torch.tensor([0, -2**31, 0x7fc00000, 0x7fc00001], dtype=torch.int32))
    _, ra, num = ops.reduce_by_key(keys, torch.arange(5, dtype=torch.int32), "max")
    assert num.item() == 4 and ra[:4].tolist() == [0, 1, 3, 4]


def test_2d_and_noncontiguous_inputs_are_flattened():
    keys = torch.tensor([[1, 1, 2], [2, 2, 3]], dtype=torch.int32)
    assert ops.unique_consecutive(keys).tolist() == [1, 2, 3]
    assert ops.unique_consecutive(keys.t()).tolist() == [1, 2, 1, 2, 3]  # 1 2 1 2 2 3
    vals = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    _, ra, num = ops.reduce_by_key(keys, vals, "sum")
    assert num.item() == 3 and ra[:3].tolist() == [1.0, 9.0, 5.0]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", KEY_DTYPES)
def test_unique_against_torch(n, dtype):
    g = torch.Generator().manual_seed(7 + n)
    x = torch.randint(-9, 9, (n,), generator=g).to(dtype)
    if dtype == torch.float32 and n >= 5:
        x[1], x[3] = -0.0, 0.0  # both zeros: one value, as in torch.unique
    ref_v, ref_c = torch.unique(x, return_counts=True)
    v, c = ops.unique(x, return_counts=True)
    assert v.dtype == dtype and c.dtype == torch.int32 and v.shape == ref_v.shape
    assert torch.equal(v, ref_v) and torch.equal(c.long(), ref_c)
    assert torch.equal(ops.unique(x), ref_v)
    if dtype == torch.float32 and n >= 5:
        assert (_bits(v) == -2**31).sum().item() == 0  # the zero comes out as +0.0


def test_unique_float_nans_are_one_value():
    x = torch.tensor([2.0, float("nan"), 1.0, -float("nan"), 2.0])
    v, c = ops.unique(x, return_counts=True)
    assert v[:2].tolist() == [1.0, 2.0] and torch.isnan(v[2]) and c.tolist() == [1, 2, 2]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kdt", KEY_DTYPES)
@pytest.mark.parametrize("vdt", VAL_DTYPES)
def test_sum_by_key_against_index_add(n, kdt, vdt):
    g = torch.Generator().manual_seed(11 + n)
    keys = torch.randint(-6, 6, (n,), generator=g).to(kdt)
    values = torch.randint(-50, 50, (n,), generator=g).to(vdt)  # integer-valued floats: exact
    ref_k, inv = torch.unique(keys, return_inverse=True)
    ref = torch.zeros(ref_k.numel(), dtype=torch.float64).index_add_(0, inv, values.double())
    uk, s = ops.sum_by_key(keys, values)
    assert uk.dtype == kdt and s.dtype == vdt and uk.shape == ref_k.shape and s.shape == ref_k.shape
    assert torch.equal(uk, ref_k) and torch.equal(s.double(), ref)


def test_errors():
    k = torch.zeros(4, dtype=torch.int32)
    v = torch.zeros(4)
    with pytest.raises(TypeError):
        ops.run_length_encode(k.long())
    with pytest.raises(TypeError):
        ops.run_length_encode(k.double())
    with pytest.raises(TypeError):
        ops.reduce_by_key(k, v.double())
    with pytest.raises(TypeError):
        ops.reduce_by_key(k.long(), v)
    with pytest.raises(ValueError):
        ops.reduce_by_key(k, v[:3])
    with pytest.raises(ValueError):
        ops.reduce_by_key(k, v, "prod")
    with pytest.raises(TypeError):
        ops.run_length_encode(k, out_keys=torch.zeros(4))  # wrong dtype
    with pytest.raises(TypeError):
        ops.run_length_encode(k, out_counts=torch.zeros(4))
    with pytest.raises(ValueError):
        ops.run_length_encode(k, out_keys=torch.zeros(3, dtype=torch.int32))  # too small
    with pytest.raises(ValueError):
        ops.reduce_by_key(k, v, out=torch.zeros(2, 4))  # not 1-D
    with pytest.raises(TypeError):
        ops.reduce_by_key(k, v, out=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.unique(k.long())
    with pytest.raises(TypeError):
        ops.sum_by_key(k, v.double())
    with pytest.raises(ValueError):
        ops.sum_by_key(k, v[:2])
    assert set(ops.OP_CODES) == {"sum", "min", "max"}


@pytest.mark.parametrize("mode", ["rle", "sum", "unique"])
@pytest.mark.parametrize("dtype", ["f32", "i32"])
@pytest.mark.parametrize("mean_run", [0, 1, 3.5])
def test_workload_on_cpu(mode, dtype, mean_run):
    from parallel_c_programs_amd.models import WORKLOADS, build_workload
    from parallel_c_programs_amd.parallel.dist import Context

    assert "segreduce" in WORKLOADS
    w = build_workload("segreduce", Context(device=torch.device("cpu")), n=5000, mean_run=mean_run, mode=mode, dtype=dtype)
    w.step()
    r = w.check(chunk=1234)  # several chunks: runs are joined across chunk borders
    assert r["check_passed"] and r["lookback_ok"] and r["runs"] == r["runs_torch"], r
    if mode != "unique":
        assert r["runs"] == (1 if mean_run == 0 else r["runs"])
        if mean_run == 1:
            assert r["runs"] == 5000
    assert w.work_per_step() > 0
    t = w.torch_step()
    assert t[0].numel() == r["runs"]
    with pytest.raises(ValueError):
        build_workload("segreduce", Context(device=torch.device("cpu")), n=8, mode="nope")
