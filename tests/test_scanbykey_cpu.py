"""scan_by_key, segmented_scan and run_positions on CPU tensors (the host path of ops/vector.py) against a plain Python
loop: every op, both value dtypes, inclusive and exclusive, run structures from all distinct to all equal; the
bit-pattern key rule, NaN containment, in-place output, the error cases, and the ScanByKey workload in its three modes.
No GPU needed."""
import math

import pytest
import torch

from parallel_c_programs_amd import ops

SIZES = [0, 1, 2, 5, 257, 5000]
MEAN_RUNS = [1, 1.5, 7, 0]  # 0: all keys equal
IDENT = {("sum", torch.float32): 0.0, ("min", torch.float32): math.inf, ("max", torch.float32): -math.inf,
         ("sum", torch.int32): 0, ("min", torch.int32): 2**31 - 1, ("max", torch.int32): -2**31}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ids(n, mean_run, seed=0):
    g = torch.Generator().manual_seed(300 + seed)
    p = 0.0 if mean_run == 0 else 1.0 / mean_run
    return torch.cumsum(torch.rand(n, generator=g) < p, 0)


def _wrap(x):
    return ((x + 2**31) % 2**32) - 2**31


def _loop(head, values, op, exclusive):
    """The contract, element by element: Python ints for int32 (wrapped), Python floats of integer-valued float32."""
    is_int = values.dtype == torch.int32
    f = {"sum": lambda a, b: a + b, "min": min, "max": max}[op]
    ident = IDENT[(op, values.dtype)]
    out, acc = [], ident
    for h, x in zip(head.tolist(), values.tolist()):
        if h:
            acc = ident
        before = acc
        acc = f(acc, x)
        if is_int:
            acc = _wrap(acc)
        out.append(before if exclusive else acc)
    return torch.tensor(out, dtype=values.dtype).reshape(values.shape)


def _heads_of(keys):
    kb = _bits(keys.reshape(-1))
    head = torch.ones(kb.numel(), dtype=torch.bool)
    head[1:] = kb[1:] != kb[:-1]
    return head


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mean_run", MEAN_RUNS)
@pytest.mark.parametrize("vdt", [torch.float32, torch.int32])
def test_against_loop(n, mean_run, vdt):
    ids = _ids(n, mean_run, seed=n)
    g = torch.Generator().manual_seed(n + 1)
    values = torch.randint(-50, 50, (n,), generator=g).to(vdt)  # integer-valued: float sums are exact in any order
    for keys in ((ids * 7 - 11).int(), (ids * 7 - 11).float()):
        head = _heads_of(keys)
        for op in ("sum", "min", "max"):
            for exclusive in (False, True):
                ref = _loop(head, values, op, exclusive)
                got = ops.scan_by_key(keys, values, op, exclusive)
                assert got.dtype == vdt and got.shape == values.shape
                assert torch.equal(got, ref), (op, exclusive)
                for flags in (head, head.to(torch.uint8) * 3):
                    seg = ops.segmented_scan(values, flags, op, exclusive)
                    assert seg.dtype == vdt and torch.equal(seg, ref), (op, exclusive, flags.dtype)
    pos = ops.run_positions(keys)
    _, inv, cnt = torch.unique_consecutive(_bits(keys), return_inverse=True, return_counts=True)
    starts = torch.cumsum(cnt, 0) - cnt
    assert pos.dtype == torch.int32 and pos.shape == keys.shape
    assert torch.equal(pos.long(), torch.arange(n) - starts[inv])
    assert torch.equal(pos, _loop(_heads_of(keys), torch.ones(n, dtype=torch.int32), "sum", True))


def test_heads_first_flag_is_ignored():
    v = torch.tensor([1, 2, 3, 4], dtype=torch.int32)
    for first in (0, 1):
        h = torch.tensor([first, 0, 1, 0], dtype=torch.uint8)
        assert ops.segmented_scan(v, h).tolist() == [1, 3, 3, 7]
        assert ops.segmented_scan(v, h.bool(), exclusive=True).tolist() == [0, 1, 0, 3]
    assert h.tolist() == [1, 0, 1, 0]  # the caller's flags are not written


def test_int32_sum_wraps():
    keys = torch.tensor([1, 1, 1, 2], dtype=torch.int32)
    values = torch.tensor([2**31 - 1, 2**31 - 1, 5, -3], dtype=torch.int32)
    assert ops.scan_by_key(keys, values).tolist() == [2**31 - 1, -2, 3, -3]
    assert ops.scan_by_key(keys, values, exclusive=True).tolist() == [0, 2**31 - 1, -2, 0]


def test_exclusive_identities():
    keys = torch.tensor([4, 4, 9], dtype=torch.int32)
    vf, vi = torch.tensor([-0.0, 2.0, 3.0]), torch.tensor([5, 6, 7], dtype=torch.int32)
    s = ops.scan_by_key(keys, vf, "sum", True)
    assert _bits(s)[0].item() == 0 and _bits(s)[2].item() == 0  # +0.0 at the heads
    assert ops.scan_by_key(keys, vf, "min", True).tolist() == [math.inf, -0.0, math.inf]
    assert ops.scan_by_key(keys, vf, "max", True).tolist() == [-math.inf, -0.0, -math.inf]
    assert ops.scan_by_key(keys, vi, "min", True).tolist() == [2**31 - 1, 5, 2**31 - 1]
    assert ops.scan_by_key(keys, vi, "max", True).tolist() == [-2**31, 5, -2**31]


def test_keys_are_compared_as_bit_patterns():
    bits = torch.tensor([0, -2**31, 0x7fc00000, 0x7fc00000, 0x7fc00001], dtype=torch.int32)  # 0.0 -0.0 nan nan nan'
    keys = bits.view(torch.float32)
    v = torch.arange(1, 6, dtype=torch.int32)
    assert ops.scan_by_key(keys, v).tolist() == [1, 2, 3, 7, 5]
    assert ops.run_positions(keys).tolist() == [0, 0, 0, 1, 0]


def test_nan_and_inf_stay_inside_their_run():
    keys = torch.tensor([1, 1, 1, 2, 2, 3, 3, 3], dtype=torch.int32)
    v = torch.tensor([1.0, math.nan, 2.0, 3.0, 4.0, math.inf, -math.inf, 5.0])
    for op in ("sum", "min", "max"):
        for exclusive in (False, True):
            got = ops.scan_by_key(keys, v, op, exclusive)
            clean = ops.scan_by_key(keys, torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0), op, exclusive)
            assert torch.equal(_bits(got[3:5]), _bits(clean[3:5])), (op, exclusive)  # the middle run is untouched
            assert not torch.isnan(got[3:5]).any()
    incl = ops.scan_by_key(keys, v, "min")
    assert incl[0].item() == 1.0 and torch.isnan(incl[1:3]).all()  # the NaN goes on to the end of its run
    assert torch.isnan(ops.scan_by_key(keys, v, "sum")[7])  # inf + -inf
    assert ops.scan_by_key(keys, v, "max").tolist()[5:] == [math.inf, math.inf, math.inf]


def test_out_and_in_place():
    n = 1000
    keys = (_ids(n, 4, seed=5)).int()
    for vdt in (torch.float32, torch.int32):
        values = torch.randint(-9, 9, (n,), generator=torch.Generator().manual_seed(8)).to(vdt)
        ref = ops.scan_by_key(keys, values, "sum")
        out = torch.full((n,), -7, dtype=vdt)
        r = ops.scan_by_key(keys, values, "sum", out=out)
        assert r.data_ptr() == out.data_ptr() and torch.equal(out, ref)
        work = values.clone()
        r = ops.scan_by_key(keys, work, "sum", out=work)  # in place
        assert r.data_ptr() == work.data_ptr() and torch.equal(work, ref)
        work = values.clone()
        ops.segmented_scan(work, _heads_of(keys), "sum", out=work)
        assert torch.equal(work, ref)
    v2 = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    k2 = torch.tensor([[1, 1, 2], [2, 2, 3]], dtype=torch.int32)
    got = ops.scan_by_key(k2, v2)
    assert got.shape == (2, 3) and got.flatten().tolist() == [0.0, 1.0, 2.0, 5.0, 9.0, 5.0]
    assert ops.run_positions(k2).tolist() == [[0, 1, 0], [1, 2, 0]]
    assert ops.run_positions(k2.t()).flatten().tolist() == [0, 0, 0, 0, 1, 0]  # 1 2 1 2 2 3


def test_errors():
    k = torch.zeros(4, dtype=torch.int32)
    v = torch.zeros(4)
    h = torch.zeros(4, dtype=torch.bool)
    with pytest.raises(TypeError):
        ops.scan_by_key(k.long(), v)
    with pytest.raises(TypeError):
        ops.scan_by_key(k, v.double())
    with pytest.raises(ValueError):
        ops.scan_by_key(k, v[:3])
    with pytest.raises(ValueError):
        ops.scan_by_key(k, v, "prod")
    with pytest.raises(TypeError):
        ops.scan_by_key(k, v, out=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.scan_by_key(k, v, out=torch.zeros(5))
    with pytest.raises(ValueError):
        ops.scan_by_key(k, v, out=torch.zeros(8)[::2])
    with pytest.raises(ValueError):
        ops.scan_by_key(k, v.to("meta"))
    with pytest.raises(TypeError):
        ops.segmented_scan(v, h.int())
    with pytest.raises(TypeError):
        ops.segmented_scan(v.double(), h)
    with pytest.raises(ValueError):
        ops.segmented_scan(v, h[:3])
    with pytest.raises(ValueError):
        ops.segmented_scan(v, h, "prod")
    with pytest.raises(ValueError):
        ops.segmented_scan(v, h.to("meta"))
    with pytest.raises(ValueError):
        ops.segmented_scan(v, h, out=torch.zeros(4, device="meta"))
    with pytest.raises(TypeError):
        ops.run_positions(k.double())


@pytest.mark.parametrize("mode", ["keys", "heads", "positions"])
@pytest.mark.parametrize("dtype,op,exclusive", [("f32", "sum", False), ("i32", "sum", True), ("f32", "min", True),
                                                ("i32", "max", False)])
@pytest.mark.parametrize("mean_run", [0, 1, 3.5])
def test_workload_on_cpu(mode, dtype, op, exclusive, mean_run):
    from parallel_c_programs_amd.models import WORKLOADS, build_workload
    from parallel_c_programs_amd.parallel.dist import Context

    assert "scanbykey" in WORKLOADS
    w = build_workload("scanbykey", Context(device=torch.device("cpu")), n=5000, mean_run=mean_run, op=op, dtype=dtype,
                       exclusive=exclusive, mode=mode)
    w.step()
    r = w.check(chunk=1234)  # several chunks: the carry crosses chunk borders
    assert r["check_passed"] and r["elements_checked"] == 5000, r
    assert r["runs"] == (1 if mean_run == 0 else 5000 if mean_run == 1 else r["runs"])
    assert w.work_per_step() > 0
    t = w.torch_step()
    assert t.shape == w.out.shape and t.dtype == w.out.dtype
    if dtype == "i32" or op != "sum" or mode == "positions":
        assert torch.equal(t, w.out)
    w.out = w.out.clone()
    w.out[4321] = -12345  # the check sees one wrong element (no output here is negative)
    assert not w.check(chunk=1234)["check_passed"]
    with pytest.raises(ValueError):
        build_workload("scanbykey", Context(device=torch.device("cpu")), n=8, mode="nope")
