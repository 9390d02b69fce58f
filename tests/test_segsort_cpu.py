"""Sort inside ragged segments given by offsets (segment_sort_keys / segment_sort / segment_argsort /
segment_sort_by_key) on the host path: restricted to a segment every output equals the 1-D op on that slice, bit for
bit; elements outside the segments come through unchanged; the refusals; sort_csr_columns, the workload and the CLI. No
GPU needed."""
import itertools

import pytest
import torch

from conftest import run_cli
from parallel_c_programs_amd import ops
from parallel_c_programs_amd.models import WORKLOADS, build_workload
from parallel_c_programs_amd.ops import sparse
from parallel_c_programs_amd.ops import vector as V
from parallel_c_programs_amd.parallel.dist import Context

# the float specials of tests/test_rowsort_cpu.py: six NaNs (quiet, signalling, negative, all-ones), both zeros twice,
# both infinities, the smallest denormals of either sign
SPECIAL = [0x7fc00000, 0x7fc00001, 0x7f800001, 0xffc12345 - (1 << 32), 0x7fffffff, 0xffffffff - (1 << 32), 0, -2**31,
           0x7f800000, 0xff800000 - (1 << 32), 1, 0x80000001 - (1 << 32), 0, -2**31]

# offsets over n = 300 keys: empty segments (front, middle, back), one-key segments, offsets[0] > 0, offsets[S] < n
OFFSETS = {
    "plain": [0, 40, 41, 41, 170, 300],
    "inside": [7, 7, 30, 31, 31, 31, 200, 288, 288],
    "all_empty": [12, 12, 12],
    "one": [0, 300],
    "none": [25],  # S = 0: everything is outside
}
N = 300


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(_bits(a), _bits(b))


def _keys(n, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        x = torch.round(torch.randn(n, generator=g) * 8) / 8  # ties in every longer segment
        at = torch.randperm(n, generator=g)[:2 * len(SPECIAL)]
        _bits(x)[at] = torch.tensor(SPECIAL + SPECIAL, dtype=torch.int32)[:at.numel()]
        return x
    return torch.randint(-(1 << 31), 1 << 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)


def _expect(x, v, off, descending, bits=None):
    """(keys, flat indices, values) assembled from the 1-D ops on every slice; the elements outside as they came"""
    xf = x.reshape(-1)
    ek, ei, ev = xf.clone(), torch.arange(xf.numel(), dtype=torch.int32), v.reshape(-1).clone()
    for b, e in zip(off[:-1], off[1:]):
        sk, si = ops.sort(xf[b:e], descending, bits)
        pk, pv = ops.sort_by_key(xf[b:e], v.reshape(-1)[b:e], descending, bits)
        _same(ops.sort_keys(xf[b:e], descending, bits), sk)
        _same(pk, sk)
        _bits(ek)[b:e] = _bits(sk)
        ei[b:e] = si + b
        _bits(ev)[b:e] = _bits(pv)
    return ek.view(x.shape), ei.view(x.shape), ev.view(x.shape)


@pytest.mark.parametrize("name", list(OFFSETS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
@pytest.mark.parametrize("descending", [False, True])
def test_every_op_equals_the_1d_op_per_segment(name, dtype, descending):
    off = OFFSETS[name]
    o = torch.tensor(off, dtype=torch.int32)
    x = _keys(N, dtype, seed=len(off)).view(3, 10, 10)  # any shape, read flattened
    v = _keys(N, torch.float32 if dtype == torch.int32 else torch.int32, seed=99).view(3, 10, 10)
    x0, v0, o0 = x.clone(), v.clone(), o.clone()
    ek, ei, ev = _expect(x, v, off, descending)
    _same(ops.segment_sort_keys(x, o, descending), ek)
    sv, si = ops.segment_sort(x, o, descending)
    _same(sv, ek), _same(si, ei)
    _same(ops.segment_argsort(x, o, descending), ei)
    pk, pv = ops.segment_sort_by_key(x, v, o, descending)
    _same(pk, ek), _same(pv, ev)
    # flat indices gather the values (inside a segment the sorted keys are canonical: compare through that form)
    gathered = _bits(x).view(-1)[si.view(-1).long()]
    inside = torch.zeros(N, dtype=torch.bool)
    inside[off[0]:off[-1]] = True
    assert torch.equal(_bits(V._canonical_f32(gathered.view(dtype)))[inside], _bits(sv).view(-1)[inside])
    assert torch.equal(gathered[~inside], _bits(sv).view(-1)[~inside])  # outside: the raw bits, not canonical
    assert torch.equal(si.view(-1)[~inside], torch.arange(N, dtype=torch.int32)[~inside])
    # routes and promises do not change the host result; validate accepts these offsets
    for kw in (dict(route="classes"), dict(route="global"), dict(max_len=N), dict(validate=True), dict(validate=True, max_len=N)):
        for a, b in zip(ops.segment_sort(x, o, descending, **kw), (ek, ei)):
            _same(a, b)
    _same(x, x0), _same(v, v0), _same(o, o0)  # inputs unchanged


def test_outside_elements_keep_their_bits():
    """A NaN payload and a -0.0 before offsets[0] and behind offsets[S] come back as they were; inside they are canonical"""
    x = torch.zeros(12)
    _bits(x)[:] = torch.tensor([0x7fc12345, -2**31, 5, 0x7fc12345, -2**31, 4, 3, 2, 1, 0x7fc12345, -2**31, 9], dtype=torch.int32)
    o = torch.tensor([2, 9], dtype=torch.int32)
    k = ops.segment_sort_keys(x, o)
    assert _bits(k)[:2].tolist() == [0x7fc12345, -2**31] and _bits(k)[9:].tolist() == [0x7fc12345, -2**31, 9]
    assert _bits(k)[2:9].tolist() == [0, 1, 2, 3, 4, 5, 0x7fffffff]


@pytest.mark.parametrize("bits", [1, 5, 12, 32])
def test_bits_sorts_by_the_low_bits(bits):
    x = _keys(N, torch.int32, seed=bits)
    v = torch.arange(N, dtype=torch.int32)
    off = OFFSETS["inside"]
    o = torch.tensor(off, dtype=torch.int32)
    ek, ei, ev = _expect(x, v, off, False, bits)
    _same(ops.segment_sort_keys(x, o, bits=bits), ek)
    _same(ops.segment_argsort(x, o, bits=bits), ei)
    for a, b in zip(ops.segment_sort_by_key(x, v, o, bits=bits), (ek, ev)):
        _same(a, b)
    small = x & 0xfff
    _same(ops.segment_sort(small, o, bits=12)[1], ops.segment_sort(small, o)[1])


def test_no_keys_and_no_segments():
    o3 = torch.zeros(4, dtype=torch.int32)
    for dtype in (torch.float32, torch.int32):
        x0 = torch.empty(0, dtype=dtype)
        assert ops.segment_sort_keys(x0, o3).shape == (0,) and ops.segment_sort_keys(x0, o3).dtype == dtype
        v, i = ops.segment_sort(x0.view(0, 4), o3[:1])
        assert v.shape == (0, 4) and i.shape == (0, 4) and i.dtype == torch.int32
        assert ops.segment_argsort(x0, o3).dtype == torch.int32
        pk, pv = ops.segment_sort_by_key(x0, torch.empty(0, dtype=torch.int32), o3)
        assert pk.dtype == dtype and pv.dtype == torch.int32 and pv.shape == (0,)


def test_refusals():
    x = _keys(20, torch.float32)
    xi = _keys(20, torch.int32)
    o = torch.tensor([0, 5, 20], dtype=torch.int32)
    fns = (ops.segment_sort_keys, ops.segment_sort, ops.segment_argsort)
    for f in fns:
        for bad in (x.double(), x.half(), xi.long()):  # dtypes
            with pytest.raises(TypeError):
                f(bad, o)
        with pytest.raises(TypeError):
            f(x, o.long())
        with pytest.raises(TypeError):
            f(x, o, bits=8)  # bits is for int32 keys
        with pytest.raises(TypeError):
            f(xi, o, bits=True)
        with pytest.raises(ValueError):
            f(xi, o, bits=33)
        with pytest.raises(TypeError):
            f(x, o, max_len=4.0)
        with pytest.raises(TypeError):
            f(x, o, max_len=True)
        with pytest.raises(ValueError):
            f(x, o, max_len=-1)
        for route in ("wave", "block", "loop", "", 3):
            with pytest.raises(ValueError, match="route"):
                f(x, o, route=route)
        for oo in (o.view(3, 1), o[::2], o[:0], torch.tensor(5, dtype=torch.int32)):  # shapes of the offsets
            with pytest.raises(ValueError):
                f(x, oo)
        with pytest.raises(ValueError, match="contiguous"):
            f(torch.ones(4, 10)[:, ::2], o)
        with pytest.raises(ValueError, match="offsets are on"):
            f(x, o.to("meta"))
        big = torch.zeros(1, dtype=torch.int32).expand(V.SORT_MAX_N + 1)  # no memory behind it
        with pytest.raises(ValueError, match="2\\^30"):
            f(big, o)
        with pytest.raises(ValueError, match="segments; at most 2\\^30 - 1"):
            f(xi, torch.zeros(1, dtype=torch.int32).expand(V.SEGSORT_MAX_S + 2))
    with pytest.raises(TypeError):
        ops.segment_sort_by_key(x, x.double(), o)
    with pytest.raises(TypeError):
        ops.segment_sort_by_key(x.double(), x, o)
    with pytest.raises(ValueError, match="shape"):
        ops.segment_sort_by_key(x, x[:19], o)
    with pytest.raises(ValueError, match="shape"):
        ops.segment_sort_by_key(x.view(4, 5), x, o)
    with pytest.raises(ValueError, match="contiguous"):
        ops.segment_sort_by_key(x.view(4, 5), torch.ones(5, 4).t(), o)
    with pytest.raises(ValueError, match="values are on"):
        ops.segment_sort_by_key(x, x.to("meta"), o)


def test_validate_messages_and_max_len():
    x = torch.ones(100)
    for bad, index in (([0, 50, 40, 100], 2), ([-1, 50, 60, 100], 0), ([0, 50, 60, 101], 3)):
        ob = torch.tensor(bad, dtype=torch.int32)
        for f in (ops.segment_sort_keys, ops.segment_sort, ops.segment_argsort):
            with pytest.raises(ValueError, match=rf"offsets\[{index}\]"):
                f(x, ob, validate=True)
        with pytest.raises(ValueError, match=rf"offsets\[{index}\]"):
            ops.segment_sort_by_key(x, x, ob, validate=True)
    good = torch.tensor([0, 50, 60, 100], dtype=torch.int32)
    with pytest.raises(ValueError, match=r"segment 0 has 50 keys, more than max_len = 49"):
        ops.segment_sort_keys(x, good, validate=True, max_len=49)
    assert ops.segment_sort_keys(x, good, validate=True, max_len=50).shape == (100,)
    # without validate broken offsets give an unspecified result, but a result: clamped, nothing raised
    for bad in ([0, 50, 40, 100], [-7, 50, 60, 1000], [90, 10]):
        v, i = ops.segment_sort(x, torch.tensor(bad, dtype=torch.int32))
        assert v.shape == (100,) and int(i.min()) >= 0 and int(i.max()) < 100


def test_route_classes_refuses_a_long_segment():
    n = V.SEGSORT_MAX_LEN + 1
    x = _keys(n + 10, torch.int32)
    with pytest.raises(ValueError, match="classes"):
        ops.segment_sort_keys(x, torch.tensor([3, 3 + n], dtype=torch.int32), route="classes")
    o = torch.tensor([3, 3 + n - 1, n + 10], dtype=torch.int32)
    _same(ops.segment_sort_keys(x, o, route="classes"), ops.segment_sort_keys(x, o))


def test_exported_constants():
    lim = V.SEGSORT_CLASS_LIMITS
    assert list(lim) == sorted(set(lim)) and lim[-1] == V.SEGSORT_MAX_LEN == V.ROWSORT_MAX_COLS
    assert lim[V.SEGSORT_WAVE_CLASSES - 1] == V.ROWSORT_WAVE_COLS
    assert V.SEGSORT_GRID_MULT >= 1
    for name in ("segment_sort_keys", "segment_sort", "segment_argsort", "segment_sort_by_key"):
        assert name in ops.__all__ and callable(getattr(ops, name))


@pytest.mark.parametrize("vdtype", [torch.float32, torch.int32])
def test_sort_csr_columns_against_a_per_row_host_sort(vdtype):
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(0, 9, (40,), generator=g)
    rp = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    nnz = int(rp[-1])
    col = torch.randint(0, 12, (nnz,), generator=g, dtype=torch.int64).to(torch.int32)  # repeated columns in a row
    val = torch.arange(nnz).to(vdtype)
    col0, val0 = col.clone(), val.clone()
    for row_ptr in (rp, rp.int()):
        c, v = sparse.sort_csr_columns(row_ptr, col, val)
        assert c.dtype == torch.int32 and v.dtype == vdtype and c.shape == col.shape
        for r in range(40):
            b, e = int(rp[r]), int(rp[r + 1])
            order = torch.sort(col[b:e], stable=True).indices
            assert torch.equal(c[b:e], col[b:e][order]) and torch.equal(v[b:e], val[b:e][order]), r
    assert torch.equal(col, col0) and torch.equal(val, val0)
    _same(sparse.sort_csr_columns(rp, col, val, max_len=8)[1], v)
    with pytest.raises(TypeError):
        sparse.sort_csr_columns(rp.float(), col, val)
    with pytest.raises(TypeError):
        sparse.sort_csr_columns(rp, col.long(), val)
    with pytest.raises(ValueError):
        sparse.sort_csr_columns(rp, col, val[:-1])


@pytest.mark.parametrize("mode,dtype,dist", list(itertools.product(["keys", "index", "pairs"], ["f32", "i32"],
                                                                    ["uniform", "powerlaw"])))
def test_workload_on_cpu(mode, dtype, dist):
    assert "segsort" in WORKLOADS
    w = build_workload("segsort", Context(device=torch.device("cpu")), n=2000, mean_len=9, dist=dist, mode=mode, dtype=dtype,
                       descending=dtype == "i32")
    w.step()
    r = w.check()
    assert r["check_passed"] and r["elements_checked"] == 2000
    w.torch_step()
    assert w.work_per_step() > 0 and w.report(1.0, 1)["segments"] == 2000 // 9
    # the check has power: one changed output element fails it
    w.out[0].view(-1)[3] += 1
    assert not w.check()["check_passed"]
    with pytest.raises(ValueError):
        build_workload("segsort", Context(device=torch.device("cpu")), n=100, mode="sideways")
    with pytest.raises(ValueError):
        build_workload("segsort", Context(device=torch.device("cpu")), n=100, dist="bimodal")


def test_run_segsort_cli_on_the_cpu():
    r = run_cli("run_segsort", 3000, "--mean-len", 11, "--dist", "equal", "--mode", "index", "--dtype", "i32", "--descending",
                "--route", "classes", "--device", "cpu", "--steps", 1, "--warmup", 0, check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.endswith("Gkeys/s") for ln in lines)
    assert any(ln.endswith("GB/s") for ln in lines)
    assert '"check_passed": true' in r.stdout and '"elements_checked": 3000' in r.stdout and '"workload": "segsort"' in r.stdout
