"""Top-k and k-th value by radix select on the MI355X (csrc/kernels/topk.hip): every comparison is exact. The oracle is
the first k entries of torch.sort(..., stable=True), on a host copy where float specials are involved (test_gpu_sort.py
explains why torch's device order differs); at the largest size it comes from a device sort. The tests run
method="select" unless stated: the default method would let the sort route hide the new kernels. The gather's tile is
32768 keys, the survivor sort's 16384; the sizes cover partial rows and tiles for either, more tiles than the 256 CUs
(ticket reuse) and more than 64 predecessors (several look-back windows)."""
import pytest
import torch

from conftest import run_cli
from parallel_c_programs_amd import ops

pytestmark = pytest.mark.gpu

TILE = 32768
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 32767, 32768, 32769, 2 * TILE + 7, 300 * TILE + 13]
N_SWEEP = 70 * TILE + 5
K_SWEEP = [1, 2, 64, 65, 1000, 32768, 32769, N_SWEEP // 2, N_SWEEP - 1, N_SWEEP]
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


def _order(x, largest, host=False):
    """int64 indices of the stable sort of flat x, computed once per input and direction."""
    flat = x.flatten()
    return torch.sort(flat.cpu() if host else flat, stable=True, descending=largest).indices.to(x.device)


def _check(x, k, largest, order, sorted_=True, method="select"):
    """ops.topk against the first k entries of `order`; returns (values, indices)."""
    flat = x.flatten()
    vals, idx = ops.topk(x, k, largest=largest, sorted=sorted_, method=method)
    ri = order[:k]
    if not sorted_:
        ri = torch.sort(ri).values
    assert vals.dtype == x.dtype and idx.dtype == torch.int32 and vals.shape == idx.shape == (k,)
    assert torch.equal(idx, ri.int())
    assert torch.equal(_bits(vals), _bits(_canonical(flat[ri])))
    return vals, idx


def _ks(n):
    return sorted({k for k in (1, min(n, 65), n // 2, n - 1, n) if 1 <= k <= n})


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, n):
    g = torch.Generator(device=gpu).manual_seed(3000 + n % 9973)
    xf = (torch.randn(n, device=gpu, generator=g) * 64).round() / 64  # ties in every tile
    xi = torch.randint(-2**31, 2**31, (n,), device=gpu, generator=g, dtype=torch.int64).to(torch.int32)
    for x, largest in ((xf, True), (xi, False)):
        keep = x.clone()
        order = _order(x, largest)  # (no NaN and no need of the host order here; the largest n sorts on the device)
        for k in _ks(n):
            _check(x, k, largest, order)
        ops.scan_check(gpu)
        assert torch.equal(_bits(x), _bits(keep))  # the input is never written


@pytest.mark.parametrize("sorted_", [True, False])
def test_k_sweep(gpu, sorted_):
    g = torch.Generator(device=gpu).manual_seed(77)
    x = (torch.randn(N_SWEEP, device=gpu, generator=g) * 4096).round() / 4096
    keep = x.clone()
    order = _order(x, True)
    for k in K_SWEEP:
        _check(x, k, True, order, sorted_=sorted_)
    ops.scan_check(gpu)
    assert torch.equal(_bits(x), _bits(keep))


def test_ties_across_tiles(gpu):
    """All keys equal but 37 better ones: need_eq ends in the middle of tile 41, so the indices are the 37 and then the
    first need_eq equal ones. A wrong second prefix (the count of equal keys before a tile) shows here."""
    n = 70 * TILE + 5
    x = torch.full((n,), 2.5, device=gpu)
    better = (torch.arange(37, device=gpu) * 61001 + 123) % n  # scattered over the tiles, distinct
    assert better.unique().numel() == 37
    x[better] = 7.0 + torch.arange(37, device=gpu).float()
    # the equal keys taken are the lowest indices that are not among the better ones, up to the middle of tile 41
    last = 41 * TILE + TILE // 2
    need_eq = last + 1 - int((better <= last).sum().item())
    k = 37 + need_eq
    vals, idx = ops.topk(x, k, sorted=False, method="select")
    expect =torch.cat([better[better > last], torch.arange(last + 1, device=gpu)]).sort().values
    assert torch.equal(idx, expect.int()) and torch.equal(vals, x[expect])
    vals, idx = ops.topk(x, k, sorted=True, method="select")
    by_value = better[torch.arange(36, -1, -1, device=gpu)]  # 43.0 down to 7.0
    eq = torch.ones(last + 1, dtype=torch.bool, device=gpu)
    eq[better[better <= last]] = False
    assert torch.equal(idx, torch.cat([by_value, eq.nonzero().flatten()]).int())
    assert bool((vals[37:] == 2.5).all())
    # every key equal: the first k indices
    y = torch.full((n,), -3, device=gpu, dtype=torch.int32)
    for largest in (True, False):
        for sorted_ in (True, False):
            vals, idx = ops.topk(y, n // 2, largest=largest, sorted=sorted_, method="select")
            assert torch.equal(idx, torch.arange(n // 2, device=gpu, dtype=torch.int32)) and bool((vals == -3).all())
    ops.scan_check(gpu)


def _patterns(dev):
    n = N_SWEEP
    i = torch.arange(n, device=dev, dtype=torch.int64)
    g = torch.Generator(device=dev).manual_seed(41)
    full = torch.randint(-2**31, 2**31, (n,), device=dev, generator=g, dtype=torch.int64)
    full[:4] = torch.tensor([-2**31, 2**31 - 1, 0, -1], device=dev)
    d = (i // 16384 * 37) % 256  # one digit per 16384 keys, a different one in neighbouring blocks, in every pass
    pats = {
        "all_equal": torch.full((n,), 12345, device=dev),
        "sorted": i - n // 2,
        "reverse": n // 2 - i,
        "two_values": (i * 2654435761 >> 7) % 2 * 1000003 - 17,
        "top_byte_only": ((i * 2654435761 >> 5) % 256 - 128) << 24,  # decided in pass 1
        "low_byte_only": (i * 2654435761 >> 5) % 256 + 0x01020300,   # three passes with one bin, decided in the last
        "one_digit_per_tile": d | d << 8 | d << 16 | (d & 0x7f) << 24,
        "full_range": full,
    }
    return {k: v.to(torch.int32) for k, v in pats.items()}


@pytest.mark.parametrize("pattern", ["all_equal", "sorted", "reverse", "two_values", "top_byte_only", "low_byte_only",
                                     "one_digit_per_tile", "full_range"])
def test_key_patterns(gpu, pattern):
    x = _patterns(gpu)[pattern]
    keep = x.clone()
    n = x.numel()
    for largest in (True, False):
        order = _order(x, largest)
        # k = 1 and 3: the threshold lies in the best first-pass bin that holds keys; n - 2 and n: in the worst
        for k in (1, 3, 1000, n // 2, n - 2, n):
            _check(x, k, largest, order)
        _check(x, 1000, largest, order, sorted_=False)
    ops.scan_check(gpu)
    assert torch.equal(x, keep)


def test_first_pass_bins_0_and_255(gpu):
    """INT_MIN / INT_MAX present: for either direction k = 1 has its threshold in first-pass bin 0 (the best keys) and
    k = n in bin 255."""
    x = _patterns(gpu)["full_range"]
    n = x.numel()
    for largest in (True, False):
        v1, i1 = ops.topk(x, 1, largest=largest, method="select")
        assert v1.item() == (2**31 - 1 if largest else -2**31) and i1.item() == (1 if largest else 0)
        assert ops.kth_value(x, n, largest=largest).item() == (-2**31 if largest else 2**31 - 1)
    ops.scan_check(gpu)


def test_f32_specials(gpu):
    n = 3 * TILE + 77
    g = torch.Generator(device=gpu).manual_seed(5)
    x = torch.randn(n, device=gpu, generator=g).abs() + 0.5  # positive: the zeros are the smallest finite keys but -inf
    pos = torch.arange(len(SPECIAL), device=gpu) * 7001 + 2  # spread over the three tiles
    _bits(x)[pos] = torch.tensor(SPECIAL, dtype=torch.int32, device=gpu)
    x[TILE + 5], x[2 * TILE + 9] = -1.5, -2.5
    assert torch.isnan(x).sum().item() == 6
    keep = x.clone()
    for largest in (True, False):
        order = _order(x, largest, host=True)
        # largest: into the NaN block, past it, into the zeros, past -inf; smallest: the same from the other end
        for k in (3, 6, 7, 8, n - 9, n - 7, n - 4, n - 3, n):
            for sorted_ in (True, False):
                _check(x, k, largest, order, sorted_=sorted_)
    vals, idx = ops.topk(x, 7, method="select")
    assert bool((_bits(vals[:6]) == NAN_BITS).all()) and torch.equal(idx[:6], pos[:6].int())  # tied NaNs by index
    assert _bits(vals[6]).item() == 0x7f800000
    vals, idx = ops.topk(x, 8, largest=False, method="select")  # -inf, -2.5, -1.5, -denormal, then the four zeros
    assert idx[4:].tolist() == sorted(pos[[6, 7, 12, 13]].tolist()) and bool((_bits(vals[4:]) == 0).all())
    assert _bits(ops.kth_value(x, 3, largest=True)).item() == NAN_BITS
    assert _bits(ops.kth_value(x, 6)).item() == 0  # a zero, canonical
    ops.scan_check(gpu)
    assert torch.equal(_bits(x), _bits(keep))


def test_unsorted_is_index_order(gpu):
    g = torch.Generator(device=gpu).manual_seed(31)
    x = (torch.randn(5 * TILE + 99, device=gpu, generator=g) * 8).round() / 8
    x[::1000] = -0.0
    for k in (1, 777, 2 * TILE + 1):
        for largest in (True, False):
            vals, idx = ops.topk(x, k, largest=largest, sorted=False, method="select")
            assert bool((idx[1:] > idx[:-1]).all())  # strictly ascending
            assert torch.equal(_bits(vals), _bits(_canonical(x[idx.long()])))
    ops.scan_check(gpu)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_kth_value(gpu, dtype):
    g = torch.Generator(device=gpu).manual_seed(77)
    x = (torch.randn(N_SWEEP, device=gpu, generator=g) * 4096).round()
    x = x / 4096 if dtype == torch.float32 else (x * 50000).to(torch.int32)
    keep = x.clone()
    for largest in (False, True):
        s = ops.sort_keys(x, descending=largest)
        got = [ops.kth_value(x, k, largest=largest) for k in K_SWEEP]  # queued back to back: nothing synchronises
        for k, v in zip(K_SWEEP, got):
            assert v.dtype == dtype and v.shape == () and v.device == x.device
            assert _bits(v).item() == _bits(s[k - 1]).item()
    ops.scan_check(gpu)
    assert torch.equal(_bits(x), _bits(keep))


def test_methods_agree(gpu):
    g = torch.Generator(device=gpu).manual_seed(13)
    x = (torch.randn(9 * TILE + 321, device=gpu, generator=g) * 16).round() / 16
    n = x.numel()
    for k in (5, 4 * TILE + 3, n):
        for sorted_ in (True, False):
            a = ops.topk(x, k, sorted=sorted_, method="select")
            for method in ("sort", None):
                b = ops.topk(x, k, sorted=sorted_, method=method)
                assert b[1].dtype == torch.int32 and torch.equal(a[1], b[1]) and torch.equal(_bits(a[0]), _bits(b[0]))
    ops.scan_check(gpu)


def test_side_stream_and_repeat(gpu):
    n = 40 * TILE + 11
    g = torch.Generator(device=gpu).manual_seed(29)
    a = torch.randint(-5000, 5000, (n,), device=gpu, generator=g, dtype=torch.int32)
    order = _order(a, True)
    torch.cuda.synchronize(gpu)
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        v1, i1 = ops.topk(a, 3000, method="select")
        v2, i2 = ops.topk(a, 3000, method="select")  # back to back on one stream: the flags are reset per call
        kv = ops.kth_value(a, 3000, largest=True)
        ops.scan_check(gpu)  # the side stream's word
    ops.scan_check(gpu)
    assert torch.equal(i1, order[:3000].int()) and torch.equal(v1, a[order[:3000]])
    assert torch.equal(i1, i2) and torch.equal(v1, v2)  # two calls, identical bits
    assert kv.item() == v1[-1].item()


def test_layout(gpu):
    g = torch.Generator(device=gpu).manual_seed(23)
    n = 2 * TILE + 9
    xbuf = torch.randn(n + 8, device=gpu, generator=g)
    x = xbuf[1:n + 1]  # a view at element offset 1
    assert x.data_ptr() % 16 == 4
    _check(x, 100, True, _order(x, True))
    x3 = torch.randint(-999, 999, (300, 257), device=gpu, generator=g, dtype=torch.int32).t()  # transposed 2-D
    assert not x3.is_contiguous()
    _check(x3, 5000, False, _order(x3, False))
    vals, idx = ops.topk(torch.empty(0, device=gpu), 0, method="select")
    assert vals.shape == idx.shape == (0,) and idx.dtype == torch.int32
    vals, idx = ops.topk(x, 0, method="select")
    assert vals.shape == idx.shape == (0,) and vals.dtype == torch.float32
    ops.scan_check(gpu)


def test_workload_and_cli(gpu):
    r = run_cli("run_topk", 1048576, "--k", 1000, "--dtype", "i32", "--smallest", "--steps", 2, "--warmup", 1,
                check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.startswith("k : 1000") for ln in lines)
    assert any(ln.endswith("GB/s") for ln in lines)
    assert '"check_passed": true' in r.stdout


def test_c_abi_arguments(gpu):
    """The C entry points: bad n, k, key type and misaligned pointers are PCMX_ERR_ARG (-1) and launch nothing; n = 0 and
    k = 0 return 0 without a launch; pcmx_scan_check reads a top-k workspace."""
    import ctypes

    from parallel_c_programs_amd._native import hip_lib

    lib = hip_lib()
    lib.pcmx_topk_workspace_bytes.restype = ctypes.c_longlong
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    stream = P(torch.cuda.current_stream().cuda_stream)
    n, k, I32 = TILE + 5, 100, 1
    size = lib.pcmx_topk_workspace_bytes(LL(n), LL(k), I(1))
    assert size % 16 == 0 and size > lib.pcmx_topk_workspace_bytes(LL(n), LL(k), I(0)) > 4096
    g = torch.Generator(device=gpu).manual_seed(3)
    x = torch.randint(-2**31, 2**31, (n + 4,), device=gpu, generator=g, dtype=torch.int64).to(torch.int32)
    vo = torch.full((k + 4,), -7, device=gpu, dtype=torch.int32)
    io = torch.full((k + 4,), -7, device=gpu, dtype=torch.int32)
    ws = torch.zeros(size, dtype=torch.uint8, device=gpu)

    def topk(xp, m, kk, vop, iop, key_type=I32, wsp=ws.data_ptr()):
        return lib.pcmx_topk_b32(P(xp), LL(m), LL(kk), I(key_type), I(1), I(1), P(vop), P(iop), P(wsp), None, stream)

    def kth(xp, m, kk, op, key_type=I32):
        return lib.pcmx_kth_key_b32(P(xp), LL(m), LL(kk), I(key_type), I(1), P(op), P(ws.data_ptr()), None, stream)

    xp, vop, iop = x.data_ptr(), vo.data_ptr(), io.data_ptr()
    assert topk(xp, 1 << 30, k, vop, iop) == -1 and topk(xp, n, n + 1, vop, iop) == -1 and topk(xp, n, -1, vop, iop) == -1
    assert topk(xp, -1, 1, vop, iop) == -1 and topk(xp, n, k, vop, iop, key_type=3) == -1
    assert topk(xp + 4, n, k, vop, iop) == -1 and topk(xp, n, k, vop + 4, iop) == -1 and topk(xp, n, k, vop, iop + 4) == -1
    assert topk(None, n, k, vop, iop) == -1 and topk(xp, n, k, None, iop) == -1 and topk(xp, n, k, vop, iop, wsp=None) == -1
    assert kth(xp, n, 0, vop) == -1 and kth(xp, n, n + 1, vop) == -1 and kth(xp, 0, 0, vop) == -1
    assert kth(xp, n, 1, None) == -1 and kth(xp, n, 1, vop, key_type=-1) == -1
    assert topk(xp, 0, 0, vop, iop) == 0 and topk(xp, n, 0, vop, iop) == 0
    torch.cuda.synchronize()
    assert bool((vo == -7).all()) and bool((io == -7).all()) and bool((ws == 0).all())  # nothing ran
    ref = torch.sort(x[:n], stable=True, descending=True)
    assert topk(xp, n, k, vop, iop) == 0
    assert lib.pcmx_scan_check(P(ws.data_ptr()), stream) == 0
    assert torch.equal(vo[:k], ref.values[:k]) and torch.equal(io[:k], ref.indices[:k].int())
    assert bool((vo[k:] == -7).all()) and bool((io[k:] == -7).all())
    assert kth(xp, n, k, vop) == 0
    torch.cuda.synchronize()
    assert vo[0].item() == ref.values[k - 1].item()
