"""Run-length encode / reduce-by-key on the MI355X (csrc/kernels/segreduce.hip). Oracles: torch.unique_consecutive on
the int32 view of the keys for run keys and lengths, the exclusive cumsum of the lengths for the start offsets, int64
index_add_ / scatter_reduce_ (wrapped) for int32 values. Every integer comparison is torch.equal, also on the int32
views of the run keys. Integer-valued float32 values with every run sum below 2^24 must sum bit-exactly; float min /
max are exact; random float sums are held to the bound of ANY summation order, |got - ref| <= g * sum|x| per run with
g = (L-1)u / (1 - (L-1)u), u = 2^-24, L the run length, against an fp64 index_add_. The tile is T = 32768 keys; sizes
cover the tail of the last tile for every n mod 4, one and several tiles, more tiles than CUs (ticket reuse) and more
than 64 predecessors (a multi-window look-back)."""
import pytest
import torch

from conftest import run_cli
from parallel_c_programs_amd import ops

pytestmark = pytest.mark.gpu

T = 32768
SIZES = [0, 1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, T - 1, T, T + 1, 2 * T + 7, 300 * T + 13]
N_PAT = 70 * T + 5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _geometric_ids(n, mean_run, gen, dev):
    """int64 run ids of n elements with geometric run lengths of the given mean (0: one run; 1: all distinct)."""
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev)
    p = 0.0 if mean_run == 0 else 1.0 / mean_run
    return torch.cumsum(torch.rand(n, device=dev, generator=gen) < p, 0)


def _ref_runs(keys):
    return torch.unique_consecutive(_bits(keys.reshape(-1)), return_inverse=True, return_counts=True)


def _wrap(s):
    return (((s + 2**31) % 2**32) - 2**31).int()


def _ref_reduce(inv, k, values, op):
    v = values.reshape(-1)
    if op == "sum":
        if v.dtype == torch.int32:
            return _wrap(torch.zeros(k, dtype=torch.int64, device=v.device).index_add_(0, inv, v.long()))
        return torch.zeros(k, dtype=torch.float64, device=v.device).index_add_(0, inv, v.double())
    return torch.zeros(k, dtype=v.dtype, device=v.device).scatter_reduce_(0, inv, v, "amin" if op == "min" else "amax",
                                                                          include_self=False)


def _check_all(keys, gen, ops_list=("sum",)):
    """Run-length encode (with starts) and reduce_by_key (int32 values, integer-valued float32 values) of one key
    tensor against the oracles; returns the run count."""
    dev, n = keys.device, keys.numel()
    rk_ref, inv, cnt_ref = _ref_runs(keys)
    k = rk_ref.numel()
    rk, rc, rs, num = ops.run_length_encode(keys, starts=True)
    assert num.dtype == torch.int64 and num.dim() == 0 and num.device == keys.device
    assert rk.dtype == keys.dtype and rc.dtype == torch.int32 and rs.dtype == torch.int32
    assert rk.numel() == n and rc.numel() == n and rs.numel() == n
    assert num.item() == k
    assert torch.equal(_bits(rk[:k]), rk_ref)
    assert torch.equal(rc[:k].long(), cnt_ref)
    assert torch.equal(rs[:k].long(), torch.cumsum(cnt_ref, 0) - cnt_ref)
    rk2, rc2, num2 = ops.run_length_encode(keys)
    assert num2.item() == k and torch.equal(_bits(rk2[:k]), rk_ref) and torch.equal(rc2[:k].long(), cnt_ref)
    vi = torch.randint(-1000, 1000, (n,), device=dev, generator=gen, dtype=torch.int64).int()
    vf = torch.randint(0, 4, (n,), device=dev, generator=gen, dtype=torch.int64).float()  # run sums < 2^24: exact
    assert n * 3 < 2**24 or cnt_ref.numel() == 0 or cnt_ref.max().item() * 3 < 2**24
    for op in ops_list:
        for v in (vi, vf):
            gk, ga, gnum = ops.reduce_by_key(keys, v, op)
            assert ga.dtype == v.dtype and gnum.item() == k
            assert torch.equal(_bits(gk[:k]), rk_ref)
            ref = _ref_reduce(inv, k, v, op)
            assert torch.equal(ga[:k], ref.to(v.dtype)), (op, v.dtype)
    return k


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, n):
    g = torch.Generator(device=gpu).manual_seed(2000 + n % 9973)
    ids = _geometric_ids(n, 3.0, g, gpu)
    _check_all(ids.int(), g)
    _check_all(ids.float(), g)  # ids < 2^24: exact, neighbouring runs stay different
    ops.scan_check(gpu)


@pytest.mark.parametrize("regime", ["all_equal", "all_distinct", "mean_1.5", "mean_100", "mean_1e5"])
def test_run_length_regimes(gpu, regime):
    g = torch.Generator(device=gpu).manual_seed(41)
    mean = {"all_equal": 0, "all_distinct": 1, "mean_1.5": 1.5, "mean_100": 100, "mean_1e5": 1e5}[regime]
    keys = (_geometric_ids(N_PAT, mean, g, gpu) * 3 - 5).int()
    k = _check_all(keys, g, ("sum", "min", "max"))
    if regime == "all_equal":
        assert k == 1  # one run across every tile: the lead chain at full length
    if regime == "all_distinct":
        assert k == N_PAT
    ops.scan_check(gpu)


def _border_patterns(dev):
    n = N_PAT
    i = torch.arange(n, device=dev)
    t = i // T
    one_head = (i % T) == (t * 997 + 31) % T
    one_head[0] = True
    no_head_in_last = torch.clamp(t, max=n // T - 1)  # the 5-element last tile goes on with the previous tile's key
    last_own = torch.zeros(n, dtype=torch.int64, device=dev)
    last_own[-1] = 1
    return {
        "tile_aligned": t,
        "tile_aligned_plus1": (i + 1) // T,
        "tile_aligned_minus1": (i + T - 1) // T,
        "runs_3T_plus_1": i // (3 * T + 1),
        "runs_4096": i // 4096,
        "runs_256": i // 256,
        "one_head_per_tile": torch.cumsum(one_head, 0),
        "distinct_tile_then_two_equal_tiles": torch.where(t % 3 == 0, i, -t),
        "last_element_own_run": last_own,
        "no_head_in_last_tile": no_head_in_last,
    }


@pytest.mark.parametrize("pattern", ["tile_aligned", "tile_aligned_plus1", "tile_aligned_minus1", "runs_3T_plus_1",
                                     "runs_4096", "runs_256", "one_head_per_tile", "distinct_tile_then_two_equal_tiles",
                                     "last_element_own_run", "no_head_in_last_tile"])
def test_border_patterns(gpu, pattern):
    g = torch.Generator(device=gpu).manual_seed(43)
    keys = _border_patterns(gpu)[pattern].int()
    k = _check_all(keys, g)
    expect = {"tile_aligned": 71, "tile_aligned_plus1": 71, "tile_aligned_minus1": 72, "one_head_per_tile": 71,
              "last_element_own_run": 2, "no_head_in_last_tile": 70, "runs_4096": 70 * 8 + 1}.get(pattern)
    if expect is not None:
        assert k == expect
    ops.scan_check(gpu)


def test_key_bits(gpu):
    """Float keys with both zeros, NaNs of several payloads, infinities and a denormal at run borders, and int32
    extremes: compared as bit patterns, run keys come back bit-identical."""
    n = 3 * T + 77
    g = torch.Generator(device=gpu).manual_seed(47)
    special = torch.tensor([0, -2**31, 0x7fc00000, 0x7fc00000, 0x7fc00001, 0x7f800001, 0xffc12345 - (1 << 32), 0x7fffffff,
                            0x7f800000, 0xff800000 - (1 << 32), 1, 1, 0, 0, -2**31, -2**31],
                           dtype=torch.int32, device=gpu)
    kb = _bits(_geometric_ids(n, 3.0, g, gpu).float()).clone()
    for base in (0, 4090, T - 8, 2 * T - 3, n - special.numel()):  # lane, row, wave and tile borders, both ends
        kb[base:base + special.numel()] = special
    keys = kb.view(torch.float32)
    k = _check_all(keys, g)
    rk, rc, num = ops.run_length_encode(keys[:5])
    assert num.item() == 4 and rc[:4].tolist() == [1, 1, 2, 1]  # 0.0 | -0.0 | nan nan | nan'
    assert torch.isnan(ops.unique_consecutive(keys)).sum().item() >= 5 and k > 0
    ki = _geometric_ids(n, 3.0, g, gpu).int()
    ki[:6] = torch.tensor([-2**31, -2**31, 2**31 - 1, 2**31 - 1, 0, -1], dtype=torch.int32, device=gpu)
    ki[T - 1], ki[T] = 2**31 - 1, -2**31
    _check_all(ki, g)


@pytest.mark.parametrize("op", ["sum", "min", "max"])
def test_ops_both_dtypes(gpu, op):
    n = 5 * T + 3
    g = torch.Generator(device=gpu).manual_seed(53)
    keys = _geometric_ids(n, 40.0, g, gpu).int()
    _, inv, _ = _ref_runs(keys)
    k = int(inv[-1].item()) + 1
    vi = torch.randint(-2**31, 2**31 - 1, (n,), device=gpu, generator=g, dtype=torch.int64).int()  # sums wrap
    _, ga, num = ops.reduce_by_key(keys, vi, op)
    ref = _ref_reduce(inv, k, vi, op)
    assert num.item() == k and torch.equal(ga[:k], ref)
    if op == "sum":
        exact = torch.zeros(k, dtype=torch.int64, device=gpu).index_add_(0, inv, vi.long())
        assert bool((exact.abs() >= 2**31).any())  # the test does wrap
    vf = torch.randn(n, device=gpu, generator=g)  # NaN-free
    _, gf, num = ops.reduce_by_key(keys, vf, op)
    assert num.item() == k
    if op != "sum":
        assert torch.equal(gf[:k], _ref_reduce(inv, k, vf, op))


def test_float_sum_within_any_order_bound(gpu):
    n = N_PAT
    g = torch.Generator(device=gpu).manual_seed(59)
    u = 2.0 ** -24
    for mean in (2, 100, 1e5):
        keys = _geometric_ids(n, mean, g, gpu).int()
        x = torch.rand(n, device=gpu, generator=g)
        _, inv, cnt = _ref_runs(keys)
        k = cnt.numel()
        ref = torch.zeros(k, dtype=torch.float64, device=gpu).index_add_(0, inv, x.double())  # = sum|x|: x >= 0
        _, ga, num = ops.reduce_by_key(keys, x, "sum")
        assert num.item() == k
        lu = (cnt.double() - 1) * u
        bound = lu / (1 - lu) * ref
        err = (ga[:k].double() - ref).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"mean run {mean}: worst err / bound = {worst:.3f}")
        assert bool((err <= bound).all()), worst


def test_float_sum_is_deterministic(gpu):
    n = 300 * T + 13
    g = torch.Generator(device=gpu).manual_seed(61)
    keys = _geometric_ids(n, 1e5, g, gpu).int()
    x = torch.rand(n, device=gpu, generator=g)
    _, a, num = ops.reduce_by_key(keys, x, "sum")
    _, b, _ = ops.reduce_by_key(keys, x, "sum")
    k = num.item()
    torch.cuda.synchronize(gpu)
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        _, c, cnum = ops.reduce_by_key(keys, x, "sum")
    s.synchronize()
    assert cnum.item() == k and k > 50
    assert torch.equal(a[:k], b[:k]) and torch.equal(a[:k], c[:k])


def test_layout(gpu):
    n = 2 * T + 9
    g = torch.Generator(device=gpu).manual_seed(67)
    # keys and values as views at element offset 1 of larger buffers
    kbuf = _geometric_ids(n + 8, 3.0, g, gpu).int()
    vbuf = torch.randint(-9, 9, (n + 8,), device=gpu, generator=g, dtype=torch.int64).int()
    keys, vals = kbuf[1:n + 1], vbuf[1:n + 1]
    assert keys.data_ptr() % 16 == 4 and vals.data_ptr() % 16 == 4
    rk_ref, inv, cnt_ref = _ref_runs(keys)
    k = rk_ref.numel()
    ref = _ref_reduce(inv, k, vals, "sum")
    _check_all(keys, g)
    gk, ga, num = ops.reduce_by_key(keys, vals, "sum")
    assert num.item() == k and torch.equal(ga[:k], ref) and torch.equal(_bits(gk[:k]), rk_ref)
    # non-contiguous views: every other element, and a transposed 2-D view
    k2 = _geometric_ids(2 * n, 1.3, g, gpu).int()[::2]
    assert not k2.is_contiguous()
    _check_all(k2, g)
    k3 = torch.randint(0, 2, (300, 257), device=gpu, generator=g, dtype=torch.int64).int().t()
    v3 = torch.randint(-9, 9, (300, 257), device=gpu, generator=g, dtype=torch.int64).int().t()
    r3, i3, _ = _ref_runs(k3)
    _, a3, n3 = ops.reduce_by_key(k3, v3, "sum")
    assert n3.item() == r3.numel() and torch.equal(a3[:r3.numel()], _ref_reduce(i3, r3.numel(), v3, "sum"))
    _check_all(k3, g)
    # caller outputs larger than needed are left untouched past the count (aligned, then misaligned)
    for shift in (0, 1):
        ok = torch.full((n + 64 + shift,), -7, device=gpu, dtype=torch.int32)[shift:]
        oc = torch.full((n + 64 + shift,), -7, device=gpu, dtype=torch.int32)[shift:]
        os_ = torch.full((n + 64 + shift,), -7, device=gpu, dtype=torch.int32)[shift:]
        oa = torch.full((n + 64 + shift,), -7, device=gpu, dtype=torch.int32)[shift:]
        rk, rc, rs, num = ops.run_length_encode(keys, starts=True, out_keys=ok, out_counts=oc, out_starts=os_)
        assert rk.data_ptr() == ok.data_ptr() and rc.data_ptr() == oc.data_ptr() and rs.data_ptr() == os_.data_ptr()
        assert num.item() == k and torch.equal(ok[:k], rk_ref) and torch.equal(oc[:k].long(), cnt_ref)
        assert torch.equal(os_[:k].long(), torch.cumsum(cnt_ref, 0) - cnt_ref)
        assert bool((ok[k:] == -7).all()) and bool((oc[k:] == -7).all()) and bool((os_[k:] == -7).all())
        ok.fill_(-7)
        _, ra, num = ops.reduce_by_key(keys, vals, "sum", out_keys=ok, out=oa)
        assert ra.data_ptr() == oa.data_ptr() and torch.equal(oa[:k], ref) and torch.equal(ok[:k], rk_ref)
        assert bool((oa[k:] == -7).all()) and bool((ok[k:] == -7).all())
    # outputs that overlap the inputs: the inputs are cloned first
    kb2, vb2 = kbuf.clone(), vbuf.clone()
    gk, ga, num = ops.reduce_by_key(kb2[4:n + 4], vb2[4:n + 4], "sum", out_keys=kb2[:n + 4], out=vb2[:n + 4])
    r4, i4, _ = _ref_runs(kbuf[4:n + 4])
    assert num.item() == r4.numel() and torch.equal(gk[:r4.numel()], r4)
    assert torch.equal(ga[:r4.numel()], _ref_reduce(i4, r4.numel(), vbuf[4:n + 4], "sum"))


def test_stream_error_word_and_neighbours(gpu):
    """scan, two reduce_by_key with different keys, select, sort, scan and scan_check back to back on one side stream:
    the workspace is zeroed per launch and the error word is shared."""
    n = 40 * T + 11
    g = torch.Generator(device=gpu).manual_seed(71)
    k1 = _geometric_ids(n, 5.0, g, gpu).int()
    k2 = _geometric_ids(n, 5000.0, g, gpu).int()
    v = torch.randint(-100, 100, (n,), device=gpu, generator=g, dtype=torch.int64).int()
    mask = torch.rand(n, device=gpu, generator=g) < 0.3
    xi = torch.randint(0, 4, (n,), device=gpu, generator=g).float()  # integer-valued: the f32 scan is exact
    ref_scan = torch.cumsum(xi.double(), 0).float()
    torch.cuda.synchronize(gpu)
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        y0 = ops.scan(xi)
        _, a1, n1 = ops.reduce_by_key(k1, v, "sum")
        _, a2, n2 = ops.reduce_by_key(k2, v, "sum")
        o, c = ops.compact(v, mask)
        srt = ops.sort_keys(v)
        y1 = ops.scan(xi)
        ops.scan_check(gpu)  # synchronises s and raises if any look-back on it gave up
    for keys, a, num in ((k1, a1, n1), (k2, a2, n2)):
        r, inv, _ = _ref_runs(keys)
        assert num.item() == r.numel() and torch.equal(a[:r.numel()], _ref_reduce(inv, r.numel(), v, "sum"))
    assert c.item() == mask.sum().item() and torch.equal(o[:c.item()], v[mask])
    assert torch.equal(srt, torch.sort(v).values)
    assert torch.equal(y0, ref_scan) and torch.equal(y1, ref_scan)


def test_compositions(gpu):
    n = 3 * T + 77
    g = torch.Generator(device=gpu).manual_seed(73)
    for dtype in (torch.int32, torch.float32):
        x = torch.randint(-500, 500, (n,), device=gpu, generator=g, dtype=torch.int64).to(dtype)
        if dtype == torch.float32:
            x[::101] = -0.0
            x[1::101] = 0.0
        rv, rc = torch.unique(x, return_counts=True)
        v, c = ops.unique(x, return_counts=True)
        assert v.dtype == dtype and c.dtype == torch.int32 and v.shape == rv.shape
        assert torch.equal(v, rv) and torch.equal(c.long(), rc) and torch.equal(ops.unique(x), rv)
        vals = torch.randint(-50, 50, (n,), device=gpu, generator=g, dtype=torch.int64).float()  # exact sums
        uk, sums = ops.sum_by_key(x, vals)
        sk, order = torch.sort(x, stable=True)
        rk, inv = torch.unique_consecutive(sk, return_inverse=True)
        ref = torch.zeros(rk.numel(), dtype=torch.float32, device=gpu).index_add_(0, inv, vals[order])
        assert torch.equal(uk, rk) and torch.equal(sums, ref)
    ops.scan_check(gpu)


def test_c_abi_arguments_and_workspace_check(gpu):
    """The C entry points: n >= 2^31, a null or misaligned pointer and a bad op are PCMX_ERR_ARG (-1) and launch
    nothing, n <= 0 stores 0 runs, and pcmx_scan_check reads a segreduce workspace."""
    import ctypes

    from parallel_c_programs_amd._native import hip_lib

    lib = hip_lib()
    lib.pcmx_segreduce_workspace_bytes.restype = ctypes.c_longlong
    P, LL = ctypes.c_void_p, ctypes.c_longlong
    stream = P(torch.cuda.current_stream().cuda_stream)
    n = T + 5
    wsb = lib.pcmx_segreduce_workspace_bytes(LL(n))
    assert wsb >= 16 + 2 * 8 + 3 * 8 and wsb % 16 == 0
    keys = (torch.arange(n + 4, device=gpu) // 3).int()
    vals = torch.arange(n + 4, device=gpu, dtype=torch.int32)
    fvals = vals.float()
    ok, oc, os_, oa = (torch.full((n + 4,), -7, device=gpu, dtype=torch.int32) for _ in range(4))
    of = torch.full((n + 4,), -7.0, device=gpu)
    num = torch.full((), -1, device=gpu, dtype=torch.int64)
    ws = torch.empty(wsb, dtype=torch.uint8, device=gpu)
    kp, vp, fp = keys.data_ptr(), vals.data_ptr(), fvals.data_ptr()
    okp, ocp, osp, oap, ofp = ok.data_ptr(), oc.data_ptr(), os_.data_ptr(), oa.data_ptr(), of.data_ptr()
    numA, wsA = P(num.data_ptr()), P(ws.data_ptr())

    def rle(k, m, rk, c, st):
        return lib.pcmx_run_length_encode_b32(P(k), LL(m), P(rk), P(c), P(st), numA, wsA, None, stream)

    def rbk_i(k, v, m, op, rk, a):
        return lib.pcmx_reduce_by_key_i32(P(k), P(v), LL(m), op, P(rk), P(a), numA, wsA, None, stream)

    def rbk_f(k, v, m, op, rk, a):
        return lib.pcmx_reduce_by_key_f32(P(k), P(v), LL(m), op, P(rk), P(a), numA, wsA, None, stream)

    assert rle(kp, 1 << 31, okp, ocp, osp) == -1
    assert rle(kp + 4, n, okp, ocp, osp) == -1 and rle(kp, n, okp + 4, ocp, osp) == -1
    assert rle(kp, n, okp, ocp + 4, osp) == -1 and rle(kp, n, okp, ocp, osp + 4) == -1
    assert rle(None, n, okp, ocp, osp) == -1 and rle(kp, n, None, ocp, osp) == -1 and rle(kp, n, okp, None, osp) == -1
    assert rbk_i(kp, vp, 1 << 31, 0, okp, oap) == -1 and rbk_i(kp, vp + 4, n, 0, okp, oap) == -1
    assert rbk_i(kp, None, n, 0, okp, oap) == -1 and rbk_i(kp, vp, n, 0, okp, oap + 8) == -1
    assert rbk_i(kp, vp, n, 3, okp, oap) == -1 and rbk_i(kp, vp, n, -1, okp, oap) == -1
    assert rbk_f(kp, fp, n, 3, okp, ofp) == -1 and rbk_f(kp + 4, fp, n, 0, okp, ofp) == -1
    assert rbk_f(kp, fp, n, 0, okp, None) == -1
    assert lib.pcmx_run_length_encode_b32(P(kp), LL(n), P(okp), P(ocp), P(osp), numA, None, None, stream) == -1
    torch.cuda.synchronize()
    untouched = all(bool((t == -7).all()) for t in (ok, oc, os_, oa, of))
    assert num.item() == -1 and untouched  # nothing ran
    assert rle(kp, 0, okp, ocp, osp) == 0
    torch.cuda.synchronize()
    assert num.item() == 0 and all(bool((t == -7).all()) for t in (ok, oc, os_))
    num.fill_(-1)
    assert rbk_f(kp, fp, 0, 0, okp, ofp) == 0
    torch.cuda.synchronize()
    assert num.item() == 0 and bool((of == -7).all())
    # a real call: starts NULL, then run keys NULL for reduce_by_key
    rk_ref, inv, cnt_ref = _ref_runs(keys[:n])
    k = rk_ref.numel()
    assert rle(kp, n, okp, ocp, None) == 0
    assert lib.pcmx_scan_check(wsA, stream) == 0
    assert num.item() == k and torch.equal(ok[:k], rk_ref) and torch.equal(oc[:k].long(), cnt_ref)
    assert bool((ok[k:] == -7).all()) and bool((oc[k:] == -7).all()) and bool((os_ == -7).all())
    ok.fill_(-7)
    assert rbk_i(kp, vp, n, 2, None, oap) == 0
    assert lib.pcmx_scan_check(wsA, stream) == 0
    assert num.item() == k and torch.equal(oa[:k], _ref_reduce(inv, k, vals[:n], "max")) and bool((ok == -7).all())
    assert bool((oa[k:] == -7).all())


@pytest.mark.parametrize("mode", ["rle", "sum", "unique"])
def test_workload(gpu, mode):
    from parallel_c_programs_amd.models import build_workload
    from parallel_c_programs_amd.parallel.dist import Context

    for dtype, mean_run in (("f32", 4.0), ("i32", 0 if mode != "unique" else 1000.0)):
        w = build_workload("segreduce", Context(device=gpu), n=1 << 20, mean_run=mean_run, mode=mode, dtype=dtype)
        w.step()
        r = w.check()
        assert r["check_passed"] and r["lookback_ok"] and r["runs"] == r["runs_torch"], r
        if mode != "unique" and mean_run == 4.0:
            assert abs(r["runs"] / (1 << 20) - 0.25) < 0.01
        assert w.torch_step()[0].numel() == r["runs"]


@pytest.mark.parametrize("mode", ["rle", "sum", "unique"])
def test_cli(gpu, mode):
    r = run_cli("run_segreduce", 1048576, "--mean-run", 10, "--mode", mode, "--dtype", "i32", "--steps", 2, "--warmup", 1,
                check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.startswith("runs : ") for ln in lines)
    assert any(ln.endswith("GB/s") for ln in lines)
    assert '"check_passed": true' in r.stdout
