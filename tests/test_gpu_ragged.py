"""Reduction and scan over ragged segments given by offsets on the GPU (csrc/kernels/ragged.hip) against oracles
computed on a HOST copy. Every case holds at most 2^22 elements. T = RAGGED_TILE path steps (elements plus segment ends)
go to one block and RAGGED_LANE_ITEMS of them to one lane, so the cases are placed by n + S and by the path position
e_j + j of segment end j (e_j = offsets[j+1] - offsets[0]).

Oracles (torch.segment_reduce and int64 prefix differences on the host copy; the families of test_gpu_axis.py):
 * int32, full range: torch.equal with the int64 prefix differences wrapped mod 2^32 (sum) or with torch.segment_reduce
   of the float64 copy, which holds every int32 exactly (min / max); empty segments give 0 / INT32_MAX / INT32_MIN.
 * float32 min / max: torch.equal with torch.segment_reduce on multiples of 1/64: full of ties, exact.
 * float32 sums, exact form: whole numbers in [-8, 8]: every partial sum in any association order is an integer below
   2^24 (at most 2^20 elements), so the result must be torch.equal to the int64 prefix differences.
 * float32 sums, dense form: uniform(-1, 1) against the float64 result, within (terms - 1) * 2^-24 * sum|x| * (1 + 2^-10)
   per segment: the error bound of ANY summation order (each of the terms - 1 additions rounds by at most 2^-24 of a
   partial sum that is at most sum|x| (1 + 2^-24)^(terms-1)); derived, not measured. The worst observed fraction of the
   bound is printed by the last test.
No test hands the kernels offsets that break the precondition: validate=True raises before anything is launched."""
import ctypes

import pytest
import torch

from conftest import run_cli
from parallel_c_programs_amd import ops
from parallel_c_programs_amd.ops import vector as V
from parallel_c_programs_amd.ops.sparse import powerlaw_row_ptr

pytestmark = pytest.mark.gpu

OPS = ("sum", "min", "max")
T = V.RAGGED_TILE
L = V.RAGGED_LANE_ITEMS
IDENT = {"sum": (0.0, 0), "min": (float("inf"), 2**31 - 1), "max": (float("-inf"), -2**31)}
WORST = {"fraction": 0.0, "where": None}
SENTINEL = 0x5A5A5A5A


def _wrap(t):
    return (((t + 2**31) % 2**32) - 2**31).int()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(n, gpu, seed):
    """name -> (x [n] on the GPU, the ops it is checked with)"""
    g = torch.Generator(device=gpu).manual_seed(seed)
    ties = torch.round(torch.randn(n, device=gpu, generator=g) * 64) / 64
    return {
        "i32": (torch.randint(-(1 << 31), 1 << 31, (n,), device=gpu, generator=g, dtype=torch.int64).to(torch.int32), OPS),
        "ties": (torch.where(ties == 0, torch.zeros_like(ties), ties), ("min", "max")),
        "exact": (torch.randint(-8, 9, (n,), device=gpu, generator=g, dtype=torch.int64).float(), ("sum",)),
        "dense": (torch.rand(n, device=gpu, generator=g) * 2 - 1, ("sum",)),
    }


def _prefix_diff(xh, oh):
    """int64 (float64 for floating xh) sums of the segments of a host tensor, by prefix differences"""
    acc = xh.double() if xh.is_floating_point() else xh.long()
    c = torch.cat([acc.new_zeros(1), torch.cumsum(acc, 0)])
    return c[oh[1:]] - c[oh[:-1]]


def _oracle(xh, oh, name, op):
    """The expected [S] tensor in x's dtype (dense: the float64 sums), from a host copy of x and int64 host offsets"""
    s = oh.numel() - 1
    if name == "dense":
        return _prefix_diff(xh, oh)
    if op == "sum":
        r = _prefix_diff(xh.long() if name == "exact" else xh, oh)
        return _wrap(r) if name == "i32" else r.float()
    ident = IDENT[op][0 if xh.dtype == torch.float32 else 1]
    if s == 0 or xh.numel() == 0:
        return torch.full((s,), ident, dtype=xh.dtype)
    r = torch.segment_reduce(xh.double(), op, offsets=oh)
    r = torch.where(oh[1:] == oh[:-1], torch.full_like(r, float(ident)), r)  # (torch gives +-inf here as well)
    return r.to(xh.dtype)


def _within_bound(got, ref64, terms, mag, where):
    """|got - ref64| <= (terms - 1) * 2^-24 * mag * (1 + 2^-10) for every segment; remembers the worst fraction"""
    bound = (terms - 1).clamp(min=0) * 2.0 ** -24 * mag * (1 + 2.0 ** -10)
    err = (got.double() - ref64).abs()
    assert bool((err <= bound).all()), (where, float((err - bound).max()))
    frac = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    if frac > WORST["fraction"]:
        WORST["fraction"], WORST["where"] = frac, where
    return True


def _check(gpu, n, offsets, seed=0, names=("i32", "ties", "exact", "dense"), where=()):
    """ops.segment_reduce of every family and op over the given host offsets (an int64 tensor or a list)"""
    oh = torch.as_tensor(offsets, dtype=torch.int64)
    assert int(oh[0]) >= 0 and int(oh[-1]) <= n and bool((oh[1:] >= oh[:-1]).all()), "the test's own offsets"
    od = oh.to(torch.int32).to(gpu)
    od_before = od.clone()
    s = oh.numel() - 1
    data = _inputs(n, gpu, seed)
    for name in names:
        x, family_ops = data[name]
        before, xh = x.clone(), x.cpu()
        for op in family_ops:
            w = where + (n, s, name, op)
            got = ops.segment_reduce(x, od, op)
            assert got.shape == (s,) and got.dtype == x.dtype and got.device == x.device, w
            ref = _oracle(xh, oh, name, op)
            if name == "dense":
                terms = (oh[1:] - oh[:-1]).double()
                _within_bound(got.cpu(), ref, terms, _prefix_diff(xh.abs(), oh), w)
                assert not bool(torch.signbit(got.cpu()[terms == 0]).any()), w + ("an empty segment is +0.0",)
            else:
                assert torch.equal(got.cpu(), ref), w
        assert torch.equal(_bits(x), _bits(before)), (name, "the input was written")
    assert torch.equal(od, od_before), "the offsets were written"


def _random_offsets(n, s, seed, lo=0, hi=None):
    """s + 1 sorted offsets from lo to hi (n by default) with uniformly drawn borders in between"""
    hi = n if hi is None else hi
    g = torch.Generator().manual_seed(seed)
    cuts = torch.sort(torch.randint(lo, hi + 1, (max(s - 1, 0),), generator=g)).values
    return torch.cat([torch.tensor([lo]), cuts, torch.tensor([hi])])[:s + 1] if s else torch.tensor([lo])


def _offsets_from_positions(positions, n):
    """Offsets (from 0 to n) whose segment ends sit at the given ascending path positions: e_j = p_j - j; one more end
    at n closes the rest"""
    ends = [p - j for j, p in enumerate(positions)]
    assert all(0 <= a <= b for a, b in zip(ends, ends[1:])) and ends[0] >= 0 and ends[-1] <= n, ends
    return [0] + ends + [n]


# ---------------------------------------------------------------- tile counts
@pytest.mark.parametrize("path", [T - 1, T, T + 1, 3 * T + 5])
def test_path_lengths_around_the_tile(gpu, path):
    """n + S of T - 1, T, T + 1 and 3 T + 5: one tile, the exact fit, the clipped last tile, several tiles"""
    s = path // 5
    n = path - s
    _check(gpu, n, _random_offsets(n, s, path), seed=path, where=("path", path))


def test_one_segment_over_every_tile(gpu):
    """Every tile is open and the carry chain runs over all of them"""
    _check(gpu, 4 * T, [0, 4 * T], seed=1, where=("one segment",))
    _check(gpu, 4 * T, [0, 0, 4 * T, 4 * T], seed=2, where=("one segment between two empty ones",))


def test_ends_at_the_tile_borders(gpu):
    """A tile border exactly before an end (the end is the tile's first step), exactly after one (its last step), and
    between two equal ends"""
    pos = [5, 11, T, 2 * T - 1, 3 * T - 1, 3 * T]
    _check(gpu, 4 * T, _offsets_from_positions(pos, 4 * T), seed=3, where=("tile borders",))
    # many short segments around a triple end
    oh = torch.tensor(_offsets_from_positions(pos, 4 * T))
    more = torch.unique(torch.cat([oh, torch.arange(0, 4 * T, 37)]))
    _check(gpu, 4 * T, torch.sort(torch.cat([more, oh[5:7]])).values, seed=4, where=("short segments and a triple end",))


def test_ends_at_the_lane_borders(gpu):
    """The same three placements at multiples of RAGGED_LANE_ITEMS inside the first and the second tile"""
    pos = [3, 5 * L, 9 * L - 1, 12 * L - 1, 12 * L, 64 * L, 64 * L + 1, 65 * L - 1, T + 3 * L, T + 7 * L - 1,
           T + 70 * L - 1, T + 70 * L]
    _check(gpu, 2 * T + 100, _offsets_from_positions(pos, 2 * T + 100), seed=5, where=("lane borders",))


def test_long_runs_of_empty_segments(gpu):
    """At least 2 T empty segments in a row at the front, in the middle and at the back: tiles that hold only ends, and
    with the single long segment in between tiles that hold no end at all"""
    n, k = 3 * T, 2 * T + 3
    mid = n // 2 + 1
    front, back = _random_offsets(mid, 40, 6), _random_offsets(n, 3, 7, lo=mid)
    oh = torch.cat([torch.zeros(k, dtype=torch.int64), front, torch.full((k,), mid), back, torch.full((k,), n)])
    _check(gpu, n, oh, seed=6, where=("empty runs",))


def test_every_segment_one_element(gpu):
    n = 2 * T + 7
    _check(gpu, n, torch.arange(n + 1), seed=8, where=("length 1",))


def test_powerlaw_lengths(gpu):
    rp = powerlaw_row_ptr(3000, 50000)
    _check(gpu, int(rp[-1]), rp, seed=9, where=("powerlaw",))


def test_mostly_empty_segments(gpu):
    n = T + 11
    _check(gpu, n, _random_offsets(n, 4 * n, 10), seed=10, where=("S = 4 n",))


def test_a_case_at_the_size_limit_of_the_tests(gpu):
    n = (1 << 20) - 3  # the exact family's limit: partial sums stay below 2^24
    _check(gpu, n, _random_offsets(n, 5000, 11), seed=11, where=("2^20",))


# ---------------------------------------------------------------- what is read and written
@pytest.mark.parametrize("out_shift", [0, 1])
def test_offsets_inside_the_tensor_and_sentinels(gpu, out_shift):
    """offsets[0] = 7 and offsets[S] = n - 5 with x and out inside sentinel-filled buffers: the elements outside the
    segments are not read (NaN there would poison a float result), nothing outside out[:S] is written, the inputs are
    unchanged. out_shift = 1: an out that is not 16-B aligned."""
    n, s = 3 * T + 5, 700
    oh = _random_offsets(n, s, 12, lo=7, hi=n - 5)
    od = oh.to(torch.int32).to(gpu)
    for name, (src, family_ops) in _inputs(n, gpu, 12).items():
        xbuf = torch.full((n + 64,), SENTINEL, device=gpu, dtype=torch.int32).view(src.dtype)
        x = xbuf[32:32 + n]
        x.copy_(src)
        if src.dtype == torch.float32:
            x[:7] = float("nan")
            x[n - 5:] = float("nan")
        xbuf_before, xh = xbuf.clone(), torch.nan_to_num(x.cpu(), nan=0.0)  # (the oracles sum prefixes: no NaN there)
        for op in family_ops:
            obuf = torch.full((s + 80,), SENTINEL, device=gpu, dtype=torch.int32).view(src.dtype)
            out = obuf[16 + out_shift:16 + out_shift + s + 10]
            got = ops.segment_reduce(x, od, op, out=out)
            assert got.data_ptr() == out.data_ptr() and got.shape == (s,), (name, op)
            ref = _oracle(xh, oh, name, op)
            if name == "dense":
                _within_bound(got.cpu(), ref, (oh[1:] - oh[:-1]).double(), _prefix_diff(xh.abs(), oh), (name, op))
            else:
                assert torch.equal(got.cpu(), ref), (name, op)
            ob = _bits(obuf).cpu()
            lo = 16 + out_shift
            assert bool((ob[:lo] == SENTINEL).all()) and bool((ob[lo + s:] == SENTINEL).all()), (name, op, "out past S")
        assert torch.equal(_bits(xbuf), _bits(xbuf_before)), (name, "x or its surroundings were written")
    assert torch.equal(od.cpu().long(), oh)


def test_no_elements_no_segments_and_other_shapes(gpu):
    o3 = torch.zeros(4, device=gpu, dtype=torch.int32)
    for dtype, col in ((torch.float32, 0), (torch.int32, 1)):
        x0 = torch.empty(0, device=gpu, dtype=dtype)
        for op in OPS:
            r = ops.segment_reduce(x0, o3, op)
            assert torch.equal(r.cpu(), torch.full((3,), IDENT[op][col], dtype=dtype)), (dtype, op)
            assert not bool(torch.signbit(r.float()).any()) or op == "max"
            e = ops.segment_reduce(torch.ones(10, device=gpu).to(dtype), o3[:1], op)
            assert e.shape == (0,) and e.dtype == dtype and e.device.type == "cuda"
    x = torch.randint(-8, 9, (5, 7, 11), device=gpu).float()
    oh = _random_offsets(385, 20, 13)
    assert torch.equal(ops.segment_reduce(x, oh.int().to(gpu)).cpu(), _prefix_diff(x.cpu().reshape(-1).long(), oh).float())


def test_nan_and_inf_stay_in_their_segment(gpu):
    n = 3 * T + 5
    oh = _random_offsets(n, 300, 14)
    lens = oh[1:] - oh[:-1]
    j = int(torch.nonzero(lens >= 3)[100 if int((lens >= 3).sum()) > 100 else 0])  # a segment with room for both
    k = int(torch.argmax(lens))  # the longest one crosses tile and lane borders
    od = oh.int().to(gpu)
    for seg in {j, k}:
        a = int(oh[seg])
        x = torch.randint(-8, 9, (n,), device=gpu).float()
        clean = {op: ops.segment_reduce(x, od, op).cpu() for op in OPS}
        others = torch.arange(300) != seg
        xi = x.clone()
        xi[a + 1] = float("inf")
        assert float(ops.segment_reduce(xi, od, "sum")[seg]) == float("inf")
        assert float(ops.segment_reduce(xi, od, "max")[seg]) == float("inf")
        xi[a + 2] = float("nan")
        for op in OPS:
            r = ops.segment_reduce(xi, od, op).cpu()
            assert bool(torch.isnan(r[seg])), (seg, op)
            assert torch.equal(r[others], clean[op][others]), (seg, op, "a neighbouring segment changed")


def test_same_bits_on_every_call(gpu):
    for n, oh in ((3 * T + 5 - 800, _random_offsets(3 * T + 5 - 800, 800, 15)), (4 * T, torch.tensor([0, 4 * T]))):
        x = torch.rand(n, device=gpu) * 2 - 1
        od = oh.int().to(gpu)
        first = ops.segment_reduce(x, od)
        for _ in range(3):
            assert torch.equal(_bits(ops.segment_reduce(x, od)), _bits(first))


def test_validate_raises_before_any_launch(gpu):
    x = torch.ones(100, device=gpu)
    out = torch.full((8,), 123.0, device=gpu)
    for bad, index in (([0, 50, 40, 100], 2), ([-1, 50, 60, 100], 0), ([0, 50, 60, 101], 3)):
        with pytest.raises(ValueError, match=rf"offsets\[{index}\]"):
            ops.segment_reduce(x, torch.tensor(bad, device=gpu, dtype=torch.int32), out=out, validate=True)
    assert bool((out == 123.0).all())
    good = torch.tensor([0, 50, 60, 100], device=gpu, dtype=torch.int32)
    assert ops.segment_reduce(x, good, out=out, validate=True).tolist() == [50.0, 10.0, 40.0]
    assert bool((out[3:] == 123.0).all())


def test_wrong_arguments(gpu):
    x = torch.ones(10, device=gpu)
    o = torch.tensor([0, 4, 10], device=gpu, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.segment_reduce(x.double(), o)
    with pytest.raises(TypeError):
        ops.segment_reduce(x, o.long())
    with pytest.raises(TypeError):
        ops.segment_reduce(x, o, out=torch.empty(2, device=gpu, dtype=torch.int32))
    for kw in (dict(op="prod"), dict(out=torch.empty(1, device=gpu)), dict(out=torch.empty(2)),
               dict(out=torch.empty(4, device=gpu)[::2]), dict(out=x[2:6])):
        with pytest.raises(ValueError):
            ops.segment_reduce(x, o, **kw)
    for xx, oo in ((x, o.cpu()), (x, o.view(3, 1)), (x, o[::2]), (x, o[:0]), (torch.ones(4, 10, device=gpu)[:, ::2], o)):
        with pytest.raises(ValueError):
            ops.segment_reduce(xx, oo)
        with pytest.raises(ValueError):
            ops.segment_scan(xx, oo)


# ---------------------------------------------------------------- segment_scan
@pytest.mark.parametrize("exclusive", [False, True])
def test_segment_scan_against_the_host_segmented_scan(gpu, exclusive):
    path = 3 * T + 5
    s = path // 5
    n = path - s
    oh = _random_offsets(n, s, 16, lo=3, hi=n - 4)  # with empty segments; a run before offsets[0] and one after offsets[S]
    od = oh.int().to(gpu)
    heads = torch.zeros(n, dtype=torch.uint8)
    heads[oh[oh < n]] = 1
    data = _inputs(n, gpu, 16)
    for name in ("i32", "ties", "exact"):
        x, family_ops = data[name]
        for op in family_ops:
            got = ops.segment_scan(x.view(-1, 1), od, op, exclusive)
            assert got.shape == (n, 1) and got.dtype == x.dtype
            ref = ops.segmented_scan(x.cpu().view(-1, 1), heads, op, exclusive)
            assert torch.equal(got.cpu(), ref), (name, op)
    x = data["exact"][0]
    out = torch.empty_like(x)
    assert ops.segment_scan(x, od, "sum", exclusive, out=out).data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu(), ops.segmented_scan(x.cpu(), heads, "sum", exclusive))
    assert ops.segment_scan(x[:0], od[:1] * 0).shape == (0,)


# ---------------------------------------------------------------- the C entry points
ERR_ARG = -1


def _lib():
    from parallel_c_programs_amd._native import hip_lib

    lib = hip_lib()
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    for f in (lib.pcmx_segment_reduce_f32, lib.pcmx_segment_reduce_i32):
        f.argtypes = [P, LL, P, LL, I, P, P, P]
    lib.pcmx_segment_heads.argtypes = [P, LL, LL, P, P]
    lib.pcmx_segment_workspace_bytes.argtypes = [LL, LL]
    lib.pcmx_segment_workspace_bytes.restype = LL
    return lib


def test_c_abi_refusals(gpu):
    lib = _lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    n, s = 1000, 4
    x = torch.ones(n, device=gpu)
    off = torch.tensor([0, 10, 10, 500, 1000], device=gpu, dtype=torch.int32)
    out = torch.full((16,), SENTINEL, device=gpu, dtype=torch.int32)
    heads = torch.full((n,), 7, device=gpu, dtype=torch.uint8)
    ws = torch.zeros(lib.pcmx_segment_workspace_bytes(n, s), device=gpu, dtype=torch.uint8)
    xp, fp, op, wp = x.data_ptr(), off.data_ptr(), out.data_ptr(), ws.data_ptr()
    ok = dict(x=xp, n=n, off=fp, s=s, op=0, out=op, ws=wp)

    def call(fn, **kw):
        a = {**ok, **kw}
        return fn(a["x"], a["n"], a["off"], a["s"], a["op"], a["out"], a["ws"], stream)

    bad = [dict(x=None), dict(off=None), dict(out=None), dict(ws=None), dict(out=op + 4), dict(ws=wp + 4), dict(x=xp + 2),
           dict(off=fp + 2), dict(op=3), dict(op=-1), dict(n=-1), dict(s=-1), dict(n=(1 << 31) - s), dict(n=1 << 31),
           dict(n=1 << 30, s=1 << 30), dict(out=xp), dict(out=fp)]
    for fn in (lib.pcmx_segment_reduce_f32, lib.pcmx_segment_reduce_i32):
        for kw in bad:
            assert call(fn, **kw) == ERR_ARG, kw
        assert call(fn, s=0) == 0
    for args in ((None, s, n, heads.data_ptr()), (fp, s, n, None), (fp + 2, s, n, heads.data_ptr()), (fp, -1, n, heads.data_ptr()),
                 (fp, s, -1, heads.data_ptr()), (fp, s, 1 << 31, heads.data_ptr())):
        assert lib.pcmx_segment_heads(*args, stream) == ERR_ARG, args
    assert lib.pcmx_segment_heads(fp, s, 0, None, stream) == 0
    torch.cuda.synchronize(gpu)
    assert bool((out == SENTINEL).all()) and bool((x == 1).all()) and bool((heads == 7).all())  # nothing was launched
    # the accepted forms
    assert lib.pcmx_segment_workspace_bytes(n, s) % 16 == 0 and lib.pcmx_segment_workspace_bytes(-5, -5) >= 16
    off2 = torch.tensor([0, 10, 10, 500, 999], device=gpu, dtype=torch.int32)
    assert call(lib.pcmx_segment_reduce_f32, x=xp + 4, n=n - 1, off=off2.data_ptr()) == 0  # a 4-B aligned x
    assert lib.pcmx_segment_heads(fp, s, n, heads.data_ptr(), stream) == 0
    torch.cuda.synchronize(gpu)
    assert out.view(torch.float32)[:4].tolist() == [10.0, 0.0, 490.0, 499.0] and bool((out[4:] == SENTINEL).all())
    assert torch.nonzero(heads).view(-1).tolist() == [0, 10, 500] and int(heads.sum()) == 3


def test_run_ragged_cli(gpu):
    r = run_cli("run_ragged", 200000, "--mean-len", 9, "--dist", "powerlaw", "--op", "min", "--dtype", "i32", "--steps", 2,
                "--warmup", 1, check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.endswith("Gelements/s") for ln in lines)
    assert any(ln.endswith("GB/s") for ln in lines)
    assert '"check_passed": true' in r.stdout and '"elements_checked": 22222' in r.stdout


def test_zz_worst_fraction_of_the_dense_bound(gpu):
    """Runs last in this file: prints the worst observed fraction of the dense sum's bound (it is below 1 by the
    assertions above)."""
    print(f"ragged dense float32 sums: worst |error| / bound = {WORST['fraction']:.4f} at {WORST['where']}")
    assert WORST["fraction"] <= 1.0
