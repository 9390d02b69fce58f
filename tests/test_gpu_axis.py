"""Reduce and scan along a dimension on the GPU (csrc/kernels/axis.hip) against oracles computed on a HOST copy. Routes
are forced with route= so the default rule cannot hide a kernel; one test runs the default rule over the same shapes.
Every case holds at most 2^22 elements.

Oracles (one host cumulative per input and op; the reduce is its last entry along the dimension):
 * int32: torch.equal with the int64 result wrapped mod 2^32.
 * float32 min / max: torch.equal with torch.cummin / cummax (amin / amax) on multiples of 1/64 from a normal
   distribution with no zeros of mixed sign: full of ties, exact.
 * float32 sums, exact form: whole numbers in [-8, 8]: every partial sum in any association order is an integer below
   2^24 for n <= 2^20, so the result must be torch.equal to the int64 sum: a dropped, doubled or misplaced element shows
   in any route with no tolerance.
 * float32 sums, dense form: uniform(-1, 1) against the float64 result, within (m - 1) * 2^-24 * sum|x| * (1 + 2^-10)
   per output, m its number of terms: the error bound of ANY summation order (each of the m - 1 additions rounds by at
   most 2^-24 of a partial sum that is at most sum|x| (1 + 2^-24)^(m-1)); derived, not measured. The worst observed
   fraction of the bound is printed by the last test."""
import ctypes

import pytest
import torch

from conftest import run_cli
from parallel_c_programs_amd import ops
from parallel_c_programs_amd.ops import vector as V

pytestmark = pytest.mark.gpu

OPS = ("sum", "min", "max")
MAX_ELEMS = 1 << 22
TILE = 1024
IDENT = {"sum": (0.0, 0), "min": (float("inf"), 2**31 - 1), "max": (float("-inf"), -2**31)}
WORST = {"fraction": 0.0, "where": None}


def _wrap(t):
    return (((t + 2**31) % 2**32) - 2**31).int()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(outer, n, inner, gpu, seed):
    """name -> (x [outer, n, inner] on the GPU, the ops it is checked with)"""
    g = torch.Generator(device=gpu).manual_seed(seed)
    shape = (outer, n, inner)
    ties = torch.round(torch.randn(shape, device=gpu, generator=g) * 64) / 64
    return {
        "i32": (torch.randint(-(1 << 31), 1 << 31, shape, device=gpu, generator=g, dtype=torch.int64).to(torch.int32), OPS),
        "ties": (torch.where(ties == 0, torch.zeros_like(ties), ties), ("min", "max")),
        "exact": (torch.randint(-8, 9, shape, device=gpu, generator=g, dtype=torch.int64).float(), ("sum",)),
        "dense": (torch.rand(shape, device=gpu, generator=g) * 2 - 1, ("sum",)),
    }


def _host_inclusive(xh, name, op):
    if op == "sum":
        return torch.cumsum(xh.double() if name == "dense" else xh.long(), 1)
    return (torch.cummin if op == "min" else torch.cummax)(xh, 1).values


def _exclusive(incl, ident):
    return torch.cat([torch.full_like(incl[:, :1], ident), incl[:, :-1]], 1)


def _final(t, name, dtype):
    return _wrap(t) if name == "i32" and t.dtype == torch.int64 else t.to(dtype)


def _within_bound(got, ref64, terms, mag, where):
    """|got - ref64| <= (terms - 1) * 2^-24 * mag * (1 + 2^-10) for every output; remembers the worst fraction"""
    bound = (terms - 1).clamp(min=0) * 2.0 ** -24 * mag * (1 + 2.0 ** -10)
    err = (got.double() - ref64).abs()
    assert bool((err <= bound).all()), (where, float((err - bound).max()))
    frac = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    if frac > WORST["fraction"]:
        WORST["fraction"], WORST["where"] = frac, where
    return True


def _check_shape(outer, n, inner, gpu, route, chunk=None, seed=0, names=("i32", "ties", "exact", "dense")):
    data = _inputs(outer, n, inner, gpu, seed)
    for name in names:
        x, family_ops = data[name]
        before, xh = x.clone(), x.cpu()
        for op in family_ops:
            where = (route, chunk, outer, n, inner, name, op)
            ident = IDENT[op][0 if x.dtype == torch.float32 else 1]
            incl = _host_inclusive(xh, name, op)
            excl = _exclusive(incl, 0 if op == "sum" else ident)
            red = ops.reduce(x, op, dim=1, route=route, chunk=chunk)
            si = ops.scan(x, False, dim=1, op=op, route=route, chunk=chunk)
            se = ops.scan(x, True, dim=1, op=op, route=route, chunk=chunk)
            assert red.shape == (outer, inner) and si.shape == x.shape and se.shape == x.shape, where
            assert red.dtype == x.dtype and si.dtype == x.dtype and se.dtype == x.dtype, where
            if name == "dense":
                mag = torch.cumsum(xh.abs().double(), 1)
                idx = torch.arange(1, n + 1, dtype=torch.float64).view(1, n, 1).expand_as(mag)
                _within_bound(red.cpu(), incl[:, -1], idx[:, -1], mag[:, -1], where + ("reduce",))
                _within_bound(si.cpu(), incl, idx, mag, where + ("inclusive",))
                _within_bound(se.cpu(), excl, idx - 1, _exclusive(mag, 0.0), where + ("exclusive",))
            else:
                assert torch.equal(red.cpu(), _final(incl[:, -1], name, x.dtype)), where + ("reduce",)
                assert torch.equal(si.cpu(), _final(incl, name, x.dtype)), where + ("inclusive",)
                assert torch.equal(se.cpu(), _final(excl, name, x.dtype)), where + ("exclusive",)
        assert torch.equal(_bits(x), _bits(before)), (route, name, "the input was written")


def _outers(candidates, n, inner=1):
    return [o for o in candidates if o * n * inner <= MAX_ELEMS]


# ---------------------------------------------------------------- inner == 1
G_BORDERS = [4 << i for i in range(7)]  # n at which the group takes twice the lanes: 4, 8, ..., 256
GROUP_N = sorted({1, 2, 3, 4, 5, 63, 64, 65, *(b + d for b in G_BORDERS for d in (-1, 0, 1)),
                  V.AXIS_GROUP_SCAN_N - 1, V.AXIS_GROUP_SCAN_N, V.AXIS_GROUP_SCAN_N + 1, V.AXIS_GROUP_N - 1, V.AXIS_GROUP_N,
                  V.AXIS_GROUP_N + 1, V.AXIS_GROUP_MAX_N - 1, V.AXIS_GROUP_MAX_N})


@pytest.mark.parametrize("n", GROUP_N)
def test_group(gpu, n):
    for outer in _outers([1, 2, 3, 9, 257, 3001], n):
        _check_shape(outer, n, 1, gpu, "group", seed=n + outer)


BLOCK_N = sorted({1, 65, V.AXIS_GROUP_SCAN_N + 1, V.AXIS_GROUP_N + 1, 1000, 4095, 4097, V.AXIS_BLOCK_MAX_N - 1, V.AXIS_BLOCK_MAX_N})


@pytest.mark.parametrize("n", BLOCK_N)
def test_block(gpu, n):
    for outer in _outers([1, 2, 9, 257], n):
        _check_shape(outer, n, 1, gpu, "block", seed=n + outer)


@pytest.mark.parametrize("chunk,n", [(TILE, TILE + 1), (TILE, 2 * TILE), (TILE, 2 * TILE + 1), (TILE, 5 * TILE + 3),
                                     (2 * TILE, 5 * TILE + 3), (TILE, 1000), (TILE, TILE * TILE + 1),
                                     (None, V.AXIS_SPLIT_CHUNK + 1), (None, 3 * V.AXIS_SPLIT_CHUNK - 1)])
def test_split(gpu, chunk, n):
    """(1024, 1024 * 1024 + 1): more partials per row than one tile of the fold pass holds (1024)"""
    for outer in _outers([1, 3], n):
        _check_shape(outer, n, 1, gpu, "split", chunk, seed=n + outer)


# ---------------------------------------------------------------- inner > 1
INNERS = [2, 3, 4, 5, 63, 64, 65, 256, 257, 1025]


@pytest.mark.parametrize("inner", INNERS)
def test_column(gpu, inner):
    for n in (1, 2, 3, 17, 1000):
        for outer in _outers([1, 2, 5], n, inner):
            _check_shape(outer, n, inner, gpu, "column", seed=n + outer + inner)


@pytest.mark.parametrize("inner", INNERS)
def test_column_split(gpu, inner):
    c = V.AXIS_COLUMN_MIN_CHUNK
    for chunk, n in ((c, c + 1), (c, 4 * c + 3), (2 * c, 4 * c + 3), (None, 4 * c + 3), (c, 5)):
        for outer in _outers([1, 3], n, inner):
            _check_shape(outer, n, inner, gpu, "column_split", chunk, seed=n + outer + inner)


def test_column_split_fold_splits_again(gpu):
    """more partials per column than the fold takes in one launch (a scan 1024, a reduce 4096): the fold is a
    column_split of its own"""
    c = V.AXIS_COLUMN_MIN_CHUNK
    for inner in (2, 5, 64):
        _check_shape(1, 1024 * c + 1, inner, gpu, "column_split", c, seed=inner)
    _check_shape(3, 1030 * c, 4, gpu, "column_split", c, seed=9, names=("i32", "exact"))
    _check_shape(1, 4096 * c + 1, 5, gpu, "column_split", c, seed=10)
    _check_shape(2, 4100 * c, 64, gpu, "column_split", c, seed=11, names=("i32", "exact"))


# ---------------------------------------------------------------- the default rule, dims, layouts
def test_default_routes(gpu):
    for n in sorted(set(GROUP_N + BLOCK_N[2:-2])) + [V.AXIS_SPLIT_MIN_N, V.AXIS_BLOCK_MAX_N + 1]:
        for outer in _outers([3, 257], n):
            _check_shape(outer, n, 1, gpu, None, seed=n, names=("i32", "exact"))
    for inner in INNERS:
        for n in (3, V.AXIS_COLUMN_SPLIT_MIN_N - 1, V.AXIS_COLUMN_SPLIT_MIN_N, 1000):
            _check_shape(2, n, inner, gpu, None, seed=inner, names=("i32", "exact"))
    _check_shape(V.AXIS_COLUMN_MIN_UNITS // 4, 5, 16, gpu, None, names=("i32",))
    n = V.AXIS_COLUMN_SPLIT_MIN_N
    _check_shape(V.AXIS_COLUMN_MIN_BLOCKS, n, 8, gpu, None, names=("i32", "exact"))       # reduce: column at its border
    _check_shape(V.AXIS_COLUMN_MIN_BLOCKS - 1, n, 8, gpu, None, names=("i32", "exact"))   # ... and column_split below


def _torch_ref(x, op, dim):
    xh = x.cpu()
    if op == "sum":
        return xh.sum(dim, dtype=torch.int64), torch.cumsum(xh, dim, dtype=torch.int64)
    return (torch.amin if op == "min" else torch.amax)(xh, dim), (torch.cummin if op == "min" else torch.cummax)(xh, dim).values


@pytest.mark.parametrize("shape", [(5, 7, 33), (3, 4, 5, 6), (2, 1, 70, 1)])
def test_every_dim_of_3d_and_4d(gpu, shape):
    g = torch.Generator(device=gpu).manual_seed(len(shape))
    xi = torch.randint(-(1 << 31), 1 << 31, shape, device=gpu, generator=g, dtype=torch.int64).to(torch.int32)
    xf = torch.randint(-8, 9, shape, device=gpu, generator=g, dtype=torch.int64).float()
    for dim in range(-len(shape), len(shape)):
        for x in (xi, xf):
            for op in OPS:
                red, cum = _torch_ref(x, op, dim)
                if op == "sum":
                    red, cum = (_wrap(red), _wrap(cum)) if x.dtype == torch.int32 else (red.float(), cum.float())
                assert torch.equal(ops.reduce(x, op, dim).cpu(), red)
                kd = ops.reduce(x, op, dim=dim, keepdim=True)
                assert kd.shape == red.unsqueeze(dim % x.dim()).shape and torch.equal(kd.cpu().squeeze(dim % x.dim()), red)
                assert torch.equal(ops.scan(x, dim=dim, op=op).cpu(), cum)


def test_layouts_in_place_and_the_cpu_path(gpu):
    g = torch.Generator(device=gpu).manual_seed(3)
    base = torch.randint(-8, 9, (40, 2000), device=gpu, generator=g, dtype=torch.int64).float()
    for z in (base.t(), base[::3, 5:1500:2]):  # a transposed view, a strided slice with a misaligned first element
        assert not z.is_contiguous()
        zc, before = z.contiguous(), z.clone()
        for dim in (0, 1):
            for op in OPS:
                assert torch.equal(ops.reduce(z, op, dim=dim), ops.reduce(zc, op, dim=dim))
                assert torch.equal(ops.scan(z, True, dim=dim, op=op), ops.scan(zc, True, dim=dim, op=op))
                assert torch.equal(ops.reduce(z, op, dim=dim).cpu(), ops.reduce(z.cpu(), op, dim=dim))
                assert torch.equal(ops.scan(z, dim=dim, op=op).cpu(), ops.scan(z.cpu(), dim=dim, op=op))
        assert torch.equal(z, before)
    xi = torch.randint(-(1 << 31), 1 << 31, (300, 1111), device=gpu, generator=g, dtype=torch.int64).to(torch.int32)
    for x, dim, route in ((xi, 1, "block"), (xi, 1, "split"), (xi, 0, "column"), (xi, 0, "column_split"), (base, 1, "block"),
                          (base[:, :200].contiguous(), 1, "group")):
        for op in OPS:
            want = ops.scan(x.cpu(), dim=dim, op=op)   # the CPU path: equal for int32, min / max and the exact form
            assert torch.equal(ops.scan(x, dim=dim, op=op, route=route).cpu(), want)
            assert torch.equal(ops.reduce(x, op, dim=dim, route=route).cpu(), ops.reduce(x.cpu(), op, dim=dim))
            y = x.clone()
            assert ops.scan(y, dim=dim, op=op, route=route, out=y) is y and torch.equal(y.cpu(), want)  # in place
            out = torch.empty(x.numel() + 1, device=gpu, dtype=x.dtype)[1:]  # a 4-B aligned out is copied into
            assert ops.scan(x, dim=dim, op=op, route=route, out=out) is out and torch.equal(out.cpu().view(x.shape), want)
    one = torch.randint(-(1 << 31), 1 << 31, (70001,), device=gpu, generator=g, dtype=torch.int64).to(torch.int32)
    assert torch.equal(ops.scan(one, dim=0, op="max").cpu(), torch.cummax(one.cpu(), 0).values)  # a flat tensor: one row
    assert torch.equal(ops.scan(one, True, dim=0).cpu()[1:], _wrap(torch.cumsum(one.cpu().long(), 0))[:-1])
    ops.scan(one, dim=0, check=True)  # nothing of this call's to report


ROUTE_CASES = [("group", None, 1000, 1), ("block", None, 5000, 1), ("split", TILE, 5 * TILE + 3, 1),
               ("column", None, 1000, 5), ("column", None, 1000, 64), ("column_split", 16, 4 * 16 + 3, 5),
               ("column_split", 16, 4 * 16 + 3, 64), ("column_split", None, 1000, 8)]


@pytest.mark.parametrize("route,chunk,n,inner", ROUTE_CASES)
def test_same_bits_wherever_the_row_stands(gpu, route, chunk, n, inner):
    g = torch.Generator(device=gpu).manual_seed(n)
    row = torch.rand(n, device=gpu, generator=g) * 2 - 1
    results = []
    for outer in (1, 3, 257):
        for o, c in {(0, 0), (outer // 2, inner // 2), (outer - 1, inner - 1)}:
            x = torch.rand((outer, n, inner), device=gpu, generator=g) * 2 - 1
            x[o, :, c] = row
            a = (ops.reduce(x, "sum", dim=1, route=route, chunk=chunk), ops.scan(x, dim=1, route=route, chunk=chunk),
                 ops.scan(x, True, dim=1, route=route, chunk=chunk))
            b = (ops.reduce(x, "sum", dim=1, route=route, chunk=chunk), ops.scan(x, dim=1, route=route, chunk=chunk),
                 ops.scan(x, True, dim=1, route=route, chunk=chunk))
            for s, t in zip(a, b):
                assert torch.equal(_bits(s), _bits(t))  # the same forced call twice
            results.append((_bits(a[0][o, c]).item(), _bits(a[1][o, :, c]).cpu(), _bits(a[2][o, :, c]).cpu()))
    for r in results[1:]:
        assert r[0] == results[0][0] and torch.equal(r[1], results[0][1]) and torch.equal(r[2], results[0][2])


@pytest.mark.parametrize("route,chunk,n,inner", ROUTE_CASES)
def test_nan_stays_in_its_row(gpu, route, chunk, n, inner):
    g = torch.Generator(device=gpu).manual_seed(n + inner)
    clean = torch.rand((5, n, inner), device=gpu, generator=g) * 2 - 1
    o, pos, c = 2, n // 3, inner // 2
    clean[o, pos, c] = 0.0
    x = clean.clone()
    x[o, pos, c] = float("nan")
    mask = torch.ones((5, inner), dtype=torch.bool, device=gpu)
    mask[o, c] = False
    for op in OPS:
        r, rc = ops.reduce(x, op, dim=1, route=route, chunk=chunk), ops.reduce(clean, op, dim=1, route=route, chunk=chunk)
        assert bool(torch.isnan(r[o, c])) and torch.equal(_bits(r[mask]), _bits(rc[mask]))
        for exclusive in (False, True):
            s = ops.scan(x, exclusive, dim=1, op=op, route=route, chunk=chunk).movedim(1, -1)
            sc = ops.scan(clean, exclusive, dim=1, op=op, route=route, chunk=chunk).movedim(1, -1)
            first = pos + 1 if exclusive else pos
            assert bool(torch.isnan(s[o, c, first:]).all()) and not bool(torch.isnan(s[o, c, :first]).any())
            assert torch.equal(_bits(s[o, c, :first]), _bits(sc[o, c, :first]))
            assert torch.equal(_bits(s[mask]), _bits(sc[mask]))


# ---------------------------------------------------------------- the C entry points
SENTINEL = 0x5A5A5A5A
ERR_ARG = -1


def _lib():
    from parallel_c_programs_amd._native import hip_lib

    lib = hip_lib()
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    for f in (lib.pcmx_axis_reduce_f32, lib.pcmx_axis_reduce_i32):
        f.argtypes = [P, P, LL, LL, LL, I, I, LL, P, P]
    for f in (lib.pcmx_axis_scan_f32, lib.pcmx_axis_scan_i32):
        f.argtypes = [P, P, LL, LL, LL, I, I, I, LL, P, P]
    lib.pcmx_axis_workspace_bytes.argtypes = [LL, LL, LL]
    lib.pcmx_axis_workspace_bytes.restype = LL
    return lib


def test_c_abi_refusals(gpu):
    lib = _lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    x = torch.ones(4 * 100 * 8, device=gpu)
    out = torch.full((4 * 100 * 8,), SENTINEL, device=gpu, dtype=torch.int32)
    ws = torch.zeros(lib.pcmx_axis_workspace_bytes(4, 100 * 8, 8), device=gpu, dtype=torch.uint8)
    xp, op, wp = x.data_ptr(), out.data_ptr(), ws.data_ptr()
    ok = dict(x=xp, out=op, outer=4, n=100, inner=8, op=0, excl=0, route=0, chunk=0, ws=wp)

    def reduce(fn, **kw):
        a = {**ok, **kw}
        return fn(a["x"], a["out"], a["outer"], a["n"], a["inner"], a["op"], a["route"], a["chunk"], a["ws"], stream)

    def scan(fn, **kw):
        a = {**ok, **kw}
        return fn(a["x"], a["out"], a["outer"], a["n"], a["inner"], a["op"], a["excl"], a["route"], a["chunk"], a["ws"], stream)

    row = dict(n=800, inner=1)
    bad = [dict(x=None), dict(out=None), dict(x=xp + 4), dict(out=op + 4), dict(ws=wp + 4), dict(op=3), dict(op=-1),
           dict(route=6), dict(route=-1), dict(outer=-1), dict(n=-1), dict(inner=-1),
           dict(outer=1 << 11, n=1 << 10, inner=1 << 10), dict(outer=1 << 31, n=1, inner=1), dict(out=xp + 16),
           dict(route=V.AXIS_GROUP), dict(route=V.AXIS_BLOCK), dict(route=V.AXIS_SPLIT),       # inner > 1
           dict(route=V.AXIS_COLUMN, **row), dict(route=V.AXIS_COLUMN_SPLIT, **row),          # inner == 1
           dict(route=V.AXIS_GROUP, outer=1, n=V.AXIS_GROUP_MAX_N + 1, inner=1),
           dict(route=V.AXIS_BLOCK, outer=1, n=V.AXIS_BLOCK_MAX_N + 1, inner=1),
           dict(chunk=-1), dict(route=V.AXIS_COLUMN, chunk=16), dict(route=V.AXIS_COLUMN_SPLIT, chunk=15),
           dict(route=V.AXIS_SPLIT, chunk=1000, **row), dict(route=V.AXIS_BLOCK, chunk=1024, **row),
           dict(route=V.AXIS_SPLIT, ws=None, **row), dict(route=V.AXIS_COLUMN_SPLIT, ws=None)]
    for fn in (lib.pcmx_axis_reduce_f32, lib.pcmx_axis_reduce_i32):
        for kw in bad + [dict(out=xp)]:
            assert reduce(fn, **kw) == ERR_ARG, kw
        for kw in (dict(outer=0), dict(inner=0), dict(n=0, op=1), dict(n=0, op=2)):
            assert reduce(fn, **kw) == 0, kw
    for fn in (lib.pcmx_axis_scan_f32, lib.pcmx_axis_scan_i32):
        for kw in bad:
            assert scan(fn, **kw) == ERR_ARG, kw
        for kw in (dict(outer=0), dict(inner=0), dict(n=0)):
            assert scan(fn, **kw) == 0, kw
    torch.cuda.synchronize(gpu)
    assert bool((out == SENTINEL).all()) and bool((x == 1).all())  # nothing was launched
    # the accepted forms: a sum over an empty dimension fills zeros; a scan may run in place
    assert reduce(lib.pcmx_axis_reduce_f32, n=0) == 0
    assert scan(lib.pcmx_axis_scan_f32, out=xp, n=100, inner=8) == 0
    torch.cuda.synchronize(gpu)
    assert bool((out[:32] == 0).all()) and bool((out[32:] == SENTINEL).all())
    assert torch.equal(x.view(4, 100, 8)[:, :, 0].cpu(), torch.arange(1.0, 101.0).expand(4, 100))


def test_run_axis_cli(gpu):
    r = run_cli("run_axis", 300, 1000, 3, "--mode", "scan", "--op", "max", "--dtype", "i32", "--exclusive", "--steps", 2,
                "--warmup", 1, check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.endswith("Gelements/s") for ln in lines)
    assert any(ln.endswith("GB/s") for ln in lines)
    assert '"check_passed": true' in r.stdout and '"elements_checked": 900000' in r.stdout


def test_zz_worst_fraction_of_the_dense_bound(gpu):
    """Runs last in this file: prints the worst observed fraction of the dense sum's bound (it is below 1 by the
    assertions above)."""
    print(f"axis dense float32 sums: worst |error| / bound = {WORST['fraction']:.4f} at {WORST['where']}")
    assert WORST["fraction"] <= 1.0
