"""The device-wide reduce, dot and scan kernels (csrc/kernels/reduce.hip, scan.hip) against exact truths (GPU only).

Operand families, the index model of the kernels (`coverage`), the sizes where that model changes shape and the
assertion functions come from tests/_reduce_oracle.py; tests/test_reduce_oracle_cpu.py proves on the CPU that those
assertions reject thirteen single-fault mutants of the model. Every test asserts from `coverage` that the sizes it ran
reached the loop regions it names. Dense float32 data is held to bounds derived in the oracle's docstring (not
measured); the worst observed fraction of each bound is printed by the last test.

Routes: max_blocks None is ops.reduce / ops.dot (the production grid of 16384 blocks); 1, 3 and 7 are the capped C
entries pcmx_reduce_f32_grid / pcmx_reduce_i32_grid / pcmx_dot_f32_grid, which take the second and third grid-stride
trip at a few ten thousand elements."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _reduce_oracle as ro
from parallel_c_programs_amd import ops
from parallel_c_programs_amd._native import hip_lib
from parallel_c_programs_amd._native import ops as native_ops

pytestmark = pytest.mark.gpu

OP_CODES = {"sum": 0, "min": 1, "max": 2}
WORST = {"reduce": (0.0, None), "dot": (0.0, None), "scan": (0.0, None)}
TILE = ro.TILE


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    lib = hip_lib()
    lib.pcmx_reduce_workspace_bytes.restype = ctypes.c_longlong
    lib.pcmx_scan_workspace_bytes.restype = ctypes.c_longlong
    return lib


def _err_arg() -> int:
    header = Path(__file__).resolve().parents[1] / "csrc" / "include" / "pcmx_errors.h"
    return int(re.search(r"PCMX_ERR_ARG\s*=\s*(-?\d+)", header.read_text()).group(1))


def _workspace(n, dev):
    return torch.empty(max(16, _lib().pcmx_reduce_workspace_bytes(ctypes.c_longlong(n))), dtype=torch.uint8, device=dev)


def c_reduce(op, x, y, max_blocks, out=None, ws=None, n=None):
    """The capped C entry on the current stream; returns (rc, out)."""
    lib, n = _lib(), x.numel() if n is None else n
    ws = _workspace(max(n, 0), x.device) if ws is None else ws
    out = torch.full((1,), -77, dtype=x.dtype, device=x.device) if out is None else out
    if op == "dot":
        rc = lib.pcmx_dot_f32_grid(_ptr(x), _ptr(y), ctypes.c_longlong(n), _ptr(out), _ptr(ws), ctypes.c_int(max_blocks),
                                   _stream())
    else:
        fn = lib.pcmx_reduce_f32_grid if x.dtype == torch.float32 else lib.pcmx_reduce_i32_grid
        code = OP_CODES[op] if isinstance(op, str) else op
        rc = fn(_ptr(x), ctypes.c_longlong(n), ctypes.c_int(code), _ptr(out), _ptr(ws), ctypes.c_int(max_blocks), _stream())
    return rc, out


class GpuRun:
    """run(op, x, y, max_blocks) of the oracle's assertion functions on the GPU. repeat=True runs every case a second
    time and on a side stream and asserts the same bits (pass 2 folds in a fixed order)."""

    def __init__(self, dev, repeat=False):
        self.dev, self.repeat, self.cache, self.side = dev, repeat, [], torch.cuda.Stream(device=dev)

    def _to_dev(self, t):
        for src, version, d in self.cache:  # the same tensor, not written in place since it was copied
            if src is t and version == t._version:
                return d
        d = t.to(self.dev)
        self.cache = self.cache[-5:] + [(t, t._version, d)]
        return d

    def _once(self, op, x, y, max_blocks):
        if max_blocks is None:
            out = ops.dot(x, y) if op == "dot" else ops.reduce(x, op)
        else:
            rc, out = c_reduce(op, x, y, max_blocks)
            assert rc == 0, (op, x.numel(), max_blocks, rc)
        return out.cpu().numpy().reshape(-1)[0]

    def __call__(self, op, x, y=None, max_blocks=None):
        xd, yd = self._to_dev(x), None if y is None else self._to_dev(y)
        got = self._once(op, xd, yd, max_blocks)
        if self.repeat:
            again = self._once(op, xd, yd, max_blocks)
            self.side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.side):
                aside = self._once(op, xd, yd, max_blocks)
            nd = np.float32 if x.dtype == torch.float32 else np.int32
            assert ro.same_bits(got, again, nd) and ro.same_bits(got, aside, nd), ("not reproducible", op, x.numel(), max_blocks)
        return got


# ------------------------------------------------------------------------------------------ reduce and dot: exact
@pytest.mark.parametrize("max_blocks", ro.ROUTES)
def test_reduce_dot_exact_families_every_interesting_size(gpu, max_blocks):
    """Sum, min, max (float32, int32) and the dot on the exact and weighted families, bit-equal to the int64 truth, at
    every size where the loop structure changes; each case twice and on a side stream with the same bits. Capped
    grids: two and three grid-stride trips, a trip that is partly clean-up; production grid: 1..9 partials and every
    np & 3, the pass-2 identity fill live."""
    cap = ro.CAP if max_blocks is None else max_blocks
    sizes = ro.interesting_n(cap)
    cs = [ro.coverage(n, cap) for n in sizes]
    assert all(c.exactly_once for c in cs)
    assert {c.n & 3 for c in cs} == {0, 1, 2, 3} and any(c.cleanup_taken for c in cs)
    if max_blocks is None:
        assert {c.nb for c in cs} >= set(range(1, 10)) and {c.np_tail for c in cs} == {0, 1, 2, 3}
        assert any(c.fill_live for c in cs)
    else:
        assert max(c.trips for c in cs) >= 3 and any(c.trips == 2 for c in cs) and max(sizes) < 400_000
        assert any(("unrolled", 1) in c.regions and ("cleanup", 1) in c.regions for c in cs)
        assert any(("unrolled", 2) in c.regions or ("cleanup", 2) in c.regions for c in cs)
    run = GpuRun(gpu, repeat=True)
    for n in sizes:
        ro.check_exact_size(run, n, max_blocks)


def _device_family(kind, n, dev):
    """The exact and the weighted family generated on the device as int32 (no 270-MB host staging)."""
    i = torch.arange(n, device=dev, dtype=torch.int32)
    if kind == "exact":
        return (i * 7 + (i >> 5)) % 17 - 8
    if kind == "partner":
        return (i * 5 + (i >> 7)) % 7 - 3
    return (1 + i % 251) * (1 - 2 * (i & 1))


def test_reduce_dot_production_grid_second_trip(gpu):
    """2^26 + 4096 * 5 + 3 elements through the production entries: the only way to run trip two of the shipped grid
    of 16384 blocks (five blocks take it, unrolled); a second size puts a sixth block partly into the clean-up loop of
    its second trip. Device-generated integer families, bit-equal to the int64 truth."""
    c = [ro.coverage_counts(n) for n in ro.BIG_N]
    assert all(k.exactly_once and k.nb == ro.CAP and k.trips == 2 for k in c)
    assert ("cleanup", 1) not in c[0].regions and c[1].regions[("cleanup", 1)] > 0 and c[0].n & 3 == 3
    full = {k: _device_family(k, max(ro.BIG_N), gpu) for k in ("exact", "weighted", "partner")}
    for n in ro.BIG_N:
        b = full["partner"][:n]
        bf = b.float()
        for kind in ("exact", "weighted"):
            xi = full[kind][:n]
            total = int(xi.sum())
            assert abs(total) < 2 ** 24 and int(xi.abs().max()) * 2 * 4096 < 2 ** 24  # a block's share: two trips
            xf = xi.float()
            for op, want in (("sum", total), ("min", int(xi.min())), ("max", int(xi.max()))):
                assert ops.reduce(xf, op).item() == want, (kind, op, n)
                assert ops.reduce(xi, op).item() == want, (kind, op, n, "int32")
            want = int((xi * b).sum())
            assert abs(want) < 2 ** 24 and int((xi * b).abs().max()) * 2 * 4096 < 2 ** 24
            assert ops.dot(xf, bf).item() == want and ops.dot(bf, xf).item() == want, (kind, n)
            del xf
    # one planted element in the second trip and one in the last vector of the first
    x = torch.zeros(ro.BIG_N[1], device=gpu)
    for p in ((1 << 26) + 5, (1 << 26) - 1, ro.BIG_N[1] - 1, (1 << 26) + 4096 * 5 + 7):
        x[p] = 1.0
        assert ops.reduce(x, "sum").item() == 1.0 and ops.reduce(x, "max").item() == 1.0, p
        x[p] = 0.0


@pytest.mark.parametrize("case", ro.PROBE_CASES)
def test_reduce_dot_probes(gpu, case):
    """One planted element at the first and last position of every loop region (one block; five blocks with a partial
    last one; capped at 7 blocks with a second trip that is partly clean-up): the sum is exactly 1, min and max are
    exactly the planted value, float32 and int32; the dot with the probe in a and then in b is exactly 3."""
    n, max_blocks = case
    c = ro.coverage(n, ro.CAP if max_blocks is None else max_blocks)
    assert c.cleanup_taken and c.tail_taken and ("unrolled", 0) in c.regions
    if max_blocks is not None:
        assert c.trips == 2 and ("unrolled", 1) in c.regions and ("cleanup", 1) in c.regions
    ro.check_probes(GpuRun(gpu), n, max_blocks)


@pytest.mark.parametrize("case", ro.SPECIAL_CASES)
def test_reduce_dot_specials(gpu, case):
    """Min and max skip a NaN in any loop region, in the tail and alone in a block, and keep its float4 neighbours;
    all-NaN gives +inf / -inf; the sum and the dot hand on NaN and inf, +inf with -inf gives NaN; a sum of -0.0 alone
    is +0.0; an int32 sum past 2^31 is the wrapped int64 sum and the CPU path's result; INT_MIN as a max input and
    INT_MAX as a min input survive."""
    n, max_blocks = case
    c = ro.coverage(n, ro.CAP if max_blocks is None else max_blocks)
    assert c.cleanup_taken and c.tail_taken and (max_blocks is None or c.trips == 2)
    ro.check_specials(GpuRun(gpu), n, max_blocks, cpu_sum=lambda xi: ops.reduce(xi, "sum").numpy())


@pytest.mark.parametrize("max_blocks", ro.ROUTES)
def test_reduce_dot_empty_gives_the_identities(gpu, max_blocks):
    """numel() == 0 launches one block and returns +0.0, +inf, -inf (0, INT_MAX, INT_MIN), bit for bit."""
    ro.check_empty(GpuRun(gpu), max_blocks)


@pytest.mark.parametrize("n,max_blocks", [(4 * 900 + 3, None), (100_003, None), (1 << 20, None), ((1 << 22) - 1, None),
                                          (86_023, 7), (36_871, 3), (34_839, 1)])
def test_reduce_dot_dense_within_the_derived_bound(gpu, n, max_blocks):
    """Full-mantissa float32 over five binades, mixed signs: |got - ref64| <= (depth 2^-24 sum|x| + 2^-24 |ref64|)
    (1 + 2^-10), depth from the model (17 on the production grid below its cap; more with trips); twice and on a side
    stream with the same bits."""
    cap = ro.CAP if max_blocks is None else max_blocks
    run = GpuRun(gpu, repeat=True)
    for seed in (2, 3):
        x, ref, mag = ro.dense_family(n, seed)
        got = float(run("sum", x, None, max_blocks))
        bound = ro.sum_bound(ro.depth(n, cap), mag, ref)
        frac = abs(got - ref) / bound
        print(f"dense sum n={n} cap={cap}: |err| / bound = {frac:.4f}")
        if frac > WORST["reduce"][0]:
            WORST["reduce"] = (frac, (n, cap))
        assert frac <= 1.0, (n, cap, got, ref, bound)
        y, _, _ = ro.dense_family(n, seed + 7)
        prod = x.double() * y.double()
        ref, mag = float(prod.sum()), float(prod.abs().sum())
        got = float(run("dot", x, y, max_blocks))
        bound = ro.sum_bound(ro.depth(n, cap, prod=True), mag, ref)
        frac = abs(got - ref) / bound
        print(f"dense dot n={n} cap={cap}: |err| / bound = {frac:.4f}")
        if frac > WORST["dot"][0]:
            WORST["dot"] = (frac, (n, cap))
        assert frac <= 1.0, (n, cap, got, ref, bound)


def test_reduce_dot_layouts(gpu):
    """A 2-D tensor, a transposed view, a [::2] slice and views starting 4, 8 and 12 bytes into an aligned buffer (the
    binding's aligned_contig copies them); for the dot every combination of aligned and misaligned operands. The
    result has the bits of the contiguous case and the input is unchanged."""
    n = 37 * 1001
    x, total = ro.weighted_family(n)
    xd = x.to(gpu)
    yd = ro.dot_partner(n).to(gpu)
    want = {op: ops.reduce(xd, op).item() for op in ro.OPS}
    assert want["sum"] == total
    views = {"2d": xd.view(37, 1001), "transposed": xd.view(1001, 37).t()}
    wide = torch.stack([xd, torch.full_like(xd, 1e6)], 1).reshape(-1)
    views["[::2]"] = wide[::2]
    for off in (1, 2, 3):
        buf = torch.full((n + 8,), 1e6, device=gpu)
        buf[off:off + n] = xd
        views[f"+{4 * off}B"] = buf[off:off + n]
        assert buf.data_ptr() % 16 == 0 and views[f"+{4 * off}B"].data_ptr() % 16 == 4 * off
    for name, v in views.items():
        before = v.clone()
        ref = v.contiguous().clone().view(-1)
        for op in ro.OPS:
            got = ops.reduce(v, op).item()
            assert got == ops.reduce(ref, op).item() == want[op], (name, op)  # exact in any order: one truth
        assert ops.reduce(v.to(torch.int32), "sum").item() == total, name
        assert torch.equal(v, before), name
    dot_want = ops.dot(xd, yd).item()
    assert dot_want == int((x.long() * yd.cpu().long()).sum())
    for oa in (0, 1, 2, 3):
        for ob in (0, 1, 2, 3):
            ba, bb = torch.zeros(n + 8, device=gpu), torch.zeros(n + 8, device=gpu)
            ba[oa:oa + n], bb[ob:ob + n] = xd, yd
            assert ops.dot(ba[oa:oa + n], bb[ob:ob + n]).item() == dot_want, (oa, ob)
            assert torch.equal(ba[oa:oa + n], xd) and torch.equal(bb[ob:ob + n], yd)
    assert ops.dot(wide[::2], yd.view(37, 1001)).item() == dot_want


def test_reduce_dot_refusals_at_the_c_entries(gpu):
    """max_blocks of 0, -1 and 16385, an unknown op, a misaligned x, y or workspace, a null workspace and n < 0 are
    PCMX_ERR_ARG (read from pcmx_errors.h) and out keeps its sentinel."""
    err = _err_arg()
    n = 4099
    buf = torch.ones(n + 4, device=gpu)
    x, xm = buf[:n], buf[1:1 + n]
    xi = torch.ones(n + 4, device=gpu, dtype=torch.int32)
    ws = _workspace(n, gpu)

    class Raw:  # a bare address where a tensor is expected
        def __init__(self, addr, like):
            self.addr, self.dtype, self.device = addr, like.dtype, like.device

        def data_ptr(self):
            return self.addr

        def numel(self):
            return n

    cases = []
    for mb in (0, -1, ro.CAP + 1):
        cases += [("sum", x, None, mb, ws, n), ("sum", xi[:n], None, mb, ws, n), ("dot", x, x, mb, ws, n)]
    for op in (3, -1, 99):
        cases += [(op, x, None, 7, ws, n), (op, xi[:n], None, ro.CAP, ws, n)]
    cases += [("sum", xm, None, 7, ws, n), ("max", xi[1:1 + n], None, 7, ws, n), ("dot", xm, x, 7, ws, n),
              ("dot", x, xm, 7, ws, n), ("sum", x, None, 7, Raw(ws.data_ptr() + 8, ws), n),
              ("sum", x, None, 7, Raw(0, ws), n), ("dot", x, x, 7, Raw(0, ws), n), ("min", x, None, 7, ws, -1),
              ("dot", x, x, ro.CAP, ws, -5)]
    for op, a, b, mb, w, m in cases:
        rc, out = c_reduce(op, a, b, mb, ws=w, n=m)
        assert rc == err, (op, mb, m, rc)
        assert out.item() == -77, (op, mb, m)
    lib = _lib()  # the production entries refuse through the same checks
    out = torch.full((1,), -77.0, device=gpu)
    assert lib.pcmx_reduce_f32(_ptr(x), ctypes.c_longlong(n), 3, _ptr(out), _ptr(ws), _stream()) == err
    assert lib.pcmx_reduce_f32(_ptr(xm), ctypes.c_longlong(n), 0, _ptr(out), _ptr(ws), _stream()) == err
    assert lib.pcmx_dot_f32(_ptr(x), _ptr(xm), ctypes.c_longlong(n), _ptr(out), _ptr(ws), _stream()) == err
    assert lib.pcmx_reduce_f32(_ptr(x), ctypes.c_longlong(n), 0, _ptr(out), None, _stream()) == err
    assert out.item() == -77.0
    rc, out = c_reduce("sum", x, None, ro.CAP, ws=ws)  # and the largest cap is accepted
    assert rc == 0 and out.item() == n


# ------------------------------------------------------------------------------------------ scan
def c_scan(x, out, exclusive, init, variant):
    lib, n = _lib(), x.numel()
    ws = torch.empty(lib.pcmx_scan_workspace_bytes(ctypes.c_longlong(n)), dtype=torch.uint8, device=x.device)
    rc = lib.pcmx_scan_f32_variant(_ptr(x), _ptr(out), ctypes.c_longlong(n), int(exclusive),
                                   None if init is None else _ptr(init), _ptr(ws), None, variant, _stream())
    assert rc == 0 and lib.pcmx_scan_check(_ptr(ws), _stream()) == 0
    return out


SENTINEL = -12345.5


def _scan_every_mode(gpu, x, ref, where):
    """Inclusive and exclusive, with and without init, out of place (ops.scan, and scan_out into a buffer with 8
    sentinel elements past the end) and in place: bit-equal to the integer truth."""
    n = x.numel()
    xd = x.to(gpu)
    init = torch.tensor([3.0], device=gpu)
    for exclusive in (False, True):
        for ini in (None, init):
            want = ro.scan_truth(ref, exclusive, None if ini is None else 3.0).to(gpu)
            assert torch.equal(ops.scan(xd, exclusive=exclusive, init=ini), want), (where, n, exclusive, ini is not None)
            buf = torch.full((n + 8,), SENTINEL, device=gpu)
            native_ops().scan_out(xd, buf[:n], exclusive, ini)
            assert torch.equal(buf[:n], want) and bool((buf[n:] == SENTINEL).all()), (where, n, exclusive, "out of place")
            buf = torch.full((n + 8,), SENTINEL, device=gpu)
            buf[:n] = xd
            native_ops().scan_out(buf[:n], buf[:n], exclusive, ini)
            assert torch.equal(buf[:n], want) and bool((buf[n:] == SENTINEL).all()), (where, n, exclusive, "in place")
    assert torch.equal(xd.cpu(), x)


@pytest.mark.parametrize("family", ["exact", "weighted"])
def test_scan_tile_edges_every_mode(gpu, family):
    """n = 32768 k + r, k in 0, 1, 2, 5 and r in 1..5, 32765..32767 and 0: the straddling last f32x4 row of load_tile
    and store_row (r % 4 != 0), a last tile of one row, full tiles. The weighted family catches a row written at the
    wrong offset, which small integers alone can hide."""
    sizes = ro.scan_sizes()
    assert {n % TILE for n in sizes} == {0, 1, 2, 3, 4, 5, TILE - 3, TILE - 2, TILE - 1}
    assert {(n - 1) // TILE for n in sizes} >= {0, 1, 2, 5} and len(sizes) == 35
    fam = ro.scan_exact_family if family == "exact" else ro.scan_weighted_family
    for n in sizes:
        x, ref = fam(n)
        _scan_every_mode(gpu, x, ref, family)
    ops.scan_check(gpu)


def test_scan_more_tiles_than_compute_units(gpu):
    """The number of CUs plus 3 tiles: every persistent block owns one tile and three take a second ticket."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n = (cus + 3) * TILE
    for fam in (ro.scan_exact_family, ro.scan_weighted_family):
        x, ref = fam(n)
        xd = x.to(gpu)
        for exclusive in (False, True):
            assert torch.equal(ops.scan(xd, exclusive=exclusive), ro.scan_truth(ref, exclusive, None).to(gpu))
    ops.scan_check(gpu)


def test_scan_dense_within_the_derived_bound(gpu):
    """Full-mantissa data at 5 tiles + 3: |out_i - ref64_i| <= scan_depth(i, n) 2^-24 sum_{j<=i} |x_j| (1 + 2^-10) for
    every i (exclusive: the bound of i - 1)."""
    n = 5 * TILE + 3
    for seed in (4, 5):
        x, _, _ = ro.dense_family(n, seed)
        ref = torch.cumsum(x.double(), 0).numpy()
        bound = ro.scan_bound(x)
        for exclusive in (False, True):
            got = ops.scan(x.to(gpu), exclusive=exclusive).cpu().double().numpy()
            r, b = (np.concatenate([[0.0], ref[:-1]]), np.concatenate([[0.0], bound[:-1]])) if exclusive else (ref, bound)
            err = np.abs(got - r)
            frac = float((err[b > 0] / b[b > 0]).max())
            print(f"dense scan n={n} exclusive={exclusive}: worst |err| / bound = {frac:.4f}")
            if frac > WORST["scan"][0]:
                WORST["scan"] = (frac, (n, exclusive, int(np.argmax(err / np.maximum(b, 1e-300)))))
            assert (err <= b).all(), (exclusive, int(np.argmax(err - b)))
    ops.scan_check(gpu)


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_scan_poison_reaches_everything_after_and_nothing_before(gpu, variant):
    """A NaN, +inf or -inf at p (0, the last of tile 0, the first of tile 1, the middle of tile 3, n - 1): out[:p]
    (exclusive: out[:p + 1]) has the bits of the clean run and everything after is NaN / that inf; +inf and a later
    -inf give NaN from the second on. The value travels through the {flag, value} granule and the look-back of every
    schedule."""
    n = 5 * TILE + 3
    x, _ = ro.scan_exact_family(n)
    xd = x.to(gpu)
    nan, inf = float("nan"), float("inf")
    for exclusive in (False, True):
        clean = c_scan(xd, torch.empty_like(xd), exclusive, None, variant)
        s = 1 if exclusive else 0
        for p in (0, TILE - 1, TILE, 3 * TILE + TILE // 2 + 1, n - 1):
            for v in (nan, inf, -inf):
                y = xd.clone()
                y[p] = v
                out = c_scan(y, torch.empty_like(y), exclusive, None, variant)
                assert torch.equal(out[:p + s], clean[:p + s]), (variant, exclusive, p, v)
                rest = out[p + s:]
                assert bool(torch.isnan(rest).all() if v != v else (rest == v).all()), (variant, exclusive, p, v)
            q = min(n - 1, p + TILE + 7)
            if q > p:
                y = xd.clone()
                y[p], y[q] = inf, -inf
                out = c_scan(y, torch.empty_like(y), exclusive, None, variant)
                assert torch.equal(out[:p + s], clean[:p + s]) and bool((out[p + s:q + s] == inf).all())
                assert bool(torch.isnan(out[q + s:]).all()), (variant, exclusive, p, q)
    ops.scan_check(gpu)


def test_scan_layouts(gpu):
    """A [a, b, c] input gives the flattened scan in x's shape; a transposed view scans the logical (row-major
    flattened) order; a view 4 bytes into a buffer as input, as out of scan_out, and both: the same bits, and the
    buffer outside the view is untouched."""
    a, b, c = 7, 33, 151
    n = a * b * c
    x, ref = ro.scan_weighted_family(n)
    xd, want = x.to(gpu), ro.scan_truth(ref, False, None).to(gpu)
    out = ops.scan(xd.view(a, b, c))
    assert out.shape == (a, b, c) and torch.equal(out.view(-1), want)
    t = xd.view(b, a * c).t()  # logical order: t.reshape(-1)
    tw = torch.cumsum(t.reshape(-1).cpu().long(), 0).float().to(gpu)
    before = t.clone()
    out = ops.scan(t)
    assert out.shape == t.shape and torch.equal(out.reshape(-1), tw) and torch.equal(t, before)
    for in_off, out_off in ((1, 0), (0, 1), (1, 1), (1, 3)):
        src = torch.full((n + 8,), SENTINEL, device=gpu)
        dst = torch.full((n + 8,), SENTINEL, device=gpu)
        src[in_off:in_off + n] = xd
        vin, vout = src[in_off:in_off + n], dst[out_off:out_off + n]
        assert vin.data_ptr() % 16 == 4 * in_off and vout.data_ptr() % 16 == 4 * out_off
        for exclusive in (False, True):
            dst.fill_(SENTINEL)
            native_ops().scan_out(vin, vout, exclusive, None)
            assert torch.equal(vout, ro.scan_truth(ref, exclusive, None).to(gpu)), (in_off, out_off, exclusive)
            assert bool((dst[:out_off] == SENTINEL).all()) and bool((dst[out_off + n:] == SENTINEL).all())
            assert torch.equal(vin, xd) and bool((src[:in_off] == SENTINEL).all()) and bool((src[in_off + n:] == SENTINEL).all())
        assert torch.equal(ops.scan(vin), want)
    src = torch.full((n + 8,), SENTINEL, device=gpu)  # in place on a misaligned view
    src[1:1 + n] = xd
    native_ops().scan_out(src[1:1 + n], src[1:1 + n], False, None)
    assert torch.equal(src[1:1 + n], want) and src[0].item() == SENTINEL and bool((src[1 + n:] == SENTINEL).all())
    ops.scan_check(gpu)


def test_scan_empty_returns_empty(gpu):
    for shape in ((0,), (3, 0, 5)):
        e = torch.empty(shape, device=gpu)
        for exclusive in (False, True):
            out = ops.scan(e, exclusive=exclusive, init=torch.tensor([3.0], device=gpu))
            assert out.shape == e.shape and out.dtype == torch.float32
    ops.scan_check(gpu)


def test_zz_worst_fractions_of_the_dense_bounds(gpu):
    """Runs last in this file: prints the worst observed fraction of each derived bound (recorded in
    profiles/r22_reduce_scan_tests/README.md)."""
    for k, (frac, where) in WORST.items():
        print(f"dense float32 {k}: worst |error| / bound = {frac:.4f} at {where}")
        assert frac <= 1.0, k
