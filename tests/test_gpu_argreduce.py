"""argmin / argmax on the GPU (csrc/kernels/argreduce.hip): flat, along a dimension and over ragged segments, against
tests/_argreduce_oracle.py's first_extreme computed on a HOST copy. Everything is compared for equality: positions as
integers, values as int32 bit patterns gathered from the host copy at the expected positions.

Flat sizes come from the kernel's constants (ARG_BLOCK elements per block and grid-stride trip); the capped C entry
pcmx_arg_reduce_b32_grid at max_blocks 1, 3 and 7 takes the second and third trip and the clean-up loop at a few ten
thousand elements. `planted` puts the unique extremum at the first and last position of every loop region, so the
failing position names the region. Along a dimension every route is forced; over segments the sizes stand around the
tile of 4352 path steps. Every case holds at most 2^22 elements except the production-grid case at 2^24 + 5."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _argreduce_oracle as ao
from conftest import run_cli
from parallel_c_programs_amd import ops
from parallel_c_programs_amd._native import hip_lib
from parallel_c_programs_amd._native import ops as native_ops
from parallel_c_programs_amd.ops import vector as V

pytestmark = pytest.mark.gpu

OPS = ("max", "min")
OP_CODE = {"sum": 0, "min": 1, "max": 2}
KEY_I32, KEY_F32 = 1, 2  # PCMX_KEY_*
B = V.ARG_BLOCK          # elements per block and trip of the flat first pass
T = V.RAGGED_TILE        # path steps per block of the segment form
SENTINEL = -77


def _err_arg() -> int:
    header = Path(__file__).resolve().parents[1] / "csrc" / "include" / "pcmx_errors.h"
    return int(re.search(r"PCMX_ERR_ARG\s*=\s*(-?\d+)", header.read_text()).group(1))


def _lib():
    lib = hip_lib()
    for f in ("pcmx_arg_reduce_workspace_bytes", "pcmx_axis_arg_workspace_bytes", "pcmx_segment_arg_workspace_bytes"):
        getattr(lib, f).restype = ctypes.c_longlong
    return lib


def _ptr(t):
    return ctypes.c_void_p(None if t is None else (t if isinstance(t, int) else t.data_ptr()))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ll(v):
    return ctypes.c_longlong(v)


def key_type(t) -> int:
    return KEY_F32 if t.dtype == torch.float32 else KEY_I32


def c_flat(x, op, max_blocks, n=None, vals="new", idx="new", ws="new", xptr=None, kt=None):
    """pcmx_arg_reduce_b32_grid on the current stream: (rc, value bits tensor, index tensor)."""
    lib, n = _lib(), x.numel() if n is None else n
    if isinstance(ws, str):
        ws = torch.empty(max(16, lib.pcmx_arg_reduce_workspace_bytes(_ll(max(n, 0)))), dtype=torch.uint8, device=x.device)
    if isinstance(vals, str):
        vals = torch.full((1,), SENTINEL, dtype=torch.int32, device=x.device)
    if isinstance(idx, str):
        idx = torch.full((1,), SENTINEL, dtype=torch.int32, device=x.device)
    rc = lib.pcmx_arg_reduce_b32_grid(_ptr(x if xptr is None else xptr), _ll(n), key_type(x) if kt is None else kt,
                                      OP_CODE[op] if isinstance(op, str) else op, _ptr(vals), _ptr(idx), _ptr(ws),
                                      ctypes.c_int(max_blocks), _stream())
    return rc, vals, idx


def flat_run(x, op, max_blocks):
    """(value bits, index) as device tensors through ops.arg_reduce (max_blocks None) or the capped C entry."""
    if max_blocks is None:
        v, i = ops.arg_reduce(x, op)
        assert torch.equal(ops.argmax(x) if op == "max" else ops.argmin(x), i)
        return v.view(torch.int32).reshape(1), i.reshape(1)
    rc, v, i = c_flat(x, op, max_blocks)
    assert rc == 0
    return v, i


def blocks_of(n, max_blocks):
    return max(1, min(-(-(n >> 2) // (B // 4)), 16384 if max_blocks is None else max_blocks))


def flat_regions(n, max_blocks):
    """{position: region name}: the first and last position of every loop region of the flat first pass at size n."""
    nb, n4 = blocks_of(n, max_blocks), n >> 2
    out = {0: "first element", n - 1: "last element"}
    if n & 3:
        out[n4 * 4] = "first of the n & 3 tail"
        if n4:
            out[n4 * 4 - 1] = "last of the 16-byte part"
    chunks = -(-n4 // (B // 4))
    for c in range(chunks):
        trip, blk = divmod(c, nb)
        lo, hi = c * B, min((c + 1) * B, n4 * 4) - 1
        full = (c + 1) * B <= n4 * 4
        where = f"trip {trip} block {blk}" + ("" if full else " (partly clean-up loop)")
        out.setdefault(lo, f"first of {where}")
        out.setdefault(hi, f"last of {where}")
        if not full:  # the lanes whose four loads fit take the main loop, the others the clean-up loop, 256 quads a step
            for u in range(1, 4):
                q = lo + u * (B // 4)
                if q <= hi:
                    out.setdefault(q, f"load slot {u} of {where}")
                    out.setdefault(q - 1, f"end of load slot {u - 1} of {where}")
    return {p: r for p, r in out.items() if 0 <= p < n}


def flat_sizes(max_blocks):
    cap = 7 if max_blocks is None else max_blocks
    sizes = [1, 2, 3, 4, 5] + list(range(B - 5, B + 6)) + [2 * B + 1, cap * B + 2, cap * B + B + 3, 2 * cap * B + 1,
                                                         2 * cap * B + 2 * B + 7, cap * B + B // 2 + 3, cap * B + 5 * (B // 8) + 2]
    return sorted(set(sizes))


def dense_families(shape, op, axis, seed):
    return [("ties", ao.ties(shape, seed)), ("nans", ao.nans(shape, axis, seed + 1)), ("zeros", ao.zeros(shape, seed + 2)),
            ("i32", ao.i32(shape, seed + 3))]


def assert_flat(x_np, op, max_blocks, dev, name):
    x = torch.from_numpy(x_np).to(dev)
    v, i = flat_run(x, op, max_blocks)
    want = int(ao.first_extreme(x_np, op))
    got_i, got_v = int(i.cpu()[0]), int(v.cpu()[0])
    assert got_i == want, f"{name} n={x_np.size} op={op} max_blocks={max_blocks}: position {got_i}, expected {want}"
    assert got_v == int(ao.bits_of(x_np).reshape(-1)[want]), f"{name}: the value is not the element at {want}"
    assert np.array_equal(ao.bits_of(x), ao.bits_of(x_np)), "the input was written"


# ================================================================================================ flat
@pytest.mark.parametrize("max_blocks", [None, 1, 3, 7])
def test_flat_planted_names_the_region(gpu, max_blocks):
    reached = set()
    for n in flat_sizes(max_blocks):
        regions = flat_regions(n, max_blocks)
        reached |= {re.sub(r"\d+", "#", r) for r in regions.values()}
        for dtype in (torch.float32, torch.int32):
            for op in OPS:
                x = torch.ones(n, dtype=dtype, device=gpu)
                got = []
                for p in regions:
                    x[p] = 2 if op == "max" else 0
                    v, i = flat_run(x, op, max_blocks)
                    got.append(torch.cat([i, v]))
                    x[p] = 1
                got = torch.stack(got).cpu()
                win = np.array([2 if op == "max" else 0], dtype=np.float32 if dtype == torch.float32 else np.int32).view(np.int32)[0]
                for (p, region), (gi, gv) in zip(regions.items(), got.tolist()):
                    assert gi == p and gv == win, f"n={n} {dtype} {op} max_blocks={max_blocks}: extremum planted at {p} ({region}) " \
                                                  f"came back at {gi}"
    assert any("tail" in r for r in reached) and any("clean-up" in r for r in reached)
    if max_blocks is not None:  # the capped grids take a second and a third trip
        assert any(r.startswith("first of trip #") for r in reached)
        assert max(c // blocks_of(n, max_blocks) for n in flat_sizes(max_blocks) for c in range(-(-(n >> 2) // (B // 4)))) >= 2


@pytest.mark.parametrize("max_blocks", [None, 1, 3, 7])
def test_flat_families(gpu, max_blocks):
    for n in flat_sizes(max_blocks):
        for op in OPS:
            for dtype in (np.float32, np.int32):
                for name, x in (("flat_equal", ao.flat_equal(n, dtype, 3)), ("floor", ao.floor(n, dtype, op))):
                    assert int(ao.first_extreme(x, op)) == 0
                    assert_flat(x, op, max_blocks, gpu, name)  # a later lane, wave or block must not win the tie
            for name, x in dense_families(n, op, None, n):
                assert_flat(x, op, max_blocks, gpu, name)


def test_flat_production_grid_indices_above_2_pow_24(gpu):
    n = (1 << 24) + 5
    x = torch.zeros(n, device=gpu)
    x[n - 1] = 7.0
    for t in (x, x.int()):
        v, i = ops.arg_reduce(t, "max")
        assert int(i) == n - 1 and float(v) == 7.0  # n - 1 = 2^24 + 4 is no float32
    x[(1 << 24) + 1] = 7.0  # an equal value at a lower odd position above 2^24 must win
    for t in (x, x.int()):
        v, i = ops.arg_reduce(t, "max")
        assert int(i) == (1 << 24) + 1 and float(v) == 7.0
        assert int(ops.argmin(-t)) == (1 << 24) + 1


def test_flat_views_second_stream_and_outputs(gpu):
    n = 3 * B + 77
    base_np = ao.nans(n + 8, None, 21)
    base = torch.from_numpy(base_np).to(gpu)
    for op in OPS:
        for off in (1, 2, 3):  # not 16-byte aligned
            view = base[off:off + n]
            assert view.data_ptr() % 16 == 4 * off
            v, i = ops.arg_reduce(view, op)
            want = int(ao.first_extreme(base_np[off:off + n], op))
            assert int(i) == want and int(v.view(torch.int32)) == int(ao.bits_of(base_np)[off + want])
        strided = base[::3]
        v, i = ops.arg_reduce(strided, op)
        want = int(ao.first_extreme(base_np[::3], op))
        assert int(i) == want and int(v.view(torch.int32)) == int(ao.bits_of(base_np[::3])[want])
        m = base[:4 * 1000].view(4, 1000).t()  # the index is into the row-major flattening of the view
        assert int(ops.argmax(m) if op == "max" else ops.argmin(m)) == int(ao.first_extreme(np.ascontiguousarray(base_np[:4000].reshape(4, 1000).T), op))
    assert np.array_equal(ao.bits_of(base), ao.bits_of(base_np))
    # the same result on a second stream
    x = torch.from_numpy(ao.ties(5 * B + 3, 22)).to(gpu)
    first = ops.arg_reduce(x, "max")
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = ops.arg_reduce(x, "max")
        third = c_flat(x, "max", 3)
    side.synchronize()
    assert torch.equal(first[1], second[1]) and torch.equal(first[0], second[0]) and int(third[2]) == int(first[1])
    # one output alone: the other is not written
    rc, v, i = c_flat(x, "max", 7, vals=None)
    assert rc == 0 and v is None and int(i) == int(first[1])
    rc, v, i = c_flat(x, "max", 7, idx=None)
    assert rc == 0 and i is None and int(v) == int(first[0].view(torch.int32))


def test_c_refusals_launch_nothing(gpu):
    lib, err, st = _lib(), _err_arg(), _stream()
    n = 2 * B
    x = torch.ones(n + 4, device=gpu)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=gpu)
    flat_bad = [dict(op="sum"), dict(op=3), dict(kt=0), dict(kt=3), dict(n=-1), dict(n=1 << 31), dict(max_blocks=0),
                dict(max_blocks=16385), dict(xptr=x.data_ptr() + 4), dict(xptr=0), dict(ws=None), dict(ws=ws.data_ptr() + 8),
                dict(vals=None, idx=None)]
    for bad in flat_bad:
        kw = dict(op="max", max_blocks=7, n=n, ws=ws)
        kw.update(bad)
        rc, v, i = c_flat(x, **kw)
        torch.cuda.synchronize(gpu)
        assert rc == err, bad
        assert (v is None or int(v) == SENTINEL) and (i is None or int(i) == SENTINEL), bad
    # along a dimension
    vals = torch.full((64,), SENTINEL, dtype=torch.int32, device=gpu)
    idx = torch.full((64,), SENTINEL, dtype=torch.int32, device=gpu)

    def axis(outer=4, n=512, inner=1, kt=KEY_F32, op=2, route=0, chunk=0, xp=None, w=ws, v=vals, i=idx):
        return lib.pcmx_axis_arg_reduce_b32(_ptr(x if xp is None else xp), _ptr(v), _ptr(i), _ll(outer), _ll(n), _ll(inner), kt, op,
                                            route, _ll(chunk), _ptr(w), st)

    for bad in (dict(op=0), dict(kt=0), dict(outer=-1), dict(n=-1), dict(inner=-1), dict(n=0), dict(outer=1 << 16, n=1 << 16),
                dict(route=6), dict(route=-1), dict(chunk=-1), dict(route=V.AXIS_COLUMN), dict(outer=2, n=512, inner=2, route=V.AXIS_GROUP),
                dict(outer=1, n=4097, route=V.AXIS_GROUP), dict(route=V.AXIS_SPLIT, chunk=1000), dict(route=V.AXIS_BLOCK, chunk=1024),
                dict(outer=2, n=512, inner=2, route=V.AXIS_COLUMN_SPLIT, chunk=8), dict(route=V.AXIS_SPLIT, w=None),
                dict(xp=x.data_ptr() + 4), dict(xp=0), dict(v=None, i=None), dict(w=ws.data_ptr() + 4)):
        assert axis(**bad) == err, bad
    assert axis(outer=0) == 0 and axis(inner=0) == 0 and axis(w=None) == 0  # nothing to do; group needs no workspace
    torch.cuda.synchronize(gpu)
    assert bool((vals[4:] == SENTINEL).all()) and bool((idx[4:] == SENTINEL).all()) and idx[:4].tolist() == [0, 0, 0, 0]
    # segments
    off = torch.tensor([0, 10, 10, 500, 999], device=gpu, dtype=torch.int32)
    vals.fill_(SENTINEL), idx.fill_(SENTINEL)

    def seg(n=1000, s=4, kt=KEY_F32, op=2, xp=None, o=off, w=ws, v=vals, i=idx):
        return lib.pcmx_segment_arg_reduce_b32(_ptr(x if xp is None else xp), _ll(n), _ptr(o), _ll(s), kt, op, _ptr(v), _ptr(i),
                                               _ptr(w), st)

    for bad in (dict(op=0), dict(kt=0), dict(n=-1), dict(s=-1), dict(n=(1 << 31) - 4), dict(o=None), dict(o=off.data_ptr() + 2),
                dict(xp=0), dict(xp=x.data_ptr() + 2), dict(w=None), dict(w=ws.data_ptr() + 8), dict(v=None, i=None),
                dict(v=x), dict(i=off)):
        assert seg(**bad) == err, bad
    torch.cuda.synchronize(gpu)
    assert bool((vals == SENTINEL).all()) and bool((idx == SENTINEL).all())
    assert seg(s=0) == 0 and seg(xp=x.data_ptr() + 4, n=999) == 0  # a 4-byte aligned x is fine here
    torch.cuda.synchronize(gpu)
    assert idx[:4].tolist() == [0, -1, 10, 500] and bool((idx[4:] == SENTINEL).all())
    assert lib.pcmx_segment_arg_workspace_bytes(_ll(1000), _ll(4)) % 16 == 0 and lib.pcmx_axis_arg_workspace_bytes(_ll(-1), _ll(2), _ll(2)) >= 16


# ================================================================================================ along a dimension
def edges(n, steps, every_up_to=70):
    """Positions along a row of n: all of them for short rows, else both ends and both sides of every multiple of the
    steps (tile and chunk borders); thinned to the first and last borders of a step when there are many."""
    if n <= every_up_to:
        return list(range(n))
    out = {0, n - 1}
    for s in steps:
        ks = list(range(1, -(-n // s)))
        if len(ks) > 12:
            ks = ks[:4] + ks[len(ks) // 2:len(ks) // 2 + 2] + ks[-4:]
        for k in ks:
            out |= {k * s - 1, k * s}
    return sorted(p for p in out if 0 <= p < n)


def axis_check(x_np, op, axis, dev, route, chunk, name):
    x = torch.from_numpy(x_np).to(dev)
    v, i = ops.arg_reduce(x, op, dim=axis, route=route, chunk=chunk)
    want = ao.first_extreme(x_np, op, axis)
    assert i.dtype == torch.int32 and v.dtype == x.dtype and tuple(i.shape) == want.shape == tuple(v.shape)
    got = i.cpu().numpy()
    if not np.array_equal(got, want):
        at = tuple(int(a[0]) for a in np.nonzero(got != want))
        raise AssertionError(f"{name} shape={x_np.shape} dim={axis} op={op} route={route} chunk={chunk}: position {got[at]} at "
                             f"{at}, expected {want[at]}")
    assert np.array_equal(ao.bits_of(v), ao.gathered_bits(x_np, want, axis)), f"{name}: values are not the elements at the positions"
    assert np.array_equal(ao.bits_of(x), ao.bits_of(x_np)), "the input was written"
    return i


def axis_suite(shape, axis, dev, route, chunk, steps, seed):
    """All families for both ops on one shape, then planted extrema at `edges`."""
    n = shape[axis]
    for op in OPS:
        for dtype in (np.float32, np.int32):
            for name, x in (("flat_equal", ao.flat_equal(shape, dtype, 3)), ("floor", ao.floor(shape, dtype, op))):
                i = axis_check(x, op, axis, dev, route, chunk, name)
                assert int(i.abs().max()) == 0  # position 0 in every row and column
        for name, x in dense_families(shape, op, axis, seed):
            axis_check(x, op, axis, dev, route, chunk, name)
        for dtype in (torch.float32, torch.int32):
            x = torch.ones(shape, dtype=dtype, device=dev)
            ps, got = edges(n, steps), []
            for p in ps:
                x.select(axis, p).fill_(2 if op == "max" else 0)
                got.append(ops.arg_reduce(x, op, dim=axis, route=route, chunk=chunk)[1].reshape(-1))
                x.select(axis, p).fill_(1)
            got = torch.stack(got).cpu()
            for p, row in zip(ps, got):
                assert bool((row == p).all()), f"shape={shape} dim={axis} {dtype} {op} route={route} chunk={chunk}: the extremum " \
                                               f"planted at {p} came back at {sorted(set(row.tolist()))}"


GROUP_N = (1, 3, 4, 5, 63, 64, 65, 255, 257, 2048, 4096)
BLOCK_N = (1023, 1024, 1025, 4097, (1 << 17) + 3)
SPLIT = (((1 << 17) + 3, 1024), ((1 << 17) + 3, 32768), (3 * 1024 + 1, 1024))
COL_INNER = (2, 3, 4, 5, 255, 256, 257)
COL_N = (1, 15, 16, 17, 300)
COLSPLIT_N = (33, 1000)


def group_rows(n):
    return 37 if n <= 257 else 5  # neither fills the last wave: 64 / G rows share a wave, 4 waves a block


@pytest.mark.parametrize("n", GROUP_N)
def test_axis_group(gpu, n):
    assert n <= V.AXIS_GROUP_MAX_N
    axis_suite((group_rows(n), n), 1, gpu, "group", None, (4, 256), n)


@pytest.mark.parametrize("n", BLOCK_N)
def test_axis_block(gpu, n):
    axis_suite((3, n), 1, gpu, "block", None, (1024,), n)


@pytest.mark.parametrize("n,chunk", SPLIT)
def test_axis_split(gpu, n, chunk):
    axis_suite((2, n), 1, gpu, "split", chunk, (1024, chunk), n + chunk)


@pytest.mark.parametrize("inner", COL_INNER)
def test_axis_column(gpu, inner):
    for n in COL_N:
        axis_suite((2, n, inner), 1, gpu, "column", None, (4, 16, 64), n + inner)


@pytest.mark.parametrize("inner", COL_INNER)
def test_axis_column_split(gpu, inner):
    for n in COLSPLIT_N:
        axis_suite((2, n, inner), 1, gpu, "column_split", 16, (16,), n + inner)


def test_axis_column_split_second_level_fold(gpu):
    n = 16 * 4097 + 5  # 4098 chunks of 16: above the 4096 that one `column` launch folds
    axis_suite((1, n, 5), 1, gpu, "column_split", 16, (16, 16 * 4096), 5)
    axis_suite((n, 3), 0, gpu, "column_split", None, (1024,), 6)  # the default chunk


def test_axis_default_route_over_the_same_shapes(gpu):
    shapes = [((group_rows(n), n), 1) for n in GROUP_N] + [((3, n), 1) for n in BLOCK_N] + \
             [((2, n, inner), 1) for inner in COL_INNER for n in COL_N + COLSPLIT_N] + [((4100, 5), 0), ((1, (1 << 20) + 8), 1)]
    taken = set()
    for shape, axis in shapes:
        outer, n, inner = int(np.prod(shape[:axis])), shape[axis], int(np.prod(shape[axis + 1:]))
        taken.add(V._axis_route("reduce", outer, n, inner))  # the rule of reduce(dim=), unchanged
        for op in OPS:
            axis_check(ao.nans(shape, axis, n), op, axis, gpu, None, None, "default")
            axis_check(ao.i32(shape, n), op, axis, gpu, None, None, "default")
    assert taken == {"group", "block", "split", "column", "column_split"}


def test_axis_keepdim_negative_dim_and_views(gpu):
    x_np = ao.nans((3, 4, 67, 5), 2, 31)
    x = torch.from_numpy(x_np).to(gpu)
    for op in OPS:
        for dim in (-1, -2, -3, 0, 2):
            want = ao.first_extreme(x_np, op, dim % 4)
            v, i = ops.arg_reduce(x, op, dim=dim, keepdim=True)
            shape = list(x_np.shape)
            shape[dim % 4] = 1
            assert list(v.shape) == list(i.shape) == shape
            assert np.array_equal(i.squeeze(dim).cpu().numpy(), want)
            assert np.array_equal(ao.bits_of(v.squeeze(dim)), ao.gathered_bits(x_np, want, dim % 4))
            only = (ops.argmax if op == "max" else ops.argmin)(x, dim)
            assert np.array_equal(only.cpu().numpy(), want)
        view = x.permute(3, 0, 2, 1)[:, 1:, ::2]  # not contiguous
        view_np = np.ascontiguousarray(view.cpu().numpy())
        for dim in (0, 2, 3):
            v, i = ops.arg_reduce(view, op, dim=dim)
            want = ao.first_extreme(view_np, op, dim)
            assert np.array_equal(i.cpu().numpy(), want) and np.array_equal(ao.bits_of(v), ao.gathered_bits(view_np, want, dim))
    assert np.array_equal(ao.bits_of(x), ao.bits_of(x_np))


# ================================================================================================ segments
def seg_check(x_np, off, op, dev, name):
    x, o = torch.from_numpy(x_np).to(dev), torch.tensor(np.asarray(off), dtype=torch.int32, device=dev)
    v, i = ops.segment_arg_reduce(x, o, op)
    only = (ops.segment_argmax if op == "max" else ops.segment_argmin)(x, o)
    want_bits, want_idx = ao.segment_first_extreme(x_np, np.asarray(off), op)
    got = i.cpu().numpy()
    assert i.dtype == torch.int32 and v.dtype == x.dtype and got.shape == want_idx.shape == tuple(v.shape)
    if not np.array_equal(got, want_idx):
        j = int(np.nonzero(got != want_idx)[0][0])
        raise AssertionError(f"{name} n={x_np.size} S={len(off) - 1} op={op}: segment {j} [{off[j]}, {off[j + 1]}) gave "
                             f"{got[j]}, expected {want_idx[j]}")
    assert torch.equal(only, i) and np.array_equal(ao.bits_of(v), want_bits), name
    assert np.array_equal(ao.bits_of(x), ao.bits_of(x_np)), "the input was written"
    return got


def seg_families(n, op, seed):
    return [("ties", ao.ties(n, seed)), ("i32", ao.i32(n, seed + 1)), ("flat_equal", ao.flat_equal(n)),
            ("floor_f32", ao.floor(n, np.float32, op)), ("floor_i32", ao.floor(n, np.int32, op)), ("zeros", ao.zeros(n, seed + 2)),
            ("nans", ao.nans((n // 10 + 1, 10), 1, seed + 3).reshape(-1)[:n].copy())]


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 3 * T + 7])
def test_segments_offset_shapes_around_the_tile(gpu, n):
    for op in OPS:
        for fam, x in seg_families(n, op, n):
            for shape, off in ao.segment_offset_shapes(n).items():
                got = seg_check(x, off, op, gpu, f"{fam}-{shape}")
                if fam.startswith("floor") or fam == "flat_equal":  # a segment of identities gives its first index, not -1
                    o = np.asarray(off)
                    full = o[1:] > o[:-1]
                    assert np.array_equal(got[full], o[:-1][full]) and (got[~full] == -1).all()


@pytest.mark.parametrize("length", [1, 4, 17, 100])
def test_segments_equal_lengths(gpu, length):
    n = 3 * T + 7
    off = list(range(0, n + 1, length))
    for op in OPS:
        for fam, x in seg_families(n, op, length):
            seg_check(x, off, op, gpu, f"{fam}-equal{length}")


def test_segments_one_segment_over_five_tiles(gpu):
    lo, n = 3, 5 * T - 40
    off = [lo, n - 2]  # S = 1: the path is the elements of the segment and one end, tile borders every T elements
    m = off[1] - lo
    ps = sorted({0, 1, T // 2, m - 1, m - 2, m - T // 2} | {k * T + d for k in range(1, 5) for d in (-2, -1, 0, 1) if k * T + d < m})
    o = torch.tensor(off, dtype=torch.int32, device=gpu)
    for op in OPS:
        for dtype in (torch.float32, torch.int32):
            x = torch.ones(n, dtype=dtype, device=gpu)
            x[:lo] = 5 if op == "max" else -5  # outside the segment: never reported
            x[off[1]:] = 5 if op == "max" else -5
            got = []
            for p in ps:
                x[lo + p] = 2 if op == "max" else 0
                got.append(ops.segment_arg_reduce(x, o, op)[1])
                x[lo + p] = 1
            got = torch.cat(got).cpu().tolist()
            assert got == [lo + p for p in ps], f"{dtype} {op}: planted at {[lo + p for p in ps]}, came back at {got}"
            # all equal: the carry from an earlier tile wins the tie in the fix-up
            v, i = ops.segment_arg_reduce(x, o, op)
            assert i.tolist() == [lo] and float(v) == 1.0
        for fam, xf in seg_families(n, op, 41):
            seg_check(xf, off, op, gpu, f"{fam}-one-segment")


def test_segments_across_a_tile_border_and_empty_runs(gpu):
    # segment 1 starts in the last lane of tile 0 (path steps T - 3 .. T - 1) and ends in the first lane of tile 1
    n = T + 300
    off = [0, T - 4, T + 1, n]
    o = torch.tensor(off, dtype=torch.int32, device=gpu)
    for op in OPS:
        x = torch.ones(n, device=gpu)
        for p in range(off[1], off[2]):
            x[p] = 2 if op == "max" else 0
            assert ops.segment_arg_reduce(x, o, op)[1].tolist() == [0, p, off[2]], (op, p)
            x[p] = 1
        assert ops.segment_arg_reduce(x, o, op)[1].tolist() == [0, off[1], off[2]]
        for fam, xf in seg_families(n, op, 43):
            seg_check(xf, off, op, gpu, f"{fam}-border")
        # runs of empty segments spanning whole tiles, in front, in the middle and behind
        m = 100
        for fam, xf in seg_families(m, op, 44):
            seg_check(xf, [0] * (T + 5) + [50] * (2 * T + 3) + [m] * (T + 9), op, gpu, f"{fam}-empty-runs")
        # S = 4 n
        rng = np.random.default_rng(45)
        n4 = 2000
        off4 = np.sort(rng.integers(0, n4 + 1, size=4 * n4 + 1)).tolist()
        for fam, xf in seg_families(n4, op, 46):
            seg_check(xf, off4, op, gpu, f"{fam}-S=4n")


def test_segments_outside_elements_and_sentinel_outputs(gpu):
    n = 2 * T + 50
    off = [7, 40, 40, T + 3, 2 * T - 1, n - 9]
    s = len(off) - 1
    o = torch.tensor(off, dtype=torch.int32, device=gpu)
    for op in OPS:
        for outside in (np.float32(np.nan), np.float32(np.inf if op == "max" else -np.inf)):
            x_np = ao.ties(n, 47)
            x_np[:off[0]] = outside
            x_np[off[-1]:] = outside
            got = seg_check(x_np, off, op, gpu, "outside")
            assert ((got >= off[0]) & (got < off[-1]) | (got == -1)).all()
        # outputs one element longer than S stay intact past S
        x = torch.from_numpy(ao.ties(n, 48)).to(gpu)
        ov = torch.full((s + 1,), float(SENTINEL), device=gpu)
        oi = torch.full((s + 1,), SENTINEL, dtype=torch.int32, device=gpu)
        v, i = native_ops().segment_arg_reduce(x, o, OP_CODE[op], True, True, ov, oi)
        assert v.data_ptr() == ov.data_ptr() and i.data_ptr() == oi.data_ptr() and v.shape == i.shape == (s,)
        assert float(ov[s]) == SENTINEL and int(oi[s]) == SENTINEL
        ref = ops.segment_arg_reduce(x, o, op)
        assert torch.equal(oi[:s], ref[1]) and torch.equal(ov[:s], ref[0])


# ================================================================================================ cross-form identities
def test_cross_form_identities(gpu):
    x = torch.from_numpy(ao.ties(3 * B + 5, 51)).to(gpu)
    assert torch.equal(ops.argmax(x), ops.topk(x, 1)[1][0])
    assert torch.equal(ops.argmax(x.view(torch.int32) >> 3), ops.topk(x.view(torch.int32) >> 3, 1)[1][0])
    rows, cols = 37, 333
    for m_np in (ao.nans((rows, cols), 1, 52), ao.i32((rows, cols), 53)):
        m = torch.from_numpy(m_np).to(gpu)
        starts = torch.arange(rows + 1, dtype=torch.int32, device=gpu) * cols
        for op in OPS:
            v, i = ops.arg_reduce(m, op, dim=-1)
            sv, si = ops.segment_arg_reduce(m, starts, op)
            assert torch.equal(i, si - starts[:-1]) and torch.equal(v.view(torch.int32), sv.view(torch.int32))
    # every route of one shape gives the same positions
    a = torch.from_numpy(ao.ties((3, 4096), 54)).to(gpu)
    b = torch.from_numpy(ao.nans((2, 1000, 5), 1, 55)).to(gpu)
    for op in OPS:
        ref = ops.arg_reduce(a, op, dim=1)[1]
        for route, chunk in (("group", None), ("block", None), ("split", 1024), ("split", 2048)):
            assert torch.equal(ops.arg_reduce(a, op, dim=1, route=route, chunk=chunk)[1], ref), route
        assert torch.equal(ops.arg_reduce(a.t().contiguous(), op, dim=0)[1], ref)
        ref = ops.arg_reduce(b, op, dim=1)[1]
        for route, chunk in (("column", None), ("column_split", 16), ("column_split", 100)):
            assert torch.equal(ops.arg_reduce(b, op, dim=1, route=route, chunk=chunk)[1], ref), route
        assert torch.equal(ops.arg_reduce(b.permute(0, 2, 1).contiguous(), op, dim=2)[1], ref)


# ================================================================================================ CLI
@pytest.mark.parametrize("args,results", [
    (("4000", "--form", "flat", "--op", "min", "--dtype", "i32"), 1),
    (("300", "--form", "dim", "--outer", "12", "--inner", "3", "--op", "max", "--route", "column_split", "--chunk", "16"), 36),
    (("5000", "--form", "segments", "--mean-len", "9", "--dist", "powerlaw", "--op", "max"), 555),
])
def test_run_argreduce_cli(gpu, args, results):
    r = run_cli("run_argreduce", *args, "--steps", 2, "--warmup", 1, check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.endswith("Gelements/s") for ln in lines)
    assert '"check_passed": true' in r.stdout and f'"results": {results}' in r.stdout and '"device": "cuda"' in r.stdout
