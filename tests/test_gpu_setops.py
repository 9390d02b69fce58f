"""Set operations on sorted sequences on the MI355X (csrc/kernels/setops.hip): ops.set_compact, set_compact_by_key,
set_intersection / set_union / set_difference / set_symmetric_difference, set_op_by_key and the numpy-style forms.
Every comparison is torch.equal on int32 views against the oracle of tests/_setops_oracle.py computed with torch on the
GPU: keys, indices, values and the count; there is no tolerance anywhere.

Sorted inputs are made by the stable GPU sort of the int64 keys (the order of the ops for NaNs of either sign too: see
the docstring of tests/test_gpu_merge.py), never with the ops under test. No test feeds unsorted input.

Sizes: T = SETOP_TILE merged positions per block. The grid is {0, 1, 63, 64, 65, T-1, T, T+1, 2T+7}^2 plus
(257T+13, 3), (3, 257T+13) and (129T+5, 128T+9): 257 tiles, a second partition block, and look-backs that need more
than one 64-granule poll."""
import ctypes

import pytest
import torch

import _setops_oracle as so
from _setops_oracle import DTYPES, KINDS, OPS, SIZE_PAIRS, T, bits, capacity, set_oracle, set_oracle_all
from conftest import run_cli
from parallel_c_programs_amd import ops
from parallel_c_programs_amd._native import hip_lib, ops as native_ops
from parallel_c_programs_amd.ops.vector import SET_OP_CODES, SETOP_TILE

pytestmark = pytest.mark.gpu

EXACT = {"intersection": ops.set_intersection, "union": ops.set_union, "difference": ops.set_difference,
         "symmetric_difference": ops.set_symmetric_difference}


def _values(a, b):
    """int32 values that name every element's place in the concatenation"""
    na, nb = a.numel(), b.numel()
    return (torch.arange(na, device=a.device, dtype=torch.int32).reshape(a.shape),
            torch.arange(na, na + nb, device=a.device, dtype=torch.int32).reshape(b.shape))


def _check(a, b, descending, pairs=True, ref=None):
    """all four ops in the three modes against the oracle; the inputs must come back unchanged"""
    keep_a, keep_b = bits(a).clone(), bits(b).clone()
    ref = set_oracle_all(a, b, descending) if ref is None else ref
    va, vb = _values(a, b)
    for op in OPS:
        ref_bits, ref_idx = ref[op]
        k, cap = ref_idx.numel(), capacity(op, a.numel(), b.numel())
        keys, count = ops.set_compact(a, b, op, descending=descending)
        assert keys.dtype == a.dtype and keys.shape == (cap,) and count.dtype == torch.int64 and count.dim() == 0
        assert count.device == a.device and int(count) == k, f"{op}: count {int(count)} != {k}"
        assert torch.equal(bits(keys)[:k], ref_bits), f"{op}: keys"
        keys, idx, count = ops.set_compact(a, b, op, descending=descending, indices=True)
        assert idx.dtype == torch.int32 and idx.shape == (cap,) and int(count) == k, f"{op}: index count"
        assert torch.equal(bits(keys)[:k], ref_bits) and torch.equal(idx[:k], ref_idx), f"{op}: index"
        if pairs:
            k2, v2, c2 = ops.set_compact_by_key(a, va, b, vb, op, descending=descending)
            assert v2.dtype == torch.int32 and int(c2) == k, f"{op}: pairs count"
            assert torch.equal(bits(k2)[:k], ref_bits) and torch.equal(v2[:k], ref_idx), f"{op}: pairs"
    assert torch.equal(bits(a), keep_a) and torch.equal(bits(b), keep_b), "inputs changed"


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_sizes_and_data(gpu, kind, dtype, descending):
    assert SETOP_TILE == T
    g = torch.Generator(device=gpu).manual_seed(31)
    for na, nb in SIZE_PAIRS:
        a = so.side(kind, 0, na, dtype, descending, g, gpu)
        b = so.side(kind, 1, nb, dtype, descending, g, gpu)
        ref = set_oracle_all(a, b, descending)
        if kind == "ties" and na == nb and na >= 64:  # the grid is not trivial: every op keeps and drops something
            for op in OPS:
                assert 0 < ref[op][1].numel() < capacity(op, na, nb), (na, op)
        _check(a, b, descending, ref=ref)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_runs_across_tile_borders(gpu, dtype, descending):
    """key i // L with a different L per side: runs that end on, just before and just after a tile border and runs
    that span whole tiles, so ranks and partner counts come from other tiles"""
    na, nb = 7 * T + 3, 5 * T + 11
    for la in so.RUN_LENGTHS:
        a = so.runs_side(na, la, dtype, descending, gpu)
        for lb in so.RUN_LENGTHS:
            if lb != la:
                _check(a, so.runs_side(nb, lb, dtype, descending, gpu), descending, pairs=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_equal_exact_indices(gpu, dtype):
    na, nb = 3 * T + 5, 2 * T + 1
    a, b = torch.full((na,), 5, device=gpu).to(dtype), torch.full((nb,), 5, device=gpu).to(dtype)
    ar = lambda lo, hi: torch.arange(lo, hi, device=gpu, dtype=torch.int32)  # noqa: E731
    assert torch.equal(ops.set_intersection(a, b, return_indices=True)[1], ar(0, nb))           # 0 .. 2T
    assert torch.equal(ops.set_difference(a, b, return_indices=True)[1], ar(nb, na))            # 2T+1 .. 3T+4
    assert torch.equal(ops.set_union(a, b, return_indices=True)[1], ar(0, na))                  # nothing from b
    assert torch.equal(ops.set_symmetric_difference(a, b, return_indices=True)[1], ar(nb, na))
    # sides swapped: all of the shorter side, and the union adds the last T+4 of the longer one
    assert torch.equal(ops.set_intersection(b, a, return_indices=True)[1], ar(0, nb))
    assert ops.set_difference(b, a).numel() == 0
    assert torch.equal(ops.set_union(b, a, return_indices=True)[1], torch.cat([ar(0, nb), ar(nb + nb, nb + na)]))
    assert torch.equal(ops.set_symmetric_difference(b, a, return_indices=True)[1], ar(nb + nb, nb + na))
    _check(a, b, False)
    _check(b, a, True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_identical_and_disjoint_sides(gpu, dtype):
    g = torch.Generator(device=gpu).manual_seed(37)
    a = so.side("a_below_b", 0, 9 * T + 3, dtype, False, g, gpu)
    b = a.clone()
    # identical: every tile of difference and symmetric_difference publishes a zero aggregate
    for op in ("difference", "symmetric_difference"):
        keys, idx, count = ops.set_compact(a, b, op, indices=True)
        assert int(count) == 0
    assert torch.equal(bits(ops.set_intersection(a, b)), bits(a)) and torch.equal(bits(ops.set_union(a, b)), bits(a))
    _check(a, b, False)
    # disjoint: nothing in common, and the union is the merge
    hi = so.side("a_below_b", 1, 4 * T + 9, dtype, False, g, gpu)
    for x, y in ((a, hi), (hi, a)):
        assert ops.set_intersection(x, y).numel() == 0
        keys, idx = ops.set_union(x, y, return_indices=True)
        mk, mi = ops.merge(x, y)
        assert torch.equal(bits(keys), bits(mk)) and torch.equal(idx, mi)
        assert torch.equal(bits(ops.set_difference(x, y)), bits(x))
        _check(x, y, False)


def test_zero_signs_and_nan_payloads(gpu):
    neg, pos = torch.full((2 * T + 3,), -0.0, device=gpu), torch.zeros(T + 9, device=gpu)
    assert torch.equal(bits(ops.set_intersection(neg, pos)), bits(neg[:T + 9]))  # a's bits: -0.0
    assert torch.equal(bits(ops.set_union(neg, pos)), bits(neg))
    assert torch.equal(bits(ops.set_intersection(pos, neg)), bits(pos))
    assert torch.equal(bits(ops.set_union(pos, neg)), bits(torch.cat([pos, neg[:T - 6]])))
    _check(neg, pos, False)
    _check(neg, pos, True)
    g = torch.Generator(device=gpu).manual_seed(41)
    a, b = (so.side("specials", w, 3 * T + 1, torch.float32, False, g, gpu) for w in (0, 1))
    va = so.specials(torch.float32, gpu)[torch.randint(0, 13, (a.numel(),), device=gpu, generator=g)]
    vb = so.specials(torch.float32, gpu)[torch.randint(0, 13, (b.numel(),), device=gpu, generator=g)]
    for op in OPS:  # float32 values are moved as bits too
        ref_bits, ref_idx = set_oracle(a, b, op)
        k, v = ops.set_op_by_key(a, va, b, vb, op)
        assert v.dtype == torch.float32 and torch.equal(bits(k), ref_bits)
        assert torch.equal(bits(v), bits(torch.cat([va, vb]))[ref_idx.long()])


@pytest.mark.parametrize("dtype", DTYPES)
def test_output_buffers_keep_their_sentinel(gpu, dtype):
    """caller buffers larger than the capacity, aligned and not: everything from count on keeps the sentinel, and so
    do the guard elements in front"""
    g = torch.Generator(device=gpu).manual_seed(43)
    pcmx = native_ops()
    for na, nb in ((T + 1, 2 * T + 7), (0, 65), (63, 0), (129 * T + 5, 3)):
        a, b = so.side("ties", 0, na, dtype, False, g, gpu), so.side("ties", 1, nb, dtype, False, g, gpu)
        keep_a, keep_b = bits(a).clone(), bits(b).clone()
        ref = set_oracle_all(a, b, False)
        for op in OPS:
            ref_bits, ref_idx = ref[op]
            k, cap = ref_idx.numel(), capacity(op, na, nb)
            for off in (4, 3):  # 16-byte aligned, and through a copy
                kb = torch.full((cap + 12,), -77, device=gpu, dtype=torch.int32)
                ib = torch.full((cap + 12,), -77, device=gpu, dtype=torch.int32)
                kv, iv = kb[off:off + cap + 4].view(dtype), ib[off:off + cap + 4]
                keys, idx, count = ops.set_compact(a, b, op, indices=True, out_keys=kv, out_indices=iv)
                assert keys.data_ptr() == kv.data_ptr() and idx.data_ptr() == iv.data_ptr() and int(count) == k
                assert torch.equal(kb[off:off + k], ref_bits) and torch.equal(ib[off:off + k], ref_idx), (op, off)
                for buf in (kb, ib):
                    assert bool((buf[:off] == -77).all()) and bool((buf[off + k:] == -77).all()), (op, off)
            kb = torch.full((cap + 4,), -77, device=gpu, dtype=torch.int32)
            keys, empty, count = pcmx.set_op(a, b, SET_OP_CODES[op], False, False, kb.view(dtype), None)
            assert empty.numel() == 0 and int(count) == k and torch.equal(kb[:k], ref_bits) and bool((kb[k:] == -77).all())
        assert torch.equal(bits(a), keep_a) and torch.equal(bits(b), keep_b)


def test_repeat_streams_and_scan_check(gpu):
    g = torch.Generator(device=gpu).manual_seed(47)
    a1, b1 = (so.side("ties", w, 20 * T + 11, torch.float32, False, g, gpu) for w in (0, 1))
    a2, b2 = (so.side("specials", w, 9 * T + 5, torch.int32, True, g, gpu) for w in (0, 1))
    first = {op: ops.set_compact(a1, b1, op, indices=True) for op in OPS}
    again = {op: ops.set_compact(a1, b1, op, indices=True) for op in OPS}
    for op in OPS:  # the same bits on a second call
        k = int(first[op][2])
        assert int(again[op][2]) == k and all(torch.equal(bits(x)[:k], bits(y)[:k]) for x, y in zip(first[op][:2], again[op][:2]))
    torch.cuda.synchronize(gpu)
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s1):
        r1 = [ops.set_compact(a1, b1, op, indices=True) for op in OPS for _ in range(2)]
        ops.scan_check()
    with torch.cuda.stream(s2):
        r2 = [ops.set_compact(a2, b2, op, descending=True, indices=True) for op in OPS for _ in range(2)]
        ops.scan_check()
    s1.synchronize(), s2.synchronize()
    for rs, a, b, d in ((r1, a1, b1, False), (r2, a2, b2, True)):
        ref = set_oracle_all(a, b, d)
        for i, (keys, idx, count) in enumerate(rs):
            ref_bits, ref_idx = ref[OPS[i // 2]]
            k = ref_idx.numel()
            assert int(count) == k and torch.equal(bits(keys)[:k], ref_bits) and torch.equal(idx[:k], ref_idx)
    ops.scan_check()  # no look-back gave up


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_by_key_and_numpy_forms(gpu, dtype):
    g = torch.Generator(device=gpu).manual_seed(53)
    for na, nb in ((65, 64), (T + 1, T - 1), (5 * T + 3, 6 * T + 1)):
        a, b = so.side("ties", 0, na, dtype, False, g, gpu), so.side("ties", 1, nb, dtype, False, g, gpu)
        va, vb = _values(a, b)
        ref = set_oracle_all(a, b, False)
        for op in OPS:
            ref_bits, ref_idx = ref[op]
            got = EXACT[op](a, b)
            assert got.shape == ref_bits.shape and torch.equal(bits(got), ref_bits)
            got, gi = EXACT[op](a, b, return_indices=True)
            assert torch.equal(bits(got), ref_bits) and torch.equal(gi, ref_idx)
            k, v = ops.set_op_by_key(a, va, b, vb, op)
            assert torch.equal(bits(k), ref_bits) and torch.equal(v, ref_idx)
        # unsorted input of any shape: the sorted distinct values, by torch on int64 copies
        x = torch.randint(-na, na, (na,), device=gpu, generator=g).to(dtype)
        y = torch.randint(-nb // 2, 2 * nb, (nb,), device=gpu, generator=g).to(dtype).reshape(-1, 1)
        ux, uy = torch.unique(x.long()), torch.unique(y.long())
        in_y, in_x = torch.isin(ux, uy), torch.isin(uy, ux)
        assert torch.equal(ops.intersect1d(x, y).long(), ux[in_y])
        assert torch.equal(ops.setdiff1d(x, y).long(), ux[~in_y])
        assert torch.equal(ops.union1d(x, y).long(), torch.unique(torch.cat([ux, uy])))
        assert torch.equal(ops.setxor1d(x, y).long(), torch.sort(torch.cat([ux[~in_y], uy[~in_x]])).values)
        assert ops.intersect1d(x, y).dtype == dtype


@pytest.mark.parametrize("dtype", DTYPES)
def test_layouts(gpu, dtype):
    g = torch.Generator(device=gpu).manual_seed(59)
    big_a, big_b = so.side("ties", 0, 3 * T + 9, dtype, False, g, gpu), so.side("ties", 1, 2 * T + 2, dtype, False, g, gpu)
    for off in (1, 2, 3):
        _check(big_a[off:], big_b[off + 1:], False)           # slices that start at an odd element: 4-B alignment
    _check(big_a[::2], big_b[1::3], False)                    # non-contiguous views of sorted data are sorted
    _check(big_a[:6 * 100].view(6, 100), big_b[:T], False)    # 2-D input, flattened row-major


def test_argument_errors(gpu):
    f, i = torch.zeros(8, device=gpu), torch.zeros(8, dtype=torch.int32, device=gpu)
    with pytest.raises(TypeError):
        ops.set_union(f, i)
    with pytest.raises(TypeError):
        ops.set_intersection(f.double(), f.double())
    with pytest.raises(ValueError):
        ops.set_difference(f, torch.zeros(8))  # b on the CPU
    with pytest.raises(ValueError):
        ops.set_compact(f, f, "xor")
    with pytest.raises(ValueError):
        ops.set_compact(f, f, "union", out_keys=torch.zeros(16))  # out on the CPU
    with pytest.raises(ValueError):
        ops.set_compact(f, f, "union", out_keys=torch.zeros(15, device=gpu))  # capacity is 16
    with pytest.raises(ValueError):
        ops.set_op_by_key(f, i, f, i[:7], "union")
    with pytest.raises(RuntimeError):
        native_ops().set_op(f, f, 4, False, False, None, None)  # unknown op code
    with pytest.raises(RuntimeError):
        native_ops().set_op(f, f, 1, False, False, torch.zeros(15, device=gpu), None)  # too small


ERR_ARG = -1
KEY_F32, MODE_KEYS, MODE_PAIRS, MODE_INDEX = 2, 0, 1, 2


def test_c_abi_refusals(gpu):
    """the refusals of pcmx_set_op_b32 are pcmx_merge_b32's, with its code; a refused call launches nothing"""
    lib = hip_lib()
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    lib.pcmx_set_op_b32.argtypes = [P, P, LL, P, P, LL, P, P, P, I, I, I, I, P, LL, P, P]
    lib.pcmx_set_op_workspace_bytes.argtypes = [LL, LL]
    lib.pcmx_set_op_workspace_bytes.restype = LL
    n = 64
    a = torch.arange(n, device=gpu, dtype=torch.float32)
    b = torch.arange(n, device=gpu, dtype=torch.float32) + 32
    out = torch.full((2 * n + 4,), -7.0, device=gpu)
    aux = torch.full((2 * n + 4,), -7, device=gpu, dtype=torch.int32)
    count = torch.full((2,), -7, device=gpu, dtype=torch.int64)
    need = lib.pcmx_set_op_workspace_bytes(n, n)
    assert need >= 16 + 8 + 2 * 16 and need % 16 == 0 and lib.pcmx_set_op_workspace_bytes(-5, 0) >= 16
    ws = torch.zeros(need + 16, device=gpu, dtype=torch.uint8)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(ka=a.data_ptr(), va=None, na=n, kb=b.data_ptr(), vb=None, nb=n, ko=out.data_ptr(), ao=aux.data_ptr(),
                cnt=count.data_ptr(), op=1, mode=MODE_KEYS, kt=KEY_F32, desc=0, ws=ws.data_ptr(), wsb=need, err=None)

    def call(**kw):
        v = {**good, **kw}
        rc = lib.pcmx_set_op_b32(v["ka"], v["va"], v["na"], v["kb"], v["vb"], v["nb"], v["ko"], v["ao"], v["cnt"], v["op"],
                                 v["mode"], v["kt"], v["desc"], v["ws"], v["wsb"], v["err"], stream)
        torch.cuda.synchronize()
        return rc

    bad = [dict(na=-1), dict(nb=-1), dict(na=2**31 - 1, nb=1), dict(kt=3), dict(kt=-1), dict(mode=3), dict(mode=-1),
           dict(op=4), dict(op=-1), dict(cnt=None), dict(cnt=count.data_ptr() + 4), dict(ka=None), dict(kb=None),
           dict(ka=a.data_ptr() + 2), dict(kb=b.data_ptr() + 1), dict(ws=None), dict(ws=ws.data_ptr() + 8),
           dict(wsb=need - 1), dict(wsb=0), dict(ko=None), dict(ko=out.data_ptr() + 4), dict(ao=aux.data_ptr() + 8),
           dict(mode=MODE_INDEX, ao=None), dict(mode=MODE_PAIRS, ao=None), dict(mode=MODE_PAIRS),  # no values
           dict(mode=MODE_PAIRS, va=a.data_ptr(), vb=b.data_ptr() + 2)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    assert bool((out == -7.0).all()) and bool((aux == -7).all()) and bool((count == -7).all())
    # index mode may leave the keys out; a capacity of 0 writes the count alone
    assert call(mode=MODE_INDEX, ko=None) == 0 and int(count[0]) == n + 32 and bool((out == -7.0).all())
    assert torch.equal(aux[:n + 32], set_oracle(a, b, "union")[1]) and bool((aux[n + 32:] == -7).all())
    assert call(op=0, nb=0, kb=None) == 0 and int(count[0]) == 0 and int(count[1]) == -7
    assert call() == 0 and int(count[0]) == n + 32
    assert torch.equal(out[:n + 32], torch.arange(n + 32, device=gpu, dtype=torch.float32)) and bool((out[n + 32:] == -7.0).all())


@pytest.mark.parametrize("op,mode", [("intersection", "keys"), ("union", "index"), ("difference", "pairs"),
                                     ("symmetric_difference", "keys")])
def test_cli(gpu, op, mode):
    r = run_cli("run_setops", 300000, "--op", op, "--mode", mode, "--dist", "ties", "--split", 0.3, "--steps", 2,
                "--warmup", 1, check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.startswith("elements checked : ") for ln in lines)
    assert any(ln.startswith("elements kept : ") for ln in lines) and '"check_passed": true' in r.stdout
