"""Sort inside ragged segments given by offsets on the GPU (csrc/kernels/segsort.hip) against an oracle computed on a
HOST copy: a stable torch.sort of the keys, then a stable torch.sort of the segment ids, never the op under test. Floats
are compared as bits. Every case holds at most 2^22 keys. The cases are placed by V.SEGSORT_CLASS_LIMITS (the capacity
of every length class), V.SEGSORT_MAX_LEN (longer segments take the device-wide kernels), V.SEGSORT_WAVE_CLASSES (those
classes put 4 segments into a block) and V.SEGSORT_GRID_MULT (blocks per compute unit of a class launch).

The float32 keys are multiples of 1/8 (ties in every longer segment) with the float specials of test_rowsort_cpu.py
spread over them; the int32 keys cover the full range. No test hands the kernels offsets that break the precondition:
validate=True raises before anything is launched."""
import ctypes

import pytest
import torch

from conftest import run_cli
from parallel_c_programs_amd import ops
from parallel_c_programs_amd.ops import sparse
from parallel_c_programs_amd.ops import vector as V
from parallel_c_programs_amd.ops.sparse import powerlaw_row_ptr

pytestmark = pytest.mark.gpu

LIMITS = V.SEGSORT_CLASS_LIMITS
MAX = V.SEGSORT_MAX_LEN
SENTINEL = 0x5A5A5A5A
NAN_BITS = 0x7FFFFFFF
SPECIAL = [0x7fc00000, 0x7fc00001, 0x7f800001, 0xffc12345 - (1 << 32), 0x7fffffff, 0xffffffff - (1 << 32), 0, -2**31,
           0x7f800000, 0xff800000 - (1 << 32), 1, 0x80000001 - (1 << 32), 0, -2**31]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _keys(n, dtype, seed):
    """host keys: float32 multiples of 1/8 with the specials in about one key of 16, or full-range int32"""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int32:
        return torch.randint(-(1 << 31), 1 << 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    x = torch.round(torch.randn(n, generator=g) * 8) / 8
    pick = torch.rand(n, generator=g) < 1 / 16
    sp = torch.tensor(SPECIAL, dtype=torch.int32)[torch.randint(0, len(SPECIAL), (n,), generator=g)]
    _bits(x)[pick] = sp[pick]
    return x


def _canonical(v):
    if v.dtype != torch.float32:
        return v
    v = torch.where(v == 0, torch.zeros_like(v), v)
    return torch.where(torch.isnan(v), torch.full_like(_bits(v), NAN_BITS).view(torch.float32), v)


def _oracle(xh, vh, oh, descending, nbits=32):
    """(keys, flat int32 indices, values) on the host: stable sort by key, then stable sort by segment id; the elements
    before offsets[0] and from offsets[S] on as they came"""
    n, s = xh.numel(), oh.numel() - 1
    pos = torch.arange(n)
    sid = torch.searchsorted(oh, pos, right=True)
    key = xh if nbits == 32 else xh.long() & ((1 << nbits) - 1)
    by_key = torch.sort(key, stable=True, descending=descending).indices
    order = by_key[torch.sort(sid[by_key], stable=True).indices]
    inside = (sid >= 1) & (sid <= s)
    order = torch.where(inside, order, pos)
    keys = torch.where(inside, _bits(_canonical(_bits(xh)[order].view(xh.dtype))), _bits(xh)).view(xh.dtype)
    return keys, order.int(), _bits(vh)[order].view(vh.dtype)


def _eq(got, ref, where):
    got = got.cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, where + (got.dtype, got.shape)
    same = _bits(got) == _bits(ref)
    assert bool(same.all()), where + ("first difference at", int(torch.nonzero(~same.view(-1))[0]), "of", got.numel())


def _offsets_of(lengths, lo=0):
    return torch.cat([torch.tensor([lo]), lo + torch.cumsum(torch.as_tensor(lengths, dtype=torch.int64), 0)])


def _check(gpu, n, offsets, seed=0, dtypes=(torch.float32, torch.int32), directions=(False, True), where=(), routes=True):
    """Every op and mode over the given host offsets (an int64 tensor or a list) against the host oracle; the other
    routes against the default one where they apply"""
    oh = torch.as_tensor(offsets, dtype=torch.int64)
    assert int(oh[0]) >= 0 and int(oh[-1]) <= n and bool((oh[1:] >= oh[:-1]).all()), "the test's own offsets"
    od = oh.to(torch.int32).to(gpu)
    od_before = od.clone()
    longest = int((oh[1:] - oh[:-1]).max()) if oh.numel() > 1 else 0
    for dtype in dtypes:
        xh = _keys(n, dtype, seed)
        vh = _keys(n, torch.int32 if dtype == torch.float32 else torch.float32, seed + 1)  # both payload dtypes
        x, v = xh.to(gpu), vh.to(gpu)
        x_before, v_before = x.clone(), v.clone()
        for desc in directions:
            w = where + (n, oh.numel() - 1, dtype, "descending" if desc else "ascending")
            ek, ei, ev = _oracle(xh, vh, oh, desc)
            sv, si = ops.segment_sort(x, od, desc)
            _eq(sv, ek, w + ("sort values",)), _eq(si, ei, w + ("sort indices",))
            _eq(ops.segment_sort_keys(x, od, desc), ek, w + ("keys",))
            _eq(ops.segment_argsort(x, od, desc), ei, w + ("argsort",))
            pk, pv = ops.segment_sort_by_key(x, v, od, desc)
            _eq(pk, ek, w + ("pair keys",)), _eq(pv, ev, w + ("pair values",))
            if not routes:
                continue
            gv, gi = ops.segment_sort(x, od, desc, route="global")
            assert torch.equal(_bits(gv), _bits(sv)) and torch.equal(gi, si), w + ("route global",)
            gk, gp = ops.segment_sort_by_key(x, v, od, desc, route="global")
            assert torch.equal(_bits(gk), _bits(pk)) and torch.equal(_bits(gp), _bits(pv)), w + ("route global, pairs",)
            if longest <= MAX:
                for kw in (dict(route="classes"), dict(max_len=longest), dict(max_len=MAX, route="classes")):
                    cv, ci = ops.segment_sort(x, od, desc, **kw)
                    assert torch.equal(_bits(cv), _bits(sv)) and torch.equal(ci, si), w + (kw,)
            else:
                with pytest.raises(ValueError, match="classes"):
                    ops.segment_sort(x, od, desc, route="classes")
                mv, mi = ops.segment_sort(x, od, desc, max_len=longest)
                assert torch.equal(_bits(mv), _bits(sv)) and torch.equal(mi, si), w + ("max_len",)
        assert torch.equal(_bits(x), _bits(x_before)) and torch.equal(_bits(v), _bits(v_before)), "an input was written"
    assert torch.equal(od, od_before), "the offsets were written"


def _border_lengths(extra=()):
    """0, 1, 2 and L - 1, L, L + 1 for every class limit L, shuffled, with an empty segment after every second one"""
    lens = [0, 1, 2] + [L + d for L in LIMITS for d in (-1, 0, 1) if L + d <= MAX] + list(extra)
    perm = torch.randperm(len(lens), generator=torch.Generator().manual_seed(3)).tolist()
    out = []
    for k, p in enumerate(perm):
        out.append(lens[p])
        if k % 2:
            out.append(0)
    return out


# ---------------------------------------------------------------- length classes and the long route
def test_class_borders_in_one_call(gpu):
    """Every class at its border lengths in one call, nothing above the in-CU limit: no long route"""
    lens = _border_lengths()
    oh = _offsets_of(lens)
    _check(gpu, int(oh[-1]), oh, seed=1, where=("borders",))


def test_class_borders_and_two_long_segments(gpu):
    """The same with a 16385-key and a 40000-key segment: the default route takes the long path for two segments, so the
    sort by long-segment rank runs"""
    lens = _border_lengths(extra=(MAX + 1, 40000))
    oh = _offsets_of(lens)
    _check(gpu, int(oh[-1]), oh, seed=2, where=("borders + 2 long",))


def test_exactly_one_long_segment(gpu):
    """One long segment between short ones: the sort by rank is skipped"""
    oh = _offsets_of([5, 700, MAX + 1, 0, 100, 1], lo=2)
    _check(gpu, int(oh[-1]) + 3, oh, seed=3, where=("one long",))


def test_odd_offsets_no_aligned_start(gpu):
    """offsets[0] = 1 and even lengths: every segment starts at an odd element, none at a 16-byte border"""
    g = torch.Generator().manual_seed(4)
    lens = 2 * torch.randint(0, 700, (300,), generator=g)
    lens[::50] = 2 * torch.randint(600, 4000, (6,), generator=g)  # block classes too
    oh = _offsets_of(lens, lo=1)
    assert bool((oh % 2 == 1).all())
    _check(gpu, int(oh[-1]) + 1, oh, seed=4, where=("odd offsets",))


def test_pass_through_outside_the_segments(gpu):
    """offsets[0] = 3 and offsets[S] = n - 5 with sentinel keys outside (float32: a NaN payload and a -0.0, which a sort
    would make canonical): they come back untouched, their indices are the identity"""
    n = 5000
    oh = torch.cat([torch.tensor([3]), torch.sort(torch.randint(3, n - 4, (60,), generator=torch.Generator().manual_seed(5))).values,
                    torch.tensor([n - 5])])
    od = oh.int().to(gpu)
    outside = torch.tensor([0, 1, 2, n - 5, n - 4, n - 3, n - 2, n - 1])
    for dtype, marks in ((torch.float32, [0x7fc12345, -2**31, SENTINEL]), (torch.int32, [SENTINEL, -2**31, 7])):
        xh = _keys(n, dtype, 5)
        _bits(xh)[outside] = torch.tensor((marks * 3)[:8], dtype=torch.int32)
        x = xh.to(gpu)
        for desc in (False, True):
            ek, ei, _ = _oracle(xh, xh, oh, desc)
            for route in (None, "classes", "global"):
                v, i = ops.segment_sort(x, od, desc, route=route)
                _eq(v, ek, (dtype, desc, route)), _eq(i, ei, (dtype, desc, route))
                assert torch.equal(_bits(v.cpu())[outside], _bits(xh)[outside]) and i.cpu()[outside].tolist() == outside.tolist()
                pk, pv = ops.segment_sort_by_key(x, x, od, desc, route=route)
                assert torch.equal(_bits(pv.cpu())[outside], _bits(xh)[outside])
                assert torch.equal(_bits(ops.segment_sort_keys(x, od, desc, route=route)), _bits(v))
    _check(gpu, n, oh, seed=6, where=("pass-through",))


def test_a_class_longer_than_one_round_of_its_grid(gpu):
    """40000 segments of 3 .. 70 keys (about 1.5M keys): the first class holds more segments than one round of its fixed
    grid takes, so the stride loop runs several rounds and the last one is partly empty"""
    g = torch.Generator().manual_seed(7)
    lens = torch.randint(3, 71, (40000,), generator=g)
    per_round = V.SEGSORT_GRID_MULT * torch.cuda.get_device_properties(gpu).multi_processor_count * 4
    first_class = int((lens <= LIMITS[0]).sum())
    assert first_class > 2 * per_round and first_class % per_round != 0, (first_class, per_round)
    oh = _offsets_of(lens)
    _check(gpu, int(oh[-1]), oh, seed=7, dtypes=(torch.float32,), directions=(False,), where=("grid stride",))
    _check(gpu, int(oh[-1]), oh, seed=8, dtypes=(torch.int32,), directions=(True,), where=("grid stride",), routes=False)


@pytest.mark.parametrize("s", [1, 2, 3, 5, 7])
def test_segment_counts_that_do_not_fill_a_block(gpu, s):
    """S not a multiple of the 4 segments a wave-class block takes; the same S in a block class"""
    _check(gpu, 40 * s + 2, _offsets_of([40] * s, lo=1), seed=s, where=("wave class", s))
    _check(gpu, 700 * s, _offsets_of([700] * s), seed=s, dtypes=(torch.int32,), directions=(False,), where=("block class", s))


@pytest.mark.parametrize("length", [100, MAX, MAX + 1])
def test_one_segment_covers_everything(gpu, length):
    _check(gpu, length, [0, length], seed=length, where=("one segment",))


def test_no_segments_no_keys_and_only_empty_segments(gpu):
    _check(gpu, 1000, [400], seed=9, where=("S = 0",))
    _check(gpu, 1000, [0, 0, 0, 1000, 1000], seed=10, where=("empty around one",))
    _check(gpu, 1000, [17] * 300, seed=11, where=("every segment empty",))
    _check(gpu, 1000, [0] * 5, seed=12, where=("every segment empty at 0",))
    _check(gpu, 1000, [1000] * 5, seed=13, where=("every segment empty at n",))
    o3 = torch.zeros(4, device=gpu, dtype=torch.int32)
    for dtype in (torch.float32, torch.int32):
        x0 = torch.empty(0, device=gpu, dtype=dtype)
        k = ops.segment_sort_keys(x0, o3)
        assert k.shape == (0,) and k.dtype == dtype and k.device.type == "cuda"
        v, i = ops.segment_sort(x0.view(0, 3), o3[:1])
        assert v.shape == (0, 3) and i.shape == (0, 3) and i.dtype == torch.int32
        pk, pv = ops.segment_sort_by_key(x0, x0, o3, route="global")
        assert pk.shape == (0,) and pv.dtype == dtype
    x = _keys(385, torch.float32, 14).to(gpu).view(5, 7, 11)  # any shape, read flattened; outputs have it
    oh = _offsets_of([100, 0, 200, 85])
    v, i = ops.segment_sort(x, oh.int().to(gpu))
    ek, ei, _ = _oracle(x.cpu().view(-1), x.cpu().view(-1), oh, False)
    assert v.shape == i.shape == (5, 7, 11)
    _eq(v.view(-1), ek, ("shape",)), _eq(i.view(-1), ei, ("shape",))


def test_bits_on_small_int32_keys(gpu):
    """bits=12 on int32 keys below 4096: two passes instead of four, the same result; and bits=5 on full-range keys is
    the stable sort by the low five bits"""
    lens = _border_lengths(extra=(MAX + 1, 20000))
    oh = _offsets_of(lens)
    n = int(oh[-1])
    od = oh.int().to(gpu)
    xh = _keys(n, torch.int32, 15)
    for keys_h, bits in ((xh & 0xfff, 12), (xh, 5)):
        x = keys_h.to(gpu)
        for desc in (False, True):
            ek, ei, ev = _oracle(keys_h, xh, oh, desc, bits)
            for route in (None, "global"):
                v, i = ops.segment_sort(x, od, desc, bits=bits, route=route)
                _eq(v, ek, (bits, desc, route)), _eq(i, ei, (bits, desc, route))
            pk, pv = ops.segment_sort_by_key(x, xh.to(gpu), od, desc, bits=bits)
            _eq(pk, ek, (bits, desc)), _eq(pv, ev, (bits, desc))
        if bits == 12:
            _eq(ops.segment_sort(x, od, bits=12)[1], ops.segment_sort(x, od)[1].cpu(), ("bits=12 against all bits",))


def test_float_specials_equal_the_1d_op_on_every_slice(gpu):
    """Segments dense with NaNs of every kind, signed zeros, infinities and denormals: bit equality with ops.sort and
    ops.sort_by_key applied to each slice, beside the host oracle"""
    lens = [len(SPECIAL), 1, 63, 64, 65, 0, 513, 1025, 3000, MAX + 1, 2]
    oh = _offsets_of(lens, lo=1)
    n = int(oh[-1]) + 2
    g = torch.Generator().manual_seed(16)
    xh = _keys(n, torch.float32, 16)
    dense = torch.rand(n, generator=g) < 0.5
    sp = torch.tensor(SPECIAL, dtype=torch.int32)[torch.randint(0, len(SPECIAL), (n,), generator=g)]
    _bits(xh)[dense] = sp[dense]
    _bits(xh)[1:1 + len(SPECIAL)] = torch.tensor(SPECIAL, dtype=torch.int32)
    vh = torch.arange(n, dtype=torch.int32)
    x, v, od = xh.to(gpu), vh.to(gpu), oh.int().to(gpu)
    for desc in (False, True):
        ek, ei, ev = _oracle(xh, vh, oh, desc)
        sv, si = ops.segment_sort(x, od, desc)
        pk, pv = ops.segment_sort_by_key(x, v, od, desc)
        _eq(sv, ek, (desc,)), _eq(si, ei, (desc,)), _eq(pk, ek, (desc,)), _eq(pv, ev, (desc,))
        for b, e in zip(oh[:-1].tolist(), oh[1:].tolist()):
            if e == b:
                continue
            rv, ri = ops.sort(x[b:e].clone(), desc)
            assert torch.equal(_bits(sv[b:e]), _bits(rv)) and torch.equal(si[b:e] - b, ri), (desc, b, e)
            rk, rp = ops.sort_by_key(x[b:e].clone(), v[b:e].clone(), desc)
            assert torch.equal(_bits(pk[b:e]), _bits(rk)) and torch.equal(pv[b:e], rp), (desc, b, e)


def test_powerlaw_lengths(gpu):
    rp = powerlaw_row_ptr(3000, 50000)
    _check(gpu, int(rp[-1]), rp, seed=17, where=("powerlaw",))


def test_same_bits_on_every_call(gpu):
    lens = _border_lengths(extra=(MAX + 1, 20000))
    oh = _offsets_of(lens)
    x = _keys(int(oh[-1]), torch.float32, 18).to(gpu)
    od = oh.int().to(gpu)
    first = ops.segment_sort(x, od)
    for _ in range(3):
        again = ops.segment_sort(x, od)
        assert torch.equal(_bits(again[0]), _bits(first[0])) and torch.equal(again[1], first[1])


def test_validate_and_routes_raise_before_any_result(gpu):
    x = torch.ones(100, device=gpu)
    for bad, index in (([0, 50, 40, 100], 2), ([-1, 50, 60, 100], 0), ([0, 50, 60, 101], 3)):
        with pytest.raises(ValueError, match=rf"offsets\[{index}\]"):
            ops.segment_sort(x, torch.tensor(bad, device=gpu, dtype=torch.int32), validate=True)
    good = torch.tensor([0, 50, 60, 100], device=gpu, dtype=torch.int32)
    with pytest.raises(ValueError, match="max_len = 49"):
        ops.segment_sort_keys(x, good, validate=True, max_len=49)
    assert ops.segment_sort_keys(x, good, validate=True, max_len=50).shape == (100,)
    with pytest.raises(ValueError, match="route"):
        ops.segment_sort(x, good, route="wave")
    with pytest.raises(TypeError):
        ops.segment_sort(x.double(), good)
    with pytest.raises(TypeError):
        ops.segment_sort(x, good.long())
    for xx, oo in ((x, good.cpu()), (x, good.view(4, 1)), (x, good[::2]), (x, good[:0]),
                   (torch.ones(4, 10, device=gpu)[:, ::2], good)):
        with pytest.raises(ValueError):
            ops.segment_sort(xx, oo)
    with pytest.raises(ValueError):
        ops.segment_sort_by_key(x, torch.ones(100), good)
    with pytest.raises(ValueError):
        ops.segment_sort_by_key(x, x[:99], good)


def test_sort_csr_columns(gpu):
    m = sparse.powerlaw_csr(500, 20000, seed=3)
    g = torch.Generator().manual_seed(19)
    col = m.col[torch.randperm(m.nnz, generator=g)].contiguous()  # columns out of order in every row
    c, v = sparse.sort_csr_columns(m.row_ptr.to(gpu), col.to(gpu), m.val.to(gpu))
    ec, ev = sparse.sort_csr_columns(m.row_ptr, col, m.val)
    _eq(c, ec, ("csr col",)), _eq(v, ev, ("csr val",))
    sid = torch.searchsorted(m.row_ptr, torch.arange(m.nnz), right=True)
    assert bool(((c.cpu()[1:] >= c.cpu()[:-1]) | (sid[1:] != sid[:-1])).all())


# ---------------------------------------------------------------- the C entry point
ERR_ARG = -1


def _lib():
    from parallel_c_programs_amd._native import hip_lib

    lib = hip_lib()
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    lib.pcmx_segment_sort_b32.argtypes = [P, P, P, P, LL, P, LL, I, I, I, I, I, P, P]
    lib.pcmx_segment_sort_workspace_bytes.argtypes = [LL, LL]
    lib.pcmx_segment_sort_workspace_bytes.restype = LL
    return lib


def test_c_abi_refusals(gpu):
    lib = _lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    n, s = 1000, 4
    KEYS, PAIRS, INDEX, F32 = 0, 1, 2, 2
    x = torch.arange(n, 0, -1, device=gpu).float()
    vals = torch.arange(n, device=gpu, dtype=torch.int32)
    off = torch.tensor([0, 10, 10, 500, 1000], device=gpu, dtype=torch.int32)
    ko = torch.full((n + 16,), SENTINEL, device=gpu, dtype=torch.int32)
    vo = torch.full((n + 16,), SENTINEL, device=gpu, dtype=torch.int32)
    ws_bytes = lib.pcmx_segment_sort_workspace_bytes(n, s)
    assert ws_bytes % 16 == 0 and ws_bytes >= 256 + 4 * s and lib.pcmx_segment_sort_workspace_bytes(-5, -5) >= 256
    ws = torch.full((ws_bytes // 4,), SENTINEL, device=gpu, dtype=torch.int32)
    xp, vp, fp, kp, op, wp = x.data_ptr(), vals.data_ptr(), off.data_ptr(), ko.data_ptr(), vo.data_ptr(), ws.data_ptr()
    ok = dict(ki=xp, ko=kp, vi=vp, vo=op, n=n, off=fp, s=s, kt=F32, mode=PAIRS, desc=0, b0=0, b1=32, ws=wp)

    def call(**kw):
        a = {**ok, **kw}
        return lib.pcmx_segment_sort_b32(a["ki"], a["ko"], a["vi"], a["vo"], a["n"], a["off"], a["s"], a["kt"], a["mode"],
                                         a["desc"], a["b0"], a["b1"], a["ws"], stream)

    bad = [dict(ki=None), dict(ko=None), dict(vi=None), dict(vo=None), dict(off=None), dict(ws=None),
           dict(mode=KEYS, ko=None), dict(mode=INDEX, vo=None),
           dict(ki=xp + 4), dict(ko=kp + 4), dict(vi=vp + 4), dict(vo=op + 4), dict(ws=wp + 4), dict(off=fp + 2),
           dict(ko=xp), dict(vo=xp), dict(ko=vp), dict(vo=vp), dict(vo=kp), dict(ko=fp), dict(vo=fp), dict(ws=xp), dict(ws=kp),
           dict(ws=fp), dict(kt=-1), dict(kt=3), dict(mode=-1), dict(mode=3), dict(mode=PAIRS | (65 << 8)),
           dict(b0=-1), dict(b1=33), dict(b0=8, b1=8), dict(b0=9, b1=8),
           dict(n=-1), dict(s=-1), dict(n=1 << 30), dict(s=1 << 30)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize(gpu)
    assert bool((ko == SENTINEL).all()) and bool((vo == SENTINEL).all()) and bool((ws == SENTINEL).all())  # nothing ran
    assert torch.equal(x, torch.arange(n, 0, -1, device=gpu).float()) and torch.equal(vals, torch.arange(n, device=gpu, dtype=torch.int32))
    # the accepted forms: pairs; index without keys; a 4-B aligned offsets pointer; n == 0 clears the summary only
    assert call() == 0
    torch.cuda.synchronize(gpu)
    ek, _, ev = _oracle(x.cpu(), vals.cpu(), off.cpu().long(), False)
    assert torch.equal(ko[:n].cpu(), _bits(ek)) and torch.equal(vo[:n].cpu(), ev)
    assert bool((ko[n:] == SENTINEL).all()) and bool((vo[n:] == SENTINEL).all())
    assert ws[32:36].tolist() == [0, 0, 500, 0]  # the summary: no long segment, the longest has 500 keys
    off2 = torch.tensor([9, 0, 10, 10, 500, 1000], device=gpu, dtype=torch.int32)
    vo.fill_(SENTINEL)
    assert call(mode=INDEX, ko=None, vi=None, off=off2.data_ptr() + 4) == 0
    torch.cuda.synchronize(gpu)
    assert torch.equal(vo[:n].cpu(), _oracle(x.cpu(), vals.cpu(), off.cpu().long(), False)[1]) and bool((vo[n:] == SENTINEL).all())
    ko.fill_(SENTINEL)
    assert call(n=0, mode=KEYS) == 0
    torch.cuda.synchronize(gpu)
    assert bool((ko == SENTINEL).all()) and ws[32:36].tolist() == [0, 0, 0, 0]
    # a segment above the in-CU limit is reported and left unwritten
    big = MAX + 1
    xb = torch.arange(big + 8, 0, -1, device=gpu, dtype=torch.int32)
    kb = torch.full((big + 8,), SENTINEL, device=gpu, dtype=torch.int32)
    ob = torch.tensor([0, 5, 5 + big, big + 8], device=gpu, dtype=torch.int32)
    wb = torch.zeros(lib.pcmx_segment_sort_workspace_bytes(big + 8, 3) // 4, device=gpu, dtype=torch.int32)
    assert lib.pcmx_segment_sort_b32(xb.data_ptr(), kb.data_ptr(), None, None, big + 8, ob.data_ptr(), 3, 1, KEYS, 0, 0, 32,
                                     wb.data_ptr(), stream) == 0
    torch.cuda.synchronize(gpu)
    assert wb[32:36].tolist() == [1, big, big, 0]
    assert bool((kb[5:5 + big] == SENTINEL).all())
    assert torch.equal(kb[:5], xb[:5].flip(0)) and torch.equal(kb[5 + big:], xb[5 + big:].flip(0))


def test_run_segsort_cli(gpu):
    r = run_cli("run_segsort", 200000, "--mean-len", 9, "--dist", "powerlaw", "--mode", "pairs", "--dtype", "i32",
                "--descending", "--steps", 2, "--warmup", 1, check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.endswith("Gkeys/s") for ln in lines)
    assert any(ln.endswith("GB/s") for ln in lines)
    assert '"check_passed": true' in r.stdout and '"elements_checked": 200000' in r.stdout and '"device": "cuda"' in r.stdout
