"""Merge of sorted sequences and sorted search on the MI355X (csrc/kernels/merge.hip): ops.merge_keys, ops.merge,
ops.merge_by_key, ops.searchsorted, ops.bucketize. Every comparison is torch.equal; keys are compared on their int32
view; there is no tolerance anywhere.

Oracles: the merge is the stable torch.sort of the concatenation on the GPU (its indices, and the concatenation's bits
gathered with them); the search is torch.searchsorted on the keys transformed to int64 (the transform of
csrc/kernels/radix_key.h written here with torch ops), which also covers NaN needles by the ops' rule. One exception:
torch's own GPU sort orders NaNs with the sign bit set BEFORE -inf (the vendor radix sort's bit order), unlike
torch.sort on the host, whose order (every NaN last, all NaNs tied) is the ops' order. Data that may hold such NaNs (the
float32 specials, the NaN needles) is therefore sorted, and its merge oracle computed, by the stable GPU sort of those
int64 keys, which is the host's torch.sort order.

Sizes come from the module constants: T = MERGE_TILE (outputs per block; more than 256 tiles makes the partition kernel
run a second block), S = SEARCH_LDS_KEYS (a longer sequence is sampled into LDS and finished in global memory). Sorted
inputs are made with torch.sort, never with the ops under test. No test feeds unsorted input."""
import math

import pytest
import torch

from conftest import run_cli
from parallel_c_programs_amd import ops
from parallel_c_programs_amd._native import ops as native_ops
from parallel_c_programs_amd.ops.vector import MERGE_TILE, SEARCH_LDS_KEYS

pytestmark = pytest.mark.gpu

T, S = MERGE_TILE, SEARCH_LDS_KEYS
DTYPES = [torch.float32, torch.int32]
SMALL = [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 7]
SIZE_PAIRS = [(na, nb) for na in SMALL for nb in SMALL] + [(257 * T + 13, 3), (3, 257 * T + 13), (129 * T + 5, 128 * T + 9)]
KINDS = ["ties", "a_below_b", "a_above_b", "interleaved", "all_equal", "specials"]
F32_SPECIAL_BITS = [0xff800000, 0xc0000000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x3f800000, 0x7f800000,
                    0x7fc00000, 0xffc12345, 0x7f800001, 0x7fffffff, 0xffffffff]
I32_EXTREMES = [-2**31, -2**31 + 1, -1, 0, 1, 2**31 - 2, 2**31 - 1]


def _bits(t):
    return t.view(torch.int32)


def _specials(dtype, dev):
    if dtype == torch.float32:
        return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in F32_SPECIAL_BITS], dtype=torch.int32,
                            device=dev).view(torch.float32)
    return torch.tensor(I32_EXTREMES, dtype=torch.int32, device=dev)


def _key64(x, descending):
    """radix_key.h to_key with torch ops: int64 keys whose ascending order is the ops' order"""
    b = _bits(x.reshape(-1).contiguous()).long() & 0xFFFFFFFF
    if x.dtype == torch.float32:
        mag = b & 0x7FFFFFFF
        k = torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)
        k = torch.where(mag == 0, torch.full_like(k, 0x80000000), k)
        k = torch.where(mag > 0x7F800000, torch.full_like(k, 0xFFFFFFFF), k)
    else:
        k = b ^ 0x80000000
    return 0xFFFFFFFF - k if descending else k


def _order(x, descending, nans):
    """indices of the stable sort of flat x; nans: x may hold NaNs with the sign bit set (module docstring)"""
    if nans:
        return torch.sort(_key64(x, descending), stable=True).indices
    return torch.sort(x, stable=True, descending=descending).indices


def _sorted(x, descending, nans=False):
    return _bits(x)[_order(x, descending, nans)].view(x.dtype)


def _side(kind, which, n, dtype, descending, gen, dev):
    """n sorted keys of side `which` (0 = a, 1 = b)"""
    if kind == "ties":
        x = torch.randint(0, 8, (n,), device=dev, generator=gen)
    elif kind in ("a_below_b", "a_above_b"):
        low = (which == 0) == (kind == "a_below_b")
        x = torch.randint(0, 100, (n,), device=dev, generator=gen) + (0 if low else 100)
    elif kind == "interleaved":
        x = 2 * torch.arange(n, device=dev) + which
    elif kind == "all_equal":
        x = torch.full((n,), 5, device=dev)
    else:
        sp = _specials(dtype, dev)
        return _sorted(sp[torch.randint(0, sp.numel(), (n,), device=dev, generator=gen)], descending, nans=True)
    return _sorted(x.to(dtype), descending)


def _oracle(a, b, descending, nans=False):
    cat = torch.cat([a.reshape(-1), b.reshape(-1)])
    idx = _order(cat, descending, nans)
    return _bits(cat)[idx], idx.int()


def _check_merge(a, b, descending, pairs=True, nans=False):
    keep_a, keep_b = _bits(a).clone(), _bits(b).clone()
    ref_bits, ref_idx = _oracle(a, b, descending, nans)
    only = ops.merge_keys(a, b, descending=descending)
    keys, idx = ops.merge(a, b, descending=descending)
    assert only.dtype == a.dtype and keys.dtype == a.dtype and idx.dtype == torch.int32
    assert torch.equal(_bits(only), ref_bits), "merge_keys"
    assert torch.equal(idx, ref_idx) and torch.equal(_bits(keys), ref_bits), "merge"
    if pairs:
        # values of a and b from disjoint ranges: a value names its side and its place, which shows stability
        va = torch.arange(a.numel(), device=a.device, dtype=torch.int32).reshape(a.shape)
        vb = torch.arange(b.numel(), device=a.device, dtype=torch.int32).reshape(b.shape) + a.numel()
        k2, v2 = ops.merge_by_key(a, va, b, vb, descending=descending)
        assert v2.dtype == torch.int32 and torch.equal(_bits(k2), ref_bits) and torch.equal(v2, ref_idx), "merge_by_key"
    assert torch.equal(_bits(a), keep_a) and torch.equal(_bits(b), keep_b), "inputs changed"


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_merge_sizes_and_data(gpu, kind, dtype, descending):
    g = torch.Generator(device=gpu).manual_seed(31)
    for na, nb in SIZE_PAIRS:
        a = _side(kind, 0, na, dtype, descending, g, gpu)
        b = _side(kind, 1, nb, dtype, descending, g, gpu)
        _check_merge(a, b, descending, nans=kind == "specials")


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_long_equal_run_in_the_middle(gpu, dtype, descending):
    """one run of equal keys longer than 2T in the middle of both sides: whole tiles, and whole lanes, see nothing but
    ties, and the indices show that every tie went to a"""
    g = torch.Generator(device=gpu).manual_seed(37)

    def side(n_low, n_run, n_high):
        low = torch.randint(0, 50, (n_low,), device=gpu, generator=g)
        high = torch.randint(51, 100, (n_high,), device=gpu, generator=g)
        return _sorted(torch.cat([low, torch.full((n_run,), 50, device=gpu), high]).to(dtype), descending)

    a, b = side(T + 3, 2 * T + 5, T // 2), side(T // 3, 3 * T + 1, T + 11)
    _check_merge(a, b, descending)
    _check_merge(b, a, descending)


@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_float_values_and_layouts(gpu, dtype):
    g = torch.Generator(device=gpu).manual_seed(41)
    big_a, big_b = _side("ties", 0, 3 * T + 9, dtype, False, g, gpu), _side("ties", 1, 2 * T + 2, dtype, False, g, gpu)
    for off in (1, 2, 3):
        _check_merge(big_a[off:], big_b[off + 1:], False)       # slices that start at an odd element: 4-B alignment
    _check_merge(big_a[::2], big_b[1::3], False)                # non-contiguous views of sorted data are sorted
    _check_merge(big_a[:6 * 100].view(6, 100), big_b[:T], False)  # 2-D input, flattened row-major
    # float32 values are moved as bits: NaN payloads survive
    sp = _specials(torch.float32, gpu)
    va = sp[torch.randint(0, sp.numel(), (big_a.numel(),), device=gpu, generator=g)]
    vb = sp[torch.randint(0, sp.numel(), (big_b.numel(),), device=gpu, generator=g)]
    ref_bits, ref_idx = _oracle(big_a, big_b, False)
    k, v = ops.merge_by_key(big_a, va, big_b, vb)
    assert v.dtype == torch.float32 and torch.equal(_bits(k), ref_bits)
    assert torch.equal(_bits(v), _bits(torch.cat([va, vb]))[ref_idx.long()])


@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_guards_and_repeat(gpu, dtype):
    """the torch ops take out tensors: guard elements on both ends of over-allocated outputs stay as they were, and a
    second call gives identical outputs"""
    g = torch.Generator(device=gpu).manual_seed(43)
    pcmx = native_ops()
    for na, nb in ((T + 1, 2 * T + 7), (0, 65), (63, 0), (129 * T + 5, 3)):
        a, b = _side("ties", 0, na, dtype, False, g, gpu), _side("ties", 1, nb, dtype, False, g, gpu)
        n = na + nb
        ref_bits, ref_idx = _oracle(a, b, False)
        va = torch.arange(na, device=gpu, dtype=torch.int32)
        vb = torch.arange(nb, device=gpu, dtype=torch.int32) + na

        def padded(dt):
            buf = torch.full((n + 8,), -77, device=gpu, dtype=torch.int32).view(dt)
            return buf, buf[4:4 + n]

        def guards_ok(buf):
            return bool((_bits(buf)[:4] == -77).all()) and bool((_bits(buf)[4 + n:] == -77).all())

        for _ in range(2):
            kb, kv = padded(dtype)
            assert pcmx.merge_keys(a, b, False, kv).data_ptr() == kv.data_ptr()
            assert guards_ok(kb) and torch.equal(_bits(kv), ref_bits)
            kb, kv = padded(dtype)
            ib, iv = padded(torch.int32)
            pcmx.merge_index(a, b, False, True, kv, iv)
            assert guards_ok(kb) and guards_ok(ib) and torch.equal(_bits(kv), ref_bits) and torch.equal(iv, ref_idx)
            ib, iv = padded(torch.int32)
            empty, _ = pcmx.merge_index(a, b, False, False, None, iv)  # no keys written at all
            assert empty.numel() == 0 and guards_ok(ib) and torch.equal(iv, ref_idx)
            kb, kv = padded(dtype)
            ib, iv = padded(torch.int32)
            pcmx.merge_pairs(a, va, b, vb, False, kv, iv)
            assert guards_ok(kb) and guards_ok(ib) and torch.equal(_bits(kv), ref_bits) and torch.equal(iv, ref_idx)
        # an out tensor that is not 16-byte aligned is written through a temporary
        buf = torch.full((n + 8,), -77, device=gpu, dtype=torch.int32).view(dtype)
        pcmx.merge_keys(a, b, False, buf[3:3 + n])
        assert torch.equal(_bits(buf[3:3 + n]), ref_bits) and bool((_bits(buf)[:3] == -77).all())
        assert bool((_bits(buf)[3 + n:] == -77).all())


# ---------------------------------------------------------------- sorted search
HAY_SIZES = [0, 1, 2, 63, 64, 65, S - 1, S, S + 1, 2 * S + 3, 2**20 + 5]
NEEDLE_SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 257 * T + 13]


def _search_oracle(hay, needles, right, descending):
    return torch.searchsorted(_key64(hay, descending), _key64(needles, descending), right=right).int().reshape(needles.shape)


def _haystack(kind, n, dtype, descending, gen, dev):
    """even values only (odd ones are absent); "runs": equal runs of length 3 * ceil(n / S) and of length 1 in turn, so
    that a run spans several LDS samples"""
    if kind == "all_equal":
        x = torch.full((n,), 10, device=dev)
    elif kind == "runs":
        r = 3 * max(1, math.ceil(n / S))
        groups = 2 * (n // (r + 1) + 1)
        counts = torch.tensor([r, 1], device=dev).repeat(groups // 2)
        x = 2 * torch.repeat_interleave(torch.arange(groups, device=dev), counts)[:n]
    else:
        x = 2 * torch.randint(0, max(1, n // 3), (n,), device=dev, generator=gen)
    return _sorted(x.to(dtype), descending)


def _needle_pool(hay, m, dtype, gen, dev):
    """m needles: present, absent (odd), below all, above all and, for float32, NaN of two payloads, shuffled"""
    n = hay.numel()
    picks = hay[torch.randint(0, n, (m,), device=dev, generator=gen)] if n else torch.zeros(m, device=dev, dtype=dtype)
    kind = torch.randint(0, 6, (m,), device=dev, generator=gen)
    x = torch.where(kind == 1, picks + 1, picks)
    x = torch.where(kind == 2, torch.full_like(x, -5), x)
    x = torch.where(kind == 3, torch.full_like(x, 2**24), x)
    if dtype == torch.float32:
        x = torch.where(kind == 4, torch.full_like(x, float("nan")), x)
        x = torch.where(kind == 5, torch.full_like(_bits(x), 0xffc12345 - (1 << 32)).view(torch.float32), x)
    return x


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("right", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["random", "all_equal", "runs"])
def test_searchsorted_sizes_and_data(gpu, kind, dtype, right, descending):
    g = torch.Generator(device=gpu).manual_seed(47)
    for n in HAY_SIZES:
        hay = _haystack(kind, n, dtype, descending, g, gpu)
        keep = _bits(hay).clone()
        pool = _needle_pool(hay, NEEDLE_SIZES[-1], dtype, g, gpu)
        for m in NEEDLE_SIZES:
            needles = pool[:m]
            ref = _search_oracle(hay, needles, right, descending)
            got = ops.searchsorted(hay, needles, right=right, descending=descending)
            assert got.dtype == torch.int32 and got.shape == needles.shape
            assert torch.equal(got, ref), f"n={n} m={m}"
            sn = _sorted(needles, descending, nans=True)
            by_merge = ops.searchsorted(hay, sn, right=right, descending=descending, values_sorted=True)
            general = ops.searchsorted(hay, sn, right=right, descending=descending)
            assert torch.equal(by_merge, general) and torch.equal(general, _search_oracle(hay, sn, right, descending)), \
                f"sorted needles n={n} m={m}"
        if kind == "all_equal" and n:
            same = hay[:1].expand(5).contiguous()
            assert bool((ops.searchsorted(hay, same, right=right, descending=descending) == (n if right else 0)).all())
        assert torch.equal(_bits(hay), keep)


def test_searchsorted_equals_torch_and_bucketize(gpu):
    g = torch.Generator(device=gpu).manual_seed(53)
    hay = _sorted(torch.randn(2 * S + 3, device=gpu, generator=g), False)
    vals = torch.randn(7, 11, 13, device=gpu, generator=g)
    vals[0, 0, :5] = hay[:5]
    for right in (False, True):
        ref = torch.searchsorted(hay, vals, right=right).int()
        assert torch.equal(ops.searchsorted(hay, vals, right=right), ref)
        assert torch.equal(ops.bucketize(vals, hay, right=right), torch.bucketize(vals, hay, right=right).int())
        assert torch.equal(ops.searchsorted(hay[1:], vals.transpose(0, 2), right=right),
                           torch.searchsorted(hay[1:].contiguous(), vals.transpose(0, 2).contiguous(), right=right).int())
        assert torch.equal(ops.searchsorted(hay[::2], vals, right=right),
                           torch.searchsorted(hay[::2].contiguous(), vals, right=right).int())
    # the NaN rule: a NaN ties with the NaNs at the end of the sequence, torch sends it past them
    seq = torch.tensor([-1.0, 0.0, 0.0, 2.0, 3.0, float("inf"), float("nan")], device=gpu)
    nan = torch.tensor([float("nan")], device=gpu)
    assert ops.searchsorted(seq, nan).item() == 6 and ops.searchsorted(seq, nan, right=True).item() == 7
    assert ops.searchsorted(seq, nan, values_sorted=True).item() == 6


def test_searchsorted_out_guards_and_repeat(gpu):
    g = torch.Generator(device=gpu).manual_seed(59)
    hay = _sorted(torch.randint(0, 5000, (2 * S + 3,), device=gpu, generator=g).int(), False)
    for m in (65, T + 1, 3 * T + 2):
        needles = torch.randint(-5, 5005, (m,), device=gpu, generator=g).int()
        sn = _sorted(needles, False)
        for vals, promise in ((needles, False), (sn, True)):
            ref = _search_oracle(hay, vals, False, False)
            for off in (4, 3):  # 16-byte aligned, and through a temporary
                buf = torch.full((m + 8,), -77, device=gpu, dtype=torch.int32)
                out = buf[off:off + m]
                assert ops.searchsorted(hay, vals, values_sorted=promise, out=out) is out
                assert torch.equal(out, ref) and bool((buf[:off] == -77).all()) and bool((buf[off + m:] == -77).all())
            assert torch.equal(ops.searchsorted(hay, vals, values_sorted=promise),
                               ops.searchsorted(hay, vals, values_sorted=promise))
        strided = torch.full((2 * m,), -77, device=gpu, dtype=torch.int32)
        assert torch.equal(ops.searchsorted(hay, needles, out=strided[::2]), _search_oracle(hay, needles, False, False))
        assert bool((strided[1::2] == -77).all())


def test_two_streams(gpu):
    g = torch.Generator(device=gpu).manual_seed(61)
    a1, b1 = (_side("ties", w, 20 * T + 11, torch.float32, False, g, gpu) for w in (0, 1))
    a2, b2 = (_side("interleaved", w, 9 * T + 5, torch.int32, True, g, gpu) for w in (0, 1))
    needles = torch.randint(-5, 40000, (5 * T + 3,), device=gpu, generator=g).int()
    torch.cuda.synchronize(gpu)
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s1):
        r1 = [ops.merge(a1, b1) for _ in range(3)]
        q1 = ops.searchsorted(a2, needles, descending=True)
    with torch.cuda.stream(s2):
        r2 = [ops.merge(a2, b2, descending=True) for _ in range(3)]
        q2 = ops.searchsorted(b2, _sorted(needles, True), descending=True, values_sorted=True)
    s1.synchronize(), s2.synchronize()
    for (rs, a, b, d) in ((r1, a1, b1, False), (r2, a2, b2, True)):
        ref_bits, ref_idx = _oracle(a, b, d)
        assert all(torch.equal(_bits(k), ref_bits) and torch.equal(i, ref_idx) for k, i in rs)
    assert torch.equal(q1, _search_oracle(a2, needles, False, True))
    assert torch.equal(q2, _search_oracle(b2, _sorted(needles, True), False, True))


def test_argument_errors(gpu):
    f, i = torch.zeros(8, device=gpu), torch.zeros(8, dtype=torch.int32, device=gpu)
    with pytest.raises(TypeError):
        ops.merge_keys(f, i)
    with pytest.raises(TypeError):
        ops.merge(f.double(), f.double())
    with pytest.raises(ValueError):
        ops.merge_keys(f, torch.zeros(8))  # b on the CPU
    with pytest.raises(ValueError):
        ops.merge_by_key(f, i, f, i[:7])
    with pytest.raises(ValueError):
        ops.searchsorted(f, torch.zeros(8))
    with pytest.raises(TypeError):
        ops.searchsorted(f, f, out=torch.zeros(8, device=gpu))
    with pytest.raises(ValueError):
        ops.searchsorted(f, f, out=torch.zeros(8, dtype=torch.int32))  # out on the CPU
    with pytest.raises(RuntimeError):
        native_ops().merge_keys(f, f, False, torch.zeros(15, device=gpu))  # out of the wrong size


@pytest.mark.parametrize("mode", ["keys", "pairs", "index", "search", "search_sorted"])
def test_cli(gpu, mode):
    r = run_cli("run_merge", 300000, "--mode", mode, "--dist", "interleaved", "--split", 0.3, "--steps", 2, "--warmup", 1,
                check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.startswith("elements checked : ") for ln in lines)
    assert '"check_passed": true' in r.stdout
