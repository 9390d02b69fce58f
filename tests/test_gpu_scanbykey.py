"""Scan-by-key on the MI355X (csrc/kernels/scanbykey.hip). Oracles, all exact in int64 / fp64: the run structure is
torch.unique_consecutive on the int32 view of the keys (inv, cnt, starts = cumsum(cnt) - cnt); a sum is
c - (c - v)[starts][inv] with c = cumsum(v) (minus v for exclusive; int32 wrapped to 32 bits); min / max is a cummax over
+-v + inv * 4096 minus the offset (valid for |v| <= 1000: later runs dominate), shifted by one with the identity at the
heads for exclusive. Integer-valued float32 values with every run sum below 2^24 must scan bit-exactly; float sums on
the 2^-20 grid (k / 2^20, |k| < 2^20, n <= 2^22 + a few: the fp64 reference is exact) are held to the bound of ANY
summation order, |got - ref| <= g * sum|x| over the element's run prefix, g = (L-1)u / (1 - (L-1)u), u = 2^-24, L the
number of summands. The tile is T = 32768; sizes cover every n mod 4, the partial last tile, one and several tiles, and
more tiles than CUs (ticket reuse)."""
import math

import pytest
import torch

from conftest import run_cli
from parallel_c_programs_amd import ops

pytestmark = pytest.mark.gpu

T = 32768
SIZES = [0, 1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, T - 1, T, T + 1, 2 * T + 7, 300 * T + 13]
N_PAT = 70 * T + 5
REGIMES = {"all_equal": 0, "all_distinct": 1, "mean_1.5": 1.5, "mean_100": 100, "mean_1e5": 1e5}
IDENT = {("sum", torch.float32): 0.0, ("min", torch.float32): math.inf, ("max", torch.float32): -math.inf,
         ("sum", torch.int32): 0, ("min", torch.int32): 2**31 - 1, ("max", torch.int32): -2**31}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _geometric_ids(n, mean_run, gen, dev):
    """int64 run ids of n elements with geometric run lengths of the given mean (0: one run; 1: all distinct)."""
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev)
    p = 0.0 if mean_run == 0 else 1.0 / mean_run
    return torch.cumsum(torch.rand(n, device=dev, generator=gen) < p, 0)


class Runs:
    """The run structure of a key tensor: inv, cnt, starts, the bool head flags and the position inside the run."""

    def __init__(self, keys):
        kb = _bits(keys.reshape(-1))
        self.n = kb.numel()
        _, self.inv, self.cnt = torch.unique_consecutive(kb, return_inverse=True, return_counts=True)
        self.starts = torch.cumsum(self.cnt, 0) - self.cnt
        self.head = torch.ones(self.n, dtype=torch.bool, device=kb.device)
        self.head[1:] = self.inv[1:] != self.inv[:-1]
        self.pos = torch.arange(self.n, device=kb.device) - self.starts[self.inv] if self.n else self.inv


def _wrap(s):
    return ((s + 2**31) % 2**32) - 2**31


def _ref(runs, values, op, exclusive):
    """The oracle in int64 (int32 values, sums wrapped) or fp64 (float32 values)."""
    v = values.reshape(-1)
    acc = torch.int64 if v.dtype == torch.int32 else torch.float64
    va = v.to(acc)
    if runs.n == 0:
        return va
    if op == "sum":
        c = torch.cumsum(va, 0)
        ref = c - (c - va)[runs.starts][runs.inv]
        if exclusive:
            ref = ref - va
        return _wrap(ref) if acc == torch.int64 else ref
    assert bool((va.abs() <= 1000).all())
    sign = 1 if op == "max" else -1
    off = runs.inv.to(acc) * 4096
    ref = sign * (torch.cummax(sign * va + off, 0).values - off)
    if exclusive:
        ident = IDENT[(op, v.dtype)]
        ref = torch.cat([ref.new_full((1,), ident), ref[:-1]])
        ref[runs.head] = ident
    return ref


def _values(n, gen, dev):
    vi = torch.randint(-1000, 1000, (n,), device=dev, generator=gen, dtype=torch.int64).int()
    vf = torch.randint(0, 4, (n,), device=dev, generator=gen, dtype=torch.int64).float()  # run sums < 2^24: exact
    return vi, vf


def _check_all(keys, gen, ops_list=("sum",), runs=None):
    """scan_by_key of one key tensor (int32 values and integer-valued float32 values, inclusive and exclusive, the ops
    of ops_list) and run_positions against the oracles; returns the run structure."""
    runs = runs or Runs(keys)
    n = runs.n
    assert n * 3 < 2**24 or runs.cnt.max().item() * 3 < 2**24
    for v in _values(n, gen, keys.device):
        for op in ops_list:
            for exclusive in (False, True):
                got = ops.scan_by_key(keys, v, op, exclusive)
                assert got.dtype == v.dtype and got.shape == v.shape
                assert torch.equal(got, _ref(runs, v, op, exclusive).to(v.dtype)), (op, v.dtype, exclusive)
    pos = ops.run_positions(keys)
    assert pos.dtype == torch.int32 and pos.shape == keys.shape and torch.equal(pos.reshape(-1).long(), runs.pos)
    return runs


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, n):
    g = torch.Generator(device=gpu).manual_seed(3000 + n % 9973)
    ids = _geometric_ids(n, 3.0, g, gpu)
    _check_all(ids.int(), g)
    _check_all(ids.float(), g)  # ids < 2^24: exact, neighbouring runs stay different


@pytest.mark.parametrize("regime", list(REGIMES))
def test_run_length_regimes(gpu, regime):
    g = torch.Generator(device=gpu).manual_seed(41)
    keys = (_geometric_ids(N_PAT, REGIMES[regime], g, gpu) * 3 - 5).int()
    runs = _check_all(keys, g, ("sum", "min", "max"))
    if regime == "all_equal":
        # one run: the carry chain crosses every tile and the lead kernel rewrites every tile after the first
        assert runs.cnt.numel() == 1 and runs.pos[-1].item() == N_PAT - 1
    if regime == "all_distinct":
        assert runs.cnt.numel() == N_PAT


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
    runs = _check_all(keys, g)
    expect = {"tile_aligned": 71, "tile_aligned_plus1": 71, "tile_aligned_minus1": 72, "one_head_per_tile": 71,
              "last_element_own_run": 2, "no_head_in_last_tile": 70, "runs_4096": 70 * 8 + 1}.get(pattern)
    if expect is not None:
        assert runs.cnt.numel() == expect
    # the same runs as flags, with heads[0] = 0: element 0 starts a run whatever its flag says
    heads = runs.head.clone()
    heads[0] = False
    vi, vf = _values(N_PAT, g, gpu)
    for v, op, exclusive in ((vi, "sum", False), (vf, "sum", True), (vi, "max", True), (vf, "min", False)):
        got = ops.segmented_scan(v, heads, op, exclusive)
        assert torch.equal(got, _ref(runs, v, op, exclusive).to(v.dtype)), (op, exclusive)


def test_key_bits(gpu):
    """Float keys with both zeros, NaNs of several payloads, infinities and a denormal at run borders, and int32
    extremes: compared as bit patterns."""
    n = 3 * T + 77
    g = torch.Generator(device=gpu).manual_seed(47)
    special = torch.tensor([0, -2**31, 0x7fc00000, 0x7fc00000, 0x7fc00001, 0x7f800001, 0xffc12345 - (1 << 32), 0x7fffffff,
                            0x7f800000, 0xff800000 - (1 << 32), 1, 1, 0, 0, -2**31, -2**31],
                           dtype=torch.int32, device=gpu)
    kb = _bits(_geometric_ids(n, 3.0, g, gpu).float()).clone()
    for base in (0, 4090, T - 8, 2 * T - 3, n - special.numel()):  # lane, row, wave and tile borders, both ends
        kb[base:base + special.numel()] = special
    keys = kb.view(torch.float32)
    _check_all(keys, g)
    assert ops.run_positions(keys[:5]).tolist() == [0, 0, 0, 1, 0]  # 0.0 | -0.0 | nan nan | nan'
    ki = _geometric_ids(n, 3.0, g, gpu).int()
    ki[:6] = torch.tensor([-2**31, -2**31, 2**31 - 1, 2**31 - 1, 0, -1], dtype=torch.int32, device=gpu)
    ki[T - 1], ki[T] = 2**31 - 1, -2**31
    _check_all(ki, g)


def test_int32_extremes_wrap_and_exclusive_identities(gpu):
    n = 5 * T + 3
    g = torch.Generator(device=gpu).manual_seed(53)
    keys = _geometric_ids(n, 40.0, g, gpu).int()
    runs = Runs(keys)
    vi = torch.randint(-2**31, 2**31 - 1, (n,), device=gpu, generator=g, dtype=torch.int64).int()  # sums wrap
    c = torch.cumsum(vi.long(), 0)
    exact = c - (c - vi.long())[runs.starts][runs.inv]
    assert bool((exact.abs() >= 2**31).any())  # the test does wrap
    for exclusive in (False, True):
        assert torch.equal(ops.scan_by_key(keys, vi, "sum", exclusive).long(), _ref(runs, vi, "sum", exclusive))
    vf = torch.randint(-1000, 1000, (n,), device=gpu, generator=g, dtype=torch.int64).float()
    vf[runs.starts] = -0.0
    for op in ("sum", "min", "max"):
        for v in (vf, vf.int()):
            got = ops.scan_by_key(keys, v, op, True)
            ident = torch.full((1,), IDENT[(op, v.dtype)], dtype=v.dtype, device=gpu)
            assert bool((_bits(got[runs.head]) == _bits(ident)).all()), (op, v.dtype)  # +0.0 for a float sum


@pytest.mark.parametrize("op", ["sum", "min", "max"])
@pytest.mark.parametrize("exclusive", [False, True])
def test_nan_and_inf_stay_inside_their_run(gpu, op, exclusive):
    """A NaN, a +inf and a -inf, each inside a run that crosses a tile border: every output outside that run is
    bit-identical to the output with those values replaced by 0."""
    n = 3 * T + 2000
    g = torch.Generator(device=gpu).manual_seed(59)
    keys = (torch.arange(n, device=gpu) // 3000).int()  # runs 10, 21 and 32 cross the borders at T, 2T and 3T
    clean = torch.randint(-9, 9, (n,), device=gpu, generator=g, dtype=torch.int64).float()
    where = {32000: math.nan, 65000: math.inf, 97000: -math.inf}
    for at in where:
        assert at // 3000 == ((at // T + 1) * T) // 3000  # its run reaches into the next tile
        clean[at] = 0.0
    dirty = clean.clone()
    for at, x in where.items():
        dirty[at] = x
    got, ref = ops.scan_by_key(keys, dirty, op, exclusive), ops.scan_by_key(keys, clean, op, exclusive)
    outside = torch.ones(n, dtype=torch.bool, device=gpu)
    for at in where:
        outside[at // 3000 * 3000:(at // 3000 + 1) * 3000] = False
    assert torch.equal(_bits(got)[outside], _bits(ref)[outside])
    assert torch.equal(ref, _ref(Runs(keys), clean, op, exclusive).float())
    first = 32000 + (1 if exclusive else 0)
    assert torch.isnan(got[first:33000]).all() and not torch.isnan(got[30000:first]).any()  # to the end of the run
    if op == "sum":
        first = 65000 + (1 if exclusive else 0)
        assert bool((got[first:66000] == math.inf).all()) and bool((got[97001:99000] == -math.inf).all())
        assert torch.isfinite(got[63000:first]).all()


@pytest.mark.parametrize("regime", ["mean_1000", "all_equal"])
def test_float_sum_within_any_order_bound(gpu, regime):
    n = N_PAT
    g = torch.Generator(device=gpu).manual_seed(61)
    u = 2.0 ** -24
    keys = _geometric_ids(n, 1000 if regime == "mean_1000" else 0, g, gpu).int()
    runs = Runs(keys)
    k = torch.randint(-2**20 + 1, 2**20, (n,), device=gpu, generator=g, dtype=torch.int64)
    x = (k.double() / 2**20).float()
    assert torch.equal(x.double() * 2**20, k.double())  # on the grid: the fp64 cumsums below are exact
    for exclusive in (False, True):
        ref = _ref(runs, x, "sum", exclusive)
        sum_abs = _ref(runs, x.abs(), "sum", exclusive)
        lu = (runs.pos.double() + (0 if exclusive else 1) - 1).clamp_min(0) * u  # (L - 1) u, L summands
        bound = lu / (1 - lu) * sum_abs
        got = ops.scan_by_key(keys, x, "sum", exclusive)
        err = (got.double() - ref).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"{regime} exclusive={exclusive}: inexact outputs {int((err > 0).sum())}, worst err / bound = {worst:.4f}")
        assert bool((err <= bound).all()), worst
        again = ops.scan_by_key(keys, x, "sum", exclusive)
        torch.cuda.synchronize(gpu)
        s = torch.cuda.Stream(device=gpu)
        with torch.cuda.stream(s):
            third = ops.scan_by_key(keys, x, "sum", exclusive)
        s.synchronize()
        assert torch.equal(_bits(got), _bits(again)) and torch.equal(_bits(got), _bits(third))


def test_in_place_flags_and_layout(gpu):
    n = 3 * T + 9
    g = torch.Generator(device=gpu).manual_seed(67)
    kbuf = _geometric_ids(n + 8, 50.0, g, gpu).int()
    vbuf = torch.randint(-9, 9, (n + 8,), device=gpu, generator=g, dtype=torch.int64).int()
    for shift in (0, 1):  # aligned, then views at element offset 1 of larger buffers
        keys, vals = kbuf[shift:n + shift], vbuf[shift:n + shift]
        assert keys.data_ptr() % 16 == 4 * shift
        runs = Runs(keys)
        for v in (vals, vals.float()):
            for op, exclusive in (("sum", False), ("max", True)):
                ref = _ref(runs, v, op, exclusive).to(v.dtype)
                assert torch.equal(ops.scan_by_key(keys, v, op, exclusive), ref)
                out = torch.full((n + 1,), -7, device=gpu, dtype=v.dtype)[shift:n + shift]
                r = ops.scan_by_key(keys, v, op, exclusive, out=out)
                assert r.data_ptr() == out.data_ptr() and torch.equal(out, ref)
                work = v.clone() if shift == 0 else torch.cat([v[:1], v])[1:]
                assert work.data_ptr() % 16 == 4 * shift
                r = ops.scan_by_key(keys, work, op, exclusive, out=work)  # in place
                assert r.data_ptr() == work.data_ptr() and torch.equal(work, ref)
                for flags in (runs.head, runs.head.to(torch.uint8) * 255, torch.cat([runs.head[:1], runs.head])[1:]):
                    assert torch.equal(ops.segmented_scan(v, flags, op, exclusive), ref)
                work = v.clone()
                ops.segmented_scan(work, runs.head, op, exclusive, out=work)
                assert torch.equal(work, ref)
    # non-contiguous views: every other element, and a transposed 2-D view (the result has the values' shape)
    k2 = _geometric_ids(2 * n, 1.3, g, gpu).int()[::2]
    assert not k2.is_contiguous()
    _check_all(k2, g)
    k3 = torch.randint(0, 2, (300, 257), device=gpu, generator=g, dtype=torch.int64).int().t()
    v3 = torch.randint(-9, 9, (300, 257), device=gpu, generator=g, dtype=torch.int64).int().t()
    got = ops.scan_by_key(k3, v3, "sum")
    assert got.shape == v3.shape and torch.equal(got.reshape(-1).long(), _ref(Runs(k3), v3, "sum", False))
    assert ops.run_positions(k3).shape == k3.shape
    # an output that overlaps the keys or the flags: they are cloned first
    kb2 = kbuf.clone()
    ref = _ref(Runs(kbuf[4:n + 4]), vbuf[4:n + 4], "sum", False).int()
    got = ops.scan_by_key(kb2[4:n + 4], vbuf[4:n + 4], "sum", out=kb2[:n])
    assert got.data_ptr() == kb2.data_ptr() and torch.equal(got, ref)
    hb = Runs(kbuf[:n]).head.to(torch.uint8)
    buf = torch.zeros(4 * n, dtype=torch.uint8, device=gpu)
    buf[:n] = hb
    got = ops.segmented_scan(vbuf[:n], buf[:n], "sum", out=buf.view(torch.int32))
    assert torch.equal(got, _ref(Runs(kbuf[:n]), vbuf[:n], "sum", False).int())
    # partly overlapping values and out
    vb2 = vbuf.clone()
    got = ops.scan_by_key(kbuf[4:n + 4], vb2[4:n + 4], "sum", out=vb2[:n])
    assert torch.equal(got, ref)


def test_many_calls_on_one_stream_share_nothing(gpu):
    """scan_by_key with two key sets, run_positions, reduce_by_key and scan back to back on a side stream: each call
    has its own workspace and the ticket is zeroed per launch."""
    n = 40 * T + 11
    g = torch.Generator(device=gpu).manual_seed(71)
    k1 = _geometric_ids(n, 5.0, g, gpu).int()
    k2 = _geometric_ids(n, 5000.0, g, gpu).int()
    v = torch.randint(-100, 100, (n,), device=gpu, generator=g, dtype=torch.int64).int()
    torch.cuda.synchronize(gpu)
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        a1 = ops.scan_by_key(k1, v, "sum")
        a2 = ops.scan_by_key(k2, v, "min", True)
        p2 = ops.run_positions(k2)
        _, ra, rn = ops.reduce_by_key(k2, v, "sum")
        a3 = ops.scan_by_key(k1, v, "sum")
        ops.scan_check(gpu)
    r1, r2 = Runs(k1), Runs(k2)
    assert torch.equal(a1.long(), _ref(r1, v, "sum", False)) and torch.equal(a3, a1)
    assert torch.equal(a2.long(), _ref(r2, v, "min", True)) and torch.equal(p2.long(), r2.pos)
    # the last inclusive sum of every run is reduce_by_key's aggregate
    ends = r2.starts + r2.cnt - 1
    assert rn.item() == r2.cnt.numel() and torch.equal(ops.scan_by_key(k2, v, "sum")[ends], ra[:rn.item()])


def test_c_abi_arguments(gpu):
    """The C entry points: n >= 2^31, a null or misaligned pointer, a bad op and a bad head mode are PCMX_ERR_ARG (-1)
    and launch nothing; n <= 0 returns 0 and touches nothing."""
    import ctypes

    from parallel_c_programs_amd._native import hip_lib

    lib = hip_lib()
    lib.pcmx_scanbykey_workspace_bytes.restype = ctypes.c_longlong
    P, LL = ctypes.c_void_p, ctypes.c_longlong
    stream = P(torch.cuda.current_stream().cuda_stream)
    n = T + 5
    wsb = lib.pcmx_scanbykey_workspace_bytes(LL(n))
    assert wsb >= 16 + 2 * 12 and wsb % 16 == 0 and lib.pcmx_scanbykey_workspace_bytes(LL(0)) >= 0
    keys = (torch.arange(n + 4, device=gpu) // 3).int()
    heads = (torch.arange(n + 16, device=gpu) % 3 == 0).to(torch.uint8)
    vals = torch.arange(n + 4, device=gpu, dtype=torch.int32)
    fvals = vals.float()
    oi = torch.full((n + 4,), -7, device=gpu, dtype=torch.int32)
    of = torch.full((n + 4,), -7.0, device=gpu)
    ws = torch.empty(wsb + 16, dtype=torch.uint8, device=gpu)
    kp, hp, vp, fp, oip, ofp, wp = (t.data_ptr() for t in (keys, heads, vals, fvals, oi, of, ws))

    def sbk_i(k, mode, v, o, m, op, w=wp):
        return lib.pcmx_scan_by_key_i32(P(k), mode, P(v), P(o), LL(m), op, 0, P(w), stream)

    def sbk_f(k, mode, v, o, m, op, w=wp):
        return lib.pcmx_scan_by_key_f32(P(k), mode, P(v), P(o), LL(m), op, 1, P(w), stream)

    def rpos(k, o, m, w=wp):
        return lib.pcmx_run_positions_b32(P(k), P(o), LL(m), P(w), stream)

    assert sbk_i(kp, 0, vp, oip, 1 << 31, 0) == -1 and sbk_f(kp, 0, fp, ofp, 1 << 31, 0) == -1
    assert sbk_i(kp + 4, 0, vp, oip, n, 0) == -1 and sbk_i(kp, 0, vp + 4, oip, n, 0) == -1
    assert sbk_i(kp, 0, vp, oip + 8, n, 0) == -1 and sbk_i(kp, 0, vp, oip, n, 0, wp + 4) == -1
    assert sbk_i(None, 0, vp, oip, n, 0) == -1 and sbk_i(kp, 0, None, oip, n, 0) == -1
    assert sbk_i(kp, 0, vp, None, n, 0) == -1 and sbk_i(kp, 0, vp, oip, n, 0, None) == -1
    assert sbk_i(kp, 0, vp, oip, n, 3) == -1 and sbk_i(kp, 0, vp, oip, n, -1) == -1
    assert sbk_i(kp, 2, vp, oip, n, 0) == -1 and sbk_i(kp, -1, vp, oip, n, 0) == -1
    assert sbk_i(hp + 2, 1, vp, oip, n, 0) == -1 and sbk_i(hp + 1, 1, vp, oip, n, 0) == -1  # flags: 4-B aligned
    assert sbk_f(kp, 0, fp, ofp, n, 3) == -1 and sbk_f(kp + 4, 0, fp, ofp, n, 0) == -1
    assert sbk_f(kp, 0, fp, None, n, 0) == -1 and sbk_f(kp, 5, fp, ofp, n, 0) == -1
    assert rpos(kp, oip, 1 << 31) == -1 and rpos(kp + 4, oip, n) == -1 and rpos(kp, oip + 4, n) == -1
    assert rpos(None, oip, n) == -1 and rpos(kp, None, n) == -1 and rpos(kp, oip, n, None) == -1
    assert sbk_i(kp, 0, vp, oip, 0, 0) == 0 and sbk_f(kp, 0, fp, ofp, -5, 0) == 0 and rpos(kp, oip, 0) == 0
    torch.cuda.synchronize()
    assert bool((oi == -7).all()) and bool((of == -7).all())  # nothing ran
    # real calls: keys, then flags at a 4-byte (not 16-byte) aligned address, then positions
    runs = Runs(keys[:n])
    assert sbk_i(kp, 0, vp, oip, n, 2) == 0
    torch.cuda.synchronize()
    assert torch.equal(oi[:n], vals[:n]) and bool((oi[n:] == -7).all())  # increasing values: the running max is the value
    c = torch.cumsum(vals[:n].long(), 0)
    hruns = Runs(torch.cumsum(heads[4:n + 4].long(), 0).int())
    assert sbk_f(hp + 4, 1, fp, ofp, n, 0) == 0
    torch.cuda.synchronize()
    ref = c - (c - vals[:n].long())[hruns.starts][hruns.inv] - vals[:n].long()  # exclusive sums (below 2^24: exact)
    assert int(ref.max()) < 2**24 and torch.equal(of[:n].long(), ref) and bool((of[n:] == -7).all())
    assert rpos(kp, oip, n) == 0
    torch.cuda.synchronize()
    assert torch.equal(oi[:n].long(), runs.pos) and bool((oi[n:] == -7).all())


@pytest.mark.parametrize("mode", ["keys", "heads", "positions"])
def test_workload(gpu, mode):
    from parallel_c_programs_amd.models import build_workload
    from parallel_c_programs_amd.parallel.dist import Context

    for dtype, op, exclusive, mean_run in (("f32", "sum", False, 4.0), ("i32", "sum", True, 0), ("f32", "max", True, 300.0),
                                           ("i32", "min", False, 1.0)):
        w = build_workload("scanbykey", Context(device=gpu), n=1 << 20, mean_run=mean_run, op=op, dtype=dtype,
                           exclusive=exclusive, mode=mode)
        w.step()
        r = w.check(chunk=300000)
        assert r["check_passed"] and r["elements_checked"] == 1 << 20, r
        if mean_run == 4.0:
            assert abs(r["runs"] / (1 << 20) - 0.25) < 0.01
        if mean_run == 0:
            assert r["runs"] == 1
        t = w.torch_step()
        assert t.shape == w.out.shape and t.dtype == w.out.dtype
        if dtype == "i32" or op != "sum" or mode == "positions":
            assert torch.equal(t, w.out)


@pytest.mark.parametrize("mode", ["keys", "heads", "positions"])
def test_cli(gpu, mode):
    r = run_cli("run_scanbykey", 1048576, "--mean-run", 10, "--mode", mode, "--dtype", "i32", "--op", "sum", "--exclusive",
                "--steps", 2, "--warmup", 1, check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.startswith("runs : ") for ln in lines)
    assert any(ln.endswith("GB/s") for ln in lines)
    assert '"check_passed": true' in r.stdout
