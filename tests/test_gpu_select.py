"""Stream compaction on the MI355X (csrc/kernels/select.hip): every comparison is exact (torch.equal on int32 views of
the payload, == on the count) against torch's x[mask] / torch.nonzero. The tile is 32768 elements; the sizes cover the
tail of the last tile for every n mod 4, one and several tiles, more tiles than CUs (ticket reuse) and more than 64
predecessors (a multi-window look-back)."""
import pytest
import torch

from conftest import run_cli
from parallel_c_programs_amd import ops

pytestmark = pytest.mark.gpu

TILE = 32768
SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 32767, 32768, 32769, 65536 + 7, 300 * TILE + 13]
N_PAT = 70 * TILE + 5
OPS = {"gt": torch.gt, "ge": torch.ge, "lt": torch.lt, "le": torch.le, "eq": torch.eq, "ne": torch.ne}


def _bits(t):
    return t.view(torch.int32)


def _check_mask_modes(x, mask):
    """mask and index mode of one (x, mask) against torch, counts included; returns the count."""
    keep = mask.flatten() != 0
    ref = x.flatten()[keep]
    out, count = ops.compact(x, mask)
    assert count.dtype == torch.int64 and count.dim() == 0 and count.device == x.device
    assert out.numel() == x.numel() and out.dtype == x.dtype
    k = count.item()
    assert k == ref.numel()
    assert torch.equal(_bits(out[:k]), _bits(ref))
    idx, icount = ops.compact_indices(mask)
    assert idx.dtype == torch.int32 and icount.dtype == torch.int64 and icount.dim() == 0
    assert icount.item() == k
    assert torch.equal(idx[:k], torch.nonzero(keep).flatten().int())
    return k


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, n):
    g = torch.Generator(device=gpu).manual_seed(1000 + n % 9973)
    x = torch.randn(n, device=gpu, generator=g)
    mask = torch.rand(n, device=gpu, generator=g) < 0.5
    _check_mask_modes(x, mask)
    ops.scan_check(gpu)


def _patterns(dev):
    n = N_PAT
    i = torch.arange(n, device=dev)
    pats = {
        "all_drop": torch.zeros(n, dtype=torch.bool, device=dev),
        "all_keep": torch.ones(n, dtype=torch.bool, device=dev),
        "first_only": i == 0,
        "last_only": i == n - 1,
        "one_per_tile": (i % TILE) == ((i // TILE) * 997 + 31) % TILE,
        "alternating_tiles": (i // TILE) % 2 == 0,
    }
    pats["one_per_tile"][n - 1] = True  # the 5-element last tile keeps one too
    return pats


@pytest.mark.parametrize("pattern", ["all_drop", "all_keep", "first_only", "last_only", "one_per_tile", "alternating_tiles"])
def test_keep_patterns(gpu, pattern):
    mask = _patterns(gpu)[pattern]
    x = torch.arange(N_PAT, device=gpu, dtype=torch.int32)
    k = _check_mask_modes(x, mask)
    expect = {"all_drop": 0, "all_keep": N_PAT, "first_only": 1, "last_only": 1, "one_per_tile": 71}.get(pattern)
    if expect is not None:
        assert k == expect


def test_payload_bits(gpu):
    n = 3 * TILE + 77
    g = torch.Generator(device=gpu).manual_seed(5)
    mask = (torch.rand(n, device=gpu, generator=g) < 0.5).to(torch.uint8) * 37  # any nonzero byte keeps
    xi = torch.randint(-2**31, 2**31 - 1, (n,), device=gpu, generator=g, dtype=torch.int64).to(torch.int32)
    xi[:4] = torch.tensor([-2**31, 2**31 - 1, 0, -1], dtype=torch.int32, device=gpu)
    mask[:4] = 255
    _check_mask_modes(xi, mask)
    # f32 payload: NaNs with distinct payload bits (quiet and signalling, both signs), +-0, +-inf, a denormal
    special = torch.tensor([0x7fc00000, 0x7fc00001, 0x7f800001, 0xffc12345 - (1 << 32), 0x7fffffff, 0, -2**31,
                            0x7f800000, 0xff800000 - (1 << 32), 1], dtype=torch.int32, device=gpu)
    xf = torch.randn(n, device=gpu, generator=g)
    pos = torch.arange(special.numel(), device=gpu) * 3001 + 2
    _bits(xf)[pos] = special
    mask[pos] = 1
    out, count = ops.compact(xf, mask)
    ref = _bits(xf)[mask != 0]
    assert count.item() == ref.numel() and torch.equal(_bits(out[:ref.numel()]), ref)
    assert torch.isnan(out[:ref.numel()]).sum().item() == 5


@pytest.mark.parametrize("op", sorted(OPS))
def test_predicate(gpu, op):
    n = 5 * TILE + 3
    g = torch.Generator(device=gpu).manual_seed(17)
    x = (torch.rand(n, device=gpu, generator=g) * 16).floor() / 16  # 16 distinct values: the threshold occurs often
    x[::1001] = float("nan")
    x[5::4099] = float("inf")
    x[7::4099] = -float("inf")
    t = 0.5
    assert (x == t).sum().item() > 100
    keep = OPS[op](x, t)
    vals, count = ops.compact_where(x, op, t)
    k = count.item()
    assert count.dtype == torch.int64 and count.dim() == 0 and k == keep.sum().item()
    assert torch.equal(_bits(vals[:k]), _bits(x[keep]))
    idx, icount = ops.compact_where(x, op, t, indices=True)
    assert idx.dtype == torch.int32 and icount.item() == k
    assert torch.equal(idx[:k], torch.nonzero(keep).flatten().int())
    assert (torch.isnan(vals[:k]).sum().item() > 0) == (op == "ne")  # NaN is kept only by ne


def test_layout(gpu):
    n = 2 * TILE + 9
    g = torch.Generator(device=gpu).manual_seed(23)
    # a mask that is a view starting at byte offset 1 of a larger buffer
    mbuf = (torch.rand(n + 8, device=gpu, generator=g) < 0.5).to(torch.uint8)
    mask = mbuf[1:n + 1]
    assert mask.data_ptr() % 4 == 1
    # x as a view at element offset 1
    xbuf = torch.randn(n + 8, device=gpu, generator=g)
    x = xbuf[1:n + 1]
    assert x.data_ptr() % 16 == 4
    _check_mask_modes(x, mask)
    # a non-contiguous x (and mask): every other element, and a transposed 2-D view
    x2 = torch.randn(2 * n, device=gpu, generator=g)[::2]
    m2 = (torch.rand(2 * n, device=gpu, generator=g) < 0.5)[::2]
    assert not x2.is_contiguous()
    _check_mask_modes(x2, m2)
    x3 = torch.randn(300, 257, device=gpu, generator=g).t()
    m3 = (torch.rand(300, 257, device=gpu, generator=g) < 0.5).t()
    _check_mask_modes(x3, m3)
    # a caller-given out larger than needed: elements past count are left untouched (aligned, then misaligned)
    ref = x[mask != 0]
    for obuf in (torch.full((n + 64,), -7.0, device=gpu), torch.full((n + 65,), -7.0, device=gpu)[1:]):
        out, count = ops.compact(x, mask, out=obuf)
        k = count.item()
        assert out.data_ptr() == obuf.data_ptr() and k == ref.numel()
        assert torch.equal(_bits(obuf[:k]), _bits(ref)) and bool((obuf[k:] == -7.0).all())
    ibuf = torch.full((n + 64,), -7, device=gpu, dtype=torch.int32)
    _, count = ops.compact_indices(mask, out=ibuf)
    k = count.item()
    assert torch.equal(ibuf[:k], torch.nonzero(mask).flatten().int()) and bool((ibuf[k:] == -7).all())
    # an out that overlaps x: the input is cloned first
    xo = xbuf.clone()
    out, count = ops.compact(xo[4:n + 4], mask, out=xo[:n + 4])
    assert torch.equal(_bits(out[:count.item()]), _bits(xbuf[4:n + 4][mask != 0]))


def test_stream_error_word_and_scan_around(gpu):
    n = 40 * TILE + 11
    g = torch.Generator(device=gpu).manual_seed(29)
    x = torch.randn(n, device=gpu, generator=g)
    m1 = torch.rand(n, device=gpu, generator=g) < 0.5
    m2 = torch.rand(n, device=gpu, generator=g) < 0.1
    xi = torch.randint(0, 4, (n,), device=gpu, generator=g).float()  # integer-valued: the f32 scan is exact (sum < 2^24)
    ref_scan = torch.cumsum(xi.double(), 0).float()
    torch.cuda.synchronize(gpu)
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        y0 = ops.scan(xi)
        o1, c1 = ops.compact(x, m1)  # two back-to-back selects on one stream: the workspace is zeroed per launch
        o2, c2 = ops.compact(x, m2)
        i2, ic2 = ops.compact_indices(m2)
        y1 = ops.scan(xi)
        ops.scan_check(gpu)  # synchronises s and raises if any look-back on it gave up
    assert c1.item() == m1.sum().item() and torch.equal(_bits(o1[:c1.item()]), _bits(x[m1]))
    assert c2.item() == m2.sum().item() and torch.equal(_bits(o2[:c2.item()]), _bits(x[m2]))
    assert ic2.item() == c2.item() and torch.equal(i2[:c2.item()], torch.nonzero(m2).flatten().int())
    assert torch.equal(y0, ref_scan) and torch.equal(y1, ref_scan)


def test_count_and_exact_size_forms(gpu):
    n = TILE + 100
    g = torch.Generator(device=gpu).manual_seed(31)
    x = torch.randn(n, device=gpu, generator=g)
    mask = torch.rand(n, device=gpu, generator=g) < 0.25
    _, count = ops.compact(x, mask)
    assert count.dtype == torch.int64 and count.dim() == 0 and count.is_cuda
    sel = ops.select(x, mask)
    assert sel.shape == (count.item(),) and torch.equal(_bits(sel), _bits(x[mask]))
    idx = ops.select_indices(mask)
    assert idx.shape == (count.item(),) and torch.equal(idx, torch.nonzero(mask.flatten()).flatten().int())
    assert torch.equal(ops.select(x.reshape(4, -1), mask.reshape(4, -1)), x[mask])


@pytest.mark.parametrize("mode", ["mask", "index", "where"])
def test_workload(gpu, mode):
    from parallel_c_programs_amd.models import build_workload
    from parallel_c_programs_amd.parallel.dist import Context

    w = build_workload("select", Context(device=gpu), n=1 << 20, keep=0.3, mode=mode)
    w.step()
    r = w.check()
    assert r["check_passed"] and r["lookback_ok"] and r["kept"] == r["kept_torch"], r
    assert abs(r["kept"] / (1 << 20) - 0.3) < 0.01


@pytest.mark.parametrize("mode", ["mask", "index", "where"])
def test_cli(gpu, mode):
    r = run_cli("run_select", 1048576, "--keep", 0.3, "--mode", mode, "--steps", 2, "--warmup", 1, check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.startswith("count : ") for ln in lines)
    assert any(ln.endswith("GB/s") for ln in lines)
    assert '"check_passed": true' in r.stdout


def test_c_abi_arguments_and_workspace_check(gpu):
    """The C entry points: n >= 2^31 and misaligned x / out / mask are PCMX_ERR_ARG (-1) and launch nothing, n <= 0
    stores count 0, and pcmx_scan_check reads a select workspace."""
    import ctypes

    from parallel_c_programs_amd._native import hip_lib

    lib = hip_lib()
    lib.pcmx_select_workspace_bytes.restype = ctypes.c_longlong
    P, LL = ctypes.c_void_p, ctypes.c_longlong
    stream = P(torch.cuda.current_stream().cuda_stream)
    n = TILE + 5
    assert lib.pcmx_select_workspace_bytes(LL(n)) >= 16 + 2 * 8 and lib.pcmx_select_workspace_bytes(LL(n)) % 16 == 0
    x = torch.arange(n + 4, device=gpu, dtype=torch.int32)
    mask = (x % 3 == 0).to(torch.uint8)
    out = torch.full((n + 4,), -7, device=gpu, dtype=torch.int32)
    count = torch.full((), -1, device=gpu, dtype=torch.int64)
    ws = torch.empty(lib.pcmx_select_workspace_bytes(LL(n)), dtype=torch.uint8, device=gpu)

    def b32(xp, mp, op, m):
        return lib.pcmx_select_b32(P(xp), P(mp), P(op), LL(m), P(count.data_ptr()), P(ws.data_ptr()), None, stream)

    xp, mp, op = x.data_ptr(), mask.data_ptr(), out.data_ptr()
    assert b32(xp, mp, op, 1 << 31) == -1
    assert b32(xp + 4, mp, op, n) == -1 and b32(xp, mp, op + 4, n) == -1 and b32(xp, mp + 1, op, n) == -1
    assert lib.pcmx_select_index(P(mp + 2), P(op), LL(n), P(count.data_ptr()), P(ws.data_ptr()), None, stream) == -1
    assert lib.pcmx_select_if_f32(P(xp), 6, ctypes.c_float(0.0), P(op), 0, LL(n), P(count.data_ptr()), P(ws.data_ptr()),
                                  None, stream) == -1
    torch.cuda.synchronize()
    assert count.item() == -1 and bool((out == -7).all())  # nothing ran
    assert b32(xp, mp, op, 0) == 0
    torch.cuda.synchronize()
    assert count.item() == 0 and bool((out == -7).all())
    assert b32(xp, mp, op, n) == 0
    assert lib.pcmx_scan_check(P(ws.data_ptr()), stream) == 0
    k = count.item()
    assert k == (mask[:n] != 0).sum().item() and torch.equal(out[:k], x[:n][mask[:n] != 0]) and bool((out[k:] == -7).all())
