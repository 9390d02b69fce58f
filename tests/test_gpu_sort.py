"""Radix sort on the MI355X (csrc/kernels/sort.hip): every comparison is exact. The oracle is torch.sort(..., stable=True)
on the same tensor (or on the masked key for `bits`); indices are compared with torch.equal after .int(), int32 keys and
all values bitwise, f32 sorted values with torch.equal after nan_to_num of both sides plus equal NaN positions. The
tile is 16384 keys; the sizes cover partial rows and tiles, one and several tiles, more tiles than the 256 CUs (ticket
reuse) and more than 64 predecessors (several look-back windows)."""
import pytest
import torch

from conftest import run_cli
from parallel_c_programs_amd import ops

pytestmark = pytest.mark.gpu

TILE = 16384
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 7, 300 * TILE + 13]
N_PAT = 70 * TILE + 5
# NaNs of both signs and several payloads (quiet and signalling), +-0 interleaved, +-inf, a denormal
SPECIAL = [0x7fc00000, 0x7fc00001, 0x7f800001, 0xffc12345 - (1 << 32), 0x7fffffff, 0xffffffff - (1 << 32), 0, -2**31,
           0x7f800000, 0xff800000 - (1 << 32), 1, 0x80000001 - (1 << 32), 0, -2**31]


def _bits(t):
    return t.view(torch.int32)


def _same_values(got, ref):
    """Sorted keys against the oracle's: bitwise for int32; for f32 equal after nan_to_num, equal NaN positions."""
    assert got.dtype == ref.dtype and got.shape == ref.shape
    if got.dtype == torch.int32:
        assert torch.equal(got, ref)
        return
    assert torch.isnan(got).sum().item() == torch.isnan(ref).sum().item()
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(ref))


def _check_modes(x, descending=False, bits=None, oracle_key=None, modes=("keys", "pairs", "argsort", "sort"),
                 host_oracle=False):
    """The entry points on x against ONE torch.sort(stable=True) of x (or of oracle_key); returns the oracle indices.
    host_oracle sorts a host copy of the tensor: torch's own GPU sort orders NaNs with the sign bit set BEFORE -inf (the
    vendor radix sort's bit order), unlike torch.sort on the host, whose order (every NaN last, all NaNs tied) is the
    one this op is specified to have."""
    flat = x.flatten()
    keep = flat.clone()
    src = flat if oracle_key is None else oracle_key
    ref_idx = torch.sort(src.cpu() if host_oracle else src, stable=True, descending=descending).indices.to(x.device)
    ref_vals = flat[ref_idx]
    n = flat.numel()
    kw = {"descending": descending, "bits": bits}
    if "keys" in modes:
        _same_values(ops.sort_keys(x, **kw), ref_vals)
    if "argsort" in modes:
        idx = ops.argsort(x, **kw)
        assert idx.dtype == torch.int32 and idx.shape == (n,) and torch.equal(idx, ref_idx.int())
    if "sort" in modes:
        vals, idx = ops.sort(x, **kw)
        assert idx.dtype == torch.int32 and torch.equal(idx, ref_idx.int())
        _same_values(vals, ref_vals)
    if "pairs" in modes:
        payload = torch.arange(n, device=x.device, dtype=torch.int32) * 3 - 7
        ks, vs = ops.sort_by_key(x, payload, **kw)
        _same_values(ks, ref_vals)
        assert vs.dtype == torch.int32 and torch.equal(vs, payload[ref_idx])
    ops.scan_check(x.device)
    assert torch.equal(_bits(flat), _bits(keep))  # the input is never written
    return ref_idx


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, n):
    g = torch.Generator(device=gpu).manual_seed(2000 + n % 9973)
    xf = (torch.randn(n, device=gpu, generator=g) * 64).round() / 64  # ties in every tile
    for mode in ("keys", "pairs", "argsort"):  # each mode on its own, the look-back word checked after each
        _check_modes(xf, modes=(mode,))
    xi = torch.randint(-2**31, 2**31, (n,), device=gpu, generator=g, dtype=torch.int64).to(torch.int32)
    _check_modes(xi, descending=True, modes=("sort", "pairs"))


def _patterns(dev):
    n = N_PAT
    i = torch.arange(n, device=dev, dtype=torch.int64)
    g = torch.Generator(device=dev).manual_seed(41)
    full = torch.randint(-2**31, 2**31, (n,), device=dev, generator=g, dtype=torch.int64)
    full[:4] = torch.tensor([-2**31, 2**31 - 1, 0, -1], device=dev)
    d = (i // TILE * 37) % 256  # one digit per tile, a different one in neighbouring tiles, in every pass
    pats = {
        "all_equal": torch.full((n,), 12345, device=dev),
        "sorted": i - n // 2,
        "reverse": n // 2 - i,
        "two_values": (i * 2654435761 >> 7) % 2 * 1000003 - 17,
        "top_byte_only": ((i * 2654435761 >> 5) % 256 - 128) << 24,
        "low_byte_only": (i * 2654435761 >> 5) % 256 + 0x01020300,
        "one_digit_per_tile": d | d << 8 | d << 16 | (d & 0x7f) << 24,
        "full_range": full,
    }
    return {k: v.to(torch.int32) for k, v in pats.items()}


@pytest.mark.parametrize("pattern", ["all_equal", "sorted", "reverse", "two_values", "top_byte_only", "low_byte_only",
                                     "one_digit_per_tile", "full_range"])
def test_key_patterns(gpu, pattern):
    k = _patterns(gpu)[pattern]
    ref_idx = _check_modes(k, modes=("argsort", "pairs"))
    if pattern in ("all_equal", "sorted"):
        assert torch.equal(ref_idx, torch.arange(N_PAT, device=gpu))


@pytest.mark.parametrize("descending", [False, True])
def test_stability(gpu, descending):
    n = 9 * TILE + 321
    g = torch.Generator(device=gpu).manual_seed(43)
    k = torch.randint(0, 7, (n,), device=gpu, generator=g, dtype=torch.int32) * 300007 - 900000
    pos = torch.arange(n, device=gpu, dtype=torch.int32)
    ref = torch.sort(k, stable=True, descending=descending)
    ks, vs = ops.sort_by_key(k, pos, descending=descending)  # payload = position
    assert torch.equal(ks, ref.values) and torch.equal(vs, ref.indices.int())
    assert torch.equal(ops.argsort(k, descending=descending), ref.indices.int())
    _check_modes(k.float(), descending=descending, modes=("sort",))
    ops.scan_check(gpu)


@pytest.mark.parametrize("descending", [False, True])
def test_f32_specials(gpu, descending):
    n = 3 * TILE + 77
    g = torch.Generator(device=gpu).manual_seed(5)
    x = torch.randn(n, device=gpu, generator=g)
    pos = torch.arange(len(SPECIAL), device=gpu) * 3001 + 2
    _bits(x)[pos] = torch.tensor(SPECIAL, dtype=torch.int32, device=gpu)
    assert torch.isnan(x).sum().item() == 6
    ref_idx = _check_modes(x, descending=descending, modes=("keys", "sort", "argsort"), host_oracle=True)
    vals = ops.sort_keys(x, descending=descending)
    nan_at = slice(0, 6) if descending else slice(n - 6, n)
    assert bool(torch.isnan(vals[nan_at]).all()) and bool((_bits(vals[nan_at]) == 0x7fffffff).all())
    assert not bool((_bits(vals) == -2**31).any())  # both zeros come out as +0.0
    # values are moved as bits: the NaN payloads of VALUES survive
    ks, vs = ops.sort_by_key(x, x, descending=descending)
    _same_values(ks, x[ref_idx])
    assert torch.equal(_bits(vs), _bits(x)[ref_idx])
    assert sorted(_bits(vs)[torch.isnan(vs)].tolist()) == sorted(SPECIAL[:6])
    ops.scan_check(gpu)


@pytest.mark.parametrize("bits", [1, 7, 8, 9, 16, 20, 31, 32])
def test_bits(gpu, bits):
    n = 2 * TILE + 7
    g = torch.Generator(device=gpu).manual_seed(50 + bits)
    lo, hi = (0, 1 << bits) if bits < 32 else (-2**31, 2**31)
    k = torch.randint(lo, hi, (n,), device=gpu, generator=g, dtype=torch.int64).to(torch.int32)
    _check_modes(k, bits=bits, modes=("keys", "pairs", "argsort"))
    _check_modes(k, bits=bits, descending=True, modes=("sort",))


def test_bits_with_stray_high_bits(gpu):
    """The defined semantics: the stable sort by the low `bits` bits, whatever lies above them."""
    n = 2 * TILE + 7
    g = torch.Generator(device=gpu).manual_seed(61)
    k = torch.randint(-2**31, 2**31, (n,), device=gpu, generator=g, dtype=torch.int64).to(torch.int32)
    for bits in (9, 20):
        masked = k.long() & ((1 << bits) - 1)
        assert bool((k.long() >> bits != 0).any())
        _check_modes(k, bits=bits, oracle_key=masked)
    _check_modes(k, bits=12, descending=True, oracle_key=k.long() & 0xfff, modes=("sort", "pairs"))


def test_layout(gpu):
    n = 2 * TILE + 9
    g = torch.Generator(device=gpu).manual_seed(23)
    xbuf = torch.randn(n + 8, device=gpu, generator=g)
    x = xbuf[1:n + 1]  # a view at element offset 1
    assert x.data_ptr() % 16 == 4
    _check_modes(x)
    vbuf = torch.arange(n + 8, device=gpu, dtype=torch.int32)
    ks, vs = ops.sort_by_key(x, vbuf[3:n + 3])  # misaligned values too
    ref = torch.sort(x, stable=True)
    assert torch.equal(ks, ref.values) and torch.equal(vs, ref.indices.int() + 3)
    x2 = torch.randn(2 * n, device=gpu, generator=g)[::2]  # every other element
    assert not x2.is_contiguous()
    _check_modes(x2, descending=True)
    x3 = torch.randint(-999, 999, (300, 257), device=gpu, generator=g, dtype=torch.int32).t()  # transposed 2-D
    assert not x3.is_contiguous()
    _check_modes(x3)
    ops.scan_check(gpu)


def test_two_streams(gpu):
    n = 40 * TILE + 11
    g = torch.Generator(device=gpu).manual_seed(29)
    a = torch.randn(n, device=gpu, generator=g)
    b = torch.randint(-2**31, 2**31, (n,), device=gpu, generator=g, dtype=torch.int64).to(torch.int32)
    ra, rb = torch.sort(a, stable=True), torch.sort(b, stable=True, descending=True)
    torch.cuda.synchronize(gpu)
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        va, ia = ops.sort(a)
        ia2 = ops.argsort(a)  # back to back on one stream: the flags are reset per call
    vb, ib = ops.sort(b, descending=True)
    ops.scan_check(gpu)  # the current stream's word
    with torch.cuda.stream(side):
        ops.scan_check(gpu)  # the side stream's word
    assert torch.equal(va, ra.values) and torch.equal(ia, ra.indices.int()) and torch.equal(ia2, ia)
    assert torch.equal(vb, rb.values) and torch.equal(ib, rb.indices.int())


def test_cli(gpu):
    r = run_cli("run_sort", 1048576, "--mode", "pairs", "--dtype", "i32", "--bits", 20, "--steps", 2, "--warmup", 1,
                check=False, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Time : ") for ln in lines) and any(ln.startswith("passes : 3") for ln in lines)
    assert any(ln.endswith("GB/s") for ln in lines)
    assert '"check_passed": true' in r.stdout


def test_c_abi_arguments_and_workspace_check(gpu):
    """The C entry point: n >= 2^30, misaligned pointers, bad enums and bit ranges are PCMX_ERR_ARG (-1) and launch
    nothing, n <= 0 returns 0 and touches nothing, keys_out may be NULL in index mode, and pcmx_scan_check reads a sort
    workspace."""
    import ctypes

    from parallel_c_programs_amd._native import hip_lib

    lib = hip_lib()
    lib.pcmx_sort_workspace_bytes.restype = ctypes.c_longlong
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    stream = P(torch.cuda.current_stream().cuda_stream)
    n = TILE + 5
    U32, I32, KEYS, PAIRS, INDEX = 0, 1, 0, 1, 2
    size = lib.pcmx_sort_workspace_bytes(LL(n), I(INDEX))
    assert size % 16 == 0 and size >= lib.pcmx_sort_workspace_bytes(LL(n), I(PAIRS)) >= \
        lib.pcmx_sort_workspace_bytes(LL(n), I(KEYS)) >= 4 * n
    g = torch.Generator(device=gpu).manual_seed(3)
    k = torch.randint(0, 1 << 16, (n + 4,), device=gpu, generator=g, dtype=torch.int32)
    ko = torch.full((n + 4,), -7, device=gpu, dtype=torch.int32)
    vo = torch.full((n + 4,), -7, device=gpu, dtype=torch.int32)
    ws = torch.zeros(size, dtype=torch.uint8, device=gpu)

    def sort(kp, kop, vip, vop, m, key_type=U32, mode=INDEX, begin=0, end=16):
        return lib.pcmx_radix_sort(P(kp), P(kop), P(vip), P(vop), LL(m), I(key_type), I(mode), I(0), I(begin), I(end),
                                   P(ws.data_ptr()), None, stream)

    kp, kop, vop = k.data_ptr(), ko.data_ptr(), vo.data_ptr()
    assert sort(kp, kop, None, vop, 1 << 30) == -1
    assert sort(kp + 4, kop, None, vop, n) == -1 and sort(kp, kop + 4, None, vop, n) == -1
    assert sort(kp, kop, None, vop + 4, n) == -1 and sort(kp, kop, None, None, n) == -1
    assert sort(kp, kop, kp + 4, vop, n, mode=PAIRS) == -1 and sort(kp, kop, None, vop, n, mode=PAIRS) == -1
    assert sort(kp, None, None, None, n, mode=KEYS) == -1
    assert sort(kp, kop, None, vop, n, key_type=3) == -1 and sort(kp, kop, None, vop, n, mode=3) == -1
    assert sort(kp, kop, None, vop, n, begin=8, end=8) == -1 and sort(kp, kop, None, vop, n, end=33) == -1
    assert sort(kp, kop, None, vop, n, begin=-1) == -1
    assert sort(kp, kop, None, vop, 0) == 0 and sort(None, None, None, None, -5) == 0
    torch.cuda.synchronize()
    assert bool((ko == -7).all()) and bool((vo == -7).all()) and bool((ws == 0).all())  # nothing ran
    ref = torch.sort(k[:n], stable=True)
    assert sort(kp, None, None, vop, n) == 0  # u32 keys, 2 passes, indices alone
    assert lib.pcmx_scan_check(P(ws.data_ptr()), stream) == 0
    assert torch.equal(vo[:n], ref.indices.int()) and bool((vo[n:] == -7).all()) and bool((ko == -7).all())
    assert sort(kp, kop, None, vop, n, begin=0, end=9) == 0  # a 1-bit last digit; the keys land in keys_out
    assert lib.pcmx_scan_check(P(ws.data_ptr()), stream) == 0
    ref9 = torch.sort(k[:n] & 0x1ff, stable=True).indices
    assert torch.equal(vo[:n], ref9.int()) and torch.equal(ko[:n], k[:n][ref9]) and bool((ko[n:] == -7).all())
