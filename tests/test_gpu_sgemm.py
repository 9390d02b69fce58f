"""SGEMM on the GPU against exact references: integer operands (every summation order exact), single products by
powers of two (bit-exact planes of the x6 split), single products of full-mantissa operands (8 ulp), dense operands
against CPU models of the two accumulation schemes (tests/_sgemm_oracle.py), leading dimensions with sentinels,
the alpha/beta epilogue, the input contract of ops.sgemm and the refusals of the C ABI.

Variants (sgemm.hip): 0 / 1 LDS-DMA 256 / 128 tiles, 16 register-staged, 17 direct-register persistent, 18 the same
on 7 blocks, 20 bf16x6 (sgemm_x6.hip), -1 the default dispatch (the 128-tile kernel at these sizes).

The figures measured on an MI355X stand in the docstrings of the tests that measure them and, with the per-test
times, in profiles/r15_sgemm_tests/README.md.
"""
import ctypes
import functools
import re
from pathlib import Path

import pytest
import torch

import _sgemm_oracle as so
from parallel_c_programs_amd import ops

pytestmark = pytest.mark.gpu

VARIANTS = [0, 1, 16, 17, 18, 20, -1]
F32_VARIANTS = [0, 1, 16, 17, 18, -1]


def _tile(v):
    return 128 if v in (1, -1) else 256


def _kq(v):
    return 64 if v in (17, 18) else 32


@functools.lru_cache(maxsize=None)
def _int_case(m, n, k):
    """Seeded integer operands and their exact product (int64), shared by every test of that shape; never modified."""
    a, b = so.small_ints((m, k), seed=3 * m + k), so.small_ints((k, n), seed=5 * n + k + 1)
    return a, b, (a.long() @ b.long()).float()


def _int_on(gpu, m, n, k):
    return tuple(t.to(gpu) for t in _int_case(m, n, k))


# ------------------------------------------------------------ 1. integer-exact K edges
@pytest.mark.parametrize("variant", VARIANTS)
def test_k_edges_integer_exact(gpu, variant):
    """K of one, two and three pipeline steps (32-k stages of variants 0 / 1 / 16: nk = 1, 2, 3 picks each
    stage(t, WRITE, LOAD) combination and the DMA kernels' `t + 1 < nk`; 64-k chunk pairs of variants 17 / 18: at
    K = 64 the first pair is the last and the look-ahead leaves the tile straight out of the prologue) on two tiles."""
    t, q = _tile(variant), _kq(variant)
    for k in (q, 2 * q, 3 * q):
        a, b, expected = _int_on(gpu, 2 * t, t, k)
        so.assert_exact(ops.sgemm(a, b, variant=variant), expected, f"variant {variant} K={k}")


@pytest.mark.parametrize("variant", [17, 18])
@pytest.mark.parametrize("mn", [(512, 512), (1792, 256), (512, 1024), (768, 1280)])
def test_direct_tile_grids_integer_exact(gpu, variant, mn):
    """4, 7, 8 and 15 tiles at K = 64. Variant 18 (7 blocks) runs them as one block per tile, exactly 7 blocks, 7 blocks
    of which one has two tiles and six clamp their look-ahead past the end, and 3 / 2 tiles per block."""
    a, b, expected = _int_on(gpu, mn[0], mn[1], 64)
    so.assert_exact(ops.sgemm(a, b, variant=variant), expected, f"variant {variant} {mn}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_two_m_groups_integer_exact(gpu, variant):
    """Nine tile rows: a full group of 8 and a partial group of 1 in the grouped tile order."""
    m, n, k = (1152, 384, 32) if _tile(variant) == 128 else (2304, 512, 64)
    a, b, expected = _int_on(gpu, m, n, k)
    so.assert_exact(ops.sgemm(a, b, variant=variant), expected, f"variant {variant}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", [(257, 255, 33), (1, 1, 1), (100, 70, 33)])
def test_ragged_shapes_integer_exact(gpu, variant, shape):
    a, b, expected = _int_on(gpu, *shape)
    so.assert_exact(ops.sgemm(a, b, variant=variant), expected, f"variant {variant} {shape}")


@pytest.mark.parametrize("shape", [(1, 1, 1), (65, 63, 17), (300, 200, 100)])
def test_simt_integer_exact(gpu, shape):
    a, b, expected = _int_on(gpu, *shape)
    so.assert_exact(ops.sgemm_simt(a, b), expected, f"simt {shape}")


# ------------------------------------------------------------ 2. planes by selector
@functools.lru_cache(maxsize=None)
def _selector_case(m, n, k):
    a = so.full_mantissa((m, k), seed=m + k)
    b = so.full_mantissa((k, n), seed=n + k + 1)
    b_side = [(s, a[:, rows] * vals) for s, rows, vals in
              (so.selector(k, n, seed=21, part=p) for p in range(so.selector_parts(k, n)))]
    a_side = [(s.t().contiguous(), vals[:, None] * b[cols]) for s, cols, vals in
              (so.selector(k, m, seed=22, part=p) for p in range(so.selector_parts(k, m)))]
    return a, b, b_side, a_side


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", [(512, 256, 256), (256, 512, 512), (256, 256, 512)])
def test_planes_by_selector_bit_exact(gpu, variant, shape):
    """Every output is ONE product of a full-mantissa operand with +-2^e, so it is exact in every variant. For variant
    20 a full-mantissa A times a selector B pins a0 b0, a1 b0 and a2 b0 at every (row, k), and a selector A times a
    full-mantissa B pins a0 b0, a0 b1 and a0 b2 at every (k, column); with K = 512 two selectors cover every k."""
    a, b, b_side, a_side = _selector_case(*shape)
    ag, bg = a.to(gpu), b.to(gpu)
    for p, (sel, expected) in enumerate(b_side):
        c = ops.sgemm(ag, sel.to(gpu), variant=variant)
        so.assert_exact(c.cpu(), expected, f"variant {variant} B selector {p}")
    for p, (sel, expected) in enumerate(a_side):
        c = ops.sgemm(sel.to(gpu), bg, variant=variant)
        so.assert_exact(c.cpu(), expected, f"variant {variant} A selector {p}")


# ------------------------------------------------------------ 3. a1 b1 and the six-product sum
@pytest.mark.parametrize("family", ["sig16", "full_mantissa"])
def test_x6_single_products_8ulp(gpu, family):
    """Variant 20, one product per output (A has one entry per row, B is dense), both operands from `family`:
    relative error at most 8 * 2^-24 (derivation: so.assert_single_product). sig16 operands have p2 = 0, so a1 b1 is
    the only low product; full_mantissa operands exercise all six.
    Measured on an MI355X: largest error 1.90 ulp (sig16, either side), 2.32 ulp (full_mantissa, A side) and 2.60 ulp
    (full_mantissa, B side); the CPU model gives 1.00 and 1.48."""
    fam = getattr(so, family)
    m = n = k = 256
    av = fam((m,), seed=31)
    a1, cols, _ = so.selector(k, m, seed=32, values=av)
    bd = fam((k, n), seed=33)
    c = ops.sgemm(a1.t().contiguous().to(gpu), bd.to(gpu), variant=20)
    print(f"single-product max error, {family}: {so.single_product_ulps(c, av, bd[cols]):.3f} ulp")
    so.assert_single_product(c, av, bd[cols], family)
    # the same on the B side: B has one entry per column, A is dense
    bv = fam((n,), seed=34)
    b1, rows, _ = so.selector(k, n, seed=35, values=bv)
    ad = fam((m, k), seed=36)
    c = ops.sgemm(ad.to(gpu), b1.to(gpu), variant=20)
    print(f"single-product max error, {family}, B side: {so.single_product_ulps(c.t(), bv, ad[:, rows].t()):.3f} ulp")
    so.assert_single_product(c.t(), bv, ad[:, rows].t(), family + " B side")


@pytest.mark.parametrize("low", [True, False], ids=["2^-110", "0x7f7f7fff"])
def test_x6_single_products_at_the_ends_of_the_split_range(gpu, low):
    """|x| in [2^-110, 2^-100) and in [2^120, 0x7f7f7fff] (both limits included) on either side, the partner a dense
    +-2^e that keeps every product normal: within 8 * 2^-24.
    Measured on an MI355X: 0 ulp at both ends and on both sides (a product by a power of two is exact)."""
    m = n = k = 256
    e = (40, 80) if low else (-100, -40)
    av = so.range_end_values(m, low, seed=41)
    a1, cols, _ = so.selector(k, m, seed=42, values=av)
    bd = so.pow2_dense((k, n), 43, *e)
    c = ops.sgemm(a1.t().contiguous().to(gpu), bd.to(gpu), variant=20)
    print(f"range end low={low}, A side: {so.single_product_ulps(c, av, bd[cols]):.3f} ulp")
    so.assert_single_product(c, av, bd[cols], "A side")
    bv = so.range_end_values(n, low, seed=44)
    b1, rows, _ = so.selector(k, n, seed=45, values=bv)
    ad = so.pow2_dense((m, k), 46, *e)
    c = ops.sgemm(ad.to(gpu), b1.to(gpu), variant=20)
    print(f"range end low={low}, B side: {so.single_product_ulps(c.t(), bv, ad[:, rows].t()):.3f} ulp")
    so.assert_single_product(c.t(), bv, ad[:, rows].t(), "B side")


def test_operands_above_the_x6_split_limit(gpu):
    """0x7f7f8000 .. 0x7f7fffff are finite floats that bf16 rounds to infinity. The f32 kernels multiply them exactly;
    variant 20 documents NaN for them (sgemm_x6.hip, ops.sgemm) and must never return a wrong finite value.
    Measured on an MI355X: NaN in all 1024 outputs of the four rows that hold such an operand, exact elsewhere."""
    n = 256
    big = torch.tensor([so.SPLIT_MAX_BITS + 1, 0x7F7FFFFF], dtype=torch.int32).view(torch.float32)
    av = torch.ones(n)
    av[:2], av[2:4] = big, -big
    a1, cols, _ = so.selector(n, n, seed=47, values=av)
    bd = so.pow2_dense((n, n), 48, -100, -40)
    expected = av[:, None] * bd[cols]
    a, b = a1.t().contiguous().to(gpu), bd.to(gpu)
    for variant in F32_VARIANTS:
        so.assert_exact(ops.sgemm(a, b, variant=variant).cpu(), expected, f"variant {variant}")
    c = ops.sgemm(a, b, variant=20).cpu()
    so.assert_exact(c[4:], expected[4:], "variant 20, rows inside the range")
    print(f"variant 20 above the split limit: {int(c[:4].isnan().sum())} of {c[:4].numel()} NaN")
    assert (c[:4].isnan() | (c[:4] == expected[:4])).all()


# ------------------------------------------------------------ 4. dense accuracy against the models
@functools.lru_cache(maxsize=None)
def _dense_case(m, n, k):
    a, b = so.full_mantissa((m, k), seed=m + 2 * k), so.full_mantissa((k, n), seed=n + 3 * k)
    return a, b, so.x6_model(a, b), so.f32_chain_model(a, b)


@pytest.mark.parametrize("variant", [0, 1, 16, 17, 20])
@pytest.mark.parametrize("shape", [(256, 256, 32), (512, 768, 96), (256, 256, 512)])
def test_dense_rms_against_model(gpu, variant, shape):
    """rms of |c - fp64| / sum |a||b| at most 4x the rms of the CPU model of the variant's accumulation (x6_model for
    variant 20, f32_chain_model for the f32 MFMA kernels) on the same full-mantissa operands; the model rounds once
    per MFMA, the hardware at most 16 times. The max stays under the bound of test_gpu_core.py.
    Measured kernel / model rms ratios on an MI355X, (256,256,32) / (512,768,96) / (256,256,512):
      variants 0, 1, 16   1.400 / 1.410 / 1.410   (the three kernels add in the same k order: identical results)
      variant 17          1.384 / 1.408 / 1.417
      variant 20          1.450 / 1.407 / 1.380
    i.e. sqrt(2): the hardware rounds about twice where the model rounds once. Largest max error 5.5e-7 (bound 4e-6)."""
    a, b, x6, chain = _dense_case(*shape)
    c = ops.sgemm(a.to(gpu), b.to(gpu), variant=variant)
    ratio, cmax, mmax = so.assert_dense_rms(c, x6 if variant == 20 else chain, a, b, f"variant {variant} {shape}")
    print(f"dense variant {variant} {shape}: rms ratio {ratio:.3f}, max {cmax:.3e} (model max {mmax:.3e})")


# ------------------------------------------------------------ 5. leading dimensions and sentinels
SENTINEL = -12345.0


def _embed(x, ld, dev, offset=4):
    """x as a view with row stride `ld` at storage offset `offset` inside a sentinel-filled buffer. Returns
    (buffer, view, mask of the buffer's elements that belong to the view)."""
    rows, cols = x.shape
    buf = torch.full((offset + rows * ld + 8,), SENTINEL, device=dev)
    mask = torch.zeros_like(buf, dtype=torch.bool)
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    mask[offset:offset + rows * ld].view(rows, ld)[:, :cols] = True
    view.copy_(x)
    return buf, view, mask


def _assert_surround_intact(buf, mask, what):
    outside = buf.view(torch.int32)[~mask]
    want = torch.tensor([SENTINEL]).view(torch.int32).item()
    assert bool((outside == want).all()), f"{what}: {int((outside != want).sum())} sentinel elements overwritten"


@pytest.mark.parametrize("variant", VARIANTS)
def test_leading_dimensions_and_sentinels(gpu, variant):
    """lda = K + 4, ldb = N + 8, ldc = N + 12, every view 4 elements into its buffer: the result equals the contiguous
    call of the same variant (and the exact integer product), and nothing outside C's view changes."""
    m, n, k = 512, 512, 64
    a, b, expected = _int_on(gpu, m, n, k)
    c0 = so.small_ints((m, n), seed=51).to(gpu)
    _, av, _ = _embed(a, k + 4, gpu)
    _, bv, _ = _embed(b, n + 8, gpu)
    assert av.data_ptr() % 16 == 0 and av.stride(0) == k + 4 and bv.stride(0) == n + 8
    plain = ops.sgemm(a, b, variant=variant)
    so.assert_exact(plain, expected, f"variant {variant} contiguous")
    so.assert_exact(ops.sgemm(av, bv, variant=variant), plain, f"variant {variant} strided a, b")
    for alpha, beta in ((1.0, 0.0), (2.0, -1.0)):
        want = ops.sgemm_out(a, b, c0.clone(), alpha=alpha, beta=beta, variant=variant)
        so.assert_exact(want, alpha * expected + beta * c0, f"variant {variant} contiguous beta={beta}")
        for (x, y) in ((a, b), (av, bv)):
            cbuf, cv, cmask = _embed(c0, n + 12, gpu)
            out = ops.sgemm_out(x, y, cv, alpha=alpha, beta=beta, variant=variant)
            assert out.data_ptr() == cv.data_ptr()
            so.assert_exact(cv, want, f"variant {variant} strided c beta={beta}")
            _assert_surround_intact(cbuf, cmask, f"variant {variant} beta={beta}")


# ------------------------------------------------------------ 6. epilogue
@pytest.mark.parametrize("variant", VARIANTS)
def test_epilogue_integer_exact(gpu, variant):
    """beta == 0 never reads C (a C full of NaN and +-Inf gives the plain product), and alpha / beta scale exactly, on
    2 x 3 tiles of the variant's own tile size."""
    t = _tile(variant)
    m, n, k = 2 * t, 3 * t, 64
    a, b, expected = _int_on(gpu, m, n, k)
    poison = torch.tensor([float("nan"), float("inf"), float("-inf")], device=gpu).repeat(m * n // 3 + 1)[:m * n]
    out = ops.sgemm_out(a, b, poison.view(m, n).clone(), alpha=1.0, beta=0.0, variant=variant)
    so.assert_exact(out, expected, f"variant {variant} beta=0 on NaN/Inf C")
    so.assert_exact(out, ops.sgemm(a, b, variant=variant), f"variant {variant} sgemm_out vs sgemm")
    c0 = so.small_ints((m, n), seed=61).to(gpu)
    for alpha, beta in ((1.0, 1.0), (-2.0, 1.0), (0.5, -1.0), (0.0, 0.25)):
        want = (alpha * expected.double() + beta * c0.double()).float()
        out = ops.sgemm_out(a, b, c0.clone(), alpha=alpha, beta=beta, variant=variant)
        so.assert_exact(out, want, f"variant {variant} alpha={alpha} beta={beta}")


# ------------------------------------------------------------ 7. input contract of ops.sgemm
def _misaligned(x):
    buf = torch.empty(x.numel() + 1, device=x.device)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("variant", VARIANTS)
def test_ops_sgemm_input_contract(gpu, variant):
    """ops.sgemm takes any view: contiguous but not 16-B aligned, transposed, column-sliced, expanded (row stride 0).
    Each gives the product of the materialised operands."""
    m, n, k = 256, 256, 64
    a, b, expected = _int_on(gpu, m, n, k)
    cases = {
        "misaligned a": (_misaligned(a), b),
        "misaligned b": (a, _misaligned(b)),
        "misaligned a and b": (_misaligned(a), _misaligned(b)),
        "a.t()": (a.t().contiguous().t(), b),
        "b.t()": (a, b.t().contiguous().t()),
        "a[:, ::2]": (torch.stack((a, a + 1), dim=2).view(m, 2 * k)[:, ::2], b),
    }
    for name, (x, y) in cases.items():
        so.assert_exact(ops.sgemm(x, y, variant=variant), expected, f"variant {variant} {name}")
    arow, brow = a[3], b[5]
    ea, eb = arow.expand(m, k), brow.expand(k, n)
    assert ea.stride(0) == 0 and eb.stride(0) == 0
    so.assert_exact(ops.sgemm(ea, b, variant=variant), (arow.double() @ b.double()).float().expand(m, n),
                    f"variant {variant} expanded a")
    so.assert_exact(ops.sgemm(a, eb, variant=variant), (a.double().sum(1, keepdim=True) * brow.double()).float(),
                    f"variant {variant} expanded b")


# ------------------------------------------------------------ 8. refusals through the C ABI
def _err_arg():
    header = Path(__file__).resolve().parents[1] / "csrc" / "include" / "pcmx_errors.h"
    return int(re.search(r"PCMX_ERR_ARG\s*=\s*(-?\d+)", header.read_text()).group(1))


def _abi_call(variant, A, B, C, m, n, k, lda, ldb, ldc, alpha=1.0, beta=0.0):
    """pcmx_sgemm_f32_variant (variant None: pcmx_sgemm_f32, the default dispatch) on raw addresses."""
    from parallel_c_programs_amd._native import hip_lib

    lib = hip_lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [ctypes.c_void_p(A), ctypes.c_void_p(B), ctypes.c_void_p(C), *map(ctypes.c_int, (m, n, k, lda, ldb, ldc)),
            ctypes.c_float(alpha), ctypes.c_float(beta)]
    if variant is None:
        rc = lib.pcmx_sgemm_f32(*args, stream)
    else:
        rc = lib.pcmx_sgemm_f32_variant(*args, ctypes.c_int(variant), stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("variant", [0, 1, 16, 17, 18, 20, None])
def test_c_abi_refusals(gpu, variant):
    """Each malformed call returns PCMX_ERR_ARG and leaves a sentinel-filled C untouched. Every buffer holds the
    rounded-up tile shape at the largest leading dimension used, so a missing check shows as a written C, never as an
    access outside an allocation. Variants 0 / 1 store C by the element: ldc % 4 and a C pointer off by 4 bytes are
    legal there and must give the exact product."""
    err = _err_arg()
    t = 128 if variant in (1, None) else 256
    m = n = t
    k = 64
    side = 2 * 256 + 64
    a, b, expected = _int_on(gpu, m, n, k)
    abuf = torch.zeros(side * side, device=gpu)
    bbuf = torch.zeros(side * side, device=gpu)
    abuf[:m * k].view(m, k).copy_(a)
    bbuf[:k * n].view(k, n).copy_(b)
    cbuf = torch.full((side * side,), SENTINEL, device=gpu)
    A, B, C = abuf.data_ptr(), bbuf.data_ptr(), cbuf.data_ptr()
    assert A % 16 == 0 and B % 16 == 0 and C % 16 == 0

    assert _abi_call(variant, A, B, C, m, n, k, k, n, n) == 0  # the well-formed call, so the harness itself is checked
    so.assert_exact(cbuf[:m * n].view(m, n), expected, f"variant {variant} well-formed")
    cbuf.fill_(SENTINEL)

    store16 = variant in (16, 17, 18, 20)
    bad = {
        "M % tile": (A, B, C, m + 4, n, k, k, n, n),
        "N % tile": (A, B, C, m, n + 4, k, k, n + 4, n + 4),
        "K % 32": (A, B, C, m, n, k + 16, k + 16, n, n),
        "lda % 4": (A, B, C, m, n, k, k + 2, n, n),
        "ldb % 4": (A, B, C, m, n, k, k, n + 2, n),
        "A off by 4 bytes": (A + 4, B, C, m, n, k, k, n, n),
        "B off by 4 bytes": (A, B + 4, C, m, n, k, k, n, n),
        "lda < K": (A, B, C, m, n, k, k - 4, n, n),
        "lda == 0": (A, B, C, m, n, k, 0, n, n),
        "ldb < N": (A, B, C, m, n, k, k, n - 4, n),
        "ldc < N": (A, B, C, m, n, k, k, n, n - 4),
        "M == 0": (A, B, C, 0, n, k, k, n, n),
    }
    if variant in (17, 18):
        bad["K % 64"] = (A, B, C, m, n, 96, 96, n, n)
    if store16:
        bad["ldc % 4"] = (A, B, C, m, n, k, k, n, n + 2)
        bad["C off by 4 bytes"] = (A, B, C + 4, m, n, k, k, n, n)
    for name, args in bad.items():
        assert _abi_call(variant, *args) == err, f"variant {variant}: {name} accepted"
        assert bool((cbuf == SENTINEL).all()), f"variant {variant}: {name} wrote C"
    if not store16:
        for name, cptr, ldc, off in (("ldc % 4", C, n + 2, 0), ("C off by 4 bytes", C + 4, n, 1)):
            assert _abi_call(variant, A, B, cptr, m, n, k, k, n, ldc) == 0, name
            so.assert_exact(cbuf[off:off + m * ldc].view(m, ldc)[:, :n], expected, f"variant {variant} {name}")
            cbuf.fill_(SENTINEL)


def test_c_abi_unknown_variant_refused(gpu):
    err = _err_arg()
    m = n = 256
    k = 64
    a, b, _ = _int_on(gpu, m, n, k)
    c = torch.full((m, n), SENTINEL, device=gpu)
    for variant in (2, 15, 19, 21, 99, -1, -7):
        assert _abi_call(variant, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, k, n, n) == err, variant
        assert bool((c == SENTINEL).all()), variant
