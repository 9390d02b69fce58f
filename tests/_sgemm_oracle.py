"""CPU models, operand families and assertion functions for the SGEMM tests (torch only, no GPU).

The GPU tests (test_gpu_sgemm.py) call the assertion functions on kernel output; test_sgemm_oracle_cpu.py calls the
same functions on `x6_model` and on nine mutants of it, which is the proof that they discriminate.

Models
  split3(x)             the x6 kernel's operand split: p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1)
  x6_model(a, b, ...)   sgemm_x6.hip: per 16-k step the six piece products, smallest first (kPA / kPB), each one MFMA
                        = an exact (fp64) 16-term dot product and ONE f32 rounding into the accumulator
  f32_chain_model(a, b) sgemm.hip: a sequential f32 chain, two k per v_mfma_f32_32x32x2_f32, one rounding per MFMA
The hardware may round after every k inside an MFMA (up to 16 times per bf16 MFMA): at most sqrt(16) = 4x the model
in rms, which is the margin of `assert_dense_rms`.

Every generator is seeded and returns CPU tensors; the GPU tests move them with `.to(device)`.
"""
from __future__ import annotations

import torch

# (plane of A, plane of B) in the kernel's accumulation order: smallest first
SIX = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))
LOW = ((2, 0), (1, 1), (0, 2))  # the three products of weight 2^-16: invisible to a 4e-6 bound

U = 2.0 ** -24                   # unit roundoff of f32
SPLIT_MIN = 2.0 ** -110          # the split is exact on [SPLIT_MIN, SPLIT_MAX]
SPLIT_MAX_BITS = 0x7F7F7FFF      # bf16 round-to-nearest sends 0x7f7f8000 and above to infinity
SINGLE_PRODUCT_ULPS = 8.0        # see assert_single_product
DENSE_MARGIN = 4.0               # see module docstring


def _swap12(products):
    return tuple(({1: 2, 2: 1}.get(i, i), j) for i, j in products)


def _replace(products, old, new):
    return tuple(new if p == old else p for p in products)


# The nine mutants: each product dropped, two wrong pairings (a product issued twice in place of its partner), and
# planes 1 and 2 of A swapped. TOUCH_LOW names those whose error is of the order 2^-16 |a||b| only.
MUTANTS = {f"drop_a{i}b{j}": tuple(p for p in SIX if p != (i, j)) for i, j in SIX}
MUTANTS["a1b0_twice_for_a0b1"] = _replace(SIX, (0, 1), (1, 0))
MUTANTS["a1b1_twice_for_a0b2"] = _replace(SIX, (0, 2), (1, 1))
MUTANTS["a_planes_1_2_swapped"] = _swap12(SIX)
TOUCH_LOW = ("drop_a2b0", "drop_a1b1", "drop_a0b2", "a1b1_twice_for_a0b2", "a_planes_1_2_swapped")


def max_split_float() -> float:
    return torch.tensor([SPLIT_MAX_BITS], dtype=torch.int32).view(torch.float32).item()


def bf16(x: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even to bf16, returned as f32 (v_cvt_pk_bf16_f32)."""
    return x.to(torch.bfloat16).to(torch.float32)


def split3(x: torch.Tensor):
    assert x.dtype == torch.float32
    p0 = bf16(x)
    r = x - p0
    p1 = bf16(r)
    return p0, p1, bf16(r - p1)


def x6_model(a: torch.Tensor, b: torch.Tensor, products=SIX, kstep: int = 16) -> torch.Tensor:
    a, b = a.cpu(), b.cpu()
    k = a.shape[1]
    pad = -k % kstep  # ops.sgemm zero-pads K; zeros split to zeros
    if pad:
        a = torch.nn.functional.pad(a, (0, pad))
        b = torch.nn.functional.pad(b, (0, 0, 0, pad))
    pa = [p.double() for p in split3(a)]
    pb = [p.double() for p in split3(b)]
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k0 in range(0, k + pad, kstep):
        for i, j in products:
            acc = (acc.double() + pa[i][:, k0:k0 + kstep] @ pb[j][k0:k0 + kstep]).float()
    return acc


def f32_chain_model(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    ad, bd = a.cpu().double(), b.cpu().double()
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k0 in range(0, a.shape[1], 2):
        acc = (acc.double() + ad[:, k0:k0 + 2] @ bd[k0:k0 + 2]).float()
    return acc


def scaled_error(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor):
    """Per-element |c - fp64 product| / sum_k |a||b|, its max and its rms."""
    ad, bd = a.cpu().double(), b.cpu().double()
    e = (c.cpu().double() - ad @ bd).abs() / (ad.abs() @ bd.abs()).clamp_min(1e-300)
    return e, e.max().item(), e.pow(2).mean().sqrt().item()


# ------------------------------------------------------------ operand families
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _pow2(shape, g, emin, emax) -> torch.Tensor:
    return torch.ldexp(torch.ones(shape), torch.randint(emin, emax + 1, shape, generator=g))


def _sign(shape, g) -> torch.Tensor:
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def small_ints(shape, seed: int = 0) -> torch.Tensor:
    """Integers in [-8, 8]: with K <= 2048 no partial sum exceeds 2^17, so every summation order is exact."""
    return torch.randint(-8, 9, shape, generator=_gen(seed)).float()


def full_mantissa(shape, seed: int = 0, emin: int = -4, emax: int = 4) -> torch.Tensor:
    """(rand + 0.5) * sign * 2^e: all 24 significand bits in use, so all three planes of the split are live."""
    g = _gen(seed)
    x = (torch.rand(shape, generator=g) + 0.5) * _sign(shape, g) * _pow2(shape, g, emin, emax)
    _, p1, p2 = split3(x)
    if x.numel() >= 4096:  # occupancy of the planes (a smaller draw is too noisy to judge)
        assert (p1 != 0).float().mean().item() > 0.99
        assert (p2 != 0).float().mean().item() >= 0.80
    return x


def sig16(shape, seed: int = 0, emin: int = -4, emax: int = 4) -> torch.Tensor:
    """16-bit significands: p2 == 0 everywhere and p1 != 0 for 255/256 of the values, so a product of two of them
    is a0 b0 + a0 b1 + a1 b0 + a1 b1 exactly and a1 b1 is the only term of weight 2^-16."""
    g = _gen(seed)
    x = (torch.randint(1 << 15, 1 << 16, shape, generator=g).float() * _sign(shape, g)
         * _pow2(shape, g, emin - 15, emax - 15))
    _, p1, p2 = split3(x)
    assert not p2.any()
    if x.numel() >= 4096:
        assert (p1 != 0).float().mean().item() > 0.99
    return x


def pow2_dense(shape, seed: int, emin: int, emax: int) -> torch.Tensor:
    """+-2^e, e uniform in [emin, emax]: a partner that scales without rounding."""
    g = _gen(seed)
    return _sign(shape, g) * _pow2(shape, g, emin, emax)


def selector_parts(k: int, n: int) -> int:
    """How many selectors of n columns it takes to pick every one of k rows."""
    return -(-k // n)


def selector(k: int, n: int, seed: int = 0, part: int = 0, values: torch.Tensor | None = None):
    """A k x n matrix with ONE nonzero per column: column c holds values[c] (default: a random +-2^e, |e| <= 8) at
    row pi[(part * n + c) % k], pi a seeded permutation of the k rows. A @ selector picks (and scales) columns of A;
    parts 0 .. selector_parts(k, n) - 1 together pick every k. Returns (matrix, rows, values); the transposed matrix
    is the A-side form (one nonzero per row)."""
    g = _gen(seed)
    pi = torch.randperm(k, generator=g)
    rows = pi[(part * n + torch.arange(n)) % k]
    if values is None:
        values = _sign((n,), g) * _pow2((n,), g, -8, 8)
    s = torch.zeros(k, n)
    s[rows, torch.arange(n)] = values
    return s, rows, values


def range_end_values(n: int, low: bool, seed: int = 0) -> torch.Tensor:
    """Full-mantissa values at an end of the split's range: |x| in [2^-110, 2^-100) or in [2^120, 0x7f7f7fff], the two
    limits themselves included."""
    g = _gen(seed)
    m = (torch.rand(n, generator=g) + 1.0) * _sign((n,), g)  # [1, 2)
    if low:
        x = m * _pow2((n,), g, -110, -101)
        x[0], x[1] = SPLIT_MIN, -SPLIT_MIN
    else:
        x = (m * _pow2((n,), g, 120, 127)).clamp(-max_split_float(), max_split_float())
        x[0], x[1] = max_split_float(), -max_split_float()
    return x


# ------------------------------------------------------------ assertion functions
def assert_exact(c: torch.Tensor, expected: torch.Tensor, what: str = "") -> None:
    """Bit-for-bit (integer-valued operands, or a single product by a power of two)."""
    if not torch.equal(c, expected):
        bad = (c != expected) | (c.isnan() != expected.isnan())
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {c.numel()} elements differ, first at {idx}: "
                             f"{c[tuple(idx)].item()!r} != {expected[tuple(idx)].item()!r}")


def single_product_ulps(c: torch.Tensor, a_vals: torch.Tensor, b_rows: torch.Tensor) -> float:
    """max |c[r, :] - a_vals[r] * b_rows[r, :]| / |a_vals[r] * b_rows[r, :]| in units of 2^-24."""
    ref = a_vals.cpu().double()[:, None] * b_rows.cpu().double()
    return ((c.cpu().double() - ref).abs() / ref.abs()).max().item() / U


def assert_single_product(c: torch.Tensor, a_vals: torch.Tensor, b_rows: torch.Tensor, what: str = "") -> float:
    """Every output is ONE product a * b computed as six exact piece products: at most five roundings of partial sums
    no larger than |ab| (1 + 2^-7), plus the three dropped products (two of weight 2^-24 |ab|, one of 2^-32):
    5 (1 + 2^-7) 2^-24 + 2 * 2^-24 + 2^-32 < 8 * 2^-24 relative."""
    ulps = single_product_ulps(c, a_vals, b_rows)
    assert ulps <= SINGLE_PRODUCT_ULPS, f"{what}: single-product error {ulps:.2f} ulp > {SINGLE_PRODUCT_ULPS}"
    return ulps


def existing_max_bound(k: int) -> float:
    """The bound of test_gpu_core.py's dense tests, kept as the bound on the max."""
    return 4e-6 * max(1.0, (k / 256) ** 0.5)


def assert_dense_rms(c: torch.Tensor, model_c: torch.Tensor, a: torch.Tensor, b: torch.Tensor, what: str = ""):
    """rms of the scaled error at most DENSE_MARGIN x the model's on the same operands; max under the old bound.
    Returns (kernel rms / model rms, kernel max, model max)."""
    _, cmax, crms = scaled_error(c, a, b)
    _, mmax, mrms = scaled_error(model_c, a, b)
    ratio = crms / mrms
    assert ratio <= DENSE_MARGIN, f"{what}: rms {crms:.3e} is {ratio:.2f}x the model's {mrms:.3e} (> {DENSE_MARGIN}x)"
    assert cmax < existing_max_bound(a.shape[1]), f"{what}: max scaled error {cmax:.3e}"
    return ratio, cmax, mmax
