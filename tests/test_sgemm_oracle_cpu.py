"""The SGEMM oracle on the CPU: the split model is exact over its stated range, the operand families have the
properties the GPU tests rely on, and the assertion functions of tests/_sgemm_oracle.py accept the unmutated x6 model
and reject each of nine mutants of it (a dropped product, a wrong pairing, swapped planes). The host GEMM runs the
ragged integer shapes of the GPU tests."""
import pytest
import torch

import _sgemm_oracle as so
from parallel_c_programs_amd import ops


def _bits(x):
    return x.view(torch.int32)


# ------------------------------------------------------------ the split
def test_split3_sums_back_bit_for_bit_over_its_range():
    g = torch.Generator().manual_seed(1)
    lo = torch.tensor([so.SPLIT_MIN]).view(torch.int32).item()
    bits = torch.randint(lo, so.SPLIT_MAX_BITS + 1, (1 << 20,), generator=g, dtype=torch.int64).to(torch.int32)
    bits[:4] = torch.tensor([lo, lo + 1, so.SPLIT_MAX_BITS - 1, so.SPLIT_MAX_BITS], dtype=torch.int32)
    for sign in (1.0, -1.0):
        x = bits.view(torch.float32) * sign
        p0, p1, p2 = so.split3(x)
        for p in (p0, p1, p2):  # each plane is a bf16
            assert torch.equal(p, so.bf16(p))
        assert torch.equal(_bits((p0 + p1) + p2), _bits(x))  # both partial sums are exact in f32
        assert torch.equal(_bits(p0.double() + p1.double() + p2.double()).view(torch.int64),
                           _bits(x.double()).view(torch.int64))


def test_split3_upper_limit_is_0x7f7f7fff():
    """One ulp above the documented limit bf16 rounds to infinity and the planes no longer sum to x."""
    above = torch.tensor([so.SPLIT_MAX_BITS + 1, 0x7F7FFFFF], dtype=torch.int32).view(torch.float32)
    assert above.isfinite().all()
    p0, p1, p2 = so.split3(above)
    assert p0.isinf().all() and (p0 + p1 + p2).isnan().all()
    top = torch.tensor([so.max_split_float()])
    assert torch.equal(sum(so.split3(top)), top)


def test_operand_families():
    x = so.sig16((256, 256), seed=3)
    p0, p1, p2 = so.split3(x)
    assert not p2.any() and torch.equal(p0 + p1, x)
    assert (p1 != 0).float().mean().item() > 0.99
    y = so.full_mantissa((256, 256), seed=4)  # asserts p1 / p2 occupancy itself
    assert (so.split3(y)[2] != 0).float().mean().item() >= 0.80
    z = so.small_ints((64, 2048), seed=5)
    assert z.abs().max().item() == 8 and torch.equal(z, z.round())
    assert 2048 * 8 * 8 <= 1 << 17  # every partial sum is an integer of at most 18 bits
    for low in (True, False):
        r = so.range_end_values(256, low, seed=6)
        assert r.isfinite().all()
        assert ((r.abs() >= so.SPLIT_MIN) & (_bits(r.abs()) <= so.SPLIT_MAX_BITS)).all()
        assert torch.equal(sum(so.split3(r)), r)


@pytest.mark.parametrize("k,n", [(256, 256), (512, 256), (96, 256), (100, 30)])
def test_selectors_cover_every_k(k, n):
    seen = torch.zeros(k, dtype=torch.bool)
    for part in range(so.selector_parts(k, n)):
        s, rows, vals = so.selector(k, n, seed=7, part=part)
        assert ((s != 0).sum(0) == 1).all()  # one entry per column
        assert torch.equal(s[rows, torch.arange(n)], vals)
        assert torch.equal(vals.abs(), torch.exp2(torch.log2(vals.abs()).round()))  # powers of two
        seen[rows] = True
    assert seen.all()
    a = so.full_mantissa((8, k), seed=8)
    s, rows, vals = so.selector(k, n, seed=7)
    assert torch.equal((a.double() @ s.double()).float(), a[:, rows] * vals)  # a single exact product per output


# ------------------------------------------------------------ mutation checks
def _x6_checks(products):
    """Every x6 assertion of test_gpu_sgemm.py, run on x6_model(products) in place of the kernel. Returns the names of
    the assertions that failed."""
    failed = []

    def run(name, f):
        try:
            f()
        except AssertionError:
            failed.append(name)

    m = n = k = 64
    a_full, b_full = so.full_mantissa((m, k), seed=11), so.full_mantissa((k, n), seed=12)
    sel_b, rows, vals = so.selector(k, n, seed=13)
    run("selector_b", lambda: so.assert_exact(so.x6_model(a_full, sel_b, products), a_full[:, rows] * vals))
    sel_a, cols, avals = so.selector(k, m, seed=14)
    run("selector_a", lambda: so.assert_exact(so.x6_model(sel_a.t(), b_full, products), avals[:, None] * b_full[cols]))
    for fam in (so.sig16, so.full_mantissa):
        av = fam((m,), seed=15)
        a1, cols1, _ = so.selector(k, m, seed=16, values=av)
        bd = fam((k, n), seed=17)
        run(f"single_product_{fam.__name__}",
            lambda: so.assert_single_product(so.x6_model(a1.t(), bd, products), av, bd[cols1]))
    for kk in (32, 96):
        a, b = so.full_mantissa((128, kk), seed=18 + kk), so.full_mantissa((kk, 128), seed=19 + kk)
        run(f"dense_rms_k{kk}", lambda: so.assert_dense_rms(so.x6_model(a, b, products), so.x6_model(a, b), a, b))
    return failed


def test_unmutated_model_passes_every_x6_assertion():
    assert _x6_checks(so.SIX) == []
    assert len(so.MUTANTS) == 9 and len(set(so.MUTANTS.values())) == 9


@pytest.mark.parametrize("name", sorted(so.MUTANTS))
def test_each_mutant_is_rejected(name):
    failed = _x6_checks(so.MUTANTS[name])
    assert failed, f"mutant {name} passes every assertion"
    if name in so.TOUCH_LOW:
        assert {"dense_rms_k32", "dense_rms_k96", "single_product_full_mantissa"} <= set(failed), failed


@pytest.mark.parametrize("k", [32, 96])
def test_low_product_mutants_miss_the_dense_rms_bound_by_2x(k):
    """Measured: a mutant's rms is 48-75x the model's at K = 32 and 25-39x at K = 96 (the margin is 4x); its max
    error, 4e-6 to 1.2e-5 on these wide-exponent operands, is what the old 4e-6 bound sees only now and then."""
    a, b = so.full_mantissa((128, k), seed=18 + k), so.full_mantissa((k, 128), seed=19 + k)
    _, _, model_rms = so.scaled_error(so.x6_model(a, b), a, b)
    for name in so.TOUCH_LOW:
        _, mut_max, mut_rms = so.scaled_error(so.x6_model(a, b, so.MUTANTS[name]), a, b)
        print(f"K={k} {name}: rms {mut_rms / model_rms:.1f}x model, max {mut_max:.2e}")
        assert mut_rms >= 2 * so.DENSE_MARGIN * model_rms, (name, mut_rms / model_rms)


def test_low_product_mutants_miss_the_single_product_bound():
    """Measured: the model's largest single-product error is 1.62 ulp; with a low product gone most outputs are off by
    more than 8 ulp."""
    m = n = k = 128
    av = so.full_mantissa((m,), seed=21)
    a1, cols, _ = so.selector(k, m, seed=22, values=av)
    bd = so.full_mantissa((k, n), seed=23)
    ok = so.assert_single_product(so.x6_model(a1.t(), bd), av, bd[cols])
    print(f"model single-product max {ok:.2f} ulp")
    assert ok < 2.0
    for name in so.TOUCH_LOW:
        c = so.x6_model(a1.t(), bd, so.MUTANTS[name])
        with pytest.raises(AssertionError):
            so.assert_single_product(c, av, bd[cols])


def test_f32_chain_model_is_an_f32_chain():
    a, b = so.small_ints((16, 64), seed=24), so.small_ints((64, 16), seed=25)
    so.assert_exact(so.f32_chain_model(a, b), (a.long() @ b.long()).float())
    a, b = so.full_mantissa((64, 96), seed=26), so.full_mantissa((96, 64), seed=27)
    _, fmax, frms = so.scaled_error(so.f32_chain_model(a, b), a, b)
    assert 0 < frms < so.U and fmax < so.existing_max_bound(96)


# ------------------------------------------------------------ host GEMM
@pytest.mark.parametrize("shape", [(257, 255, 33), (1, 1, 1), (100, 70, 33), (65, 63, 17), (300, 200, 100)])
def test_host_sgemm_integer_exact_ragged(shape):
    m, n, k = shape
    a, b = so.small_ints((m, k), seed=m), so.small_ints((k, n), seed=n + 1)
    expected = (a.long() @ b.long()).float()
    so.assert_exact(ops.sgemm(a, b), expected, "host")
    so.assert_exact(ops.sgemm(a.t().contiguous().t(), b[:, :].t().contiguous().t()), expected, "host, strided")
    so.assert_exact(ops.sgemm_naive_host(a, b), expected, "naive host")
