"""The device functions of csrc/mc_math.h and csrc/ds_arith.h over the whole fp32 range, through the hooks of libmc_compute_test.so.

PARITY: bit for bit against the oracle (sin, cos, log2, exp2, pow, the two-float packages) and against numpy's IEEE arithmetic (sqrt,
1 / sqrt, 1 / x, the shared-divisor division) on tests/math_edge_cases.py's strata — zeros of both signs, subnormals, inf, NaN, every
exponent, unnormalised pairs, overflow inside the Dekker split, underflowing products — in sorted order (homogeneous waves: the short forms
run) and in a fixed shuffle (every wave mixes lanes inside and outside the short forms' window).  The one allowance: two NaNs are equal
whatever their sign or payload.  Zero signs must match.

ACCURACY: tests/test_math_accuracy_host.py's assertion functions applied to the DEVICE's outputs directly, so the GPU check against the
mathematics does not rest on the parity tests having passed.

Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

import math_edge_cases as E

pytestmark = pytest.mark.gpu

ORDERS = ("sorted", "shuffled")


def strata(order):
    srt, sh = E.fp32_strata()
    if order == "shuffled":   # the inputs do mix inside and outside the window within waves: in every wave
        assert E.waves_mixing_the_window(sh) == sh.size // 64
        return sh
    assert E.waves_mixing_the_window(srt) == 0
    return srt


# ---------------------------------------------------------------------------------------------------------------------------------------
# strict mc_test_math, fn 0..9
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fn", ["sin", "cos", "log2", "exp2", "pow045"])
def test_strict_math_equals_the_oracle_on_every_stratum(ctx, O, fn, order):
    x = strata(order)
    E.assert_same_bits(ctx.test_math(fn, x), O.mc_math(fn, x), f"{fn} ({order})", (x,))


@pytest.mark.parametrize("order", ORDERS)
def test_fused_sincos_equals_sin_and_cos_on_every_stratum(ctx, O, order):
    x = strata(order)
    E.assert_same_bits(ctx.test_math("sincos_s", x), O.mc_math("sin", x), f"sincos_s ({order})", (x,))
    E.assert_same_bits(ctx.test_math("sincos_c", x), O.mc_math("cos", x), f"sincos_c ({order})", (x,))


def test_sincos_beyond_the_int32_quadrant_range_equals_the_oracle(ctx, O):
    """|x| >= 2^31 * pi/2 ~ 3.37e9, inf, NaN: the quadrant conversion saturates / gives 0 on the device, and the oracle writes the same
    definition out (oracle_core.h quadrant_i32; tests/test_math_accuracy_host.py pins which definition that is)."""
    srt, _ = E.fp32_strata()
    x = srt[~(np.abs(srt) < 3.0e9)]
    assert np.isnan(x).any() and np.isinf(x).any() and (x > 3.37e9).sum() > 90 * 2048 and (x < -3.37e9).sum() > 90 * 2048
    for fn, ref in (("sin", "sin"), ("cos", "cos"), ("sincos_s", "sin"), ("sincos_c", "cos")):
        E.assert_same_bits(ctx.test_math(fn, x), O.mc_math(ref, x), f"{fn} beyond int32", (x,))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fn", ["sqrt", "rsqrt", "rcp"])
def test_strict_sqrt_rsqrt_rcp_are_ieee_on_every_stratum(ctx, fn, order):
    x = strata(order)
    E.assert_same_bits(ctx.test_math(fn, x), E.ieee(fn, x), f"{fn} ({order})", (x,))


# ---------------------------------------------------------------------------------------------------------------------------------------
# mc_test_ds_op, all thirteen ops
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["add", "sub", "mul", "compare", "sqrt", "df64_add", "df64_mult", "df64_sqrt", "twoprod", "div",
                                "twodiff", "df64_eqneq"])
def test_two_float_ops_equal_the_oracle_at_the_edges(ctx, O, op):
    a, b = E.ds_pairs()
    E.assert_same_bits(ctx.test_ds_op(op, a, b), O.ds_op(op, a, b), op, (a, b))


def test_ds_mul_fma_equals_the_dekker_product_inside_its_precondition_at_the_edges(ctx, O):
    """No oracle entry for the one-fma product: what tests/test_gpu_parity.py asserts of it (equal to the oracle's literal ds_mul up to
    the sign of a zero word), on the rows of ds_pairs() inside the stated precondition only."""
    a, b = E.ds_pairs()
    keep = E.mul_fma_precondition(a, b)
    assert keep.sum() >= 50000                       # the input set does leave rows of the precondition region in
    a, b = a[keep], b[keep]
    got, ref = ctx.test_ds_op("mul_fma", a, b), O.ds_op("mul", a, b)
    same = (E.bits(got) == E.bits(ref)) | ((got == 0) & (ref == 0))
    assert same.all(), int((~same).sum())


# ---------------------------------------------------------------------------------------------------------------------------------------
# mc_test_div3
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_y", [False, True])
def test_shared_divisor_division_is_ieee_with_mixed_lanes(ctx, with_y):
    a, s = E.div3_cases()
    with np.errstate(all="ignore"):
        want = a / s[:, None]
    # lanes inside div3's window ([2^-60, 2^60), numerators also +0) and outside it side by side in the waves
    def inside(x):
        return (E.bits(x) - np.uint32(0x21800000)) < np.uint32(0x3C000000)
    win = (inside(s) & (inside(a) | (E.bits(a) == 0)).all(1)).reshape(-1, 64)
    assert (win.any(1) & ~win.all(1)).mean() > 0.99
    E.assert_same_bits(ctx.test_div3(a, s, with_y=with_y), want, f"div3 with_y={with_y}", (a, s))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the careful tier: the short forms WITHOUT their window tests (mc_math.h fsqrt<2>, inversesqrt<2>, fdiv<2>)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fn", ["sqrt", "rsqrt", "rcp"])
def test_careful_tier_is_ieee_inside_its_stated_windows(ctx, fn, order):
    """Windows as mc_math.h states them: [2^-100, 2^100) for the square root and its reciprocal, [2^-60, 2^60) for the division 1 / x.
    Outside them nothing is asserted but the written exceptions (next test)."""
    x = strata(order)
    win = E.in_short_window(x) if fn != "rcp" else (E.bits(x) - np.uint32(0x21800000)) < np.uint32(0x3C000000)
    assert win.sum() >= 119 * 2048
    got = ctx.test_math(fn, x, fast=2)
    E.assert_same_bits(got[win], E.ieee(fn, x)[win], f"careful {fn} ({order})", (x[win],))


def test_careful_tier_sqrt_written_exceptions(ctx):
    """mc_math.h fsqrt<2>: -0 gives +0 (the reference keeps -0), +0 gives +0, a denormal argument gives NaN."""
    srt, _ = E.fp32_strata()
    den = srt[(srt > 0) & (srt < np.float32(1.17549435e-38))]
    assert den.size >= 2000 and den[0] == np.float32(1e-45)
    x = np.concatenate([np.array([-0.0, 0.0], np.float32), den])
    got = ctx.test_math("sqrt", x, fast=2)
    assert E.bits(got[:2]).tolist() == [0, 0]
    assert np.isnan(got[2:]).all(), int((~np.isnan(got[2:])).sum())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fast tier, on the domains the kernels feed: the bounds of tests/test_gpu_parity.py::test_fast_math_within_a_few_ulp
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_fast_tier_within_its_bounds_on_the_kernels_domains(ctx):
    x = E.fast_tier_domain()
    assert x.size == 200 * 2048
    x64 = x.astype(np.float64)
    for fn, ref in (("sqrt", np.sqrt(x64)), ("rcp", 1.0 / x64), ("rsqrt", 1.0 / np.sqrt(x64))):
        got = ctx.test_math(fn, x, fast=True).astype(np.float64)
        err = np.abs(got - ref) / ref
        print(f"fast {fn}: max relative error {err.max() / 2.0 ** -23:.3f} x 2^-23 at {x[np.argmax(err)]!r}")
        assert err.max() < 3 * 2.0 ** -23, fn
    ang = E.fast_tier_angles()
    assert ang.size == 127 * 2048 and ang.min() == 0.0 and ang.max() <= np.float32(2.0 * np.pi)
    for fn, ref in (("sin", np.sin(ang.astype(np.float64))), ("cos", np.cos(ang.astype(np.float64)))):
        err = np.abs(ctx.test_math(fn, ang, fast=True).astype(np.float64) - ref)
        print(f"fast {fn}: max absolute error {err.max():.3e} at {ang[np.argmax(err)]!r}")
        assert err.max() < 5e-6, fn


# ---------------------------------------------------------------------------------------------------------------------------------------
# accuracy against high precision, on the device's own outputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_device_scalar_functions_against_float64(ctx):
    E.check_scalar_accuracy(ctx.test_math)


def test_device_two_float_packages_against_float64(ctx):
    E.check_twofloat_accuracy(ctx.test_ds_op)


def test_device_two_float_exact_properties(ctx):
    E.check_exact_properties(ctx.test_ds_op)
