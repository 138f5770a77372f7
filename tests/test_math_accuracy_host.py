"""How far the project's fp32 math is from the mathematics — measured on the CPU oracle (oracle/oracle_core.h), which the strict device
functions equal bit for bit (tests/test_gpu_parity.py, tests/test_gpu_math_edges.py).  Every other check of these functions is
"device == oracle", and the oracle restates the same sequence: a wrong coefficient, a dropped error term or a mistyped constant copied to
both sides passes all of them.  Here the yardstick is numpy float64 (scalar functions), float64 and fractions.Fraction (two-float
packages).  Input sets, bounds and the assertion functions live in tests/math_edge_cases.py; tests/test_gpu_math_edges.py applies the same
functions to the device's outputs.  No GPU needed."""
import numpy as np

import math_edge_cases as E


def test_input_sets_are_what_they_claim():
    srt, sh = E.fp32_strata()
    assert srt.size == sh.size == 1 << 20 and np.array_equal(np.sort(E.bits(sh)), E.bits(srt))
    u = E.bits(srt)
    assert np.array_equal(np.unique((u >> 23) & 0xff), np.arange(256)) and {0, 0x80000000, 0x7f800000, 0xff800000} <= set(u[::1].tolist())
    assert (np.isnan(srt).sum(), np.isinf(srt).sum()) == (2 * 2047, 2)
    for m in E.CRAFTED_MANTISSAS:                                  # every crafted mantissa at every exponent, both signs
        assert (u & 0x007fffff == m).sum() >= 512
    assert E.waves_mixing_the_window(srt) == 0                     # sorted: every wave wholly inside or wholly outside
    assert E.waves_mixing_the_window(sh) == sh.size // 64          # shuffled: every wave mixes
    a, b = E.ds_pairs()
    assert a.shape == b.shape and a.shape[0] > 400000
    for p in (a, b):
        h, l = p[:, 0], p[:, 1]
        assert np.isnan(h).any() and np.isinf(h).any() and (E.bits(h) == 0x80000000).any() and (E.bits(h) == 0).any()
        assert ((h != 0) & (np.abs(h) < 1.17549435e-38)).any() and (np.abs(h) >= 2.0 ** 114).any()
        assert (np.isfinite(h) & (h != 0) & (np.abs(l) == np.abs(h))).any()          # unnormalised, |lo| = |hi|
    with np.errstate(all="ignore"):
        prod = np.abs(a[:, 0].astype(np.float64) * b[:, 0].astype(np.float64))
    assert ((prod > 0) & (prod < 2.0 ** -126)).sum() > 40000 and (prod == np.inf).any()
    assert 50000 <= E.mul_fma_precondition(a, b).sum() < a.shape[0] // 2
    assert (np.all(a == -b, 1)).sum() >= 20000 and np.all(E.bits(a) == E.bits(b), 1).sum() >= 20000


def test_scalar_functions_against_float64(O):
    measured = E.check_scalar_accuracy(O.mc_math)
    # the oracle's own maxima are recorded: the arithmetic has a fixed order, so they reproduce
    for key, (recorded, _) in E.SCALAR_BOUNDS.items():
        assert abs(measured[key] - recorded) < 1e-3, (key, measured[key], recorded)


def test_two_float_packages_against_float64(O):
    E.check_twofloat_accuracy(O.ds_op)


def test_two_float_exact_properties(O):
    E.check_exact_properties(O.ds_op)


def test_sincos_quadrant_conversion_saturates_beyond_int32(O):
    """|x * 2/pi| >= 2^31 (|x| >= ~3.37e9): the quadrant count k saturates (oracle_core.h quadrant_i32 — the definition of the device's
    conversion instruction), it is not whatever the host's out-of-range cast yields.  With k = INT32_MAX for x > 0 (bits 0 and 1 set,
    k + 1 wraps) and INT32_MIN for x < 0 (both clear), and the reduced argument odd in x, the definition reads
        sin(-x) = -cos(x)   and   cos(-x) = -sin(x)   bit for bit;
    a conversion that yields INT32_MIN on both sides (x86's) gives sin(-x) = -sin(x) instead.  Accuracy is NOT claimed out there."""
    srt, _ = E.fp32_strata()
    x = srt[(srt >= 2.0 ** 32) & np.isfinite(srt)]
    assert x.size > 90 * 2048
    s, c, sn, cn = O.mc_math("sin", x), O.mc_math("cos", x), O.mc_math("sin", -x), O.mc_math("cos", -x)
    E.assert_same_bits(sn, -c, "sin(-x) == -cos(x) beyond int32", (x,))
    E.assert_same_bits(cn, -s, "cos(-x) == -sin(x) beyond int32", (x,))
    fin = np.isfinite(s) & (s != 0)
    assert fin.sum() > 10000 and (E.bits(sn[fin]) != E.bits(-s[fin])).any()      # ... and it is not the odd symmetry of the in-range case
    small = srt[(np.abs(srt) < 3.0e9) & (srt != 0)]                                     # in range: sin odd (but sin(-0) = +0), cos even, as ever
    E.assert_same_bits(O.mc_math("sin", -small), -O.mc_math("sin", small), "sin odd in range", (small,))
    E.assert_same_bits(O.mc_math("cos", -small), O.mc_math("cos", small), "cos even in range", (small,))
    nan = np.array([np.nan, np.inf, -np.inf], np.float32)
    assert np.isnan(O.mc_math("sin", nan)).all() and np.isnan(O.mc_math("cos", nan)).all()
