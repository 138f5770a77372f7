"""The arithmetic of mc_mandelbrot_orbit_create_device without a GPU: the shared header's product and rounding
(csrc/mandel_orbit_fix.h, run as lane loops on the CPU through libmc_compute_test.so) against Python integers, its to_double against
fractions.Fraction, the whole iteration as lane loops against the host constructor, and the argument checks that need no device."""
import ctypes as C
import fractions
import random
import struct

import numpy as np
import pytest

import mandel_orbit_device_cases as K

KS = (1, 2, 3, 17, 64, 65, 130)


@pytest.fixture(scope="module")
def T(B):
    return B.test_lib()


def host_mul(T, k, a, b):
    A, Bv, out = K.limbs(a, k), K.limbs(b, k), np.zeros(k + 1, np.uint64)
    assert T.mc_hook_orbit_mul_host(k, A.ctypes.data, Bv.ctypes.data, out.ctypes.data) == 0
    return K.value(out)


@pytest.mark.parametrize("k", KS)
def test_product_random(T, k):
    rng = random.Random(1000 + k)
    for _ in range(200):
        a, b = K.random_operand(rng, k), K.random_operand(rng, k)
        assert host_mul(T, k, a, b) == K.rounded_product(a, b, k)


@pytest.mark.parametrize("k", KS)
def test_product_crafted(T, k):
    for name, a, b in K.crafted_operands(k):
        assert host_mul(T, k, a, b) == K.rounded_product(a, b, k), (k, name)


def test_product_refuses_bad_k(T):
    z = np.zeros(140, np.uint64)
    for k in (0, -1, 131):
        assert T.mc_hook_orbit_mul_host(k, z.ctypes.data, z.ctypes.data, z.ctypes.data) == 1


def to_double(T, k, v, neg=0):
    out = C.c_double(0.0)
    assert T.mc_hook_orbit_to_double_host(k, K.limbs(v, k).ctypes.data, neg, C.byref(out)) == 0
    return out.value


def same_bits(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b)


@pytest.mark.parametrize("k", (1, 2, 16, 17, 18, 54, 130))
def test_to_double_against_fraction(T, k):
    F = 64 * k
    rng = random.Random(2000 + k)
    values = [0, 1, (1 << (F + 64)) - 1, 1 << F, (1 << F) - 1]
    for _ in range(300):
        nbits = rng.randrange(1, F + 64)
        v = rng.getrandbits(nbits) | (1 << (nbits - 1))
        kind = rng.randrange(4)
        if kind == 1 and nbits > 60:      # a short mantissa: exact, or a tie once the half bit is set
            v = (v >> (nbits - 54)) << (nbits - 54)
        elif kind == 2:                   # all ones: the carry out of the mantissa
            v = (1 << nbits) - 1
        elif kind == 3 and nbits > 70:    # half bit set, sticky one bit far below
            v = ((v >> (nbits - 54) | 1) << (nbits - 54)) | rng.randrange(2)
        values.append(v)
    for v in values:
        want = float(fractions.Fraction(v, 1 << F))
        assert same_bits(to_double(T, k, v), want), (k, hex(v))
        assert same_bits(to_double(T, k, v, 1), -want if v else 0.0), (k, hex(v))


def test_to_double_subnormal_and_mantissa_carry(T):
    k = 18                                # F = 1152: the quantum 2^-1074 is bit 78
    F = 64 * k
    q = F - 1074
    cases = {
        "subnormal, exact": 0x123456789 << q,
        "subnormal, rounds up": (0x123456789 << q) | (1 << (q - 1)) | 1,
        "subnormal tie to even (down)": (0x123456788 << q) | (1 << (q - 1)),
        "subnormal tie to even (up)": (0x123456789 << q) | (1 << (q - 1)),
        "half the quantum: ties to zero": 1 << (q - 1),
        "just above half the quantum": (1 << (q - 1)) | 1,
        "below half the quantum": (1 << (q - 1)) - 1,
        "largest subnormal rounds to the smallest normal": ((1 << 52) - 1) << q | (1 << (q - 1)),
        "carry out of the mantissa": ((1 << 54) - 1) << 500,
        "carry out of the mantissa into the integer limb": ((1 << 60) - 1) << (F - 60),
    }
    for name, v in cases.items():
        want = float(fractions.Fraction(v, 1 << F))
        assert same_bits(to_double(T, k, v), want), name
    assert to_double(T, k, 0x123456789 << q) < 2.0 ** -1022
    assert same_bits(to_double(T, k, (1 << (q - 1)) - 1, 1), -0.0)      # the host's -0.0 for a negative value that rounds to zero
    assert to_double(T, k, ((1 << 54) - 1) << 500) == 2.0 ** (554 - F)


def lanes_orbit(B, T, cx, cy, m, E, M):
    h = C.c_void_p()
    rc = T.mc_hook_orbit_create_lanes_host(cx.encode(), cy.encode(), m, m, E, M, C.byref(h))
    if rc:
        return rc, B.lib().mc_last_error_detail().decode()
    L = B.lib()
    n, mi, bits = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert L.mc_mandelbrot_orbit_info(h, C.byref(n), C.byref(mi), C.byref(bits)) == 0
    Z = np.empty((n.value + 1, 2), np.float64)
    assert L.mc_mandelbrot_orbit_copy(h, Z.ctypes.data) == 0
    L.mc_mandelbrot_orbit_destroy(h)
    return n.value, mi.value, bits.value, Z


@pytest.mark.parametrize("k", (2, 17, 18, 65, 130))
def test_lane_loops_make_the_host_orbit(B, T, k):
    """The kernel's phases, lane by lane on the CPU: the same table as FixOps, every sign path, escape and exact zeros included."""
    E = K.exp2_for(k)
    for cx, cy, M in (("-0.1", "0.2", 200), ("0.1", "-0.2", 60), ("-0.75", "0.01", 400), ("-2", "0", 5), ("0", "0", 20), ("-1", "0", 20),
                      ("0", "1", 20), ("0.26", "-0.001", 60), ("-0.75", "3e-320", 40)):
        with B.Orbit(cx, cy, 1.0, 1.0, M, E) as o:
            assert (o.bits + 63) // 64 == k
            got = lanes_orbit(B, T, cx, cy, 1.0, E, M)
            assert got[:3] == (o.length, o.max_iter, o.bits), (cx, cy)
            assert np.array_equal(got[3].view(np.uint64), o.table().view(np.uint64)), (cx, cy)


def test_entry_points_without_a_device(B):
    L = B.lib()
    h = C.c_void_p()
    assert L.mc_mandelbrot_orbit_create_device(None, b"-0.75", b"0.1", 1.0, 1.0, -3000, 10, C.byref(h)) == 1
    assert not h.value
    assert L.mc_last_error_detail().decode().startswith("mc_mandelbrot_orbit_create_device: ")
    ms, n, limbs = C.c_double(0), C.c_uint32(0), C.c_uint32(0)
    assert L.mc_context_last_orbit_timing(None, C.byref(ms), C.byref(n), C.byref(limbs)) == 1
    assert L.mc_context_last_orbit_timing(None, None, None, None) == 1
    assert "mc_mandelbrot_orbit_create_device" in B.declared_symbols() and "mc_context_last_orbit_timing" in B.declared_symbols()
