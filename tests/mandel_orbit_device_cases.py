"""Operands and views shared by tests/test_mandel_orbit_device_host.py and tests/test_gpu_mandel_orbit_device.py: numbers of the device
orbit's fixed point as Python integers (k fractional 64-bit limbs and one integer limb), the rounded product they must give, and the
scale exponent that asks the constructors for a given limb count."""
import numpy as np

MASK64 = (1 << 64) - 1


def limbs(v, k):
    return np.array([(v >> (64 * i)) & MASK64 for i in range(k + 1)], np.uint64)


def value(a):
    return sum(int(x) << (64 * i) for i, x in enumerate(a))


def rounded_product(a, b, k):
    """FixOps::mul: the full product plus the first dropped bit, the k + 1 limbs from limb k on."""
    return ((a * b + (1 << (64 * k - 1))) >> (64 * k)) & ((1 << (64 * (k + 1))) - 1)


def random_operand(rng, k):
    return rng.getrandbits(64 * (k + 1))


def crafted_operands(k):
    """(name, a, b): all-ones limbs (the longest carry chain), a single set bit in every limb position, zero, and operands whose dropped
    half is exactly 0x8000...0, 0x7FFF...F and 0x8000...1 (the tie and its neighbours)."""
    import random
    rng = random.Random(77 + k)
    n, F = k + 1, 64 * k
    ones = (1 << (64 * n)) - 1
    out = [("all ones squared", ones, ones), ("all ones x one ulp", ones, 1), ("all ones x 1.0", ones, 1 << F),
           ("fraction all ones squared", (1 << F) - 1, (1 << F) - 1), ("zero x random", 0, random_operand(rng, k)),
           ("random x zero", random_operand(rng, k), 0), ("zero x zero", 0, 0)]
    other = random_operand(rng, k)
    for i in range(n):
        bit = 1 << (64 * i + rng.randrange(64))
        out.append((f"single bit in limb {i} x random", bit, other))
        out.append((f"random x single bit in limb {i}", other, bit))
        out.append((f"single bit in limb {i} x all ones", bit, ones))
    half = 1 << (F - 1)
    for name, low in (("tie", half), ("just below the tie", half - 1), ("just above the tie", half + 1)):
        for t in range(4):
            b = random_operand(rng, k) | 1                      # odd: invertible modulo 2^F
            a_low = (low * pow(b, -1, 1 << F)) % (1 << F)       # a_low * b = low (mod 2^F)
            a = (rng.getrandbits(64) << F) | a_low
            assert (a * b) % (1 << F) == low
            out.append((f"dropped half {name} #{t}", a, b))
        out.append((f"dropped half {name}, times one ulp", (rng.getrandbits(64) << F) | low, 1))
    return out


def exp2_for(k):
    """scale_exp2 for the mantissas (1.0, 1.0) that makes the constructors use k fractional limbs: bits = 1 - (E + 1) + 96 = 64 k - 40,
    which is shallow up to k = 17 and deep from k = 18 (min |scale| < 2^-960), and at most 2^-8192's 8288 bits at k = 130."""
    return 136 - 64 * k
