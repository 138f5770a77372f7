"""The contract of the exact counts (include/mc_compute.h: "exact counts of sampled pixels") restated on Python integers.

- `parse_centre`: the orbit constructor's fixed point of a decimal: truncated at 64 k fractional bits, the last bit set when anything
  nonzero was dropped (round to odd), sign and magnitude.
- `pixel_c`: c_ref extended by the extra limbs plus an offset double * 2^dc_exp2, exactly; Unsupported when a bit would drop or a part
  of |c| exceeds 4.
- `count`: the iteration; `counts`: all of it for arrays of offsets.
Not a conftest: the test files import it."""
from fractions import Fraction


class Unsupported(Exception):
    """What the library refuses with MC_ERR_UNSUPPORTED."""


def limbs_of(bits, extra_limbs=0):
    """n = ceil(bits / 64) + 1 + extra_limbs."""
    return (bits + 63) // 64 + 1 + extra_limbs


def parse_centre(text, bits):
    """The signed integer c_ref * 2^(64 k), k = ceil(bits / 64), as the constructor parses the decimal `text`."""
    F0 = 64 * ((bits + 63) // 64)
    v = Fraction(text)
    mag = abs(v) * (1 << F0)
    m = mag.numerator // mag.denominator
    if m * mag.denominator != mag.numerator:
        m |= 1
    return -m if v < 0 else m


def mul(a, b, F):
    """sign * ((|a| |b| + 2^(F - 1)) >> F)"""
    m = (abs(a) * abs(b) + (1 << (F - 1))) >> F
    return -m if (a < 0) != (b < 0) else m


def count(cx, cy, F, max_iter):
    """n for c = (cx, cy) / 2^F."""
    two = 2 << F
    zx = zy = sx = sy = 0
    for j in range(max_iter):
        zx, zy = (sx - sy) + cx, 2 * mul(zx, zy, F) + cy
        sx, sy = mul(zx, zx, F), mul(zy, zy, F)
        if sx + sy > two:
            return j
    return max_iter


def pixel_c(cref, bits, extra_limbs, d, dc_exp2):
    """One part of c as an integer scaled by 2^F, F = 64 (n - 1): cref (parse_centre's) shifted up by the extra limbs, plus d * 2^dc_exp2."""
    n = limbs_of(bits, extra_limbs)
    if n > 131:
        raise Unsupported("more than 131 limbs")
    F = 64 * (n - 1)
    off = Fraction(float(d)) * Fraction(2) ** (dc_exp2 + F)
    if off.denominator != 1:
        raise Unsupported("the offset has bits below 2^-F")
    c = (cref << (64 * extra_limbs)) + off.numerator
    if abs(c) > (4 << F):
        raise Unsupported("|c| above 4")
    return c


def counts(centre, bits, dcx, dcy, dc_exp2, max_iter, extra_limbs=0):
    """The exact counts for the centre (two decimal texts) of an orbit of `bits` and the offsets (dcx[i], dcy[i]) * 2^dc_exp2: a list."""
    F = 64 * (limbs_of(bits, extra_limbs) - 1)
    rx, ry = parse_centre(centre[0], bits), parse_centre(centre[1], bits)
    return [count(pixel_c(rx, bits, extra_limbs, x, dc_exp2), pixel_c(ry, bits, extra_limbs, y, dc_exp2), F, max_iter)
            for x, y in zip(dcx, dcy)]
