"""Input sets and assertion functions of the device-math tests, shared by tests/test_math_accuracy_host.py (the oracle, no GPU) and
tests/test_gpu_math_edges.py (the device hooks).  Not a conftest: the test files import it.

Everything is deterministic (fixed seeds, fixed permutations) and cached; the arrays handed out are read-only.

Two kinds of check live here:
  * PARITY at the edges of fp32 — zeros of both signs, subnormals, inf, NaN, unnormalised two-float pairs, overflow inside the Dekker
    split, underflowing products — compared by bits, with one allowance: two NaNs are equal whatever their sign or payload (x86's default
    NaN is negative, gfx950's positive);
  * ACCURACY against the mathematics: numpy float64 for the scalar functions, float64 / fractions.Fraction for the two-float packages.
    The implementation under test is passed in as a function, so the same assertions run on the oracle and on the device's outputs."""
import functools
from fractions import Fraction

import numpy as np

F32 = np.float32
U24 = 2.0 ** -24
U44 = 2.0 ** -44


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# parity by bits
# ---------------------------------------------------------------------------------------------------------------------------------------
def same_bits_or_both_nan(got, want):
    """Elementwise: identical bit patterns (so zero signs must match), or both NaN."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def assert_same_bits(got, want, what, inputs=()):
    """inputs: arrays aligned with the first axis of got, printed for the first mismatching rows."""
    ok = same_bits_or_both_nan(got, want)
    if ok.all():
        return
    rows = np.unique(np.argwhere(~ok)[:, 0])
    lines = []
    for r in rows[:8]:
        ins = " ".join(str([hex(int(v)) for v in np.atleast_1d(bits(np.asarray(x)[r]))]) for x in inputs)
        lines.append(f"  row {r}: in {ins} got {[hex(int(v)) for v in np.atleast_1d(bits(got[r]))]} "
                     f"want {[hex(int(v)) for v in np.atleast_1d(bits(want[r]))]}")
    raise AssertionError(f"{what}: {rows.size} of {ok.shape[0]} rows differ\n" + "\n".join(lines))


# ---------------------------------------------------------------------------------------------------------------------------------------
# A. input generators
# ---------------------------------------------------------------------------------------------------------------------------------------
CRAFTED_MANTISSAS = (0, 1, 2, 0x7fffff, 0x7ffffe, 0x400000, 0x3fffff, 0x400001, 0x1000, 0xfff, 0x1fff, 0x7ff000)


@functools.lru_cache(maxsize=None)
def fp32_strata():
    """(sorted, shuffled): the same 2^20 fp32 values in two orders.  Every exponent field 0..255 with both signs, each with the twelve
    crafted mantissas and 2036 random ones: every kind of zero, subnormal, inf and NaN is in by construction.  `sorted` is in bit-pattern
    order, so each wave of 64 lies inside one exponent (the strict short forms' wave-wide window test is all-in or all-out); `shuffled` is
    a fixed permutation, so every wave mixes values inside and outside the window."""
    rng = np.random.default_rng(0x51A7A)
    mant = np.empty((2, 256, 2048), np.uint32)
    mant[:, :, :12] = np.array(CRAFTED_MANTISSAS, np.uint32)
    mant[:, :, 12:] = rng.integers(0, 1 << 23, (2, 256, 2036), dtype=np.uint32)
    sign = (np.arange(2, dtype=np.uint32) << 31)[:, None, None]
    expo = (np.arange(256, dtype=np.uint32) << 23)[None, :, None]
    u = np.sort((sign | expo | mant).reshape(-1))
    assert u.size == 1 << 20
    perm = np.random.default_rng(0x5B0FF1E).permutation(u.size)
    return _ro(from_bits(u), from_bits(u[perm]))


def in_short_window(x):
    """mc_math.h in_short_window: 2^-100 <= x < 2^100."""
    return (bits(x) - np.uint32(0x0D800000)) < np.uint32(0x64000000)


def waves_mixing_the_window(x):
    """Number of waves of 64 consecutive values that hold values inside AND outside the short-form window."""
    w = in_short_window(x).reshape(-1, 64)
    return int((w.any(1) & ~w.all(1)).sum())


def _hi_from(sign, efield, mant):
    return from_bits((sign.astype(np.uint32) << 31) | (efield.astype(np.uint32) << 23) | mant.astype(np.uint32))


def _lo_for(hi, kind, u):
    """The low word for `hi`: kind 0 normalised (|lo| < ulp(hi) / 2), 1 +0, 2 -0, 3 unnormalised (|lo| up to |hi|); u in (-1, 1)."""
    with np.errstate(all="ignore"):
        half_ulp = 0.5 * np.spacing(np.abs(hi)).astype(np.float64)
        norm = (u * 0.999 * half_ulp).astype(np.float32)
        unnorm = (u * hi.astype(np.float64)).astype(np.float32)
    lo = np.where(kind == 0, norm, np.where(kind == 3, unnorm, F32(0.0))).astype(np.float32)
    lo[kind == 2] = F32(-0.0)
    lo[~np.isfinite(hi)] = F32(0.0)   # inf / NaN hi (exponent field 255): the low word is a zero here; the specials vary it
    return lo


SPECIAL_HI = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, 1.17549435e-38, 2.0 ** -51, 2.0 ** -50, 1.0, -1.0, 2.0, 8193.0, 2.0 ** 60,
                       2.0 ** 114, 2.0 ** 115, 3e38, -3e38, np.inf, -np.inf, np.nan], np.float32)


def _special_operands():
    """Every special hi with 8 special low words: +0, -0, the smallest subnormal, a normalised one of each sign, -hi (the pair is worth 0),
    inf and NaN."""
    hi = np.repeat(SPECIAL_HI, 8)
    with np.errstate(all="ignore"):
        h = SPECIAL_HI.astype(np.float64)
        lo = np.stack([np.zeros_like(h), -np.zeros_like(h), np.full_like(h, 1e-45), h * 2.0 ** -24, h * -0.75 * 2.0 ** -24, -h,
                       np.full_like(h, np.inf), np.full_like(h, np.nan)], 1).astype(np.float32).reshape(-1)
    return np.stack([hi, lo], 1)


@functools.lru_cache(maxsize=None)
def ds_pairs():
    """(a, b): float32 (n, 2) operand pairs (hi, lo) for the two-float hooks.
    Part 1: the cross product of the 160 special operands with themselves (25 600 pairs).
    Part 2: about 400 000 stratified pairs — every exponent field for a.hi with exponent gaps 0..60 to b.hi in both directions and low
    words normalised, +-0 and unnormalised; b = -a, b = a, b = -a with another low word; |hi| in [2^113, 2^128) (hi * 8193 overflows from
    2^114 on); products and squares below 2^-126; the region where ds_mul_fma's precondition holds."""
    sp = _special_operands()
    i, j = np.meshgrid(np.arange(len(sp)), np.arange(len(sp)), indexing="ij")
    parts_a, parts_b = [sp[i.reshape(-1)]], [sp[j.reshape(-1)]]
    rng = np.random.default_rng(0xD5A17)

    def operand(n, efield, kind):
        hi = _hi_from(rng.integers(0, 2, n), efield, rng.integers(0, 1 << 23, n))
        return np.stack([hi, _lo_for(hi, kind, rng.uniform(-1, 1, n))], 1)

    # (i) every exponent field x gap 0..60 (either direction) x 4 kinds of a.lo x 3 kinds of b.lo
    n = 256 * 61 * 12
    k = np.arange(n)
    ea, gap, v = k % 256, (k // 256) % 61, k // (256 * 61)
    eb = np.clip(np.where(k % 2 == 0, ea - gap, ea + gap), 0, 254)
    parts_a.append(operand(n, ea, v % 4))
    parts_b.append(operand(n, eb, np.array([0, 1, 3])[v // 4]))
    # (ii) b = -a, b = a, b = -a with another low word; every finite exponent field
    n = 20000
    for variant in range(3):
        a = operand(n, np.arange(n) % 255, (np.arange(n) // 255) % 4)
        b = a.copy() if variant == 1 else -a
        if variant == 2:
            b[:, 1] = _lo_for(b[:, 0], np.zeros(n, int), rng.uniform(-1, 1, n))
        parts_a.append(a); parts_b.append(b)
    # (iii) |a.hi| in [2^113, 2^128); b the same, of the order of 1, or small enough for the product to stay finite
    n = 51000
    a = operand(n, rng.integers(113 + 127, 255, n), np.arange(n) % 4)
    eb = np.where(np.arange(n) % 3 == 0, rng.integers(113 + 127, 255, n), np.where(np.arange(n) % 3 == 1, rng.integers(120, 134, n),
                                                                                  rng.integers(1, 14, n)))
    parts_a.append(a); parts_b.append(operand(n, eb, (np.arange(n) // 4) % 4))
    # (iv) products below 2^-126 (down to total underflow), and squares below 2^-126
    n = 40000
    e1 = rng.integers(-100, 1, n)
    e2 = rng.integers(-152, -126, n) - e1
    parts_a.append(operand(n, e1 + 127, np.arange(n) % 4))
    parts_b.append(operand(n, np.clip(e2 + 127, 0, 254), (np.arange(n) // 4) % 4))
    n = 10000
    a = operand(n, rng.integers(-76, -62, n) + 127, np.arange(n) % 4)
    parts_a.append(a); parts_b.append(a.copy())
    # (v) the precondition region of ds_mul_fma: normalised pairs, |hi| in [2^-50, 2^60); squares included
    n = 50000
    a, b = operand(n, rng.integers(-50, 60, n) + 127, np.zeros(n, int)), operand(n, rng.integers(-50, 60, n) + 127, np.zeros(n, int))
    b[: n // 4] = a[: n // 4]
    parts_a.append(a); parts_b.append(b)
    return _ro(np.ascontiguousarray(np.concatenate(parts_a), np.float32), np.ascontiguousarray(np.concatenate(parts_b), np.float32))


def mul_fma_precondition(a, b):
    """Rows where ds_mul_fma is stated to equal ds_mul (ds_arith.h; tests/test_gpu_parity.py): both pairs normalised, |hi| in
    [2^-50, 2^60), |a.hi * b.hi| < 2^100."""
    def ok(p):
        h, l = np.abs(p[:, 0].astype(np.float64)), np.abs(p[:, 1].astype(np.float64))
        with np.errstate(all="ignore"):
            return (h >= 2.0 ** -50) & (h < 2.0 ** 60) & (l <= 0.5 * np.spacing(np.abs(p[:, 0])).astype(np.float64))
    with np.errstate(all="ignore"):
        return ok(a) & ok(b) & (np.abs(a[:, 0].astype(np.float64) * b[:, 0].astype(np.float64)) < 2.0 ** 100)


@functools.lru_cache(maxsize=None)
def div3_cases():
    """(a (n, 3), s (n,)) from the shuffled strata: numerators and divisors inside and outside div3's window ([2^-60, 2^60), numerators
    also +0) side by side in every wave.  A third of the rows has all operands folded into the window's exponents, so that whole triples
    inside the window sit in the same waves as rows outside it."""
    _, sh = fp32_strata()
    n = sh.size // 4
    a = sh[: 3 * n].reshape(n, 3).copy()
    s = sh[3 * n:].copy()
    def fold(x):   # same sign and mantissa, exponent folded into [2^-60, 2^60), sign cleared (the window is positive)
        u = bits(x)
        e = (u >> 23) & np.uint32(0xff)
        return from_bits((u & np.uint32(0x007fffff)) | ((e % np.uint32(120) + np.uint32(67)) << 23))
    rows = np.arange(n) % 3 == 0
    a[rows] = fold(a[rows].reshape(-1)).reshape(-1, 3)
    s[rows] = fold(s[rows])
    a[np.arange(n) % 12 == 0, 1] = F32(0.0)
    return _ro(a, s)


# ---------------------------------------------------------------------------------------------------------------------------------------
# C. accuracy of the scalar functions against numpy float64
# ---------------------------------------------------------------------------------------------------------------------------------------
def _every(first_bits, last_bits, step):
    return from_bits(np.arange(first_bits, last_bits + 1, step, dtype=np.uint64).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def scalar_sets():
    """name -> float32 inputs.  Committed and deterministic: the bounds below were measured on exactly these."""
    two_pi = F32(2.0 * np.pi)
    sets = {}
    near = [np.arange(0, 1025, dtype=np.int64)]
    for k in range(1, 5):
        c = int(bits(np.array([k * np.pi / 2], np.float32))[0])
        near.append(np.arange(c - 1024, c + 1025, dtype=np.int64))
    sets["trig_0_2pi"] = np.concatenate([_every(0, int(bits(np.array([two_pi]))[0]), 257), from_bits(np.concatenate(near).astype(np.uint32))])
    rng = np.random.default_rng(0x7216)
    e = np.repeat(np.arange(-20, 6), 4096)     # 2^-20 .. 2^6, both signs, random mantissas; clipped to [-50, 50]
    x = _hi_from(rng.integers(0, 2, e.size), e + 127, rng.integers(0, 1 << 23, e.size))
    sets["trig_pm50"] = np.concatenate([x[np.abs(x) <= 50.0], np.linspace(-50.0, 50.0, 100001).astype(np.float32)])
    sets["unit_0_1"] = _every(1, 0x3f800000, 251)                                   # (0, 1]: subnormals included; ends on 1.0 - n ulp
    sets["unit_0_1"] = np.concatenate([sets["unit_0_1"], np.array([1.0], np.float32)])
    sets["unit_2m12_1"] = np.concatenate([_every(0x39800000, 0x3f800000, 61), np.array([1.0], np.float32)])   # [2^-12, 1]
    sets["exp2_m125_0"] = np.concatenate([np.random.default_rng(0xE2).uniform(-125.0, 0.0, 2000000).astype(np.float32),
                                          np.arange(-250, 1, dtype=np.float32) * F32(0.5)])
    return {k: _ro(np.ascontiguousarray(v, np.float32)) for k, v in sets.items()}


POW_Y = np.float64(np.float32(0.45))   # the exponent the function is given is the float 0.45f


def _ulp_of(ref):
    """ulp of the fp32 binade that holds |ref| (ref float64, nonzero)."""
    _, e = np.frexp(np.abs(ref))
    return np.ldexp(1.0, e - 24)


def scalar_error(fn, x, got):
    """Worst error of `got` = fn(x), in the unit the bound of `fn` is written in, and the input it occurs at."""
    x64, g = x.astype(np.float64), got.astype(np.float64)
    with np.errstate(all="ignore"):
        if fn in ("sin", "cos"):
            err = np.abs(g - (np.sin(x64) if fn == "sin" else np.cos(x64))) / U24                    # absolute, 2^-24
        elif fn == "log2":
            ref = np.log2(x64)
            err = np.where(ref == 0.0, np.where(g == 0.0, 0.0, np.inf), np.abs(g - ref) / _ulp_of(np.where(ref == 0.0, 1.0, ref)))   # ulps of the result
        elif fn == "exp2":
            ref = np.exp2(x64)
            err = np.abs(g - ref) / ref / U24                                                         # relative, 2^-24
        elif fn == "pow045":
            ref = np.power(x64, POW_Y)
            err = np.abs(g - ref) / ref / U24                                                         # relative, 2^-24
        else:
            raise KeyError(fn)
    assert not np.isnan(err).any(), fn
    i = int(np.argmax(err))
    return float(err[i]), float(x[i])


# (function, input set) -> (measured maximum of the oracle, bound).  The bound is the measured maximum rounded up to the next multiple of
# 0.25 of its unit: the arithmetic has a fixed order, so the maximum reproduces to the bit, and the quarter unit only absorbs differences
# between libm versions in the float64 reference.  Units: 2^-24 absolute (sin, cos), ulps of the result (log2), 2^-24 relative (exp2, pow).
# The table is repeated in DESIGN.md section 4.
SCALAR_BOUNDS = {
    ("sin", "trig_0_2pi"): (1.4061, 1.5),          # at x = 0.8146588802337646
    ("cos", "trig_0_2pi"): (1.5217, 1.75),         # at x = 3.9051945209503174
    ("sin", "trig_pm50"): (1.3972, 1.5),           # at x = -40.00699996948242
    ("cos", "trig_pm50"): (1.4697, 1.5),           # at x = -3.8610000610351562
    ("log2", "unit_0_1"): (1.9684, 2.0),           # at x = 0.709190845489502
    ("log2", "unit_2m12_1"): (2.0045, 2.25),       # at x = 0.7453137636184692
    ("pow045", "unit_0_1"): (58.4265, 58.5),       # at x = 1.6133681713188062e-39: the tiniest x dominate, inherent to exp2(y * log2 x) in fp32
    ("pow045", "unit_2m12_1"): (6.1986, 6.25),     # at x = 0.0010036162566393614
    ("exp2", "exp2_m125_0"): (1.5361, 1.75),       # at x = -23.4998722076416
}


def check_scalar_accuracy(impl, report=print):
    """impl(fn, x) -> float32 results.  Asserts every bound of SCALAR_BOUNDS; returns {(fn, set): measured}."""
    sets, out, bad = scalar_sets(), {}, []
    for (fn, name), (_, bound) in SCALAR_BOUNDS.items():
        x = sets[name]
        err, at = scalar_error(fn, x, impl(fn, x))
        out[(fn, name)] = err
        report(f"{fn:7s} {name:12s} max error {err:.4f} (bound {bound}) at x = {at!r}")
        if not err <= bound:
            bad.append((fn, name, err, bound, at))
    assert not bad, bad
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# C. accuracy of the two-float packages
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twofloat_operands():
    """(a, b): 400 000 normalised pairs with exponents in [-30, 30]; the first eighth are squares (b = a), the next b = -a, and a further
    eighth has b.hi = a.hi with another low word (comparisons decided by the low word)."""
    rng = np.random.default_rng(0x2F10A7)
    n = 400000
    def operand():
        hi = _hi_from(rng.integers(0, 2, n), rng.integers(-30, 31, n) + 127, rng.integers(0, 1 << 23, n))
        return np.stack([hi, _lo_for(hi, np.zeros(n, int), rng.uniform(-1, 1, n))], 1)
    a, b = operand(), operand()
    e = n // 8
    b[:e] = a[:e]
    b[e:2 * e] = -a[e:2 * e]
    b[2 * e:3 * e, 0] = a[2 * e:3 * e, 0]
    b[2 * e:3 * e, 1] = _lo_for(b[2 * e:3 * e, 0], np.zeros(e, int), rng.uniform(-1, 1, e))
    return _ro(a, b)


def value(p):
    """A two-float value as float64 (exact for a normalised pair: at most 49 significant bits)."""
    return p[:, 0].astype(np.float64) + p[:, 1].astype(np.float64)


# op -> (reference in float64, what the error is relative to).  Bound: 2^-44 each.  The oracle sits at 0.12 .. 0.47 of it; a dropped error
# term shows at 2^-24 .. 2^-30.  Relative to the RESULT ds_add and ds_sub reach ~150 x 2^-44 under cancellation: a property of the
# reference's algorithm, so it is not asserted.
TWOFLOAT_OPS = ("add", "sub", "mul", "df64_add", "df64_mult", "sqrt", "df64_sqrt")


def twofloat_error(op, a, b, got):
    va, vb, g = value(a), value(b), value(got)
    with np.errstate(all="ignore"):
        if op in ("add", "df64_add"):
            ref = va + vb
        elif op == "sub":
            ref = va - vb
        elif op in ("mul", "df64_mult"):
            ref = va * vb
        else:
            ref = np.sqrt(va)
        scale = np.abs(va) + np.abs(vb) if op in ("add", "sub") else np.abs(ref)
        err = np.where(g == ref, 0.0, np.abs(g - ref) / scale) / U44
    assert not np.isnan(err).any(), op
    i = int(np.argmax(err))
    return float(err[i]), i


def check_twofloat_accuracy(impl, report=print):
    """impl(op, a, b) -> float32 (n, 2).  Bound 2^-44 for every op of TWOFLOAT_OPS; ds_div is measured and printed only (restated "as
    written, may contain typos", used by no path)."""
    a, b = twofloat_operands()
    pos = np.where(a[:, :1] < 0, -a, a)   # the square roots' operand: |a| as a pair (negating both words is exact)
    out, bad = {}, []
    for op in TWOFLOAT_OPS:
        x = pos if op in ("sqrt", "df64_sqrt") else a
        err, i = twofloat_error(op, x, b, impl(op, x, b))
        out[op] = err
        report(f"{op:10s} max error {err:.4f} x 2^-44 at row {i}")
        if not err <= 1.0:
            bad.append((op, err, i))
    with np.errstate(all="ignore"):
        q = value(impl("div", a, b))
        ref = value(a) / value(b)
        report(f"div        max error {float(np.max(np.abs(q - ref) / np.abs(ref)) / U44):.4f} x 2^-44 (measured only, nothing asserted)")
    assert not bad, bad
    return out


def _frac(x):
    return Fraction(float(x))


def check_exact_properties(impl, n_fraction=4000):
    """impl(op, a, b) -> float32 (n, 2).  ds_twoProd: hi + lo == a * b whenever |a * b| is in [2^-100, 2^100); twoDiff: s + e == a - b;
    ds_compare / df64_eq / df64_neq against comparisons of the pairs' values.  Vectorised in float64 where float64 is exact, and with
    fractions.Fraction on a fixed subsample where it could round."""
    a, b = twofloat_operands()
    sub = np.random.default_rng(0xF2AC).choice(a.shape[0], n_fraction, replace=False)
    # twoProd: a.hi * b.hi has 48 significant bits — exact in float64, and so is hi + lo when it equals the product
    tp = impl("twoprod", a, b)
    prod = a[:, 0].astype(np.float64) * b[:, 0].astype(np.float64)
    inr = (np.abs(prod) >= 2.0 ** -100) & (np.abs(prod) < 2.0 ** 100)
    assert inr.sum() > a.shape[0] // 2
    wrong = inr & (value(tp) != prod)
    assert not wrong.any(), ("twoprod", int(wrong.sum()), int(np.argmax(wrong)))
    for i in sub[inr[sub]]:
        assert _frac(tp[i, 0]) + _frac(tp[i, 1]) == _frac(a[i, 0]) * _frac(b[i, 0]), ("twoprod", int(i))
    # twoDiff: exact for every pair of finite floats whose difference does not overflow; float64 cannot hold a difference across a gap
    # of more than 29 exponents, so the whole set goes through the gap test and the subsample through Fraction
    td = impl("twodiff", a, b)
    d64 = a[:, 0].astype(np.float64) - b[:, 0].astype(np.float64)
    _, ea = np.frexp(a[:, 0].astype(np.float64)); _, eb = np.frexp(b[:, 0].astype(np.float64))
    close = np.abs(ea - eb) <= 28
    wrong = close & (value(td) != d64)
    assert close.sum() > a.shape[0] // 4 and not wrong.any(), ("twodiff", int(wrong.sum()), int(np.argmax(wrong)))
    for i in sub:
        assert _frac(td[i, 0]) + _frac(td[i, 1]) == _frac(a[i, 0]) - _frac(b[i, 0]), ("twodiff", int(i))
    # comparisons: a normalised pair's value is exact in float64, and value order is what the package's lexicographic chain states
    va, vb = value(a), value(b)
    cmp_ = impl("compare", a, b)
    assert np.array_equal(cmp_[:, 0], np.sign(va - vb).astype(np.float32)), "compare"
    assert not cmp_[:, 1].any()
    assert all((cmp_[:, 0] == k).sum() > 1000 for k in (-1.0, 0.0, 1.0))
    eq = impl("df64_eqneq", a, b)
    assert np.array_equal(eq[:, 0] != 0, va == vb) and np.array_equal(eq[:, 1] != 0, va != vb), "df64_eq / df64_neq"
    for i in sub:
        pa, pb = (_frac(a[i, 0]) + _frac(a[i, 1])), (_frac(b[i, 0]) + _frac(b[i, 1]))
        assert cmp_[i, 0] == (pa > pb) - (pa < pb), ("compare", int(i))
        assert bool(eq[i, 0]) == (pa == pb) and bool(eq[i, 1]) == (pa != pb), ("df64_eqneq", int(i))


# ---------------------------------------------------------------------------------------------------------------------------------------
# B. IEEE references of the short forms, and the fast tier's domains
# ---------------------------------------------------------------------------------------------------------------------------------------
def ieee(fn, x):
    """sqrt / rsqrt / rcp as numpy's IEEE fp32 arithmetic computes them (rsqrt = RN(1 / RN(sqrt x)), the project's definition)."""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(all="ignore"):
        return {"sqrt": lambda: np.sqrt(x), "rsqrt": lambda: F32(1.0) / np.sqrt(x), "rcp": lambda: F32(1.0) / x}[fn]()


def fast_tier_domain():
    """The normal strata of [2^-100, 2^100): what the kernels feed the fast sqrt, rcp and rsqrt."""
    srt, _ = fp32_strata()
    return srt[in_short_window(srt)]


def fast_tier_angles():
    """angle = RN(two_pi_f32 * u) for u over the strata of [0, 1): what the kernels feed the fast sine and cosine."""
    srt, _ = fp32_strata()
    u = srt[(bits(srt) < np.uint32(0x3f800000))]
    return F32(2.0 * np.pi) * u
