"""mc_mandelbrot_orbit_rescale without a GPU: the source's table under another scale of the same centre.  Same-limb rescales equal the
fresh constructor's object bit for bit; a rescale across a limb boundary carries the deeper orbit's table (the differences are printed,
not asserted); the scale fields are the deep constructor's, the fold into plain doubles included; every refusal with its status and
text; the source stays usable.  And the host table builders, which now run the header shared with the device build
(csrc/mandel_bla_table.h), against the numpy restatements on the shapes the device test uses."""
import ctypes as C
import math

import numpy as np
import pytest

import mandel_bla_deep_ref as BD
import mandel_bla_ref as BR

K4 = ("-0.74364388703715870000000000000000", "0.13182590420531198000000000000000")   # K4's centre written to 32 digits
MX, MY = 1.0, 0.75


def limbs(bits):
    return (bits + 63) // 64


def bits_for(mx, my, E):
    """The header's formula: 1 - e + 96 (at least 64), e the frexp exponent of min |scale|."""
    e = min(math.frexp(abs(mx)), math.frexp(abs(my)), key=lambda fe: (fe[1], fe[0]))[1] + E
    return max(64, 1 - e + 96)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_object(r, f, bits):
    assert same_bits(r.table(), f.table())
    assert (r.length, r.max_iter, r.bits) == (f.length, f.max_iter, bits)
    assert (r.deep, r.scale, r.scale_exp2) == (f.deep, f.scale, f.scale_exp2)


@pytest.mark.parametrize("src,dst", [(-100, -98), (-140, -100)])
def test_same_limb_rescale_equals_the_fresh_orbit(B, src, dst):
    with B.Orbit(*K4, MX, MY, 2000, src) as o, B.Orbit(*K4, MX, MY, 2000, dst) as fresh:
        assert limbs(o.bits) == limbs(fresh.bits) == 4 and bits_for(MX, MY, dst) == fresh.bits
        before = o.table().copy()
        with o.rescale(MX, MY, dst) as r:
            same_object(r, fresh, o.bits)                       # the table's bits are the source's: it is the source's table
            assert bits_for(MX, MY, dst) <= r.bits
            # the scale the C object stores is the fresh one's: both build the same table, whose radii depend on the scale alone
            assert same_bits(np.asarray(r.bla()), np.asarray(fresh.bla()))
            assert same_bits(r.bla_table(), fresh.bla_table())
        assert same_bits(o.table(), before)                     # the source: unchanged ...
        o.bla()                                                 # ... and usable
        assert o.bla_table().shape[0] == sum(BR.level_counts(o.length))


def test_rescale_across_a_limb_boundary_returns_the_sources_table(B, capsys):
    with B.Orbit(*K4, 1.0, 1.0, 2000, -162) as o, B.Orbit(*K4, 1.0, 1.0, 2000, -160) as fresh:   # 258 and 256 bits
        assert (limbs(o.bits), limbs(fresh.bits)) == (5, 4)
        with o.rescale(1.0, 1.0, -160) as r:
            assert same_bits(r.table(), o.table()) and (r.length, r.bits) == (o.length, o.bits)
            assert (r.deep, r.scale, r.scale_exp2) == (fresh.deep, fresh.scale, fresh.scale_exp2)
            n = min(r.length, fresh.length) + 1
            differ = int((r.table()[:n].view(np.uint64) != fresh.table()[:n].view(np.uint64)).sum())
    with capsys.disabled():
        print(f"\n5-limb table against the fresh 4-limb orbit: {differ} of {2 * n} doubles differ (lengths {r.length}, {fresh.length})")


def test_deep_to_plain_folds_the_scale(B):
    with B.Orbit("-0.75", "0.1", 0.75, 0.5, 300, -1100) as o:
        assert o.deep
        with pytest.raises(B.McError):
            o.bla()
        with o.rescale(0.75, 0.5, -900) as r, B.Orbit("-0.75", "0.1", 0.75, 0.5, 300, -900) as fresh:
            assert not r.deep and r.scale == (math.ldexp(0.75, -900), math.ldexp(0.5, -900)) and r.scale_exp2 == 0
            assert r.bits == o.bits and same_bits(r.table(), o.table())
            levels, entries = r.bla()                            # mc_mandelbrot_orbit_bla accepts it: the C object is not deep
            assert entries == sum(BR.level_counts(r.length))
            want = BR.table(r.table(), r.length, r.scale)
            assert same_bits(r.bla_table(), want)
            if same_bits(r.table(), fresh.table()):              # then the whole object's tables are the fresh one's
                fresh.bla()
                assert same_bits(r.bla_table(), fresh.bla_table())


def test_deep_to_deep_moves_only_the_exponent(B):
    with B.Orbit("-0.75", "0.1", 0.75, 0.5, 300, -1100) as o:
        with o.rescale(0.75, 0.5, -1090) as r, B.Orbit("-0.75", "0.1", 0.75, 0.5, 300, -1090) as fresh:
            assert limbs(o.bits) == limbs(fresh.bits)
            assert r.deep and r.scale == (0.75, 0.5) and r.scale_exp2 == -1090
            same_object(r, fresh, o.bits)
            r.bla_deep(), fresh.bla_deep()
            for a, b in zip(r.bla_deep_table(), fresh.bla_deep_table()):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        with o.rescale(-0.5, 0.75, -1100) as r:                  # other mantissas at the same depth
            assert r.deep and r.scale == (-0.5, 0.75) and r.scale_exp2 == -1100


def test_refusals(B):
    L = B.lib()
    L.mc_last_error_detail.restype = C.c_char_p
    fn = "mc_mandelbrot_orbit_rescale: "
    h = C.c_void_p(1)

    def refused(o, mx, my, E, status, text):
        h.value = 1
        assert L.mc_mandelbrot_orbit_rescale(o._h, mx, my, E, C.byref(h)) == status
        assert h.value is None
        assert L.mc_last_error_detail().decode() == fn + text, L.mc_last_error_detail()

    with B.Orbit(*K4, MX, MY, 200, -100) as o, B.Orbit("-0.75", "0.1", 0.75, 0.5, 200, -8191) as deep:
        assert L.mc_mandelbrot_orbit_rescale(None, MX, MY, -100, C.byref(h)) == 1
        assert L.mc_last_error_detail().decode() == fn + "NULL argument"
        assert L.mc_mandelbrot_orbit_rescale(o._h, MX, MY, -100, None) == 1
        for bad in (0.0, math.inf, -math.inf, math.nan):
            refused(o, bad, MY, -100, 1, "scale_x and scale_y must be finite and nonzero")
            refused(o, MX, bad, -100, 1, "scale_x and scale_y must be finite and nonzero")
        # deeper than the source: 197 bits there, 198 asked
        refused(o, MX, MY, -101, 5, "the orbit was computed for a shallower view (it carries 197 fractional bits, this scale asks for 198)")
        refused(o, MX, MY, -1000, 5, "the orbit was computed for a shallower view (it carries 197 fractional bits, this scale asks for 1097)")
        # the constructor's refusals, word for word
        refused(deep, 0.75, 0.5, -8192, 5, "scale below 2^-8192 (the orbit's fixed point would need more than 130 limbs)")
        refused(deep, 0.75, 0.5, 2 ** 31 - 1, 5, "scale above the double range")
        refused(o, 0.75, 0.5, 1025, 5, "scale above the double range")
        for E, text in ((-8192, "scale below 2^-8192 (the orbit's fixed point would need more than 130 limbs)"),
                        (1025, "scale above the double range")):   # ... the words the deep constructor says
            with pytest.raises(B.McError) as e:
                B.Orbit("-0.75", "0.1", 0.75, 0.5, 200, E)
            assert e.value.status == 5 and str(e.value).endswith("mc_mandelbrot_orbit_create_deep: " + text)
        # the widest and the deepest accepted
        with o.rescale(0.75, 0.5, 1024) as r:
            assert r.scale == (math.ldexp(0.75, 1024), math.ldexp(0.5, 1024)) and not r.deep
        with deep.rescale(0.5, 0.75, -8191) as r:
            assert r.deep and r.scale == (0.5, 0.75) and r.scale_exp2 == -8191
        with pytest.raises(B.McError) as e:
            o.rescale(MX, MY, -101)
        assert e.value.status == 5
        assert o.table().shape == (o.length + 1, 2)              # still usable


# ---- the host builders through the shared header: the shapes tests/test_gpu_mandel_bla_table_device.py uses ----
def shape_lengths(B):
    g = B.bla_table_group_entries()
    lo, hi = g // 2, 2 * g                                      # one power of two on either side of the single-workgroup threshold
    return [2, 3, 4, 5, 6] + [n + 2 for p in (lo, g, hi) for n in (p - 1, p, p + 1)]


def test_group_threshold_is_a_power_of_two(B):
    g = B.bla_table_group_entries()
    assert g >= 2 and g & (g - 1) == 0


def check_plain(o):
    levels, entries = o.bla()
    counts = BR.level_counts(o.length)
    assert levels == len(counts) and entries == sum(counts)
    assert same_bits(o.bla_table(), BR.table(o.table(), o.length, o.scale))


def check_deep(o):
    levels, entries = o.bla_deep()
    counts = BR.level_counts(o.length)
    assert levels == len(counts) and entries == sum(counts)
    mant, exps = o.bla_deep_table()
    wm, we = BD.table(o.table(), o.length, o.scale, BD.orbit_E(o))
    assert same_bits(mant, wm) and np.array_equal(exps, we)


def test_host_builders_equal_the_restatements_on_the_level_shapes(B):
    for L in shape_lengths(B):                                   # a bounded orbit: L = max_iter
        with B.Orbit("-0.1", "0.2", 1e-14, 1e-14, L) as o:
            assert o.length == L
            check_plain(o)
            check_deep(o)


@pytest.mark.parametrize("centre,scale,M", [(K4, (2.0 ** -100, 0.75 * 2.0 ** -100), 20000), (("-0.1", "0.2"), (1e-200, 1e-200), 5000),
                                            (("0", "0"), (1e-10, 1e-10), 1000), (("-1", "0"), (1e-10, 1e-10), 1000)],
                         ids=["escaping", "bounded (the plain table overflows)", "centre 0", "centre -1"])
def test_host_builders_equal_the_restatements_on_the_orbits(B, centre, scale, M):
    with B.Orbit(centre[0], centre[1], scale[0], scale[1], M) as o:
        check_plain(o)
        check_deep(o)
        if centre[0] in ("0", "-1"):                             # zero entries: A = 0 and R = 0 at level 0, R = 0 everywhere above
            T = o.bla_table()
            zero = (o.table()[1:o.length - 1] == 0).all(axis=1)
            assert zero.any() and (T[:o.length - 2][zero][:, [0, 1, 4]] == 0).all()
            assert (T[o.length - 2:, 4] == 0).all()


@pytest.mark.parametrize("E", [-1100, -8000])
def test_host_deep_builder_equals_the_restatement_below_the_double_range(B, E):
    with B.Orbit("-0.75", "0.1", 0.75, 0.5, 700, E) as o:
        assert o.deep
        check_deep(o)
