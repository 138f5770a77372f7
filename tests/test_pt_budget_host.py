"""Per-pixel sample budgets without a GPU: mc_pathtrace_budget_levels and mc_pathtrace_budget_resolve (the kernels' own source, compiled
for the host) against tests/pt_budget_ref.py bit for bit, the three facts the chain rests on asserted in the CPU oracle, every host
refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import pt_budget_ref as R
import pt_noise_ref as N
from test_pt_denoise_host import bits

INVALID = 1
SHAPES = [(1, 1), (23, 11), (257, 130)]   # (W, H); the last: more than one block of 256 pixels with a partial last one
f32 = np.float32


def up(x):
    return np.nextafter(f32(x), f32(np.inf))


@functools.lru_cache(maxsize=None)
def variance_plane(W, H, target):
    """A noise plane around tau2 = target^2: random values over six octaves of it, then (written over them, cyclically) 0, exactly tau2,
    2 tau2 and 256 tau2, the next float above each, +inf, NaN and negatives; shared and read-only.  A 1 x 1 plane holds tau2's successor."""
    tau2 = f32(target) * f32(target)
    rng = np.random.default_rng(77 * W + H)
    v = (tau2 * np.exp2(rng.uniform(-3.0, 10.0, (H, W)))).astype(f32)
    special = np.array([0.0, tau2, up(tau2), f32(2) * tau2, up(f32(2) * tau2), f32(256) * tau2, up(f32(256) * tau2), np.inf, np.nan, -1.0,
                        -np.inf, f32(0.5) * tau2], f32)
    flat = v.reshape(-1)
    if flat.size == 1:
        flat[0] = up(tau2)
    else:
        at = np.arange(0, flat.size, 2)
        flat[at] = special[np.arange(at.size) % special.size]
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def acc_plane(W, H):
    """A linear accumulator plane: mostly inside (0, 0.5), a tenth negative, a tenth above 1 (the clamp), exact zeros; w arbitrary."""
    rng = np.random.default_rng(5 * W + H)
    a = (rng.random((H, W, 4), dtype=f32) * f32(0.5)).astype(f32)
    u = rng.random((H, W))
    a[u < 0.1] = -a[u < 0.1]
    a[u > 0.9] = a[u > 0.9] * f32(7.0) + f32(0.6)
    a[(u > 0.45) & (u < 0.5), 1] = 0.0
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def level_plane(W, H, max_level):
    lv = np.random.default_rng(3 * W + H + max_level).integers(0, max_level + 1, (H, W)).astype(np.uint8)
    lv.setflags(write=False)
    return lv


def test_symbols(B):
    for s in ("mc_pathtrace_budget_default_params", "mc_pathtrace_budget_levels", "mc_pathtrace_budget_resolve",
              "mc_pathtrace_budget_levels_device_async", "mc_pathtrace_budget_lists_device_async", "mc_pathtrace_budget_resolve_device_async",
              "mc_pathtrace_render_list_device_async", "mc_pathtrace_render_budgeted", "mc_context_last_budget"):
        assert s in B.declared_symbols() and hasattr(B.lib(), s)
    b = B.pathtrace_budget_params()
    assert (b.max_level, b.radius, b.flags) == (4, B.pathtrace_noise_defaults()[1], 0) and b.target > 0
    assert C.sizeof(B.PathtraceBudgetParams) == 16
    assert B.lib().mc_abi_version() == 3


@pytest.mark.parametrize("W,H", SHAPES)
def test_levels_equal_the_restatement(B, W, H):
    for target in (8.0, 0.37):
        v = variance_plane(W, H, target)
        for max_level in (0, 1, 4, 8):
            out = B.pathtrace_budget_levels(v, target, max_level)
            assert np.array_equal(out, R.levels(v, target, max_level)), (target, max_level)
            assert out.max() <= max_level
            if max_level == 0:
                assert not out.any()
    # the stated edge cases, one by one, at max_level = 8 and tau2 = 64
    tau2 = f32(64)
    cases = [(0.0, 0), (tau2, 0), (up(tau2), 1), (f32(2) * tau2, 1), (up(f32(2) * tau2), 2), (f32(256) * tau2, 8), (up(f32(256) * tau2), 8),
             (np.inf, 8), (np.nan, 0), (-1.0, 0), (-np.inf, 0)]
    plane = np.array([[c[0] for c in cases]], f32)
    assert B.pathtrace_budget_levels(plane, 8.0, 8).tolist() == [[c[1] for c in cases]]
    assert B.pathtrace_budget_levels(plane, 8.0, 3).tolist() == [[min(c[1], 3) for c in cases]]


@pytest.mark.parametrize("W,H", SHAPES)
def test_resolve_equals_the_restatement(B, O, W, H):
    acc = acc_plane(W, H)
    for max_level in (0, 4):
        lv = level_plane(W, H, max_level)
        out = B.pathtrace_budget_resolve(acc, lv)
        ref = R.resolve(O, acc, lv)
        assert np.array_equal(bits(out), bits(ref)), int((bits(out) != bits(ref)).any(-1).sum())
        assert np.array_equal(bits(out[..., 3]), bits(acc[..., 3]))
        buf = np.array(acc)
        assert B.pathtrace_budget_resolve(buf, lv, in_place=True) is buf
        assert np.array_equal(bits(buf), bits(ref)), "in place"
    # unaligned host planes
    store = np.zeros(2 * (W * H * 4) + 2, f32)
    a = store[1:1 + W * H * 4].reshape(H, W, 4)
    o = store[W * H * 4 + 2:].reshape(H, W, 4)
    assert a.ctypes.data % 16 != 0 and o.ctypes.data % 16 != 0
    a[...] = acc
    lv = level_plane(W, H, 4)
    assert B.lib().mc_pathtrace_budget_resolve(W, H, B._ptr(a), B._ptr(lv), B._ptr(o)) == 0
    assert np.array_equal(bits(o), bits(R.resolve(O, acc, lv)))


@pytest.mark.parametrize("W,H,n0", [(48, 32, 4), (33, 21, 2)])
def test_the_three_facts_in_the_oracle(B, O, W, H, n0):
    """Pilot = plain, the same noise plane, doublings = plain at 2 n0, 4 n0, 8 n0: strict oracle renders of the reference scene."""
    mc = dict(math_mode=O.MATH_MC)
    plain = {n: O.pathtrace(W, H, n, **mc) for n in (n0, 2 * n0, 4 * n0, 8 * n0)}
    zero = np.zeros((H, W), np.uint8)
    # 1. the plane spp = 2 n0 leaves after [0, n0) is half the plain accumulator: doubled and encoded it IS the plain render ...
    pilot = O.pathtrace(W, H, 2 * n0, sample_end=n0, **mc)
    assert np.array_equal(bits(B.pathtrace_budget_resolve(pilot, zero)), bits(plain[n0]))
    assert np.array_equal(bits(R.resolve(O, pilot, zero)), bits(plain[n0]))
    # ... and its [0, n0 / 2) part is half the plain render's: the two noise planes are one
    h = n0 // 2
    pilot_half = O.pathtrace(W, H, 2 * n0, sample_end=h, **mc)
    plain_half = O.pathtrace(W, H, n0, sample_end=h, **mc)
    assert np.array_equal(bits(pilot_half * f32(2)), bits(plain_half))
    nz = np.abs(pilot_half[..., :3][pilot_half[..., :3] != 0])
    assert nz.min() > 2.0 ** -100, "the one condition: nothing near the subnormal range"
    scale_pilot, scale_plain = float(f32(2 * n0) / f32(h)), float(f32(n0) / f32(h))
    var = B.pathtrace_noise(pilot_half, scale_pilot, B.pathtrace_budget_resolve(pilot, zero), 3)
    assert np.array_equal(bits(var), bits(B.pathtrace_noise(plain_half, scale_plain, plain[n0], 3)))
    assert np.array_equal(bits(var), bits(N.noise(O, plain_half, scale_plain, plain[n0], 3)))
    # 2. a doubling continues exactly, three deep: the start of round r is the plane of round r - 1 (times 0.5 after the first)
    acc = pilot
    one = np.ones((H, W), np.uint8)
    for r in (1, 2, 3):
        spp = n0 << r
        acc = R.linear_range(O, spp, spp // 2, spp, acc=acc, prescale=1.0 if r == 1 else 0.5, W=W, H=H)
        assert np.array_equal(bits(B.pathtrace_budget_resolve(acc, one)), bits(plain[spp])), r
    # (the helper's own premise: a prefix at divisor 2 m is half the prefix at divisor m, sample by sample)
    for m, k in ((n0, n0 - 1), (2 * n0, n0 + 1), (4 * n0, 4 * n0 - 1)):
        a = O.pathtrace(W, H, m, sample_end=k, **mc)
        b2 = O.pathtrace(W, H, 2 * m, sample_end=k, **mc)
        assert np.array_equal(bits(a * f32(0.5)), bits(b2)), (m, k)


def test_reference_chain_shares(O):
    """The two cases of the GPU chain test hold at least 5 % of the pixels at every level, from the oracle alone."""
    for W, H, n0, L, T in ((48, 32, 4, 2, 37.5), (33, 21, 2, 3, 30.0)):
        _, lv, _ = R.chain(O, W, H, n0, L, T, 3)
        share = np.bincount(lv.reshape(-1), minlength=L + 1) / lv.size
        assert (share >= 0.05).all(), (W, H, share)


def test_host_refusals(B):
    L = B.lib()
    W, H = 4, 3
    v = np.zeros((H, W), f32)
    lv = np.zeros((H, W), np.uint8)
    acc = np.zeros((H, W, 4), f32)
    out = np.zeros((H, W, 4), f32)

    def refused(rc, word):
        assert rc == INVALID and word in L.mc_last_error_detail().decode(), (rc, L.mc_last_error_detail())

    L.mc_last_error_detail.restype = C.c_char_p
    levels = lambda w, h, pv, t, m, po: L.mc_pathtrace_budget_levels(w, h, pv, t, m, po)   # noqa: E731
    refused(levels(0, H, B._ptr(v), 8.0, 4, B._ptr(lv)), "width and height")
    refused(levels(W, 0, B._ptr(v), 8.0, 4, B._ptr(lv)), "width and height")
    refused(levels(W, H, None, 8.0, 4, B._ptr(lv)), "NULL")
    refused(levels(W, H, B._ptr(v), 8.0, 4, None), "NULL")
    refused(levels(W, H, B._ptr(v), 8.0, 9, B._ptr(lv)), "max_level")
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30):
        refused(levels(W, H, B._ptr(v), bad, 4, B._ptr(lv)), "target")
    refused(levels(1 << 16, (1 << 15) + 1, B._ptr(v), 8.0, 4, B._ptr(lv)), "2^31")
    res = lambda w, h, pa, pl, po: L.mc_pathtrace_budget_resolve(w, h, pa, pl, po)   # noqa: E731
    refused(res(0, H, B._ptr(acc), B._ptr(lv), B._ptr(out)), "width and height")
    refused(res(W, H, None, B._ptr(lv), B._ptr(out)), "NULL")
    refused(res(W, H, B._ptr(acc), None, B._ptr(out)), "NULL")
    refused(res(W, H, B._ptr(acc), B._ptr(lv), None), "NULL")
    assert L.mc_pathtrace_budget_default_params(None) == INVALID
    assert L.mc_context_last_budget(None, None, None) == INVALID
    # the chain refuses its arguments before it asks for the context: every one of them shows without a device
    planes, spheres = B.default_scene()
    o8 = np.zeros((H, W, 4), np.uint8)

    def chain(p, b, f=out, u=None):
        return L.mc_pathtrace_render_budgeted(None, C.byref(p) if p else None, C.byref(b) if b else None, B._ptr(planes), planes.size // 12,
                                              B._ptr(spheres), spheres.size // 12, B._ptr(f), B._ptr(u), None)

    ok_p, ok_b = B.pathtrace_params(W, H, 4), B.pathtrace_budget_params()
    refused(chain(None, ok_b), "NULL")
    refused(chain(ok_p, None), "NULL")
    refused(chain(ok_p, ok_b, None, None), "exactly one")
    refused(chain(ok_p, ok_b, out, o8), "exactly one")
    refused(chain(B.pathtrace_params(W, H, 3), ok_b), "even")
    refused(chain(B.pathtrace_params(W, H, 1), ok_b), "even")
    refused(chain(B.pathtrace_params(W, H, 1 << 17), ok_b), "2^20")
    refused(chain(B.pathtrace_params(W, H, 4, row_begin=0, row_end=2), ok_b), "whole images")
    refused(chain(B.pathtrace_params(W, H, 4, row_block=1, row_stride=2), ok_b), "whole images")
    refused(chain(B.pathtrace_params(W, H, 4, sample_end=2), ok_b), "whole renders")
    refused(chain(B.pathtrace_params(W, H, 4, sample_begin=2), ok_b), "whole renders")
    refused(chain(ok_p, B.pathtrace_budget_params(radius=5)), "radius")
    refused(chain(ok_p, B.pathtrace_budget_params(max_level=9)), "max_level")
    refused(chain(ok_p, B.pathtrace_budget_params(flags=1)), "flags")
    for bad in (0.0, -2.0, float("nan"), float("inf"), 1e30):
        refused(chain(ok_p, B.pathtrace_budget_params(target=bad)), "target")
    refused(chain(ok_p, ok_b), "context")   # everything else in order: only the context is missing
