"""Per-pixel sample budgets restated in numpy (TEST INFRASTRUCTURE): include/mc_compute.h's contract of mc_pathtrace_budget_levels,
mc_pathtrace_budget_resolve and the bucketed lists, one ufunc per fp32 operation in the order the contract states, so the library's host
calls and device kernels must agree with it bit for bit; and the expected result of mc_pathtrace_render_budgeted built from nothing but
renders of the CPU oracle.  pow045 goes through the oracle's mc_math, the library's strict one."""
import numpy as np

import pt_noise_ref as N

f32 = np.float32


def levels(variance, target, max_level):
    """mc_pathtrace_budget_levels: uint8, the shape of variance.  t = V; l = 0; while (l < max_level && t > tau2) { t = t * 0.5f; l++; }"""
    tau2 = f32(target) * f32(target)
    t = np.array(variance, f32)
    lv = np.zeros(t.shape, np.uint8)
    with np.errstate(all="ignore"):
        for _ in range(max_level):
            go = t > tau2                       # NaN: False, the pixel stays where it is; +inf: True at every step
            lv = np.where(go, lv + np.uint8(1), lv).astype(np.uint8)
            t = np.where(go, t * f32(0.5), t).astype(f32)   # (a pixel that stopped would not pass the test again: its t stays)
    return lv


def encode(O, x):
    """encode_strict of every element: pow045(min(max(x, 0), 1)) * 255 + 0.5 with GLSL's min and max."""
    x = np.ascontiguousarray(x, f32)
    with np.errstate(all="ignore"):
        lo = np.where(x < f32(0), f32(0), x)
        cl = np.where(f32(1) < lo, f32(1), lo).astype(f32)
        return (O.mc_math("pow045", cl).reshape(cl.shape) * f32(255) + f32(0.5)).astype(f32)


def resolve(O, acc, lv):
    """mc_pathtrace_budget_resolve: out.rgb = encode_strict(acc.rgb * (level == 0 ? 2 : 1)), out.w = acc.w."""
    acc = np.ascontiguousarray(acc, f32)
    m = np.where(np.asarray(lv) == 0, f32(2), f32(1)).astype(f32)[..., None]
    out = acc.copy()
    with np.errstate(all="ignore"):
        out[..., :3] = encode(O, acc[..., :3] * m)
    return out


def lists(lv, max_level):
    """The list's specification: (counts[0 .. max_level], the storage indices of each level sorted, highest level first)."""
    flat = np.asarray(lv, np.uint8).reshape(-1)
    counts = np.bincount(flat, minlength=max_level + 1)
    buckets = [np.flatnonzero(flat == l).astype(np.uint32) for l in range(max_level, -1, -1)]
    return counts, buckets


def sorted_buckets(lst, counts, max_level):
    """A device list cut into its buckets (highest level first), each sorted: the order inside a bucket is unspecified."""
    out, at = [], 0
    for l in range(max_level, -1, -1):
        out.append(np.sort(lst[at:at + int(counts[l])]))
        at += int(counts[l])
    return out


def linear_range(O, spp, begin, end, acc=None, prescale=1.0, **scene):
    """What the list render leaves in a listed pixel, from the oracle alone: acc * prescale continued over samples [begin, end) at divisor
    spp, LINEAR even when end == spp.  The oracle encodes after sample spp - 1, so the range is rendered at divisor 2 spp from half the
    start and doubled: exact scalings by 2 (fact 1 of the contract, asserted in test_pt_budget_host.py)."""
    start = None
    if begin > 0:
        start = (np.ascontiguousarray(acc, f32) * f32(prescale) * f32(0.5)).astype(f32)
    half = O.pathtrace(scene.pop("W"), scene.pop("H"), 2 * spp, math_mode=O.MATH_MC, sample_begin=begin, sample_end=end, acc=start, **scene)
    return (half * f32(2)).astype(f32)


def chain(O, W, H, n0, max_level, target, radius, **scene):
    """mc_pathtrace_render_budgeted's promise from oracle renders alone: (image, levels, variance).  levels: the numpy levels of the numpy
    noise plane of the plain n0 render; image[p]: the plain oracle render at spp = n0 << levels[p]."""
    plain = [O.pathtrace(W, H, n0 << l, math_mode=O.MATH_MC, **scene) for l in range(max_level + 1)]
    half = O.pathtrace(W, H, n0, math_mode=O.MATH_MC, sample_end=n0 // 2, **scene)
    var = N.noise(O, half, f32(n0) / f32(n0 // 2), plain[0], radius)
    lv = levels(var, target, max_level)
    image = np.zeros((H, W, 4), f32)
    for l in range(max_level + 1):
        image[lv == l] = plain[l][lv == l]
    return image, lv, var
