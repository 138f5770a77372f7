"""The cases of the fast-block audit (mc_hook_mandel_block_audit, mc_hook_mandel_perturb_block_audit), shared by
tests/test_gpu_mandel_block_audit.py (the device audit) and tests/test_mandel_block_audit_host.py (the CPU census of the branches the
cases reach).  Plain data and host-only helpers: no device is touched here.  Not a conftest: the test files import it."""
import numpy as np

import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R

NONE = 0xFFFFFFFF   # first_bad of a lane without a bad block

REF_VIEW = dict(centre=(-0.445, 0.0), scale=(2.34, 2.34))
K4_CENTRE = (-0.7436438870371587, 0.13182590420531198)

# ---- F32, DS, F64: views the parity tests trust (tests/test_gpu_parity.py, tests/test_gpu_mandel_f64.py), at small shapes -------------
F32_CASES = [
    dict(id="f32 default M523", W=64, H=48, M=523, fma=False, **REF_VIEW),                                    # M % 8 != 0: the tail
    dict(id="f32 seahorse M2049", W=64, H=48, M=2049, fma=False, centre=(-0.75, 0.1), scale=(0.05, 0.05)),    # escaping beside cycling lanes
    dict(id="f32 default fma", W=64, H=48, M=523, fma=True, **REF_VIEW),
]
DS_CASES = [   # c ~ i: zx passes below 2^-50 every other iteration, the fma product hands over to the Dekker one
    dict(id="ds c~i 1e-15", W=64, H=48, M=600, centre=(0.0, 1.0), scale=(1e-15, 1e-15)),
    dict(id="ds c~i 3e-14", W=64, H=48, M=600, centre=(0.0, 1.0), scale=(3e-14, 2e-14)),
    dict(id="ds K4 1e-8", W=48, H=32, M=2000, centre=K4_CENTRE, scale=(1e-8, 1e-8 * 2 / 3)),
]
F64_CASES = [
    dict(id="f64 K4 1e-12", W=64, H=48, M=20000, centre=K4_CENTRE, scale=(1e-12, 0.75e-12)),
    dict(id="f64 K4 1e-8", W=64, H=48, M=5000, centre=K4_CENTRE, scale=(1e-8, 1e-8 * 2.0 / 3.0)),
]
BLOCK = {"f32": 8, "ds": 4, "f64": 8, "perturb": 8, "deep": 8}   # the block length U each state's kernel is launched with

# ---- PERTURB (deep = 0): real orbits, offsets dc ------------------------------------------------------------------------------------
PERTURB_CASES = [
    dict(id="perturb boundary 1e-20", W=64, H=48, M=4000, centre="boundary", scale=(1e-20, 1e-20)),   # escaping reference: L < M
    dict(id="perturb K4 1e-20", W=64, H=48, M=20000, centre=R.DEEP_CENTRE, scale=(1e-20, 1e-20)),
    dict(id="perturb 1e-100", W=40, H=24, M=3000, centre=("-0.75", "0.1"), scale=(1e-100, 1e-100)),
]

# ---- Deep (deep = 1) ----------------------------------------------------------------------------------------------------------------
# kind "view": a Misiurewicz point at a decimal depth (D.view); "centre": a decimal centre at a depth; "shallow": a plain orbit run by
# the rescaled loop with E = 0 (what MC_MANDEL_PERTURB_FORCE_DEEP renders); "table": an orbit table no centre gives, with its own lanes.
# zeros: the table holds Z_j = 0 (1 <= j < L) and every lane stays scaled (or L is no longer than a block), so no fast block may be
# accepted (the host test checks the premise).


def _low_window_table():
    """Z_1 .. Z_210 = 1.2: |delta| grows by 2.4 per step, so |w| passes 2^256 after about 203 steps and S is raised (the high side).
    Then entries of 2^-400: w' = (2 Z + delta) w + u 2^(E - S) falls to |u| 2^-257 < 2^-256 in one step (the low side)."""
    Z = np.zeros((241, 2))
    Z[1:211, 0] = 1.2
    Z[211:, 0] = 2.0 ** -400
    Z[211::2, 1] = -(2.0 ** -400)
    return Z


_LOW_LANES = [(0.3, -0.2), (-0.5, 0.5), (0.71, 0.0), (0.0, -0.33), (0.999, 0.999), (-0.125, 0.0625), (0.45, 0.45), (-0.6, -0.01)]

DEEP_CASES = [
    dict(id="deep M33 5e-290", kind="view", point=D.M33, depth="5e-290", M=2000, W=48, H=32, mant=None),
    dict(id="deep M33 1e-300", kind="view", point=D.M33, depth="1e-300", M=2000, W=48, H=32, mant=None),
    dict(id="deep M33 1e-1000", kind="view", point=D.M33, depth="1e-1000", M=6000, W=48, H=32, mant=None),
    dict(id="deep M41 1e-900", kind="view", point=D.M41, depth="1e-900", M=8000, W=48, H=32, mant=(-0.7, 0.45)),
    dict(id="deep centre 0", kind="centre", centre=("0", "0"), depth="1e-1000", M=200, W=48, H=32, zeros=True),
    dict(id="deep centre -1", kind="centre", centre=("-1", "0"), depth="1e-1000", M=200, W=48, H=32, zeros=True),
    dict(id="deep nucleus3", kind="centre", centre="nucleus3", depth="1e-1000", M=300, W=48, H=32),
    dict(id="deep exterior 0.26", kind="centre", centre=("0.26", "0"), depth="1e-1000", M=100, W=48, H=32),
    dict(id="deep exterior -0.75+0.05i", kind="centre", centre=("-0.75", "0.05"), depth="1e-1000", M=200, W=48, H=32),
    dict(id="deep synthetic zeros", kind="table", Z=np.array([[0.0, 0.0], [-1.0, 0.0], [0.0, 0.0], [-1.0, 0.0]]), E=-3000, M=40,
         lanes=[(0.3, -0.2), (0.0, 0.0), (-0.5, 0.5)], zeros=True),
    dict(id="deep low window", kind="table", Z=_low_window_table(), E=-3000, M=256, lanes=_LOW_LANES),
    dict(id="deep forced 1e-100", kind="shallow", centre=("-0.75", "0.1"), scale=(1e-100, 1e-100), M=3000, W=40, H=24),
    dict(id="deep forced 2^-950", kind="shallow", centre=("-1.25", "0.001"), scale=(2.0 ** -950, 2.0 ** -950), M=2000, W=24, H=16),
    dict(id="deep forced 0.05", kind="shallow", centre=("-0.75", "0.1"), scale=(0.05, 0.03), M=1003, W=77, H=45),
]


def ids(cases):
    return [c["id"] for c in cases]


def boundary_centre():
    """The boundary point of tests/test_gpu_mandel_perturb.py: 2^-70 deep, its own orbit escapes (L < 4000)."""
    return R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 4000, 70, 134)


def _grid(ax, ay):
    """Per-lane offsets of an H x W image, row-major: lane y * W + x has (ax[x], ay[y])."""
    X = np.broadcast_to(ax[None, :], (ay.size, ax.size))
    Y = np.broadcast_to(ay[:, None], (ay.size, ax.size))
    return np.ascontiguousarray(X).ravel(), np.ascontiguousarray(Y).ravel()


def perturb_orbit(B, case):
    """The B.Orbit of a PERTURB case or a deep case of kind view / centre / shallow (the caller closes it)."""
    if case.get("kind") == "view":
        c, m, E = D.view(case["point"], case["depth"])
        return B.Orbit(c[0], c[1], *(case["mant"] or m), case["M"], E)
    if case.get("kind") == "centre":
        c = D.nucleus(3, D.NUCLEUS3, 4000, 200) if case["centre"] == "nucleus3" else case["centre"]
        m, E = B.scale_from_text(case["depth"])
        return B.Orbit(c[0], c[1], m, m, case["M"], E)
    c = boundary_centre() if case["centre"] == "boundary" else case["centre"]
    return B.Orbit(c[0], c[1], case["scale"][0], case["scale"][1], case["M"])


def lanes(B, case):
    """(Z, ux, uy, E, orbit or None) of a PERTURB or deep case: the orbit table ((L + 1, 2) float64), the per-lane offsets (dc for
    PERTURB and the shallow kind with E = 0, the mantissa offsets u otherwise) and the exponent.  The orbit is open: the caller closes it."""
    if case.get("kind") == "table":
        ux, uy = (np.array([l[k] for l in case["lanes"]], np.float64) for k in (0, 1))
        return np.ascontiguousarray(case["Z"], np.float64), ux, uy, case["E"], None
    o = perturb_orbit(B, case)
    deep = case.get("kind") in ("view", "centre")
    assert o.deep == deep, case["id"]
    ux, uy = _grid(R.dc_axis(case["W"], o.scale[0]), R.dc_axis(case["H"], o.scale[1]))
    return o.table(), ux, uy, (o.scale_exp2 if deep else 0), o


def fma_iters(W, H, M, centre, scale):
    """The fp32 loop of MC_MANDEL_FMA restated: nzx = fma(zx, zx, -sy) + cx, nzy = fma(2 zx, zy, cy), everything else as the parity
    loop.  c as mandelbrot.hip's c table (fp32, source order).  Each fma is evaluated in float64 with round-to-odd (53 >= 2 * 24 + 2
    bits), so the final rounding to float32 is the single rounding of a true fma."""
    f32 = np.float32
    gx = np.arange(W, dtype=f32) / f32(W)
    gy = np.arange(H, dtype=f32) / f32(H)
    cxa = f32(centre[0]) + (gx - f32(0.5)) * f32(scale[0])
    cya = f32(centre[1]) + (gy - f32(0.5)) * f32(scale[1])
    cx, cy = _grid(cxa.astype(f32), cya.astype(f32))
    n = np.full(cx.size, M, np.uint32)
    live = np.arange(cx.size)
    zx = np.zeros_like(cx); zy = np.zeros_like(cx); sy = np.zeros_like(cx)
    two = f32(2.0)
    with np.errstate(all="ignore"):
        for i in range(M):
            nzx = fma32(zx, zx, -sy) + cx
            nzy = fma32(two * zx, zy, cy)
            zx, zy = nzx, nzy
            sx = zx * zx
            sy = zy * zy
            esc = (sx + sy) > two
            if esc.any():
                n[live[esc]] = i
                keep = ~esc
                live, cx, cy, zx, zy, sy = live[keep], cx[keep], cy[keep], zx[keep], zy[keep], sy[keep]
                if live.size == 0:
                    break
    return n.reshape(H, W)


def fma32(a, b, c):
    """fma(a, b, c) on float32 arrays, correctly rounded once (finite operands): the product is exact in float64; the sum is rounded
    to odd in float64 (TwoSum gives the exact error), then to nearest in float32."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    inexact = (err != 0.0) & np.isfinite(s)
    # truncate towards zero where the exact sum lies between s and zero, then force the last bit to 1
    towards_zero = inexact & ((err < 0.0) == (s > 0.0)) & (s != 0.0)
    bits = np.where(towards_zero, bits - 1, bits)
    bits = np.where(inexact, bits | 1, bits)
    return bits.view(np.float64).astype(np.float32)
