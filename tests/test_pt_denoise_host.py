"""The path-tracer denoiser without a GPU: mc_pathtrace_guides and mc_pathtrace_denoise (the kernels' own source, compiled for the host)
against tests/pt_denoise_ref.py bit for bit, the guides against a float64 computation, the quality condition on strict oracle renders,
every host refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import pt_denoise_ref as R

INVALID = 1
FILTER_SHAPES = [(1, 1), (7, 5), (64, 4), (130, 67)]   # (W, H)
OPEN_PLANES = np.array([0, 1, 0, 2.0, 0, 0, 0, 0, .75, .75, .75, 1], np.float32)           # the ceiling alone: rays going down miss
OPEN_SPHERES = np.array([0.3, 0.2, 0.5, 1.1, 0, 0, 0, 0, .9, .9, .9, 1], np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d ** 2).mean()))


def scenes(O):
    return {"reference": (O.DEFAULT_PLANES, O.DEFAULT_SPHERES), "large-sphere-walls": (O.LARGE_SPHERE_PLANES, O.LARGE_SPHERE_SPHERES),
            "open": (OPEN_PLANES, OPEN_SPHERES)}


@functools.lru_cache(maxsize=None)
def planes_for(W, H, all_miss=False):
    """A random colour plane in [0, 255.5], unit normals scattered around one direction, positions in [-0.3, 0.3] (so that the exponent e of a
    tap spreads over 0 .. 20 and the weights over many binades, not just 0 and 1), ids in {-1, 0 .. 3} in 8 x 8 patches with single pixels
    sprinkled in; shared and read-only."""
    rng = np.random.default_rng(7000 * W + H)
    rgba = (rng.random((H, W, 4), dtype=np.float32) * np.float32(255.5)).astype(np.float32)
    rgba[..., 3] = rng.random((H, W), dtype=np.float32)
    n = (np.float32([0.3, -0.5, 0.8]) + np.float32(0.3) * rng.standard_normal((H, W, 3)).astype(np.float32)).astype(np.float32)
    n = (n / np.sqrt((n * n).sum(-1, keepdims=True))).astype(np.float32)
    nt = np.concatenate([n, rng.random((H, W, 1), dtype=np.float32) * np.float32(9)], -1).astype(np.float32)
    ids = rng.integers(-1, 4, ((H + 7) // 8, (W + 7) // 8)).repeat(8, 0).repeat(8, 1)[:H, :W].astype(np.float32)
    lone = rng.random((H, W)) < 0.1
    ids[lone] = rng.integers(-1, 4, int(lone.sum()))
    if all_miss:
        ids[...] = -1
    pos = (rng.random((H, W, 3), dtype=np.float32) * np.float32(0.6) - np.float32(0.3)).astype(np.float32)
    pid = np.concatenate([pos, ids[..., None]], -1).astype(np.float32)
    for a in (rgba, nt, pid):
        a.setflags(write=False)
    return rgba, nt, pid


def test_symbols(B):
    for s in ("mc_pathtrace_denoise_default_params", "mc_pathtrace_guides", "mc_pathtrace_guides_device_async", "mc_pathtrace_denoise",
              "mc_pathtrace_denoise_device_async", "mc_pathtrace_render_denoised"):
        assert s in B.declared_symbols() and hasattr(B.lib(), s)
    d = B.pathtrace_denoise_params(12, 8)
    assert (d.width, d.height, d.passes, d.sigma_colour, d.k_normal, d.k_position, d.flags) == (12, 8, 5, 128.0, 8.0, 4.0, 0)
    assert B.lib().mc_abi_version() == 3


@pytest.mark.parametrize("scene,W,H", [("reference", 7, 5), ("reference", 60, 40), ("reference", 130, 67), ("large-sphere-walls", 60, 40),
                                       ("large-sphere-walls", 7, 5), ("open", 60, 40), ("open", 33, 9)])
def test_guides_equal_the_restatement(B, O, scene, W, H):
    planes, spheres = scenes(O)[scene]
    nt, pid = B.pathtrace_guides(W, H, planes, spheres)
    rnt, rpid = R.guides(W, H, planes, spheres)
    assert np.array_equal(bits(pid), bits(rpid)), f"position_id differs on {int((bits(pid) != bits(rpid)).any(-1).sum())} pixels"
    assert np.array_equal(bits(nt), bits(rnt)), f"normal_t differs on {int((bits(nt) != bits(rnt)).any(-1).sum())} pixels"
    ids = pid[..., 3]
    if scene == "open":   # misses, and exactly their constants
        miss = ids < 0
        assert 0 < miss.sum() < W * H
        assert np.array_equal(nt[miss], np.broadcast_to(np.float32([0, 0, 0, 1e20]), nt[miss].shape))
        assert np.array_equal(pid[miss], np.broadcast_to(np.float32([0, 0, 0, -1]), pid[miss].shape))
    else:
        assert (ids >= 0).all()
    if scene == "reference" and W >= 60:   # planes 0 .. 5, spheres 6 .. 8: the walls, the mirror and the glass are all in view
        assert {0.0, 1.0, 2.0, 3.0, 4.0, 6.0, 7.0} <= set(np.unique(ids).tolist())
    hit = ids >= 0
    assert np.allclose(np.sqrt((nt[hit][:, :3].astype(np.float64) ** 2).sum(-1)), 1.0, atol=1e-5)


def test_guides_empty_scene_is_all_miss(B):
    nt, pid = B.pathtrace_guides(9, 4, np.zeros(0, np.float32), np.zeros(0, np.float32))
    assert (nt == np.float32([0, 0, 0, 1e20])).all() and (pid == np.float32([0, 0, 0, -1])).all()


def test_guides_agree_with_float64(B, O):
    """Ids and t of the fp32 contract against the same geometry in float64 at 60 x 40: they may differ on object silhouettes only (a pixel
    whose id differs from one of its eight neighbours'), and on at most 1 % of the image.  t agrees when |dt| <= 1e-4 * t: the terms of
    det = b*b - |oc|^2 + r^2 are below 70, a dozen roundings of 2^-24 * 70 leave |d det| < 5e-5, and off the silhouettes sqrt(det) > 0.1, so
    |dt| < 3e-4 on t of 5 .. 11 - the bound asks for 2 to 4 times less than that worst case and far more than an ulp (6e-7)."""
    W, H = 60, 40
    _, pid = B.pathtrace_guides(W, H, O.DEFAULT_PLANES, O.DEFAULT_SPHERES)
    nt, _ = B.pathtrace_guides(W, H, O.DEFAULT_PLANES, O.DEFAULT_SPHERES)
    t64, id64 = R.guides64(W, H, O.DEFAULT_PLANES, O.DEFAULT_SPHERES)
    ids, t = pid[..., 3].astype(np.int64), nt[..., 3].astype(np.float64)
    pad = np.pad(ids, 1, mode="edge")
    silhouette = np.zeros((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            silhouette |= pad[dy:dy + H, dx:dx + W] != ids
    differ = (ids != id64) | (np.abs(t - t64) > 1e-4 * t64)
    share = differ.mean()
    print(f"guides fp32 against fp64 at {W} x {H}: {int(differ.sum())} of {W * H} pixels differ ({100 * share:.3f} %), "
          f"{int(silhouette.sum())} silhouette pixels; max |dt| / t elsewhere {np.max(np.abs(t - t64)[~silhouette] / t64[~silhouette]):.2e}")
    assert not (differ & ~silhouette).any(), "an id or a t differs away from every silhouette"
    assert share <= 0.01


@pytest.mark.parametrize("W,H", FILTER_SHAPES)
def test_filter_equals_the_restatement(B, O, W, H):
    rgba, nt, pid = planes_for(W, H)
    d = B.pathtrace_denoise_params(W, H)
    out = B.pathtrace_denoise(d, rgba, nt, pid)
    ref = R.denoise(O, rgba, nt, pid)
    assert np.array_equal(bits(out), bits(ref)), f"{int((bits(out) != bits(ref)).any(-1).sum())} pixels differ"
    assert np.array_equal(bits(out[..., 3]), bits(rgba[..., 3]))
    miss = pid[..., 3] < 0
    assert np.array_equal(bits(out[miss]), bits(rgba[miss]))
    if W * H > 1:
        assert not np.array_equal(out, rgba)


def test_filter_late_passes_fall_outside(B, O):
    """9 x 9 with 8 passes: from step 16 on (passes 4 .. 7) every non-centre tap of every pixel lies outside the image, and at step 8 all but
    the taps that join column or row 0 to column or row 8; the late passes run on the centre tap alone: (9/64 * c) / (9/64), which need not
    be c's bits."""
    rgba, nt, pid = planes_for(9, 9)
    out8 = B.pathtrace_denoise(B.pathtrace_denoise_params(9, 9, passes=8), rgba, nt, pid)
    assert np.array_equal(bits(out8), bits(R.denoise(O, rgba, nt, pid, passes=8)))
    assert np.isfinite(out8).all()


@pytest.mark.parametrize("kw", [dict(k_normal=0.0, k_position=0.0), dict(k_normal=0.0), dict(k_position=0.0),
                                dict(sigma_colour=1e18, k_normal=0.0, k_position=0.0, passes=2), dict(sigma_colour=0.5, passes=3),
                                dict(passes=1)])
def test_filter_weights(B, O, kw):
    W, H = 37, 21
    rgba, nt, pid = planes_for(W, H)
    out = B.pathtrace_denoise(B.pathtrace_denoise_params(W, H, **kw), rgba, nt, pid)
    assert np.array_equal(bits(out), bits(R.denoise(O, rgba, nt, pid, **kw)))


def test_filter_all_miss_returns_the_input(B, O):
    rgba, nt, pid = planes_for(23, 11, all_miss=True)
    out = B.pathtrace_denoise(B.pathtrace_denoise_params(23, 11), rgba, nt, pid)
    assert np.array_equal(bits(out), bits(rgba))
    assert np.array_equal(bits(R.denoise(O, rgba, nt, pid)), bits(rgba))


def test_filter_unaligned_host_planes(B, O):
    """A host plane that is not 16-byte aligned is taken as it is (the library copies it)."""
    W, H = 7, 5
    rgba, nt, pid = planes_for(W, H)
    store = np.zeros(W * H * 4 + 1, np.float32)
    shifted = store[1:].reshape(H, W, 4)
    assert shifted.ctypes.data % 16 != 0
    shifted[...] = rgba
    d = B.pathtrace_denoise_params(W, H)
    out = np.zeros(W * H * 4 + 1, np.float32)
    o = out[1:].reshape(H, W, 4)
    assert B.lib().mc_pathtrace_denoise(C.byref(d), B._ptr(shifted), B._ptr(nt), B._ptr(pid), B._ptr(o)) == 0
    assert np.array_equal(bits(o), bits(B.pathtrace_denoise(d, rgba, nt, pid)))


@functools.lru_cache(maxsize=None)
def oracle_render(W, H, spp):
    import __graft_entry__ as entry
    O = entry.load_oracle()
    a = O.pathtrace(W, H, spp, math_mode=O.MATH_MC)
    a.setflags(write=False)
    return a


def test_quality_on_strict_oracle_renders(B, O):
    """60 x 40, strict oracle renders: the denoised 16-spp image is at least as close to a 2048-spp render as the raw 64-spp image is
    (RMSE over RGB of the final 0 .. 255 buffer).  Measured: raw 16 spp 23.44, raw 64 spp 15.65, denoised 16 spp 11.92."""
    W, H = 60, 40
    ref = oracle_render(W, H, 2048)
    raw16, raw64 = oracle_render(W, H, 16), oracle_render(W, H, 64)
    nt, pid = B.pathtrace_guides(W, H, O.DEFAULT_PLANES, O.DEFAULT_SPHERES)
    den = B.pathtrace_denoise(B.pathtrace_denoise_params(W, H), raw16, nt, pid)
    e16, e64, eden = rmse(raw16, ref), rmse(raw64, ref), rmse(den, ref)
    spec = (pid[..., 3] == 6) | (pid[..., 3] == 7)   # first hit on the mirror or the glass sphere
    print(f"RMSE against 2048 spp at {W} x {H}: raw 16 spp {e16:.2f}, raw 64 spp {e64:.2f}, denoised 16 spp {eden:.2f}; "
          f"specular first hits ({int(spec.sum())} px): raw {rmse(raw16[spec], ref[spec]):.2f} -> {rmse(den[spec], ref[spec]):.2f}, "
          f"the rest: raw {rmse(raw16[~spec], ref[~spec]):.2f} -> {rmse(den[~spec], ref[~spec]):.2f}")
    assert eden <= e64


def _status(B, fn, *args):
    rc = fn(*args)
    return rc, B.lib().mc_last_error_detail().decode()


def test_refusals(B):
    L = B.lib()
    W, H = 7, 5
    rgba, nt, pid = planes_for(W, H)
    out = np.empty((H, W, 4), np.float32)
    planes, spheres = B.default_scene()
    p, s = B._ptr(planes), B._ptr(spheres)
    a, b = B._ptr(out), B._ptr(np.empty((H, W, 4), np.float32))
    # the guides
    for args, word in [((0, H, p, 6, s, 3, a, b), "width"), ((W, 0, p, 6, s, 3, a, b), "height"), ((W, H, None, 6, s, 3, a, b), "NULL"),
                       ((W, H, p, 6, None, 3, a, b), "NULL"), ((W, H, p, 6, s, 3, None, b), "NULL"), ((W, H, p, 6, s, 3, a, None), "NULL")]:
        rc, detail = _status(B, L.mc_pathtrace_guides, *args)
        assert rc == INVALID and "mc_pathtrace_guides" in detail and word in detail, (args, rc, detail)
    assert L.mc_pathtrace_guides(W, H, None, 0, None, 0, a, b) == 0   # empty tables may be NULL
    # the filter
    ok = dict(passes=5, sigma_colour=128.0, k_normal=8.0, k_position=4.0, flags=0)
    bad = [("passes", 0, "passes"), ("passes", 9, "passes"), ("sigma_colour", 0.0, "sigma_colour"), ("sigma_colour", -1.0, "sigma_colour"),
           ("sigma_colour", float("inf"), "sigma_colour"), ("sigma_colour", float("nan"), "sigma_colour"), ("sigma_colour", 1e-30, "sigma_colour"),
           ("sigma_colour", 1e30, "sigma_colour"), ("k_normal", -1.0, "k_normal"), ("k_normal", float("inf"), "k_normal"),
           ("k_normal", float("nan"), "k_normal"), ("k_position", -0.5, "k_position"), ("k_position", float("inf"), "k_position"),
           ("k_position", float("nan"), "k_position"), ("flags", 1, "flags")]
    for field, value, word in bad:
        d = B.pathtrace_denoise_params(W, H, **{**ok, field: value})
        rc, detail = _status(B, L.mc_pathtrace_denoise, C.byref(d), B._ptr(rgba), B._ptr(nt), B._ptr(pid), a)
        assert rc == INVALID and "mc_pathtrace_denoise" in detail and word in detail, (field, value, rc, detail)
    for w, h in [(0, H), (W, 0)]:
        d = B.pathtrace_denoise_params(w, h)
        rc, detail = _status(B, L.mc_pathtrace_denoise, C.byref(d), B._ptr(rgba), B._ptr(nt), B._ptr(pid), a)
        assert rc == INVALID and "width and height" in detail
    d = B.pathtrace_denoise_params(W, H)
    for args in [(None, B._ptr(rgba), B._ptr(nt), B._ptr(pid), a), (C.byref(d), None, B._ptr(nt), B._ptr(pid), a),
                 (C.byref(d), B._ptr(rgba), None, B._ptr(pid), a), (C.byref(d), B._ptr(rgba), B._ptr(nt), None, a),
                 (C.byref(d), B._ptr(rgba), B._ptr(nt), B._ptr(pid), None)]:
        rc, detail = _status(B, L.mc_pathtrace_denoise, *args)
        assert rc == INVALID and "NULL" in detail
    assert L.mc_pathtrace_denoise_default_params(W, H, None) == INVALID
    # a negative zero is not negative: k = -0.0 is k = 0
    d = B.pathtrace_denoise_params(W, H, k_normal=-0.0)
    assert L.mc_pathtrace_denoise(C.byref(d), B._ptr(rgba), B._ptr(nt), B._ptr(pid), a) == 0
