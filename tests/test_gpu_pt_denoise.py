"""The path-tracer denoiser on the MI355X: both device kernels against tests/pt_denoise_ref.py bit for bit between guard rows (separate
output and in place), mc_pathtrace_render_denoised against the chain of the separate calls and against the quality condition, the app's
--denoise on both save routes, the timing record, every device-side refusal."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import pt_denoise_ref as R
from test_pt_denoise_host import FILTER_SHAPES, bits, planes_for, rmse, scenes

pytestmark = pytest.mark.gpu

INVALID = 1
GUIDE_CASES = [("reference", 7, 5), ("reference", 60, 40), ("reference", 130, 67), ("large-sphere-walls", 60, 40), ("open", 60, 40),
               ("reference", 257, 130)]   # the last: 5 blocks of 64 columns and 33 of 4 rows, both with a partial last block
SHAPES = FILTER_SHAPES + [(257, 130)]     # (W, H)
GUARD = -7.0


def guarded(torch, plane=None, shape=None):
    """A device plane between two guard rows; returns (whole tensor, pointer to the plane inside it)."""
    H, W = (plane.shape if plane is not None else shape)[:2]
    t = torch.full((H + 2, W, 4), GUARD, dtype=torch.float32, device="cuda")
    if plane is not None:
        t[1:-1] = torch.from_numpy(np.array(plane, np.float32)).cuda()
    return t, t[1:].data_ptr()


def inner(t):
    a = t.cpu().numpy()
    assert (a[0] == GUARD).all() and (a[-1] == GUARD).all(), "a write outside the plane"
    return a[1:-1]


@pytest.mark.parametrize("scene,W,H", GUIDE_CASES, ids=[f"{s}-{w}x{h}" for s, w, h in GUIDE_CASES])
def test_guides_kernel_is_the_restatement(ctx, B, O, scene, W, H):
    import torch
    planes, spheres = scenes(O)[scene]
    d_nt, p_nt = guarded(torch, shape=(H, W))
    d_pid, p_pid = guarded(torch, shape=(H, W))
    torch.cuda.synchronize()
    ctx.pathtrace_guides_device(W, H, p_nt, p_pid, planes, spheres)
    ctx.synchronize()
    nt, pid = inner(d_nt), inner(d_pid)
    rnt, rpid = R.guides(W, H, planes, spheres)
    assert np.array_equal(bits(pid), bits(rpid)), int((bits(pid) != bits(rpid)).any(-1).sum())
    assert np.array_equal(bits(nt), bits(rnt)), int((bits(nt) != bits(rnt)).any(-1).sum())


def run_filter(ctx, d, rgba, nt, pid, in_place):
    """mc_pathtrace_denoise_device_async on uploaded planes, every plane between guard rows; returns the output and the three inputs as
    they are afterwards."""
    import torch
    t_rgba, p_rgba = guarded(torch, rgba)
    t_nt, p_nt = guarded(torch, nt)
    t_pid, p_pid = guarded(torch, pid)
    t_out, p_out = (t_rgba, p_rgba) if in_place else guarded(torch, shape=rgba.shape)
    torch.cuda.synchronize()
    ctx.pathtrace_denoise_device(d, p_rgba, p_nt, p_pid, p_out)
    ctx.synchronize()
    return inner(t_out), inner(t_rgba), inner(t_nt), inner(t_pid)


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_filter_kernel_is_the_restatement(ctx, B, O, W, H):
    rgba, nt, pid = planes_for(W, H)
    d = B.pathtrace_denoise_params(W, H)
    want = R.denoise(O, rgba, nt, pid)
    out, a, b, c = run_filter(ctx, d, rgba, nt, pid, in_place=False)
    assert np.array_equal(bits(out), bits(want)), int((bits(out) != bits(want)).any(-1).sum())
    assert np.array_equal(bits(a), bits(rgba)) and np.array_equal(bits(b), bits(nt)) and np.array_equal(bits(c), bits(pid)), "an input changed"
    out, _, b, c = run_filter(ctx, d, rgba, nt, pid, in_place=True)
    assert np.array_equal(bits(out), bits(want)), "in place"
    assert np.array_equal(bits(b), bits(nt)) and np.array_equal(bits(c), bits(pid)), "a guide plane changed"


@pytest.mark.parametrize("passes", [1, 2, 8])
def test_filter_kernel_pass_counts(ctx, B, O, passes):
    """One pass in place goes through the scratch and a copy; two end on the other scratch plane; eight on 9 x 9 run the late passes on the
    centre tap alone."""
    rgba, nt, pid = planes_for(9, 9)
    d = B.pathtrace_denoise_params(9, 9, passes=passes)
    want = R.denoise(O, rgba, nt, pid, passes=passes)
    for in_place in (False, True):
        out = run_filter(ctx, d, rgba, nt, pid, in_place)[0]
        assert np.array_equal(bits(out), bits(want)), (passes, in_place)


def test_filter_kernel_weights_and_all_miss(ctx, B, O):
    W, H = 37, 21
    rgba, nt, pid = planes_for(W, H)
    for kw in (dict(k_normal=0.0, k_position=0.0), dict(sigma_colour=0.5, passes=3)):
        out = run_filter(ctx, B.pathtrace_denoise_params(W, H, **kw), rgba, nt, pid, False)[0]
        assert np.array_equal(bits(out), bits(R.denoise(O, rgba, nt, pid, **kw))), kw
    rgba, nt, pid = planes_for(23, 11, all_miss=True)
    out = run_filter(ctx, B.pathtrace_denoise_params(23, 11), rgba, nt, pid, False)[0]
    assert np.array_equal(bits(out), bits(rgba))


# ---- the fused call ----------------------------------------------------------------------------------------------------------------------
W2, H2 = 120, 80


_RENDERS = {}


def strict_render(ctx, B, spp):
    """The strict render of the reference scene at 120 x 80, made once and shared read-only."""
    if spp not in _RENDERS:
        a = ctx.pathtrace(B.pathtrace_params(W2, H2, spp))
        a.setflags(write=False)
        _RENDERS[spp] = a
    return _RENDERS[spp]


def test_denoised_is_the_chain_of_the_separate_calls(ctx, B, O):
    import torch
    p = B.pathtrace_params(W2, H2, 16)
    d = B.pathtrace_denoise_params(W2, H2)
    fused = ctx.pathtrace_denoised(p, d)
    k_ms, c_ms = ctx.last_timing()
    assert k_ms > 0.0 and c_ms > 0.0, "the timing record covers the fused call"
    # render, then guides, then filter, each through its own device call
    t_rgba, p_rgba = guarded(torch, shape=(H2, W2))
    t_nt, p_nt = guarded(torch, shape=(H2, W2))
    t_pid, p_pid = guarded(torch, shape=(H2, W2))
    t_out, p_out = guarded(torch, shape=(H2, W2))
    torch.cuda.synchronize()
    ctx.pathtrace_device(p, p_rgba)
    ctx.pathtrace_guides_device(W2, H2, p_nt, p_pid)
    ctx.pathtrace_denoise_device(d, p_rgba, p_nt, p_pid, p_out)
    ctx.synchronize()
    raw, chain = inner(t_rgba), inner(t_out)
    assert np.array_equal(bits(raw), bits(strict_render(ctx, B, 16))), "the separate render is the blocking render"
    assert np.array_equal(bits(fused), bits(chain))
    # ... and the host calls on the same render
    nt, pid = B.pathtrace_guides(W2, H2)
    assert np.array_equal(bits(inner(t_nt)), bits(nt)) and np.array_equal(bits(inner(t_pid)), bits(pid))
    assert np.array_equal(bits(fused), bits(B.pathtrace_denoise(d, raw, nt, pid)))
    # the RGBA8 form: the vec4 output converted and rotated as mc_pathtrace_render_rgba8 does
    fused8 = ctx.pathtrace_denoised(p, d, rgba8=True)
    assert np.array_equal(fused8, ctx.convert_rgba8(fused, 1.0, rotate180=True))
    assert np.array_equal(fused8, O.rotate180(O.float_to_rgba8(fused, 1.0).reshape(H2, W2, 4), W2, H2))
    # a plain render afterwards is what it was
    assert np.array_equal(bits(ctx.pathtrace(p)), bits(strict_render(ctx, B, 16)))


def test_denoised_quality(ctx, B, O):
    """120 x 80 against a 4096-spp strict render: the denoised 16-spp image (strict, and fast math) is at least as close as the raw 64-spp
    strict image.  Measured: raw 16 spp 23.34, raw 64 spp 15.67, denoised 16 spp 9.39 strict and 9.39 fast (the figures are printed)."""
    ref, raw16, raw64 = strict_render(ctx, B, 4096), strict_render(ctx, B, 16), strict_render(ctx, B, 64)
    den = ctx.pathtrace_denoised(B.pathtrace_params(W2, H2, 16))
    fast = ctx.pathtrace_denoised(B.pathtrace_params(W2, H2, 16, math_mode=B.PT_MATH_FAST))
    _, pid = B.pathtrace_guides(W2, H2)
    spec = (pid[..., 3] == 6) | (pid[..., 3] == 7)
    e16, e64, eden, efast = rmse(raw16, ref), rmse(raw64, ref), rmse(den, ref), rmse(fast, ref)
    print(f"RMSE against 4096 spp at {W2} x {H2}: raw 16 spp {e16:.2f}, raw 64 spp {e64:.2f}, denoised 16 spp {eden:.2f} (fast math {efast:.2f}); "
          f"specular first hits ({int(spec.sum())} px): raw {rmse(raw16[spec], ref[spec]):.2f} -> {rmse(den[spec], ref[spec]):.2f}, "
          f"the rest: raw {rmse(raw16[~spec], ref[~spec]):.2f} -> {rmse(den[~spec], ref[~spec]):.2f}")
    assert eden <= e64
    assert efast <= e64
    assert np.array_equal(bits(den[..., 3]), bits(raw16[..., 3]))


def test_denoised_generic_scene(ctx, B, O):
    """A scene the generic kernel renders (the sphere-walled room): the fused call is the chain there too."""
    planes, spheres = O.LARGE_SPHERE_PLANES, O.LARGE_SPHERE_SPHERES
    W, H = 66, 41
    p = B.pathtrace_params(W, H, 4)
    d = B.pathtrace_denoise_params(W, H, passes=3)
    fused = ctx.pathtrace_denoised(p, d, planes, spheres)
    nt, pid = B.pathtrace_guides(W, H, planes, spheres)
    assert np.array_equal(bits(fused), bits(B.pathtrace_denoise(d, ctx.pathtrace(p, planes, spheres), nt, pid)))


# ---- the app ---------------------------------------------------------------------------------------------------------------------------
def test_app_denoise(ctx, B, O, tmp_path):
    from PIL import Image
    app = os.path.join(os.path.dirname(os.path.dirname(B.LIB_PATH)), "bin", "pathtracer")
    W, H, spp = 60, 40, 8
    p = B.pathtrace_params(W, H, spp)

    def run(*extra):
        r = subprocess.run([app, str(spp), str(H), "--out", "o.png", "--quiet", "--timing-json", "--full-teardown"] + list(extra),
                           capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"timing_ms"')][0])
        return np.asarray(Image.open(tmp_path / "o.png").convert("RGBA")), (tmp_path / "o.png").read_bytes(), r.stdout, j

    want5 = ctx.pathtrace_denoised(p, rgba8=True)
    want3 = ctx.pathtrace_denoised(p, B.pathtrace_denoise_params(W, H, passes=3), rgba8=True)
    files = []
    for route in ([], ["--gpu-postprocess"]):
        img, data, out, j = run("--denoise", *route)
        assert np.array_equal(img, want5), route
        assert j["denoise"] == 5 and j["timing_ms"]["kernel"] > 0
        line = [l for l in out.splitlines() if l.startswith("denoise: ")]
        assert len(line) == 1 and line[0].startswith("denoise: 5 passes, ") and "ms device time" in line[0], out
        files.append(data)
        img, _, out, j = run("--denoise=3", *route)
        assert np.array_equal(img, want3) and j["denoise"] == 3 and "denoise: 3 passes" in out
    assert files[0] == files[1], "both save routes write one file"
    img, _, _, j = run("--denoise", "3", "--math", "fast")
    fast = ctx.pathtrace_denoised(B.pathtrace_params(W, H, spp, math_mode=B.PT_MATH_FAST), B.pathtrace_denoise_params(W, H, passes=3), rgba8=True)
    assert j["denoise"] == 3 and np.array_equal(img, fast)
    # without the flag: the plain render's file, on both routes, and no line
    plain = O.rotate180(O.float_to_rgba8(O.pathtrace(W, H, spp, math_mode=O.MATH_MC), 1.0).reshape(H, W, 4), W, H)
    files = []
    for route in ([], ["--gpu-postprocess"]):
        img, data, out, j = run(*route)
        assert np.array_equal(img, plain) and j["denoise"] == 0 and "denoise:" not in out
        files.append(data)
    assert files[0] == files[1]
    for bad in (["--denoise", "9"], ["--denoise=0"], ["--denoise=x"], ["--denoise", "--gpus", "2"]):
        r = subprocess.run([app, str(spp), str(H), "--quiet"] + bad, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode != 0 and "--denoise" in r.stdout, (bad, r.stdout)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def refused(B, call, says=None):
    with pytest.raises(B.McError) as e:
        call()
    assert e.value.status == INVALID, e.value
    if says:
        assert says in str(e.value), e.value


def test_device_refusals(ctx, B):
    import torch
    W, H = 8, 8
    k = torch.zeros((5, H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    a, n, x, o, o2 = (k[i].data_ptr() for i in range(5))
    d = B.pathtrace_denoise_params(W, H)
    den = lambda *args: (lambda: ctx.pathtrace_denoise_device(*args))   # noqa: E731
    refused(B, den(d, 0, n, x, o), "NULL")
    refused(B, den(d, a, 0, x, o), "NULL")
    refused(B, den(d, a, n, 0, o), "NULL")
    refused(B, den(d, a, n, x, 0), "NULL")
    refused(B, den(d, a + 4, n, x, o), "aligned")
    refused(B, den(d, a, n + 8, x, o), "aligned")
    refused(B, den(d, a, n, x, o + 4), "aligned")
    refused(B, den(d, a, n, x, n), "overlaps")
    refused(B, den(d, a, n, x, x), "overlaps")
    refused(B, den(d, a, n, x, a + 16 * W), "overlaps")   # one row further: neither the input nor clear of it
    refused(B, den(d, a, a, x, o), "overlaps")
    for kw, word in [(dict(passes=0), "passes"), (dict(passes=9), "passes"), (dict(sigma_colour=0.0), "sigma_colour"),
                     (dict(sigma_colour=float("nan")), "sigma_colour"), (dict(k_normal=-1.0), "k_normal"),
                     (dict(k_position=float("inf")), "k_position"), (dict(flags=2), "flags")]:
        refused(B, den(B.pathtrace_denoise_params(W, H, **kw), a, n, x, o), word)
    refused(B, den(B.pathtrace_denoise_params(0, H), a, n, x, o), "width and height")
    gd = lambda *args: (lambda: ctx.pathtrace_guides_device(*args))   # noqa: E731
    refused(B, gd(W, H, 0, x), "NULL")
    refused(B, gd(W, H, n, 0), "NULL")
    refused(B, gd(0, H, n, x), "width and height")
    refused(B, gd(W, 0, n, x), "width and height")
    refused(B, gd(W, H, n + 4, x), "aligned")
    refused(B, gd(W, H, n, n), "overlap")
    L = B.lib()
    planes, spheres = B.default_scene()
    assert L.mc_pathtrace_guides_device_async(ctx._h, W, H, None, 6, B._ptr(spheres), 3, n, x, None) == INVALID
    assert L.mc_pathtrace_guides_device_async(None, W, H, B._ptr(planes), 6, B._ptr(spheres), 3, n, x, None) == INVALID
    assert L.mc_pathtrace_denoise_device_async(None, C.byref(d), a, n, x, o, None) == INVALID
    ctx.pathtrace_guides_device(W, H, n, x)
    ctx.pathtrace_denoise_device(d, a, n, x, a)   # in place is the stated exception
    ctx.pathtrace_denoise_device(d, a, n, x, o2)
    ctx.synchronize()


def test_fused_refusals(ctx, B):
    L = B.lib()
    W, H = 16, 8
    planes, spheres = B.default_scene()
    P, S = B._ptr(planes), B._ptr(spheres)
    f = np.empty((H, W, 4), np.float32)
    u = np.empty((H, W, 4), np.uint8)

    def call(p, d, out_f=B._ptr(f), out_u=None, pl=P, sp=S, c=ctx._h):
        rc = L.mc_pathtrace_render_denoised(c, C.byref(p) if p is not None else None, C.byref(d) if d is not None else None, pl, 6, sp, 3, out_f, out_u)
        return rc, L.mc_last_error_detail().decode()

    ok_p, ok_d = B.pathtrace_params(W, H, 2), B.pathtrace_denoise_params(W, H)
    assert call(ok_p, ok_d)[0] == 0
    for args, word in [((None, ok_d), "NULL"), ((ok_p, None), "NULL"), ((ok_p, ok_d, None, None), "exactly one"),
                       ((ok_p, ok_d, B._ptr(f), B._ptr(u)), "exactly one"),
                       ((B.pathtrace_params(W, H, 2, row_begin=0, row_end=4), ok_d), "whole images"),
                       ((B.pathtrace_params(W, H, 2, row_begin=4), ok_d), "whole images"),
                       ((B.pathtrace_params(W, H, 2, row_block=2, row_stride=4), ok_d), "whole images"),
                       ((B.pathtrace_params(W, H, 2, sample_end=1), ok_d), "whole renders"),
                       ((B.pathtrace_params(W, H, 2, sample_begin=1), ok_d), "whole renders"),
                       ((ok_p, B.pathtrace_denoise_params(W, H + 1)), "width and height must be the render's"),
                       ((ok_p, B.pathtrace_denoise_params(W, H, passes=9)), "passes"),
                       ((ok_p, B.pathtrace_denoise_params(W, H, sigma_colour=-2.0)), "sigma_colour"),
                       ((ok_p, B.pathtrace_denoise_params(W, H, k_normal=float("nan"))), "k_normal"),
                       ((ok_p, B.pathtrace_denoise_params(W, H, flags=1)), "flags"),
                       ((B.pathtrace_params(0, H, 2), ok_d), "width and height")]:
        rc, detail = call(*args)
        assert rc == INVALID and "mc_pathtrace_render_denoised" in detail and word in detail, (word, rc, detail)
    assert call(ok_p, ok_d, c=None)[0] == INVALID
    assert call(ok_p, ok_d, pl=None)[0] == INVALID
    assert call(B.pathtrace_params(W, H, 2, math_mode=7), ok_d)[0] == INVALID
    assert call(ok_p, ok_d)[0] == 0   # the context renders on after every refusal
