"""The noise plane and the noise-guided filter on the MI355X: the device kernels against the host calls bit for bit between guard rows
(separate output and in place, twice), mc_pathtrace_render_denoised_adaptive against the host calls on the plain render (strict) and
against the chain of the separate device calls (fast math), the plain fused call before and after it, the app's --noise-guided, every
device-side refusal."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_pt_denoise import GUARD, guarded, inner, refused
from test_pt_denoise_host import bits, planes_for
from test_pt_noise_host import SHAPES as HOST_SHAPES
from test_pt_noise_host import noise_inputs, variance_for

pytestmark = pytest.mark.gpu

INVALID = 1
SHAPES = HOST_SHAPES + [(257, 130)]   # the last: 5 blocks of 64 columns and 33 of 4 rows, both with a partial last block


def guarded_plane(torch, plane=None, shape=None):
    """A device plane of one float per pixel between two guard rows; returns (whole tensor, pointer to the plane inside it)."""
    H, W = (plane.shape if plane is not None else shape)[:2]
    t = torch.full((H + 2, W), GUARD, dtype=torch.float32, device="cuda")
    if plane is not None:
        t[1:-1] = torch.from_numpy(np.array(plane, np.float32)).cuda()
    return t, t[1:].data_ptr()


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_noise_kernels_are_the_host_call(ctx, B, W, H):
    import torch
    half, full = noise_inputs(W, H)
    t_half, p_half = guarded(torch, half)
    t_full, p_full = guarded(torch, full)
    for scale, radius in ((2.0, 0), (2.0, 3), (2.5, 1), (2.5, 4)):
        want = B.pathtrace_noise(half, scale, full, radius)
        for _ in range(2):   # twice: the same bits
            t_var, p_var = guarded_plane(torch, shape=(H, W))
            torch.cuda.synchronize()
            ctx.pathtrace_noise_device(W, H, p_half, scale, p_full, radius, p_var)
            ctx.synchronize()
            got = inner(t_var)
            assert np.array_equal(bits(got), bits(want)), (scale, radius, int((bits(got) != bits(want)).sum()))
    assert np.array_equal(bits(inner(t_half)), bits(half)) and np.array_equal(bits(inner(t_full)), bits(full)), "an input changed"


def run_filter(ctx, d, k_noise, rgba, nt, pid, var, in_place):
    import torch
    t_rgba, p_rgba = guarded(torch, rgba)
    t_nt, p_nt = guarded(torch, nt)
    t_pid, p_pid = guarded(torch, pid)
    t_var, p_var = guarded_plane(torch, var)
    t_out, p_out = (t_rgba, p_rgba) if in_place else guarded(torch, shape=rgba.shape)
    torch.cuda.synchronize()
    ctx.pathtrace_denoise_adaptive_device(d, k_noise, p_rgba, p_nt, p_pid, p_var, p_out)
    ctx.synchronize()
    return inner(t_out), inner(t_rgba), inner(t_nt), inner(t_pid), inner(t_var)


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_filter_kernel_is_the_host_call(ctx, B, W, H):
    rgba, nt, pid = planes_for(W, H)
    for kind, passes in (("varying", 5), ("zero", 1), ("huge", 2), ("varying", 8)):
        var = variance_for(W, H, kind)
        d = B.pathtrace_denoise_params(W, H, passes=passes)
        want = B.pathtrace_denoise_adaptive(d, rgba, nt, pid, var, 4.0)
        out, a, b, c, v = run_filter(ctx, d, 4.0, rgba, nt, pid, var, in_place=False)
        assert np.array_equal(bits(out), bits(want)), (kind, passes, int((bits(out) != bits(want)).any(-1).sum()))
        assert np.array_equal(bits(a), bits(rgba)) and np.array_equal(bits(b), bits(nt)) and np.array_equal(bits(c), bits(pid)) and \
            np.array_equal(bits(v), bits(var)), "an input changed"
        for _ in range(2):
            out, _, b, c, v = run_filter(ctx, d, 4.0, rgba, nt, pid, var, in_place=True)
            assert np.array_equal(bits(out), bits(want)), ("in place", kind, passes)
            assert np.array_equal(bits(b), bits(nt)) and np.array_equal(bits(c), bits(pid)) and np.array_equal(bits(v), bits(var))


def test_filter_kernel_all_miss(ctx, B):
    rgba, nt, pid = planes_for(23, 11, all_miss=True)
    out = run_filter(ctx, B.pathtrace_denoise_params(23, 11), 4.0, rgba, nt, pid, variance_for(23, 11, "varying"), False)[0]
    assert np.array_equal(bits(out), bits(rgba))


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,spp", [(24, 16, 6), (25, 17, 5), (24, 16, 2)])
def test_chain_strict_is_the_host_calls_on_the_plain_render(ctx, B, O, W, H, spp):
    """In strict math the plane the filter receives is mc_pathtrace_render's: the chain equals the host filter applied to that render, the
    host noise plane of its [0, h) part and the host guides.  5 spp: h = 2, scale = 2.5."""
    h = spp // 2
    p = B.pathtrace_params(W, H, spp)
    d = B.pathtrace_denoise_params(W, H)
    k, radius = B.pathtrace_noise_defaults()
    plain = ctx.pathtrace(p)
    half = ctx.pathtrace(B.pathtrace_params(W, H, spp, sample_end=h))
    assert np.array_equal(bits(ctx.pathtrace(B.pathtrace_params(W, H, spp, sample_begin=h), acc=half)), bits(plain)), "sample ranges compose"
    nt, pid = B.pathtrace_guides(W, H)
    var = B.pathtrace_noise(half, float(np.float32(spp) / np.float32(h)), plain, radius)
    want = B.pathtrace_denoise_adaptive(d, plain, nt, pid, var, k)
    fused = ctx.pathtrace_denoised_adaptive(p, d)
    k_ms, c_ms = ctx.last_timing()
    assert k_ms > 0.0 and c_ms > 0.0, "the timing record covers the chain"
    assert np.array_equal(bits(fused), bits(want)), int((bits(fused) != bits(want)).any(-1).sum())
    assert not np.array_equal(bits(fused), bits(plain))
    fused8 = ctx.pathtrace_denoised_adaptive(p, d, rgba8=True)
    assert np.array_equal(fused8, O.rotate180(O.float_to_rgba8(want, 1.0).reshape(H, W, 4), W, H))
    # other parameters than the defaults reach the kernels
    var1 = B.pathtrace_noise(half, float(np.float32(spp) / np.float32(h)), plain, 1)
    d3 = B.pathtrace_denoise_params(W, H, passes=3)
    assert np.array_equal(bits(ctx.pathtrace_denoised_adaptive(p, d3, k_noise=2.0, radius=1)),
                          bits(B.pathtrace_denoise_adaptive(d3, plain, nt, pid, var1, 2.0)))


@pytest.mark.parametrize("mode", ["PT_MATH_FAST", "PT_MATH_FAST_CAREFUL"])
def test_chain_fast_is_the_chain_of_the_separate_calls(ctx, B, mode):
    import torch
    W, H, spp = 24, 16, 6
    h = spp // 2
    m = getattr(B, mode)
    p = B.pathtrace_params(W, H, spp, math_mode=m)
    d = B.pathtrace_denoise_params(W, H)
    k, radius = B.pathtrace_noise_defaults()
    fused = ctx.pathtrace_denoised_adaptive(p, d)
    t_rgba, p_rgba = guarded(torch, shape=(H, W))
    t_half, p_half = guarded(torch, shape=(H, W))
    t_nt, p_nt = guarded(torch, shape=(H, W))
    t_pid, p_pid = guarded(torch, shape=(H, W))
    t_var, p_var = guarded_plane(torch, shape=(H, W))
    torch.cuda.synchronize()
    ctx.pathtrace_guides_device(W, H, p_nt, p_pid)
    ctx.pathtrace_device(B.pathtrace_params(W, H, spp, math_mode=m, sample_end=h), p_rgba)
    ctx.synchronize()
    t_half[1:-1].copy_(t_rgba[1:-1])
    torch.cuda.synchronize()
    ctx.pathtrace_device(B.pathtrace_params(W, H, spp, math_mode=m, sample_begin=h), p_rgba)
    ctx.pathtrace_noise_device(W, H, p_half, 2.0, p_rgba, radius, p_var)
    ctx.pathtrace_denoise_adaptive_device(d, k, p_rgba, p_nt, p_pid, p_var, p_rgba)
    ctx.synchronize()
    assert np.array_equal(bits(fused), bits(inner(t_rgba)))
    inner(t_half), inner(t_nt), inner(t_pid), inner(t_var)   # the guard rows


def test_plain_denoised_before_and_after_an_adaptive_call(ctx, B):
    """The scratch the two fused calls share is not left in a state that matters."""
    W, H, spp = 24, 16, 6
    p = B.pathtrace_params(W, H, spp)
    before = ctx.pathtrace_denoised(p)
    adaptive = ctx.pathtrace_denoised_adaptive(p)
    after = ctx.pathtrace_denoised(p)
    assert np.array_equal(bits(before), bits(after))
    assert np.array_equal(bits(adaptive), bits(ctx.pathtrace_denoised_adaptive(p))), "twice: the same bits"
    assert np.array_equal(bits(ctx.pathtrace(p)), bits(ctx.pathtrace(p)))


# ---- the app ---------------------------------------------------------------------------------------------------------------------------
def test_app_noise_guided(ctx, B, tmp_path):
    from PIL import Image
    app = os.path.join(os.path.dirname(os.path.dirname(B.LIB_PATH)), "bin", "pathtracer")
    W, H, spp = 60, 40, 8
    p = B.pathtrace_params(W, H, spp)

    def run(*extra):
        r = subprocess.run([app, str(spp), str(H), "--out", "o.png", "--quiet", "--timing-json", "--full-teardown"] + list(extra),
                           capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"timing_ms"')][0])
        return np.asarray(Image.open(tmp_path / "o.png").convert("RGBA")), r.stdout, j

    want = ctx.pathtrace_denoised_adaptive(p, rgba8=True)
    for route in ([], ["--gpu-postprocess"]):
        img, out, j = run("--denoise", "--noise-guided", *route)
        assert np.array_equal(img, want), route
        assert j["denoise"] == 5 and j["noise_guided"] == 4.0
        line = [l for l in out.splitlines() if l.startswith("denoise: ")]
        assert len(line) == 1 and "noise-guided" in line[0] and "k_noise 4" in line[0], out
    img, out, j = run("--denoise=3", "--noise-guided=2")
    want3 = ctx.pathtrace_denoised_adaptive(p, B.pathtrace_denoise_params(W, H, passes=3), k_noise=2.0, rgba8=True)
    assert np.array_equal(img, want3) and j["denoise"] == 3 and j["noise_guided"] == 2.0
    _, out, j = run("--denoise")
    assert j["noise_guided"] == 0 and "noise-guided" not in out
    for bad in (["--noise-guided"], ["--denoise", "--noise-guided=0"], ["--denoise", "--noise-guided=x"],
                ["--denoise", "--noise-guided", "--gpus", "2"]):
        r = subprocess.run([app, str(spp), str(H), "--quiet"] + bad, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode != 0 and "--noise-guided" in r.stdout, (bad, r.stdout)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_device_refusals(ctx, B):
    import torch
    W, H = 8, 8
    k = torch.zeros((6, H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    a, n, x, o, hf = (k[i].data_ptr() for i in range(5))
    v = k[5].data_ptr()
    d = B.pathtrace_denoise_params(W, H)
    noise = lambda *args: (lambda: ctx.pathtrace_noise_device(*args))   # noqa: E731
    refused(B, noise(W, H, 0, 2.0, a, 3, v), "NULL")
    refused(B, noise(W, H, hf, 2.0, 0, 3, v), "NULL")
    refused(B, noise(W, H, hf, 2.0, a, 3, 0), "NULL")
    refused(B, noise(0, H, hf, 2.0, a, 3, v), "width and height")
    refused(B, noise(W, 0, hf, 2.0, a, 3, v), "width and height")
    refused(B, noise(W, H, hf, 2.0, a, 5, v), "radius")
    refused(B, noise(W, H, hf + 4, 2.0, a, 3, v), "aligned")
    refused(B, noise(W, H, hf, 2.0, a, 3, v + 2), "aligned")
    refused(B, noise(W, H, hf, 2.0, a, 3, a + 64), "overlaps")
    den = lambda *args: (lambda: ctx.pathtrace_denoise_adaptive_device(*args))   # noqa: E731
    refused(B, den(d, 4.0, 0, n, x, v, o), "NULL")
    refused(B, den(d, 4.0, a, n, x, 0, o), "NULL")
    refused(B, den(d, 4.0, a, n, x, v, 0), "NULL")
    refused(B, den(d, 4.0, a + 4, n, x, v, o), "aligned")
    refused(B, den(d, 4.0, a, n, x, v + 1, o), "aligned")
    refused(B, den(d, 4.0, a, n, x, v, n), "overlaps")
    refused(B, den(d, 4.0, a, n, x, o + 16, o), "overlaps")
    refused(B, den(d, 4.0, a, n, x, v, a + 16 * W), "overlaps")
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30):
        refused(B, den(d, bad, a, n, x, v, o), "k_noise")
    for kw, word in [(dict(passes=0), "passes"), (dict(passes=9), "passes"), (dict(flags=1), "flags"), (dict(flags=2), "flags")]:
        refused(B, den(B.pathtrace_denoise_params(W, H, **kw), 4.0, a, n, x, v, o), word)
    L = B.lib()
    assert L.mc_pathtrace_noise_device_async(None, W, H, hf, 2.0, a, 3, v, None) == INVALID
    assert L.mc_pathtrace_denoise_adaptive_device_async(None, C.byref(d), 4.0, a, n, x, v, o, None) == INVALID
    ctx.pathtrace_noise_device(W, H, hf, 2.0, a, 4, v)
    ctx.pathtrace_denoise_adaptive_device(d, 4.0, a, n, x, v, a)   # in place is the stated exception
    ctx.synchronize()


def test_chain_refusals(ctx, B):
    W, H = 16, 8
    ok_d = B.pathtrace_denoise_params(W, H)
    chain = lambda p, d=ok_d, **kw: (lambda: ctx.pathtrace_denoised_adaptive(p, d, **kw))   # noqa: E731
    refused(B, chain(B.pathtrace_params(W, H, 1)), "spp")
    refused(B, chain(B.pathtrace_params(W, H, 4, row_begin=0, row_end=4)), "whole images")
    refused(B, chain(B.pathtrace_params(W, H, 4, row_block=2, row_stride=4)), "whole images")
    refused(B, chain(B.pathtrace_params(W, H, 4, sample_end=2)), "whole renders")
    refused(B, chain(B.pathtrace_params(W, H, 4, sample_begin=2)), "whole renders")
    ok_p = B.pathtrace_params(W, H, 4)
    refused(B, chain(ok_p, radius=5), "radius")
    refused(B, chain(ok_p, k_noise=0.0), "k_noise")
    refused(B, chain(ok_p, k_noise=1e30), "k_noise")
    refused(B, chain(ok_p, B.pathtrace_denoise_params(W, H, passes=9)), "passes")
    refused(B, chain(ok_p, B.pathtrace_denoise_params(W, H, flags=1)), "flags")
    refused(B, chain(B.pathtrace_params(W, H, 4, math_mode=7)))
    ctx.pathtrace_denoised_adaptive(ok_p)   # the context renders on after every refusal
