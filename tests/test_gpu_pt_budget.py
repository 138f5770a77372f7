"""Per-pixel sample budgets on the MI355X: the level, list and resolve kernels against the host calls and numpy between guard rows, the
list render against the CPU oracle bit for bit (slab, generic in LDS, generic from memory; every width), mc_pathtrace_render_budgeted
against an image built from oracle renders alone (strict) and against the chain of the separate device calls (fast math), the plain
render before and after it, the app's --budget, every device-side refusal."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pt_budget_ref as R
from test_gpu_pt_denoise import guarded, inner, refused
from test_gpu_pt_noise import guarded_plane
from test_gpu_scenes import random_scene
from test_pt_budget_host import SHAPES, acc_plane, level_plane, variance_plane
from test_pt_denoise_host import bits

pytestmark = pytest.mark.gpu

INVALID = 1
f32 = np.float32


def guarded_bytes(torch, plane=None, shape=None, dtype=None, fill=0xEE):
    """A device plane of one small integer per pixel between two guard rows; returns (whole tensor, pointer to the plane inside it)."""
    H, W = (plane.shape if plane is not None else shape)[:2]
    t = torch.full((H + 2, W), fill, dtype=dtype or torch.uint8, device="cuda")
    if plane is not None:
        t[1:-1] = torch.from_numpy(np.array(plane)).cuda()
    return t, t[1:].data_ptr()


def inner_int(t, fill=0xEE):
    a = t.cpu().numpy()
    assert (a[0] == fill).all() and (a[-1] == fill).all(), "a write outside the plane"
    return a[1:-1]


# ---- levels, lists, resolve ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_level_and_resolve_kernels_are_the_host_calls(ctx, B, W, H):
    import torch
    v = variance_plane(W, H, 8.0)
    t_v, p_v = guarded_plane(torch, v)
    for max_level in (0, 4, 8):
        want = B.pathtrace_budget_levels(v, 8.0, max_level)
        for _ in range(2):   # twice: the same bytes
            t_lv, p_lv = guarded_bytes(torch, shape=(H, W))
            torch.cuda.synchronize()
            ctx.pathtrace_budget_levels_device(W, H, p_v, 8.0, max_level, p_lv)
            ctx.synchronize()
            assert np.array_equal(inner_int(t_lv), want), max_level
    assert np.array_equal(bits(inner(t_v)), bits(v)), "an input changed"
    acc = acc_plane(W, H)
    lv = level_plane(W, H, 4)
    want = B.pathtrace_budget_resolve(acc, lv)
    t_lv, p_lv = guarded_bytes(torch, lv)
    for in_place in (False, True, True):
        t_acc, p_acc = guarded(torch, acc)
        t_out, p_out = (t_acc, p_acc) if in_place else guarded(torch, shape=acc.shape)
        torch.cuda.synchronize()
        ctx.pathtrace_budget_resolve_device(W, H, p_acc, p_lv, p_out)
        ctx.synchronize()
        assert np.array_equal(bits(inner(t_out)), bits(want)), in_place
        if not in_place:
            assert np.array_equal(bits(inner(t_acc)), bits(acc)), "an input changed"
    assert np.array_equal(inner_int(t_lv), lv), "an input changed"


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_lists_are_the_buckets(ctx, B, W, H):
    import torch
    P = W * H
    planes = [(4, level_plane(W, H, 4)), (8, level_plane(W, H, 8)), (0, np.zeros((H, W), np.uint8)), (4, np.zeros((H, W), np.uint8)),
              (4, np.full((H, W), 4, np.uint8)), (8, np.full((H, W), 8, np.uint8))]
    for max_level, lv in planes:
        counts_want, buckets_want = R.lists(lv, max_level)
        t_lv, p_lv = guarded_bytes(torch, lv)
        for _ in range(2):
            t_list, p_list = guarded_bytes(torch, shape=(H, W), dtype=torch.int32, fill=-3)
            t_counts = torch.full((3, 9), -3, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.pathtrace_budget_lists_device(W, H, p_lv, max_level, p_list, t_counts[1].data_ptr())
            ctx.synchronize()
            counts = inner_int(t_counts, fill=-3)[0]
            assert counts[:max_level + 1].tolist() == counts_want.tolist() and not counts[max_level + 1:].any(), (max_level, counts)
            lst = inner_int(t_list, fill=-3).reshape(-1).view(np.uint32)
            got = R.sorted_buckets(lst, counts, max_level)
            assert all(np.array_equal(g, w) for g, w in zip(got, buckets_want)), max_level
            assert np.array_equal(np.sort(lst), np.arange(P, dtype=np.uint32)), "every pixel once"
        assert np.array_equal(inner_int(t_lv), lv), "an input changed"


# ---- the list render against the oracle --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def list_scene(name):
    """(planes, spheres, W, H, kernel): the reference scene (slab), a room of 40 spheres (generic, records in LDS), a room of 1494 (72 KB
    of records, past the automatic LDS limit: read from memory)."""
    if name == "slab":
        return None, None, 33, 21, "PT_KERNEL_SLAB"
    if name == "lds":
        planes, spheres = random_scene(np.random.default_rng(140), 6, 40, 3)
        return planes, spheres, 33, 21, "PT_KERNEL_GENERIC"
    planes, spheres = random_scene(np.random.default_rng(7), 6, 1494, 4)
    return planes, spheres, 16, 8, "PT_KERNEL_GENERIC_MEMORY"


def pixel_list(W, H):
    """Every third storage index and the four corners, shuffled, and one entry past the image."""
    idx = np.unique(np.concatenate([np.arange(0, W * H, 3), [0, W - 1, (H - 1) * W, W * H - 1]])).astype(np.uint32)
    np.random.default_rng(W).shuffle(idx)
    return idx, np.concatenate([idx[:5], np.array([W * H + 5], np.uint32), idx[5:]])


_CASES = {}


def list_cases(O, name):
    """(label, p.spp, begin, end, prescale, start plane or None, expected plane) from the oracle alone; the sample counts 4, 4, 16 and 2
    (memory scene: 2, 2, 16, 4) take the launcher through its widths 4, 16 and 1."""
    if name in _CASES:
        return _CASES[name]
    planes, spheres, W, H, _ = list_scene(name)
    sc = {} if planes is None else dict(planes=planes, spheres=spheres)
    ora = lambda spp, end: O.pathtrace(W, H, spp, math_mode=O.MATH_MC, sample_end=end, **sc)   # noqa: E731
    u = 2 if name == "memory" else 4
    want = ora(4 * u, 2 * u)
    cases = [("continue", 4 * u, u, 2 * u, 1.0, ora(4 * u, u), want),
             ("continue-halved", 4 * u, u, 2 * u, 0.5, ora(2 * u, u), want),
             ("from-zero-to-spp", 16, 0, 16, 1.0, None, R.linear_range(O, 16, 0, 16, W=W, H=H, **sc)),
             ("short", 16, 8, 8 + 8 // u, 1.0, ora(16, 8), ora(16, 8 + 8 // u))]
    _CASES[name] = cases
    return cases


@pytest.mark.parametrize("name", ["slab", "lds", "memory"])
def test_list_render_is_the_oracle(ctx, B, O, name):
    import torch
    planes, spheres, W, H, kernel = list_scene(name)
    info = B.pathtrace_select_kernel(B.pathtrace_params(W, H, 16, flags=B.pt_force_s(4)), planes, spheres)
    assert info.kernel == getattr(B, kernel), "the family the list render runs for this scene"
    listed, lst = pixel_list(W, H)
    mask = np.zeros(W * H, bool)
    mask[listed] = True
    mask = mask.reshape(H, W)
    t_list = torch.from_numpy(lst.view(np.int32)).cuda()
    for label, spp, begin, end, prescale, start, want in list_cases(O, name):
        widths = (0, 1, 4, 16) if label == "continue" else (0,)
        for S in widths:
            before = np.full((H, W, 4), np.nan, f32) if start is None else start
            t_acc, p_acc = guarded(torch, before)
            torch.cuda.synchronize()
            p = B.pathtrace_params(W, H, spp, sample_begin=begin, sample_end=end, flags=B.pt_force_s(S) if S else 0)
            ctx.pathtrace_list_device(p, t_list.data_ptr(), lst.size, prescale, p_acc, planes, spheres)
            ctx.synchronize()
            got = inner(t_acc)
            assert np.array_equal(bits(got[mask]), bits(want[mask])), (label, S, int((bits(got[mask]) != bits(want[mask])).any(-1).sum()))
            assert np.array_equal(bits(got[~mask]), bits(before[~mask])), (label, S, "a pixel that is not listed changed")
    assert np.array_equal(t_list.cpu().numpy().view(np.uint32), lst), "the list changed"
    # an empty list launches nothing
    t_acc, p_acc = guarded(torch, want)
    torch.cuda.synchronize()
    ctx.pathtrace_list_device(B.pathtrace_params(W, H, 16, sample_begin=4, sample_end=8), 0, 0, 1.0, p_acc, planes, spheres)
    ctx.pathtrace_list_device(B.pathtrace_params(W, H, 16, sample_begin=4, sample_end=8), t_list.data_ptr(), 0, 1.0, p_acc, planes, spheres)
    ctx.synchronize()
    assert np.array_equal(bits(inner(t_acc)), bits(want))


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
CHAINS = [(48, 32, 4, 2, 37.5), (33, 21, 2, 3, 30.0)]


@pytest.mark.parametrize("W,H,n0,L,T", CHAINS, ids=[f"{c[0]}x{c[1]}" for c in CHAINS])
def test_chain_strict_is_the_oracle_at_each_pixels_own_spp(ctx, B, O, W, H, n0, L, T):
    want, lv, _ = R.chain(O, W, H, n0, L, T, 3)
    counts = np.bincount(lv.reshape(-1), minlength=L + 1)
    assert (counts / lv.size >= 0.05).all(), ("every level holds at least 5 % of the pixels", counts / lv.size)
    p = B.pathtrace_params(W, H, n0)
    b = B.pathtrace_budget_params(max_level=L, target=T, radius=3)
    plain_before = ctx.pathtrace(p)
    got, got_lv = ctx.pathtrace_budgeted(p, b, want_levels=True)
    k_ms, c_ms = ctx.last_timing()
    per_level, mean = ctx.last_budget()
    assert np.array_equal(got_lv, lv), int((got_lv != lv).sum())
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).any(-1).sum())
    assert k_ms > 0.0 and c_ms > 0.0, "the timing record covers the chain"
    assert per_level == counts.tolist() + [0] * (8 - L)
    assert mean == float(sum(int(c) * (n0 << l) for l, c in enumerate(counts))) / (W * H)
    got8 = ctx.pathtrace_budgeted(p, b, rgba8=True)
    assert np.array_equal(got8, O.rotate180(O.float_to_rgba8(want, 1.0).reshape(H, W, 4), W, H))
    # no level beyond the pilot, by max_level or by a target nothing exceeds: the plain n0 render
    plain = O.pathtrace(W, H, n0, math_mode=O.MATH_MC)
    for kw in (dict(max_level=0, target=T), dict(max_level=L, target=1e6)):
        out, out_lv = ctx.pathtrace_budgeted(p, B.pathtrace_budget_params(radius=3, **kw), want_levels=True)
        assert np.array_equal(bits(out), bits(plain)) and not out_lv.any(), kw
        assert ctx.last_budget() == ([W * H] + [0] * 8, float(n0))
    # a target everything exceeds: the plain render at n0 << L
    out, out_lv = ctx.pathtrace_budgeted(p, B.pathtrace_budget_params(max_level=L, target=1e-3, radius=3), want_levels=True)
    deep = O.pathtrace(W, H, n0 << L, math_mode=O.MATH_MC)
    assert np.array_equal(bits(out), bits(deep)) and (out_lv == L).all()
    # the scratch the chain shares with the plain render is not left in a state that matters
    assert np.array_equal(bits(ctx.pathtrace(p)), bits(plain_before)) and np.array_equal(bits(plain_before), bits(plain))


@pytest.mark.parametrize("mode", ["PT_MATH_FAST", "PT_MATH_FAST_CAREFUL"])
def test_chain_fast_is_the_chain_of_the_separate_calls(ctx, B, mode):
    import torch
    W, H, n0, L, T = 48, 32, 4, 2, 37.5
    m = getattr(B, mode)
    p = B.pathtrace_params(W, H, n0, math_mode=m)
    b = B.pathtrace_budget_params(max_level=L, target=T, radius=3)
    fused, fused_lv = ctx.pathtrace_budgeted(p, b, want_levels=True)
    again, again_lv = ctx.pathtrace_budgeted(p, b, want_levels=True)
    assert np.array_equal(bits(fused), bits(again)) and np.array_equal(fused_lv, again_lv), "twice: the same bits"
    t_acc, p_acc = guarded(torch, shape=(H, W))
    t_half, p_half = guarded(torch, shape=(H, W))
    t_enc, p_enc = guarded(torch, shape=(H, W))
    t_var, p_var = guarded_plane(torch, shape=(H, W))
    t_zero, p_zero = guarded_bytes(torch, np.zeros((H, W), np.uint8))
    t_lv, p_lv = guarded_bytes(torch, shape=(H, W))
    t_list, p_list = guarded_bytes(torch, shape=(H, W), dtype=torch.int32, fill=-3)
    t_counts = torch.zeros(9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.pathtrace_device(B.pathtrace_params(W, H, 2 * n0, math_mode=m, sample_end=n0 // 2), p_acc)
    ctx.synchronize()
    t_half[1:-1].copy_(t_acc[1:-1])
    torch.cuda.synchronize()
    ctx.pathtrace_device(B.pathtrace_params(W, H, 2 * n0, math_mode=m, sample_begin=n0 // 2, sample_end=n0), p_acc)
    ctx.pathtrace_budget_resolve_device(W, H, p_acc, p_zero, p_enc)
    ctx.pathtrace_noise_device(W, H, p_half, float(f32(2 * n0) / f32(n0 // 2)), p_enc, 3, p_var)
    ctx.pathtrace_budget_levels_device(W, H, p_var, T, L, p_lv)
    ctx.pathtrace_budget_lists_device(W, H, p_lv, L, p_list, t_counts.data_ptr())
    ctx.synchronize()
    counts = t_counts.cpu().numpy()
    for r in range(1, L + 1):
        n = int(counts[r:].sum())
        if n:
            ctx.pathtrace_list_device(B.pathtrace_params(W, H, n0 << r, math_mode=m, sample_begin=n0 << (r - 1), sample_end=n0 << r), p_list, n,
                                      1.0 if r == 1 else 0.5, p_acc)
    ctx.pathtrace_budget_resolve_device(W, H, p_acc, p_lv, p_acc)
    ctx.synchronize()
    assert np.array_equal(inner_int(t_lv), fused_lv)
    assert np.array_equal(bits(inner(t_acc)), bits(fused))
    assert len(np.unique(fused_lv)) == L + 1, "every level is exercised"
    inner(t_half), inner(t_enc), inner(t_var), inner_int(t_zero), inner_int(t_list, fill=-3)   # the guard rows


# ---- the app -----------------------------------------------------------------------------------------------------------------------------
def test_app_budget(ctx, B, tmp_path):
    from PIL import Image
    app = os.path.join(os.path.dirname(os.path.dirname(B.LIB_PATH)), "bin", "pathtracer")
    W, H, n0 = 48, 32, 4
    p = B.pathtrace_params(W, H, n0)
    want = ctx.pathtrace_budgeted(p, B.pathtrace_budget_params(max_level=2, target=37.5), rgba8=True)
    per_level, mean = ctx.last_budget()
    for route in ([], ["--gpu-postprocess"]):
        r = subprocess.run([app, str(n0), str(H), "--out", "o.png", "--quiet", "--full-teardown", "--budget=2", "--noise-target", "37.5"] + route,
                           capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        assert np.array_equal(np.asarray(Image.open(tmp_path / "o.png").convert("RGBA")), want), route
        line = [l for l in r.stdout.splitlines() if l.startswith("budget: ")]
        assert len(line) == 1, r.stdout
        words = line[0].split()
        assert [int(x) for x in words[1:4]] == per_level[:3] and words[4] == "mean" and abs(float(words[5]) - mean) < 1e-3 and words[6] == "spp", line
    for bad in (["--budget", "--denoise"], ["--budget=9"], ["--noise-target", "8"], ["--budget", "--noise-target", "0"], ["--budget", "--gpus", "2"]):
        r = subprocess.run([app, str(n0), str(H), "--quiet"] + bad, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode != 0 and ("--budget" in r.stdout or "--noise-target" in r.stdout), (bad, r.stdout)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_device_refusals(ctx, B):
    import torch
    W, H = 8, 8
    k = torch.zeros((4, H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    acc, out, v, lst = (k[i].data_ptr() for i in range(4))
    lv, counts = v + 4 * W * H, lst + 4 * W * H   # (behind the float plane and the list, inside their vec4 planes)
    levels = lambda *a: (lambda: ctx.pathtrace_budget_levels_device(*a))   # noqa: E731
    refused(B, levels(0, H, v, 8.0, 4, lv), "width and height")
    refused(B, levels(W, 0, v, 8.0, 4, lv), "width and height")
    refused(B, levels(W, H, 0, 8.0, 4, lv), "NULL")
    refused(B, levels(W, H, v, 8.0, 4, 0), "NULL")
    refused(B, levels(W, H, v + 2, 8.0, 4, lv), "aligned")
    refused(B, levels(W, H, v, 8.0, 9, lv), "max_level")
    refused(B, levels(W, H, v, 8.0, 4, v + 16), "overlaps")
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30):
        refused(B, levels(W, H, v, bad, 4, lv), "target")
    lists = lambda *a: (lambda: ctx.pathtrace_budget_lists_device(*a))   # noqa: E731
    refused(B, lists(0, H, lv, 4, lst, counts), "width and height")
    refused(B, lists(W, H, 0, 4, lst, counts), "NULL")
    refused(B, lists(W, H, lv, 4, 0, counts), "NULL")
    refused(B, lists(W, H, lv, 4, lst, 0), "NULL")
    refused(B, lists(W, H, lv, 9, lst, counts), "max_level")
    refused(B, lists(W, H, lv, 4, lst + 2, counts), "aligned")
    refused(B, lists(W, H, lv, 4, lst, counts + 1), "aligned")
    refused(B, lists(W, H, lv, 4, lst, lst + 8), "overlap")
    refused(B, lists(W, H, lv, 4, lv - 8, counts), "overlap")
    res = lambda *a: (lambda: ctx.pathtrace_budget_resolve_device(*a))   # noqa: E731
    refused(B, res(0, H, acc, lv, out), "width and height")
    refused(B, res(W, H, 0, lv, out), "NULL")
    refused(B, res(W, H, acc, 0, out), "NULL")
    refused(B, res(W, H, acc, lv, 0), "NULL")
    refused(B, res(W, H, acc + 4, lv, out), "aligned")
    refused(B, res(W, H, acc, lv, out + 8), "aligned")
    refused(B, res(W, H, acc, lv, acc + 16), "overlaps")
    refused(B, res(W, H, acc, lv, lv - 16), "overlaps")
    ok = dict(sample_begin=2, sample_end=4)
    render = lambda p, *a: (lambda: ctx.pathtrace_list_device(p, *a))   # noqa: E731
    ok_p = B.pathtrace_params(W, H, 4, **ok)
    refused(B, render(ok_p, 0, 3, 1.0, acc), "NULL")
    refused(B, render(ok_p, lst, 3, 1.0, 0), "NULL")
    refused(B, render(ok_p, lst + 2, 3, 1.0, acc), "aligned")
    refused(B, render(ok_p, lst, 3, 1.0, acc + 4), "aligned")
    refused(B, render(ok_p, acc + 16, 3, 1.0, acc), "overlaps")
    refused(B, render(B.pathtrace_params(W, H, 4, row_begin=0, row_end=4, **ok), lst, 3, 1.0, acc), "whole-image")
    refused(B, render(B.pathtrace_params(W, H, 4, row_block=2, row_stride=4, **ok), lst, 3, 1.0, acc), "whole-image")
    refused(B, render(B.pathtrace_params(W, H, 4, flags=B.pt_precision(B.PT_PREC_DS), **ok), lst, 3, 1.0, acc), "MC_PT_PRECISION")
    refused(B, render(B.pathtrace_params(W, H, 4, sample_begin=3, sample_end=3), lst, 3, 1.0, acc))
    refused(B, render(B.pathtrace_params(W, H, 4, math_mode=7, **ok), lst, 3, 1.0, acc))
    L = B.lib()
    assert L.mc_pathtrace_budget_levels_device_async(None, W, H, v, 8.0, 4, lv, None) == INVALID
    assert L.mc_pathtrace_budget_lists_device_async(None, W, H, lv, 4, lst, counts, None) == INVALID
    assert L.mc_pathtrace_budget_resolve_device_async(None, W, H, acc, lv, out, None) == INVALID
    assert L.mc_pathtrace_render_list_device_async(None, C.byref(ok_p), None, 0, None, 0, lst, 3, 1.0, acc, None) == INVALID
    # the stated exceptions and the context after every refusal: a list of zeros is not distinct, so one entry only
    ctx.pathtrace_budget_levels_device(W, H, v, 8.0, 8, lv)
    ctx.pathtrace_budget_lists_device(W, H, lv, 8, lst, counts)
    ctx.pathtrace_budget_resolve_device(W, H, acc, lv, acc)
    ctx.pathtrace_list_device(ok_p, lst, 1, 0.5, acc)
    ctx.synchronize()


def test_chain_refusals(ctx, B):
    W, H = 16, 8
    chain = lambda p, **kw: (lambda: ctx.pathtrace_budgeted(p, B.pathtrace_budget_params(**kw)))   # noqa: E731
    refused(B, chain(B.pathtrace_params(W, H, 3)), "even")
    refused(B, chain(B.pathtrace_params(W, H, 0)))
    refused(B, chain(B.pathtrace_params(W, H, 1 << 17)), "2^20")
    refused(B, chain(B.pathtrace_params(W, H, 4, row_begin=0, row_end=4)), "whole images")
    refused(B, chain(B.pathtrace_params(W, H, 4, row_block=2, row_stride=4)), "whole images")
    refused(B, chain(B.pathtrace_params(W, H, 4, sample_end=2)), "whole renders")
    refused(B, chain(B.pathtrace_params(W, H, 4, sample_begin=2)), "whole renders")
    ok_p = B.pathtrace_params(W, H, 4)
    refused(B, chain(ok_p, radius=5), "radius")
    refused(B, chain(ok_p, max_level=9), "max_level")
    refused(B, chain(ok_p, flags=1), "flags")
    refused(B, chain(ok_p, target=0.0), "target")
    refused(B, chain(ok_p, target=1e30), "target")
    refused(B, chain(B.pathtrace_params(W, H, 4, math_mode=7)))
    refused(B, chain(B.pathtrace_params(W, H, 4, flags=B.pt_precision(B.PT_PREC_DS))), "MC_PT_PRECISION")
    assert B.lib().mc_context_last_budget(None, None, None) == INVALID
    ctx.pathtrace_budgeted(ok_p)   # the context renders on after every refusal
    assert sum(ctx.last_budget()[0]) == W * H
