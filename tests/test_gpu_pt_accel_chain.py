"""What runs behind a render, for mc_pathtrace_accel scenes, on the MI355X: the guide kernel through the tree, the
denoised and the noise-guided chain, the list render and the budgeted chain.  ONE definition: a call returns what its table form returns
for the tables the object was made from - so every strict test compares float32 words (as uint32) with the table form's, and one case
of each kind is tied to the CPU oracle alone.  The careful tier (MC_PT_MATH_FAST and _FAST_CAREFUL) is held to the table forms' weaker
promise: the bits of the same chain made from the separate public accel calls.  Then the app's --accel bvh chains and every refusal
that needs a context."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pt_budget_ref as R
from pt_accel_chain_cases import bits, scene
from test_gpu_pt_budget import guarded_bytes, inner_int
from test_gpu_pt_denoise import guarded, inner
from test_gpu_pt_noise import guarded_plane

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 5
f32 = np.float32
W0, H0 = 24, 16   # the shape most cases share


@pytest.fixture(scope="module")
def world(B, O):
    """The accel objects and the oracle's renders, each made once and shared (never modified)."""
    class World:
        def __init__(self):
            self.accels, self.refs = {}, {}

        def accel(self, name):
            if name not in self.accels:
                self.accels[name] = B.PathtraceAccel(*scene(name))
            return self.accels[name]

        def ref(self, name, W, H, spp, **kw):
            key = (name, W, H, spp, tuple(sorted(kw.items())))
            if key not in self.refs:
                planes, spheres = scene(name)
                a = O.pathtrace(W, H, spp, planes=planes, spheres=spheres, math_mode=O.MATH_MC, **kw)
                a.setflags(write=False)
                self.refs[key] = a
            return self.refs[key]

    w = World()
    yield w
    for a in w.accels.values():
        a.close()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def differing(a, b):
    return int((bits(a) != bits(b)).any(-1).sum())


# ---- guides ----------------------------------------------------------------------------------------------------------------------------
GUIDE_CASES = [("random200", 1, 1), ("random200", 37, 23), ("random200", 257, 130), ("unboxable", 24, 16), ("none", 24, 16)]


@pytest.mark.parametrize("name,W,H", GUIDE_CASES, ids=[f"{n}-{w}x{h}" for n, w, h in GUIDE_CASES])
def test_guides_device_is_the_host_form_is_the_table_form(ctx, B, world, name, W, H):
    import torch
    planes, spheres = scene(name)
    a = world.accel(name)
    host_nt, host_pid = a.guides(W, H)
    t_nt, p_nt = guarded(torch, shape=(H, W))
    t_pid, p_pid = guarded(torch, shape=(H, W))
    t_tnt, p_tnt = guarded(torch, shape=(H, W))
    t_tpid, p_tpid = guarded(torch, shape=(H, W))
    torch.cuda.synchronize()
    for _ in range(2):   # twice: the same bits, and no second device copy
        ctx.pathtrace_accel_guides_device(a, W, H, p_nt, p_pid)
        ctx.synchronize()
        assert a.info()["device_copies"] == 1
        nt, pid = inner(t_nt), inner(t_pid)
        assert same(pid, host_pid), (name, differing(pid, host_pid))
        assert same(nt, host_nt), (name, differing(nt, host_nt))
    ctx.pathtrace_guides_device(W, H, p_tnt, p_tpid, planes, spheres)
    ctx.synchronize()
    assert same(inner(t_tpid), host_pid) and same(inner(t_tnt), host_nt), "the table form's device guides"
    if name == "random200" and W * H > 1:
        assert (host_pid[..., 3] >= planes.size // 12).any(), "a sphere is some pixel's first hit"


# ---- the denoised chain, strict ----------------------------------------------------------------------------------------------------------
DENOISED = [("random200", 37, 23, 5), ("lattice700", 24, 16, 6), ("duplicates", 24, 16, 6), ("unboxable", 24, 16, 6)]


@pytest.mark.parametrize("passes", [1, 5])
@pytest.mark.parametrize("name,W,H,spp", DENOISED, ids=[c[0] for c in DENOISED])
def test_denoised_strict_is_the_table_form(ctx, B, world, name, W, H, spp, passes):
    planes, spheres = scene(name)
    p = B.pathtrace_params(W, H, spp)
    d = B.pathtrace_denoise_params(W, H, passes=passes)
    want = ctx.pathtrace_denoised(p, d, planes, spheres)
    got = ctx.pathtrace_accel_denoised(world.accel(name), p, d)
    k_ms, c_ms = ctx.last_timing()
    assert k_ms > 0.0 and c_ms > 0.0, "the timing record covers the chain"
    assert same(got, want), (name, passes, differing(got, want))
    want8 = ctx.pathtrace_denoised(p, d, planes, spheres, rgba8=True)
    got8 = ctx.pathtrace_accel_denoised(world.accel(name), p, d, rgba8=True)
    assert np.array_equal(got8, want8), (name, passes)


def test_denoised_strict_is_the_host_filter_over_the_oracle(ctx, B, O, world):
    W, H, spp = W0, H0, 6
    planes, spheres = scene("random200")
    d = B.pathtrace_denoise_params(W, H)
    nt, pid = B.pathtrace_guides(W, H, planes, spheres)
    plain = world.ref("random200", W, H, spp)
    want = B.pathtrace_denoise(d, plain, nt, pid)
    got = ctx.pathtrace_accel_denoised(world.accel("random200"), B.pathtrace_params(W, H, spp), d)
    assert same(got, want), differing(got, want)
    assert not same(got, plain), "the filter changed the picture"
    got8 = ctx.pathtrace_accel_denoised(world.accel("random200"), B.pathtrace_params(W, H, spp), d, rgba8=True)
    assert np.array_equal(got8, O.rotate180(O.float_to_rgba8(want, 1.0).reshape(H, W, 4), W, H))


# ---- the noise-guided chain, strict ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [6, 5])
@pytest.mark.parametrize("name,W,H,_", DENOISED, ids=[c[0] for c in DENOISED])
def test_noise_guided_strict_is_the_table_form(ctx, B, world, name, W, H, _, spp):
    """spp = 5: h = 2, scale = 2.5."""
    planes, spheres = scene(name)
    p = B.pathtrace_params(W, H, spp)
    d = B.pathtrace_denoise_params(W, H)
    want = ctx.pathtrace_denoised_adaptive(p, d, planes=planes, spheres=spheres)
    got = ctx.pathtrace_accel_denoised_adaptive(world.accel(name), p, d)
    assert same(got, want), (name, spp, differing(got, want))
    want8 = ctx.pathtrace_denoised_adaptive(p, d, planes=planes, spheres=spheres, rgba8=True)
    assert np.array_equal(ctx.pathtrace_accel_denoised_adaptive(world.accel(name), p, d, rgba8=True), want8), (name, spp)
    # other parameters than the defaults reach the kernels
    d3 = B.pathtrace_denoise_params(W, H, passes=3)
    assert same(ctx.pathtrace_accel_denoised_adaptive(world.accel(name), p, d3, k_noise=2.0, radius=1),
                ctx.pathtrace_denoised_adaptive(p, d3, k_noise=2.0, radius=1, planes=planes, spheres=spheres))


def test_noise_guided_strict_is_the_host_calls_over_the_oracle(ctx, B, world):
    W, H, spp = W0, H0, 6
    h = spp // 2
    planes, spheres = scene("random200")
    d = B.pathtrace_denoise_params(W, H)
    k, radius = B.pathtrace_noise_defaults()
    nt, pid = B.pathtrace_guides(W, H, planes, spheres)
    plain = world.ref("random200", W, H, spp)
    half = world.ref("random200", W, H, spp, sample_end=h)
    var = B.pathtrace_noise(half, float(f32(spp) / f32(h)), plain, radius)
    want = B.pathtrace_denoise_adaptive(d, plain, nt, pid, var, k)
    got = ctx.pathtrace_accel_denoised_adaptive(world.accel("random200"), B.pathtrace_params(W, H, spp), d)
    assert same(got, want), differing(got, want)
    assert not same(got, plain)


# ---- the list render, strict -------------------------------------------------------------------------------------------------------------
def pixel_list(W, H):
    """test_gpu_pt_budget.py's kind of list: a scattered subset (every third storage index and the corners, shuffled) with entries past
    the image among and behind them.  Returns (the listed indices, the list)."""
    idx = np.unique(np.concatenate([np.arange(0, W * H, 3), [0, W - 1, (H - 1) * W, W * H - 1]])).astype(np.uint32)
    np.random.default_rng(W).shuffle(idx)
    return idx, np.concatenate([idx[:5], np.array([W * H + 5], np.uint32), idx[5:], np.array([W * H, 0xffffffff, 1 << 31], np.uint32)])


# (label, p.spp, begin, end, prescale): counts 2, 4 and 16 reach the S = 1, 4 and 16 kernels (the list is far below 65536 waves)
LIST_CASES = [(f"{kind}-{n}", 32, b, b + n, s) for n in (2, 4, 16) for kind, b, s in (("from-zero", 0, 1.0), ("continue", n, 1.0),
                                                                                         ("continue-halved", n, 0.5))]
LIST_CASES.append(("ragged", 16, 3, 9, 0.5))   # 6 samples at S = 4: a head of 4 and a tail launch of 2 x S = 1, which must not rescale


@pytest.mark.parametrize("label,spp,begin,end,prescale", LIST_CASES, ids=[c[0] for c in LIST_CASES])
def test_list_render_strict_is_the_table_form(ctx, B, world, label, spp, begin, end, prescale):
    import torch
    W, H = W0, H0
    planes, spheres = scene("random200")
    a = world.accel("random200")
    listed, lst = pixel_list(W, H)
    mask = np.zeros(W * H, bool)
    mask[listed] = True
    mask = mask.reshape(H, W)
    t_list = torch.from_numpy(lst.view(np.int32)).cuda()
    if begin == 0:
        before = np.full((H, W, 4), np.nan, f32)   # not read when sample_begin == 0
    else:
        before = ctx.pathtrace(B.pathtrace_params(W, H, spp, sample_end=begin), planes=planes, spheres=spheres)   # linear: end < spp
    p = B.pathtrace_params(W, H, spp, sample_begin=begin, sample_end=end)
    t_want, p_want = guarded(torch, before)
    t_got, p_got = guarded(torch, before)
    torch.cuda.synchronize()
    ctx.pathtrace_list_device(p, t_list.data_ptr(), lst.size, prescale, p_want, planes, spheres)
    ctx.pathtrace_accel_list_device(a, p, t_list.data_ptr(), lst.size, prescale, p_got)
    ctx.synchronize()
    want, got = inner(t_want), inner(t_got)   # (inner: the guard rows are untouched, at every width, S = 16 among them)
    assert same(got[mask], want[mask]), (label, differing(got[mask], want[mask]))
    assert same(got[~mask], before[~mask]), (label, "a pixel that is not listed changed")
    assert np.isfinite(got[mask]).all() and (got[mask][..., :3] > 0).any()
    if begin:
        assert not same(got[mask], before[mask]), "the range was added"
    assert np.array_equal(t_list.cpu().numpy().view(np.uint32), lst), "the list changed"
    assert a.info()["device_copies"] == 1


def test_list_render_strict_is_the_oracle_alone(ctx, B, O, world):
    """pt_budget_ref.linear_range: from zero to spp stays LINEAR (never the :453 encode), and the ragged continuation with its prescale."""
    import torch
    W, H = W0, H0
    planes, spheres = scene("random200")
    sc = dict(W=W, H=H, planes=planes, spheres=spheres)
    listed, lst = pixel_list(W, H)
    mask = np.zeros(W * H, bool)
    mask[listed] = True
    mask = mask.reshape(H, W)
    t_list = torch.from_numpy(lst.view(np.int32)).cuda()
    start = world.ref("random200", W, H, 8, sample_end=3)   # the accumulator of [0, 3) at divisor 8: times 0.5 it is divisor 16's
    for label, spp, begin, end, prescale, before in (("from-zero-to-spp", 16, 0, 16, 1.0, None), ("ragged", 16, 3, 9, 0.5, start)):
        want = R.linear_range(O, spp, begin, end, acc=before, prescale=prescale, **sc)
        plane = np.full((H, W, 4), np.nan, f32) if before is None else before
        t_acc, p_acc = guarded(torch, plane)
        torch.cuda.synchronize()
        ctx.pathtrace_accel_list_device(world.accel("random200"), B.pathtrace_params(W, H, spp, sample_begin=begin, sample_end=end),
                                        t_list.data_ptr(), lst.size, prescale, p_acc)
        ctx.synchronize()
        got = inner(t_acc)
        assert same(got[mask], want[mask]), (label, differing(got[mask], want[mask]))
        assert same(got[~mask], plane[~mask]), label
    # the ragged case is the oracle's plain [0, 9) accumulator at divisor 16
    assert same(want, world.ref("random200", W, H, 16, sample_end=9))


def test_list_render_of_an_empty_list_launches_nothing(ctx, B, world):
    import torch
    W, H = W0, H0
    a = world.accel("random200")
    plane = world.ref("random200", W, H, 16, sample_end=4)
    t_acc, p_acc = guarded(torch, plane)
    t_list = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = B.pathtrace_params(W, H, 16, sample_begin=4, sample_end=8)
    ctx.pathtrace_accel_list_device(a, p, 0, 0, 1.0, p_acc)
    ctx.pathtrace_accel_list_device(a, p, t_list.data_ptr(), 0, 0.5, p_acc)
    ctx.synchronize()
    assert same(inner(t_acc), plane)


# ---- the budgeted chain, strict ------------------------------------------------------------------------------------------------------------
BUDGET = dict(n0=4, L=2, T=48.0, radius=3)


def test_budgeted_strict_is_the_table_form_and_the_oracle(ctx, B, O, world):
    """random200, 24 x 16, n0 = 4, L = 2, T = 48: the oracle alone puts 103 / 172 / 109 pixels on levels 0 / 1 / 2, so both doubling
    rounds run on a proper subset."""
    W, H = W0, H0
    n0, L, T, radius = BUDGET["n0"], BUDGET["L"], BUDGET["T"], BUDGET["radius"]
    planes, spheres = scene("random200")
    a = world.accel("random200")
    want, lv, _ = R.chain(O, W, H, n0, L, T, radius, planes=planes, spheres=spheres)
    counts = np.bincount(lv.reshape(-1), minlength=L + 1)
    print("levels from the oracle alone:", counts.tolist())
    assert (counts / lv.size >= 0.10).all(), ("every level holds at least 10 % of the pixels", counts.tolist())
    assert counts.tolist() == [103, 172, 109]
    p = B.pathtrace_params(W, H, n0)
    b = B.pathtrace_budget_params(max_level=L, target=T, radius=radius)
    table, table_lv = ctx.pathtrace_budgeted(p, b, planes, spheres, want_levels=True)
    table_budget = ctx.last_budget()
    got, got_lv = ctx.pathtrace_accel_budgeted(a, p, b, want_levels=True)
    k_ms, c_ms = ctx.last_timing()
    got_budget = ctx.last_budget()
    assert k_ms > 0.0 and c_ms > 0.0, "the timing record covers the chain"
    assert np.array_equal(got_lv, table_lv) and np.array_equal(got_lv, lv), int((got_lv != lv).sum())
    assert same(got, table), differing(got, table)
    assert same(got, want), differing(got, want)
    assert got_budget == table_budget
    assert got_budget[0] == counts.tolist() + [0] * (8 - L)
    assert got_budget[1] == float(sum(int(c) * (n0 << l) for l, c in enumerate(counts))) / (W * H)
    # the promise, stated with the accelerated render itself: out[p] is mc_pathtrace_render_accel at n0 << level[p]
    for l in range(L + 1):
        plain = ctx.pathtrace_accel(a, B.pathtrace_params(W, H, n0 << l))
        assert same(got[lv == l], plain[lv == l]), l
    got8 = ctx.pathtrace_accel_budgeted(a, p, b, rgba8=True)
    assert np.array_equal(got8, ctx.pathtrace_budgeted(p, b, planes, spheres, rgba8=True))
    assert np.array_equal(got8, O.rotate180(O.float_to_rgba8(want, 1.0).reshape(H, W, 4), W, H))


def test_budgeted_strict_degenerate_ends(ctx, B, world):
    W, H = W0, H0
    n0, L = BUDGET["n0"], BUDGET["L"]
    a = world.accel("random200")
    p = B.pathtrace_params(W, H, n0)
    out, out_lv = ctx.pathtrace_accel_budgeted(a, p, B.pathtrace_budget_params(max_level=L, target=1e6, radius=3), want_levels=True)
    assert same(out, world.ref("random200", W, H, n0)) and not out_lv.any(), "a target nothing exceeds: the plain n0 render"
    assert ctx.last_budget() == ([W * H] + [0] * 8, float(n0))
    out, out_lv = ctx.pathtrace_accel_budgeted(a, p, B.pathtrace_budget_params(max_level=L, target=1e-3, radius=3), want_levels=True)
    assert same(out, world.ref("random200", W, H, n0 << L)) and (out_lv == L).all(), "a target everything exceeds: the plain n0 << L render"
    assert ctx.last_budget() == ([0] * L + [W * H] + [0] * (8 - L), float(n0 << L))


# ---- the careful tier ------------------------------------------------------------------------------------------------------------------
MODES = ["PT_MATH_FAST", "PT_MATH_FAST_CAREFUL"]


@pytest.mark.parametrize("mode", MODES)
def test_noise_guided_fast_is_the_chain_of_the_separate_accel_calls(ctx, B, world, mode):
    import torch
    W, H, spp = W0, H0, 6
    h = spp // 2
    m = getattr(B, mode)
    a = world.accel("random200")
    p = B.pathtrace_params(W, H, spp, math_mode=m)
    info = a.select_kernel(p)
    assert (info.kernel, info.math_mode) == (B.PT_KERNEL_BVH, B.PT_MATH_FAST_CAREFUL)
    d = B.pathtrace_denoise_params(W, H)
    k, radius = B.pathtrace_noise_defaults()
    fused = ctx.pathtrace_accel_denoised_adaptive(a, p, d)
    assert same(fused, ctx.pathtrace_accel_denoised_adaptive(a, p, d)), "twice: the same bits"
    t_rgba, p_rgba = guarded(torch, shape=(H, W))
    t_half, p_half = guarded(torch, shape=(H, W))
    t_nt, p_nt = guarded(torch, shape=(H, W))
    t_pid, p_pid = guarded(torch, shape=(H, W))
    t_var, p_var = guarded_plane(torch, shape=(H, W))
    torch.cuda.synchronize()
    ctx.pathtrace_accel_guides_device(a, W, H, p_nt, p_pid)
    ctx.pathtrace_accel_device(a, B.pathtrace_params(W, H, spp, math_mode=m, sample_end=h), p_rgba)
    ctx.synchronize()
    t_half[1:-1].copy_(t_rgba[1:-1])
    torch.cuda.synchronize()
    ctx.pathtrace_accel_device(a, B.pathtrace_params(W, H, spp, math_mode=m, sample_begin=h), p_rgba)
    ctx.pathtrace_noise_device(W, H, p_half, 2.0, p_rgba, radius, p_var)
    ctx.pathtrace_denoise_adaptive_device(d, k, p_rgba, p_nt, p_pid, p_var, p_rgba)
    ctx.synchronize()
    assert same(fused, inner(t_rgba)), differing(fused, inner(t_rgba))
    inner(t_half), inner(t_nt), inner(t_pid), inner(t_var)   # the guard rows
    # the plain fixed-tolerance chain likewise
    fused = ctx.pathtrace_accel_denoised(a, p, d)
    t_out, p_out = guarded(torch, shape=(H, W))
    torch.cuda.synchronize()
    ctx.pathtrace_accel_device(a, p, p_out)
    ctx.pathtrace_denoise_device(d, p_out, p_nt, p_pid, p_out)
    ctx.synchronize()
    assert same(fused, inner(t_out))


@pytest.mark.parametrize("mode", MODES)
def test_budgeted_fast_is_the_chain_of_the_separate_accel_calls(ctx, B, world, mode):
    import torch
    W, H = W0, H0
    n0, L, T = BUDGET["n0"], BUDGET["L"], BUDGET["T"]
    m = getattr(B, mode)
    a = world.accel("random200")
    p = B.pathtrace_params(W, H, n0, math_mode=m)
    info = a.select_kernel(p)
    assert (info.kernel, info.math_mode) == (B.PT_KERNEL_BVH, B.PT_MATH_FAST_CAREFUL)
    b = B.pathtrace_budget_params(max_level=L, target=T, radius=3)
    fused, fused_lv = ctx.pathtrace_accel_budgeted(a, p, b, want_levels=True)
    again, again_lv = ctx.pathtrace_accel_budgeted(a, p, b, want_levels=True)
    assert same(fused, again) and np.array_equal(fused_lv, again_lv), "twice: the same bits"
    t_acc, p_acc = guarded(torch, shape=(H, W))
    t_half, p_half = guarded(torch, shape=(H, W))
    t_enc, p_enc = guarded(torch, shape=(H, W))
    t_var, p_var = guarded_plane(torch, shape=(H, W))
    t_zero, p_zero = guarded_bytes(torch, np.zeros((H, W), np.uint8))
    t_lv, p_lv = guarded_bytes(torch, shape=(H, W))
    t_list, p_list = guarded_bytes(torch, shape=(H, W), dtype=torch.int32, fill=-3)
    t_counts = torch.zeros(9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.pathtrace_accel_device(a, B.pathtrace_params(W, H, 2 * n0, math_mode=m, sample_end=n0 // 2), p_acc)
    ctx.synchronize()
    t_half[1:-1].copy_(t_acc[1:-1])
    torch.cuda.synchronize()
    ctx.pathtrace_accel_device(a, B.pathtrace_params(W, H, 2 * n0, math_mode=m, sample_begin=n0 // 2, sample_end=n0), p_acc)
    ctx.pathtrace_budget_resolve_device(W, H, p_acc, p_zero, p_enc)
    ctx.pathtrace_noise_device(W, H, p_half, float(f32(2 * n0) / f32(n0 // 2)), p_enc, 3, p_var)
    ctx.pathtrace_budget_levels_device(W, H, p_var, T, L, p_lv)
    ctx.pathtrace_budget_lists_device(W, H, p_lv, L, p_list, t_counts.data_ptr())
    ctx.synchronize()
    counts = t_counts.cpu().numpy()
    list_equals_plain = []
    for r in range(1, L + 1):
        n = int(counts[r:].sum())
        if n:
            q = B.pathtrace_params(W, H, n0 << r, math_mode=m, sample_begin=n0 << (r - 1), sample_end=n0 << r)
            if r == 1:   # measured, not promised: the list kernel's careful samples against the plain BVH kernel's over the same range.
                # The plain kernel would encode at sample_end == spp, so it runs at divisor 2 spp from half the plane and is doubled:
                # exact scalings by 2 (the divisors are powers of two).
                t_plain, p_plain = guarded(torch, inner(t_acc) * f32(0.5))
                torch.cuda.synchronize()
                ctx.pathtrace_accel_device(a, B.pathtrace_params(W, H, 2 * (n0 << r), math_mode=m, sample_begin=q.sample_begin,
                                                                 sample_end=q.sample_end), p_plain)
            ctx.pathtrace_accel_list_device(a, q, p_list, n, 1.0 if r == 1 else 0.5, p_acc)
            if r == 1:
                ctx.synchronize()
                lst = inner_int(t_list, fill=-3).reshape(-1).view(np.uint32)[:n]
                list_equals_plain.append(same(inner(t_acc).reshape(-1, 4)[lst], inner(t_plain).reshape(-1, 4)[lst] * f32(2)))
    ctx.pathtrace_budget_resolve_device(W, H, p_acc, p_lv, p_acc)
    ctx.synchronize()
    print(f"{mode}: careful list kernel bit-equal to the plain BVH kernel over the same range: {list_equals_plain}")
    assert np.array_equal(inner_int(t_lv), fused_lv)
    assert same(inner(t_acc), fused), differing(inner(t_acc), fused)
    assert len(np.unique(fused_lv)) == L + 1, "every level is exercised"
    inner(t_half), inner(t_enc), inner(t_var), inner_int(t_zero), inner_int(t_list, fill=-3)   # the guard rows


# ---- the app -----------------------------------------------------------------------------------------------------------------------------
def _app(B):
    return os.path.join(os.path.dirname(os.path.dirname(B.LIB_PATH)), "bin", "pathtracer")


def _write_room(tmp_path):
    planes, spheres = scene("random200")
    with open(tmp_path / "room.scene", "w") as f:
        for kind, table in (("plane", planes), ("sphere", spheres)):
            for rec in np.asarray(table, f32).reshape(-1, 12):
                f.write(kind + " " + " ".join(repr(float(x)) for x in rec) + "\n")


APP_CHAINS = {"noise-guided": ["--denoise", "--noise-guided"], "budget": ["--budget=2", "--noise-target", "48"]}


@pytest.mark.parametrize("chain", list(APP_CHAINS))
def test_app_accel_chains(B, tmp_path, chain):
    """--scene FILE --accel bvh with --denoise --noise-guided, and with --budget: the PNG bytes of --accel linear, on both save routes, and
    the same `budget:` line."""
    _write_room(tmp_path)
    spp, H = 4, 16

    def run(*extra):
        r = subprocess.run([_app(B), str(spp), str(H), "--out", "o.png", "--quiet", "--full-teardown", "--scene", "room.scene"] + list(extra),
                           capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        return (tmp_path / "o.png").read_bytes(), [l for l in r.stdout.splitlines() if l.startswith("budget:")]

    for route in ([], ["--gpu-postprocess"]):
        want, want_budget = run("--accel", "linear", *APP_CHAINS[chain], *route)
        got, got_budget = run("--accel", "bvh", *APP_CHAINS[chain], *route)
        assert got == want, (chain, route)
        assert got_budget == want_budget and len(got_budget) == (1 if chain == "budget" else 0), (chain, route, got_budget)


def test_app_refusals_that_stay(B, tmp_path):
    _write_room(tmp_path)
    for bad in (["--accel", "bvh", "--denoise"], ["--accel", "bvh", "--budget", "--gpus", "2"],
                ["--accel", "bvh", "--budget", "--sphere-precision", "ds"]):
        r = subprocess.run([_app(B), "4", "16", "--quiet", "--scene", "room.scene"] + bad, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode != 0 and "now running app" not in r.stdout, (bad, r.stdout)
        assert ("--accel" in r.stdout) or ("--budget" in r.stdout), (bad, r.stdout)
    r = subprocess.run([_app(B), "4", "16", "--quiet", "--accel", "bvh", "--denoise"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0 and "--accel" in r.stdout and "--noise-guided" in r.stdout, r.stdout


# ---- refusals that need a context ----------------------------------------------------------------------------------------------------------
def refused(B, call, says=None, status=INVALID):
    with pytest.raises(B.McError) as e:
        call()
    assert e.value.status == status, e.value
    if says:
        assert says in str(e.value), e.value


def test_refusals(ctx, B, world):
    import torch
    W, H = 16, 8
    a = world.accel("random200")
    L = B.lib()
    ok_p = B.pathtrace_params(W, H, 4)
    ok_d = B.pathtrace_denoise_params(W, H)
    ok_b = B.pathtrace_budget_params(max_level=1)
    k = torch.zeros((3, H, W, 4), dtype=torch.float32, device="cuda")
    t_list = torch.arange(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nt, pid, acc = (k[i].data_ptr() for i in range(3))
    lst = t_list.data_ptr()
    # the four calls that take render parameters, each as a function of them
    with_p = {
        "denoised": lambda p: ctx.pathtrace_accel_denoised(a, p, ok_d),
        "adaptive": lambda p: ctx.pathtrace_accel_denoised_adaptive(a, p, ok_d),
        "budgeted": lambda p: ctx.pathtrace_accel_budgeted(a, p, ok_b),
        "list": lambda p: ctx.pathtrace_accel_list_device(a, p, lst, 8, 1.0, acc),
    }
    whole = ("denoised", "adaptive", "budgeted")
    for name, call in with_p.items():
        # a row tile, an interleave
        says = "whole-image" if name == "list" else "whole images"
        refused(B, lambda: call(B.pathtrace_params(W, H, 4, row_begin=0, row_end=4)), says)
        refused(B, lambda: call(B.pathtrace_params(W, H, 4, row_block=2, row_stride=4)), says)
        # flags, an extended precision (MC_ERR_UNSUPPORTED, named)
        refused(B, lambda: call(B.pathtrace_params(W, H, 4, flags=B.PT_NO_BOX_KERNEL)), "flags must be 0")
        refused(B, lambda: call(B.pathtrace_params(W, H, 4, flags=B.pt_precision(B.PT_PREC_DS))), "MC_PT_PREC_DS", status=UNSUPPORTED)
        refused(B, lambda: call(B.pathtrace_params(W, H, 4, flags=B.pt_precision(B.PT_PREC_FP64))), "MC_PT_PREC_FP64", status=UNSUPPORTED)
        refused(B, lambda: call(B.pathtrace_params(W, H, 4, math_mode=7)), "math_mode")
    for name in whole:
        # a sample range
        refused(B, lambda: with_p[name](B.pathtrace_params(W, H, 4, sample_end=2)), "whole renders")
        refused(B, lambda: with_p[name](B.pathtrace_params(W, H, 4, sample_begin=2)), "whole renders")
    # odd n0, and the budget's own parameters
    refused(B, lambda: with_p["budgeted"](B.pathtrace_params(W, H, 3)), "even")
    refused(B, lambda: ctx.pathtrace_accel_budgeted(a, ok_p, B.pathtrace_budget_params(flags=1)), "flags")
    refused(B, lambda: ctx.pathtrace_accel_budgeted(a, ok_p, B.pathtrace_budget_params(radius=5)), "radius")
    refused(B, lambda: ctx.pathtrace_accel_denoised_adaptive(a, B.pathtrace_params(W, H, 1), ok_d), "spp")
    refused(B, lambda: ctx.pathtrace_accel_denoised_adaptive(a, ok_p, ok_d, k_noise=0.0), "k_noise")
    refused(B, lambda: ctx.pathtrace_accel_denoised(a, ok_p, B.pathtrace_denoise_params(W, H, passes=9)), "passes")
    refused(B, lambda: ctx.pathtrace_accel_denoised(a, ok_p, B.pathtrace_denoise_params(W + 1, H)), "width and height")
    # NULL outputs; both or neither image output
    out = np.zeros((H, W, 4), f32)
    out8 = np.zeros((H, W, 4), np.uint8)
    o, o8 = out.ctypes.data_as(C.c_void_p), out8.ctypes.data_as(C.c_void_p)
    detail = lambda: L.mc_last_error_detail().decode()   # noqa: E731
    for both in ((None, None), (o, o8)):
        assert L.mc_pathtrace_render_accel_denoised(ctx._h, a._h, C.byref(ok_p), C.byref(ok_d), *both) == INVALID and "exactly one" in detail()
        assert L.mc_pathtrace_render_accel_denoised_adaptive(ctx._h, a._h, C.byref(ok_p), C.byref(ok_d), 4.0, 3, *both) == INVALID
        assert "exactly one" in detail()
        assert L.mc_pathtrace_render_accel_budgeted(ctx._h, a._h, C.byref(ok_p), C.byref(ok_b), *both, None) == INVALID and "exactly one" in detail()
    assert L.mc_pathtrace_render_accel_denoised(ctx._h, a._h, None, C.byref(ok_d), o, None) == INVALID and "NULL" in detail()
    assert L.mc_pathtrace_render_accel_denoised(ctx._h, a._h, C.byref(ok_p), None, o, None) == INVALID and "NULL" in detail()
    assert L.mc_pathtrace_render_accel_budgeted(ctx._h, a._h, C.byref(ok_p), None, o, None, None) == INVALID and "NULL" in detail()
    assert L.mc_pathtrace_render_accel_denoised(ctx._h, None, C.byref(ok_p), C.byref(ok_d), o, None) == INVALID and "NULL" in detail()
    guides = lambda *args: (lambda: ctx.pathtrace_accel_guides_device(a, *args))   # noqa: E731
    refused(B, guides(W, H, 0, pid), "NULL")
    refused(B, guides(W, H, nt, 0), "NULL")
    refused(B, guides(0, H, nt, pid), "width and height")
    refused(B, guides(W, 0, nt, pid), "width and height")
    # a misaligned plane, planes that overlap
    refused(B, guides(W, H, nt + 4, pid), "aligned")
    refused(B, guides(W, H, nt, pid + 8), "aligned")
    refused(B, guides(W, H, nt, nt + 16 * W), "overlap")
    lr = lambda *args: (lambda: ctx.pathtrace_accel_list_device(a, B.pathtrace_params(W, H, 8, sample_begin=4), *args))   # noqa: E731
    refused(B, lr(lst, 8, 1.0, 0), "NULL")
    refused(B, lr(0, 8, 1.0, acc), "NULL")
    refused(B, lr(lst, 8, 1.0, acc + 4), "aligned to 16")
    refused(B, lr(lst + 2, 4, 1.0, acc), "aligned to 4")
    # a list that overlaps the plane
    refused(B, lr(acc + 64, 8, 1.0, acc), "overlaps")
    refused(B, lambda: ctx.pathtrace_accel_list_device(a, B.pathtrace_params(W, H, 8, sample_begin=4, sample_end=4), lst, 8, 1.0, acc))
    # a destroyed object
    live = B.PathtraceAccel(*scene("one"))
    dead = C.c_void_p(live._h.value)
    live.close()
    assert L.mc_pathtrace_accel_guides_device_async(ctx._h, dead, W, H, nt, pid, None) == INVALID and "destroyed" in detail()
    assert L.mc_pathtrace_render_accel_budgeted(ctx._h, dead, C.byref(ok_p), C.byref(ok_b), o, None, None) == INVALID and "destroyed" in detail()
    # the context renders on after every refusal
    ctx.pathtrace_accel_guides_device(a, W, H, nt, pid)
    ctx.pathtrace_accel_list_device(a, B.pathtrace_params(W, H, 8, sample_begin=4), lst, 8, 0.5, acc)
    ctx.synchronize()
    ctx.pathtrace_accel_budgeted(a, ok_p, ok_b)
    ctx.pathtrace_accel_denoised_adaptive(a, ok_p, ok_d)
