"""The Buddhabrot on the MI355X: every case checks the device plane AND the five statistics EQUAL to the numpy restatement of
include/mc_compute.h (tests/buddhabrot_ref.py) — integer adds commute, so a kernel with a dynamic schedule has one right answer — for the
shipped form and for both forms through their measurement bits.  The shapes are the smallest at which the kernels can still go wrong:
one lane, one wave and one more, a run that is refilled and its tail, k across 2^32, planes of one bin and of no round size, waves that
never plot, a wave whose lanes are in both phases with orbit lengths from 0 to 2000.  Then the calls around the kernel (composition,
streams, NULL statistics, the blocking render), the tone-map kernel against the host form, the rank-map route, and the app end to end."""
import os
import subprocess

import numpy as np
import pytest

import buddhabrot_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
VIEW = (-0.5, 0.0, 3.0, 2.0)
SMALL = dict(width=48, height=32, max_iter=64, view=VIEW)
FORMS = [0, 1, 2]   # the shipped choice, MC_BUDDHA_KERNEL_PLAIN, MC_BUDDHA_KERNEL_POOLED

CASES = {
    "cross-check M64": dict(SMALL, samples=1 << 14),
    "cross-check M200 min20": dict(width=48, height=32, samples=1 << 16, max_iter=200, min_iter=20, view=VIEW),
    "cross-check 1x1": dict(width=1, height=1, samples=1000, max_iter=64, seed=3, view=(0.0, 0.0, 8.0, 8.0)),
    "1 sample": dict(SMALL, samples=1),
    "63 samples": dict(SMALL, samples=63),
    "64 samples": dict(SMALL, samples=64),
    "65 samples": dict(SMALL, samples=65),
    "1000 samples": dict(SMALL, samples=1000),
    "2^16 + 1 samples": dict(SMALL, samples=(1 << 16) + 1),
    "k across 2^32": dict(SMALL, samples=65, sample_begin=(5 << 32) - 17),
    "7 x 5": dict(width=7, height=5, samples=1 << 12, max_iter=64, view=VIEW),
    "mirrored": dict(SMALL, samples=1 << 12, view=(-0.5, 0.0, -3.0, 2.0)),
    "all skipped": dict(SMALL, samples=1 << 12, sample_window=(-0.1, 0.0, 0.2, 0.2)),
    "all outside": dict(SMALL, samples=1 << 12, sample_window=(3.0, 3.0, 0.5, 0.5)),
    "min_iter = M": dict(SMALL, samples=1 << 12, min_iter=64),
    "M = 1": dict(SMALL, samples=1 << 12, max_iter=1),
    "boundary-hugging window": dict(width=48, height=32, samples=1 << 12, max_iter=2000, view=VIEW, sample_window=(-0.75, 0.1, 0.05, 0.05)),
}
EXPECTED = {   # the header's table: (contributing, points, added, largest bin)
    "cross-check M64": (14785, 28561, 17509, 32),
    "cross-check M200 min20": (816, 40097, 38739, 134),
    "cross-check 1x1": (None, None, None, 1850),
}
_reference = {}


def reference(name):
    """(plane, stats tuple) of a case by the restatement: computed once, shared, never written to."""
    if name not in _reference:
        plane, st = R.density(R.params(**CASES[name]))
        plane.setflags(write=False)
        _reference[name] = (plane, R.stats_tuple(st))
    return _reference[name]


def device_density(ctx, B, kws, flags=0, plane=None, want_stats=True, streams=None):
    """The sum of the requests `kws` (a list of params() keywords of one plane size) launched into ONE device plane and one statistics
    record; plane: the words it starts from.  Returns (plane uint32, stats tuple or None)."""
    import torch
    p0 = B.buddhabrot_params(**kws[0])
    start = np.zeros((p0.height, p0.width), np.uint32) if plane is None else plane
    d_plane = torch.from_numpy(start.view(np.int32).copy()).cuda()
    d_stats = torch.zeros(5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for j, kw in enumerate(kws):
        ctx.buddhabrot_device(B.buddhabrot_params(flags=flags, **kw), d_plane.data_ptr(), d_stats.data_ptr() if want_stats else 0,
                              stream=streams[j % len(streams)].cuda_stream if streams else 0)
    ctx.synchronize()
    torch.cuda.synchronize()
    st = tuple(int(v) for v in d_stats.cpu().numpy().view(np.uint64))
    return d_plane.cpu().numpy().view(np.uint32), (st if want_stats else None)


@pytest.mark.parametrize("flags", FORMS, ids=["shipped", "plain", "pooled"])
@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_restatement(ctx, B, name, flags):
    want, ws = reference(name)
    got, gs = device_density(ctx, B, [CASES[name]], flags)
    assert gs == ws, (gs, ws)
    assert np.array_equal(got, want), int((got != want).sum())
    if name in EXPECTED:
        contributing, points, added, largest = EXPECTED[name]
        assert int(got.max()) == largest and (contributing is None or gs[2:] == (contributing, points, added))
    if name == "boundary-hugging window" and flags == 0:   # the case is what it is meant to be: skipped, short, long and never-escaping samples side by side
        k = np.arange(1 << 12, dtype=np.uint64)
        cx, cy = R.sample_c(R.params(**CASES[name]), k)
        n = R.classify(cx, cy, 2000)[~R.interior(cx, cy)]
        assert gs[1] > 1000 and n.min() < 30 and ((n > 1000) & (n < 2000)).any() and (n == 2000).any()


@pytest.mark.parametrize("flags", FORMS, ids=["shipped", "plain", "pooled"])
def test_ranges_compose_on_the_device(ctx, B, flags):
    want, ws = reference("cross-check M64")
    N = 1 << 14
    parts = [dict(SMALL, samples=N // 3), dict(SMALL, samples=N - N // 3, sample_begin=N // 3)]
    got, gs = device_density(ctx, B, parts, flags)
    assert gs == ws and np.array_equal(got, want)


@pytest.mark.parametrize("flags", FORMS, ids=["shipped", "plain", "pooled"])
def test_two_streams_into_one_plane(ctx, B, flags):
    import torch
    want, ws = reference("cross-check M64")
    N = 1 << 14
    parts = [dict(SMALL, samples=N // 2), dict(SMALL, samples=N - N // 2, sample_begin=N // 2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got, gs = device_density(ctx, B, parts, flags, streams=streams)
    for s in streams:
        s.synchronize()
    assert gs == ws and np.array_equal(got, want)


@pytest.mark.parametrize("flags", FORMS, ids=["shipped", "plain", "pooled"])
def test_prefilled_plane_guard_words_and_null_stats(ctx, B, flags):
    import torch
    kw = CASES["7 x 5"]
    fresh, ws = reference("7 x 5")
    rng = np.random.default_rng(5)
    before = rng.integers(0, 2 ** 32, 35 + 32, dtype=np.uint32)
    before[16 + 3] = 2 ** 32 - 1                                           # a bin that wraps
    buf = torch.from_numpy(before.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    ctx.buddhabrot_device(B.buddhabrot_params(flags=flags, **kw), buf.data_ptr() + 64, 0)   # d_stats = NULL
    ctx.synchronize()
    after = buf.cpu().numpy().view(np.uint32)
    assert np.array_equal(after[16:16 + 35], before[16:16 + 35] + fresh.reshape(-1))        # (uint32: wraps as the plane does)
    assert np.array_equal(after[:16], before[:16]) and np.array_equal(after[-16:], before[-16:])
    assert fresh.reshape(-1)[3] > 0


def test_render_equals_the_device_call_and_the_host_call(ctx, B):
    for name in ("cross-check M64", "7 x 5", "all skipped"):
        want, ws = reference(name)
        for flags in FORMS:
            plane, st = ctx.buddhabrot(B.buddhabrot_params(flags=flags, **CASES[name]))
            assert st.as_tuple() == ws and np.array_equal(plane, want), (name, flags)
        k, c = ctx.last_timing()
        assert k > 0 and c >= 0
    plane, st = ctx.buddhabrot(B.buddhabrot_params(**CASES["1 sample"]))   # a second render starts from zero again, whatever came before
    assert np.array_equal(plane, reference("1 sample")[0]) and st.as_tuple() == reference("1 sample")[1]
    host, hs = B.buddhabrot_density(B.buddhabrot_params(**CASES["cross-check M64"]))
    assert np.array_equal(host, reference("cross-check M64")[0]) and hs.as_tuple() == reference("cross-check M64")[1]


def test_device_refusals(ctx, B):
    import torch
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for change, detail in ((dict(flags=3), "names both"), (dict(flags=8), "unknown bits"), (dict(max_iter=0), "max_iter is 0"),
                           (dict(view_scale_x=0.0), "view_scale_x is zero")):
        p = B.buddhabrot_params(8, 8, 10, max_iter=8)
        for k, v in change.items():
            setattr(p, k, v)
        with pytest.raises(B.McError) as e:
            ctx.buddhabrot_device(p, d.data_ptr())
        assert e.value.status == 1 and detail in str(e.value)
        with pytest.raises(B.McError) as e:
            ctx.buddhabrot(p)
        assert e.value.status == 1 and detail in str(e.value) and "mc_buddhabrot_render" in str(e.value)
    with pytest.raises(B.McError):
        ctx.buddhabrot_device(B.buddhabrot_params(8, 8, 10, max_iter=8), 0)
    ctx.synchronize()
    assert not d.cpu().numpy().any()


# ---- the tone map -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (65, 3), (257, 130)])
def test_tonemap_kernel_equals_the_host_form(ctx, B, W, H):
    import torch
    rng = np.random.default_rng(W)
    for L in (1, 255, 1 << 20):
        planes = [rng.integers(0, 2 * L + 2, (H, W)).astype(np.uint32) for _ in range(3)]
        planes[0].reshape(-1)[0] = 2 ** 32 - 1
        maps = [B.buddhabrot_sqrt_map(L), rng.integers(0, L + 1, L + 1).astype(np.uint32), np.arange(L + 1, dtype=np.uint32)]
        dev = [torch.from_numpy(q.view(np.int32)).cuda() for q in planes]
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for which, ms in (((0, 1, 2), maps), ((0, 0, 0), [maps[0]] * 3), ((0, 1, 2), maps)):   # three planes, one plane aliased, the cached table
            ctx.buddhabrot_tonemap_device(W, H, *(dev[j].data_ptr() for j in which), L, *ms, out.data_ptr())
            ctx.synchronize()
            want = B.buddhabrot_tonemap(*(planes[j] for j in which), L, *ms)
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), (L, which)
            assert np.array_equal(want.view(np.uint32), R.tonemap(*(planes[j] for j in which), L, *ms).view(np.uint32))
    bad = maps[2].copy()
    bad[1] = L + 1
    with pytest.raises(B.McError) as e:
        ctx.buddhabrot_tonemap_device(W, H, dev[0].data_ptr(), dev[0].data_ptr(), dev[0].data_ptr(), L, maps[0], maps[0], bad, out.data_ptr())
    assert e.value.status == 1 and "a map entry exceeds levels" in str(e.value)


def test_rank_map_route(ctx, B):
    """A density plane is a count plane: histogram -> mc_mandelbrot_equalise_map -> tone map, against numpy."""
    import torch
    plane, _ = reference("cross-check M200 min20")
    L = R.white_level([plane], 99.0)
    assert 1 < L < int(plane.max())
    d_plane = torch.from_numpy(plane.view(np.int32).copy()).cuda()
    d_hist = torch.zeros(L + 1, dtype=torch.int32, device="cuda")
    out = torch.zeros(plane.shape + (4,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.mandelbrot_histogram_device(d_plane.data_ptr(), 4, plane.size, L, d_hist.data_ptr())
    ctx.synchronize()
    hist = d_hist.cpu().numpy().view(np.uint32)
    assert np.array_equal(hist, np.bincount(np.minimum(plane, L).reshape(-1), minlength=L + 1))
    m = B.equalise_map(L, hist)
    below = np.concatenate([[0], np.cumsum(hist[:L], dtype=np.uint64)])   # C(j), j = 0 .. L
    want_map = np.append((np.uint64(L) * below[:L]) // below[L], L).astype(np.uint32)
    assert np.array_equal(m, want_map) and m[L] == L and (np.diff(m.astype(np.int64)) >= 0).all()
    ctx.buddhabrot_tonemap_device(plane.shape[1], plane.shape[0], d_plane.data_ptr(), d_plane.data_ptr(), d_plane.data_ptr(), L, m, m, m,
                                  out.data_ptr())
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), R.tonemap(plane, plane, plane, L, m, m, m).view(np.uint32))


# ---- the app ------------------------------------------------------------------------------------------------------------------------
def run_app(tmp_path, name, *args):
    out = tmp_path / name
    r = subprocess.run([APP, "--out", str(out), "--quiet"] + list(args), capture_output=True, text=True, cwd=tmp_path, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    from PIL import Image
    return np.asarray(Image.open(out).convert("RGBA")), r.stdout


def test_app_end_to_end(ctx, B, tmp_path):
    W, H, N = 96, 64, 1 << 16
    size = ["--width", str(W), "--height", str(H)]
    # grey, the defaults: render -> white level -> sqrt map -> tone map -> mc_convert_rgba8, by hand
    plane, st = ctx.buddhabrot(B.buddhabrot_params(W, H, N))
    L = R.white_level([plane], 99.9)
    m = B.buddhabrot_sqrt_map(L)
    want = ctx.convert_rgba8(B.buddhabrot_tonemap(plane, plane, plane, L, m, m, m), 255.0)
    img, text = run_app(tmp_path, "buddha.png", "--buddhabrot", str(N), *size)
    assert np.array_equal(img, want) and len(np.unique(img[..., 0])) > 16
    assert (f"samples {st.samples}, skipped {st.skipped}, contributing {st.contributing}, points {st.points}, added {st.added}" in text), text
    assert f"white level {L} " in text
    # the Nebulabrot, every option, converted on the device
    Ms = (50, 200, 1000)
    kw = dict(min_iter=5, seed=7, view=(-0.4, 0.1, 2.5, 2.0), sample_window=(-0.5, 0.0, 3.0, 3.0))
    planes = [ctx.buddhabrot(B.buddhabrot_params(W, H, N, max_iter=M, **kw))[0] for M in Ms]
    L = R.white_level(planes, 99.0)
    maps = []
    for q in planes:
        h = np.bincount(np.minimum(q, L).reshape(-1), minlength=L + 1).astype(np.uint32)
        h[0] = 0
        maps.append(B.equalise_map(L, h))
    want = ctx.convert_rgba8(B.buddhabrot_tonemap(*planes, L, *maps), 255.0)
    img, text = run_app(tmp_path, "nebula.png", "--buddhabrot", str(N), *size, "--nebula", *map(str, Ms), "--tone", "equalised", "--white", "99",
                        "--min-iter", "5", "--seed", "7", "--centre", "-0.4", "0.1", "--scale", "2.5", "2.0", "--sample-window", "-0.5", "0",
                        "3", "3", "--gpu-postprocess")
    assert np.array_equal(img, want)
    assert not np.array_equal(img[..., 0], img[..., 2]) and text.count("buddhabrot: max_iter") == 3
    # without --buddhabrot: what the app has always written for these options
    img, text = run_app(tmp_path, "plain.png", *size)
    assert np.array_equal(img, ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H))) and "buddhabrot" not in text
