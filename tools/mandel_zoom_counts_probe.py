"""Zoom sequences from count keyframes (mc_mandelbrot_zoom_counts_*) measured on one context.

1. The compose stage alone at 1920 x 1280 and 7680 x 5120, M = 50 000, on the F64 K4 pair (scales 4e-7 and 2e-7): the existing vec4 compose
   (mc_mandelbrot_zoom_compose_device_async, unchanged code: the yardstick) and the count compose
   (mc_mandelbrot_zoom_compose_counts_device_async) in each colouring, to vec4 and to RGBA8, at r = 0.5, 0.75 and 1.  HIP events, warm
   launches, best of ROUNDS rounds, the variants alternating.
2. The sequence object: a push of each kind against mc_mandelbrot_zoom_push of the same view (plain colouring), and a mid-octave frame to RGBA8 (table
   kernel + compose for the equalised colourings), device time from mc_context_last_timing.  The by-hand stage checks and compares its
   host map on every call (200 KB at M = 50 000), which an event pair around a 20-microsecond kernel sees; the sequence object keeps its
   tables on the device, so its frame is the figure to read at the small size.  The table kernel alone: a 64-pixel frame at M = 50 000,
   with and without it.
3. The seam in the library's terms at 1920 x 1280: mean and maximum of |map_wide[n] - map_deep[n]| / M over the wide keyframe's escaped
   pixels, the maps taken from mc_mandelbrot_zoom_counts_maps.
    On an MI355X:  python tools/mandel_zoom_counts_probe.py > profiles/mandel_zoom_counts_probe.txt"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import mandel_perturb_ref as R  # noqa: E402

B = entry.load_package().bindings
ROUNDS = 5
ASPECT = 2.0 / 3.0
M = 50000
SCALES = (4e-7, 2e-7)
K4 = (float(R.DEEP_CENTRE[0]), float(R.DEEP_CENTRE[1]))
MODES = (("plain", 0), ("equalised", B.MANDEL_COLOUR_EQUALISED), ("smooth", B.MANDEL_COLOUR_SMOOTH),
         ("smooth-equalised", B.MANDEL_COLOUR_SMOOTH_EQUALISED))
RS = (0.5, 0.75, 1.0)


def event_ms(stream, launch, warm):
    for _ in range(warm):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    launch()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def best_of(stream, variants, rounds=ROUNDS):
    """{name: (best ms, worst ms)} over `rounds` rounds alternating the variants (two warm launches in the first round)."""
    out = {}
    for r in range(rounds):
        for name, launch in variants:
            ms = event_ms(stream, launch, warm=2 if r == 0 else 0)
            lo, hi = out.get(name, (ms, ms))
            out[name] = (min(lo, ms), max(hi, ms))
    return out


def k4_params(W, H, scale, flags=0):
    return B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_F64, centre=K4, scale=(scale, scale * ASPECT), flags=flags)


def histogram(plane, shift):
    return np.bincount(np.minimum(plane.reshape(-1).astype(np.int64) >> shift, M), minlength=M + 1).astype(np.uint32)


def stage(ctx, stream, W, H):
    """The compose stage's times; returns {(mode, r): best ms to RGBA8} for the sequence's table-kernel line."""
    s = stream.cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    key = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    n = [torch.empty((H, W), **i32) for _ in range(2)]
    q = [torch.empty((H, W), **i32) for _ in range(2)]
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    out8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    for i, scale in enumerate(SCALES):
        ctx.mandelbrot_device(k4_params(W, H, scale), key[i].data_ptr(), n[i].data_ptr(), stream=s)
        ctx.mandelbrot_smooth_device(k4_params(W, H, scale, B.MANDEL_COLOUR_SMOOTH), 0, 0, q[i].data_ptr(), stream=s)
    stream.synchronize()
    # a mid-octave frame's maps: the blend of the two keyframes' own
    hn = [histogram(a.cpu().numpy().view(np.uint32), 0) for a in n]
    hq = [histogram(a.cpu().numpy().view(np.uint32), 8) for a in q]
    rank = B.zoom_blend_map(B.equalise_map(M, hn[0]), B.equalise_map(M, hn[1]), 1, 2)
    knots = B.zoom_blend_map(B.smooth_equalise_map(M, hq[0]), B.smooth_equalise_map(M, hq[1]), 1, 2)
    planes = {"plain": (n, None), "equalised": (n, rank), "smooth": (q, None), "smooth-equalised": (q, knots)}
    variants = []
    for r in RS:
        variants.append((f"vec4 keyframes        -> vec4  r={r}",
                         lambda r=r: ctx.zoom_compose_device(W, H, key[0].data_ptr(), key[1].data_ptr(), r, out.data_ptr(), 0, stream=s)))
        variants.append((f"vec4 keyframes        -> rgba8 r={r}",
                         lambda r=r: ctx.zoom_compose_device(W, H, key[0].data_ptr(), key[1].data_ptr(), r, 0, out8.data_ptr(), stream=s)))
    for mode, flag in MODES:
        p = k4_params(W, H, SCALES[0], flag)
        pl, table = planes[mode]
        for r in RS:
            variants.append((f"counts {mode:16s}-> vec4  r={r}", lambda r=r, p=p, pl=pl, table=table: ctx.zoom_compose_counts_device(
                p, pl[0].data_ptr(), pl[1].data_ptr(), table, r, out.data_ptr(), 0, stream=s)))
            variants.append((f"counts {mode:16s}-> rgba8 r={r}", lambda r=r, p=p, pl=pl, table=table: ctx.zoom_compose_counts_device(
                p, pl[0].data_ptr(), pl[1].data_ptr(), table, r, 0, out8.data_ptr(), stream=s)))
    with torch.cuda.stream(stream):
        t = best_of(stream, variants)
    print(f"{W} x {H}, M = {M}:")
    for name, _ in variants:
        lo, hi = t[name]
        yard = t[f"vec4 keyframes        -> {name.split('-> ')[1]}"][0]
        print(f"    {name:42s} {lo:8.4f} ms (worst {hi:8.4f})   {lo / yard:5.2f} x the vec4 compose", flush=True)
    return {(mode, r): t[f"counts {mode:16s}-> rgba8 r={r}"][0] for mode, _ in MODES for r in RS}


def sequence(ctx, W, H, compose_ms):
    print(f"{W} x {H}, M = {M}: the sequence object (device time of mc_context_last_timing, best of {ROUNDS})")
    for mode, flag in (("vec4 keyframes", None),) + MODES:
        best_push, best_frame = [], []
        for _ in range(ROUNDS):
            with (ctx.zoom(W, H) if flag is None else ctx.zoom_counts(W, H)) as z:
                push = []
                for scale in SCALES:
                    z.push(k4_params(W, H, scale, flag or 0))
                    push.append(ctx.last_timing()[0])
                if flag is None:
                    z.frame(B.zoom_ratio(1, 2), want_rgba=False, want_rgba8=True)
                else:
                    z.frame(1, 2, want_rgba=False, want_rgba8=True)
                k, c = ctx.last_timing()
                best_push.append(min(push))
                best_frame.append((k, c))
        k, c = min(best_frame)
        line = f"    {mode:18s} push {min(best_push):9.3f} ms   mid-octave frame to RGBA8: kernels {k:7.4f} ms, copy {c:7.4f} ms"
        if flag is not None:
            line += f"   (the stage by hand at r = 0.75, its host-side map checks inside the event pair: {compose_ms[(mode, 0.75)]:7.4f} ms)"
        print(line, flush=True)


def table_kernel(ctx, W=8, H=8):
    """The table kernel's time, where the compose has nothing to do: a frame of 64 pixels at M = 50 000.  Plain and smooth launch no table
    kernel and are the baseline; the equalised colourings add it (M + 1 or M threads)."""
    times = {}
    for mode, flag in MODES:
        best = []
        with ctx.zoom_counts(W, H) as z:
            for scale in SCALES:
                z.push(k4_params(W, H, scale, flag))
            for _ in range(2 + ROUNDS):
                z.frame(1, 2, want_rgba=False, want_rgba8=True)
                best.append(ctx.last_timing()[0])
        times[mode] = min(best[2:])
    print(f"table kernel, {W} x {H} frame at M = {M} (frame kernels, best of {ROUNDS}): " +
          ", ".join(f"{mode} {ms:.4f} ms" for mode, ms in times.items()) +
          f"; equalised - plain = {times['equalised'] - times['plain']:.4f} ms, smooth-equalised - smooth = "
          f"{times['smooth-equalised'] - times['smooth']:.4f} ms", flush=True)


def seam(ctx, W, H):
    with ctx.zoom_counts(W, H) as z:
        for scale in SCALES:
            z.push(k4_params(W, H, scale, B.MANDEL_COLOUR_EQUALISED))
        mw, md = z.maps()
    n = ctx.mandelbrot(k4_params(W, H, SCALES[0]), want_rgba=False)[1]
    esc = n[n < M].astype(np.int64)
    d = np.abs(mw.astype(np.int64)[esc] - md.astype(np.int64)[esc]) / M
    print(f"seam, {W} x {H}, K4 centre, scales {SCALES[0]:g} and {SCALES[1]:g}, equalised: |map_wide[n] - map_deep[n]| / M over the wide "
          f"keyframe's {esc.size} escaped pixels: mean {d.mean():.4f}, max {d.max():.4f} of a palette turn (the step the vec4 sequence "
          f"shows along the deep keyframe's rectangle; a count frame shows none)", flush=True)


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# zoom sequences from count keyframes: device {name}, {cus} CUs; shader clock under load {ctx.measure_clock():.0f} MHz; "
          f"build {B.build_id()}", flush=True)
    print(f"# stage: device forms; HIP events; best of {ROUNDS} rounds after two warm launches, the variants alternating")
    stream = torch.cuda.Stream()
    for W, H in ((1920, 1280), (7680, 5120)):
        compose_ms = stage(ctx, stream, W, H)
        torch.cuda.synchronize()
        sequence(ctx, W, H, compose_ms)
    table_kernel(ctx)
    seam(ctx, 1920, 1280)
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
