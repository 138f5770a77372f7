"""Zoom sequences (mc_mandelbrot_zoom_*) measured on one context.

1. The compose kernel alone (mc_mandelbrot_zoom_compose_device_async) at 1920 x 1280 and 7680 x 5120, vec4 output and RGBA8 output, at
   r = 0.5, 0.75 and 1, beside the existing memory-bound yardsticks in the same process: mc_convert_rgba8_device_async (16 B read, 4 B
   written per pixel) and a device-to-device copy of 16 B per pixel.  HIP events, warm launches, best of ROUNDS rounds, the variants
   alternating.  The keyframes are two renders of the K4 view an octave apart.
2. A K = 4, F = 30 sequence of the K4 centre in F64 at 1920 x 1280, M = 50 000, ending at scale 1e-8: 5 keyframes + 121 composed frames
   through the sequence object, against direct renders of the same 121 views (mc_mandelbrot_render_rgba8 each); both leave RGBA8 on the
   host.  Device time from mc_context_last_timing (kernels + copy), and wall time of the calls.
    On an MI355X:  python tools/mandel_zoom_probe.py > profiles/mandel_zoom_probe.txt"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import mandel_perturb_ref as R  # noqa: E402

B = entry.load_package().bindings
ROUNDS = 5
ASPECT = 2.0 / 3.0
K4 = (float(R.DEEP_CENTRE[0]), float(R.DEEP_CENTRE[1]))


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


def k4_params(W, H, scale, max_iter):
    return B.mandelbrot_params(W, H, max_iter=max_iter, precision=B.PRECISION_F64, centre=K4, scale=(scale, scale * ASPECT))


def stage(ctx, stream, W, H):
    s = stream.cuda_stream
    key = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    out8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    for k, scale in zip(key, (2e-8, 1e-8)):
        ctx.mandelbrot_device(k4_params(W, H, scale, 2000), k.data_ptr(), 0, stream=s)
    stream.synchronize()
    w, d = key[0].data_ptr(), key[1].data_ptr()
    variants = [("copy 16 B", lambda: out.copy_(key[0], non_blocking=True)),
                ("convert_rgba8", lambda: ctx.convert_rgba8_device(w, W, H, 255.0, False, out8.data_ptr(), stream=s))]
    for r in (0.5, 0.75, 1.0):
        variants.append((f"compose vec4  r={r}", lambda r=r: ctx.zoom_compose_device(W, H, w, d, r, out.data_ptr(), 0, stream=s)))
        variants.append((f"compose rgba8 r={r}", lambda r=r: ctx.zoom_compose_device(W, H, w, d, r, 0, out8.data_ptr(), stream=s)))
    with torch.cuda.stream(stream):
        t = best_of(stream, variants)
    px = W * H
    print(f"{W} x {H}:")
    for name, _ in variants:
        lo, hi = t[name]
        moved = 32 if name.startswith("copy") else 20 if "rgba8" in name else 32   # the output pixel's own bytes: 16 read + what is written
        print(f"    {name:22s} {lo:8.4f} ms (worst {hi:8.4f})   {px * moved / lo / 1e9:6.2f} TB/s at {moved} B per pixel   "
              f"{lo / t['copy 16 B'][0]:5.2f} x the copy   {lo / t['convert_rgba8'][0]:5.2f} x convert_rgba8", flush=True)


def sequence(ctx, W=1920, H=1280, K=4, F=30, M=50000, deepest=1e-8):
    views = []           # (keyframe index j, step s) -> the frame's own scale: deepest * 2^(K - j) * ratio
    for i in range(K * F + 1):
        j = 0 if i == 0 else (i - 1) // F
        step = 0 if i == 0 else i - j * F
        views.append(deepest * 2.0 ** (K - j) * B.zoom_ratio(step, F))
    for attempt in range(2):                                                       # (the first pass warms both routes up)
        t0 = time.perf_counter()
        dev_direct = 0.0
        for scale in views:
            ctx.mandelbrot_rgba8(k4_params(W, H, scale, M))
            k, c = ctx.last_timing()
            dev_direct += k + c
        wall_direct = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        dev_key = dev_frames = 0.0
        with ctx.zoom(W, H) as z:
            for j in range(K + 1):
                z.push(k4_params(W, H, deepest * 2.0 ** (K - j), M))
                dev_key += ctx.last_timing()[0]
                for r in ([1.0] if j == 0 else [B.zoom_ratio(s, F) for s in range(1, F + 1)]):
                    z.frame(r, want_rgba=False, want_rgba8=True)
                    k, c = ctx.last_timing()
                    dev_frames += k + c
        wall_seq = (time.perf_counter() - t0) * 1e3
    n = len(views)
    print(f"K4 centre, F64, {W} x {H}, M = {M}, K = {K}, F = {F}: {n} views from scale {views[0]:.3g} to {views[-1]:.3g}, RGBA8 on the host")
    print(f"    direct renders   device {dev_direct:9.3f} ms ({dev_direct / n:7.3f} per frame)   wall {wall_direct:9.3f} ms")
    print(f"    keyframes+frames device {dev_key + dev_frames:9.3f} ms = {K + 1} keyframes {dev_key:9.3f} + {n} frames {dev_frames:9.3f} "
          f"({dev_frames / n:7.4f} per frame)   wall {wall_seq:9.3f} ms")
    print(f"    direct / sequence: device {dev_direct / (dev_key + dev_frames):5.2f} x, wall {wall_direct / wall_seq:5.2f} x", flush=True)


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# zoom sequences: device {name}, {cus} CUs; shader clock under load {ctx.measure_clock():.0f} MHz; build {B.build_id()}", flush=True)
    print(f"# stage: device forms; HIP events; best of {ROUNDS} rounds after two warm launches, the variants alternating")
    stream = torch.cuda.Stream()
    for W, H in ((1920, 1280), (7680, 5120)):
        stage(ctx, stream, W, H)
    torch.cuda.synchronize()
    sequence(ctx)
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
