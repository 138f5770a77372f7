"""The path-tracer denoiser (mc_pathtrace_guides_*, mc_pathtrace_denoise_*, mc_pathtrace_render_denoised) measured on one context
(DESIGN.md §3.17).

1. The two kernels alone through the device forms at K2's size (900 x 600) and at 3840 x 2560, on a 16-spp strict render of the reference
   scene: the guides call (its scene upload included: the call copies the tables and synchronises before it launches), the filter with
   P = 1 .. 5 passes (separate output) and P = 5 in place, beside a device-to-device copy of one 16-B-per-pixel plane, the floor of a
   plane kernel; the filter is set beside P such copies.  HIP events, warm launches, best of ROUNDS rounds, the variants alternating.
2. Quality against time at K2's size: RMSE over RGB of the final 0 .. 255 buffer against a 4096-spp strict render, and the device time of
   the blocking call (mc_context_last_timing, kernels only), for raw renders at 16 .. 1024 spp and for denoised renders at 16, 32 and 64
   spp, strict and fast math; the split of the error into pixels whose first hit is specular (the mirror and the glass sphere) and the rest.
    On an MI355X:  python tools/pt_denoise_probe.py > profiles/pt_denoise_probe.txt"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

B = entry.load_package().bindings
ROUNDS = 5


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
    out = {}
    for r in range(rounds):
        for name, launch in variants:
            ms = event_ms(stream, launch, warm=2 if r == 0 else 0)
            lo, hi = out.get(name, (ms, ms))
            out[name] = (min(lo, ms), max(hi, ms))
    return out


def stage(ctx, stream, W, H):
    s = stream.cuda_stream
    rgba, nt, pid, out = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    work = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    ctx.pathtrace_device(B.pathtrace_params(W, H, 16), rgba.data_ptr(), stream=s)
    ctx.pathtrace_guides_device(W, H, nt.data_ptr(), pid.data_ptr(), stream=s)
    stream.synchronize()
    variants = [("copy 16 B", lambda: out.copy_(rgba, non_blocking=True)),
                ("guides (upload + kernel)", lambda: ctx.pathtrace_guides_device(W, H, nt.data_ptr(), pid.data_ptr(), stream=s))]
    for P in range(1, 6):
        d = B.pathtrace_denoise_params(W, H, passes=P)
        variants.append((f"filter P={P}", lambda d=d: ctx.pathtrace_denoise_device(d, rgba.data_ptr(), nt.data_ptr(), pid.data_ptr(), out.data_ptr(), stream=s)))
    d5 = B.pathtrace_denoise_params(W, H)
    work.copy_(rgba)
    variants.append(("filter P=5 in place", lambda: ctx.pathtrace_denoise_device(d5, work.data_ptr(), nt.data_ptr(), pid.data_ptr(), work.data_ptr(), stream=s)))
    with torch.cuda.stream(stream):
        t = best_of(stream, variants)
    px = W * H
    copy = t["copy 16 B"][0]
    print(f"{W} x {H} ({px / 1e6:.2f} Mpixel):")
    for name, _ in variants:
        lo, hi = t[name]
        line = f"    {name:26s} {lo:8.4f} ms (worst {hi:8.4f})   {lo * 1e6 / px:7.3f} ns per pixel   {lo / copy:6.2f} x one copy"
        if name.startswith("filter P="):
            P = int(name.split("=")[1].split()[0])
            line += f"   {lo / (P * copy):5.2f} x {P} copies   {px * P * 64 / lo / 1e9:6.2f} TB/s at 64 B per pixel and pass"
        print(line, flush=True)
    steps = [t["filter P=1"][0]] + [t[f"filter P={P}"][0] - t[f"filter P={P - 1}"][0] for P in range(2, 6)]
    print("    per pass (differences), steps 1 2 4 8 16: " + "  ".join(f"{x:7.4f}" for x in steps) + " ms", flush=True)


def rmse(a, b, mask=None):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    if mask is not None:
        d = d[mask]
    return float(np.sqrt((d ** 2).mean()))


def timed(ctx, call, repeats=3):
    best, out = None, None
    for _ in range(repeats):
        out = call()
        k = ctx.last_timing()[0]
        best = k if best is None else min(best, k)
    return out, best


def quality(ctx, W=900, H=600):
    ref = ctx.pathtrace(B.pathtrace_params(W, H, 4096))
    _, pid = B.pathtrace_guides(W, H)
    spec = (pid[..., 3] == 6) | (pid[..., 3] == 7)
    print(f"reference scene, {W} x {H}, RMSE over RGB of the final buffer against 4096 spp strict; device time = kernels of the blocking call, best of 3")
    print(f"    first hit specular (mirror or glass sphere): {int(spec.sum())} of {W * H} pixels ({100 * spec.mean():.2f} %)")
    for mode, name in ((B.PT_MATH_STRICT, "strict"), (B.PT_MATH_FAST, "fast")):
        for spp in (16, 32, 64, 128, 256, 512, 1024):
            p = B.pathtrace_params(W, H, spp, math_mode=mode)
            img, ms = timed(ctx, lambda: ctx.pathtrace(p))
            print(f"    {name:6s} raw      {spp:5d} spp  RMSE {rmse(img, ref):6.2f} (specular {rmse(img, ref, spec):6.2f}, rest {rmse(img, ref, ~spec):6.2f})   "
                  f"{ms:8.3f} ms", flush=True)
        for spp in (16, 32, 64):
            p = B.pathtrace_params(W, H, spp, math_mode=mode)
            img, ms = timed(ctx, lambda: ctx.pathtrace_denoised(p))
            print(f"    {name:6s} denoised {spp:5d} spp  RMSE {rmse(img, ref):6.2f} (specular {rmse(img, ref, spec):6.2f}, rest {rmse(img, ref, ~spec):6.2f})   "
                  f"{ms:8.3f} ms", flush=True)


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# path-tracer denoiser: device {name}, {cus} CUs; shader clock under load {ctx.measure_clock():.0f} MHz; build {B.build_id()}", flush=True)
    print(f"# stage: device forms; HIP events; best of {ROUNDS} rounds after two warm launches, the variants alternating")
    stream = torch.cuda.Stream()
    for W, H in ((900, 600), (3840, 2560)):
        stage(ctx, stream, W, H)
    torch.cuda.synchronize()
    quality(ctx)
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
