"""The noise plane and the noise-guided filter (mc_pathtrace_noise_*, mc_pathtrace_denoise_adaptive_*, mc_pathtrace_render_denoised_adaptive)
measured on one context, by the method of tools/pt_denoise_probe.py.

1. The kernels alone through the device forms at K2's size (900 x 600) and at 3840 x 2560, on a 16-spp strict render of the reference scene
   made in two sample ranges: the noise plane (both kernels) at radius 1, 3 and 4, the noise-guided filter at P = 1 and P = 5 beside the
   fixed filter at the same P in the same process, and a device-to-device copy of one 16-B-per-pixel plane.  HIP events, warm launches,
   best of ROUNDS rounds, the variants alternating.
2. The chain against mc_pathtrace_render_denoised at K2's size and 16, 64 and 256 spp, strict and fast math: the device time of the
   blocking call (mc_context_last_timing, kernels only), which shows the cost of the split render (one more launch tail, one plane copy),
   and at 1024 spp strict; RMSE over RGB of the final 0 .. 255 buffer against a 4096-spp strict render for the raw render, the fixed
   filter and the noise-guided one.
    On an MI355X:  python tools/pt_noise_probe.py > profiles/pt_noise_probe.txt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pt_denoise_probe import B, ROUNDS, best_of, rmse, timed  # noqa: E402


def stage(ctx, stream, W, H, spp=16):
    s = stream.cuda_stream
    rgba, half, nt, pid, out = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(5))
    var = torch.empty((H, W), dtype=torch.float32, device="cuda")
    k, radius = B.pathtrace_noise_defaults()
    with torch.cuda.stream(stream):
        ctx.pathtrace_device(B.pathtrace_params(W, H, spp, sample_end=spp // 2), rgba.data_ptr(), stream=s)
        half.copy_(rgba, non_blocking=True)
        ctx.pathtrace_device(B.pathtrace_params(W, H, spp, sample_begin=spp // 2), rgba.data_ptr(), stream=s)
        ctx.pathtrace_guides_device(W, H, nt.data_ptr(), pid.data_ptr(), stream=s)
        ctx.pathtrace_noise_device(W, H, half.data_ptr(), 2.0, rgba.data_ptr(), radius, var.data_ptr(), stream=s)
    stream.synchronize()
    variants = [("copy 16 B", lambda: out.copy_(rgba, non_blocking=True))]
    for r in (0, 1, 3, 4):
        variants.append((f"noise plane r={r}", lambda r=r: ctx.pathtrace_noise_device(W, H, half.data_ptr(), 2.0, rgba.data_ptr(), r, var.data_ptr(), stream=s)))
    for P in (1, 5):
        d = B.pathtrace_denoise_params(W, H, passes=P)
        variants.append((f"fixed filter P={P}", lambda d=d: ctx.pathtrace_denoise_device(d, rgba.data_ptr(), nt.data_ptr(), pid.data_ptr(), out.data_ptr(), stream=s)))
        variants.append((f"guided filter P={P}", lambda d=d: ctx.pathtrace_denoise_adaptive_device(d, k, rgba.data_ptr(), nt.data_ptr(), pid.data_ptr(),
                                                                                                    var.data_ptr(), out.data_ptr(), stream=s)))
    with torch.cuda.stream(stream):
        t = best_of(stream, variants)
        ctx.pathtrace_noise_device(W, H, half.data_ptr(), 2.0, rgba.data_ptr(), radius, var.data_ptr(), stream=s)   # (the filter rows above ran on r = 4's plane)
    stream.synchronize()
    px = W * H
    copy = t["copy 16 B"][0]
    print(f"{W} x {H} ({px / 1e6:.2f} Mpixel):")
    for name, _ in variants:
        lo, hi = t[name]
        print(f"    {name:22s} {lo:8.4f} ms (worst {hi:8.4f})   {lo * 1e6 / px:7.3f} ns per pixel   {lo / copy:6.2f} x one copy", flush=True)
    for P in (1, 5):
        print(f"    guided / fixed at P={P}: {t[f'guided filter P={P}'][0] / t[f'fixed filter P={P}'][0]:.3f}")
    print(f"    noise plane r={radius} / one fixed pass (P=5 over 5): {t[f'noise plane r={radius}'][0] / (t['fixed filter P=5'][0] / 5):.3f}", flush=True)


def chain(ctx, W=900, H=600):
    ref = ctx.pathtrace(B.pathtrace_params(W, H, 4096))
    print(f"reference scene, {W} x {H}, RMSE over RGB of the final buffer against 4096 spp strict; device time = kernels of the blocking call, best of 3")
    for mode, name, spps in ((B.PT_MATH_STRICT, "strict", (16, 64, 256, 1024)), (B.PT_MATH_FAST, "fast", (16, 64, 256))):
        for spp in spps:
            p = B.pathtrace_params(W, H, spp, math_mode=mode)
            raw, t_raw = timed(ctx, lambda: ctx.pathtrace(p))
            fixed, t_fixed = timed(ctx, lambda: ctx.pathtrace_denoised(p))
            guided, t_guided = timed(ctx, lambda: ctx.pathtrace_denoised_adaptive(p))
            print(f"    {name:6s} {spp:5d} spp  raw RMSE {rmse(raw, ref):6.2f} {t_raw:9.3f} ms   fixed {rmse(fixed, ref):6.2f} {t_fixed:9.3f} ms   "
                  f"noise-guided {rmse(guided, ref):6.2f} {t_guided:9.3f} ms   (guided - fixed {t_guided - t_fixed:+7.3f} ms)", flush=True)


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# noise-guided denoiser: device {name}, {cus} CUs; shader clock under load {ctx.measure_clock():.0f} MHz; build {B.build_id()}", flush=True)
    print(f"# stage: device forms; HIP events; best of {ROUNDS} rounds after two warm launches, the variants alternating")
    stream = torch.cuda.Stream()
    for W, H in ((900, 600), (3840, 2560)):
        stage(ctx, stream, W, H)
    torch.cuda.synchronize()
    chain(ctx)
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
