"""Distance shading (MC_MANDEL_COLOUR_DISTANCE) measured on one context.

Per view, HIP events, warm launches, best of ROUNDS rounds, the variants alternating:
  - the stencil kernel alone (mc_mandelbrot_distance_device_async: colours only, and colours + D) beside its yardstick,
    mandel_recolour_kernel (mc_mandelbrot_recolour_device_async with the identity map) on the same image's count plane: both read 4 B and
    write 16 B per pixel;
  - the whole chain (the smooth render of the q plane alone, then the stencil) against the smooth call that writes the vec4 plane itself;
  - the blocking calls' own record (mc_context_last_timing of mc_mandelbrot_render_rgba8), distance against smooth;
  - the share of pixels with D < 1, the ones the shading darkens.
Views: K1 (3200 x 2400, M = 1000, fp32), K4 in F64 (7680 x 5120, M = 50 000, 1e-8), deep BLA at M(3,3) 1e-1000 (7680 x 5120, M = 6000).
    On an MI355X:  python tools/mandel_distance_probe.py > profiles/mandel_distance_probe.txt
                   python tools/mandel_distance_probe.py --plain-only    (the plain render alone: run on this build and on the parent's,
                                                                          MC_LIB_PATH, alternating processes on one box)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import mandel_perturb_deep_ref as D  # noqa: E402
import mandel_perturb_ref as R  # noqa: E402

B = entry.load_package().bindings
ROUNDS = 3
ASPECT = 2.0 / 3.0
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))
DISTANCE = getattr(B, "MANDEL_COLOUR_DISTANCE", 0)


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
    """{name: (best ms, worst ms)} over `rounds` rounds alternating the variants (warm launches in the first round)."""
    out = {}
    for r in range(rounds):
        for name, launch in variants:
            ms = event_ms(stream, launch, warm=2 if r == 0 else 0)
            lo, hi = out.get(name, (ms, ms))
            out[name] = (min(lo, ms), max(hi, ms))
    return out


def views():
    c33, m33, e33 = D.view(D.M33, "1e-1000")
    k4 = (float(R.DEEP_CENTRE[0]), float(R.DEEP_CENTRE[1]))
    return [("K1 F32 3200x2400 M1000", 3200, 2400, dict(max_iter=1000, precision=B.PRECISION_F32), None),
            ("K4 F64 7680x5120 M50000 1e-8", 7680, 5120, dict(max_iter=50000, precision=B.PRECISION_F64, centre=k4, scale=(1e-8, 1e-8 * ASPECT)),
             None),
            ("BLA_DEEP M33 1e-1000 7680x5120 M6000", 7680, 5120, dict(max_iter=6000, precision=B.PRECISION_PERTURB_BLA_DEEP, **ZERO),
             lambda: B.Orbit(c33[0], c33[1], m33[0], m33[0] * ASPECT, 6000, e33))]


def main():
    plain_only = "--plain-only" in sys.argv or not DISTANCE
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# {'plain only' if plain_only else 'distance shading'}: device {name}, {cus} CUs; shader clock under load "
          f"{ctx.measure_clock():.0f} MHz; build {B.build_id()}", flush=True)
    print(f"# device forms; HIP events; best of {ROUNDS} rounds after two warm launches, the variants alternating")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    for tag, W, H, kw, make in views():
        o = None
        if make:
            o = make()
            o.bla_deep()
            ctx.bind_mandelbrot_orbit(o)
        M = kw["max_iter"]
        rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        plain = B.mandelbrot_params(W, H, **kw)
        if plain_only:
            t = best_of(stream, [("plain", lambda: ctx.mandelbrot_device(plain, rgba.data_ptr(), 0, stream=s))])
            print(f"{tag}: plain {t['plain'][0]:9.4f} ms (worst {t['plain'][1]:9.4f})", flush=True)
        else:
            smooth = B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_SMOOTH, **kw)
            dist = B.mandelbrot_params(W, H, flags=DISTANCE, **kw)
            d_n = torch.empty((H, W), dtype=torch.int32, device="cuda")
            d_q = torch.empty((H, W), dtype=torch.int32, device="cuda")
            d_D = torch.empty((H, W), dtype=torch.float32, device="cuda")
            ident = np.arange(M + 1, dtype=np.uint32)
            ctx.mandelbrot_smooth_device(smooth, 0, d_n.data_ptr(), d_q.data_ptr(), stream=s)
            stream.synchronize()

            def chain():
                ctx.mandelbrot_smooth_device(smooth, 0, 0, d_q.data_ptr(), stream=s)
                ctx.mandelbrot_distance_device(dist, d_q.data_ptr(), 1.0, 0, rgba.data_ptr(), stream=s)

            t = best_of(stream, [
                ("recolour", lambda: ctx.mandelbrot_recolour_device(plain, d_n.data_ptr(), 4, ident, rgba.data_ptr(), stream=s)),
                ("stencil", lambda: ctx.mandelbrot_distance_device(dist, d_q.data_ptr(), 1.0, 0, rgba.data_ptr(), stream=s)),
                ("stencil+D", lambda: ctx.mandelbrot_distance_device(dist, d_q.data_ptr(), 1.0, d_D.data_ptr(), rgba.data_ptr(), stream=s)),
                ("D only", lambda: ctx.mandelbrot_distance_device(dist, d_q.data_ptr(), 1.0, d_D.data_ptr(), 0, stream=s)),
                ("plain", lambda: ctx.mandelbrot_device(plain, rgba.data_ptr(), 0, stream=s)),
                ("smooth", lambda: ctx.mandelbrot_device(smooth, rgba.data_ptr(), 0, stream=s)),
                ("chain", chain)])
            px = W * H
            print(f"{tag}:", flush=True)
            for k, bytes_px in (("recolour", 20), ("stencil", 20), ("stencil+D", 24), ("D only", 8)):
                print(f"    {k:10s} {t[k][0]:8.4f} ms (worst {t[k][1]:8.4f})   {px * bytes_px / t[k][0] / 1e9:7.2f} TB/s of {bytes_px} B per pixel"
                      f"   {t[k][0] / t['recolour'][0]:5.2f} x recolour")
            d = t["chain"][0] - t["smooth"][0]
            print(f"    plain {t['plain'][0]:9.4f} ms   smooth {t['smooth'][0]:9.4f} ms (worst {t['smooth'][1]:9.4f})   chain {t['chain'][0]:9.4f} ms "
                  f"(worst {t['chain'][1]:9.4f})   chain - smooth {d:8.4f} ms = {d / t['smooth'][0] * 100:6.2f} %", flush=True)
            torch.cuda.synchronize()
            u8s = ctx.mandelbrot_rgba8(smooth)
            ks = ctx.last_timing()[0]
            u8d = ctx.mandelbrot_rgba8(dist)
            kd = ctx.last_timing()[0]
            ks = min(ks, (ctx.mandelbrot_rgba8(smooth), ctx.last_timing()[0])[1])
            kd = min(kd, (ctx.mandelbrot_rgba8(dist), ctx.last_timing()[0])[1])
            Dp = ctx.mandelbrot_distance(dist, want_rgba=False, want_iters=False, want_smooth=False)[3]
            print(f"    mc_mandelbrot_render_rgba8, device time of the blocking call (best of 2): smooth {ks:9.4f} ms   distance {kd:9.4f} ms; "
                  f"pictures differ on {100.0 * (u8s != u8d).any(axis=-1).mean():.2f} % of the pixels")
            print(f"    D < 1 on {100.0 * (Dp < 1).mean():.2f} % of the pixels (D = 0: {100.0 * (Dp == 0).mean():.2f} %), D = 4096 on "
                  f"{100.0 * (Dp == 4096).mean():.2f} %; median D {np.median(Dp):.2f}", flush=True)
        if o is not None:
            ctx.bind_mandelbrot_orbit(None)
            o.close()
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
