"""Smooth equalised colouring (MC_MANDEL_COLOUR_SMOOTH_EQUALISED) measured on one context.

Per view, HIP events, warm launches, best of ROUNDS rounds, the variants alternating:
  - the two new kernels alone on the view's own q plane (mc_mandelbrot_smooth_histogram_device_async into a table zeroed once;
    mc_mandelbrot_smooth_remap_device_async writing colours, q', both) beside their yardsticks: a read-only pass over the plane
    (torch.sum of the int32 plane), §3.10's histogram of the count plane, and §3.10's recolour kernel (4 B read, 16 B written);
  - the blocking whole-image calls (mc_mandelbrot_render_rgba8, the device time mc_context_last_timing records: the whole chain, the
    table's round trip and the host map included): plain, smooth, integer equalised, smooth equalised, alternating;
  - what the picture gains: distinct palette positions and the 1st..99th percentile span of q' / (256 M) over the escaped pixels.
Views: K4 in F64 (7680 x 5120, M = 50 000, 1e-8) and deep BLA at M(3,3) 1e-1000 (7680 x 5120, M = 6000).
    On an MI355X:  python tools/mandel_smooth_equalise_probe.py > profiles/mandel_smooth_equalise_probe.txt
                   python tools/mandel_smooth_equalise_probe.py --existing-only   (plain, smooth and integer equalised alone: run on this
                                                                                   build and on the parent's, MC_LIB_PATH, alternating
                                                                                   processes on one box)"""
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
ROUNDS = 5
ASPECT = 2.0 / 3.0
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))
FLAG = getattr(B, "MANDEL_COLOUR_SMOOTH_EQUALISED", 0)


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


def blocking_best(ctx, variants, rounds=ROUNDS):
    """{name: (best ms, worst ms)} of mc_context_last_timing's kernel time over alternating blocking RGBA8 renders (one warm render each)."""
    out = {}
    for r in range(rounds + 1):
        for name, p in variants:
            ctx.mandelbrot_rgba8(p)
            if r == 0:
                continue
            ms = ctx.last_timing()[0]
            lo, hi = out.get(name, (ms, ms))
            out[name] = (min(lo, ms), max(hi, ms))
    return out


def views():
    c33, m33, e33 = D.view(D.M33, "1e-1000")
    k4 = (float(R.DEEP_CENTRE[0]), float(R.DEEP_CENTRE[1]))
    return [("K4 F64 7680x5120 M50000 1e-8", 7680, 5120, dict(max_iter=50000, precision=B.PRECISION_F64, centre=k4, scale=(1e-8, 1e-8 * ASPECT)),
             None),
            ("BLA_DEEP M33 1e-1000 7680x5120 M6000", 7680, 5120, dict(max_iter=6000, precision=B.PRECISION_PERTURB_BLA_DEEP, **ZERO),
             lambda: B.Orbit(c33[0], c33[1], m33[0], m33[0] * ASPECT, 6000, e33))]


def span(t):
    a, b = np.percentile(np.asarray(t, np.float64).reshape(-1), [1, 99])
    return float(b - a)


def main():
    existing_only = "--existing-only" in sys.argv or not FLAG
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# {'existing colourings only' if existing_only else 'smooth equalised colouring'}: device {name}, {cus} CUs; shader clock under "
          f"load {ctx.measure_clock():.0f} MHz; build {B.build_id()}", flush=True)
    print(f"# HIP events; best of {ROUNDS} rounds after warm launches, the variants alternating on one context")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    for tag, W, H, kw, make in views():
        o = None
        if make:
            o = make()
            o.bla_deep()
            ctx.bind_mandelbrot_orbit(o)
        M = kw["max_iter"]
        px = W * H
        plain = B.mandelbrot_params(W, H, **kw)
        smooth = B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_SMOOTH, **kw)
        equalised = B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_EQUALISED, **kw)
        calls = [("plain", plain), ("smooth", smooth), ("equalised", equalised)]
        if not existing_only:
            flagged = B.mandelbrot_params(W, H, flags=FLAG, **kw)
            calls.append(("smooth equalised", flagged))
        t = blocking_best(ctx, calls)
        print(f"{tag}:", flush=True)
        print("    mc_mandelbrot_render_rgba8, device time of the blocking call: " +
              "   ".join(f"{k} {t[k][0]:9.4f} ms (worst {t[k][1]:9.4f})" for k, _ in calls), flush=True)
        if not existing_only:
            d1, d2 = t["smooth equalised"][0] - t["smooth"][0], t["smooth equalised"][0] - t["equalised"][0]
            print(f"    smooth equalised - smooth {d1:8.4f} ms = {100 * d1 / t['smooth'][0]:6.2f} %;   smooth equalised - equalised {d2:8.4f} ms = "
                  f"{100 * d2 / t['equalised'][0]:6.2f} %", flush=True)
            rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
            d_n = torch.empty((H, W), dtype=torch.int32, device="cuda")
            d_q = torch.empty((H, W), dtype=torch.int32, device="cuda")
            d_r = torch.empty((H, W), dtype=torch.int32, device="cuda")
            tab = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
            ctx.mandelbrot_smooth_device(smooth, 0, d_n.data_ptr(), d_q.data_ptr(), stream=s)
            ctx.mandelbrot_smooth_histogram_device(d_q.data_ptr(), px, M, tab.data_ptr(), stream=s)
            stream.synchronize()
            hist = tab.cpu().numpy().view(np.uint32)
            qmap = B.smooth_equalise_map(M, hist)
            ident = np.arange(M + 1, dtype=np.uint32)
            with torch.cuda.stream(stream):
                k = best_of(stream, [
                    ("read-only pass", lambda: d_q.sum()),
                    ("histogram of n", lambda: ctx.mandelbrot_histogram_device(d_n.data_ptr(), 4, px, M, tab.data_ptr(), stream=s)),
                    ("histogram of q >> 8", lambda: ctx.mandelbrot_smooth_histogram_device(d_q.data_ptr(), px, M, tab.data_ptr(), stream=s)),
                    ("recolour", lambda: ctx.mandelbrot_recolour_device(plain, d_n.data_ptr(), 4, ident, rgba.data_ptr(), stream=s)),
                    ("remap, colours", lambda: ctx.mandelbrot_smooth_remap_device(flagged, d_q.data_ptr(), qmap, 0, rgba.data_ptr(), stream=s)),
                    ("remap, q' only", lambda: ctx.mandelbrot_smooth_remap_device(flagged, d_q.data_ptr(), qmap, d_r.data_ptr(), 0, stream=s)),
                    ("remap, both", lambda: ctx.mandelbrot_smooth_remap_device(flagged, d_q.data_ptr(), qmap, d_r.data_ptr(), rgba.data_ptr(),
                                                                               stream=s))])
            for key, bytes_px in (("read-only pass", 4), ("histogram of n", 4), ("histogram of q >> 8", 4), ("recolour", 20), ("remap, colours", 20),
                                  ("remap, q' only", 8), ("remap, both", 24)):
                print(f"    {key:20s} {k[key][0]:8.4f} ms (worst {k[key][1]:8.4f})   {px * bytes_px / k[key][0] / 1e9:7.2f} TB/s of {bytes_px} B per pixel",
                      flush=True)
            torch.cuda.synchronize()
            q = d_q.cpu().numpy().view(np.uint32)
            n = d_n.cpu().numpy().view(np.uint32)
            ctx.mandelbrot_smooth_remap_device(flagged, d_q.data_ptr(), qmap, d_r.data_ptr(), 0)
            ctx.synchronize()
            r = d_r.cpu().numpy().view(np.uint32)
            esc = q < 256 * M
            imap = B.equalise_map(M, np.bincount(np.minimum(n, M).ravel(), minlength=M + 1).astype(np.uint32))
            print(f"    escaped {int(esc.sum())} of {px}, occupied bins {int((hist[:M] > 0).sum())} of {M}; distinct: integer ranks "
                  f"{np.unique(imap[np.minimum(n, M)][esc]).size}, q {np.unique(q[esc]).size}, q' {np.unique(r[esc]).size}; 1st..99th percentile span "
                  f"over the escaped pixels: integer equalised {span(imap[np.minimum(n, M)][esc] / float(M)):.4f}, smooth {span(q[esc] / (256.0 * M)):.4f}, "
                  f"smooth equalised {span(r[esc] / (256.0 * M)):.4f}", flush=True)
        if o is not None:
            ctx.bind_mandelbrot_orbit(None)
            o.close()
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
