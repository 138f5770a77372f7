"""Smooth supersampling (MC_MANDEL_SUPERSAMPLE_SMOOTH) measured at K4 geometry, 7680 x 5120, on one context.

1. The resolve over fractional counts alone, s = 2 and 4, both forms, on the smooth sample planes of K4's F64 1e-8 view (the library's own
   smooth render of the sample grid), beside the integer resolve (mc_mandelbrot_resolve_device_async) on a uint32_t count plane of the same
   size and beside the floor: the plain 16-B-per-lane read-only pass over the same plane (tools/mandel_equalise_probe.hip), all in the same
   rounds.  Per case: time, bytes read + written per second, the multiple of the floor.
2. The whole call: mc_mandelbrot_render_rgba8(W, H, s) with the bit (mc_context_last_timing's kernel time), both colourings, against the
   smooth count-only render of its sample grid (mc_mandelbrot_render_smooth_device_async, q plane only, HIP events), alternating.
3. --existing-only: the plain, smooth and smooth-equalised mc_mandelbrot_render_rgba8 alone, whose kernels this feature leaves as they
   were — run on this build and on the parent's (MC_LIB_PATH), processes alternating, for the no-regression record.
All times: HIP events, warm launches, best of ROUNDS rounds alternating the variants; the box clock (mc_context_measure_clock) beside them.
No hardware counters are collected.
    On an MI355X:  python tools/mandel_smooth_supersample_probe.py > profiles/mandel_smooth_supersample_probe.txt
                   python tools/mandel_smooth_supersample_probe.py --existing-only >> profiles/mandel_smooth_supersample_probe.txt"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mandel_equalise_probe as P  # noqa: E402  (helper(), event timing, the views)

B = P.B
W, H, NPIX = P.W, P.H, P.NPIX
ROUNDS = 5


def flagged(s, ranked, **kw):
    colour = B.MANDEL_COLOUR_SMOOTH_EQUALISED if ranked else B.MANDEL_COLOUR_SMOOTH
    return B.mandelbrot_params(W, H, flags=colour, supersample=s, smooth_samples=True, **kw)


def resolve_section(ctx, stream, Hp, cus):
    s_ = stream.cuda_stream
    blocks = cus * 8
    sink = torch.zeros(blocks, dtype=torch.int32, device="cuda")
    tag, kw, _ = P.render_views()[0]
    M = kw["max_iter"]
    print(f"## 1. the resolves alone on the sample planes of {tag} (floor = the read-only pass of tools/mandel_equalise_probe.hip over the "
          f"smooth plane, same rounds, best of {ROUNDS}); bytes = 4 B per sample read + 16 B per pixel written")
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    hist = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    for s in (2, 4):
        p, pr, pi = flagged(s, False, **kw), flagged(s, True, **kw), B.mandelbrot_params(W, H, supersample=s, **kw)
        g = B.supersample_params(p)
        q = torch.empty((H * s, W * s), dtype=torch.int32, device="cuda")
        ctx.mandelbrot_smooth_device(g, 0, 0, q.data_ptr(), stream=s_)
        n = torch.empty((H * s, W * s), dtype=torch.int32, device="cuda")
        ctx.mandelbrot_device(B.supersample_params(pi), 0, n.data_ptr(), stream=s_)
        hist.zero_()
        ctx.mandelbrot_smooth_histogram_device(q.data_ptr(), q.numel(), M, hist.data_ptr(), stream=s_)
        stream.synchronize()
        qmap = B.smooth_equalise_map(M, hist.cpu().numpy().view(np.uint32))
        size = q.numel() * 4
        t = P.best_of(stream, [("floor", lambda: Hp.probe_read_pass(q.data_ptr(), size, sink.data_ptr(), blocks, s_)),
                               ("integer", lambda: ctx.mandelbrot_resolve_device(pi, n.data_ptr(), 4, None, rgba.data_ptr(), stream=s_)),
                               ("smooth", lambda: ctx.mandelbrot_resolve_smooth_device(p, q.data_ptr(), None, rgba.data_ptr(), stream=s_)),
                               ("ranked", lambda: ctx.mandelbrot_resolve_smooth_device(pr, q.data_ptr(), qmap, rgba.data_ptr(), stream=s_))],
                      rounds=ROUNDS)
        stream.synchronize()
        rows = [0, 2560, H - 1]   # spot check of the last variant (ranked) against the host call
        got = rgba.cpu().numpy()
        ok = all(np.array_equal(got[r].view(np.uint32), B.resolve_smooth(M, s, q[r * s:(r + 1) * s].cpu().numpy().view(np.uint32), qmap)[0].view(np.uint32))
                 for r in rows)
        moved = size + NPIX * 16
        print(f"s = {s}: plane {size / 1e6:7.1f} MB, ranked == host call in the checked rows: {ok}")
        print(f"    floor  : best {t['floor'][0]:8.4f} ms (worst {t['floor'][1]:8.4f})  {size / t['floor'][0] / 1e6:8.1f} GB/s read")
        for name in ("integer", "smooth", "ranked"):
            print(f"    {name:7s}: best {t[name][0]:8.4f} ms (worst {t[name][1]:8.4f})  {moved / t[name][0] / 1e6:8.1f} GB/s read + written  "
                  f"{t[name][0] / t['floor'][0]:6.2f} x floor  {t[name][0] / t['integer'][0]:5.2f} x integer", flush=True)
        del q, n


def whole_section(ctx, stream):
    s_ = stream.cuda_stream
    tag, kw, _ = P.render_views()[0]
    print("## 2. whole call: mc_mandelbrot_render_rgba8 with MC_MANDEL_SUPERSAMPLE_SMOOTH (mc_context_last_timing kernel ms) against the smooth "
          f"count-only render of its sample grid (q plane only, HIP events), alternating, best of {ROUNDS} rounds after a warm one")
    for s in (2, 4):
        p, pr = flagged(s, False, **kw), flagged(s, True, **kw)
        g = B.supersample_params(p)
        q = torch.empty((H * s, W * s), dtype=torch.int32, device="cuda")
        variants = [("samples", None), ("smooth", p), ("ranked", pr)]
        best = {}
        for r in range(ROUNDS + 1):   # round 0 is the warm one; every round starts one variant later, so each follows each
            for name, which in variants[r % 3:] + variants[:r % 3]:
                if which is None:
                    v = P.event_ms(stream, lambda: ctx.mandelbrot_smooth_device(g, 0, 0, q.data_ptr(), stream=s_), warm=0)
                else:
                    ctx.mandelbrot_rgba8(which)
                    v = ctx.last_timing()[0]
                if r:
                    lo, hi = best.get(name, (v, v))
                    best[name] = (min(lo, v), max(hi, v))
        base = best["samples"][0]
        print(f"{tag}, s = {s}: sample grid's smooth counts {base:9.3f} ms (worst {best['samples'][1]:9.3f})")
        for name in ("smooth", "ranked"):
            d = best[name][0] - base
            print(f"    {name:7s}: {best[name][0]:9.3f} ms (worst {best[name][1]:9.3f})   over the samples' render {d:7.3f} ms = {100 * d / base:6.2f} %",
                  flush=True)
        del q


def existing_section(ctx):
    tag, kw, _ = P.render_views()[0]
    print(f"## 3. {tag}, whole image: mc_mandelbrot_render_rgba8 (mc_context_last_timing kernel ms), best of {ROUNDS} rounds after a warm one")
    calls = [("plain", B.mandelbrot_params(W, H, **kw)), ("smooth", B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_SMOOTH, **kw)),
             ("smooth-equalised", B.mandelbrot_params(W, H, flags=B.MANDEL_COLOUR_SMOOTH_EQUALISED, **kw))]
    best = {}
    for r in range(ROUNDS + 1):
        for name, p in calls:
            ctx.mandelbrot_rgba8(p)
            v = ctx.last_timing()[0]
            if r:
                lo, hi = best.get(name, (v, v))
                best[name] = (min(lo, v), max(hi, v))
    print("   ".join(f"{name} {best[name][0]:9.3f} ms (worst {best[name][1]:9.3f})" for name, _ in calls), flush=True)


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# {' '.join(sys.argv[1:]) or 'resolve + whole call'}: K4 geometry {W} x {H}; device {name}, {cus} CUs; shader clock under load "
          f"{ctx.measure_clock():.0f} MHz; build {B.build_id()}; no hardware counters collected", flush=True)
    stream = torch.cuda.Stream()
    if "--existing-only" in sys.argv:
        existing_section(ctx)
    else:
        resolve_section(ctx, stream, P.helper(), cus)
        whole_section(ctx, stream)
        print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
