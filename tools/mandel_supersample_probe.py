"""s x s supersampling (MC_MANDEL_SUPERSAMPLE) measured at K4 geometry, 7680 x 5120, on one context.

1. The resolve kernel alone, s = 2 and 4, uint16_t and uint32_t sample planes of K4's F64 view (the library's own plain render of the
   sample grid), against the floor: a plain 16-B-per-lane read-only pass over the SAME plane (tools/mandel_equalise_probe.hip) timed in
   the same rounds.  Per case: time, bytes read + written per second, the multiple of the floor.
2. The whole call: mc_mandelbrot_render_rgba8(W, H, s) (mc_context_last_timing's kernel time: first launch to the end of the RGBA8
   conversion) against the plain count-only render of the sample grid (mc_mandelbrot_render_device_async, HIP events) on the same build
   and context, alternating: F64 at K4's 1e-8 view and deep BLA at M33 1e-1000, s = 2 and 4, plain and equalised.  The difference is what
   the feature adds to the render of its samples: the resolve, the conversion of W x H pixels, and for the equalised colouring the
   histogram of s * s as many samples and the table's round trip.
3. --plain-only: the plain (s = 0) mc_mandelbrot_render_rgba8 alone — run on this build and on the parent's (MC_LIB_PATH), processes
   alternating, for the no-regression record.
All times: HIP events, warm launches, best of ROUNDS rounds alternating the variants; the box clock (mc_context_measure_clock) beside them.
    On an MI355X:  python tools/mandel_supersample_probe.py > profiles/mandel_supersample_probe.txt
                   python tools/mandel_supersample_probe.py --plain-only >> profiles/mandel_supersample_probe.txt"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mandel_equalise_probe as P  # noqa: E402  (helper(), event timing, the two views)
import mandel_supersample_ref as S  # noqa: E402

B = P.B
W, H, NPIX, ROUNDS = P.W, P.H, P.NPIX, P.ROUNDS


def resolve_section(ctx, stream, Hp, cus):
    s_ = stream.cuda_stream
    blocks = cus * 8
    sink = torch.zeros(blocks, dtype=torch.int32, device="cuda")
    tag, kw, _ = P.render_views()[0]
    M = kw["max_iter"]
    lut = B.colour_lut(M)
    print(f"## 1. the resolve kernel alone on the sample planes of {tag} (floor = the read-only pass of tools/mandel_equalise_probe.hip over "
          "the same plane, same rounds); bytes = counts read + 16 B per pixel written")
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    for s in (2, 4):
        p = B.mandelbrot_params(W, H, supersample=s, **kw)
        q = B.supersample_params(p)
        for nbytes in (2, 4):
            plane = torch.empty((H * s, W * s), dtype=torch.int16 if nbytes == 2 else torch.int32, device="cuda")
            q.flags = (q.flags & ~B.MANDEL_ITERS_U16) | (B.MANDEL_ITERS_U16 if nbytes == 2 else 0)
            ctx.mandelbrot_device(q, 0, plane.data_ptr(), stream=s_)
            stream.synchronize()
            size = plane.numel() * nbytes
            t = P.best_of(stream, [("floor", lambda: Hp.probe_read_pass(plane.data_ptr(), size, sink.data_ptr(), blocks, s_)),
                                   ("resolve", lambda: ctx.mandelbrot_resolve_device(p, plane.data_ptr(), nbytes, None, rgba.data_ptr(), stream=s_))])
            stream.synchronize()
            rows = [0, 2560, H - 1]   # spot check against the restatement
            host = plane.cpu().numpy().view(np.uint16 if nbytes == 2 else np.uint32)
            got = rgba.cpu().numpy()
            ok = all(np.array_equal(got[r].view(np.uint32), S.resolve(host[r * s:(r + 1) * s], s, M, lut)[0].view(np.uint32)) for r in rows)
            mixed = np.mean([S.mixed_share(host[r * s:(r + 1) * s], s)[0] for r in rows])
            moved = size + NPIX * 16
            print(f"s = {s}, uint{8 * nbytes}_t: plane {size / 1e6:7.1f} MB, mixed pixels in the checked rows {100 * mixed:4.1f} %, == restatement: {ok}")
            print(f"    floor  : best {t['floor'][0]:8.4f} ms (worst {t['floor'][1]:8.4f})  {size / t['floor'][0] / 1e6:8.1f} GB/s read")
            print(f"    resolve: best {t['resolve'][0]:8.4f} ms (worst {t['resolve'][1]:8.4f})  {moved / t['resolve'][0] / 1e6:8.1f} GB/s read + written  "
                  f"{t['resolve'][0] / t['floor'][0]:6.2f} x floor", flush=True)
            del plane


def whole_section(ctx, stream):
    s_ = stream.cuda_stream
    print("## 2. whole call: mc_mandelbrot_render_rgba8 with MC_MANDEL_SUPERSAMPLE(s) (mc_context_last_timing kernel ms) against the plain "
          f"count-only render of its sample grid (uint16_t plane, HIP events), alternating, best of {ROUNDS} rounds after a warm one")
    for tag, kw, make in P.render_views():
        o = None
        if make:
            o = make()
            o.bla_deep()
            ctx.bind_mandelbrot_orbit(o)
        for s in (2, 4):
            p = B.mandelbrot_params(W, H, supersample=s, **kw)
            pe = B.mandelbrot_params(W, H, supersample=s, flags=B.MANDEL_COLOUR_EQUALISED, **kw)
            q = B.supersample_params(p)
            q.flags |= B.MANDEL_ITERS_U16
            plane = torch.empty((H * s, W * s), dtype=torch.int16, device="cuda")
            variants = [("samples", None), ("plain", p), ("equalised", pe)]
            best = {}
            for r in range(ROUNDS + 1):   # round 0 is the warm one; every round starts one variant later, so each follows each
                for name, which in variants[r % 3:] + variants[:r % 3]:
                    if which is None:
                        v = P.event_ms(stream, lambda: ctx.mandelbrot_device(q, 0, plane.data_ptr(), stream=s_), warm=0)
                    else:
                        ctx.mandelbrot_rgba8(which)
                        v = ctx.last_timing()[0]
                    if r:
                        lo, hi = best.get(name, (v, v))
                        best[name] = (min(lo, v), max(hi, v))
            base = best["samples"][0]
            print(f"{tag}, s = {s}: sample grid's counts {base:9.3f} ms (worst {best['samples'][1]:9.3f})")
            for name in ("plain", "equalised"):
                d = best[name][0] - base
                print(f"    {name:9s}: {best[name][0]:9.3f} ms (worst {best[name][1]:9.3f})   over the samples' render {d:7.3f} ms = {100 * d / base:6.2f} %",
                      flush=True)
            del plane
        if o is not None:
            ctx.bind_mandelbrot_orbit(None)
            o.close()


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# {' '.join(sys.argv[1:]) or 'resolve + whole call'}: K4 geometry {W} x {H}; device {name}, {cus} CUs; shader clock under load "
          f"{ctx.measure_clock():.0f} MHz; build {B.build_id()}", flush=True)
    stream = torch.cuda.Stream()
    if "--plain-only" in sys.argv:
        P.render_section(ctx, stream, plain_only=True)
    else:
        resolve_section(ctx, stream, P.helper(), cus)
        whole_section(ctx, stream)
        print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
