"""The area filter of zoom sequences (MC_MANDEL_ZOOM_FILTER_AREA) measured on one context.

The compose stage alone at 1920 x 1280 and 7680 x 5120, M = 2000, on an F64 pair an octave apart in the seahorse valley, at the in-between
steps 1 .. F - 1 of F = 4: the bilinear frame (the unfiltered device calls) and the AREA frame (the filtered device calls), from vec4
keyframes to vec4 and to RGBA8 and from count keyframes in each colouring to RGBA8, beside a plain device-to-device copy of the vec4
plane and of the count plane.  HIP events, warm launches, best of ROUNDS rounds, the variants alternating.

  --unfiltered-only   the unfiltered calls alone: run on this build and on the parent's (MC_LIB_PATH=<the parent's library>), processes
                      alternating, three each; they must agree within the run-to-run spread.
    On an MI355X:  python tools/mandel_zoom_filter_probe.py > profiles/mandel_zoom_filter_probe.txt"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

B = entry.load_package().bindings
ROUNDS = 7
ASPECT = 2.0 / 3.0
M = 2000
F = 4
CENTRE = (-0.7436438870371587, 0.13182590420531198)
SCALES = (0.02, 0.01)
MODES = (("plain", 0), ("equalised", B.MANDEL_COLOUR_EQUALISED), ("smooth", B.MANDEL_COLOUR_SMOOTH),
         ("smooth-equalised", B.MANDEL_COLOUR_SMOOTH_EQUALISED))


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


def params(W, H, scale, flags=0):
    return B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_F64, centre=CENTRE, scale=(scale, scale * ASPECT), flags=flags)


def histogram(plane, shift):
    return np.bincount(np.minimum(plane.reshape(-1).astype(np.int64) >> shift, M), minlength=M + 1).astype(np.uint32)


def stage(ctx, stream, W, H, filtered):
    s = stream.cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    key = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    n = [torch.empty((H, W), **i32) for _ in range(2)]
    q = [torch.empty((H, W), **i32) for _ in range(2)]
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    out8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    spare = torch.empty((H, W), **i32)
    for i, scale in enumerate(SCALES):
        ctx.mandelbrot_device(params(W, H, scale), key[i].data_ptr(), n[i].data_ptr(), stream=s)
        ctx.mandelbrot_smooth_device(params(W, H, scale, B.MANDEL_COLOUR_SMOOTH), 0, 0, q[i].data_ptr(), stream=s)
    stream.synchronize()
    hn = [histogram(a.cpu().numpy().view(np.uint32), 0) for a in n]
    hq = [histogram(a.cpu().numpy().view(np.uint32), 8) for a in q]
    rank = [B.equalise_map(M, h) for h in hn]
    knots = [B.smooth_equalise_map(M, h) for h in hq]
    w, d, o, o8 = key[0].data_ptr(), key[1].data_ptr(), out.data_ptr(), out8.data_ptr()
    variants = [("copy of the vec4 plane (16 B / pixel)", lambda: out.copy_(key[0])),
                ("copy of the count plane (4 B / pixel)", lambda: spare.copy_(n[0]))]
    rows = []
    for step in range(1, F):
        r = B.zoom_ratio(step, F)
        tables = {"plain": (n, None), "equalised": (n, B.zoom_blend_map(rank[0], rank[1], step, F)), "smooth": (q, None),
                  "smooth-equalised": (q, B.zoom_blend_map(knots[0], knots[1], step, F))}
        for form, f, b in (("vec4 ", o, 0), ("rgba8", 0, o8)):
            name = f"step {step}/{F} vec4 keyframes          -> {form}"
            variants.append((name + " bilinear", lambda r=r, f=f, b=b: ctx.zoom_compose_device(W, H, w, d, r, f, b, stream=s)))
            if filtered:
                variants.append((name + " area", lambda r=r, f=f, b=b: ctx.zoom_compose_filtered_device(W, H, w, d, r, B.ZOOM_FILTER_AREA, f, b, stream=s)))
            rows.append(name)
        for mode, flag in MODES:
            p = params(W, H, SCALES[0], flag)
            pl, table = tables[mode]
            name = f"step {step}/{F} counts {mode:16s} -> rgba8"
            variants.append((name + " bilinear", lambda r=r, p=p, pl=pl, table=table: ctx.zoom_compose_counts_device(
                p, pl[0].data_ptr(), pl[1].data_ptr(), table, r, 0, o8, stream=s)))
            if filtered:
                variants.append((name + " area", lambda r=r, p=p, pl=pl, table=table: ctx.zoom_compose_counts_filtered_device(
                    p, pl[0].data_ptr(), pl[1].data_ptr(), table, r, B.ZOOM_FILTER_AREA, 0, o8, stream=s)))
            rows.append(name)
    with torch.cuda.stream(stream):
        t = best_of(stream, variants)
    print(f"{W} x {H}, M = {M}:")
    for name in [v[0] for v in variants[:2]]:
        print(f"    {name:52s} {t[name][0]:8.4f} ms (worst {t[name][1]:8.4f})", flush=True)
    for name in rows:
        lo, hi = t[name + " bilinear"]
        line = f"    {name:52s} bilinear {lo:8.4f} ms (worst {hi:8.4f})"
        if filtered:
            alo, ahi = t[name + " area"]
            line += f"   area {alo:8.4f} ms (worst {ahi:8.4f})   {alo / lo:5.2f} x"
        print(line, flush=True)


def main():
    filtered = "--unfiltered-only" not in sys.argv[1:]
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# the area filter of zoom sequences: device {name}, {cus} CUs; shader clock under load {ctx.measure_clock():.0f} MHz; "
          f"library {os.environ.get('MC_LIB_PATH', 'this build')}; build {B.build_id()}", flush=True)
    print(f"# stage: device forms; HIP events; best of {ROUNDS} rounds after two warm launches, the variants alternating"
          + ("" if filtered else "; the unfiltered calls alone"))
    stream = torch.cuda.Stream()
    for W, H in ((1920, 1280), (7680, 5120)):
        stage(ctx, stream, W, H, filtered)
        torch.cuda.synchronize()
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
