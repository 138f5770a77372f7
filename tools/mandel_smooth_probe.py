"""Smooth colouring (MC_MANDEL_COLOUR_SMOOTH) measured against the plain colouring on one context.

Per view, mc_mandelbrot_render_device_async writing the vec4 plane only, plain and smooth alternating on one context, HIP events, warm
launches, best of ROUNDS rounds; the overhead in ms and as a share of the plain render; how the smooth plane looks (distinct values,
pixels that hit the continuation's cap).  Views: K1 (3200 x 2400, M = 1000, fp32), K4 in F64 (7680 x 5120, M = 50 000, 1e-8), deep BLA
at M(3,3) 1e-1000 (7680 x 5120, M = 6000), and the two kernels whose smooth instantiation runs at 4 waves per SIMD: PERTURB at K4's
centre, 1e-20 (7680 x 5120, M = 20 000) and PERTURB on the deep orbit at M(3,3) 1e-1000 (the rescaled loop, same size, M = 6000).
    On an MI355X:  python tools/mandel_smooth_probe.py > profiles/mandel_smooth_probe.txt
                   python tools/mandel_smooth_probe.py --plain-only    (the plain render alone: run on this build and on the parent's,
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
SMOOTH = getattr(B, "MANDEL_COLOUR_SMOOTH", 0)


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
             lambda: B.Orbit(c33[0], c33[1], m33[0], m33[0] * ASPECT, 6000, e33)),
            ("PERTURB K4 centre 1e-20 7680x5120 M20000", 7680, 5120, dict(max_iter=20000, precision=B.PRECISION_PERTURB, **ZERO),
             lambda: B.Orbit(R.DEEP_CENTRE[0], R.DEEP_CENTRE[1], 1e-20, 1e-20 * ASPECT, 20000)),
            ("PERTURB (deep kernel) M33 1e-1000 7680x5120 M6000", 7680, 5120, dict(max_iter=6000, precision=B.PRECISION_PERTURB, **ZERO),
             lambda: B.Orbit(c33[0], c33[1], m33[0], m33[0] * ASPECT, 6000, e33))]


def main():
    plain_only = "--plain-only" in sys.argv or not SMOOTH
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# {'plain only' if plain_only else 'plain and smooth alternating'}: device {name}, {cus} CUs; shader clock under load "
          f"{ctx.measure_clock():.0f} MHz; build {B.build_id()}", flush=True)
    print(f"# mc_mandelbrot_render_device_async, vec4 plane only; HIP events; best of {ROUNDS} rounds after two warm launches")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    for tag, W, H, kw, make in views():
        o = None
        if make:
            o = make()
            if kw["precision"] == B.PRECISION_PERTURB_BLA_DEEP:
                o.bla_deep()
            ctx.bind_mandelbrot_orbit(o)
        rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        plain = B.mandelbrot_params(W, H, **kw)
        variants = [("plain", lambda: ctx.mandelbrot_device(plain, rgba.data_ptr(), 0, stream=s))]
        if not plain_only:
            smooth = B.mandelbrot_params(W, H, flags=SMOOTH, **kw)
            variants.append(("smooth", lambda: ctx.mandelbrot_device(smooth, rgba.data_ptr(), 0, stream=s)))
        t = best_of(stream, variants)
        line = f"{tag}: plain {t['plain'][0]:9.4f} ms (worst {t['plain'][1]:9.4f})"
        if not plain_only:
            d = t["smooth"][0] - t["plain"][0]
            line += f"   smooth {t['smooth'][0]:9.4f} ms (worst {t['smooth'][1]:9.4f})   overhead {d:8.4f} ms = {d / t['plain'][0] * 100:6.2f} %"
        print(line, flush=True)
        if not plain_only:
            d_n = torch.empty((H, W), dtype=torch.int32, device="cuda")
            d_q = torch.empty((H, W), dtype=torch.int32, device="cuda")
            ctx.mandelbrot_smooth_device(smooth, 0, d_n.data_ptr(), d_q.data_ptr(), stream=s)
            stream.synchronize()
            n, q = d_n.cpu().numpy().view(np.uint32), d_q.cpu().numpy().view(np.uint32)
            M = kw["max_iter"]
            esc = n < M
            k = (q[esc] >> 8).astype(np.int64) - n[esc]
            capped = (q[esc].astype(np.int64) == 256 * (n[esc].astype(np.int64) + 64) + 256)
            print(f"    escaped {int(esc.sum())} of {n.size}; distinct n {np.unique(n[esc]).size}, distinct q {np.unique(q[esc]).size}; "
                  f"continuation iterations (from q >> 8): median {int(np.median(k))}, 95th percentile {int(np.percentile(k, 95))}; "
                  f"hit the cap: {int(capped.sum())} ({capped.mean() * 100:.4f} %)", flush=True)
        if o is not None:
            ctx.bind_mandelbrot_orbit(None)
            o.close()
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
