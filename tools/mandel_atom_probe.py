"""Atom domains measured on one context: the atom render against the plain render of the same view, and the domains'
launches against a device copy of the plane.

One process, HIP events, warm launches, best of ROUNDS rounds alternating the variants; the plain kernels (unchanged by the atom
instantiations: `make asm` gives them their old bodies) are the yardstick in the same process.
 - render: mc_mandelbrot_render_device_async writing the count plane only against mc_mandelbrot_render_atom_device_async writing n,
   period and amin, on K1 (3200 x 2400, M = 1000, F32), K4's view in F64 (1920 x 1280, M = 50 000) and PERTURB at K4's centre, 1e-30
   (1920 x 1280, M = 20 000).
 - domains: mc_mandelbrot_atom_domains_device_async (the table initialisation, the histogram, the 64-bit min pass, the index pass) at
   7680 x 5120 on a plane of one period, on K4's rendered period plane tiled to that size and on a plane of random periods, against a
   device-to-device copy of the period plane.
    On an MI355X:  python tools/mandel_atom_probe.py > profiles/mandel_atom_probe.txt"""
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
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))


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
    """{name: (best ms, worst ms)} over `rounds` rounds alternating the variants (one warm launch each in the first round)."""
    out = {}
    for r in range(rounds):
        for name, launch in variants:
            ms = event_ms(stream, launch, warm=1 if r == 0 else 0)
            lo, hi = out.get(name, (ms, ms))
            out[name] = (min(lo, ms), max(hi, ms))
    return out


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# device {name}, {cus} CUs; shader clock under load {ctx.measure_clock():.0f} MHz; build {B.build_id()}", flush=True)
    print(f"# HIP events on one stream; best (worst) of {ROUNDS} rounds alternating the variants, one warm launch each")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    k4 = (float(R.DEEP_CENTRE[0]), float(R.DEEP_CENTRE[1]))
    views = [("K1 F32 3200x2400 M1000", 3200, 2400, dict(max_iter=1000, precision=B.PRECISION_F32), None),
             ("K4 F64 1920x1280 M50000 1e-8", 1920, 1280, dict(max_iter=50000, precision=B.PRECISION_F64, centre=k4, scale=(1e-8, 1e-8 * ASPECT)), None),
             ("PERTURB K4 centre 1e-30 1920x1280 M20000", 1920, 1280, dict(max_iter=20000, precision=B.PRECISION_PERTURB, **ZERO),
              lambda: B.Orbit(R.DEEP_CENTRE[0], R.DEEP_CENTRE[1], 1e-30, 1e-30 * ASPECT, 20000))]
    k4_period = None
    for tag, W, H, kw, make in views:
        o = make() if make else None
        if o is not None:
            ctx.bind_mandelbrot_orbit(o)
        d_n = torch.empty((H, W), dtype=torch.int32, device="cuda")
        d_p = torch.empty((H, W), dtype=torch.int32, device="cuda")
        d_a = torch.empty((H, W), dtype=torch.float64, device="cuda")
        p = B.mandelbrot_params(W, H, **kw)
        t = best_of(stream, [("plain", lambda: ctx.mandelbrot_device(p, 0, d_n.data_ptr(), stream=s)),
                             ("atom", lambda: ctx.mandelbrot_atom_device(p, d_n.data_ptr(), d_p.data_ptr(), d_a.data_ptr(), stream=s))])
        per = d_p.cpu().numpy().view(np.uint32)
        print(f"{tag}: plain {t['plain'][0]:9.4f} ms (worst {t['plain'][1]:9.4f})   atom {t['atom'][0]:9.4f} ms (worst {t['atom'][1]:9.4f})   "
              f"ratio {t['atom'][0] / t['plain'][0]:6.2f}; {np.unique(per).size} distinct periods", flush=True)
        if tag.startswith("K4"):
            k4_period, k4_amin, k4_M = per.copy(), d_a.cpu().numpy().copy(), kw["max_iter"]
        if o is not None:
            ctx.bind_mandelbrot_orbit(None)
            o.close()
    W, H = 7680, 5120
    rng = np.random.default_rng(3)
    planes = [("one period", np.full((H, W), 78, np.uint32), rng.random((H, W)), 3000),
              ("K4's period plane, tiled", np.tile(k4_period, (4, 4)), np.tile(k4_amin, (4, 4)), k4_M),
              ("random periods in [0, 3000]", rng.integers(0, 3001, (H, W)).astype(np.uint32), rng.random((H, W)), 3000)]
    for tag, per, am, M in planes:
        d_p = torch.from_numpy(per.view(np.int32)).cuda()
        d_a = torch.from_numpy(am).cuda()
        d_copy = torch.empty_like(d_p)
        cnt = torch.empty(M + 1, dtype=torch.int32, device="cuda")
        tab = torch.empty(M + 1, dtype=torch.float64, device="cuda")
        pix = torch.empty(M + 1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            t = best_of(stream, [("copy", lambda: d_copy.copy_(d_p)),
                                 ("domains", lambda: ctx.mandelbrot_atom_domains_device(d_p.data_ptr(), d_a.data_ptr(), d_p.numel(), M, cnt.data_ptr(),
                                                                                       tab.data_ptr(), pix.data_ptr(), stream=s))])
        stream.synchronize()
        used = int((cnt.cpu().numpy().view(np.uint32) > 0).sum())
        print(f"domains {W}x{H}, {tag} (M = {M}, {used} periods in use): copy {t['copy'][0]:8.4f} ms (worst {t['copy'][1]:8.4f})   "
              f"domains {t['domains'][0]:8.4f} ms (worst {t['domains'][1]:8.4f})   ratio {t['domains'][0] / t['copy'][0]:6.2f}", flush=True)
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
