"""Perturbation (MC_PRECISION_PERTURB) against native fp64 (MC_PRECISION_F64) and two-float (MC_PRECISION_DS) at K4 geometry, 7680 x 5120.

1. On the K4 view at scale 1e-8, M = 50 000, where F64 is still fine, the three precisions alternate on one context (ROUNDS rounds): the
   like-for-like cost.  Per render the kernel time (HIP events around the device-buffer form, after two warm launches, best of REPS x
   LAUNCHES) and reference-equivalent pixel-iterations per second (sum of min(n + 1, M)), plus the share of pixels where PERTURB's n
   differs from F64's.
2. PERTURB alone at 1e-20 and 1e-50 around boundary points (a spread of counts) and at 1e-200 on an interior view: the same figures,
   the host time of the reference orbit, its length L and escape margin, and how many sampled pixels equal direct high-precision
   iteration.
    On an MI355X:  python tools/mandel_perturb_probe.py > profiles/perturb_mandel_probe.txt"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import mandel_perturb_ref as R  # noqa: E402

B = entry.load_package().bindings
W, H, M = 7680, 5120, 50000
CENTRE = ("-0.7436438870371587", "0.13182590420531198")   # bench.K4_VIEW
ASPECT = 2.0 / 3.0
REPS, LAUNCHES, ROUNDS = 3, 4, 3
SAMPLES = 24
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))


def timed(ctx, p, it, stream):
    for _ in range(2):
        ctx.mandelbrot_device(p, 0, it.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    best = None
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(LAUNCHES):
            ctx.mandelbrot_device(p, 0, it.data_ptr(), stream=stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1) / LAUNCHES
        best = ms if best is None else min(best, ms)
    return best, it.cpu().numpy().astype(np.uint32)


def line(tag, ms, n, max_iter):
    pi = int(np.minimum(n.astype(np.int64) + 1, max_iter).sum())
    interior = (n == max_iter).mean() * 100
    return f"{tag}: kernel {ms:9.3f} ms  pixel-iters {pi:.4e}  {pi / (ms * 1e-3):.3e} pixel-iters/s  interior {interior:5.2f} %  " \
           f"distinct n {len(np.unique(n))}"


def main():
    print(f"# K4 geometry {W} x {H}; kernel ms = HIP events, best of {REPS} x {LAUNCHES} launches after 2 warm")
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# device {name}, {cus} CUs, sclk {ctx.measure_clock():.0f} MHz")
    stream = torch.cuda.Stream()
    it = torch.empty((H, W), dtype=torch.int32, device="cuda")
    sc = (1e-8, 1e-8 * ASPECT)
    t = time.time()
    orbit = B.Orbit(CENTRE[0], CENTRE[1], sc[0], sc[1], M)
    print(f"# K4 view 1e-8, M = {M}: orbit L = {orbit.length}, {orbit.bits} bits, {time.time() - t:.3f} s on the host")
    ctx.bind_mandelbrot_orbit(orbit)
    params = {"F64": B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_F64, centre=tuple(map(float, CENTRE)), scale=sc),
              "DS": B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_DS, centre=tuple(map(float, CENTRE)), scale=sc),
              "PERTURB": B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB, **ZERO)}
    best, planes = {}, {}
    for r in range(ROUNDS):
        for tag, p in params.items():
            ms, n = timed(ctx, p, it, stream)
            planes[tag] = n
            best[tag] = ms if tag not in best else min(best[tag], ms)
            print(f"round {r} " + line(f"{tag:7s}", ms, n, M), flush=True)
    for tag in params:
        print("best    " + line(f"{tag:7s}", best[tag], planes[tag], M))
    print(f"PERTURB / F64 kernel time: {best['PERTURB'] / best['F64']:.2f}x;  pixels whose n differs from F64's: "
          f"{(planes['PERTURB'] != planes['F64']).mean() * 100:.2f} %", flush=True)
    # Deep views.  1e-20 and 1e-50: boundary points (mp_boundary_point), stepped outward until their own escape clears |z|^2 = 2 by
    # 1e-6 — a reference on that hair is the method's known failure.  1e-200: an interior centre (main cardioid): along the segment used
    # above no point 1e-200 from the boundary clears the hair within M <= 80 000, so this line is the rate of the all-interior loop, a
    # correct view but not a spread of counts.  Each line checks SAMPLES pixels of the GPU plane against direct high-precision iteration.
    rng = np.random.default_rng(11)
    for scale, m, centre_of in ((1e-20, 20000, lambda: R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 20000, 70, 134)),
                                (1e-50, 20000, lambda: R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 20000, 172, 236)),
                                (1e-200, 20000, lambda: ("-0.1", "0.2"))):
        t = time.time()
        centre = centre_of()
        tb = time.time() - t
        sc = (scale, scale * ASPECT)
        t = time.time()
        with B.Orbit(centre[0], centre[1], sc[0], sc[1], m) as o:
            to = time.time() - t
            ctx.bind_mandelbrot_orbit(o)
            bits = o.bits
            L = o.length
        p = B.mandelbrot_params(W, H, max_iter=m, precision=B.PRECISION_PERTURB, **ZERO)
        ms, n = timed(ctx, p, it, stream)
        _, margin = R.escape_margin(centre[0], centre[1], m, 2 * bits)
        gx, gy = rng.integers(0, W, SAMPLES), rng.integers(0, H, SAMPLES)
        gx[0], gy[0] = W // 2, H // 2   # the centre pixel: dc = 0, it follows the reference
        truth = np.array([R.mp_iters(*R.pixel_c(centre, sc, W, H, x, y, 2 * bits), m, 2 * bits) for x, y in zip(gx, gy)])
        agree = int((truth == n[gy, gx]).sum())
        print(f"scale {scale:.0e} M {m} (centre {len(centre[1])} digits, found in {tb:.1f} s): orbit L {L}, {bits} bits, {to:.3f} s on "
              f"the host, |Z_L|^2 - 2 = {margin if margin is not None else 'none (bounded)'};  " + line("PERTURB", ms, n, m), flush=True)
        print(f"    sampled pixels equal to direct iteration at {2 * bits} bits: {agree} of {SAMPLES} (centre pixel: {n[gy[0], gx[0]]} vs "
              f"{truth[0]}); disagreeing pairs (GPU, direct): {[(int(a), int(b)) for a, b in zip(n[gy, gx], truth) if a != b][:8]}",
              flush=True)
    for big_m in (200000, 1000000):   # host orbit cost at large M (an interior centre runs all M iterations)
        for scale in (1e-20, 2.0 ** -900):
            t = time.time()
            with B.Orbit("-0.1", "0.2", scale, scale, big_m) as o:
                print(f"# host orbit, interior centre, M {big_m}, {o.bits} bits: {time.time() - t:.2f} s", flush=True)
    ctx.bind_mandelbrot_orbit(None)
    orbit.close()
    ctx.close()


if __name__ == "__main__":
    main()
