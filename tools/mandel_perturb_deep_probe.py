"""The deep kernel of MC_PRECISION_PERTURB (scales below 2^-960, rescaled perturbation) on an MI355X, and the host orbit behind it.

1. Host: the reference orbit's time per iteration at about 1100, 3400 and 8300 fractional bits (Misiurewicz point M33, whose orbit stays
   bounded until the fixed point's own error has grown), and K4's PERTURB orbit (7680 x 5120 at 1e-8, M = 50 000).
2. Device, around M33 at 1e-300, 1e-1000 and 1e-2000, 1920 x 1280 and 7680 x 5120: kernel ms (mc_context_last_timing of the blocking
   call, best of REPS after one warm call), pixel-iterations per second (sum of min(n + 1, M)), and the share of iterations begun in the
   scaled phase, counted by the scalar restatement on SAMPLES pixels of sampled rows.
3. PERTURB on K4's view in the same process, and the deep kernel forced onto that view (its plain phase, MC_MANDEL_PERTURB_FORCE_DEEP).
    On an MI355X:  python tools/mandel_perturb_deep_probe.py > profiles/perturb_deep_probe.txt"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import mandel_perturb_deep_ref as D  # noqa: E402

B = entry.load_package().bindings
REPS = 3
SAMPLES = 48
K4 = ("-0.7436438870371587", "0.13182590420531198")


def params(W, H, M, flags=0):
    return B.mandelbrot_params(W, H, max_iter=M, precision=B.PRECISION_PERTURB, centre=(0.0, 0.0), scale=(0.0, 0.0), flags=flags)


def timed(ctx, p):
    _, it = ctx.mandelbrot(p, want_rgba=False)
    best = None
    for _ in range(REPS):
        ctx.mandelbrot(p, want_rgba=False)
        ms, _ = ctx.last_timing()
        best = ms if best is None else min(best, ms)
    return best, it


def rate(ms, n, M):
    pi = int(np.minimum(n.astype(np.int64) + 1, M).sum())
    return pi, pi / (ms * 1e-3)


def orbit_time(centre, m, E, M, reps=3):
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        o = B.Orbit(centre[0], centre[1], m[0], m[1], M, E)
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
        L, bits = o.length, o.bits
        o.close()
    return best, L, bits


def main():
    print("# host orbit (best of 3)")
    for depth, M in (("1e-300", 20000), ("1e-1000", 20000), ("2e-2466", 20000)):
        c, m, E = D.view(D.M33, depth)
        t, L, bits = orbit_time(c, m, E, M)
        print(f"orbit M33 {depth:>8}: bits {bits:5d}  L {L:6d}  {t * 1e3:9.2f} ms  {t / L * 1e6:8.3f} us/iteration")
    best = None
    for _ in range(5):
        t = time.perf_counter()
        B.Orbit(*K4, 1e-8, 1e-8 * 2 / 3, 50000).close()
        best = time.perf_counter() - t if best is None else min(best, time.perf_counter() - t)
    print(f"orbit K4 1e-8 M=50000: {best * 1e3:.2f} ms")
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# device {name}, {cus} CUs; kernel ms = mc_context_last_timing, best of {REPS} after one warm call")
    for depth, M in (("1e-300", 2000), ("1e-1000", 6000), ("1e-2000", 10000)):
        c, m, E = D.view(D.M33, depth)
        with B.Orbit(c[0], c[1], *m, M, E) as o:
            ctx.bind_mandelbrot_orbit(o)
            Zl = o.table().tolist()
            for W, H in ((1920, 1280), (7680, 5120)):
                ms, n = timed(ctx, params(W, H, M))
                pi, r = rate(ms, n, M)
                print(f"deep M33 {depth:>7} {W}x{H} M={M}: kernel {ms:9.3f} ms  pixel-iters {pi:.4e}  {r:.3e} pixel-iters/s  "
                      f"n {int(n.min())}..{int(n.max())}")
            rng = np.random.default_rng(5)
            gx, gy = rng.integers(0, 1920, SAMPLES), rng.integers(0, 1280, SAMPLES)
            ux, uy = D.u_axis(1920, m[0], idx=gx), D.u_axis(1280, m[1], idx=gy)
            st = {}
            for a, b in zip(ux, uy):
                D.scalar_iters(Zl, o.length, float(a), float(b), E, M, stats=st)
            print(f"   scaled-phase share of iterations ({SAMPLES} sampled pixels, restatement): {st['scaled'] / st['iters'] * 100:.1f} %")
    W, H, M = 7680, 5120, 50000
    with B.Orbit(*K4, 1e-8, 1e-8 * 2 / 3, M) as o:
        ctx.bind_mandelbrot_orbit(o)
        ms, n = timed(ctx, params(W, H, M))
        msd, nd = timed(ctx, params(W, H, M, flags=B.MANDEL_PERTURB_FORCE_DEEP))
        pi, r = rate(ms, n, M)
        print(f"PERTURB K4 1e-8 {W}x{H} M={M}: kernel {ms:9.3f} ms  {r:.3e} pixel-iters/s")
        print(f"deep kernel forced on the same view: kernel {msd:9.3f} ms  ({msd / ms:.2f}x)  plane identical: {np.array_equal(n, nd)}")
    ctx.close()


if __name__ == "__main__":
    main()
