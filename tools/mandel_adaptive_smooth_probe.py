"""Adaptive smooth supersampling (MC_MANDEL_SUPERSAMPLE_SMOOTH_ADAPTIVE) measured on one context.

1. Whole calls to RGBA8 (mc_context_last_timing's kernel time: first launch to the end of the RGBA8 conversion), per view and s = 2, 4: the
   plain smooth image, the full MC_MANDEL_SUPERSAMPLE_SMOOTH call and the adaptive chain at tau = 64, 256, 1024, alternating, best (worst) of
   ROUNDS rounds after a warm one.  tau = 256 goes through mc_mandelbrot_render_rgba8 (the flag route), the other two through
   mc_mandelbrot_render_adaptive_smooth with the RGBA8 output: the same chain.  Beside each adaptive time: the refined share
   (mc_context_last_refined), and the RMSE in RGBA8 levels (all four channels) against the full image, with the plain smooth image's RMSE
   against the full image beside it.
   Views: K1 (the reference's default view, 2000 x 2000, M = 128, F32) and the same at M = 1000; F64 at K4's 1e-8 view and deep BLA at M33
   1e-1000, both at 7680 x 5120.
2. --existing: the plain, smooth, bit-13 (s = 2) and bit-5 (s = 2) calls alone on K1 and K4 — run on this build and on the parent's
   (MC_LIB_PATH), processes alternating: the no-regression record.
--views a,b,...: a subset of k1,k1m1000,k4,bla; --rounds N.
    On an MI355X:  python tools/mandel_adaptive_smooth_probe.py > profiles/mandel_adaptive_smooth_probe.txt
                   python tools/mandel_adaptive_smooth_probe.py --existing   (this build, and MC_LIB_PATH=<the parent's library>)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mandel_adaptive_probe as AP  # noqa: E402  (the views, the orbit binding)
import mandel_equalise_probe as P  # noqa: E402

B = P.B
ROUNDS = P.ROUNDS
SM = B.MANDEL_COLOUR_SMOOTH
TAUS = (64, 256, 1024)


def rmse(a, b):
    d = a.astype(np.int16) - b.astype(np.int16)
    return float(np.sqrt((d.astype(np.float32) ** 2).mean(dtype=np.float64)))


def alternate(ctx, variants):
    """{name: (best, worst)} of the kernel ms; variants: (name, call); round 0 is the warm one, every round starts one variant later."""
    best, k = {}, len(variants)
    for r in range(ROUNDS + 1):
        for name, call in variants[r % k:] + variants[:r % k]:
            call()
            v = ctx.last_timing()[0]
            if r:
                lo, hi = best.get(name, (v, v))
                best[name] = (min(lo, v), max(hi, v))
    return best


def whole_section(ctx, which):
    print("## whole calls to RGBA8, mc_context_last_timing kernel ms, best (worst) of "
          f"{ROUNDS} alternating rounds after a warm one; RMSE in RGBA8 levels against the full MC_MANDEL_SUPERSAMPLE_SMOOTH image")
    for tag, W, H, kw, make in AP.views(which):
        with AP.bound(ctx, make, kw.get("precision")):
            plain_p = B.mandelbrot_params(W, H, flags=SM, **kw)
            print(f"{tag}, {W} x {H}:")
            for s in (2, 4):
                full_p = B.mandelbrot_params(W, H, flags=SM, supersample=s, smooth_samples=True, **kw)
                ad_p = B.mandelbrot_params(W, H, flags=SM, supersample=s, adaptive_smooth=True, **kw)
                variants = [("plain", lambda: ctx.mandelbrot_rgba8(plain_p)), ("full", lambda: ctx.mandelbrot_rgba8(full_p))]
                for tau in TAUS:
                    variants.append((f"tau {tau}", (lambda: ctx.mandelbrot_rgba8(ad_p)) if tau == B.MANDEL_ADAPTIVE_SMOOTH_THRESHOLD
                                     else (lambda tau=tau: ctx.mandelbrot_adaptive_smooth(ad_p, tau, rgba8=True))))
                t = alternate(ctx, variants)
                full = ctx.mandelbrot_rgba8(full_p)
                plain_rmse = rmse(ctx.mandelbrot_rgba8(plain_p), full)
                f, pl = t["full"], t["plain"]
                spread = f[1] - f[0]
                print(f"    s = {s}: plain {pl[0]:9.3f} ms ({pl[1]:9.3f}), RMSE {plain_rmse:6.3f};  full {f[0]:9.3f} ms ({f[1]:9.3f}), spread {spread:7.3f}")
                for tau in TAUS:
                    img = ctx.mandelbrot_adaptive_smooth(ad_p, tau, rgba8=True)
                    refined, pixels = ctx.last_refined()
                    a = t[f"tau {tau}"]
                    gain = f[0] - a[0]
                    print(f"        tau {tau:5d}: adaptive {a[0]:9.3f} ms ({a[1]:9.3f})   adaptive / full {a[0] / f[0]:5.3f}   "
                          f"faster by {gain:9.3f} ms = {gain / spread if spread > 0 else float('inf'):7.1f} x the full call's spread   "
                          f"refined {refined} of {pixels} = {100 * refined / pixels:5.2f} %   RMSE {rmse(img, full):6.3f}", flush=True)
                    del img
                del full


def existing_section(ctx, which):
    print(f"## existing calls to RGBA8 alone, kernel ms, best (worst) of {ROUNDS} alternating rounds after a warm one")
    for tag, W, H, kw, make in AP.views(which):
        with AP.bound(ctx, make, kw.get("precision")):
            ps = [("plain", B.mandelbrot_params(W, H, **kw)), ("smooth", B.mandelbrot_params(W, H, flags=SM, **kw)),
                  ("bit 13 s=2", B.mandelbrot_params(W, H, flags=SM | 8192, supersample=2, **kw)),
                  ("bit 5 s=2", B.mandelbrot_params(W, H, flags=32, supersample=2, **kw))]
            t = alternate(ctx, [(n, (lambda p=p: ctx.mandelbrot_rgba8(p))) for n, p in ps])
            print(f"{tag}, {W} x {H}: " + ";  ".join(f"{n} {t[n][0]:9.3f} ms ({t[n][1]:9.3f})" for n, _ in ps), flush=True)


def main():
    args = sys.argv[1:]
    which = ["k1", "k1m1000", "k4", "bla"]
    if "--views" in args:
        which = args[args.index("--views") + 1].split(",")
    if "--rounds" in args:
        global ROUNDS
        ROUNDS = int(args[args.index("--rounds") + 1])
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# {' '.join(args) or 'whole calls'}: device {name}, {cus} CUs; shader clock under load {ctx.measure_clock():.0f} MHz; "
          f"library {os.environ.get('MC_LIB_PATH', 'this build')}; build {B.build_id()}", flush=True)
    if "--existing" in args:
        existing_section(ctx, [v for v in which if v in ("k1", "k4")])
    else:
        whole_section(ctx, which)
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
