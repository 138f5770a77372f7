"""The exact counts of sampled pixels (mc_mandelbrot_exact_counts_device) measured: rates, the wave kernel's slice constant, and the
agreement questions DESIGN.md section 3.6 left open.

1. Pixel-iterations per second of the wave kernel at n = 3, 8, 16 limbs and of the workgroup kernel at n = 17, 55, 131, on 4096 interior
   pixels (every pixel runs M), from mc_context_last_exact_timing's device_ms, best of ROUNDS; beside them the serial host call on 64 of
   the same pixels.  For the wave kernel also the time of one iteration of one round of waves (device_ms / M at 4096 pixels = 16 waves
   on each of 256 CUs): what exact_launch_iters' linear fit (csrc/mandel_exact.h) is derived from.
2. Section 3.6's three deep views (1e-20, 1e-50, 1e-200 at K4's size, M = 20 000) re-checked on 4096 lattice pixels each.
3. K4's own view (1e-8, M = 50 000): on lattice pixels where PERTURB's and F64's planes differ, which of the two the exact count sides with.
    On an MI355X:  python tools/mandel_exact_probe.py > profiles/mandel_exact_probe.txt"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import mandel_perturb_ref as R  # noqa: E402

B = entry.load_package().bindings
ROUNDS = 3
W, H = 7680, 5120
ASPECT = 2.0 / 3.0
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))
INTERIOR = ("-0.1", "0.2")
#        n, M on the device, M on the host (64 pixels)
RATES = ((3, 20000, 20000), (8, 10000, 5000), (16, 5000, 2000), (17, 2000, 2000), (55, 600, 300), (131, 200, 100))


def lattice(count, w, h):
    """The centre pixel and count - 1 pixels on a cols x rows lattice (the app's --exact-check lattice)."""
    cols = 1
    while cols * cols < count - 1:
        cols += 1
    rows = (count - 1 + cols - 1) // cols
    px = [(w // 2, h // 2)]
    for i in range(count - 1):
        px.append(((2 * (i % cols) + 1) * w // (2 * cols), (2 * (i // cols) + 1) * h // (2 * rows)))
    return np.array(px, np.uint32)


def rates(ctx, cus):
    print("# 1. rates: 4096 interior pixels of a 64 x 64 view around -0.1 + 0.2i, every pixel runs M; device_ms best of "
          f"{ROUNDS}; host: the serial call on 64 of them")
    print("# limbs kernel        M launches iters/launch  device ms | pixel-iters/s device | us/iter of a round | host pixel-iters/s | device / host")
    px = np.array([(x, y) for y in range(64) for x in range(64)], np.uint32)
    for n, M, Mh in RATES:
        E = -8192 if n == 131 else 96 - 64 * (n - 1) + 10
        with B.Orbit(INTERIOR[0], INTERIOR[1], 1.0, 1.0, 10, E) as o:
            assert (o.bits + 63) // 64 + 1 == n
            dcx, dcy, e = o.exact_pixel_offsets(64, 64, px)
            best = float("inf")
            for _ in range(ROUNDS):
                got = o.exact_counts(M, dcx, dcy, e, device=ctx)
                assert (got == M).all()
                ms, launches, limbs, per, kind = ctx.last_exact_timing()
                best = min(best, ms)
            t = time.perf_counter()
            host = o.exact_counts(Mh, dcx[:64], dcy[:64], e)
            th = time.perf_counter() - t
            assert (host == Mh).all() and limbs == n
            dev_rate, host_rate = 4096.0 * M / (best * 1e-3), 64.0 * Mh / th
            rounds = -(-4096 // (cus * (16 if kind == 1 else 1)))
            print(f"{n:7d} {'wave' if kind == 1 else 'workgroup':9s} {M:8d} {launches:8d} {per:12d} {best:10.3f} | {dev_rate:20.4e} | "
                  f"{best * 1e3 / M / rounds:18.3f} | {host_rate:18.4e} | {dev_rate / host_rate:8.1f}", flush=True)


def check_view(ctx, tag, o, m, count, other=None):
    """PERTURB's plane of the W x H view of o against the exact counts of `count` lattice pixels; other: (name, plane) to arbitrate."""
    ctx.bind_mandelbrot_orbit(o)
    _, n = ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=m, precision=B.PRECISION_PERTURB, **ZERO), want_rgba=False)
    px = lattice(count, W, H)
    if other is not None:   # only where the two planes differ
        differ = n != other[1]
        px = np.array([p for p in lattice(16 * count, W, H) if differ[p[1], p[0]]][:count], np.uint32)
    t = time.perf_counter()
    exact = ctx.exact_counts(o, W, H, px, m)
    wall = time.perf_counter() - t
    ms, launches, limbs, per, kind = ctx.last_exact_timing()
    mine = n[px[:, 1], px[:, 0]]
    bad = [(int(x), int(y), int(a), int(b)) for (x, y), a, b in zip(px, mine, exact) if a != b]
    print(f"{tag}: orbit L {o.length}, {o.bits} bits, {limbs} limbs; {len(px)} pixels exact in {ms:.1f} ms on the device ({launches} launches, "
          f"{wall * 1e3:.1f} ms the call); PERTURB equals the exact count on {len(px) - len(bad)} of {len(px)}; "
          f"centre pixel: render {mine[0]}, exact {exact[0]}; first mismatches (x, y, render, exact): {bad[:6]}", flush=True)
    if other is not None:
        theirs = other[1][px[:, 1], px[:, 0]]
        print(f"    where PERTURB and {other[0]} differ ({100.0 * differ.mean():.2f} % of the plane; {len(px)} lattice pixels of them): exact sides "
              f"with PERTURB on {int((mine == exact).sum())}, with {other[0]} on {int((theirs == exact).sum())}, with neither on "
              f"{int(((mine != exact) & (theirs != exact)).sum())}; mean |render - exact|: PERTURB "
              f"{np.abs(mine.astype(np.int64) - exact).mean():.2f}, {other[0]} {np.abs(theirs.astype(np.int64) - exact).mean():.2f}", flush=True)


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# device {name}, {cus} CUs")
    with B.Orbit("0", "0", 1e-8, 1e-8, 10) as o:   # the code objects, once
        o.exact_counts(2, [0.0], [0.0], device=ctx)
        o.exact_counts(2, [0.0], [0.0], extra_limbs=14, device=ctx)
    rates(ctx, cus)
    print(f"# 2. section 3.6's deep views at {W} x {H}, M = 20000, on 4096 lattice pixels each (the centre pixel first)")
    for scale, m, centre_of in ((1e-20, 20000, lambda: R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 20000, 70, 134)),
                                (1e-50, 20000, lambda: R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 20000, 172, 236)),
                                (1e-200, 20000, lambda: INTERIOR)):
        centre = centre_of()
        with B.Orbit(centre[0], centre[1], scale, scale * ASPECT, m) as o:
            check_view(ctx, f"scale {scale:.0e}", o, m, 4096)
    print("# 3. K4's view (1e-8, M = 50000): PERTURB against F64, arbitrated by the exact count")
    m = 50000
    sc = (1e-8, 1e-8 * ASPECT)
    _, f64 = ctx.mandelbrot(B.mandelbrot_params(W, H, max_iter=m, precision=B.PRECISION_F64, centre=tuple(map(float, R.DEEP_CENTRE)),
                                                scale=sc), want_rgba=False)
    with B.Orbit(R.DEEP_CENTRE[0], R.DEEP_CENTRE[1], sc[0], sc[1], m) as o:
        check_view(ctx, "K4 1e-8", o, m, 1024, other=("F64", f64))
    # F64 iterates ITS OWN c, the double centre_x + (x - 0.5) * scale_x of the view words (about 48 bits of centre): the exact count of
    # that double, from an orbit at centre 0 of the same scale with the pixel's c as its offset
    px = lattice(4096, W, H)
    split = lambda d: float(np.float32(d)) + float(np.float32(d - float(np.float32(d))))
    cx, cy = split(float(R.DEEP_CENTRE[0])), split(float(R.DEEP_CENTRE[1]))
    c64x = cx + (px[:, 0].astype(np.float64) / np.float64(W) - 0.5) * sc[0]
    c64y = cy + (px[:, 1].astype(np.float64) / np.float64(H) - 0.5) * sc[1]
    with B.Orbit("0", "0", sc[0], sc[1], m) as o0:
        exact = o0.exact_counts(m, c64x, c64y, device=ctx)
    mine = f64[px[:, 1], px[:, 0]]
    print(f"    F64 against the exact count of its own double c on 4096 lattice pixels: equal on {int((mine == exact).sum())}; "
          f"mean |render - exact| {np.abs(mine.astype(np.int64) - exact).mean():.2f}", flush=True)
    ctx.bind_mandelbrot_orbit(None)
    ctx.close()


if __name__ == "__main__":
    main()
