"""BLA (MC_PRECISION_PERTURB_BLA) against plain perturbation (MC_PRECISION_PERTURB) at K4 geometry, 7680 x 5120, on one context.

The views of DESIGN.md §3.6 plus one interior view at M = 200 000.  Per view the two precisions alternate (ROUNDS rounds) on the same
bound orbit; per render the kernel time (HIP events around the device-buffer form, after two warm launches, best of REPS x LAUNCHES)
and reference-equivalent pixel-iterations per second (sum of min(n + 1, M)).  BLA's line adds the mean loop trips per pixel (one more
render under MC_MANDEL_BLA_COUNT_TRIPS), the host time of the BLA table, the share of pixels whose n equals PERTURB's, and how many
SAMPLES pixels of each plane equal direct high-precision iteration.
    On an MI355X:  python tools/mandel_bla_probe.py > profiles/perturb_bla_probe.txt"""
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
W, H = 7680, 5120
ASPECT = 2.0 / 3.0
REPS, LAUNCHES, ROUNDS = 2, 2, 2
SAMPLES = 24
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))


def timed(ctx, p, it, stream, reps=REPS, launches=LAUNCHES):
    for _ in range(2):
        ctx.mandelbrot_device(p, 0, it.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    best = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(launches):
            ctx.mandelbrot_device(p, 0, it.data_ptr(), stream=stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1) / launches
        best = ms if best is None else min(best, ms)
    return best, it.cpu().numpy().astype(np.uint32)


def rate(ms, n, max_iter):
    pi = int(np.minimum(n.astype(np.int64) + 1, max_iter).sum())
    return pi, pi / (ms * 1e-3)


def main():
    print(f"# K4 geometry {W} x {H}; kernel ms = HIP events, best of {REPS} x {LAUNCHES} launches after 2 warm, {ROUNDS} rounds "
          f"alternating PERTURB / BLA")
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# device {name}, {cus} CUs", flush=True)
    stream = torch.cuda.Stream()
    it = torch.empty((H, W), dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(11)
    views = [("K4 1e-8", 50000, (1e-8, 1e-8 * ASPECT), lambda: R.DEEP_CENTRE),
             ("boundary 1e-20", 20000, (1e-20, 1e-20 * ASPECT), lambda: R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 20000, 70, 134)),
             ("boundary 1e-50", 20000, (1e-50, 1e-50 * ASPECT), lambda: R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 20000, 172, 236)),
             ("interior 1e-200", 20000, (1e-200, 1e-200 * ASPECT), lambda: ("-0.1", "0.2")),
             ("interior 1e-200 M 200000", 200000, (1e-200, 1e-200 * ASPECT), lambda: ("-0.1", "0.2"))]
    for tag, m, sc, centre_of in views:
        centre = centre_of()
        t = time.time()
        o = B.Orbit(centre[0], centre[1], sc[0], sc[1], m)
        t_orbit = time.time() - t
        t = time.time()
        levels, entries = o.bla()
        t_bla = time.time() - t
        ctx.bind_mandelbrot_orbit(o)
        bits, L = o.bits, o.length
        print(f"{tag}: M {m}, orbit L {L}, {bits} bits, host orbit {t_orbit:.3f} s, host BLA table {t_bla * 1e3:.1f} ms "
              f"({levels} levels, {entries} entries, {entries * 40 / 1e6:.1f} MB)", flush=True)
        pp = B.mandelbrot_params(W, H, max_iter=m, precision=B.PRECISION_PERTURB, **ZERO)
        pb = B.mandelbrot_params(W, H, max_iter=m, precision=B.PRECISION_PERTURB_BLA, **ZERO)
        slow = m >= 100000   # PERTURB's all-interior frame at M = 200 000 costs seconds: one timed launch
        best, planes = {}, {}
        for r in range(1 if slow else ROUNDS):
            for ptag, p in (("PERTURB", pp), ("BLA", pb)):
                ms, n = timed(ctx, p, it, stream, reps=1 if slow else REPS, launches=1 if slow else LAUNCHES)
                planes[ptag] = n
                best[ptag] = min(best.get(ptag, ms), ms)
                pi, rt = rate(ms, n, m)
                print(f"    round {r} {ptag:7s}: kernel {ms:10.3f} ms  {rt:.3e} pixel-iters/s", flush=True)
        ptr = B.mandelbrot_params(W, H, max_iter=m, precision=B.PRECISION_PERTURB_BLA, flags=B.MANDEL_BLA_COUNT_TRIPS, **ZERO)
        ctx.mandelbrot_device(ptr, 0, it.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        trips = it.cpu().numpy().astype(np.uint32)
        nb, npt = planes["BLA"], planes["PERTURB"]
        gx, gy = rng.integers(0, W, SAMPLES), rng.integers(0, H, SAMPLES)
        gx[0], gy[0] = W // 2, H // 2
        truth = np.array([R.mp_iters(*R.pixel_c(centre, sc, W, H, x, y, 2 * bits), m, 2 * bits) for x, y in zip(gx, gy)])
        for ptag in ("PERTURB", "BLA"):
            pi, rt = rate(best[ptag], planes[ptag], m)
            print(f"    best    {ptag:7s}: kernel {best[ptag]:10.3f} ms  pixel-iters {pi:.4e}  {rt:.3e} pixel-iters/s  interior "
                  f"{(planes[ptag] == m).mean() * 100:6.2f} %  sampled = direct: {int((truth == planes[ptag][gy, gx]).sum())} of {SAMPLES}")
        print(f"    BLA / PERTURB kernel time {best['BLA'] / best['PERTURB']:.4f} (speed-up {best['PERTURB'] / best['BLA']:.2f}x);  "
              f"mean trips per pixel {trips.astype(np.float64).mean():.1f} (max {int(trips.max())});  n equal to PERTURB's on "
              f"{(nb == npt).mean() * 100:.3f} % of pixels;  disagreeing samples (PERTURB, BLA, direct): "
              f"{[(int(a), int(b), int(c)) for a, b, c in zip(npt[gy, gx], nb[gy, gx], truth) if a != c or b != c][:6]}", flush=True)
        ctx.bind_mandelbrot_orbit(None)
        o.close()
    ctx.close()


if __name__ == "__main__":
    main()
