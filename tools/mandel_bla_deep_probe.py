"""Deep BLA (MC_PRECISION_PERTURB_BLA_DEEP) against plain perturbation (MC_PRECISION_PERTURB) at K4 geometry, 7680 x 5120, on one context.

Views: M33 at 1e-1000 (M = 6000) and 1e-2000 (M = 10 000), an interior view at 1e-1000 (centre -0.1 + 0.2i, M = 20 000) and K4's view
at 1e-8 (M = 50 000, a shallow orbit).  Per view both precisions render the same bound orbit, alternating, ROUNDS rounds; per render
the kernel time (HIP events around the device-buffer form, after warm launches, best of the rounds) and reference-equivalent
pixel-iterations per second (sum of min(n + 1, M)).  Beside them: the host orbit and deep-table times, the mean loop trips per pixel
(one more render under MC_MANDEL_BLA_COUNT_TRIPS), the share of pixels whose n equals PERTURB's, and how many SAMPLES pixels of each
plane equal direct fixed-point iteration at bits + 64.
    On an MI355X:  python tools/mandel_bla_deep_probe.py > profiles/perturb_bla_deep_probe.txt"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import mandel_perturb_deep_ref as D  # noqa: E402
import mandel_perturb_ref as R  # noqa: E402

B = entry.load_package().bindings
W, H = 7680, 5120
ASPECT = 2.0 / 3.0
ROUNDS = 3
SAMPLES = 24
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))


def timed(ctx, p, it, stream, warm):
    for _ in range(warm):
        ctx.mandelbrot_device(p, 0, it.data_ptr(), stream=stream.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    ctx.mandelbrot_device(p, 0, it.data_ptr(), stream=stream.cuda_stream)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), it.cpu().numpy().astype(np.uint32)


def rate(ms, n, max_iter):
    pi = int(np.minimum(n.astype(np.int64) + 1, max_iter).sum())
    return pi, pi / (ms * 1e-3)


def main():
    print(f"# K4 geometry {W} x {H}; kernel ms = HIP events around one launch, best of {ROUNDS} rounds alternating PERTURB / BLA_DEEP")
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# device {name}, {cus} CUs", flush=True)
    stream = torch.cuda.Stream()
    it = torch.empty((H, W), dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(11)
    c33_1000, m1000, e1000 = D.view(D.M33, "1e-1000")
    c33_2000, m2000, e2000 = D.view(D.M33, "1e-2000")
    views = [("M33 1e-1000", 6000, c33_1000, m1000[0], e1000),
             ("M33 1e-2000", 10000, c33_2000, m2000[0], e2000),
             ("interior 1e-1000", 20000, ("-0.1", "0.2"), m1000[0], e1000),
             ("K4 1e-8", 50000, R.DEEP_CENTRE, 1e-8, None)]
    for tag, m, centre, mant, E in views:
        sc = (mant, mant * ASPECT)
        t = time.time()
        o = B.Orbit(centre[0], centre[1], sc[0], sc[1], m, E)
        t_orbit = time.time() - t
        t = time.time()
        levels, entries = o.bla_deep()
        t_tab = time.time() - t
        ctx.bind_mandelbrot_orbit(o)
        bits, L = o.bits, o.length
        print(f"{tag}: M {m}, orbit L {L}, {bits} bits, deep {o.deep}, host orbit {t_orbit:.3f} s, host deep table {t_tab * 1e3:.1f} ms "
              f"({levels} levels, {entries} entries, {entries * 64 / 1e6:.1f} MB)", flush=True)
        pp = B.mandelbrot_params(W, H, max_iter=m, precision=B.PRECISION_PERTURB, **ZERO)
        pd = B.mandelbrot_params(W, H, max_iter=m, precision=B.PRECISION_PERTURB_BLA_DEEP, **ZERO)
        best, planes = {}, {}
        for r in range(ROUNDS):
            for ptag, p in (("PERTURB", pp), ("BLA_DEEP", pd)):
                ms, n = timed(ctx, p, it, stream, warm=2 if r == 0 else 0)
                planes[ptag] = n
                best[ptag] = min(best.get(ptag, ms), ms)
                pi, rt = rate(ms, n, m)
                print(f"    round {r} {ptag:8s}: kernel {ms:10.3f} ms  {rt:.3e} pixel-iters/s", flush=True)
        ptr = B.mandelbrot_params(W, H, max_iter=m, precision=B.PRECISION_PERTURB_BLA_DEEP, flags=B.MANDEL_BLA_COUNT_TRIPS, **ZERO)
        ctx.mandelbrot_device(ptr, 0, it.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        trips = it.cpu().numpy().astype(np.uint32)
        nd, npt = planes["BLA_DEEP"], planes["PERTURB"]
        gx, gy = rng.integers(0, W, SAMPLES), rng.integers(0, H, SAMPLES)
        gx[0], gy[0] = W // 2, H // 2
        t = time.time()
        if E is None:
            truth = np.array([R.mp_iters(*R.pixel_c(centre, sc, W, H, x, y, bits + 64), m, bits + 64) for x, y in zip(gx, gy)])
        else:
            truth = np.array([D.mp_iters_deep(centre, sc, E, W, H, x, y, m, bits + 64) for x, y in zip(gx, gy)])
        t_truth = time.time() - t
        for ptag in ("PERTURB", "BLA_DEEP"):
            pi, rt = rate(best[ptag], planes[ptag], m)
            print(f"    best    {ptag:8s}: kernel {best[ptag]:10.3f} ms  pixel-iters {pi:.4e}  {rt:.3e} pixel-iters/s  interior "
                  f"{(planes[ptag] == m).mean() * 100:6.2f} %  sampled = direct: {int((truth == planes[ptag][gy, gx]).sum())} of {SAMPLES}")
        print(f"    BLA_DEEP / PERTURB kernel time {best['BLA_DEEP'] / best['PERTURB']:.4f} (speed-up {best['PERTURB'] / best['BLA_DEEP']:.2f}x);"
              f"  mean trips per pixel {trips.astype(np.float64).mean():.1f} (max {int(trips.max())}) against a mean count "
              f"{np.minimum(nd.astype(np.int64) + 1, m).mean():.1f};  n equal to PERTURB's on {(nd == npt).mean() * 100:.3f} % of pixels;  "
              f"disagreeing samples (PERTURB, BLA_DEEP, direct): "
              f"{[(int(a), int(b), int(c)) for a, b, c in zip(npt[gy, gx], nd[gy, gx], truth) if a != c or b != c][:6]}  "
              f"(direct iteration {t_truth:.0f} s)", flush=True)
        ctx.bind_mandelbrot_orbit(None)
        o.close()
    ctx.close()


if __name__ == "__main__":
    main()
