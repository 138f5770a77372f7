"""Two-float (MC_PRECISION_DS) against native fp64 (MC_PRECISION_F64) at K4: 7680 x 5120, M = 50 000, bench.K4_VIEW, both rendered on
one context.  Reports per precision the kernel time (HIP events around the device-buffer form, warmed, best of N), the
reference-equivalent pixel-iterations per second (sum of min(n + 1, M)), the share of pixels whose n differs between the two, and on a
few sampled rows the agreement of each with an 80-bit np.longdouble restatement of the same loop.  The DS / F64 comparison is repeated
at scales 1e-10 and 1e-12 (same centre, same aspect).  The 80-bit plane is not the truth either — boundary orbits are chaotic at any
finite precision — so it is reported as agreement, not as error.
    On an MI355X:  python tools/mandel_precision_probe.py > profiles/f64_mandel_precision_probe.txt"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

B = entry.load_package().bindings
W, H, M = 7680, 5120, 50000
CENTRE = (-0.7436438870371587, 0.13182590420531198)   # bench.K4_VIEW
ASPECT = 2.0 / 3.0
ROWS = (0, 1777, 2560, 4095)
REPS, LAUNCHES = 3, 4


def longdouble_rows(p, rows):
    """The loop of include/mc_compute.h (MC_PRECISION_F64) in np.longdouble, from the same view words, on the given rows."""
    ld = np.longdouble
    cxv = ld(np.float64(p.centre_x_hi)) + ld(np.float64(p.centre_x_lo))
    cyv = ld(np.float64(p.centre_y_hi)) + ld(np.float64(p.centre_y_lo))
    sxv = ld(np.float64(p.scale_x_hi)) + ld(np.float64(p.scale_x_lo))
    syv = ld(np.float64(p.scale_y_hi)) + ld(np.float64(p.scale_y_lo))
    cx = cxv + (np.arange(W, dtype=ld) / ld(W) - ld(0.5)) * sxv
    cy = cyv + (np.asarray(rows, dtype=ld) / ld(H) - ld(0.5)) * syv
    CX = np.broadcast_to(cx[None, :], (len(rows), W)).ravel().copy()
    CY = np.broadcast_to(cy[:, None], (len(rows), W)).ravel().copy()
    n = np.full(CX.shape, M, np.uint32)
    live = np.arange(CX.size)
    zx, zy, sx, sy = (np.zeros_like(CX) for _ in range(4))
    for i in range(M):
        nzx = (sx - sy) + CX
        nzy = ((ld(2) * zx) * zy) + CY
        zx, zy = nzx, nzy
        sx, sy = zx * zx, zy * zy
        esc = (sx + sy) > ld(2)
        if esc.any():
            n[live[esc]] = i
            k = ~esc
            live, CX, CY, zx, zy, sx, sy = live[k], CX[k], CY[k], zx[k], zy[k], sx[k], sy[k]
            if live.size == 0:
                break
    return n.reshape(len(rows), W)


def render(ctx, p, it, stream, timed):
    for _ in range(2):
        ctx.mandelbrot_device(p, 0, it.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    best = None
    if timed:
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


def main():
    nmant = np.finfo(np.longdouble).nmant
    print(f"# K4 geometry {W} x {H}, M = {M}, centre {CENTRE}; kernel ms = HIP events, best of {REPS} x {LAUNCHES} launches after 2 warm")
    print(f"# np.longdouble: nmant = {nmant}" + ("" if nmant == 63 else "  (NOT the x87 80-bit format: the agreement columns compare "
                                                                        "with this format instead)"))
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# device {name}, {cus} CUs, sclk {ctx.measure_clock():.0f} MHz")
    stream = torch.cuda.Stream()
    it = torch.empty((H, W), dtype=torch.int32, device="cuda")
    for scale in (1e-8, 1e-10, 1e-12):
        sc = (scale, scale * ASPECT)
        planes = {}
        for tag, prec in (("DS", B.PRECISION_DS), ("F64", B.PRECISION_F64)):
            p = B.mandelbrot_params(W, H, max_iter=M, precision=prec, centre=CENTRE, scale=sc)
            ms, n = render(ctx, p, it, stream, timed=scale == 1e-8)
            planes[tag] = (p, n)
            pi = int(np.minimum(n.astype(np.int64) + 1, M).sum())
            line = f"scale {scale:.0e} {tag:3s}: pixel-iters {pi}"
            if ms is not None:
                line += f"  kernel {ms:8.3f} ms  {pi / (ms * 1e-3):.3e} pixel-iters/s"
            print(line, flush=True)
        ds, f = planes["DS"][1], planes["F64"][1]
        print(f"scale {scale:.0e}: pixels whose n differs between DS and F64: {(ds != f).mean() * 100:.2f} %", flush=True)
        t = time.time()
        ref = longdouble_rows(planes["F64"][0], ROWS)
        agree = {tag: (planes[tag][1][list(ROWS)] == ref).mean() * 100 for tag in ("DS", "F64")}
        print(f"scale {scale:.0e}: rows {ROWS} ({len(ROWS) * W} pixels) equal to the {nmant + 1}-bit plane: DS {agree['DS']:.2f} %, "
              f"F64 {agree['F64']:.2f} %  ({time.time() - t:.0f} s on the host)", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
