"""Histogram-equalised colouring (MC_MANDEL_COLOUR_EQUALISED) measured at K4 geometry, 7680 x 5120, on one context.

1. The histogram kernel alone on four uint32 count planes: K4's 1e-8 view (M = 50 000), the 48 %-interior boundary view at 1e-50
   (M = 20 000), the all-interior view at 1e-200 (M = 20 000), uniformly random counts at M = 200 000.  Per plane: the floor (a plain
   16-B-per-lane read-only pass over the same plane, tools/mandel_equalise_probe.hip), the library's kernel, and the naive
   one-atomic-per-pixel kernel (the tool's own); time, bytes read per second, ratio to the floor.  K4's plane also as uint16.
2. What a range's size and a further range cost: the library's kernel on K4's plane at max_iter 1023 ... 200 000 (counts above it fall
   into the last bin, so the input keeps its skew) and on random planes of those ranges; and the switch from LDS ranges to the global
   table, max_iter 2^20 - 1 against 2^20 on the same planes.
3. The whole-image equalised mc_mandelbrot_render_rgba8 against the plain one (mc_context_last_timing's kernel time): F64 at K4's view
   and deep BLA at M33 1e-1000; the overhead split into histogram, table round trip + host map, recolouring.
All times: HIP events, warm launches, best of ROUNDS rounds alternating the variants; the box clock (mc_context_measure_clock) beside them.
    On an MI355X:  python tools/mandel_equalise_probe.py > profiles/mandel_equalise_probe.txt
                   python tools/mandel_equalise_probe.py --naive-interior >> profiles/mandel_equalise_probe.txt   (slow, not faulty: run it last, under a time limit of its own)
                   python tools/mandel_equalise_probe.py --plain-only    (the plain fused render alone: run on this build and on the parent's, MC_LIB_PATH)"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import mandel_equalise_ref as E  # noqa: E402
import mandel_perturb_deep_ref as D  # noqa: E402
import mandel_perturb_ref as R  # noqa: E402

B = entry.load_package().bindings
W, H = 7680, 5120
NPIX = W * H
ASPECT = 2.0 / 3.0
ROUNDS = 3
ZERO = dict(centre=(0.0, 0.0), scale=(0.0, 0.0))
HELPER_SRC = os.path.join(ROOT, "tools", "mandel_equalise_probe.hip")
HELPER = os.path.join(ROOT, "tools", "bin", "libmandel_equalise_probe.so")


def helper():
    if not os.path.exists(HELPER):
        os.makedirs(os.path.dirname(HELPER), exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-o", HELPER, HELPER_SRC])
    L = C.CDLL(HELPER)
    vp = C.c_void_p
    L.probe_read_pass.argtypes = [vp, C.c_uint64, vp, C.c_int, vp]
    L.probe_naive_histogram.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint32, vp, C.c_int, vp]
    return L


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


def render_plane(ctx, stream, centre, scale, M, E2=None, precision=None):
    """The uint32 count plane of a view at K4 geometry, on the device (deep BLA: every orbit, the fastest render)."""
    o = B.Orbit(centre[0], centre[1], scale[0], scale[1], M, E2)
    o.bla_deep()
    ctx.bind_mandelbrot_orbit(o)
    it = torch.empty((H, W), dtype=torch.int32, device="cuda")
    p = B.mandelbrot_params(W, H, max_iter=M, precision=precision or B.PRECISION_PERTURB_BLA_DEEP, **ZERO)
    ctx.mandelbrot_device(p, 0, it.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    ctx.bind_mandelbrot_orbit(None)
    o.close()
    return it


def describe(it, M):
    n = it.cpu().numpy().view(np.uint32)
    return (f"interior {(n == M).mean() * 100:6.2f} %, {np.unique(n).size} distinct counts, 1st..99th percentile "
            f"{int(np.percentile(n, 1))}..{int(np.percentile(n, 99))}")


def histogram_section(ctx, stream, Hp, cus, naive_interior_only=False):
    s = stream.cuda_stream
    blocks = cus * 8
    sink = torch.zeros(blocks, dtype=torch.int32, device="cuda")
    boundary = R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 20000, 172, 236)
    planes = [("K4 1e-8", 50000, lambda: render_plane(ctx, stream, R.DEEP_CENTRE, (1e-8, 1e-8 * ASPECT), 50000)),
              ("boundary 1e-50", 20000, lambda: render_plane(ctx, stream, boundary, (1e-50, 1e-50 * ASPECT), 20000)),
              ("interior 1e-200", 20000, lambda: render_plane(ctx, stream, ("-0.1", "0.2"), (1e-200, 1e-200 * ASPECT), 20000)),
              ("random M 200000", 200000, lambda: torch.randint(0, 200001, (H, W), dtype=torch.int32, device="cuda",
                                                                generator=torch.Generator(device="cuda").manual_seed(1)))]
    if naive_interior_only:
        tag, M, make = planes[2]
        it = make()
        hist = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
        stream.synchronize()
        ms = event_ms(stream, lambda: Hp.probe_naive_histogram(it.data_ptr(), 4, NPIX, M, hist.data_ptr(), blocks, s), warm=0)
        ms2 = event_ms(stream, lambda: Hp.probe_naive_histogram(it.data_ptr(), 4, NPIX, M, hist.data_ptr(), blocks, s), warm=0)
        print(f"{tag}: naive one-atomic-per-pixel kernel {ms:10.3f} ms, again {ms2:10.3f} ms  ({NPIX * 4 / min(ms, ms2) / 1e6:.1f} GB/s read); "
              f"table sums to {int(hist.cpu().numpy().view(np.uint32).sum(dtype=np.uint64))} = 2 x {NPIX}", flush=True)
        return
    print("## 1. the histogram kernel alone (uint32 planes, 157.3 MB read; floor = the read-only pass of this tool in the same rounds)")
    kept = {}
    for tag, M, make in planes:
        it = make()
        if tag != "random M 200000":
            kept[tag] = it
        hist = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
        stream.synchronize()
        variants = [("floor", lambda: Hp.probe_read_pass(it.data_ptr(), NPIX * 4, sink.data_ptr(), blocks, s)),
                    ("library", lambda: ctx.mandelbrot_histogram_device(it.data_ptr(), 4, NPIX, M, hist.data_ptr(), stream=s))]
        if tag != "interior 1e-200":   # (the naive kernel on the all-interior plane: --naive-interior, last)
            variants.append(("naive", lambda: Hp.probe_naive_histogram(it.data_ptr(), 4, NPIX, M, hist.data_ptr(), blocks, s)))
        t = best_of(stream, variants)
        hist.zero_()
        ctx.mandelbrot_histogram_device(it.data_ptr(), 4, NPIX, M, hist.data_ptr(), stream=s)
        stream.synchronize()
        ok = np.array_equal(hist.cpu().numpy().view(np.uint32), E.histogram(it.cpu().numpy().view(np.uint32), M))
        print(f"{tag}: M {M}, {describe(it, M)}; library table == bincount: {ok}")
        for name, (lo, hi) in t.items():
            print(f"    {name:8s}: best {lo:8.4f} ms (worst {hi:8.4f})  {NPIX * 4 / lo / 1e6:8.1f} GB/s read  {lo / t['floor'][0]:7.2f} x floor", flush=True)
        if tag == "K4 1e-8":
            it16 = it.to(torch.int16)
            t = best_of(stream, [("floor u16", lambda: Hp.probe_read_pass(it16.data_ptr(), NPIX * 2, sink.data_ptr(), blocks, s)),
                                 ("library u16", lambda: ctx.mandelbrot_histogram_device(it16.data_ptr(), 2, NPIX, M, hist.data_ptr(), stream=s))])
            for name, (lo, hi) in t.items():
                print(f"    {name:11s}: best {lo:8.4f} ms (worst {hi:8.4f})  {NPIX * 2 / lo / 1e6:8.1f} GB/s read  {lo / t['floor u16'][0]:7.2f} x floor (78.6 MB)",
                      flush=True)
    print("## 2. what a range's size and a further range cost: the library's kernel on K4's plane with counts above max_iter in the last bin "
          "(the input keeps its skew), and on uniformly random planes")
    k4 = kept["K4 1e-8"]
    for M in (1023, 4095, 8191, 16383, 32767, 50000, 200000):
        rnd = torch.randint(0, M + 1, (H, W), dtype=torch.int32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(M))
        hist = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
        stream.synchronize()
        t = best_of(stream, [(ptag, (lambda it: lambda: ctx.mandelbrot_histogram_device(it.data_ptr(), 4, NPIX, M, hist.data_ptr(), stream=s))(it))
                             for ptag, it in (("K4 clamped", k4), ("random", rnd))])
        print(f"    max_iter {M:6d} ({(M + 1) * 4 // 1024:3d} KB, {(M + 16384) // 16384:2d} range(s)): K4 clamped {t['K4 clamped'][0]:8.4f} ms (worst "
              f"{t['K4 clamped'][1]:8.4f})   random {t['random'][0]:8.4f} ms (worst {t['random'][1]:8.4f})", flush=True)
    print("## the switch: max_iter 2^20 - 1 (64 LDS ranges, the last table kept in LDS) against 2^20 (wave-combined atomics on the global table), same planes")
    lo, hi = (1 << 20) - 1, 1 << 20
    rnd = torch.randint(0, lo + 1, (H, W), dtype=torch.int32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    hist = torch.zeros(hi + 1, dtype=torch.int32, device="cuda")
    stream.synchronize()
    for ptag, it in list(kept.items()) + [("random 0..2^20-1", rnd)]:
        t = best_of(stream, [("lds", lambda: ctx.mandelbrot_histogram_device(it.data_ptr(), 4, NPIX, lo, hist.data_ptr(), stream=s)),
                             ("global", lambda: ctx.mandelbrot_histogram_device(it.data_ptr(), 4, NPIX, hi, hist.data_ptr(), stream=s))])
        print(f"    {ptag:17s}: LDS ranges {t['lds'][0]:8.4f} ms (worst {t['lds'][1]:8.4f})   global table {t['global'][0]:8.4f} ms (worst "
              f"{t['global'][1]:8.4f})   LDS / global {t['lds'][0] / t['global'][0]:.3f}", flush=True)

def fused_ms(ctx, p, rounds=ROUNDS, also=None):
    """Best and worst mc_context_last_timing kernel ms of mc_mandelbrot_render_rgba8(p) (and of `also`), alternating."""
    out = {}
    for r in range(rounds + 1):   # round 0 is the warm one
        for name, q in (("plain", p),) + ((("equalised", also),) if also is not None else ()):
            ctx.mandelbrot_rgba8(q)
            k, _ = ctx.last_timing()
            if r:
                lo, hi = out.get(name, (k, k))
                out[name] = (min(lo, k), max(hi, k))
    return out


def render_views():
    c33, m33, e33 = D.view(D.M33, "1e-1000")
    k4 = (float(R.DEEP_CENTRE[0]), float(R.DEEP_CENTRE[1]))
    return [("F64 K4 1e-8", dict(max_iter=50000, precision=B.PRECISION_F64, centre=k4, scale=(1e-8, 1e-8 * ASPECT)), None),
            ("BLA_DEEP M33 1e-1000", dict(max_iter=6000, precision=B.PRECISION_PERTURB_BLA_DEEP, **ZERO),
             lambda: B.Orbit(c33[0], c33[1], m33[0], m33[0] * ASPECT, 6000, e33))]


def render_section(ctx, stream, plain_only=False):
    s = stream.cuda_stream
    print("## 3. whole image: mc_mandelbrot_render_rgba8 (mc_context_last_timing kernel ms: first launch to the end of the conversion), "
          f"best of {ROUNDS} rounds after a warm one" + ("" if plain_only else ", plain and equalised alternating"))
    for tag, kw, make in render_views():
        M = kw["max_iter"]
        o = None
        if make:
            o = make()
            o.bla_deep()
            ctx.bind_mandelbrot_orbit(o)
        plain = B.mandelbrot_params(W, H, **kw)
        eq = B.mandelbrot_params(W, H, flags=getattr(B, "MANDEL_COLOUR_EQUALISED", 0), **kw)
        t = fused_ms(ctx, plain, also=None if plain_only else eq)
        print(f"{tag}: plain {t['plain'][0]:9.3f} ms (worst {t['plain'][1]:9.3f})", end="")
        if plain_only:
            print(flush=True)
        else:
            d = t["equalised"][0] - t["plain"][0]
            print(f"   equalised {t['equalised'][0]:9.3f} ms (worst {t['equalised'][1]:9.3f})   overhead {d:7.3f} ms = {d / t['plain'][0] * 100:6.2f} %", flush=True)
            it = torch.empty((H, W), dtype=torch.int32, device="cuda")
            rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
            hist = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
            ctx.mandelbrot_device(plain, 0, it.data_ptr(), stream=s)
            stream.synchronize()
            t_counts = best_of(stream, [("counts only", lambda: ctx.mandelbrot_device(plain, 0, it.data_ptr(), stream=s)),
                                        ("counts + vec4", lambda: ctx.mandelbrot_device(plain, rgba.data_ptr(), 0, stream=s))])
            t_hist = best_of(stream, [("histogram", lambda: ctx.mandelbrot_histogram_device(it.data_ptr(), 4, NPIX, M, hist.data_ptr(), stream=s))])
            hist.zero_()
            ctx.mandelbrot_histogram_device(it.data_ptr(), 4, NPIX, M, hist.data_ptr(), stream=s)
            stream.synchronize()
            trip = []
            for _ in range(ROUNDS):
                t0 = time.perf_counter()
                h = hist.cpu().numpy().view(np.uint32)
                t1 = time.perf_counter()
                m = B.equalise_map(M, h)
                t2 = time.perf_counter()
                trip.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
            first = []
            for k in range(ROUNDS):   # a new map each time: composing lut[map[.]] on the host, its upload, the kernel
                m2 = m.copy()
                m2[0] = k + 1
                t0 = time.perf_counter()
                ctx.mandelbrot_recolour_device(plain, it.data_ptr(), 4, m2, rgba.data_ptr(), stream=s)
                stream.synchronize()
                first.append((time.perf_counter() - t0) * 1e3)
            t_rec = best_of(stream, [("recolour", lambda: ctx.mandelbrot_recolour_device(plain, it.data_ptr(), 4, m2, rgba.data_ptr(), stream=s))])
            print(f"    render kernel, counts only {t_counts['counts only'][0]:9.3f} ms, vec4 only {t_counts['counts + vec4'][0]:9.3f} ms;  histogram "
                  f"{t_hist['histogram'][0]:7.4f} ms;  table to the host {min(a for a, _ in trip):6.3f} ms + host map {min(b for _, b in trip):6.3f} ms;  "
                  f"recolouring: new map (compose + upload + kernel, host clock) {min(first):7.3f} ms, kernel alone {t_rec['recolour'][0]:7.4f} ms "
                  f"({NPIX * 20 / t_rec['recolour'][0] / 1e6:.0f} GB/s of 4 B read + 16 B written)", flush=True)
        if o is not None:
            ctx.bind_mandelbrot_orbit(None)
            o.close()


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# {' '.join(sys.argv[1:]) or 'histogram + whole image'}: K4 geometry {W} x {H}; device {name}, {cus} CUs; shader clock under load "
          f"{ctx.measure_clock():.0f} MHz; build {B.build_id()}", flush=True)
    stream = torch.cuda.Stream()
    if "--plain-only" in sys.argv:
        render_section(ctx, stream, plain_only=True)
    elif "--naive-interior" in sys.argv:
        histogram_section(ctx, stream, helper(), cus, naive_interior_only=True)
    else:
        histogram_section(ctx, stream, helper(), cus)
        render_section(ctx, stream)
        print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
