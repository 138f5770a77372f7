"""The Buddhabrot kernels measured on one context: HIP events on one stream, warm launches, no hardware counters.

1. The gate between the two forms: the default view at 1920 x 1280 with 2^26 samples, at M = 1000 and at M = 5000 with min_iter 100; the
   plain form (MC_BUDDHA_KERNEL_PLAIN) and the pooled form (MC_BUDDHA_KERNEL_POOLED) alternating three times each after a warm round.
   The pooled form ships if it is faster by at least 3 x the plain form's own spread (worst - best).
2. What the shipped form delivers there, best of 5: ms, samples/s, iterations/s, adds/s.  Adds are exact (the statistics' `added`);
   iterations are the statistics' `points` (the replay) plus the classification's, which the statistics do not carry: their mean per
   sample is taken from the numpy restatement (tests/buddhabrot_ref.py) over the first 2^18 samples and scaled.
3. The same samples against an all-outside view (the same iterations, zero adds: what the atomics cost) and against a 1 x 1 view (every
   add on one address: the contention extreme).
4. The iteration rate beside the F64 Mandelbrot kernel's (mc_mandelbrot_render_device_async, counts only, 1920 x 1280, M = 1000, the
   default view), measured in the same process.
5. The tone-map kernel beside a device-to-device copy of the plane.
    On an MI355X:  python tools/buddhabrot_probe.py > profiles/buddhabrot_probe.txt"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import buddhabrot_ref as R  # noqa: E402

B = entry.load_package().bindings
W, H, N = 1920, 1280, 1 << 26
CONFIGS = [("M = 1000", dict(max_iter=1000, min_iter=0)), ("M = 5000, min_iter 100", dict(max_iter=5000, min_iter=100))]
FORMS = [("plain", B.BUDDHA_KERNEL_PLAIN), ("pooled", B.BUDDHA_KERNEL_POOLED)]
OUTSIDE = (100.0, 100.0, 3.0, 2.0)
ONE_BIN = (-0.5, 0.0, 16.0, 16.0)


def event_ms(stream, launch):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    launch()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1)


def best_of(stream, launch, rounds=5):
    launch()
    stream.synchronize()
    v = [event_ms(stream, launch) for _ in range(rounds)]
    return min(v), max(v)


def classify_iterations_per_sample(kw):
    """Mean classification iterations per sample (0 for a skipped one, n + 1 for an escaped one, M otherwise) over the first 2^18 samples."""
    p = R.params(W, H, 1 << 18, **kw)
    cx, cy = R.sample_c(p, np.arange(1 << 18, dtype=np.uint64))
    keep = ~R.interior(cx, cy)
    n = R.classify(cx[keep], cy[keep], kw["max_iter"])
    return float(np.where(n < kw["max_iter"], n + 1, kw["max_iter"]).sum()) / float(1 << 18)


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# Buddhabrot probe: {W} x {H}, 2^26 samples, default view and sample window, seed 1; device {name}, {cus} CUs; shader clock under "
          f"load {ctx.measure_clock():.0f} MHz; build {B.build_id()}; HIP events, no hardware counters", flush=True)
    stream = torch.cuda.Stream()
    s_ = stream.cuda_stream
    plane = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    stats = torch.zeros(5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def run(kw, flags=0, view=None, w=W, h=H, target=plane, d_stats=0):
        ctx.buddhabrot_device(B.buddhabrot_params(w, h, N, flags=flags, view=view, **kw), target.data_ptr(), d_stats, stream=s_)

    shipped = {}
    print("## 1. the gate: plain and pooled alternating, three rounds after a warm one (ms)")
    for tag, kw in CONFIGS:
        times = {f: [] for f, _ in FORMS}
        for r in range(4):
            for f, bit in FORMS:
                v = event_ms(stream, lambda: run(kw, bit))
                if r:
                    times[f].append(v)
        pl, po = times["plain"], times["pooled"]
        spread = max(pl) - min(pl)
        gain = min(pl) - min(po)
        verdict = "pooled passes the gate" if gain >= 3.0 * spread and gain > 0 else "pooled does NOT pass the gate"
        print(f"{tag}: plain {' '.join(f'{v:9.3f}' for v in pl)}   pooled {' '.join(f'{v:9.3f}' for v in po)}   plain's spread {spread:.3f}, "
              f"best plain - best pooled {gain:.3f} = {gain / spread if spread else float('inf'):.1f} x the spread: {verdict}", flush=True)
        shipped[tag] = min(po) < min(pl)

    print("## 2. the shipped form (no flag bit), best of 5; 3. the same samples against an all-outside view and a 1 x 1 view")
    rates = {}
    for tag, kw in CONFIGS:
        stats.zero_()
        plane.zero_()
        torch.cuda.synchronize()
        run(kw, d_stats=stats.data_ptr())
        stream.synchronize()
        st = [int(v) for v in stats.cpu().numpy().view(np.uint64)]
        per = classify_iterations_per_sample(kw)
        iters = per * N + st[3]
        lo, hi = best_of(stream, lambda: run(kw))
        rates[tag] = iters / lo * 1e3
        print(f"{tag}: samples {st[0]}, skipped {st[1]}, contributing {st[2]}, points {st[3]}, added {st[4]}; classification iterations per "
              f"sample {per:.2f} (first 2^18 samples, restated), iterations per sample {iters / N:.2f}, iterations per add {iters / max(st[4], 1):.1f}")
        print(f"    default view : best {lo:9.3f} ms (worst {hi:9.3f})  {N / lo * 1e3:.3e} samples/s  {iters / lo * 1e3:.3e} iterations/s  "
              f"{st[4] / lo * 1e3:.3e} adds/s")
        for label, form in (("plain form   ", B.BUDDHA_KERNEL_PLAIN), ("pooled form  ", B.BUDDHA_KERNEL_POOLED)):
            flo, fhi = best_of(stream, lambda: run(kw, form))
            print(f"    {label}: best {flo:9.3f} ms (worst {fhi:9.3f})  {iters / flo * 1e3:.3e} iterations/s")
        olo, ohi = best_of(stream, lambda: run(kw, view=OUTSIDE))
        print(f"    all outside  : best {olo:9.3f} ms (worst {ohi:9.3f})  {iters / olo * 1e3:.3e} iterations/s, zero adds: the adds cost "
              f"{lo - olo:.3f} ms = {100 * (lo - olo) / lo:.1f} % of the default view's time, {st[4] / max(lo - olo, 1e-9) * 1e3:.3e} adds/s if they were alone")
        for label, form in (("  plain      ", B.BUDDHA_KERNEL_PLAIN), ("  pooled     ", B.BUDDHA_KERNEL_POOLED)):
            flo, fhi = best_of(stream, lambda: run(kw, form, view=OUTSIDE))
            print(f"    {label}: best {flo:9.3f} ms (worst {fhi:9.3f})  {iters / flo * 1e3:.3e} iterations/s (all outside)")
        stats.zero_()
        torch.cuda.synchronize()
        run(kw, view=ONE_BIN, w=1, h=1, target=one, d_stats=stats.data_ptr())
        stream.synchronize()
        a1 = int(stats.cpu().numpy().view(np.uint64)[4])
        blo, bhi = best_of(stream, lambda: run(kw, view=ONE_BIN, w=1, h=1, target=one), rounds=3)
        print(f"    1 x 1 view   : best {blo:9.3f} ms (worst {bhi:9.3f})  {a1} adds on one address, {a1 / blo * 1e3:.3e} adds/s", flush=True)

    print("## 4. the F64 Mandelbrot kernel in the same process: counts only, 1920 x 1280, M = 1000, the default view")
    p = B.mandelbrot_params(W, H, max_iter=1000, precision=B.PRECISION_F64)
    it = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    lo, hi = best_of(stream, lambda: ctx.mandelbrot_device(p, 0, it.data_ptr(), stream=s_))
    n = it.cpu().numpy().view(np.uint32).astype(np.int64)
    iters = int(np.where(n < 1000, n + 1, 1000).sum())
    f64 = iters / lo * 1e3
    print(f"best {lo:9.3f} ms (worst {hi:9.3f})  {iters} iterations  {f64:.3e} iterations/s")
    for tag, _ in CONFIGS:
        print(f"    Buddhabrot, {tag}: {rates[tag]:.3e} iterations/s = {100 * rates[tag] / f64:.1f} % of it")

    print("## 5. the tone-map kernel (12 B read + 16 B written per pixel) beside a device-to-device copy of the plane (4 B + 4 B), best of 5")
    L = 1000
    m = B.buddhabrot_sqrt_map(L)
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    other = torch.empty_like(plane)
    torch.cuda.synchronize()
    d = plane.data_ptr()
    with torch.cuda.stream(stream):
        tlo, thi = best_of(stream, lambda: ctx.buddhabrot_tonemap_device(W, H, d, d, d, L, m, m, m, rgba.data_ptr(), stream=s_))
        clo, chi = best_of(stream, lambda: other.copy_(plane))
    print(f"tone map {tlo:8.4f} ms (worst {thi:8.4f})  {W * H * 28 / tlo / 1e6:8.1f} GB/s   copy {clo:8.4f} ms (worst {chi:8.4f})  "
          f"{W * H * 8 / clo / 1e6:8.1f} GB/s   tone map = {tlo / clo:.2f} x the copy")
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
