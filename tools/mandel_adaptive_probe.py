"""Adaptive supersampling (MC_MANDEL_SUPERSAMPLE_ADAPTIVE) measured on one context.

1. Whole calls, mc_mandelbrot_render_rgba8 (mc_context_last_timing's kernel time: first launch to the end of the RGBA8 conversion), per view
   and s = 2, 4: plain, full supersampling and adaptive, alternating, best of ROUNDS rounds after a warm one; beside each adaptive time the
   refined share (mc_context_last_refined) and the WORK RATIO — iterations executed by adaptive (the plain image + the s * s samples of
   every refined pixel) over iterations executed by the full grid, min(n + 1, M) per sample, by the restatement's rule
   (tests/mandel_adaptive_ref.py) evaluated on the library's own sample plane on the device.
   Views: K1 (the reference's default view, 2000 x 2000, M = 128, F32) and the same at M = 1000; F64 at K4's 1e-8 view, deep BLA at M33
   1e-1000 and PERTURB at the 48 %-interior boundary view at 1e-50, all three at 7680 x 5120.
2. --full-only: the plain and fully supersampled calls alone — run on this build and on the parent's (MC_LIB_PATH), processes alternating:
   the parent's full supersampling is what adaptive is measured against, and the pair is the no-regression record.
3. --refine: the refine-list pass alone on K4's anchor plane (uint16_t and uint32_t) against the read-only floor of
   tools/mandel_equalise_probe.hip over the same plane, same rounds; and the context scratch of K4 at s = 4, adaptive against full.
--views a,b,...: a subset of k1,k1m1000,k4,bla,perturb (the 7680 x 5120 perturbation view takes seconds per full call); --rounds N.
All times: HIP events, warm launches, best of ROUNDS rounds alternating the variants; the box clock (mc_context_measure_clock) beside them.
    On an MI355X:  python tools/mandel_adaptive_probe.py > profiles/mandel_adaptive_probe.txt
                   python tools/mandel_adaptive_probe.py --refine >> profiles/mandel_adaptive_probe.txt
                   python tools/mandel_adaptive_probe.py --full-only   (this build, and MC_LIB_PATH=<the parent's library>)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mandel_equalise_probe as P  # noqa: E402  (helper(), event timing, the K4 and M33 views)
import mandel_perturb_ref as R  # noqa: E402

B = P.B
ROUNDS = P.ROUNDS
ADAPTIVE = getattr(B, "MANDEL_SUPERSAMPLE_ADAPTIVE", 32)


def views(which):
    k4, bla = P.render_views()
    out = {
        "k1": ("K1 default view F32 M 128", 2000, 2000, dict(max_iter=128), None),
        "k1m1000": ("K1 default view F32 M 1000", 2000, 2000, dict(max_iter=1000), None),
        "k4": (k4[0], P.W, P.H, k4[1], None),
        "bla": (bla[0], P.W, P.H, bla[1], bla[2]),
    }
    if "perturb" in which:
        b = R.mp_boundary_point(("-0.5", "0"), ("-0.5", "1"), 20000, 172, 236)
        out["perturb"] = ("PERTURB boundary 1e-50", P.W, P.H, dict(max_iter=20000, precision=B.PRECISION_PERTURB, **P.ZERO),
                          lambda: B.Orbit(b[0], b[1], 1e-50, 1e-50 * P.ASPECT, 20000))
    return [out[k] for k in which]


class bound:
    def __init__(self, ctx, make, precision):
        self.ctx, self.make, self.precision, self.o = ctx, make, precision, None

    def __enter__(self):
        if self.make:
            self.o = self.make()
            if self.precision == B.PRECISION_PERTURB_BLA_DEEP:
                self.o.bla_deep()
            self.ctx.bind_mandelbrot_orbit(self.o)

    def __exit__(self, *a):
        if self.o is not None:
            self.ctx.bind_mandelbrot_orbit(None)
            self.o.close()


def alternate(ctx, variants):
    """{name: (best, worst)} of mc_context_last_timing's kernel ms; round 0 is the warm one, every round starts one variant later."""
    best, k = {}, len(variants)
    for r in range(ROUNDS + 1):
        for name, p in variants[r % k:] + variants[:r % k]:
            ctx.mandelbrot_rgba8(p)
            v = ctx.last_timing()[0]
            if r:
                lo, hi = best.get(name, (v, v))
                best[name] = (min(lo, v), max(hi, v))
    return best


def work_ratio(ctx, stream, W, H, s, kw):
    """(refined pixels, adaptive / full iterations, plain / full iterations) from the library's sample plane, the rule in torch."""
    M = kw["max_iter"]
    q = B.supersample_params(B.mandelbrot_params(W, H, supersample=s, **kw))
    q.flags |= B.MANDEL_ITERS_U16
    plane = torch.empty((H * s, W * s), dtype=torch.int16, device="cuda")
    ctx.mandelbrot_device(q, 0, plane.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    n = (plane.view(H, s, W, s).to(torch.int32) & 0xffff)
    del plane
    per_pixel = torch.clamp(n + 1, max=M).sum(dim=(1, 3), dtype=torch.int64)
    a = n[:, 0, :, 0].contiguous()
    del n
    mask = torch.zeros((H, W), dtype=torch.bool, device="cuda")
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            mask[yd, xd] |= a[ys, xs] != a[yd, xd]
    full = int(per_pixel.sum())
    plain = int(torch.clamp(a + 1, max=M).sum(dtype=torch.int64))
    return int(mask.sum()), (plain + int(per_pixel[mask].sum())) / full, plain / full


def whole_section(ctx, stream, which, full_only):
    print("## whole calls: mc_mandelbrot_render_rgba8, mc_context_last_timing kernel ms, best (worst) of "
          f"{ROUNDS} alternating rounds after a warm one" + (" — plain and full supersampling only" if full_only else ""))
    for tag, W, H, kw, make in views(which):
        with bound(ctx, make, kw.get("precision")):
            variants = [("plain", B.mandelbrot_params(W, H, **kw))]
            for s in (2, 4):
                variants.append((f"full s={s}", B.mandelbrot_params(W, H, supersample=s, **kw)))
                if not full_only:
                    variants.append((f"adaptive s={s}", B.mandelbrot_params(W, H, supersample=s, flags=ADAPTIVE, **kw)))
            t = alternate(ctx, variants)
            print(f"{tag}, {W} x {H}: plain {t['plain'][0]:9.3f} ms ({t['plain'][1]:9.3f})")
            for s in (2, 4):
                f = t[f"full s={s}"]
                line = f"    s = {s}: full {f[0]:9.3f} ms ({f[1]:9.3f})"
                if not full_only:
                    a = t[f"adaptive s={s}"]
                    ctx.mandelbrot_rgba8(B.mandelbrot_params(W, H, supersample=s, flags=ADAPTIVE, **kw))
                    refined, pixels = ctx.last_refined()
                    by_rule, work, plain_work = work_ratio(ctx, stream, W, H, s, kw)
                    assert by_rule == refined and pixels == W * H, (by_rule, refined, pixels)   # (the rule in torch against the library's count)
                    line += (f"   adaptive {a[0]:9.3f} ms ({a[1]:9.3f})   adaptive / full: time {a[0] / f[0]:5.3f}, work {work:5.3f} "
                             f"(plain pass {plain_work:5.3f})   refined {refined} of {pixels} = {100 * refined / pixels:5.2f} %")
                print(line, flush=True)


def refine_section(ctx, stream, Hp, cus):
    s_ = stream.cuda_stream
    blocks = cus * 8
    sink = torch.zeros(blocks, dtype=torch.int32, device="cuda")
    tag, kw, _ = P.render_views()[0]
    W, H = P.W, P.H
    print(f"## the refine-list pass alone on the anchor plane of {tag}, {W} x {H} (floor = the read-only pass of tools/mandel_equalise_probe.hip "
          "over the same plane, same rounds)")
    lst = torch.empty(W * H, dtype=torch.int32, device="cuda")
    for nbytes in (2, 4):
        p = B.mandelbrot_params(W, H, flags=B.MANDEL_ITERS_U16 if nbytes == 2 else 0, **kw)
        plane = torch.empty((H, W), dtype=torch.int16 if nbytes == 2 else torch.int32, device="cuda")
        ctx.mandelbrot_device(p, 0, plane.data_ptr(), stream=s_)
        stream.synchronize()
        size = plane.numel() * nbytes
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        t = P.best_of(stream, [("floor", lambda: Hp.probe_read_pass(plane.data_ptr(), size, sink.data_ptr(), blocks, s_)),
                               ("refine", lambda: ctx.test_mandel_refine(plane.data_ptr(), nbytes, W, H, lst.data_ptr(), count.data_ptr(), stream=s_))],
                      rounds=ROUNDS)
        stream.synchronize()
        n = int(count.cpu()[0])
        f, g = t["floor"], t["refine"]
        print(f"uint{8 * nbytes}_t plane {size / 1e6:6.1f} MB: floor {f[0]:7.4f} ms (worst {f[1]:7.4f}) {size / f[0] / 1e6:7.1f} GB/s read; refine list "
              f"{g[0]:7.4f} ms (worst {g[1]:7.4f}) = {g[0] / f[0]:5.2f} x floor; list {n} of {W * H} = {100 * n / (W * H):5.2f} %, "
              f"{n * 4 / 1e6:6.1f} MB written", flush=True)
    npix = W * H
    print(f"## context scratch, K4 {W} x {H}, s = 4, uint16_t counts: full = vec4 {npix * 16 / 1e6:.1f} MB + sample plane {npix * 32 / 1e6:.1f} MB = "
          f"{npix * 48 / 1e6:.1f} MB; adaptive = vec4 {npix * 16 / 1e6:.1f} MB + anchor plane {npix * 2 / 1e6:.1f} MB + list {npix * 4 / 1e6:.1f} MB = "
          f"{npix * 22 / 1e6:.1f} MB (+ RGBA8 {npix * 4 / 1e6:.1f} MB either way)")


def main():
    args = sys.argv[1:]
    which = ["k1", "k1m1000", "k4", "bla", "perturb"]
    if "--views" in args:
        which = args[args.index("--views") + 1].split(",")
    if "--rounds" in args:
        global ROUNDS
        ROUNDS = int(args[args.index("--rounds") + 1])
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# {' '.join(args) or 'whole calls'}: device {name}, {cus} CUs; shader clock under load {ctx.measure_clock():.0f} MHz; "
          f"library {os.environ.get('MC_LIB_PATH', 'this build')}; build {B.build_id()}", flush=True)
    stream = torch.cuda.Stream()
    if "--refine" in args:
        refine_section(ctx, stream, P.helper(), cus)
    else:
        whole_section(ctx, stream, which, "--full-only" in args)
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
