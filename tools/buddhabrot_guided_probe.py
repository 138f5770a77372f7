"""The Buddhabrot's importance map and guided sampling measured on one context: HIP events on one stream, warm
launches, no hardware counters.  A sibling of tools/buddhabrot_probe.py.

  --uniform   (a) one line: the uniform call (mc_buddhabrot_density_device_async, no flag bit) on the default view at 1920 x 1280 with 2^26
              samples in the two configurations of §3.26, best and worst of 5 warm launches.  Run it once per process and per build
              (MC_LIB_PATH names the library), alternating the builds, to see whether the templated kernels left the uniform call alone.
  (default)   (b) for the three zoomed views of §3.27, at M = 1000 and at M = 5000 with min_iter 100: added per millisecond of the uniform
              call and of the guided call over the chain's default list (g = 8, a pilot of 2^24 samples, threshold 1, dilate 1), at 2^22
              and 2^26 samples, with and without the pilot's time; n_cells / G^2; the coverage (the share of a second seed's uniform
              adds, 2^24 samples, that start inside the list); the sample count from which the pilot pays; the blocking chain's own timing.
              (c) the guided call's samples against an all-outside view (the same iterations, zero adds) and its adds per second.
              (d) the pilot with and without a plane, beside the uniform call on the same samples.
    On an MI355X:  python tools/buddhabrot_guided_probe.py > profiles/buddhabrot_guided_probe.txt"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

B = entry.load_package().bindings
W, H = 1920, 1280
CONFIGS = [("M = 1000", dict(max_iter=1000, min_iter=0)), ("M = 5000, min_iter 100", dict(max_iter=5000, min_iter=100))]
VIEWS = [(-0.75, 0.1, 0.2, 0.133), (-1.25, 0.0, 0.1, 0.067), (-0.1592, -1.0317, 0.05, 0.033)]
OUTSIDE = (100.0, 100.0, 3.0, 2.0)
G, PILOT = 8, 1 << 24


def event_ms(stream, launch):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    launch()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1)


def best_of(stream, launch, rounds=3):
    launch()
    stream.synchronize()
    v = [event_ms(stream, launch) for _ in range(rounds)]
    return min(v), max(v)


def uniform_line(ctx, stream):
    plane = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    out = [f"lib={B.build_id()['lib']}  {ctx.measure_clock():.0f} MHz"]
    for tag, kw in CONFIGS:
        p = B.buddhabrot_params(W, H, 1 << 26, **kw)
        lo, hi = best_of(stream, lambda: ctx.buddhabrot_device(p, plane.data_ptr(), 0, stream=stream.cuda_stream), rounds=5)
        out.append(f"{tag}: {lo:.3f} ({hi:.3f})")
    print("  ".join(out), flush=True)


def main():
    ctx = B.Context(0)
    stream = torch.cuda.Stream()
    s_ = stream.cuda_stream
    if "--uniform" in sys.argv:
        uniform_line(ctx, stream)
        ctx.close()
        return
    name, cus, _ = ctx.device_info()
    print(f"# Buddhabrot guided probe: {W} x {H}, default sample window, seed 1; list: g = {G}, pilot 2^24 samples, threshold 1, dilate 1; "
          f"device {name}, {cus} CUs; shader clock under load {ctx.measure_clock():.0f} MHz; build {B.build_id()}; HIP events, best of 3 warm "
          f"launches (worst), no hardware counters", flush=True)
    plane = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    d_map = torch.zeros(1 << (2 * G), dtype=torch.int32, device="cuda")
    stats = torch.zeros(5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def counted(launch):
        stats.zero_()
        torch.cuda.synchronize()
        launch(stats.data_ptr())
        stream.synchronize()
        return [int(v) for v in stats.cpu().numpy().view(np.uint64)]

    for view in VIEWS:
        for tag, kw in CONFIGS:
            print(f"## view {view}, {tag}")
            par = lambda n, v=view, **more: B.buddhabrot_params(W, H, n, view=v, **dict(kw, **more))
            # (d) the pilot: the uniform call, the importance call with a plane, without one
            pilot = par(PILOT)
            ulo, uhi = best_of(stream, lambda: ctx.buddhabrot_device(pilot, plane.data_ptr(), 0, stream=s_))
            mlo, mhi = best_of(stream, lambda: ctx.buddhabrot_importance_device(pilot, G, d_map.data_ptr(), plane.data_ptr(), 0, stream=s_))
            plo, phi = best_of(stream, lambda: ctx.buddhabrot_importance_device(pilot, G, d_map.data_ptr(), 0, 0, stream=s_))
            d_map.zero_()
            pst = counted(lambda ds: ctx.buddhabrot_importance_device(pilot, G, d_map.data_ptr(), 0, ds, stream=s_))
            m = d_map.cpu().numpy().view(np.uint32)
            cells = B.buddhabrot_importance_cells(G, m, 1, 1)
            print(f"    pilot, 2^24 samples: uniform call {ulo:.3f} ms ({uhi:.3f}); importance with a plane {mlo:.3f} ({mhi:.3f}); importance "
                  f"without a plane {plo:.3f} ({phi:.3f}); added {pst[4]}; list {cells.size} of {1 << (2 * G)} cells = "
                  f"{100.0 * cells.size / (1 << (2 * G)):.2f} %", flush=True)
            if not cells.size:
                print("    the list is empty: nothing to guide")
                continue
            # the coverage: a second seed's uniform adds by the cell they start in
            d_map.zero_()
            torch.cuda.synchronize()
            ctx.buddhabrot_importance_device(par(PILOT, seed=2), G, d_map.data_ptr(), 0, 0, stream=s_)
            stream.synchronize()
            m2 = d_map.cpu().numpy().view(np.uint32).astype(np.uint64)
            print(f"    coverage: {100.0 * float(m2[cells].sum()) / max(float(m2.sum()), 1.0):.2f} % of seed 2's {int(m2.sum())} uniform adds (2^24 samples) "
                  f"start inside the list")
            d_cells = torch.from_numpy(cells.view(np.int32).copy()).cuda()
            torch.cuda.synchronize()
            for n in (1 << 22, 1 << 26):
                p = par(n)
                ust = counted(lambda ds: ctx.buddhabrot_device(p, plane.data_ptr(), ds, stream=s_))
                ulo, uhi = best_of(stream, lambda: ctx.buddhabrot_device(p, plane.data_ptr(), 0, stream=s_))
                gst = counted(lambda ds: ctx.buddhabrot_guided_device(p, d_cells.data_ptr(), cells.size, G, 1, plane.data_ptr(), ds, stream=s_))
                glo, ghi = best_of(stream, lambda: ctx.buddhabrot_guided_device(p, d_cells.data_ptr(), cells.size, G, 1, plane.data_ptr(), 0, stream=s_))
                ur, gr, gpr = ust[4] / ulo, gst[4] / glo, gst[4] / (glo + plo)
                print(f"    {n} samples: uniform {ulo:.3f} ms ({uhi:.3f}), added {ust[4]}, {ur:.4e} added/ms | guided {glo:.3f} ms ({ghi:.3f}), "
                      f"added {gst[4]}, points {gst[3]}, skipped {gst[1]}, {gr:.4e} added/ms = {gr / max(ur, 1e-30):.2f} x uniform; with the pilot "
                      f"{gpr:.4e} added/ms = {gpr / max(ur, 1e-30):.2f} x uniform", flush=True)
            # the sample count from which guided + pilot delivers more added per ms than uniform, from the 2^26 figures (time and adds linear in N)
            a_u, e_u, a_g, e_g = ulo / n, ust[4] / n, glo / n, gst[4] / n
            gain = e_g * a_u - e_u * a_g
            print(f"    the pilot pays from {e_u * plo / gain:.3e} samples on" if gain > 0 else "    the pilot never pays: guided added/ms is below uniform's")
            # (c) the same guided samples against an all-outside view: the same iterations, zero adds
            po = par(n, v=OUTSIDE)
            olo, ohi = best_of(stream, lambda: ctx.buddhabrot_guided_device(po, d_cells.data_ptr(), cells.size, G, 1, plane.data_ptr(), 0, stream=s_))
            print(f"    guided, 2^26 samples, all-outside view: {olo:.3f} ms ({ohi:.3f}): the adds cost {glo - olo:.3f} ms = {100 * (glo - olo) / glo:.1f} % "
                  f"of the guided call; {gst[4] / glo * 1e3:.3e} adds/s in the call, {gst[4] / max(glo - olo, 1e-9) * 1e3:.3e} adds/s if they were alone; "
                  f"iterations (points + classification) not counted here", flush=True)
            # the blocking chain, defaults, 2^26 samples
            _, st, info = ctx.buddhabrot_guided(par(n), B.buddhabrot_guide_params())
            k, c = ctx.last_timing()
            print(f"    mc_buddhabrot_render_guided, defaults, 2^26 samples: {k:.3f} ms on the stream (pilot, map copy, list on the host, upload, guided "
                  f"render) + {c:.3f} ms copy out; n_cells {info.n_cells}, added {st.added}, {st.added / k:.4e} added/ms", flush=True)
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
