"""Per-pixel sample budgets (mc_pathtrace_render_budgeted and the calls it is made of) measured on one context, by the
method of tools/pt_denoise_probe.py.

1. The target sweep: the reference scene at 900 x 600, n0 = 16, max_level = 4, radius 3, strict, T in 2, 4, 8, 16, 32: the share of every
   level, the mean budget, the device time of the blocking call (mc_context_last_timing, kernels only, best of 3) and the RMSE over RGB of
   the final 0 .. 255 buffer against a 4096-spp strict render.  The default target is the T of lowest RMSE among those whose mean budget
   is at most 64 spp.
2. The claim, at that T: the budgeted render beside plain renders at the spp around its mean budget, and beside the plain render that
   takes the same device time (its spp from the measured time per sample, timed in this process), strict and fast math.
3. The width rule: every round of that chain through the device forms, its list render timed at S = 1, 4 and 16 and at the width the
   launcher picks (HIP events, best of ROUNDS rounds, the variants alternating), and the small kernels of the chain.
    On an MI355X:  python tools/pt_budget_probe.py > profiles/pt_budget_probe.txt"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pt_denoise_probe import B, ROUNDS, best_of, rmse, timed  # noqa: E402

W, H, N0, L, RADIUS = 900, 600, 16, 4, 3
TARGETS = (2.0, 4.0, 8.0, 16.0, 32.0)


def budgeted(ctx, T, mode=B.PT_MATH_STRICT, n0=N0, max_level=L):
    p = B.pathtrace_params(W, H, n0, math_mode=mode)
    b = B.pathtrace_budget_params(max_level=max_level, target=T, radius=RADIUS)
    out, ms = timed(ctx, lambda: ctx.pathtrace_budgeted(p, b))
    per, mean = ctx.last_budget()
    return out, ms, per, mean


def plain(ctx, spp, mode=B.PT_MATH_STRICT):
    return timed(ctx, lambda: ctx.pathtrace(B.pathtrace_params(W, H, spp, math_mode=mode)))


def sweep(ctx, ref):
    print(f"target sweep: {W} x {H}, n0 = {N0}, max_level = {L}, radius {RADIUS}, strict; RMSE against 4096 spp strict; device ms best of 3")
    rows = []
    for T in TARGETS:
        out, ms, per, mean = budgeted(ctx, T)
        share = " ".join(f"{100.0 * c / (W * H):6.2f}" for c in per[:L + 1])
        rows.append((T, rmse(out, ref), mean, ms))
        print(f"    T = {T:5.1f}   share of level 0 .. {L} in %: {share}   mean {mean:7.2f} spp   {ms:8.3f} ms   RMSE {rows[-1][1]:6.3f}", flush=True)
    ok = [r for r in rows if r[2] <= 64.0]
    best = min(ok, key=lambda r: r[1]) if ok else min(rows, key=lambda r: r[2])
    print(f"    default target: T = {best[0]:g} (the lowest RMSE among the mean budgets of at most 64 spp)")
    return best[0]


def claim(ctx, ref, T):
    for mode, name in ((B.PT_MATH_STRICT, "strict"), (B.PT_MATH_FAST, "fast")):
        out, ms, per, mean = budgeted(ctx, T, mode)
        e = rmse(out, ref)
        print(f"the claim, {name}: budgeted T = {T:g}: mean {mean:.2f} spp, {ms:.3f} ms, RMSE {e:.3f}")
        near = sorted({max(2, int(round(mean))), max(2, 2 * int(round(mean / 2))), N0, N0 << L})
        per_spp = None
        for spp in near:
            img, t = plain(ctx, spp, mode)
            per_spp = t / spp
            print(f"    plain {spp:4d} spp  {t:8.3f} ms   RMSE {rmse(img, ref):6.3f}   (budgeted / plain: time {ms / t:5.2f}, RMSE {e / rmse(img, ref):5.2f})", flush=True)
        spp_eq = max(1, int(round(ms / per_spp)))
        for _ in range(2):   # the time per sample from the nearest size, then once more from the result
            img, t = plain(ctx, spp_eq, mode)
            nxt = max(1, int(round(spp_eq * ms / t)))
            if nxt == spp_eq:
                break
            spp_eq = nxt
        img, t = plain(ctx, spp_eq, mode)
        print(f"    plain at equal device time: {spp_eq} spp  {t:8.3f} ms   RMSE {rmse(img, ref):6.3f}   -> budgeted RMSE / plain RMSE at equal time = "
              f"{e / rmse(img, ref):.3f}", flush=True)


def widths(ctx, T):
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    acc, half, enc, work = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    var = torch.empty((H, W), dtype=torch.float32, device="cuda")
    lv = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    zero = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    lst = torch.empty((H, W), dtype=torch.int32, device="cuda")
    counts = torch.zeros(9, dtype=torch.int32, device="cuda")
    scale = float(np.float32(2 * N0) / np.float32(N0 // 2))
    small = [("resolve (pilot encode)", lambda: ctx.pathtrace_budget_resolve_device(W, H, acc.data_ptr(), zero.data_ptr(), enc.data_ptr(), stream=s)),
             ("noise plane", lambda: ctx.pathtrace_noise_device(W, H, half.data_ptr(), scale, enc.data_ptr(), RADIUS, var.data_ptr(), stream=s)),
             ("levels", lambda: ctx.pathtrace_budget_levels_device(W, H, var.data_ptr(), T, L, lv.data_ptr(), stream=s)),
             ("lists (count + scatter)", lambda: ctx.pathtrace_budget_lists_device(W, H, lv.data_ptr(), L, lst.data_ptr(), counts.data_ptr(), stream=s)),
             ("copy 16 B", lambda: work.copy_(acc, non_blocking=True))]
    with torch.cuda.stream(stream):
        ctx.pathtrace_device(B.pathtrace_params(W, H, 2 * N0, sample_end=N0 // 2), acc.data_ptr(), stream=s)
        half.copy_(acc, non_blocking=True)
        ctx.pathtrace_device(B.pathtrace_params(W, H, 2 * N0, sample_begin=N0 // 2, sample_end=N0), acc.data_ptr(), stream=s)
        for _, launch in small[:4]:
            launch()
        stream.synchronize()
        t = best_of(stream, small)
    stream.synchronize()
    print(f"the chain's small kernels at {W} x {H}, T = {T:g} (HIP events, best of {ROUNDS}):")
    for name, _ in small:
        print(f"    {name:26s} {t[name][0]:8.4f} ms (worst {t[name][1]:8.4f})")
    c = counts.cpu().numpy()
    print("the rounds: list render at every width (work on a copy of the plane; same entries, same samples)")
    for r in range(1, L + 1):
        n = int(c[r:].sum())
        if not n:
            continue
        variants = []
        for S in (0, 1, 4, 16):
            p = B.pathtrace_params(W, H, N0 << r, sample_begin=N0 << (r - 1), sample_end=N0 << r, flags=B.pt_force_s(S) if S else 0)
            variants.append((f"S = {S}" if S else "rule", lambda p=p: ctx.pathtrace_list_device(p, lst.data_ptr(), n, 1.0, work.data_ptr(), stream=s)))
        with torch.cuda.stream(stream):
            work.copy_(acc, non_blocking=True)
            t = best_of(stream, variants)
        stream.synchronize()
        samples = n * (N0 << (r - 1))
        line = "   ".join(f"{name}: {t[name][0]:8.3f} ms" for name, _ in variants)
        print(f"    round {r}: {n:7d} entries x {N0 << (r - 1):4d} samples   {line}   ({t['rule'][0] * 1e6 / samples:6.3f} ns per sample by the rule)", flush=True)
    img, tp = plain(ctx, 64)
    print(f"    plain strict render, 64 spp (the pool kernel): {tp:8.3f} ms, {tp * 1e6 / (W * H * 64):6.3f} ns per sample")
    img, tp = timed(ctx, lambda: ctx.pathtrace(B.pathtrace_params(W, H, 64, flags=B.pt_force_s(16))))
    print(f"    plain strict render, 64 spp, round-synchronous S = 16: {tp:8.3f} ms, {tp * 1e6 / (W * H * 64):6.3f} ns per sample")


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# per-pixel sample budgets: device {name}, {cus} CUs; shader clock under load {ctx.measure_clock():.0f} MHz; build {B.build_id()}", flush=True)
    ref = ctx.pathtrace(B.pathtrace_params(W, H, 4096))
    T = sweep(ctx, ref)
    claim(ctx, ref, T)
    widths(ctx, T)
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
