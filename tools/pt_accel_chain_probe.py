"""What runs behind a render, table form against mc_pathtrace_accel form, on one context: the guides, the denoised and
the noise-guided chain, the budgeted chain and the list render.

900 x 600, strict math, scenes of tools/pt_bvh_probe.py: lattices of 64, 700 and 3500 spheres in the reference room and the random room
of 6000 spheres.  One process; one warm call of each variant, then the best of ROUNDS rounds with the table form and the accel form
alternating (worst in brackets).
  * guides, render of 16 spp, list render: the device forms, HIP events around one call.  The table guides call uploads the records and
    synchronises before it launches, as every call of it does; the accel call reads the object's cached device copy.
  * list render: a random quarter of the pixels, range [16, 32) of spp = 32, on a copy of the [0, 16) accumulator.
  * chains: the blocking calls, their device time from mc_context_last_timing (kernels only; the budgeted chain's includes the read-back
    of the counts): denoised and noise-guided at 16 spp, budgeted at its defaults with n0 = 16.
  * the budgeted chain step by step: the accel form made from the separate device calls (pilot halves, the small kernels, every round's
    list render in both forms on a copy of the plane), HIP events, best of 3: where the chain's time goes.
Each pair of outputs is compared bit for bit.  The last lines give table / accel per scene and measurement, and the guides' break-even
sphere count (log-linear between the two scenes where the ratio crosses 1).
    On an MI355X:  python tools/pt_accel_chain_probe.py > profiles/pt_accel_chain_probe.txt"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import pt_bvh_ref as R  # noqa: E402

B = entry.load_package().bindings
ROUNDS = 5
W, H, SPP = 900, 600, 16


def scenes():
    for n in (64, 700, 3500):
        yield f"lattice {n}", R.ROOM.copy(), R.lattice(n)
    yield ("random room 6000",) + R.random_scene(np.random.default_rng(6000), 6, 6000, 4)


def event_ms(stream, launch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    launch()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(measure_table, measure_accel):
    """One warm call each, then ROUNDS rounds alternating; returns ((best, worst) table, (best, worst) accel)."""
    measure_table(), measure_accel()
    t, a = [], []
    for _ in range(ROUNDS):
        t.append(measure_table())
        a.append(measure_accel())
    return (min(t), max(t)), (min(a), max(a))


def budget_steps(ctx, stream, accel, planes, spheres, b):
    """The budgeted chain of the accel form made from the separate device calls, every step timed (HIP events, best of 3 after one warm
    call); the rounds' list renders in both forms, on a copy of the plane (same entries, same samples)."""
    s = stream.cuda_stream
    n0, L = SPP, b.max_level
    acc, half, enc, work = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    var = torch.empty((H, W), dtype=torch.float32, device="cuda")
    lv = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    zero = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    lst = torch.empty((H, W), dtype=torch.int32, device="cuda")
    counts = torch.zeros(9, dtype=torch.int32, device="cuda")
    scale = float(np.float32(2 * n0) / np.float32(n0 // 2))
    p_a = B.pathtrace_params(W, H, 2 * n0, sample_end=n0 // 2)
    p_b = B.pathtrace_params(W, H, 2 * n0, sample_begin=n0 // 2, sample_end=n0)

    def best3(launch, before=None):
        ts = []
        for k in range(4):
            if before:
                before()
            ms = event_ms(stream, launch)
            if k:
                ts.append(ms)
        return min(ts)

    def small():
        ctx.pathtrace_budget_resolve_device(W, H, acc.data_ptr(), zero.data_ptr(), enc.data_ptr(), stream=s)
        ctx.pathtrace_noise_device(W, H, half.data_ptr(), scale, enc.data_ptr(), b.radius, var.data_ptr(), stream=s)
        ctx.pathtrace_budget_levels_device(W, H, var.data_ptr(), b.target, L, lv.data_ptr(), stream=s)
        ctx.pathtrace_budget_lists_device(W, H, lv.data_ptr(), L, lst.data_ptr(), counts.data_ptr(), stream=s)

    with torch.cuda.stream(stream):
        t_a = best3(lambda: ctx.pathtrace_accel_device(accel, p_a, acc.data_ptr(), stream=s))
        half.copy_(acc, non_blocking=True)
        t_b = best3(lambda: ctx.pathtrace_accel_device(accel, p_b, work.data_ptr(), stream=s), before=lambda: work.copy_(acc, non_blocking=True))
        ctx.pathtrace_accel_device(accel, p_b, acc.data_ptr(), stream=s)
        t_small = best3(small)
        stream.synchronize()
        c = counts.cpu().numpy()
        print(f"    budgeted chain step by step (accel form): pilot [0, {n0 // 2}) {t_a:9.3f}   pilot [{n0 // 2}, {n0}) {t_b:9.3f}   "
              f"encode + noise plane + levels + lists {t_small:7.3f}", flush=True)
        for r in range(1, L + 1):
            n = int(c[r:].sum())
            if not n:
                break
            q = B.pathtrace_params(W, H, n0 << r, sample_begin=n0 << (r - 1), sample_end=n0 << r)
            fresh = lambda: work.copy_(acc, non_blocking=True)   # noqa: E731
            t_t = best3(lambda: ctx.pathtrace_list_device(q, lst.data_ptr(), n, 1.0, work.data_ptr(), planes, spheres, stream=s), before=fresh)
            t_x = best3(lambda: ctx.pathtrace_accel_list_device(accel, q, lst.data_ptr(), n, 1.0, work.data_ptr(), stream=s), before=fresh)
            print(f"        round {r}: {n:7d} entries x {n0 << (r - 1):4d} samples   list render table {t_t:9.3f}   accel {t_x:9.3f}   table / accel = "
                  f"{t_t / t_x:6.2f}", flush=True)
    stream.synchronize()


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# accelerated chains, table form against accel form: device {name}, {cus} CUs; shader clock under load {ctx.measure_clock():.0f} MHz; "
          f"build {B.build_id()}")
    print(f"# {W} x {H}, strict, max_depth 12; one warm call each, best of {ROUNDS} alternating rounds (worst in brackets); ms", flush=True)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    planes_t = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(8)]
    nt_t, pid_t, nt_a, pid_a, acc, work_t, work_a, out = planes_t
    rng = np.random.default_rng(1)
    quarter = np.sort(rng.choice(W * H, W * H // 4, replace=False)).astype(np.uint32)
    rng.shuffle(quarter)
    d_list = torch.from_numpy(quarter.view(np.int32)).cuda()
    d = B.pathtrace_denoise_params(W, H)
    b = B.pathtrace_budget_params()
    p16 = B.pathtrace_params(W, H, SPP)
    p_head = B.pathtrace_params(W, H, 2 * SPP, sample_end=SPP)
    p_list = B.pathtrace_params(W, H, 2 * SPP, sample_begin=SPP, sample_end=2 * SPP)
    ratios = {}
    for label, planes, spheres in scenes():
        accel = B.PathtraceAccel(planes, spheres)
        n = spheres.shape[0]
        info = accel.info()
        print(f"{label}: {n} spheres, {planes.shape[0]} planes; tree: {info['nodes']} nodes, depth {info['depth']}", flush=True)

        def report(what, t, a, same, extra=""):
            ratios.setdefault(what, []).append((n, t[0] / a[0]))
            print(f"    {what:24s} table {t[0]:10.3f} ({t[1]:10.3f})   accel {a[0]:10.3f} ({a[1]:10.3f})   table / accel = {t[0] / a[0]:7.2f}   "
                  f"outputs bit-equal: {same}{extra}", flush=True)

        with torch.cuda.stream(stream):
            # the steps through the device forms
            t, a = alternate(lambda: event_ms(stream, lambda: ctx.pathtrace_guides_device(W, H, nt_t.data_ptr(), pid_t.data_ptr(), planes, spheres, stream=s)),
                             lambda: event_ms(stream, lambda: ctx.pathtrace_accel_guides_device(accel, W, H, nt_a.data_ptr(), pid_a.data_ptr(), stream=s)))
            same = bool(torch.equal(nt_t.view(torch.int32), nt_a.view(torch.int32)) and torch.equal(pid_t.view(torch.int32), pid_a.view(torch.int32)))
            report("guides", t, a, same)
            t, a = alternate(lambda: event_ms(stream, lambda: ctx.pathtrace_device(p16, work_t.data_ptr(), planes=planes, spheres=spheres, stream=s)),
                             lambda: event_ms(stream, lambda: ctx.pathtrace_accel_device(accel, p16, work_a.data_ptr(), stream=s)))
            report(f"render {SPP} spp", t, a, bool(torch.equal(work_t.view(torch.int32), work_a.view(torch.int32))))
            ctx.pathtrace_accel_device(accel, p_head, acc.data_ptr(), stream=s)
            stream.synchronize()

            def list_table():
                work_t.copy_(acc, non_blocking=True)
                return event_ms(stream, lambda: ctx.pathtrace_list_device(p_list, d_list.data_ptr(), quarter.size, 1.0, work_t.data_ptr(), planes, spheres,
                                                                          stream=s))

            def list_accel():
                work_a.copy_(acc, non_blocking=True)
                return event_ms(stream, lambda: ctx.pathtrace_accel_list_device(accel, p_list, d_list.data_ptr(), quarter.size, 1.0, work_a.data_ptr(),
                                                                                stream=s))

            t, a = alternate(list_table, list_accel)
            report(f"list render, 1/4, [{SPP}, {2 * SPP})", t, a, bool(torch.equal(work_t.view(torch.int32), work_a.view(torch.int32))))
        stream.synchronize()
        # the chains: blocking calls, device time of the kernels from the context's timing record
        keep = {}

        def chain(key, call):
            def measure():
                keep[key] = call()
                return ctx.last_timing()[0]
            return measure

        for what, table_call, accel_call in (
                (f"denoised chain, {SPP} spp", lambda: ctx.pathtrace_denoised(p16, d, planes, spheres), lambda: ctx.pathtrace_accel_denoised(accel, p16, d)),
                (f"noise-guided chain, {SPP} spp", lambda: ctx.pathtrace_denoised_adaptive(p16, d, planes=planes, spheres=spheres),
                 lambda: ctx.pathtrace_accel_denoised_adaptive(accel, p16, d)),
                (f"budgeted chain, n0 = {SPP}", lambda: ctx.pathtrace_budgeted(p16, b, planes, spheres), lambda: ctx.pathtrace_accel_budgeted(accel, p16, b))):
            t, a = alternate(chain("t", table_call), chain("a", accel_call))
            extra = ""
            if what.startswith("budgeted"):
                per, mean = ctx.last_budget()
                extra = f"   (levels 0 .. {b.max_level}: {per[:b.max_level + 1]}, mean {mean:.2f} spp)"
            report(what, t, a, bool(np.array_equal(keep["t"].view(np.uint32), keep["a"].view(np.uint32))), extra)
        budget_steps(ctx, stream, accel, planes, spheres, b)
        accel.close()
    for what, rs in ratios.items():
        line = ", ".join(f"{n}: {r:.2f}" for n, r in rs)
        print(f"# {what}: table / accel by sphere count: {line}")
    rs = ratios["guides"]
    even = "not crossed in the range measured"
    for (n0, r0), (n1, r1) in zip(rs, rs[1:]):
        if (r0 - 1.0) * (r1 - 1.0) <= 0.0 and r0 != r1:
            even = f"about {math.exp(math.log(n0) + (math.log(n1) - math.log(n0)) * (1.0 - r0) / (r1 - r0)):.0f} spheres (between {n0} and {n1})"
            break
    if all(r > 1.0 for _, r in rs):
        even = f"below {rs[0][0]} spheres (the tree is ahead on every scene measured)"
    print(f"# guides: break-even: {even}")
    print(f"# shader clock under load at the end {ctx.measure_clock():.0f} MHz", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
