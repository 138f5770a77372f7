"""The reference orbit on the device (mc_mandelbrot_orbit_create_device) against the host constructor (mc_mandelbrot_orbit_create_deep).

Both constructors in one process on one context, alternating, best of ROUNDS: the wall time of the whole call (parsing, the launches,
the reads between them and the table's copy included) and, for the device, mc_context_last_orbit_timing's device_ms and launches.  The
tables are compared bit for bit on every pair.
  * the views whose host times DESIGN.md sections 3.7 and 3.9 record: K4's 1e-8 (M = 50 000), M33 at 1e-1000 (M = 6000) and 1e-2000
    (M = 10 000), the interior view at 1e-1000 (M = 20 000), M33 at 1e-2400 (M = 20 000).
  * a sweep over the limb counts k + 1 = 3, 9, 18, 35, 54, 80, 106, 130 at the interior centre: microseconds per iteration, and the
    multiply-add rate they imply (3 (2 (k + 1))^2 32-bit multiply-adds per iteration).
  * the `auto` threshold of bin/mandelbrot --orbit: the smallest measured limb count from which the device's whole-call time is at
    least 20 % below the host's at that count and at every larger measured one (MI355X boxes differ by more than 10 % in clock).
    On an MI355X:  python tools/mandel_orbit_device_probe.py > profiles/orbit_device_probe.txt"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import mandel_perturb_deep_ref as D  # noqa: E402
import mandel_perturb_ref as R  # noqa: E402

B = entry.load_package().bindings
ROUNDS = 3
ASPECT = 2.0 / 3.0
SWEEP_LIMBS = (3, 9, 18, 35, 54, 80, 106, 130)


def pair(ctx, centre, sx, sy, M, E):
    """Best-of-ROUNDS (host s, device s, device_ms, launches, L, bits), alternating; the tables must be equal."""
    best_h = best_d = best_ms = float("inf")
    for _ in range(ROUNDS):
        t = time.perf_counter()
        h = B.Orbit(centre[0], centre[1], sx, sy, M, E)
        best_h = min(best_h, time.perf_counter() - t)
        t = time.perf_counter()
        d = B.Orbit(centre[0], centre[1], sx, sy, M, E, device=ctx)
        best_d = min(best_d, time.perf_counter() - t)
        ms, launches, limbs = ctx.last_orbit_timing()
        best_ms = min(best_ms, ms)
        if not (h.length == d.length and h.bits == d.bits and np.array_equal(h.table().view(np.uint64), d.table().view(np.uint64))):
            raise SystemExit(f"the device orbit differs from the host orbit: centre {centre}, M {M}, E {E}")
        out = (best_h, best_d, best_ms, launches, h.length, h.bits, limbs)
        h.close()
        d.close()
    return out


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# device {name}, {cus} CUs; host vs device constructor, wall time of the whole call, best of {ROUNDS} alternating; every pair "
          f"of tables equal bit for bit")
    with B.Orbit("-0.1", "0.2", 1.0, 1.0, 200, -3000, device=ctx):   # the code object, the state and the events, once
        pass
    c1000, m1000, e1000 = D.view(D.M33, "1e-1000")
    c2000, m2000, e2000 = D.view(D.M33, "1e-2000")
    c2400, m2400, e2400 = D.view(D.M33, "1e-2400")
    views = [("K4 1e-8", 50000, R.DEEP_CENTRE, 1e-8, 0),
             ("M33 1e-1000", 6000, c1000, m1000[0], e1000),
             ("M33 1e-2000", 10000, c2000, m2000[0], e2000),
             ("interior 1e-1000", 20000, ("-0.1", "0.2"), m1000[0], e1000),
             ("M33 1e-2400", 20000, c2400, m2400[0], e2400)]
    print("# view                 M      L   bits limbs |  host ms | device ms (call)  device_ms launches | device / host")
    for tag, M, centre, mant, E in views:
        th, td, ms, launches, L, bits, limbs = pair(ctx, centre, mant, mant * ASPECT, M, E)
        print(f"{tag:18s} {M:6d} {L:6d} {bits:6d} {limbs:5d} | {th * 1e3:8.2f} | {td * 1e3:16.2f} {ms:10.2f} {launches:8d} | {td / th:6.3f}",
              flush=True)
    print("# sweep: interior centre -0.1 + 0.2i, mantissas (1, 1), scale_exp2 = 136 - 64 k")
    print("# limbs  bits      M |  host ms  us/iter | device ms (call)  device_ms  us/iter launches | device / host | G 32-bit multiply-adds/s")
    rows = []
    for limbs in SWEEP_LIMBS:
        k = limbs - 1
        M = 20000 if limbs <= 18 else 6000 if limbs <= 54 else 3000
        th, td, ms, launches, L, bits, got = pair(ctx, ("-0.1", "0.2"), 1.0, 1.0, M, 136 - 64 * k)
        assert got == limbs and L == M
        rows.append((limbs, th, td))
        mads = 3.0 * (2 * limbs) ** 2 * L
        print(f"{limbs:7d} {bits:5d} {M:6d} | {th * 1e3:8.2f} {th * 1e6 / L:8.3f} | {td * 1e3:16.2f} {ms:10.2f} {ms * 1e3 / L:8.3f} {launches:8d} | "
              f"{td / th:13.3f} | {mads / (ms * 1e-3) / 1e9:8.2f}", flush=True)
    threshold = None
    for i, (limbs, _, _) in enumerate(rows):
        if all(td <= 0.8 * th for _, th, td in rows[i:]):
            threshold = limbs
            break
    print(f"# auto threshold (device at least 20 % below the host from here upward): "
          f"{threshold if threshold is not None else 'none: the device never wins by 20 %'} limbs")
    ctx.close()


if __name__ == "__main__":
    main()
