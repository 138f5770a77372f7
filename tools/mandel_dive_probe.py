"""Dives: BLA tables built on the device (mc_context_bind_mandelbrot_orbit_tables) against the host builders plus their upload, and one
shared orbit (mc_mandelbrot_orbit_rescale) against an orbit per keyframe.

Part 1, one process, one context, alternating rounds.  Per orbit and table kind, each round times on a fresh table-less copy of the orbit
  * host:   mc_mandelbrot_orbit_bla[_deep] + mc_context_bind_mandelbrot_orbit (the host build, then Z and the table uploaded): the path a
            keyframe takes without the switch, timed here in the same run;
  * device: mc_context_bind_mandelbrot_orbit_tables (Z uploaded, the table built in place), with mc_context_last_table_timing's
            device_ms and launches;
  * bare:   mc_context_bind_mandelbrot_orbit of the copy without any table (Z's upload alone), for what either bind costs besides.
Wall times in ms: the median over ROUNDS, and the spread (max - min).  The device tables are compared with the host's once per case.
Orbits: the escaping K4 orbit (L about 8000) and the interior orbit at M = 200 000, both table kinds.

Part 2, a dive as bin/mandelbrot runs it: 1920 x 1280, perturb-bla, M = 200 000, the interior centre, --zoom 8 1.  The sum of the run's
"keyframe" lines (orbit or rescale, table, bind, render) with the defaults, with each switch alone and with both, alternating, DIVES
rounds: median and spread.
    On an MI355X:  python tools/mandel_dive_probe.py > profiles/mandel_dive_probe.txt"""
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

B = entry.load_package().bindings
APP = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "mandelbrot")
ROUNDS = 7
DIVES = 3
K4 = ("-0.74364388703715870000000000000000", "0.13182590420531198000000000000000")
INTERIOR = ("-0.1", "0.2")


def stats(v):
    return statistics.median(v), max(v) - min(v)


def same(dev, host):
    nan = np.isnan(host)
    return np.array_equal(nan, np.isnan(dev)) and np.array_equal(dev.view(np.uint64)[~nan], host.view(np.uint64)[~nan])


def table_case(ctx, tag, centre, mant, E, M, deep_kind):
    which = B.ORBIT_TABLE_BLA_DEEP if deep_kind else B.ORBIT_TABLE_BLA
    with B.Orbit(centre[0], centre[1], *mant, M, E) as src:
        copy = lambda: src.rescale(*mant, E)                     # the same object without a table
        host, dev, dev_ms, bare = [], [], [], []
        launches = 0
        with copy() as o:                                        # code objects, buffers and events once; and the comparison
            ctx.bind_mandelbrot_orbit(o, device_tables=which)
            got = ctx.bound_bla_deep_table()[:2] if deep_kind else (ctx.bound_bla_table()[0],)
            (o.bla_deep if deep_kind else o.bla)()
            want = o.bla_deep_table() if deep_kind else (o.bla_table(),)
            if not (same(got[0], want[0]) and (not deep_kind or np.array_equal(got[1], want[1]))):
                raise SystemExit(f"{tag}: the device table differs from the host's")
            entries = want[0].shape[0]
        for _ in range(ROUNDS):
            with copy() as o:
                t = time.perf_counter()
                (o.bla_deep if deep_kind else o.bla)()
                ctx.bind_mandelbrot_orbit(o)
                host.append((time.perf_counter() - t) * 1e3)
            with copy() as o:
                t = time.perf_counter()
                ctx.bind_mandelbrot_orbit(o, device_tables=which)
                dev.append((time.perf_counter() - t) * 1e3)
                ms, launches = ctx.last_table_timing()
                dev_ms.append(ms)
            with copy() as o:
                t = time.perf_counter()
                ctx.bind_mandelbrot_orbit(o)
                bare.append((time.perf_counter() - t) * 1e3)
        (h, hs), (d, ds), (k, ks), (b, bs) = stats(host), stats(dev), stats(dev_ms), stats(bare)
        verdict = "yes" if h - d >= 3.0 * max(hs, ds) else "NO"
        print(f"{tag:24s} {'bla_deep' if deep_kind else 'bla':8s} {src.length:7d} {entries:8d} | {h:8.3f} {hs:7.3f} | {d:8.3f} {ds:7.3f} | "
              f"{k:8.3f} {ks:7.3f} {launches:3d} | {b:7.3f} {bs:6.3f} | {h / d:6.1f}x  {verdict}", flush=True)


def dive(extra, workdir):
    r = subprocess.run([APP, "--quiet", "--width", "1920", "--height", "1280", "--precision", "perturb-bla", "--max-iter", "200000",
                        "--centre", INTERIOR[0], INTERIOR[1], "--scale", "1e-200", "1e-200", "--zoom", "8", "1"] + extra,
                       capture_output=True, text=True, cwd=workdir, timeout=240)
    if r.returncode != 0:
        raise SystemExit(f"bin/mandelbrot {' '.join(extra)} exited {r.returncode}:\n{r.stdout}{r.stderr}")
    keys = [float(m) for m in re.findall(r"^keyframe \d+ of \d+: .*?, ([0-9.]+) ms \(kernels", r.stdout, flags=re.M)]
    kernels = [float(m) for m in re.findall(r"\(kernels ([0-9.]+) ms\)", r.stdout)]
    if len(keys) != 9:
        raise SystemExit(f"expected 9 keyframe lines:\n{r.stdout}")
    return sum(keys), sum(kernels)


def main():
    ctx = B.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"# device {name}, {cus} CUs; wall ms, median and spread (max - min) of {ROUNDS} alternating rounds in one process")
    print("# host = host build + bind (Z and table uploaded); device = bind with the table built in place; bare = bind of Z alone")
    print("# 'beats' = host - device >= 3 x the larger spread")
    print("# orbit                    table          L  entries |  host ms  spread | device ms spread | device_ms spread launches |"
          "  bare ms spread | host/device beats")
    m200, e200 = B.scale_from_text("1e-200")
    for tag, centre, mant, E, M in (("K4 2^-100 (escaping)", K4, (1.0, 0.75), -100, 20000),
                                    ("interior 1e-200", INTERIOR, (m200, m200), e200, 200000)):
        for deep_kind in (False, True):
            table_case(ctx, tag, centre, mant, E, M, deep_kind)
    ctx.close()
    print(f"# dive: bin/mandelbrot 1920 x 1280 perturb-bla M 200000 centre {INTERIOR[0]} {INTERIOR[1]} scale 1e-200 --zoom 8 1; the sum of "
          f"the 9 'keyframe' lines, ms; median and spread of {DIVES} alternating rounds (and the render kernels' share of it)")
    configs = [("defaults", []), ("--zoom-orbit shared", ["--zoom-orbit", "shared"]), ("--bla-table device", ["--bla-table", "device"]),
               ("both", ["--zoom-orbit", "shared", "--bla-table", "device"])]
    sums = {tag: [] for tag, _ in configs}
    kern = {tag: [] for tag, _ in configs}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(DIVES):
            for tag, extra in configs:
                s, k = dive(extra, tmp)
                sums[tag].append(s)
                kern[tag].append(k)
    base = statistics.median(sums["defaults"])
    for tag, _ in configs:
        m, sp = stats(sums[tag])
        print(f"{tag:22s} keyframes {m:9.1f} ms  spread {sp:7.1f}  kernels {statistics.median(kern[tag]):8.1f} ms  | {base / m:5.2f}x the defaults",
              flush=True)


if __name__ == "__main__":
    main()
