"""Recorder of tests/golden/mandel_api_matrix.json: what the blocking Mandelbrot entry points of ONE build of libmc_compute.so answer
over every subset of nine flag bits, three row shapes and eleven doors -- status, detail text and a SHA-256 of the outputs.

    python tests/golden/make_mandel_api_matrix.py <libmc_compute.so> [<out.json>]

The fixture is recorded from the build BEFORE a change to csrc/api.hip (needs the GPU) and replayed on the build under test by
tests/test_gpu_mandel_api_matrix.py, which imports record() from here.  Plain ctypes: the library to load is an argument.

The detail text is thread-local and a refusal that sets none leaves the previous call's in place, so one fixed call that sets a known
detail (mc_mandelbrot_zoom_create without a context) precedes every recorded call; finding that text afterwards is recorded as NO_DETAIL.
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

W, H, MAX_ITER = 20, 24, 48
EQUALISED, ADAPTIVE, SMOOTH, DISTANCE = 16, 32, 64, 128
SUPERSAMPLE_2, SMOOTH_EQUALISED, SUPERSAMPLE_SMOOTH, SUPERSAMPLE_SMOOTH_ADAPTIVE, ITERS_U16 = 2 << 8, 4096, 8192, 16384, 2
BITS = (EQUALISED, SUPERSAMPLE_2, ADAPTIVE, SMOOTH, DISTANCE, SMOOTH_EQUALISED, SUPERSAMPLE_SMOOTH, SUPERSAMPLE_SMOOTH_ADAPTIVE, ITERS_U16)
# the eight modes' own flag sets, in the order of MandelPlan::Mode
SINGLE_MODE = (0, EQUALISED, SUPERSAMPLE_2, SUPERSAMPLE_2 | ADAPTIVE, DISTANCE, SMOOTH_EQUALISED,
               SUPERSAMPLE_2 | SUPERSAMPLE_SMOOTH | SMOOTH, SUPERSAMPLE_2 | SUPERSAMPLE_SMOOTH_ADAPTIVE | SMOOTH)
ROWS = ((0, H, 0, 0), (8, 16, 0, 0), (0, H, 8, 16))   # (row_begin, row_end, row_block, row_stride): whole, band, interleaved tile
DOORS = ("render_colours", "render_both", "render_counts", "rgba8", "distance", "smooth_equalised", "adaptive_smooth",
         "warmup_0", "warmup_1", "warmup_3", "zoom")
NO_DETAIL = "<no detail set>"
FILL = 0xA5   # every output buffer before every call: what a call leaves unwritten hashes the same


class Params(C.Structure):   # mc_mandelbrot_params (include/mc_compute.h)
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_iter", C.c_uint32), ("precision", C.c_uint32),
                ("view", C.c_float * 8), ("k_color", C.c_float * 4), ("row_begin", C.c_uint32), ("row_end", C.c_uint32),
                ("row_block", C.c_uint32), ("row_stride", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


def load(path):
    L = C.CDLL(path)
    vp, u32, pp = C.c_void_p, C.c_uint32, C.POINTER(Params)
    L.mc_last_error_detail.restype = C.c_char_p
    L.mc_context_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.mc_context_destroy.argtypes = [vp]
    L.mc_context_synchronize.argtypes = [vp]
    L.mc_context_warmup_mandelbrot.argtypes = [vp, pp, C.c_int]
    L.mc_mandelbrot_default_params.argtypes = [u32, u32, pp]
    L.mc_mandelbrot_render.argtypes = [vp, pp, vp, vp]
    L.mc_mandelbrot_render_rgba8.argtypes = [vp, pp, vp]
    L.mc_mandelbrot_render_distance.argtypes = [vp, pp, vp, vp, vp, vp]
    L.mc_mandelbrot_render_smooth_equalised.argtypes = [vp, pp, vp, vp, vp, vp]
    L.mc_mandelbrot_render_adaptive_smooth.argtypes = [vp, pp, u32, vp, vp]
    L.mc_mandelbrot_zoom_create.argtypes = [vp, u32, u32, C.POINTER(vp)]
    L.mc_mandelbrot_zoom_push.argtypes = [vp, pp]
    L.mc_mandelbrot_zoom_frame.argtypes = [vp, C.c_double, vp, vp]
    L.mc_mandelbrot_zoom_destroy.argtypes = [vp]
    return L


def cases():
    """(flags, rows, max_iter) of the matrix, in the fixture's order."""
    for r in range(len(BITS) + 1):
        for subset in itertools.combinations(BITS, r):
            for rows in ROWS:
                yield sum(subset), rows, MAX_ITER
    for flags in SINGLE_MODE:
        yield flags, ROWS[0], 0


def record_door(L, door):
    """The door's records over cases(): a list of (status, detail, sha256 hex of the outputs or None)."""
    ctx = C.c_void_p()
    if L.mc_context_create(0, C.byref(ctx)) != 0:
        raise RuntimeError("mc_context_create failed: " + L.mc_last_error_detail().decode())
    npix = W * H
    f32, n, q, third, u8 = (C.create_string_buffer(npix * b) for b in (16, 4, 4, 4, 4))
    out = []

    def call(fn, *args, buffers=()):
        for b in buffers:
            C.memset(b, FILL, len(b))
        nothing = C.c_void_p()
        L.mc_mandelbrot_zoom_create(None, 1, 1, C.byref(nothing))   # the known detail
        sentinel = L.mc_last_error_detail()
        status = fn(*args)
        detail = L.mc_last_error_detail()
        digest = None
        if status == 0 and buffers:
            h = hashlib.sha256()
            for b in buffers:
                h.update(b.raw)
            digest = h.hexdigest()
        out.append((status, NO_DETAIL if detail == sentinel else detail.decode(), digest))
        return status

    try:
        for flags, (rb, re, blk, stride), max_iter in cases():
            p = Params()
            L.mc_mandelbrot_default_params(W, H, C.byref(p))
            p.max_iter, p.flags = max_iter, flags
            p.row_begin, p.row_end, p.row_block, p.row_stride = rb, re, blk, stride
            P = C.byref(p)
            if door == "render_colours":
                call(L.mc_mandelbrot_render, ctx, P, f32, None, buffers=(f32,))
            elif door == "render_both":
                call(L.mc_mandelbrot_render, ctx, P, f32, n, buffers=(f32, n))
            elif door == "render_counts":
                call(L.mc_mandelbrot_render, ctx, P, None, n, buffers=(n,))
            elif door == "rgba8":
                call(L.mc_mandelbrot_render_rgba8, ctx, P, u8, buffers=(u8,))
            elif door == "distance":
                call(L.mc_mandelbrot_render_distance, ctx, P, f32, n, q, third, buffers=(f32, n, q, third))
            elif door == "smooth_equalised":
                call(L.mc_mandelbrot_render_smooth_equalised, ctx, P, f32, n, q, third, buffers=(f32, n, q, third))
            elif door == "adaptive_smooth":
                call(L.mc_mandelbrot_render_adaptive_smooth, ctx, P, 256, f32, None, buffers=(f32,))
            elif door.startswith("warmup_"):
                call(L.mc_context_warmup_mandelbrot, ctx, P, int(door[-1]))
                call(L.mc_context_synchronize, ctx)
            elif door == "zoom":
                z = C.c_void_p()
                if L.mc_mandelbrot_zoom_create(ctx, W, H, C.byref(z)) != 0:
                    raise RuntimeError("mc_mandelbrot_zoom_create failed: " + L.mc_last_error_detail().decode())
                call(L.mc_mandelbrot_zoom_push, z, P)
                call(L.mc_mandelbrot_zoom_frame, z, 1.0, f32, u8, buffers=(f32, u8))
                L.mc_mandelbrot_zoom_destroy(z)
            else:
                raise ValueError(door)
    finally:
        L.mc_context_destroy(ctx)
    return out


def pack(per_door):
    """{door: records} as the fixture: every string, hash and (status, detail, hash) triple once, the doors as lists of triple indices."""
    details, hashes, triples = [], [], []

    def index(table, v):
        if v not in table:
            table.append(v)
        return table.index(v)

    doors = {}
    for door, records in per_door.items():
        doors[door] = [index(triples, [s, index(details, d), -1 if h is None else index(hashes, h)]) for s, d, h in records]
    return {"image": [W, H, MAX_ITER], "details": details, "hashes": hashes, "records": triples, "doors": doors}


def unpack(fixture, door):
    t = fixture
    return [(s, t["details"][d], None if h < 0 else t["hashes"][h]) for s, d, h in (t["records"][i] for i in t["doors"][door])]


def main(argv):
    lib = argv[1]
    dest = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "mandel_api_matrix.json")
    L = load(lib)
    fixture = pack({door: record_door(L, door) for door in DOORS})
    with open(dest, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in fixture.items()) + "\n}\n")
    accepted = sum(1 for door in DOORS for s, _, _ in unpack(fixture, door) if s == 0)
    print(f"{dest}: {sum(len(v) for v in fixture['doors'].values())} records, {accepted} accepted, {len(fixture['details'])} detail texts, "
          f"{len(fixture['hashes'])} hashes")


if __name__ == "__main__":
    main(sys.argv)
