"""CPU tests of the drop-in boundary: the C-ABI library loads without a GPU and exports every symbol
include/mc_compute.h declares; POD layouts match the ctypes mirrors; argument validation and error
strings work; the host helpers (PNG writer, x86 cast, tiling arithmetic) are correct.  No compute calls."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import REFERENCE, ROOT


def test_library_exports_every_declared_symbol(B):
    L = B.lib()
    names = B.declared_symbols()
    assert len(names) >= 25
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert L.mc_abi_version() == B.ABI_VERSION == 3


def test_test_hooks_live_in_their_own_library(B):
    """The device self-test hooks (include/mc_compute_test.h) are test infrastructure: exported by libmc_compute_test.so, absent
    from the product library and from the header a binding of the reference reads."""
    names = B.declared_test_symbols()
    assert len(names) == 5
    T = B.test_lib()
    assert not [n for n in names if not hasattr(T, n)]
    assert not [n for n in names if hasattr(B.lib(), n)], "test hooks exported by the product library"
    assert not [n for n in B.declared_symbols() if n.startswith("mc_test_")]
    # ... and the mc_hook_* functions, which run kernels of the product library on a caller's data (the refine list, the device orbit's
    # arithmetic, the fast-block audits mc_hook_mandel_block_audit and mc_hook_mandel_perturb_block_audit)
    hooks = B.declared_hook_symbols()
    assert len(hooks) == 7 and "mc_hook_mandel_block_audit" in hooks and "mc_hook_mandel_perturb_block_audit" in hooks
    assert not [n for n in hooks if not hasattr(T, n)]
    assert not [n for n in hooks if hasattr(B.lib(), n)], "hooks exported by the product library"
    assert not [n for n in B.declared_symbols() if n.startswith("mc_hook_")]
    pub = open(B.HEADER_PATH).read()
    assert "block_audit" not in pub


def test_public_header_offers_no_measurement_switch(B, tmp_path):
    """the header a reference maintainer binds offers precision, math mode, tiling and the sample
    range — none of this repository's A/B switches (forced kernels, the unguarded fast kernels, the contracting Mandelbrot), which
    live with the test hooks in include/mc_compute_test.h under the same bit values the library honours for tools/ and tests/."""
    import re
    pub = re.sub(r"/\*.*?\*/", "", open(B.HEADER_PATH).read(), flags=re.S)
    switches = ["MC_PT_GENERIC_KERNEL", "MC_PT_NO_BOX_KERNEL", "MC_PT_NO_POOL_KERNEL", "MC_PT_NO_FAST_GUARD", "MC_PT_FORCE_S",
                "MC_PT_SCENE_IN_LDS", "MC_PT_SCENE_IN_MEMORY", "MC_MANDEL_FMA"]
    assert not [w for w in switches if w in pub]
    assert "mc_compute_test.h" not in pub and "mc_debug" not in pub
    diag = open(B.TEST_HEADER_PATH).read()
    assert not [w for w in switches if w not in diag]
    # same bit values as the Python mirror the tools use; the test header is plain C too
    src = tmp_path / "flags.c"
    src.write_text('#include <stdio.h>\n#include "mc_compute_test.h"\nint main(void){printf("%u %u %u %u %u %u %u %u %u\\n", (unsigned)MC_MANDEL_FMA,'
                   '(unsigned)MC_PT_GENERIC_KERNEL, (unsigned)MC_PT_NO_BOX_KERNEL, (unsigned)MC_PT_NO_POOL_KERNEL, (unsigned)MC_PT_SCENE_IN_LDS,'
                   '(unsigned)MC_PT_SCENE_IN_MEMORY, (unsigned)MC_PT_NO_FAST_GUARD, (unsigned)MC_PT_FORCE_S(16), (unsigned)MC_MANDEL_ITERS_U16);return 0;}\n')
    exe = tmp_path / "flags"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [B.MANDEL_FMA, B.PT_GENERIC_KERNEL, B.PT_NO_BOX_KERNEL, B.PT_NO_POOL_KERNEL, B.PT_SCENE_IN_LDS, B.PT_SCENE_IN_MEMORY,
                   B.PT_NO_FAST_GUARD, B.pt_force_s(16), B.MANDEL_ITERS_U16]


def test_param_struct_layouts(B, tmp_path):
    """The header is plain C (gcc -std=c99 compiles it) and the ctypes mirrors have the compiler's layout."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mc_compute.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mc_mandelbrot_params),'
                   'offsetof(mc_mandelbrot_params,k_color), offsetof(mc_mandelbrot_params,row_begin),'
                   'offsetof(mc_mandelbrot_params,flags), sizeof(mc_pathtrace_params),'
                   'offsetof(mc_pathtrace_params,math_mode), offsetof(mc_pathtrace_params,row_block));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    mine = [C.sizeof(B.MandelbrotParams), B.MandelbrotParams.k_color.offset, B.MandelbrotParams.row_begin.offset,
            B.MandelbrotParams.flags.offset, C.sizeof(B.PathtraceParams), B.PathtraceParams.math_mode.offset,
            B.PathtraceParams.row_block.offset]
    assert got == mine == [88, 48, 64, 80, 48, 40, 32]


def test_defaults_match_the_reference(B):
    p = B.mandelbrot_params(2000, 2000)
    assert (p.width, p.height, p.max_iter, p.precision) == (2000, 2000, 128, 0)         # main.cpp:20, mandelbrot.comp:40
    assert (p.centre_x_hi, p.centre_y_hi) == (np.float32(-0.445), 0.0)                  # mandelbrot.comp:38
    assert p.scale_x_hi == np.float32(2.34) == np.float32(2.0 + 1.7 * 0.2)
    assert list(p.k_color) == [np.float32(0.1), np.float32(0.7), np.float32(0.6), 0.0]  # mandelbrotApp.h:139
    q = B.pathtrace_params(900, 600, 500)
    assert (q.width, q.height, q.spp, q.sample_begin, q.sample_end, q.max_depth) == (900, 600, 500, 0, 500, 12)
    planes, spheres = B.default_scene()
    assert planes.shape == (72,) and spheres.shape == (36,)
    assert list(planes[:4]) == [-1.0, 0.0, 0.0, np.float32(2.6)] and spheres[16 + 12 - 4] == 0.0
    assert spheres[2 * 12 + 1] == np.float32(1.6) and list(spheres[2 * 12 + 4:2 * 12 + 7]) == [100, 100, 100]


def test_colour_lut_host_function_matches_oracle(B, O):
    for M, kc in ((128, (0.1, 0.7, 0.6, 0.0)), (1000, (0.9, 0.1, 0.3, 0.0))):
        lut = np.empty((M + 1, 4), np.float32)
        kcf = (C.c_float * 4)(*kc)
        assert B.lib().mc_mandelbrot_colour_lut(M, kcf, lut.ctypes.data_as(C.c_void_p)) == 0
        f, _ = O.mandel_lut(M, np.array(kc, np.float32))
        assert np.array_equal(lut.view(np.uint32), f.view(np.uint32))


def test_tile_rows_arithmetic(B):
    L = B.lib()
    assert L.mc_tile_rows(0, 600, 0, 0) == 600 and L.mc_tile_rows(5, 17, 0, 0) == 12
    for H in (600, 601, 70, 16, 5):
        for n in (1, 2, 3, 8):
            blk = 16
            tot = 0
            for rank in range(n):
                rows = [r for r in range(H) if (r // blk) % n == rank]
                got = L.mc_tile_rows(rank * blk, H, blk, n * blk) if rank * blk < H else 0
                assert got == len(rows), (H, n, rank)
                tot += got
            assert tot == H


def test_error_strings_and_argument_validation_without_gpu(B):
    L = B.lib()
    assert L.mc_error_string(0) == b"ok" and b"invalid" in L.mc_error_string(1) and b"device" in L.mc_error_string(2)
    n = C.c_int(-1)
    rc = L.mc_device_count(C.byref(n))
    assert rc in (0, 2)
    assert L.mc_device_count(None) == 1
    assert L.mc_mandelbrot_default_params(1, 1, None) == 1
    assert L.mc_context_synchronize(None) == 1
    assert L.mc_mandelbrot_render(None, None, None, None) == 1
    assert L.mc_pathtrace_render(None, None, None, 0, None, 0, None) == 1
    if rc == 2 or n.value == 0:   # CPU-only container: creating a context must fail loudly, never fall back
        h = C.c_void_p()
        assert L.mc_context_create(0, C.byref(h)) == 2 and not h
        with pytest.raises(B.McError):
            B.Context(0)


def test_round5_entry_points_without_gpu(B):
    """mc_build_id names the sources each kernel family was built from (16 hex digits each; the same ids a checkout anywhere else
    computes: the Makefile leaves the -I paths out of the hashed flags); mc_host_alloc / mc_host_free / mc_context_last_timing validate
    their arguments, and without a device the allocation fails loudly with a NULL pointer — never a pageable stand-in."""
    import re
    L = B.lib()
    assert re.fullmatch(r"pt=[0-9a-f]{16} mandel=[0-9a-f]{16} lib=[0-9a-f]{16} variant=shipped", L.mc_build_id().decode())
    assert set(B.build_id()) == {"pt", "mandel", "lib", "variant"}
    assert L.mc_host_alloc(0, C.byref(C.c_void_p())) == 1 and L.mc_host_alloc(16, None) == 1     # MC_ERR_INVALID_ARGUMENT
    assert L.mc_host_free(None) == 0
    assert L.mc_context_last_timing(None, None, None) == 1
    n = C.c_int(0)
    if not (L.mc_device_count(C.byref(n)) == 0 and n.value > 0):
        p = C.c_void_p(1)
        assert L.mc_host_alloc(4096, C.byref(p)) != 0 and not p.value
        with pytest.raises(B.McError):
            B.HostBuffer((4, 4, 4))


# ---- host helpers -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostutil(B):
    path = os.environ.get("MC_HOSTUTIL_LIB_PATH") or os.path.join(os.path.dirname(B.LIB_PATH), "libmc_hostutil.so")
    H = C.CDLL(path)
    H.mcu_png_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.POINTER(C.c_ubyte)), C.POINTER(C.c_size_t)]
    H.mcu_free.argtypes = [C.c_void_p]
    H.mcu_float_to_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    return H


def _encode(H, img):
    h, w = img.shape[:2]
    out, n = C.POINTER(C.c_ubyte)(), C.c_size_t(0)
    assert H.mcu_png_encode(img.ctypes.data_as(C.c_void_p), w, h, C.byref(out), C.byref(n)) == 0
    data = C.string_at(out, n.value)
    H.mcu_free(out)
    return data


def test_png_writer_round_trips(hostutil, O):
    import io
    from PIL import Image
    rng = np.random.default_rng(0)
    opaque = rng.integers(0, 256, size=(37, 53, 4), dtype=np.uint8); opaque[..., 3] = 255
    translucent = rng.integers(0, 256, size=(5, 3, 4), dtype=np.uint8)
    _, lut_u8 = O.mandel_lut(128)
    mandel = np.ascontiguousarray(lut_u8[O.mandelbrot_iters(200, 120, 128)])
    for img in (opaque, translucent, mandel, np.full((1, 1, 4), 255, np.uint8)):
        data = _encode(hostutil, np.ascontiguousarray(img))
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        dec = np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))
        assert np.array_equal(dec, img)
        if O.ref_lodepng() is not None:      # the reference's own decoder reads our file to the same pixels
            assert np.array_equal(O.ref_png_decode(data), img)
    # chunk CRCs are valid
    pos = 8
    while pos < len(data):
        ln = int.from_bytes(data[pos:pos + 4], "big")
        assert zlib.crc32(data[pos + 4:pos + 8 + ln]) == int.from_bytes(data[pos + 8 + ln:pos + 12 + ln], "big")
        pos += 12 + ln


def test_host_x86_cast_matches_oracle(hostutil, O):
    v = np.concatenate([np.random.default_rng(1).uniform(-600, 600, 5000), [np.nan, np.inf, -np.inf, 2.2e9, -2.2e9, 255.999, -0.999]]).astype(np.float32)
    out = np.empty(v.size, np.uint8)
    hostutil.mcu_float_to_u8(v.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), v.size)
    quad = np.zeros((v.size, 4), np.float32); quad[:, 0] = v
    assert np.array_equal(out, O.float_to_rgba8(quad, 1.0)[:, 0])


def test_host_storage_conversion_equals_the_reference_loops(hostutil, O):
    """The apps' host post-process (round 5: row stripes on all cores, conversion and rotation in ONE pass) against the reference's two
    serial loops as the oracle restates them — getRenderedImage's cast (mandelbrotApp.h:159-166, pathtracerApp.h:212-219; x86-64 semantics
    for out-of-range values) and the 180-degree swap loop with its odd-width middle column (pathtracerApp.h:236-243) — for even and odd
    widths, heights below and above one stripe per thread, 1 / 3 / all threads."""
    hostutil.mcu_convert_storage.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_int]
    rng = np.random.default_rng(7)
    for (w, h) in ((64, 48), (51, 34), (7, 5), (333, 211), (1, 40), (2, 17)):
        buf = rng.uniform(-40.0, 300.0, (h, w, 4)).astype(np.float32)
        buf[rng.integers(h), rng.integers(w), :3] = (np.nan, np.inf, -3.0e9)
        for scale in (1.0, 255.0):
            plain = O.float_to_rgba8(buf, scale).reshape(h, w, 4)
            for rotate, expect in ((0, plain), (1, O.rotate180(plain, w, h))):
                for threads in (1, 3, 0):
                    out = np.zeros((h, w, 4), np.uint8)
                    hostutil.mcu_convert_storage(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), w, h, scale, rotate, threads)
                    assert np.array_equal(out, expect), (w, h, scale, rotate, threads)


def test_apps_report_missing_device_like_the_reference(B):
    """main.cpp:35-38: a std::runtime_error is printed and the process exits with EXIT_FAILURE.  On the CPU-only
    container the apps have no device: they must say so and fail (no silent fallback)."""
    n = C.c_int(0)
    if B.lib().mc_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present: covered by the gpu tests")
    bindir = os.path.join(os.path.dirname(os.path.dirname(B.LIB_PATH)), "bin")
    for exe, args in (("pathtracer", ["1", "16"]), ("mandelbrot", ["--width", "16", "--height", "16"])):
        r = subprocess.run([os.path.join(bindir, exe)] + args, capture_output=True, text=True, cwd="/tmp")
        assert r.returncode == 1
        assert "starting main!" in r.stdout and "could not find a device" in r.stdout


def test_scene_classification_host_logic(B, O):
    """mc_pathtrace_scene_class exposes the host analysis that selects the path tracer's exact specialisations (slab
    kernels; shadow rays that skip the walls).  The decisions below are the ones the GPU parity tests rely on
    (tests/test_gpu_scenes.py::test_shadow_ray_plane_skip_is_exact renders the same scenes against the oracle)."""
    SLAB, INSIDE, DISJOINT = B.PT_SCENE_SLAB, B.PT_SCENE_LIGHTS_INSIDE, B.PT_SCENE_SPHERES_DISJOINT
    P = O.DEFAULT_PLANES.copy().reshape(6, 12)
    S = O.DEFAULT_SPHERES.copy().reshape(3, 12)
    assert B.pathtrace_scene_class(P, S) == SLAB | INSIDE | DISJOINT   # the reference scene, pathtracerApp.h:14-39
    # bit 2: the three spheres pairwise disjoint with a margin (the fast sample-pool kernel's premise)
    touch = S.copy(); touch[1, 0:3] = touch[0, 0:3] + np.float32([1.6, 0, 0])          # radii 0.8 + 0.8: tangent -> refused
    assert B.pathtrace_scene_class(P, touch) & DISJOINT == 0
    touch[1, 0] += np.float32(0.01)                                                     # 0.01 apart: clears 1e-3 (1 + 1.6)
    assert B.pathtrace_scene_class(P, touch) & DISJOINT == DISJOINT
    nested = S.copy(); nested[2, 0:3] = nested[1, 0:3]                                   # the light inside the glass sphere
    assert B.pathtrace_scene_class(P, nested) & DISJOINT == 0

    def cls(planes, spheres):   # (the cases below are about bits 0 and 1)
        return B.pathtrace_scene_class(planes, spheres) & ~DISJOINT

    def light(**kw):
        s = S.copy()
        for k, v in kw.items():
            s[2, {"x": 0, "y": 1, "z": 2, "r": 3}[k]] = v
        return s
    # margin = 16 sqrt(eps) * scale = 16 * 3.4527e-4 * 7.9 = 0.0436 (pathtrace.hip, lights_inside_box)
    assert cls(P, light(y=1.75)) == SLAB | INSIDE     # 0.05 below the ceiling: clears the margin
    assert cls(P, light(y=1.76)) == SLAB              # 0.04 below: inside the margin -> refused
    assert cls(P, light(y=1.79)) == SLAB              # 0.01 below (taken in round 1; the sphere root of a
                                                                          # grazing shadow ray is only good to ~1e-2 there)
    assert cls(P, light(y=1.95)) == SLAB              # pokes through the ceiling
    assert cls(P, light(x=-2.45, r=0.15)) == SLAB     # touches the left wall
    assert cls(P, light(y=3.5, r=0.3)) == SLAB        # outside the room
    assert cls(P, light(r=0.0)) == SLAB               # degenerate radius
    dark = S.copy(); dark[2, 4:7] = 0
    assert cls(P, dark) == SLAB                       # no emissive sphere: nothing to skip
    two = S.copy(); two[0, 4:7] = (30, 20, 10); two[0, 1] = -1.0         # (as shipped it rests ON the floor: refused)
    on_floor = two.copy(); on_floor[0, 1] = S[0, 1]
    assert cls(P, on_floor) == SLAB
    assert cls(P, two) == SLAB | INSIDE               # every emissive sphere is checked
    two[0, 1] = -1.9                                                      # ... the second light dips through the floor
    assert cls(P, two) == SLAB
    # camera outside the box (front wall moved in front of the pinhole at z = 7.4 - 0.035)
    near = P.copy(); near[5, 3] = 7.0
    assert cls(near, S) == SLAB
    # inverted box: the two x planes swapped offsets so that lo > hi
    inv = P.copy(); inv[0, 3] = -3.0
    assert cls(inv, S) == SLAB
    # not an index-ordered axis-aligned box -> generic kernel
    perm = P[[2, 3, 0, 1, 4, 5]]
    assert B.pathtrace_scene_class(perm, S) == 0
    tilt = P.copy(); tilt[2, :3] = (0.0, 0.99, 0.14)
    assert B.pathtrace_scene_class(tilt, S) == 0
    nan = P.copy(); nan[1, 3] = np.nan
    assert B.pathtrace_scene_class(nan, S) == 0
    assert B.pathtrace_scene_class(P[:5], S) == 0
    # 1 .. 8 spheres take the slab kernels (round 4; the reference loops over spheres.length(), pathTracer.comp:127,403)
    assert B.pathtrace_scene_class(P, S[:2]) == SLAB | DISJOINT                       # (no light: nothing to skip)
    assert B.pathtrace_scene_class(P, S[1:]) == SLAB | INSIDE | DISJOINT
    five = np.concatenate([S, S[:2] + np.float32([0, 0, 2.2] + [0] * 9)])             # two more spheres in front, clear of the others
    MANY = B.PT_SCENE_MANY_SPHERES     # four or more spheres: a fast request is rendered by the careful tier (round 5: five; round 6: four)
    assert B.pathtrace_scene_class(P, five) == SLAB | INSIDE | DISJOINT | MANY
    assert B.pathtrace_scene_class(P, five[:4]) == SLAB | INSIDE | DISJOINT | MANY
    assert B.pathtrace_scene_class(P, five[:3]) == SLAB | INSIDE | DISJOINT          # the reference scene: the fast tier
    # up to three spheres: more specular surface than the reference scene's (one mirror and one glass sphere, r = 0.8: sum r^2 = 0.64 of each
    # kind against 0.65; diffuse walls) -> careful tier
    SPEC = B.PT_SCENE_SPECULAR
    dark = ~S[:, 4:7].any(axis=1)
    for kind in (2, 3):
        (i,) = [i for i in range(3) if int(S[i, 11]) == kind]
        assert abs(float(S[i, 3]) - 0.8) < 1e-6
        bigger = S.copy(); bigger[i, 3] = 0.81
        assert B.pathtrace_scene_class(P, bigger) & SPEC, kind
        smaller = S.copy(); smaller[i, 3] = 0.5
        assert not B.pathtrace_scene_class(P, smaller) & SPEC, kind
        two = S.copy(); two[:, 11] = np.where(dark, kind, S[:, 11]); two[:, 3] = np.where(dark, 0.58, S[:, 3])
        assert B.pathtrace_scene_class(P, two) & SPEC, kind                            # 2 x 0.58^2 = 0.67
        two[:, 3] = np.where(dark, 0.56, S[:, 3])
        assert not B.pathtrace_scene_class(P, two) & SPEC, kind                        # 2 x 0.56^2 = 0.63
        wall = P.copy(); wall[4, 11] = kind
        assert B.pathtrace_scene_class(wall, smaller) & SPEC, kind                     # any specular wall
    assert B.pathtrace_scene_class(tilt, bigger) == SPEC                               # generic scenes, too
    lit = S.copy(); lit[:, 11] = np.where(dark, S[:, 11], 2.0); lit[:, 3] = np.where(dark, 0.3, 0.81)
    assert B.pathtrace_scene_class(P, lit) & SPEC                                      # a light that is a mirror reflects, too (pathTracer.comp:391, :432)
    fastq3 = B.pathtrace_params(300, 200, 500, math_mode=B.PT_MATH_FAST)
    assert B.pathtrace_select_kernel(fastq3, P, bigger).math_mode == B.PT_MATH_FAST_CAREFUL
    assert B.pathtrace_select_kernel(fastq3, wall, S).math_mode == B.PT_MATH_FAST_CAREFUL
    assert B.pathtrace_select_kernel(fastq3, P, S).math_mode == B.PT_MATH_FAST
    assert B.pathtrace_select_kernel(B.pathtrace_params(300, 200, 500, math_mode=B.PT_MATH_FAST, flags=B.PT_NO_FAST_GUARD), wall, bigger).math_mode == B.PT_MATH_FAST
    assert not B.pathtrace_scene_class(P, five) & SPEC                                 # four or more spheres: MANY has decided already
    nine = np.concatenate([S] * 3)
    assert B.pathtrace_scene_class(P, nine) & SLAB == 0                               # beyond 8: the generic kernel
    assert B.pathtrace_scene_class(P, nine) & MANY
    # ... and what mc_pathtrace_select_kernel reports for it: the careful tier runs; the fast tier only when a tool forces it
    fastq = B.pathtrace_params(300, 200, 500, math_mode=B.PT_MATH_FAST)
    assert B.pathtrace_select_kernel(fastq, P, five).math_mode == B.PT_MATH_FAST_CAREFUL
    assert B.pathtrace_select_kernel(fastq, P, five[:4]).math_mode == B.PT_MATH_FAST_CAREFUL
    assert B.pathtrace_select_kernel(fastq, P, five[:3]).math_mode == B.PT_MATH_FAST
    assert B.pathtrace_select_kernel(B.pathtrace_params(300, 200, 500, math_mode=B.PT_MATH_FAST_CAREFUL), P, five[:3]).math_mode == B.PT_MATH_FAST_CAREFUL
    assert B.pathtrace_select_kernel(B.pathtrace_params(300, 200, 500, math_mode=B.PT_MATH_FAST, flags=B.PT_NO_FAST_GUARD), P, five).math_mode == B.PT_MATH_FAST
    assert B.pathtrace_select_kernel(B.pathtrace_params(300, 200, 500), P, five).math_mode == B.PT_MATH_STRICT
    with pytest.raises(B.McError):
        B.pathtrace_select_kernel(B.pathtrace_params(300, 200, 500, math_mode=3), P, five)
    assert B.pathtrace_scene_class(np.zeros((0, 12), np.float32), np.zeros((0, 12), np.float32)) == 0
    # argument validation
    out = C.c_uint32()
    fn = B.lib().mc_pathtrace_scene_class
    assert fn(None, 6, None, 0, C.byref(out)) == 1 and fn(None, 0, None, 0, None) == 1   # MC_ERR_INVALID_ARGUMENT


# The scene tools/fuzz_fast.py found in round 3 (seed 42): light sphere 1 pokes 0.0099 out of the diffuse sphere 2.
ENCLOSED_LIGHT_PLANES = [[-1.0, 0.0, 0.0, 3.028991460800171, 0.0, 0.0, 0.0, 0.0, 0.35169631242752075, 0.34318363666534424, 0.3693005442619324, 1.0], [1.0, 0.0, 0.0, 2.2744364738464355, 0.0, 0.0, 0.0, 0.0, 0.5065174102783203, 0.6979612708091736, 0.37550920248031616, 1.0], [0.0, 1.0, 0.0, 1.999233365058899, 0.0, 0.0, 0.0, 0.0, 0.6414122581481934, 0.12747998535633087, 0.9308241009712219, 1.0], [0.0, -1.0, 0.0, 2.2489571571350098, 0.0, 0.0, 0.0, 0.0, 0.27769729495048523, 0.8655855655670166, 0.46052539348602295, 1.0], [0.0, 0.0, -1.0, 3.2203400135040283, 0.0, 0.0, 0.0, 0.0, 0.26442480087280273, 0.9096760153770447, 0.43677741289138794, 1.0], [0.0, 0.0, 1.0, 8.45179557800293, 0.0, 0.0, 0.0, 0.0, 0.7169037461280823, 0.9640538692474365, 0.3762871026992798, 2.0]]
ENCLOSED_LIGHT_SPHERES = [[1.5096889734268188, 0.9952030181884766, 0.4704371988773346, 0.47152015566825867, 0.0, 0.0, 0.0, 0.0, 0.2772885859012604, 0.8747192621231079, 0.6441940665245056, 1.0], [0.001190655748359859, 0.8120155930519104, -1.2923463582992554, 0.13228453695774078, 55.296485900878906, 51.39237976074219, 106.38571166992188, 0.0, 0.0, 0.0, 0.0, 1.0], [-0.2052173614501953, -0.06327978521585464, -1.4568519592285156, 1.0365451574325562, 0.0, 0.0, 0.0, 0.0, 0.13128790259361267, 0.2444259524345398, 0.9829038977622986, 1.0]]


def test_fast_math_guard_classification_and_kernel_query(B, O):
    """Bit 3 of the scene class — a light (all but) enclosed by an opaque sphere — and what mc_pathtrace_select_kernel reports:
    a fast request on such a scene runs the STRICT kernels (tests/test_gpu_fast_scenes.py renders it against the oracle)."""
    ENC = B.PT_SCENE_LIGHT_ENCLOSED
    P, S = np.float32(ENCLOSED_LIGHT_PLANES), np.float32(ENCLOSED_LIGHT_SPHERES)
    assert B.pathtrace_scene_class(P, S) & ENC
    assert B.pathtrace_scene_class(O.DEFAULT_PLANES, O.DEFAULT_SPHERES) & ENC == 0
    fast = B.pathtrace_params(300, 200, 256, math_mode=B.PT_MATH_FAST)
    k = B.pathtrace_select_kernel(fast, P, S)
    assert k.math_mode == B.PT_MATH_STRICT and k.kernel == B.PT_KERNEL_POOL and k.launches == 1
    assert B.pathtrace_select_kernel(B.pathtrace_params(300, 200, 256, math_mode=B.PT_MATH_FAST_CAREFUL), P, S).math_mode == B.PT_MATH_STRICT
    forced = B.pathtrace_params(300, 200, 256, math_mode=B.PT_MATH_FAST, flags=B.PT_NO_FAST_GUARD)
    assert B.pathtrace_select_kernel(forced, P, S).math_mode == B.PT_MATH_FAST
    # the criterion: how far the light pokes out of the opaque sphere, against its own radius
    big, light = S[2], S[1]
    axis = (light[:3] - big[:3]) / np.linalg.norm(light[:3] - big[:3])

    def with_gap(out, material=1.0, emissive_big=False):
        s = S.copy()
        s[1, :3] = big[:3] + axis * (big[3] - light[3] + out)
        s[2, 11] = material
        if emissive_big:
            s[2, 4:7] = 1.0
            s[0, 4:7] = 1.0     # (the third sphere too: the big light would sit within 1.5 of its radii of it)
        return B.pathtrace_scene_class(P, s) & ENC
    # diffuse: intersecting (out < 2 r) or closer than 1.5 light radii (out < 3.5 r)
    assert with_gap(-0.3) and with_gap(0.0) and with_gap(1.0 * light[3]) and with_gap(2.0 * light[3]) and with_gap(3.4 * light[3])
    assert not with_gap(3.6 * light[3]) and not with_gap(2 * light[3] + 0.5)
    # a mirror: only all but enclosed (out < 0.25 r); glass: never; two lights: never
    assert with_gap(0.01, material=2.0) and with_gap(0.2 * light[3], material=2.0) and not with_gap(0.3 * light[3], material=2.0)
    assert not with_gap(0.01, material=3.0) and not with_gap(0.01, emissive_big=True)
    # any scene, not only slab ones (the generic kernels have the same fast mode)
    assert B.pathtrace_scene_class(P[[2, 3, 0, 1, 4, 5]], S) == ENC | B.PT_SCENE_SPECULAR     # (the fuzz case has a mirror wall)
    # the reference scene: pool kernel in both modes, the round-synchronous kernels for what the pool kernel does not take
    q = B.pathtrace_params(900, 600, 500, math_mode=B.PT_MATH_FAST)
    k = B.pathtrace_select_kernel(q)
    assert (k.kernel, k.lanes_per_pixel, k.math_mode, k.launches) == (B.PT_KERNEL_POOL, 16, B.PT_MATH_FAST, 1)
    q.flags = B.PT_NO_POOL_KERNEL
    k = B.pathtrace_select_kernel(q)
    assert (k.kernel, k.lanes_per_pixel, k.launches) == (B.PT_KERNEL_BOX, 16, 2)          # 500 = 31 x 16 + 4: a second, narrower launch
    q.flags = B.PT_GENERIC_KERNEL
    assert B.pathtrace_select_kernel(q).kernel == B.PT_KERNEL_GENERIC
    q.flags = 2
    with pytest.raises(B.McError):
        B.pathtrace_select_kernel(q)


def _lattice_of_spheres(n):
    """n small diffuse spheres on a 16^3 lattice inside the reference room (0.25 apart, r = 0.02), the first one a light."""
    g = np.arange(16, dtype=np.float32) * np.float32(0.25) - np.float32(1.9)
    s = np.zeros((n, 12), np.float32)
    s[:, 0:3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:n]
    s[:, 3] = 0.02; s[:, 8:11] = 0.5; s[:, 11] = 1.0; s[0, 4:7] = 20.0
    return s


def test_kernel_choice_decision_table(B):
    """mc_pathtrace_select_kernel over a table of requests at K2 (900 x 600 x 500) — the choice the host makes from the request and
    the scene alone: (kernel, lanes per pixel, math mode that runs, launches)."""
    P, S = B.default_scene()
    P, S = np.float32(P).reshape(6, 12), np.float32(S).reshape(-1, 12)
    GEN, SLAB, BOX, POOL, MEM = (B.PT_KERNEL_GENERIC, B.PT_KERNEL_SLAB, B.PT_KERNEL_BOX, B.PT_KERNEL_POOL,
                                 B.PT_KERNEL_GENERIC_MEMORY)
    STRICT, FAST, CAREFUL = B.PT_MATH_STRICT, B.PT_MATH_FAST, B.PT_MATH_FAST_CAREFUL
    glass_wall = P.copy(); glass_wall[4, 11] = 3.0
    tilt = P.copy(); tilt[2, :3] = (0.0, 0.99, 0.14)                                  # a generic scene of 9 objects
    five = np.concatenate([S, S[:2] + np.float32([0, 0, 2.2] + [0] * 9)])
    enclosed = (np.float32(ENCLOSED_LIGHT_PLANES), np.float32(ENCLOSED_LIGHT_SPHERES))
    table = [   # (request, scene or None for the reference scene, expected)
        (dict(math_mode=STRICT), None, (POOL, 16, STRICT, 1)),
        (dict(math_mode=FAST), None, (POOL, 16, FAST, 1)),
        (dict(math_mode=CAREFUL), None, (POOL, 16, CAREFUL, 1)),
        (dict(math_mode=FAST, flags=B.PT_NO_POOL_KERNEL), None, (BOX, 16, FAST, 2)),          # 500 = 31 x 16 + 4
        (dict(math_mode=STRICT, flags=B.PT_NO_POOL_KERNEL), None, (SLAB, 16, STRICT, 2)),
        (dict(math_mode=FAST, flags=B.PT_NO_BOX_KERNEL), None, (SLAB, 16, FAST, 2)),
        (dict(math_mode=FAST, flags=B.PT_GENERIC_KERNEL), None, (GEN, 16, FAST, 2)),
        (dict(math_mode=FAST, flags=B.pt_force_s(4)), None, (BOX, 4, FAST, 1)),
        (dict(math_mode=FAST, row_begin=1), None, (BOX, 16, FAST, 2)),                        # wave tiles unaligned: not the pool
        (dict(math_mode=STRICT, row_begin=1), None, (POOL, 16, STRICT, 1)),                   # (strict adds in sample order)
        (dict(math_mode=FAST, max_depth=0), None, (BOX, 16, FAST, 2)),
        (dict(math_mode=FAST, max_depth=65), None, (SLAB, 16, FAST, 2)),                      # no emit_skip_ok, so no box
        (dict(math_mode=FAST, flags=B.PT_NO_FAST_GUARD), (glass_wall, S), (SLAB, 16, FAST, 2)),
        (dict(math_mode=STRICT), (glass_wall, S), (SLAB, 16, STRICT, 2)),
        (dict(math_mode=STRICT, flags=B.pt_precision(1), sample_end=499), None, (GEN, 16, STRICT, 1)),
        (dict(math_mode=FAST, flags=B.pt_precision(2), sample_begin=3, sample_end=13), None, (GEN, 1, FAST, 1)),
        (dict(math_mode=STRICT, flags=B.pt_precision(3) | B.pt_force_s(4), sample_end=17), None, (GEN, 16, STRICT, 1)),
        (dict(math_mode=FAST), (P, _lattice_of_spheres(700)), (GEN, 16, CAREFUL, 2)),
        (dict(math_mode=FAST), (P, _lattice_of_spheres(3500)), (MEM, 16, CAREFUL, 2)),
        (dict(math_mode=FAST, flags=B.PT_SCENE_IN_LDS), (tilt, S), (GEN, 16, FAST, 2)),
        (dict(math_mode=FAST, flags=B.PT_SCENE_IN_MEMORY), (tilt, S), (MEM, 16, FAST, 2)),
        (dict(math_mode=FAST), enclosed, (POOL, 16, STRICT, 1)),
        (dict(math_mode=FAST), (P, five), (POOL, 16, CAREFUL, 1)),
        (dict(math_mode=FAST, flags=B.PT_NO_FAST_GUARD), (P, five), (POOL, 16, FAST, 1)),
    ]
    for kw, scene, want in table:
        k = B.pathtrace_select_kernel(B.pathtrace_params(900, 600, 500, **kw), *(scene or (P, S)))
        assert (k.kernel, k.lanes_per_pixel, k.math_mode, k.launches) == want, (kw, want)
    # beyond the LDS-resident scene store: refused when forced into LDS or given an extended-precision sphere test
    big = _lattice_of_spheres(3500)
    for flags in (B.PT_SCENE_IN_LDS, B.pt_precision(1)):
        with pytest.raises(B.McError, match="exceeds the LDS-resident scene store") as e:
            B.pathtrace_select_kernel(B.pathtrace_params(900, 600, 500, flags=flags), P, big)
        assert e.value.status == 5   # MC_ERR_UNSUPPORTED


def test_apps_reject_values_they_do_not_know(B, tmp_path):
    """VERDICT r5 item 4 (host/main.cpp): `--math` takes strict | fast | careful — anything else (a typo, a mode of another tool) ends the
    run with EXIT_FAILURE before a device is touched, instead of silently rendering strict; the same for --precision,
    --sphere-precision and unknown options.  (No GPU needed: the refusal comes from option parsing.)"""
    bindir = os.path.join(os.path.dirname(os.path.dirname(B.LIB_PATH)), "bin")
    if not os.path.exists(os.path.join(bindir, "pathtracer")):
        pytest.skip("apps not built")
    for app, args, needle in (("pathtracer", ["--math", "carefull"], "not one of strict | fast | careful"),
                              ("pathtracer", ["--math", "precise"], "not one of strict | fast | careful"),
                              ("pathtracer", ["--sphere-precision", "fp32"], "not one of f32 | fp64 | ds | df64"),
                              ("mandelbrot", ["--precision", "double"], "not one of f32 | ds"),
                              ("mandelbrot", ["--no-such-option"], "unknown option"),
                              ("pathtracer", ["--math"], "missing value")):
        r = subprocess.run([os.path.join(bindir, app)] + args, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and needle in r.stdout, (app, args, r.stdout)
        assert "now running app" not in r.stdout
    # the three public modes are accepted by the parser (without a GPU the run then fails at init(), with the device message)
    for mode in ("strict", "fast", "careful"):
        r = subprocess.run([os.path.join(bindir, "pathtracer"), "2", "8", "--math", mode, "--quiet"], capture_output=True, text=True, cwd=tmp_path)
        assert "not one of" not in r.stdout


def test_round6_entry_points_validate_without_gpu(B):
    """mc_context_warmup_*, mc_assemble_rgba8_device_async: NULL contexts / parameters are refused
    with MC_ERR_INVALID_ARGUMENT (1) — no device needed; RCCL is not a link dependency of the library any more (it is loaded on demand
    by mc_multi_create for more than one device)."""
    L = B.lib()
    vp = C.c_void_p
    L.mc_context_warmup_pathtrace.argtypes = [vp, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_int]
    L.mc_context_warmup_mandelbrot.argtypes = [vp, vp, C.c_int]
    assert L.mc_context_warmup_pathtrace(None, None, None, 0, None, 0, 0) == 1
    assert L.mc_context_warmup_mandelbrot(None, None, 0) == 1
    assert L.mc_assemble_rgba8_device_async(None, None, 1, 1, 1, 8, 1, 0, None, None) == 1
    L.mc_mandelbrot_render_banded.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp]
    assert L.mc_mandelbrot_render_banded(None, None, None, None, 64, None, None) == 1
    out = subprocess.check_output(["readelf", "-d", B.LIB_PATH], text=True)
    assert "librccl" not in out and "libamdhip64" in out


def test_host_alloc_refuses_what_the_process_cannot_take(B):
    """mc_host_alloc touches (or pins) every page it hands out: a request beyond MemAvailable / the cgroup's room would end in the
    kernel's out-of-memory killer instead of an error code (16 B x W x H of a mistyped resolution is all it takes).  Refused up front,
    before a page is touched and before any device call — so this holds on a machine without a GPU too."""
    L = B.lib()
    L.mc_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    L.mc_last_error_detail.restype = C.c_char_p
    L.mc_error_string.restype = C.c_char_p
    p = C.c_void_p(1)
    rc = L.mc_host_alloc(1 << 50, C.byref(p))
    assert rc == 6 and p.value is None                       # MC_ERR_OUT_OF_MEMORY, nothing handed out
    assert b"page-locked host memory" in L.mc_error_string(rc)
    detail = L.mc_last_error_detail().decode()
    assert str(1 << 50) in detail and "available to this process" in detail
