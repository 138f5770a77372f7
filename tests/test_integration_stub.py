"""INTEGRATION.md route B is code, not prose: integration/vulkanComputeApp.h (the replacement of the reference's Vulkan
runtime header) is compiled with the reference's own language level (g++ -std=c++11, Makefile:13) against
include/mc_compute.h, linked to libmc_compute.so, and — on the GPU box — driven through init / preRun / run exactly as
src/main.cpp does; the storage buffers it produces hash like the oracle's."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INTEG = os.path.join(ROOT, "integration")
LIBDIR = os.path.join(ROOT, "vulkan-compute-tests_amd", "lib")
EXE = os.path.join(ROOT, "vulkan-compute-tests_amd", "bin", "stub_check")


def fnv1a(b):
    h = 1469598103934665603
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def build_stub(B):
    assert os.path.exists(B.LIB_PATH)
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + INTEG,
           os.path.join(INTEG, "stub_check.cpp"), "-o", EXE, "-L" + LIBDIR, "-lmc_compute", "-Wl,-rpath," + LIBDIR]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr


def test_route_b_stub_compiles_and_links_as_cxx11(B):
    build_stub(B)
    # the header alone, as the first include of a translation unit (what the reference's apps would see)
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-x", "c++",
                        os.path.join(INTEG, "vulkanComputeApp.h")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    # without a device the stub fails the way the reference does: runtime_error text, EXIT_FAILURE (main.cpp:35-38)
    n = __import__("ctypes").c_int(0)
    if not (B.lib().mc_device_count(__import__("ctypes").byref(n)) == 0 and n.value > 0):
        r = subprocess.run([EXE, "mandelbrot", "16", "16", "8"], capture_output=True, text=True)
        assert r.returncode == 1 and "could not find a HIP device" in r.stdout


@pytest.mark.gpu
def test_route_b_stub_renders_the_oracle_buffers(B, O):
    build_stub(B)
    r = subprocess.run([EXE, "mandelbrot", "96", "64", "128"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lut_f, _ = O.mandel_lut(128)
    ref = lut_f[O.mandelbrot_iters(96, 64, 128)]
    assert r.stdout.split() == ["mandelbrot", str(fnv1a(np.ascontiguousarray(ref, np.float32).tobytes()))]
    r = subprocess.run([EXE, "pathtracer", "48", "32", "8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ref = O.pathtrace(48, 32, 8, math_mode=O.MATH_MC)
    assert r.stdout.split() == ["pathtracer", str(fnv1a(np.ascontiguousarray(ref, np.float32).tobytes()))]


def test_reference_lodepng_bytes_of_the_mandelbrot_image_are_pinned(O):
    """The "bit-identical PNG" half of route B: the reference's own lodepng (oracle/_ref, compiled where it lies) encodes
    the oracle's default Mandelbrot image (256x256, M = 128 -> RGBA8 through the host cast) to a fixed byte stream; its
    SHA-256 is committed, so an identical iteration plane provably yields the identical mandelbrot.png.  The stream itself
    is committed too (tests/golden/mandelbrot_256_M128_lodepng.png): its pixels are checked on every machine, the codec's
    own encode wherever oracle/_ref is built."""
    import hashlib
    import io
    from PIL import Image
    _, lut_u8 = O.mandel_lut(128)
    img = np.ascontiguousarray(lut_u8[O.mandelbrot_iters(256, 256, 128)])
    golden = open(os.path.join(ROOT, "tests", "golden", "mandelbrot_256_M128_lodepng.sha256")).read().split()[0]
    stored = open(os.path.join(ROOT, "tests", "golden", "mandelbrot_256_M128_lodepng.png"), "rb").read()
    assert hashlib.sha256(stored).hexdigest() == golden
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(stored)).convert("RGBA")), img)
    if O.ref_lodepng() is not None:
        png = O.ref_png_encode(img, 256, 256)
        assert np.array_equal(O.ref_png_decode(png), img)
        digest = hashlib.sha256(png).hexdigest()
        assert digest == golden, digest
