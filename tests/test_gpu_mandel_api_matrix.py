"""The blocking Mandelbrot entry points against tests/golden/mandel_api_matrix.json, which tests/golden/make_mandel_api_matrix.py recorded
from the library as it was BEFORE csrc/api.hip got one plan for all eight modes: every subset of nine flag bits x three row shapes (and
max_iter == 0 for the eight modes' own flag sets) through eleven doors -- the status, the detail text (or that none was set) and, where
accepted, a SHA-256 of every output -- must come back record for record.  Then the eight modes in turn on ONE context, whose scratch they
share, against the same requests on fresh contexts."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_mandel_api_matrix", os.path.join(GOLDEN, "make_mandel_api_matrix.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "mandel_api_matrix.json")) as f:
        return json.load(f)


def test_fixture_covers_the_modes(recorded):
    """The fixture can catch a change: each of the eight modes' whole-image requests is accepted through mc_mandelbrot_render and
    mc_mandelbrot_render_rgba8 with a hash of its own (the two integer sampled modes may agree on so small an image)."""
    cases = list(R.cases())
    assert recorded["image"] == [R.W, R.H, R.MAX_ITER] and sorted(recorded["doors"]) == sorted(R.DOORS)
    for door in ("render_colours", "rgba8"):
        rec = R.unpack(recorded, door)
        assert len(rec) == len(cases)
        hashes = [rec[cases.index((flags, R.ROWS[0], R.MAX_ITER))] for flags in R.SINGLE_MODE]
        assert all(s == 0 and h for s, _, h in hashes), hashes
        assert len({h for _, _, h in hashes}) >= 7


@pytest.mark.gpu
@pytest.mark.parametrize("door", R.DOORS)
def test_door_answers_as_recorded(B, recorded, door):
    want = R.unpack(recorded, door)
    got = R.record_door(R.load(B.LIB_PATH), door)
    assert len(got) == len(want)
    per_case = len(want) // len(list(R.cases()))
    for i, (case, g, w) in enumerate(zip((c for c in R.cases() for _ in range(per_case)), got, want)):
        assert g == w, f"{door} record {i}: flags {case[0]:#x} rows {case[1]} max_iter {case[2]}: got {g}, recorded {w}"


# ---- the eight modes on one context ------------------------------------------------------------------------
SHAPES = ((16, 8), (37, 19))   # alternating: the scratch buffers grow in the middle of the sequence


def _render(B, L, c, flags, w, h, warm):
    """The mode's whole-image request through mc_mandelbrot_render (colours, and counts where the mode has them) and
    mc_mandelbrot_render_rgba8, [each behind its warm-up]: the bytes of every output."""
    p = B.mandelbrot_params(w, h, max_iter=48, flags=flags)
    rgba, u8 = np.full((h, w, 4), -7.0, np.float32), np.full((h, w, 4), 0xA5, np.uint8)
    counts = None if flags & R.SUPERSAMPLE_2 else np.full((h, w), 0xA5A5A5A5, np.uint32)
    if warm:
        assert L.mc_context_warmup_mandelbrot(c._h, C.byref(p), 0) == 0
    B._check(L.mc_mandelbrot_render(c._h, C.byref(p), B._ptr(rgba), B._ptr(counts)), "mc_mandelbrot_render")
    if warm:
        assert L.mc_context_warmup_mandelbrot(c._h, C.byref(p), 1) == 0
    B._check(L.mc_mandelbrot_render_rgba8(c._h, C.byref(p), B._ptr(u8)), "mc_mandelbrot_render_rgba8")
    return rgba.tobytes() + u8.tobytes() + (b"" if counts is None else counts.tobytes())


@pytest.fixture(scope="module")
def fresh(B):
    """Every (mode, shape) request on a context of its own, rendered once."""
    L = B.lib()
    L.mc_context_warmup_mandelbrot.argtypes = [C.c_void_p, C.POINTER(B.MandelbrotParams), C.c_int]
    out = {}
    for flags in R.SINGLE_MODE:
        for w, h in SHAPES:
            with B.Context(0) as c:
                out[flags, w, h] = _render(B, L, c, flags, w, h, False)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warmed"])
def test_modes_share_one_contexts_scratch(B, fresh, warm):
    L = B.lib()
    order = list(R.SINGLE_MODE) + list(reversed(R.SINGLE_MODE))
    with B.Context(0) as c:
        for i, flags in enumerate(order):
            w, h = SHAPES[i % 2]
            assert _render(B, L, c, flags, w, h, warm) == fresh[flags, w, h], f"step {i}: flags {flags:#x} at {w} x {h} differs from a fresh context's"
