"""The direct Mandelbrot kernels (F32, DS, F64) on views nothing validates: overflowing, infinite, NaN, negative, denormal and zero
scales and centres.  The three precisions define different outcomes there — a NaN pixel never escapes and never cycles in F32 and F64
(n = M), while ds_compare's if / else chain reports +1 for a NaN (n = 0) — and the fast filters ("|z|^2 >= 0, or NaN"), the cycle exit
(a NaN never compares equal) and the LUT index (n <= M always) are built on exactly these cases.

27 x 19 leaves ragged 8 x 8 tiles; M = 37 leaves a tail in both the U = 8 and the U = 4 block loops; at M = 200 NaN lanes hold a wave
through several fast blocks and Brent reference updates.  Planes are compared with the oracle (F32, DS) and with the numpy float64
restatement (F64); the anchors at the end state the outcomes outright, so that a bug shared with a reference cannot hide."""
import functools

import numpy as np
import pytest

import mandel_f64_ref as R

pytestmark = pytest.mark.gpu

W, H = 27, 19
INF, NAN = float("inf"), float("nan")
VIEWS = {                                              # name: (centre, scale)
    "scale_1e30": ((0.0, 0.0), (1e30, 1e30)),          # c finite, c^2 overflows to inf in the first iteration
    "scale_4e19": ((0.0, 0.0), (4e19, 4e19)),          # c^2 ~ 2^128: some pixels overflow in the first square, some do not
    "scale_6e38": ((0.0, 0.0), (6e38, 6e38)),          # the scale itself is inf in fp32 (and inf + -inf = NaN once split for F64)
    "centre_inf": ((INF, 0.0), (1.0, 1.0)),
    "scale_inf_x": ((0.0, 0.0), (INF, 2.0)),           # (x - 0.5) * inf: +-inf (and NaN in a column with x == 0.5, which 27 columns do not have)
    "centre_nan_y": ((-0.5, NAN), (2.0, 2.0)),
    "scale_denormal": ((-0.5, 0.0), (1e-42, 1e-42)),
    "scale_negative": ((-0.5, 0.1), (-2.5, -2.0)),     # the image mirrored on both axes: an ordinary plane
    "scale_zero": ((0.3, 0.5), (0.0, 0.0)),            # every pixel is the centre
}
PRECISIONS = ("f32", "ds", "f64")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def params(B, precision, view, M, W=W, H=H, **kw):
    centre, scale = VIEWS[view]
    prec = {"f32": B.PRECISION_F32, "ds": B.PRECISION_DS, "f64": B.PRECISION_F64}[precision]
    with np.errstate(all="ignore"):                    # the views overflow on purpose when they are split into (hi, lo) floats
        return B.mandelbrot_params(W, H, max_iter=M, precision=prec, centre=centre, scale=scale, **kw)


@functools.lru_cache(maxsize=None)
def _reference(precision, view, M, W=W, H=H):
    import __graft_entry__ as entry
    O = entry.load_oracle()
    centre, scale = VIEWS[view]
    with np.errstate(all="ignore"):
        if precision == "f64":
            ref = R.mandelbrot_iters_f64(W, H, M, centre, scale)
        else:
            ref = O.mandelbrot_iters(W, H, M, view=O.make_view(centre[0], centre[1], scale[0], scale[1]), precision=int(precision == "ds"))
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("M", [37, 200])
@pytest.mark.parametrize("view", list(VIEWS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_extreme_view_plane_colours_and_u16_counts(ctx, B, O, precision, view, M):
    import torch
    ref = _reference(precision, view, M)
    assert ref.max() <= M
    rgba, it = ctx.mandelbrot(params(B, precision, view, M))
    assert np.array_equal(it, ref), (int((it != ref).sum()), np.unique(it)[:8], np.unique(ref)[:8])
    lut, _ = O.mandel_lut(M)
    assert np.array_equal(bits(rgba), bits(lut[ref]))
    t16 = torch.full((H, W), -1, dtype=torch.int16, device="cuda")
    ctx.mandelbrot_device(params(B, precision, view, M, flags=B.MANDEL_ITERS_U16), 0, t16.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(t16.cpu().numpy().view(np.uint16).astype(np.uint32), ref)


@pytest.mark.parametrize("M", [37, 200])
def test_nan_view_anchor_f32_and_f64_never_escape_ds_escapes_at_once(ctx, B, M):
    """Stated outright, not through a reference: with a NaN centre F32 and F64 give n == M everywhere (a NaN magnitude is not > 2 and a
    NaN state never equals the Brent reference), DS gives n == 0 everywhere (ds_compare's chain ends in +1 for a NaN)."""
    for precision, want in (("f32", M), ("f64", M), ("ds", 0)):
        _, it = ctx.mandelbrot(params(B, precision, "centre_nan_y", M), want_rgba=False)
        assert it.shape == (H, W) and (it == want).all(), (precision, np.unique(it))
        assert (_reference(precision, "centre_nan_y", M) == want).all(), precision


@pytest.mark.parametrize("precision", PRECISIONS)
def test_negative_scale_anchor_is_an_ordinary_plane(ctx, B, precision):
    """A negative scale mirrors the image: the plane is the positive-scale plane of the mirrored pixel grid's c values, with many
    distinct counts (not a degenerate constant a sign slip would produce)."""
    _, it = ctx.mandelbrot(params(B, precision, "scale_negative", 37), want_rgba=False)
    assert len(np.unique(it)) >= 15, np.unique(it)
    assert len(np.unique(_reference(precision, "scale_negative", 37))) >= 15


@pytest.mark.parametrize("M", [37, 200])
@pytest.mark.parametrize("view", ["scale_6e38", "scale_inf_x"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_nan_lanes_beside_escaping_lanes_in_one_wave(ctx, B, precision, view, M):
    """24 x 16 has a column (and a row) with uv == 0.5 exactly: 0 * inf = NaN there, +-inf beside it.  In F32 the NaN lanes run to M in
    the same waves whose other lanes escape at once — the wave stays for the NaN lanes' sake, through the fast blocks (M = 200: and the
    Brent updates), and the escaped lanes keep their n = 0."""
    w, h = 24, 16
    ref = _reference(precision, view, M, w, h)
    _, it = ctx.mandelbrot(params(B, precision, view, M, w, h), want_rgba=False)
    assert np.array_equal(it, ref), (int((it != ref).sum()), np.unique(it)[:8], np.unique(ref)[:8])
    if precision == "f32":
        n0, nM = int((it == 0).sum()), int((it == M).sum())
        assert n0 + nM == w * h and nM == (39 if view == "scale_6e38" else h) and n0 > 0, (n0, nM)
