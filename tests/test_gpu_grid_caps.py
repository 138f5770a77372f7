"""The grid-capped kernels past their cap, where the grid-stride loop repeats ("Past the grid cap").

Thirteen kernels launch at most `compute_units * 8` blocks of 256 lanes and cover the rest of their work in a grid-stride loop or in
per-wave runs.  The other test files keep their shapes small, so a lane there makes one trip at most.  Here every case is sized from the
device's CU count to 2.5 times the threshold it names plus an odd remainder — some lanes make three trips, some two — and asserts that
it is beyond that threshold, so none of them can pass without looping.  Image shapes take a prime width and an odd height: no row, wave
or block boundary coincides with a trip boundary.  Every comparison is an equality, bit for bit, with a numpy restatement that tests/
already holds; the inputs of the data-movement and histogram kernels are synthetic planes."""
import numpy as np
import pytest

import buddhabrot_guided_ref as GR
import buddhabrot_ref as R
import mandel_smooth_equalise_ref as Q
import mandel_smooth_ref as S
from test_gpu_buddhabrot import device_density
from test_gpu_buddhabrot_guided import device_guided, device_importance, to_device

pytestmark = pytest.mark.gpu

# The cap, restated once.  LANES = CUs * 8 * 256 is kBlocksPerCu * kBlock of csrc/buddhabrot.hip (the plain form's grid) and the
# `multiProcessorCount * 8u` blocks of 256 lanes of every other launcher: buddhabrot_tonemap_launch, the four of csrc/postprocess.hip,
# mandelbrot_recolour_launch, mandelbrot_smooth_remap_launch, and hist::geometry's `cus * per_cu` shares of 256 vectors with per_cu <= 8.
# The pooled form's grid is capped once a block's kPoolMinRun * kWavesPerBlock = 512 * 4 samples no longer cover the range:
# CUs * 8 * 2048 samples; only beyond that is a wave's run longer than kPoolMinRun.
BLOCKS_PER_CU, BLOCK, POOL_MIN_RUN, WAVES_PER_BLOCK = 8, 256, 512, 4
WIDTH = 1283          # prime
VIEW = (-0.5, 0.0, 3.0, 2.0)
SMALL = dict(width=48, height=32, view=VIEW)
FORMS = {"plain": 1, "pooled": 2}   # MC_BUDDHA_KERNEL_PLAIN, MC_BUDDHA_KERNEL_POOLED
CHUNK = 1 << 18
N_TILES, ROW_BLOCK = 3, 8
M = 300

_cache = {}


def cached(key, make):
    """make() once per module; what it returns is shared and never written to."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def frozen(a):
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def cus(ctx):
    return ctx.device_info()[1]


def lanes_of(cus):
    return cus * BLOCKS_PER_CU * BLOCK


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- sizes --------------------------------------------------------------------------------------------------------------------------
def plain_samples(cus):
    """2.5 times the plain form's threshold and an odd remainder; asserted beyond it."""
    samples = 5 * lanes_of(cus) // 2 + 77
    assert samples > 2 * lanes_of(cus)                       # the second `at += stride` runs, and for some lanes a third
    return samples


def pooled_samples(cus):
    """1.25 times the pooled form's threshold and an odd remainder, with the launcher's arithmetic: the grid is capped, a run is longer
    than kPoolMinRun and no multiple of 64, the last waves own nothing and one owns a partial run."""
    per_block = POOL_MIN_RUN * WAVES_PER_BLOCK
    threshold = cus * BLOCKS_PER_CU * per_block              # CUs * 16384
    samples = 5 * threshold // 4 + 77
    blocks = min(-(-samples // per_block), cus * BLOCKS_PER_CU)
    waves = blocks * WAVES_PER_BLOCK
    run = -(-samples // waves)
    assert samples > threshold and blocks == cus * BLOCKS_PER_CU
    assert run > POOL_MIN_RUN and run % 64 != 0 and waves * run > samples
    assert samples % run != 0 and -(-samples // run) < waves  # a partial run, and waves behind it that own nothing
    return samples


SIZES = {"plain size": (plain_samples, 24), "pooled size": (pooled_samples, 12)}   # name: (samples of the CU count, max_iter)


def request(cus, size, max_iter=None):
    """The params keywords of a Buddhabrot case: the high word of k changes in the middle of the range."""
    samples = SIZES[size][0](cus)
    kw = dict(SMALL, max_iter=SIZES[size][1] if max_iter is None else max_iter, samples=samples, sample_begin=(5 << 32) - samples // 2)
    assert kw["sample_begin"] >> 32 != (kw["sample_begin"] + samples - 1) >> 32
    return kw


def image_shape(threshold):
    """(W, H) with a prime width, an odd height and more than 2.5 * threshold + 77 granules: an odd total."""
    H = -(-(5 * threshold // 2 + 77) // WIDTH) | 1
    assert WIDTH * H > 5 * threshold // 2 and (WIDTH * H) % 2 == 1 and H % (N_TILES * ROW_BLOCK) != 0
    return WIDTH, H


# ---- 1. Buddhabrot, the uniform instantiation ---------------------------------------------------------------------------------------
def uniform_reference(cus, size):
    def make():
        plane, st = R.density(R.params(**request(cus, size)), chunk=CHUNK)
        return frozen(plane), R.stats_tuple(st)
    return cached(("uniform", size), make)


@pytest.mark.parametrize("size", list(SIZES))
def test_buddhabrot_uniform_equals_the_restatement(ctx, B, cus, size):
    kw = request(cus, size)
    want, ws = uniform_reference(cus, size)
    assert ws[0] == kw["samples"] and ws[1] > 0 and ws[4] > 0 and int(want.max()) < 1 << 31   # (no bin near wrap-around)
    for form, flags in FORMS.items():
        got, gs = device_density(ctx, B, [kw], flags)
        assert gs == ws, (form, gs, ws)
        assert np.array_equal(got, want), (form, int((got != want).sum()))


def test_buddhabrot_blocking_render_at_the_pooled_size(ctx, B, cus):
    kw = request(cus, "pooled size")
    want, ws = uniform_reference(cus, "pooled size")
    plane, st = ctx.buddhabrot(B.buddhabrot_params(**kw))   # flags 0: the shipped form
    assert st.as_tuple() == ws and np.array_equal(plane, want)


@pytest.mark.parametrize("form", list(FORMS))
def test_buddhabrot_prefilled_plane_inside_guard_words(ctx, B, cus, form):
    import torch
    kw = request(cus, "plain size")
    fresh, ws = uniform_reference(cus, "plain size")
    n = fresh.size
    before = np.random.default_rng(11).integers(0, 2 ** 32, n + 32, dtype=np.uint32)
    buf = to_device(before)
    d_stats = torch.zeros(5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.buddhabrot_device(B.buddhabrot_params(flags=FORMS[form], **kw), buf.data_ptr() + 64, d_stats.data_ptr())
    ctx.synchronize()
    after = buf.cpu().numpy().view(np.uint32)
    assert np.array_equal(after[16:16 + n], before[16:16 + n] + fresh.reshape(-1))   # (uint32: wraps as the plane does)
    assert np.array_equal(after[:16], before[:16]) and np.array_equal(after[-16:], before[-16:])
    assert tuple(int(v) for v in d_stats.cpu().numpy().view(np.uint64)) == ws


@pytest.mark.parametrize("form", list(FORMS))
def test_buddhabrot_two_launches_two_streams_one_plane(ctx, B, cus, form):
    """The range in two launches on two streams: every part of the plain form's is beyond its threshold, the pooled form's first part is
    (a capped grid with runs of 513) and its second starts where that one ends."""
    import torch
    size = "plain size" if form == "plain" else "pooled size"
    kw = request(cus, size)
    want, ws = uniform_reference(cus, size)
    N = kw["samples"]
    first = N // 2 if form == "plain" else cus * BLOCKS_PER_CU * POOL_MIN_RUN * WAVES_PER_BLOCK + 77
    if form == "plain":
        assert min(first, N - first) > lanes_of(cus)
    else:
        assert 0 < N - first and -(-first // (cus * BLOCKS_PER_CU * WAVES_PER_BLOCK)) > POOL_MIN_RUN
    parts = [dict(kw, samples=first), dict(kw, samples=N - first, sample_begin=kw["sample_begin"] + first)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got, gs = device_density(ctx, B, parts, FORMS[form], streams=streams)
    for s in streams:
        s.synchronize()
    assert gs == ws and np.array_equal(got, want)


# ---- 2. the importance instantiation ------------------------------------------------------------------------------------------------
def importance_reference(cus, size, g=6, want_plane=True, max_iter=None):
    def make():
        m, plane, st = GR.importance(R.params(**request(cus, size, max_iter)), g, want_plane=want_plane, chunk=CHUNK)
        return frozen(m), (frozen(plane) if want_plane else None), R.stats_tuple(st)
    return cached(("importance", size, g, want_plane, max_iter), make)


@pytest.mark.parametrize("size", list(SIZES))
def test_buddhabrot_importance_equals_the_restatement(ctx, B, cus, size):
    kw = request(cus, size)
    want_map, want_plane, ws = importance_reference(cus, size)
    assert ws[0] == kw["samples"] and ws[4] > 0 and int(want_map.astype(np.uint64).sum()) == ws[4]
    for form, flags in FORMS.items():
        for with_plane in (True, False):
            m, plane, gs = device_importance(ctx, B, [kw], 6, flags, with_plane)
            assert gs == ws, (form, with_plane, gs, ws)
            assert np.array_equal(m, want_map), (form, with_plane, int((m != want_map).sum()))
            assert plane is None or np.array_equal(plane, want_plane), (form, with_plane)


# ---- 3. the guided instantiation ----------------------------------------------------------------------------------------------------
def hottest_first(cus, g, max_iter):
    """The cells of the 2^g x 2^g grid, hottest first, by the restated importance map of the plain size's samples at max_iter: the
    max_iter of the case that uses the list (the cells hottest at 24 hold no sample that escapes within 8)."""
    def make():
        shared = g == 6 and max_iter == SIZES["plain size"][1]   # case 2's reference
        m = importance_reference(cus, "plain size", g, want_plane=shared, max_iter=None if shared else max_iter)[0]
        return frozen(np.argsort(-m.astype(np.int64), kind="stable").astype(np.uint32))
    return cached(("order", g, max_iter), make)


def guided_list(cus, name, size):
    """(list, g) of a guided case at a size (whose max_iter the map is taken at), with what makes it the case it is."""
    stride = lanes_of(cus)                                   # the plain form's, and j_step = stride % n_cells
    if name == "longer than the stride":
        n_cells, g = 3 * stride // 2, 10
        assert stride < n_cells <= 1 << (2 * g) and stride % n_cells == stride
    else:
        n_cells, g = int(name), 6
        assert (n_cells <= 64) == (name in ("3", "64"))      # the two branches of add_mod
        assert n_cells != 64 or stride % n_cells == 0        # 64 cells: j_step is 0; 1000 cells: 288 on 256 CUs
    cells = hottest_first(cus, g, GUIDED_MAX_ITER[size])[:n_cells]
    assert cells.size == n_cells
    return cells, g


GUIDED_MAX_ITER = {"plain size": 24, "pooled size": 8}
LISTS = ["3", "65", "1000", "64", "longer than the stride"]


def guided_reference(cus, size, name, weight=1):
    def make():
        cells, g = guided_list(cus, name, size)
        plane, st = GR.density_guided(R.params(**request(cus, size, GUIDED_MAX_ITER[size])), cells, g, weight, chunk=CHUNK)
        return frozen(plane), R.stats_tuple(st)
    return cached(("guided", size, name, weight), make)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("name", LISTS)
def test_buddhabrot_guided_equals_the_restatement(ctx, B, cus, name, size):
    kw = request(cus, size, GUIDED_MAX_ITER[size])
    cells, g = guided_list(cus, name, size)
    want, ws = guided_reference(cus, size, name)
    assert ws[0] == kw["samples"] and ws[4] > 0 and int(want.max()) < 1 << 31
    for form, flags in FORMS.items():
        got, gs = device_guided(ctx, B, [kw], cells, g, 1, flags)
        assert gs == ws, (form, gs, ws)
        assert np.array_equal(got, want), (form, int((got != want).sum()))


def test_buddhabrot_guided_weight_7(ctx, B, cus):
    kw = request(cus, "plain size")
    cells, g = guided_list(cus, "65", "plain size")
    want, ws = guided_reference(cus, "plain size", "65", weight=7)
    ones, os_ = guided_reference(cus, "plain size", "65")
    assert ws == os_ and np.array_equal(want, ones * np.uint32(7)) and ws[4] > 0   # added counts points, not weight
    for form, flags in FORMS.items():
        got, gs = device_guided(ctx, B, [kw], cells, g, 7, flags)
        assert gs == ws and np.array_equal(got, want), form


# ---- 4. the tone map ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [255, 1 << 20])
def test_tonemap_equals_the_restatement(ctx, B, cus, L):
    import torch
    W, H = image_shape(lanes_of(cus))
    rng = np.random.default_rng(L)
    planes = [rng.integers(0, 2 * L + 2, (H, W)).astype(np.uint32) for _ in range(3)]
    planes[1].reshape(-1)[-5] = 2 ** 32 - 1                  # in the last trip
    maps = [R.sqrt_map(L), rng.integers(0, L + 1, L + 1).astype(np.uint32), np.arange(L + 1, dtype=np.uint32)]
    dev = [to_device(q) for q in planes]
    out = torch.full((H + 2, W, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.buddhabrot_tonemap_device(W, H, *(d.data_ptr() for d in dev), L, *maps, out[1:].data_ptr())
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (got[0] == -7.0).all() and (got[-1] == -7.0).all(), "a write outside the image"
    want = R.tonemap(*planes, L, *maps)
    bad = (bits(got[1:-1]) != bits(want)).any(axis=-1)
    assert not bad.any(), int(bad.sum())


# ---- 5. conversion and assembly -----------------------------------------------------------------------------------------------------
def interleave(full, fill):
    """The tiles a gather leaves on the root, as tests/test_gpu_multi.py and tests/test_gpu_parity.py lay them out: tile t holds the rows r
    with (r // ROW_BLOCK) % N_TILES == t, in order, padded to tile 0's row count with `fill`.  Returns (tiles, padded rows)."""
    H = full.shape[0]
    owner = (np.arange(H) // ROW_BLOCK) % N_TILES
    padded = int((owner == 0).sum())
    tiles = np.full((N_TILES, padded) + full.shape[1:], fill, full.dtype)
    for t in range(N_TILES):
        rows = np.flatnonzero(owner == t)
        tiles[t, :rows.size] = full[rows]
    return tiles, padded


def test_convert_rgba8_equals_the_oracle(ctx, O, cus):
    import torch
    W, H = image_shape(lanes_of(cus))
    rng = np.random.default_rng(21)
    img = rng.uniform(-2.0, 300.0, (H, W, 4)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -25.5, -0.9, 3e9, -3e9, 2.0 ** 31, -2.0 ** 31, 1e10, 2147483520.0, 511.99], np.float32)
    where = rng.random(img.shape) < 0.02
    img[where] = special[rng.integers(0, special.size, int(where.sum()))]
    img.reshape(-1, 4)[-3:] = [[np.nan, 2.0 ** 31, -3e9, 1.0], [280.5, -25.5, np.inf, 0.0], [1e10, 255.9, -np.inf, 7.0]]   # the last trip
    d_in = torch.from_numpy(img).cuda()
    for scale in (1.0, 255.0):
        u8 = O.float_to_rgba8(img, scale).reshape(H, W, 4)
        for rotate in (0, 1):
            out = torch.full((H + 2, W), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.convert_rgba8_device(d_in.data_ptr(), W, H, scale, rotate, out[1:].data_ptr())
            ctx.synchronize()
            got = out.cpu().numpy().view(np.uint8).reshape(H + 2, W, 4)
            assert (got[0] == 0x5a).all() and (got[-1] == 0x5a).all(), "a write outside the image"
            want = O.rotate180(u8, W, H) if rotate else u8
            assert np.array_equal(got[1:-1], want), (scale, rotate, int((got[1:-1] != want).any(axis=-1).sum()))


def test_assemble_rgba8_equals_the_restatement(ctx, O, cus):
    import torch
    W, H = image_shape(lanes_of(cus))
    full = np.random.default_rng(22).integers(0, 256, (H, W, 4), dtype=np.uint8)
    tiles, padded = interleave(full, 0xab)
    d_tiles = torch.from_numpy(tiles).cuda()
    for rotate in (0, 1):
        out = torch.full((H + 2, W), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.assemble_rgba8_device(d_tiles.data_ptr(), W, H, N_TILES, ROW_BLOCK, padded, rotate, out[1:].data_ptr())
        ctx.synchronize()
        got = out.cpu().numpy().view(np.uint8).reshape(H + 2, W, 4)
        assert (got[0] == 0x5a).all() and (got[-1] == 0x5a).all(), "a write outside the image"
        want = O.rotate180(full, W, H) if rotate else full
        assert np.array_equal(got[1:-1], want), (rotate, int((got[1:-1] != want).any(axis=-1).sum()))


@pytest.mark.parametrize("case", ["16-byte pixels", "4-byte pixels, 16-byte rows", "4-byte pixels, odd width"])
def test_deinterleave_rows_equals_the_restatement(ctx, cus, case):
    """The uint4 kernel with one granule per pixel and with W / 4 granules per row (the threshold counts granules: four times the
    pixels), and the uint32_t kernel."""
    import torch
    W, H = image_shape(lanes_of(cus))
    words = 4 if case == "16-byte pixels" else 1
    if case == "4-byte pixels, 16-byte rows":
        W *= 4
    row_granules = W * words * 4 // (4 if case == "4-byte pixels, odd width" else 16)
    assert row_granules * H > 5 * lanes_of(cus) // 2 and (W * words * 4 % 16 == 0) == (case != "4-byte pixels, odd width")
    full = np.random.default_rng(23).integers(-2 ** 31, 2 ** 31, (H, W, words), dtype=np.int64).astype(np.int32)
    tiles, padded = interleave(full, -1412567295)
    d_tiles = torch.from_numpy(tiles).cuda()
    out = torch.full((H + 2, W, words), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    if case != "4-byte pixels, odd width":                   # aligned bases: nothing else sends 16-byte rows to the uint32_t kernel
        assert d_tiles.data_ptr() % 16 == 0 and out[1:].data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ctx.deinterleave_rows_device(d_tiles.data_ptr(), W, H, N_TILES, ROW_BLOCK, padded, 4 * words, out[1:].data_ptr())
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (got[0] == 0x5a5a5a5a).all() and (got[-1] == 0x5a5a5a5a).all(), "a write outside the image"
    assert np.array_equal(got[1:-1], full), int((got[1:-1] != full).sum())


@pytest.mark.parametrize("iters_bytes", [2, 4])
def test_mandelbrot_assemble_equals_the_colour_table(ctx, B, cus, iters_bytes):
    import torch
    W, H = image_shape(lanes_of(cus))
    counts = np.random.default_rng(24 + iters_bytes).integers(0, M + 1, (H, W)).astype(np.uint32)
    counts.reshape(-1)[-2:] = [M, 0]
    tiles, padded = interleave(counts.astype(np.uint16 if iters_bytes == 2 else np.uint32), M)
    d_tiles = torch.from_numpy(tiles.view(np.int16 if iters_bytes == 2 else np.int32)).cuda()
    want = B.colour_lut(M)[counts]
    p = B.mandelbrot_params(W, H, max_iter=M)
    for want_rgba, want_iters in ((True, True), (True, False), (False, True)):
        rgba = torch.full((H + 2, W, 4), -7.0, dtype=torch.float32, device="cuda")
        iters = torch.full((H + 2, W), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.mandelbrot_assemble_device(p, d_tiles.data_ptr(), iters_bytes, N_TILES, ROW_BLOCK, padded, rgba[1:].data_ptr() if want_rgba else 0,
                                       iters[1:].data_ptr() if want_iters else 0)
        ctx.synchronize()
        got_rgba, got_iters = rgba.cpu().numpy(), iters.cpu().numpy()
        for a in (got_rgba, got_iters):
            assert (a[0] == -7).all() and (a[-1] == -7).all(), "a write outside the image"
        if want_rgba:
            bad = (bits(got_rgba[1:-1]) != bits(want)).any(axis=-1)
            assert not bad.any(), (want_iters, int(bad.sum()))
        else:
            assert (got_rgba == -7.0).all()
        if want_iters:
            assert np.array_equal(got_iters[1:-1].view(np.uint32), counts), int((got_iters[1:-1].view(np.uint32) != counts).sum())
        else:
            assert (got_iters == -7).all()


# ---- 6. recolour and smooth remap ---------------------------------------------------------------------------------------------------
def rising(rng, top):
    """A random non-decreasing table of M + 1 entries from 0 .. top that ends at top."""
    t = np.sort(rng.integers(0, top + 1, M + 1)).astype(np.uint32)
    t[M] = top
    return t


@pytest.mark.parametrize("iters_bytes", [2, 4])
def test_recolour_equals_the_restatement(ctx, B, cus, iters_bytes):
    """lut[map[min(n, M)]], as tests/mandel_equalise_ref.py's colour() composes it."""
    import torch
    W, H = image_shape(lanes_of(cus))
    rng = np.random.default_rng(26 + iters_bytes)
    counts = rng.integers(0, M + 40, (H, W)).astype(np.uint32)   # some above M: the clamp
    counts.reshape(-1)[-2:] = [M + 39, 1]
    assert (counts > M).any()
    map_ = rising(rng, M)
    typed = counts.astype(np.uint16 if iters_bytes == 2 else np.uint32)
    d_counts = torch.from_numpy(typed.view(np.int16 if iters_bytes == 2 else np.int32)).cuda()
    rgba = torch.full((H + 2, W, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.mandelbrot_recolour_device(B.mandelbrot_params(W, H, max_iter=M), d_counts.data_ptr(), iters_bytes, map_, rgba[1:].data_ptr())
    ctx.synchronize()
    got = rgba.cpu().numpy()
    assert (got[0] == -7.0).all() and (got[-1] == -7.0).all(), "a write outside the image"
    want = B.colour_lut(M)[map_[np.minimum(counts, M)]]
    bad = (bits(got[1:-1]) != bits(want)).any(axis=-1)
    assert not bad.any(), int(bad.sum())


@pytest.mark.parametrize("outputs", ["ranked", "rgba", "both"])
def test_smooth_remap_equals_the_restatement(ctx, B, cus, outputs):
    import torch
    W, H = image_shape(lanes_of(cus))
    rng = np.random.default_rng(28)
    top = 256 * M
    q = rng.integers(0, top, (H, W)).astype(np.uint32)
    q[rng.random(q.shape) < 0.1] = top                        # interior
    q.reshape(-1)[-3:] = [top, top - 1, 255]
    qmap = rising(rng, top)
    d_q = to_device(q)
    d_r = torch.full((H + 2, W), -7, dtype=torch.int32, device="cuda")
    d_rgba = torch.full((H + 2, W, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = B.mandelbrot_params(W, H, max_iter=M, flags=B.MANDEL_COLOUR_SMOOTH_EQUALISED)
    ctx.mandelbrot_smooth_remap_device(p, d_q.data_ptr(), qmap, d_r[1:].data_ptr() if outputs != "rgba" else 0,
                                       d_rgba[1:].data_ptr() if outputs != "ranked" else 0)
    ctx.synchronize()
    r, rgba = d_r.cpu().numpy(), d_rgba.cpu().numpy()
    for a in (r, rgba):
        assert (a[0] == -7).all() and (a[-1] == -7).all(), "a write outside the image"
    want = Q.remap(q, qmap, M)
    if outputs == "rgba":
        assert (r == -7).all()
    else:
        assert np.array_equal(r[1:-1].view(np.uint32), want), int((r[1:-1].view(np.uint32) != want).sum())
    if outputs == "ranked":
        assert (rgba == -7.0).all()
    else:
        bad = (bits(rgba[1:-1]) != bits(S.colour(want, M, B.colour_lut(M)))).any(axis=-1)
        assert not bad.any(), int(bad.sum())


# ---- 7. the histograms --------------------------------------------------------------------------------------------------------------
def histogram_keys(rng, count, max_iter, top):
    """`count` keys below `top` in stretches of 8192: one value (the wave-uniform path), a few values (the combining rounds), random values
    up to max_iter, random values of which about half lie above max_iter (the clamp) — everywhere in the plane, so in every trip."""
    stretch = 8192
    n = -(-count // stretch)
    kind = rng.integers(0, 4, n)
    high = min(2 * max_iter + 2, top)
    keys = rng.integers(0, max_iter + 1, (n, stretch))
    keys[kind == 0] = rng.integers(0, high, (int((kind == 0).sum()), 1))
    few = rng.integers(0, high, (n, 5))
    pick = rng.integers(0, 5, (n, stretch))
    keys[kind == 1] = np.take_along_axis(few, pick, axis=1)[kind == 1]
    keys[kind == 3] = rng.integers(0, high, (int((kind == 3).sum()), stretch))
    keys = keys.reshape(-1)[:count]
    assert (keys > max_iter).any() and (keys == max_iter).sum() < count // 2
    return keys


ROUTES = {"one LDS range": 1000, "three ranges": 40000, "the global table": (1 << 20) + 5}


@pytest.mark.parametrize("plane,route", [(p, r) for p in ("uint16", "uint32", "smooth") for r in ROUTES
                                         if not (p == "uint16" and ROUTES[r] > 65535)])   # (16-bit counts hold no max_iter above 65535)
def test_histogram_equals_bincount(ctx, B, cus, plane, route):
    import torch
    max_iter = ROUTES[route]
    word = 2 if plane == "uint16" else 4
    per = 16 // word
    nvec = 5 * cus * 2048 // 2                               # 16-byte vectors: above every route's shares * 256
    head, tail = per - 1, per // 2 + 1                       # the base lies one word past a 16-byte boundary
    count = head + nvec * per + tail
    assert nvec > lanes_of(cus) and 0 < head < per and 0 < tail < per
    ranges = -(-(max_iter + 1) // 16384)                     # kHistRangeBins; more than kHistMaxRanges = 64 of them: the global table
    assert (ranges == 1, ranges == 3, ranges > 64) == tuple(route == r for r in ROUTES)
    rng = np.random.default_rng(max_iter + word + len(plane))
    keys = histogram_keys(rng, count, max_iter, 65536 if plane == "uint16" else 1 << 22)
    values = keys * 256 + rng.integers(0, 256, count) if plane == "smooth" else keys
    host = np.zeros(count + 1, np.uint16 if word == 2 else np.uint32)
    host[1:] = values
    d_in = torch.from_numpy(host.view(np.int16 if word == 2 else np.int32)).cuda()
    ptr = d_in.data_ptr() + word
    assert (16 - ptr % 16) % 16 // word == head and (count - head) // per == nvec and count - head - nvec * per == tail
    before = rng.integers(0, 2 ** 32, max_iter + 3, dtype=np.uint32)
    tab = to_device(before)
    torch.cuda.synchronize()
    if plane == "smooth":
        ctx.mandelbrot_smooth_histogram_device(ptr, count, max_iter, tab.data_ptr() + 4)
    else:
        ctx.mandelbrot_histogram_device(ptr, word, count, max_iter, tab.data_ptr() + 4)
    ctx.synchronize()
    after = tab.cpu().numpy().view(np.uint32)
    assert after[0] == before[0] and after[-1] == before[-1], "a write outside the table"
    want = np.bincount(np.minimum(keys, max_iter), minlength=max_iter + 1)
    assert int(want.max()) < 1 << 31 and np.count_nonzero(want) > max_iter // 2
    assert np.array_equal(after[1:-1], before[1:-1] + want.astype(np.uint32)), int((after[1:-1] != before[1:-1] + want.astype(np.uint32)).sum())
