"""mc_pathtrace_accel_guides on the host (no GPU): the guide planes through the tree are mc_pathtrace_guides' for the tables the object
was made from, bit for bit - every scene of tests/pt_bvh_ref.py and an open one, at sizes from 1 x 1 to 257 x 130 - and its refusals."""
import ctypes as C

import numpy as np
import pytest

from pt_accel_chain_cases import bits, scene

INVALID = 1
CASES = [("random200", 37, 23), ("random200", 1, 1), ("random200", 257, 130), ("lattice700", 24, 16), ("duplicates", 24, 16),
         ("unboxable", 24, 16), ("one", 24, 16), ("none", 24, 16), ("open", 65, 33), ("random4000", 24, 16)]

_SEEN = {"sphere": 0, "miss": 0, "plane": 0}


@pytest.mark.parametrize("name,W,H", CASES, ids=[f"{n}-{w}x{h}" for n, w, h in CASES])
def test_accel_guides_are_the_table_guides(B, name, W, H):
    planes, spheres = scene(name)
    want_nt, want_pid = B.pathtrace_guides(W, H, planes, spheres)
    with B.PathtraceAccel(planes, spheres) as a:
        nt, pid = a.guides(W, H)
        again = a.guides(W, H)
    assert nt.shape == (H, W, 4) and pid.shape == (H, W, 4)
    assert np.array_equal(bits(pid), bits(want_pid)), (name, int((bits(pid) != bits(want_pid)).any(-1).sum()))
    assert np.array_equal(bits(nt), bits(want_nt)), (name, int((bits(nt) != bits(want_nt)).any(-1).sum()))
    assert np.array_equal(bits(again[0]), bits(nt)) and np.array_equal(bits(again[1]), bits(pid)), "twice: the same bits"
    ids = want_pid[..., 3]
    n_planes = planes.size // 12
    _SEEN["miss"] += int((ids < 0).sum())
    _SEEN["sphere"] += int((ids >= n_planes).sum())
    _SEEN["plane"] += int(((ids >= 0) & (ids < n_planes)).sum())
    # a miss is written as the contract states it
    miss = ids < 0
    if miss.any():
        assert np.array_equal(bits(nt[miss]), bits(np.tile(np.array([0, 0, 0, 1e20], np.float32), (int(miss.sum()), 1))))
        assert np.array_equal(bits(pid[miss]), bits(np.tile(np.array([0, 0, 0, -1], np.float32), (int(miss.sum()), 1))))
    if name == "open":
        assert miss.any() and (~miss).any(), "the open scene has both misses and sphere hits"
    if name in ("random200", "lattice700", "random4000") and W * H > 1:
        assert (ids >= n_planes).any(), "a sphere is some pixel's first hit"


def test_the_cases_cover_spheres_planes_and_misses(B):
    """(runs after the cases above in file order; on its own it makes the two scenes it needs)"""
    if not (_SEEN["sphere"] and _SEEN["miss"] and _SEEN["plane"]):
        for name, W, H in (("random200", 37, 23), ("open", 65, 33)):
            test_accel_guides_are_the_table_guides(B, name, W, H)
    assert _SEEN["sphere"] > 0 and _SEEN["miss"] > 0 and _SEEN["plane"] > 0, _SEEN


def test_misaligned_outputs_are_written_through_a_copy(B):
    W, H = 24, 16
    planes, spheres = scene("random200")
    want_nt, want_pid = B.pathtrace_guides(W, H, planes, spheres)
    raw_nt, raw_pid = np.full(W * H * 4 + 1, -7.0, np.float32), np.full(W * H * 4 + 4, -7.0, np.float32)
    nt, pid = raw_nt[1:], raw_pid[:-4]
    misaligned = [x for x in (nt, pid) if x.ctypes.data % 16]
    assert misaligned, "one output at least does not start on a 16-byte boundary"
    with B.PathtraceAccel(planes, spheres) as a:
        rc = B.lib().mc_pathtrace_accel_guides(a._h, W, H, nt.ctypes.data_as(C.c_void_p), pid.ctypes.data_as(C.c_void_p))
    assert rc == 0
    assert np.array_equal(bits(nt), bits(want_nt).reshape(-1)) and np.array_equal(bits(pid), bits(want_pid).reshape(-1))
    assert raw_nt[0] == -7.0 and (raw_pid[-4:] == -7.0).all()


def test_refusals(B):
    L = B.lib()
    W, H = 8, 4
    nt, pid = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    p_nt, p_pid = nt.ctypes.data_as(C.c_void_p), pid.ctypes.data_as(C.c_void_p)
    live = B.PathtraceAccel(*scene("one"))   # (made before `a` is destroyed: it cannot take the dead object's address)
    a = B.PathtraceAccel(*scene("one"))
    detail = lambda: L.mc_last_error_detail().decode()   # noqa: E731
    assert L.mc_pathtrace_accel_guides(None, W, H, p_nt, p_pid) == INVALID and "NULL" in detail()
    assert L.mc_pathtrace_accel_guides(a._h, 0, H, p_nt, p_pid) == INVALID and "width and height" in detail()
    assert L.mc_pathtrace_accel_guides(a._h, W, 0, p_nt, p_pid) == INVALID and "width and height" in detail()
    assert L.mc_pathtrace_accel_guides(a._h, W, H, None, p_pid) == INVALID and "NULL" in detail()
    assert L.mc_pathtrace_accel_guides(a._h, W, H, p_nt, None) == INVALID and "NULL" in detail()
    assert L.mc_pathtrace_accel_guides(a._h, W, H, p_nt, p_pid) == 0
    dead = C.c_void_p(a._h.value)
    a.close()
    assert L.mc_pathtrace_accel_guides(dead, W, H, p_nt, p_pid) == INVALID and "destroyed" in detail()
    # the device forms check their arguments before they ask for the context: no device is needed to be refused
    p = B.pathtrace_params(W, H, 4)
    d = B.pathtrace_denoise_params(W, H)
    b = B.pathtrace_budget_params()
    out = np.zeros((H, W, 4), np.float32).ctypes.data_as(C.c_void_p)
    calls = {
        "guides_device": lambda h: L.mc_pathtrace_accel_guides_device_async(None, h, W, H, p_nt, p_pid, None),
        "denoised": lambda h: L.mc_pathtrace_render_accel_denoised(None, h, C.byref(p), C.byref(d), out, None),
        "adaptive": lambda h: L.mc_pathtrace_render_accel_denoised_adaptive(None, h, C.byref(p), C.byref(d), 4.0, 3, out, None),
        "list": lambda h: L.mc_pathtrace_render_accel_list_device_async(None, h, C.byref(p), p_nt, 1, 1.0, p_pid, None),
        "budgeted": lambda h: L.mc_pathtrace_render_accel_budgeted(None, h, C.byref(p), C.byref(b), out, None, None),
    }
    for name, call in calls.items():
        assert call(None) == INVALID and "NULL" in detail(), name
        assert call(dead) == INVALID and "destroyed" in detail(), name
        assert call(live._h) == INVALID and "context" in detail(), name
    live.close()
