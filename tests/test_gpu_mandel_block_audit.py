"""The per-lane promise of the escape loop's fast block, audited on the MI355X (mc_hook_mandel_block_audit,
mc_hook_mandel_perturb_block_audit; csrc/mandel_block_audit.h).  Each of the five states promises: when needs_exact of a block is
false, no iteration of it escaped and the state after the fast iterations equals the state after as many exact steps, bit for bit.  The
iteration-plane tests cannot see a lane that breaks it while a neighbour of its 8 x 8 tile raises the flag in the same block (both are
replayed exactly); here every lane runs alone.  Per case: no bad block; n is the state's reference plane and the shipped render's;
per state both outcomes occur; and with the filter switched off (sabotage) the audit reports what the filter is there to catch.
The cases are tests/mandel_block_audit_cases.py's; tests/test_mandel_block_audit_host.py counts on the CPU which branches they reach."""
import ctypes as C

import numpy as np
import pytest

import mandel_block_audit_cases as K
import mandel_f64_ref as F
import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R

pytestmark = pytest.mark.gpu

NONE = K.NONE
STATES = {"f32": K.F32_CASES, "ds": K.DS_CASES, "f64": K.F64_CASES, "perturb": K.PERTURB_CASES, "deep": K.DEEP_CASES}
ALL = [(s, c) for s, cases in STATES.items() for c in cases]
ALL_IDS = [c["id"] for _, c in ALL]


@pytest.fixture(scope="module")
def actx(B):
    """A context of the module's own: orbits are bound to it."""
    c = B.Context(0)
    yield c
    c.close()


def view_params(B, state, case, **kw):
    prec = {"f32": B.PRECISION_F32, "ds": B.PRECISION_DS, "f64": B.PRECISION_F64}[state]
    flags = B.MANDEL_FMA if case.get("fma") else 0
    return B.mandelbrot_params(case["W"], case["H"], max_iter=case["M"], precision=prec, centre=case["centre"], scale=case["scale"],
                               flags=flags, **kw)


def perturb_params(B, case):
    flags = B.MANDEL_PERTURB_FORCE_DEEP if case.get("kind") == "shallow" else 0
    return B.mandelbrot_params(case["W"], case["H"], max_iter=case["M"], precision=B.PRECISION_PERTURB, centre=(0.0, 0.0),
                               scale=(0.0, 0.0), flags=flags)


@pytest.fixture(scope="module")
def audited(actx, B, O):
    """run(state, case) -> dict(out (lanes, 4), sab (lanes, 4), ref (lanes,), render (lanes,) or None): each case is computed once and
    shared by the tests below."""
    cache = {}

    def run(state, case):
        if case["id"] in cache:
            return cache[case["id"]]
        M = case["M"]
        if state in ("f32", "ds", "f64"):
            p = view_params(B, state, case)
            out = actx.test_mandel_block_audit(p).reshape(-1, 4)
            sab = actx.test_mandel_block_audit(p, sabotage=True).reshape(-1, 4)
            render = actx.mandelbrot(p, want_rgba=False)[1].ravel()
            W, H, c, s = case["W"], case["H"], case["centre"], case["scale"]
            if state == "f64":
                ref = F.mandelbrot_iters_f64(W, H, M, c, s)
            elif case.get("fma"):
                ref = K.fma_iters(W, H, M, c, s)   # (the oracle has no contracted loop)
            else:
                ref = O.mandelbrot_iters(W, H, M, view=O.make_view(c[0], c[1], s[0], s[1]), precision=int(state == "ds"))
        else:
            deep = state == "deep"
            Z, ux, uy, E, o = K.lanes(B, case)
            try:
                out = actx.test_mandel_perturb_block_audit(Z, ux, uy, M, deep=deep, exp2=E)
                sab = actx.test_mandel_perturb_block_audit(Z, ux, uy, M, deep=deep, exp2=E, sabotage=True)
                render = None
                if o is not None:   # a view: the shipped wave loop on the same orbit
                    actx.bind_mandelbrot_orbit(o)
                    render = actx.mandelbrot(perturb_params(B, case), want_rgba=False)[1].ravel()
            finally:
                if o is not None:
                    o.close()
            L = Z.shape[0] - 1
            ref = D.iterate(Z, L, ux, uy, E, M) if deep else R.iterate(Z, L, ux, uy, M)
        r = dict(out=out, sab=sab, ref=np.asarray(ref, np.uint32).ravel(), render=render)
        cache[case["id"]] = r
        return r
    return run


@pytest.mark.parametrize("state,case", ALL, ids=ALL_IDS)
def test_no_accepted_block_breaks_the_promise(audited, state, case):
    r = audited(state, case)
    out = r["out"]
    n, acc, rai, bad = out[:, 0], out[:, 1].astype(np.int64), out[:, 2].astype(np.int64), out[:, 3]
    share = acc.sum() / max(1, acc.sum() + rai.sum())
    print(f"{case['id']}: accepted {int(acc.sum())} of {int(acc.sum() + rai.sum())} audited blocks ({100.0 * share:.1f} %)")
    assert (bad == NONE).all(), (case["id"], int((bad != NONE).sum()), np.nonzero(bad != NONE)[0][:8].tolist(), bad[bad != NONE][:8].tolist())
    assert np.array_equal(n, r["ref"]), (case["id"], int((n != r["ref"]).sum()))
    if r["render"] is not None:
        assert np.array_equal(n, r["render"]), (case["id"], int((n != r["render"]).sum()))
    # every block after the first, up to and including the one that escapes, is audited exactly once
    U, M = K.BLOCK[state], case["M"]
    blocks = np.where(n < (M // U) * U, n // U, M // U - 1)
    assert np.array_equal(acc + rai, np.maximum(blocks, 0)), case["id"]
    if case.get("zeros"):
        assert (acc == 0).all(), case["id"]


@pytest.mark.parametrize("state", list(STATES))
def test_every_state_accepts_and_raises(audited, state):
    acc = rai = 0
    for case in STATES[state]:
        out = audited(state, case)["out"]
        acc += int(out[:, 1].astype(np.int64).sum())
        rai += int(out[:, 2].astype(np.int64).sum())
    print(f"{state}: accepted {acc}, raised {rai}")
    assert acc > 0 and rai > 0


@pytest.mark.parametrize("state,case", ALL, ids=ALL_IDS)
def test_the_audit_has_teeth(audited, state, case):
    """sabotage: needs_exact taken as false.  Only what the audit counts as accepted changes (the lane continues from the exact
    state), so n is unchanged and the block a lane escapes in is reported bad — earlier still where the fast arithmetic had left its
    precondition (a small two-float operand, a rebase, a renormalisation, a phase change).  U is the block length the state's render
    kernel is launched with (K.BLOCK): 8, and 4 for DS, whose escape block is therefore (n // 4) * 4."""
    r = audited(state, case)
    sab, n = r["sab"], r["ref"].astype(np.int64)
    U, M = K.BLOCK[state], case["M"]
    assert np.array_equal(sab[:, 0], r["ref"]) and (sab[:, 2] == 0).all()
    assert np.array_equal(sab[:, 1], r["out"][:, 1].astype(np.int64) + r["out"][:, 2])
    bad = sab[:, 3].astype(np.int64)
    inside = (n >= U) & (n < (M // U) * U)          # the lane escapes in a block that is audited
    escape_block = (n // U) * U
    if state in ("f32", "f64"):                     # the states are trivially equal: the escape is all there is to catch
        assert np.array_equal(bad[inside], escape_block[inside]), case["id"]
        assert (bad[~inside] == NONE).all(), case["id"]
    else:
        assert (bad[inside] <= escape_block[inside]).all(), case["id"]


def test_sabotage_catches_more_than_escapes_in_the_deep_state(audited):
    """Some deep lane's first bad block is not the block it escapes in: a renormalisation, phase change or rebase was caught."""
    other = 0
    for case in K.DEEP_CASES:
        r = audited("deep", case)
        bad, n = r["sab"][:, 3].astype(np.int64), r["ref"].astype(np.int64)
        other += int(((bad != NONE) & (bad != (n // 8) * 8)).sum())
    assert other > 0


def test_a_row_range_is_rows_of_the_whole_image(actx, B, audited):
    case = K.F32_CASES[0]
    whole = audited("f32", case)["out"].reshape(case["H"], case["W"], 4)
    for rb, re_ in ((5, 37), (0, 1), (case["H"] - 1, case["H"])):
        part = actx.test_mandel_block_audit(view_params(B, "f32", case, row_begin=rb, row_end=re_))
        assert np.array_equal(part, whole[rb:re_]), (rb, re_)


def test_refusals(actx, B):
    T = B.test_lib()
    INVALID = 1   # MC_ERR_INVALID_ARGUMENT
    case = K.F32_CASES[0]
    p = view_params(B, "f32", case)
    out = np.zeros((case["H"], case["W"], 4), np.uint32)
    vp = C.c_void_p
    assert T.mc_hook_mandel_block_audit(None, C.byref(p), 0, out.ctypes.data_as(vp)) == INVALID
    assert T.mc_hook_mandel_block_audit(actx._h, None, 0, out.ctypes.data_as(vp)) == INVALID
    assert T.mc_hook_mandel_block_audit(actx._h, C.byref(p), 0, None) == INVALID
    for prec in (B.PRECISION_PERTURB, B.PRECISION_PERTURB_BLA, 7):
        q = view_params(B, "f32", case); q.precision = prec
        assert T.mc_hook_mandel_block_audit(actx._h, C.byref(q), 0, out.ctypes.data_as(vp)) == INVALID, prec
    for flags in (B.MANDEL_ITERS_U16, B.MANDEL_COLOUR_SMOOTH, B.MANDEL_PERTURB_FORCE_DEEP, B.MANDEL_SUPERSAMPLE(2)):
        q = view_params(B, "f32", case); q.flags = flags
        assert T.mc_hook_mandel_block_audit(actx._h, C.byref(q), 0, out.ctypes.data_as(vp)) == INVALID, flags
    q = view_params(B, "ds", K.DS_CASES[0]); q.flags = B.MANDEL_FMA                       # the contracted loop is fp32's
    assert T.mc_hook_mandel_block_audit(actx._h, C.byref(q), 0, out.ctypes.data_as(vp)) == INVALID
    q = view_params(B, "f32", case, row_begin=0, row_end=case["H"], row_block=8, row_stride=16)   # an interleaved tile
    assert T.mc_hook_mandel_block_audit(actx._h, C.byref(q), 0, out.ctypes.data_as(vp)) == INVALID
    assert (out == 0).all()
    Z = np.array([[0.0, 0.0], [-1.0, 0.0], [0.0, 0.0], [-1.0, 0.0]])
    u = np.array([0.25, -0.5])
    o2 = np.zeros((2, 4), np.uint32)
    f = T.mc_hook_mandel_perturb_block_audit
    zp, up, op = Z.ctypes.data_as(vp), u.ctypes.data_as(vp), o2.ctypes.data_as(vp)
    assert f(actx._h, zp, 3, 1, -3000, up, up, 2, 40, 0, op) == 0                        # (the call the refusals below vary)
    for deep in (0, 1):
        assert f(None, zp, 3, deep, -3000, up, up, 2, 40, 0, op) == INVALID
        assert f(actx._h, None, 3, deep, -3000, up, up, 2, 40, 0, op) == INVALID
        assert f(actx._h, zp, 3, deep, -3000, None, up, 2, 40, 0, op) == INVALID
        assert f(actx._h, zp, 3, deep, -3000, up, None, 2, 40, 0, op) == INVALID
        assert f(actx._h, zp, 3, deep, -3000, up, up, 2, 40, 0, None) == INVALID
        assert f(actx._h, zp, 0, deep, -3000, up, up, 2, 40, 0, op) == INVALID            # L == 0
        assert f(actx._h, zp, 3, deep, -3000, up, up, 0, 40, 0, op) == INVALID            # n_lanes == 0
        assert f(actx._h, zp, 3, deep, -3000, up, up, 2, 0, 0, op) == INVALID             # max_iter == 0
