"""CPU census of the cases of the fast-block audit (tests/mandel_block_audit_cases.py): which branches of the rescaled loop and of
PERTURB's loop the lanes of tests/test_gpu_mandel_block_audit.py take, counted by the scalar restatements with event counters
(D.scalar_iters, R.scalar_iters).  Every class of D.EVENTS must be reached by some deep case — the existing deep GPU views reach six of
the thirteen — and the PERTURB cases must rebase both ways.  No device."""
import fractions

import numpy as np
import pytest

import mandel_block_audit_cases as K
import mandel_perturb_deep_ref as D
import mandel_perturb_ref as R


def sampled(case):
    """The lanes of the census: every 6th row and 7th column of a view, every lane of a table."""
    if case.get("kind") == "table":
        return list(range(len(case["lanes"])))
    return [y * case["W"] + x for y in range(0, case["H"], 6) for x in range(0, case["W"], 7)]


@pytest.fixture(scope="module")
def deep_census(B):
    out = {}
    for case in K.DEEP_CASES:
        Z, ux, uy, E, o = K.lanes(B, case)
        if o is not None:
            o.close()
        Zl, L = Z.tolist(), Z.shape[0] - 1
        stats, ns = {}, []
        for k in sampled(case):
            ns.append(D.scalar_iters(Zl, L, float(ux[k]), float(uy[k]), E, case["M"], stats))
        ref = D.iterate(Z, L, ux[sampled(case)], uy[sampled(case)], E, case["M"])
        assert ref.tolist() == ns, case["id"]          # the counted loop is still the loop
        stats["L"] = L
        out[case["id"]] = stats
        print(case["id"], {k: v for k, v in sorted(stats.items())})
    return out


def test_deep_cases_reach_every_event_class(deep_census):
    union = set()
    for stats in deep_census.values():
        union |= {k for k in D.EVENTS if stats.get(k, 0) > 0}
    assert not [k for k in D.EVENTS if k not in union]


def test_each_deep_case_supplies_what_it_is_there_for(deep_census):
    want = {
        "deep M33 5e-290": ("renorm_hi", "to_plain", "rebase_to_plain", "escape_plain"),
        "deep M33 1e-1000": ("renorm_hi", "to_plain", "rebase_to_plain", "escape_plain"),
        "deep M41 1e-900": ("renorm_hi", "to_plain"),
        "deep centre 0": ("fresh_m_gt0", "rebase_end", "rebase_to_zero", "interior_scaled"),
        "deep centre -1": ("fresh_m_gt0", "rebase_end", "rebase_to_zero", "interior_scaled"),
        "deep nucleus3": ("rebase_to_scaled",),
        "deep exterior 0.26": ("escape_scaled",),
        "deep exterior -0.75+0.05i": ("escape_scaled",),
        "deep synthetic zeros": ("fresh_m0", "fresh_m_gt0"),
        "deep low window": ("renorm_hi", "renorm_lo"),
    }
    for cid, keys in want.items():
        missing = [k for k in keys if deep_census[cid].get(k, 0) < 1]
        assert not missing, (cid, missing, deep_census[cid])


def test_zero_tables_keep_their_lanes_scaled(deep_census):
    """The premise of the GPU test's `accepted_blocks == 0` for the tables with zeros: every iteration of every sampled lane begins
    scaled (a scaled lane of such a table never takes a fast result), or the orbit is no longer than a block (m reaches L in every
    block, so neither does a plain lane)."""
    for case in K.DEEP_CASES:
        if case.get("zeros"):
            s = deep_census[case["id"]]
            assert s["iters"] > 0 and (s["scaled"] == s["iters"] or s["L"] <= K.BLOCK["deep"]), case["id"]


def test_perturb_cases_rebase_both_ways(B):
    total = {}
    for case in K.PERTURB_CASES:
        Z, dcx, dcy, _, o = K.lanes(B, case)
        o.close()
        Zl, L = Z.tolist(), Z.shape[0] - 1
        stats = {}
        idx = sampled(case)
        ns = [R.scalar_iters(Zl, L, float(dcx[k]), float(dcy[k]), case["M"], stats) for k in idx]
        assert ns == R.iterate(Z, L, dcx[idx], dcy[idx], case["M"]).tolist(), case["id"]
        assert ns[:3] == [R.scalar_iters(Zl, L, float(dcx[k]), float(dcy[k]), case["M"]) for k in idx[:3]]   # the form without stats
        print(case["id"], stats)
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
        if case["centre"] == "boundary":
            assert L < case["M"]   # an escaping reference (its lanes reach m == L only in the step that escapes: no rebase is left to count)
    assert total.get("rebase_near", 0) > 0 and total.get("rebase_end", 0) > 0


def test_fma32_is_a_single_rounding():
    """K.fma32 (the MC_MANDEL_FMA restatement's fused multiply-add) against exact rational arithmetic rounded once to float32."""
    rng = np.random.default_rng(5)
    a = rng.uniform(-2, 2, 4000).astype(np.float32)
    b = rng.uniform(-2, 2, 4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.uniform(-1e-6, 1e-6, 4000))).astype(np.float32)   # heavy cancellation
    c[::3] = rng.uniform(-2, 2, c[::3].size).astype(np.float32)
    # ties of the double rounding: a product whose sum with c lies a hair off a float32 midpoint
    a[:8] = np.float32(1 + 2.0 ** -12); b[:8] = np.float32(1 + 2.0 ** -12); c[:8] = np.float32(2.0 ** -23) * np.arange(8, dtype=np.float32)
    got = K.fma32(a, b, c)
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = fractions.Fraction(x) * fractions.Fraction(y) + fractions.Fraction(z)
        lo = np.float32(float(exact))                   # float(): correctly rounded to double; then one more rounding: bracket instead
        cands = {float(lo), float(np.nextafter(lo, np.float32(np.inf))), float(np.nextafter(lo, np.float32(-np.inf)))}
        best = min(cands, key=lambda v: (abs(fractions.Fraction(v) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert g == best, (x, y, z, g, best)
