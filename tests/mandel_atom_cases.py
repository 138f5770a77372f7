"""Cases and helpers the CPU and the GPU atom tests share (tests/test_mandel_atom_host.py, tests/test_gpu_mandel_atom.py): the synthetic
planes of the domains, mpmath's period-3 nucleus as text, and the refusal check.  Not a conftest: the test files import it."""
import math

import mpmath
import numpy as np


def refused(B, status, *words):
    """A context manager: the call inside raises McError with `status`, and every word is in its text."""
    class Ctx:
        def __enter__(self):
            return self

        def __exit__(self, et, ev, tb):
            assert et is B.McError, f"no refusal ({et})"
            assert ev.status == status, str(ev)
            for w in words:
                assert w in str(ev), str(ev)
            return True
    return Ctx()


def synthetic_planes():
    """name -> (period uint32, amin float64, max_iter): the planes the CPU and the GPU tests share."""
    rng = np.random.default_rng(7)
    out = {}
    for n in (1, 63, 64, 65):
        out[f"one period, {n} px"] = (np.full(n, 5, np.uint32), rng.random(n), 9)
        out[f"own period each, {n} px"] = (np.arange(n, dtype=np.uint32), rng.random(n), n + 2)
    per = rng.integers(1, 6, 300).astype(np.uint32)
    am = rng.integers(1, 4, 300).astype(np.float64) * 0.125                  # few distinct values: equal minima, the lowest index wins
    out["equal minima"] = (per, am, 7)
    per = rng.integers(0, 4, 200).astype(np.uint32)
    am = np.where(per == 0, np.inf, rng.random(200))
    out["period 0 with +inf"] = (per, am, 3)
    out["all +inf"] = (np.full(70, 2, np.uint32), np.full(70, np.inf), 4)
    am = rng.random(130)
    am[::7] = -am[::7]
    am[3::11] = np.nan
    out["negatives and nans are counted only"] = (rng.integers(0, 3, 130).astype(np.uint32), am, 5)
    out["tiny and zero"] = (np.array([1, 1, 1, 2, 2], np.uint32), np.array([5e-324, 0.0, 0.0, 1e-300, 5e-324]), 2)
    return out


SYNTHETIC = synthetic_planes()


def nucleus3(digits):
    """mpmath's period-3 nucleus in the lower half plane, (re, im) as text with `digits` fractional digits."""
    with mpmath.workdps(digits + 30):
        c = mpmath.findroot(lambda c: (c * c + c) ** 2 + c, mpmath.mpc("-0.1225611668766536", "-0.7448617666197442"), tol=mpmath.mpf(10) ** -(digits + 20))
        def fmt(v):
            k = str(int(mpmath.floor(abs(v) * mpmath.mpf(10) ** digits))).rjust(digits + 1, "0")
            return ("-" if v < 0 else "") + k[:-digits] + "." + k[-digits:]
        return fmt(c.real), fmt(c.imag)
