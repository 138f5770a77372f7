"""The scenes the accelerated chains' host and GPU tests share (TEST INFRASTRUCTURE): tests/pt_bvh_ref.py's, by the names
tests/test_gpu_pt_bvh.py gives them, plus an open scene without planes, so that centre rays miss."""
import functools

import numpy as np

import pt_bvh_ref as R

f32 = np.float32


@functools.lru_cache(maxsize=None)
def scene(name):
    """(planes, spheres), made once and shared read-only."""
    if name == "random200":
        planes, spheres = R.random_scene(np.random.default_rng(100 + 200), 12, 200, 5)
    elif name == "random4000":
        planes, spheres = R.random_scene(np.random.default_rng(9), 6, 4000, 3)
    elif name == "lattice700":
        planes, spheres = R.ROOM.copy(), R.lattice(700)
    elif name == "duplicates":
        planes, spheres = R.duplicate_scene()
    elif name == "unboxable":
        planes, spheres = R.unboxable_scene()
    elif name == "one":
        planes, spheres = R.ROOM.copy(), R.lattice(1)
    elif name == "none":
        planes, spheres = R.ROOM.copy(), np.zeros((0, 12), f32)
    elif name == "open":   # random200's spheres with no wall behind them: the rays between them hit nothing
        planes, spheres = np.zeros((0, 12), f32), R.random_scene(np.random.default_rng(100 + 200), 12, 200, 5)[1]
    else:
        raise KeyError(name)
    planes, spheres = np.ascontiguousarray(planes, f32), np.ascontiguousarray(spheres, f32)
    planes.setflags(write=False)
    spheres.setflags(write=False)
    return planes, spheres


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)
