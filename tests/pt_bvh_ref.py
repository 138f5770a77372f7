"""The path tracer's linear intersect() restated in numpy (TEST INFRASTRUCTURE): pathTracer.comp:112-131, 316-341 with the fp32 sphere
test, operation for operation in float32 - one ufunc per fp32 operation, in the shader's order - for ANY batch of rays.  It is the
definition mc_pathtrace_accel_intersect (the BVH walk) must reproduce on every ray: the same id, the same bits of t.  Also the scenes
and the ray families the host and GPU tests share."""
import numpy as np

f32 = np.float32
EPS, TRI_EPS, INF = f32(1e-4), f32(1e-7), f32(1e20)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def intersect(planes, spheres, origins, dirs, block=64):
    """(id, t) per ray: id int32 (-1: miss; planes 0 .. np-1, spheres np + i), t float32 as the loop leaves it.  The spheres are taken
    `block` at a time as a (rays, block) matrix; within a block the FIRST column holding the block's minimum is the one the
    sequential `dd < t` scan would have kept, and the block's winner replaces the holder only if strictly nearer: the same result."""
    planes = np.asarray(planes, f32).reshape(-1, 12)
    spheres = np.asarray(spheres, f32).reshape(-1, 12)
    o = [np.ascontiguousarray(origins[:, k], f32) for k in range(3)]
    d = [np.ascontiguousarray(dirs[:, k], f32) for k in range(3)]
    n_rays, n_planes = o[0].shape[0], planes.shape[0]
    t = np.full(n_rays, INF, f32)
    idx = np.full(n_rays, -1, np.int32)
    with np.errstate(all="ignore"):
        for i in range(n_planes):
            n = [planes[i, 0], planes[i, 1], planes[i, 2]]
            denom = _dot(d, n)
            dd = (planes[i, 3] - _dot(o, n)) / denom
            hit = (denom > TRI_EPS) & (dd < t)
            t = np.where(hit, dd, t)
            idx = np.where(hit, np.int32(i), idx)
        oc3 = [x[:, None] for x in o]
        d3 = [x[:, None] for x in d]
        for first in range(0, spheres.shape[0], block):
            sp = spheres[first:first + block]
            oc = [sp[None, :, k] - oc3[k] for k in range(3)]
            b = _dot(oc, d3)
            det = (b * b - _dot(oc, oc)) + (sp[:, 3] * sp[:, 3])[None, :]
            ok = ~(det < f32(0))
            sq = np.sqrt(np.where(ok, det, f32(0)))
            lo, hi = b - sq, b + sq
            dd = np.where(lo <= EPS, np.where(hi <= EPS, INF, hi), lo)
            dd = np.where(ok & ~np.isnan(dd), dd, f32(np.inf))            # a NaN or a rejected sphere never passes `dd < t`
            col = np.argmin(dd, axis=1)                                    # the first column of the minimum
            best = dd[np.arange(n_rays), col]
            hit = best < t
            t = np.where(hit, best, t)
            idx = np.where(hit, (n_planes + first + col).astype(np.int32), idx)
        idx = np.where(t < INF, idx, np.int32(-1))
    return idx, t


# ---- scenes ---------------------------------------------------------------------------------------------------------
ROOM = np.array([
    -1.0, 0.0, 0.0, 2.6, 0, 0, 0, 0, .85, .25, .25, 1,
    +1.0, 0.0, 0.0, 2.6, 0, 0, 0, 0, .25, .35, .85, 1,
    0.0, +1.0, 0.0, 2.0, 0, 0, 0, 0, .75, .75, .75, 1,
    0.0, -1.0, 0.0, 2.0, 0, 0, 0, 0, .75, .75, .75, 1,
    0.0, 0.0, -1.0, 2.8, 0, 0, 0, 0, .85, .85, .25, 1,
    0.0, 0.0, +1.0, 7.9, 0, 0, 0, 0, 0.1, 0.7, 0.7, 1], f32).reshape(6, 12)


def random_scene(rng, n_planes, n_spheres, n_lights):
    """tests/test_gpu_scenes.py's random_scene, restated: a closed room (the six walls, possibly repeated further out and tilted)
    plus random spheres - the same draws in the same order, so the same tables for the same generator."""
    planes = [ROOM]
    while sum(len(p) for p in planes) < n_planes:
        extra = ROOM.copy()
        extra[:, 3] += rng.uniform(0.5, 3.0, 6).astype(f32)
        tilt = rng.normal(0, 0.05, (6, 3)).astype(f32)
        n = extra[:, :3] + tilt
        extra[:, :3] = n / np.linalg.norm(n, axis=1, keepdims=True)
        planes.append(extra)
    planes = np.concatenate(planes)[:n_planes]
    spheres = np.zeros((n_spheres, 12), f32)
    spheres[:, 0] = rng.uniform(-2.2, 2.2, n_spheres)
    spheres[:, 1] = rng.uniform(-1.8, 1.2, n_spheres)
    spheres[:, 2] = rng.uniform(-2.4, 2.5, n_spheres)
    spheres[:, 3] = rng.uniform(0.05, 0.35, n_spheres)
    spheres[:, 8:11] = rng.uniform(0.2, 0.95, (n_spheres, 3))
    spheres[:, 11] = rng.choice([1, 1, 1, 2, 3], n_spheres)
    lights = rng.choice(n_spheres, n_lights, replace=False)
    spheres[lights, 4:7] = rng.uniform(20, 80, (n_lights, 3))
    spheres[lights, 8:11] = 0
    spheres[lights, 11] = 1
    spheres[lights, 1] = rng.uniform(1.2, 1.7, n_lights)
    spheres[lights, 3] = 0.15
    return planes.astype(f32), spheres


def lattice(n):
    """tests/test_abi.py's lattice, restated: n small diffuse spheres on a 16^3 lattice inside the room (0.25 apart, r = 0.02), the
    first one a light."""
    g = np.arange(16, dtype=f32) * f32(0.25) - f32(1.9)
    s = np.zeros((n, 12), f32)
    s[:, 0:3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:n]
    s[:, 3] = 0.02
    s[:, 8:11] = 0.5
    s[:, 11] = 1.0
    s[:1, 4:7] = 20.0
    return s


def _sphere(c, r, colour=(0.6, 0.6, 0.6), mat=1, e=0.0):
    return [c[0], c[1], c[2], r, e, e, e, 0, colour[0], colour[1], colour[2], mat]


def duplicate_scene():
    """Two identical spheres with different materials (the lower index must win every tie), a light, the room."""
    s = np.array([_sphere((0.0, 1.6, 0.0), 0.2, (0, 0, 0), 1, 60.0),
                  _sphere((0.3, -0.9, -0.4), 0.7, (0.9, 0.3, 0.3), 1),
                  _sphere((0.3, -0.9, -0.4), 0.7, (0.999, 0.999, 0.999), 2),
                  _sphere((-1.4, -1.3, 0.6), 0.5, (0.3, 0.9, 0.3), 1),
                  _sphere((-1.4, -1.3, 0.6), 0.5, (0.999, 0.999, 0.999), 3)], f32)
    return ROOM.copy(), s


def concentric_scene():
    s = np.array([_sphere((0.0, 1.6, 0.0), 0.2, (0, 0, 0), 1, 60.0)] +
                 [_sphere((0.2, -0.6, -0.3), r, (0.9, 0.9, 0.9), 3) for r in (1.0, 0.8, 0.6, 0.4, 0.2, 0.05)], f32)
    return ROOM.copy(), s


def unboxable_scene():
    """Finite spheres among one with a NaN centre, one with an infinite radius, one whose box overflows, and a negative radius."""
    rng = np.random.default_rng(77)
    planes, s = random_scene(rng, 6, 24, 2)
    s[3, 0] = np.nan                       # never hit: every comparison with its NaN fails
    s[7, 3] = np.inf                       # r * r = inf: dd = b - inf, then b + inf = inf - never below t
    s[11, 0:4] = (3.0e38, 0.0, 0.0, 3.0e38)   # centre + radius overflows: no box
    s[15, 3] = -s[15, 3]                   # r * r is what the test reads: a negative radius is the positive one's sphere
    return planes, s


# ---- rays -----------------------------------------------------------------------------------------------------------
def normalize(v):
    """normalize() as the shader's fp32 code does it: a * (1 / sqrt(dot(a, a)))."""
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        s = f32(1) / np.sqrt(_dot([v[:, 0], v[:, 1], v[:, 2]], [v[:, 0], v[:, 1], v[:, 2]]))
    return (v * s[:, None]).astype(f32)


def camera_rays(n, rng):
    """Rays from the pinhole (0, 0.5179..., 7.365...) into the sensor's cone, as pathTracer.comp:352-362 aims them."""
    o = np.tile(np.array([0.0, 0.52 - 0.06 * 0.035, 7.4 - 0.035], f32), (n, 1))
    d = np.stack([rng.uniform(-0.52, 0.52, n), rng.uniform(-0.4, 0.3, n), -np.ones(n)], 1)
    return o, normalize(d)


def interior_rays(n, rng):
    o = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.9, 1.9, n), rng.uniform(-2.7, 7.8, n)], 1).astype(f32)
    return o, normalize(rng.normal(0, 1, (n, 3)))


def surface_rays(spheres, n, rng):
    """Rays starting ON sphere surfaces (x = c + r u rounded to fp32), leaving in any direction: bounce and shadow rays."""
    s = np.asarray(spheres, f32).reshape(-1, 12)
    ok = np.isfinite(s[:, :4]).all(1) & (np.abs(s[:, 3]) < 1e4)
    s = s[ok] if ok.any() else np.array([_sphere((0, 0, 0), 1.0)], f32)
    k = rng.integers(0, s.shape[0], n)
    u = normalize(rng.normal(0, 1, (n, 3)))
    o = (s[k, :3] + u * np.abs(s[k, 3:4])).astype(f32)
    return o, normalize(rng.normal(0, 1, (n, 3)))


def silhouette_rays(spheres, n, rng, distances=(1.0, 1e3, 1e5)):
    """Rays aimed at a sphere's silhouette from `distance` away: the angle to the centre is that of the tangent cone, with the miss
    distance (dist - r) / |oc| spread over +-1e-3: where the fp32 test and the geometric test disagree."""
    s = np.asarray(spheres, f32).reshape(-1, 12).astype(np.float64)
    ok = np.isfinite(s[:, :4]).all(1) & (np.abs(s[:, 3]) < 1e30)
    s = s[ok] if ok.any() else np.array([_sphere((0, 0, 0), 1.0)], np.float64)
    k = rng.integers(0, s.shape[0], n)
    c, r = s[k, :3], np.abs(s[k, 3])
    away = rng.choice(np.asarray(distances, np.float64), n) * rng.uniform(0.5, 2.0, n) + r
    u = rng.normal(0, 1, (n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = c - u * away[:, None]                       # |oc| = away
    w = np.cross(u, rng.normal(0, 1, (n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    miss = r / away + rng.uniform(-1e-3, 1e-3, n)   # sine of the angle between the ray and oc: distance of the line from c over |oc|
    miss = np.clip(miss, 0.0, 1.0)
    d = u * np.sqrt(1.0 - miss ** 2)[:, None] + w * miss[:, None]
    return o.astype(f32), normalize(d)


def nan_rays(n, rng):
    """Rays with a NaN or an infinity somewhere, zero directions, directions far from unit length: outside the cull's domain, where
    the walk culls nothing and still has to answer as the loop does."""
    o, d = interior_rays(n, rng)
    kind = np.arange(n) % 8
    o[kind == 0, 0] = np.nan
    d[kind == 1, 1] = np.nan
    o[kind == 2, 2] = np.inf
    d[kind == 3, 0] = np.inf
    d[kind == 4] = 0.0
    d[kind == 5] *= f32(3.0)
    d[kind == 6] *= f32(0.25)
    d[kind == 7] *= f32(1.004)         # inside the domain, with a measured delta of 0.008
    return o, d


def ray_families(planes, spheres, n_each, seed):
    rng = np.random.default_rng(seed)
    fam = [camera_rays(n_each, rng), interior_rays(n_each, rng), surface_rays(spheres, n_each, rng),
           silhouette_rays(spheres, n_each, rng), nan_rays(max(n_each // 8, 64), rng)]
    return np.concatenate([f[0] for f in fam]), np.concatenate([f[1] for f in fam])
