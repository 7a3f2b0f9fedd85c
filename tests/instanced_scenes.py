"""Scenes and ray sets of the instancing tests (test_instanced_cpu.py, test_instanced_gpu.py, test_instanced_host.py): BLASes built by
the PLOC spec, seeded transforms, and the pool in numpy.  World extents are about [-15, 15] so that ray_sets.edge_rays meets geometry."""
import numpy as np

from ntrace_amd import scenes

import np_bvh_ploc as pl
import np_instanced as ni
import ray_sets
import sah_sweep_scenes as ss

F = np.float32
_cache = {}


def rotation(rng):
    """A random rotation matrix (binary64) from a unit quaternion."""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def transform(rot, scale, translation):
    """objectToWorld, 12 float32: rotation x diag(scale), then the translation."""
    m = np.zeros((3, 4))
    m[:, :3] = np.asarray(rot, np.float64) @ np.diag(np.broadcast_to(np.asarray(scale, np.float64), (3,)))
    m[:, 3] = translation
    return m.astype(F).reshape(12)


def seeded_transforms(n, seed, spread=50.0, mirrored=0, size=1.0):
    """n matrices: rotation x non-uniform scale in size * [1/4, 4] x translation within +-spread; the first `mirrored` have one scale
    negated."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = size * 4.0 ** rng.uniform(-1, 1, 3)
        if i < mirrored:
            s[i % 3] = -s[i % 3]
        out.append(transform(rotation(rng), s, rng.uniform(-spread, spread, 3)))
    return np.stack(out)


def blas(name):
    """(tri, pos, spec build) of a named mesh: sah_sweep_scenes' names, 'soup100', 'one' (a single triangle), 'nested90'."""
    if name not in _cache:
        if name == "one":
            tri, pos = np.array([[0, 1, 2]], np.int32), np.array([(0, 0, 0), (1, 0, 0.25), (0, 1, 0.5)], F)
        elif name == "nested90":
            tri, pos = pl.nested_scene(90)
        elif name == "soup100":
            tri, pos = scenes.random_soup(100, seed=77, walls=False)[:2]
        else:
            tri, pos = ss.scene(name)
        mn, mx = pl.scene_box(pos)
        _cache[name] = (tri, pos, pl.build(tri, pos, mn, mx, 8))
    return _cache[name]


def pool_of(names, **gaps):
    return ni.make_pool([ss.buffers(blas(n)[2]) for n in names], **gaps)


CAMERA = dict(eye=(2.0, 3.0, -34.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=50.0, far=200.0)


def scene(name):
    """-> dict(names: the BLASes' meshes, transforms (n, 12), blas (n,)) of a named instanced scene."""
    rng = np.random.default_rng({"three": 11, "grid": 12, "mirror": 13}[name])
    if name == "three":        # three distinct BLASes that overlap around the origin
        names = ["cornell", "soup1000", "soup64"]
        tf = [transform(rotation(rng), 0.03, (-8.0, -8.0, -6.0)), transform(rotation(rng), (1.0, 0.8, 1.1), (0.5, 0.0, 0.0)),
              transform(rotation(rng), 1.2, (2.0, 1.0, 0.0))]
        which = [0, 1, 2]
    elif name == "grid":       # 8 x 8 Cornell boxes, each rotated
        names = ["cornell"]
        tf = [transform(rotation(rng), 0.004, (-10.5 + 3.0 * i, -10.5 + 3.0 * j, rng.uniform(-1, 1))) for j in range(8) for i in range(8)]
        which = [0] * 64
    else:                      # two mirrored, non-uniformly scaled soups
        names = ["soup1000"]
        tf = [transform(rotation(rng), (-1.0, 0.5, 1.3), (-4.0, 1.0, 0.0)), transform(rotation(rng), (1.2, -0.7, 0.6), (4.0, -1.0, 2.0))]
        which = [0, 0]
    return dict(names=names, transforms=np.stack(tf), blas=np.asarray(which, np.int32))


def scene_rays(primary=(128, 64), random=4096, seed=5):
    """Primary rays of CAMERA plus incoherent rays through the scenes' volume."""
    prim, _ = scenes.primary_rays(CAMERA, *primary)
    return np.concatenate([prim, scenes.random_rays(random, seed, extent=12.0)])


def finite_edge_rays():
    """ray_sets.edge_rays without the rays that have a non-finite word: an identity transform reproduces a finite ray only."""
    r = ray_sets.edge_rays()
    a = r.view(F).reshape(-1, 8)
    return r[np.isfinite(a).all(axis=1)]


def odd_rays():
    """Degenerate rays and rays that miss every scene box."""
    r = scenes.random_rays(256, 9, extent=12.0)
    r["tmax"][:64] = F(-1.0)                      # tmax < tmin
    r["tmin"][64:96] = r["tmax"][64:96] = F(3.0)  # tmin == tmax
    for k in ("ox", "oy", "oz"):                  # far outside, pointing away
        r[k][128:] = F(500.0) + np.abs(r[k][128:])
    for k in ("dx", "dy", "dz"):
        r[k][128:] = np.abs(r[k][128:])
    return r


def flatten(sc):
    """The world-space triangles of a scene in binary64: (n, 3, 3) vertices, with (instance, triangle id) per triangle."""
    verts, who = [], []
    for i, (m, b) in enumerate(zip(sc["transforms"], sc["blas"])):
        tri, pos, _ = blas(sc["names"][int(b)])
        m = m.astype(np.float64).reshape(3, 4)
        p = pos.astype(np.float64) @ m[:, :3].T + m[:, 3]
        verts.append(p[tri])
        who.append(np.stack([np.full(tri.shape[0], i), np.arange(tri.shape[0])], axis=1))
    return np.concatenate(verts), np.concatenate(who)


def brute_force(verts, rays, chunk=512):
    """Closest hit of every ray over the triangles in binary64 (Moeller-Trumbore): (hit mask, t)."""
    o = np.stack([rays[k] for k in ("ox", "oy", "oz")], axis=1).astype(np.float64)
    d = np.stack([rays[k] for k in ("dx", "dy", "dz")], axis=1).astype(np.float64)
    tmin, tmax = rays["tmin"].astype(np.float64), rays["tmax"].astype(np.float64)
    v0, e1, e2 = verts[:, 0], verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]
    best = np.full(rays.shape[0], np.inf)
    with np.errstate(all="ignore"):
        for s in range(0, rays.shape[0], chunk):
            oo, dd = o[s:s + chunk, None, :], d[s:s + chunk, None, :]
            pv = np.cross(dd, e2[None])
            det = (e1[None] * pv).sum(-1)
            tv = oo - v0[None]
            u = (tv * pv).sum(-1) / det
            qv = np.cross(tv, e1[None])
            v = (dd * qv).sum(-1) / det
            t = (e2[None] * qv).sum(-1) / det
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin[s:s + chunk, None]) & (t < tmax[s:s + chunk, None])
            best[s:s + chunk] = np.where(ok, t, np.inf).min(axis=1)
    return np.isfinite(best), best


def result_words(got):
    """A device result array (nt.RESULT_DTYPE) as (id, t bits, u bits, v bits)."""
    return got["id"], got["t"].view(np.uint32), got["padA"].view(np.uint32), got["padB"].view(np.uint32)

