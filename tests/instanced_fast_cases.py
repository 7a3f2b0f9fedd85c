"""The inputs the FAST two-level tests share (test_instanced_fast_cpu.py, test_instanced_fast_gpu.py): each case is a pool, a top-level
tree by the numpy spec (np_instanced.tlas_build, which ntr_tlas_build equals byte for byte), 64 * 3 + 17 rays -- a ragged last wave --
and what the spec alone must say of its FAST share, so that no device case passes by never running FAST:
  expect "all"    fastWaveSteps == waveSteps > 0
         "mixed"  0 < fastWaveSteps < waveSteps
         None     no condition (the case is about records)
A case dict: pool, tlas (nodes, root_link, records), rays, expect, and optionally inst_masks, ray_masks, seed (a function of any_hit),
seed_instance."""
import numpy as np

import instanced_scenes as isc
import np_instanced as ni
import np_instanced_seeded as nsd

F = np.float32
N_RAYS = 64 * 3 + 17
EYE = np.eye(3)
_cache = {}


def below(x):
    return np.nextafter(F(x), F(0))


def above(x):
    return np.nextafter(F(x), F(np.inf))


def nice_rays():
    """Primary and random rays of instanced_scenes, every zero component nudged to 2^-20: each is in the FAST ranges."""
    r = isc.scene_rays()
    r = np.concatenate([r[37:8192:68][:120], r[8192:8192 + N_RAYS - 120]]).copy()
    assert r.shape[0] == N_RAYS
    for k in ("ox", "oy", "oz", "dx", "dy", "dz"):
        r[k][r[k] == 0] = F(2.0 ** -20)
    return r


def _case(names, transforms, blas, rays, expect, plant=None, **kw):
    pool = isc.pool_of(names, gap_nodes=1, gap_rows=3)
    if plant is not None:                                # one box float of the first gap slot: slack counts
        nodes = pool["nodes"].copy()
        gap = pool["ranges"][0][0] + pool["ranges"][0][1]
        nodes[gap:gap + 4] = np.array([plant], F).view(np.uint8)
        pool = dict(pool, nodes=nodes)
    inst = ni.instances(np.stack(transforms), blas)
    t = ni.tlas_build(pool["nodes"], pool["ranges"], inst)
    return dict(pool=pool, inst=inst, tlas=(t["nodes"], t["root_link"], t["records"]), rays=rays, expect=expect, **kw)


def _three():
    sc = isc.scene("three")
    return list(sc["names"]), list(sc["transforms"]), list(sc["blas"])


def _box_centre(name):
    w = np.ascontiguousarray(isc.blas(name)[2]["nodes"]).view(np.uint8).reshape(-1)[:48].view(F).astype(np.float64)
    lo = np.minimum([w[0], w[2], w[8]], [w[4], w[6], w[10]])
    hi = np.maximum([w[1], w[3], w[9]], [w[5], w[7], w[11]])
    return (lo + hi) / 2


def _build(name):
    names, tf, blas = _three()
    rays = nice_rays()
    lane = np.arange(N_RAYS) % 64
    if name == "all_nice":
        return _case(names, tf, blas, rays, "all")
    if name == "zero_direction":
        # one lane per wave with dx == 0 and a tmax that ends it before the scene: the wave returns to FAST
        sel = lane == 5
        rays["dx"][sel] = F(0)
        rays["tmax"][sel] = F(2.0)
        return _case(names, tf, blas, rays, "mixed")
    if name in ("object_dir_small", "object_dir_large"):
        # a fourth instance whose worldToObject scales directions by 2^-45 (below 2^-40) or by 2^25 (above 2^20)
        if name == "object_dir_small":
            tf.append(isc.transform(EYE, 2.0 ** 45, (1.0, 2.0, 3.0)))        # a giant: every ray enters it
        else:
            s, t = 2.0 ** -25, np.array([2.0 ** -10, 2.0 ** -11, -2.0 ** -10])
            tf.append(isc.transform(EYE, s, t))
            sel = lane % 8 == 3                                                # rays that start inside the tiny instance
            o = (t + s * _box_centre("soup64")).astype(F)
            rays["ox"][sel], rays["oy"][sel], rays["oz"][sel] = o
        blas.append(2)
        return _case(names, tf, blas, rays, "mixed")
    if name in ("object_origin_zero", "object_origin_zero_tiny"):
        # an unscaled, unrotated fourth instance and rays whose ox is its translation's x: the object ox is exactly 0, which NOTINY
        # admits -- and a pool with one tiny float in its slack does not
        tf.append(isc.transform(EYE, 1.0, (1.5, -2.25, 0.5)))
        blas.append(2)
        sel = lane % 4 == 1
        rays["ox"][sel] = F(1.5)
        return _case(names, tf, blas, rays, "all" if name == "object_origin_zero" else "mixed",
                     plant=None if name == "object_origin_zero" else -2.0 ** -100)   # (a lo below its hi of 0: still ordered)
    if name == "pool_withheld":                          # the one-triangle BLAS: FAST on the top level only
        names.append("one")
        tf.append(isc.transform(EYE, 3.0, (0.0, 0.0, -4.0)))
        blas.append(3)
        return _case(names, tf, blas, rays, "mixed")
    if name == "tlas_withheld":                          # one instance beyond 2^55: FAST inside instances only
        tf.append(isc.transform(EYE, 1.0, (2.0 ** 56, 0.0, 0.0)))
        blas.append(2)
        return _case(names, tf, blas, rays, "mixed")
    if name == "range_ends":
        # wave 0: the last values inside the ranges; wave 1: the first outside; waves 2, 3 untouched
        for k, v in enumerate([2.0 ** -40, -2.0 ** 20, 2.0 ** -36, -below(2.0 ** 55)]):
            inside = F(v)
            outside = (below if k in (0, 2) else above)(abs(inside)) * np.sign(inside)
            key = ("dx", "dy", "oz", "oy")[k]
            rays[key][8 * k + 1] = inside
            rays[key][64 + 8 * k + 1] = outside
        return _case(names, tf, blas, rays, "mixed")
    if name == "odd_rays":
        odd = isc.odd_rays()
        return _case(names, tf, blas, odd[np.r_[0:50, 64:110, 128:241]].copy(), None)
    if name == "masks":
        inst_masks = np.array([0x80000001, 0x2, 0x80000000], np.uint32)
        ray_masks = np.where(np.arange(N_RAYS) % 3 == 0, 0x80000000, 0x3).astype(np.uint32)
        ray_masks[np.arange(N_RAYS) % 7 == 0] = 0x4      # rays that every instance refuses
        return _case(names, tf, blas, rays, "all", inst_masks=inst_masks, ray_masks=ray_masks)
    if name == "seeded":
        # hits in front of the scene, hits behind it, misses: an any-hit ray whose seed is a hit never starts
        ids = np.where(np.arange(N_RAYS) % 3 == 0, -1, 7).astype(np.int32)
        ts = np.where(np.arange(N_RAYS) % 3 == 1, F(20.0), F(150.0)).astype(F)
        seed = nsd.seed_of(ids, ts, 0x12345678, 0x7FC00001)
        return _case(names, tf, blas, rays, "all", seed=lambda any_hit: seed, seed_instance=3)
    if name == "identity":                               # one identity instance: no top-level node, rootLink ~0
        return _case(["soup1000"], [isc.transform(EYE, 1.0, (0.0, 0.0, 0.0))], [0], rays, "all")
    raise KeyError(name)


NAMES = ["all_nice", "zero_direction", "object_dir_small", "object_dir_large", "object_origin_zero", "object_origin_zero_tiny", "pool_withheld",
         "tlas_withheld", "range_ends", "odd_rays", "masks", "seeded", "identity"]


def case(name):
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]
