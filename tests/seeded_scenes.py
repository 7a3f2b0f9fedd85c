"""The scene and rays of the seeded two-level trace's tests (test_instanced_seeded_cpu.py, test_instanced_seeded_gpu.py,
test_instanced_seeded_host.py): a static world -- one BLAS of the pool in its own space -- and small instances scattered through it, in
two forms: the N instances alone (what the seeded trace sees, the world being its seed) and N + 1 instances with the world as identity
instance N (what the unseeded trace sees)."""
import numpy as np

import instanced_scenes as isc
import np_instanced as ni
import np_instanced_seeded as nsd
import np_tracer
import sah_sweep_scenes as ss

F = np.float32
_cache = {}


def world_scene():
    """-> dict(names, pool, world: the world's BLAS index, transforms (N, 12), blas (N,), inst: INSTANCE_DTYPE (N,), inst_all: (N + 1,)
    with the world as identity instance N, tlas / tlas_all: np_instanced.tlas_build of either)."""
    if "world" not in _cache:
        names = ["soup1000", "cornell", "soup64"]
        rng = np.random.default_rng(21)
        tf = [isc.transform(isc.rotation(rng), 0.004, rng.uniform(-9, 9, 3)) for _ in range(24)]
        tf += [isc.transform(isc.rotation(rng), 0.15, rng.uniform(-9, 9, 3)) for _ in range(8)]
        _cache["world"] = _finish(names, 0, np.stack(tf), np.asarray([1] * 24 + [2] * 8, np.int32))
    return _cache["world"]


def three_scene():
    """instanced_scenes.scene('three') with soup1000 of its pool as the world, in its own space, and the other two as instances."""
    if "three" not in _cache:
        sc = isc.scene("three")
        keep = np.asarray([0, 2])
        _cache["three"] = _finish(sc["names"], 1, sc["transforms"][keep], sc["blas"][keep])
    return _cache["three"]


def _finish(names, world, transforms, blas):
    pool = isc.pool_of(names)
    inst = ni.instances(transforms, blas)
    inst_all = ni.instances(np.concatenate([transforms, ni.IDENTITY[None]]), np.concatenate([blas, [world]]))
    return dict(names=names, pool=pool, world=world, transforms=transforms, blas=blas, inst=inst, inst_all=inst_all,
                tlas=ni.tlas_build(pool["nodes"], pool["ranges"], inst), tlas_all=ni.tlas_build(pool["nodes"], pool["ranges"], inst_all))


def rays():
    """The prototype's 5 704 rays: primary and incoherent rays through the volume, degenerate and far rays, finite edge rays."""
    if "rays" not in _cache:
        r = np.concatenate([isc.scene_rays(primary=(64, 32), random=2048), isc.odd_rays(), isc.finite_edge_rays()])
        assert r.shape[0] == 5704
        _cache["rays"] = r
    return _cache["rays"]


def world_seed(sc, r, any_hit=False):
    """(n, 4) uint32 seed words: np_tracer.trace of the world BLAS in its own space, w2 = w3 = 0."""
    nodes, woop, tri_index = ss.buffers(isc.blas(sc["names"][sc["world"]])[2])
    sid, st = np_tracer.trace(nodes, woop, tri_index, r, any_hit=any_hit)
    return nsd.seed_of(sid, st)


def miss_seed(r):
    """(n, 4) uint32 seed words of all misses with t = ray.tmax: what an unseeded trace starts from."""
    return nsd.seed_of(np.full(r.shape[0], -1, np.int32), r["tmax"].astype(F))
