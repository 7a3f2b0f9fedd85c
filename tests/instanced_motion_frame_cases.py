"""The inputs of the motion-blurred frame tests (tests/np_instanced_motion_frame.py is the rule): the geometry of the motion scenes as
ntr_instanced_hit_attributes takes it, hashed times and the spec's motion-traced records per scene, and the self-occlusion demonstration
-- a convex cube that turns and travels inside the shutter, whose AO rays may never hit the cube they start from."""
import numpy as np

import ntrace_amd as nt
from ntrace_amd import scenes

import instanced_motion_cases as mc
import instanced_scenes as isc
import np_bvh_ploc as pl
import np_instanced as ni
import np_instanced_motion_frame as mf
import np_raygen
import sah_sweep_scenes as ss
from test_instanced_frame_cpu import geometry

F = np.float32
_cache = {}

BIG_NAMES = ["cornell", "soup64"]          # instanced_motion_cases.big()'s pool


def names_of(name):
    return BIG_NAMES if name == "big" else isc.scene(name)["names"]


def motion_scene(name):
    return mc.big() if name == "big" else mc.named(name)


def records(rid, rt, ru, rv):
    res = np.zeros(rid.shape[0], nt.RESULT_DTYPE)
    res["id"], res["t"], res["padA"], res["padB"] = rid, rt, ru.view(np.int32), rv.view(np.int32)
    return res


def rays_and_times():
    """isc.scene_rays((64, 32), 2048) and one hashed time per ray (seed 5)."""
    if "rays" not in _cache:
        rays = isc.scene_rays((64, 32), 2048)
        _cache["rays"] = (rays, mf.ray_times_primary(rays.shape[0], None, 5))
    return _cache["rays"]


def traced(name, inst1=None, time=None):
    """The spec's closest-hit records of the scene's rays: at the hashed per-ray times, or at the scalar `time`; inst1 replaces key 1
    -> dict(ms, tri, pos, blas_tris, rays, times, res, ids)"""
    key = ("traced", name, None if inst1 is None else inst1.tobytes(), time)
    if key not in _cache:
        ms = motion_scene(name)
        if inst1 is not None:
            ms = mc.MotionScene(ms.pool, ms.inst0, inst1)
        rays, times = rays_and_times()
        kw = dict(times=times) if time is None else dict(time=time)
        rid, rt, ru, rv, rinst, _ = ms.trace(rays, False, **kw)
        tri, pos, blas_tris = geometry(names_of(name))
        _cache[key] = dict(ms=ms, tri=tri, pos=pos, blas_tris=blas_tris, rays=rays, times=times if time is None else None,
                           res=records(rid, rt, ru, rv), ids=rinst.astype(np.int32))
    return _cache[key]


def posed(inst0, inst1, t):
    """The instances of key 0 posed at the clamped scalar time t: objectToWorld = lerp, worldToObject = its inverse (zero without one)."""
    import np_instanced_motion as mo
    out = inst0.copy()
    m = mo.lerp(inst0["objectToWorld"].reshape(-1, 12), inst1["objectToWorld"].reshape(-1, 12), mo.clamp_time(t))
    w, _ = mo.invert_many(m)
    mv = mo.moving(inst0, inst1)
    out["objectToWorld"][mv] = m.reshape(out["objectToWorld"].shape)[mv]
    out["worldToObject"][mv] = w.reshape(out["worldToObject"].shape)[mv]
    return out


# ---- the demonstration ------------------------------------------------------------------------------------------------------------------------
CUBE_POS = np.array([(x, y, z) for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], F)
# two triangles per face, wound so that the geometric normal points out of the cube
CUBE_TRI = np.array([(0, 2, 1), (1, 2, 3), (4, 5, 6), (5, 7, 6), (0, 1, 4), (1, 5, 4), (2, 6, 3), (3, 6, 7), (0, 4, 2), (2, 4, 6), (1, 3, 5), (3, 7, 5)],
                    np.int32)
DEMO_CAM = dict(eye=(0.5, 1.0, -14.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=50.0, far=200.0)
DEMO_W, DEMO_H, DEMO_NS, DEMO_RADIUS, DEMO_AO_SEED = 64, 32, 8, 3.0, 0x51ed270b


def demo():
    """A unit cube BLAS; instance 0 turns and travels between its keys, instance 1 stands still below
    -> dict(ms, tri, pos, blas_tris, rays (pixel-table order), s2i)"""
    if "demo" not in _cache:
        n64 = np.cross(CUBE_POS[CUBE_TRI[:, 1]] - CUBE_POS[CUBE_TRI[:, 0]], CUBE_POS[CUBE_TRI[:, 2]] - CUBE_POS[CUBE_TRI[:, 0]]).astype(np.float64)
        assert ((n64 * CUBE_POS[CUBE_TRI].astype(np.float64).mean(axis=1)).sum(axis=1) > 0).all()     # outward winding
        mn, mx = pl.scene_box(CUBE_POS)
        pool = ni.make_pool([ss.buffers(pl.build(CUBE_TRI, CUBE_POS, mn, mx, 8))])
        rng = np.random.default_rng(1)
        key0 = isc.transform(isc.rotation(rng), 5.0, (-4.0, 0.0, 0.0))
        key1 = isc.transform(isc.rotation(rng), 5.0, (2.0, 1.0, 0.0))
        still = isc.transform(np.eye(3), 5.0, (0.0, -6.0, 0.0))
        inst0 = ni.instances(np.stack([key0, still]), [0, 0])
        inst1 = ni.instances(np.stack([key1, still]), [0, 0])
        rays, s2i = scenes.primary_rays(DEMO_CAM, DEMO_W, DEMO_H)
        _cache["demo"] = dict(ms=mc.MotionScene(pool, inst0, inst1), tri=CUBE_TRI, pos=CUBE_POS, blas_tris=np.array([(0, 12)], np.int32),
                              rays=rays, s2i=s2i.astype(np.int32))
    return _cache["demo"]


def ao_batch(rays, out, normals, ns=DEMO_NS, radius=DEMO_RADIUS, seed=DEMO_AO_SEED):
    """np_raygen.ao_rays over per-ray normals (the table indexed by slot), as binary32 rays; a zero fourth word is a missed input."""
    n = rays.shape[0]
    by_slot = out.copy()
    by_slot["id"] = np.where((out["id"] == -1) | (normals[:, 3] == 0), -1, np.arange(n))
    ro, rd, rt = np_raygen.ao_rays(rays, by_slot, normals[:, :3].copy(), ns, radius, seed)
    r = np.zeros(n * ns, nt.RAY_DTYPE)
    for k, a in zip(("ox", "oy", "oz"), ro.T):
        r[k] = a.astype(F)
    for k, a in zip(("dx", "dy", "dz"), rd.T):
        r[k] = a.astype(F)
    r["tmax"] = rt.astype(F)
    return r
